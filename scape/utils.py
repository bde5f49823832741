"""``scape.utils`` import path of the reference's two reporting commands (utils.py:319-427, :438-553)."""
from scape_amd.report import cal_exp_pa_len, ex_pa_cnt_mat  # noqa: F401
