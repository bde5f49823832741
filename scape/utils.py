"""``scape.utils`` import path of the reference's two reporting commands (utils.py:319-427, :438-553) and of
``ex_pa_pseudobulk``, which sums their count matrix over cell groups, and ``diff_pa``, which tests it between two."""
from scape_amd.report import cal_exp_pa_len, diff_pa, ex_pa_cnt_mat, ex_pa_pseudobulk  # noqa: F401
