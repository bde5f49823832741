"""``scape`` command surface for the MI355X build: ``infer_pa`` and the stages after it, ``merge_pa``,
``cal_exp_pa_len`` and ``ex_pa_cnt_mat`` (reference console script ``scape = scape:main``, pyproject.toml:34-35;
``gen_utr_annotation`` and ``prepare_input`` are outside this build's scope)."""
import time as _time

_t0 = _time.perf_counter()
from .cli import cli, display_paper_info  # noqa: E402

_IMPORT_S = _time.perf_counter() - _t0        # seconds spent importing the package (numpy, click, the host modules)


def main():
    display_paper_info()
    cli(prog_name="scape")
