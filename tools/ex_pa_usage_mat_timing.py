#!/usr/bin/env python3
"""Timing of `scape ex_pa_usage_mat` (scape_amd/report.py) on the synthetic directory of tools/diff_pa_timing.py: by
default 2,000 records (K = 2..8 pA sites, 10,000 count rows) x 20,000 cells; 95 % of the (site, cell) counts are zero,
the others 1..3.  In one process, after one warm-up run of each command:

* `ex_pa_cnt_mat --format mtx`, `--repeats` timed runs: wall time and the stage times of report.LAST_TIMES (decode =
  unpickling; h2d_counts = uploads and the count kernels; render = the totals call and the two render passes per block
  with their waits; gzip_wait = waiting for the host's gzip threads; finish = header and body into the final files).
  It is the yardstick: the same rows and columns, one matrix of digit text;
* `ex_pa_usage_mat` on the same stream, the same number of runs: the same count rows, walked once for the totals and
  once per matrix.

One JSON line goes to stdout.  Kernel times come from one kernel trace, in a process of its own, of one run of the new
command and one of `ex_pa_cnt_mat --format mtx` behind it (no warm-up, nothing timed on the host):

    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/ex_pa_usage_mat_timing.py --dir <made before> --only both

    python tools/ex_pa_usage_mat_timing.py [--records N] [--cells N] [--dir D] [--repeats N] [--min_reads N]
                                           [--only usage_mat|both]
"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=2000)
    ap.add_argument("--cells", type=int, default=20000)
    ap.add_argument("--dir", default=None, help="directory to make the inputs in, or to reuse if it holds them")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--min_reads", type=int, default=1)
    ap.add_argument("--only", choices=["usage_mat", "both"], default=None,
                    help="for a kernel trace: one run of the new command, with `both` one of ex_pa_cnt_mat --format mtx behind it")
    a = ap.parse_args()
    import contextlib
    import io
    from diff_pa_timing import DENSITY, make_dir
    from ex_pa_len_mat_timing import dir_bytes, timed
    from scape_amd import _lib, report
    root = a.dir or tempfile.mkdtemp(prefix="ex_pa_usage_mat_timing_")
    out = {"records": a.records, "cells": a.cells, "density": DENSITY, "repeats": a.repeats, "min_reads": a.min_reads}

    def usage():
        return report._ex_pa_usage_mat(root, "res.gene.pkl", min_reads=a.min_reads)

    def usage_bytes(path):
        import gzip
        sizes = dir_bytes(path)
        with gzip.open(os.path.join(path, "reads.mtx.gz"), "rt") as fh:
            fh.readline()
            sizes["reads_header"] = fh.readline().strip()
        return sizes
    try:
        if not os.path.exists(os.path.join(root, "nz.npz")):
            os.makedirs(root, exist_ok=True)
            t0 = time.perf_counter()
            make_dir(root, a.records, a.cells)
            out["make_s"] = time.perf_counter() - t0
        z = np.load(os.path.join(root, "nz.npz"))
        out.update(rows=int(z["rec_rows"][-1]), nonzeros=int(z["row_off"][-1]))
        if a.only:
            with contextlib.redirect_stdout(io.StringIO()):
                path = usage()
                out["stages_s"] = dict(report.LAST_TIMES)
                out["file_bytes"] = usage_bytes(path)
                if a.only == "both":
                    report._ex_pa_cnt_mat(root, "res.gene.pkl", fmt="mtx")
                    out["cnt_mtx_stages_s"] = dict(report.LAST_TIMES)
        else:
            out["device"] = _lib.default_context().name()
            out["ex_pa_cnt_mat_mtx"] = timed(lambda: report._ex_pa_cnt_mat(root, "res.gene.pkl", fmt="mtx"), a.repeats)
            out["ex_pa_cnt_mat_mtx"]["file_bytes"] = dir_bytes(os.path.join(root, "res.gene.cnt"))
            out["ex_pa_usage_mat"] = timed(usage, a.repeats)
            out["ex_pa_usage_mat"]["file_bytes"] = usage_bytes(os.path.join(
                root, "res.gene.usage" if a.min_reads == 1 else f"res.gene.min{a.min_reads}.usage"))
    finally:
        if a.dir is None:
            shutil.rmtree(root, ignore_errors=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
