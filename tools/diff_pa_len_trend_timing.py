#!/usr/bin/env python3
"""Timing of `scape diff_pa_len_trend` (scape_amd/report.py) on the synthetic directory and the scores of
tools/diff_pa_trend_timing.py: by default 2,000 records (K = 2..8 pA sites, about 10,000 count rows) x 20,000 cells x
9,999 permutations, 95 % of the (site, cell) counts zero, every cell with a score.  `scape diff_pa_trend` runs on the
same stream in the same process as the yardstick: both build the same permuted scores, and its test kernel
k_rep_perm_trend walks the nonzeros twice and divides in f64 where k_rep_perm_len_trend walks them once and multiplies
in integers.  With --warmup 1 (the default) one warm-up run per command with 255 permutations; then --repeats times
(default 3) the timed runs, one after the other, whose wall time, stage times (report.LAST_TIMES) and seconds inside the
library's entry points go into one JSON line.  The kernels on their own:

    rocprofv3 --kernel-trace --output-format csv -d P -- python tools/diff_pa_len_trend_timing.py --dir <made before> --warmup 0
    python tools/diff_pa_len_trend_timing.py --kernel_trace P

    python tools/diff_pa_len_trend_timing.py [--records N] [--cells N] [--n_perm N] [--dir D] [--repeats R] [--warmup 0|1]
                                             [--rank]
"""
import argparse
import csv
import glob
import json
import os
import re
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from diff_pa_markers_timing import CallClock, quiet  # noqa: E402
from diff_pa_timing import make_dir  # noqa: E402
from diff_pa_trend_timing import make_scores  # noqa: E402

KERNELS = ("k_rep_perm_scores", "k_rep_perm_len_trend", "k_rep_len_trend_obs", "k_rep_perm_trend", "k_rep_trend_obs")
CALLS = ("scape_hip_report_perm_scores", "scape_hip_report_perm_len_trend", "scape_hip_report_perm_trend")


def kernel_trace(root):
    """the ms of every launch of KERNELS in a rocprofv3 kernel trace of this script (run with --warmup 0 and launches
    that hold all permutations), in time order; k_rep_perm_scores runs once per command and repeat, diff_pa_len_trend's
    launch first"""
    launches = {name: [] for name in KERNELS}
    for f in sorted(glob.glob(os.path.join(root, "**", "*kernel_trace.csv"), recursive=True)):
        with open(f, newline="") as fh:
            for r in csv.DictReader(fh):
                name = re.sub(r"\s*\[clone.*", "", re.sub(r"\(.*", "", r["Kernel_Name"]).strip())
                if name in launches:
                    launches[name].append((int(r["Start_Timestamp"]), int(r["End_Timestamp"])))
    return {name: [(e - s) / 1e6 for s, e in sorted(runs)] for name, runs in launches.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=2000)
    ap.add_argument("--cells", type=int, default=20000)
    ap.add_argument("--n_perm", type=int, default=9999)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--dir", default=None, help="directory to make the inputs in, or to reuse if it holds them")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1, help="0: no warm-up runs (for a kernel trace)")
    ap.add_argument("--rank", action="store_true", help="run both commands with --rank")
    ap.add_argument("--kernel_trace", default=None,
                    help="summarise the rocprofv3 kernel trace under this directory and do nothing else")
    a = ap.parse_args()
    if a.kernel_trace is not None:
        print(json.dumps(kernel_trace(a.kernel_trace)))
        return
    from scape_amd import _lib, report
    root = a.dir or tempfile.mkdtemp(prefix="diff_pa_len_trend_timing_")
    out = {"records": a.records, "cells": a.cells, "n_perm": a.n_perm, "rank": a.rank, "repeats": []}
    try:
        if not os.path.exists(os.path.join(root, "nz.npz")):
            os.makedirs(root, exist_ok=True)
            make_dir(root, a.records, a.cells)
        z = np.load(os.path.join(root, "nz.npz"))
        n_cells = int(z["n_cells"])
        out.update(rows=int(z["rec_rows"][-1]), nonzeros=int(z["row_off"][-1]), device=_lib.default_context().name())
        scores = make_scores(root, n_cells)
        runs = [("diff_pa_len_trend", lambda n: report._diff_pa_len_trend(root, "res.gene.pkl", scores, a.rank, n, a.seed)),
                ("diff_pa_trend", lambda n: report._diff_pa_trend(root, "res.gene.pkl", scores, a.rank, n, a.seed))]
        if a.warmup:
            for _name, fn in runs:
                quiet(fn, 255)
        clock = CallClock(_lib.load_library(), CALLS)
        for _ in range(a.repeats):
            rep = {}
            for name, fn in runs:
                t0 = time.perf_counter()
                path = quiet(fn, a.n_perm)
                rep[name] = {"wall_s": time.perf_counter() - t0, "stages_s": dict(report.LAST_TIMES),
                             "calls_s": {k: v for k, v in clock.take().items() if v}}
                with open(path, newline="") as fh:
                    rep[name]["lines"] = sum(1 for _ in fh) - 1
            out["repeats"].append(rep)
    finally:
        if a.dir is None:
            shutil.rmtree(root, ignore_errors=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
