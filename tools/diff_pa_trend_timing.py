#!/usr/bin/env python3
"""Timing of `scape diff_pa_trend` (scape_amd/report.py) on the synthetic directory of tools/diff_pa_timing.py: by default
2,000 records (K = 2..8 pA sites, about 10,000 count rows) x 20,000 cells x 9,999 permutations, 95 % of the (site, cell)
counts zero.  Every cell gets a score (a scramble of i / cells, so no ties), and `scape diff_pa_groups` with G
equal-sized clusters for each G of --groups (default 2,12) runs on the same stream in the same process as the yardstick:
its labels kernel finds G - 1 order statistics of the keys that the scores kernel ranks completely, and its test kernel
walks the same nonzeros with a byte per label where the trend kernel reads a halfword per score.  With --warmup 1 (the
default) one warm-up run per command with 255 permutations; then --repeats times (default 3) the timed runs, one after
the other, whose wall time, stage times (report.LAST_TIMES; `render` holds everything the device does apart from the
counting) and seconds inside the library's entry points go into one JSON line.  The builders of labellings wait for
their kernel, so `calls_s` of perm_scores and perm_labels is that kernel, a launch and, where the buffers grow, their
allocation; the test entry points also compact the rows and copy the counters back.  The kernels on their own:

    rocprofv3 --kernel-trace --output-format csv -d P -- python tools/diff_pa_trend_timing.py --dir <made before> --warmup 0
    python tools/diff_pa_trend_timing.py --kernel_trace P          (with the same --groups)

    python tools/diff_pa_trend_timing.py [--records N] [--cells N] [--n_perm N] [--dir D] [--groups 2,12] [--repeats R]
                                         [--warmup 0|1] [--rank]
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

from diff_pa_groups_timing import make_groups  # noqa: E402
from diff_pa_markers_timing import CallClock, quiet  # noqa: E402
from diff_pa_timing import make_dir  # noqa: E402

KERNELS = ("k_rep_perm_scores", "k_rep_perm_trend", "k_rep_trend_obs", "k_rep_perm_labels", "k_rep_perm_groups")
CALLS = ("scape_hip_report_perm_scores", "scape_hip_report_perm_trend", "scape_hip_report_perm_labels",
         "scape_hip_report_perm_groups")


def make_scores(root, n_cells):
    path = os.path.join(root, "pseudotime.csv")
    with open(path, "w") as fh:
        fh.write("index,pseudotime\n" + "".join(f"{i},{(i * 7919) % n_cells / n_cells!r}\n" for i in range(n_cells)))
    return path


def kernel_trace(root, groups):
    """the ms of every launch of KERNELS in a rocprofv3 kernel trace of this script (run with --warmup 0 and launches
    that hold all permutations), in time order; the launches of the G-way kernels go round the --groups"""
    launches = {name: [] for name in KERNELS}
    for f in sorted(glob.glob(os.path.join(root, "**", "*kernel_trace.csv"), recursive=True)):
        with open(f, newline="") as fh:
            for r in csv.DictReader(fh):
                name = re.sub(r"\s*\[clone.*", "", re.sub(r"\(.*", "", r["Kernel_Name"]).strip())
                if name in launches:
                    launches[name].append((int(r["Start_Timestamp"]), int(r["End_Timestamp"])))
    out = {}
    for name, runs in launches.items():
        ms = [(e - s) / 1e6 for s, e in sorted(runs)]
        if name in ("k_rep_perm_labels", "k_rep_perm_groups"):
            out[name] = {f"G{G}": ms[k::len(groups)] for k, G in enumerate(groups)}
        else:
            out[name] = ms
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=2000)
    ap.add_argument("--cells", type=int, default=20000)
    ap.add_argument("--n_perm", type=int, default=9999)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--dir", default=None, help="directory to make the inputs in, or to reuse if it holds them")
    ap.add_argument("--groups", default="2,12", help="numbers of equal-sized clusters of the diff_pa_groups runs")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1, help="0: no warm-up runs (for a kernel trace)")
    ap.add_argument("--rank", action="store_true", help="run diff_pa_trend with --rank")
    ap.add_argument("--kernel_trace", default=None,
                    help="summarise the rocprofv3 kernel trace under this directory and do nothing else")
    a = ap.parse_args()
    groups = [int(g) for g in a.groups.split(",")]
    if a.kernel_trace is not None:
        print(json.dumps(kernel_trace(a.kernel_trace, groups)))
        return
    from scape_amd import _lib, report
    root = a.dir or tempfile.mkdtemp(prefix="diff_pa_trend_timing_")
    out = {"records": a.records, "cells": a.cells, "n_perm": a.n_perm, "groups": groups, "rank": a.rank, "repeats": []}
    try:
        if not os.path.exists(os.path.join(root, "nz.npz")):
            os.makedirs(root, exist_ok=True)
            make_dir(root, a.records, a.cells)
        z = np.load(os.path.join(root, "nz.npz"))
        n_cells = int(z["n_cells"])
        out.update(rows=int(z["rec_rows"][-1]), nonzeros=int(z["row_off"][-1]), device=_lib.default_context().name())
        scores = make_scores(root, n_cells)
        runs = [("diff_pa_trend", lambda n: report._diff_pa_trend(root, "res.gene.pkl", scores, a.rank, n, a.seed))]
        for G in groups:
            clu = make_groups(root, n_cells, G)
            runs.append((f"diff_pa_groups_G{G}",
                         lambda n, clu=clu: report._diff_pa_groups(root, "res.gene.pkl", clu, (), n, a.seed)))
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
