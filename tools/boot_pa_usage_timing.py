#!/usr/bin/env python3
"""Timing of `scape boot_pa_usage` (scape_amd/report.py) on the synthetic directory of tools/diff_pa_timing.py: by
default 2,000 records (K = 2..8 pA sites, about 10,000 count rows) x 20,000 cells x 9,999 bootstrap replicates, 95 % of
the (site, cell) counts zero, the cells cut into 12 equal-sized clusters (cell i in cluster i * 12 // cells).
`scape boot_pa_len` runs on the same cluster file in the same process ahead of it as the yardstick: k_rep_boot_len walks
the same nonzeros under the same multiplicities once and stores one value per (record, cluster, replicate);
k_rep_boot_usage walks them twice and stores one per (kept row, cluster, replicate).  One warm-up run of each command
with 255 replicates, then --repeats timed runs of each whose wall times and stage times (report.LAST_TIMES; `render`
holds everything the device does apart from the counting) go into one JSON line with the number of count batches
(= calls of the command's entry point, the replicates being one chunk) of the warm-up and of a timed run.  Kernel times
come from one kernel trace of this script with one repeat; the batches tell its launches apart:

    rocprofv3 --kernel-trace --stats --output-format csv -d P -- python tools/boot_pa_usage_timing.py --dir <made before> --repeats 1
    python tools/boot_pa_usage_timing.py --kernel_trace P --batches <boot_pa_len's>,<boot_pa_usage's of the timed run>

    python tools/boot_pa_usage_timing.py [--records N] [--cells N] [--n_boot N] [--dir D] [--groups 12] [--repeats 3]
"""
import argparse
import contextlib
import csv
import glob
import io
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
from diff_pa_timing import make_dir  # noqa: E402

HBM_PEAK_GBS = 8000.0           # MI355X: 8 TB/s


def kernel_trace(root, n_len, n_usage):
    """ms and launches of the timed runs' kernels in a rocprofv3 kernel trace of this script with --repeats 1: the runs
    come in the order warm-up boot_pa_len, warm-up boot_pa_usage, boot_pa_len, boot_pa_usage, and a timed run launches a
    value kernel and a select once per count batch, so the last n_usage launches of k_rep_boot_usage and of
    k_rep_boot_select are the timed boot_pa_usage's, and the n_len before them boot_pa_len's"""
    launches = {}
    for f in sorted(glob.glob(os.path.join(root, "**", "*kernel_trace.csv"), recursive=True)):
        with open(f, newline="") as fh:
            for r in csv.DictReader(fh):
                name = re.sub(r"\s*\[clone.*", "", re.sub(r"\(.*", "", r["Kernel_Name"]).strip())
                launches.setdefault(name, []).append((int(r["Start_Timestamp"]), int(r["End_Timestamp"])))
    ms = {name: [(e - s) / 1e6 for s, e in sorted(v)] for name, v in launches.items()}
    for name in ("k_rep_boot_len", "k_rep_boot_usage", "k_rep_boot_select"):
        if name not in ms:
            raise SystemExit(f"{name}: no launch in the trace")
    if len(ms["k_rep_boot_select"]) < n_len + n_usage or len(ms["k_rep_boot_usage"]) < n_usage or \
            len(ms["k_rep_boot_len"]) < n_len:
        raise SystemExit("fewer launches than the batches given")
    sel = ms["k_rep_boot_select"]
    out = {"k_rep_boot_len": {"ms": sum(ms["k_rep_boot_len"][-n_len:]), "launches": n_len},
           "k_rep_boot_usage": {"ms": sum(ms["k_rep_boot_usage"][-n_usage:]), "launches": n_usage},
           "k_rep_boot_select.boot_pa_len": {"ms": sum(sel[-n_usage - n_len:-n_usage]), "launches": n_len},
           "k_rep_boot_select.boot_pa_usage": {"ms": sum(sel[-n_usage:]), "launches": n_usage},
           "k_rep_boot_mult.last": {"ms": ms["k_rep_boot_mult"][-1], "launches": 1},
           "launches_in_trace": {k: len(ms[k]) for k in ("k_rep_boot_mult", "k_rep_boot_len", "k_rep_boot_usage",
                                                         "k_rep_boot_select")}}
    out["k_rep_boot_usage_over_k_rep_boot_len"] = out["k_rep_boot_usage"]["ms"] / out["k_rep_boot_len"]["ms"]
    return out


def run_once(fn, entry, n, seed):
    """one run: (wall seconds, stage times, calls of the library's `entry` = count batches, the file's path)"""
    from scape_amd import _lib, report
    lib = _lib.load_library()
    real, calls = getattr(lib, entry), [0]

    def counted(*a):
        calls[0] += 1
        return real(*a)
    setattr(lib, entry, counted)
    try:
        t0 = time.perf_counter()
        with contextlib.redirect_stdout(io.StringIO()):
            path = fn(n, seed)
        wall = time.perf_counter() - t0
    finally:
        setattr(lib, entry, real)
    return wall, dict(report.LAST_TIMES), calls[0], path


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=2000)
    ap.add_argument("--cells", type=int, default=20000)
    ap.add_argument("--n_boot", type=int, default=9999)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--dir", default=None, help="directory to make the inputs in, or to reuse if it holds them")
    ap.add_argument("--groups", type=int, default=12, help="number of equal-sized clusters")
    ap.add_argument("--repeats", type=int, default=3, help="timed runs per command")
    ap.add_argument("--kernel_trace", default=None,
                    help="the -d directory of a rocprofv3 kernel trace of this script: print its kernels' times and stop")
    ap.add_argument("--batches", default="1,1",
                    help="with --kernel_trace: the count batches of a timed boot_pa_len and boot_pa_usage run")
    a = ap.parse_args()
    if a.kernel_trace is not None:
        n_len, n_usage = (int(v) for v in a.batches.split(","))
        print(json.dumps(kernel_trace(a.kernel_trace, n_len, n_usage)))
        return
    from scape_amd import _lib, report
    root = a.dir or tempfile.mkdtemp(prefix="boot_pa_usage_timing_")
    out = {"records": a.records, "cells": a.cells, "n_boot": a.n_boot, "groups": a.groups, "repeats": a.repeats}
    try:
        if not os.path.exists(os.path.join(root, "nz.npz")):
            os.makedirs(root, exist_ok=True)
            make_dir(root, a.records, a.cells)
        z = np.load(os.path.join(root, "nz.npz"))
        rows = int(z["rec_rows"][-1])
        out.update(rows=rows, nonzeros=int(z["row_off"][-1]), device=_lib.default_context().name())
        # every count row of this directory is a kept row of a reported record: what k_rep_boot_usage has to store
        out["vals_bytes"] = rows * a.groups * a.n_boot * 8
        out["vals_ms_at_hbm_peak"] = out["vals_bytes"] / HBM_PEAK_GBS / 1e6
        clu = make_groups(root, int(z["n_cells"]), a.groups)
        runs = (("boot_pa_len", report._boot_pa_len, "scape_hip_report_boot_len"),
                ("boot_pa_usage", report._boot_pa_usage, "scape_hip_report_boot_usage"))
        fns = {name: (lambda n, seed, fn=fn: fn(root, "res.gene.pkl", clu, (), n, "95", seed)) for name, fn, _e in runs}
        for name, _fn, entry in runs:                                    # the warm-up of both, then the timed runs
            wall, _stages, batches, _path = run_once(fns[name], entry, 255, a.seed)
            out[name] = {"warmup_wall_s": wall, "warmup_batches": batches, "wall_s": [], "stages_s": []}
        for name, _fn, entry in runs:
            for _k in range(a.repeats):
                wall, stages, batches, path = run_once(fns[name], entry, a.n_boot, a.seed)
                out[name]["wall_s"].append(wall)
                out[name]["stages_s"].append(stages)
                out[name]["batches"] = batches
            with open(path, newline="") as fh:
                out[name]["lines"] = sum(1 for _ in fh) - 1
    finally:
        if a.dir is None:
            shutil.rmtree(root, ignore_errors=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
