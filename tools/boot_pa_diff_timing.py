#!/usr/bin/env python3
"""Timing of `scape boot_pa_len_diff` and `scape boot_pa_usage_diff` (scape_amd/report.py) on the synthetic directory of
tools/diff_pa_timing.py: by default 2,000 records (K = 2..8 pA sites, about 10,000 count rows) x 20,000 cells x 9,999
bootstrap replicates, 95 % of the (site, cell) counts zero, the cells cut into 12 equal-sized clusters (cell i in cluster
i * 12 // cells), of which the two commands compare g0 with g1.  Their yardsticks run in the same process ahead of them:
`boot_pa_len --idents g0 --idents g1` and `boot_pa_usage --idents g0 --idents g1`, whose kernels walk the same nonzeros
under the same multiplicities population by population and store two values where the fused kernels store one
difference.  One warm-up run of each of the four with 255 replicates, then --repeats timed runs of each, in the order
boot_pa_len, boot_pa_usage, boot_pa_len_diff, boot_pa_usage_diff; wall times and stage times (report.LAST_TIMES; `render`
holds everything the device does apart from the counting) go into one JSON line with the number of count batches (= calls
of the command's entry point, the replicates being one chunk).  Kernel times come from one kernel trace of this script
with one repeat; every timed run launches its value kernel and the select once per count batch:

    rocprofv3 --kernel-trace --stats --output-format csv -d P -- python tools/boot_pa_diff_timing.py --dir <made before> --repeats 1
    python tools/boot_pa_diff_timing.py --kernel_trace P --batches <the four timed runs', in their order>

    python tools/boot_pa_diff_timing.py [--records N] [--cells N] [--n_boot N] [--dir D] [--groups 12] [--repeats 3]
                                        [--sites 2,8]
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

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from boot_pa_usage_timing import run_once  # noqa: E402
from diff_pa_groups_timing import make_groups  # noqa: E402
from diff_pa_timing import make_dir  # noqa: E402

# command, its value kernel, its entry point, in the order of the runs
RUNS = (("boot_pa_len", "k_rep_boot_len", "scape_hip_report_boot_len"),
        ("boot_pa_usage", "k_rep_boot_usage", "scape_hip_report_boot_usage"),
        ("boot_pa_len_diff", "k_rep_boot_len_diff", "scape_hip_report_boot_len_diff"),
        ("boot_pa_usage_diff", "k_rep_boot_usage_diff", "scape_hip_report_boot_usage_diff"))


def kernel_trace(root, batches):
    """ms and launches of the timed runs' kernels in a rocprofv3 kernel trace of this script with --repeats 1.  The four
    warm-ups come first, then the four timed runs: the last batches[k] launches of a value kernel are its timed run's,
    and the selects of the timed runs are the last sum(batches) launches of k_rep_boot_select, in the runs' order"""
    launches = {}
    for f in sorted(glob.glob(os.path.join(root, "**", "*kernel_trace.csv"), recursive=True)):
        with open(f, newline="") as fh:
            for r in csv.DictReader(fh):
                name = re.sub(r"\s*\[clone.*", "", re.sub(r"\(.*", "", r["Kernel_Name"]).strip())
                launches.setdefault(name, []).append((int(r["Start_Timestamp"]), int(r["End_Timestamp"])))
    ms = {name: [(e - s) / 1e6 for s, e in sorted(v)] for name, v in launches.items()}
    sel = ms.get("k_rep_boot_select", [])
    if len(sel) < sum(batches):
        raise SystemExit("fewer launches of k_rep_boot_select than the batches given")
    sel = sel[len(sel) - sum(batches):]
    out, first = {}, 0
    for (cmd, kernel, _entry), n in zip(RUNS, batches):
        if len(ms.get(kernel, [])) < n:
            raise SystemExit(f"{kernel}: fewer launches than the batches given")
        out[cmd] = {kernel: sum(ms[kernel][-n:]), "k_rep_boot_select": sum(sel[first:first + n]), "launches": n}
        first += n
    out["k_rep_boot_len_diff_over_k_rep_boot_len"] = \
        out["boot_pa_len_diff"]["k_rep_boot_len_diff"] / out["boot_pa_len"]["k_rep_boot_len"]
    out["k_rep_boot_usage_diff_over_k_rep_boot_usage"] = \
        out["boot_pa_usage_diff"]["k_rep_boot_usage_diff"] / out["boot_pa_usage"]["k_rep_boot_usage"]
    out["launches_in_trace"] = {k: len(v) for k, v in ms.items() if k.startswith("k_rep_boot_")}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=2000)
    ap.add_argument("--cells", type=int, default=20000)
    ap.add_argument("--n_boot", type=int, default=9999)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--dir", default=None, help="directory to make the inputs in, or to reuse if it holds them")
    ap.add_argument("--groups", type=int, default=12, help="number of equal-sized clusters; g0 and g1 are compared")
    ap.add_argument("--repeats", type=int, default=3, help="timed runs per command")
    ap.add_argument("--sites", default="2,8", help="LO,HI: the records made have K = LO..HI pA sites (above 8: the value "
                                                   "kernels' path for long records)")
    ap.add_argument("--kernel_trace", default=None,
                    help="the -d directory of a rocprofv3 kernel trace of this script: print its kernels' times and stop")
    ap.add_argument("--batches", default="1,1,1,1",
                    help="with --kernel_trace: the count batches of the four timed runs, in their order")
    a = ap.parse_args()
    if a.kernel_trace is not None:
        print(json.dumps(kernel_trace(a.kernel_trace, [int(v) for v in a.batches.split(",")])))
        return
    from scape_amd import _lib, report
    root = a.dir or tempfile.mkdtemp(prefix="boot_pa_diff_timing_")
    out = {"records": a.records, "cells": a.cells, "n_boot": a.n_boot, "groups": a.groups, "repeats": a.repeats}
    try:
        if not os.path.exists(os.path.join(root, "nz.npz")):
            os.makedirs(root, exist_ok=True)
            make_dir(root, a.records, a.cells, sites=tuple(int(v) for v in a.sites.split(",")))
        z = np.load(os.path.join(root, "nz.npz"))
        out.update(rows=int(z["rec_rows"][-1]), nonzeros=int(z["row_off"][-1]), device=_lib.default_context().name())
        clu = make_groups(root, int(z["n_cells"]), a.groups)
        fns = {"boot_pa_len": lambda n, seed: report._boot_pa_len(root, "res.gene.pkl", clu, ("g0", "g1"), n, "95", seed),
               "boot_pa_usage": lambda n, seed: report._boot_pa_usage(root, "res.gene.pkl", clu, ("g0", "g1"), n, "95", seed),
               "boot_pa_len_diff": lambda n, seed: report._boot_pa_len_diff(root, "res.gene.pkl", clu, "g0", "g1", n, "95",
                                                                             seed),
               "boot_pa_usage_diff": lambda n, seed: report._boot_pa_usage_diff(root, "res.gene.pkl", clu, "g0", "g1", n,
                                                                                 "95", seed)}
        for name, _kernel, entry in RUNS:                                # the warm-up of all four, then the timed runs
            wall, _stages, batches, _path = run_once(fns[name], entry, 255, a.seed)
            out[name] = {"warmup_wall_s": wall, "warmup_batches": batches, "wall_s": [], "stages_s": []}
        for name, _kernel, entry in RUNS:
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
