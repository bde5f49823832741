#!/usr/bin/env python3
"""Timing of `scape boot_pa_len` (scape_amd/report.py) on the synthetic directory of tools/diff_pa_timing.py: by default
2,000 records (K = 2..8 pA sites, about 10,000 count rows) x 20,000 cells x 9,999 bootstrap replicates, 95 % of the
(site, cell) counts zero, the cells cut into 12 equal-sized clusters (cell i in cluster i * 12 // cells).
`scape diff_pa_len_groups` runs on the same cluster file in the same process ahead of it as the yardstick: its kernel
k_rep_perm_len_groups walks the same nonzeros with the same one byte per nonzero and permutation that k_rep_boot_len
reads per nonzero and replicate.  Per command: one warm-up run with 255 permutations or replicates, then one timed run
whose wall time and stage times (report.LAST_TIMES; `render` holds everything the device does apart from the counting)
go into one JSON line.  Kernel times come from one kernel trace of this script:

    rocprofv3 --kernel-trace --stats --output-format csv -d P -- python tools/boot_pa_len_timing.py --dir <made before>
    python tools/boot_pa_len_timing.py --kernel_trace P

    python tools/boot_pa_len_timing.py [--records N] [--cells N] [--n_boot N] [--dir D] [--groups 12]
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

from diff_pa_groups_timing import make_groups, timed  # noqa: E402
from diff_pa_timing import make_dir  # noqa: E402

KERNELS = ("k_rep_boot_mult", "k_rep_boot_len", "k_rep_boot_select", "k_rep_perm_labels", "k_rep_perm_len_groups",
           "k_rep_pair_segidx", "k_rep_len_groups_obs")


def kernel_trace(root):
    """ms and launches of the timed runs' kernels in a rocprofv3 kernel trace of this script: every kernel named has as
    many launches in its command's warm-up run as in its timed run, so the timed ones are the later half"""
    launches = {}
    for f in sorted(glob.glob(os.path.join(root, "**", "*kernel_trace.csv"), recursive=True)):
        with open(f, newline="") as fh:
            for r in csv.DictReader(fh):
                name = re.sub(r"\s*\[clone.*", "", re.sub(r"\(.*", "", r["Kernel_Name"]).strip())
                launches.setdefault(name, []).append((int(r["Start_Timestamp"]), int(r["End_Timestamp"])))
    out = {}
    for name in KERNELS:
        v = [(e - s) / 1e6 for s, e in sorted(launches.get(name, []))]
        if not v or len(v) % 2:
            raise SystemExit(f"{name}: {len(v)} launches do not fit a warm-up and a timed run")
        v = v[len(v) // 2:]
        out[name] = {"ms": sum(v), "launches": len(v)}
    out["k_rep_boot_len_over_k_rep_perm_len_groups"] = out["k_rep_boot_len"]["ms"] / out["k_rep_perm_len_groups"]["ms"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=2000)
    ap.add_argument("--cells", type=int, default=20000)
    ap.add_argument("--n_boot", type=int, default=9999, help="replicates, and the yardstick's permutations")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--dir", default=None, help="directory to make the inputs in, or to reuse if it holds them")
    ap.add_argument("--groups", type=int, default=12, help="number of equal-sized clusters")
    ap.add_argument("--kernel_trace", default=None,
                    help="the -d directory of a rocprofv3 kernel trace of this script: print its kernels' times and stop")
    a = ap.parse_args()
    if a.kernel_trace is not None:
        print(json.dumps(kernel_trace(a.kernel_trace)))
        return
    from scape_amd import _lib, report
    root = a.dir or tempfile.mkdtemp(prefix="boot_pa_len_timing_")
    out = {"records": a.records, "cells": a.cells, "n_boot": a.n_boot, "groups": a.groups}
    try:
        if not os.path.exists(os.path.join(root, "nz.npz")):
            os.makedirs(root, exist_ok=True)
            make_dir(root, a.records, a.cells)
        z = np.load(os.path.join(root, "nz.npz"))
        out.update(rows=int(z["rec_rows"][-1]), nonzeros=int(z["row_off"][-1]), device=_lib.default_context().name())
        clu = make_groups(root, int(z["n_cells"]), a.groups)
        out["diff_pa_len_groups"] = timed(lambda n, seed: report._diff_pa_len_groups(root, "res.gene.pkl", clu, (), n, seed),
                                          a.n_boot, a.seed)
        out["boot_pa_len"] = timed(lambda n, seed: report._boot_pa_len(root, "res.gene.pkl", clu, (), n, "95", seed),
                                   a.n_boot, a.seed)
    finally:
        if a.dir is None:
            shutil.rmtree(root, ignore_errors=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
