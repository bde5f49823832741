#!/usr/bin/env python3
"""Timing of `scape diff_pa_groups` (scape_amd/report.py) on the synthetic directory of tools/diff_pa_timing.py: by
default 2,000 records (K = 2..8 pA sites, about 10,000 count rows) x 20,000 cells x 9,999 permutations, 95 % of the
(site, cell) counts zero.  The cells are cut into G equal-sized clusters (cell i in cluster i * G // cells) for each G
of --groups (default 2, 4, 12, 32), and `scape diff_pa` (cluster A against B of the same directory) runs on the same
stream in the same process as the yardstick.  Per command: one warm-up run with 255 permutations, then one timed run
whose wall time and stage times (report.LAST_TIMES; `render` holds everything the device does apart from the counting:
labels or masks, segment sums, compaction, the test kernel and the waits for them) go into one JSON line.  Kernel times:

    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/diff_pa_groups_timing.py --dir <made before>

    python tools/diff_pa_groups_timing.py [--records N] [--cells N] [--n_perm N] [--dir D] [--groups 2,4,12,32]
"""
import argparse
import contextlib
import io
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

from diff_pa_timing import make_dir  # noqa: E402


def make_groups(root, n_cells, G):
    path = os.path.join(root, f"groups_{G}.csv")
    with open(path, "w") as fh:
        fh.write("index,group\n" + "".join(f"{i},g{i * G // n_cells}\n" for i in range(n_cells)))
    return path


def timed(fn, n_perm, seed):
    from scape_amd import report
    out = {}
    for key, n in (("warmup_wall_s", 255), ("wall_s", n_perm)):
        t0 = time.perf_counter()
        with contextlib.redirect_stdout(io.StringIO()):
            path = fn(n, seed)
        out[key] = time.perf_counter() - t0
    out["stages_s"] = dict(report.LAST_TIMES)
    with open(path, newline="") as fh:
        out["lines"] = sum(1 for _ in fh) - 1
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=2000)
    ap.add_argument("--cells", type=int, default=20000)
    ap.add_argument("--n_perm", type=int, default=9999)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--dir", default=None, help="directory to make the inputs in, or to reuse if it holds them")
    ap.add_argument("--groups", default="2,4,12,32", help="numbers of equal-sized clusters, comma separated")
    a = ap.parse_args()
    from scape_amd import _lib, report
    root = a.dir or tempfile.mkdtemp(prefix="diff_pa_groups_timing_")
    out = {"records": a.records, "cells": a.cells, "n_perm": a.n_perm}
    try:
        if not os.path.exists(os.path.join(root, "nz.npz")):
            os.makedirs(root, exist_ok=True)
            make_dir(root, a.records, a.cells)
        z = np.load(os.path.join(root, "nz.npz"))
        n_cells = int(z["n_cells"])
        out.update(rows=int(z["rec_rows"][-1]), nonzeros=int(z["row_off"][-1]), device=_lib.default_context().name())
        out["diff_pa"] = timed(lambda n, seed: report._diff_pa(root, "res.gene.pkl", os.path.join(root, "groups.csv"),
                                                               "A", "B", n, seed), a.n_perm, a.seed)
        for G in (int(g) for g in a.groups.split(",")):
            clu = make_groups(root, n_cells, G)
            out[f"diff_pa_groups_G{G}"] = timed(
                lambda n, seed: report._diff_pa_groups(root, "res.gene.pkl", clu, (), n, seed), a.n_perm, a.seed)
    finally:
        if a.dir is None:
            shutil.rmtree(root, ignore_errors=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
