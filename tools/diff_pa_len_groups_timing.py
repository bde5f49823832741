#!/usr/bin/env python3
"""Timing of `scape diff_pa_len_groups` (scape_amd/report.py) on the synthetic directory of tools/diff_pa_timing.py: by
default 2,000 records (K = 2..8 pA sites, about 10,000 count rows) x 20,000 cells x 9,999 permutations, 95 % of the
(site, cell) counts zero.  The cells are cut into G equal-sized clusters (cell i in cluster i * G // cells) for each G
of --groups (default 2, 12, 32, 64), and `scape diff_pa_groups` runs on the same cluster file in the same process as
the yardstick: its kernel walks the same label bytes twice where this command's walks them once per slice of 32
groups.  Per command and G: one warm-up run with 255 permutations, then one timed run whose wall time and stage times
(report.LAST_TIMES; `render` holds everything the device does apart from the counting: labels, segment sums,
compaction, the test kernel and the waits for them) go into one JSON line.  Kernel times:

    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/diff_pa_len_groups_timing.py --dir <made before>

    python tools/diff_pa_len_groups_timing.py [--records N] [--cells N] [--n_perm N] [--dir D] [--groups 2,12,32,64]
"""
import argparse
import json
import os
import shutil
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from diff_pa_groups_timing import make_groups, timed  # noqa: E402
from diff_pa_timing import make_dir  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=2000)
    ap.add_argument("--cells", type=int, default=20000)
    ap.add_argument("--n_perm", type=int, default=9999)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--dir", default=None, help="directory to make the inputs in, or to reuse if it holds them")
    ap.add_argument("--groups", default="2,12,32,64", help="numbers of equal-sized clusters, comma separated")
    a = ap.parse_args()
    from scape_amd import _lib, report
    root = a.dir or tempfile.mkdtemp(prefix="diff_pa_len_groups_timing_")
    out = {"records": a.records, "cells": a.cells, "n_perm": a.n_perm}
    try:
        if not os.path.exists(os.path.join(root, "nz.npz")):
            os.makedirs(root, exist_ok=True)
            make_dir(root, a.records, a.cells)
        z = np.load(os.path.join(root, "nz.npz"))
        n_cells = int(z["n_cells"])
        out.update(rows=int(z["rec_rows"][-1]), nonzeros=int(z["row_off"][-1]), device=_lib.default_context().name())
        for G in (int(g) for g in a.groups.split(",")):
            clu = make_groups(root, n_cells, G)
            for name, fn in (("diff_pa_groups", report._diff_pa_groups), ("diff_pa_len_groups", report._diff_pa_len_groups)):
                out[f"{name}_G{G}"] = timed(lambda n, seed: fn(root, "res.gene.pkl", clu, (), n, seed), a.n_perm, a.seed)
    finally:
        if a.dir is None:
            shutil.rmtree(root, ignore_errors=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
