#!/usr/bin/env python3
"""Timing of `scape diff_pa_pairs` (scape_amd/report.py) against the loop of `scape diff_pa` commands it replaces, on
the synthetic directory of tools/diff_pa_timing.py: by default 2,000 records (K = 2..8 pA sites, about 10,000 count
rows) x 20,000 cells x 9,999 permutations, 95 % of the (site, cell) counts zero, the cells cut into G = 12 equal-sized
clusters (cell i in cluster i * G // cells).  In one process and session: a warm-up run of each command with 255
permutations, then the timed `diff_pa_pairs` run and the timed loop of the G (G - 1) / 2 `diff_pa` runs, one per pair in
the order of the pairs file's blocks.  One JSON line holds both wall times, the stage times (report.LAST_TIMES; for the
loop their sums over its runs) and `blocks_equal_diff_pa`: whether every block of the pairs file equals the file of the
loop's run on that pair in every shared column but the two adjusted p-values, compared as text.  Kernel times:

    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/diff_pa_pairs_timing.py --dir <made before>

    python tools/diff_pa_pairs_timing.py [--records N] [--cells N] [--n_perm N] [--dir D] [--groups G]
"""
import argparse
import contextlib
import csv
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

from diff_pa_groups_timing import make_groups  # noqa: E402
from diff_pa_timing import make_dir  # noqa: E402


def quiet(fn, *args):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*args)


def body(path):
    with open(path, newline="") as fh:
        return list(csv.reader(fh))[1:]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=2000)
    ap.add_argument("--cells", type=int, default=20000)
    ap.add_argument("--n_perm", type=int, default=9999)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--dir", default=None, help="directory to make the inputs in, or to reuse if it holds them")
    ap.add_argument("--groups", type=int, default=12, help="number of equal-sized clusters")
    a = ap.parse_args()
    from scape_amd import _lib, report
    root = a.dir or tempfile.mkdtemp(prefix="diff_pa_pairs_timing_")
    G = a.groups
    pairs = [(f"g{g}", f"g{h}") for g in range(G) for h in range(g + 1, G)]
    out = {"records": a.records, "cells": a.cells, "n_perm": a.n_perm, "groups": G, "pairs": len(pairs)}
    try:
        if not os.path.exists(os.path.join(root, "nz.npz")):
            os.makedirs(root, exist_ok=True)
            make_dir(root, a.records, a.cells)
        z = np.load(os.path.join(root, "nz.npz"))
        clu = make_groups(root, int(z["n_cells"]), G)
        out.update(rows=int(z["rec_rows"][-1]), nonzeros=int(z["row_off"][-1]), device=_lib.default_context().name())
        quiet(report._diff_pa_pairs, root, "res.gene.pkl", clu, (), 255, a.seed)
        quiet(report._diff_pa, root, "res.gene.pkl", clu, *pairs[0], 255, a.seed)

        t0 = time.perf_counter()
        pairs_path = quiet(report._diff_pa_pairs, root, "res.gene.pkl", clu, (), a.n_perm, a.seed)
        out["diff_pa_pairs"] = {"wall_s": time.perf_counter() - t0, "stages_s": dict(report.LAST_TIMES)}

        stages, paths = {}, []
        t0 = time.perf_counter()
        for id1, id2 in pairs:
            paths.append(quiet(report._diff_pa, root, "res.gene.pkl", clu, id1, id2, a.n_perm, a.seed))
            for k, v in report.LAST_TIMES.items():
                stages[k] = stages.get(k, 0.0) + v
        out["diff_pa_loop"] = {"wall_s": time.perf_counter() - t0, "stages_s": stages}
        out["loop_over_pairs"] = out["diff_pa_loop"]["wall_s"] / out["diff_pa_pairs"]["wall_s"]

        got = body(pairs_path)
        out["diff_pa_pairs"]["lines"] = len(got)
        want = [r[:2] + list(pair) + r[2:] for pair, path in zip(pairs, paths) for r in body(path)]
        adj = (report.DIFF_PA_PAIRS_HEADER.index("p_val_adj"), report.DIFF_PA_PAIRS_HEADER.index("gene_p_val_adj"))
        strip = lambda rows: [[v for j, v in enumerate(r) if j not in adj] for r in rows]
        out["blocks_equal_diff_pa"] = strip(got) == strip(want)
    finally:
        if a.dir is None:
            shutil.rmtree(root, ignore_errors=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
