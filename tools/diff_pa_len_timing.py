#!/usr/bin/env python3
"""Timing of `scape diff_pa_len` (scape_amd/report.py) on the synthetic directory of tools/diff_pa_timing.py, by default
its shape: 2,000 records (K = 2..8 pA sites) x 20,000 cells (8,000 in cluster A, 12,000 in B) x 9,999 permutations.
One process runs a warm-up (`diff_pa`, 255 permutations), then `diff_pa` and then `diff_pa_len`, each once with
--n_perm permutations; the stage times of both (report.LAST_TIMES, keys as in tools/diff_pa_timing.py) go into one
JSON line, so that the two test kernels can be read from one kernel trace of that process:

    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/diff_pa_len_timing.py --dir <made before>

    python tools/diff_pa_len_timing.py [--records N] [--cells N] [--n_perm N] [--seed N] [--dir D]
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

from diff_pa_timing import DENSITY, make_dir  # noqa: E402


def run(command, root, n_perm, seed):
    from scape_amd import report
    fn = {"diff_pa": report._diff_pa, "diff_pa_len": report._diff_pa_len}[command]
    t0 = time.perf_counter()
    with contextlib.redirect_stdout(io.StringIO()):
        path = fn(root, "res.gene.pkl", os.path.join(root, "groups.csv"), "A", "B", n_perm, seed)
    wall = time.perf_counter() - t0
    with open(path, newline="") as fh:
        n_lines = sum(1 for _ in fh) - 1
    return {"wall_s": wall, "stages_s": dict(report.LAST_TIMES), "lines": n_lines}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=2000)
    ap.add_argument("--cells", type=int, default=20000)
    ap.add_argument("--n_perm", type=int, default=9999)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--dir", default=None, help="directory to make the inputs in, or to reuse if it holds them")
    a = ap.parse_args()
    root = a.dir or tempfile.mkdtemp(prefix="diff_pa_len_timing_")
    out = {"records": a.records, "cells": a.cells, "n_perm": a.n_perm, "density": DENSITY}
    try:
        if not os.path.exists(os.path.join(root, "nz.npz")):
            os.makedirs(root, exist_ok=True)
            t0 = time.perf_counter()
            make_dir(root, a.records, a.cells)
            out["make_s"] = time.perf_counter() - t0
        z = np.load(os.path.join(root, "nz.npz"))
        out.update(rows=int(z["rec_rows"][-1]), nonzeros=int(z["row_off"][-1]), n1=int(z["n_a"]),
                   n2=int(z["n_cells"]) - int(z["n_a"]), nz_x_perm=int(z["row_off"][-1]) * a.n_perm)
        from scape_amd import _lib
        out["device"] = _lib.default_context().name()
        out["warmup_wall_s"] = run("diff_pa", root, 255, a.seed)["wall_s"]
        out["diff_pa"] = run("diff_pa", root, a.n_perm, a.seed)
        out["diff_pa_len"] = run("diff_pa_len", root, a.n_perm, a.seed)
    finally:
        if a.dir is None:
            shutil.rmtree(root, ignore_errors=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
