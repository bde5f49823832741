#!/usr/bin/env python3
"""Timing of `scape ex_pa_len_mat` (scape_amd/report.py) on the synthetic directory of tools/diff_pa_timing.py: by
default 2,000 records (K = 2..8 pA sites, 10,000 count rows) x 20,000 cells; 95 % of the (site, cell) counts are zero,
the others 1..3.  In one process, after one warm-up run of each command:

* `ex_pa_len_mat`, `--repeats` timed runs: wall time and the stage times of report.LAST_TIMES (decode = unpickling;
  h2d_counts = uploads and the count kernels; render = the two render passes per block with their waits; gzip_wait =
  waiting for the host's gzip threads; finish = header and body into the final files);
* `ex_pa_cnt_mat --format mtx` on the same stream, the same number of runs: it walks the same count rows once, the new
  command once per matrix;
* `cal_exp_pa_len` with a cluster file that puts every cell in a cluster of its own, the only route to per-cell values
  without the command, on the first `--per_cell_records` records only (its host loop is quadratic in the cells of a
  record); `seconds_scaled_to_records` scales that time linearly to all records and is labelled as scaled.

One JSON line goes to stdout.  Kernel times come from one kernel trace, in a process of its own, of one run of the new
command and one of `ex_pa_cnt_mat --format mtx` behind it (no warm-up, nothing timed on the host):

    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/ex_pa_len_mat_timing.py --dir <made before> --only both

    python tools/ex_pa_len_mat_timing.py [--records N] [--cells N] [--dir D] [--repeats N] [--per_cell_records N]
                                         [--only len_mat|both]
"""
import argparse
import contextlib
import io
import json
import os
import pickle
import shutil
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def timed(fn, repeats):
    """one warm-up call, then `repeats` timed ones: wall seconds and the stage times of each, and the median wall"""
    from scape_amd import report
    runs = []
    for k in range(repeats + 1):
        t0 = time.perf_counter()
        with contextlib.redirect_stdout(io.StringIO()):
            fn()
        wall = time.perf_counter() - t0
        if k:
            runs.append({"wall_s": wall, "stages_s": dict(report.LAST_TIMES)})
        else:
            warm = wall
    return {"warmup_wall_s": warm, "runs": runs, "median_wall_s": statistics.median(r["wall_s"] for r in runs)}


def dir_bytes(path):
    """file sizes of a Matrix Market directory and the 'rows columns entries' line of its matrix"""
    import gzip
    out = {name: os.path.getsize(os.path.join(path, name)) for name in sorted(os.listdir(path))}
    with gzip.open(os.path.join(path, "matrix.mtx.gz"), "rt") as fh:
        fh.readline()
        out["matrix_header"] = fh.readline().strip()
    return out


def per_cell_route(root, n_cells, n_rec):
    """cal_exp_pa_len on the first n_rec records with one cluster per cell: (seconds, lines written)"""
    from scape_amd import report
    clu = os.path.join(root, "per_cell.csv")
    with open(clu, "w") as fh:
        fh.write("index,group\n" + "".join(f"{i},cell{i}\n" for i in range(n_cells)))
    with open(os.path.join(root, "res.gene.pkl"), "rb") as src, open(os.path.join(root, "res.sub.pkl"), "wb") as fh:
        for _k in range(n_rec):          # make_dir's own records, so plain pickle may read them
            pickle.dump(pickle.load(src), fh)
    t0 = time.perf_counter()
    with contextlib.redirect_stdout(io.StringIO()):
        path = report._cal_exp_pa_len(root, clu, "res.sub.pkl")
    secs = time.perf_counter() - t0
    with open(path) as fh:
        return secs, sum(1 for _ in fh) - 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=2000)
    ap.add_argument("--cells", type=int, default=20000)
    ap.add_argument("--dir", default=None, help="directory to make the inputs in, or to reuse if it holds them")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--per_cell_records", type=int, default=50)
    ap.add_argument("--only", choices=["len_mat", "both"], default=None,
                    help="for a kernel trace: one run of the new command, with `both` one of ex_pa_cnt_mat --format mtx behind it")
    a = ap.parse_args()
    from diff_pa_timing import DENSITY, make_dir
    from scape_amd import _lib, report
    root = a.dir or tempfile.mkdtemp(prefix="ex_pa_len_mat_timing_")
    out = {"records": a.records, "cells": a.cells, "density": DENSITY, "repeats": a.repeats}
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
                report._ex_pa_len_mat(root, "res.gene.pkl")
                out["stages_s"] = dict(report.LAST_TIMES)
                out["file_bytes"] = dir_bytes(os.path.join(root, "res.gene.len"))
                if a.only == "both":
                    report._ex_pa_cnt_mat(root, "res.gene.pkl", fmt="mtx")
                    out["cnt_mtx_stages_s"] = dict(report.LAST_TIMES)
        else:
            out["device"] = _lib.default_context().name()
            out["ex_pa_len_mat"] = timed(lambda: report._ex_pa_len_mat(root, "res.gene.pkl"), a.repeats)
            out["ex_pa_len_mat"]["file_bytes"] = dir_bytes(os.path.join(root, "res.gene.len"))
            out["ex_pa_cnt_mat_mtx"] = timed(lambda: report._ex_pa_cnt_mat(root, "res.gene.pkl", fmt="mtx"), a.repeats)
            out["ex_pa_cnt_mat_mtx"]["file_bytes"] = dir_bytes(os.path.join(root, "res.gene.cnt"))
            n_sub = min(a.per_cell_records, a.records)
            if n_sub:
                secs, lines = per_cell_route(root, int(z["n_cells"]), n_sub)
                out["cal_exp_pa_len_per_cell"] = {"records": n_sub, "seconds": secs, "lines": lines, "scaled": True,
                                                  "seconds_scaled_to_records": secs * a.records / n_sub}
    finally:
        if a.dir is None:
            shutil.rmtree(root, ignore_errors=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
