#!/usr/bin/env python3
"""Timing of `scape diff_pa` (scape_amd/report.py) on a synthetic directory of stated shape: by default 2,000 records
(K = 2..8 pA sites, 10,000 count rows) x 20,000 cells (8,000 in cluster A, 12,000 in B) x 9,999 permutations; 95 % of
the (site, cell) counts are zero, the others 1..3.  One warm-up run (255 permutations) and then one timed run, whose
stage times (report.LAST_TIMES) go into one JSON line: decode = unpickling; h2d_counts = uploads and the count
kernels; render = everything else the device does (the masks, the two-segment sums, compaction and the test kernel,
with the waits for them); finish = the host's numpy columns and the csv write.  `nz_x_perm` is the number of integer
additions the test stands for: nonzero counts of the tested rows x permutations.  Kernel times:

    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/diff_pa_timing.py --dir <made before> --gpu-only

`--numpy N` times a vectorised-numpy restatement of the counting (the same keys, selection, integer sums and f64
statistics; per permutation one gather over the nonzeros and one segmented sum) for N permutations on `--threads`
host threads and reports that time scaled linearly to `--n_perm`, labelled as scaled.  The restatement's counts for
its N permutations are compared with a GPU run of the same N (`numpy_equals_gpu`) unless --numpy-only is given.

`--strata N` runs the command with --strata_file: N strata of unequal sizes over the same cells (stratum k of 0 .. N-1
holds about (k + 1) / (1 + 2 + ... + N) of them, so N = 200 on 20,000 cells gives strata of 1 to 200 cells and N = 8
strata of 555 to 4,444; N = 1 is one stratum of every cell), each with about the populations' overall mix.  The numpy
restatement knows no strata and is not run with it.

    python tools/diff_pa_timing.py [--records N] [--cells N] [--n_perm N] [--dir D] [--numpy N] [--threads N]
                                   [--gpu-only | --numpy-only] [--strata N]
"""
import argparse
import contextlib
import csv
import io
import json
import math
import os
import pickle
import shutil
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

G = np.uint64(0x9E3779B97F4A7C15)
DENSITY = 0.05


def make_dir(root, n_rec, n_cells, seed=7, sites=(2, 8)):
    """output_dir with barcode_index.csv, groups.csv, res.gene.pkl and nz.npz (the nonzeros the records were made of:
    row offsets per record, per row its columns and counts); the records' K cycles through sites[0] .. sites[1]"""
    from scape.apa_core import Parameters
    rng = np.random.default_rng(seed)
    os.makedirs(os.path.join(root, "pkl_input"), exist_ok=True)
    os.makedirs(os.path.join(root, "pkl_output"), exist_ok=True)
    n_a = n_cells * 2 // 5
    with open(os.path.join(root, "barcode_index.csv"), "w") as fh:
        fh.write("CB,index\n" + "".join(f"C1_{i:016d}-1,{i}\n" for i in range(n_cells)))
    with open(os.path.join(root, "groups.csv"), "w") as fh:
        fh.write("index,group\n" + "".join(f"{i},{'A' if i < n_a else 'B'}\n" for i in range(n_cells)))
    rec_rows, row_off, cols, cnts = [0], [0], [], []
    with open(os.path.join(root, "res.gene.pkl"), "wb") as fh:
        for r in range(n_rec):
            K = sites[0] + r % (sites[1] - sites[0] + 1)
            m = (rng.random((K, n_cells)) < DENSITY) * rng.integers(1, 4, (K, n_cells))
            lab, cell = np.nonzero(m)
            c = m[lab, cell]
            for k in range(K):
                sel = lab == k
                cols.append(cell[sel].astype(np.int32))
                cnts.append(c[sel].astype(np.int32))
                row_off.append(row_off[-1] + int(sel.sum()))
            rec_rows.append(rec_rows[-1] + K)
            lab, cell = np.repeat(lab, c), np.repeat(cell, c)
            alpha = np.sort(rng.choice(np.arange(100, 3000), K, replace=False)).astype(np.int64)
            p = Parameters(title="Final Result", alpha_arr=alpha, beta_arr=rng.choice([5.0, 10.0, 30.0], K),
                           ws=np.full(K, 1.0 / K), L=0, cb_id_arr=cell.astype(np.int64),
                           readID_arr=np.arange(len(cell), dtype=np.int64))
            p.label_arr = lab.astype(np.int64)
            p.gene_info_str = f"{1 + r % 22}:ENSG{r:011d}:1:{1000 * r + 1}-{1000 * r + 4000}:{'+-'[r % 2]}"
            pickle.dump(p, fh)
    np.savez(os.path.join(root, "nz.npz"), rec_rows=np.array(rec_rows), row_off=np.array(row_off),
             cols=np.concatenate(cols), cnts=np.concatenate(cnts), n_a=n_a, n_cells=n_cells)


def make_strata(root, n_cells, n_strata):
    """strata_<N>.csv: cell i, scrambled to (7919 i) mod n_cells so that every stratum mixes the two clusters, falls
    into stratum k by the cumulative shares (k + 1) / (N (N + 1) / 2).  Returns (path, cells per stratum)"""
    if math.gcd(7919, n_cells) != 1:
        raise SystemExit("--strata needs a number of cells that is no multiple of 7919")
    total = n_strata * (n_strata + 1) // 2
    ends = (np.cumsum(np.arange(1, n_strata + 1)) * n_cells + total - 1) // total
    stratum = np.searchsorted(ends, (np.arange(n_cells) * 7919) % n_cells, side="right")
    path = os.path.join(root, f"strata_{n_strata}.csv")
    with open(path, "w") as fh:
        fh.write("index,stratum\n" + "".join(f"{i},s{k}\n" for i, k in enumerate(stratum.tolist())))
    return path, np.bincount(stratum, minlength=n_strata)


def _mix(z):
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def numpy_counts(root, n_perm, seed, threads):
    """(site_n_ge, gene_n_ge, seconds) of permutations 1 .. n_perm, restated in numpy.  Every row of the synthetic
    matrix has reads and every cell a cluster, so every row and record is tested; positions = columns."""
    z = np.load(os.path.join(root, "nz.npz"))
    rec_rows, row_off, cols, cnts = z["rec_rows"], z["row_off"], z["cols"], z["cnts"].astype(np.int64)
    n1, n = int(z["n_a"]), int(z["n_cells"])
    t0 = time.perf_counter()
    t = np.add.reduceat(cnts, row_off[:-1])
    rec_of = np.repeat(np.arange(len(rec_rows) - 1), np.diff(rec_rows))
    T = np.add.reduceat(t, rec_rows[:-1])[rec_of]
    slack = 1.0 - 2.0 ** -40

    def stats(member):
        a = np.add.reduceat(cnts * member[cols], row_off[:-1])
        A = np.add.reduceat(a, rec_rows[:-1])[rec_of]
        B = T - A
        N = (a * T - t * A).astype(np.float64)
        ab = A.astype(np.float64) * B.astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            d = np.where(ab > 0, N / ab, 0.0)
            term = np.where(ab > 0, N * N / (t.astype(np.float64) * A.astype(np.float64) * B.astype(np.float64)), 0.0)
        return np.abs(d), np.add.reduceat(term, rec_rows[:-1])

    d0, S0 = stats((np.arange(n) < n1).astype(np.int64))
    j = np.arange(n, dtype=np.uint64)

    def one(p):
        with np.errstate(over="ignore"):
            base = _mix(np.uint64(seed) + G * np.uint64(p))
            keys = (_mix(base + G * (j + np.uint64(1))) & ~np.uint64(0xFFFFFF)) | j
        member = np.zeros(n, dtype=np.int64)
        member[np.argpartition(keys, n1 - 1)[:n1]] = 1
        d, S = stats(member)
        return d >= d0 * slack, S >= S0 * slack

    site, gene = np.zeros(len(t), np.int64), np.zeros(len(S0), np.int64)
    with ThreadPoolExecutor(threads) as pool:
        for ds, gs in pool.map(one, range(1, n_perm + 1)):
            site += ds
            gene += gs
    return site, gene, time.perf_counter() - t0


def gpu_run(root, n_perm, seed, strata_file=None):
    from scape_amd import report
    t0 = time.perf_counter()
    kw = {} if strata_file is None else {"strata_file": strata_file}
    with contextlib.redirect_stdout(io.StringIO()):
        path = report._diff_pa(root, "res.gene.pkl", os.path.join(root, "groups.csv"), "A", "B", n_perm, seed, **kw)
    return path, time.perf_counter() - t0, dict(report.LAST_TIMES)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=2000)
    ap.add_argument("--cells", type=int, default=20000)
    ap.add_argument("--n_perm", type=int, default=9999)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--dir", default=None, help="directory to make the inputs in, or to reuse if it holds them")
    ap.add_argument("--numpy", type=int, default=0, help="permutations of the numpy restatement (0: skip it)")
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--gpu-only", action="store_true")
    ap.add_argument("--numpy-only", action="store_true")
    ap.add_argument("--strata", type=int, default=0, help="permute within this many strata of unequal sizes (0: freely)")
    a = ap.parse_args()
    if a.strata and (a.numpy or a.numpy_only):
        ap.error("--strata runs the GPU command only")
    if a.strata < 0 or a.strata > a.cells:
        ap.error("--strata must lie in 0 .. --cells")
    root = a.dir or tempfile.mkdtemp(prefix="diff_pa_timing_")
    out = {"records": a.records, "cells": a.cells, "n_perm": a.n_perm, "density": DENSITY}
    try:
        if not os.path.exists(os.path.join(root, "nz.npz")):
            os.makedirs(root, exist_ok=True)
            t0 = time.perf_counter()
            make_dir(root, a.records, a.cells)
            out["make_s"] = time.perf_counter() - t0
        z = np.load(os.path.join(root, "nz.npz"))
        out.update(rows=int(z["rec_rows"][-1]), nonzeros=int(z["row_off"][-1]), n1=int(z["n_a"]),
                   n2=int(z["n_cells"]) - int(z["n_a"]))
        strata_file = None
        if a.strata:
            strata_file, sizes = make_strata(root, int(z["n_cells"]), a.strata)
            out["strata"] = {"n": a.strata, "smallest": int(sizes.min()), "largest": int(sizes.max()),
                             "up_to_64_cells": int((sizes <= 64).sum()), "up_to_256_cells": int((sizes <= 256).sum())}
        if not a.numpy_only:
            from scape_amd import _lib
            out["device"] = _lib.default_context().name()
            _path, out["warmup_wall_s"], _ = gpu_run(root, 255, a.seed, strata_file)
            path, wall, stages = gpu_run(root, a.n_perm, a.seed, strata_file)
            with open(path, newline="") as fh:
                n_lines = sum(1 for _ in fh) - 1
            out["diff_pa"] = {"wall_s": wall, "stages_s": stages, "lines": n_lines,
                              "nz_x_perm": out["nonzeros"] * a.n_perm}
        if a.numpy and not a.gpu_only:
            site, gene, secs = numpy_counts(root, a.numpy, a.seed, a.threads)
            out["numpy"] = {"n_perm": a.numpy, "threads": a.threads, "seconds": secs,
                            "seconds_scaled_to_n_perm": secs * a.n_perm / a.numpy, "scaled": True}
            if not a.numpy_only:
                path, _w, _s = gpu_run(root, a.numpy, a.seed)
                with open(path, newline="") as fh:
                    body = list(csv.reader(fh))[1:]
                same = [int(r[8]) for r in body] == site.tolist() and \
                    [int(r[12]) for r in body] == np.repeat(gene, np.diff(z["rec_rows"])).tolist()
                out["numpy"]["numpy_equals_gpu"] = bool(same)
    finally:
        if a.dir is None:
            shutil.rmtree(root, ignore_errors=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
