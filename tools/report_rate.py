#!/usr/bin/env python3
"""End-to-end rate of `scape ex_pa_cnt_mat` and `scape cal_exp_pa_len` (scape_amd/report.py) on a synthetic merged
result stream: by default 20,000 records over 33,088 barcodes, 1,500-4,500 reads each (about 60 M reads), K = 1..4,
and a cluster file with 12 groups.  Prints one JSON line with the wall time of each command and its stage times
(report.LAST_TIMES): decode = unpickling the stream; h2d_counts = uploads, count / histogram kernels and the small
read-backs; render = row-length / scan / render kernels and the copy of the text to the host, as far as the host
waits for them; gzip_wait = time the host waits for the compressing threads; finish = host post-processing and the
csv write.  Kernel times: run it under `rocprofv3 --kernel-trace --stats -d <dir> -- python tools/report_rate.py ...`.
`--format mtx` runs the count matrix as the Matrix Market directory instead of the dense file (`both`: one after the
other on the same stream) and adds its text bytes per file, rows and nnz (entries); its `finish` is the header write
and the copy of the body behind it.
`--pseudobulk` adds `ex_pa_pseudobulk` on the same stream with groups.csv (12 clusters x 6 splits = 72 samples): its
`render` is the segment-sum kernel and the read-back of its sums, `finish` the pct division and the csv lines.
`--repeat N` runs every command N times and reports the median wall time (and that run's stage times).

    python tools/report_rate.py [--records N] [--reads N] [--cells N] [--format tsv|mtx|both] [--pseudobulk]
                                [--repeat N]
"""
import argparse
import contextlib
import gzip
import io
import json
import os
import pickle
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make_dir(root, n_rec, reads, n_cells, seed=7):
    """output_dir with barcode_index.csv, groups.csv and res.gene.pkl (records pickled as merge_pa writes them)"""
    from scape.apa_core import Parameters
    rng = np.random.default_rng(seed)
    os.makedirs(os.path.join(root, "pkl_input"), exist_ok=True)
    os.makedirs(os.path.join(root, "pkl_output"), exist_ok=True)
    with open(os.path.join(root, "barcode_index.csv"), "w") as fh:
        fh.write("CB,index\n" + "".join(f"C1_{i:016d}-1,{i}\n" for i in range(n_cells)))
    with open(os.path.join(root, "groups.csv"), "w") as fh:
        fh.write("index,group\n" + "".join(f"{i},type{i % 12}\n" for i in range(n_cells)))
    n_reads = 0
    with open(os.path.join(root, "res.gene.pkl"), "wb") as fh:
        for r in range(n_rec):
            K = int(rng.integers(1, 5))
            alpha = np.sort(rng.choice(np.arange(100, 3000), K, replace=False)).astype(np.int64)
            n = int(rng.integers(reads // 2, reads * 3 // 2 + 1))
            p = Parameters(title="Final Result", alpha_arr=alpha, beta_arr=rng.choice([5.0, 10.0, 30.0], K),
                           ws=np.full(K, 1.0 / K), L=0, cb_id_arr=rng.integers(0, n_cells, n).astype(np.int64),
                           readID_arr=np.arange(n, dtype=np.int64))
            p.label_arr = rng.integers(0, K, n).astype(np.int64)
            p.gene_info_str = f"{1 + r % 22}:ENSG{r:011d}:1:{1000 * r + 1}-{1000 * r + 4000}:{'+-'[r % 2]}"
            pickle.dump(p, fh)
            n_reads += n
    return n_reads


def gz_text(path):
    """decompressed bytes of a gzip file and its first 256 decompressed bytes"""
    text, head = 0, b""
    with gzip.open(path, "rb") as fh:
        while True:
            b = fh.read(1 << 26)
            if not b:
                break
            head = head or b[:256]
            text += len(b)
    return text, head


def size(path):
    if os.path.isdir(path):
        return sum(os.path.getsize(os.path.join(path, n)) for n in os.listdir(path))
    return os.path.getsize(path)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=20000)
    ap.add_argument("--reads", type=int, default=3000)
    ap.add_argument("--cells", type=int, default=33088)
    ap.add_argument("--format", choices=("tsv", "mtx", "both"), default="tsv",
                    help="count matrix: the dense file (default), the Matrix Market directory, or both")
    ap.add_argument("--pseudobulk", action="store_true", help="also run ex_pa_pseudobulk with the 12-group file")
    ap.add_argument("--repeat", type=int, default=1, help="runs per command; the median wall time is reported")
    a = ap.parse_args()
    from scape_amd import _lib, report
    root = tempfile.mkdtemp(prefix="report_rate_")
    out = {"records": a.records, "cells": a.cells}
    try:
        t0 = time.perf_counter()
        out["reads"] = make_dir(root, a.records, a.reads, a.cells)
        out["make_s"] = time.perf_counter() - t0
        out["res_pkl_bytes"] = os.path.getsize(os.path.join(root, "res.gene.pkl"))
        out["device"] = _lib.default_context().name()
        runs = []
        if a.format in ("tsv", "both"):
            runs.append(("ex_pa_cnt_mat", lambda: report._ex_pa_cnt_mat(root, "res.gene.pkl")))
        if a.format in ("mtx", "both"):
            runs.append(("ex_pa_cnt_mat_mtx", lambda: report._ex_pa_cnt_mat(root, "res.gene.pkl", fmt="mtx")))
        if a.pseudobulk:
            runs.append(("ex_pa_pseudobulk",
                         lambda: report._ex_pa_pseudobulk(root, "res.gene.pkl", os.path.join(root, "groups.csv"))))
        runs += [("cal_exp_pa_len", lambda: report._cal_exp_pa_len(root, "None", "res.gene.pkl")),
                 ("cal_exp_pa_len_groups",
                  lambda: report._cal_exp_pa_len(root, os.path.join(root, "groups.csv"), "res.gene.pkl"))]
        for name, fn in runs:
            tries = []
            for _ in range(max(a.repeat, 1)):
                t0 = time.perf_counter()
                with contextlib.redirect_stdout(io.StringIO()):
                    path = fn()
                tries.append((time.perf_counter() - t0, dict(report.LAST_TIMES)))
            wall, stages = sorted(tries, key=lambda t: t[0])[len(tries) // 2]
            out[name] = {"wall_s": wall, "stages_s": stages, "walls_s": [t[0] for t in tries],
                         "out_bytes": sum(size(p) for p in path) if isinstance(path, list) else size(path)}
        if "ex_pa_cnt_mat" in out:
            m = out["ex_pa_cnt_mat"]
            m["text_bytes"] = gz_text(os.path.join(root, "res.gene.cnt.tsv.gz"))[0]
            m["text_GB_per_s"] = m["text_bytes"] / m["wall_s"] / 1e9
        if "ex_pa_cnt_mat_mtx" in out:
            m = out["ex_pa_cnt_mat_mtx"]
            d = os.path.join(root, "res.gene.cnt")
            m["text_bytes_per_file"] = {n: gz_text(os.path.join(d, n))[0] for n in report.MTX_FILES}
            m["out_bytes_per_file"] = {n: os.path.getsize(os.path.join(d, n)) for n in report.MTX_FILES}
            m["text_bytes"] = sum(m["text_bytes_per_file"].values())
            m["text_GB_per_s"] = m["text_bytes"] / m["wall_s"] / 1e9
            rows, cols, nnz = gz_text(os.path.join(d, "matrix.mtx.gz"))[1].split(b"\n")[1].split()
            m.update(rows=int(rows), cols=int(cols), nnz=int(nnz))
        if "ex_pa_pseudobulk" in out:
            m = out["ex_pa_pseudobulk"]
            with open(os.path.join(root, "groups.gene.pseudobulk.cnt.csv")) as fh:
                lines = fh.read().splitlines()
            m.update(rows=len(lines) - 1, samples=lines[0].count(","),
                     count_bytes_summed=(len(lines) - 1) * a.cells * 4)
    finally:
        shutil.rmtree(root, ignore_errors=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
