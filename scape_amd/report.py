"""``scape cal_exp_pa_len``, ``scape ex_pa_cnt_mat``, ``scape ex_pa_pseudobulk``, ``scape diff_pa``,
``scape diff_pa_len``, ``scape diff_pa_groups``, ``scape diff_pa_len_groups``, ``scape diff_pa_pairs``,
``scape diff_pa_markers``, ``scape diff_pa_trend``, ``scape diff_pa_len_trend`` and ``scape boot_pa_len``: the stages
after ``merge_pa`` (reference ``src/scape/utils.py:319-427`` and ``:438-553``, with ``exp_pa_len`` /
``cal_exp_pa_len_by_cluster`` of ``apa_core.py:1038-1063``).

All of them stream the ``Parameters`` records of ``res.gene.pkl`` / ``res.utr.pkl`` (``safe_pickle.iter_pickles``, like
``merge_pa``), batch them for the device and hand the per-read work to the HIP kernels of ``csrc/report.inc`` and ``csrc/perm.inc``.  They
share one host core (section "shared host core" below): ``_Run`` frames a command (stage times, ``.part`` targets, the
device context and its release), ``_read_inputs`` reads what the count-matrix commands need before the device is
opened, ``_count`` / ``_kept_rows`` give the label rows with reads of a batch, and ``_two_slot_blocks`` overlaps the
device's rendering of one text block with the gzip of the previous one.

* ``ex_pa_cnt_mat``: the device counts (record, label < K, barcode column), flags the records whose pandas pivot would
  be complete, and renders every CSV row; the host builds the quoted ``pa_info`` prefixes and gzips finished blocks on
  ``host_threads()`` threads (zlib releases the GIL) while the device renders the next block.  The file is a
  multi-member gzip whose decompressed text equals the reference's.  ``--format mtx`` writes the same rows and columns
  as a 10x-style Matrix Market directory instead; the device renders its nonzero entries from the same counts.
* ``cal_exp_pa_len``: the device builds, per record, the cluster codes present and the (cluster, label) histogram; the
  host names and orders the clusters with the reference's own ``np.unique(np.array(...))`` and finishes
  ``exp_pa_len`` with the reference's numpy expressions, so every printed digit matches by construction.
* ``ex_pa_len_mat``: ``exp_pa_len`` per (record, cell) as a Matrix Market directory, with the reads behind each value
  in a second matrix.  The host forms ``n_arr`` with the reference's numpy expression; the device divides, multiplies
  and adds in the order of numpy's pairwise sum and renders ``'%.6f'`` in exact integers (section ex_pa_len_mat below).
* ``ex_pa_usage_mat``: the usage (PSI) of every pA site per cell, the count of the site over the cell's reads of the
  record, as a Matrix Market directory on the rows and columns of ``ex_pa_cnt_mat --format mtx``, with the cell's reads
  of the record in a second matrix.  The device forms the records' column totals once, divides and renders ``'%.6f'``
  in exact integers (section ex_pa_usage_mat below).
* ``ex_pa_pseudobulk``: the count matrix summed over cell groups, the input of the reference's DEXSeq script
  (``examples/Rscript-DEXseq/DifferentialTest.R:63-104``, ``:159-184``).  The host permutes the barcode columns so
  that every pseudo-replicate is one contiguous segment of a count row; the device counts as for ``ex_pa_cnt_mat``
  and returns, per row and segment, the sum and the number of nonzero counts.  Nothing cell-level leaves the device.
* ``diff_pa``: which pA sites two cell populations use differently, by permuting the cell labels (section diff_pa
  below states the test).  The device builds the permutations' membership bits, compacts the count rows to their
  nonzeros and counts, per site and record, the permutations whose statistic reaches the observed one; the host
  turns the integers into p-values, Benjamini-Hochberg adjusted, and writes one csv.
* ``diff_pa_len``: whether one of the two populations uses longer 3'UTRs, per gene: the same populations, kept rows and
  label permutations as ``diff_pa`` (they share the code), tested on the difference of the mean pA position (section
  diff_pa_len below).  The device walks the same membership bits with one weighted sum per population; the host adds
  the exact means and the reference's ``exp_pa_len`` of both populations.
  Both take ``--strata_file`` (cell type, donor, batch, ... per cell): the labels are then permuted within each
  stratum only, which keeps a difference between strata of unequal composition out of the p-values.  Only the
  membership bits change (``k_rep_perm_mask_strata`` builds them either way: without the option every cell is in one
  stratum); the statistics stay pooled over the strata.
* ``diff_pa_groups``: the omnibus form of ``diff_pa`` for 2 to 64 populations at once (every cluster of the cluster
  file, or the ones named): the same keys rank the cells, the device cuts the ranking into the populations' sizes (one
  byte per cell and permutation) and accumulates one sum per row, population and permutation in LDS (section
  diff_pa_groups below).
* ``diff_pa_len_groups``: the omnibus form of ``diff_pa_len`` on the labellings of ``diff_pa_groups``, and every
  population's mean pA position against all the others (section diff_pa_len_groups below).
* ``diff_pa_pairs``: ``diff_pa`` for every pair of those populations from one pass over the result file, the p-values
  adjusted over all pairs (section diff_pa_pairs below).
* ``diff_pa_markers``: ``diff_pa --idents_1 X`` for every cluster X against all other clustered cells from one pass
  over the result file, the p-values adjusted over all markers (section diff_pa_markers below).
* ``diff_pa_trend`` and ``diff_pa_len_trend``: pA usage and 3'UTR length along a per-cell score such as pseudotime, by
  permuting the scores (sections diff_pa_trend and diff_pa_len_trend below).
* ``boot_pa_len``: how well a cluster's 3'UTR length is known: percentile intervals of the mean pA position and of
  ``exp_length`` per record and cluster from the cell bootstrap (section boot_pa_len below).  The device draws a
  Poisson(1) multiplicity per cell and replicate from the permutation tests' hash, forms every replicate's mean position
  from exact integer sums and selects the interval's two order statistics; the file is exact text.

Reference behaviour kept on purpose: the pivot prints integers only when it is complete (otherwise "2.0"); rows are
the labels < K with reads, in label order; ``alpha_arr`` is indexed by label, never sorted; cluster values present in a
record decide the dtype of its partition (strings mixed with NaN make NaN the string 'nan'; all-float partitions keep
NaN, whose group never matches itself and gets NaN); unknown barcode or cluster ids raise ``KeyError``.
"""
from __future__ import annotations

import contextlib
import csv
import ctypes
import decimal
import functools
import io
import math
import os
import re
import shutil
import tempfile
import zlib
from concurrent.futures import ThreadPoolExecutor
from fractions import Fraction
from timeit import default_timer as timer
from types import SimpleNamespace

import click
import numpy as np

from . import _hostlib, _lib, safe_pickle
from ._lib import P_i8, P_i32, P_i64, check, ptr

# device bytes one batch may take (None: a quarter of what the device has free) and text bytes per render block;
# the tests set both small to run several batches and blocks
MAX_BATCH_BYTES = None
MAX_BLOCK_BYTES = 256 << 20
GZIP_LEVEL = 9            # gzip.open's default, what the reference writes with
GZIP_PART = 8 << 20       # text bytes per gzip member (one host thread each)
MAX_ID_SPAN = 1 << 30     # barcode ids are looked up in a dense table over [min id, max id]
MAX_PERM_BYTES = None     # diff_pa: device bytes of one chunk of permutation bits (None: half of the batch budget)

_TIMES_KEYS = ("decode", "h2d_counts", "render", "gzip_wait", "finish")


class ReportTimes(dict):
    """Wall seconds per stage of the last command (tools/report_rate.py)."""


LAST_TIMES = ReportTimes()


# ---------------------------------------------------------------- inputs
class _IdMap:
    """dense int32 table id -> slot over [id_min, id_min + span), -1 = no such id"""

    def __init__(self, ids, slots, what):
        ids = np.asarray(ids)
        if ids.dtype.kind not in "iu":
            raise ValueError(f"{what}: the index column must hold integer ids")
        ids = ids.astype(np.int64)
        self.id_min = int(ids.min()) if len(ids) else 0
        span = (int(ids.max()) - self.id_min + 1) if len(ids) else 0
        if span > MAX_ID_SPAN:
            raise ValueError(f"{what}: barcode ids span {span} values, more than {MAX_ID_SPAN}")
        self.span = span
        self.table = np.full(max(span, 1), -1, dtype=np.int32)
        self.table[ids - self.id_min] = slots        # a repeated id keeps its last row, as DataFrame.to_dict does


def _record_arrays(recs):
    """read offsets, K, labels and cell ids of a batch of records (int64, concatenated)"""
    n = np.array([len(p.label_arr) for p in recs], dtype=np.int64)
    off = np.zeros(len(recs) + 1, dtype=np.int64)
    np.cumsum(n, out=off[1:])
    K = np.array([int(p.K) for p in recs], dtype=np.int32)
    lab = np.concatenate([np.asarray(p.label_arr) for p in recs]).astype(np.int64, copy=False) if off[-1] else \
        np.zeros(1, np.int64)
    cb = np.concatenate([np.asarray(p.cb_id_arr) for p in recs]).astype(np.int64, copy=False) if off[-1] else \
        np.zeros(1, np.int64)
    if len(lab) != max(off[-1], 1) or len(cb) != max(off[-1], 1):
        raise ValueError("a record's cb_id_arr and label_arr differ in length")
    return off, K, np.ascontiguousarray(lab), np.ascontiguousarray(cb)


def _batches(path, cost, budget, times):
    """records of the result stream in file order, grouped so that the sum of cost(record) stays within budget
    (a record above the budget goes alone)"""
    t0 = timer()
    batch, used = [], 0
    for para in safe_pickle.iter_pickles(path):
        c = cost(para)
        if batch and used + c > budget:
            times["decode"] += timer() - t0
            yield batch
            t0 = timer()
            batch, used = [], 0
        batch.append(para)
        used += c
    times["decode"] += timer() - t0
    if batch:
        yield batch


def _budget(ctx):
    if MAX_BATCH_BYTES is not None:
        return int(MAX_BATCH_BYTES)
    free = ctypes.c_int64(0)
    check(ctx.lib.scape_hip_batch_bytes(ctx.h, None, ctypes.byref(free), None), "batch_bytes")
    return max(64 << 20, free.value // 4)


def _raise_bad_read(bad, recs, off, cb, what):
    if bad[1] >= 0:
        r = int(np.searchsorted(off, bad[1], side="right") - 1)
        raise ValueError(f"{recs[r].gene_info_str}: negative label in label_arr")
    r = int(np.searchsorted(off, bad[0], side="right") - 1)
    raise KeyError(f"{recs[r].gene_info_str}: cell barcode id {int(cb[bad[0]])} is not in {what}")


# ---------------------------------------------------------------- shared host core
class _Run:
    """frame of one command, a context manager: the stage times and the start timer, one .part target per final path,
    the device context (opened by device(), after whatever the command does first) and its release.  Leaving the body
    without an exception renames every .part file to its final path and fills LAST_TIMES; leaving it either way
    removes the .part files that are left and releases the device"""

    def __init__(self, device, finals):
        self.finals, self.parts = list(finals), [p + ".part" for p in finals]
        self._device, self.ctx, self.total = device, None, None
        self.times = ReportTimes({k: 0.0 for k in _TIMES_KEYS})

    def __enter__(self):
        self.start = timer()
        return self

    def device(self):
        self.ctx = _lib.default_context(self._device)
        return self.ctx

    def release(self):
        if self.ctx is not None:
            self.ctx.lib.scape_hip_report_free(self.ctx.h)
            self.ctx = None

    def __exit__(self, exc_type, exc, tb):
        try:
            if exc_type is None:
                for tmp, path in zip(self.parts, self.finals):
                    os.replace(tmp, path)
        finally:
            for tmp in self.parts:
                if os.path.exists(tmp):
                    os.remove(tmp)
            self.release()
        if exc_type is None:
            self.total = timer() - self.start
            LAST_TIMES.clear()
            LAST_TIMES.update(self.times)
            LAST_TIMES["total"] = self.total


def _read_inputs(output_dir, res_pkl_file, cell_cluster_file=None, idents=(None, None), with_cb=False):
    """what ex_pa_cnt_mat and the cluster-aware commands read before the device is opened, after their own argument
    checks: the paths, barcode_index.csv (the CB column when with_cb, the column ids, the number of columns) and,
    with a cluster file, the populations of _populations and the cluster names in order of first appearance"""
    import pandas as pd
    res_pkl = os.path.join(output_dir, res_pkl_file)
    if not (os.path.exists(output_dir)):
        raise Exception("Given output_dir folder does not exists.")
    if not (os.path.exists(res_pkl)):
        raise Exception(f"Invalid file {res_pkl}. Given res_pkl_file is not in output_dir.")
    if cell_cluster_file is not None and not (os.path.exists(cell_cluster_file)):
        raise Exception("Given cell_cluster_file file does not exists")
    cb_df = pd.read_csv(os.path.join(output_dir, "barcode_index.csv"), index_col="index")
    cb_lst = cb_df["CB"].tolist() if with_cb else None
    n_cols = len(cb_df)
    if n_cols == 0:
        raise ValueError("barcode_index.csv lists no barcode")
    col_ids = cb_df.index.to_numpy()
    if col_ids.dtype.kind not in "iu":
        raise ValueError("barcode_index.csv: the index column must hold integer ids")
    pops = order = None
    if cell_cluster_file is not None:
        col_clu, order = _column_clusters(col_ids.astype(np.int64), *_read_clusters(cell_cluster_file))
        pops = _populations(col_clu, order, *idents)
    return SimpleNamespace(res_pkl=res_pkl, cb_lst=cb_lst, col_ids=col_ids, n_cols=n_cols, pops=pops, clusters=order)


def _out_stem(output_dir, res_pkl_file, cell_cluster_file, idents_1, idents_2):
    """<output_dir>/<cluster file stem>.<gene|utr>[.<A>_vs_<B|rest>]"""
    tag = "" if idents_1 is None else f".{idents_1}_vs_{idents_2 if idents_2 is not None else 'rest'}"
    if os.sep in tag:
        raise ValueError(f"an ident with {os.sep!r} cannot be part of a file name")
    return os.path.join(output_dir, os.path.splitext(os.path.basename(cell_cluster_file))[0] + "." +
                        res_pkl_file.replace(".pkl", "").replace("res.", "") + tag)


def _batch_cost(n_cols, count_bytes=4):
    """device bytes of a record: its counts (count_bytes per label and column) and its reads"""
    return lambda p: int(p.K) * n_cols * count_bytes + len(p.label_arr) * 16 + 64


def _count(ctx, recs, idmap, n_cols, times):
    """a counted batch: the counts stay on the device; the records, K, the row totals and the pivot-complete flags
    on the host"""
    t0 = timer()
    off, K, lab, cb = _record_arrays(recs)
    row_tot = np.zeros(int(K.sum()), dtype=np.int64)
    complete = np.zeros(len(recs), dtype=np.int8)
    bad = np.zeros(2, dtype=np.int64)
    check(ctx.lib.scape_hip_report_counts(ctx.h, len(recs), ptr(off, P_i64), ptr(K, P_i32), ptr(lab, P_i64),
                                          ptr(cb, P_i64), idmap.id_min, idmap.span, ptr(idmap.table, P_i32), n_cols,
                                          ptr(row_tot, P_i64), ptr(complete, P_i8), ptr(bad, P_i64)), "report_counts")
    times["h2d_counts"] += timer() - t0
    if bad[0] >= 0 or bad[1] >= 0:
        _raise_bad_read(bad, recs, off, cb, "barcode_index.csv")
    return SimpleNamespace(recs=recs, K=K, row_tot=row_tot, complete=complete)


def _counted(ctx, res_pkl, idmap, n_cols, cost, budget, times):
    """the counted batches of a result stream"""
    for recs in _batches(res_pkl, cost, budget, times):
        yield _count(ctx, recs, idmap, n_cols, times)


def _kept_rows(bat):
    """the label rows with reads of a counted batch: (first count row of every record, the count rows with reads
    ascending (int64), the record of each, its label within that record)"""
    K = bat.K.astype(np.int64)
    rowbase = np.cumsum(K) - K
    rows = np.nonzero(bat.row_tot > 0)[0].astype(np.int64)
    owner = np.repeat(np.arange(len(K), dtype=np.int64), K)[rows]
    return rowbase, rows, owner, rows - rowbase[owner]


def _pa_infos(recs, owner, label):
    """pa_info of kept rows, in row order (record by record, labels ascending)"""
    out = []
    first = np.nonzero(np.diff(owner, prepend=-1))[0].tolist() + [len(owner)]
    for a, b in zip(first[:-1], first[1:]):
        out.extend(_pa_info(recs[owner[a]], label[a:b]))
    return out


# ---------------------------------------------------------------- ex_pa_cnt_mat
def _csv_field(s):
    return '"' + s.replace('"', '""') + '"'


def _pa_info(para, labels):
    """pa_info of the rows `labels` of one record (utils.py:494-512: the same fields, str() of the same numpy values)"""
    gene_info = para.gene_info_str.split(sep=":")
    st, en = gene_info[3].split(sep="-")
    alpha = np.asarray(para.alpha_arr)[labels]
    loc = alpha + int(st) if gene_info[4] == "+" else int(en) - alpha + 1
    beta = np.asarray(para.beta_arr)[labels]
    head, tail = str(gene_info[0]) + ":", ":" + str(gene_info[4]) + ":"
    end = ":" + str(gene_info[1]) + ":" + str(gene_info[2])
    return [head + str(a) + ":" + str(b) + tail + str(lb + 1) + end
            for a, b, lb in zip(loc.tolist(), beta.tolist(), labels.tolist())]


def _gzip_part(view):
    co = zlib.compressobj(GZIP_LEVEL, zlib.DEFLATED, 31)
    return co.compress(view) + co.flush()


class _GzipWriter:
    """multi-member gzip: each part of the text is compressed on a pool thread, members are written in order"""

    def __init__(self, fh, pool, times):
        self.fh, self.pool, self.times = fh, pool, times
        self.pending = []        # futures in file order

    def submit(self, view):
        n = len(view)
        for a in range(0, n, GZIP_PART):
            self.pending.append(self.pool.submit(_gzip_part, view[a:min(n, a + GZIP_PART)]))

    def drain(self):
        t0 = timer()
        for f in self.pending:
            self.fh.write(f.result())
        self.pending = []
        self.times["gzip_wait"] += timer() - t0


def _hand_over(ctx, slot, writer, times):
    hp, nb = ctypes.c_void_p(), ctypes.c_int64(0)
    t0 = timer()
    check(ctx.lib.scape_hip_report_fetch(ctx.h, slot, ctypes.byref(hp), ctypes.byref(nb)), "report_fetch")
    times["render"] += timer() - t0
    writer.submit(memoryview((ctypes.c_char * nb.value).from_address(hp.value)).cast("B"))


def _two_slot_blocks(ctx, writer, blocks, render, times):
    """render(slot, a, b) for every block (a, b) of `blocks`, alternating between the device's two text slots: block
    n is gzipped on the writer's pool while the device renders block n + 1 into the other slot"""
    queued = []                  # slots rendered, not yet handed to the pool
    gzipping = False             # some slot's pinned buffer is still read by pool threads
    for blk, (a, b) in enumerate(blocks):
        slot = blk % 2
        if gzipping and blk >= 2:
            writer.drain()       # the slot's host buffer is about to be overwritten
            gzipping = False
        render(slot, a, b)
        if queued:               # the previous block is complete behind this one's scan: compress it now
            _hand_over(ctx, queued.pop(0), writer, times)
            gzipping = True
        queued.append(slot)
    for s in queued:
        _hand_over(ctx, s, writer, times)
    writer.drain()


def _cut_blocks(bound):
    """[(a, b)]: the rows 0 .. len(bound) in runs whose summed upper bounds of the text stay within MAX_BLOCK_BYTES (a
    row above it goes alone), at most 2^20 rows each"""
    cum = np.zeros(len(bound) + 1, dtype=np.int64)
    np.cumsum(bound, out=cum[1:])
    blocks, a = [], 0
    while a < len(bound):
        b = int(np.searchsorted(cum, cum[a] + MAX_BLOCK_BYTES, side="right")) - 1
        b = min(len(bound), a + (1 << 20), max(a + 1, b))
        blocks.append((a, b))
        a = b
    return blocks


def _render_batch(ctx, bat, n_cols, writer, times):
    """every row of one counted batch: prefixes on the host, text on the device, in blocks of a fixed number of rows"""
    _rowbase, rows, owner, label = _kept_rows(bat)
    if not len(rows):
        return
    is_int = np.ascontiguousarray(bat.complete[owner])
    pre_b = [_csv_field(s).encode() for s in _pa_infos(bat.recs, owner, label)]
    plen = np.array([len(b) for b in pre_b], dtype=np.int64)
    # rows per block from an upper bound of the row length (every field ',"<10 digits>.0"')
    per_row = int(plen.max()) + 15 * n_cols + 2
    step = max(1, min(1 << 20, MAX_BLOCK_BYTES // per_row))

    def render(slot, a, b):
        poff = np.zeros(b - a + 1, dtype=np.int64)
        np.cumsum(plen[a:b], out=poff[1:])
        blob = b"".join(pre_b[a:b])
        nbytes = ctypes.c_int64(0)
        t0 = timer()
        check(ctx.lib.scape_hip_report_render(ctx.h, slot, b - a, ptr(rows[a:b], P_i64), ptr(is_int[a:b], P_i8),
                                              ptr(poff, P_i64), blob, ctypes.byref(nbytes)), "report_render")
        times["render"] += timer() - t0
    _two_slot_blocks(ctx, writer, ((a, min(len(rows), a + step)) for a in range(0, len(rows), step)), render, times)


def _ex_pa_cnt_mat(output_dir: str, res_pkl_file: str, device=None, fmt="tsv"):
    """fmt "tsv": the reference's dense <res>.cnt.tsv.gz; "mtx": the directory <res>.cnt/ with matrix.mtx.gz,
    features.tsv.gz and barcodes.tsv.gz (_ex_pa_cnt_mtx)"""
    if fmt not in ("tsv", "mtx"):
        raise ValueError(f"unknown count matrix format {fmt!r} (tsv or mtx)")
    if fmt == "mtx":
        return _ex_pa_cnt_mtx(output_dir, res_pkl_file, device)
    inp = _read_inputs(output_dir, res_pkl_file, with_cb=True)
    n_cols = inp.n_cols
    idmap = _IdMap(inp.col_ids, np.arange(n_cols, dtype=np.int32), "barcode_index.csv")
    outpath = os.path.join(output_dir, res_pkl_file.replace(".pkl", ".cnt.tsv.gz"))
    hdr = io.StringIO()
    csv.writer(hdr, delimiter=',', quoting=csv.QUOTE_ALL, lineterminator='\n').writerow(["pa_info"] + inp.cb_lst)
    with _Run(device, [outpath]) as run:
        with open(run.parts[0], "wb") as fh, ThreadPoolExecutor(_hostlib.host_threads()) as pool:
            writer = _GzipWriter(fh, pool, run.times)
            writer.submit(memoryview(hdr.getvalue().encode()))
            writer.drain()
            ctx = run.device()
            for bat in _counted(ctx, inp.res_pkl, idmap, n_cols, _batch_cost(n_cols), _budget(ctx), run.times):
                _render_batch(ctx, bat, n_cols, writer, run.times)
    print("Finish counting for each gene")
    print(f"Finish {inp.res_pkl} in {run.total / 60} min.")
    return outpath


# ---------------------------------------------------------------- ex_pa_cnt_mat --format mtx
MTX_FILES = ("matrix.mtx.gz", "features.tsv.gz", "barcodes.tsv.gz")
MTX_BANNER = "%%MatrixMarket matrix coordinate integer general\n"
_POW10 = np.array([10 ** k for k in range(1, 19)], dtype=np.int64)


def _digits(a):
    """decimal digits of non-negative int64 values"""
    return 1 + np.searchsorted(_POW10, a, side="right")


def _tsv_lines(fields, per_line, what):
    """the lines of a .tsv text; a field with a tab, a newline or a carriage return is a ValueError naming it"""
    text = "".join(per_line(s) for s in fields)
    n_tabs = per_line("").count("\t")
    if "\r" in text or text.count("\n") != len(fields) or text.count("\t") != n_tabs * len(fields):
        for s in fields:
            if "\t" in s or "\n" in s or "\r" in s:
                raise ValueError(f"{what} {s!r} holds a tab or a line break: it cannot be a field of a .tsv file")
    return text


class _MtxSink:
    """gzip writers of the matrix body and of features.tsv, and the rows / entries written so far"""

    def __init__(self, matrix, features):
        self.matrix, self.features = matrix, features
        self.n_rows = self.nnz = 0


@contextlib.contextmanager
def _dir_run(device, out_dir, names):
    """the _Run of a command that writes the files `names` of the directory out_dir: the directory is made inside the
    frame, and a run that fails removes it again if it made it, so nothing of that run stays behind"""
    if os.path.exists(out_dir) and not os.path.isdir(out_dir):
        raise FileExistsError(f"{out_dir} exists and is not a directory")
    made_dir = not os.path.isdir(out_dir)
    try:
        with _Run(device, [os.path.join(out_dir, name) for name in names]) as run:
            os.makedirs(out_dir, exist_ok=True)
            yield run
    except BaseException:
        if made_dir:
            try:
                os.rmdir(out_dir)
            except OSError:
                pass
        raise


def _write_gzip(path, text, pool, times):
    with open(path, "wb") as fh:
        w = _GzipWriter(fh, pool, times)
        w.submit(memoryview(text.encode()))
        w.drain()


def _finish_mtx(path, header, body, times):
    """a Matrix Market file from its header, which holds the number of entries and so is known last, and the gzip
    members of its body, collected in the anonymous temporary file `body`"""
    t0 = timer()
    with open(path, "wb") as mfh:
        mfh.write(_gzip_part(header.encode()))
        body.seek(0)
        shutil.copyfileobj(body, mfh, 16 << 20)
    times["finish"] += timer() - t0


def _mtx_run(output_dir, res_pkl_file, tag, names, banners, device, cost, batch, refuse, done):
    """A 10x-style directory <res><tag>/ of one matrix per banner: names = the matrices' files, features.tsv.gz and
    barcodes.tsv.gz (the CB column).  batch(ctx, bat, n_cols, sinks, times) renders a counted batch of at most
    cost(n_cols) device bytes per record into the sinks, one per matrix; the first one carries features.tsv and the
    row count.  A matrix's header holds its nnz, known only at the end: its body's gzip members go to an anonymous
    temporary file and are copied behind the header's member.  refuse(*sinks), if given, returns what is wrong with
    the finished entry counts, or None.  The files are renamed from .part once all are complete; `done` is the
    command's closing message."""
    inp = _read_inputs(output_dir, res_pkl_file, with_cb=True)
    n_cols, m = inp.n_cols, len(banners)
    idmap = _IdMap(inp.col_ids, np.arange(n_cols, dtype=np.int32), "barcode_index.csv")
    bc_text = _tsv_lines([str(b) for b in inp.cb_lst], lambda s: s + "\n", "barcode")
    out_dir = os.path.join(output_dir, res_pkl_file.replace(".pkl", tag))
    with _dir_run(device, out_dir, names) as run, contextlib.ExitStack() as stack:
        bodies = [stack.enter_context(tempfile.TemporaryFile(dir=out_dir)) for _ in banners]
        ffh = stack.enter_context(open(run.parts[m], "wb"))
        pool = stack.enter_context(ThreadPoolExecutor(_hostlib.host_threads()))
        _write_gzip(run.parts[m + 1], bc_text, pool, run.times)
        sinks = [_MtxSink(_GzipWriter(body, pool, run.times), None if k else _GzipWriter(ffh, pool, run.times))
                 for k, body in enumerate(bodies)]
        ctx = run.device()
        for bat in _counted(ctx, inp.res_pkl, idmap, n_cols, cost(n_cols), _budget(ctx), run.times):
            batch(ctx, bat, n_cols, sinks, run.times)
        wrong = refuse(*sinks) if refuse else None
        if wrong:
            raise _lib.ScapeHipError(wrong)
        for path, banner, sink, body in zip(run.parts, banners, sinks, bodies):
            _finish_mtx(path, f"{banner}{sinks[0].n_rows} {n_cols} {sink.nnz}\n", body, run.times)
    print(done)
    print(f"Finish {inp.res_pkl} in {run.total / 60} min.")
    return out_dir


def _render_entries(ctx, sinks, names, noun, blocks, call, times):
    """The len(names) rows of one counted batch, numbered on from sinks[0].n_rows: their features lines (`names`, a
    `noun` each) on the host, then for every sink the Matrix Market entries on the device, in the blocks (a, b) of
    blocks[what], what = the sink's place.  call(slot, a, b, what, nbytes, nnz) issues the entry point's call for one
    block; it looks the entry point up on ctx.lib when it is called."""
    first = sinks[0]
    first.features.submit(memoryview(_tsv_lines(names, lambda s: f"{s}\t{s}\tGene Expression\n", noun).encode()))

    def render(sink, what, slot, a, b):
        nbytes, nnz = ctypes.c_int64(0), ctypes.c_int64(0)
        t0 = timer()
        call(slot, a, b, what, ctypes.byref(nbytes), ctypes.byref(nnz))
        times["render"] += timer() - t0
        sink.nnz += nnz.value
    for what, sink in enumerate(sinks):
        _two_slot_blocks(ctx, sink.matrix, blocks[what], functools.partial(render, sink, what), times)
    first.features.drain()
    first.n_rows += len(names)


def _ex_pa_cnt_mtx(output_dir, res_pkl_file, device):
    """the count matrix as a 10x-style directory <res>.cnt/: matrix.mtx.gz (the dense file's rows and columns, nonzero
    counts only, row-major), features.tsv.gz (per row: pa_info, pa_info, "Gene Expression"; Seurat's Read10X names rows
    from column 2, scanpy's read_10x_mtx from column 2 and keeps only "Gene Expression" rows) and barcodes.tsv.gz"""
    return _mtx_run(output_dir, res_pkl_file, ".cnt", MTX_FILES, (MTX_BANNER,), device, _batch_cost, _render_mtx_batch,
                    None, "Finish counting for each gene")


def _render_mtx_batch(ctx, bat, n_cols, sinks, times):
    """the kept rows of one counted batch, in blocks cut by their text size"""
    _rowbase, rows, owner, label = _kept_rows(bat)
    if not len(rows):
        return
    # blocks cut against an upper bound of each row's text: at most min(reads, barcodes) entries
    # "<row number> <column> <count>\n", the count at most the row's reads
    row_no0 = sinks[0].n_rows + 1
    tot = bat.row_tot[rows]
    width = len(str(row_no0 + len(rows) - 1)) + len(str(n_cols)) + 3 + _digits(tot)

    def call(slot, a, b, _what, nbytes, nnz):
        check(ctx.lib.scape_hip_report_render_mtx(ctx.h, slot, b - a, ptr(rows[a:b], P_i64), row_no0 + a, nbytes, nnz),
              "report_render_mtx")
    _render_entries(ctx, sinks, _pa_infos(bat.recs, owner, label), "pa_info",
                    [_cut_blocks(np.minimum(tot, n_cols) * width)], call, times)


# ---------------------------------------------------------------- ex_pa_len_mat
# Row r is the r-th record of the stream, the columns are ex_pa_cnt_mat's.  An entry stands for a cell with T >= 1 reads
# of label < K in the record: matrix.mtx.gz holds '%.6f' of the reference's exp_pa_len(record, labels of that cell's
# reads) (apa_core.py:1038-1052), reads.mtx.gz holds T at the same places.  The host forms n_arr with the reference's
# numpy expression; the weights, numpy's pairwise sum and the decimal text are the device's (include/scape_hip.h states
# them).  A record of K >= 2 whose n_arr is not all finite (a NaN alpha, alpha[-1] == alpha[0]) or reaches LEN_MAX_N is
# named on stderr and keeps its row without an entry in either matrix.
LEN_MTX_FILES = ("matrix.mtx.gz", "reads.mtx.gz", "features.tsv.gz", "barcodes.tsv.gz")
LEN_MTX_BANNER = "%%MatrixMarket matrix coordinate real general\n"
LEN_MAX_N = 2.0 ** 31 / 9     # |n_l| below it keeps |value| < 2^31, what the device's decimal text is stated for


def _len_n_arr(para):
    """(n_arr of exp_pa_len as the reference's numpy expression gives it, whether the record has values); K == 1 has
    the value 1.0 and no n_arr"""
    K = int(para.K)
    if K == 1:
        return np.ones(1), True
    a_arr = np.asarray(para.alpha_arr)
    if len(a_arr) != K:
        raise ValueError(f"{para.gene_info_str}: alpha_arr holds {len(a_arr)} values, K is {K}")
    with np.errstate(all="ignore"):
        n_arr = np.asarray(1.0 + 9.0 * (a_arr - a_arr[0]) / (a_arr[-1] - a_arr[0]), dtype=np.float64)
        ok = bool(np.all(np.isfinite(n_arr)) and np.all(np.abs(n_arr) < LEN_MAX_N))
    return n_arr, ok


def _render_len_batch(ctx, bat, n_cols, sinks, times):
    """the records of one counted batch into the value and the reads matrix (from the same counts), in blocks cut by
    their text size"""
    recs, K = bat.recs, bat.K.astype(np.int64)
    n_rec = len(recs)
    rowbase = np.ascontiguousarray(np.cumsum(K) - K)
    n_arrs, oks = zip(*(_len_n_arr(p) for p in recs))
    for p, ok in zip(recs, oks):
        if not ok:
            click.echo(f"{p.gene_info_str}: alpha_arr gives no finite expected pA length below 2^31: no entry", err=True)
    skip = np.array([not ok for ok in oks], dtype=np.int8)
    n_len = np.array([len(a) for a in n_arrs], dtype=np.int64)
    n_off = np.ascontiguousarray(np.cumsum(n_len) - n_len)
    n_arr = np.ascontiguousarray(np.concatenate(n_arrs))
    n_arr[np.repeat(skip, n_len) != 0] = 0.0     # never read by the device
    Ks = np.ascontiguousarray(bat.K)
    # blocks cut against an upper bound of each record's text: at most min(reads, barcodes) entries "<row number>
    # <column> <field>\n", the field at most the sign, the digits of the record's largest |n_l| + 1, the point and six
    # digits, or the digits of the record's reads
    row_no0 = sinks[0].n_rows + 1
    tot = np.add.reduceat(bat.row_tot, rowbase) * (skip == 0)
    big = np.array([float(np.max(np.abs(a))) for a in n_arrs])
    big[skip != 0] = 0.0
    field = np.maximum(8 + _digits(big.astype(np.int64) + 1), _digits(tot))
    width = len(str(row_no0 + n_rec - 1)) + len(str(n_cols)) + 3 + field
    blocks = _cut_blocks(np.minimum(tot, n_cols) * width)

    def call(slot, a, b, what, nbytes, nnz):
        first = int(n_off[a])            # the block's part of n_arr
        check(ctx.lib.scape_hip_report_render_len_mtx(
            ctx.h, slot, b - a, ptr(rowbase[a:b], P_i64), ptr(Ks[a:b], P_i32), ptr(n_off[a:b] - first, P_i64),
            ptr(n_arr[first:]), ptr(skip[a:b], P_i8), row_no0 + a, what, nbytes, nnz), "report_render_len_mtx")
    _render_entries(ctx, sinks, [":".join(p.gene_info_str.split(":")[1:3]) for p in recs], "gene_id", [blocks, blocks],
                    call, times)


def _len_refuse(values, reads):
    return "report_render_len_mtx: the two matrices differ in their entries" if values.nnz != reads.nnz else None


def _ex_pa_len_mat(output_dir: str, res_pkl_file: str, device=None):
    """the gene x cell matrix of the expected pA length as a 10x-style directory <res>.len/: matrix.mtx.gz (real),
    reads.mtx.gz (integer, the reads each value is computed from: the same entries in the same order), features.tsv.gz
    (per record: gene_id:utr_id, gene_id:utr_id, "Gene Expression") and barcodes.tsv.gz (the CB column).  The four are
    renamed from .part once all are complete."""
    return _mtx_run(output_dir, res_pkl_file, ".len", LEN_MTX_FILES, (LEN_MTX_BANNER, MTX_BANNER), device, _batch_cost,
                    _render_len_batch, _len_refuse, "Finish expected pA length for each gene and cell")


# ---------------------------------------------------------------- ex_pa_usage_mat
# The rows and columns are those of ex_pa_cnt_mat --format mtx (the kept rows of every batch, whatever min_reads is), so
# features.tsv.gz and barcodes.tsv.gz are that command's byte for byte.  With c the count of a row in a cell and T the
# cell's reads of label < K in the row's record (ex_pa_len_mat's T): matrix.mtx.gz holds '%.6f' of the double c / T where
# c > 0 and T >= min_reads, reads.mtx.gz holds T wherever T >= min_reads, at the record's sites without a read of the
# cell as well.  An entry there without one in the value matrix is an observed usage of 0; no entry there is a usage
# that is not defined, which a single sparse matrix could not tell apart.  The division and the decimal text are the
# device's (include/scape_hip.h states them), from per-record totals that the device forms once per batch.
USAGE_MAX_MIN_READS = 2 ** 31 - 1


def _usage_batch_cost(n_cols):
    """device bytes of a record: _batch_cost's and its row of column totals (int32)"""
    cost = _batch_cost(n_cols)
    return lambda p: cost(p) + 4 * n_cols


def _render_usage_batch(min_reads, ctx, bat, n_cols, sinks, times):
    """the kept rows of one counted batch into the value and the reads matrix: the records' column totals once on the
    device, then the entries of both (from the same counts and totals), each in blocks cut by its own text size"""
    rowbase, rows, owner, label = _kept_rows(bat)
    if not len(rows):
        return
    t0 = timer()
    check(ctx.lib.scape_hip_report_usage_totals(ctx.h, len(bat.recs), ptr(np.ascontiguousarray(rowbase), P_i64),
                                                ptr(np.ascontiguousarray(bat.K), P_i32)), "report_usage_totals")
    times["render"] += timer() - t0
    row_rec = np.ascontiguousarray(owner.astype(np.int32))
    # each matrix's blocks are cut against an upper bound of its rows' text, "<row number> <column> <field>\n" per entry:
    # the value matrix has at most min(the row's reads, barcodes) entries of an 8-byte field; the reads matrix has one
    # wherever the cell has a read of the RECORD, so at most min(the record's reads, barcodes), of at most the digits of
    # the record's reads.  (One bound for both would cut the value matrix into blocks too small to keep the gzip
    # threads busy: a block is compressed in GZIP_PART pieces, one block at a time.)
    row_no0 = sinks[0].n_rows + 1
    base = len(str(row_no0 + len(rows) - 1)) + len(str(n_cols)) + 3
    rec_tot = np.add.reduceat(bat.row_tot, rowbase)[owner]
    bounds = (np.minimum(bat.row_tot[rows], n_cols) * (base + 8), np.minimum(rec_tot, n_cols) * (base + _digits(rec_tot)))

    def call(slot, a, b, what, nbytes, nnz):
        check(ctx.lib.scape_hip_report_render_usage_mtx(
            ctx.h, slot, b - a, ptr(rows[a:b], P_i64), ptr(row_rec[a:b], P_i32), row_no0 + a, min_reads, what, nbytes,
            nnz), "report_render_usage_mtx")
    _render_entries(ctx, sinks, _pa_infos(bat.recs, owner, label), "pa_info", [_cut_blocks(b) for b in bounds], call,
                    times)


def _usage_refuse(values, reads):
    return "report_render_usage_mtx: the value matrix holds entries that the reads matrix lacks" \
        if values.nnz > reads.nnz else None


def _ex_pa_usage_mat(output_dir: str, res_pkl_file: str, min_reads: int = 1, device=None):
    """the pA site x cell matrix of the per-cell site usage (PSI) as a 10x-style directory <res>.usage/ (<res>.min<N>.usage/
    for min_reads N > 1): matrix.mtx.gz (real, c / T where c > 0 and T >= min_reads), reads.mtx.gz (integer, T wherever
    T >= min_reads), features.tsv.gz and barcodes.tsv.gz (those of ex_pa_cnt_mat --format mtx).  The four are renamed
    from .part once all are complete."""
    if isinstance(min_reads, bool) or not isinstance(min_reads, (int, np.integer)) or \
            not 1 <= min_reads <= USAGE_MAX_MIN_READS:
        raise ValueError(f"min_reads must be an integer from 1 to {USAGE_MAX_MIN_READS}, not {min_reads!r}")
    min_reads = int(min_reads)
    return _mtx_run(output_dir, res_pkl_file, ".usage" if min_reads == 1 else f".min{min_reads}.usage", LEN_MTX_FILES,
                    (LEN_MTX_BANNER, MTX_BANNER), device, _usage_batch_cost,
                    functools.partial(_render_usage_batch, min_reads), _usage_refuse, "Finish pA site usage for each cell")


# ---------------------------------------------------------------- ex_pa_pseudobulk
def _split_sizes(n, k):
    """sizes of the chunks R's ``split(cells, sort(1:n %% k))`` cuts n cells into (DifferentialTest.R:63-104), empty
    chunks dropped.  ``1:n %% k`` holds remainder 0 for n // k cells and remainder v = 1..k-1 for (n - v) // k + 1
    cells when v <= n; ``sort`` puts equal remainders side by side, ascending, and ``split`` cuts where the value
    changes.  The rule is derived from R's documented ``%%``, ``sort`` and ``split``; it has not been run in R."""
    sizes = [n // k] + [(n - v) // k + 1 if v <= n else 0 for v in range(1, k)]
    return [c for c in sizes if c]


def _read_clusters(cell_cluster_file):
    """(ids, cluster names) of the rows of a cluster file: the file as cal_exp_pa_len reads it (index_col="index",
    first other column), the cluster read as text exactly as written; "" = no cluster"""
    import pandas as pd
    others = [c for c in pd.read_csv(cell_cluster_file, nrows=0).columns if c != "index"]
    if not others:
        raise ValueError(f"{cell_cluster_file}: no cluster column beside index")
    df = pd.read_csv(cell_cluster_file, index_col="index", dtype={others[0]: str}, keep_default_na=False)
    ids = df.index.to_numpy()
    if ids.dtype.kind not in "iu":
        raise ValueError(f"{cell_cluster_file}: the index column must hold integer ids")
    return ids.astype(np.int64), df.iloc[:, 0].tolist()


def _column_clusters(col_ids, clu_ids, clu_names):
    """cluster name of every matrix column (None: no group) and the cluster names in order of first appearance among
    the rows of the cluster file.  A repeated id keeps its last row; ids without a column are ignored."""
    last = dict(zip(clu_ids.tolist(), clu_names))
    order = list(dict.fromkeys(c for c in clu_names if c != ""))
    return [last.get(i) or None for i in col_ids.tolist()], order


def _populations(col_clu, order, idents_1, idents_2):
    """[(population name, its columns ascending)], populations without a cell dropped"""
    col_clu = np.array([c if c is not None else "" for c in col_clu], dtype=object)
    if idents_1 is None:
        pops = [(c, np.nonzero(col_clu == c)[0]) for c in order]
    else:
        for ident in (idents_1, idents_2):
            if ident is not None and ident not in order:
                raise ValueError(f"ident {ident!r} names no cluster of the cell_cluster_file")
        rest = (col_clu == idents_2) if idents_2 is not None else ((col_clu != "") & (col_clu != idents_1))
        pops = [("Population1", np.nonzero(col_clu == idents_1)[0]), ("Population2", np.nonzero(rest)[0])]
    return [(name, cols) for name, cols in pops if len(cols)]


def _samples(pops, num_splits, n_cols):
    """pseudo-replicates of the populations: (rows of samples.csv, slot of every column, segment offsets, population of
    every segment).  The slots put sample 0's columns first, then sample 1's, ...; columns of no group come last."""
    table, order, seg_pop = [], [], []
    seg_off = [0]
    for p, (name, cols) in enumerate(pops):
        a = 0
        for i, c in enumerate(_split_sizes(len(cols), num_splits)):
            table.append([f"{name}_{i + 1}", name, i + 1, c])
            order.append(cols[a:a + c])
            seg_off.append(seg_off[-1] + c)
            seg_pop.append(p)
            a += c
    order = np.concatenate(order) if order else np.zeros(0, dtype=np.int64)
    grouped = np.zeros(n_cols, dtype=bool)
    grouped[order] = True
    order = np.concatenate([order, np.nonzero(~grouped)[0]])
    slot = np.empty(n_cols, dtype=np.int32)
    slot[order] = np.arange(n_cols, dtype=np.int32)
    return table, slot, np.array(seg_off, dtype=np.int32), np.array(seg_pop, dtype=np.int64)


def _group_sums_batch(ctx, bat, seg_off, seg_pop, n_cells, cnt_w, pct_w, times):
    """the table lines of one counted batch: segment sums on the device, pa_info and the pct division on the host"""
    _rowbase, rows, owner, label = _kept_rows(bat)
    if not len(rows):
        return 0
    pa = _pa_infos(bat.recs, owner, label)
    n_seg = len(seg_off) - 1
    sums = np.zeros((len(rows), n_seg), dtype=np.int32)
    nz = np.zeros((len(rows), n_seg), dtype=np.int32)
    if n_seg:
        t0 = timer()
        check(ctx.lib.scape_hip_report_group_sums(ctx.h, n_seg, ptr(seg_off, P_i32), len(rows), ptr(rows, P_i64),
                                                  ptr(sums, P_i32), ptr(nz, P_i32)), "report_group_sums")
        times["render"] += timer() - t0
    t0 = timer()
    nz_pop = np.zeros((len(rows), len(n_cells)), dtype=np.int64)
    if n_seg:
        # a population's columns are the union of its samples' columns (consecutive segments)
        first = np.nonzero(np.diff(seg_pop, prepend=-1))[0]
        nz_pop = np.add.reduceat(nz.astype(np.int64), first, axis=1)
    pct = nz_pop / n_cells.astype(np.float64)
    cnt_w.writerows([p] + c for p, c in zip(pa, sums.tolist()))
    pct_w.writerows([p] + [repr(v) for v in c] for p, c in zip(pa, pct.tolist()))
    times["finish"] += timer() - t0
    return len(rows)


def _ex_pa_pseudobulk(output_dir: str, res_pkl_file: str, cell_cluster_file: str, num_splits: int = 6,
                      idents_1=None, idents_2=None, device=None):
    """pA x pseudo-replicate counts and the per-population share of cells with a count above 0, as three csv files
    in output_dir (<prefix>.<kind>[.<A>_vs_<B>].pseudobulk.{cnt,pct,samples}.csv); returns their paths"""
    if num_splits < 1:
        raise ValueError(f"num_splits must be at least 1, not {num_splits}")
    if idents_2 is not None and idents_1 is None:
        raise ValueError("idents_2 needs idents_1")
    if idents_1 is not None and idents_1 == idents_2:
        raise ValueError(f"idents_1 and idents_2 are the same cluster {idents_1!r}")
    inp = _read_inputs(output_dir, res_pkl_file, cell_cluster_file, (idents_1, idents_2))
    n_cols, pops = inp.n_cols, inp.pops
    table, slot, seg_off, seg_pop = _samples(pops, num_splits, n_cols)
    n_cells = np.array([len(cols) for _name, cols in pops], dtype=np.int64)
    idmap = _IdMap(inp.col_ids, slot, "barcode_index.csv")
    stem = _out_stem(output_dir, res_pkl_file, cell_cluster_file, idents_1, idents_2) + ".pseudobulk."
    final = [stem + what + ".csv" for what in ("cnt", "pct", "samples")]
    n_rows = 0
    with _Run(device, final) as run:
        with open(run.parts[0], "w", newline="") as cfh, open(run.parts[1], "w", newline="") as pfh, \
                open(run.parts[2], "w", newline="") as sfh:
            cnt_w, pct_w, smp_w = (csv.writer(fh, delimiter=',', quoting=csv.QUOTE_MINIMAL, lineterminator='\n')
                                   for fh in (cfh, pfh, sfh))
            cnt_w.writerow(["pa_info"] + [row[0] for row in table])
            pct_w.writerow(["pa_info"] + [name for name, _cols in pops])
            smp_w.writerow(["sample", "population", "split", "n_cells"])
            smp_w.writerows(table)
            ctx = run.device()
            for bat in _counted(ctx, inp.res_pkl, idmap, n_cols, _batch_cost(n_cols), _budget(ctx), run.times):
                n_rows += _group_sums_batch(ctx, bat, seg_off, seg_pop, n_cells, cnt_w, pct_w, run.times)
    print(f"Finish pseudo-bulk counts of {n_rows} pA sites in {len(table)} samples of {len(pops)} populations")
    print(f"Finish {inp.res_pkl} in {run.total / 60} min.")
    return final


# ---------------------------------------------------------------- diff_pa
# Tested columns: population 1's matrix columns ascending, then population 2's: positions j = 0 .. n-1.  Permutation p of
# 1 .. n_perm gives population 1 the n1 positions with the smallest key(p, j) (include/scape_hip.h states the hash; it
# is counter-based, so nothing sequential runs anywhere); p = 0 is the observed labelling.  Per record, with t_i / a_i
# the sums of row i over the tested columns / over population 1, T = sum t_i, A = sum a_i, B = T - A and the integer
# N_i = a_i T - t_i A:  S = sum_i N_i^2 / (t_i A B) (Pearson's chi-square of the rows x 2 table) tests the record,
# d_i = N_i / (A B) = a_i / A - b_i / B (two-sided) the site.  Rows with t_i = 0 are dropped; a record is tested when two
# rows or more remain and both populations have reads.  p = (1 + #{p: stat(p) >= stat(0)}) / (1 + n_perm).
# With --strata_file the positions of each population are ordered by stratum (first appearance among the rows of the
# strata file; columns ascending within a stratum), tested cells without a stratum are left out of both populations, and
# permutation p gives population 1, in every stratum s separately, the m1[s] positions of that stratum with the smallest
# key(p, j): same key, same seed, and with one stratum the same labellings.  S, d_i and delta are unchanged (pooled).
DIFF_PA_HEADER = ["gene", "pa_info", "pct.1", "pct.2", "versus", "usage.1", "usage.2", "delta_usage", "n_ge", "p_val",
                  "p_val_adj", "gene_stat", "gene_n_ge", "gene_p_val", "gene_p_val_adj", "n_perm"]
MAX_PERM_CELLS = 1 << 24  # a key keeps the position in its low 24 bits


def _bh(p):
    """Benjamini-Hochberg adjusted p-values (R's p.adjust(method = "BH"))"""
    p = np.asarray(p, dtype=np.float64)
    m = len(p)
    if m == 0:
        return p
    order = np.argsort(-p, kind="stable")
    adj = np.minimum.accumulate(p[order] * (m / np.arange(m, 0, -1)))
    out = np.empty(m)
    out[order] = np.minimum(adj, 1.0)
    return out


def _check_perm_args(n_perm, seed):
    if n_perm < 1:
        raise ValueError(f"n_perm must be at least 1, not {n_perm}")
    if n_perm >= 1 << 31:
        raise ValueError(f"n_perm must be below 2^31, not {n_perm}")
    if not 0 <= seed < 1 << 64:
        raise ValueError(f"seed must lie in 0 .. 2^64 - 1, not {seed}")


def _check_row_sums(call, t, a0, sums, a0_sums):
    """the device's row sums t and a0 against report_group_sums' `sums` and the part of them that a0 restates"""
    if not (np.array_equal(t, sums.sum(axis=1)) and np.array_equal(a0, a0_sums)):
        raise _lib.ScapeHipError(f"{call}: row sums differ from report_group_sums")


def _check_exact(call, rec, what, got, exact, tol, shown=None):
    """the device's f64 `got` lies within tol of the exact Fraction, else ScapeHipError naming call, gene and quantity:
    what = (the quantity's name, then, where it is one of several, whose kind and which)"""
    if not abs(Fraction(float(got)) - exact) <= tol:
        whose = f" of {what[1]} {what[2]!r}" if len(what) > 1 else ""
        raise _lib.ScapeHipError(f"{call}: {rec.gene_info_str}: the device's {what[0]} {got!r}{whose} differs from "
                                 f"{shown or repr(float(exact))}")


def _check_reads(rec, T):
    if int(T) >= 1 << 31:
        raise ValueError(f"{rec.gene_info_str}: 2^31 or more reads in the tested cells")


def _perm_masks(ctx, su, p_first, p_count, times):
    """the labellings of p_count permutations from p_first on, as the run's setup function describes them:
    su.labellings(ctx, p_first, p_count) is its one library call"""
    t0 = timer()
    su.labellings(ctx, p_first, p_count)
    times["render"] += timer() - t0


def _perm_rows(ctx, bat, seg_off, times, each_kept=None, min_pops=2):
    """the tested records of one counted batch and their kept rows: (batch indices of the tested records, row offsets
    per tested record, count rows, cells with a count above 0 per row and population, sums per row and population,
    first count row of every record of the batch), or None when no record of the batch is tested: a record is tested
    when it has two kept rows or more and min_pops populations or more (of the len(seg_off) - 1) with reads; diff_pa_trend,
    whose scored cells are one segment, asks for one.  each_kept(r, labels), when given, is called for every record of
    K >= 2 that has a kept row, tested or not, with the labels of its kept rows"""
    recs, K = bat.recs, bat.K
    rowbase, cand, owner, label = _kept_rows(bat)
    if not len(cand):
        return None
    n_seg = len(seg_off) - 1
    sums = np.zeros((len(cand), n_seg), dtype=np.int32)
    nz = np.zeros((len(cand), n_seg), dtype=np.int32)
    t0 = timer()
    check(ctx.lib.scape_hip_report_group_sums(ctx.h, n_seg, ptr(seg_off, P_i32), len(cand), ptr(cand, P_i64),
                                              ptr(sums, P_i32), ptr(nz, P_i32)), "report_group_sums")
    times["render"] += timer() - t0
    t0 = timer()
    sums = sums.astype(np.int64)
    keep = sums.sum(axis=1) > 0
    n_kept = np.bincount(owner[keep], minlength=len(recs))
    if each_kept is not None:
        cut = np.cumsum(n_kept)
        labs = label[keep]
        for r in np.nonzero((n_kept > 0) & (K >= 2))[0].tolist():
            each_kept(r, labs[cut[r] - n_kept[r]:cut[r]])
    with_reads = sum(np.bincount(owner, weights=sums[:, g], minlength=len(recs)) > 0 for g in range(n_seg))
    tested = (n_kept >= 2) & (with_reads >= min_pops)    # two populations: both have reads
    keep &= tested[owner]
    which = np.nonzero(tested)[0]
    times["finish"] += timer() - t0
    if not len(which):
        return None
    off = np.zeros(len(which) + 1, dtype=np.int64)
    np.cumsum(n_kept[which], out=off[1:])
    return which, off, cand[keep], nz[keep], sums[keep], rowbase


def _perm_chunks(ctx, su, n_perm, chunk, times, test):
    """test() once per chunk of permutations, behind that chunk's masks"""
    for p_first in range(1, n_perm + 1, chunk):
        if chunk < n_perm:       # otherwise the one set of masks was built before the first batch
            _perm_masks(ctx, su, p_first, min(chunk, n_perm + 1 - p_first), times)
        t0 = timer()
        test()
        times["render"] += timer() - t0


def _diff_pa_batch(su, n_perm, lines, genes, ctx, bat, chunk, times):
    """one counted batch: the kept rows of its tested records go through the permutation test; appends the per-line
    integers to `lines` and the per-record ones to `genes`"""
    sel = _perm_rows(ctx, bat, su.seg_off, times)
    if sel is None:
        return
    recs = bat.recs
    which, off, rows, nz, sums, rowbase = sel
    t, a0 = np.zeros(len(rows), np.int64), np.zeros(len(rows), np.int64)
    site_ge, gene_ge = np.zeros(len(rows), np.int64), np.zeros(len(which), np.int64)
    stat0 = np.zeros(len(which), np.float64)
    _perm_chunks(ctx, su, n_perm, chunk, times, lambda: check(
        ctx.lib.scape_hip_report_perm_test(ctx.h, len(which), ptr(off, P_i64), ptr(rows, P_i64), ptr(t, P_i64),
                                           ptr(a0, P_i64), ptr(site_ge, P_i64), ptr(stat0), ptr(gene_ge, P_i64)),
        "report_perm_test"))
    t0 = timer()
    _check_row_sums("report_perm_test", t, a0, sums, sums[:, 0])
    for g, r in enumerate(which.tolist()):
        a, b = int(off[g]), int(off[g + 1])
        _check_reads(recs[r], t[a:b].sum())
        labs = rows[a:b] - int(rowbase[r])
        genes.append((recs[r].gene_info_str, b - a, float(stat0[g]), int(gene_ge[g])))
        lines["pa"].extend(_pa_info(recs[r], labs))
    for key, arr in (("t", t), ("a", a0), ("nz1", nz[:, 0]), ("nz2", nz[:, 1]), ("n_ge", site_ge)):
        lines[key].append(np.asarray(arr, dtype=np.int64).copy())
    times["finish"] += timer() - t0


def _strata(col_ids, pops, strata_file):
    """the two populations restricted to the cells that have a stratum, each ordered by stratum (strata in order of
    first appearance among the rows of the strata file, columns ascending within a stratum), and per stratum with a
    tested cell its number of cells in population 1 and in population 2: (populations, m1, m2, cells left out)"""
    col_stratum, order = _column_clusters(col_ids.astype(np.int64), *_read_clusters(strata_file))
    code = {name: k for k, name in enumerate(order)}
    col_code = np.array([code[c] if c is not None else -1 for c in col_stratum], dtype=np.int64)
    out, counts, left_out = [], [], 0
    for name, cols in pops:
        c = col_code[cols]
        left_out += int((c < 0).sum())
        cols, c = cols[c >= 0], c[c >= 0]
        out.append((name, cols[np.argsort(c, kind="stable")]))
        counts.append(np.bincount(c, minlength=len(order)))
    used = counts[0] + counts[1] > 0
    return out, counts[0][used].astype(np.int32), counts[1][used].astype(np.int32), left_out


def _log10_labellings(m1, m2):
    """log10 of the number of distinct labellings: sum over the strata of log10 C(m1 + m2, m1)"""
    return sum(math.lgamma(a + b + 1) - math.lgamma(a + 1) - math.lgamma(b + 1)
               for a, b in zip(m1.tolist(), m2.tolist())) / math.log(10)


def _two_populations(output_dir, res_pkl_file, cell_cluster_file, idents_1, idents_2, check_options):
    """the head of the setups of two populations (_perm_setup, _boot_diff_setup): the checks of the idents, the
    command's own check_options(), then the prerequisites and the populations of _read_inputs, both with a cell"""
    if idents_1 is None:
        raise ValueError("idents_1 is required")
    if idents_1 == idents_2:
        raise ValueError(f"idents_1 and idents_2 are the same cluster {idents_1!r}")
    check_options()
    inp = _read_inputs(output_dir, res_pkl_file, cell_cluster_file, (idents_1, idents_2))
    pops = inp.pops
    if len(pops) < 2:
        empty = "Population2" if pops and pops[0][0] == "Population1" else "Population1"
        raise ValueError(f"{empty} ({idents_1 if empty == 'Population1' else idents_2 or 'the rest'}) has no cell in "
                         "barcode_index.csv")
    return inp


def _versus(idents_1, idents_2):
    """the `versus` column of the files of two populations"""
    return f"{idents_1}_Vs_{idents_2}" if idents_2 is not None else str(idents_1)


def _perm_setup(output_dir, res_pkl_file, cell_cluster_file, idents_1, idents_2, n_perm, seed, command,
                strata_file=None):
    """what diff_pa and diff_pa_len do before the device is opened: the argument and prerequisite checks, the two
    populations, the id -> column table that puts population 1's columns first and population 2's behind them (with a
    strata file: each ordered by stratum, cells without a stratum left out), and the output path
    <cluster file stem>.<gene|utr>.<A>_vs_<B|rest>[.by_<strata file stem>].<command>.csv"""
    inp = _two_populations(output_dir, res_pkl_file, cell_cluster_file, idents_1, idents_2,
                           lambda: _check_perm_args(n_perm, seed))
    n_cols, pops = inp.n_cols, inp.pops
    strata, left_out, by = None, 0, ""
    if strata_file is not None:
        if not os.path.exists(strata_file):
            raise ValueError(f"Given strata_file {strata_file} does not exist")
        pops, m1, m2, left_out = _strata(inp.col_ids, pops, strata_file)
        for (name, cols), ident in zip(pops, (idents_1, idents_2 or "the rest")):
            if not len(cols):
                raise ValueError(f"{name} ({ident}) has no cell with a stratum in {strata_file}")
        if not np.any((m1 > 0) & (m2 > 0)):
            raise ValueError(f"no stratum of {strata_file} holds cells of both populations: the observed labelling is "
                             "the only one")
        strata = (m1, m2)
        by = ".by_" + os.path.splitext(os.path.basename(strata_file))[0]
        if os.sep in by:
            raise ValueError(f"a strata file name with {os.sep!r} cannot be part of a file name")
    _table, slot, seg_off, _seg_pop = _samples(pops, 1, n_cols)      # population 1's columns first, then population 2's
    n1, n2 = len(pops[0][1]), len(pops[1][1])
    if n1 + n2 >= MAX_PERM_CELLS:
        raise ValueError(f"{n1 + n2} tested cells: {command} takes fewer than {MAX_PERM_CELLS}")
    outpath = _out_stem(output_dir, res_pkl_file, cell_cluster_file, idents_1, idents_2) + f"{by}.{command}.csv"
    if strata is None:
        def labellings(ctx, p_first, p_count):
            check(ctx.lib.scape_hip_report_perm_masks(ctx.h, n1, n2, p_first, p_count, seed), "report_perm_masks")
    else:
        def labellings(ctx, p_first, p_count):
            check(ctx.lib.scape_hip_report_perm_masks_strata(ctx.h, len(m1), ptr(m1, P_i32), ptr(m2, P_i32), p_first,
                                                             p_count, seed), "report_perm_masks_strata")
    # per permutation the device holds the bits, and its key bound per stratum (one stratum without --strata_file)
    perm_bytes = (n1 + n2 + 63) // 64 * 8 + (1 if strata is None else len(m1)) * 8
    return SimpleNamespace(res_pkl=inp.res_pkl, n_cols=n_cols, seg_off=seg_off, n1=n1, n2=n2, outpath=outpath,
                           strata=strata, left_out=left_out, labellings=labellings, perm_bytes=perm_bytes,
                           idmap=_IdMap(inp.col_ids, slot, "barcode_index.csv"),
                           versus=_versus(idents_1, idents_2))


def _print_strata(su):
    if su.strata is not None:
        m1, m2 = su.strata
        print(f"Labels permuted within {len(m1)} strata ({int(((m1 > 0) & (m2 > 0)).sum())} with cells of both "
              f"populations): 10^{_log10_labellings(m1, m2):.1f} distinct labellings; {su.left_out} cells of the two "
              "clusters have no stratum and were left out")


def _perm_run(su, n_perm, device, batch, write, record_bytes=0):
    """the run the permutation commands share: the masks (once, when all permutations, at su.perm_bytes device bytes
    each, fit MAX_PERM_BYTES; otherwise per chunk inside every batch), batch(ctx, counted batch, chunk, times) per
    counted batch, then write(csv writer) into the .part file that is renamed when complete.  record_bytes = device
    bytes a record takes beside its counts and nonzeros (boot_pa_len's replicate values), a number or, where they depend
    on the record (boot_pa_usage's), a function of it.  Returns the wall seconds; LAST_TIMES holds the stages"""
    counts_cost = _batch_cost(su.n_cols, 12)
    extra = record_bytes if callable(record_bytes) else lambda p: record_bytes
    with _Run(device, [su.outpath]) as run:
        times = run.times
        with open(run.parts[0], "w", newline="") as fh:
            ctx = run.device()
            budget = _budget(ctx)
            perm_bytes = int(MAX_PERM_BYTES) if MAX_PERM_BYTES is not None else budget // 2
            chunk = max(1, min(n_perm, perm_bytes // su.perm_bytes))
            if chunk == n_perm:
                _perm_masks(ctx, su, 1, n_perm, times)
            if MAX_BATCH_BYTES is None:
                budget //= 2
            # the counts of a record and, at worst, as many 8-byte nonzeros as it has tested counts
            for bat in _counted(ctx, su.res_pkl, su.idmap, su.n_cols, lambda p: counts_cost(p) + extra(p), budget,
                                times):
                batch(ctx, bat, chunk, times)
            t0 = timer()
            write(csv.writer(fh, delimiter=',', quoting=csv.QUOTE_MINIMAL, lineterminator='\n'))
            times["finish"] += timer() - t0
    return run.total


def _reprs(v):
    return [repr(x) for x in v.tolist()]


def _usage_columns(t, a, n_lines):
    """usage.1, usage.2 and delta_usage of every line as text, from the line's reads t and those of population 1, a,
    records of n_lines lines each, both populations with reads: a / A, (t - a) / B and the integer a T - t A over the
    f64 product A B, one division each; and rec_of = the record of every line, A and B per line"""
    rec_of = np.repeat(np.arange(len(n_lines)), n_lines)
    first = np.concatenate([[0], np.cumsum(n_lines)[:-1]])
    A, T = np.add.reduceat(a, first), np.add.reduceat(t, first)
    Al, Tl = A[rec_of], T[rec_of]
    Bl = Tl - Al
    N = (a * Tl - t * Al).astype(np.float64)
    ab = Al.astype(np.float64) * Bl.astype(np.float64)
    return [_reprs(v) for v in (a / Al, (t - a) / Bl, N / ab)], rec_of, Al, Bl


def _diff_pa_columns(genes, lines, n1, n2, n_perm):
    """what diff_pa's lines hold apart from the adjusted p-values, from the per-line integers `lines` and `genes` =
    (gene_info_str, lines, S(0), gene_n_ge) per tested record of populations with n1 and n2 cells: the text columns
    gene, pa, pct1, pct2, usage (usage.1, usage.2, delta_usage), n_ge, stat0 and gene_ge per line, the p-values p_val
    per line and gene_p per record as arrays, and rec_of = the record of every line"""
    t, a, nz1, nz2, n_ge = (np.concatenate(lines[k]) for k in ("t", "a", "nz1", "nz2", "n_ge"))
    usage, rec_of, _Al, _Bl = _usage_columns(t, a, np.array([g[1] for g in genes], dtype=np.int64))
    gene_ge = np.array([g[3] for g in genes], dtype=np.int64)
    stat0 = np.array([g[2] for g in genes])
    return SimpleNamespace(gene=[genes[g][0] for g in rec_of.tolist()], pa=lines["pa"], pct1=_reprs(nz1 / n1),
                           pct2=_reprs(nz2 / n2), usage=usage,
                           n_ge=n_ge.tolist(), p_val=(1 + n_ge) / (1 + n_perm), stat0=_reprs(stat0[rec_of]),
                           gene_ge=gene_ge[rec_of].tolist(), gene_p=(1 + gene_ge) / (1 + n_perm), rec_of=rec_of)


def _diff_pa(output_dir: str, res_pkl_file: str, cell_cluster_file: str, idents_1: str, idents_2=None,
             n_perm: int = 9999, seed: int = 1, device=None, strata_file=None):
    """permutation test of pA usage between the cells of cluster idents_1 and those of idents_2 (None: every other cell
    that has a cluster); writes <cluster file stem>.<gene|utr>.<A>_vs_<B|rest>.diff_pa.csv in output_dir, returns its path.
    strata_file (a file like the cluster file): the labels are permuted within its strata only, cells without a stratum
    are left out, and the file name carries .by_<strata file stem> before .diff_pa.csv"""
    su = _perm_setup(output_dir, res_pkl_file, cell_cluster_file, idents_1, idents_2, n_perm, seed, "diff_pa",
                     strata_file)
    n1, n2, versus = su.n1, su.n2, su.versus
    lines = {k: [] for k in ("pa", "t", "a", "nz1", "nz2", "n_ge")}
    genes = []                   # (gene_info_str, lines, S(0), gene_n_ge) per tested record

    batch = functools.partial(_diff_pa_batch, su, n_perm, lines, genes)

    def write(w):
        w.writerow(DIFF_PA_HEADER)
        if not genes:
            return
        c = _diff_pa_columns(genes, lines, n1, n2, n_perm)
        gene_adj = _bh(c.gene_p)
        w.writerows(zip(c.gene, c.pa, c.pct1, c.pct2, [versus] * len(c.pa), *c.usage, c.n_ge, _reprs(c.p_val),
                        _reprs(_bh(c.p_val)), c.stat0, c.gene_ge, _reprs(c.gene_p[c.rec_of]), _reprs(gene_adj[c.rec_of]),
                        [n_perm] * len(c.pa)))

    wall = _perm_run(su, n_perm, device, batch, write)
    print(f"Finish {n_perm} permutations of {n1} + {n2} cells for {sum(g[1] for g in genes)} pA sites of "
          f"{len(genes)} tested records")
    _print_strata(su)
    print(f"Finish {su.res_pkl} in {wall / 60} min.")
    return su.outpath


# ---------------------------------------------------------------- diff_pa_len
# Does one population use longer 3'UTRs than the other?  Populations, tested columns, kept rows and permutations are
# diff_pa's (same --seed = same labellings).  Kept row i of a record has the position x_i = alpha_arr[label_i] (f64,
# nucleotides from the UTR's 5' end along the transcript on either strand; _pa_info turns the same number into the
# genomic loc), so larger = more distal = longer 3'UTR.  With a_i / b_i = t_i - a_i a row's sums over population 1 / 2
# under a labelling, A = sum a_i, B = sum b_i:
#     mean_pos.1 = sum a_i x_i / A,   mean_pos.2 = sum b_i x_i / B,   delta = mean_pos.1 - mean_pos.2
# (delta = 0 when A = 0 or B = 0; delta > 0: population 1's reads end further out).  Two-sided on |delta|:
# n_ge = #{p in 1..n_perm: |delta(p)| >= |delta(0)| - tol}, tol = 2^-40 span, span = max x_i - min x_i over the kept rows;
# p_val = (1 + n_ge) / (1 + n_perm), Benjamini-Hochberg over the file's lines.  The reference's own scale (exp_pa_len's
# 1 + 9 (a - a[0]) / (a[-1] - a[0])) is an affine map of x, so a two-sided test on it is the same test: the file carries
# both scales and one p-value.  A record is tested when diff_pa would test it (two kept rows or more, reads in both
# populations) and span > 0; a non-finite position of a kept row of any record with K >= 2 is a ValueError.  The device gets
# w_i = x_i - min x and tol per record (include/scape_hip.h states its arithmetic and the bound that makes n_ge exact).
DIFF_PA_LEN_HEADER = ["gene", "versus", "num_pa", "reads.1", "reads.2", "mean_pos.1", "mean_pos.2", "delta_pos",
                      "exp_length.1", "exp_length.2", "delta_exp_length", "n_ge", "p_val", "p_val_adj", "n_perm"]


def _mean_positions(x, a, b):
    """(mean_pos.1, mean_pos.2, delta_pos) of positions x (finite f64) under the integer row sums a and b: the exact
    rationals, each rounded once (both populations have reads)"""
    _mean, (m1, m2), (delta, _delta2) = _mean_positions_groups(x, list(zip(a, b)))
    return m1, m2, delta


def _finite_positions(recs, pos):
    """the each_kept callback of _perm_rows for the tests of the pA position: pos[r] = the positions of record r's kept
    rows (f64); a non-finite one is a ValueError naming the record"""
    def positions(r, labs):
        x = np.asarray(recs[r].alpha_arr, dtype=np.float64)[labs]
        if not (np.all(np.isfinite(x)) and np.isfinite(x.max() - x.min())):
            raise ValueError(f"{recs[r].gene_info_str}: alpha_arr holds a non-finite position of a pA site with reads")
        pos[r] = x
    return positions


def _with_span(sel, pos, times):
    """the records of _perm_rows' result whose kept rows lie at two positions or more (span = max x - min x > 0): (batch
    indices, row offsets, count rows, sums per row and population, first count row of every record of the batch,
    positions of the kept rows per record), or None when none is left"""
    which, off, rows, _nz, sums, rowbase = sel
    t0 = timer()
    tested = [g for g, r in enumerate(which.tolist()) if float(pos[r].max() - pos[r].min()) > 0]
    times["finish"] += timer() - t0
    if not tested:
        return None
    n_kept = np.diff(off)[tested]
    pick = np.concatenate([np.arange(off[g], off[g + 1]) for g in tested])
    which = which[tested]
    off = np.zeros(len(which) + 1, dtype=np.int64)
    np.cumsum(n_kept, out=off[1:])
    return which, off, np.ascontiguousarray(rows[pick]), sums[pick], rowbase, [pos[r] for r in which.tolist()]


def _exp_lengths(ctx, seg_off, bat, which, rowbase, times):
    """the reference's exp_pa_len of every population (_exp_len_rows, one value per segment of seg_off) for the records
    `which` of a counted batch, from the populations' counts of ALL K labels of those records"""
    recs, K = bat.recs, bat.K
    G = len(seg_off) - 1
    all_rows = np.concatenate([int(rowbase[r]) + np.arange(int(K[r]), dtype=np.int64) for r in which.tolist()])
    full = np.zeros((len(all_rows), G), dtype=np.int32)
    full_nz = np.zeros((len(all_rows), G), dtype=np.int32)
    t0 = timer()
    check(ctx.lib.scape_hip_report_group_sums(ctx.h, G, ptr(seg_off, P_i32), len(all_rows), ptr(all_rows, P_i64),
                                              ptr(full, P_i32), ptr(full_nz, P_i32)), "report_group_sums")
    times["render"] += timer() - t0
    t0 = timer()
    out, k0 = [], 0
    for r in which.tolist():
        k = int(K[r])
        counts = np.zeros((G, k + 1), dtype=np.int64)    # slot k: reads of no site, which never weigh
        counts[:, :k] = full[k0:k0 + k].T
        k0 += k
        out.append(_exp_len_rows(k, recs[r].alpha_arr, counts))
    times["finish"] += timer() - t0
    return out


def _diff_pa_len_batch(su, n_perm, out, ctx, bat, chunk, times):
    """one counted batch: appends (gene, num_pa, A, B, mean_pos.1, mean_pos.2, delta_pos, exp_length.1, exp_length.2,
    n_ge) per tested record to `out`"""
    recs = bat.recs
    pos = {}                     # record -> positions of its kept rows (f64, finite)
    sel = _perm_rows(ctx, bat, su.seg_off, times, _finite_positions(recs, pos))
    sel = sel and _with_span(sel, pos, times)
    if sel is None:
        return
    which, off, rows, sums, rowbase, xs = sel
    w = np.ascontiguousarray(np.concatenate([x - x.min() for x in xs]))
    tol = np.array([np.ldexp(float(x.max() - x.min()), -40) for x in xs], dtype=np.float64)
    t, a0 = np.zeros(len(rows), np.int64), np.zeros(len(rows), np.int64)
    delta0, n_ge = np.zeros(len(which), np.float64), np.zeros(len(which), np.int64)
    _perm_chunks(ctx, su, n_perm, chunk, times, lambda: check(
        ctx.lib.scape_hip_report_perm_len(ctx.h, len(which), ptr(off, P_i64), ptr(rows, P_i64), ptr(w), ptr(tol),
                                          ptr(t, P_i64), ptr(a0, P_i64), ptr(delta0), ptr(n_ge, P_i64)),
        "report_perm_len"))
    _check_row_sums("report_perm_len", t, a0, sums, sums[:, 0])
    exp_len = _exp_lengths(ctx, su.seg_off, bat, which, rowbase, times)
    t0 = timer()
    for g, r in enumerate(which.tolist()):
        sl = slice(int(off[g]), int(off[g + 1]))
        a, b = a0[sl], t[sl] - a0[sl]
        m1, m2, d = _mean_positions(xs[g], a.tolist(), b.tolist())
        if not abs(float(delta0[g]) - d) <= tol[g]:
            raise _lib.ScapeHipError(f"report_perm_len: {recs[r].gene_info_str}: the device's delta {delta0[g]!r} "
                                     f"differs from {d!r}")
        e = exp_len[g]
        out.append((recs[r].gene_info_str, int(off[g + 1] - off[g]), int(a.sum()), int(b.sum()), m1, m2, d,
                    float(e[0]), float(e[1]), int(n_ge[g])))
    times["finish"] += timer() - t0


def _diff_pa_len(output_dir: str, res_pkl_file: str, cell_cluster_file: str, idents_1: str, idents_2=None,
                 n_perm: int = 9999, seed: int = 1, device=None, strata_file=None):
    """permutation test of the mean pA position (3'UTR length) between the cells of cluster idents_1 and those of
    idents_2 (None: every other cell that has a cluster); writes <cluster file stem>.<gene|utr>.<A>_vs_<B|rest>
    .diff_pa_len.csv in output_dir, one line per tested record, and returns its path.  strata_file: as for _diff_pa"""
    su = _perm_setup(output_dir, res_pkl_file, cell_cluster_file, idents_1, idents_2, n_perm, seed, "diff_pa_len",
                     strata_file)
    out = []

    batch = functools.partial(_diff_pa_len_batch, su, n_perm, out)

    def write(w):
        w.writerow(DIFF_PA_LEN_HEADER)
        if not out:
            return
        n_ge = np.array([o[9] for o in out], dtype=np.int64)
        p_val = (1 + n_ge) / (1 + n_perm)
        with np.errstate(invalid="ignore"):
            d_exp = np.array([o[7] for o in out]) - np.array([o[8] for o in out])
        w.writerows([o[0], su.versus, o[1], o[2], o[3]] + [repr(v) for v in o[4:9]] + [repr(de), o[9], repr(p), repr(q),
                                                                                         n_perm]
                    for o, de, p, q in zip(out, d_exp.tolist(), p_val.tolist(), _bh(p_val).tolist()))

    wall = _perm_run(su, n_perm, device, batch, write)
    print(f"Finish {n_perm} permutations of {su.n1} + {su.n2} cells for {len(out)} tested records")
    _print_strata(su)
    print(f"Finish {su.res_pkl} in {wall / 60} min.")
    return su.outpath


# ---------------------------------------------------------------- diff_pa_groups
# The omnibus form of diff_pa: which records use their pA sites differently across G = 2..64 populations at all.  One
# population per cluster of the cluster file (order of first appearance, clusters without a column dropped, as
# ex_pa_pseudobulk), or the clusters named by --idents, in the order given.  Tested columns: population 0's matrix
# columns ascending, then population 1's, ...: positions j = 0 .. n-1.  Permutation p of 1 .. n_perm ranks the keys
# key(p, j) of diff_pa (same hash, same seed) and gives the n_0 smallest to group 0, the next n_1 to group 1, ...; p = 0
# is the observed labelling.  Per record, with a_ig the sum of kept row i over group g, A_g = sum_i a_ig, t_i = sum_g
# a_ig, T = sum t_i and the integer N_ig = a_ig T - t_i A_g:
#     s_i = sum_{g: A_g > 0} N_ig^2 / A_g  tests the site,   S = sum_i s_i / (T t_i)  the record
# (S is Pearson's chi-square of the rows x G table and, for G = 2, diff_pa's S as a rational).  A record is tested when
# it has two kept rows or more and two populations or more with reads.  p = (1 + #{p: stat(p) >= stat(0)}) / (1 + n_perm),
# Benjamini-Hochberg over the file's lines (sites) and over the tested records (genes).  Not part of this command:
# --strata_file (blocked G-way relabelling needs cut points per stratum and group).  The omnibus form of diff_pa_len is
# diff_pa_len_groups, below.
DIFF_PA_GROUPS_HEADER = ["gene", "pa_info", "num_groups", "top_group", "top_delta_usage", "site_stat", "n_ge", "p_val",
                         "p_val_adj", "gene_stat", "gene_n_ge", "gene_p_val", "gene_p_val_adj", "n_perm"]
MAX_GROUPS = 64                  # a group is one byte on the device, and its sums 2 KiB of LDS
MAX_ROWS_AND_GROUPS = 4000       # kept rows + populations of a record: the rounding bound of S (include/scape_hip.h)


def _ident_populations(output_dir, res_pkl_file, cell_cluster_file, idents):
    """what --idents asks of a cluster file, for _groups_setup and _boot_setup: (the idents as text, the file name's tag
    .<A>+<B>+... or "", _read_inputs' result, the populations: the named clusters in the order given, or every cluster
    that has a column in order of first appearance); a repeated, unknown or cell-less ident is a ValueError"""
    idents = [str(i) for i in idents or ()]
    for k, ident in enumerate(idents):
        if ident in idents[:k]:
            raise ValueError(f"ident {ident!r} is given twice")
    tag = "." + "+".join(idents) if idents else ""
    if os.sep in tag:
        raise ValueError(f"an ident with {os.sep!r} cannot be part of a file name")
    inp = _read_inputs(output_dir, res_pkl_file, cell_cluster_file)
    pops = inp.pops
    if idents:
        with_cells = dict(pops)
        for ident in idents:
            if ident not in inp.clusters:
                raise ValueError(f"ident {ident!r} names no cluster of the cell_cluster_file")
            if ident not in with_cells:
                raise ValueError(f"cluster {ident!r} has no cell in barcode_index.csv")
        pops = [(ident, with_cells[ident]) for ident in idents]
    return idents, tag, inp, pops


def _groups_setup(output_dir, res_pkl_file, cell_cluster_file, idents, n_perm, seed, command="diff_pa_groups",
                  pairs=False, markers=False):
    """what diff_pa_groups, diff_pa_len_groups, diff_pa_pairs (pairs=True: su.pairs = the two groups of every pair,
    all (g, h) with g < h in lexicographic order, and the labellings are every pair's membership bits, not the group
    bytes) and diff_pa_markers (markers=True: 1 to 64 populations, each against every other cell that has a cluster;
    those of no population follow the populations as one more column segment, su.seg_off has that segment even when it
    is empty, su.n counts all tested cells, and the labellings are every marker's membership bits) do before the device
    is opened: the argument and prerequisite checks, the populations, the id -> column table that puts population 0's
    columns first, then population 1's, ..., and the output path
    <cluster file stem>.<gene|utr>[.<A>+<B>+...].<command>.csv"""
    _check_perm_args(n_perm, seed)
    idents, tag, inp, pops = _ident_populations(output_dir, res_pkl_file, cell_cluster_file, idents)
    if markers and not idents and len(pops) > MAX_GROUPS:
        raise ValueError(f"{len(pops)} clusters: {command} takes at most {MAX_GROUPS} at once, name them with --idents")
    if not (1 if markers else 2) <= len(pops) <= MAX_GROUPS:
        raise ValueError(f"{len(pops)} populations: {command} takes {1 if markers else 2} to {MAX_GROUPS}")
    sizes = np.array([len(cols) for _name, cols in pops], dtype=np.int32)
    n = int(sizes.sum())
    segments = pops
    if markers:
        tested = np.sort(np.concatenate([cols for _name, cols in inp.pops]))
        others = np.setdiff1d(tested, np.concatenate([cols for _name, cols in pops]))
        n = len(tested)
        for name, cols in pops:
            if len(cols) == n:
                raise ValueError(f"cluster {name!r} holds every cell that has a cluster: the rest has no cell in "
                                 "barcode_index.csv")
        segments = pops + [("", others)]
    _table, slot, seg_off, _seg_pop = _samples(segments, 1, inp.n_cols)
    if n >= MAX_PERM_CELLS:
        raise ValueError(f"{n} tested cells: {command} takes fewer than {MAX_PERM_CELLS}")
    outpath = _out_stem(output_dir, res_pkl_file, cell_cluster_file, None, None) + tag + f".{command}.csv"
    su = SimpleNamespace(res_pkl=inp.res_pkl, n_cols=inp.n_cols, seg_off=seg_off, sizes=sizes,
                         names=[name for name, _cols in pops], outpath=outpath,
                         idmap=_IdMap(inp.col_ids, slot, "barcode_index.csv"))
    if markers:
        if not len(others):
            su.seg_off = np.append(seg_off, seg_off[-1])     # _samples drops an empty segment
        su.n = n
        # the rank of every slot's column among the tested columns ascending: diff_pa's order of a marker's rest
        orig_rank = np.searchsorted(tested, np.concatenate([cols for _name, cols in segments])).astype(np.int32)
        # per permutation and marker the device holds the marker's bits over all tested cells and its key bound
        su.perm_bytes = len(sizes) * ((n + 63) // 64 * 8 + 8)

        def labellings(ctx, p_first, p_count):
            check(ctx.lib.scape_hip_report_perm_marker_masks(ctx.h, len(sizes), ptr(sizes, P_i32), len(others),
                                                             ptr(orig_rank, P_i32), p_first, p_count, seed),
                  "report_perm_marker_masks")
    elif pairs:
        G = len(sizes)
        pair_g = np.array([g for g in range(G) for _h in range(g + 1, G)], dtype=np.int32)
        pair_h = np.array([h for g in range(G) for h in range(g + 1, G)], dtype=np.int32)
        su.pairs = (pair_g, pair_h)
        # per permutation and pair the device holds the pair's bits and its key bound
        su.perm_bytes = int(sum((int(sizes[g]) + int(sizes[h]) + 63) // 64 * 8 + 8 for g, h in zip(pair_g, pair_h)))

        def labellings(ctx, p_first, p_count):
            check(ctx.lib.scape_hip_report_perm_pair_masks(ctx.h, G, ptr(sizes, P_i32), len(pair_g), ptr(pair_g, P_i32),
                                                           ptr(pair_h, P_i32), p_first, p_count, seed),
                  "report_perm_pair_masks")
    else:
        su.perm_bytes = int(sizes.sum())                 # one byte per tested cell and permutation

        def labellings(ctx, p_first, p_count):
            check(ctx.lib.scape_hip_report_perm_labels(ctx.h, len(sizes), ptr(sizes, P_i32), p_first, p_count, seed),
                  "report_perm_labels")
    su.labellings = labellings
    return su


def _diff_pa_groups_batch(su, n_perm, lines, genes, ctx, bat, chunk, times):
    """one counted batch: the kept rows of its tested records go through the G-way permutation test; appends the
    per-line arrays to `lines` and (gene_info_str, lines, S(0), gene_n_ge) per tested record to `genes`"""
    sel = _perm_rows(ctx, bat, su.seg_off, times)
    if sel is None:
        return
    recs, G = bat.recs, len(su.sizes)
    which, off, rows, nz, sums, rowbase = sel
    for g, r in enumerate(which.tolist()):
        if int(off[g + 1] - off[g]) + G > MAX_ROWS_AND_GROUPS:
            raise ValueError(f"{recs[r].gene_info_str}: {int(off[g + 1] - off[g])} pA sites with reads and {G} "
                             f"populations, together more than {MAX_ROWS_AND_GROUPS}: beyond the rounding bound of "
                             "the statistic")
    t, a0 = np.zeros(len(rows), np.int64), np.zeros((len(rows), G), np.int64)
    site_ge, gene_ge = np.zeros(len(rows), np.int64), np.zeros(len(which), np.int64)
    stat0, site_stat0 = np.zeros(len(which), np.float64), np.zeros(len(rows), np.float64)
    _perm_chunks(ctx, su, n_perm, chunk, times, lambda: check(
        ctx.lib.scape_hip_report_perm_groups(ctx.h, len(which), ptr(off, P_i64), ptr(rows, P_i64), G,
                                             ptr(su.seg_off, P_i32), ptr(t, P_i64), ptr(a0, P_i64),
                                             ptr(site_ge, P_i64), ptr(stat0), ptr(site_stat0), ptr(gene_ge, P_i64)),
        "report_perm_groups"))
    t0 = timer()
    _check_row_sums("report_perm_groups", t, a0, sums, sums)
    for g, r in enumerate(which.tolist()):
        a, b = int(off[g]), int(off[g + 1])
        _check_reads(recs[r], t[a:b].sum())
        genes.append((recs[r].gene_info_str, b - a, float(stat0[g]), int(gene_ge[g])))
        lines["pa"].extend(_pa_info(recs[r], rows[a:b] - int(rowbase[r])))
    for key, arr in (("a", a0), ("nz", nz), ("n_ge", site_ge), ("site_stat", site_stat0)):
        lines[key].append(np.array(arr))
    times["finish"] += timer() - t0


def _diff_pa_groups(output_dir: str, res_pkl_file: str, cell_cluster_file: str, idents=(), n_perm: int = 9999,
                    seed: int = 1, device=None):
    """permutation test of pA usage across the populations of a cluster file (every cluster, or the clusters `idents` in
    the order given); writes <cluster file stem>.<gene|utr>[.<A>+<B>+...].diff_pa_groups.csv in output_dir, one line per
    kept row of a tested record, and returns its path"""
    su = _groups_setup(output_dir, res_pkl_file, cell_cluster_file, idents, n_perm, seed)
    names, G = su.names, len(su.sizes)
    lines = {k: [] for k in ("pa", "a", "nz", "n_ge", "site_stat")}
    genes = []                   # (gene_info_str, lines, S(0), gene_n_ge) per tested record

    batch = functools.partial(_diff_pa_groups_batch, su, n_perm, lines, genes)

    def write(w):
        w.writerow(DIFF_PA_GROUPS_HEADER + [f"usage.{n}" for n in names] + [f"pct.{n}" for n in names])
        if not genes:
            return
        a, nz, n_ge, site_stat = (np.concatenate(lines[k]) for k in ("a", "nz", "n_ge", "site_stat"))
        n_lines = np.array([g[1] for g in genes], dtype=np.int64)
        rec_of = np.repeat(np.arange(len(genes)), n_lines)
        first = np.concatenate([[0], np.cumsum(n_lines)[:-1]])
        A = np.add.reduceat(a, first, axis=0)            # [record][group]
        p_val = (1 + n_ge) / (1 + n_perm)
        gene_ge = np.array([g[3] for g in genes], dtype=np.int64)
        gene_p = (1 + gene_ge) / (1 + n_perm)
        gene_adj = _bh(gene_p)
        with np.errstate(divide="ignore", invalid="ignore"):
            usage = a / A[rec_of]                        # nan where the population has no read in the record
        pct = nz / su.sizes.astype(np.float64)
        # the population with the largest N_ig^2 / A_g, compared exactly (Python ints, cross-multiplied); the first wins ties
        top, top_delta = [], []
        for ai, Ar in zip(a.tolist(), A[rec_of].tolist()):
            ti, T = sum(ai), sum(Ar)
            best = None
            for g in range(G):
                if Ar[g] > 0:
                    N = ai[g] * T - ti * Ar[g]
                    if best is None or N * N * best[2] > best[1] * best[1] * Ar[g]:
                        best = (g, N, Ar[g])
            top.append(names[best[0]])
            top_delta.append(repr(best[1] / (best[2] * T)))
        cols = [[genes[g][0] for g in rec_of.tolist()], lines["pa"], (A > 0).sum(axis=1)[rec_of].tolist(), top,
                top_delta, [repr(x) for x in site_stat.tolist()], n_ge.tolist()]
        stat0 = np.array([g[2] for g in genes])
        for v in (p_val, _bh(p_val), stat0[rec_of]):
            cols.append([repr(x) for x in v.tolist()])
        cols.append(gene_ge[rec_of].tolist())
        for v in (gene_p[rec_of], gene_adj[rec_of]):
            cols.append([repr(x) for x in v.tolist()])
        cols.append([n_perm] * len(n_ge))
        for v in (usage, pct):
            cols.extend([repr(x) for x in v[:, g].tolist()] for g in range(G))
        w.writerows(zip(*cols))

    wall = _perm_run(su, n_perm, device, batch, write)
    print(f"Finish {n_perm} permutations of {int(su.sizes.sum())} cells in {G} populations for "
          f"{sum(g[1] for g in genes)} pA sites of {len(genes)} tested records")
    print(f"Finish {su.res_pkl} in {wall / 60} min.")
    return su.outpath


# ---------------------------------------------------------------- diff_pa_pairs
# What lies behind a significant diff_pa_groups: every pair of the populations tested as diff_pa tests two, in one run.
# Options, populations, checks, column layout and file naming are diff_pa_groups's.  The pairs are all (g, h), g < h in
# population order, in lexicographic order; that is also the order of the file's blocks.  Pair (A, B) is exactly
# `diff_pa --idents_1 A --idents_2 B` with the same --seed and --n_perm: local positions 0 .. n_A - 1 for A's columns
# ascending, then n_A .. n_A + n_B - 1 for B's, permutation p gives A the n_A local positions with the smallest
# key(p, local position), the kept rows are the record's label rows with a read in a cell of A or B, the pair tests a
# record when two such rows or more remain and both A and B have reads, and S and d_i go through the device function of
# diff_pa with its slack: t, a, n_ge, gene_n_ge and the bits of gene_stat are diff_pa's.  One line per (pair, kept row
# of a record that the pair tests).  p_val_adj is Benjamini-Hochberg over ALL lines of the file, gene_p_val_adj over all
# tested (pair, record) combinations of the file: the correction across the G (G - 1) / 2 runs.  The counts are read and
# counted once; the device holds, per permutation, the sum over the pairs of (mask words x 8 + one 8-byte key bound).
DIFF_PA_PAIRS_HEADER = DIFF_PA_HEADER[:2] + ["group_1", "group_2"] + DIFF_PA_HEADER[2:]
MAX_PAIR_RESULT_BYTES = 256 << 20     # host and device bytes of the counters of one call: more pairs are taken in ranges


def _write_diff_pa_blocks(w, header, blocks, n_perm):
    """the file of diff_pa_pairs and diff_pa_markers: one block of diff_pa lines per entry of blocks = (the group fields
    behind pa_info, versus, the block's _diff_pa_columns), p_val_adj Benjamini-Hochberg over all lines of the file and
    gene_p_val_adj over all tested (block, record) combinations"""
    w.writerow(header)
    if not blocks:
        return
    p_adj = _bh(np.concatenate([c.p_val for _groups, _versus, c in blocks]))
    gene_adj = _bh(np.concatenate([c.gene_p for _groups, _versus, c in blocks]))
    line0 = gene0 = 0
    for groups, versus, c in blocks:
        n = len(c.pa)
        adj = gene_adj[gene0:gene0 + len(c.gene_p)]
        w.writerows(zip(c.gene, c.pa, *([g] * n for g in groups), c.pct1, c.pct2, [versus] * n, *c.usage, c.n_ge,
                        _reprs(c.p_val), _reprs(p_adj[line0:line0 + n]), c.stat0, c.gene_ge,
                        _reprs(c.gene_p[c.rec_of]), _reprs(adj[c.rec_of]), [n_perm] * n))
        line0 += n
        gene0 += len(c.gene_p)


def _pair_items(su, sums, nz):
    """per pair (g, h), in the file's order: g, every row's reads in the two populations (a row that has none is not the
    pair's, and a record of fewer than two such rows not tested) and its cells with a read in h"""
    return [(g, sums[:, g] + sums[:, h], nz[:, h]) for g, h in zip(su.pairs[0].tolist(), su.pairs[1].tolist())]


def _marker_items(su, sums, nz):
    """per marker g: g, every row's reads in the tested cells and its cells with a read in the marker's rest"""
    t, nz_all = sums.sum(axis=1), nz.astype(np.int64).sum(axis=1)
    return [(g, t, nz_all - nz[:, g]) for g in range(len(su.sizes))]


# what diff_pa_pairs and diff_pa_markers test in blocks, by the blocks' noun: the entry point, the cap on one call's
# counters (read at the call) and the items
_BLOCK_TESTS = {"pair": ("scape_hip_report_perm_pairs", lambda: MAX_PAIR_RESULT_BYTES, _pair_items),
                "marker": ("scape_hip_report_perm_markers", lambda: MAX_MARKER_RESULT_BYTES, _marker_items)}


def _diff_pa_blocks_batch(su, n_perm, noun, blocks, ctx, bat, chunk, times):
    """one counted batch: the rows kept over all segments of the records that two segments or more have reads in go
    through the test of every item (pair, marker), the items in ranges of at most the cap's bytes of counters; appends to
    blocks[k] = (lines, genes) of item k what _diff_pa_batch appends for the item's two populations.  An item tests a
    record when two of its rows or more have reads in the item's cells, and both of its populations have reads"""
    sel = _perm_rows(ctx, bat, su.seg_off, times)
    if sel is None:
        return
    entry, cap, items = _BLOCK_TESTS[noun]
    call = entry[len("scape_hip_"):]
    recs, n_seg, n_items = bat.recs, len(su.seg_off) - 1, len(blocks)
    which, off, rows, nz, sums, rowbase = sel
    n_rows, n_rec = len(rows), len(which)
    t, a0 = np.zeros(n_rows, np.int64), np.zeros((n_rows, n_seg), np.int64)
    site_ge, gene_ge = np.zeros((n_items, n_rows), np.int64), np.zeros((n_items, n_rec), np.int64)
    stat0 = np.zeros((n_items, n_rec), np.float64)
    step = int(max(1, min(n_items, cap() // (12 * n_rows + 20 * n_rec))))

    def test():
        for k in range(0, n_items, step):
            m = min(step, n_items - k)
            check(getattr(ctx.lib, entry)(ctx.h, n_rec, ptr(off, P_i64), ptr(rows, P_i64), n_seg, ptr(su.seg_off, P_i32),
                                          k, m, ptr(t, P_i64), ptr(a0, P_i64), ptr(site_ge[k:k + m], P_i64),
                                          ptr(stat0[k:k + m]), ptr(gene_ge[k:k + m], P_i64)), call)
    _perm_chunks(ctx, su, n_perm, chunk, times, test)
    t0 = timer()
    _check_row_sums(call, t, a0, sums, sums)
    rec_of = np.repeat(np.arange(n_rec), np.diff(off))
    pa = np.array(_pa_infos(recs, which[rec_of], rows - rowbase[which[rec_of]]), dtype=object)
    for k, ((g, tk, nz2), (lines, genes)) in enumerate(zip(items(su, sums, nz), blocks)):
        A, T = np.add.reduceat(sums[:, g], off[:-1]), np.add.reduceat(tk, off[:-1])
        tested = (np.bincount(rec_of[tk > 0], minlength=n_rec) >= 2) & (A > 0) & (A < T)
        keep = (tk > 0) & tested[rec_of]
        if not keep.any():
            continue
        n_lines = np.bincount(rec_of[keep], minlength=n_rec)
        for r in np.nonzero(tested)[0].tolist():
            genes.append((recs[which[r]].gene_info_str, int(n_lines[r]), float(stat0[k, r]), int(gene_ge[k, r])))
        lines["pa"].extend(pa[keep].tolist())
        for key, arr in (("t", tk), ("a", sums[:, g]), ("nz1", nz[:, g]), ("nz2", nz2), ("n_ge", site_ge[k])):
            lines[key].append(np.asarray(arr[keep], dtype=np.int64))
    times["finish"] += timer() - t0


def _diff_pa_blocks(su, n_perm, device, noun, header, block_ids, tested_among):
    """the run of diff_pa_pairs and diff_pa_markers: one block of the file per entry of block_ids = (the group fields,
    versus, cells of population 1, cells of population 2); returns the file's path"""
    blocks = [({k: [] for k in ("pa", "t", "a", "nz1", "nz2", "n_ge")}, []) for _ in block_ids]

    def write(w):
        _write_diff_pa_blocks(w, header, [
            (groups, versus, _diff_pa_columns(genes, lines, n1, n2, n_perm))
            for (groups, versus, n1, n2), (lines, genes) in zip(block_ids, blocks) if genes], n_perm)

    wall = _perm_run(su, n_perm, device, functools.partial(_diff_pa_blocks_batch, su, n_perm, noun, blocks), write)
    print(f"Finish {n_perm} permutations of {len(blocks)} {noun}s {tested_among} for "
          f"{sum(g[1] for _l, genes in blocks for g in genes)} lines of {sum(len(genes) for _l, genes in blocks)} tested "
          f"({noun}, record) combinations")
    print(f"Finish {su.res_pkl} in {wall / 60} min.")
    return su.outpath


def _diff_pa_pairs(output_dir: str, res_pkl_file: str, cell_cluster_file: str, idents=(), n_perm: int = 9999,
                   seed: int = 1, device=None):
    """diff_pa for every pair of the populations of a cluster file (every cluster, or the clusters `idents` in the order
    given) from one pass over the result file; writes <cluster file stem>.<gene|utr>[.<A>+<B>+...].diff_pa_pairs.csv in
    output_dir, one block per pair, the p-values adjusted over the whole file, and returns its path"""
    su = _groups_setup(output_dir, res_pkl_file, cell_cluster_file, idents, n_perm, seed, "diff_pa_pairs", pairs=True)
    names, sizes = su.names, su.sizes.tolist()
    return _diff_pa_blocks(su, n_perm, device, "pair", DIFF_PA_PAIRS_HEADER,
                           [((names[g], names[h]), f"{names[g]}_Vs_{names[h]}", sizes[g], sizes[h])
                            for g, h in zip(su.pairs[0].tolist(), su.pairs[1].tolist())],
                           f"of {len(sizes)} populations ({sum(sizes)} cells)")


# ---------------------------------------------------------------- diff_pa_markers
# For every cluster, which pA sites does it use differently from all other cells (the FindAllMarkers question): every
# marker population tested as diff_pa tests idents_1 without idents_2, in one run.  Options, ident checks and file naming
# are diff_pa_groups's; the markers are every cluster of the file that has a cell (at most 64), or the 1 to 64 named
# ones in the order given, and that is the order of the file's blocks.  Marker X is exactly `diff_pa --idents_1 X` with
# the same --seed and --n_perm.  The tested cells are every column that has a cluster, n of them, the same for every
# marker, and the rest of X is every other tested cell, whether its cluster was named or not.  X's columns ascending
# take the local positions 0 .. n_X - 1, all other tested columns ascending n_X .. n - 1, and permutation p gives X the
# n_X local positions with the smallest key(p, local position): the labellings of diff_pa's masks call for (n_X, n - n_X).
# The kept rows are a record's label rows with a read in any tested cell, the same for every marker; X tests a record
# when two such rows or more remain and both X and its rest have reads; S and d_i go through the device function of
# diff_pa with its slack: t, a, n_ge, gene_n_ge and the bits of gene_stat are diff_pa's.  One line per (marker, kept row
# of a record that the marker tests), `group` = `versus` = the marker.  p_val_adj is Benjamini-Hochberg over ALL lines
# of the file, gene_p_val_adj over all tested (marker, record) combinations: the correction across the runs of the loop.
# The count matrix puts the markers' columns first, segment by segment, then the other tested cells; the device keeps
# every marker's bits in that order and finds a column's local position from its rank among the tested columns
# (include/scape_hip.h), so the counts are read, counted and compacted once for all markers.  No --strata_file.
DIFF_PA_MARKERS_HEADER = DIFF_PA_HEADER[:2] + ["group"] + DIFF_PA_HEADER[2:]
MAX_MARKER_RESULT_BYTES = 256 << 20   # host and device bytes of the counters of one call: more markers are taken in ranges


def _diff_pa_markers(output_dir: str, res_pkl_file: str, cell_cluster_file: str, idents=(), n_perm: int = 9999,
                     seed: int = 1, device=None):
    """diff_pa of every cluster of a cluster file (or of the clusters `idents`, in the order given) against all other
    cells that have a cluster, from one pass over the result file; writes
    <cluster file stem>.<gene|utr>[.<A>+<B>+...].diff_pa_markers.csv in output_dir, one block per marker, the p-values
    adjusted over the whole file, and returns its path"""
    su = _groups_setup(output_dir, res_pkl_file, cell_cluster_file, idents, n_perm, seed, "diff_pa_markers", markers=True)
    return _diff_pa_blocks(su, n_perm, device, "marker", DIFF_PA_MARKERS_HEADER,
                           [((name,), name, n_g, su.n - n_g) for name, n_g in zip(su.names, su.sizes.tolist())],
                           f"among {su.n} cells")


# ---------------------------------------------------------------- diff_pa_len_pairs, diff_pa_len_markers
# What lies behind a significant diff_pa_len_groups, as diff_pa_pairs and diff_pa_markers lie behind diff_pa_groups: every
# pair of the populations, or every population against all other cells that have a cluster, tested as diff_pa_len tests
# two, in one run.  Options, ident checks, populations, their order, column layout, labellings and file naming are
# diff_pa_pairs's and diff_pa_markers's (_groups_setup).  Pair (A, B) is exactly `diff_pa_len --idents_1 A --idents_2 B`
# and marker X exactly `diff_pa_len --idents_1 X` with the same --seed and --n_perm: the item's kept rows are the
# record's label rows with a read in one of its cells (for a marker: in any tested cell, the same for every marker), it
# tests a record when K > 1, two such rows or more remain, both of its populations have reads and span = max x - min x
# over THOSE rows is > 0, and w_i = x_i - min x, tol = 2^-40 span, delta and n_ge are diff_pa_len's over those rows (the
# device walks the one compaction and passes a row without a read in the item over; include/scape_hip.h).  One line per
# (item, record the item tests); every field is diff_pa_len's on that pair or marker as text, p_val_adj aside, which is
# Benjamini-Hochberg over ALL lines of the file: the correction across the runs of the loop.  A non-finite position of a
# row with a read in any tested cell, in any record of K > 1, is diff_pa_len's ValueError.  No --strata_file.
DIFF_PA_LEN_PAIRS_HEADER = DIFF_PA_LEN_HEADER[:1] + ["group_1", "group_2"] + DIFF_PA_LEN_HEADER[1:]
DIFF_PA_LEN_MARKERS_HEADER = DIFF_PA_LEN_HEADER[:1] + ["group"] + DIFF_PA_LEN_HEADER[1:]
MAX_LEN_BLOCK_RESULT_BYTES = 256 << 20    # host and device bytes of the counters of one call: more items are taken in ranges


def _len_pair_items(su, sums):
    """per pair (g, h), in the file's order: g, every row's reads in the two populations, and the two rows of the
    record's exp_length table (below) that are its populations"""
    G = len(su.sizes)
    return [(g, sums[:, g] + sums[:, h], g, h) for g, h in zip(su.pairs[0].tolist(), su.pairs[1].tolist())], \
        lambda cnt: cnt[:G]


def _len_marker_items(su, sums):
    """per marker g: g, every row's reads in the tested cells, and the rows of the record's exp_length table: the
    markers' reads per label first, then those of every marker's rest"""
    M = len(su.sizes)
    t = sums.sum(axis=1)
    return [(g, t, g, M + g) for g in range(M)], lambda cnt: np.concatenate([cnt[:M], cnt.sum(axis=0) - cnt[:M]])


_LEN_BLOCK_TESTS = {"pair": ("scape_hip_report_perm_len_pairs", _len_pair_items),
                    "marker": ("scape_hip_report_perm_len_markers", _len_marker_items)}


def _diff_pa_len_blocks_batch(su, n_perm, noun, blocks, ctx, bat, chunk, times):
    """one counted batch: the rows kept over all segments of its records with two segments or more with reads and a
    span go through diff_pa_len's test of every item (pair, marker), the items in ranges of at most
    MAX_LEN_BLOCK_RESULT_BYTES of counters; appends to blocks[k] what _diff_pa_len_batch appends for the two populations
    of item k, per record that the item tests (decided here, from the sums and the positions)"""
    recs, K = bat.recs, bat.K
    pos = {}                     # record -> positions of its kept rows (f64, finite)
    sel = _perm_rows(ctx, bat, su.seg_off, times, _finite_positions(recs, pos))
    sel = sel and _with_span(sel, pos, times)
    if sel is None:
        return
    entry, items = _LEN_BLOCK_TESTS[noun]
    call = entry[len("scape_hip_"):]
    which, off, rows, sums, rowbase, xs = sel
    n_seg, n_items, n_rows, n_rec = len(su.seg_off) - 1, len(blocks), len(rows), len(which)
    x = np.ascontiguousarray(np.concatenate(xs))
    t, a0 = np.zeros(n_rows, np.int64), np.zeros((n_rows, n_seg), np.int64)
    delta0, n_ge = np.zeros((n_items, n_rec), np.float64), np.zeros((n_items, n_rec), np.int64)
    step = int(max(1, min(n_items, MAX_LEN_BLOCK_RESULT_BYTES // (28 * n_rec))))

    def test():
        for k in range(0, n_items, step):
            m = min(step, n_items - k)
            check(getattr(ctx.lib, entry)(ctx.h, n_rec, ptr(off, P_i64), ptr(rows, P_i64), n_seg, ptr(su.seg_off, P_i32),
                                          k, m, ptr(x), ptr(t, P_i64), ptr(a0, P_i64), ptr(delta0[k:k + m]),
                                          ptr(n_ge[k:k + m], P_i64)), call)
    _perm_chunks(ctx, su, n_perm, chunk, times, test)
    t0 = timer()
    _check_row_sums(call, t, a0, sums, sums)
    rec_of = np.repeat(np.arange(n_rec), np.diff(off))
    item_list, exp_rows = items(su, sums)
    tested = np.zeros((n_items, n_rec), dtype=bool)
    for k, (g, tk, _e1, _e2) in enumerate(item_list):
        own = tk > 0
        A, T = np.add.reduceat(sums[:, g], off[:-1]), np.add.reduceat(tk, off[:-1])
        lo = np.minimum.reduceat(np.where(own, x, np.inf), off[:-1])
        hi = np.maximum.reduceat(np.where(own, x, -np.inf), off[:-1])
        with np.errstate(invalid="ignore"):
            tested[k] = (np.bincount(rec_of[own], minlength=n_rec) >= 2) & (A > 0) & (A < T) & (hi - lo > 0)
        if not np.all(delta0[k][~tested[k]] == 0.0):
            r = int(np.nonzero(~tested[k] & (delta0[k] != 0.0))[0][0])
            raise _lib.ScapeHipError(f"{call}: {recs[which[r]].gene_info_str}: the device's delta {delta0[k, r]!r} of a "
                                     f"record that {noun} {k} does not test")
    times["finish"] += timer() - t0
    any_item = np.nonzero(tested.any(axis=0))[0]
    if not len(any_item):
        return
    # the segments' counts of ALL K labels of the records that any item tests, for the reference's exp_pa_len
    all_rows = np.concatenate([int(rowbase[r]) + np.arange(int(K[r]), dtype=np.int64) for r in which[any_item].tolist()])
    full = np.zeros((len(all_rows), n_seg), dtype=np.int32)
    full_nz = np.zeros((len(all_rows), n_seg), dtype=np.int32)
    t0 = timer()
    check(ctx.lib.scape_hip_report_group_sums(ctx.h, n_seg, ptr(su.seg_off, P_i32), len(all_rows), ptr(all_rows, P_i64),
                                              ptr(full, P_i32), ptr(full_nz, P_i32)), "report_group_sums")
    times["render"] += timer() - t0
    t0 = timer()
    exp_len, k0 = {}, 0          # record -> exp_length of every population an item may name
    for g in any_item.tolist():
        r = which[g]
        k = int(K[r])
        cnt = exp_rows(full[k0:k0 + k].T.astype(np.int64))
        counts = np.zeros((len(cnt), k + 1), dtype=np.int64)     # slot k: reads of no site, which never weigh
        counts[:, :k] = cnt
        k0 += k
        exp_len[g] = _exp_len_rows(k, recs[r].alpha_arr, counts)
    for k, (g, tk, e1, e2) in enumerate(item_list):
        for j in np.nonzero(tested[k])[0].tolist():
            r = which[j]
            own = np.nonzero(tk[off[j]:off[j + 1]] > 0)[0]
            xk = xs[j][own]
            a = sums[off[j]:off[j + 1], g][own]
            b = tk[off[j]:off[j + 1]][own] - a
            m1, m2, d = _mean_positions(xk, a.tolist(), b.tolist())
            if not abs(float(delta0[k, j]) - d) <= np.ldexp(float(xk.max() - xk.min()), -40):
                raise _lib.ScapeHipError(f"{call}: {recs[r].gene_info_str}: the device's delta {delta0[k, j]!r} "
                                         f"differs from {d!r}")
            e = exp_len[j]
            blocks[k].append((recs[r].gene_info_str, len(own), int(a.sum()), int(b.sum()), m1, m2, d, float(e[e1]),
                              float(e[e2]), int(n_ge[k, j])))
    times["finish"] += timer() - t0


def _diff_pa_len_blocks(su, n_perm, device, noun, header, block_ids, tested_among):
    """the run of diff_pa_len_pairs and diff_pa_len_markers: one block of the file per entry of block_ids = (the group
    fields, versus); returns the file's path"""
    blocks = [[] for _ in block_ids]

    def write(w):
        w.writerow(header)
        out = [o for block in blocks for o in block]
        if not out:
            return
        p_val = (1 + np.array([o[9] for o in out], dtype=np.int64)) / (1 + n_perm)
        with np.errstate(invalid="ignore"):
            d_exp = np.array([o[7] for o in out]) - np.array([o[8] for o in out])
        ids = [ident for ident, block in zip(block_ids, blocks) for _o in block]
        w.writerows([o[0], *groups, versus, o[1], o[2], o[3]] + [repr(v) for v in o[4:9]] + [repr(de), o[9], repr(p),
                                                                                              repr(q), n_perm]
                    for (groups, versus), o, de, p, q in zip(ids, out, d_exp.tolist(), p_val.tolist(),
                                                             _bh(p_val).tolist()))

    wall = _perm_run(su, n_perm, device, functools.partial(_diff_pa_len_blocks_batch, su, n_perm, noun, blocks), write)
    print(f"Finish {n_perm} permutations of {len(blocks)} {noun}s {tested_among} for "
          f"{sum(len(block) for block in blocks)} tested ({noun}, record) combinations")
    print(f"Finish {su.res_pkl} in {wall / 60} min.")
    return su.outpath


def _diff_pa_len_pairs(output_dir: str, res_pkl_file: str, cell_cluster_file: str, idents=(), n_perm: int = 9999,
                       seed: int = 1, device=None):
    """diff_pa_len for every pair of the populations of a cluster file (every cluster, or the clusters `idents` in the
    order given) from one pass over the result file; writes <cluster file stem>.<gene|utr>[.<A>+<B>+...]
    .diff_pa_len_pairs.csv in output_dir, one block per pair, p_val_adj over the whole file, and returns its path"""
    su = _groups_setup(output_dir, res_pkl_file, cell_cluster_file, idents, n_perm, seed, "diff_pa_len_pairs", pairs=True)
    names, sizes = su.names, su.sizes.tolist()
    return _diff_pa_len_blocks(su, n_perm, device, "pair", DIFF_PA_LEN_PAIRS_HEADER,
                               [((names[g], names[h]), f"{names[g]}_Vs_{names[h]}")
                                for g, h in zip(su.pairs[0].tolist(), su.pairs[1].tolist())],
                               f"of {len(sizes)} populations ({sum(sizes)} cells)")


def _diff_pa_len_markers(output_dir: str, res_pkl_file: str, cell_cluster_file: str, idents=(), n_perm: int = 9999,
                         seed: int = 1, device=None):
    """diff_pa_len of every cluster of a cluster file (or of the clusters `idents`, in the order given) against all
    other cells that have a cluster, from one pass over the result file; writes <cluster file stem>.<gene|utr>
    [.<A>+<B>+...].diff_pa_len_markers.csv in output_dir, one block per marker, p_val_adj over the whole file, and
    returns its path"""
    su = _groups_setup(output_dir, res_pkl_file, cell_cluster_file, idents, n_perm, seed, "diff_pa_len_markers",
                       markers=True)
    return _diff_pa_len_blocks(su, n_perm, device, "marker", DIFF_PA_LEN_MARKERS_HEADER,
                               [((name,), name) for name in su.names], f"among {su.n} cells")


# ---------------------------------------------------------------- diff_pa_len_groups
# The omnibus form of diff_pa_len: which records change their mean pA position (3'UTR length) across G = 2..64
# populations at all, and which population has the longer or shorter 3'UTRs against all the others.  Options,
# populations, tested columns, permutations and output naming are diff_pa_groups's (same --seed = same labellings; with
# two populations, population 0 is diff_pa_len's population 1); kept rows, positions x_i = alpha_arr[label_i] and the
# refusal of a non-finite position are diff_pa_len's.  A record is tested when diff_pa_groups would test it and
# span = max x - min x > 0.  The G sums per permutation are exact integers on the device, so per record the positions
# become integers first:  w_i = fl(x_i - min x),  frexp(span) = (m, e),  s = 22 - e,  q_i = rint(ldexp(w_i, s)) (half to
# even), so 2^21 <= qspan = max q_i <= 2^22.  Positions that are multiples of 2^-s (integers: the theta grid) are exact,
# others are rounded at about span 2^-22; the p-values are those of the test on the q_i, the position columns of the
# file come from the exact x_i.  With a_ig the sum of kept row i over group g under a labelling:
#     A_g = sum_i a_ig,  T = sum_g A_g < 2^31,  Q_g = sum_i a_ig q_i,  Q = sum_g Q_g
#     D   = sum_{g: A_g > 0} A_g (Q_g / A_g - Q / T)^2 = sum Q_g^2 / A_g - Q^2 / T     tests the record
#     d_g = Q_g / A_g - (Q - Q_g) / (T - A_g)   (0 when A_g = 0 or A_g = T)            tests group g against the others
# D is the between-cluster sum of squares of the position weighted by reads (for G = 2: (A_0 A_1 / T) d_0^2); d_g is
# two-sided.  n_ge = #{p: D(p) >= D(0) - 2^-40 T qspan^2},  n_ge.<g> = #{p: |d_g(p)| >= |d_g(0)| - 2^-40 qspan}, reported
# for the groups whose observed A_g is neither 0 nor T (the others get empty fields);  p = (1 + n_ge) / (1 + n_perm).
# Benjamini-Hochberg over the file's lines for the record, and once over all reported (record, group) pairs of the file
# for the groups.  eta2 = D / sum_i t_i (q_i - Q / T)^2, the share of the position's variance that lies between the
# clusters.  No --strata_file and no exp_length columns.  (include/scape_hip.h states the device's arithmetic and the
# bound that makes the counts exact.)
DIFF_PA_LEN_GROUPS_HEADER = ["gene", "num_pa", "num_groups", "reads", "mean_pos", "eta2", "n_ge", "p_val", "p_val_adj",
                             "top_group", "top_delta_pos", "n_perm"]
DIFF_PA_LEN_GROUPS_PER_GROUP = ["reads", "mean_pos", "delta_pos", "n_ge", "p_val", "p_val_adj"]
LEN_GROUPS_Q_BITS = 22           # qspan lies in 2^21 .. 2^22: T qspan < 2^53, the sums stay exact as integers and in f64


def _quantise_positions(x, bits=LEN_GROUPS_Q_BITS):
    """the integer positions q_i (int32) of a record's kept rows at x (finite f64, span > 0), at `bits` bits: 2^(bits - 1)
    <= max q_i <= 2^bits"""
    w = x - x.min()
    _m, e = math.frexp(float(x.max() - x.min()))
    return np.rint(np.ldexp(w, bits - e)).astype(np.int32)


def _mean_positions_groups(x, a):
    """(mean_pos, [mean_pos.<g>], [delta_pos.<g>]) of positions x (finite f64) under the integer sums a[row][group]:
    delta_pos.<g> = mean_pos.<g> - the mean position of all other groups' reads; the exact rationals, each rounded
    once; None where a group has no read, or every read"""
    ratios = [float(v).as_integer_ratio() for v in x]
    D = max(d for _n, d in ratios)                       # denominators are powers of two
    X = [n * (D // d) for n, d in ratios]
    G = len(a[0])
    A = [sum(int(row[g]) for row in a) for g in range(G)]
    S = [sum(int(row[g]) * Xi for row, Xi in zip(a, X)) for g in range(G)]
    T, St = sum(A), sum(S)
    mean = [float(Fraction(S[g], A[g] * D)) if A[g] else None for g in range(G)]
    delta = [float(Fraction(S[g], A[g] * D) - Fraction(St - S[g], (T - A[g]) * D)) if 0 < A[g] < T else None
             for g in range(G)]
    return float(Fraction(St, T * D)), mean, delta


def _diff_pa_len_groups_batch(su, n_perm, out, ctx, bat, chunk, times):
    """one counted batch: appends (gene, num_pa, [A_g], mean_pos, eta2, n_ge, top group, [mean_pos.<g>],
    [delta_pos.<g>], [n_ge.<g>]) per tested record to `out`"""
    recs, G = bat.recs, len(su.sizes)
    pos = {}                     # record -> positions of its kept rows (f64, finite)
    sel = _perm_rows(ctx, bat, su.seg_off, times, _finite_positions(recs, pos))
    sel = sel and _with_span(sel, pos, times)
    if sel is None:
        return
    which, off, rows, sums, _rowbase, xs = sel
    t0 = timer()
    qs = [_quantise_positions(x) for x in xs]
    q = np.ascontiguousarray(np.concatenate(qs))
    T = np.add.reduceat(sums.sum(axis=1), off[:-1])
    for g, r in enumerate(which.tolist()):
        _check_reads(recs[r], T[g])
    qspan = [int(qi.max()) for qi in qs]
    tol_stat = np.array([math.ldexp(float(int(Tr) * sp * sp), -40) for Tr, sp in zip(T.tolist(), qspan)])
    tol_delta = np.array([math.ldexp(float(sp), -40) for sp in qspan])
    times["finish"] += timer() - t0
    t, a0 = np.zeros(len(rows), np.int64), np.zeros((len(rows), G), np.int64)
    stat0, delta0 = np.zeros(len(which), np.float64), np.zeros((len(which), G), np.float64)
    n_ge, group_ge = np.zeros(len(which), np.int64), np.zeros((len(which), G), np.int64)
    _perm_chunks(ctx, su, n_perm, chunk, times, lambda: check(
        ctx.lib.scape_hip_report_perm_len_groups(ctx.h, len(which), ptr(off, P_i64), ptr(rows, P_i64), G,
                                                 ptr(su.seg_off, P_i32), ptr(q, P_i32), ptr(tol_stat), ptr(tol_delta),
                                                 ptr(t, P_i64), ptr(a0, P_i64), ptr(stat0), ptr(delta0),
                                                 ptr(n_ge, P_i64), ptr(group_ge, P_i64)), "report_perm_len_groups"))
    t0 = timer()
    _check_row_sums("report_perm_len_groups", t, a0, sums, sums)
    for g, r in enumerate(which.tolist()):
        sl = slice(int(off[g]), int(off[g + 1]))
        a, qi = a0[sl].tolist(), qs[g].tolist()
        # the statistics of the observed labelling, exactly, in Python ints on the q_i
        A = [sum(row[k] for row in a) for k in range(G)]
        Qg = [sum(row[k] * v for row, v in zip(a, qi)) for k in range(G)]
        Tr, Q = sum(A), sum(Qg)
        D = sum(Fraction(Qg[k] * Qg[k], A[k]) for k in range(G) if A[k]) - Fraction(Q * Q, Tr)
        _check_exact("report_perm_len_groups", recs[r], ("statistic",), stat0[g], D, Fraction(float(tol_stat[g])))
        # d_k = N_k / M_k with N_k = Q_k T - Q A_k and M_k = A_k (T - A_k) > 0 for a reported group
        N = [Qg[k] * Tr - Q * A[k] for k in range(G)]
        M = [A[k] * (Tr - A[k]) for k in range(G)]
        top = None
        for k in range(G):
            if M[k] == 0:
                continue
            _check_exact("report_perm_len_groups", recs[r], ("delta", "population", su.names[k]), delta0[g, k],
                         Fraction(N[k], M[k]), Fraction(float(tol_delta[g])))
            if top is None or abs(N[k]) * M[top] > abs(N[top]) * M[k]:       # the first wins ties
                top = k
        ss_total = sum(int(ti) * v * v for ti, v in zip(t[sl].tolist(), qi)) - Fraction(Q * Q, Tr)
        mean, mean_g, delta_g = _mean_positions_groups(xs[g], a)
        out.append((recs[r].gene_info_str, len(qi), A, mean, float(D / ss_total), int(n_ge[g]), top, mean_g, delta_g,
                    group_ge[g].tolist()))
    times["finish"] += timer() - t0


def _diff_pa_len_groups(output_dir: str, res_pkl_file: str, cell_cluster_file: str, idents=(), n_perm: int = 9999,
                        seed: int = 1, device=None):
    """permutation test of the mean pA position (3'UTR length) across the populations of a cluster file (every cluster,
    or the clusters `idents` in the order given), and of every population against all the others; writes <cluster file
    stem>.<gene|utr>[.<A>+<B>+...].diff_pa_len_groups.csv in output_dir, one line per tested record, and returns its
    path"""
    su = _groups_setup(output_dir, res_pkl_file, cell_cluster_file, idents, n_perm, seed, "diff_pa_len_groups")
    names, G = su.names, len(su.sizes)
    out = []

    batch = functools.partial(_diff_pa_len_groups_batch, su, n_perm, out)

    def write(w):
        w.writerow(DIFF_PA_LEN_GROUPS_HEADER + [f"{c}.{n}" for n in names for c in DIFF_PA_LEN_GROUPS_PER_GROUP])
        if not out:
            return
        p_val = (1 + np.array([o[5] for o in out], dtype=np.int64)) / (1 + n_perm)
        # one family for the groups: every reported (record, group) pair of the file
        pairs = [(k, g) for k, o in enumerate(out) for g in range(G) if o[8][g] is not None]
        pair_p = (1 + np.array([out[k][9][g] for k, g in pairs], dtype=np.int64)) / (1 + n_perm)
        group_p = {pair: (repr(p), repr(adj)) for pair, p, adj in zip(pairs, pair_p.tolist(), _bh(pair_p).tolist())}
        for k, (o, p, adj) in enumerate(zip(out, p_val.tolist(), _bh(p_val).tolist())):
            gene, num_pa, A, mean, eta2, n_ge, top, mean_g, delta_g, group_ge = o
            line = [gene, num_pa, sum(Ag > 0 for Ag in A), sum(A), repr(mean), repr(eta2), n_ge, repr(p), repr(adj),
                    names[top], repr(delta_g[top]), n_perm]
            for g in range(G):
                line += [A[g], repr(mean_g[g]) if A[g] else ""]
                line += [repr(delta_g[g]), group_ge[g], *group_p[(k, g)]] if (k, g) in group_p else [""] * 4
            w.writerow(line)

    wall = _perm_run(su, n_perm, device, batch, write)
    print(f"Finish {n_perm} permutations of {int(su.sizes.sum())} cells in {G} populations for {len(out)} tested records")
    print(f"Finish {su.res_pkl} in {wall / 60} min.")
    return su.outpath


# ---------------------------------------------------------------- diff_pa_trend
# Does pA usage shift ALONG a per-cell score (pseudotime, a differentiation, cell-cycle or activation score)?  The score
# file has the cluster file's format; its first other column is parsed with float(), and a cell with an empty field, NA
# or nan has no score and is left out (the pseudotime of another lineage).  The tested columns are the scored cells,
# ascending, in front of the count matrix; kept rows are the labels < K with a read in a scored cell, a record is tested
# when it has two or more.  --rank replaces the score x_j by r_j = #{x < x_j} + #{x <= x_j} = 2 x mid-rank - 1.  The
# scores are made integers as diff_pa_len_groups makes positions, at 15 bits: w_j = x_j - min x, frexp(span) = (m, e),
# s = 15 - e, q_j = rint(ldexp(w_j, s)), so 2^14 <= qspan = max q <= 2^15; the test is the test on the q_j, and the
# file's score columns are in units of the quantised scores min x + q 2^-s.  Permutation p >= 1 ranks the cells by
# diff_pa's key(p, j) and gives cell j the score z_p(j) = q[rank of key(p, j)].  Per record, with c_ij the count of kept
# row i in cell j, t_i = sum_j c_ij, T = sum t_i, s_i = sum_j c_ij z(j), S = sum s_i:
#     D   = sum_i t_i (s_i / t_i - S / T)^2                 the gene statistic: between-site sum of squares of the score
#     d_i = s_i / t_i - (S - s_i) / (T - t_i)               site i's reads against the record's other reads (two-sided)
# n_ge = #{p: |d_i(p)| >= |d_i(0)| - 2^-40 qspan}, gene_n_ge = #{p: D(p) >= D(0) - 2^-40 T qspan^2}, p = (1 + n_ge) /
# (1 + n_perm), Benjamini-Hochberg over the file's lines for the sites and over the tested records for the genes.
# mean_score = min x + (s_i / t_i) 2^-s, delta_score = d_i 2^-s (> 0: the site is used by cells further along), eta2 =
# D / (sum_j C_j q_j^2 - S^2 / T), the share of the score's variance over the record's reads that lies between its sites
# (empty when that variance is 0).  (include/scape_hip.h states the device's arithmetic and the bound that makes the
# counts exact: at most 4,000 kept rows per record.)
DIFF_PA_TREND_HEADER = ["gene", "pa_info", "reads", "pct", "mean_score", "delta_score", "n_ge", "p_val", "p_val_adj",
                        "num_pa", "gene_reads", "eta2", "gene_n_ge", "gene_p_val", "gene_p_val_adj", "n_perm"]
TREND_Q_BITS = 15                # qspan lies in 2^14 .. 2^15: a score is a halfword, s_i < 2^46 and S stay exact
MAX_TREND_ROWS = 4000            # kept rows of a record: the rounding bound of D (include/scape_hip.h)


def _read_scores(cell_score_file):
    """{id: score (finite float) or None} of the rows of a score file; a repeated id keeps its last row"""
    ids, texts = _read_clusters(cell_score_file)
    out = {}
    for k, (i, field) in enumerate(zip(ids.tolist(), texts)):
        field = field.strip()
        if field == "" or field.lower() in ("na", "nan"):
            out[i] = None
            continue
        try:
            v = float(field)
        except ValueError:
            raise ValueError(f"{cell_score_file}: row {k + 1} (id {i}): {field!r} is not a number") from None
        if math.isinf(v):
            raise ValueError(f"{cell_score_file}: row {k + 1} (id {i}): the score {field!r} is not finite")
        out[i] = None if math.isnan(v) else v
    return out


def _rank_scores(x):
    """r_j = #{x < x_j} + #{x <= x_j} (f64 holding integers): twice the mid-rank minus one, so ties share a value"""
    srt = np.sort(x)
    return (np.searchsorted(srt, x, side="left") + np.searchsorted(srt, x, side="right")).astype(np.float64)


def _quantise_scores(x):
    """(q_j (uint16), s) of the scores x (finite f64, span > 0): q_j = rint((x_j - min x) 2^s), half to even"""
    w = x - x.min()
    _m, e = math.frexp(float(x.max() - x.min()))
    return np.rint(np.ldexp(w, TREND_Q_BITS - e)).astype(np.uint16), TREND_Q_BITS - e


def _trend_setup(output_dir, res_pkl_file, cell_score_file, rank, n_perm, seed, command="diff_pa_trend"):
    """what diff_pa_trend and diff_pa_len_trend do before the device is opened: the argument and prerequisite checks, the
    scored cells and their integer scores, the id -> column table that puts the scored columns first, ascending, and the
    output path <score file stem>.<gene|utr>[.rank].<command>.csv"""
    _check_perm_args(n_perm, seed)
    inp = _read_inputs(output_dir, res_pkl_file)
    if not os.path.exists(cell_score_file):
        raise Exception("Given cell_score_file file does not exists")
    score = _read_scores(cell_score_file)
    col_score = [score.get(i) for i in inp.col_ids.tolist()]
    cols = np.array([j for j, v in enumerate(col_score) if v is not None], dtype=np.int64)
    n = len(cols)
    if n < 2:
        raise ValueError(f"{n} cells of barcode_index.csv have a score in {cell_score_file}: {command} takes 2 or more")
    if n >= MAX_PERM_CELLS:
        raise ValueError(f"{n} tested cells: {command} takes fewer than {MAX_PERM_CELLS}")
    x = np.array([col_score[j] for j in cols.tolist()], dtype=np.float64)
    if not float(x.max() - x.min()) > 0:
        raise ValueError(f"every scored cell of {cell_score_file} has the score {x[0]!r}: there is no trend to test")
    if not np.isfinite(x.max() - x.min()):
        raise ValueError(f"the scores of {cell_score_file} span more than a float holds")
    if rank:
        x = _rank_scores(x)
    q, shift = _quantise_scores(x)
    _table, slot, seg_off, _seg_pop = _samples([("scored", cols)], 1, inp.n_cols)
    outpath = _out_stem(output_dir, res_pkl_file, cell_score_file, None, None) + (".rank" if rank else "") + \
        f".{command}.csv"

    def labellings(ctx, p_first, p_count):
        check(ctx.lib.scape_hip_report_perm_scores(ctx.h, n, ptr(q, _lib.P_u16), p_first, p_count, seed),
              "report_perm_scores")
    # per permutation the device holds a halfword per cell, and the cells sorted into key buckets (an int32 each)
    return SimpleNamespace(res_pkl=inp.res_pkl, n_cols=inp.n_cols, seg_off=seg_off, n=n, q=q, shift=shift,
                           lo=float(x.min()), outpath=outpath, labellings=labellings, perm_bytes=6 * n,
                           idmap=_IdMap(inp.col_ids, slot, "barcode_index.csv"))


def _diff_pa_trend_batch(su, n_perm, lines, genes, ctx, bat, chunk, times):
    """one counted batch: the kept rows of its tested records go through the trend test; appends the per-line integers
    to `lines` and (gene_info_str, lines, T, S, eta2, gene_n_ge) per tested record to `genes`"""
    sel = _perm_rows(ctx, bat, su.seg_off, times, min_pops=1)
    if sel is None:
        return
    recs = bat.recs
    which, off, rows, nz, sums, rowbase = sel
    for g, r in enumerate(which.tolist()):
        if int(off[g + 1] - off[g]) > MAX_TREND_ROWS:
            raise ValueError(f"{recs[r].gene_info_str}: {int(off[g + 1] - off[g])} pA sites with reads, more than "
                             f"{MAX_TREND_ROWS}: beyond the rounding bound of the statistic")
    t, s0, sq0 = (np.zeros(len(rows), np.int64) for _ in range(3))
    site_ge, gene_ge = np.zeros(len(rows), np.int64), np.zeros(len(which), np.int64)
    d0, stat0 = np.zeros(len(rows), np.float64), np.zeros(len(which), np.float64)
    _perm_chunks(ctx, su, n_perm, chunk, times, lambda: check(
        ctx.lib.scape_hip_report_perm_trend(ctx.h, len(which), ptr(off, P_i64), ptr(rows, P_i64), ptr(t, P_i64),
                                            ptr(s0, P_i64), ptr(sq0, P_i64), ptr(site_ge, P_i64), ptr(d0), ptr(stat0),
                                            ptr(gene_ge, P_i64)), "report_perm_trend"))
    t0 = timer()
    if not np.array_equal(t, sums[:, 0]):
        raise _lib.ScapeHipError("report_perm_trend: row sums differ from report_group_sums")
    qspan = int(su.q.max())
    for g, r in enumerate(which.tolist()):
        a, b = int(off[g]), int(off[g + 1])
        ti, si = t[a:b].tolist(), s0[a:b].tolist()
        T, S = sum(ti), sum(si)
        _check_reads(recs[r], T)
        # the statistics of the observed scores, exactly, in Python ints on the q_j
        D = sum(Fraction(s * s, tt) for s, tt in zip(si, ti)) - Fraction(S * S, T)
        _check_exact("report_perm_trend", recs[r], ("statistic",), stat0[g], D, Fraction(T * qspan * qspan, 1 << 40))
        for k, (s, tt) in enumerate(zip(si, ti)):
            _check_exact("report_perm_trend", recs[r], ("delta", "kept row", k), d0[a + k],
                         Fraction(s * T - S * tt, tt * (T - tt)), Fraction(qspan, 1 << 40), "the exact one")
        ss_total = int(sq0[a:b].sum()) - Fraction(S * S, T)
        genes.append((recs[r].gene_info_str, b - a, T, S, float(D / ss_total) if ss_total else None, int(gene_ge[g])))
        lines["pa"].extend(_pa_info(recs[r], rows[a:b] - int(rowbase[r])))
    for key, arr in (("t", t), ("s", s0), ("nz", nz[:, 0]), ("n_ge", site_ge)):
        lines[key].append(np.asarray(arr, dtype=np.int64).copy())
    times["finish"] += timer() - t0


def _diff_pa_trend(output_dir: str, res_pkl_file: str, cell_score_file: str, rank: bool = False, n_perm: int = 9999,
                   seed: int = 1, device=None):
    """permutation test of pA usage along the per-cell score of a score file (its ranks with rank=True); writes <score
    file stem>.<gene|utr>[.rank].diff_pa_trend.csv in output_dir, one line per kept row of a tested record, and
    returns its path"""
    su = _trend_setup(output_dir, res_pkl_file, cell_score_file, rank, n_perm, seed)
    lines = {k: [] for k in ("pa", "t", "s", "nz", "n_ge")}
    genes = []                   # (gene_info_str, lines, T, S, eta2, gene_n_ge) per tested record

    batch = functools.partial(_diff_pa_trend_batch, su, n_perm, lines, genes)

    def write(w):
        w.writerow(DIFF_PA_TREND_HEADER)
        if not genes:
            return
        t, s, nz, n_ge = (np.concatenate(lines[k]) for k in ("t", "s", "nz", "n_ge"))
        p_val = (1 + n_ge) / (1 + n_perm)
        gene_p = (1 + np.array([g[5] for g in genes], dtype=np.int64)) / (1 + n_perm)
        p_adj, gene_adj = _bh(p_val).tolist(), _bh(gene_p).tolist()
        # a score of the file is min x + q 2^-s: exact rationals, each rounded once
        lo, unit = Fraction(su.lo), Fraction(2) ** -su.shift
        k = 0
        for g, (gene, n_lines, T, S, eta2, gene_ge) in enumerate(genes):
            tail = [n_lines, T, "" if eta2 is None else repr(eta2), gene_ge, repr(float(gene_p[g])), repr(gene_adj[g]),
                    n_perm]
            for _ in range(n_lines):
                ti, si = int(t[k]), int(s[k])
                w.writerow([gene, lines["pa"][k], ti, repr(float(nz[k] / su.n)), repr(float(lo + Fraction(si, ti) * unit)),
                            repr(float(Fraction(si * T - S * ti, ti * (T - ti)) * unit)), int(n_ge[k]),
                            repr(float(p_val[k])), repr(p_adj[k])] + tail)
                k += 1

    wall = _perm_run(su, n_perm, device, batch, write)
    print(f"Finish {n_perm} permutations of the scores of {su.n} cells for {sum(g[1] for g in genes)} pA sites of "
          f"{len(genes)} tested records")
    print(f"Finish {su.res_pkl} in {wall / 60} min.")
    return su.outpath


# ---------------------------------------------------------------- diff_pa_len_trend
# Do 3'UTRs lengthen or shorten ALONG a per-cell score?  The length form of diff_pa_trend, as diff_pa_len is diff_pa's:
# options, score file, scored cells, integer scores q_j and permutations are diff_pa_trend's (same --seed = same permuted
# scores); kept rows, positions x_i = alpha_arr[label_i] and the refusal of a non-finite position are diff_pa_len's.  A
# record is tested when it has two kept rows or more in scored cells and they lie at two positions or more.  Per record
# the positions become integers by diff_pa_len_groups's rule at B = min(22, 48 - T.bit_length()) bits (22 bits below 2^26
# reads, 17 at the limit of 2^31 - 1), and the scores z under a labelling give, with c_ij the count of kept row i in
# cell j:
#     t_i = sum_j c_ij,  T = sum t_i < 2^31,  Sx = sum t_i x_i < 2^48                                   (fixed)
#     s_i = sum_j c_ij z(j),  Sz = sum s_i < 2^46,  Sxz = sum x_i s_i < 2^63                            (per labelling)
#     C   = T Sxz - Sx Sz     = T^2 x the covariance of position and score over the record's reads
# T, Sx and sum t_i x_i^2 are fixed, so |C| orders the labellings as the absolute slope of the score regressed on the
# position does: diff_pa_trend's reading (the score as the response), carried from sites to positions.  n_ge = #{p in
# 1..n_perm: |C(p)| >= |C(0)|}, two-sided and compared as 128-bit integers on the device: no rounding, no band.  p =
# (1 + n_ge) / (1 + n_perm), Benjamini-Hochberg over the file's lines.  With Vz = T sum_j C_j q_j^2 - Sz^2 and Vx = T sum
# t_i x_i^2 - Sx^2 (T^2 x the variances over the reads):  slope = C / Vz in nucleotides per unit of score, delta_pos =
# slope x the span of the quantised scores (the shift from the first to the last cell; > 0: 3'UTRs lengthen along the
# score - the column to read beside diff_pa_len's), r = C / sqrt(Vz Vx) (Pearson); the three are empty when Vz = 0, where
# C(0) = 0, every permutation is counted and p = 1.  mean_pos comes from the exact x_i, mean_score = min x + (Sz / T)
# 2^-s.  No --strata_file, no exp_length columns, and no per-site lines: the test is per gene.
DIFF_PA_LEN_TREND_HEADER = ["gene", "num_pa", "reads", "mean_pos", "mean_score", "slope", "delta_pos", "r", "n_ge",
                            "p_val", "p_val_adj", "n_perm"]
LEN_TREND_MAX_Q_BITS = 22        # the device takes positions of up to 2^22
LEN_TREND_TX_BITS = 48           # T max x < 2^48: at scores of up to 2^15, Sxz stays below 2^63


def _len_trend_bits(T):
    """the bits of a record's integer positions: T < 2^T.bit_length() and max x <= 2^B give T max x < 2^48"""
    return min(LEN_TREND_MAX_Q_BITS, LEN_TREND_TX_BITS - int(T).bit_length())


def _diff_pa_len_trend_batch(su, n_perm, out, ctx, bat, chunk, times):
    """one counted batch: appends (gene, num_pa, T, mean_pos, mean_score, slope, delta_pos, r, n_ge) per tested record
    to `out`; slope, delta_pos and r are None when the score has no variance over the record's reads"""
    recs = bat.recs
    pos = {}                     # record -> positions of its kept rows (f64, finite)
    sel = _perm_rows(ctx, bat, su.seg_off, times, _finite_positions(recs, pos), min_pops=1)
    sel = sel and _with_span(sel, pos, times)
    if sel is None:
        return
    which, off, rows, sums, _rowbase, xs = sel
    t0 = timer()
    Ts = np.add.reduceat(sums[:, 0], off[:-1]).tolist()
    for g, r in enumerate(which.tolist()):
        _check_reads(recs[r], Ts[g])
    bits = [_len_trend_bits(T) for T in Ts]
    qs = [_quantise_positions(x, b) for x, b in zip(xs, bits)]
    q = np.ascontiguousarray(np.concatenate(qs))
    times["finish"] += timer() - t0
    t, s0, sq0 = (np.zeros(len(rows), np.int64) for _ in range(3))
    c0, n_ge = np.zeros(2 * len(which), np.int64), np.zeros(len(which), np.int64)
    _perm_chunks(ctx, su, n_perm, chunk, times, lambda: check(
        ctx.lib.scape_hip_report_perm_len_trend(ctx.h, len(which), ptr(off, P_i64), ptr(rows, P_i64), ptr(q, P_i32),
                                                ptr(t, P_i64), ptr(s0, P_i64), ptr(sq0, P_i64), ptr(c0, P_i64),
                                                ptr(n_ge, P_i64)), "report_perm_len_trend"))
    t0 = timer()
    if not np.array_equal(t, sums[:, 0]):
        raise _lib.ScapeHipError("report_perm_len_trend: row sums differ from report_group_sums")
    lo, unit_z, qspan = Fraction(su.lo), Fraction(2) ** -su.shift, int(su.q.max())
    for g, r in enumerate(which.tolist()):
        sl = slice(int(off[g]), int(off[g + 1]))
        ti, si, xi = t[sl].tolist(), s0[sl].tolist(), qs[g].tolist()
        # the statistic of the observed scores, exactly, in Python ints
        T, Sx, Sz = Ts[g], sum(a * b for a, b in zip(ti, xi)), sum(si)
        C = T * sum(a * b for a, b in zip(xi, si)) - Sx * Sz
        if (int(c0[2 * g + 1]) << 64) + (int(c0[2 * g]) & ((1 << 64) - 1)) != C:
            raise _lib.ScapeHipError(f"report_perm_len_trend: {recs[r].gene_info_str}: the device's C(0), halves "
                                     f"{int(c0[2 * g])} and {int(c0[2 * g + 1])}, differs from {C}")
        Vz = T * sum(sq0[sl].tolist()) - Sz * Sz
        Vx = T * sum(a * b * b for a, b in zip(ti, xi)) - Sx * Sx
        _m, e = math.frexp(float(xs[g].max() - xs[g].min()))
        unit_x = Fraction(2) ** (e - bits[g])
        slope = delta = corr = None
        if Vz:
            slope = float(Fraction(C, Vz) * unit_x / unit_z)
            delta = float(Fraction(C * qspan, Vz) * unit_x)
            corr = math.copysign(math.sqrt(float(Fraction(C * C, Vz * Vx))), C)
        mean_pos, _mean_g, _delta_g = _mean_positions_groups(xs[g], [[a] for a in ti])
        out.append((recs[r].gene_info_str, len(ti), T, mean_pos, float(lo + Fraction(Sz, T) * unit_z), slope, delta,
                    corr, int(n_ge[g])))
    times["finish"] += timer() - t0


def _diff_pa_len_trend(output_dir: str, res_pkl_file: str, cell_score_file: str, rank: bool = False, n_perm: int = 9999,
                       seed: int = 1, device=None):
    """permutation test of the pA position (3'UTR length) along the per-cell score of a score file (its ranks with
    rank=True); writes <score file stem>.<gene|utr>[.rank].diff_pa_len_trend.csv in output_dir, one line per tested
    record, and returns its path"""
    su = _trend_setup(output_dir, res_pkl_file, cell_score_file, rank, n_perm, seed, "diff_pa_len_trend")
    out = []

    batch = functools.partial(_diff_pa_len_trend_batch, su, n_perm, out)

    def write(w):
        w.writerow(DIFF_PA_LEN_TREND_HEADER)
        if not out:
            return
        p_val = (1 + np.array([o[8] for o in out], dtype=np.int64)) / (1 + n_perm)
        w.writerows(list(o[:3]) + [repr(o[3]), repr(o[4])] + ["" if v is None else repr(v) for v in o[5:8]] +
                    [o[8], repr(p), repr(adj), n_perm] for o, p, adj in zip(out, p_val.tolist(), _bh(p_val).tolist()))

    wall = _perm_run(su, n_perm, device, batch, write)
    print(f"Finish {n_perm} permutations of the scores of {su.n} cells for {len(out)} tested records")
    print(f"Finish {su.res_pkl} in {wall / 60} min.")
    return su.outpath


# ---------------------------------------------------------------- boot_pa_len
# How well is a cluster's 3'UTR length known?  Percentile intervals of the mean pA position, and of the reference's
# exp_length, per record and population, by the cell bootstrap: cells are the exchangeable units, as in the permutation
# tests.  One population per cluster of the cluster file that has a column (order of first appearance, at most 64), or
# the 1 to 64 clusters named by --idents in the order given, or, without a cluster file, the one population all_cell of
# every column.  Tested columns: population 0's matrix columns ascending, then population 1's, ... (_samples): positions
# j = 0 .. n-1, and position j carries cell[j], the 0-based column its cell has in ex_pa_cnt_mat's matrix (inp.col_ids
# order).  The Poisson bootstrap: cell c gets the multiplicity m(b, c) in replicate b = 1 .. n_boot, all arithmetic mod
# 2^64, G and mix those of diff_pa's key:
#     h(b, c) = mix(mix(seed + G b) + G (c + 1)),   m(b, c) = #{k in 0..14: h(b, c) >= P[k]},   replicate 0: m = 1
#     P[k] = floor(2^64 e^-1 sum_{i <= k} 1 / i!) = BOOT_THRESHOLDS[k]: Poisson(1), the tail beyond 15 folded into 15
# The hash sees the cell, not the position: replicate b is the same resampled data set for every cluster, every
# --idents choice and every later command.  Kept rows are the labels < K with a read in a tested cell; a record is
# reported when it has two or more and span = max x - min x > 0 over their positions x_i = alpha_arr[label] (a
# non-finite one is diff_pa_len's ValueError); q_i and s are diff_pa_len_groups's (_quantise_positions, 22 bits); a record
# of 2^27 reads or more in the tested cells is a ValueError.  With c_ij the count of kept row i at position j:
#     A_g(b) = sum_i sum_{j in g} m(b, cell[j]) c_ij,   Q_g(b) = sum_i q_i sum_{j in g} m(b, cell[j]) c_ij   (exact integers)
#     v_g(b) = (double)Q_g(b) / (double)A_g(b), one IEEE division;  +infinity when A_g(b) = 0
#     D_g = #{b in 1..n_boot: A_g(b) > 0},   k = max(1, (D_g + 1) (10000 - L) // 20000),   L = the level in basis points
#     lo = the k-th smallest of the n_boot values,  hi = the (D_g + 1 - k)-th smallest;  no interval when D_g = 0
# One line per reported record and population with A_g(0) > 0: reads = A_g(0), mean_pos = the exact rational of the exact
# x_i rounded once (diff_pa_len_groups's mean_pos.<g>), mean_pos_lo / _hi = min x + ldexp(lo / hi, -s), exp_length =
# _exp_len_rows of the population's counts over all K labels, exp_length_lo / _hi = 1.0 + 9.0 * (y - a[0]) / (a[-1] - a[0])
# with y = mean_pos_lo / _hi and a = alpha_arr (empty when exp_length is nan or a[-1] - a[0] is not finite and positive),
# n_empty = n_boot - D_g.  Everything is an integer up to one correctly rounded division per value, so the file is exact
# text.  (include/scape_hip.h states the device's side.)
BOOT_PA_LEN_HEADER = ["gene", "group", "num_pa", "reads", "mean_pos", "mean_pos_lo", "mean_pos_hi", "exp_length",
                      "exp_length_lo", "exp_length_hi", "n_empty", "n_boot", "level"]
BOOT_THRESHOLDS = (0x5E2D58D8B3BCDF1A, 0xBC5AB1B16779BE35, 0xEB715E1DC1582DC2, 0xFB23979734A252F1, 0xFF1025F59174DC3D,
                   0xFFD90F3BA4055E19, 0xFFFA8B71FC72C913, 0xFFFF540C0914B3C9, 0xFFFFED1F4AA8F120, 0xFFFFFE216E641462,
                   0xFFFFFFD4D85D3183, 0xFFFFFFFC6DA262B4, 0xFFFFFFFFBA12D178, 0xFFFFFFFFFB07C64C, 0xFFFFFFFFFFAB8EA5)
BOOT_MAX_READS = 1 << 27         # reads of a record in the tested cells: 15 T stays below 2^31 and 15 T 2^22 below 2^53


def _parse_level(level):
    """the level in basis points: a decimal string in percent with at most two decimals, 0 < level < 100, through
    decimal, never a float ("95" -> 9500, "99.5" -> 9950, "90.00" -> 9000)"""
    text = str(level)
    if not re.fullmatch(r"[0-9]+(\.[0-9]{1,2})?", text):
        raise ValueError(f"level must be a percentage with at most two decimals, such as 95 or 99.5, not {text!r}")
    bp = int(decimal.Decimal(text) * 100)
    if not 0 < bp < 10000:
        raise ValueError(f"level must lie above 0 and below 100, not {text!r}")
    return bp


def _boot_rank(n_def, level_bp):
    """k of the interval rule: lo is the k-th smallest value and hi the (n_def + 1 - k)-th"""
    return max(1, (n_def + 1) * (10000 - level_bp) // 20000)


def _check_boot_args(n_boot, level, seed):
    """the option checks of the bootstrap commands; returns the level in basis points"""
    if n_boot < 1:
        raise ValueError(f"n_boot must be at least 1, not {n_boot}")
    if n_boot >= 1 << 31:
        raise ValueError(f"n_boot must be below 2^31, not {n_boot}")
    if not 0 <= seed < 1 << 64:
        raise ValueError(f"seed must lie in 0 .. 2^64 - 1, not {seed}")
    return _parse_level(level)


def _boot_populations(inp, pops, outpath, level, level_bp, seed, command):
    """the tail of the bootstrap commands' setups, from the populations on: the id -> column table that puts population
    0's columns first, the cell of every position and the multiplicities' call"""
    sizes = np.array([len(cols) for _name, cols in pops], dtype=np.int32)
    n = int(sizes.sum())
    if n >= MAX_PERM_CELLS:
        raise ValueError(f"{n} tested cells: {command} takes fewer than {MAX_PERM_CELLS}")
    _table, slot, seg_off, _seg_pop = _samples(pops, 1, inp.n_cols)
    cell = np.ascontiguousarray(np.concatenate([cols for _name, cols in pops]), dtype=np.int32)

    def labellings(ctx, b_first, b_count):
        check(ctx.lib.scape_hip_report_boot_mult(ctx.h, n, ptr(cell, P_i32), b_first, b_count, seed), "report_boot_mult")
    return SimpleNamespace(res_pkl=inp.res_pkl, n_cols=inp.n_cols, seg_off=seg_off, sizes=sizes, n=n, cell=cell,
                           names=[name for name, _cols in pops], outpath=outpath, level=str(level), level_bp=level_bp,
                           perm_bytes=n,                 # one byte per tested cell and replicate
                           labellings=labellings, idmap=_IdMap(inp.col_ids, slot, "barcode_index.csv"))


def _boot_setup(output_dir, res_pkl_file, cell_cluster_file, idents, n_boot, level, seed, command="boot_pa_len"):
    """what boot_pa_len and boot_pa_usage (`command`: the name in messages and the output suffix) do before the device
    is opened: the option checks, then the prerequisites and the populations (_groups_setup's checks of --idents;
    without a cluster file the one population all_cell), the id -> column table that puts population 0's columns
    first, the cell of every position, and the output path
    <cluster file stem>.<gene|utr>[.<A>+<B>+...].<command>.csv or all_cell.<gene|utr>.<command>.csv"""
    level_bp = _check_boot_args(n_boot, level, seed)
    if cell_cluster_file is None:
        if idents:
            raise ValueError("idents needs a cell_cluster_file")
        inp = _read_inputs(output_dir, res_pkl_file)
        pops = [("all_cell", np.arange(inp.n_cols, dtype=np.int64))]
        outpath = os.path.join(output_dir, "all_cell." + res_pkl_file.replace(".pkl", "").replace("res.", "") +
                               f".{command}.csv")
    else:
        idents, tag, inp, pops = _ident_populations(output_dir, res_pkl_file, cell_cluster_file, idents)
        if not idents and len(pops) > MAX_GROUPS:
            raise ValueError(f"{len(pops)} clusters: {command} takes at most {MAX_GROUPS} at once, name them with "
                             "--idents")
        if not 1 <= len(pops) <= MAX_GROUPS:
            raise ValueError(f"{len(pops)} populations: {command} takes 1 to {MAX_GROUPS}")
        outpath = _out_stem(output_dir, res_pkl_file, cell_cluster_file, None, None) + tag + f".{command}.csv"
    return _boot_populations(inp, pops, outpath, level, level_bp, seed, command)


def _boot_diff_setup(output_dir, res_pkl_file, cell_cluster_file, idents_1, idents_2, n_boot, level, seed, command):
    """what boot_pa_len_diff and boot_pa_usage_diff do before the device is opened: diff_pa's checks of the idents and
    its two populations (_two_populations), _boot_setup's option checks between them, then _boot_setup's tail on
    population 1's columns followed by population 2's; the output path is
    <cluster file stem>.<gene|utr>.<A>_vs_<B|rest>.<command>.csv"""
    inp = _two_populations(output_dir, res_pkl_file, cell_cluster_file, idents_1, idents_2,
                           lambda: _check_boot_args(n_boot, level, seed))
    outpath = _out_stem(output_dir, res_pkl_file, cell_cluster_file, idents_1, idents_2) + f".{command}.csv"
    su = _boot_populations(inp, inp.pops, outpath, level, _parse_level(level), seed, command)
    su.versus = _versus(idents_1, idents_2)
    return su


def _boot_columns(lo, hi, x_min, s, alpha_arr, exp_length):
    """the four interval fields of a line as text, from the order statistics lo and hi of the integer positions (None:
    no replicate has a read), min x and the scale s of the record: mean_pos_lo / _hi = min x + ldexp(lo / hi, -s), one
    f64 add each, and exp_length_lo / _hi = 1.0 + 9.0 * (y - a[0]) / (a[-1] - a[0]) in f64 in that order of operations,
    empty when exp_length is nan or a[-1] - a[0] is not finite and positive"""
    if lo is None:
        return ["", "", "", ""]
    ys = [float(x_min) + math.ldexp(float(v), -s) for v in (lo, hi)]
    a = np.asarray(alpha_arr, dtype=np.float64)
    a0, width = float(a[0]), float(a[-1]) - float(a[0])
    if math.isnan(exp_length) or not (math.isfinite(width) and width > 0):
        return [repr(ys[0]), repr(ys[1]), "", ""]
    return [repr(y) for y in ys] + [repr(1.0 + 9.0 * (y - a0) / width) for y in ys]


def _check_boot_reads(recs, which, off, sums):
    """a record of BOOT_MAX_READS reads or more in the tested cells is a ValueError (sums: per kept row and population)"""
    T = np.add.reduceat(sums.sum(axis=1), off[:-1])
    for g, r in enumerate(which.tolist()):
        if int(T[g]) >= BOOT_MAX_READS:
            raise ValueError(f"{recs[r].gene_info_str}: 2^27 or more reads in the tested cells")


def _boot_positions(xs):
    """the integer positions q of the kept rows of the records with positions xs, one array, and the scale s per record:
    q_i = (x_i - min x) 2^s rounded (_quantise_positions)"""
    q = np.ascontiguousarray(np.concatenate([_quantise_positions(x) for x in xs]))
    return q, [LEN_GROUPS_Q_BITS - math.frexp(float(x.max() - x.min()))[1] for x in xs]


def _boot_quantiles(ctx, su, n_series, times):
    """(lo, hi, D) per series of the record set on the device, at the run's level"""
    lo, hi = np.zeros(n_series, np.float64), np.zeros(n_series, np.float64)
    n_def = np.zeros(n_series, np.int64)
    t0 = timer()
    check(ctx.lib.scape_hip_report_boot_quantiles(ctx.h, su.level_bp, ptr(lo), ptr(hi), ptr(n_def, P_i64)),
          "report_boot_quantiles")
    times["render"] += timer() - t0
    return lo, hi, n_def


def _boot_batch(kind, su, n_boot, out, ctx, bat, chunk, times):
    """one counted batch of a bootstrap command, `kind` its description: what the four commands share, from the tested
    records to the intervals, then kind.lines(su, n_boot, out, recs, b) appends the file's lines (lists of fields) of
    the batch's reported records to `out` and counts them in su.  kind.positions: the command is about positions, so it
    takes the records with a span, hands the device their integer positions and reports exp_length, and a series
    belongs to a record, otherwise to a kept row; kind.diff: the populations are two, both with reads, and a series is
    their difference, otherwise one population with reads is enough and every population has a series; kind.call: the
    entry point.  b holds which, off, rows, rowbase, t, a0 and lo, hi, n_def by [record or kept row, series], and of a
    command with positions xs, scale, exp_len"""
    recs, G = bat.recs, len(su.sizes)
    pos = {}                     # record -> positions of its kept rows (f64, finite)
    sel = _perm_rows(ctx, bat, su.seg_off, times, _finite_positions(recs, pos) if kind.positions else None,
                     min_pops=2 if kind.diff else 1)
    if kind.positions:
        sel = sel and _with_span(sel, pos, times)
    if sel is None:
        return
    b = SimpleNamespace(xs=None, scale=None, exp_len=None)
    if kind.positions:
        b.which, b.off, b.rows, sums, b.rowbase, b.xs = sel
    else:
        b.which, b.off, b.rows, _nz, sums, b.rowbase = sel
    t0 = timer()
    _check_boot_reads(recs, b.which, b.off, sums)
    if kind.positions:
        q, b.scale = _boot_positions(b.xs)
    times["finish"] += timer() - t0
    b.t, b.a0 = np.zeros(len(b.rows), np.int64), np.zeros((len(b.rows), G), np.int64)
    args = ([ctx.h, len(b.which), ptr(b.off, P_i64), ptr(b.rows, P_i64), G, ptr(su.seg_off, P_i32)] +
            ([ptr(q, P_i32)] if kind.positions else []) + [n_boot, ptr(b.t, P_i64), ptr(b.a0, P_i64)])
    entry = getattr(ctx.lib, "scape_hip_" + kind.call)
    _perm_chunks(ctx, su, n_boot, chunk, times, lambda: check(entry(*args), kind.call))
    _check_row_sums(kind.call, b.t, b.a0, sums, sums)
    shape = (len(b.which) if kind.positions else len(b.rows), 1 if kind.diff else G)
    b.lo, b.hi, b.n_def = (v.reshape(shape) for v in _boot_quantiles(ctx, su, shape[0] * shape[1], times))
    if kind.positions:
        b.exp_len = _exp_lengths(ctx, su.seg_off, bat, b.which, b.rowbase, times)
    t0 = timer()
    kind.lines(su, n_boot, out, recs, b)
    times["finish"] += timer() - t0


def _boot_run(kind, su, n_boot, device):
    """the run of a bootstrap command (`kind`: its description) behind its setup su: _boot_batch's batches through
    _perm_run and the file, kind.header and the lines; returns the lines, and su.wall holds the wall seconds"""
    su.n_records = su.n_sites = 0
    out = []
    # the replicate values, 8 bytes each, of every series: per record, or per label of a record (at most that many
    # kept rows), of every population or of the one difference
    series = 1 if kind.diff else len(su.sizes)

    def write(w):
        w.writerow(kind.header)
        w.writerows(out)

    su.wall = _perm_run(su, n_boot, device, functools.partial(_boot_batch, kind, su, n_boot, out), write,
                        record_bytes=lambda p: (1 if kind.positions else int(p.K)) * series * n_boot * 8)
    return out


def _boot_pa_len_lines(su, n_boot, out, recs, b):
    for g, r in enumerate(b.which.tolist()):
        sl = slice(int(b.off[g]), int(b.off[g + 1]))
        a = b.a0[sl]
        _mean, mean_g, _delta = _mean_positions_groups(b.xs[g], a.tolist())
        e = b.exp_len[g]
        A = a.sum(axis=0)
        for p in range(len(su.sizes)):
            if A[p] == 0:
                continue
            D = int(b.n_def[g, p])
            ends = (float(b.lo[g, p]), float(b.hi[g, p])) if D else (None, None)
            iv = _boot_columns(*ends, float(b.xs[g].min()), b.scale[g], recs[r].alpha_arr, float(e[p]))
            out.append([recs[r].gene_info_str, su.names[p], int(b.off[g + 1] - b.off[g]), int(A[p]), repr(mean_g[p])] +
                       iv[:2] + [repr(float(e[p]))] + iv[2:] + [n_boot - D, n_boot, su.level])
        su.n_records += 1


_BOOT_PA_LEN = SimpleNamespace(header=BOOT_PA_LEN_HEADER, call="report_boot_len", positions=True, diff=False,
                               lines=_boot_pa_len_lines)


def _boot_pa_len(output_dir: str, res_pkl_file: str, cell_cluster_file=None, idents=(), n_boot: int = 9999,
                 level="95", seed: int = 1, device=None):
    """percentile bootstrap intervals of the mean pA position and of exp_length per record and population (every cluster
    of the cluster file, the clusters `idents` in the order given, or all cells without a cluster file), by resampling
    the cells; writes <cluster file stem>.<gene|utr>[.<A>+<B>+...].boot_pa_len.csv or all_cell.<gene|utr>
    .boot_pa_len.csv in output_dir, one line per reported record and population with reads, and returns its path"""
    su = _boot_setup(output_dir, res_pkl_file, cell_cluster_file, idents, n_boot, level, seed)
    _boot_run(_BOOT_PA_LEN, su, n_boot, device)
    print(f"Finish {n_boot} bootstrap replicates of {su.n} cells in {len(su.sizes)} populations for {su.n_records} "
          "reported records")
    print(f"Finish {su.res_pkl} in {su.wall / 60} min.")
    return su.outpath


# ---------------------------------------------------------------- boot_pa_usage
# How well is a cluster's usage of a pA site known?  Percentile intervals of the quantity the diff_pa family tests, per
# record, kept row (site) and population, from boot_pa_len's cell bootstrap: options, checks, populations, tested columns
# and the multiplicities m(b, c) are boot_pa_len's (_boot_setup), so replicate b is the same resampled data set in both
# files.  Kept rows of a record are the labels < K with a read in a tested cell; a record is reported when it has two or
# more.  Positions play no part: no span condition, and alpha_arr need not be finite.  A record of 2^27 reads or more in
# the tested cells is boot_pa_len's ValueError.  With c_ij the count of kept row i at position j, m = 1 for b = 0:
#     a_ig(b) = sum_{j in g} m(b, cell[j]) c_ij,   A_g(b) = sum_i a_ig(b)                 (exact integers, A <= 15 T < 2^31)
#     u_ig(b) = (double)a_ig(b) / (double)A_g(b), one IEEE division;  +infinity when A_g(b) = 0
#     D_g, k, lo, hi: boot_pa_len's rule, per series (kept row i, population g) over u_ig(1 .. n_boot)
# Every defined value lies in 0 .. 1, so the bit patterns order as the values do and the select is boot_pa_len's.  One
# line per reported record, kept row and population with A_g(0) > 0, records in file order, then kept rows by ascending
# label, then populations in their order: pa_info = diff_pa's, num_pa = the kept rows, reads = a_ig(0), gene_reads =
# A_g(0), usage = repr(a_ig(0) / A_g(0)) (diff_pa's usage.1 text for the same populations), usage_lo / _hi = repr of lo /
# hi (empty when D_g = 0), n_empty = n_boot - D_g.  A site the population has no read at keeps its line (reads 0, usage
# 0.0): its upper end is information.  Nothing rounds but the one division, so the file is exact text.
BOOT_PA_USAGE_HEADER = ["gene", "pa_info", "group", "num_pa", "reads", "gene_reads", "usage", "usage_lo", "usage_hi",
                        "n_empty", "n_boot", "level"]


def _boot_pa_usage_lines(su, n_boot, out, recs, b):
    for g, r in enumerate(b.which.tolist()):
        i0, i1 = int(b.off[g]), int(b.off[g + 1])
        A = b.a0[i0:i1].sum(axis=0).tolist()
        pa = _pa_info(recs[r], b.rows[i0:i1] - int(b.rowbase[r]))
        for i in range(i0, i1):
            a, D = b.a0[i].tolist(), b.n_def[i].tolist()
            for p in range(len(su.sizes)):
                if A[p] == 0:
                    continue
                ends = [repr(float(b.lo[i, p])), repr(float(b.hi[i, p]))] if D[p] else ["", ""]
                out.append([recs[r].gene_info_str, pa[i - i0], su.names[p], i1 - i0, a[p], A[p], repr(a[p] / A[p])] +
                           ends + [n_boot - D[p], n_boot, su.level])
        su.n_records += 1
        su.n_sites += i1 - i0


_BOOT_PA_USAGE = SimpleNamespace(header=BOOT_PA_USAGE_HEADER, call="report_boot_usage", positions=False, diff=False,
                                 lines=_boot_pa_usage_lines)


def _boot_pa_usage(output_dir: str, res_pkl_file: str, cell_cluster_file=None, idents=(), n_boot: int = 9999,
                   level="95", seed: int = 1, device=None):
    """percentile bootstrap intervals of the usage of every pA site per record and population (every cluster of the
    cluster file, the clusters `idents` in the order given, or all cells without a cluster file), by resampling the
    cells with boot_pa_len's replicates; writes <cluster file stem>.<gene|utr>[.<A>+<B>+...].boot_pa_usage.csv or
    all_cell.<gene|utr>.boot_pa_usage.csv in output_dir, one line per reported record, site and population with reads,
    and returns its path"""
    su = _boot_setup(output_dir, res_pkl_file, cell_cluster_file, idents, n_boot, level, seed, "boot_pa_usage")
    _boot_run(_BOOT_PA_USAGE, su, n_boot, device)
    print(f"Finish {n_boot} bootstrap replicates of {su.n} cells in {len(su.sizes)} populations for {su.n_sites} pA sites "
          f"of {su.n_records} reported records")
    print(f"Finish {su.res_pkl} in {su.wall / 60} min.")
    return su.outpath


# ---------------------------------------------------------------- boot_pa_len_diff, boot_pa_usage_diff
# The effect size beside diff_pa_len's and diff_pa's p-values, with its uncertainty: percentile intervals of population 1
# minus population 2.  They cannot be read off the two populations' own intervals, whose replicate values are correlated
# within a replicate.  Populations and tested columns are diff_pa's (_two_populations; population 1's matrix columns
# first, ascending, then population 2's; without --idents_2 population 2 is every other cell that has a cluster), options,
# cell[j] and m(b, c) are boot_pa_len's: replicate b is the same resampled data set in all four bootstrap files.
# boot_pa_len_diff reports diff_pa_len's tested records (two kept rows or more, span > 0, reads in both populations; q_i
# and s as in boot_pa_len), one series per record:
#     d(b) = (double)Q_1(b) / (double)A_1(b) - (double)Q_2(b) / (double)A_2(b);  +infinity when A_1(b) = 0 or A_2(b) = 0
# two IEEE divisions and one subtraction; D, k, lo, hi by boot_pa_len's rule over the D defined values.  The eleven columns
# it shares with diff_pa_len are that command's text.  delta_pos_lo / _hi = ldexp(lo / hi, -s) (exact, min x cancels),
# delta_exp_length_lo / _hi = 9.0 * y / (a[-1] - a[0]) with y that end of delta_pos (empty when either exp_length is nan or
# the width is not finite and positive, _boot_columns' rule), n_empty = n_boot - D.  delta_pos > 0: population 1's 3'UTRs
# are longer.  boot_pa_usage_diff reports diff_pa's records and lines (two kept rows or more, reads in both populations,
# one line per kept row), one series per kept row:
#     d_i(b) = (double)a_i1(b) / (double)A_1(b) - (double)a_i2(b) / (double)A_2(b);  +infinity when either A is 0
# with pa_info, usage.1, usage.2 and delta_usage diff_pa's text (_usage_columns) and delta_usage_lo / _hi = repr of lo / hi.
# The interval fields are empty when D = 0.  A replicate's difference is three correctly rounded operations, not the exact
# rational rounded once as delta_pos and delta_usage are: the ends may differ from such a value in the last place, and
# they are the same bits as the difference of boot_pa_len's and boot_pa_usage's replicate values.
BOOT_PA_LEN_DIFF_HEADER = DIFF_PA_LEN_HEADER[:8] + ["delta_pos_lo", "delta_pos_hi"] + DIFF_PA_LEN_HEADER[8:11] + [
    "delta_exp_length_lo", "delta_exp_length_hi", "n_empty", "n_boot", "level"]
BOOT_PA_USAGE_DIFF_HEADER = ["gene", "pa_info", "versus", "num_pa", "reads.1", "reads.2", "gene_reads.1", "gene_reads.2",
                             "usage.1", "usage.2", "delta_usage", "delta_usage_lo", "delta_usage_hi", "n_empty", "n_boot",
                             "level"]


def _boot_pa_len_diff_lines(su, n_boot, out, recs, b):
    for g, r in enumerate(b.which.tolist()):
        sl = slice(int(b.off[g]), int(b.off[g + 1]))
        a1, a2 = b.a0[sl, 0], b.a0[sl, 1]
        m1, m2, d = _mean_positions(b.xs[g], a1.tolist(), a2.tolist())
        e1, e2 = float(b.exp_len[g][0]), float(b.exp_len[g][1])
        D = int(b.n_def[g, 0])
        ends = [math.ldexp(float(v), -b.scale[g]) for v in (b.lo[g, 0], b.hi[g, 0])] if D else []
        alpha = np.asarray(recs[r].alpha_arr, dtype=np.float64)
        width = float(alpha[-1]) - float(alpha[0])
        scaled = not (math.isnan(e1) or math.isnan(e2)) and math.isfinite(width) and width > 0
        out.append([recs[r].gene_info_str, su.versus, int(b.off[g + 1] - b.off[g]), int(a1.sum()), int(a2.sum()),
                    repr(m1), repr(m2), repr(d)] + ([repr(y) for y in ends] or ["", ""]) +
                   [repr(e1), repr(e2), repr(e1 - e2)] +
                   ([repr(9.0 * y / width) for y in ends] if scaled and D else ["", ""]) + [n_boot - D, n_boot, su.level])


def _boot_pa_usage_diff_lines(su, n_boot, out, recs, b):
    n_lines = np.diff(b.off)
    usage, rec_of, A, B = _usage_columns(b.t, np.ascontiguousarray(b.a0[:, 0]), n_lines)
    pa = [p for g, r in enumerate(b.which.tolist())
          for p in _pa_info(recs[r], b.rows[b.off[g]:b.off[g + 1]] - int(b.rowbase[r]))]
    for i, g in enumerate(rec_of.tolist()):
        D = int(b.n_def[i, 0])
        ends = [repr(float(b.lo[i, 0])), repr(float(b.hi[i, 0]))] if D else ["", ""]
        out.append([recs[b.which[g]].gene_info_str, pa[i], su.versus, int(n_lines[g]), int(b.a0[i, 0]), int(b.a0[i, 1]),
                    int(A[i]), int(B[i]), usage[0][i], usage[1][i], usage[2][i]] + ends + [n_boot - D, n_boot, su.level])
    su.n_records += len(b.which)


_BOOT_PA_LEN_DIFF = SimpleNamespace(header=BOOT_PA_LEN_DIFF_HEADER, call="report_boot_len_diff", positions=True,
                                    diff=True, lines=_boot_pa_len_diff_lines)
_BOOT_PA_USAGE_DIFF = SimpleNamespace(header=BOOT_PA_USAGE_DIFF_HEADER, call="report_boot_usage_diff", positions=False,
                                      diff=True, lines=_boot_pa_usage_diff_lines)


def _boot_pa_len_diff(output_dir: str, res_pkl_file: str, cell_cluster_file: str, idents_1: str, idents_2=None,
                      n_boot: int = 9999, level="95", seed: int = 1, device=None):
    """percentile bootstrap intervals of the difference of the mean pA position, and of exp_length, between the cells of
    cluster idents_1 and those of idents_2 (None: every other cell that has a cluster), by resampling the cells with
    boot_pa_len's replicates; writes <cluster file stem>.<gene|utr>.<A>_vs_<B|rest>.boot_pa_len_diff.csv in output_dir,
    one line per record diff_pa_len tests, and returns its path"""
    su = _boot_diff_setup(output_dir, res_pkl_file, cell_cluster_file, idents_1, idents_2, n_boot, level, seed,
                          "boot_pa_len_diff")
    out = _boot_run(_BOOT_PA_LEN_DIFF, su, n_boot, device)
    print(f"Finish {n_boot} bootstrap replicates of {su.sizes[0]} + {su.sizes[1]} cells for {len(out)} reported records")
    print(f"Finish {su.res_pkl} in {su.wall / 60} min.")
    return su.outpath


def _boot_pa_usage_diff(output_dir: str, res_pkl_file: str, cell_cluster_file: str, idents_1: str, idents_2=None,
                        n_boot: int = 9999, level="95", seed: int = 1, device=None):
    """percentile bootstrap intervals of the difference of the usage of every pA site between the cells of cluster
    idents_1 and those of idents_2 (None: every other cell that has a cluster), by resampling the cells with
    boot_pa_len's replicates; writes <cluster file stem>.<gene|utr>.<A>_vs_<B|rest>.boot_pa_usage_diff.csv in
    output_dir, one line per line of diff_pa, and returns its path"""
    su = _boot_diff_setup(output_dir, res_pkl_file, cell_cluster_file, idents_1, idents_2, n_boot, level, seed,
                          "boot_pa_usage_diff")
    out = _boot_run(_BOOT_PA_USAGE_DIFF, su, n_boot, device)
    print(f"Finish {n_boot} bootstrap replicates of {su.sizes[0]} + {su.sizes[1]} cells for {len(out)} pA sites of "
          f"{su.n_records} reported records")
    print(f"Finish {su.res_pkl} in {su.wall / 60} min.")
    return su.outpath


# ---------------------------------------------------------------- cal_exp_pa_len
def _exp_len_rows(K, alpha_arr, counts):
    """exp_pa_len (apa_core.py:1038-1052) for every row of counts [groups, K + 1] (slot K: reads with label >= K);
    row-wise numpy reductions run the same pairwise sums as the reference's 1-D np.sum"""
    out = np.zeros(counts.shape[0])
    if K == 1:
        out[:] = 1.0
        return out
    below = counts[:, :K]
    n_all = counts.sum(axis=1)
    n_below = below.sum(axis=1)
    live = (n_all > 0) & (n_below > 0)
    out[~live] = np.nan
    if np.any(live):
        ws = below[live].astype(np.float64)
        ws = ws / np.sum(ws, axis=1, keepdims=True)
        a_arr = alpha_arr
        with np.errstate(all="ignore"):
            n_arr = 1.0 + 9.0 * (a_arr - a_arr[0]) / (a_arr[-1] - a_arr[0])
            out[live] = np.sum(ws * n_arr, axis=1)
    return out


def _cal_exp_pa_len(output_dir: str, cell_cluster_file: str, res_pkl_file: str, device=None):
    import pandas as pd
    if not os.path.exists(os.path.join(output_dir, "pkl_output")):
        raise Exception("Please use the same directory that stores res pickle files by infer_pa")
    if not os.path.exists(os.path.join(output_dir, "pkl_input")):
        raise Exception("Please use the same directory that stores res pickle files by prepare_input")
    final_res = os.path.join(output_dir, res_pkl_file)
    if not (os.path.exists(final_res)):
        raise Exception("Must run apajunction before apaexppalen")
    if not (os.path.exists(os.path.join(output_dir, "barcode_index.csv"))):
        raise Exception("Please use the same output directory as in prepare_input and infer_pa")
    pd.read_csv(os.path.join(output_dir, "barcode_index.csv"), index_col="index")   # read (and checked) as the reference does
    if cell_cluster_file == "None":
        idmap, values = None, None
        output_path = os.path.join(output_dir, "all_cell." + res_pkl_file.replace(".pkl", ".pa.len.csv").replace("res.", ""))
    else:
        if not (os.path.exists(cell_cluster_file)):
            raise Exception("Given cell_cluster_file file does not exists")
        cluster_df = pd.read_csv(cell_cluster_file, index_col="index")
        prefix = os.path.splitext(os.path.basename(cell_cluster_file))[0]
        output_path = os.path.join(output_dir, prefix + "." + res_pkl_file.replace(".pkl", ".pa.len.csv").replace("res.", ""))
        col = cluster_df.iloc[:, 0]
        vals = col.tolist()                             # the Python objects cluster_dict holds (utils.py:387)
        codes, _uniq = pd.factorize(pd.Series(vals, dtype=object), use_na_sentinel=False)
        codes = np.asarray(codes, dtype=np.int32)
        first = np.unique(codes, return_index=True)[1]  # factorize numbers values by first appearance
        values = [vals[i] for i in first]               # one representative object per code
        idmap = _IdMap(col.index.to_numpy(), codes, cell_cluster_file)

    exp_len_lst = []
    with _Run(device, [output_path]) as run:
        n_codes = len(values) if values is not None else 1
        n_words = (max(n_codes, 1) + 31) // 32

        def cost(p):
            n = len(p.label_arr)
            return n * 16 + n_words * 8 + min(n, n_codes) * (int(p.K) + 1) * 4 + 64

        ctx = run.device()
        for recs in _batches(final_res, cost, _budget(ctx), run.times):
            _hist_batch(ctx, recs, idmap, values, n_codes, exp_len_lst, run.times, cell_cluster_file)
        run.release()
        print(f"Done calculating expected pa length each gene in {(timer() - run.start) / 60} min.")
        t0 = timer()
        if cell_cluster_file == "None":
            final_df = pd.DataFrame(exp_len_lst, columns=["gene_id", "exp_length", "num_pa"])
        else:
            final_df = pd.DataFrame(exp_len_lst, columns=["gene_id", "cell_cluster", "exp_length", "num_pa"])
        final_df.to_csv(run.parts[0], header=True, index=False)
        run.times["finish"] += timer() - t0
    print(f"Done in {run.total / 60} min. ")
    return output_path


def _hist_batch(ctx, recs, idmap, values, n_codes, exp_len_lst, times, cell_cluster_file):
    t0 = timer()
    off, K, lab, cb = _record_arrays(recs)
    n_groups = np.zeros(len(recs), dtype=np.int64)
    bad = np.zeros(2, dtype=np.int64)
    lib = ctx.lib
    table = ptr(idmap.table, P_i32) if idmap is not None else None
    check(lib.scape_hip_report_hist(ctx.h, len(recs), ptr(off, P_i64), ptr(K, P_i32), ptr(lab, P_i64), ptr(cb, P_i64),
                                    idmap.id_min if idmap else 0, idmap.span if idmap else 0, table, n_codes,
                                    ptr(n_groups, P_i64), ptr(bad, P_i64)), "report_hist")
    if bad[0] >= 0 or bad[1] >= 0:
        _raise_bad_read(bad, recs, off, cb, cell_cluster_file)
    n_hist = int(np.sum(n_groups * (K.astype(np.int64) + 1)))
    codes = np.zeros(max(int(n_groups.sum()), 1), dtype=np.int32)
    hist = np.zeros(max(n_hist, 1), dtype=np.int32)
    check(lib.scape_hip_report_hist_fetch(ctx.h, int(n_groups.sum()), ptr(codes, P_i32), n_hist, ptr(hist, P_i32)),
          "report_hist_fetch")
    times["h2d_counts"] += timer() - t0
    t0 = timer()
    g0 = h0 = 0
    for r, para in enumerate(recs):
        chrom, gene_id, utr_id, st_en, strand = para.gene_info_str.split(":")
        k, g = int(K[r]), int(n_groups[r])
        cnt = hist[h0:h0 + g * (k + 1)].reshape(g, k + 1).astype(np.int64)
        alpha = para.alpha_arr
        if values is None:
            exp_len = _exp_len_rows(k, alpha, cnt.sum(axis=0, keepdims=True))[0] if g else \
                (1.0 if para.K == 1 else np.nan)
            exp_len_lst.append([gene_id + ":" + utr_id, exp_len, para.K])
        elif g:
            # the partition of the record holds exactly these values: np.array of them has the dtype the reference's
            # per-read np.array gets, and np.unique orders / merges them the same way (apa_core.py:1056-1057)
            part = np.array([values[c] for c in codes[g0:g0 + g].tolist()])
            uni_clusters = np.unique(part)
            grp = np.zeros((len(uni_clusters), k + 1), dtype=np.int64)
            for i, c in enumerate(uni_clusters):
                m = part == c
                if np.any(m):
                    grp[i] = cnt[m].sum(axis=0)
            avg_len_arr = np.zeros(len(uni_clusters))
            avg_len_arr[:] = _exp_len_rows(k, alpha, grp)
            for idx in range(len(uni_clusters)):
                exp_len_lst.append([gene_id + ":" + utr_id, uni_clusters[idx], avg_len_arr[idx], para.K])
        g0 += g
        h0 += g * (k + 1)
    times["finish"] += timer() - t0


# ---------------------------------------------------------------- commands (reference utils.py:323-342, :442-454)
@click.command(name="cal_exp_pa_len")
@click.option('--output_dir', type=str, required=True,
              help='Directory which was used in previous steps to save output by prepare_input and infer_pa')
@click.option('--cell_cluster_file', type=str, default="None",
              help='An csv file containing two columns in order: cell barcode (CB) and respective group '
                   '(cell_cluster_file). Its name will be included in the file name of final result.')
@click.option('--res_pkl_file', type=str, default="None",
              help='Name of res pickle file that contains PASs for calculating expected PA length. Its name will be '
                   'included in the file name of final result.')
def cal_exp_pa_len(output_dir: str, cell_cluster_file: str, res_pkl_file: str):
    """Expected pA length per gene (and per cell cluster) from res.gene.pkl / res.utr.pkl (reference utils.py:319-427)."""
    _cal_exp_pa_len(output_dir, cell_cluster_file, res_pkl_file)


@click.command(name="ex_pa_cnt_mat")
@click.option('--output_dir', type=str, required=True,
              help='Directory which was used in previous steps to save output by prepare_input and infer_pa.')
@click.option('--res_pkl_file', type=str, default="None",
              help='Name of res pickle file that contains PASs for calculating expected PA length. Its name will be '
                   'included in the file name of final result.')
@click.option('--format', 'fmt', type=click.Choice(["tsv", "mtx"]), default="tsv", show_default=True,
              help='tsv: the dense matrix <res name>.cnt.tsv.gz. mtx: the directory <res name>.cnt/ with '
                   'matrix.mtx.gz, features.tsv.gz and barcodes.tsv.gz (sparse Matrix Market, as read by Seurat '
                   'Read10X and scanpy read_10x_mtx).')
def ex_pa_cnt_mat(output_dir: str, res_pkl_file: str, fmt: str):
    """pA x cell read-count matrix <res name>.cnt.tsv.gz from res.gene.pkl / res.utr.pkl (reference utils.py:438-553)."""
    _ex_pa_cnt_mat(output_dir, res_pkl_file, fmt=fmt)


@click.command(name="ex_pa_len_mat")
@click.option('--output_dir', type=str, required=True,
              help='Directory which was used in previous steps to save output by prepare_input and infer_pa.')
@click.option('--res_pkl_file', type=str, default="None",
              help='Name of res pickle file that contains PASs. Its name will be included in the name of the final '
                   'result.')
def ex_pa_len_mat(output_dir: str, res_pkl_file: str):
    """Gene x cell matrix of the expected pA length, the quantity cal_exp_pa_len reports per cluster, from res.gene.pkl /
    res.utr.pkl: the directory <res name>.len/ with matrix.mtx.gz, reads.mtx.gz (the reads behind each value),
    features.tsv.gz and barcodes.tsv.gz (sparse Matrix Market, as read by Seurat Read10X and scanpy read_10x_mtx)."""
    _ex_pa_len_mat(output_dir, res_pkl_file)


@click.command(name="ex_pa_usage_mat")
@click.option('--output_dir', type=str, required=True,
              help='Directory which was used in previous steps to save output by prepare_input and infer_pa.')
@click.option('--res_pkl_file', type=str, default="None",
              help='Name of res pickle file that contains PASs. Its name will be included in the name of the final '
                   'result.')
@click.option('--min_reads', type=click.IntRange(1, USAGE_MAX_MIN_READS), default=1, show_default=True,
              help='A cell has a usage in a gene (or UTR) record only with at least this many reads of the '
                   'record\'s pA sites; above 1 the directory is named <res name>.min<N>.usage/.')
def ex_pa_usage_mat(output_dir: str, res_pkl_file: str, min_reads: int):
    """pA site x cell matrix of the per-cell site usage (PSI: the site's reads in a cell over the cell's reads of the
    whole gene or UTR record) from res.gene.pkl / res.utr.pkl: the directory <res name>.usage/ with matrix.mtx.gz,
    reads.mtx.gz (the cell's reads of the record wherever the usage is defined, an observed 0 included), features.tsv.gz
    and barcodes.tsv.gz (those of ex_pa_cnt_mat --format mtx; sparse Matrix Market, as read by Seurat Read10X and scanpy
    read_10x_mtx)."""
    _ex_pa_usage_mat(output_dir, res_pkl_file, min_reads)


@click.command(name="ex_pa_pseudobulk")
@click.option('--output_dir', type=str, required=True,
              help='Directory which was used in previous steps to save output by prepare_input and infer_pa.')
@click.option('--res_pkl_file', type=str, default="None",
              help='Name of res pickle file that contains PASs. Its name will be included in the file names of the '
                   'final result.')
@click.option('--cell_cluster_file', type=str, required=True,
              help='An csv file containing two columns in order: cell barcode index (index) and respective group. '
                   'Cells with an empty group, or not listed, are left out. Its name will be included in the file '
                   'names of the final result.')
@click.option('--num_splits', type=int, default=6, show_default=True,
              help='Pseudo-replicates per population: its cells, in barcode_index.csv order, are cut into this many '
                   'consecutive chunks (num.splits of FindDE in DifferentialTest.R).')
@click.option('--idents_1', type=str, default=None,
              help='Compare this cluster (Population1) with --idents_2, or with every other cluster. Default: one '
                   'population per cluster.')
@click.option('--idents_2', type=str, default=None, help='The cluster of Population2 (needs --idents_1).')
def ex_pa_pseudobulk(output_dir: str, res_pkl_file: str, cell_cluster_file: str, num_splits: int, idents_1, idents_2):
    """pA x pseudo-replicate read counts (the input of DEXSeq) and the share of each population's cells with a read
    per pA site, from res.gene.pkl / res.utr.pkl and a cell cluster file (reference DifferentialTest.R:63-104, :159-184)."""
    _ex_pa_pseudobulk(output_dir, res_pkl_file, cell_cluster_file, num_splits, idents_1, idents_2)


# the options every command below starts with, and the cluster file of those that take one
_OUTPUT_OPTIONS = (
    click.option('--output_dir', type=str, required=True,
                 help='Directory which was used in previous steps to save output by prepare_input and infer_pa.'),
    click.option('--res_pkl_file', type=str, default="None",
                 help='Name of res pickle file that contains PASs. Its name will be included in the file name of the '
                      'final result.'))
_CLUSTER_FILE_OPTION = click.option(
    '--cell_cluster_file', type=str, required=True,
    help='An csv file containing two columns in order: cell barcode index (index) and respective group. Cells with an '
         'empty group, or not listed, are left out. Its name will be included in the file name of the final result.')


def _options(*options):
    """a decorator that adds the options, in their order"""
    def decorate(f):
        for option in reversed(options):
            f = option(f)
        return f
    return decorate


# the two populations of diff_pa, diff_pa_len, boot_pa_len_diff and boot_pa_usage_diff
_TWO_IDENTS_OPTIONS = (
    click.option('--idents_1', type=str, required=True, help='The cluster of population 1.'),
    click.option('--idents_2', type=str, default=None,
                 help='The cluster of population 2. Default: every other cell that has a cluster.'))
# diff_pa and diff_pa_len (--seed's help differs)
_perm_options = _options(
    *_OUTPUT_OPTIONS, _CLUSTER_FILE_OPTION, *_TWO_IDENTS_OPTIONS,
    click.option('--n_perm', type=int, default=9999, show_default=True,
                 help='Permutations of the cell labels; the smallest p-value is 1 / (1 + n_perm).'),
    click.option('--strata_file', type=str, default=None,
                 help='A csv file like the cell_cluster_file, naming a stratum (cell type, donor, batch, ...) per cell: '
                      'the labels are then permuted within each stratum only. Cells with an empty stratum, or not '
                      'listed, are left out. Its name will be included in the file name of the final result.'))


def _idents_options(idents_help):
    """diff_pa_groups, diff_pa_len_groups, diff_pa_pairs, diff_pa_markers, diff_pa_len_pairs and diff_pa_len_markers (the
    help of --n_perm and --seed differs, and the two markers commands have their own for --idents)"""
    return _options(*_OUTPUT_OPTIONS, _CLUSTER_FILE_OPTION,
                    click.option('--idents', type=str, multiple=True, help=idents_help))


_groups_options = _idents_options('A cluster to test; give the option once per cluster (2 to 64), the order is kept. '
                                  'Default: every cluster of the cell_cluster_file, in order of first appearance.')
_markers_options = _idents_options(
    'A cluster to test against all other cells that have a cluster, whether named or not; give the option once per '
    'cluster (1 to 64), the order is kept. Default: every cluster of the cell_cluster_file (at most 64), in order of '
    'first appearance.')
# diff_pa_trend and diff_pa_len_trend
_trend_options = _options(
    *_OUTPUT_OPTIONS,
    click.option('--cell_score_file', type=str, required=True,
                 help='An csv file containing two columns in order: cell barcode index (index) and the score of the cell '
                      '(pseudotime, a differentiation, cell-cycle or activation score). Cells with an empty score, NA or '
                      'nan, or not listed, are left out. Its name will be included in the file name of the final '
                      'result.'),
    click.option('--rank', is_flag=True, default=False,
                 help='Test along the ranks of the scores (ties share their mid-rank), not the scores themselves.'),
    click.option('--n_perm', type=int, default=9999, show_default=True,
                 help='Permutations of the cell scores; the smallest p-value is 1 / (1 + n_perm).'),
    click.option('--seed', type=int, default=1, show_default=True,
                 help='Seed of the permutations, 0 .. 2^64 - 1 (the keys are those of diff_pa).'))


@click.command(name="diff_pa")
@_perm_options
@click.option('--seed', type=int, default=1, show_default=True, help='Seed of the permutations, 0 .. 2^64 - 1.')
def diff_pa(output_dir: str, res_pkl_file: str, cell_cluster_file: str, idents_1: str, idents_2, n_perm: int,
            strata_file, seed: int):
    """pA sites used differently by two cell populations: a permutation test of the cell labels on the pA x cell counts
    of res.gene.pkl / res.utr.pkl (the question of the reference's FindDE, DifferentialTest.R:159-196, without DEXSeq)."""
    _diff_pa(output_dir, res_pkl_file, cell_cluster_file, idents_1, idents_2, n_perm, seed, strata_file=strata_file)


@click.command(name="diff_pa_len")
@_perm_options
@click.option('--seed', type=int, default=1, show_default=True,
              help='Seed of the permutations, 0 .. 2^64 - 1. The same seed gives the same relabellings of the cells '
                   'as in diff_pa.')
def diff_pa_len(output_dir: str, res_pkl_file: str, cell_cluster_file: str, idents_1: str, idents_2, n_perm: int,
                strata_file, seed: int):
    """3'UTR lengthening or shortening between two cell populations: per gene, a two-sided permutation test of the cell
    labels on the difference of the mean pA position (delta_pos > 0: population 1 uses longer 3'UTRs), with the
    reference's expected pA length (cal_exp_pa_len's 1..10 scale) of both populations beside it."""
    _diff_pa_len(output_dir, res_pkl_file, cell_cluster_file, idents_1, idents_2, n_perm, seed, strata_file=strata_file)


@click.command(name="diff_pa_groups")
@_groups_options
@click.option('--n_perm', type=int, default=9999, show_default=True,
              help='Permutations of the cell labels; the smallest p-value is 1 / (1 + n_perm).')
@click.option('--seed', type=int, default=1, show_default=True,
              help='Seed of the permutations, 0 .. 2^64 - 1 (the keys are those of diff_pa).')
def diff_pa_groups(output_dir: str, res_pkl_file: str, cell_cluster_file: str, idents, n_perm: int, seed: int):
    """pA sites and genes whose pA usage differs across the cell populations of a cluster file at all: the omnibus
    form of diff_pa, a permutation test of the cell labels on Pearson's chi-square of the sites x populations table."""
    _diff_pa_groups(output_dir, res_pkl_file, cell_cluster_file, idents, n_perm, seed)


@click.command(name="diff_pa_len_groups")
@_groups_options
@click.option('--n_perm', type=int, default=9999, show_default=True,
              help='Permutations of the cell labels; the smallest p-value is 1 / (1 + n_perm).')
@click.option('--seed', type=int, default=1, show_default=True,
              help='Seed of the permutations, 0 .. 2^64 - 1. The same seed gives the same relabellings of the cells '
                   'as in diff_pa_groups.')
def diff_pa_len_groups(output_dir: str, res_pkl_file: str, cell_cluster_file: str, idents, n_perm: int, seed: int):
    """Genes whose 3'UTR length differs across the cell populations of a cluster file at all, and the populations with
    longer or shorter 3'UTRs than all the others: the omnibus form of diff_pa_len, a permutation test of the cell labels
    on the between-population sum of squares of the mean pA position, and on every population's mean against the rest."""
    _diff_pa_len_groups(output_dir, res_pkl_file, cell_cluster_file, idents, n_perm, seed)


@click.command(name="diff_pa_pairs")
@_groups_options
@click.option('--n_perm', type=int, default=9999, show_default=True,
              help='Permutations of the cell labels per pair; the smallest p-value is 1 / (1 + n_perm).')
@click.option('--seed', type=int, default=1, show_default=True,
              help='Seed of the permutations, 0 .. 2^64 - 1. The same seed gives every pair the relabellings of diff_pa '
                   'on its two clusters.')
def diff_pa_pairs(output_dir: str, res_pkl_file: str, cell_cluster_file: str, idents, n_perm: int, seed: int):
    """Every pair of the cell populations of a cluster file tested as diff_pa tests two, in one run over the result
    file: the post-hoc tests behind diff_pa_groups, with the p-values adjusted over all pairs (Benjamini-Hochberg)."""
    _diff_pa_pairs(output_dir, res_pkl_file, cell_cluster_file, idents, n_perm, seed)


@click.command(name="diff_pa_markers")
@_markers_options
@click.option('--n_perm', type=int, default=9999, show_default=True,
              help='Permutations of the cell labels per marker; the smallest p-value is 1 / (1 + n_perm).')
@click.option('--seed', type=int, default=1, show_default=True,
              help='Seed of the permutations, 0 .. 2^64 - 1. The same seed gives every marker the relabellings of '
                   'diff_pa on that cluster against the rest.')
def diff_pa_markers(output_dir: str, res_pkl_file: str, cell_cluster_file: str, idents, n_perm: int, seed: int):
    """Every cell population of a cluster file (or each of the 1 to 64 named with --idents) tested against all other
    cells that have a cluster, as diff_pa tests one cluster against the rest, in one run over the result file: the
    markers of every cluster, with the p-values adjusted over all of them (Benjamini-Hochberg)."""
    _diff_pa_markers(output_dir, res_pkl_file, cell_cluster_file, idents, n_perm, seed)


@click.command(name="diff_pa_len_pairs")
@_groups_options
@click.option('--n_perm', type=int, default=9999, show_default=True,
              help='Permutations of the cell labels per pair; the smallest p-value is 1 / (1 + n_perm).')
@click.option('--seed', type=int, default=1, show_default=True,
              help='Seed of the permutations, 0 .. 2^64 - 1. The same seed gives every pair the relabellings of '
                   'diff_pa_len on its two clusters.')
def diff_pa_len_pairs(output_dir: str, res_pkl_file: str, cell_cluster_file: str, idents, n_perm: int, seed: int):
    """Every pair of the cell populations of a cluster file tested as diff_pa_len tests two, in one run over the result
    file: the post-hoc tests behind diff_pa_len_groups, with the p-values adjusted over all pairs (Benjamini-Hochberg)."""
    _diff_pa_len_pairs(output_dir, res_pkl_file, cell_cluster_file, idents, n_perm, seed)


@click.command(name="diff_pa_len_markers")
@_markers_options
@click.option('--n_perm', type=int, default=9999, show_default=True,
              help='Permutations of the cell labels per marker; the smallest p-value is 1 / (1 + n_perm).')
@click.option('--seed', type=int, default=1, show_default=True,
              help='Seed of the permutations, 0 .. 2^64 - 1. The same seed gives every marker the relabellings of '
                   'diff_pa_len on that cluster against the rest.')
def diff_pa_len_markers(output_dir: str, res_pkl_file: str, cell_cluster_file: str, idents, n_perm: int, seed: int):
    """Every cell population of a cluster file (or each of the 1 to 64 named with --idents) tested against all other
    cells that have a cluster, as diff_pa_len tests one cluster against the rest, in one run over the result file: the
    clusters with longer or shorter 3'UTRs than the rest, with the p-values adjusted over all of them
    (Benjamini-Hochberg)."""
    _diff_pa_len_markers(output_dir, res_pkl_file, cell_cluster_file, idents, n_perm, seed)


@click.command(name="diff_pa_trend")
@_trend_options
def diff_pa_trend(output_dir: str, res_pkl_file: str, cell_score_file: str, rank: bool, n_perm: int, seed: int):
    """pA sites and genes whose pA usage shifts along a per-cell score such as pseudotime: a permutation test of the
    cell scores on the mean score of every site's reads against the gene's other reads, and on the between-site sum of
    squares of the score (delta_score > 0: the site is used by cells further along)."""
    _diff_pa_trend(output_dir, res_pkl_file, cell_score_file, rank, n_perm, seed)


@click.command(name="diff_pa_len_trend")
@_trend_options
def diff_pa_len_trend(output_dir: str, res_pkl_file: str, cell_score_file: str, rank: bool, n_perm: int, seed: int):
    """Genes whose 3'UTRs lengthen or shorten along a per-cell score such as pseudotime: an exact permutation test of
    the cell scores on the covariance of the pA position and the score over the gene's reads, the score's permutations
    those of diff_pa_trend (delta_pos > 0: longer 3'UTRs in cells further along)."""
    _diff_pa_len_trend(output_dir, res_pkl_file, cell_score_file, rank, n_perm, seed)


# the replicates and the level of the four bootstrap commands
_BOOT_REPLICATE_OPTIONS = (
    click.option('--n_boot', type=int, default=9999, show_default=True,
                 help='Bootstrap replicates of the cells.'),
    click.option('--level', type=str, default="95", show_default=True,
                 help='Level of the percentile intervals in percent, above 0 and below 100, with at most two '
                      'decimals.'))
# boot_pa_len and boot_pa_usage
_boot_options = _options(
    *_OUTPUT_OPTIONS,
    click.option('--cell_cluster_file', type=str, default=None,
                 help='An csv file containing two columns in order: cell barcode index (index) and respective group. '
                      'Cells with an empty group, or not listed, are left out. Its name will be included in the file '
                      'name of the final result. Default: one population, all_cell, of every cell.'),
    click.option('--idents', type=str, multiple=True,
                 help='A cluster to report; give the option once per cluster (1 to 64), the order is kept. Needs '
                      '--cell_cluster_file. Default: every cluster of the cell_cluster_file (at most 64), in order '
                      'of first appearance.'),
    *_BOOT_REPLICATE_OPTIONS,
    click.option('--seed', type=int, default=1, show_default=True,
                 help='Seed of the replicates, 0 .. 2^64 - 1. The same seed resamples the same cells whatever the '
                      'cluster file and the idents.'))


# boot_pa_len_diff and boot_pa_usage_diff: diff_pa's populations, the bootstrap's other options
_boot_diff_options = _options(
    *_OUTPUT_OPTIONS, _CLUSTER_FILE_OPTION, *_TWO_IDENTS_OPTIONS, *_BOOT_REPLICATE_OPTIONS,
    click.option('--seed', type=int, default=1, show_default=True,
                 help='Seed of the replicates, 0 .. 2^64 - 1. The same seed resamples the same cells as in boot_pa_len '
                      'and boot_pa_usage.'))


@click.command(name="boot_pa_len")
@_boot_options
def boot_pa_len(output_dir: str, res_pkl_file: str, cell_cluster_file, idents, n_boot: int, level: str, seed: int):
    """How well a cluster's 3'UTR length is known: per gene and cell population, percentile bootstrap intervals of the
    mean pA position and of the reference's expected pA length (cal_exp_pa_len's 1..10 scale), by resampling the cells
    (the Poisson bootstrap, in exact integers on the device)."""
    if idents and cell_cluster_file is None:
        raise click.UsageError("--idents needs --cell_cluster_file")
    _boot_pa_len(output_dir, res_pkl_file, cell_cluster_file, idents, n_boot, level, seed)


@click.command(name="boot_pa_usage")
@_boot_options
def boot_pa_usage(output_dir: str, res_pkl_file: str, cell_cluster_file, idents, n_boot: int, level: str, seed: int):
    """How well a cluster's usage of a pA site is known: per gene, pA site and cell population, the site's share of the
    population's reads of the gene (diff_pa's usage) with a percentile bootstrap interval, by resampling the cells (the
    replicates of boot_pa_len, in exact integers on the device)."""
    if idents and cell_cluster_file is None:
        raise click.UsageError("--idents needs --cell_cluster_file")
    _boot_pa_usage(output_dir, res_pkl_file, cell_cluster_file, idents, n_boot, level, seed)


@click.command(name="boot_pa_len_diff")
@_boot_diff_options
def boot_pa_len_diff(output_dir: str, res_pkl_file: str, cell_cluster_file: str, idents_1: str, idents_2, n_boot: int,
                     level: str, seed: int):
    """How much longer one population's 3'UTRs are than the other's, and how well that is known: per gene diff_pa_len
    tests, the difference of the mean pA position and of the expected pA length (population 1 minus population 2) with
    a percentile bootstrap interval, by resampling the cells (the replicates of boot_pa_len)."""
    _boot_pa_len_diff(output_dir, res_pkl_file, cell_cluster_file, idents_1, idents_2, n_boot, level, seed)


@click.command(name="boot_pa_usage_diff")
@_boot_diff_options
def boot_pa_usage_diff(output_dir: str, res_pkl_file: str, cell_cluster_file: str, idents_1: str, idents_2, n_boot: int,
                       level: str, seed: int):
    """How much more one population uses a pA site than the other, and how well that is known: per pA site diff_pa
    tests, delta_usage (population 1 minus population 2) with a percentile bootstrap interval, by resampling the cells
    (the replicates of boot_pa_len)."""
    _boot_pa_usage_diff(output_dir, res_pkl_file, cell_cluster_file, idents_1, idents_2, n_boot, level, seed)
