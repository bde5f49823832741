"""The boundary ladder of the report side's oldest device layer (scape_amd/csrc/report.inc: k_rep_count,
k_rep_complete, k_rep_rowlen, k_rep_scan, k_rep_render, k_rep_segsum, k_rep_present, k_rep_groups, k_rep_hist and the
block helpers rep_block_sum / rep_block_excl; scape_amd/csrc/report_mtx.inc: k_rep_entries_rowlen / k_rep_entries_render
under the count rule): the cases and the exact oracle.  Nothing
here imports from scape_amd (the rule of tests/report_cases.py); tests/test_report_ladder.py runs the cases,
tests/test_host.py checks the ladder against the constants of the source.

The oracle restates the outputs in Python ints, str and bytes; nothing is floating point, no tolerance exists:
  dense row       the prefix bytes, one field per column, "\\n"; a field is ,"0.0" for a zero count, ,"<v>" for a count
                  of a pivot-complete record and ,"<v>.0" otherwise (reference utils.py:438-553 as the goldens record it:
                  pandas keeps a pivot without a hole int64 and prints "2", one with a hole float64 and "2.0")
  pivot-complete  every column that has a read (label < K) in the record has a read in every row of the record that has
                  any read
  row totals      plain sums
  Matrix Market   "<row> <col + 1> <count>\\n" for the nonzero counts of a row, ascending by column
  segment sums    per row and segment the sum and the number of nonzero counts
  histogram       per record the codes present, ascending, and per (code, min(label, K)) the number of reads; reads with
                  label >= K count towards presence and towards slot K

A case states its dense matrix; each count becomes that many reads, shuffled, so the input pins the matrix and the
matrix does not depend on a generator (the bad-read search below is the one place that looks at the read arrays, with
exact integer comparisons).  Every shape is the smallest that can still go wrong; a case's `note` says which boundary
it sits on.  Counts of 8 to 10 digits are NOT reached: they need 10^7 reads or more in one cell."""
import functools

import numpy as np

THREADS = 256          # REP_THREADS: the column tile of the three render kernels, the word tile of k_rep_groups
SCAN = 1024            # REP_SCAN_THREADS: the one workgroup of k_rep_scan
WAVE = 64              # the wavefront rep_block_sum / rep_block_excl hard-code
ZERO_FIELD = 6         # REP_ZERO_FIELD: len(',"0.0"')

COLS = (1, 63, 64, 65, 255, 256, 257, 511, 512, 513)
ROWS = (1, 1023, 1024, 1025, 2048, 2049)
CODES = (1, 31, 32, 33, 64, 8191, 8192, 8193)
WIDTH_COUNTS = (9, 10, 99, 100, 999, 1000, 9999, 10000, 99999, 100000, 999999, 1000000)
WIDTH_COLS = {0: 10, 2: 9, 62: 99, 63: 100, 64: 1000, 65: 999, 130: 99999, 200: 999999, 254: 9999, 255: 10000,
              256: 100000, 257: 1000000}
PREFIX_CYCLE = (0, 1, 7, 40)
PREFIX_LENGTHS = (0, 1, 255, 256, 257, 600)
RECORD_KS = (1, 63, 64, 70)
SEG_LENGTHS = {1: (300,), 3: (0, 63, 1), 4: (64, 65, 0, 300), 5: (1, 0, 300, 64, 63), 9: (0, 1, 63, 64, 65, 300, 0, 1, 64)}
SEG_FIRST, SEG_COLS = 5, 570
ROW_NO0 = (1, 9, 10, 99999)


# ---------------------------------------------------------------- the oracle
def field(v, is_int):
    if v == 0:
        return ',"0.0"'
    return f',"{v}"' if is_int else f',"{v}.0"'


def dense_row(prefix, counts, is_int):
    """bytes of one dense row: prefix (bytes), counts (Python ints), the record's form"""
    texts = {v: field(v, is_int) for v in set(counts)}
    return prefix + "".join([texts[v] for v in counts]).encode() + b"\n"


def complete(rows):
    """pivot-complete flag of a record given as its K rows of counts"""
    live = [r for r in rows if any(r)]
    for col in zip(*live):
        n = sum(1 for v in col if v)
        if n and n != len(live):
            return False
    return True


def row_total(counts):
    return sum(counts)


def mtx_row(row_no, counts):
    return "".join([f"{row_no} {c + 1} {v}\n" for c, v in enumerate(counts) if v]).encode()


def seg_sums(counts, seg_off):
    """([sum], [nonzero counts]) per segment [seg_off[s], seg_off[s + 1]) of one row"""
    parts = [counts[a:b] for a, b in zip(seg_off[:-1], seg_off[1:])]
    return [sum(p) for p in parts], [sum(1 for v in p if v) for p in parts]


def histogram(K, labels, codes):
    """(codes present, ascending; per present code its K + 1 slots) of one record's reads"""
    present = sorted(set(codes))
    at = {c: g for g, c in enumerate(present)}
    hist = [[0] * (K + 1) for _ in present]
    for lab, c in zip(labels, codes):
        hist[at[c]][min(lab, K)] += 1
    return present, hist


def prefix_bytes(i, n):
    """n bytes that differ from position to position and from row to row (every byte value occurs, 0 and "\\n" too)"""
    return bytes((i * 37 + k * 11 + 1) % 256 for k in range(n))


# ---------------------------------------------------------------- the cases of the count and render kernels
class Case:
    """mats: the records' [K, n_cols] count matrices; ids: the cell id of every column (None: the column itself);
    n_over: reads with a label >= K per record, in known cells; raw: per record further (label, cell id) reads, which
    may name unknown cells or carry negative labels and add to no count; rows / pre_len: the count rows a render block
    names and the length of each one's prefix; segs: the seg_off lists of family g"""

    def __init__(self, name, family, note, mats, ids=None, n_over=None, raw=None, rows=None, pre_len=None, segs=(),
                 want_complete=None, seed=0):
        self.name, self.family, self.note, self.seed = name, family, note, seed
        self.mats = [np.asarray(m, dtype=np.int64) for m in mats]
        self.n_cols = self.mats[0].shape[1]
        self.Ks = [m.shape[0] for m in self.mats]
        self.ids = np.arange(self.n_cols, dtype=np.int64) if ids is None else np.asarray(ids, dtype=np.int64)
        self.n_over = list(n_over) if n_over is not None else [0] * len(mats)
        self.raw = raw if raw is not None else [[] for _ in mats]
        self.counts = [r for m in self.mats for r in m.tolist()]          # every count row, Python ints
        self.rows = list(range(len(self.counts))) if rows is None else [int(i) for i in rows]
        cyc = [PREFIX_CYCLE[i % len(PREFIX_CYCLE)] for i in range(len(self.rows))]
        self.pre_len = cyc if pre_len is None else list(pre_len)
        self.segs, self.want_complete = list(segs), want_complete
        assert len(self.pre_len) == len(self.rows) and len(set(self.ids.tolist())) == self.n_cols

    # ---- what the device is given
    @functools.cached_property
    def reads(self):
        """(K int32, read offsets, labels, cell ids int64; id_min, the id table int32 with -1 in its gaps)"""
        rng = np.random.default_rng(self.seed)
        lab, cb, off = [], [], [0]
        for m, over, raw in zip(self.mats, self.n_over, self.raw):
            K = m.shape[0]
            l, c = np.nonzero(m)
            rep = m[l, c]
            l, c = np.repeat(l, rep), np.repeat(c, rep)
            l = np.concatenate([l, rng.integers(K, K + 3, over), np.array([x for x, _i in raw], dtype=np.int64)])
            i = np.concatenate([self.ids[c], self.ids[rng.integers(0, self.n_cols, over)],
                                np.array([x for _l, x in raw], dtype=np.int64)])
            mixo = rng.permutation(len(l))
            lab.append(l[mixo])
            cb.append(i[mixo])
            off.append(off[-1] + len(l))
        id_min = int(self.ids.min())
        table = np.full(int(self.ids.max()) - id_min + 1, -1, dtype=np.int32)
        table[self.ids - id_min] = np.arange(self.n_cols, dtype=np.int32)
        return (np.array(self.Ks, dtype=np.int32), np.array(off, dtype=np.int64),
                np.concatenate(lab).astype(np.int64), np.concatenate(cb).astype(np.int64), id_min, table)

    # ---- what the oracle expects
    @functools.cached_property
    def row_tot(self):
        return [row_total(r) for r in self.counts]

    @functools.cached_property
    def complete(self):
        out, at = [], 0
        for K in self.Ks:
            out.append(int(complete(self.counts[at:at + K])))
            at += K
        return out

    @functools.cached_property
    def bad(self):
        """[first read (label < K) of an unknown cell, first read with a negative label], -1 for none"""
        K, off, lab, cb, _id_min, _table = self.reads
        k_of = np.repeat(K.astype(np.int64), np.diff(off))
        known = np.isin(cb, self.ids)
        first = lambda m: int(np.nonzero(m)[0][0]) if m.any() else -1
        return [first((lab >= 0) & (lab < k_of) & ~known), first(lab < 0)]

    def prefixes(self):
        return [prefix_bytes(i, n) for i, n in enumerate(self.pre_len)]

    def dense_text(self, is_int, a=0, b=None):
        """the bytes of the block's rows [a, b) with the per-row forms is_int"""
        pre = self.prefixes()
        return b"".join(dense_row(pre[i], self.counts[self.rows[i]], is_int[i]) for i in range(a, len(self.rows) if b is None else b))

    def mtx_text(self, row_no0):
        """(bytes, entries) of the block as Matrix Market entries, the first row numbered row_no0"""
        text = b"".join(mtx_row(row_no0 + i, self.counts[r]) for i, r in enumerate(self.rows))
        return text, sum(1 for r in self.rows for v in self.counts[r] if v)


def _sparse(rng, K, n_cols, density=0.4, hi=30):
    return ((rng.random((K, n_cols)) < density) * rng.integers(1, hi, (K, n_cols))).astype(np.int64)


def _scrambled_ids(rng, n, first=17, step=3):
    """distinct ids above 0 in a scrambled order, with gaps between them"""
    return rng.permutation(first + step * np.arange(n)).astype(np.int64)


def _column_cases():
    out = []
    for n_cols in COLS:
        rng = np.random.default_rng(1000 + n_cols)
        mats = [_sparse(rng, K, n_cols) for K in (1, 3, 5)]
        for j, c in enumerate(sorted({c for c in (0, 63, 64, 255, 256, n_cols - 1) if c < n_cols})):
            mats[1 + j % 2][j % 3, c] = 10 + j                # the edge columns are nonzero in at least one row
        mats[2][4, :] = 0
        mats[2][4, n_cols - 1] = 7                            # a row that is all zero except the last column
        out.append(Case(f"cols{n_cols}", "a", f"{n_cols} columns: the 256-column tile loop and the 64-lane scan of "
                        "rep_block_excl, one short of an edge, on it and one over", mats, seed=n_cols))
    return out


def _width_case():
    """One record, K = 2, 258 columns; about 2.2 M reads.  Counts of 8 to 10 digits are not reached."""
    m = np.zeros((2, 258), dtype=np.int64)
    for c, v in WIDTH_COLS.items():
        m[0, c] = v
    rng = np.random.default_rng(7)
    m[1] = (rng.random(258) < 0.4) * rng.integers(1, 10, 258)
    return Case("widths", "b", "counts of 1 to 7 digits (rep_digits, rep_extra) with a multi-digit one at columns 0, 63, "
                "64, 255, 256, 257: unequal field lengths scanned across a wavefront and a tile edge", [m], seed=7)


def _rows_case(n, permuted=False):
    rng = np.random.default_rng(5000 + n)
    Ks = []
    while sum(Ks) < n:
        Ks.append(min(1 + len(Ks) % 3, n - sum(Ks)))
    mats = [(rng.random((K, 3)) < 0.6) * rng.integers(1, 130, (K, 3)) for K in Ks]
    mats[0][0, 0] = 5                                         # a Matrix Market block needs an entry
    rows, name = None, f"rows{n}"
    if permuted:
        rows = rng.permutation(n)
        rows[5 % n] = rows[n - 3]                             # one row named twice (another not at all)
        name += "_permuted"
    return Case(name, "c", f"{n} rendered rows of unequal byte length: k_rep_scan's 1024-row step and its carry"
                + (", rows[] a permuted index list with one row named twice" if permuted else ""), mats, rows=rows, seed=n)


def _prefix_case():
    rng = np.random.default_rng(11)
    return Case("prefixes", "d", "prefixes of 0, 1, 255, 256, 257 and 600 bytes in one block: the strided prefix copy",
                [_sparse(rng, len(PREFIX_LENGTHS), 5)], pre_len=PREFIX_LENGTHS, seed=11)


def _record_cases():
    out = []
    rng = np.random.default_rng(21)
    n_cols = 67
    mats = [_sparse(rng, K, n_cols) for K in RECORD_KS] + [np.zeros((3, n_cols), np.int64), np.zeros((2, n_cols), np.int64)]
    out.append(Case("records_K", "e", "K = 1, 63, 64, 70, a record without reads and one whose reads all have label >= K; "
                    "scrambled ids with id_min > 0 and gaps in the id table", mats, ids=_scrambled_ids(rng, n_cols),
                    n_over=[3, 3, 3, 3, 0, 9], seed=21))
    # ---- pivot-completeness, 257 columns
    n_cols, S = 257, [0, 5, 63, 64, 255, 256]
    full = np.zeros((3, n_cols), np.int64)
    full[:, S] = rng.integers(1, 9, (3, len(S)))
    hole = full.copy()
    hole[1, 64] = 0                                           # a single (row, cell) count removed
    last = full.copy()
    last[2, 256] = 0                                          # the only incomplete column is column 256 of 257
    gap = np.zeros((4, n_cols), np.int64)
    gap[[0, 1, 3]] = full                                     # a row without reads is no row of the pivot
    one = np.zeros((1, n_cols), np.int64)
    one[0, [3, 256]] = 2
    out.append(Case("records_complete", "e", "a complete record, the same with one (row, cell) count removed, one whose "
                    "only incomplete column is column 256 of 257, a complete one with a row without reads, K = 1",
                    [full, hole, last, gap, one], n_over=[2, 0, 2, 0, 1], want_complete=[1, 0, 0, 1, 1], seed=22))
    # ---- reads that add to no count
    ids = np.array([40, 12, 19, 33, 26, 61, 47, 54, 68], dtype=np.int64)      # id_min 12, gaps everywhere
    small = lambda: [_sparse(rng, K, len(ids), 0.6) for K in (2, 3, 2)]
    out.append(Case("unknown_id_no_site", "e", "reads with label >= K of unknown cells (below id_min, in a gap, beyond the "
                    "table): not looked up, no error", small(), ids=ids, raw=[[], [(3, 5), (4, 13), (3, 900), (5, -2)], []],
                    seed=23))
    out.append(Case("unknown_id_site", "e", "reads with label < K of unknown cells: bad_read_out[0] is the first one's "
                    "read index", small(), ids=ids, raw=[[], [(0, 13), (2, 900)], [(1, 5)]], seed=24))
    out.append(Case("negative_label", "e", "reads with a negative label: bad_read_out[1] is the first one's read index",
                    small(), ids=ids, raw=[[], [(-1, 12)], [(-7, 900)]], seed=25))
    out.append(Case("unknown_and_negative", "e", "both errors in one call, each reported in its own slot", small(), ids=ids,
                    raw=[[(1, 11)], [(-1, 40), (2, 69)], []], seed=26))
    return out


def _segment_case():
    rng = np.random.default_rng(31)
    mats = [_sparse(rng, K, SEG_COLS) for K in (2, 3, 4)]
    last = SEG_FIRST + max(sum(v) for v in SEG_LENGTHS.values())
    assert last < SEG_COLS
    for m in mats:                                            # large counts in the columns of no segment
        m[:, :SEG_FIRST] = 3000
        m[:, last:] = 3000
    segs = [[SEG_FIRST + sum(v[:k]) for k in range(len(v) + 1)] for _n, v in sorted(SEG_LENGTHS.items())]
    rows = np.random.default_rng(32).permutation(9)
    return Case("segments", "g", "1, 3, 4, 5 and 9 segments (four wavefronts per workgroup) of 0, 1, 63, 64, 65 and 300 "
                "columns, seg_off[0] > 0 and seg_off[n_seg] < n_cols with large counts outside, rows permuted", mats,
                rows=rows, segs=segs, seed=31)


@functools.lru_cache(maxsize=None)
def cases():
    out = _column_cases() + [_width_case()] + [_rows_case(n) for n in ROWS] + [_rows_case(ROWS[-1], permuted=True)]
    out += [_prefix_case()] + _record_cases() + [_segment_case()]
    assert len({c.name for c in out}) == len(out)
    return out


# ---------------------------------------------------------------- the cases of the histogram kernels
class HistCase:
    """n_codes cluster codes (None: id2code = NULL, one group); records of Ks[r] with the reads (label, code) recs[r]"""

    def __init__(self, name, note, n_codes, Ks, recs, seed):
        self.name, self.note, self.n_codes, self.Ks, self.recs, self.seed = name, note, n_codes, Ks, recs, seed

    @functools.cached_property
    def reads(self):
        """(K, read offsets, labels, cell ids; id_min, the id -> code table or None): every code has a cell of its own,
        the first few a second one; ids are odd numbers from 7 on, the even ones are gaps of the table"""
        rng = np.random.default_rng(self.seed)
        n = self.n_codes or 1
        extra = min(n, 5)
        code_of_cell = np.concatenate([np.arange(n), np.arange(extra)])
        ids = 7 + 2 * rng.permutation(n + extra).astype(np.int64)
        lab, cb, off = [], [], [0]
        for reads in self.recs:
            l = np.array([x for x, _c in reads], dtype=np.int64)
            c = np.array([x for _l, x in reads], dtype=np.int64)
            second = (c < extra) & (rng.random(len(c)) < 0.5)
            lab.append(l)
            cb.append(ids[np.where(second, n + c, c)] if len(c) else np.zeros(0, np.int64))
            off.append(off[-1] + len(l))
        table = None
        if self.n_codes is not None:
            table = np.full(int(ids.max()) - 7 + 1, -1, dtype=np.int32)
            table[ids - 7] = code_of_cell
        return (np.array(self.Ks, dtype=np.int32), np.array(off, dtype=np.int64), np.concatenate(lab).astype(np.int64),
                np.concatenate(cb).astype(np.int64), 7, table)

    @functools.cached_property
    def expected(self):
        """(groups per record, the codes of all records, the histograms of all records flattened)"""
        n_groups, codes, hist = [], [], []
        for K, reads in zip(self.Ks, self.recs):
            present, h = histogram(K, [l for l, _c in reads], [c for _l, c in reads])
            n_groups.append(len(present))
            codes += present
            hist += [v for row in h for v in row]
        return n_groups, codes, hist


def _hist_reads(rng, K, codes):
    """1 to 3 reads per code with labels 0 .. K + 1; the first code's reads all have a label >= K"""
    out = []
    for j, c in enumerate(codes):
        for _ in range(int(rng.integers(1, 4))):
            out.append((int(rng.integers(K, K + 2)) if j == 0 else int(rng.integers(0, K + 2)), int(c)))
    order = rng.permutation(len(out)).tolist()
    return [out[i] for i in order]


def _hist_case(n_codes):
    rng = np.random.default_rng(9000 + n_codes)
    ends = sorted({0, n_codes - 1})
    bits = [c for c in range(n_codes) if c % 32 in (0, 31)]
    third = sorted(rng.choice(n_codes, size=max(1, n_codes // 3), replace=False).tolist())
    Ks, recs = [], []
    for K in (1, 4):
        for codes in (ends, bits, third, []):
            Ks.append(K)
            recs.append(_hist_reads(rng, K, codes))
    return HistCase(f"codes{n_codes}", f"{n_codes} cluster codes: {(n_codes + 31) // 32} bitmap words of 32 codes, walked "
                    "256 at a time with a carry; reads only in code 0 and the last code, in every code on bit 0 and bit 31 "
                    "of a word, in a third of the codes, and none, K = 1 and 4", n_codes, Ks, recs, n_codes)


@functools.lru_cache(maxsize=None)
def hist_cases():
    rng = np.random.default_rng(9999)
    null = HistCase("no_cluster_file", "id2code = NULL: every read is of the one group, code 0", None, [1, 4, 3],
                    [[(int(rng.integers(0, 3)), 0) for _ in range(300)], [(int(rng.integers(0, 6)), 0) for _ in range(700)], []], 1)
    return [_hist_case(n) for n in CODES] + [null]


# ---------------------------------------------------------------- the directory of the command tests
COMMAND_SEED = 3


@functools.lru_cache(maxsize=None)
def command_records(gen_seed=COMMAND_SEED, n_rec=1400):
    """1,400 records of K = 2..3 with a few reads each on 5 barcodes (scrambled ids; A: two cells, B: three): more than
    2,048 matrix rows and more than 1,024 records with two kept rows, so with the production block rule every caller of
    k_rep_scan sees n > 1024.  Returns (records, barcode_index.csv text, cluster file text)"""
    rng = np.random.default_rng(gen_seed)
    ids = np.array([31, 4, 18, 9, 25], dtype=np.int64)
    bc = "CB,index\n" + "".join(f"L{j}-1,{i}\n" for j, i in enumerate(ids.tolist()))
    clu = "index,group\n" + "".join(f"{i},{'AABBB'[j]}\n" for j, i in enumerate(ids.tolist()))
    records = []
    for r in range(n_rec):
        K = 2 + r % 2
        n = int(rng.integers(4, 13))
        lab = rng.integers(0, K + 1, n)                       # some reads of no site
        lab[:2] = (0, K - 1)
        records.append(dict(gene_info_str=f"{1 + r % 4}:LG{r}:{1 + r % 2}:{100 * r + 1}-{100 * r + 90}:{'+-'[r % 2]}", K=K,
                            alpha_arr=np.sort(rng.choice(np.arange(1, 80), K, replace=False)).astype(np.int64),
                            beta_arr=rng.choice([5.0, 7.5, 10.0], K), label_arr=lab.astype(np.int64),
                            cb_id_arr=ids[rng.integers(0, 5, n)].astype(np.int64)))
    return records, bc, clu
