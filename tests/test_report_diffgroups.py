"""`scape diff_pa_groups`: the omnibus permutation test of pA usage across G = 2..64 cell populations
(scape_amd/report.py, section diff_pa_groups; kernels k_rep_perm_labels, k_rep_groups_rowstat, k_rep_groups_obs and
k_rep_perm_groups of scape_amd/csrc/perm.inc).

The oracle below restates the command's contract in exact arithmetic and imports nothing from scape_amd: Python ints for
keys, ranks, labels and sums, and - for the statistics - integers over a common denominator: with D = the product of the
A_g > 0 of a labelling, W_g = D / A_g and L = lcm(t_i),
    s_i = (sum_g N_ig^2 W_g) / D = n_i / D          S = sum_i s_i / (T t_i) = (sum_i n_i L / t_i) / (T L D) = Q / (T L D)
so two labellings compare by cross-multiplying with the other's D (T and L belong to the record).  The Fractions of the
printed floats are formed from the same integers.  For every count the oracle gives lo = #{stat(p) >= stat(0)} and
hi = #{stat(p) >= stat(0) (1 - 2^-39)}; every GPU test first asserts lo == hi for every site and record of its case, on
the oracle alone, and then that the device's or the file's counts EQUAL lo.  That lo == hi holds for every case of this
file (generator seeds included) was checked on a CPU before the GPU saw them; no case is excused.

Rounding bound of the record statistic (include/scape_hip.h): kept rows + populations <= 4,000, because the device sums
the groups inside a row and the rows inside the record; test_groups_entry_point_refusals holds the entry point to it."""
import bisect
import csv
import functools
import io
import math
import os
from fractions import Fraction

import numpy as np
import pytest

import report_cases as rc
from report_cases import G as GOLD, M64, bh, members, mix, no_gpu, run as _run  # noqa: F401  (no_gpu: fixture)

HEADER = ["gene", "pa_info", "num_groups", "top_group", "top_delta_usage", "site_stat", "n_ge", "p_val", "p_val_adj",
          "gene_stat", "gene_n_ge", "gene_p_val", "gene_p_val_adj", "n_perm"]
SLACKS = ((1, 1), ((1 << 39) - 1, 1 << 39))
MAX_ROWS_AND_GROUPS = 4000


# ---------------------------------------------------------------- the contract, restated
def labels(seed, p, sizes):
    """group of every position under permutation p >= 1: the sizes[0] smallest keys form group 0, the next sizes[1]
    group 1, ...; g = #{h in 1..G-1 : c_h <= rank}"""
    n = sum(sizes)
    base = mix((seed + GOLD * p) & M64)
    keys = sorted((mix((base + GOLD * (j + 1)) & M64) & ~0xFFFFFF & M64) | j for j in range(n))
    cuts = [sum(sizes[:h]) for h in range(1, len(sizes))]
    out = [0] * n
    for rank, k in enumerate(keys):
        out[k & 0xFFFFFF] = bisect.bisect_right(cuts, rank)
    return out


def observed(sizes):
    return [g for g, m in enumerate(sizes) for _ in range(m)]


class _Rec:
    """a tested record: per kept row its nonzeros [(position, count)] and t_i; integers only"""

    def __init__(self, gene, pas, nzs, sizes):
        self.gene, self.pas, self.nzs, self.G = gene, pas, nzs, len(sizes)
        self.t = [sum(v for _j, v in nz) for nz in nzs]
        self.T = sum(self.t)
        self.L = math.lcm(*self.t)
        self.a0 = self.sums(observed(sizes))
        self.n0, self.Q0, self.D0 = self.stat(self.a0)
        self.site = [[0, 0] for _ in nzs]                  # lo, hi
        self.gene_ge = [0, 0]

    def sums(self, lab):
        out = []
        for nz in self.nzs:
            a = [0] * self.G
            for j, v in nz:
                a[lab[j]] += v
            out.append(a)
        return out

    def stat(self, a):
        """([n_i], Q, D) with s_i = n_i / D and S = Q / (T L D)"""
        A = [sum(row[g] for row in a) for g in range(self.G)]
        live = [g for g in range(self.G) if A[g] > 0]
        D = math.prod(A[g] for g in live)
        W = {g: D // A[g] for g in live}
        n = [sum((row[g] * self.T - ti * A[g]) ** 2 * W[g] for g in live) for row, ti in zip(a, self.t)]
        return n, sum(ni * (self.L // ti) for ni, ti in zip(n, self.t)), D

    def count(self, lab):
        n, Q, D = self.stat(self.sums(lab))
        for w, (num, den) in enumerate(SLACKS):
            self.gene_ge[w] += Q * self.D0 * den >= self.Q0 * D * num
            for i in range(len(n)):
                self.site[i][w] += n[i] * self.D0 * den >= self.n0[i] * D * num

    def A0(self):
        return [sum(row[g] for row in self.a0) for g in range(self.G)]

    def S0(self):
        return Fraction(self.Q0, self.T * self.L * self.D0)

    def share0(self, i):
        return Fraction(self.n0[i], self.D0 * self.T * self.t[i])


def oracle_records(rec_rows, pop_cols, n_perm, seed):
    """rec_rows: [(gene, [(pa_info, counts over every matrix column)])] in file order; pop_cols: the matrix columns of
    every population, ascending.  Returns the tested records, counted over permutations 1 .. n_perm."""
    sizes = [len(c) for c in pop_cols]
    cols = np.array([j for c in pop_cols for j in c], dtype=np.int64)
    assert 2 <= len(sizes) <= 64 and min(sizes) >= 1 and len(cols) < 1 << 24
    recs = []
    for gene, rows in rec_rows:
        pas, nzs = [], []
        for pa, row in rows:
            nz = [(j, int(v)) for j, v in enumerate(np.asarray(row)[cols].tolist()) if v]
            if nz:
                pas.append(pa)
                nzs.append(nz)
        if len(nzs) < 2:
            continue
        r = _Rec(gene, pas, nzs, sizes)
        if sum(A > 0 for A in r.A0()) >= 2:
            assert r.T < 1 << 31
            recs.append(r)
    for p in range(1, n_perm + 1):
        lab = labels(seed, p, sizes)
        for r in recs:
            r.count(lab)
    return recs


def oracle(rec_rows, pop_cols, names, n_perm, seed):
    """the expected lines: dicts of the text columns, the exact counts (lo, hi) and the Fractions of the float columns"""
    recs = oracle_records(rec_rows, pop_cols, n_perm, seed)
    sizes = [len(c) for c in pop_cols]
    bounds = np.concatenate([[0], np.cumsum(sizes)]).tolist()
    lines = []
    for r in recs:
        A, S0 = r.A0(), r.S0()
        assert S0 == sum(Fraction((a * r.T - ti * Ag) ** 2, Ag * r.T * ti)
                         for row, ti in zip(r.a0, r.t) for a, Ag in zip(row, A) if Ag > 0)
        for i, pa in enumerate(r.pas):
            terms = [(Fraction((r.a0[i][g] * r.T - r.t[i] * A[g]) ** 2, A[g]), g) for g in range(r.G) if A[g] > 0]
            top = max(terms, key=lambda tg: (tg[0], -tg[1]))[1]          # the first population wins ties
            cells = [sum(1 for j, _v in r.nzs[i] if bounds[g] <= j < bounds[g + 1]) for g in range(r.G)]
            lines.append(dict(gene=r.gene, pa=pa, num_groups=sum(Ag > 0 for Ag in A), top=names[top],
                              top_delta=Fraction(r.a0[i][top], A[top]) - Fraction(r.t[i], r.T),
                              site_stat=r.share0(i), site=tuple(r.site[i]), S0=S0, gene_ge=tuple(r.gene_ge),
                              usage=[Fraction(r.a0[i][g], A[g]) if A[g] > 0 else None for g in range(r.G)],
                              pct=[repr(cells[g] / sizes[g]) for g in range(r.G)], first=i == 0))
    p_site = bh([Fraction(1 + ln["site"][0], 1 + n_perm) for ln in lines])
    firsts = [k for k, ln in enumerate(lines) if ln["first"]]
    p_gene = bh([Fraction(1 + lines[k]["gene_ge"][0], 1 + n_perm) for k in firsts])
    g = -1
    for k, ln in enumerate(lines):
        g += ln["first"]
        ln["p_adj"], ln["gene_p_adj"] = p_site[k], p_gene[g]
    return lines


def assert_no_near_tie(lines, what):
    """lo == hi for every site and record: no permutation's statistic lies within 2^-39 below the observed one, so the
    device's f64 comparison (slack 2^-40) can hide nothing"""
    for ln in lines:
        assert ln["site"][0] == ln["site"][1], (what, ln["gene"], ln["pa"], ln["site"])
        assert ln["gene_ge"][0] == ln["gene_ge"][1], (what, ln["gene"], ln["gene_ge"])


def populations_all(bc_csv, clu_csv, idents=None):
    """[(name, matrix columns ascending)]: the named clusters in the order given, or every cluster in order of first
    appearance in the file, those without a column dropped; clusters as text, a repeated id keeps its last row"""
    last = {}
    for i, name in rc.cluster_rows(clu_csv):
        last[i] = name
    col_clu = [last.get(i, "") for i in rc.column_ids(bc_csv)]
    names = list(idents) if idents else rc.first_clusters(clu_csv)
    pops = [(name, [j for j, x in enumerate(col_clu) if x == name]) for name in names]
    return [(name, cols) for name, cols in pops if cols]


def _float_ok(got, want):
    if want is None:
        return got == "nan"
    if want == 0:
        return float(got) == 0.0 and repr(float(got)) == got
    return rc.close(got, want)


def compare(text, lines, names, n_perm, what):
    rows = list(csv.reader(io.StringIO(text)))
    G = len(names)
    assert rows[0] == HEADER + [f"usage.{n}" for n in names] + [f"pct.{n}" for n in names], what
    body = rows[1:]
    print(what, "lines", len(body), "expected", len(lines))
    assert len(body) == len(lines), what
    for got, ln in zip(body, lines):
        ctx = (what, ln["gene"], ln["pa"], got)
        assert len(got) == 14 + 2 * G, ctx
        assert got[0] == ln["gene"] and got[1] == ln["pa"] and got[13] == str(n_perm), ctx
        assert got[2] == str(ln["num_groups"]) and got[3] == ln["top"], ctx
        assert got[6] == str(ln["site"][0]), ctx
        assert got[10] == str(ln["gene_ge"][0]), ctx
        assert got[7] == repr((1 + ln["site"][0]) / (1 + n_perm)), ctx
        assert got[11] == repr((1 + ln["gene_ge"][0]) / (1 + n_perm)), ctx
        for col, want in ((4, ln["top_delta"]), (5, ln["site_stat"]), (8, ln["p_adj"]), (9, ln["S0"]),
                          (12, ln["gene_p_adj"])):
            assert _float_ok(got[col], want), (ctx, col, float(want))
        for g in range(G):
            assert _float_ok(got[14 + g], ln["usage"][g]), (ctx, "usage", g)
            assert got[14 + G + g] == ln["pct"][g], (ctx, "pct", g)


# ---------------------------------------------------------------- the command
def _args(root, clu, res="res.gene.pkl", idents=(), n_perm=None, seed=None):
    a = ["diff_pa_groups", "--output_dir", str(root), "--res_pkl_file", res, "--cell_cluster_file", str(clu)]
    for i in idents:
        a += ["--idents", i]
    for opt, v in (("--n_perm", n_perm), ("--seed", seed)):
        if v is not None:
            a += [opt, str(v)]
    return a


def _path(root, clu, res, idents=()):
    kind = res[len("res."):-len(".pkl")]
    stem = os.path.splitext(os.path.basename(str(clu)))[0]
    tag = "." + "+".join(idents) if idents else ""
    return os.path.join(str(root), f"{stem}.{kind}{tag}.diff_pa_groups.csv")


def _command(root, clu, res, idents, n_perm, seed, what=""):
    r = _run(_args(root, clu, res, idents, n_perm, seed))
    assert r.exit_code == 0, (what, r.output, repr(r.exception))
    assert not rc.parts_left(root)
    with open(_path(root, clu, res, idents), newline="") as fh:
        return fh.read()


# ---------------------------------------------------------------- CPU
SIZE_SETS = {"1-1": (1, 1), "1-1-1": (1, 1, 1), "1-63-64-65-7": (1, 63, 64, 65, 7),
             "64-groups": tuple(1 + g % 5 for g in range(64)), "300-5-40": (300, 5, 40)}


@pytest.mark.parametrize("sizes", list(SIZE_SETS.values()), ids=list(SIZE_SETS))
def test_labelling_is_a_bijection_with_the_groups_sizes(sizes):
    seen = set()
    for p in (1, 2, 257, 999):
        lab = labels(5, p, sizes)
        assert len(lab) == sum(sizes) and [lab.count(g) for g in range(len(sizes))] == list(sizes)
        ks = sorted(rc.key(5, p, j) for j in range(len(lab)))
        assert [lab[k & 0xFFFFFF] for k in ks] == observed(sizes)       # ranks in order walk the groups in order
        seen.add(tuple(lab))
    assert len(lab) <= 3 or len(seen) > 1


@pytest.mark.parametrize("n1,n2,seed", [(1, 1, 0), (1, 63, 1), (63, 1, 2), (230, 301, 1), (64, 64, M64)])
def test_two_groups_are_diff_pa_populations(n1, n2, seed):
    for p in (1, 2, 300):
        lab = labels(seed, p, (n1, n2))
        assert sorted(j for j, g in enumerate(lab) if g == 0) == sorted(members(seed, p, n1, n1 + n2))


def test_two_groups_statistic_is_diff_pa_statistic():
    """with G = 2 the oracle's S equals diff_pa's sum N_i^2 / (t_i A B) as a Fraction, on random small tables, and the
    integer comparison of _Rec.count is the Fraction comparison"""
    rng = np.random.default_rng(3)
    for trial in range(20):
        R, n1, n2 = int(rng.integers(2, 6)), int(rng.integers(1, 8)), int(rng.integers(1, 8))
        n = n1 + n2
        m = (rng.random((R, n)) < 0.6) * rng.integers(1, 5, (R, n))
        m[:, 0] |= 1                                                      # every row has a read, population 0 too
        m[0, n1] |= 1                                                     # and population 1
        rows = [(f"r{i}", m[i]) for i in range(R)]
        recs = oracle_records([("g", rows)], [list(range(n1)), list(range(n1, n))], 25, trial)
        assert len(recs) == 1
        r = recs[0]

        def diff_pa_S(a):
            A = sum(a)
            B = r.T - A
            if A == 0 or B == 0:
                return Fraction(0)
            return sum(Fraction((ai * r.T - ti * A) ** 2, ti * A * B) for ai, ti in zip(a, r.t))
        assert r.S0() == diff_pa_S([row[0] for row in r.a0])
        lo = hi = 0
        for p in range(1, 26):
            a = r.sums(labels(trial, p, (n1, n2)))
            n_i, Q, D = r.stat(a)
            S = Fraction(Q, r.T * r.L * D)
            assert S == diff_pa_S([row[0] for row in a])
            lo += S >= r.S0()
            hi += S >= r.S0() * Fraction(*SLACKS[1])
        assert r.gene_ge == [lo, hi]


def test_help_and_import_path():
    r = _run(["--help"])
    assert r.exit_code == 0 and "diff_pa_groups" in r.output
    r = _run(["diff_pa_groups", "--help"])
    assert r.exit_code == 0, r.output
    for o in ("--output_dir", "--res_pkl_file", "--cell_cluster_file", "--idents", "--n_perm", "--seed"):
        assert o in r.output
    assert "--strata_file" not in r.output
    import scape.utils as su
    from scape_amd import report
    assert su.diff_pa_groups is report.diff_pa_groups


def test_prerequisites_and_argument_errors(tmp_path, no_gpu):
    clu = tmp_path / "groups.csv"
    r = _run(_args(tmp_path / "nope", clu))
    assert r.exit_code != 0 and "Given output_dir folder does not exists." in str(r.exception)
    r = _run(_args(tmp_path, clu))
    assert "Given res_pkl_file is not in output_dir." in str(r.exception)
    (tmp_path / "res.gene.pkl").write_bytes(b"")
    r = _run(_args(tmp_path, clu))
    assert "Given cell_cluster_file file does not exists" in str(r.exception)
    clu.write_text("index,group\n3,A\n4,B\n5,\n6,a/b\n77,ghost\n")
    (tmp_path / "barcode_index.csv").write_text("CB,index\nA-1,3\nB-1,4\nC-1,5\nD-1,6\n")
    for extra, word in ((["--idents", "A", "--idents", "Z"], "'Z'"), (["--idents", "A", "--idents", "A"], "twice"),
                        (["--idents", "A", "--idents", "ghost"], "has no cell"), (["--idents", "A"], "1 populations"),
                        (["--idents", "A", "--idents", ""], "names no cluster"),
                        (["--idents", "A", "--idents", "a/b"], "file name"),
                        (["--n_perm", "0"], "n_perm"), (["--n_perm", str(1 << 31)], "n_perm"),
                        (["--seed", "-1"], "seed"), (["--seed", str(1 << 64)], "seed")):
        r = _run(_args(tmp_path, clu) + extra)
        assert isinstance(r.exception, ValueError) and word in str(r.exception), (extra, repr(r.exception))
    clu.write_text("index,group\n3,A\n4,A\n5,\n77,ghost\n")              # one cluster with a cell
    r = _run(_args(tmp_path, clu))
    assert isinstance(r.exception, ValueError) and "1 populations" in str(r.exception)
    ids = list(range(100, 166))
    (tmp_path / "barcode_index.csv").write_text("CB,index\n" + "".join(f"C{i}-1,{i}\n" for i in ids))
    clu.write_text("index,group\n" + "".join(f"{i},g{i}\n" for i in ids[:65]))
    r = _run(_args(tmp_path, clu))
    assert isinstance(r.exception, ValueError) and "65 populations" in str(r.exception)
    r = _run(["diff_pa_groups", "--output_dir", str(tmp_path), "--res_pkl_file", "res.gene.pkl"])
    assert r.exit_code == 2 and "--cell_cluster_file" in r.output
    assert sorted(os.listdir(tmp_path)) == ["barcode_index.csv", "groups.csv", "res.gene.pkl"]


# ---------------------------------------------------------------- GPU: the labels
def _label_bits(lab):
    words = [0] * ((len(lab) + 63) // 64)
    for j, g in enumerate(lab):
        if g == 0:
            words[j >> 6] |= 1 << (j & 63)
    return words


@pytest.mark.gpu
@pytest.mark.parametrize("p_first", [1, 257])
@pytest.mark.parametrize("sizes", list(SIZE_SETS.values()), ids=list(SIZE_SETS))
def test_labels_entry_point(sizes, p_first):
    """scape_hip_report_perm_labels + _get against the oracle's labels for each of 300 permutations (one full tile of
    the test kernel plus a part); with two groups, group 0 is population 1 of scape_hip_report_perm_masks"""
    import ctypes
    from scape_amd import _lib
    from scape_amd._lib import P_i32, check as chk, ptr
    seed, p_count, n = 77, 300, sum(sizes)
    ctx = _lib.default_context(None)
    lib = ctx.lib
    sz = np.array(sizes, dtype=np.int32)
    got = np.zeros(n, dtype=np.uint8)
    try:
        chk(lib.scape_hip_report_perm_labels(ctx.h, len(sizes), ptr(sz, P_i32), p_first, p_count, seed), "perm_labels")
        if len(sizes) == 2:
            chk(lib.scape_hip_report_perm_masks(ctx.h, sizes[0], sizes[1], p_first, p_count, seed), "perm_masks")
        words = np.zeros((n + 63) // 64, dtype=np.uint64)
        for p in range(p_count):
            chk(lib.scape_hip_report_perm_labels_get(ctx.h, p, ptr(got, ctypes.POINTER(ctypes.c_uint8))), "labels_get")
            want = labels(seed, p_first + p, sizes)
            assert got.tolist() == want, (sizes, p_first + p)
            if len(sizes) == 2:
                chk(lib.scape_hip_report_perm_bits_get(ctx.h, p, ptr(words, ctypes.POINTER(ctypes.c_uint64))), "bits_get")
                assert words.tolist() == _label_bits(got.tolist()), (sizes, p_first + p)
        assert lib.scape_hip_report_perm_labels_get(ctx.h, p_count, ptr(got, ctypes.POINTER(ctypes.c_uint8))) != 0
        assert lib.scape_hip_report_perm_labels_get(ctx.h, -1, ptr(got, ctypes.POINTER(ctypes.c_uint8))) != 0
        assert lib.scape_hip_report_perm_labels_get(ctx.h, 0, None) != 0
    finally:
        lib.scape_hip_report_free(ctx.h)


@pytest.mark.gpu
def test_labels_argument_checks():
    import ctypes
    from scape_amd import _lib
    from scape_amd._lib import P_i32, ptr
    ctx = _lib.default_context(None)
    lib = ctx.lib

    def call(sizes, p_first=1, p_count=1):
        sz = np.array(sizes, dtype=np.int32)
        return lib.scape_hip_report_perm_labels(ctx.h, len(sizes), ptr(sz, P_i32), p_first, p_count, 0)
    try:
        for args, word in ((([5],), "2 .. 64"), (([1] * 65,), "2 .. 64"), (([3, 0, 2],), "at least one cell"),
                           (([3, -1],), "at least one cell"), (([1 << 23, 1 << 23],), "2^24"),
                           (([3, 3], 0, 1), "p_first"), (([3, 3], 1, 0), "p_count")):
            assert call(*args) != 0 and word in _lib.last_error(), args
        assert lib.scape_hip_report_perm_labels(ctx.h, 2, None, 1, 1, 0) != 0
        assert lib.scape_hip_report_perm_labels(None, 2, None, 1, 1, 0) != 0
        got = np.zeros(8, dtype=np.uint8)
        assert lib.scape_hip_report_perm_labels_get(ctx.h, 0, ptr(got, ctypes.POINTER(ctypes.c_uint8))) != 0
        assert "perm_labels" in _lib.last_error()                         # no refused call left labels behind
    finally:
        lib.scape_hip_report_free(ctx.h)


# ---------------------------------------------------------------- GPU: the test kernel
N_TESTED, N_REST, EP_SEED, EP_PERM = 171, 6, 31, 300


@functools.lru_cache(maxsize=None)
def groups_matrix():
    """the hand-made matrix of the test kernel's tests: records of 2, 5 and 70 rows over 171 tested columns in front of
    6 others; the 5-row record reads only from columns < 100, so with three groups or more its last group has no read
    as observed.  Returns (Ks, read offsets, labels, cell ids, dense counts, kept count rows, their offsets)"""
    rng = np.random.default_rng(21)
    n_cols = N_TESTED + N_REST
    Ks = np.array([2, 5, 70], dtype=np.int32)
    lab, cb, off = [], [], [0]
    for K in Ks.tolist():
        m = 40 * K + 300
        lab.append(rng.integers(0, K + 1, m))
        cb.append(rng.integers(0, 100, m) if K == 5 else (rng.integers(0, n_cols, m) ** 2) // n_cols)
        off.append(off[-1] + m)
    lab, cb, off = np.concatenate(lab).astype(np.int64), np.concatenate(cb).astype(np.int64), np.array(off, np.int64)
    rowbase = np.concatenate([[0], np.cumsum(Ks)])
    dense = np.zeros((int(Ks.sum()), n_cols), dtype=np.int64)
    for r, K in enumerate(Ks.tolist()):
        l, c = lab[off[r]:off[r + 1]], cb[off[r]:off[r + 1]]
        np.add.at(dense, (rowbase[r] + l[l < K], c[l < K]), 1)
    kept = [np.nonzero(dense[rowbase[r]:rowbase[r + 1], :N_TESTED].sum(axis=1) > 0)[0] + rowbase[r] for r in range(3)]
    assert [len(k) for k in kept] == [2, 5, 70]
    rows = np.concatenate(kept).astype(np.int64)
    roff = np.concatenate([[0], np.cumsum([len(k) for k in kept])]).astype(np.int64)
    return Ks, off, lab, cb, dense, rows, roff


def _split(n, G):
    """G group sizes that differ by at most one"""
    return [n // G + (g < n % G) for g in range(G)]


@functools.lru_cache(maxsize=None)
def groups_oracle(G):
    _Ks, _off, _lab, _cb, dense, rows, roff = groups_matrix()
    sizes = _split(N_TESTED, G)
    bounds = np.concatenate([[0], np.cumsum(sizes)]).tolist()
    rec_rows = [(f"rec{r}", [(f"row{i}", dense[i]) for i in rows[roff[r]:roff[r + 1]].tolist()]) for r in range(3)]
    recs = oracle_records(rec_rows, [list(range(bounds[g], bounds[g + 1])) for g in range(G)], EP_PERM, EP_SEED)
    assert len(recs) == 3
    return sizes, recs


@pytest.mark.gpu
@pytest.mark.parametrize("G", [2, 3, 5, 17, 64])
def test_groups_entry_point(G):
    """scape_hip_report_perm_groups on the hand-made matrix: t, a0 and both counts equal the oracle's, S(0) and the
    sites' shares within RTOL of the Fractions; one call with 300 permutations equals three that accumulate"""
    from scape_amd import _lib
    from scape_amd._lib import P_d, P_i32, P_i64, check as chk, ptr
    Ks, off, lab, cb, dense, rows, roff = groups_matrix()
    sizes, recs = groups_oracle(G)
    for r in recs:
        assert r.gene_ge[0] == r.gene_ge[1] and all(lo == hi for lo, hi in r.site), (G, r.gene)
    if G >= 3:
        assert recs[1].A0()[-1] == 0                                      # a group without a read as observed
    seg = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    sz = np.array(sizes, dtype=np.int32)
    ctx = _lib.default_context(None)
    lib = ctx.lib

    def outs():
        return (np.full(len(rows), -1, np.int64), np.full((len(rows), G), -1, np.int64), np.zeros(len(rows), np.int64),
                np.full(3, -1.0), np.full(len(rows), -1.0), np.zeros(3, np.int64))

    def test(o):
        return lib.scape_hip_report_perm_groups(ctx.h, 3, ptr(roff, P_i64), ptr(rows, P_i64), G, ptr(seg, P_i32),
                                                ptr(o[0], P_i64), ptr(o[1], P_i64), ptr(o[2], P_i64), ptr(o[3], P_d),
                                                ptr(o[4], P_d), ptr(o[5], P_i64))
    try:
        assert np.array_equal(rc.device_counts(ctx, Ks, off, lab, cb, N_TESTED + N_REST), dense.sum(axis=1))
        chk(lib.scape_hip_report_perm_labels(ctx.h, G, ptr(sz, P_i32), 1, EP_PERM, EP_SEED), "perm_labels")
        one = outs()
        chk(test(one), "perm_groups")
        want = dict(t=[ti for r in recs for ti in r.t], a0=[row for r in recs for row in r.a0],
                    site=[lo for r in recs for lo, _hi in r.site], gene=[r.gene_ge[0] for r in recs])
        for got, name in ((one[0], "t"), (one[1], "a0"), (one[2], "site"), (one[5], "gene")):
            print(G, name, "equal", got.tolist() == want[name])
            assert got.tolist() == want[name], (G, name)
        for got, exact in zip(one[3].tolist(), [r.S0() for r in recs]):
            assert abs(Fraction(got) - exact) <= rc.RTOL * exact, (G, got, float(exact))
        for got, exact in zip(one[4].tolist(), [r.share0(i) for r in recs for i in range(len(r.t))]):
            assert abs(Fraction(got) - exact) <= rc.RTOL * exact, (G, got, float(exact))
        assert 0 < min(want["gene"]) and min(want["site"]) < max(want["site"]) and max(want["gene"]) <= EP_PERM
        acc = outs()
        for p_first, p_count in ((1, 100), (101, 156), (257, 44)):
            chk(lib.scape_hip_report_perm_labels(ctx.h, G, ptr(sz, P_i32), p_first, p_count, EP_SEED), "perm_labels")
            chk(test(acc), "perm_groups")
        assert acc[2].tolist() == want["site"] and acc[5].tolist() == want["gene"]
        assert np.array_equal(acc[3], one[3]) and np.array_equal(acc[4], one[4])
    finally:
        lib.scape_hip_report_free(ctx.h)


@pytest.mark.gpu
def test_groups_entry_point_refusals():
    """a record beyond the rounding bound (kept rows + groups > 4,000) and the other argument errors return non-zero
    before anything runs"""
    from scape_amd import _lib
    from scape_amd._lib import P_d, P_i32, P_i64, check as chk, ptr
    Ks, off, lab, cb, dense, rows, roff = groups_matrix()
    G = 3
    sizes = _split(N_TESTED, G)
    seg = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    sz = np.array(sizes, dtype=np.int32)
    ctx = _lib.default_context(None)
    lib = ctx.lib

    def test(roff_, rows_, G_=G, seg_=seg):
        n = len(rows_)
        o = (np.zeros(n, np.int64), np.zeros((n, G_), np.int64), np.zeros(n, np.int64), np.zeros(len(roff_) - 1),
             np.zeros(n), np.zeros(len(roff_) - 1, np.int64))
        return lib.scape_hip_report_perm_groups(ctx.h, len(roff_) - 1, ptr(roff_, P_i64), ptr(rows_, P_i64), G_,
                                                ptr(seg_, P_i32), ptr(o[0], P_i64), ptr(o[1], P_i64), ptr(o[2], P_i64),
                                                ptr(o[3], P_d), ptr(o[4], P_d), ptr(o[5], P_i64))
    try:
        assert test(roff, rows) != 0 and "report_counts" in _lib.last_error()
        rc.device_counts(ctx, Ks, off, lab, cb, N_TESTED + N_REST)
        assert test(roff, rows) != 0 and "perm_labels" in _lib.last_error()
        chk(lib.scape_hip_report_perm_labels(ctx.h, G, ptr(sz, P_i32), 1, 10, 1), "perm_labels")
        assert test(roff, rows) == 0
        at_bound = np.resize(rows[7:], MAX_ROWS_AND_GROUPS - G).astype(np.int64)   # the 70-row record's rows, repeated
        assert test(np.array([0, len(at_bound)], np.int64), at_bound) == 0
        beyond = np.resize(rows[7:], MAX_ROWS_AND_GROUPS - G + 1).astype(np.int64)
        assert test(np.array([0, 2, 2 + len(beyond)], np.int64), np.concatenate([rows[:2], beyond])) != 0
        assert "record 1" in _lib.last_error() and "rounding bound" in _lib.last_error()
        assert test(roff, rows, 2, seg[:3].copy()) != 0 and "n_groups" in _lib.last_error()
        bad_seg = seg.copy()
        bad_seg[1] += 1
        assert test(roff, rows, G, bad_seg) != 0 and "seg_off" in _lib.last_error()
        bad_roff = roff.copy()
        bad_roff[1], bad_roff[2] = roff[2], roff[1]
        assert test(bad_roff, rows) != 0 and "non-decreasing" in _lib.last_error()
        bad_rows = rows.copy()
        bad_rows[3] = int(Ks.sum())
        assert test(roff, bad_rows) != 0 and "out of range" in _lib.last_error()
        wide = np.array([N_TESTED, N_REST + 1], dtype=np.int32)
        chk(lib.scape_hip_report_perm_labels(ctx.h, 2, ptr(wide, P_i32), 1, 10, 1), "perm_labels")
        assert test(roff, rows, 2, np.array([0, N_TESTED, N_TESTED + N_REST + 1], np.int32)) != 0
        assert "fewer columns" in _lib.last_error()
    finally:
        lib.scape_hip_report_free(ctx.h)


# ---------------------------------------------------------------- GPU: the synthetic directory
@functools.lru_cache(maxsize=None)
def _syn():
    records, bc, clu_text = rc.synthetic()
    return dict(records=records, bc=bc, clu=clu_text, rec_rows=rc.rec_rows_of(records, rc.column_ids(bc)))


@functools.lru_cache(maxsize=None)
def _syn_lines(idents, n_perm, seed, n_rec=None):
    s = _syn()
    pops = populations_all(s["bc"], s["clu"], idents)
    names = [name for name, _c in pops]
    return names, oracle(s["rec_rows"][:n_rec], [c for _n, c in pops], names, n_perm, seed)


def _check_syn(tmp_path, idents, n_perm, seed, what, n_rec=None):
    names, lines = _syn_lines(idents, n_perm, seed, n_rec)
    assert_no_near_tie(lines, what)
    path = rc.write_synthetic(tmp_path, n_rec)
    text = _command(tmp_path, path, "res.gene.pkl", idents, n_perm, seed, what)
    compare(text, lines, names, n_perm, what)
    return text, lines


def _planted_reach_zero(pairs, what):
    planted = {f"GENE{r}" for r in range(rc.N_PLANTED)}
    seen = {gene.split(":")[1] for gene, ge in pairs if gene.split(":")[1] in planted and ge == 0}
    assert seen == planted, (what, seen)


@pytest.mark.gpu
def test_synthetic_directory_all_clusters(tmp_path):
    """999 permutations of 230 + 301 + 40 cells in the clusters A, B, C (order of first appearance in the file): every
    column of the file against the exact oracle; the planted records reach gene_n_ge = 0, on the oracle and in the file"""
    text, lines = _check_syn(tmp_path, (), 999, 1, "syn/all")
    names, _ = _syn_lines((), 999, 1)
    assert sorted(names) == ["A", "B", "C"]
    genes = {ln["gene"].split(":")[1] for ln in lines}
    assert "GENE5" not in genes and "GENE6" not in genes and len(genes) >= 30    # reads only in A; K = 1
    _planted_reach_zero([(ln["gene"], ln["gene_ge"][0]) for ln in lines if ln["first"]], "oracle")
    body = list(csv.reader(io.StringIO(text)))[1:]
    _planted_reach_zero([(r[0], int(r[10])) for r in body], "file")
    assert len({ln["top"] for ln in lines}) == 3


@pytest.mark.gpu
def test_synthetic_directory_idents_in_the_order_given(tmp_path):
    """--idents B --idents A: population 0 is B, the file name carries .B+A, the columns are usage.B, usage.A, ..."""
    text, lines = _check_syn(tmp_path, ("B", "A"), 999, 1, "syn/B+A")
    assert os.path.basename(_path(tmp_path, "syn_groups.csv", "res.gene.pkl", ("B", "A"))) == \
        "syn_groups.gene.B+A.diff_pa_groups.csv"
    assert text.split("\n", 1)[0].endswith(",usage.B,usage.A,pct.B,pct.A")
    _planted_reach_zero([(ln["gene"], ln["gene_ge"][0]) for ln in lines if ln["first"]], "oracle")


@pytest.mark.gpu
def test_two_idents_count_what_diff_pa_counts(tmp_path):
    """--idents A --idents B against diff_pa --idents_1 A --idents_2 B, same seed and n_perm: the same tested records
    and, record for record, the same gene_n_ge (for G = 2 the two statistics are the same rational)"""
    path = rc.write_synthetic(tmp_path)
    mine = list(csv.reader(io.StringIO(_command(tmp_path, path, "res.gene.pkl", ("A", "B"), 999, 1))))[1:]
    theirs = list(csv.reader(io.StringIO(rc.perm_command("diff_pa", tmp_path, path, "res.gene.pkl", "A", "B", 999, 1))))[1:]
    assert len(mine) == len(theirs) > 100
    assert [(r[0], r[1], r[10]) for r in mine] == [(r[0], r[1], r[12]) for r in theirs]
    for m, t in zip(mine, theirs):
        assert abs(float(m[9]) - float(t[11])) <= 1e-12 * float(t[11])


@pytest.mark.gpu
def test_batch_chunk_and_seed_invariance(tmp_path, monkeypatch):
    """records split over several count batches and the permutations over several chunks: the same bytes; the same seed
    again: the same bytes; another seed: other counts"""
    from scape_amd import _lib, report
    path = rc.write_synthetic(tmp_path)
    big = _command(tmp_path, path, "res.gene.pkl", (), 299, 1)
    assert _command(tmp_path, path, "res.gene.pkl", (), 299, 1) == big
    other = _command(tmp_path, path, "res.gene.pkl", (), 299, 2)
    col = lambda text: [r[6] for r in csv.reader(io.StringIO(text))]
    assert col(big) != col(other) and len(col(big)) == len(col(other)) > 100
    lib = _lib.load_library()
    calls = {"labels": [], "test": 0}
    real_l, real_t = lib.scape_hip_report_perm_labels, lib.scape_hip_report_perm_groups

    def make_labels(*a):
        calls["labels"].append((a[3], a[4]))
        return real_l(*a)

    def test(*a):
        calls["test"] += 1
        return real_t(*a)
    monkeypatch.setattr(lib, "scape_hip_report_perm_labels", make_labels)
    monkeypatch.setattr(lib, "scape_hip_report_perm_groups", test)
    monkeypatch.setattr(report, "MAX_BATCH_BYTES", 1 << 16)             # a record of K = 8 alone takes 57 KB
    monkeypatch.setattr(report, "MAX_PERM_BYTES", 1 << 30)
    assert _command(tmp_path, path, "res.gene.pkl", (), 299, 1) == big
    assert calls["labels"] == [(1, 299)] and calls["test"] > 5
    n_batches = calls["test"]
    calls.update(labels=[], test=0)
    monkeypatch.setattr(report, "MAX_PERM_BYTES", 571 * 100)             # one byte per tested cell: 100 permutations
    assert _command(tmp_path, path, "res.gene.pkl", (), 299, 1) == big
    assert calls["test"] == 3 * n_batches and calls["labels"][:3] == [(1, 100), (101, 100), (201, 99)]


@pytest.mark.gpu
@pytest.mark.parametrize("n_perm", [1, 255, 256, 257])
def test_tile_edges(n_perm, tmp_path):
    """a workgroup of the test kernel takes 256 permutations: one short of a tile, a full tile, one over, and one"""
    _check_syn(tmp_path, ("C", "A", "B"), n_perm, 5, f"tile/{n_perm}", 12)


# ---------------------------------------------------------------- GPU: golden directories
@pytest.mark.gpu
@pytest.mark.parametrize("c,j", rc.golden_perm_params())
def test_golden_case_and_cluster_file(c, j, tmp_path):
    """every golden case and cluster file (empty fields and NaN-like text among them), all clusters, 199 permutations
    (39 where more than 5,000 cells are tested: the oracle sorts every permutation's keys in Python): the file equals
    the exact oracle's, also when no record is tested (header only); a cluster file with fewer than 2 or more than 64
    clusters that have a cell is a ValueError that leaves nothing behind"""
    cs = rc.fixture_case(c)
    texts = rc.cluster_texts(cs)
    bc, paths = rc.write_case(cs, tmp_path)
    fn = cs["clu_files"][j]
    what = f"{cs['name']}/{fn}"
    pops = populations_all(bc, texts[fn])
    if not 2 <= len(pops) <= 64:
        r = _run(_args(tmp_path, paths[j], cs["res"], (), 199, 1))
        assert isinstance(r.exception, ValueError) and "populations" in str(r.exception), what
        assert not rc.parts_left(tmp_path) and not os.path.exists(_path(tmp_path, paths[j], cs["res"]))
        return
    n_cols = len(rc.column_ids(bc))
    pas, dense = rc.dense_of_body(cs["mat_body"], n_cols)
    rec_rows, k = [], 0
    for rec in cs["records"]:
        lab = np.asarray(rec["label_arr"])
        n = len(np.unique(lab[lab < int(rec["K"])]))
        rec_rows.append((rec["gene_info_str"], [(pas[k + i], dense[k + i]) for i in range(n)]))
        k += n
    names = [name for name, _c in pops]
    n_perm = 199 if sum(len(cols) for _n, cols in pops) <= 5000 else 39
    lines = oracle(rec_rows, [cols for _n, cols in pops], names, n_perm, 1)
    assert_no_near_tie(lines, what)
    text = _command(tmp_path, paths[j], cs["res"], (), n_perm, 1, what)
    compare(text, lines, names, n_perm, what)
    kind = cs["res"][len("res."):-len(".pkl")]
    assert os.path.basename(_path(tmp_path, paths[j], cs["res"])).split(".")[-3] == kind


def test_golden_cases_cover_the_edges():
    """among the golden directories: a res.utr.pkl, cluster names that look like NaN, and empty fields"""
    kinds, nanlike, empty = set(), False, False
    for c in rc.case_ids(rc.fixture()):
        cs = rc.fixture_case(c)
        kinds.add(cs["res"])
        for t in rc.cluster_texts(cs).values():
            names = [name for _i, name in rc.cluster_rows(t)]
            nanlike |= any(n.lower() in ("nan", "na", "n/a", "null", "none") for n in names)
            empty |= "" in names
    assert {"res.gene.pkl", "res.utr.pkl"} <= kinds and empty
    print("NaN-like cluster names among the golden cases:", nanlike)
