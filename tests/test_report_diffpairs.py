"""`scape diff_pa_pairs`: diff_pa for every pair of the populations of a cluster file, from one pass over the result file
(scape_amd/report.py, section diff_pa_pairs; kernels k_rep_perm_pair_masks, k_rep_pair_segidx and k_rep_perm_pairs of
scape_amd/csrc/perm.inc).

The contract is "pair (A, B) is exactly `diff_pa --idents_1 A --idents_2 B`", so the yardsticks are diff_pa's: its
exact-integer oracle (tests/test_report_diffpa.py), the Python-int `members` of tests/report_cases.py, and the entry
points and the command of diff_pa themselves.  pair_oracle below restates that oracle for a whole matrix of labellings at
once (numpy for the row sums, which are exact in int64, Python ints in object arrays for the cross-multiplied
comparisons); test_pair_oracle_is_the_diff_pa_oracle checks it against tests/test_report_diffpa.py's, pair by pair.
Like that oracle it gives lo = #{stat(p) >= stat(0)} and hi = #{stat(p) >= stat(0) (1 - 2^-39)} for every count;
test_no_near_tie asserts lo == hi for every case that a GPU test of this file compares with it, no case left out, and
the GPU tests then assert that the device's counts EQUAL lo."""
import csv
import functools
import io
import math
import os
from fractions import Fraction

import numpy as np
import pytest

import report_cases as rc
import test_report_diffpa as dp
from report_cases import no_gpu  # noqa: F401  (fixture)

HEADER = ["gene", "pa_info", "group_1", "group_2"] + dp.HEADER.split(",")[2:]
NUM, DEN = (1 << 39) - 1, 1 << 39


def pair_list(G):
    return [(g, h) for g in range(G) for h in range(g + 1, G)]


# ---------------------------------------------------------------- the contract, restated
def pair_members(seed, n_g, n_h, p_first, p_count):
    """[permutation][local position] membership of the pair's first population: dp._np_members, which
    test_report_diffpa.test_numpy_selection_is_the_python_selection holds against the Python-int selection"""
    return np.stack([dp._np_members(seed, p, n_g, n_g + n_h) for p in range(p_first, p_first + p_count)])


def pair_oracle(mats, n_g, n_h, n_perm, seed):
    """mats: per record its counts [row][local position of the pair] (int64).  Per record None when the pair does not
    test it, else dict(kept = its rows with a read, t, a0 (lists), site = [(lo, hi)] per kept row, gene = (lo, hi),
    S0 = the observed statistic and d0 = the observed d_i as Fractions)"""
    member = pair_members(seed, n_g, n_h, 1, n_perm).T.astype(np.int64)           # [position][permutation]
    out = []
    for m in mats:
        m = np.asarray(m, dtype=np.int64)
        kept = np.nonzero(m.sum(axis=1) > 0)[0]
        sub = m[kept]
        t = [int(v) for v in sub.sum(axis=1)]
        a0 = [int(v) for v in sub[:, :n_g].sum(axis=1)]
        T, A0 = sum(t), sum(a0)
        if len(kept) < 2 or A0 == 0 or A0 == T:
            out.append(None)
            continue
        assert T < 1 << 31
        L = math.lcm(*t)
        tt, w = np.array(t, dtype=object)[:, None], np.array([L // ti for ti in t], dtype=object)[:, None]
        a = np.concatenate([np.array(a0, dtype=np.int64)[:, None], sub @ member], axis=1).astype(object)
        A = a.sum(axis=0)
        ab = A * (T - A)
        N = a * T - tt * A
        dead = ab == 0                                   # A = 0 or B = 0: every statistic is 0
        N[:, dead] = 0
        ab[dead] = 1
        q = (N * N * w).sum(axis=0)                      # S = q / (L A B)
        absN = np.abs(N)
        gene = tuple(int(np.sum(q[1:] * ab[0] * den >= q[0] * ab[1:] * num)) for num, den in ((1, 1), (NUM, DEN)))
        site = [tuple(int(np.sum(absN[i, 1:] * ab[0] * den >= absN[i, 0] * ab[1:] * num)) for num, den in ((1, 1), (NUM, DEN)))
                for i in range(len(kept))]
        out.append(dict(kept=kept, t=t, a0=a0, site=site, gene=gene, S0=Fraction(int(q[0]), L * int(ab[0])),
                        d0=[Fraction(int(N[i, 0]), int(ab[0])) for i in range(len(kept))]))
    return out


def near_ties(results):
    """the (lo, hi) pairs of a pair_oracle result that differ"""
    return [c for r in results if r is not None for c in r["site"] + [r["gene"]] if c[0] != c[1]]


# ---------------------------------------------------------------- the cases the GPU tests compare with the oracle
ENTRY_SIZES = {2: (70, 91), 3: (70, 27, 64), 5: (70, 27, 1, 62, 1)}


@functools.lru_cache(maxsize=None)
def entry_case():
    """rc.entry_point_matrix() (records of 2, 5, 70 and 150 label rows over 161 tested columns and 9 others) and two
    records more.  Record 4, 4 rows: rows 0 and 1 have reads in columns 0..19 and 70..79, row 2 in columns 100..104
    only, row 3 in the untested columns only.  Record 5, 3 rows: rows 0 and 1 have reads in columns 0..19 only, row 2 in
    columns 100..104 only, so a pair without one of the two ranges does not test it.  Returns (Ks, read offsets,
    labels, cell ids, dense counts, n_cols, seed, n_perm)"""
    n1, n2, n_cols, seed, n_perm, Ks, off, lab, cb, dense, _rows, _roff, rng = rc.entry_point_matrix()
    extra = [(4, np.concatenate([rng.integers(0, 2, 120), np.full(30, 2), np.full(10, 3)]),
              np.concatenate([rng.integers(0, 20, 60), rng.integers(70, 80, 60), rng.integers(100, 105, 30),
                              rng.integers(n1 + n2, n_cols, 10)])),
             (3, np.concatenate([rng.integers(0, 2, 80), np.full(25, 2)]),
              np.concatenate([rng.integers(0, 20, 80), rng.integers(100, 105, 25)]))]
    for K, e_lab, e_cb in extra:
        block = np.zeros((K, n_cols), dtype=np.int64)
        np.add.at(block, (e_lab, e_cb), 1)
        Ks, dense = np.concatenate([Ks, [K]]).astype(np.int32), np.concatenate([dense, block])
        lab, cb = np.concatenate([lab, e_lab]).astype(np.int64), np.concatenate([cb, e_cb]).astype(np.int64)
        off = np.concatenate([off, [off[-1] + len(e_lab)]]).astype(np.int64)
    return Ks, off, lab, cb, dense, n_cols, seed, n_perm


@functools.lru_cache(maxsize=None)
def entry_oracle(G):
    """the kept rows over all groups (count rows, offsets per record) and pair_oracle of every pair of ENTRY_SIZES[G]"""
    Ks, _off, _lab, _cb, dense, _n_cols, seed, n_perm = entry_case()
    sizes = ENTRY_SIZES[G]
    seg = np.concatenate([[0], np.cumsum(sizes)])
    rowbase = np.concatenate([[0], np.cumsum(Ks)])
    kept = [np.nonzero(dense[rowbase[r]:rowbase[r + 1], :seg[-1]].sum(axis=1) > 0)[0] + rowbase[r] for r in range(len(Ks))]
    rows = np.concatenate(kept).astype(np.int64)
    roff = np.concatenate([[0], np.cumsum([len(k) for k in kept])]).astype(np.int64)
    res = []
    for g, h in pair_list(G):
        cols = list(range(seg[g], seg[g + 1])) + list(range(seg[h], seg[h + 1]))
        res.append(pair_oracle([dense[k][:, cols] for k in kept], sizes[g], sizes[h], n_perm, seed))
    return rows, roff, res


SYN_PERM, SYN_SEED = 257, 1


@functools.lru_cache(maxsize=None)
def syn_rec_rows():
    records, bc, clu_text = rc.synthetic()
    return rc.rec_rows_of(records, rc.column_ids(bc)), bc, clu_text


def syn_names():
    """the populations of the synthetic directory without --idents: its clusters in order of first appearance"""
    names = tuple(rc.first_clusters(rc.synthetic()[2]))
    assert sorted(names) == ["A", "B", "C"]
    return names


@functools.lru_cache(maxsize=None)
def syn_pair_oracle(id1, id2, n_perm=SYN_PERM, seed=SYN_SEED):
    rec_rows, bc, clu_text = syn_rec_rows()
    c1, c2 = rc.populations(bc, clu_text, id1, id2)
    n_cols = len(rc.column_ids(bc))
    mats = [np.array([row for _pa, row in rows], dtype=np.int64).reshape(len(rows), n_cols)[:, c1 + c2]
            for _gene, rows in rec_rows]
    return pair_oracle(mats, len(c1), len(c2), n_perm, seed)


# ---------------------------------------------------------------- CPU
def test_pair_oracle_is_the_diff_pa_oracle():
    """three populations of 5, 9 and 6 cells, four records (one with reads in two populations only, one with a row
    that a pair leaves out): per pair, lines, exact counts and Fractions equal tests/test_report_diffpa.py's oracle"""
    rng = np.random.default_rng(3)
    sizes, n_perm, seed = (5, 9, 6), 60, 4
    seg = np.concatenate([[0], np.cumsum(sizes)])
    mats = [(rng.random((R, 20)) < 0.5) * rng.integers(1, 4, (R, 20)) for R in (2, 4, 3, 5)]
    mats[1][:, seg[2]:] = 0
    mats[2][1, :seg[2]] = 0
    mats[3][0, :] = 0
    rec_rows = [(f"g{r}", [(f"g{r}p{i}", m[i]) for i in range(len(m))]) for r, m in enumerate(mats)]
    seen = {"untested": 0, "dropped_row": 0, "counts": set()}
    for g, h in pair_list(3):
        c1, c2 = list(range(seg[g], seg[g + 1])), list(range(seg[h], seg[h + 1]))
        lines = dp.oracle(rec_rows, c1, c2, n_perm, seed)
        got = pair_oracle([m[:, c1 + c2] for m in mats], sizes[g], sizes[h], n_perm, seed)
        flat = []
        for r, res in enumerate(got):
            seen["untested"] += res is None
            if res is not None:
                seen["dropped_row"] += len(res["kept"]) < len(mats[r])
                flat += [dict(gene=f"g{r}", pa=f"g{r}p{k}", site=res["site"][i], gene_ge=res["gene"], S0=res["S0"],
                              delta=res["d0"][i], first=i == 0) for i, k in enumerate(res["kept"].tolist())]
        assert len(flat) == len(lines)
        for a, b in zip(flat, lines):
            assert a == {k: b[k] for k in a}, (g, h, a, b)
            seen["counts"].add(a["gene_ge"][0])
    assert seen["untested"] >= 2 and seen["dropped_row"] >= 2 and len(seen["counts"]) > 3


def test_no_near_tie():
    """no permuted statistic of a case that the GPU tests below compare with the oracle lies within 2^-39 below the
    observed one, so the device's f64 comparison (slack 2^-40) can hide nothing: the entry point cases with 2, 3 and 5
    groups, and the three pairs of the synthetic directory"""
    for G in ENTRY_SIZES:
        _rows, _roff, res = entry_oracle(G)
        for k, r in enumerate(res):
            assert near_ties(r) == [], (G, k)
    names = syn_names()
    for g, h in pair_list(3):
        assert near_ties(syn_pair_oracle(names[g], names[h])) == [], (g, h)


def test_entry_cases_cover_the_paths():
    """on the oracle: a record with more than 64 kept rows, a record that some pairs test and others do not, and kept
    rows whose reads all lie outside a pair that tests their record"""
    for G in (3, 5):
        rows, roff, res = entry_oracle(G)
        assert np.diff(roff).max() > 64
        tested = np.array([[r is not None for r in pair] for pair in res])
        assert np.any(tested.any(axis=0) & ~tested.all(axis=0))
        assert any(r is not None and len(r["kept"]) < n for pair in res for r, n in zip(pair, np.diff(roff).tolist()))
        assert any(r is not None and len(r["kept"]) > 64 for pair in res for r in pair)
    assert all(r is not None for r in entry_oracle(2)[2][0][:4])


def _args(root, clu, res="res.gene.pkl", idents=(), n_perm=None, seed=None):
    a = ["diff_pa_pairs", "--output_dir", str(root), "--res_pkl_file", res, "--cell_cluster_file", str(clu)]
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
    return os.path.join(str(root), f"{stem}.{kind}{tag}.diff_pa_pairs.csv")


def _command(root, clu, res, idents, n_perm, seed, what=""):
    r = rc.run(_args(root, clu, res, idents, n_perm, seed))
    assert r.exit_code == 0, (what, r.output, repr(r.exception))
    assert not rc.parts_left(root)
    with open(_path(root, clu, res, idents), newline="") as fh:
        return fh.read()


def test_help_and_import_path():
    r = rc.run(["--help"])
    assert r.exit_code == 0 and "diff_pa_pairs" in r.output
    r = rc.run(["diff_pa_pairs", "--help"])
    assert r.exit_code == 0, r.output
    for o in ("--output_dir", "--res_pkl_file", "--cell_cluster_file", "--idents", "--n_perm", "--seed"):
        assert o in r.output
    assert "--strata_file" not in r.output
    flat = " ".join(r.output.split())
    assert "[default: 9999]" in flat and "[default: 1]" in flat
    import scape.utils as su
    from scape_amd import report
    assert su.diff_pa_pairs is report.diff_pa_pairs


def test_prerequisites_and_argument_errors(tmp_path, no_gpu):
    clu = tmp_path / "groups.csv"
    r = rc.run(_args(tmp_path / "nope", clu))
    assert r.exit_code != 0 and "Given output_dir folder does not exists." in str(r.exception)
    r = rc.run(_args(tmp_path, clu))
    assert "Given res_pkl_file is not in output_dir." in str(r.exception)
    (tmp_path / "res.gene.pkl").write_bytes(b"")
    r = rc.run(_args(tmp_path, clu))
    assert "Given cell_cluster_file file does not exists" in str(r.exception)
    clu.write_text("index,group\n3,A\n4,B\n5,\n6,a/b\n77,ghost\n")
    (tmp_path / "barcode_index.csv").write_text("CB,index\nA-1,3\nB-1,4\nC-1,5\nD-1,6\n")
    for extra, word in ((["--idents", "A"], "1 populations"), (["--idents", "A", "--idents", "A"], "twice"),
                        (["--idents", "A", "--idents", "Z"], "'Z'"), (["--idents", "A", "--idents", "ghost"], "has no cell"),
                        (["--idents", "A", "--idents", "a/b"], "file name"), (["--n_perm", "0"], "n_perm"),
                        (["--n_perm", str(1 << 31)], "n_perm"), (["--seed", "-1"], "seed")):
        r = rc.run(_args(tmp_path, clu) + extra)
        assert isinstance(r.exception, ValueError) and word in str(r.exception), (extra, repr(r.exception))
    clu.write_text("index,group\n3,A\n4,A\n5,\n77,ghost\n")              # one cluster with a cell
    r = rc.run(_args(tmp_path, clu))
    assert isinstance(r.exception, ValueError) and "1 populations: diff_pa_pairs takes 2 to 64" in str(r.exception)
    ids = list(range(100, 165))
    (tmp_path / "barcode_index.csv").write_text("CB,index\n" + "".join(f"X{i}-1,{i}\n" for i in ids))
    clu.write_text("index,group\n" + "".join(f"{i},c{i}\n" for i in ids))
    r = rc.run(_args(tmp_path, clu))
    assert isinstance(r.exception, ValueError) and "65 populations: diff_pa_pairs takes 2 to 64" in str(r.exception)
    assert sorted(os.listdir(tmp_path)) == ["barcode_index.csv", "groups.csv", "res.gene.pkl"]


# ---------------------------------------------------------------- GPU: the membership bits
def _words(member):
    """uint64 words of a boolean membership vector, bit j % 64 of word j / 64"""
    n_words = (len(member) + 63) // 64
    bits = np.zeros(n_words * 64, dtype=np.uint64)
    bits[:len(member)] = member
    return (bits.reshape(n_words, 64) << np.arange(64, dtype=np.uint64)).sum(axis=1, dtype=np.uint64)


def test_words_helper():
    m = np.zeros(130, dtype=bool)
    m[[0, 63, 64, 129]] = True
    assert _words(m).tolist() == [1 | 1 << 63, 1, 2]


def _pair_masks(ctx, sizes, pairs, p_first, p_count, seed):
    from scape_amd._lib import P_i32, ptr
    s = np.array(sizes, dtype=np.int32)
    g, h = np.array([p[0] for p in pairs], dtype=np.int32), np.array([p[1] for p in pairs], dtype=np.int32)
    return ctx.lib.scape_hip_report_perm_pair_masks(ctx.h, len(s), ptr(s, P_i32), len(pairs), ptr(g, P_i32),
                                                    ptr(h, P_i32), p_first, p_count, seed)


def _pair_bits(ctx, pair, p, n):
    import ctypes
    from scape_amd._lib import check as chk
    w = np.zeros((n + 63) // 64, dtype=np.uint64)
    chk(ctx.lib.scape_hip_report_perm_pair_bits_get(ctx.h, pair, p, w.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))),
        "pair_bits_get")
    return w


def _mask_bits(ctx, p, n):
    import ctypes
    from scape_amd._lib import check as chk
    w = np.zeros((n + 63) // 64, dtype=np.uint64)
    chk(ctx.lib.scape_hip_report_perm_bits_get(ctx.h, p, w.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))), "bits_get")
    return w


@pytest.mark.gpu
@pytest.mark.parametrize("sizes", [(1, 1, 1), (1, 63, 64, 65, 7), (130, 140, 3)], ids=["1-1-1", "1-63-64-65-7", "130-140-3"])
@pytest.mark.parametrize("p_first", [1, 257])
def test_pair_masks(sizes, p_first):
    """pairs of 2, 8, 64, 65, 66, 70, 71, 72, 127, 128, 129 cells (one wave, across word edges), of 133 and 143 (one
    wave, four keys per lane) and of 270 (the radix select): the words of every pair and permutation equal the
    Python-int selection and the words of scape_hip_report_perm_masks on the pair's two sizes"""
    from scape_amd import _lib
    from scape_amd._lib import check as chk
    seed, p_count = 1234567, 300
    pairs = pair_list(len(sizes))
    ctx = _lib.default_context(None)
    try:
        chk(_pair_masks(ctx, sizes, pairs, p_first, p_count, seed), "pair_masks")
        for k, (g, h) in enumerate(pairs):
            n_g, n = sizes[g], sizes[g] + sizes[h]
            chk(ctx.lib.scape_hip_report_perm_masks(ctx.h, n_g, sizes[h], p_first, p_count, seed), "perm_masks")
            for p in range(p_count):
                member = np.zeros(n, dtype=bool)
                member[rc.members(seed, p_first + p, n_g, n)] = True
                got = _pair_bits(ctx, k, p, n)
                assert np.array_equal(got, _words(member)), (k, p)
                assert np.array_equal(got, _mask_bits(ctx, p, n)), (k, p)
    finally:
        ctx.lib.scape_hip_report_free(ctx.h)


@pytest.mark.gpu
def test_pair_masks_refusals():
    """every refused call returns non-zero with a message, before anything is released: the earlier bits stay"""
    import ctypes
    from scape_amd import _lib
    from scape_amd._lib import P_i32, check as chk, ptr
    ctx = _lib.default_context(None)
    lib = ctx.lib
    w = np.zeros(4, dtype=np.uint64)
    pw = w.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))
    try:
        lib.scape_hip_report_free(ctx.h)
        assert lib.scape_hip_report_perm_pair_bits_get(ctx.h, 0, 0, pw) != 0 and "pair_masks" in _lib.last_error()
        chk(_pair_masks(ctx, (3, 4, 5), pair_list(3), 1, 10, 7), "pair_masks")
        before = [_pair_bits(ctx, k, 9, 9) for k in range(3)]
        for sizes, pairs, p_first, p_count, word in (
                ((3,), [(0, 0)], 1, 1, "n_groups"), (tuple([1] * 65), [(0, 1)], 1, 1, "n_groups"),
                ((3, 0, 5), [(0, 1)], 1, 1, "at least one cell"), ((3, 4), [], 1, 1, "n_pairs"),
                ((3, 4), [(0, 1)] * 2017, 1, 1, "n_pairs"), ((3, 4, 5), [(1, 1)], 1, 1, "g < h"),
                ((3, 4, 5), [(2, 1)], 1, 1, "g < h"), ((3, 4, 5), [(0, 3)], 1, 1, "g < h"),
                ((3, 4, 5), [(-1, 1)], 1, 1, "g < h"), ((1 << 23, 1 << 23), [(0, 1)], 1, 1, "2^24"),
                ((3, 4), [(0, 1)], 0, 1, "p_first"), ((3, 4), [(0, 1)], 1, 0, "p_count")):
            assert _pair_masks(ctx, sizes, pairs, p_first, p_count, 7) != 0 and word in _lib.last_error(), (sizes, pairs)
        s = np.array([3, 4], dtype=np.int32)
        z = np.zeros(1, dtype=np.int32)
        assert lib.scape_hip_report_perm_pair_masks(ctx.h, 2, None, 1, ptr(z, P_i32), ptr(z, P_i32), 1, 1, 0) != 0
        assert lib.scape_hip_report_perm_pair_masks(ctx.h, 2, ptr(s, P_i32), 1, None, ptr(z, P_i32), 1, 1, 0) != 0
        assert lib.scape_hip_report_perm_pair_masks(None, 2, ptr(s, P_i32), 1, ptr(z, P_i32), ptr(z, P_i32), 1, 1, 0) != 0
        for k in range(3):                                           # a refused call keeps the earlier bits
            assert np.array_equal(_pair_bits(ctx, k, 9, 9), before[k])
        for pair, p in ((-1, 0), (3, 0), (0, -1), (0, 10)):
            assert lib.scape_hip_report_perm_pair_bits_get(ctx.h, pair, p, pw) != 0 and _lib.last_error() != ""
        assert lib.scape_hip_report_perm_pair_bits_get(ctx.h, 0, 0, None) != 0
    finally:
        lib.scape_hip_report_free(ctx.h)


# ---------------------------------------------------------------- GPU: the test entry point
@pytest.mark.gpu
@pytest.mark.parametrize("G", [2, 3, 5])
def test_entry_point(G):
    """scape_hip_report_perm_pairs on entry_case(): t, a0 and every counter equal the exact oracle (zero where a pair
    does not test a record or a row has no read in the pair); S(0) has the bits, and the counters the values, of
    scape_hip_report_perm_test on the pair's own two populations; the pairs in two ranges and the permutations in two
    chunks give the same totals; then the refusals"""
    from scape_amd import _lib
    from scape_amd._lib import P_d, P_i32, P_i64, check as chk, ptr
    Ks, off, lab, cb, dense, n_cols, seed, n_perm = entry_case()
    sizes = ENTRY_SIZES[G]
    seg = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    pairs = pair_list(G)
    rows, roff, res = entry_oracle(G)
    n_rows, n_rec, n_pairs = len(rows), len(Ks), len(pairs)
    site_want, gene_want = np.zeros((n_pairs, n_rows), np.int64), np.zeros((n_pairs, n_rec), np.int64)
    for k, pair in enumerate(res):
        for r, one in enumerate(pair):
            if one is not None:
                assert near_ties([one]) == []
                gene_want[k, r] = one["gene"][0]
                site_want[k, roff[r] + one["kept"]] = [c[0] for c in one["site"]]
    ctx = _lib.default_context(None)
    lib = ctx.lib

    def outs(m=n_pairs):
        return (np.full(n_rows, -1, np.int64), np.full((n_rows, G), -1, np.int64), np.zeros((m, n_rows), np.int64),
                np.full((m, n_rec), -1.0), np.zeros((m, n_rec), np.int64))

    def test(o, first=0, count=n_pairs, roff_=roff, seg_=seg, n_groups=G):
        return lib.scape_hip_report_perm_pairs(ctx.h, n_rec, ptr(roff_, P_i64), ptr(rows, P_i64), n_groups,
                                               ptr(seg_, P_i32), first, count, ptr(o[0], P_i64), ptr(o[1], P_i64),
                                               ptr(o[2], P_i64), ptr(o[3], P_d), ptr(o[4], P_i64))
    try:
        assert np.array_equal(rc.device_counts(ctx, Ks, off, lab, cb, n_cols), dense.sum(axis=1))
        chk(_pair_masks(ctx, sizes, pairs, 1, n_perm, seed), "pair_masks")
        one = outs()
        chk(test(one), "perm_pairs")
        sub = dense[rows]
        a0_want = np.stack([sub[:, seg[g]:seg[g + 1]].sum(axis=1) for g in range(G)], axis=1)
        for got, want, name in ((one[0], a0_want.sum(axis=1), "t"), (one[1], a0_want, "a0"), (one[2], site_want, "site_n_ge"),
                                (one[4], gene_want, "gene_n_ge")):
            print(name, "equal", np.array_equal(got, want))
            assert np.array_equal(got, want), name
        tested = np.array([[r is not None for r in pair] for pair in res])
        assert np.all(one[3][~tested] == 0.0)
        for k, pair in enumerate(res):
            want = np.array([float(r["S0"]) for r in pair if r is not None])
            assert np.allclose(one[3][k][tested[k]], want, rtol=1e-12, atol=0), k
        assert gene_want[tested].min() < gene_want[tested].max() and site_want.max() > 0
        if n_pairs >= 2:                                             # the pairs in two ranges
            cut = n_pairs // 2
            lo, hi = outs(cut), outs(n_pairs - cut)
            chk(test(lo, 0, cut), "perm_pairs")
            chk(test(hi, cut, n_pairs - cut), "perm_pairs")
            for j in (2, 3, 4):
                assert np.array_equal(np.concatenate([lo[j], hi[j]]), one[j]), j
        acc = outs()                                                 # the permutations in two chunks that accumulate
        for p_first, p_count in ((1, 100), (101, n_perm - 100)):
            chk(_pair_masks(ctx, sizes, pairs, p_first, p_count, seed), "pair_masks")
            chk(test(acc), "perm_pairs")
        assert np.array_equal(acc[2], site_want) and np.array_equal(acc[4], gene_want)
        assert np.array_equal(acc[3].view(np.uint64), one[3].view(np.uint64))
        # refusals: the group layout must be that of the pair masks call, the range one of its pairs
        o = outs()
        bad_seg = seg.copy()
        bad_seg[1] += 1
        assert test(o, seg_=bad_seg) != 0 and "seg_off differs" in _lib.last_error()
        assert test(o, n_groups=G + 1, seg_=np.concatenate([seg, [seg[-1] + 1]]).astype(np.int32)) != 0
        assert "n_groups differs" in _lib.last_error()
        for first, count in ((-1, 1), (0, 0), (0, n_pairs + 1), (n_pairs, 1)):
            assert test(o, first, count) != 0 and "pair_first" in _lib.last_error(), (first, count)
        bad_roff = roff.copy()
        bad_roff[1], bad_roff[2] = roff[2], roff[1]
        assert test(o, roff_=bad_roff) != 0 and "non-decreasing" in _lib.last_error()
        assert lib.scape_hip_report_perm_pairs(ctx.h, n_rec, ptr(roff, P_i64), ptr(rows, P_i64), G, ptr(seg, P_i32), 0,
                                               n_pairs, ptr(o[0], P_i64), ptr(o[1], P_i64), None, ptr(o[3], P_d),
                                               ptr(o[4], P_i64)) != 0
        assert test(outs()) == 0                                     # a refused call keeps masks and counts
        # scape_hip_report_perm_test on each pair's own two populations, their columns moved to the front
        for k, (g, h) in enumerate(pairs):
            front = list(range(seg[g], seg[g + 1])) + list(range(seg[h], seg[h + 1]))
            order = np.array(front + [c for c in range(n_cols) if c not in set(front)])
            col_of = np.empty(n_cols, dtype=np.int64)
            col_of[order] = np.arange(n_cols)
            rc.device_counts(ctx, Ks, off, lab, col_of[cb], n_cols)
            chk(lib.scape_hip_report_perm_masks(ctx.h, sizes[g], sizes[h], 1, n_perm, seed), "perm_masks")
            which = np.nonzero(tested[k])[0]
            rows_k = np.concatenate([rows[roff[r] + res[k][r]["kept"]] for r in which]).astype(np.int64)
            roff_k = np.concatenate([[0], np.cumsum([len(res[k][r]["kept"]) for r in which])]).astype(np.int64)
            t, a, site, gene = (np.zeros(len(rows_k), np.int64), np.zeros(len(rows_k), np.int64),
                                np.zeros(len(rows_k), np.int64), np.zeros(len(which), np.int64))
            stat = np.zeros(len(which))
            chk(lib.scape_hip_report_perm_test(ctx.h, len(which), ptr(roff_k, P_i64), ptr(rows_k, P_i64), ptr(t, P_i64),
                                               ptr(a, P_i64), ptr(site, P_i64), ptr(stat, P_d), ptr(gene, P_i64)),
                "perm_test")
            assert np.array_equal(stat.view(np.uint64), one[3][k][which].view(np.uint64)), (k, stat, one[3][k][which])
            assert np.array_equal(gene, one[4][k][which]), k
            assert np.array_equal(site, one[2][k][np.searchsorted(rows, rows_k)]), k
            assert np.array_equal(a, one[1][np.searchsorted(rows, rows_k), g]), k
        lib.scape_hip_report_free(ctx.h)
        assert test(outs()) != 0 and "report_counts" in _lib.last_error()
        rc.device_counts(ctx, Ks, off, lab, cb, n_cols)
        assert test(outs()) != 0 and "pair_masks" in _lib.last_error()   # counts, but no pair masks yet
    finally:
        lib.scape_hip_report_free(ctx.h)


@pytest.mark.gpu
def test_single_pair_is_perm_test_bit_for_bit():
    """rc.entry_point_matrix() as it stands, 70 + 91 cells, 300 permutations in one chunk: scape_hip_report_perm_test
    behind scape_hip_report_perm_masks(70, 91) and scape_hip_report_perm_pairs behind the pair masks of the single pair
    (0, 1), on the same rows, offsets and seed, return the same t, a0, counters and the same bits of S(0).  No row is
    passed over and no record skipped: every kept row has a read in the 161 columns, every record two such rows or more
    and reads in both populations (checked on the dense matrix first)"""
    from scape_amd import _lib
    from scape_amd._lib import P_d, P_i32, P_i64, check as chk, ptr
    n1, n2, n_cols, seed, n_perm, Ks, off, lab, cb, dense, rows, roff, _rng = rc.entry_point_matrix()
    sub = dense[rows]
    assert np.all(sub[:, :n1 + n2].sum(axis=1) > 0) and np.all(np.diff(roff) >= 2)
    A0, B0 = np.add.reduceat(sub[:, :n1].sum(axis=1), roff[:-1]), np.add.reduceat(sub[:, n1:n1 + n2].sum(axis=1), roff[:-1])
    assert np.all(A0 > 0) and np.all(B0 > 0)
    n_rows, n_rec = len(rows), len(Ks)
    seg = np.array([0, n1, n1 + n2], dtype=np.int32)
    ctx = _lib.default_context(None)
    lib = ctx.lib
    try:
        assert np.array_equal(rc.device_counts(ctx, Ks, off, lab, cb, n_cols), dense.sum(axis=1))
        t, a0, site, gene = (np.full(n_rows, -1, np.int64), np.full(n_rows, -1, np.int64), np.zeros(n_rows, np.int64),
                             np.zeros(n_rec, np.int64))
        stat = np.full(n_rec, -1.0)
        chk(lib.scape_hip_report_perm_masks(ctx.h, n1, n2, 1, n_perm, seed), "perm_masks")
        chk(lib.scape_hip_report_perm_test(ctx.h, n_rec, ptr(roff, P_i64), ptr(rows, P_i64), ptr(t, P_i64), ptr(a0, P_i64),
                                           ptr(site, P_i64), ptr(stat, P_d), ptr(gene, P_i64)), "perm_test")
        pt, pa0, psite, pgene = (np.full(n_rows, -1, np.int64), np.full((n_rows, 2), -1, np.int64),
                                 np.zeros((1, n_rows), np.int64), np.zeros((1, n_rec), np.int64))
        pstat = np.full((1, n_rec), -1.0)
        chk(_pair_masks(ctx, (n1, n2), [(0, 1)], 1, n_perm, seed), "pair_masks")
        chk(lib.scape_hip_report_perm_pairs(ctx.h, n_rec, ptr(roff, P_i64), ptr(rows, P_i64), 2, ptr(seg, P_i32), 0, 1,
                                            ptr(pt, P_i64), ptr(pa0, P_i64), ptr(psite, P_i64), ptr(pstat, P_d),
                                            ptr(pgene, P_i64)), "perm_pairs")
        assert np.array_equal(pt, t) and np.array_equal(t, sub[:, :n1 + n2].sum(axis=1))
        assert np.array_equal(pa0[:, 0], a0)
        assert np.array_equal(psite[0], site)
        assert np.array_equal(pgene[0], gene)
        assert np.array_equal(pstat[0].view(np.uint64), stat.view(np.uint64)) and np.all(stat > 0)
    finally:
        lib.scape_hip_report_free(ctx.h)


# ---------------------------------------------------------------- GPU: the command
def _blocks(text):
    """header check; {(group_1, group_2): the lines of that block}, the blocks in file order"""
    rows = list(csv.reader(io.StringIO(text)))
    assert rows[0] == HEADER
    out, last = {}, None
    for r in rows[1:]:
        key = (r[2], r[3])
        assert key == last or key not in out                         # a pair's lines are one contiguous block
        out.setdefault(key, []).append(r)
        last = key
    return out


def _diff_pa_rows(root, clu, id1, id2, n_perm, seed):
    return list(csv.reader(io.StringIO(rc.perm_command("diff_pa", root, clu, "res.gene.pkl", id1, id2, n_perm, seed))))[1:]


ADJ = (HEADER.index("p_val_adj"), HEADER.index("gene_p_val_adj"))


def _shared(diff_pa_row):
    """a line of diff_pa's layout without its two adjusted p-values"""
    return [v for j, v in enumerate(diff_pa_row) if j + 2 not in ADJ]


def _assert_blocks_are_diff_pa(root, clu, text, names, n_perm, seed):
    """every pair's block equals diff_pa's file on that pair as text, the two adjusted p-values left aside; those equal
    rc.bh over all lines and over all (pair, record) combinations of the file.  Returns the blocks"""
    blocks = _blocks(text)
    want_keys = []
    for g, h in pair_list(len(names)):
        want = _diff_pa_rows(root, clu, names[g], names[h], n_perm, seed)
        if want:
            want_keys.append((names[g], names[h]))
            got = blocks[want_keys[-1]]
            assert len(got) == len(want)
            for a, b in zip(got, want):
                assert _shared(a[:2] + a[4:]) == _shared(b), (a, b)
    assert list(blocks) == want_keys
    body = [r for b in blocks.values() for r in b]
    ix = {name: HEADER.index(name) for name in ("n_ge", "gene_n_ge", "gene")}
    p_site = rc.bh([Fraction(1 + int(r[ix["n_ge"]]), 1 + n_perm) for r in body])
    genes = list(dict.fromkeys((r[2], r[3], r[0]) for r in body))
    first = {k: next(r for r in body if (r[2], r[3], r[0]) == k) for k in genes}
    p_gene = dict(zip(genes, rc.bh([Fraction(1 + int(first[k][ix["gene_n_ge"]]), 1 + n_perm) for k in genes])))
    for r, want in zip(body, p_site):
        assert rc.close(r[ADJ[0]], want) and rc.close(r[ADJ[1]], p_gene[(r[2], r[3], r[0])]), r
    return blocks


@pytest.mark.gpu
def test_synthetic_directory(tmp_path):
    """A (230 cells), B (301) and C (40) in the cluster file's order, 257 permutations: three blocks, each diff_pa's file on that pair; the counts of
    every block equal the exact oracle; G = 2 gives exactly one block; the idents reversed swap the sign and the .1 / .2
    columns"""
    clu = rc.write_synthetic(tmp_path)
    text = _command(tmp_path, clu, "res.gene.pkl", (), SYN_PERM, SYN_SEED)
    names = syn_names()
    blocks = _assert_blocks_are_diff_pa(tmp_path, clu, text, names, SYN_PERM, SYN_SEED)
    assert list(blocks) == [(names[g], names[h]) for g, h in pair_list(3)]
    rec_rows, _bc, _clu_text = syn_rec_rows()
    ix = {name: HEADER.index(name) for name in ("n_ge", "gene_n_ge", "versus")}
    for (a, b), got in blocks.items():
        res = syn_pair_oracle(a, b)
        assert near_ties(res) == []
        want = [(gene, rows[i][0], r["site"][j][0], r["gene"][0]) for (gene, rows), r in zip(rec_rows, res) if r is not None
                for j, i in enumerate(r["kept"].tolist())]
        assert [(r[0], r[1], int(r[ix["n_ge"]]), int(r[ix["gene_n_ge"]])) for r in got] == want, (a, b)
        assert {r[ix["versus"]] for r in got} == {f"{a}_Vs_{b}"} and len(got) > 100
    two = _command(tmp_path, clu, "res.gene.pkl", ("A", "B"), SYN_PERM, SYN_SEED)
    one = _assert_blocks_are_diff_pa(tmp_path, clu, two, ("A", "B"), SYN_PERM, SYN_SEED)
    assert list(one) == [("A", "B")]
    same = blocks.get(("A", "B")) or blocks[("B", "A")]
    assert len(same) == len(one[("A", "B")]) and [r[:2] for r in same] == [r[:2] for r in one[("A", "B")]]
    back = _assert_blocks_are_diff_pa(tmp_path, clu, _command(tmp_path, clu, "res.gene.pkl", ("B", "A"), SYN_PERM, SYN_SEED),
                                      ("B", "A"), SYN_PERM, SYN_SEED)
    if ("B", "A") in blocks:                       # the same pair alone and among three: only the adjustments differ
        assert [_shared(r[:2] + r[4:]) for r in back[("B", "A")]] == [_shared(r[:2] + r[4:]) for r in blocks[("B", "A")]]
    c = {name: HEADER.index(name) for name in ("pct.1", "pct.2", "usage.1", "usage.2", "delta_usage")}
    assert len(back[("B", "A")]) == len(one[("A", "B")])
    for r, s in zip(back[("B", "A")], one[("A", "B")]):
        assert r[:2] == s[:2] and (r[c["pct.1"]], r[c["usage.1"]]) == (s[c["pct.2"]], s[c["usage.2"]])
        assert (r[c["pct.2"]], r[c["usage.2"]]) == (s[c["pct.1"]], s[c["usage.1"]])
        assert float(r[c["delta_usage"]]) == -float(s[c["delta_usage"]])


@pytest.mark.gpu
@pytest.mark.parametrize("n_perm", [1, 255, 256, 257])
def test_tile_edges(n_perm, tmp_path):
    """a workgroup of the test kernel takes 256 permutations: one, one short of a tile, a full tile, one over"""
    clu = rc.write_synthetic(tmp_path, 12)
    text = _command(tmp_path, clu, "res.gene.pkl", (), n_perm, 5)
    assert len(_assert_blocks_are_diff_pa(tmp_path, clu, text, syn_names(), n_perm, 5)) == 3


@pytest.mark.gpu
def test_batch_chunk_and_range_invariance(tmp_path, monkeypatch):
    """records over several count batches, the permutations over several chunks, the pairs over several ranges: the
    same bytes"""
    from scape_amd import _lib, report
    clu = rc.write_synthetic(tmp_path)
    big = _command(tmp_path, clu, "res.gene.pkl", (), SYN_PERM, SYN_SEED)
    lib = _lib.load_library()
    calls = {"masks": [], "test": []}
    real_m, real_t = lib.scape_hip_report_perm_pair_masks, lib.scape_hip_report_perm_pairs

    def masks(*a):
        calls["masks"].append((a[6], a[7]))
        return real_m(*a)

    def test(*a):
        calls["test"].append((a[6], a[7]))
        return real_t(*a)
    monkeypatch.setattr(lib, "scape_hip_report_perm_pair_masks", masks)
    monkeypatch.setattr(lib, "scape_hip_report_perm_pairs", test)
    assert _command(tmp_path, clu, "res.gene.pkl", (), SYN_PERM, SYN_SEED) == big
    assert calls["masks"] == [(1, SYN_PERM)] and calls["test"] == [(0, 3)]
    calls.update(masks=[], test=[])
    monkeypatch.setattr(report, "MAX_BATCH_BYTES", 1 << 16)             # a record of K = 8 alone takes 57 KB
    monkeypatch.setattr(report, "MAX_PERM_BYTES", 1 << 30)
    assert _command(tmp_path, clu, "res.gene.pkl", (), SYN_PERM, SYN_SEED) == big
    assert calls["masks"] == [(1, SYN_PERM)] and len(calls["test"]) > 5
    n_batches = len(calls["test"])
    calls.update(masks=[], test=[])
    # per permutation: pairs of 531, 270 and 341 cells = 9 + 5 + 6 words and 3 key bounds; room for 100 permutations
    monkeypatch.setattr(report, "MAX_PERM_BYTES", (20 + 3) * 8 * 100)
    assert _command(tmp_path, clu, "res.gene.pkl", (), SYN_PERM, SYN_SEED) == big
    assert len(calls["test"]) == 3 * n_batches and calls["masks"][:3] == [(1, 100), (101, 100), (201, 57)]
    calls.update(masks=[], test=[])
    monkeypatch.setattr(report, "MAX_PERM_BYTES", 1 << 30)
    monkeypatch.setattr(report, "MAX_PAIR_RESULT_BYTES", 1)            # one pair per call
    assert _command(tmp_path, clu, "res.gene.pkl", (), SYN_PERM, SYN_SEED) == big
    assert calls["test"][:3] == [(0, 1), (1, 1), (2, 1)] and len(calls["test"]) == 3 * n_batches


@pytest.mark.gpu
def test_failed_run_leaves_no_part_file(tmp_path, monkeypatch):
    from scape_amd import _lib
    clu = rc.write_synthetic(tmp_path, 12)
    lib = _lib.load_library()
    monkeypatch.setattr(lib, "scape_hip_report_perm_pairs", lambda *a: 1)
    r = rc.run(_args(tmp_path, clu, n_perm=10))
    assert r.exit_code != 0 and isinstance(r.exception, _lib.ScapeHipError), repr(r.exception)
    assert not rc.parts_left(tmp_path) and not os.path.exists(_path(tmp_path, clu, "res.gene.pkl"))
