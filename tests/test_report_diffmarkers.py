"""`scape diff_pa_markers`: diff_pa of every cluster against all other clustered cells, from one pass over the result
file (scape_amd/report.py, section diff_pa_markers; kernels k_rep_perm_marker_masks and k_rep_perm_markers of
scape_amd/csrc/perm.inc).

The contract is "marker X is exactly `diff_pa --idents_1 X`", so the yardsticks are diff_pa's: the Python-int `key` and
`members` of tests/report_cases.py, the exact oracle of tests/test_report_diffpa.py in the form that
tests/test_report_diffpairs.py restates for a whole matrix of labellings (pair_oracle, Python ints in object arrays,
held against the _Rec oracle by that file's test_pair_oracle_is_the_diff_pa_oracle), and the entry points and the command
of diff_pa themselves.  What is new here is the place of a marker's bits: the device keeps them in the order of the
count matrix's columns (slots) and finds the local position diff_pa would give a slot from the rank of its column;
local_positions below restates that map, and test_local_positions_are_diff_pa_s holds it against diff_pa's own
populations.  The oracle gives lo = #{stat(p) >= stat(0)} and hi = #{stat(p) >= stat(0) (1 - 2^-39)};
test_entry_oracle_has_no_near_tie asserts lo == hi for every case the GPU test compares with it, which then asserts
that the device's counts EQUAL lo."""
import csv
import ctypes
import functools
import io
import os
from fractions import Fraction

import numpy as np
import pytest

import report_cases as rc
import test_report_diffpa as dp
import test_report_diffpairs as dpp
from report_cases import no_gpu  # noqa: F401  (fixture)
from test_report_strata import select_passes

HEADER = ["gene", "pa_info", "group"] + dp.HEADER.split(",")[2:]
NAMES = ("scape_hip_report_perm_marker_masks", "scape_hip_report_perm_marker_bits_get", "scape_hip_report_perm_markers")


# ---------------------------------------------------------------- the contract, restated
def local_positions(sizes, rank, g):
    """the local position diff_pa gives every slot when marker g is its population 1: g's own slots 0 .. n_g - 1 in
    order, every other slot n_g + its column's rank among the tested columns - the columns of g below that column"""
    seg = np.concatenate([[0], np.cumsum(sizes)])
    rank = np.asarray(rank, dtype=np.int64)
    mine = rank[seg[g]:seg[g + 1]]
    out = sizes[g] + rank - np.searchsorted(mine, rank)
    out[seg[g]:seg[g + 1]] = np.arange(sizes[g])
    return out


def slot_members(seed, p, sizes, rank, g):
    """boolean membership of marker g's population under permutation p, per slot: rc.members on the local positions"""
    chosen = np.zeros(len(rank), dtype=bool)
    chosen[rc.members(seed, p, sizes[g], len(rank))] = True
    return chosen[local_positions(sizes, rank, g)]


def layout(sizes, n_others, gen_seed=1):
    """the columns 0 .. n - 1 dealt to the markers and the others at random: (columns of every segment ascending, the
    others' last; orig_rank = the column of every slot).  Never the identity"""
    counts = list(sizes) + [n_others]
    while True:
        seg_of = np.random.default_rng(gen_seed).permutation(np.repeat(np.arange(len(counts)), counts))
        cols = [np.nonzero(seg_of == g)[0] for g in range(len(counts))]
        rank = np.concatenate(cols).astype(np.int32)
        if not np.array_equal(rank, np.arange(len(rank))):
            return cols, rank
        gen_seed += 1


# ---------------------------------------------------------------- the cases the GPU test compares with the oracle
ENTRY_CASES = {"70-50-41": ((70, 50, 41), 0), "70-60+31": ((70, 60), 31)}
ENTRY_PERMS = (1, 257)


@functools.lru_cache(maxsize=None)
def entry_oracle(case):
    """rc.entry_point_matrix() with its 161 tested columns dealt to the markers (and others) of ENTRY_CASES[case]:
    (columns per segment, orig_rank, {n_perm: per marker dpp.pair_oracle of the kept rows on diff_pa's layout})"""
    n1, n2, _n_cols, seed, _n_perm, _Ks, _off, _lab, _cb, dense, rows, roff, _rng = rc.entry_point_matrix()
    sizes, n_others = ENTRY_CASES[case]
    assert sum(sizes) + n_others == n1 + n2
    cols, rank = layout(sizes, n_others)
    res = {}
    for n_perm in ENTRY_PERMS:
        res[n_perm] = []
        for g in range(len(sizes)):
            rest = np.setdiff1d(np.arange(n1 + n2), cols[g])
            order = np.concatenate([cols[g], rest])
            mats = [dense[rows[roff[r]:roff[r + 1]]][:, order] for r in range(len(roff) - 1)]
            res[n_perm].append(dpp.pair_oracle(mats, sizes[g], n1 + n2 - sizes[g], n_perm, seed))
    return cols, rank, res


# ---------------------------------------------------------------- CPU
def _args(root, clu, res="res.gene.pkl", idents=(), n_perm=None, seed=None):
    a = ["diff_pa_markers", "--output_dir", str(root), "--res_pkl_file", res, "--cell_cluster_file", str(clu)]
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
    return os.path.join(str(root), f"{stem}.{kind}{tag}.diff_pa_markers.csv")


def _command(root, clu, res, idents, n_perm, seed, what=""):
    r = rc.run(_args(root, clu, res, idents, n_perm, seed))
    assert r.exit_code == 0, (what, r.output, repr(r.exception))
    assert not rc.parts_left(root)
    with open(_path(root, clu, res, idents), newline="") as fh:
        return fh.read()


def test_help_and_import_path():
    r = rc.run(["--help"])
    assert r.exit_code == 0 and "diff_pa_markers" in r.output
    r = rc.run(["diff_pa_markers", "--help"])
    assert r.exit_code == 0, r.output
    for o in ("--output_dir", "--res_pkl_file", "--cell_cluster_file", "--idents", "--n_perm", "--seed"):
        assert o in r.output
    assert "--idents_1" not in r.output and "--strata_file" not in r.output
    flat = " ".join(r.output.split())
    assert "[default: 9999]" in flat and "[default: 1]" in flat
    import scape.utils as su
    from scape_amd import _lib, report
    assert su.diff_pa_markers is report.diff_pa_markers
    assert all(name in _lib.SIGNATURES for name in NAMES)
    assert report.DIFF_PA_MARKERS_HEADER == HEADER
    assert report.DIFF_PA_MARKERS_HEADER[:2] + report.DIFF_PA_MARKERS_HEADER[3:] == report.DIFF_PA_HEADER


def test_prerequisites_and_argument_errors(tmp_path, no_gpu):
    """diff_pa_len_groups's list of errors, with this command's name in the messages, before the device is opened; one
    ident is a run, 65 clusters need --idents, and a marker that holds every clustered cell has no rest"""
    from scape_amd import report
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
    for extra, word in ((["--idents", "A", "--idents", "Z"], "'Z'"), (["--idents", "A", "--idents", "A"], "twice"),
                        (["--idents", "A", "--idents", "ghost"], "has no cell"),
                        (["--idents", "A", "--idents", ""], "names no cluster"),
                        (["--idents", "A", "--idents", "a/b"], "file name"),
                        (["--n_perm", "0"], "n_perm"), (["--n_perm", str(1 << 31)], "n_perm"),
                        (["--seed", "-1"], "seed"), (["--seed", str(1 << 64)], "seed")):
        r = rc.run(_args(tmp_path, clu) + extra)
        assert isinstance(r.exception, ValueError) and word in str(r.exception), (extra, repr(r.exception))
    one = report._groups_setup(str(tmp_path), "res.gene.pkl", str(clu), ("B",), 9, 1, "diff_pa_markers", markers=True)
    assert one.names == ["B"] and one.n == 3 and one.seg_off.tolist() == [0, 1, 3]      # one ident is accepted
    assert one.outpath.endswith("groups.gene.B.diff_pa_markers.csv")
    ids = list(range(100, 166))
    (tmp_path / "barcode_index.csv").write_text("CB,index\n" + "".join(f"C{i}-1,{i}\n" for i in ids))
    clu.write_text("index,group\n" + "".join(f"{i},g{i}\n" for i in ids[:65]))
    r = rc.run(_args(tmp_path, clu))
    assert isinstance(r.exception, ValueError) and "65 clusters: diff_pa_markers" in str(r.exception)
    assert "--idents" in str(r.exception)
    two = report._groups_setup(str(tmp_path), "res.gene.pkl", str(clu), ("g101", "g100"), 9, 1, "diff_pa_markers",
                               markers=True)
    assert two.names == ["g101", "g100"] and two.n == 65 and two.seg_off.tolist() == [0, 1, 2, 65]
    clu.write_text("index,group\n" + "".join(f"{i},only\n" for i in ids[:40]) + f"{ids[50]},\n")
    for extra in ([], ["--idents", "only"]):
        r = rc.run(_args(tmp_path, clu) + extra)
        assert isinstance(r.exception, ValueError) and "the rest has no cell" in str(r.exception), repr(r.exception)
    r = rc.run(["diff_pa_markers", "--output_dir", str(tmp_path), "--res_pkl_file", "res.gene.pkl"])
    assert r.exit_code == 2 and "--cell_cluster_file" in r.output
    r = rc.run(_args(tmp_path, clu) + ["--strata_file", str(clu)])
    assert r.exit_code == 2 and "--strata_file" in r.output
    assert sorted(os.listdir(tmp_path)) == ["barcode_index.csv", "groups.csv", "res.gene.pkl"]


INTERLEAVED = "BAC.ABBCA.CCAB.DADB"      # the cluster of every column of a hand-made barcode file; "." = none


def test_local_positions_are_diff_pa_s(tmp_path):
    """a cluster file with interleaved columns: for every marker, the columns that the slot-order membership selects
    are the columns diff_pa's own two populations give when ranked directly, with every cluster a marker (no others)
    and with two named in reversed order (the others hold two clusters); the host's layout is the one restated"""
    from scape_amd import report
    ids = [11 + 3 * j for j in range(len(INTERLEAVED))]
    bc = "CB,index\n" + "".join(f"X{j}-1,{i}\n" for j, i in enumerate(ids))
    clu = "index,group\n" + "".join(f"{i},{'' if c == '.' else c}\n" for i, c in zip(reversed(ids), reversed(INTERLEAVED)))
    col_clu = np.array(list(INTERLEAVED))
    tested = np.nonzero(col_clu != ".")[0]
    seed = 5
    (tmp_path / "res.gene.pkl").write_bytes(b"")
    (tmp_path / "barcode_index.csv").write_text(bc)
    (tmp_path / "m.csv").write_text(clu)
    assert rc.first_clusters(clu) == ["B", "D", "A", "C"]
    for idents, markers in (((), ["B", "D", "A", "C"]), (("C", "A"), ["C", "A"])):
        cols = [np.nonzero(col_clu == m)[0] for m in markers]
        others = np.setdiff1d(tested, np.concatenate(cols))
        assert (len(others) > 0) == bool(idents)
        slot_col = np.concatenate(cols + [others])
        rank = np.searchsorted(tested, slot_col)
        sizes = [len(c) for c in cols]
        su = report._groups_setup(str(tmp_path), "res.gene.pkl", str(tmp_path / "m.csv"), idents, 9, seed,
                                  "diff_pa_markers", markers=True)
        assert su.names == markers and su.sizes.tolist() == sizes and su.n == len(tested)
        assert su.seg_off.tolist() == np.concatenate([[0], np.cumsum(sizes), [len(tested)]]).tolist()
        assert su.idmap.table[np.array(ids)[slot_col] - su.idmap.id_min].tolist() == list(range(len(tested)))
        for g, m in enumerate(markers):
            c1, c2 = rc.populations(bc, clu, m, None)
            assert c1 == cols[g].tolist() and sorted(c1 + c2) == tested.tolist()
            loc = local_positions(sizes, rank, g)
            assert sorted(loc.tolist()) == list(range(len(tested)))
            assert [(c1 + c2)[k] for k in loc.tolist()] == slot_col.tolist()
            for p in (1, 2, 77):
                want = sorted((c1 + c2)[k] for k in rc.members(seed, p, len(c1), len(tested)))
                assert sorted(slot_col[slot_members(seed, p, sizes, rank, g)].tolist()) == want, (m, p)


def test_entry_oracle_has_no_near_tie():
    """no permuted statistic of the cases test_entry_point compares with the oracle lies within 2^-39 below the
    observed one, for every marker, after 1 and after 257 permutations; every marker tests every record, the records of
    70 and 150 rows among them, and a record count lies strictly inside 0 .. 257"""
    roff = rc.entry_point_matrix()[11]
    assert sorted(np.diff(roff).tolist())[-2] > 64 and np.diff(roff).max() > 128
    for case in ENTRY_CASES:
        _cols, rank, res = entry_oracle(case)
        assert not np.array_equal(rank, np.arange(len(rank)))
        for n_perm in ENTRY_PERMS:
            for g, one in enumerate(res[n_perm]):
                assert all(r is not None for r in one), (case, g)
                assert dpp.near_ties(one) == [], (case, n_perm, g)
        assert any(0 < r["gene"][0] < 257 for one in res[257] for r in one), case


# ---------------------------------------------------------------- GPU: the membership bits
def _marker_masks(ctx, sizes, n_others, rank, p_first, p_count, seed, n_markers=None):
    from scape_amd._lib import P_i32, ptr
    s, r = np.array(sizes, dtype=np.int32), np.array(rank, dtype=np.int32)
    return ctx.lib.scape_hip_report_perm_marker_masks(ctx.h, len(s) if n_markers is None else n_markers, ptr(s, P_i32),
                                                      n_others, ptr(r, P_i32), p_first, p_count, seed)


def _marker_bits(ctx, marker, p, n):
    from scape_amd._lib import check as chk
    w = np.zeros((n + 63) // 64, dtype=np.uint64)
    chk(ctx.lib.scape_hip_report_perm_marker_bits_get(ctx.h, marker, p, w.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))),
        "marker_bits_get")
    return w


SMALL_CHUNKS = ((1, 1), (1, 257), (200, 3))
MASK_CASES = [((1, 1), 0, 1234567, SMALL_CHUNKS), ((3, 60, 1), 0, 1234567, SMALL_CHUNKS),
              ((70, 60), 31, 1234567, SMALL_CHUNKS), ((100, 156), 0, 1234567, SMALL_CHUNKS),
              ((100, 157), 0, 1234567, SMALL_CHUNKS), ((1500, 2500), 0, 3, ((25, 4), (3128, 4)))]


@pytest.mark.gpu
@pytest.mark.parametrize("sizes,n_others,seed,chunks", MASK_CASES,
                         ids=["1-1", "3-60-1", "70-60+31", "100-156", "100-157", "1500-2500"])
def test_marker_masks(sizes, n_others, seed, chunks):
    """n = 2, 64 (one word), 161 (one wave, four keys per lane), 256 (the largest wave), 257 (the smallest select) and
    4,000 cells (chunks that hold a select of 3 and of 4 passes at rank 1,499, asserted first), the columns dealt to the
    segments at random: the slot-order words of every marker and permutation equal the Python membership"""
    from scape_amd import _lib
    from scape_amd._lib import check as chk
    n = sum(sizes) + n_others
    _cols, rank = layout(sizes, n_others)
    seg = np.cumsum(sizes)
    assert n < 128 or any(a // 64 != (b - 1) // 64 for a, b in zip([0] + seg.tolist(), seg.tolist()))
    if n == 4000:
        for (p_first, p_count), passes in zip(chunks, (3, 4)):
            deep = [select_passes([rc.key(seed, p, j) for j in range(n)], sizes[0] - 1)
                    for p in range(p_first, p_first + p_count)]
            assert max(deep) == passes, (p_first, deep)
    ctx = _lib.default_context(None)
    try:
        for p_first, p_count in chunks:
            chk(_marker_masks(ctx, sizes, n_others, rank, p_first, p_count, seed), "marker_masks")
            for g in range(len(sizes)):
                for p in range(p_count):
                    member = slot_members(seed, p_first + p, sizes, rank, g)
                    assert member.sum() == sizes[g]
                    assert np.array_equal(_marker_bits(ctx, g, p, n), dpp._words(member)), (g, p_first, p)
    finally:
        ctx.lib.scape_hip_report_free(ctx.h)


# ---------------------------------------------------------------- GPU: the test entry point
@pytest.mark.gpu
@pytest.mark.parametrize("case", list(ENTRY_CASES))
def test_entry_point(case):
    """scape_hip_report_perm_markers on rc.entry_point_matrix(), its 161 tested columns dealt to the markers at random:
    after permutation 1 and after 257 permutations t, a0 and every counter equal the exact oracle for every marker; the
    markers in two ranges give the same; and S(0) has the bits, the counters the values, of
    scape_hip_report_perm_masks + scape_hip_report_perm_test on the count matrix laid out as diff_pa lays it out"""
    from scape_amd import _lib
    from scape_amd._lib import P_d, P_i32, P_i64, check as chk, ptr
    _n1, _n2, n_cols, seed, _n_perm, Ks, off, lab, cb, dense, rows, roff, _rng = rc.entry_point_matrix()
    sizes, n_others = ENTRY_CASES[case]
    cols, rank, res = entry_oracle(case)
    M, n, n_rows, n_rec = len(sizes), len(rank), len(rows), len(Ks)
    n_seg = M + 1
    seg = np.concatenate([[0], np.cumsum(sizes), [n]]).astype(np.int32)

    def to_front(front):
        order = np.concatenate([front, np.setdiff1d(np.arange(n_cols), front)])
        col_of = np.empty(n_cols, dtype=np.int64)
        col_of[order] = np.arange(n_cols)
        return col_of

    def want(n_perm):
        site, gene = np.zeros((M, n_rows), np.int64), np.zeros((M, n_rec), np.int64)
        for g, one in enumerate(res[n_perm]):
            for r, rec in enumerate(one):
                gene[g, r] = rec["gene"][0]
                site[g, roff[r]:roff[r + 1]] = [c[0] for c in rec["site"]]
        return site, gene
    ctx = _lib.default_context(None)
    lib = ctx.lib

    def outs(m=M):
        return (np.full(n_rows, -1, np.int64), np.full((n_rows, n_seg), -1, np.int64), np.zeros((m, n_rows), np.int64),
                np.full((m, n_rec), -1.0), np.zeros((m, n_rec), np.int64))

    def test(o, first=0, count=M, seg_=seg, n_seg_=n_seg):
        return lib.scape_hip_report_perm_markers(ctx.h, n_rec, ptr(roff, P_i64), ptr(rows, P_i64), n_seg_,
                                                 ptr(seg_, P_i32), first, count, ptr(o[0], P_i64), ptr(o[1], P_i64),
                                                 ptr(o[2], P_i64), ptr(o[3], P_d), ptr(o[4], P_i64))
    try:
        assert test(outs()) != 0 and "report_counts" in _lib.last_error()
        rc.device_counts(ctx, Ks, off, lab, to_front(rank)[cb], n_cols)
        assert test(outs()) != 0 and "marker_masks" in _lib.last_error()     # counts, but no marker masks yet
        sub = dense[rows][:, rank]
        a0_want = np.stack([sub[:, seg[g]:seg[g + 1]].sum(axis=1) for g in range(n_seg)], axis=1)
        acc, split = outs(), (outs(1), outs(M - 1))
        for (p_first, p_count), n_perm in zip(((1, 1), (2, 256)), ENTRY_PERMS):
            chk(_marker_masks(ctx, sizes, n_others, rank, p_first, p_count, seed), "marker_masks")
            chk(test(acc), "perm_markers")
            chk(test(split[0], 0, 1), "perm_markers")
            chk(test(split[1], 1, M - 1), "perm_markers")
            site_want, gene_want = want(n_perm)
            for got, exp, name in ((acc[0], sub.sum(axis=1), "t"), (acc[1], a0_want, "a0"), (acc[2], site_want, "site_n_ge"),
                                   (acc[4], gene_want, "gene_n_ge")):
                print(n_perm, name, "equal", np.array_equal(got, exp))
                assert np.array_equal(got, exp), (n_perm, name)
            for j in (2, 3, 4):
                assert np.array_equal(np.concatenate([split[0][j], split[1][j]]), acc[j]), (n_perm, j)
        for g, one in enumerate(res[257]):
            assert np.allclose(acc[3][g], [float(r["S0"]) for r in one], rtol=1e-12, atol=0), g
        # refusals: the segments must be those of the marker masks call, the range one of its markers
        o = outs()
        bad_seg = seg.copy()
        bad_seg[1] += 1
        assert test(o, seg_=bad_seg) != 0 and "seg_off differs" in _lib.last_error()
        assert test(o, n_seg_=M, seg_=seg[:-1].copy()) != 0 and "n_groups differs" in _lib.last_error()
        for first, count in ((-1, 1), (0, 0), (0, M + 1), (M, 1)):
            assert test(o, first, count) != 0 and "marker_first" in _lib.last_error(), (first, count)
        assert lib.scape_hip_report_perm_markers(ctx.h, n_rec, ptr(roff, P_i64), ptr(rows, P_i64), n_seg, ptr(seg, P_i32),
                                                 0, M, ptr(o[0], P_i64), ptr(o[1], P_i64), None, ptr(o[3], P_d),
                                                 ptr(o[4], P_i64)) != 0
        # diff_pa's own entry points, marker by marker, on diff_pa's layout of the columns
        for g in range(M):
            rc.device_counts(ctx, Ks, off, lab, to_front(np.concatenate([cols[g], np.setdiff1d(np.arange(n), cols[g])]))[cb],
                             n_cols)
            t, a, site, gene = (np.zeros(n_rows, np.int64), np.zeros(n_rows, np.int64), np.zeros(n_rows, np.int64),
                                np.zeros(n_rec, np.int64))
            stat = np.zeros(n_rec)
            for p_first, p_count in ((1, 1), (2, 256)):
                chk(lib.scape_hip_report_perm_masks(ctx.h, sizes[g], n - sizes[g], p_first, p_count, seed), "perm_masks")
                chk(lib.scape_hip_report_perm_test(ctx.h, n_rec, ptr(roff, P_i64), ptr(rows, P_i64), ptr(t, P_i64),
                                                   ptr(a, P_i64), ptr(site, P_i64), ptr(stat, P_d), ptr(gene, P_i64)),
                    "perm_test")
            assert np.array_equal(stat.view(np.uint64), acc[3][g].view(np.uint64)), (g, stat, acc[3][g])
            assert np.array_equal(gene, acc[4][g]) and np.array_equal(site, acc[2][g]), g
            assert np.array_equal(a, acc[1][:, g]) and np.array_equal(t, acc[0]), g
    finally:
        lib.scape_hip_report_free(ctx.h)


@pytest.mark.gpu
def test_entry_point_refusals():
    """every check of the masks call returns non-zero with a message before anything is released, so the earlier bits
    stay; bits_get refuses a marker or a permutation outside the last call.  (The bound of 2^31 mask words cannot be
    reached while n < 2^24 and at most 64 markers are taken: 64 x 2^18 words.)"""
    from scape_amd import _lib
    from scape_amd._lib import P_i32, check as chk, ptr
    ctx = _lib.default_context(None)
    lib = ctx.lib
    w = np.zeros(4, dtype=np.uint64)
    pw = w.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))
    try:
        lib.scape_hip_report_free(ctx.h)
        assert lib.scape_hip_report_perm_marker_bits_get(ctx.h, 0, 0, pw) != 0 and "marker_masks" in _lib.last_error()
        sizes, n_others = (3, 4), 5
        _cols, rank = layout(sizes, n_others)
        chk(_marker_masks(ctx, sizes, n_others, rank, 1, 10, 7), "marker_masks")
        before = [_marker_bits(ctx, g, 9, 12) for g in range(2)]
        twice, outside, down = rank.copy(), rank.copy(), rank.copy()
        twice[5] = twice[4]
        outside[0] = 12
        down[[0, 1]] = down[[1, 0]]
        for s, others, r, p_first, p_count, n_markers, word in (
                ((3, 4), 5, rank, 1, 1, 0, "n_markers"), ((1,) * 65, 5, np.arange(70), 1, 1, None, "n_markers"),
                ((3, 0), 5, rank, 1, 1, None, "at least one cell"), ((3, 4), -1, rank, 1, 1, None, "n_others"),
                ((1,), 0, [0], 1, 1, None, "at least 2"), ((1 << 23, 1 << 23), 0, [0], 1, 1, None, "2^24"),
                ((12,), 0, np.arange(12), 1, 1, None, "every tested cell"),
                ((3, 4), 5, twice, 1, 1, None, "permutation"), ((3, 4), 5, outside, 1, 1, None, "permutation"),
                ((3, 4), 5, -rank - 1, 1, 1, None, "permutation"), ((3, 4), 5, down, 1, 1, None, "ascend"),
                ((3, 4), 5, rank, 0, 1, None, "p_first"), ((3, 4), 5, rank, 1, 0, None, "p_count")):
            assert _marker_masks(ctx, s, others, r, p_first, p_count, 7, n_markers) != 0, (s, others, word)
            assert word in _lib.last_error(), (word, _lib.last_error())
        s = np.array(sizes, dtype=np.int32)
        assert lib.scape_hip_report_perm_marker_masks(ctx.h, 2, None, 5, ptr(rank, P_i32), 1, 1, 0) != 0
        assert lib.scape_hip_report_perm_marker_masks(ctx.h, 2, ptr(s, P_i32), 5, None, 1, 1, 0) != 0
        assert lib.scape_hip_report_perm_marker_masks(None, 2, ptr(s, P_i32), 5, ptr(rank, P_i32), 1, 1, 0) != 0
        for g in range(2):                                           # a refused call keeps the earlier bits
            assert np.array_equal(_marker_bits(ctx, g, 9, 12), before[g])
        for marker, p in ((-1, 0), (2, 0), (0, -1), (0, 10)):
            assert lib.scape_hip_report_perm_marker_bits_get(ctx.h, marker, p, pw) != 0 and _lib.last_error() != ""
        assert lib.scape_hip_report_perm_marker_bits_get(ctx.h, 0, 0, None) != 0
    finally:
        lib.scape_hip_report_free(ctx.h)


# ---------------------------------------------------------------- GPU: the command
ADJ = (HEADER.index("p_val_adj"), HEADER.index("gene_p_val_adj"))


def _blocks(text):
    """header check; {marker: the lines of its block}, the blocks in file order"""
    rows = list(csv.reader(io.StringIO(text)))
    assert rows[0] == HEADER
    out, last = {}, None
    for r in rows[1:]:
        assert r[2] == last or r[2] not in out                       # a marker's lines are one contiguous block
        out.setdefault(r[2], []).append(r)
        last = r[2]
    return out


def _shared(marker_row):
    """a line without its group and its two adjusted p-values: what diff_pa's line has to equal as text"""
    return [v for j, v in enumerate(marker_row) if j != 2 and j not in ADJ]


def _assert_blocks_are_diff_pa(root, clu, res, text, names, n_perm, seed):
    """every marker's block equals the file of `diff_pa --idents_1 <marker>` as text, group and the two adjusted
    p-values left aside (a marker whose diff_pa file has no line has no block); the adjusted ones equal rc.bh over all
    lines and over all (marker, record) combinations of the file.  Returns the blocks"""
    blocks = _blocks(text)
    want_keys = []
    for name in names:
        want = list(csv.reader(io.StringIO(rc.perm_command("diff_pa", root, clu, res, name, None, n_perm, seed))))[1:]
        if want:
            want_keys.append(name)
            got = blocks[name]
            assert len(got) == len(want), name
            for a, b in zip(got, want):
                assert _shared(a) == [v for j, v in enumerate(b) if j + 1 not in ADJ], (a, b)
                assert a[HEADER.index("versus")] == name
    assert list(blocks) == want_keys
    body = [r for b in blocks.values() for r in b]
    ix = {name: HEADER.index(name) for name in ("n_ge", "gene_n_ge")}
    p_site = rc.bh([Fraction(1 + int(r[ix["n_ge"]]), 1 + n_perm) for r in body])
    genes = list(dict.fromkeys((r[2], r[0]) for r in body))
    first = {k: next(r for r in body if (r[2], r[0]) == k) for k in genes}
    p_gene = dict(zip(genes, rc.bh([Fraction(1 + int(first[k][ix["gene_n_ge"]]), 1 + n_perm) for k in genes])))
    for r, want in zip(body, p_site):
        assert rc.close(r[ADJ[0]], want) and rc.close(r[ADJ[1]], p_gene[(r[2], r[0])]), r
    return blocks


@pytest.mark.gpu
def test_command_is_the_loop_of_diff_pa(tmp_path):
    """the first 14 records of the synthetic directory (clusters of 230, 301 and 40 cells; 29 cells have no cluster),
    199 permutations: one block per cluster, each the file of diff_pa on that cluster against the rest; then C and A
    named in that order: two blocks in that order, the 301 cells of B the others, the tag in the file name"""
    clu = rc.write_synthetic(tmp_path, 14)
    names = tuple(rc.first_clusters(rc.synthetic()[2]))
    assert sorted(names) == ["A", "B", "C"]
    text = _command(tmp_path, clu, "res.gene.pkl", (), 199, 1)
    blocks = _assert_blocks_are_diff_pa(tmp_path, clu, "res.gene.pkl", text, names, 199, 1)
    assert list(blocks) == list(names) and all(len(b) > 20 for b in blocks.values())
    assert len({r[HEADER.index("gene_stat")] for b in blocks.values() for r in b}) > 20
    named = _command(tmp_path, clu, "res.gene.pkl", ("C", "A"), 199, 1)
    assert os.path.basename(_path(tmp_path, clu, "res.gene.pkl", ("C", "A"))) == "syn_groups.gene.C+A.diff_pa_markers.csv"
    two = _assert_blocks_are_diff_pa(tmp_path, clu, "res.gene.pkl", named, ("C", "A"), 199, 1)
    assert list(two) == ["C", "A"]
    for name in two:                                 # the same marker alone and among three: only the adjustments differ
        assert [_shared(r) for r in two[name]] == [_shared(r) for r in blocks[name]]


def _sparse_dir(root):
    """40 barcodes, the clusters A, B, D, E dealt in turn (10 cells each); record 0 has reads in A, B and D, record 1
    in A and B only, record 2 in A only; E has no read at all: (cluster file path, names)"""
    from scape.apa_core import Parameters
    rng = np.random.default_rng(2)
    ids = np.arange(40) * 5 + 1
    names = ["A", "B", "D", "E"]
    of = np.array([names[j % 4] for j in range(40)])
    bc = "CB,index\n" + "".join(f"S{j}-1,{i}\n" for j, i in enumerate(ids.tolist()))
    clu_text = "index,group\n" + "".join(f"{i},{c}\n" for i, c in zip(ids.tolist(), of.tolist()))
    records = []
    for r, used in enumerate(("ABD", "AB", "A")):
        cells = np.nonzero(np.isin(of, list(used)))[0]
        K, m = 3 + r, 300
        records.append(dict(gene_info_str=f"3:MG{r}:1:{500 * r + 1}-{500 * r + 400}:+", K=K,
                            alpha_arr=np.arange(K) * 40 + 10, beta_arr=np.full(K, 10.0),
                            label_arr=rng.integers(0, K, m).astype(np.int64),
                            cb_id_arr=ids[rng.choice(cells, m)].astype(np.int64)))
    return rc.write_dir(str(root), "res.gene.pkl", records, bc, {"sparse.csv": clu_text}, Parameters)[0], names


@pytest.mark.gpu
def test_marker_without_reads(tmp_path):
    """a cluster without a read in a record has no line for it, a cluster without a tested record no block, and a
    record with reads in one cluster only no line at all; the adjustments are over what is left (checked against
    rc.bh over the file by _assert_blocks_are_diff_pa)"""
    clu, names = _sparse_dir(tmp_path)
    text = _command(tmp_path, clu, "res.gene.pkl", (), 199, 4)
    blocks = _assert_blocks_are_diff_pa(tmp_path, clu, "res.gene.pkl", text, names, 199, 4)
    genes = {name: list(dict.fromkeys(r[0].split(":")[1] for r in b)) for name, b in blocks.items()}
    assert genes == {"A": ["MG0", "MG1"], "B": ["MG0", "MG1"], "D": ["MG0"]}
    assert len(blocks["A"]) == 3 + 4 and len(blocks["D"]) == 3


@pytest.mark.gpu
def test_batch_chunk_and_range_invariance(tmp_path, monkeypatch):
    """records over several count batches, the permutations over several chunks, the markers over several ranges: the
    same bytes"""
    from scape_amd import _lib, report
    clu = rc.write_synthetic(tmp_path)
    n_perm, seed = 199, 1
    big = _command(tmp_path, clu, "res.gene.pkl", (), n_perm, seed)
    lib = _lib.load_library()
    calls = {"masks": [], "test": []}
    real_m, real_t = lib.scape_hip_report_perm_marker_masks, lib.scape_hip_report_perm_markers

    def masks(*a):
        calls["masks"].append((a[5], a[6]))
        return real_m(*a)

    def test(*a):
        calls["test"].append((a[6], a[7]))
        return real_t(*a)
    monkeypatch.setattr(lib, "scape_hip_report_perm_marker_masks", masks)
    monkeypatch.setattr(lib, "scape_hip_report_perm_markers", test)
    assert _command(tmp_path, clu, "res.gene.pkl", (), n_perm, seed) == big
    assert calls["masks"] == [(1, n_perm)] and calls["test"] == [(0, 3)]
    calls.update(masks=[], test=[])
    monkeypatch.setattr(report, "MAX_BATCH_BYTES", 1 << 16)             # a record of K = 8 alone takes 57 KB
    monkeypatch.setattr(report, "MAX_PERM_BYTES", 1 << 30)
    assert _command(tmp_path, clu, "res.gene.pkl", (), n_perm, seed) == big
    assert calls["masks"] == [(1, n_perm)] and len(calls["test"]) > 5
    n_batches = len(calls["test"])
    calls.update(masks=[], test=[])
    # per permutation: three markers, each 9 words over the 571 clustered cells and a key bound; room for 80 permutations
    monkeypatch.setattr(report, "MAX_PERM_BYTES", 3 * (9 + 1) * 8 * 80)
    assert _command(tmp_path, clu, "res.gene.pkl", (), n_perm, seed) == big
    assert len(calls["test"]) == 3 * n_batches and calls["masks"][:3] == [(1, 80), (81, 80), (161, 39)]
    calls.update(masks=[], test=[])
    monkeypatch.setattr(report, "MAX_PERM_BYTES", 1 << 30)
    monkeypatch.setattr(report, "MAX_MARKER_RESULT_BYTES", 1)          # one marker per call
    assert _command(tmp_path, clu, "res.gene.pkl", (), n_perm, seed) == big
    assert calls["test"][:3] == [(0, 1), (1, 1), (2, 1)] and len(calls["test"]) == 3 * n_batches
