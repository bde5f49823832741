"""`scape diff_pa_len_markers`: diff_pa_len of every cluster of a cluster file against all other cells that have a
cluster, from one pass over the result file (scape_amd/report.py, section diff_pa_len_pairs / diff_pa_len_markers;
kernel k_rep_perm_len_markers and entry point scape_hip_report_perm_len_markers of scape_amd/csrc/perm.inc).

The contract is "marker X is exactly `diff_pa_len --idents_1 X`", so the yardstick is the exact oracle of
tests/test_report_difflen.py, applied per marker with cols1 = X's columns ascending and cols2 = every other tested
column ascending, and diff_pa_len's own entry point and command.  The inputs of the entry point test are
tests/test_report_diffmarkers.py's (layout, ENTRY_CASES: interleaved columns, with and without others) with the
positions of tests/test_report_difflenpairs.py, whose helpers this file uses.  Every GPU comparison first asserts
lo == hi on the oracle for every record of its case, no record excused, and then equality with lo."""
import functools
import os

import numpy as np
import pytest

import report_cases as rc
import test_report_difflen as dl
import test_report_difflenpairs as lp
import test_report_diffmarkers as dm
import test_report_diffpairs as dpp
from report_cases import no_gpu  # noqa: F401  (fixture)

HEADER = lp.LEN_HEADER[:1] + ["group"] + lp.LEN_HEADER[1:]
CMD = "diff_pa_len_markers"
POS_SEED = 100                            # of lp.positions: no near tie for any marker of ENTRY_CASES (checked below)


# ---------------------------------------------------------------- the cases the GPU test compares with the oracle
@functools.lru_cache(maxsize=None)
def entry_inputs():
    """rc.entry_point_matrix() with its positions: (recs for the oracle, alpha per record)"""
    Ks, dense = rc.entry_point_matrix()[5], rc.entry_point_matrix()[9]
    alpha = lp.positions(Ks, POS_SEED)
    return lp.oracle_recs(Ks, dense, alpha), alpha


@functools.lru_cache(maxsize=None)
def entry_oracle(case):
    """(columns per segment, orig_rank, lp.item_want of every marker of dm.ENTRY_CASES[case]) after 300 permutations"""
    n1, n2, _n_cols, seed, n_perm = rc.entry_point_matrix()[:5]
    sizes, n_others = dm.ENTRY_CASES[case]
    assert sum(sizes) + n_others == n1 + n2
    cols, rank = dm.layout(sizes, n_others)
    recs, _alpha = entry_inputs()
    return cols, rank, [lp.item_want(recs, cols[g].tolist(), np.setdiff1d(np.arange(n1 + n2), cols[g]).tolist(), n_perm,
                                     seed) for g in range(len(sizes))]


# ---------------------------------------------------------------- CPU
def test_entry_oracle_has_no_near_tie():
    """for every marker of the two layouts: no near tie, every record tested (the records of 70 and 150 rows among
    them), the columns interleaved, and counts strictly inside 0 .. 300"""
    n_perm = rc.entry_point_matrix()[4]
    for case in dm.ENTRY_CASES:
        _cols, rank, wants = entry_oracle(case)
        assert not np.array_equal(rank, np.arange(len(rank)))
        for g, want in enumerate(wants):
            assert all(w is not None for w in want), (case, g)
            assert lp.near_ties(want) == [], (case, g)
        assert max(len(w["own"]) for w in wants[0]) > 128
        assert any(0 < w["line"]["lo"] < n_perm for want in wants for w in want), case


def test_command_oracles_have_no_near_tie():
    """the synthetic directory, 257 permutations, seed 1: 36 lines for each of its three markers, none with a near tie;
    and its first 12 records with seed 5 after 1, 255, 256 and 257 permutations"""
    for name in dpp.syn_names():
        lines = lp.syn_oracle(name, None)
        assert len(lines) == 36
        dl.assert_no_near_tie(lines, name)
        for n_perm in (1, 255, 256, 257):
            dl.assert_no_near_tie(lp.syn_oracle(name, None, n_perm, 5, 12), (name, n_perm))


def test_help_and_import_path():
    r = rc.run(["--help"])
    assert r.exit_code == 0 and CMD in r.output
    r = rc.run([CMD, "--help"])
    assert r.exit_code == 0, r.output
    for o in ("--output_dir", "--res_pkl_file", "--cell_cluster_file", "--idents", "--n_perm", "--seed"):
        assert o in r.output
    assert "--idents_1" not in r.output and "--strata_file" not in r.output
    flat = " ".join(r.output.split())
    assert "[default: 9999]" in flat and "[default: 1]" in flat and "(1 to 64)" in flat
    import scape.utils as su
    from scape_amd import report
    assert su.diff_pa_len_markers is report.diff_pa_len_markers
    assert report.DIFF_PA_LEN_MARKERS_HEADER == HEADER


def test_prerequisites_and_argument_errors(tmp_path, no_gpu):
    """diff_pa_markers's list of errors with this command's name in the messages, before the device is opened"""
    from scape_amd import report
    args = functools.partial(lp._args, cmd=CMD)
    clu = tmp_path / "groups.csv"
    r = rc.run(args(tmp_path / "nope", clu))
    assert r.exit_code != 0 and "Given output_dir folder does not exists." in str(r.exception)
    r = rc.run(args(tmp_path, clu))
    assert "Given res_pkl_file is not in output_dir." in str(r.exception)
    (tmp_path / "res.gene.pkl").write_bytes(b"")
    r = rc.run(args(tmp_path, clu))
    assert "Given cell_cluster_file file does not exists" in str(r.exception)
    clu.write_text("index,group\n3,A\n4,B\n5,\n6,a/b\n77,ghost\n")
    (tmp_path / "barcode_index.csv").write_text("CB,index\nA-1,3\nB-1,4\nC-1,5\nD-1,6\n")
    for extra, word in ((["--idents", "A", "--idents", "Z"], "'Z'"), (["--idents", "A", "--idents", "A"], "twice"),
                        (["--idents", "A", "--idents", "ghost"], "has no cell"),
                        (["--idents", "A", "--idents", ""], "names no cluster"),
                        (["--idents", "A", "--idents", "a/b"], "file name"),
                        (["--n_perm", "0"], "n_perm"), (["--n_perm", str(1 << 31)], "n_perm"),
                        (["--seed", "-1"], "seed"), (["--seed", str(1 << 64)], "seed")):
        r = rc.run(args(tmp_path, clu) + extra)
        assert isinstance(r.exception, ValueError) and word in str(r.exception), (extra, repr(r.exception))
    one = report._groups_setup(str(tmp_path), "res.gene.pkl", str(clu), ("B",), 9, 1, CMD, markers=True)
    assert one.names == ["B"] and one.n == 3 and one.outpath.endswith("groups.gene.B.diff_pa_len_markers.csv")
    ids = list(range(100, 166))
    (tmp_path / "barcode_index.csv").write_text("CB,index\n" + "".join(f"C{i}-1,{i}\n" for i in ids))
    clu.write_text("index,group\n" + "".join(f"{i},g{i}\n" for i in ids[:65]))
    r = rc.run(args(tmp_path, clu))
    assert isinstance(r.exception, ValueError) and "65 clusters: diff_pa_len_markers" in str(r.exception)
    clu.write_text("index,group\n" + "".join(f"{i},only\n" for i in ids[:40]) + f"{ids[50]},\n")
    for extra in ([], ["--idents", "only"]):
        r = rc.run(args(tmp_path, clu) + extra)
        assert isinstance(r.exception, ValueError) and "the rest has no cell" in str(r.exception), repr(r.exception)
    r = rc.run(args(tmp_path, clu) + ["--strata_file", str(clu)])
    assert r.exit_code == 2 and "--strata_file" in r.output
    assert sorted(os.listdir(tmp_path)) == ["barcode_index.csv", "groups.csv", "res.gene.pkl"]


# ---------------------------------------------------------------- GPU: the entry point
@pytest.mark.gpu
@pytest.mark.parametrize("case", list(dm.ENTRY_CASES))
def test_entry_point(case):
    """scape_hip_report_perm_len_markers on rc.entry_point_matrix(), its 161 tested columns dealt to the markers (and
    others) at random, with lp.positions(): t and a0 equal the dense sums, n_ge the oracle's lo and delta(0) lies within
    tol of the Fraction for every marker; the markers in two ranges and the permutations in two chunks give the same
    totals and bits; the refusals leave masks and counts usable; and every marker has the n_ge and the bits of delta(0)
    of scape_hip_report_perm_len on the count matrix laid out as diff_pa_len lays it out"""
    from scape_amd import _lib
    from scape_amd._lib import P_d, P_i32, P_i64, check as chk, ptr
    _n1, _n2, n_cols, seed, n_perm, Ks, off, lab, cb, dense, rows, roff, _rng = rc.entry_point_matrix()
    _recs, alpha = entry_inputs()
    sizes, n_others = dm.ENTRY_CASES[case]
    cols, rank, wants = entry_oracle(case)
    M, n, n_rows, n_rec = len(sizes), len(rank), len(rows), len(Ks)
    n_seg = M + 1
    seg = np.concatenate([[0], np.cumsum(sizes), [n]]).astype(np.int32)
    x = lp.row_positions(rows, Ks, alpha)
    ctx = _lib.default_context(None)
    lib = ctx.lib

    def outs(m=M):
        return (np.full(n_rows, -1, np.int64), np.full((n_rows, n_seg), -1, np.int64), np.full((m, n_rec), -1.0),
                np.zeros((m, n_rec), np.int64))

    def test(o, first=0, count=M, roff_=roff, rows_=rows, seg_=seg, n_seg_=n_seg, x_=x, n_rec_=n_rec):
        return lib.scape_hip_report_perm_len_markers(ctx.h, n_rec_, ptr(roff_, P_i64), ptr(rows_, P_i64), n_seg_,
                                                     ptr(seg_, P_i32), first, count, ptr(x_, P_d), ptr(o[0], P_i64),
                                                     ptr(o[1], P_i64), ptr(o[2], P_d), ptr(o[3], P_i64))
    try:
        lib.scape_hip_report_free(ctx.h)
        assert test(outs()) != 0 and "report_counts" in _lib.last_error()
        rc.device_counts(ctx, Ks, off, lab, lp.to_front(rank, n_cols)[cb], n_cols)
        assert test(outs()) != 0 and "marker_masks" in _lib.last_error()     # counts, but no marker masks yet
        chk(dm._marker_masks(ctx, sizes, n_others, rank, 1, n_perm, seed), "marker_masks")
        one = outs()
        chk(test(one), "perm_len_markers")
        sub = dense[rows][:, rank]
        a0_want = np.stack([sub[:, seg[g]:seg[g + 1]].sum(axis=1) for g in range(n_seg)], axis=1)
        assert np.array_equal(one[0], sub.sum(axis=1)) and np.array_equal(one[1], a0_want)
        lp.assert_items_equal_oracle(wants, one[3], one[2])
        lo, hi = outs(1), outs(M - 1)                                # the markers in two ranges
        chk(test(lo, 0, 1), "perm_len_markers")
        chk(test(hi, 1, M - 1), "perm_len_markers")
        assert np.array_equal(np.concatenate([lo[3], hi[3]]), one[3])
        assert np.array_equal(np.concatenate([lo[2], hi[2]]).view(np.uint64), one[2].view(np.uint64))
        acc = outs()                                                 # the permutations in two chunks that accumulate
        for p_first, p_count in ((1, 100), (101, n_perm - 100)):
            chk(dm._marker_masks(ctx, sizes, n_others, rank, p_first, p_count, seed), "marker_masks")
            chk(test(acc), "perm_len_markers")
        assert np.array_equal(acc[3], one[3]) and np.array_equal(acc[2].view(np.uint64), one[2].view(np.uint64))
        chk(dm._marker_masks(ctx, sizes, n_others, rank, 1, n_perm, seed), "marker_masks")
        # refusals, each before anything is queued: outputs untouched, masks and counts usable afterwards
        o = outs()
        bad_seg = seg.copy()
        bad_seg[1] += 1
        assert test(o, seg_=bad_seg) != 0 and "seg_off differs" in _lib.last_error()
        assert test(o, n_seg_=M, seg_=seg[:-1].copy()) != 0 and "n_groups differs" in _lib.last_error()
        for first, count in ((-1, 1), (0, 0), (0, M + 1), (M, 1)):
            assert test(o, first, count) != 0 and "marker_first" in _lib.last_error(), (first, count)
        bad_roff = roff.copy()
        bad_roff[1], bad_roff[2] = roff[2], roff[1]
        assert test(o, roff_=bad_roff) != 0 and "non-decreasing" in _lib.last_error()
        for k in (8, 9, 10, 11, 12):                                 # x and every output, NULL in turn
            a = [ctx.h, n_rec, ptr(roff, P_i64), ptr(rows, P_i64), n_seg, ptr(seg, P_i32), 0, M, ptr(x, P_d),
                 ptr(o[0], P_i64), ptr(o[1], P_i64), ptr(o[2], P_d), ptr(o[3], P_i64)]
            a[k] = None
            assert lib.scape_hip_report_perm_len_markers(*a) != 0 and "bad argument" in _lib.last_error(), k
        bad_x = x.copy()
        bad_x[roff[1] + 2] = np.nan
        assert test(o, x_=bad_x) != 0 and "record 1" in _lib.last_error() and "finite" in _lib.last_error()
        many = (np.zeros(1025, np.int64), np.zeros((1025, n_seg), np.int64), np.zeros((M, 1)), np.zeros((M, 1), np.int64))
        assert test(many, roff_=np.array([0, 1025], np.int64), rows_=np.zeros(1025, np.int64), x_=np.zeros(1025),
                    n_rec_=1) != 0 and "more than 1024 rows" in _lib.last_error()
        assert np.all(o[0] == -1) and np.all(o[1] == -1) and np.all(o[2] == -1.0) and not o[3].any()
        again = outs()
        chk(test(again), "perm_len_markers")                         # a refused call keeps masks and counts
        assert np.array_equal(again[3], one[3]) and np.array_equal(again[2].view(np.uint64), one[2].view(np.uint64))
        # scape_hip_report_perm_len, marker by marker, on diff_pa_len's layout of the columns
        for g in range(M):
            front = np.concatenate([cols[g], np.setdiff1d(np.arange(n), cols[g])])
            lp.assert_item_is_perm_len(ctx, Ks, off, lab, lp.to_front(front, n_cols)[cb], n_cols, sizes[g], n - sizes[g],
                                       n_perm, seed, rows, roff, x, wants[g], one[3][g], one[2][g])
    finally:
        lib.scape_hip_report_free(ctx.h)


# ---------------------------------------------------------------- GPU: the command
def _marker_items(names):
    return [((name,), name, None) for name in names]


def _command(root, clu, idents, n_perm, seed):
    return lp._command(root, clu, "res.gene.pkl", idents, n_perm, seed, cmd=CMD)


@pytest.mark.gpu
def test_synthetic_directory(tmp_path):
    """clusters B, A and C (301, 230 and 40 cells; 29 cells have no cluster), 257 permutations: three blocks in the
    cluster file's order, each the file of `diff_pa_len --idents_1 X`, 36 lines each, n_ge the exact oracle's; then C
    and A named in that order (B's cells are the others), and C alone"""
    clu = rc.write_synthetic(tmp_path)
    names = dpp.syn_names()
    n_perm, seed = lp.SYN_PERM, lp.SYN_SEED
    text = _command(tmp_path, clu, (), n_perm, seed)
    oracles = {(name,): lp.syn_oracle(name, None) for name in names}
    blocks = lp.assert_blocks_are_diff_pa_len(tmp_path, clu, "res.gene.pkl", text, HEADER, _marker_items(names), n_perm,
                                              seed, oracles)
    assert list(blocks) == [(name,) for name in names]
    ix = {name: HEADER.index(name) for name in HEADER}
    for (name,), got in blocks.items():
        assert len(got) == 36 and {(r[ix["group"]], r[ix["versus"]]) for r in got} == {(name, name)}
    named = _command(tmp_path, clu, ("C", "A"), n_perm, seed)
    assert os.path.basename(lp._path(tmp_path, clu, "res.gene.pkl", ("C", "A"), CMD)) == \
        "syn_groups.gene.C+A.diff_pa_len_markers.csv"
    two = lp.assert_blocks_are_diff_pa_len(tmp_path, clu, "res.gene.pkl", named, HEADER, _marker_items(("C", "A")),
                                           n_perm, seed, {k: oracles[k] for k in (("C",), ("A",))})
    assert list(two) == [("C",), ("A",)]
    single = _command(tmp_path, clu, ("C",), n_perm, seed)       # a single --idents is a run
    alone = lp.assert_blocks_are_diff_pa_len(tmp_path, clu, "res.gene.pkl", single, HEADER, _marker_items(("C",)),
                                             n_perm, seed, {("C",): oracles[("C",)]})
    drop = lambda r: r[:ix["p_val_adj"]] + r[ix["p_val_adj"] + 1:]
    for key in two:                                # the same marker among one, two and three: only the adjustment differs
        assert [drop(r) for r in two[key]] == [drop(r) for r in blocks[key]]
    assert [drop(r) for r in alone[("C",)]] == [drop(r) for r in blocks[("C",)]]


@pytest.mark.gpu
def test_marker_without_reads(tmp_path):
    """dm._sparse_dir: record 0 has reads in A, B and D, record 1 in A and B only, record 2 in A only, E none at all: a
    marker without reads in a record has no line for it, a marker without a tested record no block, and the adjustment
    is over what is left"""
    clu, names = dm._sparse_dir(tmp_path)
    text = _command(tmp_path, clu, (), 199, 4)
    blocks = lp.assert_blocks_are_diff_pa_len(tmp_path, clu, "res.gene.pkl", text, HEADER, _marker_items(names), 199, 4)
    genes = {name: [r[0].split(":")[1] for r in b] for (name,), b in blocks.items()}
    assert genes == {"A": ["MG0", "MG1"], "B": ["MG0", "MG1"], "D": ["MG0"]}


@pytest.mark.gpu
@pytest.mark.parametrize("n_perm", [1, 255, 256, 257])
def test_tile_edges(n_perm, tmp_path):
    """a workgroup of the test kernel takes 256 permutations: one, one short of a tile, a full tile, one over"""
    clu = rc.write_synthetic(tmp_path, 12)
    names = dpp.syn_names()
    text = _command(tmp_path, clu, (), n_perm, 5)
    oracles = {(name,): lp.syn_oracle(name, None, n_perm, 5, 12) for name in names}
    assert len(lp.assert_blocks_are_diff_pa_len(tmp_path, clu, "res.gene.pkl", text, HEADER, _marker_items(names), n_perm,
                                                5, oracles)) == 3


@pytest.mark.gpu
def test_batch_chunk_and_range_invariance(tmp_path, monkeypatch):
    # per permutation: three markers, each 9 words over the 571 clustered cells and a key bound; room for 100 permutations
    lp.assert_invariance(tmp_path, monkeypatch, CMD, "scape_hip_report_perm_marker_masks",
                         "scape_hip_report_perm_len_markers", 5, 3 * (9 + 1) * 8 * 100, [(1, 100), (101, 100), (201, 57)])


@pytest.mark.gpu
def test_failed_run_leaves_no_part_file(tmp_path, monkeypatch):
    from scape_amd import _lib
    clu = rc.write_synthetic(tmp_path, 12)
    lib = _lib.load_library()
    monkeypatch.setattr(lib, "scape_hip_report_perm_len_markers", lambda *a: 1)
    r = rc.run(lp._args(tmp_path, clu, n_perm=10, cmd=CMD))
    assert r.exit_code != 0 and isinstance(r.exception, _lib.ScapeHipError), repr(r.exception)
    assert not rc.parts_left(tmp_path) and not os.path.exists(lp._path(tmp_path, clu, "res.gene.pkl", (), CMD))
