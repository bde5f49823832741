"""`scape diff_pa_len_pairs`: diff_pa_len for every pair of the populations of a cluster file, from one pass over the
result file (scape_amd/report.py, section diff_pa_len_pairs; kernel k_rep_perm_len_pairs and entry point
scape_hip_report_perm_len_pairs of scape_amd/csrc/perm.inc).

The contract is "pair (A, B) is exactly `diff_pa_len --idents_1 A --idents_2 B`", so the yardsticks are diff_pa_len's:
the exact oracle of tests/test_report_difflen.py (`oracle`, `assert_no_near_tie`, `compare`), applied per pair with
cols1 = A's columns ascending and cols2 = B's, and the entry point and the command of diff_pa_len themselves.  The
inputs of the entry point tests are tests/test_report_diffpairs.py's (entry_case, ENTRY_SIZES) with positions drawn per
record.  Every GPU comparison first asserts lo == hi on the oracle for every record of its case, no record excused, and
then equality with lo.  tests/test_report_difflenmarkers.py uses the helpers of this file for the markers."""
import csv
import functools
import io
import os
from fractions import Fraction

import numpy as np
import pytest

import report_cases as rc
import test_report_difflen as dl
import test_report_diffpairs as dpp
from report_cases import no_gpu  # noqa: F401  (fixture)

LEN_HEADER = dl.HEADER.split(",")
HEADER = LEN_HEADER[:1] + ["group_1", "group_2"] + LEN_HEADER[1:]
ADJ = LEN_HEADER.index("p_val_adj")       # in a line of diff_pa_len's layout
NAMES = ("scape_hip_report_perm_len_pairs", "scape_hip_report_perm_len_markers")


# ---------------------------------------------------------------- the cases the GPU tests compare with the oracle
def positions(Ks, gen_seed=100):
    """alpha_arr of record r: K_r distinct integer positions in 50 .. 4999, unsorted"""
    return [np.random.default_rng(gen_seed + r).permutation(np.arange(50, 5000))[:int(K)].astype(np.float64)
            for r, K in enumerate(np.asarray(Ks).tolist())]


def oracle_recs(Ks, dense, alpha):
    """the records of a dense matrix [all count rows, columns] as tests/test_report_difflen.py's oracle takes them"""
    rowbase = np.concatenate([[0], np.cumsum(Ks)])
    return [dict(gene=f"r{r}", K=int(K), alpha=alpha[r], dense=dense[rowbase[r]:rowbase[r + 1]])
            for r, K in enumerate(np.asarray(Ks).tolist())]


def item_want(recs, cols1, cols2, n_perm, seed):
    """dl.oracle of one item (pair, marker) and, per record, None when the item does not test it, else dict(line = the
    oracle's line, own = the labels with a read in the item's cells, span = max x - min x over them (Fraction))"""
    lines = {ln["gene"]: ln for ln in dl.oracle(recs, cols1, cols2, n_perm, seed)}
    out = []
    for rec in recs:
        ln = lines.get(rec["gene"])
        if ln is None:
            out.append(None)
            continue
        own = np.nonzero(np.asarray(rec["dense"])[:, list(cols1) + list(cols2)].sum(axis=1) > 0)[0]
        x = [Fraction(float(v)) for v in np.asarray(rec["alpha"])[own]]
        out.append(dict(line=ln, own=own, span=max(x) - min(x)))
        assert len(own) == ln["num_pa"]
    return out


def near_ties(want):
    return [(w["line"]["gene"], w["line"]["lo"], w["line"]["hi"]) for w in want
            if w is not None and w["line"]["lo"] != w["line"]["hi"]]


@functools.lru_cache(maxsize=None)
def entry_inputs():
    """dpp.entry_case() with its positions: (recs for the oracle, alpha per record)"""
    Ks, _off, _lab, _cb, dense, _n_cols, _seed, _n_perm = dpp.entry_case()
    alpha = positions(Ks)
    return oracle_recs(Ks, dense, alpha), alpha


@functools.lru_cache(maxsize=None)
def entry_oracle(G):
    """item_want of every pair of dpp.ENTRY_SIZES[G], in pair order"""
    seed, n_perm = dpp.entry_case()[6:8]
    recs, _alpha = entry_inputs()
    seg = np.concatenate([[0], np.cumsum(dpp.ENTRY_SIZES[G])])
    return [item_want(recs, range(seg[g], seg[g + 1]), range(seg[h], seg[h + 1]), n_perm, seed)
            for g, h in dpp.pair_list(G)]


def row_positions(rows, Ks, alpha):
    """the position of every count row of `rows`"""
    rowbase = np.concatenate([[0], np.cumsum(Ks)])
    rec = np.searchsorted(rowbase, rows, side="right") - 1
    return np.ascontiguousarray([alpha[r][i - rowbase[r]] for r, i in zip(rec.tolist(), rows.tolist())], dtype=np.float64)


SYN_PERM, SYN_SEED = 257, 1


@functools.lru_cache(maxsize=None)
def syn_oracle(id1, id2, n_perm=SYN_PERM, seed=SYN_SEED, n_rec=None):
    """dl.oracle's lines of the synthetic directory (its first n_rec records) for id1 against id2 (None: the rest)"""
    s = dl._syn()
    c1, c2 = rc.populations(s["bc"], s["clu"], id1, id2)
    return dl.oracle(s["recs"][:n_rec], c1, c2, n_perm, seed)


# ---------------------------------------------------------------- CPU
def test_entry_oracle_no_near_tie_and_paths():
    """on the oracle alone, for every pair of the three size sets: no near tie; a tested combination whose span differs
    from the record's and one whose min x differs; the pair of two 1-cell groups ties in every labelling; records that
    some pairs test and others do not"""
    recs, alpha = entry_inputs()
    n_perm = dpp.entry_case()[7]
    rows_all = {G: dpp.entry_oracle(G)[:2] for G in dpp.ENTRY_SIZES}
    for G in dpp.ENTRY_SIZES:
        for k, want in enumerate(entry_oracle(G)):
            assert near_ties(want) == [], (G, k)

    def kept_x(G, r):
        rows, roff = rows_all[G]
        rowbase = np.concatenate([[0], np.cumsum(dpp.entry_case()[0])])
        return alpha[r][rows[roff[r]:roff[r + 1]] - rowbase[r]]
    w = entry_oracle(3)[dpp.pair_list(3).index((0, 1))][4]               # its most distal kept row has no read in the pair
    x = kept_x(3, 4)
    assert w is not None and w["span"] < Fraction(float(x.max() - x.min())) and len(w["own"]) < len(x)
    assert alpha[4][w["own"]].min() == x.min()
    pair24 = entry_oracle(5)[dpp.pair_list(5).index((2, 4))]
    w = pair24[2]
    x = kept_x(5, 2)
    assert w is not None and alpha[2][w["own"]].min() > x.min()
    tested24 = [r for r, w in enumerate(pair24) if w is not None]
    assert len(tested24) == 4 and all(pair24[r]["line"]["lo"] == n_perm for r in tested24)
    partly = set()                                                        # records that some pairs test and others do not
    for G in (3, 5):
        tested = np.array([[w is not None for w in want] for want in entry_oracle(G)])
        partly |= {(G, r) for r in range(tested.shape[1]) if tested[:, r].any() and not tested[:, r].all()}
        counts = {w["line"]["lo"] for want in entry_oracle(G) for w in want if w is not None}
        assert len(counts) > 5 and min(counts) < n_perm // 4
    assert {(3, 5), (5, 4), (5, 5)} <= partly, partly
    assert all(w is not None for w in entry_oracle(2)[0][:4])


def test_command_oracles_have_no_near_tie():
    """the synthetic directory, 257 permutations, seed 1: 36 lines for each of its three pairs, none with a near tie;
    and its first 12 records with seed 5 after 1, 255, 256 and 257 permutations"""
    names = dpp.syn_names()
    for g, h in dpp.pair_list(3):
        lines = syn_oracle(names[g], names[h])
        assert len(lines) == 36
        dl.assert_no_near_tie(lines, (names[g], names[h]))
        for n_perm in (1, 255, 256, 257):
            dl.assert_no_near_tie(syn_oracle(names[g], names[h], n_perm, 5, 12), (names[g], names[h], n_perm))


def _args(root, clu, res="res.gene.pkl", idents=(), n_perm=None, seed=None, cmd="diff_pa_len_pairs"):
    a = [cmd, "--output_dir", str(root), "--res_pkl_file", res, "--cell_cluster_file", str(clu)]
    for i in idents:
        a += ["--idents", i]
    for opt, v in (("--n_perm", n_perm), ("--seed", seed)):
        if v is not None:
            a += [opt, str(v)]
    return a


def _path(root, clu, res, idents=(), cmd="diff_pa_len_pairs"):
    kind = res[len("res."):-len(".pkl")]
    stem = os.path.splitext(os.path.basename(str(clu)))[0]
    tag = "." + "+".join(idents) if idents else ""
    return os.path.join(str(root), f"{stem}.{kind}{tag}.{cmd}.csv")


def _command(root, clu, res, idents, n_perm, seed, what="", cmd="diff_pa_len_pairs"):
    r = rc.run(_args(root, clu, res, idents, n_perm, seed, cmd))
    assert r.exit_code == 0, (what, r.output, repr(r.exception))
    assert not rc.parts_left(root)
    with open(_path(root, clu, res, idents, cmd), newline="") as fh:
        return fh.read()


def test_help_and_import_path():
    r = rc.run(["--help"])
    assert r.exit_code == 0 and "diff_pa_len_pairs" in r.output
    r = rc.run(["diff_pa_len_pairs", "--help"])
    assert r.exit_code == 0, r.output
    for o in ("--output_dir", "--res_pkl_file", "--cell_cluster_file", "--idents", "--n_perm", "--seed"):
        assert o in r.output
    assert "--strata_file" not in r.output and "--idents_1" not in r.output
    flat = " ".join(r.output.split())
    assert "[default: 9999]" in flat and "[default: 1]" in flat
    import scape.utils as su
    from scape_amd import _lib, report
    assert su.diff_pa_len_pairs is report.diff_pa_len_pairs
    assert all(name in _lib.SIGNATURES for name in NAMES)
    assert report.DIFF_PA_LEN_PAIRS_HEADER == HEADER


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
    assert isinstance(r.exception, ValueError) and "1 populations: diff_pa_len_pairs takes 2 to 64" in str(r.exception)
    ids = list(range(100, 165))
    (tmp_path / "barcode_index.csv").write_text("CB,index\n" + "".join(f"X{i}-1,{i}\n" for i in ids))
    clu.write_text("index,group\n" + "".join(f"{i},c{i}\n" for i in ids))
    r = rc.run(_args(tmp_path, clu))
    assert isinstance(r.exception, ValueError) and "65 populations: diff_pa_len_pairs takes 2 to 64" in str(r.exception)
    r = rc.run(_args(tmp_path, clu) + ["--strata_file", str(clu)])
    assert r.exit_code == 2 and "--strata_file" in r.output
    assert sorted(os.listdir(tmp_path)) == ["barcode_index.csv", "groups.csv", "res.gene.pkl"]


# ---------------------------------------------------------------- GPU: the entry point
def to_front(front, n_cols):
    """old column -> new column when the columns `front` move to the front, the others following in order"""
    order = np.concatenate([np.asarray(front, dtype=np.int64), np.setdiff1d(np.arange(n_cols), front)])
    col_of = np.empty(n_cols, dtype=np.int64)
    col_of[order] = np.arange(n_cols)
    return col_of


def assert_item_is_perm_len(ctx, Ks, off, lab, cb_front, n_cols, n1, n2, n_perm, seed, rows, roff, x, want, n_ge, delta0):
    """scape_hip_report_perm_len behind scape_hip_report_perm_masks(n1, n2) on a count matrix whose first n1 + n2
    columns are the item's two populations (cb_front = the reads' columns in that layout), on the item's own rows of the
    records it tests, with w and tol formed as diff_pa_len forms them: the same n_ge and the same bits of delta(0) as
    the item's line n_ge / delta0 [record] of the ranged call"""
    from scape_amd._lib import P_d, P_i64, check as chk, ptr
    which = [r for r, w in enumerate(want) if w is not None]
    rowbase = np.concatenate([[0], np.cumsum(Ks)])
    rows_k = np.concatenate([rowbase[r] + want[r]["own"] for r in which]).astype(np.int64)
    assert np.all(np.isin(rows_k, rows))
    roff_k = np.concatenate([[0], np.cumsum([len(want[r]["own"]) for r in which])]).astype(np.int64)
    xk = x[np.searchsorted(rows, rows_k)]
    w = np.concatenate([xk[a:b] - xk[a:b].min() for a, b in zip(roff_k[:-1], roff_k[1:])])
    tol = np.array([np.ldexp(float(xk[a:b].max() - xk[a:b].min()), -40) for a, b in zip(roff_k[:-1], roff_k[1:])])
    rc.device_counts(ctx, Ks, off, lab, cb_front, n_cols)
    chk(ctx.lib.scape_hip_report_perm_masks(ctx.h, n1, n2, 1, n_perm, seed), "perm_masks")
    t, a = np.zeros(len(rows_k), np.int64), np.zeros(len(rows_k), np.int64)
    d0, ge = np.zeros(len(which)), np.zeros(len(which), np.int64)
    chk(ctx.lib.scape_hip_report_perm_len(ctx.h, len(which), ptr(roff_k, P_i64), ptr(rows_k, P_i64), ptr(w, P_d),
                                          ptr(tol, P_d), ptr(t, P_i64), ptr(a, P_i64), ptr(d0, P_d), ptr(ge, P_i64)),
        "perm_len")
    assert np.array_equal(ge, n_ge[which]), (ge, n_ge[which])
    assert np.array_equal(d0.view(np.uint64), delta0[which].view(np.uint64)), (d0, delta0[which])
    assert np.all(t > 0)


def assert_items_equal_oracle(wants, n_ge, delta0):
    """n_ge [item][record] equals the oracle's lo and delta0 lies within tol of its Fraction where the item tests the
    record; both are exactly 0 where it does not.  lo == hi is asserted first, for every record"""
    for k, want in enumerate(wants):
        assert near_ties(want) == [], k
        for r, w in enumerate(want):
            if w is None:
                assert n_ge[k, r] == 0 and delta0[k, r] == 0.0 and not np.signbit(delta0[k, r]), (k, r)
                continue
            print("item", k, "record", r, "n_ge", int(n_ge[k, r]), "oracle", w["line"]["lo"], "delta0", float(delta0[k, r]))
            assert n_ge[k, r] == w["line"]["lo"], (k, r)
            assert abs(Fraction(float(delta0[k, r])) - w["line"]["delta"]) <= w["span"] / (1 << 40), (k, r)


@pytest.mark.gpu
@pytest.mark.parametrize("G", [2, 3, 5])
def test_entry_point(G):
    """scape_hip_report_perm_len_pairs on dpp.entry_case() with positions(): t and a0 equal the dense sums, n_ge the
    oracle's lo (0 where a pair does not test a record), delta(0) lies within tol of the Fraction (exactly 0.0 where
    untested); the pairs in two ranges and the permutations in two chunks give the same totals and bits; the refusals
    leave masks and counts usable; and every pair has the n_ge and the bits of delta(0) of scape_hip_report_perm_len
    on its own two populations"""
    from scape_amd import _lib
    from scape_amd._lib import P_d, P_i32, P_i64, check as chk, ptr
    Ks, off, lab, cb, dense, n_cols, seed, n_perm = dpp.entry_case()
    _recs, alpha = entry_inputs()
    sizes = dpp.ENTRY_SIZES[G]
    seg = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    pairs = dpp.pair_list(G)
    rows, roff, _res = dpp.entry_oracle(G)
    wants = entry_oracle(G)
    x = row_positions(rows, Ks, alpha)
    n_rows, n_rec, n_pairs = len(rows), len(Ks), len(pairs)
    ctx = _lib.default_context(None)
    lib = ctx.lib

    def outs(m=n_pairs):
        return (np.full(n_rows, -1, np.int64), np.full((n_rows, G), -1, np.int64), np.full((m, n_rec), -1.0),
                np.zeros((m, n_rec), np.int64))

    def test(o, first=0, count=n_pairs, roff_=roff, rows_=rows, seg_=seg, n_groups=G, x_=x, n_rec_=n_rec):
        return lib.scape_hip_report_perm_len_pairs(ctx.h, n_rec_, ptr(roff_, P_i64), ptr(rows_, P_i64), n_groups,
                                                   ptr(seg_, P_i32), first, count, ptr(x_, P_d), ptr(o[0], P_i64),
                                                   ptr(o[1], P_i64), ptr(o[2], P_d), ptr(o[3], P_i64))
    try:
        lib.scape_hip_report_free(ctx.h)
        assert test(outs()) != 0 and "report_counts" in _lib.last_error()
        assert np.array_equal(rc.device_counts(ctx, Ks, off, lab, cb, n_cols), dense.sum(axis=1))
        assert test(outs()) != 0 and "pair_masks" in _lib.last_error()   # counts, but no pair masks yet
        chk(dpp._pair_masks(ctx, sizes, pairs, 1, n_perm, seed), "pair_masks")
        one = outs()
        chk(test(one), "perm_len_pairs")
        sub = dense[rows]
        a0_want = np.stack([sub[:, seg[g]:seg[g + 1]].sum(axis=1) for g in range(G)], axis=1)
        assert np.array_equal(one[0], a0_want.sum(axis=1)) and np.array_equal(one[1], a0_want)
        assert_items_equal_oracle(wants, one[3], one[2])
        if n_pairs >= 2:                                             # the pairs in two ranges
            cut = n_pairs // 2
            lo, hi = outs(cut), outs(n_pairs - cut)
            chk(test(lo, 0, cut), "perm_len_pairs")
            chk(test(hi, cut, n_pairs - cut), "perm_len_pairs")
            assert np.array_equal(np.concatenate([lo[3], hi[3]]), one[3])
            assert np.array_equal(np.concatenate([lo[2], hi[2]]).view(np.uint64), one[2].view(np.uint64))
        acc = outs()                                                 # the permutations in two chunks that accumulate
        for p_first, p_count in ((1, 100), (101, n_perm - 100)):
            chk(dpp._pair_masks(ctx, sizes, pairs, p_first, p_count, seed), "pair_masks")
            chk(test(acc), "perm_len_pairs")
        assert np.array_equal(acc[3], one[3]) and np.array_equal(acc[2].view(np.uint64), one[2].view(np.uint64))
        chk(dpp._pair_masks(ctx, sizes, pairs, 1, n_perm, seed), "pair_masks")
        # refusals, each before anything is queued: outputs untouched, masks and counts usable afterwards
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
        for k in (8, 9, 10, 11, 12):                                 # x and every output, NULL in turn
            a = [ctx.h, n_rec, ptr(roff, P_i64), ptr(rows, P_i64), G, ptr(seg, P_i32), 0, n_pairs, ptr(x, P_d),
                 ptr(o[0], P_i64), ptr(o[1], P_i64), ptr(o[2], P_d), ptr(o[3], P_i64)]
            a[k] = None
            assert lib.scape_hip_report_perm_len_pairs(*a) != 0 and "bad argument" in _lib.last_error(), k
        for bad in (np.nan, np.inf, -np.inf):
            bad_x = x.copy()
            bad_x[roff[2] + 3] = bad
            assert test(o, x_=bad_x) != 0 and "record 2" in _lib.last_error() and "finite" in _lib.last_error(), bad
        bad_x = x.copy()
        bad_x[roff[3]], bad_x[roff[3] + 1] = 1.5e308, -1.5e308        # finite, their difference is not
        assert test(o, x_=bad_x) != 0 and "record 3" in _lib.last_error() and "span" in _lib.last_error()
        many = (np.zeros(1025, np.int64), np.zeros((1025, G), np.int64), np.zeros((n_pairs, 1)),
                np.zeros((n_pairs, 1), np.int64))
        assert test(many, roff_=np.array([0, 1025], np.int64), rows_=np.zeros(1025, np.int64), x_=np.zeros(1025),
                    n_rec_=1) != 0 and "more than 1024 rows" in _lib.last_error()
        assert np.all(o[0] == -1) and np.all(o[1] == -1) and np.all(o[2] == -1.0) and not o[3].any()
        again = outs()
        chk(test(again), "perm_len_pairs")                           # a refused call keeps masks and counts
        assert np.array_equal(again[3], one[3]) and np.array_equal(again[2].view(np.uint64), one[2].view(np.uint64))
        # scape_hip_report_perm_len on each pair's own two populations, their columns moved to the front
        for k, (g, h) in enumerate(pairs):
            front = list(range(seg[g], seg[g + 1])) + list(range(seg[h], seg[h + 1]))
            assert_item_is_perm_len(ctx, Ks, off, lab, to_front(front, n_cols)[cb], n_cols, sizes[g], sizes[h], n_perm,
                                    seed, rows, roff, x, wants[k], one[3][k], one[2][k])
    finally:
        lib.scape_hip_report_free(ctx.h)


# ---------------------------------------------------------------- GPU: the command
def blocks_of(text, header, n_group_cols):
    """header check; {the group fields: the lines of that block}, the blocks in file order"""
    rows = list(csv.reader(io.StringIO(text)))
    assert rows[0] == header
    out, last = {}, None
    for r in rows[1:]:
        key = tuple(r[1:1 + n_group_cols])
        assert key == last or key not in out                         # an item's lines are one contiguous block
        out.setdefault(key, []).append(r)
        last = key
    return out


def len_line(row, n_group_cols):
    """a line in diff_pa_len's layout: the group fields taken out"""
    return row[:1] + row[1 + n_group_cols:]


def assert_blocks_are_diff_pa_len(root, clu, res, text, header, items, n_perm, seed, oracles=None):
    """items = [(group fields, idents_1, idents_2 or None)] in the order of the file's blocks.  Every block equals the
    file of diff_pa_len on that item as text, p_val_adj aside (an item whose file has no line has no block); n_ge equals
    the oracle's lo where oracles[group fields] gives its lines (lo == hi asserted first); p_val_adj equals rc.bh over
    all lines of the file.  Returns the blocks"""
    n_group_cols = len(items[0][0])
    blocks = blocks_of(text, header, n_group_cols)
    want_keys = []
    for key, id1, id2 in items:
        want = list(csv.reader(io.StringIO(rc.perm_command("diff_pa_len", root, clu, res, id1, id2, n_perm, seed))))[1:]
        if oracles is not None:
            dl.assert_no_near_tie(oracles[key], key)
            assert [(r[0], int(r[LEN_HEADER.index("n_ge")])) for r in want] == [(ln["gene"], ln["lo"]) for ln in oracles[key]]
        if not want:
            continue
        want_keys.append(tuple(key))
        got = blocks[tuple(key)]
        assert len(got) == len(want), key
        for a, b in zip(got, want):
            a = len_line(a, n_group_cols)
            assert a[:ADJ] + a[ADJ + 1:] == b[:ADJ] + b[ADJ + 1:], (key, a, b)
            for name in ("exp_length.1", "exp_length.2", "delta_exp_length", "mean_pos.1", "mean_pos.2", "delta_pos", "n_ge"):
                assert a[LEN_HEADER.index(name)] == b[LEN_HEADER.index(name)], (key, name)
    assert list(blocks) == want_keys
    body = [len_line(r, n_group_cols) for b in blocks.values() for r in b]
    adj = rc.bh([Fraction(1 + int(r[LEN_HEADER.index("n_ge")]), 1 + n_perm) for r in body])
    for r, want in zip(body, adj):
        assert rc.close(r[ADJ], want), r
        assert r[LEN_HEADER.index("n_perm")] == str(n_perm)
    return blocks


def _pair_items(names):
    return [((names[g], names[h]), names[g], names[h]) for g, h in dpp.pair_list(len(names))]


@pytest.mark.gpu
def test_synthetic_directory(tmp_path):
    """clusters B, A and C (301, 230 and 40 cells) in the cluster file's order, 257 permutations: three blocks in pair
    order, each diff_pa_len's file on that pair, 36 lines each, n_ge the exact oracle's; --idents A --idents B gives one
    block; the idents reversed give the same genes, sites and read counts with delta_pos negated and the .1 / .2 columns
    swapped (n_ge is that of `diff_pa_len --idents_1 B --idents_2 A`, whose relabellings put B's cells at the first local
    positions: it equals the oracle on (B, A), not the count of (A, B))"""
    clu = rc.write_synthetic(tmp_path)
    names = dpp.syn_names()
    text = _command(tmp_path, clu, "res.gene.pkl", (), SYN_PERM, SYN_SEED)
    items = _pair_items(names)
    oracles = {key: syn_oracle(id1, id2) for key, id1, id2 in items}
    blocks = assert_blocks_are_diff_pa_len(tmp_path, clu, "res.gene.pkl", text, HEADER, items, SYN_PERM, SYN_SEED, oracles)
    assert list(blocks) == [(names[g], names[h]) for g, h in dpp.pair_list(3)]
    ix = {name: HEADER.index(name) for name in HEADER}
    for (a, b), got in blocks.items():
        assert len(got) == 36 and {r[ix["versus"]] for r in got} == {f"{a}_Vs_{b}"}
        assert {(r[ix["group_1"]], r[ix["group_2"]]) for r in got} == {(a, b)}
    assert len({r[ix["n_ge"]] for got in blocks.values() for r in got}) > 20
    two = _command(tmp_path, clu, "res.gene.pkl", ("A", "B"), SYN_PERM, SYN_SEED)
    assert os.path.basename(_path(tmp_path, clu, "res.gene.pkl", ("A", "B"))) == "syn_groups.gene.A+B.diff_pa_len_pairs.csv"
    one = assert_blocks_are_diff_pa_len(tmp_path, clu, "res.gene.pkl", two, HEADER, _pair_items(("A", "B")), SYN_PERM,
                                        SYN_SEED, {("A", "B"): syn_oracle("A", "B")})
    assert list(one) == [("A", "B")]
    back = assert_blocks_are_diff_pa_len(tmp_path, clu, "res.gene.pkl",
                                         _command(tmp_path, clu, "res.gene.pkl", ("B", "A"), SYN_PERM, SYN_SEED), HEADER,
                                         _pair_items(("B", "A")), SYN_PERM, SYN_SEED, {("B", "A"): syn_oracle("B", "A")})
    assert list(back) == [("B", "A")] and len(back[("B", "A")]) == len(one[("A", "B")]) == 36
    for r, s in zip(back[("B", "A")], one[("A", "B")]):
        assert r[0] == s[0] and r[ix["num_pa"]] == s[ix["num_pa"]]
        for f in ("reads", "mean_pos", "exp_length"):
            assert (r[ix[f + ".1"]], r[ix[f + ".2"]]) == (s[ix[f + ".2"]], s[ix[f + ".1"]]), f
        assert float(r[ix["delta_pos"]]) == -float(s[ix["delta_pos"]])
    same = blocks.get(("B", "A"))                  # the same pair alone and among three: only the adjustment differs
    assert same is not None
    drop = lambda r: r[:ix["p_val_adj"]] + r[ix["p_val_adj"] + 1:]
    assert [drop(r) for r in same] == [drop(r) for r in back[("B", "A")]]


@pytest.mark.gpu
@pytest.mark.parametrize("n_perm", [1, 255, 256, 257])
def test_tile_edges(n_perm, tmp_path):
    """a workgroup of the test kernel takes 256 permutations: one, one short of a tile, a full tile, one over"""
    clu = rc.write_synthetic(tmp_path, 12)
    text = _command(tmp_path, clu, "res.gene.pkl", (), n_perm, 5)
    items = _pair_items(dpp.syn_names())
    oracles = {key: syn_oracle(id1, id2, n_perm, 5, 12) for key, id1, id2 in items}
    assert len(assert_blocks_are_diff_pa_len(tmp_path, clu, "res.gene.pkl", text, HEADER, items, n_perm, 5, oracles)) == 3


def assert_invariance(tmp_path, monkeypatch, cmd, masks_name, test_name, masks_args, perm_bytes, chunks):
    """records over several count batches, the permutations over several chunks, the items over several ranges: the same
    bytes, with the calls counted"""
    from scape_amd import _lib, report
    clu = rc.write_synthetic(tmp_path)
    big = _command(tmp_path, clu, "res.gene.pkl", (), SYN_PERM, SYN_SEED, cmd=cmd)
    lib = _lib.load_library()
    calls = {"masks": [], "test": []}
    real_m, real_t = getattr(lib, masks_name), getattr(lib, test_name)

    def masks(*a):
        calls["masks"].append((a[masks_args], a[masks_args + 1]))
        return real_m(*a)

    def test(*a):
        calls["test"].append((a[6], a[7]))
        return real_t(*a)
    monkeypatch.setattr(lib, masks_name, masks)
    monkeypatch.setattr(lib, test_name, test)
    assert _command(tmp_path, clu, "res.gene.pkl", (), SYN_PERM, SYN_SEED, cmd=cmd) == big
    assert calls["masks"] == [(1, SYN_PERM)] and calls["test"] == [(0, 3)]
    calls.update(masks=[], test=[])
    monkeypatch.setattr(report, "MAX_BATCH_BYTES", 1 << 16)             # a record of K = 8 alone takes 57 KB
    monkeypatch.setattr(report, "MAX_PERM_BYTES", 1 << 30)
    assert _command(tmp_path, clu, "res.gene.pkl", (), SYN_PERM, SYN_SEED, cmd=cmd) == big
    assert calls["masks"] == [(1, SYN_PERM)] and len(calls["test"]) > 5
    n_batches = len(calls["test"])
    calls.update(masks=[], test=[])
    monkeypatch.setattr(report, "MAX_PERM_BYTES", perm_bytes)
    assert _command(tmp_path, clu, "res.gene.pkl", (), SYN_PERM, SYN_SEED, cmd=cmd) == big
    assert len(calls["test"]) == len(chunks) * n_batches and calls["masks"][:len(chunks)] == chunks
    calls.update(masks=[], test=[])
    monkeypatch.setattr(report, "MAX_PERM_BYTES", 1 << 30)
    monkeypatch.setattr(report, "MAX_LEN_BLOCK_RESULT_BYTES", 1)       # one item per call
    assert _command(tmp_path, clu, "res.gene.pkl", (), SYN_PERM, SYN_SEED, cmd=cmd) == big
    assert calls["test"][:3] == [(0, 1), (1, 1), (2, 1)] and len(calls["test"]) == 3 * n_batches


@pytest.mark.gpu
def test_batch_chunk_and_range_invariance(tmp_path, monkeypatch):
    # per permutation: pairs of 531, 270 and 341 cells = 9 + 5 + 6 words and 3 key bounds; room for 100 permutations
    assert_invariance(tmp_path, monkeypatch, "diff_pa_len_pairs", "scape_hip_report_perm_pair_masks",
                      "scape_hip_report_perm_len_pairs", 6, (20 + 3) * 8 * 100, [(1, 100), (101, 100), (201, 57)])


@pytest.mark.gpu
def test_failed_run_leaves_no_part_file(tmp_path, monkeypatch):
    from scape_amd import _lib
    clu = rc.write_synthetic(tmp_path, 12)
    lib = _lib.load_library()
    monkeypatch.setattr(lib, "scape_hip_report_perm_len_pairs", lambda *a: 1)
    r = rc.run(_args(tmp_path, clu, n_perm=10))
    assert r.exit_code != 0 and isinstance(r.exception, _lib.ScapeHipError), repr(r.exception)
    assert not rc.parts_left(tmp_path) and not os.path.exists(_path(tmp_path, clu, "res.gene.pkl"))


@pytest.mark.gpu
def test_non_finite_position_is_refused(tmp_path):
    """a NaN position of a pA site with reads in a tested cell: diff_pa_len's ValueError naming the record, no file"""
    path, _clu, _bc, _recs = dl._two_group_dir(tmp_path, [[30, 200, 410], [25.0, float("nan"), 300.0]])
    r = rc.run(_args(tmp_path, path, n_perm=50))
    assert isinstance(r.exception, ValueError) and "TG1" in str(r.exception), repr(r.exception)
    assert not rc.parts_left(tmp_path) and not os.path.exists(_path(tmp_path, path, "res.gene.pkl"))
