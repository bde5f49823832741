"""`--strata_file` of `scape diff_pa` / `scape diff_pa_len`: cell labels permuted within strata only (scape_amd/report.py;
kernel k_rep_perm_mask_strata and the entry points scape_hip_report_perm_masks_strata / _perm_bits_get of
scape_amd/csrc/perm.inc; include/scape_hip.h states the labelling scheme).

The scheme, restated here in plain Python ints (nothing below imports from scape_amd outside the tests that run it):
population 1's positions first, then population 2's, each ordered by stratum (first appearance among the rows of the
strata file, columns ascending within a stratum); stratum s owns [o1, o1 + m1[s]) and [n1 + o2, n1 + o2 + m2[s]);
permutation p >= 1 gives population 1, per stratum, the m1[s] positions of the stratum with the smallest rc.key(seed, p,
j), j the global position.  Tested cells without a stratum are left out of both populations.

The statistics are those of tests/test_report_diffpa.py and tests/test_report_difflen.py: their exact oracles are
reused with `members` replaced (monkeypatch) by the stratified selection below.  As there, every GPU test that compares
counts first asserts lo == hi on the oracle alone (no labelling within 2^-39 of a tie), then that the device's counts
EQUAL lo; the generator seeds were picked on a CPU so that this holds, and no case is excused.

Sizes: the device takes a stratum of up to 64 cells with one key per lane of a wave, one of 65..256 cells with four keys
per lane, a larger one with the workgroup's radix select, whose number of passes grows with the stratum (about
log256(cells) + 1); a stratum without a cell of one population takes none of them.  The layouts below put strata on
both sides of 64 and of 256, and one of 3,000 cells; test_bits_behind_deep_selects pins permutations whose select needs
three and four passes."""
import csv
import functools
import io
import os

import numpy as np
import pytest

import report_cases as rc
import test_report_difflen as dl
import test_report_diffpa as dp
from report_cases import no_gpu  # noqa: F401  (fixture)


# ---------------------------------------------------------------- the scheme, restated
def stratified_members(m1, m2):
    """members(seed, p, n1, n) for strata of m1[s] + m2[s] cells: per stratum the m1[s] smallest keys"""
    m1, m2 = [int(v) for v in m1], [int(v) for v in m2]

    def members(seed, p, n1, n):
        assert n1 == sum(m1) and n == n1 + sum(m2)
        out, o1, o2 = [], 0, n1
        for a, b in zip(m1, m2):
            pos = list(range(o1, o1 + a)) + list(range(o2, o2 + b))
            out += sorted(pos, key=lambda j: rc.key(seed, p, j))[:a]
            o1, o2 = o1 + a, o2 + b
        return out
    return members


def stratified_populations(bc, clu_text, strata_text, id1, id2):
    """(columns of population 1 in position order, those of population 2, m1, m2, tested cells without a stratum)"""
    last = {}
    for i, name in rc.cluster_rows(strata_text):
        last[i] = name
    col_stratum = [last.get(i, "") for i in rc.column_ids(bc)]
    order = rc.first_clusters(strata_text)
    c1, c2 = rc.populations(bc, clu_text, id1, id2)
    left_out = sum(col_stratum[j] == "" for j in c1 + c2)
    used = [s for s in order if any(col_stratum[j] == s for j in c1 + c2)]
    by = lambda cols: [[j for j in cols if col_stratum[j] == s] for s in used]
    p1, p2 = by(c1), by(c2)
    return (sum(p1, []), sum(p2, []), [len(x) for x in p1], [len(x) for x in p2], left_out)


def words_of(member_positions, n):
    w = [0] * ((n + 63) // 64)
    for j in member_positions:
        w[j // 64] |= 1 << (j % 64)
    return w


# ---------------------------------------------------------------- CPU: the restatement itself
@pytest.mark.parametrize("n1,n2,seed", [(1, 1, 0), (70, 91, 77), (230, 301, 1), (5, 700, 12345)])
def test_one_stratum_is_the_free_selection(n1, n2, seed):
    for p in (1, 2, 300):
        assert sorted(stratified_members([n1], [n2])(seed, p, n1, n1 + n2)) == sorted(rc.members(seed, p, n1, n1 + n2))


@pytest.mark.parametrize("m1,m2", [([1, 0, 30, 25, 14], [0, 2, 33, 40, 16]), ([0, 5], [3, 1]), ([4, 1], [0, 1]),
                                   ([1] * 7, [1] * 7), ([3, 0, 0, 2], [0, 4, 1, 2])])
def test_every_stratum_keeps_its_count(m1, m2):
    n1, n = sum(m1), sum(m1) + sum(m2)
    seen = set()
    for p in (1, 2, 3, 999):
        mem = stratified_members(m1, m2)(5, p, n1, n)
        assert len(mem) == len(set(mem)) == n1
        o1, o2 = 0, n1
        for a, b in zip(m1, m2):
            own = set(range(o1, o1 + a)) | set(range(o2, o2 + b))
            assert len(own & set(mem)) == a
            if a == 0 or b == 0:                          # nobody to swap with: the cells keep their labels
                assert own & set(mem) == set(range(o1, o1 + a))
            o1, o2 = o1 + a, o2 + b
        seen.add(tuple(sorted(mem)))
    assert len(seen) > 1


def test_positions_follow_the_strata_file(tmp_path):
    bc = "CB,index\n" + "".join(f"c{j},{10 + j}\n" for j in range(8))
    clu = "index,g\n" + "".join(f"{10 + j},{'A' if j in (0, 3, 4, 6) else 'B'}\n" for j in range(8))
    strata = "index,s\n13,y\n10,x\n11,y\n12,\n14,x\n15,y\n16,y\n17,x\n10,y\n"       # id 10: its last row counts; id 12: none
    c1, c2, m1, m2, left = stratified_populations(bc, clu, strata, "A", "B")
    assert (c1, c2, m1, m2, left) == ([0, 3, 6, 4], [1, 5, 7], [3, 1], [2, 1], 1)
    from scape_amd import report
    pops = [("Population1", np.array([0, 3, 4, 6])), ("Population2", np.array([1, 2, 5, 7]))]
    (tmp_path / "s.csv").write_text(strata)
    got, g1, g2, gl = report._strata(np.arange(10, 18), pops, str(tmp_path / "s.csv"))
    assert [c.tolist() for _n, c in got] == [c1, c2] and g1.tolist() == m1 and g2.tolist() == m2 and gl == left
    assert abs(report._log10_labellings(np.array([3, 1]), np.array([2, 1])) - np.log10(10 * 2)) < 1e-12


@pytest.mark.parametrize("cmd", ["diff_pa", "diff_pa_len"])
def test_help_lists_the_option(cmd):
    r = rc.run([cmd, "--help"])
    assert r.exit_code == 0 and "--strata_file" in r.output, r.output


@pytest.mark.parametrize("cmd", ["diff_pa", "diff_pa_len"])
def test_prerequisite_errors(cmd, tmp_path, no_gpu):
    clu, strata = tmp_path / "groups.csv", tmp_path / "strata.csv"
    (tmp_path / "res.gene.pkl").write_bytes(b"")
    (tmp_path / "barcode_index.csv").write_text("CB,index\nA-1,3\nB-1,4\nC-1,5\nD-1,6\n")
    clu.write_text("index,group\n3,A\n4,B\n5,A\n6,B\n")

    def err(text):
        if text is not None:
            strata.write_text(text)
        r = rc.run(rc.perm_args(cmd, tmp_path, clu, id1="A", id2="B", n_perm=9) + ["--strata_file", str(strata)])
        assert r.exit_code != 0 and isinstance(r.exception, ValueError), (text, r.output, repr(r.exception))
        return str(r.exception)
    assert "strata_file" in err(None) and "does not exist" in err(None)                   # the file is missing
    assert "Population1" in err("index,s\n3,\n4,x\n6,x\n") and "has no cell" in err("index,s\n3,\n4,x\n6,x\n")
    assert "Population2" in err("index,s\n3,x\n5,y\n") and "has no cell" in err("index,s\n3,x\n5,y\n")
    assert "both populations" in err("index,s\n3,x\n5,x\n4,y\n6,z\n")                    # nothing can be relabelled
    assert sorted(os.listdir(tmp_path)) == ["barcode_index.csv", "groups.csv", "res.gene.pkl", "strata.csv"]


# ---------------------------------------------------------------- GPU: the entry points
def _bits(ctx, p, n):
    import ctypes
    from scape_amd._lib import check as chk
    w = np.zeros((n + 63) // 64, dtype=np.uint64)
    chk(ctx.lib.scape_hip_report_perm_bits_get(ctx.h, p, w.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))), "bits_get")
    return [int(v) for v in w]


def _masks_strata(ctx, m1, m2, p_first, p_count, seed):
    from scape_amd._lib import P_i32, ptr
    a, b = np.asarray(m1, dtype=np.int32), np.asarray(m2, dtype=np.int32)
    return ctx.lib.scape_hip_report_perm_masks_strata(ctx.h, len(a), ptr(a, P_i32), ptr(b, P_i32), p_first, p_count, seed)


# strata of the 70 + 91 tested columns of rc.entry_point_matrix(): (m1, m2) per layout
LAYOUTS = {
    # 1, 2, 63, 65 and 30 cells; one stratum without population 2, one without population 1; population 1's range of the
    # last stratum is [56, 70) and population 2's range of the fourth is 70 + [35, 75): both cross a 64-bit word
    "1-2-63-65-30": ([1, 0, 30, 25, 14], [0, 2, 33, 40, 16]),
    "64-97": ([20, 50], [44, 47]),
    "135-26": ([60, 10], [75, 16]),
}
EP_PERMS = 257


@functools.lru_cache(maxsize=None)
def _entry_oracle(layout):
    """the exact counts of diff_pa's statistic on the entry point matrix under the layout's labellings: per record a
    dp._Rec; its counts after permutation 1 and after all EP_PERMS"""
    n1, n2, _n_cols, seed, _n_perm, Ks, _off, _lab, _cb, dense, rows, roff, _rng = rc.entry_point_matrix()
    m1, m2 = LAYOUTS[layout]
    assert sum(m1) == n1 and sum(m2) == n2
    n = n1 + n2
    sub = dense[rows][:, :n]
    recs = []
    for r in range(len(Ks)):
        nzs = [[(j, int(v)) for j, v in enumerate(row) if v] for row in sub[roff[r]:roff[r + 1]].tolist()]
        recs.append(dp._Rec(f"r{r}", [str(i) for i in range(len(nzs))], nzs, n1))
    pick = stratified_members(m1, m2)
    mem, first = [], None
    for p in range(1, EP_PERMS + 1):
        pop1 = pick(seed, p, n1, n)
        mem.append(pop1)
        member = bytearray(n)
        for j in pop1:
            member[j] = 1
        for rec in recs:
            rec.count(member)
        if p == 1:
            first = ([s[0] for rec in recs for s in rec.site], [rec.gene_ge[0] for rec in recs])
    for rec in recs:
        assert all(lo == hi for lo, hi in rec.site) and rec.gene_ge[0] == rec.gene_ge[1], (layout, rec.gene)
    return mem, first, ([s[0] for rec in recs for s in rec.site], [rec.gene_ge[0] for rec in recs])


def test_entry_oracle_has_no_near_tie():
    for layout in LAYOUTS:
        _mem, _first, (site, gene) = _entry_oracle(layout)
        assert 0 < min(gene) and max(gene) < EP_PERMS and min(site) < max(site)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_entry_point(layout):
    """scape_hip_report_perm_masks_strata on rc.entry_point_matrix(): the words of every permutation equal the Python
    membership (p_count 1 and 257, and a chunk that starts at permutation 200), then scape_hip_report_perm_test behind
    them gives the exact oracle's counts"""
    from scape_amd import _lib
    from scape_amd._lib import P_d, P_i64, check as chk, ptr
    n1, n2, n_cols, seed, _n_perm, Ks, off, lab, cb, dense, rows, roff, _rng = rc.entry_point_matrix()
    n = n1 + n2
    m1, m2 = LAYOUTS[layout]
    mem, first, full = _entry_oracle(layout)
    ctx = _lib.default_context(None)
    lib = ctx.lib

    def test():
        o = (np.zeros(len(rows), np.int64), np.zeros(len(rows), np.int64), np.zeros(len(rows), np.int64),
             np.zeros(len(Ks)), np.zeros(len(Ks), np.int64))
        chk(lib.scape_hip_report_perm_test(ctx.h, len(Ks), ptr(roff, P_i64), ptr(rows, P_i64), ptr(o[0], P_i64),
                                           ptr(o[1], P_i64), ptr(o[2], P_i64), ptr(o[3], P_d), ptr(o[4], P_i64)),
            "perm_test")
        return o[2].tolist(), o[4].tolist()
    try:
        assert np.array_equal(rc.device_counts(ctx, Ks, off, lab, cb, n_cols), dense.sum(axis=1))
        for p_first, p_count, want in ((1, 1, first), (200, 58, None), (1, EP_PERMS, full)):
            chk(_masks_strata(ctx, m1, m2, p_first, p_count, seed), "perm_masks_strata")
            bad = [p for p in range(p_count) if _bits(ctx, p, n) != words_of(mem[p_first - 1 + p], n)]
            print(layout, "p_first", p_first, "p_count", p_count, "permutations with other bits:", bad[:10])
            assert not bad
            if want is not None:
                site, gene = test()
                print("site counts equal", site == want[0], "record counts equal", gene == want[1])
                assert site == want[0] and gene == want[1]
        assert lib.scape_hip_report_perm_bits_get(ctx.h, EP_PERMS, None) != 0
    finally:
        lib.scape_hip_report_free(ctx.h)


# strata around the sizes at which the kernel changes its path: (m1, m2), permutations
SIZE_LAYOUTS = {
    "256-257": ([100, 128, 3], [156, 129, 1], 40),                 # four keys per lane at its limit; the smallest select
    "3000-only-one-population": ([1400, 300, 0, 2], [1600, 0, 270, 3], 6),     # more select passes; large fixed strata
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SIZE_LAYOUTS))
def test_bits_at_the_path_thresholds(name):
    from scape_amd import _lib
    from scape_amd._lib import check as chk
    m1, m2, n_perm = SIZE_LAYOUTS[name]
    n1, n = sum(m1), sum(m1) + sum(m2)
    pick = stratified_members(m1, m2)
    ctx = _lib.default_context(None)
    try:
        chk(_masks_strata(ctx, m1, m2, 1, n_perm, 3), "perm_masks_strata")
        bad = [p for p in range(1, n_perm + 1) if _bits(ctx, p - 1, n) != words_of(pick(3, p, n1, n), n)]
        print(name, "permutations with other bits:", bad)
        assert not bad
    finally:
        ctx.lib.scape_hip_report_free(ctx.h)


def select_passes(keys, rank):
    """histogram passes of the device's radix select for the key of that rank: it stops after the first byte at which the
    key is alone in its bin, so 1 + the larger number of leading bytes it shares with either sorted neighbour"""
    ks = sorted(keys)

    def shared(a, b):
        n = 0
        while n < 8 and (a >> (56 - 8 * n)) & 255 == (b >> (56 - 8 * n)) & 255:
            n += 1
        return n
    return 1 + max(shared(ks[rank], ks[i]) for i in (rank - 1, rank + 1) if 0 <= i < len(ks))


# (p_first, p_count, the labelling whose select goes deep, its passes): seed 3, 1,500 + 2,500 cells, freely or within
# the two strata below.  Found on a CPU with select_passes: of the free permutations 1 .. 200,000, 188,055 settle in 2
# passes, 11,894 need 3 and 51 need 4, the first of them 27 and 3,130; within the strata both chunks settle in 2, and
# 17 is the first permutation with a stratum that needs 3
DEEP_CHUNKS = ((25, 4, "free", 3), (3128, 4, "free", 4), (17, 4, "strata", 3))
DEEP_STRATA = ([700, 800], [1200, 1300])


@pytest.mark.gpu
@pytest.mark.parametrize("p_first,p_count,deep,n_passes", DEEP_CHUNKS)
def test_bits_behind_deep_selects(p_first, p_count, deep, n_passes):
    """the one radix select past its second histogram pass: every permutation of the chunk, from
    scape_hip_report_perm_masks and from scape_hip_report_perm_masks_strata with two strata, against the Python
    membership; the chunk is first shown to hold a select of n_passes passes"""
    from scape_amd import _lib
    from scape_amd._lib import check as chk
    seed, (m1, m2) = 3, DEEP_STRATA
    n1, n = sum(m1), sum(m1) + sum(m2)
    assert (n1, n) == (1500, 4000)
    perms = range(p_first, p_first + p_count)
    keys = {p: [rc.key(seed, p, j) for j in range(n)] for p in perms}
    free = [select_passes(keys[p], n1 - 1) for p in perms]
    cells = [list(range(0, 700)) + list(range(1500, 2700)), list(range(700, 1500)) + list(range(2700, 4000))]
    strata = [max(select_passes([keys[p][j] for j in pos], a - 1) for pos, a in zip(cells, m1)) for p in perms]
    print("chunk", p_first, p_count, "select passes, free:", free, "largest per stratum:", strata)
    assert max(free if deep == "free" else strata) >= n_passes
    pick = stratified_members(m1, m2)
    ctx = _lib.default_context(None)
    try:
        chk(ctx.lib.scape_hip_report_perm_masks(ctx.h, n1, n - n1, p_first, p_count, seed), "perm_masks")
        bad = [p for p in perms if _bits(ctx, p - p_first, n) != words_of(rc.members(seed, p, n1, n), n)]
        print("free permutations with other bits:", bad)
        assert not bad
        chk(_masks_strata(ctx, m1, m2, p_first, p_count, seed), "perm_masks_strata")
        bad = [p for p in perms if _bits(ctx, p - p_first, n) != words_of(pick(seed, p, n1, n), n)]
        print("stratified permutations with other bits:", bad)
        assert not bad
    finally:
        ctx.lib.scape_hip_report_free(ctx.h)


@pytest.mark.gpu
def test_one_stratum_is_perm_masks_and_argument_errors():
    """scape_hip_report_perm_masks and scape_hip_report_perm_masks_strata with one stratum give identical words (both
    read through scape_hip_report_perm_bits_get); every refused argument returns non-zero with a message"""
    from scape_amd import _lib
    from scape_amd._lib import check as chk
    ctx = _lib.default_context(None)
    lib = ctx.lib
    try:
        for n1, n2, seed, p_first, p_count in ((70, 91, 77, 1, 257), (1, 1, 0, 1, 3), (300, 401, rc.M64, 5, 20)):
            n = n1 + n2
            chk(lib.scape_hip_report_perm_masks(ctx.h, n1, n2, p_first, p_count, seed), "perm_masks")
            free = [_bits(ctx, p, n) for p in range(p_count)]
            chk(_masks_strata(ctx, [n1], [n2], p_first, p_count, seed), "perm_masks_strata")
            blocked = [_bits(ctx, p, n) for p in range(p_count)]
            assert free == blocked, (n1, n2)
            assert free[0] == words_of(rc.members(seed, p_first, n1, n), n)
        for args, word in ((([], [], 1, 1, 0), "at least one stratum"), (([3, -1], [2, 4], 1, 1, 0), "negative"),
                           (([3, 2], [2, -4], 1, 1, 0), "negative"), (([3, 0], [2, 0], 1, 1, 0), "no cell"),
                           (([0, 0], [2, 3], 1, 1, 0), "at least one cell"), (([2, 3], [0, 0], 1, 1, 0), "at least one cell"),
                           (([1 << 23], [1 << 23], 1, 1, 0), "2^24"), (([1 << 23, 5], [1 << 22, 1 << 22], 1, 1, 0), "2^24"),
                           (([3], [2], 0, 1, 0), "p_first"), (([3], [2], 1, 0, 0), "p_count")):
            assert _masks_strata(ctx, *args) != 0 and word in _lib.last_error(), (args, _lib.last_error())
        assert lib.scape_hip_report_perm_masks_strata(ctx.h, 1, None, None, 1, 1, 0) != 0
        assert lib.scape_hip_report_perm_masks_strata(None, 1, None, None, 1, 1, 0) != 0
        assert _bits(ctx, 19, 701) == blocked[19]                                  # a refused call keeps the earlier masks
        import ctypes
        w = np.zeros(11, dtype=np.uint64)
        wp = w.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))
        for p in (-1, 20):
            assert lib.scape_hip_report_perm_bits_get(ctx.h, p, wp) != 0 and "last masks call" in _lib.last_error()
        lib.scape_hip_report_free(ctx.h)
        assert lib.scape_hip_report_perm_bits_get(ctx.h, 0, wp) != 0 and "perm_masks" in _lib.last_error()
    finally:
        lib.scape_hip_report_free(ctx.h)


# ---------------------------------------------------------------- GPU: the commands
def _command(cmd, root, clu, res, id1, id2, n_perm, seed, strata=None, what=""):
    """the text of the file the command writes, with --strata_file when given"""
    a = rc.perm_args(cmd, root, clu, res, id1, id2, n_perm, seed)
    path = rc.perm_path(cmd, root, clu, res, id1, id2)
    if strata is not None:
        a += ["--strata_file", str(strata)]
        stem = os.path.splitext(os.path.basename(str(strata)))[0]
        path = path[:-len(f".{cmd}.csv")] + f".by_{stem}.{cmd}.csv"
    r = rc.run(a)
    assert r.exit_code == 0, (what, r.output, repr(r.exception))
    assert not rc.parts_left(root)
    with open(path, newline="") as fh:
        return fh.read(), r.output


SYN_STRATA_SEED = 3
SYN_PERM_SEED = 1
SYN_PERMS = 257


@functools.lru_cache(maxsize=None)
def _syn_strata_text():
    """strata of the 600 cells of rc.synthetic(): three large uneven ones whose shares differ between the clusters, one
    that holds cells of cluster A only, one of 3 cells; about 6 % of the cells have an empty stratum and 3 % no row"""
    _records, bc, clu_text = rc.synthetic()
    rng = np.random.default_rng(SYN_STRATA_SEED)
    clu = dict(rc.cluster_rows(clu_text))
    ids = rc.column_ids(bc)
    a_ids = [i for i in ids if clu.get(i) == "A"]
    b_ids = [i for i in ids if clu.get(i) == "B"]
    tiny = {a_ids[5], b_ids[7], b_ids[200]}
    rows = []
    for i in ids:
        u, c = rng.random(), clu.get(i, "")
        if i in tiny:
            s = "tiny"
        elif u < 0.03:
            continue
        elif u < 0.09:
            s = ""
        elif c == "A" and u < 0.25:
            s = "onlyA"
        else:
            s = str(rng.choice(["s1", "s2", "s3"], p=[0.6, 0.3, 0.1] if c == "A" else [0.15, 0.35, 0.5]))
        rows.append(f"{i},{s}\n")
    return "index,stratum\n" + "".join(rows[k] for k in rng.permutation(len(rows)).tolist())


@functools.lru_cache(maxsize=None)
def _syn():
    records, bc, clu_text = rc.synthetic()
    c1, c2, m1, m2, left = stratified_populations(bc, clu_text, _syn_strata_text(), "A", "B")
    return dict(bc=bc, clu=clu_text, c1=c1, c2=c2, m1=m1, m2=m2, left=left,
                rec_rows=rc.rec_rows_of(records, rc.column_ids(bc)), recs=dl.dense_of(records, rc.column_ids(bc)))


def test_synthetic_strata_have_the_stated_shape():
    s = _syn()
    sizes = [a + b for a, b in zip(s["m1"], s["m2"])]
    assert len(sizes) == 5 and 3 in sizes and len(set(sizes)) == 5 and s["left"] > 20
    assert sum(b == 0 for b in s["m2"]) == 1 and min(s["m1"]) > 0
    assert sum(s["m1"]) + sum(s["m2"]) + s["left"] == 230 + 301


def _write_syn(root, n_rec=None):
    clu = rc.write_synthetic(root, n_rec)
    strata = os.path.join(str(root), "syn_strata.csv")
    with open(strata, "w") as fh:
        fh.write(_syn_strata_text())
    return clu, strata


@pytest.mark.gpu
def test_diff_pa_on_the_synthetic_directory(tmp_path, monkeypatch):
    s = _syn()
    monkeypatch.setattr(dp, "members", stratified_members(s["m1"], s["m2"]))
    lines = dp.oracle(s["rec_rows"], s["c1"], s["c2"], SYN_PERMS, SYN_PERM_SEED)
    dp.assert_no_near_tie(lines, "syn strata")
    clu, strata = _write_syn(tmp_path)
    text, out = _command("diff_pa", tmp_path, clu, "res.gene.pkl", "A", "B", SYN_PERMS, SYN_PERM_SEED, strata)
    dp.compare(text, lines, "A_Vs_B", SYN_PERMS, "syn strata")
    assert len(lines) > 100
    assert f"{sum(s['m1'])} + {sum(s['m2'])} cells" in out and f"{s['left']} cells" in out and "5 strata" in out


@pytest.mark.gpu
def test_diff_pa_len_on_the_synthetic_directory(tmp_path, monkeypatch):
    s = _syn()
    monkeypatch.setattr(rc, "members", stratified_members(s["m1"], s["m2"]))
    lines = dl.oracle(s["recs"], s["c1"], s["c2"], SYN_PERMS, SYN_PERM_SEED)
    dl.assert_no_near_tie(lines, "syn strata")
    clu, strata = _write_syn(tmp_path)
    text, out = _command("diff_pa_len", tmp_path, clu, "res.gene.pkl", "A", "B", SYN_PERMS, SYN_PERM_SEED, strata)
    dl.compare(text, lines, "A_Vs_B", SYN_PERMS, "syn strata")
    assert len(lines) > 30 and f"{s['left']} cells" in out


@pytest.mark.gpu
@pytest.mark.parametrize("cmd", ["diff_pa", "diff_pa_len"])
def test_one_stratum_gives_the_unstratified_file(cmd, tmp_path):
    _records, bc, _clu = rc.synthetic()
    clu = rc.write_synthetic(tmp_path, 14)
    strata = tmp_path / "everyone.csv"
    strata.write_text("index,s\n" + "".join(f"{i},all\n" for i in rc.column_ids(bc)))
    for id2 in ("B", None):
        free, _ = _command(cmd, tmp_path, clu, "res.gene.pkl", "A", id2, 99, 4)
        blocked, _ = _command(cmd, tmp_path, clu, "res.gene.pkl", "A", id2, 99, 4, strata)
        assert free == blocked and free.count("\n") > 10


@pytest.mark.gpu
@pytest.mark.parametrize("cmd", ["diff_pa", "diff_pa_len"])
def test_chunk_invariance(cmd, tmp_path, monkeypatch):
    """the permutations in chunks of 100 (a permutation takes its words of bits and 5 bounds): the same bytes"""
    from scape_amd import _lib, report
    words = (sum(_syn()["m1"]) + sum(_syn()["m2"]) + 63) // 64
    clu, strata = _write_syn(tmp_path, 14)
    one, _ = _command(cmd, tmp_path, clu, "res.gene.pkl", "A", "B", SYN_PERMS, 2, strata)
    lib = _lib.load_library()
    calls = []
    real = lib.scape_hip_report_perm_masks_strata

    def masks(*a):
        calls.append((a[1], a[4], a[5]))
        return real(*a)
    monkeypatch.setattr(lib, "scape_hip_report_perm_masks_strata", masks)
    monkeypatch.setattr(report, "MAX_PERM_BYTES", (words + 5) * 8 * 100)
    chunked, _ = _command(cmd, tmp_path, clu, "res.gene.pkl", "A", "B", SYN_PERMS, 2, strata)
    assert chunked == one
    assert calls == [(5, 1, 100), (5, 101, 100), (5, 201, 57)]


# ---------------------------------------------------------------- GPU: what the option is for
PURPOSE_SEED = 0
PURPOSE_PERMS = 255


@functools.lru_cache(maxsize=None)
def _purpose(gen_seed=PURPOSE_SEED):
    """200 cells in two strata; cluster A has 80 cells of stratum x and 20 of y, cluster B 20 and 80.  Records 0..7 use
    their first site with probability 0.75 in stratum x and 0.25 in y, whatever the cluster; records 8..11 with 0.75
    in A and 0.25 in B, whatever the stratum.  Each cell has 0..5 reads per record"""
    rng = np.random.default_rng(gen_seed)
    n = 200
    ids = np.arange(n) * 3 + 5
    is_a = np.array([True] * 80 + [False] * 20 + [True] * 20 + [False] * 80)
    in_x = np.arange(n) < 100
    mixo = rng.permutation(n)
    bc = "CB,index\n" + "".join(f"P{j}-1,{i}\n" for j, i in enumerate(ids[mixo].tolist()))
    clu = "index,group\n" + "".join(f"{ids[j]},{'A' if is_a[j] else 'B'}\n" for j in range(n))
    strata = "index,stratum\n" + "".join(f"{ids[j]},{'x' if in_x[j] else 'y'}\n" for j in range(n))
    records = []
    for r in range(12):
        p0 = np.where(in_x if r < 8 else is_a, 0.75, 0.25)
        reads = rng.integers(0, 6, n)
        cell = np.repeat(np.arange(n), reads)
        lab = (rng.random(len(cell)) >= p0[cell]).astype(np.int64)
        records.append(dict(gene_info_str=f"4:PG{r}:1:{900 * r + 1}-{900 * r + 800}:+", K=2,
                            alpha_arr=np.array([100, 500]), beta_arr=np.full(2, 10.0), label_arr=lab,
                            cb_id_arr=ids[cell].astype(np.int64)))
    return records, bc, clu, strata


def _gene_ge(lines):
    return [ln["gene_ge"][0] for ln in lines if ln["first"]]


@functools.lru_cache(maxsize=None)
def _purpose_oracle(blocked):
    records, bc, clu, strata = _purpose()
    rec_rows = rc.rec_rows_of(records, rc.column_ids(bc))
    if blocked:
        c1, c2, m1, m2, left = stratified_populations(bc, clu, strata, "A", "B")
        assert (sorted(m1), sorted(m2), left) == ([20, 80], [20, 80], 0)
        with pytest.MonkeyPatch.context() as mp:
            mp.setattr(dp, "members", stratified_members(m1, m2))
            lines = dp.oracle(rec_rows, c1, c2, PURPOSE_PERMS, 1)
    else:
        c1, c2 = rc.populations(bc, clu, "A", "B")
        lines = dp.oracle(rec_rows, c1, c2, PURPOSE_PERMS, 1)
    dp.assert_no_near_tie(lines, f"purpose/{blocked}")
    return lines


def test_purpose_on_the_oracle():
    """free relabelling calls all 12 records different at the smallest p-value; blocked relabelling keeps the 4 real
    ones there and lets at least 6 of the 8 records that differ by stratum only go (p >= 0.05)"""
    free, blocked = _gene_ge(_purpose_oracle(False)), _gene_ge(_purpose_oracle(True))
    print("gene_n_ge free", free, "blocked", blocked)
    assert len(free) == len(blocked) == 12
    assert free == [0] * 12
    assert blocked[8:] == [0] * 4
    assert sum((1 + ge) / (1 + PURPOSE_PERMS) >= 0.05 for ge in blocked[:8]) >= 6


@pytest.mark.gpu
def test_purpose_on_the_device(tmp_path):
    from scape.apa_core import Parameters
    records, bc, clu, strata = _purpose()
    paths = rc.write_dir(str(tmp_path), "res.gene.pkl", records, bc, {"groups.csv": clu, "cells.csv": strata}, Parameters)
    free, _ = _command("diff_pa", tmp_path, paths[0], "res.gene.pkl", "A", "B", PURPOSE_PERMS, 1)
    dp.compare(free, _purpose_oracle(False), "A_Vs_B", PURPOSE_PERMS, "purpose/free")
    blocked, _ = _command("diff_pa", tmp_path, paths[0], "res.gene.pkl", "A", "B", PURPOSE_PERMS, 1, paths[1])
    dp.compare(blocked, _purpose_oracle(True), "A_Vs_B", PURPOSE_PERMS, "purpose/blocked")
    p_of = lambda text: [float(r[13]) for r in list(csv.reader(io.StringIO(text)))[1::2]]     # two lines per record
    assert p_of(free) == [1 / 256] * 12
    assert p_of(blocked)[8:] == [1 / 256] * 4 and sum(p >= 0.05 for p in p_of(blocked)[:8]) >= 6
