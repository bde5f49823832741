"""`scape boot_pa_len_diff`: percentile bootstrap intervals of the difference of the mean pA position, and of exp_length,
between two cell populations (scape_amd/report.py, section boot_pa_len_diff, boot_pa_usage_diff; kernel
k_rep_boot_len_diff, the entry point scape_hip_report_boot_len_diff and the signed order of k_rep_boot_select in
scape_amd/csrc/perm.inc).  tests/test_report_bootusagediff.py is the sibling for pA usage and imports this file's helpers.

The contract.  Populations and tested columns are diff_pa's (rc.populations: population 1's matrix columns ascending,
then population 2's; without --idents_2 every other cell that has a cluster); cell[j], the multiplicities m(b, c), q_i, s
and the rank rule are boot_pa_len's (tests/test_report_bootlen.py).  Reported records are diff_pa_len's tested ones: two
kept rows or more, span > 0, reads in both populations.  With c_ij the count of kept row i at position j, m = 1 for b = 0:
    A_g(b) = sum_i sum_{j in g} m(b, cell[j]) c_ij,   Q_g(b) = sum_i q_i sum_{j in g} m(b, cell[j]) c_ij     g = 1, 2
    d(b) = (double)Q_1(b) / (double)A_1(b) - (double)Q_2(b) / (double)A_2(b),  +infinity when A_1(b) = 0 or A_2(b) = 0
    D = #{b in 1..n_boot: d(b) defined},   k = max(1, (D + 1)(10000 - L) // 20000),   lo / hi = the k-th / (D + 1 - k)-th
    smallest of the defined values, which may be negative
One line per reported record; the columns are stated at `oracle_lines`.

Two correctly rounded divisions and one correctly rounded subtraction of exact integers: the numpy oracle below gives the
device's values to the bit and the file as exact text.  No test of this file has a tolerance."""
import csv
import functools
import io
import math
import os
from fractions import Fraction

import numpy as np
import pytest

import report_cases as rc
from report_cases import no_gpu, run as _run  # noqa: F401  (no_gpu: fixture)
from test_report_bootlen import (_bits, _boot_len, _boot_mult, _p, _quantiles, _reads_of, _vals_get, interval, level_bp,
                                 mult, series_values)
from test_report_difflen import exp_length
from test_report_difflengroups import quantise

HEADER = ["gene", "versus", "num_pa", "reads.1", "reads.2", "mean_pos.1", "mean_pos.2", "delta_pos", "delta_pos_lo",
          "delta_pos_hi", "exp_length.1", "exp_length.2", "delta_exp_length", "delta_exp_length_lo",
          "delta_exp_length_hi", "n_empty", "n_boot", "level"]
SHARED = ["gene", "versus", "num_pa", "reads.1", "reads.2", "mean_pos.1", "mean_pos.2", "delta_pos", "exp_length.1",
          "exp_length.2", "delta_exp_length"]                         # diff_pa_len's text for the same populations
M63, ALL = 1 << 63, (1 << 64) - 1


# ---------------------------------------------------------------- the contract, restated
def key(bits):
    """the select's order on the bit pattern of a double: monotone over the finite doubles, +infinity above them"""
    return bits ^ (ALL if bits >> 63 else M63)


def unkey(k):
    return k ^ (M63 if k >> 63 else ALL)


def subtract(v):
    """d [replicates] from the two populations' values v [replicates, 2] (+infinity: no read): the f64 subtraction"""
    with np.errstate(invalid="ignore"):
        d = v[:, 0] - v[:, 1]
    d[np.isinf(v[:, 0]) | np.isinf(v[:, 1])] = np.inf
    assert not np.isnan(d).any() and not np.signbit(d[d == 0]).any()
    return d


def len_diff_values(sub, q, n1, M):
    """d(b) [replicates] from the counts sub [kept rows, positions], the integer positions q, population 1's n1
    positions and the multiplicities M [replicates, positions]"""
    return subtract(series_values(sub, q, [0, n1, np.asarray(sub).shape[1]], M)[0])


def two_populations(bc, clu_text, id1, id2):
    """(cell of every position, n1, the versus text)"""
    c1, c2 = rc.populations(bc, clu_text, id1, id2)
    assert c1 and c2
    return np.array(c1 + c2, dtype=np.int64), len(c1), f"{id1}_Vs_{id2}" if id2 is not None else id1


def oracle_lines(records, bc, clu_text, id1, id2, n_boot, level, seed):
    """the file's lines as lists of text fields.  Columns: gene = gene_info_str; versus; num_pa = kept rows; reads.g =
    A_g(0); mean_pos.g and delta_pos = the exact rationals of the exact x_i, each rounded once; delta_pos_lo / _hi =
    ldexp(lo / hi, -s); exp_length.g = the reference's exp_pa_len of the population's counts of all K labels and
    delta_exp_length their f64 difference; delta_exp_length_lo / _hi = 9.0 * y / (a[-1] - a[0]) with y that end of
    delta_pos, empty when an exp_length is nan or a[-1] - a[0] is not finite and positive; n_empty = n_boot - D;
    n_boot; level = the option's text.  The four interval fields are empty when D = 0"""
    cell, n1, versus = two_populations(bc, clu_text, id1, id2)
    M = mult(seed, 1, n_boot, cell)
    L = level_bp(level)
    lines = []
    for rec, dense in zip(records, rc.dense_counts(records, rc.column_ids(bc))):
        K, alpha = int(rec["K"]), np.asarray(rec["alpha_arr"])
        sub = dense[:, cell]
        kept = [lb for lb in range(K) if sub[lb].any()]
        x = [float(alpha[lb]) for lb in kept]
        a, b = sub[kept][:, :n1].sum(axis=1).tolist(), sub[kept][:, n1:].sum(axis=1).tolist()
        if len(kept) < 2 or not max(x) - min(x) > 0 or sum(a) == 0 or sum(b) == 0:
            continue
        q, s = quantise(x)
        lo, hi, D = interval(len_diff_values(sub[kept], q, n1, M), L)
        m1 = sum(ai * Fraction(xi) for ai, xi in zip(a, x)) / sum(a)
        m2 = sum(bi * Fraction(xi) for bi, xi in zip(b, x)) / sum(b)
        e1, e2 = exp_length(K, alpha, sub[:, :n1].sum(axis=1)), exp_length(K, alpha, sub[:, n1:].sum(axis=1))
        with np.errstate(invalid="ignore"):
            de = float(np.float64(e1) - np.float64(e2))
        ends = [math.ldexp(v, -s) for v in (lo, hi)] if D else []
        width = float(alpha[-1]) - float(alpha[0])
        scaled = D and not (math.isnan(e1) or math.isnan(e2)) and math.isfinite(width) and width > 0
        lines.append([rec["gene_info_str"], versus, str(len(kept)), str(sum(a)), str(sum(b)), repr(float(m1)),
                      repr(float(m2)), repr(float(m1 - m2))] + ([repr(y) for y in ends] or ["", ""]) +
                     [repr(e1), repr(e2), repr(de)] + ([repr(9.0 * y / width) for y in ends] if scaled else ["", ""]) +
                     [str(n_boot - D), str(n_boot), level])
    return lines


def as_text(lines, header=HEADER):
    out = io.StringIO()
    w = csv.writer(out, delimiter=',', quoting=csv.QUOTE_MINIMAL, lineterminator='\n')
    w.writerow(header)
    w.writerows(lines)
    return out.getvalue()


# ---------------------------------------------------------------- the command
CMD = "boot_pa_len_diff"


def diff_args(cmd, root, clu, res="res.gene.pkl", id1=None, id2=None, n_boot=None, level=None, seed=None):
    a = [cmd, "--output_dir", str(root), "--res_pkl_file", res, "--cell_cluster_file", str(clu)]
    for opt, v in (("--idents_1", id1), ("--idents_2", id2), ("--n_boot", n_boot), ("--level", level), ("--seed", seed)):
        if v is not None:
            a += [opt, str(v)]
    return a


def diff_command(cmd, root, clu, res, id1, id2, n_boot, level, seed, what=""):
    """the text of the file that the command writes"""
    r = _run(diff_args(cmd, root, clu, res, id1, id2, n_boot, level, seed))
    assert r.exit_code == 0, (what, r.output, repr(r.exception))
    assert not rc.parts_left(root)
    with open(rc.perm_path(cmd, root, clu, res, id1, id2), newline="") as fh:
        return fh.read()


def same_text(text, want, what):
    if text != want:
        for a, b in zip(text.split("\n"), want.split("\n")):
            assert a == b, (what, a, b)
    assert text == want, what


# ---------------------------------------------------------------- CPU
def help_and_import_path(cmd, header_name, header, entry):
    r = _run(["--help"])
    assert r.exit_code == 0 and cmd in r.output.split()
    r = _run([cmd, "--help"])
    assert r.exit_code == 0, r.output
    for o in ("--output_dir", "--res_pkl_file", "--cell_cluster_file", "--idents_1", "--idents_2", "--n_boot", "--level",
              "--seed"):
        assert o in r.output
    assert "--strata_file" not in r.output and "--n_perm" not in r.output and "--idents " not in r.output
    flat = " ".join(r.output.split())
    assert "[default: 9999]" in flat and "[default: 95]" in flat and "[default: 1]" in flat
    import scape.utils as su
    from scape_amd import _lib, report
    assert getattr(su, cmd) is getattr(report, cmd)
    assert entry in _lib.SIGNATURES and getattr(report, header_name) == header


def test_help_and_import_path():
    help_and_import_path(CMD, "BOOT_PA_LEN_DIFF_HEADER", HEADER, "scape_hip_report_boot_len_diff")
    assert [c for c in HEADER if c in SHARED] == SHARED


def prerequisites_and_argument_errors(cmd, tmp_path):
    """diff_pa's errors in diff_pa's words and boot_pa_len's in boot_pa_len's, all before the device is opened; a
    refused run leaves the directory as it was"""
    clu = tmp_path / "groups.csv"

    def both(root, id1=None, id2=None):
        a = _run(rc.perm_args("diff_pa", root, clu, "res.gene.pkl", id1, id2))
        b = _run(diff_args(cmd, root, clu, "res.gene.pkl", id1, id2))
        assert type(a.exception) is type(b.exception) and str(a.exception) == str(b.exception), (a.exception, b.exception)
        assert b.exit_code != 0
        return b

    assert "Given output_dir folder does not exists." in str(both(tmp_path / "nope", "A").exception)
    assert "Given res_pkl_file is not in output_dir." in str(both(tmp_path, "A").exception)
    (tmp_path / "res.gene.pkl").write_bytes(b"")
    assert "Given cell_cluster_file file does not exists" in str(both(tmp_path, "A").exception)
    clu.write_text("index,group\n3,A\n4,B\n5,\n6,a/b\n77,ghost\n")
    r = both(tmp_path, "A")
    assert isinstance(r.exception, FileNotFoundError) and "barcode_index.csv" in str(r.exception)
    (tmp_path / "barcode_index.csv").write_text("CB,index\nA-1,3\nB-1,4\nC-1,5\nD-1,6\n")
    for ids, word in ((("A", "A"), "same"), (("Z", None), "'Z'"), (("A", "Z"), "'Z'"), (("", None), "names no cluster"),
                      (("ghost", None), "has no cell"), (("A", "ghost"), "has no cell"), (("a/b", None), "file name")):
        r = both(tmp_path, *ids)
        assert isinstance(r.exception, ValueError) and word in str(r.exception), (ids, repr(r.exception))
    for extra, word in ((["--n_boot", "0"], "n_boot"), (["--n_boot", str(1 << 31)], "n_boot"), (["--seed", "-1"], "seed"),
                        (["--seed", str(1 << 64)], "seed"), (["--level", "0"], "level"), (["--level", "100"], "level"),
                        (["--level", "95.123"], "level"), (["--level", "-1"], "level"), (["--level", "abc"], "level")):
        r = _run(diff_args(cmd, tmp_path, clu, id1="A") + extra)
        theirs = _run(["boot_pa_len", "--output_dir", str(tmp_path), "--res_pkl_file", "res.gene.pkl"] + extra)
        assert isinstance(r.exception, ValueError) and word in str(r.exception), (extra, repr(r.exception))
        assert str(r.exception) == str(theirs.exception), (extra, r.exception, theirs.exception)
    from scape_amd import report
    with pytest.raises(ValueError, match="idents_1 is required"):
        getattr(report, "_" + cmd)(str(tmp_path), "res.gene.pkl", str(clu), None)
    clu.write_text("index,group\n3,A\n4,A\n5,\n")                     # nobody left for "the rest"
    r = both(tmp_path, "A")
    assert isinstance(r.exception, ValueError) and "has no cell" in str(r.exception)
    r = _run([cmd, "--output_dir", str(tmp_path), "--res_pkl_file", "res.gene.pkl", "--cell_cluster_file", str(clu)])
    assert r.exit_code == 2 and "--idents_1" in r.output
    r = _run([cmd, "--output_dir", str(tmp_path), "--res_pkl_file", "res.gene.pkl", "--idents_1", "A"])
    assert r.exit_code == 2 and "--cell_cluster_file" in r.output
    r = _run(diff_args(cmd, tmp_path, clu, id1="A") + ["--strata_file", str(clu)])
    assert r.exit_code == 2 and "--strata_file" in r.output
    assert sorted(os.listdir(tmp_path)) == ["barcode_index.csv", "groups.csv", "res.gene.pkl"]


def test_prerequisites_and_argument_errors(tmp_path, no_gpu):
    prerequisites_and_argument_errors(CMD, tmp_path)


def test_too_many_cells_is_refused_before_the_device(tmp_path, no_gpu, monkeypatch):
    """n1 + n2 < 2^24, in diff_pa's words (the limit lowered to the directory's 4 cells)"""
    from scape_amd import report
    clu = tmp_path / "groups.csv"
    (tmp_path / "res.gene.pkl").write_bytes(b"")
    clu.write_text("index,group\n3,A\n4,B\n5,B\n6,A\n")
    (tmp_path / "barcode_index.csv").write_text("CB,index\nA-1,3\nB-1,4\nC-1,5\nD-1,6\n")
    monkeypatch.setattr(report, "MAX_PERM_CELLS", 4)
    for cmd in (CMD, "boot_pa_usage_diff", "diff_pa"):
        r = _run((diff_args if cmd != "diff_pa" else rc.perm_args)(cmd, tmp_path, clu, "res.gene.pkl", "A"))
        assert isinstance(r.exception, ValueError), (cmd, repr(r.exception))
        assert str(r.exception) == f"4 tested cells: {cmd} takes fewer than 4"


def test_key_map():
    """sorted finite doubles of both signs, with the subnormals and 0.0, have strictly increasing keys; +infinity lies
    above them all; the inverse map returns the bits; over the non-negative ones the keys order as the bits do"""
    rng = np.random.default_rng(1)
    tiny = np.array([5e-324, 2.2250738585072014e-308, 1e-300])
    x = np.concatenate([rng.standard_normal(500) * 10.0 ** rng.integers(-200, 200, 500), tiny, -tiny, [0.0],
                        [np.finfo(np.float64).max, -np.finfo(np.float64).max, 1.0, -1.0, 0.5, -0.5, 1 << 22]])
    x = np.unique(x)                                                  # sorted, distinct
    assert len(x) > 500 and (x < 0).sum() > 200 and (x > 0).sum() > 200
    keys = [key(int(b)) for b in _bits(x)]
    assert all(a < b for a, b in zip(keys, keys[1:]))
    inf_key = key(int(_bits([np.inf])[0]))
    assert inf_key == 0xFFF0000000000000 and keys[-1] < inf_key
    assert [unkey(k) for k in keys] == [int(b) for b in _bits(x)] and unkey(inf_key) == int(_bits([np.inf])[0])
    pos = [int(b) for b in _bits(x[x >= 0])]
    assert sorted(pos) == pos and [key(b) for b in pos] == [b | M63 for b in pos]
    # the rule of `interval` (np.sort, +infinity last) is the select by keys
    d = np.concatenate([x[::7], [np.inf] * 9])[rng.permutation(len(x[::7]) + 9)]
    by_key = sorted(int(b) for b in _bits(d))
    by_key.sort(key=key)
    assert by_key == [int(b) for b in _bits(np.sort(d))]
    lo, hi, D = interval(d, 9500)
    assert D == len(d) - 9 and lo < 0 < hi


def test_purpose_on_the_oracle():
    """20 + 20 cells, sites at 100 and 900 nt.  A record whose population 1 reads sit at the distal site and
    population 2's at the proximal one has an interval wholly above 0; a record with the same table in both
    populations has one that contains 0"""
    rng = np.random.default_rng(2)
    n1 = n = 20
    M = mult(1, 1, 999, np.arange(2 * n))
    q, _s = quantise([100.0, 900.0])
    apart = np.zeros((2, 2 * n), dtype=np.int64)
    apart[1, :n1] = rng.integers(1, 5, n)                             # population 1: distal
    apart[0, n1:] = rng.integers(1, 5, n)                             # population 2: proximal
    apart[0, :n1] = apart[1, n1:] = rng.random(n) < 0.2               # and a few reads at the other site
    lo, hi, D = interval(len_diff_values(apart, q, n1, M), 9500)
    print("apart", lo, hi, D)
    assert D == 999 and 0 < lo <= hi
    table = rng.integers(0, 4, (2, n))
    lo, hi, D = interval(len_diff_values(np.concatenate([table, table], axis=1), q, n1, M), 9500)
    print("same table", lo, hi, D)
    assert D == 999 and lo < 0 < hi


@functools.lru_cache(maxsize=None)
def _syn_lines(id1, id2, n_boot, level, seed, n_rec=None):
    records, bc, clu_text = rc.synthetic()
    return oracle_lines(records[:n_rec], bc, clu_text, id1, id2, n_boot, level, seed)


def test_oracle_on_the_synthetic_directory():
    """999 replicates, A against B: GENE0..GENE2 (a planted excess of the first site in A) have an interval wholly below
    0, as diff_pa_len finds them; the file's shape"""
    lines = _syn_lines("A", "B", 999, "95", 1)
    by = {ln[0].split(":")[1]: ln for ln in lines}
    assert len(by) == len(lines) == 36 and "GENE5" not in by and "GENE6" not in by
    for gene in ("GENE0", "GENE1", "GENE2"):
        print(gene, by[gene][7:10])
        assert float(by[gene][8]) <= float(by[gene][9]) < 0 and float(by[gene][7]) < 0
    assert all(float(ln[8]) <= float(ln[9]) for ln in lines)
    assert max(int(ln[2]) for ln in lines) == 63 and all(ln[15] == "0" for ln in lines[:4])


# ---------------------------------------------------------------- GPU: the entry points
EP_CHUNKS = (150, 120)                    # 270 replicates: one tile of 256 and a part, written in two chunks
EP_SEED = 77
EP_KEPT = (2, 3, 8, 9, 63)                # 8 and 9: the two sides of k_rep_boot_usage_diff's limit of 8 register rows
EP_POPS = ((1, 7), (5, 5), (40, 1))       # population sizes: the tested columns are the first n1 + n2
EP_COLS = 48


@functools.lru_cache(maxsize=None)
def ep_matrix():
    """records of 2, 3, 8, 9 and 63 kept rows over 48 columns, about a third of the counts above 0.  The rows 2..5 of
    the three largest records have their nonzeros in the columns {5, 6, 40}, {0..4}, {0} and {40}: under every size
    of EP_POPS some row has reads in population 1 only and some in population 2 only.  One count is above 2^16"""
    rng = np.random.default_rng(9)
    Ks = np.array(EP_KEPT, dtype=np.int32)
    base = np.concatenate([[0], np.cumsum(Ks)])
    shape = (int(Ks.sum()), EP_COLS)
    dense = ((rng.random(shape) < 0.35) * rng.integers(1, 4, shape)).astype(np.int64)
    for r in (2, 3, 4):
        for k, cols in zip((2, 3, 4, 5), ([5, 6, 40], [0, 1, 2, 3, 4], [0], [40])):
            dense[base[r] + k] = 0
            dense[base[r] + k, cols] = rng.integers(1, 4, len(cols))
    dense[base[1], 3] = 70000
    rows = np.arange(int(Ks.sum()), dtype=np.int64)
    off, lab, cb = _reads_of(dense, Ks)
    q = rng.integers(0, (1 << 22) + 1, len(rows)).astype(np.int32)
    q[0], q[1] = 0, 1 << 22
    return dict(Ks=Ks, off=off, lab=lab, cb=cb, n_cols=EP_COLS, rows=rows, roff=base.astype(np.int64), dense=dense, q=q)


@functools.lru_cache(maxsize=None)
def ep_case(sizes, n_boot=sum(EP_CHUNKS)):
    """(matrix, cell, seg, multiplicities, t [rows], a0 [rows, 2]) of the populations `sizes`"""
    m = ep_matrix()
    n = sum(sizes)
    cell = (7 * np.arange(n) + 3).astype(np.int32)
    seg = np.array([0, sizes[0], n], dtype=np.int32)
    sub = m["dense"][:, :n]
    a0 = np.stack([sub[:, :sizes[0]].sum(axis=1), sub[:, sizes[0]:].sum(axis=1)], axis=1)
    assert ((a0[:, 0] > 0) & (a0[:, 1] == 0)).any() and ((a0[:, 0] == 0) & (a0[:, 1] > 0)).any(), sizes
    return m, cell, seg, mult(EP_SEED, 1, n_boot, cell), sub.sum(axis=1), a0


def _boot_len_diff(ctx, m, G, seg, q, n_boot, roff=None, rows=None):
    roff, rows = m["roff"] if roff is None else roff, m["rows"] if rows is None else rows
    t, a0 = np.full(len(rows), -1, np.int64), np.full((len(rows), G), -1, np.int64)
    rc_ = ctx.lib.scape_hip_report_boot_len_diff(ctx.h, len(roff) - 1, _p(roff), _p(rows), G, _p(seg), _p(q), n_boot,
                                                 _p(t), _p(a0))
    return rc_, t, a0


def _boot_usage_diff(ctx, m, G, seg, n_boot, roff=None, rows=None):
    roff, rows = m["roff"] if roff is None else roff, m["rows"] if rows is None else rows
    t, a0 = np.full(len(rows), -1, np.int64), np.full((len(rows), G), -1, np.int64)
    rc_ = ctx.lib.scape_hip_report_boot_usage_diff(ctx.h, len(roff) - 1, _p(roff), _p(rows), G, _p(seg), n_boot, _p(t),
                                                   _p(a0))
    return rc_, t, a0


def in_chunks(ctx, cell, seed, chunks, call):
    """call() behind the multiplicities of every chunk of replicates; its last result"""
    from scape_amd import _lib
    first = 1
    for b_count in chunks:
        _lib.check(_boot_mult(ctx, cell, first, b_count, seed), "boot_mult")
        out = call()
        _lib.check(out[0], "entry point")
        first += b_count
    return out


def all_values(ctx, n_series, n_boot):
    return np.stack([_vals_get(ctx, k, n_boot) for k in range(n_series)])


def same_bits(got, want, what):
    assert got.shape == want.shape and np.array_equal(_bits(got), _bits(want)), \
        (what, np.argwhere(_bits(got) != _bits(want))[:5])


@pytest.mark.gpu
@pytest.mark.parametrize("sizes", EP_POPS, ids=["1+7", "5+5", "40+1"])
def test_boot_len_diff(sizes):
    """scape_hip_report_boot_len_diff on the hand-made matrix, 270 replicates written in chunks of 150 and 120 (the
    second with b_first = 151): t and a0 are exact, every value equals the oracle's bit for bit, and equals the numpy
    f64 difference of the two populations' values of a scape_hip_report_boot_len call at G = 2 on the same rows and q"""
    from scape_amd import _lib
    m, cell, seg, M, t_want, a0_want = ep_case(sizes)
    n_boot, n_rec, n = sum(EP_CHUNKS), len(EP_KEPT), sum(sizes)
    want = np.stack([len_diff_values(m["dense"][m["roff"][r]:m["roff"][r + 1], :n], m["q"][m["roff"][r]:m["roff"][r + 1]],
                                     sizes[0], M) for r in range(n_rec)])
    ctx = _lib.default_context(None)
    try:
        rc.device_counts(ctx, m["Ks"], m["off"], m["lab"], m["cb"], m["n_cols"])
        _rc, t, a0 = in_chunks(ctx, cell, EP_SEED, EP_CHUNKS, lambda: _boot_len_diff(ctx, m, 2, seg, m["q"], n_boot))
        got = all_values(ctx, n_rec, n_boot)
        assert ctx.lib.scape_hip_report_boot_vals_get(ctx.h, n_rec, _p(np.zeros(n_boot))) != 0
        in_chunks(ctx, cell, EP_SEED, (n_boot,), lambda: _boot_len(ctx, m, 2, seg, m["q"], n_boot))
        parts = all_values(ctx, n_rec * 2, n_boot).reshape(n_rec, 2, n_boot)
    finally:
        ctx.lib.scape_hip_report_free(ctx.h)
    assert np.array_equal(t, t_want) and np.array_equal(a0, a0_want)
    same_bits(got, want, sizes)
    same_bits(got, np.stack([subtract(parts[r].T) for r in range(n_rec)]), sizes)
    D = np.isfinite(want).sum(axis=1)
    print(sizes, "D", D.tolist(), "negative", int((want < 0).sum()), "positive", int(((want > 0) & np.isfinite(want)).sum()))
    assert (want < 0).any() and ((want > 0) & np.isfinite(want)).any()
    assert 1 not in sizes or (D < n_boot).any()                          # a population of one cell: empty replicates


# the select: two populations of three cells each; a record is two rows at q = 0 and 2^22 unless stated
S_N1 = 3
S_DENSE = np.array([[3, 0, 2, 0, 1, 4],       # record 0: mixed sign
                    [0, 4, 1, 2, 2, 0],
                    [2, 1, 3, 0, 0, 0],       # record 1: all negative (population 1 at q <= 100, 2 at q >= 2^21)
                    [1, 2, 0, 0, 0, 0],
                    [0, 0, 0, 1, 0, 2],
                    [0, 0, 0, 2, 3, 1],
                    [2, 0, 0, 2, 0, 0],       # record 2: one cell with reads per population, the same table: 0.0 or
                    [3, 0, 0, 3, 0, 0],       # undefined
                    [3, 0, 0, 1, 0, 0],       # record 3: the same, other tables: the constant -2^21 or undefined
                    [1, 0, 0, 3, 0, 0],
                    [0, 2, 0, 1, 0, 3],       # record 4: population 1's reads sit in one cell (position 1): n_empty > 0,
                    [0, 1, 0, 0, 2, 1]],      # mixed values
                   dtype=np.int64)
S_KS = np.array([2, 4, 2, 2, 2], dtype=np.int32)
S_ROFF = np.array([0, 2, 6, 8, 10, 12], dtype=np.int64)
S_POS = np.array([0, 1 << 22, 0, 100, 1 << 21, 1 << 22, 0, 1 << 22, 0, 1 << 22, 0, 1 << 22], dtype=np.int32)
S_CELL = np.arange(6, dtype=np.int32) * 11
S_LEVELS = (9500, 5000, 9999, 1)              # 95, 50, 99.99 and 0.01 percent


def select_seed(n_boot):
    """the first seed of 0..63 under which record 4's series has the property the test is for: at one replicate D = 0
    because the multiplicity of population 1's one cell with reads is 0, otherwise 0 < D < n_boot"""
    sl = slice(int(S_ROFF[4]), int(S_ROFF[5]))
    for seed in range(64):
        M = mult(seed, 1, n_boot, S_CELL)
        D = int(np.isfinite(len_diff_values(S_DENSE[sl], S_POS[sl], S_N1, M)).sum())
        if M[0, 1] == 0 if n_boot == 1 else 0 < D < n_boot:
            return seed
    raise AssertionError("no seed of 0..63 found")


def select_case(n_boot):
    """(seed, len_diff series [5, n_boot], usage_diff series [12, n_boot]) of the fixture, from the oracle"""
    from test_report_bootusage import usage_values
    seed = select_seed(n_boot)
    M = mult(seed, 1, n_boot, S_CELL)
    seg = [0, S_N1, 6]
    by_rec = [slice(int(S_ROFF[r]), int(S_ROFF[r + 1])) for r in range(5)]
    d_len = np.stack([len_diff_values(S_DENSE[sl], S_POS[sl], S_N1, M) for sl in by_rec])
    d_use = np.concatenate([np.stack([subtract(u_i) for u_i in usage_values(S_DENSE[sl], seg, M)[0]]) for sl in by_rec])
    return seed, d_len, d_use


def test_select_fixture_on_the_oracle():
    """the series the select is tested on are what their comments say, at every n_boot of the test"""
    for n_boot in (1, 2, 39, 255, 256, 257, 1000):
        _seed, d, u = select_case(n_boot)
        fin = np.isfinite(d)
        D = fin.sum(axis=1)
        assert (0 < D[4] < n_boot) if n_boot > 1 else D[4] == 0, (n_boot, D)
        assert np.all(d[1][fin[1]] < 0) and np.all(d[2][fin[2]] == 0) and np.all(d[3][fin[3]] == -float(1 << 21))
        assert not np.signbit(d[2][fin[2]]).any()
        assert np.all(u[6:8][np.isfinite(u[6:8])] == 0) and set(u[8][np.isfinite(u[8])].tolist()) <= {0.5}
        assert set(u[9][np.isfinite(u[9])].tolist()) <= {-0.5}
        if n_boot >= 39:
            assert (d[0] < 0).any() and ((d[0] > 0) & fin[0]).any() and D[1] > 0 and D[2] > 0 and D[3] > 0
            assert (d[4] < 0).any() and ((d[4] > 0) & fin[4]).any()


@pytest.mark.gpu
@pytest.mark.parametrize("n_boot", [1, 2, 39, 255, 256, 257, 1000])
def test_boot_quantiles_signed(n_boot):
    """lo, hi and D of k_rep_boot_select against np.sort at four levels, around the 256-thread stride, on series of
    mixed sign, all negative, tied at 0.0, constant and negative, with empty replicates, and (n_boot = 1) with D = 0:
    the len_diff record set (one series per record) and the usage_diff one (one per kept row)"""
    from scape_amd import _lib
    seed, d_len, d_use = select_case(n_boot)
    seg = np.array([0, S_N1, 6], dtype=np.int32)
    off, lab, cb = _reads_of(S_DENSE, S_KS)
    rows = np.arange(12, dtype=np.int64)
    ctx = _lib.default_context(None)
    got = {}
    try:
        rc.device_counts(ctx, S_KS, off, lab, cb, 6)
        _lib.check(_boot_mult(ctx, S_CELL, 1, n_boot, seed), "boot_mult")
        _lib.check(_boot_len_diff(ctx, None, 2, seg, S_POS, n_boot, S_ROFF, rows)[0], "boot_len_diff")
        same_bits(all_values(ctx, 5, n_boot), d_len, "len_diff")
        got["len"] = {L: _quantiles(ctx, L, 5) for L in S_LEVELS}
        _lib.check(_boot_usage_diff(ctx, None, 2, seg, n_boot, S_ROFF, rows)[0], "boot_usage_diff")
        same_bits(all_values(ctx, 12, n_boot), d_use, "usage_diff")
        got["usage"] = {L: _quantiles(ctx, L, 12) for L in S_LEVELS}
    finally:
        ctx.lib.scape_hip_report_free(ctx.h)
    for kind, series in (("len", d_len), ("usage", d_use)):
        for L, (rc_, lo, hi, D) in got[kind].items():
            assert rc_ == 0
            for k, v in enumerate(series):
                want = interval(v, L)
                print(n_boot, kind, L, k, "got", lo[k], hi[k], D[k], "want", want)
                assert (_bits(lo[k:k + 1])[0], _bits(hi[k:k + 1])[0], int(D[k])) == \
                    (_bits([want[0]])[0], _bits([want[1]])[0], want[2]), (n_boot, kind, L, k)
    _rc, lo, hi, D = got["len"][9500]
    if n_boot == 1:
        assert D[4] == 0 and np.isinf(lo[4]) and np.isinf(hi[4]) and lo[4] > 0
    else:
        assert 0 < D[4] < n_boot
    if n_boot >= 39:
        assert lo[0] < 0 < hi[0] and hi[1] < 0 and lo[3] == hi[3] == -float(1 << 21)
        assert _bits(lo[2:3])[0] == _bits(hi[2:3])[0] == 0                   # +0.0


def _doubled(m):
    """the matrix's rows twice over, in 2 x 5 records: usage_diff then has as many series as boot_usage at G = 2"""
    n = len(m["rows"])
    return np.concatenate([m["roff"], m["roff"][1:] + n]), np.concatenate([m["rows"], m["rows"]])


@pytest.mark.gpu
def test_refusals():
    """each refused call returns non-zero with its entry point's name in the message, and the valid calls before and
    after it give the same outputs.  A later chunk through another of the four entry points is refused in both
    directions although the numbers of series, groups and replicates agree"""
    from test_report_bootusage import _boot_usage
    from scape_amd import _lib
    n_boot = 270
    m, cell, seg, _M, _t, _a0 = ep_case((5, 5))
    q, n_rows, n = m["q"], len(m["rows"]), 10
    one_each = np.arange(n_rows + 1, dtype=np.int64)
    ten = np.array([0, 1, 2, 3, 5, 13, 20, 22, 40, 60, n_rows], dtype=np.int64)
    roff2, rows2 = _doubled(m)
    q2 = np.concatenate([q, q])
    ctx = _lib.default_context(None)
    lib = ctx.lib
    new_len, new_use = "scape_hip_report_boot_len_diff", "scape_hip_report_boot_usage_diff"
    calls = {                                  # entry point -> (call on its usual rows, number of series)
        new_len: (lambda **kw: _boot_len_diff(ctx, m, 2, seg, q, n_boot, **kw), len(EP_KEPT)),
        new_use: (lambda **kw: _boot_usage_diff(ctx, m, 2, seg, n_boot, **kw), n_rows)}

    def build(b_first=1, b_count=n_boot):
        return _boot_mult(ctx, cell, b_first, b_count, EP_SEED)

    def good(entry):
        call, n_series = calls[entry]
        _lib.check(build(), "boot_mult")
        rc_, t, a0 = call()
        _lib.check(rc_, entry)
        rc_, lo, hi, D = _quantiles(ctx, 9500, n_series)
        _lib.check(rc_, "boot_quantiles")
        return [a.tobytes() for a in (t, a0, lo, hi, D, _vals_get(ctx, 3, n_boot), _vals_get(ctx, n_series - 1, n_boot))]

    def refused(rc_, name, word):
        assert rc_ != 0 and name in _lib.last_error() and word in _lib.last_error(), _lib.last_error()

    def crossed(begin, then, name):
        """a record set begun by begin() with 150 of the 270 replicates; then() behind the next 120 is refused"""
        _lib.check(build(1, 150), "boot_mult")
        _lib.check(begin()[0], "first chunk")
        _lib.check(build(151, 120), "boot_mult")
        refused(then()[0], name, "later chunk")
    try:
        for entry, (call, n_series) in calls.items():
            refused(call()[0], entry, "report_counts")
        rc.device_counts(ctx, m["Ks"], m["off"], m["lab"], m["cb"], m["n_cols"])
        for entry, (call, n_series) in calls.items():
            refused(call()[0], entry, "boot_mult has not been called")
        refused(_quantiles(ctx, 9500, 5)[0], "scape_hip_report_boot_quantiles", "boot_len has not been called")
        first = {entry: good(entry) for entry in calls}
        assert first[new_len] != first[new_use]
        seg1, seg3 = np.array([0, n], np.int32), np.array([0, 5, 7, n], np.int32)
        refused(_boot_len_diff(ctx, m, 1, seg1, q, n_boot)[0], new_len, "n_groups")
        refused(_boot_len_diff(ctx, m, 3, seg3, q, n_boot)[0], new_len, "n_groups")
        refused(_boot_usage_diff(ctx, m, 1, seg1, n_boot)[0], new_use, "n_groups")
        refused(_boot_usage_diff(ctx, m, 3, seg3, n_boot)[0], new_use, "n_groups")
        refused(_boot_len_diff(ctx, m, 2, np.array([0, 5, n - 1], np.int32), q, n_boot)[0], new_len, "seg_off")
        refused(_boot_usage_diff(ctx, m, 2, np.array([1, 5, n], np.int32), n_boot)[0], new_use, "seg_off must start at 0")
        bad_q = q.copy()
        bad_q[3] = (1 << 22) + 1
        refused(_boot_len_diff(ctx, m, 2, seg, bad_q, n_boot)[0], new_len, "2^22")
        refused(_boot_len_diff(ctx, m, 2, seg, q, n_boot - 1)[0], new_len, "n_boot")
        refused(lib.scape_hip_report_boot_vals_get(ctx.h, n_rows, _p(np.zeros(n_boot))),
                "scape_hip_report_boot_vals_get", "series")
        t_rows = np.frombuffer(first[new_use][0], dtype=np.int64)
        heavy_row, reads = int(m["rows"][int(np.argmax(t_rows))]), int(t_rows.max())
        assert reads > 70000
        heavy = np.full(-(-(1 << 27) // reads), heavy_row, dtype=np.int64)
        one_rec = np.array([0, len(heavy)], np.int64)
        refused(_boot_usage_diff(ctx, m, 2, seg, n_boot, roff=one_rec, rows=heavy)[0], new_use, "2^27 or more reads")
        refused(_boot_len_diff(ctx, None, 2, seg, np.zeros(len(heavy), np.int32), n_boot, one_rec, heavy)[0], new_len,
                "2^27 or more reads")
        for entry in calls:
            assert good(entry) == first[entry], entry
        # quantiles before every column is written, and a later chunk of other records
        for entry, (call, n_series) in calls.items():
            _lib.check(build(1, 150), "boot_mult")
            _lib.check(call()[0], entry)
            refused(_quantiles(ctx, 9500, n_series)[0], "scape_hip_report_boot_quantiles", "replicate 151")
            _lib.check(build(151, 120), "boot_mult")
            refused(call(roff=m["roff"][:3].copy(), rows=m["rows"][:int(m["roff"][2])].copy())[0], entry, "later chunk")
            _lib.check(call()[0], entry)
            rc_, lo, hi, D = _quantiles(ctx, 9500, n_series)
            assert rc_ == 0 and [a.tobytes() for a in (lo, hi, D)] == first[entry][2:5]
        # new <-> new: one series per row on both sides
        crossed(lambda: _boot_len_diff(ctx, m, 2, seg, q, n_boot, one_each), calls[new_use][0], new_use)
        crossed(calls[new_use][0], lambda: _boot_len_diff(ctx, m, 2, seg, q, n_boot, one_each), new_len)
        # boot_len at G = 2 over 5 records <-> len_diff over 10: 10 series each
        crossed(lambda: _boot_len(ctx, m, 2, seg, q, n_boot), lambda: _boot_len_diff(ctx, m, 2, seg, q, n_boot, ten),
                new_len)
        crossed(lambda: _boot_len_diff(ctx, m, 2, seg, q, n_boot, ten), lambda: _boot_len(ctx, m, 2, seg, q, n_boot),
                "scape_hip_report_boot_len")
        # boot_usage at G = 2 over the rows <-> usage_diff over the rows twice: 2 x rows series each
        crossed(lambda: _boot_usage(ctx, m, 2, seg, n_boot), lambda: _boot_usage_diff(ctx, m, 2, seg, n_boot, roff2, rows2),
                new_use)
        crossed(lambda: _boot_usage_diff(ctx, m, 2, seg, n_boot, roff2, rows2), lambda: _boot_usage(ctx, m, 2, seg, n_boot),
                "scape_hip_report_boot_usage")
        # old <-> new across the two quantities: boot_usage over the rows <-> len_diff over 2 x rows records of one row
        crossed(lambda: _boot_usage(ctx, m, 2, seg, n_boot),
                lambda: _boot_len_diff(ctx, m, 2, seg, q2, n_boot, np.arange(2 * n_rows + 1, dtype=np.int64), rows2), new_len)
        crossed(lambda: _boot_len(ctx, m, 2, seg, q, n_boot, ten), lambda: _boot_usage_diff(
            ctx, m, 2, seg, n_boot, np.array([0, 20], np.int64), m["rows"][:20].copy()), new_use)
        for entry in calls:
            assert good(entry) == first[entry], entry
    finally:
        lib.scape_hip_report_free(ctx.h)


# ---------------------------------------------------------------- GPU: the command
def check_syn(cmd, lines_of, header, tmp_path, id1, id2, n_boot, level, seed, what, n_rec=None):
    lines = lines_of(id1, id2, n_boot, level, seed, n_rec)
    path = rc.write_synthetic(tmp_path, n_rec)
    text = diff_command(cmd, tmp_path, path, "res.gene.pkl", id1, id2, n_boot, level, seed, what)
    same_text(text, as_text(lines, header), what)
    return text, lines


@pytest.mark.gpu
@pytest.mark.parametrize("id2", ["B", None], ids=["A_vs_B", "A_vs_rest"])
def test_synthetic_directory(id2, tmp_path):
    """999 replicates of 230 + 301 cells (with --idents_2) and of 230 + 341 (without): the whole file equals the
    oracle's text; read from the file, GENE0..GENE2 have an interval wholly below 0"""
    text, lines = check_syn(CMD, _syn_lines, HEADER, tmp_path, "A", id2, 999, "95", 1, f"syn/{id2}")
    assert len(lines) == 36 and max(int(ln[2]) for ln in lines) == 63
    body = {r[0].split(":")[1]: r for r in list(csv.reader(io.StringIO(text)))[1:]}
    for gene in ("GENE0", "GENE1", "GENE2"):
        assert float(body[gene][8]) <= float(body[gene][9]) < 0, body[gene]
    name = f"syn_groups.gene.A_vs_{id2 or 'rest'}.boot_pa_len_diff.csv"
    assert os.path.exists(os.path.join(str(tmp_path), name))
    assert body["GENE0"][1] == ("A_Vs_B" if id2 else "A") and body["GENE0"][16:] == ["999", "95"]


@pytest.mark.gpu
def test_small_directory_utr(tmp_path):
    """res.utr.pkl, 15 + 25 cells, level 99.5 and the largest seed"""
    path, clu_text, bc, records, _ids = rc.small_dir(tmp_path, 40, 15, 6)
    text = diff_command(CMD, tmp_path, path, "res.utr.pkl", "B", "A", 299, "99.5", 2 ** 64 - 1)
    lines = oracle_lines(records, bc, clu_text, "B", "A", 299, "99.5", 2 ** 64 - 1)
    same_text(text, as_text(lines), "small")
    assert len(lines) == 8 and lines[0][17] == "99.5"
    assert os.path.exists(os.path.join(str(tmp_path), "small.utr.B_vs_A.boot_pa_len_diff.csv"))


@pytest.mark.gpu
@pytest.mark.parametrize("n_boot", [1, 255, 256, 257])
def test_tile_edges(n_boot, tmp_path):
    """a workgroup of k_rep_boot_len_diff takes 256 replicates: one, one short of a tile, a full tile and one over;
    cluster C's 40 cells leave replicates without a read"""
    _text, lines = check_syn(CMD, _syn_lines, HEADER, tmp_path, "C", "A", n_boot, "95", 5, f"tile/{n_boot}", n_rec=12)
    assert len(lines) == 10
    assert n_boot == 1 or any(int(ln[15]) > 0 for ln in lines)


def batch_chunk_and_seed_invariance(cmd, entry, interval_cols, n_empty_col, tmp_path, monkeypatch, batch_bytes):
    from scape_amd import _lib, report
    path = rc.write_synthetic(tmp_path)
    big = diff_command(cmd, tmp_path, path, "res.gene.pkl", "A", None, 299, "95", 1)
    other = list(csv.reader(io.StringIO(diff_command(cmd, tmp_path, path, "res.gene.pkl", "A", None, 299, "95", 2))))
    mine = list(csv.reader(io.StringIO(big)))
    moving = set(interval_cols) | {n_empty_col}
    fixed = [c for c in range(len(mine[0])) if c not in moving]
    assert [[r[c] for c in fixed] for r in mine] == [[r[c] for c in fixed] for r in other] and len(mine) > 30
    assert [[r[c] for c in interval_cols] for r in mine] != [[r[c] for c in interval_cols] for r in other]
    lib = _lib.load_library()
    calls = {"mult": [], "diff": 0}
    real_m, real_d = lib.scape_hip_report_boot_mult, getattr(lib, entry)

    def make_mult(*a):
        calls["mult"].append((a[3], a[4]))
        return real_m(*a)

    def diff(*a):
        calls["diff"] += 1
        return real_d(*a)
    monkeypatch.setattr(lib, "scape_hip_report_boot_mult", make_mult)
    monkeypatch.setattr(lib, entry, diff)
    monkeypatch.setattr(report, "MAX_BATCH_BYTES", batch_bytes)
    monkeypatch.setattr(report, "MAX_PERM_BYTES", 1 << 30)
    assert diff_command(cmd, tmp_path, path, "res.gene.pkl", "A", None, 299, "95", 1) == big
    assert calls["mult"] == [(1, 299)] and calls["diff"] > 3
    n_batches = calls["diff"]
    calls.update(mult=[], diff=0)
    monkeypatch.setattr(report, "MAX_PERM_BYTES", 571 * 100)             # one byte per tested cell: 100 replicates
    assert diff_command(cmd, tmp_path, path, "res.gene.pkl", "A", None, 299, "95", 1) == big
    assert calls["diff"] == 3 * n_batches and calls["mult"][:3] == [(1, 100), (101, 100), (201, 99)]


@pytest.mark.gpu
def test_batch_chunk_and_seed_invariance(tmp_path, monkeypatch):
    """records split over several count batches and the replicates over several chunks: the same bytes.  Another seed
    changes the four interval columns and n_empty only"""
    batch_chunk_and_seed_invariance(CMD, "scape_hip_report_boot_len_diff", [8, 9, 13, 14], 15, tmp_path, monkeypatch,
                                    1 << 16)                             # a record of K = 8 alone takes 57 KB


def swapped_idents(cmd, lo_col, hi_cols_after, key_cols, tmp_path):
    path = rc.write_synthetic(tmp_path)
    ab = list(csv.reader(io.StringIO(diff_command(cmd, tmp_path, path, "res.gene.pkl", "A", "B", 299, "95", 1))))[1:]
    ba = list(csv.reader(io.StringIO(diff_command(cmd, tmp_path, path, "res.gene.pkl", "B", "A", 299, "95", 1))))[1:]
    assert len(ab) == len(ba) > 30 and [[r[c] for c in key_cols] for r in ab] == [[r[c] for c in key_cols] for r in ba]
    seen = 0
    for x, y in zip(ab, ba):
        for c in [lo_col] + hi_cols_after:
            if x[c] == "":
                assert (x[c + 1], y[c], y[c + 1]) == ("", "", ""), (x, y)
                continue
            assert float(y[c]) == -float(x[c + 1]) and float(y[c + 1]) == -float(x[c]), (c, x, y)
            seen += 1
    return seen


@pytest.mark.gpu
def test_swapped_idents(tmp_path):
    """B against A: lo' = -hi and hi' = -lo for both intervals, as floats (the sign of a zero flips)"""
    assert swapped_idents(CMD, 8, [13], [0, 2, 15], tmp_path) > 60


@pytest.mark.gpu
@pytest.mark.parametrize("id2", ["B", None], ids=["A_vs_B", "A_vs_rest"])
def test_shared_columns_are_diff_pa_len_s(id2, tmp_path):
    """the eleven columns the file shares with diff_pa_len's are that command's text, line for line"""
    path = rc.write_synthetic(tmp_path)
    mine = list(csv.DictReader(io.StringIO(diff_command(CMD, tmp_path, path, "res.gene.pkl", "A", id2, 99, "95", 1))))
    theirs = list(csv.DictReader(io.StringIO(rc.perm_command("diff_pa_len", tmp_path, path, "res.gene.pkl", "A", id2, 9, 1))))
    assert len(mine) == len(theirs) == 36
    assert [[r[c] for c in SHARED] for r in mine] == [[r[c] for c in SHARED] for r in theirs]


@pytest.mark.gpu
def test_non_finite_position_and_unscaled_exp_length(tmp_path):
    """a NaN position of a pA site with reads is diff_pa_len's ValueError, with no file left.  An alpha_arr whose first
    and last entries are equal, or in descending order, gives the reference's exp_length as numpy prints it and no
    delta_exp_length interval; a record whose kept rows share one position has no line"""
    from test_report_difflen import _two_group_dir
    root = tmp_path / "nan"
    path, _clu, _bc, _recs = _two_group_dir(root, [[30, 200, 410], [25.0, float("nan"), 300.0]])
    r = _run(diff_args(CMD, root, path, id1="A", id2="B", n_boot=50))
    theirs = _run(rc.perm_args("diff_pa_len", root, path, "res.gene.pkl", "A", "B", 50))
    assert isinstance(r.exception, ValueError) and "TG1" in str(r.exception), repr(r.exception)
    assert str(r.exception) == str(theirs.exception)
    assert not rc.parts_left(root) and not os.path.exists(rc.perm_path(CMD, root, path, "res.gene.pkl", "A", "B"))
    root = tmp_path / "fine"
    alphas = [[30, 200, 410], [500, 20, 260, 90], [120, 480, 120], [77, 77], [10.5, 99.25, 300.0, 301.0, 580.75]]
    path, clu_text, bc, recs = _two_group_dir(root, alphas)
    records = [dict(gene_info_str=r["gene"], K=r["K"], alpha_arr=r["alpha"], beta_arr=np.full(r["K"], 10.0)) for r in recs]
    cell, n1, versus = two_populations(bc, clu_text, "A", "B")
    text = diff_command(CMD, root, path, "res.gene.pkl", "A", "B", 99, "95", 1)
    rows = list(csv.DictReader(io.StringIO(text)))
    assert [r["gene"].split(":")[1] for r in rows] == ["TG0", "TG1", "TG2", "TG4"]               # TG3: span 0
    by = {r["gene"].split(":")[1]: r for r in rows}
    for gene in ("TG1", "TG2"):                                          # a[-1] - a[0] is negative, or zero
        assert by[gene]["delta_pos_lo"] != "" and by[gene]["delta_exp_length_lo"] == by[gene]["delta_exp_length_hi"] == ""
    assert by["TG0"]["delta_exp_length_lo"] != "" and by["TG4"]["delta_exp_length_hi"] != ""
    theirs = list(csv.DictReader(io.StringIO(rc.perm_command("diff_pa_len", root, path, "res.gene.pkl", "A", "B", 9, 1))))
    assert [[r[c] for c in SHARED] for r in rows] == [[r[c] for c in SHARED] for r in theirs]
    # the interval columns against the oracle's values for the same records
    M = mult(1, 1, 99, cell)
    for rec, r in zip([records[k] for k in (0, 1, 2, 4)], rows):
        dense = next(x["dense"] for x in recs if x["gene"] == rec["gene_info_str"])[:, cell]
        kept = [lb for lb in range(rec["K"]) if dense[lb].any()]
        x = [float(rec["alpha_arr"][lb]) for lb in kept]
        q, s = quantise(x)
        lo, hi, D = interval(len_diff_values(dense[kept], q, n1, M), 9500)
        assert (r["delta_pos_lo"], r["delta_pos_hi"], r["n_empty"]) == \
            (repr(math.ldexp(lo, -s)), repr(math.ldexp(hi, -s)), str(99 - D)), r
        if r["delta_exp_length_lo"]:
            width = float(rec["alpha_arr"][-1]) - float(rec["alpha_arr"][0])
            assert r["delta_exp_length_hi"] == repr(9.0 * math.ldexp(hi, -s) / width), r
