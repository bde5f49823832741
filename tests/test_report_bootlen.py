"""`scape boot_pa_len`: percentile bootstrap intervals of a record's mean pA position and of its exp_length per cell
population, by resampling the cells (scape_amd/report.py, section boot_pa_len; kernels k_rep_boot_mult, k_rep_boot_len
and k_rep_boot_select and the five scape_hip_report_boot_* entry points of scape_amd/csrc/perm.inc).

The contract.  Populations: every cluster of the cluster file that has a column, in order of first appearance (at most
64), or the clusters named by --idents in the order given, or, without a cluster file, the one population all_cell of
every column.  Tested columns: population 0's matrix columns ascending, then population 1's, ...: positions 0 .. n-1;
position j carries cell[j], the 0-based column of its cell in barcode_index.csv.  All arithmetic mod 2^64, G and mix
those of diff_pa's key (rc.G, rc.mix):
    h(b, c) = mix(mix(seed + G b) + G (c + 1)),   m(b, c) = #{k in 0..14: h(b, c) >= P[k]} for b >= 1,   m(0, c) = 1
    P[k] = floor(2^64 e^-1 sum_{i <= k} 1 / i!)
Kept rows of a record: the labels < K with a read in a tested cell; reported when there are two or more and span = max x
- min x > 0 over x_i = alpha_arr[label]; q_i and s as in tests/test_report_difflengroups.py (quantise, 22 bits).  With
c_ij the count of kept row i at position j and g(j) the population of position j:
    A_g(b) = sum_i sum_{j in g} m(b, cell[j]) c_ij,   Q_g(b) = sum_i q_i sum_{j in g} m(b, cell[j]) c_ij
    v_g(b) = (double)Q_g(b) / (double)A_g(b),  +infinity when A_g(b) = 0
    D_g = #{b in 1..n_boot: A_g(b) > 0},   k = max(1, (D_g + 1)(10000 - L) // 20000),   L = the level in basis points
    lo = the k-th smallest of the n_boot values,   hi = the (D_g + 1 - k)-th smallest;   no interval when D_g = 0
One line per reported record and population with A_g(0) > 0; the columns are stated at `oracle_text`.

Everything is an integer up to one correctly rounded f64 division per value, so the oracle below (numpy: searchsorted for
the multiplicities, integer matrix products for A and Q, one f64 division, np.sort) gives the device's values to the bit
and the file as exact text: no test of this file has a tolerance."""
import csv
import functools
import io
import math
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import report_cases as rc
from report_cases import no_gpu, run as _run  # noqa: F401  (no_gpu: fixture)
from test_report_diffgroups import populations_all
from test_report_difflengroups import quantise

HEADER = ["gene", "group", "num_pa", "reads", "mean_pos", "mean_pos_lo", "mean_pos_hi", "exp_length", "exp_length_lo",
          "exp_length_hi", "n_empty", "n_boot", "level"]
P = [0x5E2D58D8B3BCDF1A, 0xBC5AB1B16779BE35, 0xEB715E1DC1582DC2, 0xFB23979734A252F1, 0xFF1025F59174DC3D,
     0xFFD90F3BA4055E19, 0xFFFA8B71FC72C913, 0xFFFF540C0914B3C9, 0xFFFFED1F4AA8F120, 0xFFFFFE216E641462,
     0xFFFFFFD4D85D3183, 0xFFFFFFFC6DA262B4, 0xFFFFFFFFBA12D178, 0xFFFFFFFFFB07C64C, 0xFFFFFFFFFFAB8EA5]
P_ARR = np.array(P, dtype=np.uint64)
U64 = np.uint64


# ---------------------------------------------------------------- the contract, restated
def np_mix(z):
    """rc.mix on a uint64 array (array arithmetic wraps mod 2^64)"""
    z = (z ^ (z >> U64(30))) * U64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> U64(27))) * U64(0x94D049BB133111EB)
    return z ^ (z >> U64(31))


def hashes(seed, b_first, b_count, cells):
    """h(b, c) for b = b_first .. b_first + b_count - 1 and the cells given: uint64 [b_count, len(cells)]"""
    base = np.array([rc.mix((seed + rc.G * b) & rc.M64) for b in range(b_first, b_first + b_count)], dtype=np.uint64)
    step = (np.asarray(cells).astype(np.uint64) + U64(1)) * U64(rc.G)
    return np_mix(base[:, None] + step[None, :])


def mult(seed, b_first, b_count, cells):
    """m(b, c): uint8 [b_count, len(cells)]; searchsorted(side="right") counts the P[k] <= h"""
    return np.searchsorted(P_ARR, hashes(seed, b_first, b_count, cells), side="right").astype(np.uint8)


def rank_k(n_def, level_bp):
    return max(1, (n_def + 1) * (10000 - level_bp) // 20000)


def series_values(sub, q, seg, M):
    """v_g(b) as f64 [replicates, G] and A_g(b), from the counts sub [kept rows, positions], the integer positions q,
    the segment offsets and the multiplicities M [replicates, positions]: integer matrix products, one division"""
    sub = np.asarray(sub, dtype=np.int64)
    n, G = sub.shape[1], len(seg) - 1
    w, wq = sub.sum(axis=0), (np.asarray(q, dtype=np.int64)[:, None] * sub).sum(axis=0)
    one = np.zeros((n, G), dtype=np.int64)
    for g in range(G):
        one[seg[g]:seg[g + 1], g] = 1
    A, Q = M.astype(np.int64) @ (one * w[:, None]), M.astype(np.int64) @ (one * wq[:, None])
    assert A.max(initial=0) < 1 << 31 and Q.max(initial=0) < 1 << 53
    with np.errstate(divide="ignore", invalid="ignore"):
        v = Q.astype(np.float64) / A.astype(np.float64)
    v[A == 0] = np.inf
    return v, A


def interval(v, level_bp):
    """(lo, hi, D) of one series"""
    D = int(np.isfinite(v).sum())
    if D == 0:
        return np.inf, np.inf, 0
    k, s = rank_k(D, level_bp), np.sort(v)
    return float(s[k - 1]), float(s[D - k]), D


def level_bp(text):
    whole, _dot, frac = text.partition(".")
    return int(whole) * 100 + int((frac + "00")[:2])


def exp_len(alpha, cnt):
    """the reference's exp_pa_len (apa_core.py:1038-1052) of the counts of the K labels, K >= 2"""
    if cnt.sum() == 0:
        return float("nan")
    ws = cnt.astype(np.float64)
    ws = ws / np.sum(ws)
    with np.errstate(all="ignore"):
        n_arr = 1.0 + 9.0 * (alpha - alpha[0]) / (alpha[-1] - alpha[0])
        return float(np.sum(ws * n_arr))


def oracle_lines(records, bc, clu_text, idents, n_boot, level, seed):
    """the file's lines as lists of text fields.  Columns: gene = gene_info_str; group; num_pa = kept rows; reads =
    A_g(0); mean_pos = the exact rational sum a_ig x_i / A_g rounded once; mean_pos_lo / _hi = min x + ldexp(lo / hi,
    -s); exp_length = exp_len of the population's counts of all K labels; exp_length_lo / _hi = 1.0 + 9.0 * (y - a[0])
    / (a[-1] - a[0]) with y = mean_pos_lo / _hi, empty when exp_length is nan or a[-1] - a[0] is not finite and
    positive; n_empty = n_boot - D_g; n_boot; level = the option's text.  Interval fields are empty when D_g = 0.
    clu_text = None: one population all_cell of every column"""
    col_ids = rc.column_ids(bc)
    pops = [("all_cell", list(range(len(col_ids))))] if clu_text is None else populations_all(bc, clu_text, idents)
    cell = np.array([j for _n, cols in pops for j in cols], dtype=np.int64)
    seg = np.concatenate([[0], np.cumsum([len(cols) for _n, cols in pops])])
    M = mult(seed, 1, n_boot, cell)
    L = level_bp(level)
    lines = []
    for rec, dense in zip(records, rc.dense_counts(records, col_ids)):
        K, alpha = int(rec["K"]), np.asarray(rec["alpha_arr"])
        sub = dense[:, cell]
        kept = [lb for lb in range(K) if sub[lb].any()]
        if len(kept) < 2:
            continue
        x = [float(alpha[lb]) for lb in kept]
        assert all(math.isfinite(v) for v in x)
        if not max(x) - min(x) > 0:
            continue
        q, s = quantise(x)
        v, _A = series_values(sub[kept], q, seg, M)
        for g, (name, _cols) in enumerate(pops):
            a = sub[kept][:, seg[g]:seg[g + 1]].sum(axis=1).tolist()
            if sum(a) == 0:
                continue
            mean = float(sum(ai * Fraction(xi) for ai, xi in zip(a, x)) / sum(a))
            e = exp_len(alpha, sub[:, seg[g]:seg[g + 1]].sum(axis=1))
            lo, hi, D = interval(v[:, g], L)
            iv = ["", "", "", ""]
            if D:
                ys = [min(x) + math.ldexp(lo, -s), min(x) + math.ldexp(hi, -s)]
                a0, width = float(alpha[0]), float(alpha[-1]) - float(alpha[0])
                iv = [repr(y) for y in ys] + (["", ""] if math.isnan(e) or not (math.isfinite(width) and width > 0) else
                                              [repr(1.0 + 9.0 * (y - a0) / width) for y in ys])
            lines.append([rec["gene_info_str"], name, str(len(kept)), str(sum(a)), repr(mean)] + iv[:2] + [repr(e)] +
                         iv[2:] + [str(n_boot - D), str(n_boot), level])
    return lines


def as_text(lines):
    out = io.StringIO()
    w = csv.writer(out, delimiter=',', quoting=csv.QUOTE_MINIMAL, lineterminator='\n')
    w.writerow(HEADER)
    w.writerows(lines)
    return out.getvalue()


# ---------------------------------------------------------------- the command
def _args(root, clu=None, res="res.gene.pkl", idents=(), n_boot=None, level=None, seed=None):
    a = ["boot_pa_len", "--output_dir", str(root), "--res_pkl_file", res]
    if clu is not None:
        a += ["--cell_cluster_file", str(clu)]
    for i in idents:
        a += ["--idents", i]
    for opt, v in (("--n_boot", n_boot), ("--level", level), ("--seed", seed)):
        if v is not None:
            a += [opt, str(v)]
    return a


def _path(root, clu, res, idents=()):
    kind = res[len("res."):-len(".pkl")]
    if clu is None:
        return os.path.join(str(root), f"all_cell.{kind}.boot_pa_len.csv")
    stem = os.path.splitext(os.path.basename(str(clu)))[0]
    tag = "." + "+".join(idents) if idents else ""
    return os.path.join(str(root), f"{stem}.{kind}{tag}.boot_pa_len.csv")


def _command(root, clu, res, idents, n_boot, level, seed, what=""):
    r = _run(_args(root, clu, res, idents, n_boot, level, seed))
    assert r.exit_code == 0, (what, r.output, repr(r.exception))
    assert not rc.parts_left(root)
    with open(_path(root, clu, res, idents), newline="") as fh:
        return fh.read()


# ---------------------------------------------------------------- CPU
def test_threshold_table():
    """P recomputed from Fractions: e^-1 as the alternating series to 80 terms, whose remainder is below the first
    term left out and cannot move a floor; equal to this file's table, to report.py's and to the header's"""
    from conftest import ROOT
    from scape_amd import report
    n_terms = 80
    e_inv = sum(Fraction((-1) ** j, math.factorial(j)) for j in range(n_terms + 1))
    eps = Fraction(1, math.factorial(n_terms + 1))
    table = []
    for k in range(15):
        S = sum(Fraction(1, math.factorial(i)) for i in range(k + 1))
        below, above = math.floor((e_inv - eps) * S * 2 ** 64), math.floor((e_inv + eps) * S * 2 ** 64)
        assert below == above, k
        table.append(below)
    assert table == P and tuple(P) == report.BOOT_THRESHOLDS
    hdr = open(os.path.join(ROOT, "include", "scape_hip.h")).read()
    part = hdr[hdr.index("P[k] = floor(2^64"):hdr.index("so m is Poisson(1)")]
    assert [int(v, 16) for v in re.findall(r"0x[0-9A-F]{16}", part)] == P
    tail = 1 - e_inv * sum(Fraction(1, math.factorial(i)) for i in range(16))     # P(m > 15), folded into m = 15
    assert Fraction(18, 10 ** 15) < tail < Fraction(2, 10 ** 14)


def test_multiplicity_oracle():
    """seed 1, b = 1..1024, c = 0..1023: the counts of m = 0..7 lie within 4 binomial standard deviations of
    n e^-1 / k!; a fixed-seed check that guards the table and the direction of the comparison.  The array form of the
    hash is the scalar one"""
    m = mult(1, 1, 1024, np.arange(1024))
    n = m.size
    counts = np.bincount(m.ravel(), minlength=16)
    worst = 0.0
    for k in range(8):
        p = math.exp(-1) / math.factorial(k)
        z = abs(counts[k] - n * p) / math.sqrt(n * p * (1 - p))
        worst = max(worst, z)
        assert z < 4, (k, counts[k], n * p)
    print("counts", counts.tolist(), "worst z", worst, "max", m.max(), "mean", m.mean())
    assert counts[:8].tolist() == [384776, 386997, 192824, 64177, 15888, 3213, 601, 92] and m.max() == 9
    assert abs(m.mean() - 1) < 4 / math.sqrt(n)
    for b, c in ((1, 0), (7, 1023), (1024, 5)):
        h = rc.mix((rc.mix((1 + rc.G * b) & rc.M64) + rc.G * (c + 1)) & rc.M64)
        assert int(hashes(1, b, 1, [c])[0, 0]) == h
        assert int(m[b - 1, c]) == sum(h >= p for p in P)
    big = 2 ** 64 - 1
    h = rc.mix((rc.mix((big + rc.G * 3) & rc.M64) + rc.G * 8) & rc.M64)
    assert int(hashes(big, 3, 1, [7])[0, 0]) == h


def test_rank_rule_and_level_parser():
    from scape_amd import report
    for (D, L), k in (((9999, 9500), 250), ((39, 9500), 1), ((1, 9500), 1), ((999, 9950), 2)):
        assert report._boot_rank(D, L) == k == rank_k(D, L)
    for L in (1, 9000, 9500, 9950, 9999):
        for D in list(range(1, 300)) + [9999, 10 ** 6]:
            k = report._boot_rank(D, L)
            assert 1 <= k <= D + 1 - k
    for text, bp in (("95", 9500), ("99.5", 9950), ("90.00", 9000), ("0.01", 1), ("99.99", 9999), ("5", 500)):
        assert report._parse_level(text) == bp == level_bp(text)
    for text in ("0", "100", "95.123", "-1", "abc", "", "0.00", "1e1", "95.", ".5", "100.00", " 95"):
        with pytest.raises(ValueError):
            report._parse_level(text)


def test_help_and_import_path():
    r = _run(["--help"])
    assert r.exit_code == 0 and "boot_pa_len" in r.output
    r = _run(["boot_pa_len", "--help"])
    assert r.exit_code == 0, r.output
    for o in ("--output_dir", "--res_pkl_file", "--cell_cluster_file", "--idents", "--n_boot", "--level", "--seed"):
        assert o in r.output
    assert "--strata_file" not in r.output and "--n_perm" not in r.output
    flat = " ".join(r.output.split())
    assert "[default: 9999]" in flat and "[default: 95]" in flat and "[default: 1]" in flat
    import scape.utils as su
    from scape_amd import _lib, report
    assert su.boot_pa_len is report.boot_pa_len
    for name in ("mult", "mult_get", "len", "vals_get", "quantiles"):
        assert "scape_hip_report_boot_" + name in _lib.SIGNATURES
    assert report.BOOT_PA_LEN_HEADER == HEADER


def test_prerequisites_and_argument_errors(tmp_path, no_gpu):
    """every check runs before the device is opened, and a refused run leaves the directory as it was"""
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
                        (["--idents", "A", "--idents", "ghost"], "has no cell"),
                        (["--idents", "A", "--idents", ""], "names no cluster"),
                        (["--idents", "A", "--idents", "a/b"], "file name"),
                        (["--n_boot", "0"], "n_boot"), (["--n_boot", str(1 << 31)], "n_boot"),
                        (["--seed", "-1"], "seed"), (["--seed", str(1 << 64)], "seed"),
                        (["--level", "0"], "level"), (["--level", "100"], "level"), (["--level", "95.123"], "level"),
                        (["--level", "-1"], "level"), (["--level", "abc"], "level")):
        r = _run(_args(tmp_path, clu) + extra)
        assert isinstance(r.exception, ValueError) and word in str(r.exception), (extra, repr(r.exception))
    for extra in (["--level", "abc"], ["--n_boot", "0"]):                 # the option checks need no cluster file
        r = _run(_args(tmp_path) + extra)
        assert isinstance(r.exception, ValueError), (extra, repr(r.exception))
    r = _run(_args(tmp_path) + ["--idents", "A"])
    assert r.exit_code == 2 and "--cell_cluster_file" in r.output
    ids = list(range(100, 166))
    (tmp_path / "barcode_index.csv").write_text("CB,index\n" + "".join(f"C{i}-1,{i}\n" for i in ids))
    clu.write_text("index,group\n" + "".join(f"{i},g{i}\n" for i in ids[:65]))
    r = _run(_args(tmp_path, clu))
    assert isinstance(r.exception, ValueError) and "65 clusters: boot_pa_len" in str(r.exception)
    assert "--idents" in str(r.exception)
    r = _run(_args(tmp_path, clu) + ["--strata_file", str(clu)])
    assert r.exit_code == 2 and "--strata_file" in r.output
    r = _run(["boot_pa_len", "--res_pkl_file", "res.gene.pkl"])
    assert r.exit_code == 2 and "--output_dir" in r.output
    assert sorted(os.listdir(tmp_path)) == ["barcode_index.csv", "groups.csv", "res.gene.pkl"]


def test_host_columns():
    """mean_pos_lo / _hi and exp_length_lo / _hi from hand-made order statistics: integer positions, a position set
    that is not dyadic (tenths, s = 20), and the empty-field cases"""
    from scape_amd import report
    alpha = np.array([100, 300, 1124])                                   # span 1024 = 2^10: frexp e = 11, s = 11
    got = report._boot_columns(float(1 << 19), float(3 << 19), 100.0, 11, alpha, 4.5)
    assert got == [repr(100.0 + 256.0), repr(100.0 + 768.0), repr(1.0 + 9.0 * 256.0 / 1024.0),
                   repr(1.0 + 9.0 * 768.0 / 1024.0)] == ["356.0", "868.0", "3.25", "7.75"]
    x = [0.1, 0.7, 2.5]
    q, s = quantise(x)
    assert s == 20 and not all((Fraction(v - 0.1) * 2 ** s).denominator == 1 for v in x)
    lo, hi = 1234567.25, float(q[2]) - 0.5
    got = report._boot_columns(lo, hi, 0.1, s, np.array(x), 2.0)
    ys = [0.1 + math.ldexp(lo, -s), 0.1 + math.ldexp(hi, -s)]
    assert got == [repr(ys[0]), repr(ys[1]), repr(1.0 + 9.0 * (ys[0] - 0.1) / (2.5 - 0.1)),
                   repr(1.0 + 9.0 * (ys[1] - 0.1) / (2.5 - 0.1))]
    assert report._boot_columns(None, None, 0.1, s, np.array(x), 2.0) == ["", "", "", ""]          # D = 0
    assert report._boot_columns(lo, hi, 0.1, s, np.array(x), float("nan")) == [repr(ys[0]), repr(ys[1]), "", ""]
    for bad in ([120, 480, 120], [500, 20, 260, 90], [1.0, 2.0, float("inf")]):                   # a[-1] - a[0] <= 0, inf
        assert report._boot_columns(1.0, 2.0, 0.0, 0, np.array(bad), 2.0)[2:] == ["", ""]


@functools.lru_cache(maxsize=None)
def _syn_lines(idents, n_boot, level, seed, all_cell=False, n_rec=None):
    records, bc, clu_text = rc.synthetic()
    return oracle_lines(records[:n_rec], bc, None if all_cell else clu_text, idents, n_boot, level, seed)


def _assert_purpose(lines):
    """records 0, 1 and 2 of the synthetic directory (A uses its first site ten times as often): cluster A's
    mean_pos_hi lies below cluster B's mean_pos_lo; record 3's intervals overlap and it is left out on purpose.  The
    40 cells of cluster C leave some replicate of some record without a read"""
    by = {(ln[0].split(":")[1], ln[1]): ln for ln in lines}
    for gene in ("GENE0", "GENE1", "GENE2"):
        a_hi, b_lo = float(by[(gene, "A")][6]), float(by[(gene, "B")][5])
        print(gene, "A hi", a_hi, "B lo", b_lo)
        assert a_hi < b_lo, gene
    empty = {ln[0].split(":")[1]: int(ln[10]) for ln in lines if ln[1] == "C" and int(ln[10]) > 0}
    print("n_empty of C", empty)
    assert empty


def test_purpose_on_the_oracle():
    _assert_purpose(_syn_lines((), 999, "95", 1))


# ---------------------------------------------------------------- GPU: the entry points
def _p(a):
    from scape_amd._lib import P_d, P_i32, P_i64, ptr
    import ctypes
    return ptr(a, {np.dtype(np.float64): P_d, np.dtype(np.int32): P_i32, np.dtype(np.int64): P_i64,
                   np.dtype(np.uint8): ctypes.POINTER(ctypes.c_uint8)}[a.dtype])


def _boot_mult(ctx, cell, b_first, b_count, seed):
    cell = np.ascontiguousarray(cell, dtype=np.int32)
    return ctx.lib.scape_hip_report_boot_mult(ctx.h, len(cell), _p(cell), b_first, b_count, seed)


def _mult_get(ctx, n, b_count):
    """[b_count, n] of the last boot_mult call"""
    from scape_amd._lib import check
    out = np.full((b_count, n), 255, dtype=np.uint8)
    for b in range(b_count):
        check(ctx.lib.scape_hip_report_boot_mult_get(ctx.h, b, _p(out[b])), "boot_mult_get")
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [0, 1, 2 ** 64 - 1])
def test_boot_mult(seed):
    """the bytes of k_rep_boot_mult against the oracle: positions around a wave, chunks around the 256-replicate tile
    and one that starts past it; `cell` is a reversed map with gaps.  A cell keeps its bytes wherever it is placed"""
    from scape_amd import _lib
    ctx = _lib.default_context(None)
    try:
        for n in (1, 63, 64, 65, 257):
            cell = (3 * np.arange(n)[::-1] + 5).astype(np.int32)
            for b_first, b_count in ((1, 1), (1, 255), (1, 256), (1, 257), (257, 120)):
                _lib.check(_boot_mult(ctx, cell, b_first, b_count, seed), "boot_mult")
                got = _mult_get(ctx, n, b_count)
                assert np.array_equal(got, mult(seed, b_first, b_count, cell)), (n, b_first, b_count)
        cell = np.array([40, 7, 1000, 3, 7000], dtype=np.int32)
        _lib.check(_boot_mult(ctx, cell, 1, 300, seed), "boot_mult")
        first = _mult_get(ctx, 5, 300)
        moved = np.array([9, 8, 3, 40, 11, 12, 1000], dtype=np.int32)
        _lib.check(_boot_mult(ctx, moved, 1, 300, seed), "boot_mult")
        second = _mult_get(ctx, 7, 300)
        assert np.array_equal(first[:, [0, 2, 3]], second[:, [3, 6, 2]]) and first.max() >= 4
        assert ctx.lib.scape_hip_report_boot_mult_get(ctx.h, 300, _p(np.zeros(7, np.uint8))) != 0
        assert "scape_hip_report_boot_mult_get" in _lib.last_error()
    finally:
        ctx.lib.scape_hip_report_free(ctx.h)


EP_CHUNKS = (150, 120)                    # 270 replicates: one tile of 256 and a part, written in two chunks
EP_SEED = 77


def ep_sizes(G, n):
    """segments over the n tested columns: the first takes what the others leave, the second 7 cells, the rest one
    cell each (the sparse high columns of the matrix)"""
    if G == 1:
        return [n]
    if G == 2:
        return [n - 1, 1]
    return [n - 7 - (G - 2), 7] + [1] * (G - 2)


@functools.lru_cache(maxsize=None)
def ep_case(G):
    """rc.entry_point_matrix() with G segments: (matrix, cell, q, seg, per record (values [270, G], t, a0))"""
    n1, n2, n_cols, _seed, _n_perm, Ks, off, lab, cb, dense, rows, roff, _rng = rc.entry_point_matrix()
    n = n1 + n2
    rng = np.random.default_rng(3)
    cell = (7 * np.arange(n) + 3).astype(np.int32)
    q = rng.integers(0, (1 << 22) + 1, len(rows)).astype(np.int32)
    q[0], q[1] = 0, 1 << 22
    seg = np.concatenate([[0], np.cumsum(ep_sizes(G, n))]).astype(np.int32)
    assert seg[-1] == n
    M = mult(EP_SEED, 1, sum(EP_CHUNKS), cell)
    recs = []
    for r in range(len(Ks)):
        sub = dense[rows[roff[r]:roff[r + 1]], :n]
        v, _A = series_values(sub, q[roff[r]:roff[r + 1]], seg, M)
        a0 = np.stack([sub[:, seg[g]:seg[g + 1]].sum(axis=1) for g in range(G)], axis=1)
        recs.append((v, sub.sum(axis=1), a0))
    return dict(Ks=Ks, off=off, lab=lab, cb=cb, n_cols=n_cols, rows=rows, roff=roff, n=n), cell, q, seg, recs


def _boot_len(ctx, m, G, seg, q, n_boot, roff=None, rows=None):
    roff, rows = m["roff"] if roff is None else roff, m["rows"] if rows is None else rows
    t, a0 = np.full(len(rows), -1, np.int64), np.full((len(rows), G), -1, np.int64)
    rc_ = ctx.lib.scape_hip_report_boot_len(ctx.h, len(roff) - 1, _p(roff), _p(rows), G, _p(seg), _p(q), n_boot, _p(t),
                                            _p(a0))
    return rc_, t, a0


def _vals_get(ctx, series, n_boot):
    from scape_amd._lib import check
    out = np.full(n_boot, -1.0)
    check(ctx.lib.scape_hip_report_boot_vals_get(ctx.h, series, _p(out)), "boot_vals_get")
    return out


def _quantiles(ctx, level, n_series):
    lo, hi, D = np.full(n_series, -1.0), np.full(n_series, -1.0), np.full(n_series, -1, np.int64)
    return ctx.lib.scape_hip_report_boot_quantiles(ctx.h, level, _p(lo), _p(hi), _p(D)), lo, hi, D


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.mark.gpu
@pytest.mark.parametrize("G", [1, 2, 3, 17, 32, 33, 64])
def test_boot_len(G):
    """scape_hip_report_boot_len on the hand-made matrix (records of 2, 5, 70 and 150 rows), 270 replicates written in
    chunks of 150 and 120: every series equals the oracle bit for bit, t and a0 are exact, and so are the intervals at
    both levels.  With 17 populations or more the single-cell segments hold a population without a read in some record
    (all +infinity), one whose reads of a record sit in one cell (about 37 % of its replicates empty, every other value
    the same) and one whose reads all sit at one site (a constant value)"""
    from scape_amd import _lib
    m, cell, q, seg, recs = ep_case(G)
    n_boot = sum(EP_CHUNKS)
    ctx = _lib.default_context(None)
    try:
        rc.device_counts(ctx, m["Ks"], m["off"], m["lab"], m["cb"], m["n_cols"])
        first = 1
        for b_count in EP_CHUNKS:
            _lib.check(_boot_mult(ctx, cell, first, b_count, EP_SEED), "boot_mult")
            rc_, t, a0 = _boot_len(ctx, m, G, seg, q, n_boot)
            _lib.check(rc_, "boot_len")
            first += b_count
        got = np.stack([_vals_get(ctx, k, n_boot) for k in range(len(recs) * G)]).reshape(len(recs), G, n_boot)
        quant = {L: _quantiles(ctx, L, len(recs) * G) for L in (9500, 9950)}
    finally:
        ctx.lib.scape_hip_report_free(ctx.h)
    assert np.array_equal(t, np.concatenate([r[1] for r in recs]))
    assert np.array_equal(a0, np.concatenate([r[2] for r in recs]))
    seen = dict(empty=False, one_cell=False, constant=False)
    for r, (v, _t, _a0) in enumerate(recs):
        for g in range(G):
            assert np.array_equal(_bits(got[r, g]), _bits(v[:, g])), (G, r, g)
            D = int(np.isfinite(v[:, g]).sum())
            seen["empty"] |= D == 0
            one = seg[g + 1] - seg[g] == 1 and D > 0
            seen["one_cell"] |= one and 0.25 < 1 - D / n_boot < 0.5
            seen["constant"] |= one and len(set(v[np.isfinite(v[:, g]), g].tolist())) == 1
    print(G, seen)
    assert G < 17 or all(seen.values()), seen
    for L, (rc_, lo, hi, D) in quant.items():
        assert rc_ == 0
        for r, (v, _t, _a0) in enumerate(recs):
            for g in range(G):
                want = interval(v[:, g], L)
                k = r * G + g
                assert (_bits(lo[k:k + 1])[0], _bits(hi[k:k + 1])[0], int(D[k])) == \
                    (_bits([want[0]])[0], _bits([want[1]])[0], want[2]), (G, L, r, g)


def _reads_of(dense, Ks):
    """(read offsets, labels, cell ids) of records whose dense counts are given"""
    lab, cb, off, base = [], [], [0], 0
    for K in Ks.tolist():
        lb, c = np.nonzero(dense[base:base + K])
        rep = dense[base:base + K][lb, c]
        lab.append(np.repeat(lb, rep))
        cb.append(np.repeat(c, rep))
        off.append(off[-1] + int(rep.sum()))
        base += K
    return np.array(off, np.int64), np.concatenate(lab).astype(np.int64), np.concatenate(cb).astype(np.int64)


Q_SIZES = [2, 1, 1, 3]
Q_DENSE = np.array([[3, 0, 2, 0, 1, 0, 5],        # record 0, two rows: population 0 has one cell per site (few distinct
                    [0, 4, 1, 0, 2, 3, 0],        # values: ties), 1 is one cell (constant), 2 has no read, 3 three cells
                    [1, 1, 0, 0, 0, 0, 2],        # record 1, three rows; population 1 has no read either
                    [0, 2, 0, 0, 1, 0, 0],
                    [1, 0, 0, 0, 0, 3, 1]], dtype=np.int64)
Q_KS = np.array([2, 3], dtype=np.int32)
Q_ROFF = np.array([0, 2, 5], dtype=np.int64)
Q_POS = np.array([0, 1 << 22, 17, 3000001, 1 << 21], dtype=np.int32)


@pytest.mark.gpu
@pytest.mark.parametrize("n_boot", [1, 2, 39, 255, 256, 257, 1000])
def test_boot_quantiles(n_boot):
    """lo, hi and D of k_rep_boot_select against np.sort at two levels, around the 256-thread stride: a series of few
    distinct values with ties across rank k, a constant one (lo = hi), an all-empty one (D = 0: both +infinity)"""
    from scape_amd import _lib
    n = sum(Q_SIZES)
    seg = np.concatenate([[0], np.cumsum(Q_SIZES)]).astype(np.int32)
    cell = np.arange(n, dtype=np.int32) * 11
    off, lab, cb = _reads_of(Q_DENSE, Q_KS)
    rows = np.arange(5, dtype=np.int64)
    G = len(Q_SIZES)
    M = mult(5, 1, n_boot, cell)
    vs = [series_values(Q_DENSE[Q_ROFF[r]:Q_ROFF[r + 1]], Q_POS[Q_ROFF[r]:Q_ROFF[r + 1]], seg, M)[0] for r in range(2)]
    ctx = _lib.default_context(None)
    try:
        rc.device_counts(ctx, Q_KS, off, lab, cb, n)
        _lib.check(_boot_mult(ctx, cell, 1, n_boot, 5), "boot_mult")
        rc_, _t, _a0 = _boot_len(ctx, None, G, seg, Q_POS, n_boot, Q_ROFF, rows)
        _lib.check(rc_, "boot_len")
        quant = {L: _quantiles(ctx, L, 2 * G) for L in (9500, 9950)}
    finally:
        ctx.lib.scape_hip_report_free(ctx.h)
    for L, (rc_, lo, hi, D) in quant.items():
        assert rc_ == 0
        for r in range(2):
            for g in range(G):
                want = interval(vs[r][:, g], L)
                k = r * G + g
                print(n_boot, L, r, g, "got", lo[k], hi[k], D[k], "want", want)
                assert (_bits(lo[k:k + 1])[0], _bits(hi[k:k + 1])[0], int(D[k])) == \
                    (_bits([want[0]])[0], _bits([want[1]])[0], want[2]), (n_boot, L, r, g)
        assert D[2] == 0 and np.isinf(lo[2]) and np.isinf(hi[2])                 # no read at all
        assert D[1] == 0 or lo[1] == hi[1]                                       # one cell: a constant
    if n_boot >= 255:
        v = vs[0][:, 0]
        k = rank_k(int(np.isfinite(v).sum()), 9500)
        s = np.sort(v)
        assert s[k - 1] == s[k] or s[k - 1] == s[k - 2]                          # ties straddle rank k
        assert len(set(v.tolist())) < 60


@pytest.mark.gpu
def test_refusals():
    """each refused call returns non-zero with its entry point's name in the message, and the valid calls before and
    after it give the same outputs"""
    from scape_amd import _lib
    m, cell, q, seg, _recs = ep_case(3)
    G, n_boot = 3, 270
    n_series = len(m["Ks"]) * G
    ctx = _lib.default_context(None)
    lib = ctx.lib

    def build(b_first=1, b_count=n_boot):
        return _boot_mult(ctx, cell, b_first, b_count, EP_SEED)

    def good():
        _lib.check(build(), "boot_mult")
        rc_, t, a0 = _boot_len(ctx, m, G, seg, q, n_boot)
        _lib.check(rc_, "boot_len")
        rc_, lo, hi, D = _quantiles(ctx, 9500, n_series)
        _lib.check(rc_, "boot_quantiles")
        return [a.tobytes() for a in (t, a0, lo, hi, D, _vals_get(ctx, 4, n_boot))]

    def refused(rc_, entry, word):
        assert rc_ != 0 and entry in _lib.last_error() and word in _lib.last_error(), _lib.last_error()

    def changed(a, k, v):
        b = a.copy()
        b[k] = v
        return b
    try:
        refused(_boot_len(ctx, m, G, seg, q, n_boot)[0], "scape_hip_report_boot_len", "report_counts")
        rc.device_counts(ctx, m["Ks"], m["off"], m["lab"], m["cb"], m["n_cols"])
        refused(_boot_len(ctx, m, G, seg, q, n_boot)[0], "scape_hip_report_boot_len", "boot_mult has not been called")
        refused(_quantiles(ctx, 9500, n_series)[0], "scape_hip_report_boot_quantiles", "boot_len has not been called")
        first = good()
        refused(build(b_first=0), "scape_hip_report_boot_mult", "b_first")
        refused(build(b_count=0), "scape_hip_report_boot_mult", "b_count")
        refused(_boot_mult(ctx, changed(cell, 5, -1), 1, 10, 1), "scape_hip_report_boot_mult", "negative cell")
        refused(_boot_len(ctx, m, G, seg, changed(q, 3, (1 << 22) + 1), n_boot)[0], "scape_hip_report_boot_len", "2^22")
        refused(_boot_len(ctx, m, G, seg, changed(q, 3, -1), n_boot)[0], "scape_hip_report_boot_len", "2^22")
        refused(_boot_len(ctx, m, 0, seg[:1].copy(), q, n_boot)[0], "scape_hip_report_boot_len", "n_groups")
        seg65 = np.concatenate([np.arange(65), [m["n"]]]).astype(np.int32)
        refused(_boot_len(ctx, m, 65, seg65, q, n_boot)[0], "scape_hip_report_boot_len", "n_groups")
        refused(_boot_len(ctx, m, G, changed(seg, 3, seg[3] - 1), q, n_boot)[0], "scape_hip_report_boot_len", "seg_off")
        refused(_boot_len(ctx, m, G, changed(seg, 0, 1), q, n_boot)[0], "scape_hip_report_boot_len", "seg_off")
        refused(_boot_len(ctx, m, G, seg, q, n_boot - 1)[0], "scape_hip_report_boot_len", "n_boot")
        refused(_quantiles(ctx, 0, n_series)[0], "scape_hip_report_boot_quantiles", "level_bp")
        refused(_quantiles(ctx, 10000, n_series)[0], "scape_hip_report_boot_quantiles", "level_bp")
        refused(lib.scape_hip_report_boot_vals_get(ctx.h, n_series, _p(np.zeros(n_boot))),
                "scape_hip_report_boot_vals_get", "series")
        # a record of 2^27 reads, built from few large counts: the heaviest kept row, 2^27 / its reads times over
        t_rows = np.frombuffer(first[0], dtype=np.int64)
        heavy_row, reads = int(m["rows"][int(np.argmax(t_rows))]), int(t_rows.max())
        heavy = np.full(-(-(1 << 27) // reads), heavy_row, dtype=np.int64)
        rc_, t, _a0 = _boot_len(ctx, None, G, seg, np.zeros(len(heavy), np.int32), n_boot,
                                np.array([0, len(heavy)], np.int64), heavy)
        refused(rc_, "scape_hip_report_boot_len", "2^27 or more reads")
        assert good() == first
        # quantiles before every column is written: a record set begun with 150 of the 270 replicates
        _lib.check(build(1, 150), "boot_mult")
        _lib.check(_boot_len(ctx, m, G, seg, q, n_boot)[0], "boot_len")
        refused(_quantiles(ctx, 9500, n_series)[0], "scape_hip_report_boot_quantiles", "replicate 151")
        _lib.check(build(151, 120), "boot_mult")
        refused(_boot_len(ctx, m, G, seg, q, n_boot, m["roff"][:3].copy(), m["rows"][:int(m["roff"][2])].copy())[0],
                "scape_hip_report_boot_len", "later chunk")
        _lib.check(_boot_len(ctx, m, G, seg, q, n_boot)[0], "boot_len")
        rc_, lo, hi, D = _quantiles(ctx, 9500, n_series)
        assert rc_ == 0 and [a.tobytes() for a in (lo, hi, D)] == first[2:5]
        assert good() == first
    finally:
        lib.scape_hip_report_free(ctx.h)


# ---------------------------------------------------------------- GPU: the command
def _check_syn(tmp_path, idents, n_boot, level, seed, what, all_cell=False, n_rec=None):
    lines = _syn_lines(idents, n_boot, level, seed, all_cell, n_rec)
    path = rc.write_synthetic(tmp_path, n_rec)
    text = _command(tmp_path, None if all_cell else path, "res.gene.pkl", idents, n_boot, level, seed, what)
    want = as_text(lines)
    if text != want:
        for a, b in zip(text.split("\n"), want.split("\n")):
            assert a == b, (what, a, b)
    assert text == want, what
    return text, lines


@pytest.mark.gpu
def test_synthetic_directory_all_clusters_and_purpose(tmp_path):
    """999 replicates of 230 + 301 + 40 cells in the clusters A, B, C: the whole file equals the oracle's text; read
    from the file, cluster A's interval of GENE0..GENE2 lies below cluster B's"""
    text, lines = _check_syn(tmp_path, (), 999, "95", 1, "syn/all")
    assert len(lines) > 90 and {ln[1] for ln in lines} == {"A", "B", "C"}
    assert max(int(ln[2]) for ln in lines) == 63
    _assert_purpose(list(csv.reader(io.StringIO(text)))[1:])
    assert os.path.basename(_path(tmp_path, "syn_groups.csv", "res.gene.pkl")) == "syn_groups.gene.boot_pa_len.csv"


@pytest.mark.gpu
def test_synthetic_directory_idents_in_the_order_given(tmp_path):
    """--idents B --idents A at level 99.5: the file name carries .B+A and B's line of a record comes first"""
    _text, lines = _check_syn(tmp_path, ("B", "A"), 299, "99.5", 3, "syn/B+A")
    assert os.path.exists(os.path.join(str(tmp_path), "syn_groups.gene.B+A.boot_pa_len.csv"))
    assert [ln[1] for ln in lines[:2]] == ["B", "A"] and lines[0][12] == "99.5"


@pytest.mark.gpu
def test_synthetic_directory_all_cell(tmp_path):
    """no cluster file: one population all_cell of all 600 columns, the cells without a cluster included"""
    _text, lines = _check_syn(tmp_path, (), 299, "90.00", 1, "syn/all_cell", all_cell=True)
    assert {ln[1] for ln in lines} == {"all_cell"} and lines[0][12] == "90.00"
    assert os.path.exists(os.path.join(str(tmp_path), "all_cell.gene.boot_pa_len.csv"))


@pytest.mark.gpu
@pytest.mark.parametrize("n_boot", [1, 255, 256, 257])
def test_tile_edges(n_boot, tmp_path):
    """a workgroup of k_rep_boot_len takes 256 replicates: one short of a tile, a full tile, one over, and one"""
    _text, lines = _check_syn(tmp_path, ("C", "A", "B"), n_boot, "95", 5, f"tile/{n_boot}", n_rec=12)
    assert len(lines) >= 20


@pytest.mark.gpu
def test_batch_chunk_and_seed_invariance(tmp_path, monkeypatch):
    """records split over several count batches and the replicates over several chunks: the same bytes.  Another seed
    changes the four interval columns and n_empty only"""
    from scape_amd import _lib, report
    path = rc.write_synthetic(tmp_path)
    big = _command(tmp_path, path, "res.gene.pkl", (), 299, "95", 1)
    other = list(csv.reader(io.StringIO(_command(tmp_path, path, "res.gene.pkl", (), 299, "95", 2))))
    mine = list(csv.reader(io.StringIO(big)))
    fixed = [0, 1, 2, 3, 4, 7, 11, 12]
    assert [[r[c] for c in fixed] for r in mine] == [[r[c] for c in fixed] for r in other] and len(mine) > 90
    assert [r[5:7] for r in mine] != [r[5:7] for r in other]
    lib = _lib.load_library()
    calls = {"mult": [], "len": 0}
    real_m, real_l = lib.scape_hip_report_boot_mult, lib.scape_hip_report_boot_len

    def make_mult(*a):
        calls["mult"].append((a[3], a[4]))
        return real_m(*a)

    def boot_len(*a):
        calls["len"] += 1
        return real_l(*a)
    monkeypatch.setattr(lib, "scape_hip_report_boot_mult", make_mult)
    monkeypatch.setattr(lib, "scape_hip_report_boot_len", boot_len)
    monkeypatch.setattr(report, "MAX_BATCH_BYTES", 1 << 16)             # a record of K = 8 alone takes 57 KB
    monkeypatch.setattr(report, "MAX_PERM_BYTES", 1 << 30)
    assert _command(tmp_path, path, "res.gene.pkl", (), 299, "95", 1) == big
    assert calls["mult"] == [(1, 299)] and calls["len"] > 5
    n_batches = calls["len"]
    calls.update(mult=[], len=0)
    monkeypatch.setattr(report, "MAX_PERM_BYTES", 571 * 100)             # one byte per tested cell: 100 replicates
    assert _command(tmp_path, path, "res.gene.pkl", (), 299, "95", 1) == big
    assert calls["len"] == 3 * n_batches and calls["mult"][:3] == [(1, 100), (101, 100), (201, 99)]


@pytest.mark.gpu
def test_a_cluster_alone_has_the_lines_it_has_among_all(tmp_path):
    """a cell's multiplicity depends on the cell, not on the clustering: on a directory where every cluster has reads at
    every kept row, the lines of `--idents A` are cluster A's lines of the all-cluster file, byte for byte"""
    path, clu_text, bc, records, _ids = rc.small_dir(tmp_path, 40, 15, 6)
    for (name, cols) in populations_all(bc, clu_text):
        for dense in rc.dense_counts(records, rc.column_ids(bc)):
            assert np.array_equal(dense[:, cols].any(axis=1), dense.any(axis=1)), name
    both = _command(tmp_path, path, "res.utr.pkl", (), 299, "95", 1).split("\n")
    assert both == as_text(oracle_lines(records, bc, clu_text, (), 299, "95", 1)).split("\n")
    for name in ("A", "B"):
        alone = _command(tmp_path, path, "res.utr.pkl", (name,), 299, "95", 1).split("\n")
        assert alone[1:-1] == [ln for ln in both[1:] if ln.split(",")[1:2] == [name]] and len(alone) == 10


@pytest.mark.gpu
def test_agreement_with_the_neighbours(tmp_path):
    """reads and mean_pos are diff_pa_len_groups's reads.<g> and mean_pos.<g>, exp_length is cal_exp_pa_len's value for
    the gene and cluster, as text, on a directory whose cluster file covers every barcode"""
    from test_report_difflen import _two_group_dir
    alphas = [[30, 200, 410], [500, 20, 260, 90], [10.5, 99.25, 300.0, 301.0, 580.75], [40, 41], [77, 77]]
    path, _clu_text, _bc, _recs = _two_group_dir(tmp_path, alphas)
    mine = list(csv.reader(io.StringIO(_command(tmp_path, path, "res.gene.pkl", (), 99, "95", 1))))[1:]
    assert len(mine) == 8                                                # TG4: span 0
    r = _run(["diff_pa_len_groups", "--output_dir", str(tmp_path), "--res_pkl_file", "res.gene.pkl",
              "--cell_cluster_file", path, "--n_perm", "9"])
    assert r.exit_code == 0, (r.output, repr(r.exception))
    with open(os.path.join(str(tmp_path), "two.gene.diff_pa_len_groups.csv"), newline="") as fh:
        theirs = list(csv.DictReader(fh))
    seen = 0
    for row in theirs:
        for ln in mine:
            if ln[0] == row["gene"]:
                assert (ln[3], ln[4]) == (row["reads." + ln[1]], row["mean_pos." + ln[1]]), (ln, row)
                seen += 1
    assert seen == 8
    r = _run(["cal_exp_pa_len", "--output_dir", str(tmp_path), "--cell_cluster_file", path, "--res_pkl_file",
              "res.gene.pkl"])
    assert r.exit_code == 0, (r.output, repr(r.exception))
    with open(os.path.join(str(tmp_path), "two.gene.pa.len.csv"), newline="") as fh:
        want = {(g, c): e or "nan" for g, c, e, _k in list(csv.reader(fh))[1:]}       # pandas writes NaN as ""
    for ln in mine:
        assert ln[7] == want[(":".join(ln[0].split(":")[1:3]), ln[1])], ln
