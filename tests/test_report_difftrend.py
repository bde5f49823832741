"""`scape diff_pa_trend`: the permutation test of pA usage ALONG a per-cell score such as pseudotime
(scape_amd/report.py, section diff_pa_trend; kernels k_rep_perm_scores, k_rep_trend_obs and k_rep_perm_trend and entry
points scape_hip_report_perm_scores / _scores_get / _perm_trend of scape_amd/csrc/perm.inc).

The contract.  The score file has the cluster file's format (an `index` column, the first other column is the score,
read as text and parsed with float(); a repeated id keeps its last row).  An empty field, NA or nan (any case) is no
score: the cell is left out.  inf or an unparsable field (naming the row), fewer than 2 scored cells in
barcode_index.csv, all scores equal and 2^24 cells or more are ValueErrors before the device is opened.  The tested
columns are the scored columns, ascending, position j = the j-th of them.  --rank replaces x_j by the integer
r_j = #{x < x_j} + #{x <= x_j}.  Integer scores:  w_j = fl(x_j - min x),  frexp(span) = (m, e),  s = 15 - e,
q_j = rint(ldexp(w_j, s)), half to even; so 2^14 <= qspan = max q_j <= 2^15.  The p-values are those of the test on the
q_j, and the file's score columns are in units of the quantised scores min x + q 2^-s.

Permutation p >= 1 ranks the positions by the key(p, j) of diff_pa (report_cases.key): rho_p(j) = #{i: key(p, i) <
key(p, j)}, a bijection, and position j receives the score z_p(j) = q[rho_p(j)].  When q is the observed group index
of G column segments, z_p is byte for byte the labelling of diff_pa_groups.

Kept rows of a record are the labels < K with a read in a scored cell, in label order; a record is tested when it has
two or more.  With c_ij the count of kept row i at position j and scores z:
    t_i = sum_j c_ij,   T = sum_i t_i < 2^31,   s_i = sum_j c_ij z(j),   S = sum_i s_i
    D   = sum_i t_i (s_i / t_i - S / T)^2  =  sum_i s_i^2 / t_i - S^2 / T        the gene statistic
    d_i = s_i / t_i - (S - s_i) / (T - t_i)                                      site i against the record's other reads
    n_ge      = #{p in 1..n_perm: |d_i(p)| >= |d_i(0)| - told},   told = 2^-40 qspan       (two-sided)
    gene_n_ge = #{p in 1..n_perm: D(p) >= D(0) - tolD},           tolD = 2^-40 T qspan^2
p = (1 + n_ge) / (1 + n_perm); Benjamini-Hochberg over the file's lines for the sites and over the tested records for
the genes.  pct = the scored cells with a read at the site / n; mean_score = min x + (s_i / t_i) 2^-s; delta_score =
d_i 2^-s; eta2 = D(0) / (sum_i sum_j c_ij q_j^2 - S^2 / T), empty when that is 0.  A record may own at most 4,000 kept
rows: the device's D is within (R + 8) 2^-53 T qspan^2 and d_i within 3 x 2^-53 qspan of the exact values, so
observed value, permuted value and the threshold's subtraction are together off by at most (2 R + 17) 2^-53 <= 8,017 x
2^-53 < 2^-40 of T qspan^2.

The oracle below restates this in exact arithmetic and imports nothing from scape_amd: Python ints and cross-multiplied
comparisons (t_i and T do not depend on the permutation, so D and d_i have fixed positive denominators;
test_integer_forms_against_fractions checks the integer forms against the Fractions of the definitions).  Per site and
record it gives lo, the count at the observed value, and hi, the count down to observed - 2^-39 x (qspan, or T
qspan^2): twice the device's band.  Every GPU comparison first asserts lo == hi for every site and record of its case
on the oracle alone, then that the device's or the file's counts EQUAL lo.  Nothing is excused; the seeds of this file
were chosen so that the assertion holds."""
import csv
import ctypes
import functools
import io
import math
import os
from fractions import Fraction

import numpy as np
import pytest

import report_cases as rc
from report_cases import no_gpu, run as _run  # noqa: F401  (no_gpu: fixture)

HEADER = ["gene", "pa_info", "reads", "pct", "mean_score", "delta_score", "n_ge", "p_val", "p_val_adj", "num_pa",
          "gene_reads", "eta2", "gene_n_ge", "gene_p_val", "gene_p_val_adj", "n_perm"]
BAND = 39                                 # hi counts down to the observed value - 2^-39 x (qspan, or T qspan^2)
MAX_ROWS = 4000
MAX_BUCKETS = 1 << 14                     # the largest bucket count the host of k_rep_perm_scores ever chooses


# ---------------------------------------------------------------- the contract, restated
def ranks(seed, p, n):
    """rho_p(j) for every position: the rank of key(p, j) among the n keys"""
    base = rc.mix((seed + rc.G * p) & rc.M64)
    keys = [(rc.mix((base + rc.G * (j + 1)) & rc.M64) & ~0xFFFFFF & rc.M64) | j for j in range(n)]
    rho = [0] * n
    for r, j in enumerate(sorted(range(n), key=keys.__getitem__)):
        rho[j] = r
    return rho


def permuted(seed, p, q):
    return [q[r] for r in ranks(seed, p, len(q))]


def quantise(x):
    """(q_j as Python ints, s) of scores x (floats): Python's float subtraction is the f64 one, Fraction scaling by 2^s
    is exact and round() of a Fraction rounds half to even"""
    lo, hi = min(x), max(x)
    _m, e = math.frexp(hi - lo)
    s = 15 - e
    return [round(Fraction(v - lo) * Fraction(2) ** s) for v in x], s


def rank_ints(x):
    return [sum(v < xj for v in x) + sum(v <= xj for v in x) for xj in x]


class TrendRec:
    """a record's kept rows: per row its nonzeros [(position j, count)] among the tested columns; integers only"""

    def __init__(self, gene, nzs, q, pas=None):
        self.gene, self.nzs, self.q, self.pas = gene, nzs, q, pas
        self.qspan = max(q)
        self.t = [sum(v for _j, v in nz) for nz in nzs]
        self.T = sum(self.t)
        self.P = math.lcm(*self.t)
        self.s0 = self.sums(q)
        self.ND0, self.n0 = self.stat(self.s0)
        self.lo, self.hi = 0, 0
        self.slo, self.shi = [0] * len(nzs), [0] * len(nzs)

    def sums(self, z):
        return [sum(v * z[j] for j, v in nz) for nz in self.nzs]

    def stat(self, s):
        """(ND, [n_i]): D = ND / (P T) with ND = T sum_i s_i^2 (P / t_i) - S^2 P, and d_i = n_i / (t_i (T - t_i)) with
        n_i = s_i T - S t_i; P = lcm(t_i), so both denominators are fixed and positive"""
        S = sum(s)
        ND = self.T * sum(si * si * (self.P // ti) for si, ti in zip(s, self.t)) - S * S * self.P
        return ND, [si * self.T - S * ti for si, ti in zip(s, self.t)]

    def count(self, z):
        ND, n = self.stat(self.sums(z))
        # D >= D0 - c T qspan^2 for c = 0 and c = 2^-BAND, times P T 2^BAND
        self.lo += ND >= self.ND0
        self.hi += ND << BAND >= (self.ND0 << BAND) - self.T * self.qspan ** 2 * self.P * self.T
        for i, ti in enumerate(self.t):
            self.slo[i] += abs(n[i]) >= abs(self.n0[i])
            self.shi[i] += abs(n[i]) << BAND >= (abs(self.n0[i]) << BAND) - self.qspan * ti * (self.T - ti)

    def D(self, s):
        """D as a Fraction, straight from the definition"""
        S = sum(s)
        return sum(ti * (Fraction(si, ti) - Fraction(S, self.T)) ** 2 for si, ti in zip(s, self.t))

    def d(self, s, i):
        S = sum(s)
        return Fraction(s[i], self.t[i]) - Fraction(S - s[i], self.T - self.t[i])

    def sq0(self):
        return [sum(v * self.q[j] ** 2 for j, v in nz) for nz in self.nzs]


def count_permutations(recs, seed, perms, q):
    for p in perms:
        z = permuted(seed, p, q)
        for r in recs:
            r.count(z)


def parse_scores(score_csv):
    """{id: float or None} of a score file, the last row of an id"""
    out = {}
    for i, field in rc.cluster_rows(score_csv):
        field = field.strip()
        out[i] = None if field == "" or field.lower() in ("na", "nan") else float(field)
    return out


def oracle(records, bc_csv, score_csv, rank, n_perm, seed):
    """the expected lines of the command's file, in order: dicts of the text columns, the exact counts (lo, hi) and the
    Fractions of the float columns"""
    col_ids = rc.column_ids(bc_csv)
    score = parse_scores(score_csv)
    cols = [j for j, i in enumerate(col_ids) if score.get(i) is not None]
    x = [score[col_ids[j]] for j in cols]
    assert len(cols) >= 2 and max(x) > min(x)
    if rank:
        x = [float(r) for r in rank_ints(x)]
    q, s = quantise(x)
    assert 1 << 14 <= max(q) <= 1 << 15 and min(q) == 0
    n = len(cols)
    live = []
    for rec, dense in zip(records, rc.dense_counts(records, col_ids)):
        sub = dense[:, cols]
        kept = [l for l in range(int(rec["K"])) if sub[l].any()]
        if len(kept) < 2:
            continue
        nzs = [[(j, int(v)) for j, v in enumerate(sub[l].tolist()) if v] for l in kept]
        live.append(TrendRec(rec["gene_info_str"], nzs, q, [rc.pa_info(rec, l) for l in kept]))
        assert live[-1].T < 1 << 31 and len(kept) <= MAX_ROWS
    count_permutations(live, seed, range(1, n_perm + 1), q)
    lo_x, unit = Fraction(min(x)), Fraction(2) ** -s
    lines, genes = [], []
    for r in live:
        D0 = r.D(r.s0)
        S = sum(r.s0)
        assert D0 == Fraction(r.ND0, r.P * r.T) == sum(Fraction(si * si, ti) for si, ti in zip(r.s0, r.t)) - Fraction(S * S, r.T)
        ss = sum(r.sq0()) - Fraction(S * S, r.T)
        genes.append(dict(gene=r.gene, ge=(r.lo, r.hi)))
        for i, nz in enumerate(r.nzs):
            lines.append(dict(gene=r.gene, pa=r.pas[i], reads=r.t[i], pct=Fraction(len(nz), n),
                              mean=lo_x + Fraction(r.s0[i], r.t[i]) * unit, delta=r.d(r.s0, i) * unit,
                              ge=(r.slo[i], r.shi[i]), num_pa=len(r.nzs), T=r.T, eta2=D0 / ss if ss else None,
                              gene_ge=(r.lo, r.hi), rec=len(genes) - 1, n=n))
    for ln, adj in zip(lines, rc.bh([Fraction(1 + ln["ge"][0], 1 + n_perm) for ln in lines])):
        ln["p_adj"] = adj
    gene_adj = rc.bh([Fraction(1 + g["ge"][0], 1 + n_perm) for g in genes])
    for ln in lines:
        ln["gene_adj"] = gene_adj[ln["rec"]]
    return lines


def assert_no_near_tie(lines, what):
    """lo == hi for every site and record: no permutation's statistic lies within the 2^-39 band below the observed
    one, so the device's f64 comparison (band 2^-40) can hide nothing"""
    for ln in lines:
        assert ln["ge"][0] == ln["ge"][1], (what, ln["pa"], ln["ge"])
        assert ln["gene_ge"][0] == ln["gene_ge"][1], (what, ln["gene"], ln["gene_ge"])


def compare(text, lines, n_perm, what):
    rows = list(csv.reader(io.StringIO(text)))
    assert rows[0] == HEADER, what
    body = rows[1:]
    print(what, "lines", len(body), "expected", len(lines))
    assert len(body) == len(lines), what
    for got, ln in zip(body, lines):
        ctx = (what, ln["pa"], got)
        assert len(got) == len(HEADER), ctx
        assert got[:3] == [ln["gene"], ln["pa"], str(ln["reads"])], ctx
        assert got[6] == str(ln["ge"][0]) and got[7] == repr((1 + ln["ge"][0]) / (1 + n_perm)), ctx
        assert got[9:11] == [str(ln["num_pa"]), str(ln["T"])] and got[15] == str(n_perm), ctx
        assert got[12] == str(ln["gene_ge"][0]) and got[13] == repr((1 + ln["gene_ge"][0]) / (1 + n_perm)), ctx
        if ln["eta2"] is None:
            assert got[11] == "", ctx
        floats = [(3, ln["pct"]), (4, ln["mean"]), (8, ln["p_adj"]), (14, ln["gene_adj"])]
        floats += [(11, ln["eta2"])] if ln["eta2"] is not None else []
        for col, want in floats:
            assert rc.close(got[col], want), (ctx, col, float(want))
        if ln["delta"] == 0:
            assert float(got[5]) == 0.0, ctx
        else:
            assert rc.close(got[5], ln["delta"]), (ctx, 5, float(ln["delta"]))


# ---------------------------------------------------------------- the command
def _args(root, scores, res="res.gene.pkl", rank=False, n_perm=None, seed=None):
    a = ["diff_pa_trend", "--output_dir", str(root), "--res_pkl_file", res, "--cell_score_file", str(scores)]
    a += ["--rank"] if rank else []
    for opt, v in (("--n_perm", n_perm), ("--seed", seed)):
        if v is not None:
            a += [opt, str(v)]
    return a


def _path(root, scores, res, rank=False):
    kind = res[len("res."):-len(".pkl")]
    stem = os.path.splitext(os.path.basename(str(scores)))[0]
    return os.path.join(str(root), f"{stem}.{kind}{'.rank' if rank else ''}.diff_pa_trend.csv")


def _command(root, scores, res, rank, n_perm, seed, what=""):
    r = _run(_args(root, scores, res, rank, n_perm, seed))
    assert r.exit_code == 0, (what, r.output, repr(r.exception))
    assert not rc.parts_left(root)
    with open(_path(root, scores, res, rank), newline="") as fh:
        return fh.read()


# ---------------------------------------------------------------- CPU
def test_help_and_import_path():
    r = _run(["--help"])
    assert r.exit_code == 0 and "diff_pa_trend" in r.output
    r = _run(["diff_pa_trend", "--help"])
    assert r.exit_code == 0, r.output
    for o in ("--output_dir", "--res_pkl_file", "--cell_score_file", "--rank", "--n_perm", "--seed"):
        assert o in r.output
    assert "--strata_file" not in r.output and "--idents" not in r.output
    flat = " ".join(r.output.split())
    assert "[default: 9999]" in flat and "[default: 1]" in flat
    import scape.utils as su
    from scape_amd import _lib, report
    assert su.diff_pa_trend is report.diff_pa_trend
    for name in ("scape_hip_report_perm_scores", "scape_hip_report_perm_scores_get", "scape_hip_report_perm_trend"):
        assert name in _lib.SIGNATURES
    assert report.DIFF_PA_TREND_HEADER == HEADER and report.MAX_TREND_ROWS == MAX_ROWS


def test_integer_forms_against_fractions():
    """on random small tables: the integer comparisons of TrendRec.count are the Fraction comparisons of the
    definition; sum s_i^2 / t_i - S^2 / T is the definition's D; the d_i weighted by t_i (T - t_i) / T sum to 0; and a
    permutation of the scores is a bijection of the positions"""
    rng = np.random.default_rng(6)
    for trial in range(10):
        n, R = int(rng.integers(3, 12)), int(rng.integers(2, 6))
        m = (rng.random((R, n)) < 0.6) * rng.integers(1, 5, (R, n))
        m[:, 0] |= 1
        x = [float(v) for v in rng.integers(0, 50, n)]
        x[0], x[1] = 0.0, 49.0
        if trial % 2:
            x = [v / 3 for v in x]
        q, _s = quantise(x)
        nzs = [[(j, int(v)) for j, v in enumerate(row) if v] for row in m.tolist()]
        r = TrendRec("g", nzs, q)
        assert r.D(r.s0) == Fraction(r.ND0, r.P * r.T)
        lo = hi = 0
        slo, shi = [0] * R, [0] * R
        n_perm = 40
        for p in range(1, n_perm + 1):
            rho = ranks(trial, p, n)
            assert sorted(rho) == list(range(n))
            z = [q[k] for k in rho]
            r.count(z)
            s = r.sums(z)
            assert sum(s) == sum(v * z[j] for nz in nzs for j, v in nz)
            assert r.D(s) == sum(Fraction(si * si, ti) for si, ti in zip(s, r.t)) - Fraction(sum(s) ** 2, r.T)
            assert sum(r.d(s, i) * r.t[i] * (r.T - r.t[i]) for i in range(R)) == 0
            lo += r.D(s) >= r.D(r.s0)
            hi += r.D(s) >= r.D(r.s0) - Fraction(r.T * r.qspan ** 2, 1 << BAND)
            for i in range(R):
                slo[i] += abs(r.d(s, i)) >= abs(r.d(r.s0, i))
                shi[i] += abs(r.d(s, i)) >= abs(r.d(r.s0, i)) - Fraction(r.qspan, 1 << BAND)
        assert (r.lo, r.hi, r.slo, r.shi) == (lo, hi, slo, shi)
        assert 0 < lo <= n_perm


SCORE_SETS = {
    "integers": [3.0, 0.0, 100.0, 41.0, 41.0, 7.0],
    "two": [5.0, 6.0],
    "negative": [-2.5, 4.0, -0.125, 0.0],
    "span-a-power-of-two": [1024.0, 0.0, 512.0, 1.0],
    "tenths": [0.1, 0.3, 0.7, 0.7, 1.9],
    "pseudotime": [0.0, 1 / 3, 0.5, 2 / 3, 1.0],
    "tiny": [1e-300, 3e-300, 2.5e-300],
    "wide-integers": [0.0, 70000.0, 35001.0, 3.0],
    "halves-to-even": [0.0, float(1 << 15), 0.5, 1.5, 2.5],
}


@pytest.mark.parametrize("x", list(SCORE_SETS.values()), ids=list(SCORE_SETS))
def test_quantisation_rule(x):
    """q_j of the host equal the restated rule's; qspan lies in 2^14 .. 2^15 and min q = 0; a score that is a multiple
    of 2^-s is exact (integer scores whose span is below 2^15 are), any other is off by at most half a unit; rint rounds
    half to even"""
    from scape_amd import report
    q, s = quantise(x)
    got, got_s = report._quantise_scores(np.array(x, dtype=np.float64))
    assert got.dtype == np.uint16 and got.tolist() == q and got_s == s
    assert min(q) == 0 and 1 << 14 <= max(q) <= 1 << 15
    unit = Fraction(2) ** -s
    for v, qi in zip(x, q):
        w = Fraction(v - min(x))
        assert abs(qi * unit - w) <= unit / 2
        if (w / unit).denominator == 1:
            assert qi * unit == w
    exact = all((Fraction(v - min(x)) / unit).denominator == 1 for v in x)
    assert exact == (x not in (SCORE_SETS[k] for k in ("tenths", "pseudotime", "tiny", "wide-integers", "halves-to-even")))
    if x is SCORE_SETS["integers"]:
        assert s == 8 and q == [768, 0, 25600, 10496, 10496, 1792]
    if x is SCORE_SETS["halves-to-even"]:
        assert s == -1 and q == [0, 1 << 14, 0, 1, 1]               # 0.25 -> 0, 0.75 -> 1, 1.25 -> 1
    if x is SCORE_SETS["span-a-power-of-two"]:
        assert max(q) == 1 << 14                                    # frexp(2^k) = (0.5, k + 1)


def test_rank_integers_on_ties():
    """r_j = #{x < x_j} + #{x <= x_j}: twice the mid-rank minus one, ties share it, and the transform of a rank
    vector is itself"""
    from scape_amd import report
    x = [0.5, 0.1, 0.5, 2.0, 0.5, 0.1, 9.0]
    assert rank_ints(x) == [7, 2, 7, 11, 7, 2, 13]                   # mid-ranks 4, 1.5, 4, 6, 4, 1.5, 7
    got = report._rank_scores(np.array(x))
    assert got.dtype == np.float64 and got.tolist() == [float(r) for r in rank_ints(x)]
    assert report._rank_scores(got).tolist() == got.tolist()
    assert rank_ints([3.0, 1.0, 2.0]) == [5, 1, 3]


def _small_dir(tmp_path):
    (tmp_path / "res.gene.pkl").write_bytes(b"")
    (tmp_path / "barcode_index.csv").write_text("CB,index\nA-1,3\nB-1,4\nC-1,5\nD-1,6\n")
    return tmp_path / "pt.csv"


def test_prerequisites_and_argument_errors(tmp_path, no_gpu):
    """every error of the score file and of the arguments is raised before the device is opened, and leaves no file"""
    sc = tmp_path / "pt.csv"
    r = _run(_args(tmp_path / "nope", sc))
    assert r.exit_code != 0 and "Given output_dir folder does not exists." in str(r.exception)
    r = _run(_args(tmp_path, sc))
    assert "Given res_pkl_file is not in output_dir." in str(r.exception)
    sc = _small_dir(tmp_path)
    r = _run(_args(tmp_path, sc))
    assert "Given cell_score_file file does not exists" in str(r.exception)
    for body, word in (("3,0.5\n4,inf\n5,1\n", "row 2"), ("3,0.5\n4,1\n5,-Infinity\n", "row 3"),
                       ("3,0.5\n4,1.0\n5,late\n", "row 3"), ("3,0.5\n4,1.5\n6,0x10\n", "row 3"),
                       ("3,0.5\n4,NA\n5,\n6,nan\n", "1 cells"), ("77,0.5\n78,1.5\n", "0 cells"),
                       ("3,NaN\n4,na\n5,\n", "0 cells"), ("3,0.5\n4,0.50\n5,5e-1\n6,NA\n", "has the score"),
                       ("3,1\n3,NA\n4,2\n", "1 cells")):
        sc.write_text("index,pseudotime\n" + body)
        r = _run(_args(tmp_path, sc))
        assert isinstance(r.exception, ValueError) and word in str(r.exception), (body, repr(r.exception))
    sc.write_text("index\n3\n4\n")
    r = _run(_args(tmp_path, sc))
    assert isinstance(r.exception, ValueError), repr(r.exception)
    sc.write_text("index,pseudotime\n3,0.5\n4,1.5\n")
    for extra, word in ((["--n_perm", "0"], "n_perm"), (["--n_perm", str(1 << 31)], "n_perm"),
                        (["--seed", "-1"], "seed"), (["--seed", str(1 << 64)], "seed")):
        r = _run(_args(tmp_path, sc) + extra)
        assert isinstance(r.exception, ValueError) and word in str(r.exception), (extra, repr(r.exception))
    r = _run(["diff_pa_trend", "--output_dir", str(tmp_path), "--res_pkl_file", "res.gene.pkl"])
    assert r.exit_code == 2 and "--cell_score_file" in r.output
    r = _run(_args(tmp_path, sc) + ["--idents", "A"])
    assert r.exit_code == 2
    assert sorted(os.listdir(tmp_path)) == ["barcode_index.csv", "pt.csv", "res.gene.pkl"]


def test_too_many_cells_is_refused_before_the_device(tmp_path, no_gpu, monkeypatch):
    from scape_amd import report
    sc = _small_dir(tmp_path)
    sc.write_text("index,pseudotime\n3,0.5\n4,1.5\n5,2\n")
    monkeypatch.setattr(report, "MAX_PERM_CELLS", 3)
    r = _run(_args(tmp_path, sc))
    assert isinstance(r.exception, ValueError) and "3 tested cells" in str(r.exception), repr(r.exception)
    assert report.MAX_PERM_CELLS == 3 and 1 << 24 == 16777216


def test_max_perm_cells_is_two_to_the_24():
    from scape_amd import report
    assert report.MAX_PERM_CELLS == 1 << 24


# ---------------------------------------------------------------- GPU: the ranks
def np_ranks(seed, p, n):
    """ranks() in numpy (uint64 arithmetic wraps mod 2^64); test_np_ranks_are_the_restated_ones holds it to ranks()"""
    u = np.uint64

    def mix(z):
        z = (z ^ (z >> u(30))) * u(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> u(27))) * u(0x94D049BB133111EB)
        return z ^ (z >> u(31))
    with np.errstate(over="ignore"):
        j = np.arange(n, dtype=np.uint64)
        base = u(rc.mix((seed + rc.G * p) & rc.M64))
        keys = (mix(base + u(rc.G) * (j + u(1))) & ~u(0xFFFFFF)) | j
    rho = np.empty(n, dtype=np.int64)
    rho[np.argsort(keys, kind="stable")] = np.arange(n)
    return rho


def test_np_ranks_are_the_restated_ones():
    for seed, p, n in ((77, 1, 2), (77, 300, 161), (5, 123456789012, 700), ((1 << 64) - 1, 3, 65)):
        assert np_ranks(seed, p, n).tolist() == ranks(seed, p, n)
        keys = [rc.key(seed, p, j) for j in range(n)]
        assert ranks(seed, p, n) == [sum(k < kj for k in keys) for kj in keys]


def _scores_call(ctx, q, p_first, p_count, seed):
    from scape_amd._lib import P_u16, ptr
    q = np.ascontiguousarray(q, dtype=np.uint16)
    return ctx.lib.scape_hip_report_perm_scores(ctx.h, len(q), ptr(q, P_u16), p_first, p_count, seed)


def _scores_get(ctx, p, n):
    from scape_amd._lib import P_u16, check, ptr
    out = np.full(n, 0xFFFF, dtype=np.uint16)
    check(ctx.lib.scape_hip_report_perm_scores_get(ctx.h, p, ptr(out, P_u16)), "perm_scores_get")
    return out


RANK_SEED = 21


@pytest.mark.gpu
@pytest.mark.parametrize("n", [2, 3, 64, 65, 161, 257, 5000, 40000, 2 * MAX_BUCKETS + 1])
def test_ranks_of_every_key(n):
    """scape_hip_report_perm_scores against q[rank of key] from sorted keys, q a scramble of distinct values so that
    every rank is pinned (beyond 32,769 positions a scramble of 0 .. n - 1 goes through in two halfword digits).  Small
    n: bucket populations of 0 and 1 and, at n = 2, 3, of nothing else; 5,000: the bucket table is larger than n; 40,000
    and 2 B + 1: more positions than buckets, populations of many.  Every permutation of 300 for n <= 5,000, the first,
    the last and those around the tile edge of 256 beyond"""
    from scape_amd import _lib
    from scape_amd._lib import check as chk
    rng = np.random.default_rng(n)
    scramble = rng.permutation(n)
    digits = [scramble] if n <= (1 << 15) + 1 else [scramble & 0x7FFF, scramble >> 15]
    perms = range(1, 301) if n <= 5000 else (1, 2, 256, 257, 300)
    want = {p: np_ranks(RANK_SEED, p, n) for p in perms}
    ctx = _lib.default_context(None)
    try:
        for q in digits:
            assert q.max() <= 1 << 15
            chk(_scores_call(ctx, q, 1, 300, RANK_SEED), "perm_scores")
            bad = [p for p in perms if not np.array_equal(_scores_get(ctx, p - 1, n), q[want[p]])]
            print(n, "permutations that differ", bad[:5])
            assert not bad
    finally:
        ctx.lib.scape_hip_report_free(ctx.h)


@pytest.mark.gpu
@pytest.mark.parametrize("sizes", [(70, 91), (5, 1, 30, 125)])
def test_scores_generalise_the_group_labels(sizes):
    """with q = the observed group index, the scores of every permutation are the bytes of scape_hip_report_perm_labels"""
    from scape_amd import _lib
    from scape_amd._lib import P_i32, check as chk, ptr
    n = sum(sizes)
    q = np.repeat(np.arange(len(sizes)), sizes)
    sz = np.array(sizes, dtype=np.int32)
    ctx = _lib.default_context(None)
    try:
        chk(_scores_call(ctx, q, 1, 300, 77), "perm_scores")
        chk(ctx.lib.scape_hip_report_perm_labels(ctx.h, len(sizes), ptr(sz, P_i32), 1, 300, 77), "perm_labels")
        lab = np.zeros(n, dtype=np.uint8)
        for p in range(300):
            chk(ctx.lib.scape_hip_report_perm_labels_get(ctx.h, p, ptr(lab, ctypes.POINTER(ctypes.c_uint8))), "labels_get")
            assert np.array_equal(_scores_get(ctx, p, n), lab), p
    finally:
        ctx.lib.scape_hip_report_free(ctx.h)


# ---------------------------------------------------------------- GPU: the statistic
EP_Q_SEED = 3


@functools.lru_cache(maxsize=None)
def entry_case():
    """rc.entry_point_matrix() (records of 2, 5, 70 and 150 rows, 161 tested columns, seed 77, 300 permutations) under
    quantised random scores with ties, and its oracle counted once"""
    n1, n2, n_cols, seed, n_perm, Ks, off, lab, cb, dense, rows, roff, _rng = rc.entry_point_matrix()
    n = n1 + n2
    x = [float(v) for v in np.random.default_rng(EP_Q_SEED).integers(0, 60, n)]
    x[0], x[1] = 0.0, 59.0
    q, _s = quantise(x)
    recs = []
    for r in range(len(Ks)):
        nzs = [[(j, int(v)) for j, v in enumerate(dense[i, :n].tolist()) if v] for i in rows[roff[r]:roff[r + 1]]]
        recs.append(TrendRec(f"rec{r}", nzs, q))
    count_permutations(recs, seed, range(1, n_perm + 1), q)
    return q, recs


def _trend_outs(n_rows, n_rec):
    return dict(t=np.full(n_rows, -1, np.int64), s0=np.full(n_rows, -1, np.int64), sq0=np.full(n_rows, -1, np.int64),
                site=np.zeros(n_rows, np.int64), d0=np.full(n_rows, -1.0), stat0=np.full(n_rec, -1.0),
                gene=np.zeros(n_rec, np.int64))


def _trend_call(ctx, roff, rows, o):
    from scape_amd._lib import P_d, P_i64, ptr
    return ctx.lib.scape_hip_report_perm_trend(ctx.h, len(roff) - 1, ptr(roff, P_i64), ptr(rows, P_i64), ptr(o["t"], P_i64),
                                               ptr(o["s0"], P_i64), ptr(o["sq0"], P_i64), ptr(o["site"], P_i64),
                                               ptr(o["d0"], P_d), ptr(o["stat0"], P_d), ptr(o["gene"], P_i64))


def test_entry_case_has_no_near_tie():
    """the oracle alone, without a GPU: lo == hi for every site and record of the entry point's case"""
    _q, recs = entry_case()
    for r in recs:
        assert r.lo == r.hi and r.slo == r.shi, (r.gene, r.lo, r.hi)
    assert 0 < max(r.lo for r in recs) and min(min(r.slo) for r in recs) < 300


@pytest.mark.gpu
def test_entry_point_and_chunk_independence():
    """scape_hip_report_perm_trend on the hand-made matrix: t, s0 and sq0 equal the oracle's integers, D(0) and d_i(0)
    lie within (R + 8) 2^-53 T qspan^2 and 3 x 2^-53 qspan of the exact values, and every counter equals lo (lo == hi
    asserted first), in one call of 300 permutations and added up over the chunks 1..100 and 101..300, whose scores are
    those of the one call"""
    from scape_amd import _lib
    from scape_amd._lib import check as chk
    n1, n2, n_cols, seed, n_perm, Ks, off, lab, cb, dense, rows, roff, _rng = rc.entry_point_matrix()
    n = n1 + n2
    q, recs = entry_case()
    for r in recs:
        assert r.lo == r.hi and r.slo == r.shi, (r.gene, r.lo, r.hi)
    ctx = _lib.default_context(None)
    try:
        assert np.array_equal(rc.device_counts(ctx, Ks, off, lab, cb, n_cols), dense.sum(axis=1))
        chk(_scores_call(ctx, q, 1, n_perm, seed), "perm_scores")
        whole = [_scores_get(ctx, p, n) for p in range(n_perm)]
        one = _trend_outs(len(rows), len(Ks))
        chk(_trend_call(ctx, roff, rows, one), "perm_trend")
        parts = _trend_outs(len(rows), len(Ks))
        for p_first, p_count in ((1, 100), (101, 200)):
            chk(_scores_call(ctx, q, p_first, p_count, seed), "perm_scores")
            for p in range(p_count):
                assert np.array_equal(_scores_get(ctx, p, n), whole[p_first - 1 + p]), (p_first, p)
            chk(_trend_call(ctx, roff, rows, parts), "perm_trend")
    finally:
        ctx.lib.scape_hip_report_free(ctx.h)
    want = dict(t=[ti for r in recs for ti in r.t], s0=[s for r in recs for s in r.s0],
                sq0=[s for r in recs for s in r.sq0()], site=[c for r in recs for c in r.slo], gene=[r.lo for r in recs])
    for o, how in ((one, "one call"), (parts, "two chunks")):
        for name, w in want.items():
            print(how, name, "equal", o[name].tolist() == w, o[name].tolist()[:4], w[:4])
            assert o[name].tolist() == w, (how, name)
    assert one["stat0"].tolist() == parts["stat0"].tolist() and one["d0"].tolist() == parts["d0"].tolist()
    u = Fraction(1, 1 << 53)
    k = 0
    for g, r in enumerate(recs):
        err = abs(Fraction(float(one["stat0"][g])) - r.D(r.s0))
        print("D0", g, float(one["stat0"][g]), "error / (u T qspan^2)", float(err / (u * r.T * r.qspan ** 2)))
        assert err <= (len(r.nzs) + 8) * u * r.T * r.qspan ** 2, (g, float(err))
        for i in range(len(r.nzs)):
            assert abs(Fraction(float(one["d0"][k])) - r.d(r.s0, i)) <= 3 * u * r.qspan, (g, i)
            k += 1


@pytest.mark.gpu
def test_entry_point_refusals():
    """scores not built, a score above 32,768, n below 2, p_first below 1 and a record of more than 4,000 rows: non-zero,
    a message, nothing written and nothing added, before anything is queued"""
    from scape_amd import _lib
    from scape_amd._lib import check as chk
    n1, n2, n_cols, seed, n_perm, Ks, off, lab, cb, dense, rows, roff, _rng = rc.entry_point_matrix()
    q, _recs = entry_case()
    ctx = _lib.default_context(None)
    o = _trend_outs(len(rows), len(Ks))
    try:
        assert _trend_call(ctx, roff, rows, o) != 0 and "report_counts" in _lib.last_error()
        rc.device_counts(ctx, Ks, off, lab, cb, n_cols)
        assert _trend_call(ctx, roff, rows, o) != 0 and "perm_scores" in _lib.last_error()
        assert _scores_call(ctx, q[:3] + [(1 << 15) + 1], 1, 10, seed) != 0 and "32,768" in _lib.last_error()
        assert _scores_call(ctx, q[:1], 1, 10, seed) != 0 and "2" in _lib.last_error()
        assert _scores_call(ctx, q, 0, 10, seed) != 0 and "p_first" in _lib.last_error()
        assert _scores_call(ctx, q, 1, 0, seed) != 0 and "p_count" in _lib.last_error()
        assert _trend_call(ctx, roff, rows, o) != 0 and "perm_scores" in _lib.last_error()     # still none
        chk(_scores_call(ctx, q, 1, 10, seed), "perm_scores")
        many = np.concatenate([rows[:2], np.resize(rows, MAX_ROWS + 1)]).astype(np.int64)
        om = _trend_outs(len(many), 2)
        assert _trend_call(ctx, np.array([0, 2, len(many)], np.int64), many, om) != 0
        assert "record 1" in _lib.last_error() and "4000" in _lib.last_error()
        wide = np.ascontiguousarray(np.resize(q, n_cols + 1), dtype=np.uint16)
        chk(_scores_call(ctx, wide, 1, 10, seed), "perm_scores")
        assert _trend_call(ctx, roff, rows, o) != 0 and "fewer columns" in _lib.last_error()
        for a in (o, om):
            assert all(np.all(a[k] == -1) for k in ("t", "s0", "sq0", "d0", "stat0")) and not a["site"].any() \
                and not a["gene"].any()
        chk(_scores_call(ctx, q, 1, 10, seed), "perm_scores")
        ok = np.resize(rows, MAX_ROWS).astype(np.int64)                       # the cap itself passes
        oc = _trend_outs(len(ok), 1)
        chk(_trend_call(ctx, np.array([0, len(ok)], np.int64), ok, oc), "perm_trend")
        assert np.all(oc["t"] >= 0) and 0 <= oc["gene"][0] <= 10
    finally:
        ctx.lib.scape_hip_report_free(ctx.h)


# ---------------------------------------------------------------- GPU: the command
SYN_N_PERM, SYN_SCORE_SEED = 199, 4


@functools.lru_cache(maxsize=None)
def _syn_scores(ranked=False):
    """a score file for rc.synthetic(): cluster A's cells get the low scores (records 0..3 have a planted excess of
    their first site in A: a planted trend), some cells NA, an empty field or nan, rows in the cluster file's scrambled
    order, and two rows that share an id (the last counts).  ranked: the scores are replaced by their own rank
    transform (rounded to a tenth first, so that there are ties), a file that --rank leaves as it is"""
    _records, _bc, clu_text = rc.synthetic()
    rng = np.random.default_rng(SYN_SCORE_SEED)
    rows = []
    for k, (i, clu) in enumerate(rc.cluster_rows(clu_text)):
        v = rng.random() if clu == "A" else 1.0 + 2.0 * rng.random()
        field = f"{v:.4f}"
        if clu == "" or k % 23 == 5:
            field = ("NA", "", "nan", "NaN")[k % 4]
        rows.append([i, field])
    first_scored = next(k for k, (_i, f) in enumerate(rows) if f not in ("NA", "", "nan", "NaN"))
    rows.append([rows[first_scored][0], "2.7500"])                        # the id's last row counts
    rows.append([rows[first_scored + 1][0], "NA"])                        # and this cell ends without a score
    if ranked:
        last = {i: f for i, f in rows}
        ids = [i for i, f in last.items() if f not in ("NA", "", "nan", "NaN")]
        r = rank_ints([round(float(last[i]), 1) for i in ids])
        rank_of = dict(zip(ids, r))
        rows = [[i, str(rank_of[i])] for i in ids] + [[i, "NA"] for i in last if i not in rank_of]
    return "index,pseudotime\n" + "".join(f"{i},{f}\n" for i, f in rows)


@functools.lru_cache(maxsize=None)
def _syn_lines(ranked, rank, n_perm=SYN_N_PERM, seed=1):
    records, bc, _clu = rc.synthetic()
    return oracle(records, bc, _syn_scores(ranked), rank, n_perm, seed)


def _write_syn(root, ranked):
    from scape.apa_core import Parameters
    records, bc, _clu = rc.synthetic()
    return rc.write_dir(str(root), "res.gene.pkl", records, bc, {"pt.csv": _syn_scores(ranked)}, Parameters)[0]


def test_synthetic_case_has_no_near_tie_and_a_planted_trend():
    """the oracle alone, without a GPU: lo == hi everywhere, for the scores and for the rank file with and without
    --rank (the same lines: the file is its own rank transform); the planted records' gene count is 0; record 6 (K = 1)
    has no line, record 5 (reads only in A) has"""
    lines = _syn_lines(False, False)
    assert_no_near_tie(lines, "syn")
    by = {}
    for ln in lines:
        by.setdefault(ln["gene"].split(":")[1], []).append(ln)
    assert "GENE6" not in by and "GENE5" in by and len(by) >= 30
    for g in ("GENE0", "GENE1", "GENE2", "GENE3"):
        assert by[g][0]["gene_ge"][0] == 0 and by[g][0]["ge"][0] == 0 and by[g][0]["delta"] < 0, g
    assert max(ln["num_pa"] for ln in lines) == 63
    ranked = _syn_lines(True, True)
    assert_no_near_tie(ranked, "syn/rank")
    plain = _syn_lines(True, False)
    assert [(ln["ge"], ln["gene_ge"], ln["mean"], ln["delta"]) for ln in ranked] == \
        [(ln["ge"], ln["gene_ge"], ln["mean"], ln["delta"]) for ln in plain]
    text = _syn_scores()
    assert ",NA\n" in text and ",\n" in text and ",nan\n" in text
    ids = [i for i, _f in rc.cluster_rows(text)]
    assert len(ids) == len(set(ids)) + 2


@pytest.mark.gpu
@pytest.mark.parametrize("ranked", [False, True], ids=["scores", "rank"])
def test_synthetic_directory(tmp_path, monkeypatch, ranked):
    """199 permutations of the scored cells of the synthetic directory: every column of the file against the exact
    oracle (lo == hi asserted first), the planted records' gene p-value is 1 / 200 and record 6 (K = 1) is absent; the
    same bytes come back with the permutations in several chunks and the records in several batches; no .part file is
    left.  rank: the same with --rank on a score file that is its own rank transform, whose file without --rank differs
    in its name only"""
    from scape_amd import _lib, report
    lines = _syn_lines(ranked, ranked)
    assert_no_near_tie(lines, "syn")
    path = _write_syn(tmp_path, ranked)
    text = _command(tmp_path, path, "res.gene.pkl", ranked, SYN_N_PERM, 1, "syn")
    compare(text, lines, SYN_N_PERM, "syn")
    rows = list(csv.reader(io.StringIO(text)))[1:]
    genes = {r[0].split(":")[1]: r for r in rows}
    assert "GENE6" not in genes
    for g in ("GENE0", "GENE1", "GENE2", "GENE3"):
        assert genes[g][13] == repr(1 / 200), g
    assert os.path.basename(_path(tmp_path, path, "res.gene.pkl", ranked)) == \
        ("pt.gene.rank.diff_pa_trend.csv" if ranked else "pt.gene.diff_pa_trend.csv")
    if ranked:
        assert _command(tmp_path, path, "res.gene.pkl", False, SYN_N_PERM, 1, "syn/plain") == text
    lib = _lib.load_library()
    calls = {"scores": [], "test": 0}
    real_s, real_t = lib.scape_hip_report_perm_scores, lib.scape_hip_report_perm_trend

    def make_scores(*a):
        calls["scores"].append((a[3], a[4]))
        return real_s(*a)

    def test(*a):
        calls["test"] += 1
        return real_t(*a)
    monkeypatch.setattr(lib, "scape_hip_report_perm_scores", make_scores)
    monkeypatch.setattr(lib, "scape_hip_report_perm_trend", test)
    n = lines[0]["n"]
    monkeypatch.setattr(report, "MAX_BATCH_BYTES", 1 << 16)             # a record of K = 8 alone takes 57 KB
    monkeypatch.setattr(report, "MAX_PERM_BYTES", 6 * n * 80)           # 6 bytes per tested cell: 80 permutations
    assert _command(tmp_path, path, "res.gene.pkl", ranked, SYN_N_PERM, 1, "syn/chunks") == text
    assert calls["scores"][:3] == [(1, 80), (81, 80), (161, 39)] and calls["test"] > 3 * 5
    assert calls["test"] == len(calls["scores"]) and not rc.parts_left(tmp_path)
