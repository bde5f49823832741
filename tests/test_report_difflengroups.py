"""`scape diff_pa_len_groups`: the permutation test of a record's mean pA position (3'UTR length) across G = 2..64 cell
populations, and of every population against all the others (scape_amd/report.py, section diff_pa_len_groups; kernels
k_rep_len_groups_obs and k_rep_perm_len_groups and entry point scape_hip_report_perm_len_groups of
scape_amd/csrc/perm.inc).

The contract.  Options, populations, tested columns (population 0's, then population 1's, ...), permutations (the
key(p, j) of diff_pa ranked per permutation: the n_0 smallest keys form group 0, the next n_1 group 1, ...) and output
naming are `diff_pa_groups`'s: tests/test_report_diffgroups.py states them and its `labels` is used here.  Kept rows
(labels < K with a read in a tested column, in label order) and their positions x_i = alpha_arr[label_i] are
`diff_pa_len`'s; a non-finite position of a kept row of any record with K >= 2 is a ValueError naming the record, K = 1
records are never looked at.  A record is tested when it has two kept rows or more, two populations or more with reads,
and span = max x - min x > 0.

Integer positions, per record:  w_i = fl(x_i - min x),  frexp(span) = (m, e),  s = 22 - e,  q_i = rint(ldexp(w_i, s)),
half to even; so 2^21 <= qspan = max q_i <= 2^22.  A position that is a multiple of 2^-s (integers: the theta grid) is
exact, anything else is rounded at about span 2^-22.  The p-values are those of the test on the q_i; the position
columns of the file come from the exact x_i.

With a_ig the sum of kept row i over group g under a labelling:
    A_g = sum_i a_ig,   T = sum_g A_g < 2^31,   Q_g = sum_i a_ig q_i <= 2^53,   Q = sum_g Q_g     (Q, T: the record's)
    D   = sum_{g: A_g > 0} A_g (Q_g / A_g - Q / T)^2  =  sum Q_g^2 / A_g - Q^2 / T       the omnibus statistic
    d_g = Q_g / A_g - (Q - Q_g) / (T - A_g),  0 when A_g = 0 or A_g = T                  group g against all the others
    n_ge     = #{p in 1..n_perm: D(p) >= D(0) - tolD},           tolD = 2^-40 T qspan^2
    n_ge.<g> = #{p in 1..n_perm: |d_g(p)| >= |d_g(0)| - told},   told = 2^-40 qspan      (two-sided)
n_ge.<g> is reported for the groups whose observed A_g is neither 0 nor T; the others get empty fields.  For G = 2,
D = (A_0 A_1 / T) d_0^2 and |d_0| = |d_1| = 2^s |delta| of `diff_pa_len`.  p = (1 + n_ge) / (1 + n_perm); the omnibus
p-values get Benjamini-Hochberg over the file's lines, the per-group ones once over all reported (record, group) pairs
of the file.  eta2 = D / sum_i t_i (q_i - Q / T)^2; top_group = the reported group with the largest |d_g(0)|, the first
on ties; mean_pos, mean_pos.<g>, delta_pos.<g> (mean_pos.<g> minus the mean position of all other groups' reads) and
top_delta_pos are in nucleotides, from the exact x_i.

The oracle below restates this in exact arithmetic and imports nothing from scape_amd: Python ints for q_i, A_g and
Q_g, and cross-multiplied integer comparisons (test_integer_form_and_two_group_identities checks them against the
Fractions of the definition).  Per record and statistic it gives lo, the count at the observed value, and hi, the count
down to observed - 2^-39 x (T qspan^2, or qspan): twice the device's band.  Every GPU test first asserts lo == hi for
every record and group of its case on the oracle alone, then that the device's or the file's counts EQUAL lo.  No
record is excused; the seeds of this file were chosen so that the assertion holds.  The device's rounding stays below
(2 G + 17) 2^-53 T qspan^2 and 7 x 2^-53 qspan (include/scape_hip.h), far inside the 2^-40 bands, for any number of rows."""
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
from test_report_diffgroups import labels, observed, populations_all

HEADER = ["gene", "num_pa", "num_groups", "reads", "mean_pos", "eta2", "n_ge", "p_val", "p_val_adj", "top_group",
          "top_delta_pos", "n_perm"]
PER_GROUP = ["reads", "mean_pos", "delta_pos", "n_ge", "p_val", "p_val_adj"]
BAND = 39                                 # hi counts down to the observed value - 2^-39 x (T qspan^2, or qspan)


# ---------------------------------------------------------------- the contract, restated
def quantise(x):
    """(q_i as Python ints, s) of positions x (floats): Python's float subtraction is the f64 one, Fraction scaling by
    2^s is exact and round() of a Fraction rounds half to even"""
    lo, hi = min(x), max(x)
    _m, e = math.frexp(hi - lo)
    s = 22 - e
    return [round(Fraction(v - lo) * Fraction(2) ** s) for v in x], s


class LenGroupsRec:
    """a record's kept rows: per row its nonzeros [(position j, count)] among the tested columns and its pA position x
    (float); integers and Fractions only"""

    def __init__(self, gene, nzs, x, sizes):
        self.gene, self.nzs, self.G = gene, nzs, len(sizes)
        self.xf = [float(v) for v in x]
        self.x = [Fraction(v) for v in self.xf]
        self.t = [sum(v for _j, v in nz) for nz in nzs]
        self.T = sum(self.t)
        self.span = max(self.x) - min(self.x)
        if self.span > 0:
            self.q, self.s = quantise(self.xf)
            self.qspan = max(self.q)
            self.Q = sum(ti * qi for ti, qi in zip(self.t, self.q))
        self.a0 = self.row_sums(observed(sizes))
        self.lo, self.hi = 0, 0
        self.glo, self.ghi = [0] * self.G, [0] * self.G

    def row_sums(self, lab):
        out = []
        for nz in self.nzs:
            a = [0] * self.G
            for j, v in nz:
                a[lab[j]] += v
            out.append(a)
        return out

    def A(self, a):
        return [sum(row[g] for row in a) for g in range(self.G)]

    def tested(self):
        return len(self.nzs) >= 2 and sum(Ag > 0 for Ag in self.A(self.a0)) >= 2 and self.span > 0

    def start(self):
        self.E0, self.N0, self.M0 = self.stat(self.a0)

    def stat(self, a):
        """((E, P), [N_g], [M_g]) with sum_g Q_g^2 / A_g = E / P (P = the product of the A_g > 0; D = E / P - Q^2 / T,
        and Q^2 / T is the record's) and d_g = N_g / M_g, N_g = Q_g T - Q A_g, M_g = A_g (T - A_g), or (0, 1)"""
        A = self.A(a)
        Qg = [sum(row[g] * qi for row, qi in zip(a, self.q)) for g in range(self.G)]
        assert sum(A) == self.T and sum(Qg) == self.Q
        P = math.prod(Ag for Ag in A if Ag > 0)
        E = sum(Qg[g] * Qg[g] * (P // A[g]) for g in range(self.G) if A[g] > 0)
        N = [Qg[g] * self.T - self.Q * A[g] if 0 < A[g] < self.T else 0 for g in range(self.G)]
        M = [A[g] * (self.T - A[g]) if 0 < A[g] < self.T else 1 for g in range(self.G)]
        return (E, P), N, M

    def count(self, lab):
        (E, P), N, M = self.stat(self.row_sums(lab))
        E0, P0 = self.E0
        # E / P >= E0 / P0 - c T qspan^2 for c = 0 and c = 2^-BAND, times P P0 2^BAND (positive)
        self.lo += E * P0 >= E0 * P
        self.hi += (E * P0) << BAND >= ((E0 << BAND) - self.T * self.qspan ** 2 * P0) * P
        for g in range(self.G):
            # |N| / M >= |N0| / M0 - c qspan, times M M0 2^BAND (positive)
            self.glo[g] += abs(N[g]) * self.M0[g] >= abs(self.N0[g]) * M[g]
            self.ghi[g] += (abs(N[g]) * self.M0[g]) << BAND >= ((abs(self.N0[g]) << BAND) - self.qspan * self.M0[g]) * M[g]

    def D(self, a):
        """D as a Fraction, straight from the definition"""
        A = self.A(a)
        Qg = [sum(row[g] * qi for row, qi in zip(a, self.q)) for g in range(self.G)]
        return sum(A[g] * (Fraction(Qg[g], A[g]) - Fraction(self.Q, self.T)) ** 2 for g in range(self.G) if A[g] > 0)

    def d(self, a, g):
        A = self.A(a)[g]
        if A == 0 or A == self.T:
            return Fraction(0)
        Qg = sum(row[g] * qi for row, qi in zip(a, self.q))
        return Fraction(Qg, A) - Fraction(self.Q - Qg, self.T - A)

    def reported(self):
        return [0 < Ag < self.T for Ag in self.A(self.a0)]

    def positions(self):
        """(mean_pos, [mean_pos.<g> or None], [delta_pos.<g> or None]) in nucleotides, from the exact x_i"""
        A = self.A(self.a0)
        S = [sum(row[g] * xi for row, xi in zip(self.a0, self.x)) for g in range(self.G)]
        mean = [S[g] / A[g] if A[g] else None for g in range(self.G)]
        delta = [S[g] / A[g] - (sum(S) - S[g]) / (self.T - A[g]) if 0 < A[g] < self.T else None for g in range(self.G)]
        return sum(S) / self.T, mean, delta


def count_permutations(recs, sizes, seed, perms):
    for r in recs:
        r.start()
    for p in perms:
        lab = labels(seed, p, sizes)
        for r in recs:
            r.count(lab)


def oracle(recs, pop_cols, names, n_perm, seed):
    """recs: [dict(gene, K, alpha, dense = counts [K, every matrix column])] in file order; pop_cols: the matrix columns
    of every population, ascending.  Returns the expected lines: dicts of the text columns, the exact counts (lo, hi) and
    the Fractions of the float columns"""
    sizes = [len(c) for c in pop_cols]
    cols = np.array([j for c in pop_cols for j in c], dtype=np.int64)
    assert 2 <= len(sizes) <= 64 and min(sizes) >= 1 and len(cols) < 1 << 24
    live = []
    for rec in recs:
        K = int(rec["K"])
        sub = np.asarray(rec["dense"])[:, cols]
        kept = [l for l in range(K) if sub[l].any()]
        if K == 1 or len(kept) < 2:
            continue
        nzs = [[(j, int(v)) for j, v in enumerate(sub[l].tolist()) if v] for l in kept]
        r = LenGroupsRec(rec["gene"], nzs, [float(rec["alpha"][l]) for l in kept], sizes)
        if r.tested():
            assert r.T < 1 << 31 and 1 << 21 <= r.qspan <= 1 << 22
            live.append(r)
    count_permutations(live, sizes, seed, range(1, n_perm + 1))
    lines = []
    for r in live:
        A, rep = r.A(r.a0), r.reported()
        D0 = r.D(r.a0)
        assert D0 == Fraction(r.E0[0], r.E0[1]) - Fraction(r.Q * r.Q, r.T)
        d0 = [abs(r.d(r.a0, g)) for g in range(r.G)]
        top = max((g for g in range(r.G) if rep[g]), key=lambda g: (d0[g], -g))       # the first wins ties
        mean, mean_g, delta_g = r.positions()
        ss = sum(ti * (qi - Fraction(r.Q, r.T)) ** 2 for ti, qi in zip(r.t, r.q))
        lines.append(dict(gene=r.gene, num_pa=len(r.nzs), num_groups=sum(Ag > 0 for Ag in A), T=r.T, A=A, mean=mean,
                          eta2=D0 / ss, ge=(r.lo, r.hi), top=names[top], top_delta=delta_g[top], mean_g=mean_g,
                          delta_g=delta_g, reported=rep, gge=list(zip(r.glo, r.ghi))))
    for ln, adj in zip(lines, rc.bh([Fraction(1 + ln["ge"][0], 1 + n_perm) for ln in lines])):
        ln["p_adj"] = adj
    pairs = [(k, g) for k, ln in enumerate(lines) for g in range(len(sizes)) if ln["reported"][g]]
    adj = rc.bh([Fraction(1 + lines[k]["gge"][g][0], 1 + n_perm) for k, g in pairs])
    for ln in lines:
        ln["g_adj"] = [None] * len(sizes)
    for (k, g), v in zip(pairs, adj):
        lines[k]["g_adj"][g] = v
    return lines


def assert_no_near_tie(lines, what):
    """lo == hi for every record and group: no permutation's statistic lies within the 2^-39 band below the observed
    one, so the device's f64 comparison (band 2^-40) can hide nothing"""
    for ln in lines:
        assert ln["ge"][0] == ln["ge"][1], (what, ln["gene"], ln["ge"])
        for g, (lo, hi) in enumerate(ln["gge"]):
            assert lo == hi, (what, ln["gene"], g, lo, hi)


def compare(text, lines, names, n_perm, what):
    rows = list(csv.reader(io.StringIO(text)))
    G = len(names)
    assert rows[0] == HEADER + [f"{c}.{n}" for n in names for c in PER_GROUP], what
    body = rows[1:]
    print(what, "lines", len(body), "expected", len(lines))
    assert len(body) == len(lines), what
    for got, ln in zip(body, lines):
        ctx = (what, ln["gene"], got)
        assert len(got) == 12 + 6 * G, ctx
        assert got[:4] == [ln["gene"], str(ln["num_pa"]), str(ln["num_groups"]), str(ln["T"])], ctx
        assert got[6] == str(ln["ge"][0]) and got[11] == str(n_perm) and got[9] == ln["top"], ctx
        assert got[7] == repr((1 + ln["ge"][0]) / (1 + n_perm)), ctx
        for col, want in ((4, ln["mean"]), (5, ln["eta2"]), (8, ln["p_adj"]), (10, ln["top_delta"])):
            assert rc.close(got[col], want), (ctx, col, float(want))
        for g in range(G):
            f = got[12 + 6 * g:18 + 6 * g]
            assert f[0] == str(ln["A"][g]), (ctx, g)
            if ln["A"][g] == 0:
                assert f[1] == "", (ctx, g)
            else:
                assert rc.close(f[1], ln["mean_g"][g]), (ctx, g, "mean_pos")
            if not ln["reported"][g]:
                assert f[2:] == [""] * 4, (ctx, g)
                continue
            assert rc.close(f[2], ln["delta_g"][g]), (ctx, g, "delta_pos")
            assert f[3] == str(ln["gge"][g][0]), (ctx, g, "n_ge")
            assert f[4] == repr((1 + ln["gge"][g][0]) / (1 + n_perm)), (ctx, g)
            assert rc.close(f[5], ln["g_adj"][g]), (ctx, g, "p_val_adj")


# ---------------------------------------------------------------- the command
def dense_of(records, col_ids):
    """[dict(gene, K, alpha, dense)]: per record the (label < K, matrix column) read counts"""
    return [dict(gene=rec["gene_info_str"], K=int(rec["K"]), alpha=np.asarray(rec["alpha_arr"]), dense=m)
            for rec, m in zip(records, rc.dense_counts(records, col_ids))]


def _args(root, clu, res="res.gene.pkl", idents=(), n_perm=None, seed=None):
    a = ["diff_pa_len_groups", "--output_dir", str(root), "--res_pkl_file", res, "--cell_cluster_file", str(clu)]
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
    return os.path.join(str(root), f"{stem}.{kind}{tag}.diff_pa_len_groups.csv")


def _command(root, clu, res, idents, n_perm, seed, what=""):
    r = _run(_args(root, clu, res, idents, n_perm, seed))
    assert r.exit_code == 0, (what, r.output, repr(r.exception))
    assert not rc.parts_left(root)
    with open(_path(root, clu, res, idents), newline="") as fh:
        return fh.read()


# ---------------------------------------------------------------- CPU
def test_help_and_import_path():
    r = _run(["--help"])
    assert r.exit_code == 0 and "diff_pa_len_groups" in r.output
    r = _run(["diff_pa_len_groups", "--help"])
    assert r.exit_code == 0, r.output
    for o in ("--output_dir", "--res_pkl_file", "--cell_cluster_file", "--idents", "--n_perm", "--seed"):
        assert o in r.output
    assert "--strata_file" not in r.output and "--idents_1" not in r.output
    flat = " ".join(r.output.split())
    assert "[default: 9999]" in flat and "[default: 1]" in flat
    assert "same relabellings of the cells as in diff_pa_groups" in flat
    import scape.utils as su
    from scape_amd import _lib, report
    assert su.diff_pa_len_groups is report.diff_pa_len_groups
    assert "scape_hip_report_perm_len_groups" in _lib.SIGNATURES
    assert report.DIFF_PA_LEN_GROUPS_HEADER == HEADER and report.DIFF_PA_LEN_GROUPS_PER_GROUP == PER_GROUP


def test_prerequisites_and_argument_errors(tmp_path, no_gpu):
    """diff_pa_groups's list of errors, with this command's name in the messages, before the device is opened"""
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
                        (["--idents", "A"], "1 populations: diff_pa_len_groups takes 2 to 64"),
                        (["--idents", "A", "--idents", ""], "names no cluster"),
                        (["--idents", "A", "--idents", "a/b"], "file name"),
                        (["--n_perm", "0"], "n_perm"), (["--n_perm", str(1 << 31)], "n_perm"),
                        (["--seed", "-1"], "seed"), (["--seed", str(1 << 64)], "seed")):
        r = _run(_args(tmp_path, clu) + extra)
        assert isinstance(r.exception, ValueError) and word in str(r.exception), (extra, repr(r.exception))
    ids = list(range(100, 166))
    (tmp_path / "barcode_index.csv").write_text("CB,index\n" + "".join(f"C{i}-1,{i}\n" for i in ids))
    clu.write_text("index,group\n" + "".join(f"{i},g{i}\n" for i in ids[:65]))
    r = _run(_args(tmp_path, clu))
    assert isinstance(r.exception, ValueError) and "65 populations: diff_pa_len_groups" in str(r.exception)
    r = _run(["diff_pa_len_groups", "--output_dir", str(tmp_path), "--res_pkl_file", "res.gene.pkl"])
    assert r.exit_code == 2 and "--cell_cluster_file" in r.output
    r = _run(_args(tmp_path, clu) + ["--strata_file", str(clu)])
    assert r.exit_code == 2 and "--strata_file" in r.output
    assert sorted(os.listdir(tmp_path)) == ["barcode_index.csv", "groups.csv", "res.gene.pkl"]


POSITION_SETS = {
    "integers": [87.0, 230.0, 258.0, 268.0, 729.0],
    "two": [5.0, 6.0],
    "eighths": [3.125, 40.5, 17.875, 4999.0],
    "span-a-power-of-two": [1024.0, 0.0, 512.0, 1.0],
    "large": [3.0e9 + 7, 3.0e9 + 1.5e6, 3.0e9],
    "tenths": [0.1, 0.3, 0.7, 0.7, 1.9],
    "thirds": [1 / 3, 2 / 3, 100 / 3, 77.7],
    "tiny": [1e-300, 3e-300, 2.5e-300],
    "halves-to-even": [0.0, float(1 << 22), 0.5, 1.5, 2.5],
}


@pytest.mark.parametrize("x", list(POSITION_SETS.values()), ids=list(POSITION_SETS))
def test_quantisation_rule(x):
    """q_i of the host equal the restated rule's; qspan lies in 2^21 .. 2^22 and min q = 0; a position that is a
    multiple of 2^-s is exact, any other is off by at most half a unit; rint rounds half to even"""
    from scape_amd import report
    q, s = quantise(x)
    got = report._quantise_positions(np.array(x, dtype=np.float64))
    assert got.dtype == np.int32 and got.tolist() == q
    assert min(q) == 0 and 1 << 21 <= max(q) <= 1 << 22
    unit = Fraction(2) ** -s
    for v, qi in zip(x, q):
        w = Fraction(v - min(x))
        assert abs(qi * unit - w) <= unit / 2
        if (w / unit).denominator == 1:
            assert qi * unit == w
    exact = all((Fraction(v - min(x)) / unit).denominator == 1 for v in x)
    assert exact == (x not in (POSITION_SETS[k] for k in ("tenths", "thirds", "tiny", "halves-to-even")))
    if x is POSITION_SETS["halves-to-even"]:
        assert s == -1 and q == [0, 1 << 21, 0, 1, 1]             # 0.25 -> 0, 0.75 -> 1, 1.25 -> 1
    if x is POSITION_SETS["span-a-power-of-two"]:
        assert max(q) == 1 << 21                                    # frexp(2^k) = (0.5, k + 1)


def test_integer_form_and_two_group_identities():
    """on random small tables: the integer comparisons of LenGroupsRec.count are the Fraction comparisons of the
    definition, for G = 2 and G = 4; sum Q_g^2 / A_g - Q^2 / T is the definition's D; and for G = 2,
    D = (A_0 A_1 / T) delta^2 and |d_0| = |d_1| = 2^s |delta| with delta = diff_pa_len's mean_pos.1 - mean_pos.2 on
    positions that the q rule keeps exact"""
    rng = np.random.default_rng(5)
    for trial in range(12):
        G = 2 if trial % 2 == 0 else 4
        sizes = [int(v) for v in rng.integers(1, 6, G)]
        n, R = sum(sizes), int(rng.integers(2, 6))
        m = (rng.random((R, n)) < 0.6) * rng.integers(1, 5, (R, n))
        m[:, 0] |= 1                                                # every row has a read, population 0 too
        m[0, sizes[0]] |= 1                                         # and population 1
        x = sorted(float(v) for v in rng.choice(np.arange(5, 790), R, replace=False))
        if trial % 3 == 2:
            x = [v / 3 for v in x]                                  # not exact under the q rule
        nzs = [[(j, int(v)) for j, v in enumerate(row) if v] for row in m.tolist()]
        r = LenGroupsRec("g", nzs, x, sizes)
        assert r.tested()
        r.start()
        assert r.D(r.a0) == Fraction(r.E0[0], r.E0[1]) - Fraction(r.Q * r.Q, r.T)
        lo = hi = 0
        glo, ghi = [0] * G, [0] * G
        n_perm = 40
        for p in range(1, n_perm + 1):
            lab = labels(trial, p, sizes)
            r.count(lab)
            a = r.row_sums(lab)
            lo += r.D(a) >= r.D(r.a0)
            hi += r.D(a) >= r.D(r.a0) - Fraction(r.T * r.qspan ** 2, 1 << BAND)
            for g in range(G):
                glo[g] += abs(r.d(a, g)) >= abs(r.d(r.a0, g))
                ghi[g] += abs(r.d(a, g)) >= abs(r.d(r.a0, g)) - Fraction(r.qspan, 1 << BAND)
            if G == 2:
                A = r.A(a)
                assert r.d(a, 0) == -r.d(a, 1)
                assert r.D(a) == Fraction(A[0] * A[1], r.T) * r.d(a, 0) ** 2
                if trial % 3 != 2 and A[0] and A[1]:
                    m1 = sum(row[0] * xi for row, xi in zip(a, r.x)) / A[0]
                    m2 = sum(row[1] * xi for row, xi in zip(a, r.x)) / A[1]
                    assert r.d(a, 0) == (m1 - m2) * Fraction(2) ** r.s
        assert (r.lo, r.hi, r.glo, r.ghi) == (lo, hi, glo, ghi)
        assert 0 < lo <= n_perm


def test_host_position_columns():
    """the host's nucleotide columns follow the exact rationals, each rounded once; None where nothing is reported"""
    from scape_amd import report
    x = np.array([0.1, 0.7, 2.5])
    a = [[1, 3, 0], [2, 0, 0], [4, 1, 0]]
    mean, mean_g, delta_g = report._mean_positions_groups(x, a)
    fx = [Fraction(float(v)) for v in x]
    m0, m1 = (fx[0] + 2 * fx[1] + 4 * fx[2]) / 7, (3 * fx[0] + fx[2]) / 4
    assert mean == float((7 * m0 + 4 * m1) / 11)
    assert mean_g == [float(m0), float(m1), None] and delta_g == [float(m0 - m1), float(m1 - m0), None]
    assert report._mean_positions_groups(np.array([100.0, 300.0]), [[4, 1], [1, 7]])[2] == [-135.0, 135.0]


# ---------------------------------------------------------------- GPU: the entry point
N_TESTED, N_REST, EP_SEED = 300, 5, 31
EP_CHUNKS = (150, 120)                    # two chunks that accumulate: 270 permutations, one tile of 256 and a part


@functools.lru_cache(maxsize=None)
def entry_matrix():
    """the hand-made matrix of the entry point's tests: records of 2, 3 and 64 rows, every row with a read among the 300
    tested columns in front of 5 others, and a one-row record of 4,096 reads for the 2^31 refusal.  Positions: integers,
    tenths (not dyadic: rounded by the q rule) and eighths in no order.  Returns (Ks, read offsets, labels, cell ids,
    dense counts, row offsets per record, positions per row)"""
    rng = np.random.default_rng(44)
    n_cols = N_TESTED + N_REST
    Ks = np.array([2, 3, 64, 1], dtype=np.int32)
    dens = [0.3, 0.3, 0.05, 1.0]
    dense = np.concatenate([(rng.random((K, n_cols)) < d) * rng.integers(1, 4, (K, n_cols)) for K, d in zip(Ks, dens)])
    dense[-1, :] = 0
    dense[-1, :64] = 64                                                   # 4,096 reads in one row
    dense[:-1, 7] |= 1                                                    # every row has a read in a tested column
    lab, cb, off, base = [], [], [0], 0
    for K in Ks.tolist():
        l, c = np.nonzero(dense[base:base + K])
        rep = dense[base:base + K][l, c]
        lab.append(np.repeat(l, rep))
        cb.append(np.repeat(c, rep))
        off.append(off[-1] + int(rep.sum()))
        base += K
    roff = np.array([0, 2, 5, 69], dtype=np.int64)
    x = np.concatenate([[120.0, 455.0], [0.1, 0.7, 2.5], rng.permutation(rng.choice(40000, 64, replace=False)) / 8.0 + 3.0])
    return (Ks, np.array(off, np.int64), np.concatenate(lab).astype(np.int64), np.concatenate(cb).astype(np.int64),
            dense.astype(np.int64), roff, x)


def entry_sizes(G):
    """group sizes over the 300 tested columns: among them 1, 63, 64 and 65 cells"""
    if G == 2:
        return [63, N_TESTED - 63]
    if G == 3:
        return [1, 65, N_TESTED - 66]
    rest = N_TESTED - (1 + 63 + 64 + 65)
    return [1, 63, 64, 65] + [rest // (G - 4) + (g < rest % (G - 4)) for g in range(G - 4)]


@functools.lru_cache(maxsize=None)
def entry_oracle(G, p_first):
    _Ks, _off, _lab, _cb, dense, roff, x = entry_matrix()
    sizes = entry_sizes(G)
    assert len(sizes) == G and sum(sizes) == N_TESTED and min(sizes) >= 1
    recs = []
    for r in range(3):
        nzs = [[(j, int(v)) for j, v in enumerate(row[:N_TESTED].tolist()) if v] for row in dense[roff[r]:roff[r + 1]]]
        recs.append(LenGroupsRec(f"rec{r}", nzs, x[roff[r]:roff[r + 1]].tolist(), sizes))
        assert recs[-1].tested()
    seen_empty = [False]
    for r in recs:
        r.start()
    for p in range(p_first, p_first + sum(EP_CHUNKS)):
        lab = labels(EP_SEED, p, sizes)
        for r in recs:
            r.count(lab)
        seen_empty[0] |= 0 in recs[0].A(recs[0].row_sums(lab))
    return sizes, recs, seen_empty[0]


def _entry_call(lib, h, roff, rows, G, seg, q, tol_stat, tol_delta, o):
    from scape_amd._lib import P_d, P_i32, P_i64, ptr
    return lib.scape_hip_report_perm_len_groups(h, len(roff) - 1, ptr(roff, P_i64), ptr(rows, P_i64), G, ptr(seg, P_i32),
                                                ptr(q, P_i32), ptr(tol_stat, P_d), ptr(tol_delta, P_d), ptr(o[0], P_i64),
                                                ptr(o[1], P_i64), ptr(o[2], P_d), ptr(o[3], P_d), ptr(o[4], P_i64),
                                                ptr(o[5], P_i64))


def _entry_outs(n_rows, n_rec, G):
    return (np.full(n_rows, -1, np.int64), np.full((n_rows, G), -1, np.int64), np.full(n_rec, -1.0),
            np.full((n_rec, G), -1.0), np.zeros(n_rec, np.int64), np.zeros((n_rec, G), np.int64))


@pytest.mark.gpu
@pytest.mark.parametrize("p_first", [1, 257])
@pytest.mark.parametrize("G", [2, 3, 5, 17, 32, 33, 64])
def test_entry_point(G, p_first):
    """scape_hip_report_perm_len_groups on the hand-made matrix, on both sides of the LDS slice of 32 groups: t, a0 and
    both kinds of counts, accumulated over two chunks of permutations, equal the oracle's (lo == hi asserted first, every
    record and group); D(0) and d_g(0) within the stated (G + 8) 2^-53 T qspan^2 and 3 x 2^-53 qspan of the exact
    values.  A group of one cell has no read in the two-row record under some labelling (A_g(p) = 0)"""
    from scape_amd import _lib
    from scape_amd._lib import P_i32, check as chk, ptr
    Ks, off, lab, cb, dense, roff, _x = entry_matrix()
    sizes, recs, seen_empty = entry_oracle(G, p_first)
    for r in recs:
        assert r.lo == r.hi and r.glo == r.ghi, (G, r.gene, r.lo, r.hi, r.glo, r.ghi)
    assert seen_empty or G == 2
    rows = np.arange(int(roff[-1]), dtype=np.int64)
    seg = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    sz = np.array(sizes, dtype=np.int32)
    q = np.array([qi for r in recs for qi in r.q], dtype=np.int32)
    tol_stat = np.array([math.ldexp(float(r.T * r.qspan ** 2), -40) for r in recs])
    tol_delta = np.array([math.ldexp(float(r.qspan), -40) for r in recs])
    ctx = _lib.default_context(None)
    lib = ctx.lib
    try:
        assert np.array_equal(rc.device_counts(ctx, Ks, off, lab, cb, N_TESTED + N_REST), dense.sum(axis=1))
        o = _entry_outs(len(rows), 3, G)
        first = p_first
        for p_count in EP_CHUNKS:
            chk(lib.scape_hip_report_perm_labels(ctx.h, G, ptr(sz, P_i32), first, p_count, EP_SEED), "perm_labels")
            chk(_entry_call(lib, ctx.h, roff, rows, G, seg, q, tol_stat, tol_delta, o), "perm_len_groups")
            first += p_count
    finally:
        lib.scape_hip_report_free(ctx.h)
    want = dict(t=[ti for r in recs for ti in r.t], a0=[row for r in recs for row in r.a0], n_ge=[r.lo for r in recs],
                group=[r.glo for r in recs])
    for got, name in ((o[0], "t"), (o[1], "a0"), (o[4], "n_ge"), (o[5], "group")):
        print(G, p_first, name, "equal", got.tolist() == want[name], got.tolist()[:3], want[name][:3])
        assert got.tolist() == want[name], (G, name)
    u = Fraction(1, 1 << 53)
    for k, r in enumerate(recs):
        err = abs(Fraction(float(o[2][k])) - r.D(r.a0))
        print("D0", k, float(o[2][k]), "error / (u T qspan^2)", float(err / (u * r.T * r.qspan ** 2)))
        assert err <= (G + 8) * u * r.T * r.qspan ** 2, (G, k, float(err))
        for g in range(G):
            assert abs(Fraction(float(o[3][k, g])) - r.d(r.a0, g)) <= 3 * u * r.qspan, (G, k, g)
    assert 0 < max(want["n_ge"]) and min(min(g) for g in want["group"]) < sum(EP_CHUNKS)


@pytest.mark.gpu
def test_entry_point_refusals():
    """labels not built, a G that does not match the labels, q outside 0 .. 2^22, negative or non-finite tolerances:
    non-zero, a message, nothing written and nothing added.  2^31 reads or more in a record are known only once the
    device has summed its rows: that refusal comes behind the row sums and before the test is queued, and adds nothing
    either"""
    from scape_amd import _lib
    from scape_amd._lib import P_d, P_i32, P_i64, check as chk, ptr
    Ks, off, lab, cb, dense, roff, _x = entry_matrix()
    G = 3
    sizes, recs, _ = entry_oracle(G, 1)
    rows = np.arange(int(roff[-1]), dtype=np.int64)
    seg = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    sz = np.array(sizes, dtype=np.int32)
    q = np.array([qi for r in recs for qi in r.q], dtype=np.int32)
    tol_stat = np.array([math.ldexp(float(r.T * r.qspan ** 2), -40) for r in recs])
    tol_delta = np.array([math.ldexp(float(r.qspan), -40) for r in recs])
    ctx = _lib.default_context(None)
    lib = ctx.lib
    o = _entry_outs(len(rows), 3, G)

    def call(G_=G, seg_=seg, q_=q, ts=tol_stat, td=tol_delta, roff_=roff, rows_=rows, o_=o):
        return _entry_call(lib, ctx.h, roff_, rows_, G_, seg_, q_, ts, td, o_)

    def changed(a, k, v):
        b = a.copy()
        b[k] = v
        return b
    try:
        assert call() != 0 and "report_counts" in _lib.last_error()
        rc.device_counts(ctx, Ks, off, lab, cb, N_TESTED + N_REST)
        assert call() != 0 and "perm_labels" in _lib.last_error()           # counts, but no labels yet
        chk(lib.scape_hip_report_perm_labels(ctx.h, G, ptr(sz, P_i32), 1, 10, 1), "perm_labels")
        o2 = _entry_outs(len(rows), 3, 2)
        assert call(2, seg[:3].copy(), o_=o2) != 0 and "n_groups" in _lib.last_error()
        assert call(seg_=changed(seg, 1, seg[1] + 1)) != 0 and "seg_off" in _lib.last_error()
        assert call(q_=changed(q, 3, -1)) != 0 and "2^22" in _lib.last_error()
        assert call(q_=changed(q, 3, (1 << 22) + 1)) != 0 and "2^22" in _lib.last_error()
        for bad in (-1.0, np.inf, np.nan):
            assert call(ts=changed(tol_stat, 1, bad)) != 0 and "tolerances" in _lib.last_error(), bad
            assert call(td=changed(tol_delta, 2, bad)) != 0 and "tolerances" in _lib.last_error(), bad
        assert lib.scape_hip_report_perm_len_groups(ctx.h, 3, ptr(roff, P_i64), ptr(rows, P_i64), G, ptr(seg, P_i32), None,
                                                    ptr(tol_stat, P_d), ptr(tol_delta, P_d), ptr(o[0], P_i64),
                                                    ptr(o[1], P_i64), ptr(o[2], P_d), ptr(o[3], P_d), ptr(o[4], P_i64),
                                                    ptr(o[5], P_i64)) != 0 and "bad argument" in _lib.last_error()
        assert all(np.all(a == -1) for a in o[:4]) and not o[4].any() and not o[5].any()   # nothing written or added
        # 2^19 times the row of 4,096 reads: T = 2^31
        heavy = np.full(1 << 19, int(roff[-1]), dtype=np.int64)
        oh = _entry_outs(len(heavy), 1, G)
        assert _entry_call(lib, ctx.h, np.array([0, len(heavy)], np.int64), heavy, G, seg,
                           np.zeros(len(heavy), np.int32), tol_stat[:1], tol_delta[:1], oh) != 0
        assert "2^31 or more reads" in _lib.last_error() and not oh[4].any() and not oh[5].any()
        assert call(q_=changed(q, 3, 1 << 22)) == 0                          # the bounds themselves pass
        assert o[4].tolist() != [0, 0, 0] and np.all(o[0] >= 0)
    finally:
        lib.scape_hip_report_free(ctx.h)


# ---------------------------------------------------------------- GPU: the synthetic directory
@functools.lru_cache(maxsize=None)
def _syn():
    records, bc, clu_text = rc.synthetic()
    return dict(records=records, bc=bc, clu=clu_text, recs=dense_of(records, rc.column_ids(bc)))


@functools.lru_cache(maxsize=None)
def _syn_lines(idents, n_perm, seed, n_rec=None):
    s = _syn()
    pops = populations_all(s["bc"], s["clu"], idents)
    names = [name for name, _c in pops]
    return names, oracle(s["recs"][:n_rec], [c for _n, c in pops], names, n_perm, seed)


def _check_syn(tmp_path, idents, n_perm, seed, what, n_rec=None):
    names, lines = _syn_lines(idents, n_perm, seed, n_rec)
    assert_no_near_tie(lines, what)
    path = rc.write_synthetic(tmp_path, n_rec)
    text = _command(tmp_path, path, "res.gene.pkl", idents, n_perm, seed, what)
    compare(text, lines, names, n_perm, what)
    return text, lines, names


@pytest.mark.gpu
def test_synthetic_directory_all_clusters(tmp_path):
    """999 permutations of 230 + 301 + 40 cells in the clusters A, B, C (order of first appearance in the file): every
    column of the file against the exact oracle.  GENE0..GENE2 have a planted excess of the first site in A: their
    omnibus count and A's own count reach 0 and A's 3'UTRs are the shorter ones, on the oracle and so in the file"""
    _text, lines, names = _check_syn(tmp_path, (), 999, 1, "syn/all")
    assert sorted(names) == ["A", "B", "C"]
    by = {ln["gene"].split(":")[1]: ln for ln in lines}
    assert "GENE5" not in by and "GENE6" not in by and len(by) >= 30          # reads only in A; K = 1
    a = names.index("A")
    for g in ("GENE0", "GENE1", "GENE2"):
        assert by[g]["ge"][0] == 0 and by[g]["gge"][a][0] == 0 and by[g]["delta_g"][a] < 0 and by[g]["top"] == "A", g
    assert max(ln["num_pa"] for ln in lines) == 63 and len({ln["top"] for ln in lines}) == 3


@pytest.mark.gpu
def test_synthetic_directory_idents_in_the_order_given(tmp_path):
    """--idents B --idents A: population 0 is B, the file name carries .B+A, the columns are reads.B, ..., reads.A, ..."""
    text, _lines, _names = _check_syn(tmp_path, ("B", "A"), 999, 1, "syn/B+A")
    assert os.path.basename(_path(tmp_path, "syn_groups.csv", "res.gene.pkl", ("B", "A"))) == \
        "syn_groups.gene.B+A.diff_pa_len_groups.csv"
    assert text.split("\n", 1)[0].endswith(",n_perm,reads.B,mean_pos.B,delta_pos.B,n_ge.B,p_val.B,p_val_adj.B,"
                                           "reads.A,mean_pos.A,delta_pos.A,n_ge.A,p_val.A,p_val_adj.A")


@pytest.mark.gpu
def test_two_idents_count_what_diff_pa_len_counts(tmp_path):
    """--idents A --idents B against diff_pa_len --idents_1 A --idents_2 B, same seed and n_perm, on the synthetic
    directory, whose positions are integers below 2^22 and so exact under the q rule: the same tested records, and record
    for record n_ge.A = n_ge.B = diff_pa_len's n_ge, delta_pos.A = its delta_pos = -delta_pos.B, mean_pos.A / .B = its
    mean_pos.1 / .2"""
    for rec in _syn()["records"]:
        a = np.asarray(rec["alpha_arr"])
        assert a.dtype.kind == "i" and 0 <= a.min() and a.max() < 1 << 22
    path = rc.write_synthetic(tmp_path)
    mine = list(csv.reader(io.StringIO(_command(tmp_path, path, "res.gene.pkl", ("A", "B"), 999, 1))))[1:]
    theirs = list(csv.reader(io.StringIO(rc.perm_command("diff_pa_len", tmp_path, path, "res.gene.pkl", "A", "B", 999,
                                                         1))))[1:]
    assert len(mine) == len(theirs) > 30
    assert [(r[0], r[15], r[21]) for r in mine] == [(r[0], r[11], r[11]) for r in theirs]
    for m, t in zip(mine, theirs):
        assert (m[12], m[18], m[13], m[19], m[14]) == (t[3], t[4], t[5], t[6], t[7]), (m, t)
        assert float(m[20]) == -float(m[14])
    assert len({r[15] for r in mine}) > 10


@pytest.mark.gpu
def test_batch_chunk_and_seed_invariance(tmp_path, monkeypatch):
    """records split over several count batches and the permutations over several chunks: the same bytes; the same seed
    again: the same bytes; another seed: other counts"""
    from scape_amd import _lib, report
    path = rc.write_synthetic(tmp_path)
    big = _command(tmp_path, path, "res.gene.pkl", (), 299, 1)
    assert _command(tmp_path, path, "res.gene.pkl", (), 299, 1) == big
    other = _command(tmp_path, path, "res.gene.pkl", (), 299, 2)
    col = lambda text: [(r[6], r[15]) for r in csv.reader(io.StringIO(text))]
    assert col(big) != col(other) and len(col(big)) == len(col(other)) > 30
    lib = _lib.load_library()
    calls = {"labels": [], "test": 0}
    real_l, real_t = lib.scape_hip_report_perm_labels, lib.scape_hip_report_perm_len_groups

    def make_labels(*a):
        calls["labels"].append((a[3], a[4]))
        return real_l(*a)

    def test(*a):
        calls["test"] += 1
        return real_t(*a)
    monkeypatch.setattr(lib, "scape_hip_report_perm_labels", make_labels)
    monkeypatch.setattr(lib, "scape_hip_report_perm_len_groups", test)
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
    _text, lines, _names = _check_syn(tmp_path, ("C", "A", "B"), n_perm, 5, f"tile/{n_perm}", 12)
    assert len(lines) == 10


# ---------------------------------------------------------------- GPU: positions through the command, .part files
def _three_group_dir(root, alphas, n_cells=45, gen_seed=3, only_label=None):
    """records with the given alpha_arr each (K = its length) on n_cells barcodes, a third each in the clusters A, B and
    C.  only_label = {record: label}: every read of that record carries that label"""
    from scape.apa_core import Parameters
    rng = np.random.default_rng(gen_seed)
    ids = np.arange(n_cells) * 5 + 1
    bc = "CB,index\n" + "".join(f"T{j}-1,{i}\n" for j, i in enumerate(ids.tolist()))
    clu_text = "index,group\n" + "".join(f"{i},{'ABC'[3 * j // n_cells]}\n" for j, i in enumerate(ids.tolist()))
    records = []
    for r, alpha in enumerate(alphas):
        K = len(alpha)
        records.append(dict(gene_info_str=f"3:TG{r}:{1 + r % 2}:{700 * r + 1}-{700 * r + 600}:{'+-'[r % 2]}", K=K,
                            alpha_arr=np.asarray(alpha), beta_arr=np.full(K, 10.0),
                            label_arr=(rng.integers(0, K + 1, 300) if r not in (only_label or {}) else  # K: no site
                                       np.full(300, only_label[r])).astype(np.int64),
                            cb_id_arr=ids[rng.integers(0, n_cells, 300)].astype(np.int64)))
    path = rc.write_dir(str(root), "res.gene.pkl", records, bc, {"three.csv": clu_text}, Parameters)[0]
    return path, clu_text, bc, dense_of(records, ids.tolist())


@pytest.mark.gpu
def test_positions_and_part_files(tmp_path):
    """float positions that the q rule rounds (tenths), unsorted ones, a record whose kept rows share one position (no
    line) and a record with reads at one site only (no line): the file against the oracle, and no .part file left.  A
    NaN position of a pA site with reads - also in a record that would not be tested - is a ValueError naming the record
    that leaves neither the file nor a .part file; a NaN at a site without reads is never looked at"""
    nan = float("nan")
    root = tmp_path / "fine"
    alphas = [[30, 200, 410], [500, 20, 260, 90], [77, 77], [0.1, 0.7, 2.5, 1.9], [25.0, nan, 300.0], [40, 41]]
    path, clu_text, bc, recs = _three_group_dir(root, alphas, only_label={4: 0})
    recs[4]["alpha"] = np.array([25.0, 0.0, 300.0])               # the oracle never reads that entry either
    pops = populations_all(bc, clu_text)
    names = [n for n, _c in pops]
    lines = oracle(recs, [c for _n, c in pops], names, 199, 3)
    assert_no_near_tie(lines, "positions")
    assert [ln["gene"].split(":")[1] for ln in lines] == ["TG0", "TG1", "TG3", "TG5"]
    compare(_command(root, path, "res.gene.pkl", (), 199, 3, "positions"), lines, names, 199, "positions")
    assert not rc.parts_left(root) and os.path.exists(_path(root, path, "res.gene.pkl"))
    for k, (alphas, only) in enumerate((([[30, 200, 410], [25.0, nan, 300.0]], None),
                                        ([[30, 200, 410], [25.0, 60.0, nan]], {1: 2}))):
        root = tmp_path / f"d{k}"
        path, _clu, _bc, _recs = _three_group_dir(root, alphas, only_label=only)
        r = _run(_args(root, path, n_perm=50))
        assert isinstance(r.exception, ValueError) and "TG1" in str(r.exception), repr(r.exception)
        assert not rc.parts_left(root) and not os.path.exists(_path(root, path, "res.gene.pkl"))
