"""`scape diff_pa_len_trend`: the exact permutation test of the pA position (3'UTR length) ALONG a per-cell score
(scape_amd/report.py, section diff_pa_len_trend; kernels k_rep_len_trend_obs and k_rep_perm_len_trend and the entry
point scape_hip_report_perm_len_trend of scape_amd/csrc/perm.inc).

The contract.  Score file, scored cells, --rank, the 15-bit integer scores q_j and the permuted scores z_p(j) =
q[rank of key(p, j)] are diff_pa_trend's (tests/test_report_difftrend.py, whose restatements this file uses).  Kept
rows of a record are the labels < K with a read in a scored cell, in label order, at the positions alpha_arr[label]; a
record is tested when it has two or more and they lie at two positions or more.  Per record, with T its reads in the
scored cells, the positions become integers at B = min(22, 48 - T.bit_length()) bits:  w_i = fl(pos_i - min pos),
frexp(span) = (m, e),  x_i = rint(ldexp(w_i, B - e)), half to even, so 2^(B-1) <= max x_i <= 2^B.  With c_ij the count
of kept row i at position j and scores z:
    t_i = sum_j c_ij,  T = sum_i t_i < 2^31,  Sx = sum_i t_i x_i                    (fixed)
    s_i = sum_j c_ij z(j),  Sz = sum_i s_i,  Sxz = sum_i x_i s_i                    (per labelling)
    C   = T Sxz - Sx Sz
    n_ge = #{p in 1..n_perm: |C(p)| >= |C(0)|}                                      (two-sided, integers)
p = (1 + n_ge) / (1 + n_perm), Benjamini-Hochberg over the file's lines.  With Vz = T sum_ij c_ij q_j^2 - Sz^2 and Vx =
T sum_i t_i x_i^2 - Sx^2:  slope = (C / Vz) 2^(e - B) 2^s nucleotides per unit of score, delta_pos = slope x qspan 2^-s,
r = C / sqrt(Vz Vx); all three empty when Vz = 0.  mean_pos = sum t_i pos_i / T from the exact positions, mean_score =
min score + (Sz / T) 2^-s.

The oracle below restates this in Python ints and imports nothing from scape_amd.  The device compares integers, so
every comparison of counts is EQUALITY: there is no band, no near tie to exclude and nothing is excused."""
import csv
import functools
import io
import math
import os
from fractions import Fraction

import numpy as np
import pytest

import report_cases as rc
import test_report_difftrend as tt
from report_cases import no_gpu, run as _run  # noqa: F401  (no_gpu: fixture)

HEADER = ["gene", "num_pa", "reads", "mean_pos", "mean_score", "slope", "delta_pos", "r", "n_ge", "p_val", "p_val_adj",
          "n_perm"]
MAX_X = 1 << 22


# ---------------------------------------------------------------- the contract, restated
def position_bits(T):
    return min(22, 48 - T.bit_length())


def quantise_pos(pos, bits):
    """(x_i as Python ints, B - e) of positions pos (floats), as tests/test_report_difflengroups.py restates the rule"""
    lo, hi = min(pos), max(pos)
    _m, e = math.frexp(hi - lo)
    return [round(Fraction(v - lo) * Fraction(2) ** (bits - e)) for v in pos], bits - e


class LenTrendRec:
    """a record's kept rows: per row its nonzeros [(position j, count)] among the tested columns and its integer
    position x_i; integers only"""

    def __init__(self, gene, nzs, x, q):
        self.gene, self.nzs, self.x, self.q = gene, nzs, x, q
        self.t = [sum(v for _j, v in nz) for nz in nzs]
        self.T = sum(self.t)
        self.Sx = sum(ti * xi for ti, xi in zip(self.t, x))
        self.Vx = self.T * sum(ti * xi * xi for ti, xi in zip(self.t, x)) - self.Sx ** 2
        self.s0 = self.sums(q)
        self.sq0 = [sum(v * q[j] ** 2 for j, v in nz) for nz in nzs]
        self.C0 = self.C(self.s0)
        # per cell j: its reads and the sum of their positions, for the permutations (C needs nothing else of a cell)
        self.cell_n, self.cell_m = {}, {}
        for nz, xi in zip(nzs, x):
            for j, v in nz:
                self.cell_n[j] = self.cell_n.get(j, 0) + v
                self.cell_m[j] = self.cell_m.get(j, 0) + v * xi
        self.n_ge = 0
        self.Cp = {}

    def sums(self, z):
        return [sum(v * z[j] for j, v in nz) for nz in self.nzs]

    def C(self, s):
        return self.T * sum(xi * si for xi, si in zip(self.x, s)) - self.Sx * sum(s)

    def C_of(self, z):
        """C under scores z from the per-cell sums: Sz = sum_j n_j z_j, Sxz = sum_j m_j z_j"""
        Sz = sum(v * z[j] for j, v in self.cell_n.items())
        Sxz = sum(v * z[j] for j, v in self.cell_m.items())
        return self.T * Sxz - self.Sx * Sz

    def count(self, p, z):
        c = self.Cp[p] = self.C_of(z)
        self.n_ge += abs(c) >= abs(self.C0)

    def halves(self):
        """(low, high) 64 bits of the two's-complement C(0), as signed 64-bit integers"""
        lo, hi = self.C0 & rc.M64, self.C0 >> 64
        assert -(1 << 63) <= hi < 1 << 63
        return lo - (1 << 64) if lo >= 1 << 63 else lo, hi


def count_permutations(recs, seed, perms, q):
    qa = np.asarray(q)
    for p in perms:
        z = qa[tt.np_ranks(seed, p, len(q))].tolist()      # tt.np_ranks is held to tt.ranks by test_report_difftrend
        for r in recs:
            r.count(p, z)


def oracle(records, bc_csv, score_csv, rank, n_perm, seed):
    """the expected lines of the command's file, in order: dicts of the text columns, the exact count and the Fractions
    of the float columns (r2 = r^2 and sign = that of C(0))"""
    col_ids = rc.column_ids(bc_csv)
    score = tt.parse_scores(score_csv)
    cols = [j for j, i in enumerate(col_ids) if score.get(i) is not None]
    sc = [score[col_ids[j]] for j in cols]
    assert len(cols) >= 2 and max(sc) > min(sc)
    if rank:
        sc = [float(r) for r in tt.rank_ints(sc)]
    q, s = tt.quantise(sc)
    qspan = max(q)
    live = []
    for rec, dense in zip(records, rc.dense_counts(records, col_ids)):
        sub = dense[:, cols]
        kept = [l for l in range(int(rec["K"])) if sub[l].any()]
        pos = [float(rec["alpha_arr"][l]) for l in kept]
        if len(kept) < 2 or not max(pos) > min(pos):
            continue
        nzs = [[(j, int(v)) for j, v in enumerate(sub[l].tolist()) if v] for l in kept]
        T = sum(v for nz in nzs for _j, v in nz)
        assert T < 1 << 31
        x, xshift = quantise_pos(pos, position_bits(T))
        r = LenTrendRec(rec["gene_info_str"], nzs, x, q)
        r.pos, r.xshift = pos, xshift
        live.append(r)
    count_permutations(live, seed, range(1, n_perm + 1), q)
    lo_s, unit_z = Fraction(min(sc)), Fraction(2) ** -s
    lines = []
    for r in live:
        Sz = sum(r.s0)
        Vz = r.T * sum(r.sq0) - Sz * Sz
        unit_x = Fraction(2) ** -r.xshift
        ln = dict(gene=r.gene, num_pa=len(r.nzs), T=r.T, ge=r.n_ge, Vz=Vz, C0=r.C0,
                  mean_pos=sum(ti * Fraction(p) for ti, p in zip(r.t, r.pos)) / r.T,
                  mean_score=lo_s + Fraction(Sz, r.T) * unit_z)
        if Vz:
            ln["slope"] = Fraction(r.C0, Vz) * unit_x / unit_z
            ln["delta"] = ln["slope"] * qspan * unit_z
            ln["r2"] = Fraction(r.C0 ** 2, Vz * r.Vx)
        lines.append(ln)
    for ln, adj in zip(lines, rc.bh([Fraction(1 + ln["ge"], 1 + n_perm) for ln in lines])):
        ln["p_adj"] = adj
    return lines


def compare(text, lines, n_perm, what):
    rows = list(csv.reader(io.StringIO(text)))
    assert rows[0] == HEADER, what
    body = rows[1:]
    print(what, "lines", len(body), "expected", len(lines))
    assert len(body) == len(lines), what
    for got, ln in zip(body, lines):
        ctx = (what, ln["gene"], got)
        assert len(got) == len(HEADER), ctx
        assert got[:3] == [ln["gene"], str(ln["num_pa"]), str(ln["T"])], ctx
        assert got[8] == str(ln["ge"]) and got[9] == repr((1 + ln["ge"]) / (1 + n_perm)) and got[11] == str(n_perm), ctx
        assert rc.close(got[3], ln["mean_pos"]) and rc.close(got[4], ln["mean_score"]) and rc.close(got[10], ln["p_adj"]), ctx
        if not ln["Vz"]:
            assert got[5:8] == ["", "", ""] and ln["ge"] == n_perm, ctx
            continue
        assert rc.close(got[5], ln["slope"]) and rc.close(got[6], ln["delta"]), ctx
        # r is the float square root of the rounded r^2, relative error at most 2^-52: its square is within 3 RTOL
        rr = Fraction(float(got[7]))
        assert repr(float(got[7])) == got[7] and abs(rr * rr - ln["r2"]) <= 3 * rc.RTOL * ln["r2"], ctx
        assert (rr > 0) == (ln["C0"] > 0) and (rr < 0) == (ln["C0"] < 0) and abs(rr) <= 1, ctx


# ---------------------------------------------------------------- the command
def _args(root, scores, res="res.gene.pkl", rank=False, n_perm=None, seed=None):
    return ["diff_pa_len_trend"] + tt._args(root, scores, res, rank, n_perm, seed)[1:]


def _path(root, scores, res, rank=False):
    kind = res[len("res."):-len(".pkl")]
    stem = os.path.splitext(os.path.basename(str(scores)))[0]
    return os.path.join(str(root), f"{stem}.{kind}{'.rank' if rank else ''}.diff_pa_len_trend.csv")


def _command(root, scores, res, rank, n_perm, seed, what=""):
    r = _run(_args(root, scores, res, rank, n_perm, seed))
    assert r.exit_code == 0, (what, r.output, repr(r.exception))
    assert not rc.parts_left(root)
    with open(_path(root, scores, res, rank), newline="") as fh:
        return fh.read()


# ---------------------------------------------------------------- CPU
def test_help_and_import_path():
    r = _run(["--help"])
    assert r.exit_code == 0 and "diff_pa_len_trend" in r.output
    r = _run(["diff_pa_len_trend", "--help"])
    assert r.exit_code == 0, r.output
    for o in ("--output_dir", "--res_pkl_file", "--cell_score_file", "--rank", "--n_perm", "--seed"):
        assert o in r.output
    assert "--strata_file" not in r.output and "--idents" not in r.output
    flat = " ".join(r.output.split())
    assert "[default: 9999]" in flat and "[default: 1]" in flat
    import scape.utils as su
    from scape_amd import _lib, report
    assert su.diff_pa_len_trend is report.diff_pa_len_trend
    assert "scape_hip_report_perm_len_trend" in _lib.SIGNATURES


def test_header_row():
    from scape_amd import report
    assert report.DIFF_PA_LEN_TREND_HEADER == HEADER


def test_integer_forms_against_fractions():
    """on random small tables: C / T^2 is the covariance of position and score over the reads, straight from the
    definition in Fractions; Sx and sum t x^2 do not depend on the labelling, so |C| is |slope of z on x| times the
    fixed Vx > 0 and orders the labellings as that slope does; the per-cell form of C is the per-row one; and the
    halves put C(0) back together"""
    rng = np.random.default_rng(12)
    for trial in range(10):
        n, R = int(rng.integers(3, 12)), int(rng.integers(2, 6))
        m = (rng.random((R, n)) < 0.6) * rng.integers(1, 5, (R, n))
        m[:, 0] |= 1
        sc = [float(v) for v in rng.integers(0, 50, n)]
        sc[0], sc[1] = 0.0, 49.0
        q, _s = tt.quantise([v / 3 for v in sc] if trial % 2 else sc)
        pos = [float(v) for v in sorted(rng.choice(900, R, replace=False).tolist())]
        x, _xs = quantise_pos(pos, 22)
        nzs = [[(j, int(v)) for j, v in enumerate(row) if v] for row in m.tolist()]
        r = LenTrendRec("g", nzs, x, q)
        assert r.Vx > 0
        seen = []
        for p in range(0, 41):
            z = q if p == 0 else tt.permuted(trial, p, q)
            s = r.sums(z)
            reads = [(xi, z[j]) for nz, xi in zip(nzs, x) for j, v in nz for _ in range(v)]
            assert len(reads) == r.T
            mx, mz = Fraction(sum(a for a, _b in reads), r.T), Fraction(sum(b for _a, b in reads), r.T)
            cov = sum((a - mx) * (b - mz) for a, b in reads) / r.T
            var_x = sum((a - mx) ** 2 for a, _b in reads) / r.T
            assert Fraction(r.C(s), r.T ** 2) == cov and r.C_of(z) == r.C(s)
            assert var_x == Fraction(r.Vx, r.T ** 2)                 # the same under every labelling
            assert cov / var_x == Fraction(r.C(s), r.Vx)             # the slope of the score on the position
            seen.append((abs(r.C(s)), abs(cov / var_x)))
        assert sorted(seen) == sorted(seen, key=lambda c: c[1])      # |C| and |slope| order the labellings alike
        lo, hi = r.halves()
        assert (hi << 64) + (lo & rc.M64) == r.C0


@pytest.mark.parametrize("T, bits", [(1, 22), ((1 << 25) - 1, 22), (1 << 25, 22), ((1 << 26) - 1, 22), (1 << 26, 21),
                                     ((1 << 27) - 1, 21), (1 << 30, 17), ((1 << 31) - 1, 17)])
def test_position_bit_rule(T, bits):
    """B = min(22, 48 - T.bit_length()) at bit lengths 1, 25, 26, 27 and 31; the host quantises at B bits by the
    restated rule, max x reaches 2^B when the span's mantissa rounds up, and even then T max x < 2^48, so that with scores
    of up to 2^15 Sxz < 2^63 and Sx < 2^48"""
    from scape_amd import report
    assert T.bit_length() in (1, 25, 26, 27, 31)
    assert position_bits(T) == bits == report._len_trend_bits(T) == report._len_trend_bits(np.int64(T))
    for pos in ([5.0, 790.0, 12.5], [0.0, math.nextafter(1024.0, 0.0), 3.0], [10.0, 10.0 + 2.0 ** -30], [0.0, 1024.0]):
        x, shift = quantise_pos(pos, bits)
        got = report._quantise_positions(np.array(pos), bits)
        assert got.dtype == np.int32 and got.tolist() == x
        assert min(x) == 0 and 1 << (bits - 1) <= max(x) <= 1 << bits <= MAX_X
        assert T * max(x) < 1 << 48 and T * max(x) << 15 < 1 << 63
        assert abs(Fraction(pos[1] - pos[0]) - x[1] * Fraction(2) ** -shift) <= Fraction(2) ** -shift / 2
    assert max(quantise_pos([0.0, math.nextafter(1024.0, 0.0)], bits)[0]) == 1 << bits
    assert report._quantise_positions(np.array([5.0, 790.0])).tolist() == quantise_pos([5.0, 790.0], 22)[0]


def test_prerequisites_and_argument_errors(tmp_path, no_gpu, monkeypatch):
    """diff_pa_trend's errors, naming this command, before the device is opened, and no file is left"""
    from scape_amd import report
    sc = tmp_path / "pt.csv"
    r = _run(_args(tmp_path / "nope", sc))
    assert r.exit_code != 0 and "Given output_dir folder does not exists." in str(r.exception)
    r = _run(_args(tmp_path, sc))
    assert "Given res_pkl_file is not in output_dir." in str(r.exception)
    sc = tt._small_dir(tmp_path)
    r = _run(_args(tmp_path, sc))
    assert "Given cell_score_file file does not exists" in str(r.exception)
    for body, word in (("3,0.5\n4,inf\n5,1\n", "row 2"), ("3,0.5\n4,1.0\n5,late\n", "row 3"),
                       ("3,0.5\n4,NA\n5,\n6,nan\n", "1 cells"), ("77,0.5\n78,1.5\n", "0 cells"),
                       ("3,0.5\n4,0.50\n5,5e-1\n6,NA\n", "has the score"), ("3,1\n3,NA\n4,2\n", "1 cells")):
        sc.write_text("index,pseudotime\n" + body)
        r = _run(_args(tmp_path, sc))
        assert isinstance(r.exception, ValueError) and word in str(r.exception), (body, repr(r.exception))
        if "cells" in word:
            assert "diff_pa_len_trend takes 2 or more" in str(r.exception)
    sc.write_text("index,pseudotime\n3,0.5\n4,1.5\n5,2\n")
    for extra, word in ((["--n_perm", "0"], "n_perm"), (["--n_perm", str(1 << 31)], "n_perm"),
                        (["--seed", "-1"], "seed"), (["--seed", str(1 << 64)], "seed")):
        r = _run(_args(tmp_path, sc) + extra)
        assert isinstance(r.exception, ValueError) and word in str(r.exception), (extra, repr(r.exception))
    r = _run(["diff_pa_len_trend", "--output_dir", str(tmp_path), "--res_pkl_file", "res.gene.pkl"])
    assert r.exit_code == 2 and "--cell_score_file" in r.output
    assert _run(_args(tmp_path, sc) + ["--idents", "A"]).exit_code == 2
    monkeypatch.setattr(report, "MAX_PERM_CELLS", 3)
    r = _run(_args(tmp_path, sc))
    assert isinstance(r.exception, ValueError) and "3 tested cells: diff_pa_len_trend takes fewer" in str(r.exception)
    assert sorted(os.listdir(tmp_path)) == ["barcode_index.csv", "pt.csv", "res.gene.pkl"]


# ---------------------------------------------------------------- the entry point's case
EP_N, EP_COLS, EP_SEED, EP_N_PERM = 161, 170, 77, 600
EP_CHUNKS = ((1, 1), (2, 255), (257, 256), (513, 88))     # p_count = 1, 255 and 256: the tile's edges; 88: masked lanes
EP_ROWS = (2, 3, 5, 65)


@functools.lru_cache(maxsize=None)
def entry_case():
    """records of 2, 3, 5 and 65 kept rows on 161 tested columns in front of 9 others: (Ks, read offsets, labels, cell
    ids, kept count rows, their offsets, positions x (int32), scores q, the oracle's records counted over 600
    permutations).  Record 0's rows have 1 and 161 nonzeros, record 1's 63, 64 and 65; record 2 is read further out
    in the cells of high score (C(0) > 0), record 3 further in (C(0) < 0); the positions reach 0 and 2^22"""
    rng = np.random.default_rng(5)
    sc = [float(v) for v in rng.integers(0, 60, EP_N)]
    sc[0], sc[1] = 0.0, 59.0
    q, _s = tt.quantise(sc)
    qa = np.array(q)
    dense, xs = [], []
    for r, R in enumerate(EP_ROWS):
        m = (rng.random((R, EP_COLS)) < 0.3) * rng.integers(1, 6, (R, EP_COLS))
        x = np.sort(rng.choice(MAX_X + 1, R, replace=False))
        x[0], x[-1] = 0, MAX_X
        if r == 0:
            m[0, :EP_N], m[1, :EP_N] = 0, rng.integers(1, 6, EP_N)
            m[0, 100] = 7
        if r == 1:
            for i, k in enumerate((63, 64, 65)):
                m[i, :EP_N] = 0
                m[i, rng.choice(EP_N, k, replace=False)] = rng.integers(1, 6, k)
        if r >= 2:                       # row i's reads lean to the cells of high (record 2) or low (record 3) score
            lean = (qa / qa.max()) if r == 2 else 1 - qa / qa.max()
            for i in range(R):
                w = (i + 1) / R
                m[i, :EP_N] = (rng.random(EP_N) < 0.1 + 0.5 * (w * lean + (1 - w) * (1 - lean))) * rng.integers(1, 6, EP_N)
        m[m[:, :EP_N].sum(axis=1) == 0, 0] = 1       # every row is kept
        dense.append(m)
        xs.append(x)
    Ks = np.array(EP_ROWS, dtype=np.int32)
    lab, cb, off = [], [], [0]
    for m in dense:
        i, j = np.nonzero(m)
        rep = m[i, j]
        i, j = np.repeat(i, rep), np.repeat(j, rep)
        mixo = rng.permutation(len(i))
        lab.append(i[mixo])
        cb.append(j[mixo])
        off.append(off[-1] + len(i))
    lab, cb = np.concatenate(lab).astype(np.int64), np.concatenate(cb).astype(np.int64)
    rows = np.arange(int(Ks.sum()), dtype=np.int64)
    roff = np.concatenate([[0], np.cumsum(Ks)]).astype(np.int64)
    recs = []
    for r, m in enumerate(dense):
        nzs = [[(j, int(v)) for j, v in enumerate(row[:EP_N].tolist()) if v] for row in m]
        recs.append(LenTrendRec(f"rec{r}", nzs, xs[r].tolist(), q))
    count_permutations(recs, EP_SEED, range(1, EP_N_PERM + 1), q)
    x = np.ascontiguousarray(np.concatenate(xs), dtype=np.int32)
    return Ks, np.array(off, np.int64), lab, cb, rows, roff, x, q, recs


def test_entry_case_is_not_degenerate():
    """the oracle alone, without a GPU: the shapes the case promises, both signs of C(0), and counts that a wrong
    comparison would move"""
    _Ks, _off, _lab, _cb, _rows, roff, x, q, recs = entry_case()
    assert [len(r.nzs) for r in recs] == list(EP_ROWS) and np.diff(roff).tolist() == list(EP_ROWS)
    nnz = [len(nz) for r in recs for nz in r.nzs]
    assert nnz[:5] == [1, 161, 63, 64, 65]
    assert recs[2].C0 > 0 > recs[3].C0 and recs[2].n_ge < 6 and recs[3].n_ge < 6
    assert any(30 < r.n_ge < EP_N_PERM - 30 for r in recs[:2]), [r.n_ge for r in recs]
    assert x.min() == 0 and x.max() == MAX_X and max(q) <= 1 << 15
    assert sum(pc for _pf, pc in EP_CHUNKS) == EP_N_PERM and [pf for pf, _pc in EP_CHUNKS] == [1, 2, 257, 513]
    for r in recs:                       # every permutation's sign is used: the test is two-sided
        assert any(c > 0 for c in r.Cp.values()) and any(c < 0 for c in r.Cp.values())


def _outs(n_rows, n_rec):
    return dict(t=np.full(n_rows, -1, np.int64), s0=np.full(n_rows, -1, np.int64), sq0=np.full(n_rows, -1, np.int64),
                c0=np.full(2 * n_rec, -1, np.int64), n_ge=np.zeros(n_rec, np.int64))


def _call(ctx, roff, rows, x, o):
    from scape_amd._lib import P_i32, P_i64, ptr
    return ctx.lib.scape_hip_report_perm_len_trend(ctx.h, len(roff) - 1, ptr(roff, P_i64), ptr(rows, P_i64), ptr(x, P_i32),
                                                   ptr(o["t"], P_i64), ptr(o["s0"], P_i64), ptr(o["sq0"], P_i64),
                                                   ptr(o["c0"], P_i64), ptr(o["n_ge"], P_i64))


def _want(recs, perms=None):
    return dict(t=[v for r in recs for v in r.t], s0=[v for r in recs for v in r.s0],
                sq0=[v for r in recs for v in r.sq0], c0=[h for r in recs for h in r.halves()],
                n_ge=[r.n_ge if perms is None else sum(abs(r.Cp[p]) >= abs(r.C0) for p in perms) for r in recs])


@pytest.mark.gpu
def test_entry_point_and_chunk_independence():
    """scape_hip_report_perm_len_trend on the hand-made matrix: t, s0, sq0, both halves of C(0) and n_ge EQUAL the
    oracle's, in one call of 600 permutations and added up over chunks of 1, 255, 256 and 88 permutations, and every
    chunk on its own equals the oracle's count over its permutations"""
    from scape_amd import _lib
    from scape_amd._lib import check as chk
    Ks, off, lab, cb, rows, roff, x, q, recs = entry_case()
    ctx = _lib.default_context(None)
    try:
        rc.device_counts(ctx, Ks, off, lab, cb, EP_COLS)
        chk(tt._scores_call(ctx, q, 1, EP_N_PERM, EP_SEED), "perm_scores")
        one = _outs(len(rows), len(Ks))
        chk(_call(ctx, roff, rows, x, one), "perm_len_trend")
        parts = _outs(len(rows), len(Ks))
        for p_first, p_count in EP_CHUNKS:
            chk(tt._scores_call(ctx, q, p_first, p_count, EP_SEED), "perm_scores")
            alone = _outs(len(rows), len(Ks))
            chk(_call(ctx, roff, rows, x, alone), "perm_len_trend")
            chk(_call(ctx, roff, rows, x, parts), "perm_len_trend")
            want = _want(recs, range(p_first, p_first + p_count))
            for name, w in want.items():
                print("chunk", p_first, p_count, name, alone[name].tolist()[:6], w[:6])
                assert alone[name].tolist() == w, (p_first, p_count, name)
    finally:
        ctx.lib.scape_hip_report_free(ctx.h)
    for o, how in ((one, "one call"), (parts, "four chunks")):
        for name, w in _want(recs).items():
            print(how, name, "equal", o[name].tolist() == w, o[name].tolist()[:6], w[:6])
            assert o[name].tolist() == w, (how, name)


# ---------------------------------------------------------------- the 128-bit path
BIG_SEED, BIG_GEN, BIG_N, BIG_ROWS, BIG_N_PERM = 9, 2, 400, 6, 300


@functools.lru_cache(maxsize=None)
def big_case():
    """one record of about 2^18 reads in 6 rows on 400 cells, the rows' positions 22 bits wide, the reads of the outer
    rows in the cells of high score (a planted lengthening): (read labels, cell ids, x, q, the oracle's record counted
    over 300 permutations)"""
    rng = np.random.default_rng(BIG_GEN)
    q, _s = tt.quantise([float(v) for v in rng.permutation(BIG_N)])
    lean = np.array(q) / max(q)
    x = np.linspace(0, MAX_X, BIG_ROWS).astype(np.int64)
    m = np.zeros((BIG_ROWS, BIG_N), dtype=np.int64)
    for i in range(BIG_ROWS):
        w = i / (BIG_ROWS - 1)
        m[i] = rng.poisson(190 * (0.1 + 0.9 * (w * lean + (1 - w) * (1 - lean))))
    i, j = np.nonzero(m)
    rep = m[i, j]
    lab, cb = np.repeat(i, rep).astype(np.int64), np.repeat(j, rep).astype(np.int64)
    nzs = [[(j, int(v)) for j, v in enumerate(row.tolist()) if v] for row in m]
    rec = LenTrendRec("big", nzs, x.tolist(), q)
    count_permutations([rec], BIG_SEED, range(1, BIG_N_PERM + 1), q)
    return lab, cb, np.ascontiguousarray(x, dtype=np.int32), q, rec


def assert_big_case_needs_128_bits():
    lab, cb, x, _q, rec = big_case()
    assert 1 << 17 < rec.T == len(lab) <= 1 << 18 and lab.nbytes + cb.nbytes <= 4 << 20
    assert position_bits(rec.T) == 22 and x.max() == MAX_X and rec.T * int(x.max()) < 1 << 48
    Sxz0 = sum(xi * si for xi, si in zip(rec.x, rec.s0))
    assert abs(rec.C0) > 1 << 64 and rec.T * Sxz0 > 1 << 63 and Sxz0 < 1 << 63
    opposite = [p for p, c in rec.Cp.items() if abs(c) >= 1 << 64 and (c < 0) != (rec.C0 < 0)]
    print("C(0) bits", rec.C0.bit_length(), "permutations of the opposite sign beyond 2^64", len(opposite))
    assert opposite


def test_big_case_needs_128_bits():
    """the oracle alone, without a GPU: |C(0)| > 2^64, T Sxz(0) alone exceeds 2^63, and a permutation has |C(p)| >= 2^64
    with the opposite sign"""
    assert_big_case_needs_128_bits()


@pytest.mark.gpu
def test_128_bit_statistic():
    """a record whose C does not fit 64 bits: both halves of C(0) and n_ge over 300 permutations EQUAL the oracle's (0:
    the planted trend is strong, so what this holds is that no |C(p)| beyond 2^64, of either sign, is taken for larger
    than |C(0)|; counts between 0 and all are held by test_entry_point_and_chunk_independence)"""
    from scape_amd import _lib
    from scape_amd._lib import check as chk
    assert_big_case_needs_128_bits()
    lab, cb, x, q, rec = big_case()
    Ks, off = np.array([BIG_ROWS], np.int32), np.array([0, len(lab)], np.int64)
    rows, roff = np.arange(BIG_ROWS, dtype=np.int64), np.array([0, BIG_ROWS], np.int64)
    ctx = _lib.default_context(None)
    try:
        rc.device_counts(ctx, Ks, off, lab, cb, BIG_N)
        chk(tt._scores_call(ctx, q, 1, BIG_N_PERM, BIG_SEED), "perm_scores")
        o = _outs(BIG_ROWS, 1)
        chk(_call(ctx, roff, rows, x, o), "perm_len_trend")
    finally:
        ctx.lib.scape_hip_report_free(ctx.h)
    for name, w in _want([rec]).items():
        print(name, o[name].tolist(), w)
        assert o[name].tolist() == w, name


# ---------------------------------------------------------------- refusals
@pytest.mark.gpu
def test_entry_point_refusals():
    """no counts, no scores call, a position below 0 or above 2^22, offsets that do not start at 0, decrease or end
    nowhere, a row out of range, a missing pointer and scores wider than the count matrix: non-zero, a message, nothing
    written and nothing added; the context then serves the next call, whose results equal the oracle's"""
    from scape_amd import _lib
    from scape_amd._lib import check as chk
    Ks, off, lab, cb, rows, roff, x, q, recs = entry_case()
    ctx = _lib.default_context(None)
    o = _outs(len(rows), len(Ks))

    def refused(word, roff_=roff, rows_=rows, x_=x):
        assert _call(ctx, roff_, rows_, x_, o) != 0 and word in _lib.last_error(), (word, _lib.last_error())
    try:
        refused("report_counts")
        rc.device_counts(ctx, Ks, off, lab, cb, EP_COLS)
        refused("perm_scores")
        chk(tt._scores_call(ctx, q, 1, 10, EP_SEED), "perm_scores")
        for k, v in ((3, -1), (len(x) - 1, MAX_X + 1), (0, -(1 << 31))):
            bad = x.copy()
            bad[k] = v
            refused("2^22", x_=bad)
        bad = roff.copy()
        bad[0] = 1
        refused("start at 0", roff_=bad)
        bad = roff.copy()
        bad[2] = bad[1] - 1
        refused("non-decreasing", roff_=bad)
        bad = roff.copy()
        bad[-1] = 0
        refused("rec_row_off", roff_=bad)
        bad = rows.copy()
        bad[5] = int(Ks.sum())
        refused("out of range", rows_=bad)
        assert ctx.lib.scape_hip_report_perm_len_trend(ctx.h, len(Ks), *([None] * 8)) != 0
        assert "bad argument" in _lib.last_error()
        wide = np.ascontiguousarray(np.resize(q, EP_COLS + 1), dtype=np.uint16)
        chk(tt._scores_call(ctx, wide, 1, 10, EP_SEED), "perm_scores")
        refused("fewer columns")
        assert all(np.all(o[k] == -1) for k in ("t", "s0", "sq0", "c0")) and not o["n_ge"].any()
        chk(tt._scores_call(ctx, q, 1, 10, EP_SEED), "perm_scores")
        chk(_call(ctx, roff, rows, x, o), "perm_len_trend")
    finally:
        ctx.lib.scape_hip_report_free(ctx.h)
    for name, w in _want(recs, range(1, 11)).items():
        assert o[name].tolist() == w, name


# ---------------------------------------------------------------- the command on the synthetic directory
SYN_N_PERM = 199
PLANTED = ("GENE0", "GENE1", "GENE2", "GENE_LEN")


@functools.lru_cache(maxsize=None)
def _syn(ranked=False):
    """rc.synthetic() and tt._syn_scores() (cluster A's cells get the low scores, and records 0..3 use their first,
    innermost site more in A: their 3'UTRs lengthen along the score - GENE3's by 57 nucleotides among sites 640 apart,
    too little for 199 permutations; some cells NA, empty or nan) with three records more: GENE_FLAT has three sites at
    ONE position and is left out, GENE_ONE has all its reads in one scored cell, so the score has no variance over its
    reads, and in GENE_LEN a read lies the further out the higher its cell's score: a planted lengthening"""
    records, bc, _clu = rc.synthetic()
    text = tt._syn_scores(ranked)
    scored = {i for i, v in tt.parse_scores(text).items() if v is not None}
    ids = rc.column_ids(bc)
    rng = np.random.default_rng(31)
    some = np.array([i for i in ids if i in scored][:200], dtype=np.int64)
    flat = dict(gene_info_str="2:GENE_FLAT:1:90100-90900:+", K=3, alpha_arr=np.array([300, 300, 300]),
                beta_arr=np.array([5.0, 7.5, 10.0]), label_arr=rng.integers(0, 3, 400).astype(np.int64),
                cb_id_arr=some[rng.integers(0, len(some), 400)])
    one = dict(gene_info_str="3:GENE_ONE:1:91100-91900:-", K=3, alpha_arr=np.array([40, 300, 650]),
               beta_arr=np.array([5.0, 7.5, 10.0]), label_arr=rng.integers(0, 4, 60).astype(np.int64),
               cb_id_arr=np.full(60, some[17], dtype=np.int64))
    sc = tt.parse_scores(text)
    u = np.argsort(np.argsort([sc[int(i)] for i in some])) / len(some)
    cell = rng.integers(0, len(some), 600)
    grow = dict(gene_info_str="4:GENE_LEN:2:92100-92900:+", K=4, alpha_arr=np.array([50, 250, 450, 700]),
                beta_arr=np.array([5.0, 7.5, 10.0, 5.0]), cb_id_arr=some[cell],
                label_arr=np.minimum(3, (4 * (0.6 * u[cell] + 0.4 * rng.random(600))).astype(np.int64)))
    return list(records) + [flat, one, grow], bc, text


@functools.lru_cache(maxsize=None)
def _syn_lines(ranked, rank, n_perm=SYN_N_PERM, seed=1):
    records, bc, text = _syn(ranked)
    return oracle(records, bc, text, rank, n_perm, seed)


def test_synthetic_case_has_a_planted_trend_and_null_genes():
    """the oracle alone, without a GPU: the planted records have n_ge = 0 and lengthen along the score, a null record
    has n_ge > n_perm / 10, GENE6 (K = 1) and GENE_FLAT (one position) have no line, GENE_ONE has one without slope,
    and cells without a score exist"""
    for ranked in (False, True):
        lines = _syn_lines(ranked, ranked)
        by = {ln["gene"].split(":")[1]: ln for ln in lines}
        assert "GENE6" not in by and "GENE_FLAT" not in by and len(by) >= 30
        for g in PLANTED:
            assert by[g]["ge"] == 0 and by[g]["delta"] > 0 and by[g]["C0"] > 0, (g, by[g]["ge"])
        assert by["GENE3"]["delta"] > 0
        null = [ln["ge"] for g, ln in by.items() if g not in PLANTED + ("GENE3", "GENE_ONE")]
        assert max(null) > SYN_N_PERM / 10 and min(null) < SYN_N_PERM, sorted(null)
        assert by["GENE_ONE"]["Vz"] == 0 and by["GENE_ONE"]["ge"] == SYN_N_PERM and "slope" not in by["GENE_ONE"]
        assert any(ln["C0"] < 0 for ln in lines)
    text = tt._syn_scores()
    assert ",NA\n" in text and ",\n" in text and ",nan\n" in text


def _write_syn(root, ranked):
    from scape.apa_core import Parameters
    records, bc, text = _syn(ranked)
    return rc.write_dir(str(root), "res.gene.pkl", records, bc, {"pt.csv": text}, Parameters)[0]


@pytest.mark.gpu
@pytest.mark.parametrize("ranked", [False, True], ids=["scores", "rank"])
def test_synthetic_directory(tmp_path, monkeypatch, ranked):
    """199 permutations of the scored cells of the synthetic directory: every line of the file against the exact
    oracle (integers and p-values as text, the float columns through rc.close), the planted records' p-value is 1 / 200,
    GENE6 and GENE_FLAT are absent and GENE_ONE has empty slope, delta_pos and r; the same bytes come back with the
    permutations in several chunks and the records in several batches, whose permuted scores are diff_pa_trend's; no
    .part file is left.  rank: the same with --rank on a score file that is its own rank transform"""
    from scape_amd import _lib, report
    lines = _syn_lines(ranked, ranked)
    path = _write_syn(tmp_path, ranked)
    text = _command(tmp_path, path, "res.gene.pkl", ranked, SYN_N_PERM, 1, "syn")
    compare(text, lines, SYN_N_PERM, "syn")
    genes = {r[0].split(":")[1]: r for r in list(csv.reader(io.StringIO(text)))[1:]}
    assert "GENE6" not in genes and "GENE_FLAT" not in genes
    assert genes["GENE_ONE"][5:10] == ["", "", "", str(SYN_N_PERM), "1.0"]
    for g in PLANTED:
        assert genes[g][9] == repr(1 / 200) and float(genes[g][6]) > 0, g
    assert os.path.basename(_path(tmp_path, path, "res.gene.pkl", ranked)) == \
        ("pt.gene.rank.diff_pa_len_trend.csv" if ranked else "pt.gene.diff_pa_len_trend.csv")
    if ranked:
        assert _command(tmp_path, path, "res.gene.pkl", False, SYN_N_PERM, 1, "syn/plain") == text
    lib = _lib.load_library()
    calls = {"scores": [], "test": 0}
    real_s, real_t = lib.scape_hip_report_perm_scores, lib.scape_hip_report_perm_len_trend

    def make_scores(*a):
        calls["scores"].append((a[3], a[4], a[5]))
        return real_s(*a)

    def test(*a):
        calls["test"] += 1
        return real_t(*a)
    monkeypatch.setattr(lib, "scape_hip_report_perm_scores", make_scores)
    monkeypatch.setattr(lib, "scape_hip_report_perm_len_trend", test)
    n = len([v for v in tt.parse_scores(_syn(ranked)[2]).values() if v is not None])
    monkeypatch.setattr(report, "MAX_BATCH_BYTES", 1 << 16)             # a record of K = 8 alone takes 57 KB
    monkeypatch.setattr(report, "MAX_PERM_BYTES", 6 * n * 80)           # 6 bytes per tested cell: 80 permutations
    assert _command(tmp_path, path, "res.gene.pkl", ranked, SYN_N_PERM, 1, "syn/chunks") == text
    assert calls["scores"][:3] == [(1, 80, 1), (81, 80, 1), (161, 39, 1)] and calls["test"] > 3 * 5
    assert calls["test"] == len(calls["scores"]) and not rc.parts_left(tmp_path)
