"""`scape diff_pa_len`: the permutation test of a record's mean pA position (3'UTR length) between two cell populations
(scape_amd/report.py, section diff_pa_len; kernel k_rep_perm_len and entry point scape_hip_report_perm_len of
scape_amd/csrc/perm.inc).

The contract.  Populations, tested columns (population 1's, then population 2's), kept rows (labels < K with a read in a
tested column, in label order) and permutations (permutation p >= 1 gives population 1 the n1 positions with the smallest
key(p, j)) are `diff_pa`'s: tests/test_report_diffpa.py states them, and the mix / key / members / bh / populations of
tests/report_cases.py are used here.  Kept row i has the position x_i = alpha_arr[label_i] (f64; nucleotides from the UTR's 5' end along the
transcript, so larger = more distal = longer 3'UTR).  With a_i the row's sum over population 1 under a labelling,
b_i = t_i - a_i, A = sum a_i, B = sum b_i:

    mean_pos.1 = sum a_i x_i / A,   mean_pos.2 = sum b_i x_i / B,   delta = mean_pos.1 - mean_pos.2   (0 if A B = 0)

n_ge = #{p in 1..n_perm: |delta(p)| >= |delta(0)| - tol}, tol = 2^-40 span, span = max x_i - min x_i over the kept
rows; p_val = (1 + n_ge) / (1 + n_perm), Benjamini-Hochberg over the file's lines.  A record is tested when K > 1, two
kept rows or more remain, both populations have reads in it and span > 0; a non-finite position of a kept row of any
record with K > 1 is a ValueError.  exp_length.1 / .2 are the reference's expected pA length (1 + 9 (a - a[0]) / (a[-1] - a[0]) weighted by
the population's reads over ALL K labels).

The oracle below restates this in exact arithmetic and imports nothing from scape_amd: Fraction(float(alpha)) for the
positions, Python ints for every sum, `members()` for the labellings; the comparison per permutation is the
cross-multiplied integer form of the Fraction comparison (test_affine_maps_complement_and_integer_form checks that
claim on Fractions).  Per record it gives lo = #{|delta(p)| >= |delta(0)|} and hi = #{|delta(p)| >= |delta(0)| -
2^-39 span} (twice the device's tol); every GPU test first asserts lo == hi for every record of its case on the oracle
alone, then that the file's n_ge EQUALS lo.  No record is excused.  The device's rounding stays below half of tol for
up to 1,024 rows per record (include/scape_hip.h), so a labelling that reaches the observed |delta| exactly is always
counted and one more than 2 tol below it never."""
import csv
import functools
import io
import math
import os
import pickle
from fractions import Fraction

import numpy as np
import pytest

import report_cases as rc
from report_cases import no_gpu, parts_left as _parts_left, run as _run  # noqa: F401  (no_gpu is a fixture)

HEADER = ("gene,versus,num_pa,reads.1,reads.2,mean_pos.1,mean_pos.2,delta_pos,exp_length.1,exp_length.2,"
          "delta_exp_length,n_ge,p_val,p_val_adj,n_perm")
BAND = 39                                 # hi counts down to |delta(0)| - 2^-39 span


# ---------------------------------------------------------------- the contract, restated
def exp_length(K, alpha, counts):
    """the reference's expected pA length of one population: its reads per label (all K labels) as weights of the
    labels' positions rescaled to 1..10; numpy, as the reference computes it (nan / inf where its formula gives them)"""
    if K == 1:
        return 1.0
    ws = np.asarray(counts, dtype=np.float64)
    if ws.sum() == 0:
        return float("nan")
    ws = ws / np.sum(ws)
    a = np.asarray(alpha)
    with np.errstate(all="ignore"):
        scale = 1.0 + 9.0 * (a - a[0]) / (a[-1] - a[0])
        return float(np.sum(ws * scale))


class LenRec:
    """a record's kept rows: per row its nonzeros [(position j, count)] among the tested columns and its pA position
    x (Fraction); integers and Fractions only"""

    def __init__(self, gene, nzs, x, n1):
        self.gene, self.nzs, self.x = gene, nzs, [Fraction(v) for v in x]
        self.t = [sum(v for _j, v in nz) for nz in nzs]
        self.T = sum(self.t)
        self.a0 = [sum(v for j, v in nz if j < n1) for nz in nzs]
        self.span = max(self.x) - min(self.x)
        self.D = math.lcm(*(v.denominator for v in self.x))
        self.X = [int(v * self.D) for v in self.x]                       # x_i = X_i / D
        self.SPAN = int(self.span * self.D)
        self.XT = sum(ti * Xi for ti, Xi in zip(self.t, self.X))
        self.N0, self.ab0 = self.stat(self.a0)
        self.lo = self.hi = 0

    def tested(self):
        A = sum(self.a0)
        return len(self.nzs) >= 2 and A > 0 and self.T - A > 0 and self.span > 0

    def row_sums(self, member):
        return [sum(v for j, v in nz if member[j]) for nz in self.nzs]

    def means(self, a):
        """(mean_pos.1, mean_pos.2) as Fractions, straight from the definition; None for an empty population"""
        A = sum(a)
        B = self.T - A
        m1 = sum(ai * xi for ai, xi in zip(a, self.x)) / A if A else None
        m2 = sum((ti - ai) * xi for ai, ti, xi in zip(a, self.t, self.x)) / B if B else None
        return m1, m2

    def delta(self, a):
        m1, m2 = self.means(a)
        return Fraction(0) if m1 is None or m2 is None else m1 - m2

    def stat(self, a):
        """(N, A B) with delta = N / (A B D); (0, 1) when A B = 0"""
        A = sum(a)
        B = self.T - A
        if A == 0 or B == 0:
            return 0, 1
        s1 = sum(ai * Xi for ai, Xi in zip(a, self.X))
        return s1 * B - (self.XT - s1) * A, A * B

    def count(self, member):
        N, ab = self.stat(self.row_sums(member))
        # |N| / (ab D) >= |N0| / (ab0 D) - c SPAN / D for c = 0 and c = 2^-BAND, times ab ab0 D 2^BAND (positive)
        self.lo += abs(N) * self.ab0 >= abs(self.N0) * ab
        self.hi += (abs(N) * self.ab0) << BAND >= ((abs(self.N0) << BAND) - self.SPAN * self.ab0) * ab


def oracle(recs, cols1, cols2, n_perm, seed):
    """recs: [dict(gene, K, alpha, dense = counts [K, every matrix column])] in file order.  Returns the expected lines:
    dicts of the text columns, the exact counts lo / hi and the Fractions of the float columns"""
    cols = np.array(list(cols1) + list(cols2), dtype=np.int64)
    n1, n = len(cols1), len(cols)
    assert n1 >= 1 and n - n1 >= 1 and n < 1 << 24
    live = []
    for rec in recs:
        K = int(rec["K"])
        sub = np.asarray(rec["dense"])[:, cols]
        kept = [l for l in range(K) if sub[l].any()]
        if K == 1 or len(kept) < 2:
            continue
        nzs = [[(j, int(v)) for j, v in enumerate(sub[l].tolist()) if v] for l in kept]
        r = LenRec(rec["gene"], nzs, [Fraction(float(rec["alpha"][l])) for l in kept], n1)
        if r.tested():
            assert r.T < 1 << 31 and len(kept) <= 1024
            r.e1 = exp_length(K, rec["alpha"], sub[:, :n1].sum(axis=1))
            r.e2 = exp_length(K, rec["alpha"], sub[:, n1:].sum(axis=1))
            live.append(r)
    for p in range(1, n_perm + 1):
        member = bytearray(n)
        pop1 = rc.members(seed, p, n1, n)
        assert len(set(pop1)) == n1
        for j in pop1:
            member[j] = 1
        for r in live:
            r.count(member)
    lines = []
    for r in live:
        m1, m2 = r.means(r.a0)
        assert m1 - m2 == Fraction(r.N0, r.ab0 * r.D) == r.delta(r.a0)
        with np.errstate(invalid="ignore"):
            de = float(np.float64(r.e1) - np.float64(r.e2))
        lines.append(dict(gene=r.gene, num_pa=len(r.nzs), A=sum(r.a0), B=r.T - sum(r.a0), m1=m1, m2=m2, delta=m1 - m2,
                          e1=repr(r.e1), e2=repr(r.e2), de=repr(de), lo=r.lo, hi=r.hi))
    for ln, adj in zip(lines, rc.bh([Fraction(1 + ln["lo"], 1 + n_perm) for ln in lines])):
        ln["p_adj"] = adj
    return lines


def assert_no_near_tie(lines, what):
    """lo == hi for every record: no permutation's |delta| lies within 2^-39 span below the observed one, so the
    device's f64 comparison (band 2^-40 span) can hide nothing"""
    for ln in lines:
        assert ln["lo"] == ln["hi"], (what, ln["gene"], ln["lo"], ln["hi"])


def compare(text, lines, versus, n_perm, what):
    rows = list(csv.reader(io.StringIO(text)))
    assert ",".join(rows[0]) == HEADER
    body = rows[1:]
    print(what, "lines", len(body), "expected", len(lines))
    assert len(body) == len(lines), what
    for got, ln in zip(body, lines):
        ctx = (what, ln["gene"], got)
        assert got[0] == ln["gene"] and got[1] == versus and got[14] == str(n_perm), ctx
        assert got[2:5] == [str(ln["num_pa"]), str(ln["A"]), str(ln["B"])], ctx
        assert got[11] == str(ln["lo"]), ctx
        assert got[12] == repr((1 + ln["lo"]) / (1 + n_perm)), ctx
        assert got[8:11] == [ln["e1"], ln["e2"], ln["de"]], (ctx, ln["e1"], ln["e2"], ln["de"])
        for col, want in ((5, ln["m1"]), (6, ln["m2"]), (7, ln["delta"]), (13, ln["p_adj"])):
            assert rc.close(got[col], want), (ctx, col, float(want))


# ---------------------------------------------------------------- inputs
def read_records(path):
    """the records of a result stream as plain dicts (input plumbing: the fields the command itself reads)"""
    out = []
    with open(path, "rb") as fh:
        while True:
            try:
                p = pickle.load(fh)
            except EOFError:
                return out
            out.append(dict(gene_info_str=p.gene_info_str, K=int(p.K), alpha_arr=np.asarray(p.alpha_arr),
                            label_arr=np.asarray(p.label_arr), cb_id_arr=np.asarray(p.cb_id_arr)))


def dense_of(records, col_ids):
    """[dict(gene, K, alpha, dense)]: per record the (label < K, matrix column) read counts"""
    return [dict(gene=rec["gene_info_str"], K=int(rec["K"]), alpha=np.asarray(rec["alpha_arr"]), dense=m)
            for rec, m in zip(records, rc.dense_counts(records, col_ids))]


def _args(root, clu, res="res.gene.pkl", id1=None, id2=None, n_perm=None, seed=None, cmd="diff_pa_len"):
    return rc.perm_args(cmd, root, clu, res, id1, id2, n_perm, seed)


def _path(root, clu, res, id1, id2):
    return rc.perm_path("diff_pa_len", root, clu, res, id1, id2)


def _command(root, clu, res, id1, id2, n_perm, seed, what=""):
    return rc.perm_command("diff_pa_len", root, clu, res, id1, id2, n_perm, seed, what)


def check(root, clu_path, clu_text, res, recs, bc, id1, id2, n_perm, seed, what):
    """oracle first (and lo == hi on it), then the command; returns (file text, expected lines)"""
    c1, c2 = rc.populations(bc, clu_text, id1, id2)
    lines = oracle(recs, c1, c2, n_perm, seed)
    assert_no_near_tie(lines, what)
    text = _command(root, clu_path, res, id1, id2, n_perm, seed, what)
    compare(text, lines, f"{id1}_Vs_{id2}" if id2 is not None else id1, n_perm, what)
    return text, lines


# ---------------------------------------------------------------- CPU
def _host():
    from scape_amd import report
    return report


def test_hand_worked_record():
    """two sites at 100 and 300 nt, five cells (two in population 1).  Counts of site 1 / site 2 per cell:
    (3, 1) (1, 0) | (0, 2) (1, 1) (0, 4).  Population 1: 4 and 1 reads, mean (400 + 300) / 5 = 140; population 2: 1 and
    7 reads, mean (100 + 2100) / 8 = 275; delta = -135: population 1's 3'UTRs are shorter.  Of the C(5, 2) = 10
    labellings, by hand: {0,2} has 3 + 3 reads, mean 200, against 2 + 5, mean 1700/7: delta -300/7; {0,3} has 4 + 2, mean
    500/3, against 1 + 6, mean 1900/7: -2200/21; {0,4} has 3 + 5, mean 225, against 2 + 3, mean 220: +5; beside the
    observed {0,1} only {2,4} (the two cells with reads at site 2 alone: mean 300 against (500 + 600) / 7, delta
    +1000/7 = 142.9) reaches 135"""
    x = [100.0, 300.0]
    site1, site2 = [3, 1, 0, 1, 0], [1, 0, 2, 1, 4]
    nzs = [[(j, v) for j, v in enumerate(row) if v] for row in (site1, site2)]
    r = LenRec("g", nzs, x, 2)
    assert r.tested() and r.t == [5, 8] and r.a0 == [4, 1] and r.span == 200
    assert r.means(r.a0) == (Fraction(140), Fraction(275)) and r.delta(r.a0) == -135
    deltas = {}
    for i in range(5):
        for j in range(i + 1, 5):
            member = [k in (i, j) for k in range(5)]
            deltas[(i, j)] = r.delta(r.row_sums(member))
            r.count(member)
    assert deltas[(0, 1)] == -135 and deltas[(0, 2)] == Fraction(-300, 7) and deltas[(2, 4)] == Fraction(1000, 7)
    assert deltas[(0, 3)] == Fraction(-2200, 21) and deltas[(0, 4)] == 5
    assert sorted(k for k, d in deltas.items() if abs(d) >= 135) == [(0, 1), (2, 4)]
    assert (r.lo, r.hi) == (2, 2)
    # a labelling that leaves a population without reads has delta 0
    assert LenRec("g", [[(1, 1)], [(1, 2)]], x, 1).delta([0, 0]) == 0
    # the command's own host arithmetic and header say the same
    rep = _host()
    assert ",".join(rep.DIFF_PA_LEN_HEADER) == HEADER
    assert rep._mean_positions(np.array(x), [4, 1], [1, 7]) == (140.0, 275.0, -135.0)
    m = rep._mean_positions(np.array([0.1, 0.7, 2.5]), [1, 2, 4], [3, 0, 1])
    fx = [Fraction(0.1), Fraction(0.7), Fraction(2.5)]
    m1, m2 = (fx[0] + 2 * fx[1] + 4 * fx[2]) / 7, (3 * fx[0] + fx[2]) / 4
    assert m == (float(m1), float(m2), float(m1 - m2))


def test_affine_maps_complement_and_integer_form():
    """n_ge (lo) does not change when every x becomes c x + d (c != 0: the reference's 1..10 scale is one such map, a
    negative c mirrors the UTR), the complementary labelling gives -delta, and the integer comparisons of LenRec.count
    are the Fraction comparisons of the definition"""
    rng = np.random.default_rng(17)
    n1, n, n_perm, seed = 7, 19, 80, 4
    x = [12.0, 57.0, 58.0, 301.5, 1020.0]
    rows = [((rng.random(n) < 0.6) * rng.integers(1, 5, n)).tolist() for _ in x]
    nzs = [[(j, v) for j, v in enumerate(row) if v] for row in rows]
    labellings = []
    for p in range(1, n_perm + 1):
        pop1 = set(rc.members(seed, p, n1, n))
        labellings.append([j in pop1 for j in range(n)])

    def run(xs):
        r = LenRec("g", nzs, xs, n1)
        assert r.tested()
        d0 = abs(r.delta(r.a0))
        lo = hi = 0
        for member in labellings:
            r.count(member)
            d = abs(r.delta(r.row_sums(member)))
            lo += d >= d0
            hi += d >= d0 - r.span / (1 << BAND)
        assert (r.lo, r.hi) == (lo, hi)                      # integer form == Fraction form
        return r

    base = run([Fraction(v) for v in x])
    assert 0 < base.lo < n_perm                              # the case exercises both outcomes
    span = Fraction(x[-1]) - Fraction(x[0])
    for c, d in ((Fraction(9) / span, 1 - 9 * Fraction(x[0]) / span), (Fraction(-3, 7), Fraction(5, 3)),
                 (Fraction(1), Fraction(-10 ** 6)), (Fraction(1 << 20), Fraction(0))):
        r = run([c * Fraction(v) + d for v in x])
        assert r.lo == base.lo and r.delta(r.a0) == c * base.delta(base.a0), (c, d)
    for member in labellings[:20] + [[j < n1 for j in range(n)]]:
        a = base.row_sums(member)
        comp = base.row_sums([not m for m in member])
        assert comp == [ti - ai for ti, ai in zip(base.t, a)] and base.delta(comp) == -base.delta(a)
    # the host's means follow an exactly representable map exactly
    rep = _host()
    a, b = base.a0, [ti - ai for ti, ai in zip(base.t, base.a0)]
    m1, m2, dl = rep._mean_positions(np.array(x), a, b)
    assert (m1, m2, dl) == tuple(float(v) for v in (*base.means(a), base.delta(a)))
    k1, k2, kd = rep._mean_positions(np.array(x) * 4.0 - 1024.0, a, b)
    assert kd == float(4 * base.delta(a)) and k1 == float(4 * base.means(a)[0] - 1024)


def test_help_lists_command_and_options():
    r = _run(["--help"])
    assert r.exit_code == 0 and "diff_pa_len" in r.output
    r = _run(["diff_pa_len", "--help"])
    assert r.exit_code == 0, r.output
    for o in ("--output_dir", "--res_pkl_file", "--cell_cluster_file", "--idents_1", "--idents_2", "--n_perm", "--seed"):
        assert o in r.output
    flat = " ".join(r.output.split())
    assert "[default: 9999]" in flat and "[default: 1]" in flat
    assert "same relabellings of the cells as in diff_pa" in flat      # one seed, one set of labellings in both commands


def test_utils_import_path():
    import scape.utils as su
    assert su.diff_pa_len is _host().diff_pa_len


def test_prerequisites_and_argument_errors(tmp_path, no_gpu):
    """diff_pa's list of errors, each raised by both commands with the same exception before the device is opened"""
    clu = tmp_path / "groups.csv"

    def both(root, **kw):
        a, b = _run(_args(root, clu, cmd="diff_pa", **kw)), _run(_args(root, clu, **kw))
        assert type(a.exception) is type(b.exception) and str(a.exception) == str(b.exception), (a.exception, b.exception)
        assert b.exit_code != 0
        return b

    assert "Given output_dir folder does not exists." in str(both(tmp_path / "nope", id1="A").exception)
    assert "Given res_pkl_file is not in output_dir." in str(both(tmp_path, id1="A").exception)
    (tmp_path / "res.gene.pkl").write_bytes(b"")
    assert "Given cell_cluster_file file does not exists" in str(both(tmp_path, id1="A").exception)
    clu.write_text("index,group\n3,A\n4,B\n5,\n77,ghost\n")
    r = both(tmp_path, id1="A")
    assert isinstance(r.exception, FileNotFoundError) and "barcode_index.csv" in str(r.exception)
    (tmp_path / "barcode_index.csv").write_text("CB,index\nA-1,3\nB-1,4\nC-1,5\n")
    for kw, word in ((dict(id1="A", id2="A"), "same"), (dict(id1="Z"), "'Z'"), (dict(id1="A", id2="Z"), "'Z'"),
                     (dict(id1=""), "names no cluster"), (dict(id1="A", n_perm=0), "n_perm"),
                     (dict(id1="A", n_perm=-3), "n_perm"), (dict(id1="A", seed=-1), "seed"),
                     (dict(id1="A", seed=1 << 64), "seed"), (dict(id1="ghost"), "has no cell"),
                     (dict(id1="A", id2="ghost"), "has no cell")):
        r = both(tmp_path, **kw)
        assert isinstance(r.exception, ValueError) and word in str(r.exception), (kw, repr(r.exception))
    clu.write_text("index,group\n3,A\n4,A\n5,\n")                     # nobody left for "the rest"
    r = both(tmp_path, id1="A")
    assert isinstance(r.exception, ValueError) and "has no cell" in str(r.exception)
    r = _run(["diff_pa_len", "--output_dir", str(tmp_path), "--res_pkl_file", "res.gene.pkl", "--cell_cluster_file", str(clu)])
    assert r.exit_code == 2 and "--idents_1" in r.output
    r = _run(["diff_pa_len", "--output_dir", str(tmp_path), "--res_pkl_file", "res.gene.pkl", "--idents_1", "A"])
    assert r.exit_code == 2 and "--cell_cluster_file" in r.output
    assert sorted(os.listdir(tmp_path)) == ["barcode_index.csv", "groups.csv", "res.gene.pkl"]


# ---------------------------------------------------------------- GPU: golden cases
def _golden_dense(cs, n_cols):
    """the reference's own matrix rows (tests/golden/fixture_report.npz) as per-record [K, column] counts: a record's
    rows are its labels < K that have a read, in label order; the other labels have none"""
    _pas, vals = rc.dense_of_body(cs["mat_body"], n_cols)
    out, k = [], 0
    for rec in cs["records"]:
        K = int(rec["K"])
        lab = np.asarray(rec["label_arr"])
        labs = np.unique(lab[lab < K])
        m = np.zeros((K, n_cols), dtype=np.int64)
        m[labs] = vals[k:k + len(labs)]
        k += len(labs)
        out.append(dict(gene=rec["gene_info_str"], K=K, alpha=np.asarray(rec["alpha_arr"]), dense=m))
    assert k == len(vals)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("c,j", rc.golden_perm_params())
def test_golden_case_and_cluster_file(c, j, tmp_path):
    """every golden case and cluster file that gives two non-empty populations: the first such cluster against the
    rest, 199 permutations; n_ge equal to the exact oracle's (a case without a tested record gives the header alone)"""
    cs = rc.fixture_case(c)
    texts = rc.cluster_texts(cs)
    bc, paths = rc.write_case(cs, tmp_path)
    fn = cs["clu_files"][j]
    id1 = rc.golden_ident(bc, texts[fn])
    recs = _golden_dense(cs, len(rc.column_ids(bc)))
    check(tmp_path, paths[j], texts[fn], cs["res"], recs, bc, id1, None, 199, 1, f"{cs['name']}/{fn}")


# ---------------------------------------------------------------- GPU: the synthetic directory
@functools.lru_cache(maxsize=None)
def _syn():
    records, bc, clu_text = rc.synthetic()
    return dict(records=records, bc=bc, clu=clu_text, recs=dense_of(records, rc.column_ids(bc)))


def _sense(rows, id2, what):
    """rows: [(gene name, n_ge, delta_pos)] of the oracle or of the file.  GENE0..GENE3 have a planted excess of the
    FIRST site in cluster A and a sorted alpha_arr: A's 3'UTRs are shorter.  GENE0, GENE1 and GENE2 reach n_ge = 0 and
    no other record does.  GENE3 does not: with five sites at 87, 230, 258, 268 and 729 nt the planted first site lies
    close to three others and moves the mean by less than the cell-to-cell spread the far site causes, although
    diff_pa's chi-square puts the same record at 0 - the two tests answer different questions.  GENE5 has reads only in
    A and GENE6 has K = 1: no line"""
    by = {g: (ge, d) for g, ge, d in rows}
    assert len(by) == len(rows) == 36, what
    for g in ("GENE0", "GENE1", "GENE2"):
        assert by[g][0] == 0 and by[g][1] < 0, (what, g, by[g])
    assert [g for g, (ge, _d) in by.items() if ge == 0] == ["GENE0", "GENE1", "GENE2"], what
    assert by["GENE3"][1] < 0 and 0 < by["GENE3"][0] < 200, (what, by["GENE3"])
    assert by["GENE3"][0] == (96 if id2 else 85), (what, by["GENE3"])     # the exact oracle's count for seed 1
    assert "GENE5" not in by and "GENE6" not in by, what


@pytest.mark.gpu
@pytest.mark.parametrize("id2", ["B", None], ids=["A_vs_B", "A_vs_rest"])
def test_synthetic_directory(id2, tmp_path):
    """999 permutations of 230 + 301 cells (with --idents_2) and of 230 + 341 (without): parity with the exact oracle,
    and sense, asserted on the oracle first and then on the file"""
    s = _syn()
    path = rc.write_synthetic(tmp_path)
    text, lines = check(tmp_path, path, s["clu"], "res.gene.pkl", s["recs"], s["bc"], "A", id2, 999, 1, f"syn/{id2}")
    assert max(ln["num_pa"] for ln in lines) == 63                        # the K = 63 record keeps all its rows
    _sense([(ln["gene"].split(":")[1], ln["lo"], ln["delta"]) for ln in lines], id2, "oracle")
    body = list(csv.reader(io.StringIO(text)))[1:]
    _sense([(r[0].split(":")[1], int(r[11]), float(r[7])) for r in body], id2, "file")
    assert {r[12] for r in body if r[0].split(":")[1] in ("GENE0", "GENE1", "GENE2")} == {repr(1 / 1000)}


@pytest.mark.gpu
@pytest.mark.parametrize("n_perm", [1, 255, 256, 257])
def test_tile_edges(n_perm, tmp_path):
    """a workgroup of the kernel takes 256 permutations: one short of a tile, a full tile, one over, and one"""
    s = _syn()
    path = rc.write_synthetic(tmp_path, 12)
    _text, lines = check(tmp_path, path, s["clu"], "res.gene.pkl", s["recs"][:12], s["bc"], "C", "A", n_perm, 5,
                         f"tile/{n_perm}")
    assert len(lines) == 10


@pytest.mark.gpu
@pytest.mark.parametrize("n_cells,n_a", [(64, 1), (64, 63), (64, 32), (65, 1), (130, 129), (2, 1)],
                         ids=["64-1", "64-63", "64-32", "65-1", "130-129", "2-1"])
def test_small_and_lopsided_populations(n_cells, n_a, tmp_path):
    """populations of 1 cell and of n - 1 cells, n = 64 exactly, one over, and the smallest n (where every labelling
    ties with the observed one exactly)"""
    path, clu_text, bc, _records, _ids = rc.small_dir(tmp_path, n_cells, n_a, 100 + n_cells + n_a)
    recs = dense_of(read_records(os.path.join(str(tmp_path), "res.utr.pkl")), rc.column_ids(bc))
    _text, lines = check(tmp_path, path, clu_text, "res.utr.pkl", recs, bc, "A", None, 300, 9, f"small/{n_cells}/{n_a}")
    assert len(lines) == 8
    if n_cells == 2:
        assert all(ln["lo"] == 300 for ln in lines)


@pytest.mark.gpu
def test_seeds(tmp_path):
    """the same seed gives the same bytes, another seed other counts"""
    path = rc.write_synthetic(tmp_path)
    a = _command(tmp_path, path, "res.gene.pkl", "A", "B", 99, 1)
    b = _command(tmp_path, path, "res.gene.pkl", "A", "B", 99, 1)
    c = _command(tmp_path, path, "res.gene.pkl", "A", "B", 99, 2)
    assert a == b and a != c
    col = lambda text: [r[11] for r in csv.reader(io.StringIO(text))]
    assert col(a) != col(c) and len(col(a)) == len(col(c)) == 37


@pytest.mark.gpu
def test_batch_and_chunk_invariance(tmp_path, monkeypatch):
    """records split over several count batches and the permutations over several chunks: the same bytes, and the
    expected sequence of masks calls"""
    from scape_amd import _lib, report
    path = rc.write_synthetic(tmp_path)
    big = _command(tmp_path, path, "res.gene.pkl", "A", None, 999, 1)
    lib = _lib.load_library()
    calls = {"masks": [], "len": 0}
    real_m, real_l = lib.scape_hip_report_perm_masks, lib.scape_hip_report_perm_len

    def masks(*a):
        calls["masks"].append((a[3], a[4]))
        return real_m(*a)

    def length(*a):
        calls["len"] += 1
        return real_l(*a)
    monkeypatch.setattr(lib, "scape_hip_report_perm_masks", masks)
    monkeypatch.setattr(lib, "scape_hip_report_perm_len", length)
    assert _command(tmp_path, path, "res.gene.pkl", "A", None, 999, 1) == big
    assert calls["masks"] == [(1, 999)] and calls["len"] == 1
    calls.update(masks=[], len=0)
    monkeypatch.setattr(report, "MAX_BATCH_BYTES", 1 << 16)             # a record of K = 8 alone takes 57 KB
    monkeypatch.setattr(report, "MAX_PERM_BYTES", 1 << 30)
    assert _command(tmp_path, path, "res.gene.pkl", "A", None, 999, 1) == big
    assert calls["masks"] == [(1, 999)] and calls["len"] > 5
    n_batches = calls["len"]
    calls.update(masks=[], len=0)
    monkeypatch.setattr(report, "MAX_PERM_BYTES", (9 + 1) * 8 * 300)     # 9 words of 64 positions, 1 key bound: 300 permutations
    assert _command(tmp_path, path, "res.gene.pkl", "A", None, 999, 1) == big
    assert calls["len"] == 4 * n_batches and calls["masks"][:4] == [(1, 300), (301, 300), (601, 300), (901, 99)]
    assert len(calls["masks"]) == 4 * n_batches


# ---------------------------------------------------------------- GPU: exp_length, untested and refused records
def _two_group_dir(root, alphas, n_cells=40, n_a=15, gen_seed=3, only_label=None):
    """records with the given alpha_arr each (K = its length) on n_cells barcodes, the first n_a in cluster A, the others
    in B: every barcode has a cluster.  only_label = {record: label}: every read of that record carries that label"""
    from scape.apa_core import Parameters
    rng = np.random.default_rng(gen_seed)
    ids = np.arange(n_cells) * 5 + 1
    bc = "CB,index\n" + "".join(f"T{j}-1,{i}\n" for j, i in enumerate(ids.tolist()))
    clu_text = "index,group\n" + "".join(f"{i},{'A' if j < n_a else 'B'}\n" for j, i in enumerate(ids.tolist()))
    records = []
    for r, alpha in enumerate(alphas):
        K = len(alpha)
        records.append(dict(gene_info_str=f"3:TG{r}:{1 + r % 2}:{700 * r + 1}-{700 * r + 600}:{'+-'[r % 2]}", K=K,
                            alpha_arr=np.asarray(alpha), beta_arr=np.full(K, 10.0),
                            label_arr=(rng.integers(0, K + 1, 300) if r not in (only_label or {}) else  # K: no site
                                       np.full(300, only_label[r])).astype(np.int64),
                            cb_id_arr=ids[rng.integers(0, n_cells, 300)].astype(np.int64)))
    path = rc.write_dir(str(root), "res.gene.pkl", records, bc, {"two.csv": clu_text}, Parameters)[0]
    return path, clu_text, bc, dense_of(records, ids.tolist())


@pytest.mark.gpu
def test_exp_length_is_cal_exp_pa_len(tmp_path):
    """on a directory whose cluster file covers every barcode, exp_length.1 / .2 are the numbers `cal_exp_pa_len
    --cell_cluster_file` writes for clusters A and B - also for an unsorted alpha_arr, for one whose first and last
    entries are equal (the reference's formula divides by zero: inf / nan, printed as numpy gives them) and for float
    positions; a record whose kept rows share one position has no line"""
    alphas = [[30, 200, 410], [500, 20, 260, 90], [120, 480, 120], [77, 77], [10.5, 99.25, 300.0, 301.0, 580.75],
              [40, 41]]
    path, clu_text, bc, recs = _two_group_dir(tmp_path, alphas)
    text, lines = check(tmp_path, path, clu_text, "res.gene.pkl", recs, bc, "A", "B", 199, 3, "exp_length")
    assert [ln["gene"].split(":")[1] for ln in lines] == ["TG0", "TG1", "TG2", "TG4", "TG5"]     # TG3: span 0
    r = _run(["cal_exp_pa_len", "--output_dir", str(tmp_path), "--cell_cluster_file", path, "--res_pkl_file",
              "res.gene.pkl"])
    assert r.exit_code == 0, (r.output, repr(r.exception))
    with open(os.path.join(str(tmp_path), "two.gene.pa.len.csv"), newline="") as fh:
        want = {(g, c): float(e or "nan") for g, c, e, _k in list(csv.reader(fh))[1:]}       # pandas writes NaN as ""
    same = lambda a, b: a == b or (math.isnan(a) and math.isnan(b))
    body = list(csv.reader(io.StringIO(text)))[1:]
    assert len(body) == 5
    for row in body:
        gene_id = ":".join(row[0].split(":")[1:3])
        assert same(float(row[8]), want[(gene_id, "A")]) and same(float(row[9]), want[(gene_id, "B")]), row
    tg2 = [row for row in body if ":TG2:" in row[0]][0]
    assert not math.isfinite(float(tg2[8])) and tg2[10] == "nan" and 0 <= int(tg2[11]) <= 199


@pytest.mark.gpu
def test_non_finite_position_is_refused(tmp_path):
    """a NaN position of a pA site with reads: ValueError naming the record, no file left - also when that site is the
    record's only kept row, so that the record would not be tested anyway; a NaN at a site without reads is never
    looked at"""
    nan = float("nan")
    for k, (alphas, only) in enumerate((([[30, 200, 410], [25.0, nan, 300.0]], None),
                                        ([[30, 200, 410], [25.0, 60.0, nan]], {1: 2}))):
        root = tmp_path / f"d{k}"
        path, _clu, _bc, _recs = _two_group_dir(root, alphas, only_label=only)
        r = _run(_args(root, path, id1="A", id2="B", n_perm=50))
        assert isinstance(r.exception, ValueError) and "TG1" in str(r.exception), repr(r.exception)
        assert not _parts_left(root) and not os.path.exists(_path(root, path, "res.gene.pkl", "A", "B"))
    root = tmp_path / "fine"
    path, clu_text, bc, recs = _two_group_dir(root, [[30, 200, 410], [25.0, nan, 300.0]], only_label={1: 0})
    recs[1]["alpha"] = np.array([25.0, 0.0, 300.0])           # the oracle never reads that entry either
    _text, lines = check(root, path, clu_text, "res.gene.pkl", recs, bc, "A", "B", 50, 1, "nan without reads")
    assert [ln["gene"].split(":")[1] for ln in lines] == ["TG0"]


# ---------------------------------------------------------------- GPU: the entry point
def _f64_delta(a, t, w):
    """delta as the device forms it (include/scape_hip.h): f64, rows in order, no contraction"""
    W1 = W2 = 0.0
    A = B = 0
    for ai, ti, wi in zip(a, t, w):
        W1 = W1 + float(ai) * wi
        W2 = W2 + float(ti - ai) * wi
        A, B = A + ai, B + ti - ai
    return 0.0 if A == 0 or B == 0 else W1 / float(A) - W2 / float(B)


@pytest.mark.gpu
def test_band_counts_a_tie_that_f64_rounds_below():
    """what `- tol` is for.  Six rows at 0.1, 0.3, 0.7, 0.7, 1.9 and 1.9 (not dyadic; two pairs share a position), ten
    cells, four of them in population 1: some labellings have exactly the observed |delta| with the counts of
    equal-position rows distributed differently, so their f64 sums are added in another order.  Asserted on the CPU
    first: the exact oracle has no near tie (lo == hi), and the device's own f64 arithmetic WITHOUT the band would count
    fewer labellings than lo.  Then the entry point must return lo"""
    from scape_amd import _lib
    from scape_amd._lib import P_d, P_i64, check as chk, ptr
    n1, n, seed, n_perm = 4, 10, 77, 300
    x = np.array([0.1, 0.3, 0.7, 0.7, 1.9, 1.9])
    rng = np.random.default_rng(21)
    M = rng.integers(0, 4, (len(x), n)) * (rng.random((len(x), n)) < 0.8)
    nzs = [[(j, int(v)) for j, v in enumerate(row) if v] for row in M.tolist()]
    o = LenRec("tie", nzs, [Fraction(float(v)) for v in x], n1)
    assert o.tested() and len(o.nzs) == len(x)
    w = x - x.min()
    e0 = abs(_f64_delta(o.a0, o.t, w))
    plain = rounded_below = 0
    for p in range(1, n_perm + 1):
        member = bytearray(n)
        for j in rc.members(seed, p, n1, n):
            member[j] = 1
        o.count(member)
        a = o.row_sums(member)
        e = abs(_f64_delta(a, o.t, w))
        plain += e >= e0
        rounded_below += abs(o.delta(a)) == abs(o.delta(o.a0)) and e < e0
    print("lo", o.lo, "hi", o.hi, "f64 without the band", plain, "exact ties rounded below", rounded_below)
    assert o.lo == o.hi and rounded_below > 0 and plain == o.lo - rounded_below
    lab, cb = np.nonzero(M)
    rep = M[lab, cb]
    lab, cb = np.repeat(lab, rep).astype(np.int64), np.repeat(cb, rep).astype(np.int64)
    off, Ks = np.array([0, len(lab)], np.int64), np.array([len(x)], np.int32)
    roff, rows = np.array([0, len(x)], np.int64), np.arange(len(x), dtype=np.int64)
    tol = np.array([np.ldexp(float(w.max()), -40)])
    t, a0, d0, n_ge = np.zeros(len(x), np.int64), np.zeros(len(x), np.int64), np.zeros(1), np.zeros(1, np.int64)
    ctx = _lib.default_context(None)
    lib = ctx.lib
    try:
        rc.device_counts(ctx, Ks, off, lab, cb, n)
        chk(lib.scape_hip_report_perm_masks(ctx.h, n1, n - n1, 1, n_perm, seed), "perm_masks")
        chk(lib.scape_hip_report_perm_len(ctx.h, 1, ptr(roff, P_i64), ptr(rows, P_i64), ptr(w, P_d), ptr(tol, P_d),
                                          ptr(t, P_i64), ptr(a0, P_i64), ptr(d0, P_d), ptr(n_ge, P_i64)), "perm_len")
    finally:
        lib.scape_hip_report_free(ctx.h)
    print("device n_ge", int(n_ge[0]), "delta0", float(d0[0]), "f64 restatement", _f64_delta(o.a0, o.t, w))
    assert t.tolist() == o.t and a0.tolist() == o.a0
    assert float(d0[0]) == _f64_delta(o.a0, o.t, w)
    assert int(n_ge[0]) == o.lo


@pytest.mark.gpu
def test_entry_point():
    """scape_hip_report_perm_len on a hand-made matrix: records of 2, 5, 70 and 150 rows, tested columns in front of 9
    others; t and a0 against numpy, n_ge against the exact oracle (lo == hi asserted first), delta(0) within the stated
    (2 R + 3) 2^-53 span; one call with 300 permutations equals three calls with 100, 156 and 44 that accumulate;
    then the error paths"""
    from scape_amd import _lib
    from scape_amd._lib import P_d, P_i64, check as chk, ptr
    n1, n2, n_cols, seed, n_perm, Ks, off, lab, cb, dense, rows, roff, rng = rc.entry_point_matrix()
    n = n1 + n2
    sub = dense[rows][:, :n]
    t_want, a0_want = sub.sum(axis=1), sub[:, :n1].sum(axis=1)
    # positions with fractional parts (exact in f64), unsorted within a record
    x = np.concatenate([rng.permutation(rng.choice(40000, k, replace=False)) / 8.0 + 3.0 for k in np.diff(roff).tolist()])
    w = np.concatenate([x[roff[r]:roff[r + 1]] - x[roff[r]:roff[r + 1]].min() for r in range(len(Ks))])
    span = np.array([w[roff[r]:roff[r + 1]].max() for r in range(len(Ks))])
    tol = np.ldexp(span, -40)
    orc = []
    for r in range(len(Ks)):
        nzs = [[(j, int(v)) for j, v in enumerate(row) if v] for row in sub[roff[r]:roff[r + 1]].tolist()]
        orc.append(LenRec(f"r{r}", nzs, [Fraction(float(v)) for v in x[roff[r]:roff[r + 1]]], n1))
        assert orc[-1].tested() and orc[-1].span == Fraction(float(span[r]))
    for p in range(1, n_perm + 1):
        member = bytearray(n)
        for j in rc.members(seed, p, n1, n):
            member[j] = 1
        for o in orc:
            o.count(member)
    assert all(o.lo == o.hi for o in orc), [(o.lo, o.hi) for o in orc]
    ge_want = np.array([o.lo for o in orc], dtype=np.int64)
    print("n_ge of the oracle", ge_want.tolist())
    ctx = _lib.default_context(None)
    lib = ctx.lib

    def counts():
        assert np.array_equal(rc.device_counts(ctx, Ks, off, lab, cb, n_cols), dense.sum(axis=1))

    def outs():
        return (np.full(len(rows), -1, np.int64), np.full(len(rows), -1, np.int64), np.full(len(Ks), -1.0),
                np.zeros(len(Ks), np.int64))

    def test(o, roff_=roff, rows_=rows, w_=w, tol_=tol, n_rec=len(Ks)):
        return lib.scape_hip_report_perm_len(ctx.h, n_rec, ptr(roff_, P_i64), ptr(rows_, P_i64), ptr(w_, P_d),
                                             ptr(tol_, P_d), ptr(o[0], P_i64), ptr(o[1], P_i64), ptr(o[2], P_d),
                                             ptr(o[3], P_i64))
    try:
        counts()
        chk(lib.scape_hip_report_perm_masks(ctx.h, n1, n2, 1, n_perm, seed), "perm_masks")
        one = outs()
        chk(test(one), "perm_len")
        for got, want, name in ((one[0], t_want, "t"), (one[1], a0_want, "a0"), (one[3], ge_want, "n_ge")):
            print(name, "equal", np.array_equal(got, want), got[:8].tolist(), want[:8].tolist())
            assert np.array_equal(got, want), name
        for r, o in enumerate(orc):
            R = int(roff[r + 1] - roff[r])
            err = abs(Fraction(float(one[2][r])) - o.delta(o.a0))
            print("delta0", r, float(one[2][r]), "error / span", float(err / o.span))
            assert err <= (2 * R + 3) * o.span / (1 << 53), (r, float(err))
        assert 0 < ge_want.min() and ge_want.max() < n_perm
        acc = outs()
        for p_first, p_count in ((1, 100), (101, 156), (257, 44)):
            chk(lib.scape_hip_report_perm_masks(ctx.h, n1, n2, p_first, p_count, seed), "perm_masks")
            chk(test(acc), "perm_len")
        assert np.array_equal(acc[3], ge_want) and np.array_equal(acc[2], one[2])
        chk(lib.scape_hip_report_perm_masks(ctx.h, n1, n2, 1, n_perm, seed + 1), "perm_masks")
        other = outs()
        chk(test(other), "perm_len")
        assert not np.array_equal(other[3], ge_want) and np.array_equal(other[2], one[2])
        # the same labellings as scape_hip_report_perm_test: a record of two rows at positions 0 and 1 has
        # delta = a_1 / A - b_1 / B = d_1, so its n_ge is the site count of row 1 in diff_pa's test
        two = (np.zeros(2, np.int64), np.zeros(2, np.int64), np.zeros(1), np.zeros(1, np.int64))
        r2, o2 = rows[roff[1]:roff[1] + 2].copy(), np.array([0, 2], dtype=np.int64)
        chk(test(two, o2, r2, np.array([0.0, 1.0]), np.array([2.0 ** -40]), 1), "perm_len")
        site, gene, stat0 = np.zeros(2, np.int64), np.zeros(1, np.int64), np.zeros(1)
        chk(lib.scape_hip_report_perm_test(ctx.h, 1, ptr(o2, P_i64), ptr(r2, P_i64), ptr(two[0].copy(), P_i64),
                                           ptr(two[1].copy(), P_i64), ptr(site, P_i64), ptr(stat0, P_d),
                                           ptr(gene, P_i64)), "perm_test")
        print("two-row record: perm_len", two[3].tolist(), "perm_test sites", site.tolist())
        assert two[3][0] == site[1] == site[0]
        # error paths: each returns non-zero and leaves a message
        o = outs()
        bad_roff = roff.copy()
        bad_roff[1], bad_roff[2] = roff[2], roff[1]
        assert test(o, bad_roff) != 0 and "non-decreasing" in _lib.last_error()
        bad_roff = roff.copy()
        bad_roff[0] = 1
        assert test(o, bad_roff) != 0 and "start at 0" in _lib.last_error()
        bad_rows = rows.copy()
        bad_rows[3] = int(Ks.sum())
        assert test(o, rows_=bad_rows) != 0 and "row index out of range" in _lib.last_error()
        bad_rows[3] = -1
        assert test(o, rows_=bad_rows) != 0 and "row index out of range" in _lib.last_error()
        many = np.zeros(1025, np.int64)
        assert test((np.zeros(1025, np.int64), np.zeros(1025, np.int64), np.zeros(1), np.zeros(1, np.int64)),
                    np.array([0, 1025], np.int64), many, np.zeros(1025), np.zeros(1), 1) != 0
        assert "more than 1024 rows" in _lib.last_error()
        for k in range(2, 10):                                               # every pointer argument, NULL in turn
            a = [ctx.h, len(Ks), ptr(roff, P_i64), ptr(rows, P_i64), ptr(w, P_d), ptr(tol, P_d), ptr(o[0], P_i64),
                 ptr(o[1], P_i64), ptr(o[2], P_d), ptr(o[3], P_i64)]
            a[k] = None
            assert lib.scape_hip_report_perm_len(*a) != 0 and "bad argument" in _lib.last_error(), k
        assert lib.scape_hip_report_perm_len(None, len(Ks), ptr(roff, P_i64), ptr(rows, P_i64), ptr(w, P_d),
                                             ptr(tol, P_d), ptr(o[0], P_i64), ptr(o[1], P_i64), ptr(o[2], P_d),
                                             ptr(o[3], P_i64)) != 0
        assert test(o, n_rec=0) != 0 and "bad argument" in _lib.last_error()
        bad_w = w.copy()
        bad_w[5] = np.nan
        assert test(o, w_=bad_w) != 0 and "weights" in _lib.last_error()
        bad_w[5] = -1.0
        assert test(o, w_=bad_w) != 0 and "weights" in _lib.last_error()
        assert test(o, tol_=np.array([0.0, np.inf, 0.0, 0.0])) != 0 and "tolerances" in _lib.last_error()
        assert np.array_equal(o[3], np.zeros(len(Ks), np.int64))                 # a refused call adds nothing
        assert np.all(o[0] == -1) and np.all(o[1] == -1) and np.all(o[2] == -1.0)  # and writes nothing
        assert test(outs()) == 0                                                 # and keeps counts and masks
        lib.scape_hip_report_free(ctx.h)
        assert test(outs()) != 0 and "report_counts" in _lib.last_error()
        chk(lib.scape_hip_report_perm_masks(ctx.h, n1, n2, 1, 10, seed), "perm_masks")
        assert test(outs()) != 0 and "report_counts" in _lib.last_error()          # masks, but no counts yet
        lib.scape_hip_report_free(ctx.h)
        counts()
        assert test(outs()) != 0 and "perm_masks" in _lib.last_error()             # counts, but no masks yet
        chk(lib.scape_hip_report_perm_masks(ctx.h, n_cols, 5, 1, 10, seed), "perm_masks")
        assert test(outs()) != 0 and "fewer columns" in _lib.last_error()          # more positions than columns
    finally:
        lib.scape_hip_report_free(ctx.h)
