"""`scape diff_pa`: the permutation test of pA usage between two cell populations (scape_amd/report.py, section diff_pa;
kernels k_rep_perm_* of scape_amd/csrc/perm.inc).

The oracle below restates the command's contract in exact arithmetic and imports nothing from scape_amd: Python ints
for mix / key / the membership of every permutation / every sum, fractions.Fraction for the statistics S and d of the
observed labelling, and - for the two comparisons per statistic and permutation - the cross-multiplied integers that
`Fraction.__ge__` itself compares (test_integer_comparison_is_the_fraction_comparison checks that claim on Fractions).
For every count it gives lo = #{stat(p) >= stat(0)} and hi = #{stat(p) >= stat(0) (1 - 2^-39)}; every GPU test first
asserts lo == hi for every site and record of its case, on the oracle alone, and then that the file's counts EQUAL lo.
That lo == hi holds for every case of this file (generator seeds included) was checked on a CPU before the GPU saw
them; no case is excused.

Kernel check done once by hand (not committed), on an MI355X, the 54 GPU tests of this file against three altered
builds: with the bit test shifted by one position 48 fail (the 6 that pass cannot see it: four golden cases without a
tested record, test_seeds and test_batch_and_chunk_invariance, which compare runs with each other); with one member
fewer in the select (rank n1 - 2 for n1 - 1, unchanged where n1 = 1) 43 fail (beside those 6: the three cases with
n1 = 1, n_perm = 1, and one 4-line golden case); with `>` for `>=` in both exceedance tests 5 fail - a labelling that
ties with the observed one still lies above stat(0) (1 - 2^-40), so `>` differs only where the observed statistic is
0 (four golden cases and n = 2 have such sites)."""
import csv
import functools
import io
import math
import os
from fractions import Fraction

import numpy as np
import pytest

import report_cases as rc
from report_cases import G, M64, bh, key, members, mix, no_gpu, populations, run as _run  # noqa: F401  (no_gpu: fixture)

HEADER = ("gene,pa_info,pct.1,pct.2,versus,usage.1,usage.2,delta_usage,n_ge,p_val,p_val_adj,gene_stat,gene_n_ge,"
          "gene_p_val,gene_p_val_adj,n_perm")


# ---------------------------------------------------------------- the contract, restated (mix, key, members, bh,
# populations and the inputs' definitions: tests/report_cases.py, which imports nothing from scape_amd either)
class _Rec:
    """a tested record: per kept row its nonzeros [(position, count)], t_i and a_i(0); integers only"""

    def __init__(self, gene, pas, nzs, n1):
        self.gene, self.pas, self.nzs = gene, pas, nzs
        self.t = [sum(v for _j, v in nz) for nz in nzs]
        self.T = sum(self.t)
        self.L = math.lcm(*self.t)
        self.a0 = [sum(v for j, v in nz if j < n1) for nz in nzs]
        self.q0, self.ab0, self.N0 = self.stat(self.a0)
        self.site = [[0, 0] for _ in nzs]                  # lo, hi
        self.gene_ge = [0, 0]

    def stat(self, a):
        """(Q, A B, [N_i]) with S = Q / (L A B) and d_i = N_i / (A B); Q = 0, A B = 1, N = 0 when A B = 0"""
        A = sum(a)
        B = self.T - A
        if A == 0 or B == 0:
            return 0, 1, [0] * len(a)
        N = [ai * self.T - ti * A for ai, ti in zip(a, self.t)]
        return sum(Ni * Ni * (self.L // ti) for Ni, ti in zip(N, self.t)), A * B, N

    def count(self, member):
        a = [sum(v for j, v in nz if member[j]) for nz in self.nzs]
        q, ab, N = self.stat(a)
        # x / ab >= x0 / ab0 * (num / den), all denominators positive: cross-multiplied
        for w, (num, den) in enumerate(((1, 1), ((1 << 39) - 1, 1 << 39))):
            self.gene_ge[w] += q * self.ab0 * den >= self.q0 * ab * num
            for i in range(len(N)):
                self.site[i][w] += abs(N[i]) * self.ab0 * den >= abs(self.N0[i]) * ab * num


def oracle(rec_rows, cols1, cols2, n_perm, seed):
    """rec_rows: [(gene, [(pa_info, counts over every matrix column)])] in file order.  Returns the expected lines:
    dicts of the text columns, the exact counts (lo, hi) and the Fractions of the float columns."""
    cols = np.array(list(cols1) + list(cols2), dtype=np.int64)
    n1, n = len(cols1), len(cols)
    assert n1 >= 1 and n - n1 >= 1 and n < 1 << 24
    recs = []
    for gene, rows in rec_rows:
        pas, nzs = [], []
        for pa, row in rows:
            vals = np.asarray(row)[cols].tolist()
            nz = [(j, int(v)) for j, v in enumerate(vals) if v]
            if nz:
                pas.append(pa)
                nzs.append(nz)
        if len(nzs) < 2:
            continue
        r = _Rec(gene, pas, nzs, n1)
        if sum(r.a0) > 0 and r.T - sum(r.a0) > 0:
            assert r.T < 1 << 31
            recs.append(r)
    for p in range(1, n_perm + 1):
        member = bytearray(n)
        pop1 = members(seed, p, n1, n)
        assert len(set(pop1)) == n1
        for j in pop1:
            member[j] = 1
        for r in recs:
            r.count(member)
    lines = []
    for r in recs:
        A = sum(r.a0)
        B = r.T - A
        S0 = sum(Fraction(Ni * Ni, ti * A * B) for Ni, ti in zip(r.N0, r.t))
        assert S0 == Fraction(r.q0, r.L * r.ab0)
        for i, pa in enumerate(r.pas):
            lines.append(dict(gene=r.gene, pa=pa, pct1=repr(sum(1 for j, _v in r.nzs[i] if j < n1) / n1),
                              pct2=repr(sum(1 for j, _v in r.nzs[i] if j >= n1) / (n - n1)),
                              usage1=Fraction(r.a0[i], A), usage2=Fraction(r.t[i] - r.a0[i], B),
                              delta=Fraction(r.N0[i], A * B), site=tuple(r.site[i]), S0=S0, gene_ge=tuple(r.gene_ge),
                              first=i == 0))
    p_site = bh([Fraction(1 + ln["site"][0], 1 + n_perm) for ln in lines])
    firsts = [k for k, ln in enumerate(lines) if ln["first"]]
    p_gene = bh([Fraction(1 + lines[k]["gene_ge"][0], 1 + n_perm) for k in firsts])
    g = -1
    for k, ln in enumerate(lines):
        g += ln["first"]
        ln["p_adj"], ln["gene_p_adj"] = p_site[k], p_gene[g]
    return lines


def assert_no_near_tie(lines, what):
    """lo == hi for every site and record: no permutation's statistic lies within 2^-39 below the observed one, so the
    device's f64 comparison (slack 2^-40) can hide nothing"""
    for ln in lines:
        assert ln["site"][0] == ln["site"][1], (what, ln["gene"], ln["pa"], ln["site"])
        assert ln["gene_ge"][0] == ln["gene_ge"][1], (what, ln["gene"], ln["gene_ge"])


def compare(text, lines, versus, n_perm, what):
    rows = list(csv.reader(io.StringIO(text)))
    assert ",".join(rows[0]) == HEADER
    body = rows[1:]
    print(what, "lines", len(body), "expected", len(lines))
    assert len(body) == len(lines), what
    for got, ln in zip(body, lines):
        ctx = (what, ln["gene"], ln["pa"], got)
        assert got[0] == ln["gene"] and got[1] == ln["pa"] and got[4] == versus and got[15] == str(n_perm), ctx
        assert got[2] == ln["pct1"] and got[3] == ln["pct2"], ctx
        assert got[8] == str(ln["site"][0]), ctx
        assert got[12] == str(ln["gene_ge"][0]), ctx
        assert got[9] == repr((1 + ln["site"][0]) / (1 + n_perm)), ctx
        assert got[13] == repr((1 + ln["gene_ge"][0]) / (1 + n_perm)), ctx
        for col, want in ((5, ln["usage1"]), (6, ln["usage2"]), (7, ln["delta"]), (10, ln["p_adj"]), (11, ln["S0"]),
                          (14, ln["gene_p_adj"])):
            assert rc.close(got[col], want), (ctx, col, float(want))


# ---------------------------------------------------------------- the command
def _args(root, clu, res="res.gene.pkl", id1=None, id2=None, n_perm=None, seed=None):
    return rc.perm_args("diff_pa", root, clu, res, id1, id2, n_perm, seed)


def _command(root, clu, res, id1, id2, n_perm, seed, what=""):
    return rc.perm_command("diff_pa", root, clu, res, id1, id2, n_perm, seed, what)


def check(root, clu_path, clu_text, res, rec_rows, bc, id1, id2, n_perm, seed, what):
    """oracle first (and lo == hi on it), then the command; returns (file text, expected lines)"""
    c1, c2 = populations(bc, clu_text, id1, id2)
    lines = oracle(rec_rows, c1, c2, n_perm, seed)
    assert_no_near_tie(lines, what)
    text = _command(root, clu_path, res, id1, id2, n_perm, seed, what)
    versus = f"{id1}_Vs_{id2}" if id2 is not None else id1
    compare(text, lines, versus, n_perm, what)
    return text, lines


# ---------------------------------------------------------------- CPU
def test_mix_anchor_and_key():
    assert mix(G) == 0xE220A8397B1DCDAF          # first output of the published splitmix64 from state 0
    assert key(1, 1, 5) & 0xFFFFFF == 5 and key(1, 1, 5) >> 24 == mix((mix((1 + G) & M64) + G * 6) & M64) >> 24
    assert len({key(7, 3, j) for j in range(5000)}) == 5000
    assert key(M64, 1, 0) == (mix((mix((M64 + G) & M64) + G) & M64) & ~0xFFFFFF & M64)


@pytest.mark.parametrize("n1,n2,seed", [(1, 1, 0), (1, 63, 1), (63, 1, 2), (230, 301, 1), (64, 64, M64), (5, 700, 12345)])
def test_selection_has_n1_members(n1, n2, seed):
    seen = set()
    for p in (1, 2, 3, 999):
        m = members(seed, p, n1, n1 + n2)
        assert len(m) == n1 == len(set(m)) and all(0 <= j < n1 + n2 for j in m)
        ks = sorted(key(seed, p, j) for j in range(n1 + n2))
        assert sorted(m) == sorted(k & 0xFFFFFF for k in ks[:n1])
        seen.add(tuple(sorted(m)))
    assert n1 + n2 <= 2 or len(seen) > 1


def test_bh_hand_worked():
    # sorted: .005 .01 .03 .04 .5 -> m p / rank = .025 .025 .05 .05 .5, already monotone
    ps = [Fraction(1, 100), Fraction(4, 100), Fraction(3, 100), Fraction(5, 1000), Fraction(1, 2)]
    assert bh(ps) == [Fraction(25, 1000), Fraction(5, 100), Fraction(5, 100), Fraction(25, 1000), Fraction(1, 2)]
    # the running minimum and the cap: .01 .02 .021 .9 -> .04 .04 .028 .9 -> .028 .028 .028 .9
    ps = [Fraction(9, 10), Fraction(21, 1000), Fraction(1, 100), Fraction(2, 100)]
    assert bh(ps) == [Fraction(9, 10), Fraction(28, 1000), Fraction(28, 1000), Fraction(28, 1000)]
    assert bh([Fraction(3, 4), Fraction(4, 5)]) == [Fraction(4, 5), Fraction(4, 5)] and bh([]) == []
    from scape_amd import report
    for ps in ([0.01, 0.04, 0.03, 0.005, 0.5], [0.9, 0.021, 0.01, 0.02], [0.75, 0.8], [1.0], [0.5, 0.5, 0.001]):
        want = [float(v) for v in bh([Fraction(p) for p in ps])]
        assert np.allclose(report._bh(ps), want, rtol=1e-14, atol=0), ps
    assert len(report._bh([])) == 0


def test_integer_comparison_is_the_fraction_comparison():
    """_Rec.count compares cross-multiplied integers; the same labellings through Fractions give the same counts"""
    rng = np.random.default_rng(5)
    n1, n = 9, 20
    rows = [("r%d" % i, (rng.random(n) < 0.5) * rng.integers(1, 4, n)) for i in range(4)]
    lines = oracle([("g", rows)], range(n1), range(n1, n), 60, 3)
    assert len(lines) == 4
    t = [int(r.sum()) for _pa, r in rows]
    T = sum(t)

    def stats(member):
        a = [int(r[np.array(member, dtype=bool)].sum()) for _pa, r in rows]
        A = sum(a)
        B = T - A
        if A == 0 or B == 0:
            return Fraction(0), [Fraction(0)] * 4
        N = [ai * T - ti * A for ai, ti in zip(a, t)]
        return sum(Fraction(Ni * Ni, ti * A * B) for Ni, ti in zip(N, t)), [Fraction(Ni, A * B) for Ni in N]
    S0, d0 = stats([j < n1 for j in range(n)])
    c = 1 - Fraction(1, 1 << 39)
    lo_g = hi_g = 0
    lo, hi = [0] * 4, [0] * 4
    for p in range(1, 61):
        pop1 = set(members(3, p, n1, n))
        S, d = stats([j in pop1 for j in range(n)])
        lo_g += S >= S0
        hi_g += S >= S0 * c
        for i in range(4):
            lo[i] += abs(d[i]) >= abs(d0[i])
            hi[i] += abs(d[i]) >= abs(d0[i]) * c
    assert lines[0]["S0"] == S0 and lines[0]["gene_ge"] == (lo_g, hi_g)
    assert [ln["site"] for ln in lines] == list(zip(lo, hi)) and [ln["delta"] for ln in lines] == d0
    assert 0 < lo_g < 60                                   # the case exercises both outcomes


def test_help_lists_command_and_options():
    r = _run(["--help"])
    assert r.exit_code == 0 and "diff_pa" in r.output
    r = _run(["diff_pa", "--help"])
    assert r.exit_code == 0, r.output
    for o in ("--output_dir", "--res_pkl_file", "--cell_cluster_file", "--idents_1", "--idents_2", "--n_perm", "--seed"):
        assert o in r.output
    flat = " ".join(r.output.split())
    assert "[default: 9999]" in flat and "[default: 1]" in flat


def test_utils_import_path():
    import scape.utils as su
    from scape_amd import report
    assert su.diff_pa is report.diff_pa


def test_prerequisites_and_argument_errors(tmp_path, no_gpu):
    clu = tmp_path / "groups.csv"
    r = _run(_args(tmp_path / "nope", clu, id1="A"))
    assert r.exit_code != 0 and "Given output_dir folder does not exists." in str(r.exception)
    r = _run(_args(tmp_path, clu, id1="A"))
    assert "Given res_pkl_file is not in output_dir." in str(r.exception)
    (tmp_path / "res.gene.pkl").write_bytes(b"")
    r = _run(_args(tmp_path, clu, id1="A"))
    assert "Given cell_cluster_file file does not exists" in str(r.exception)
    clu.write_text("index,group\n3,A\n4,B\n5,\n77,ghost\n")
    r = _run(_args(tmp_path, clu, id1="A"))
    assert isinstance(r.exception, FileNotFoundError) and "barcode_index.csv" in str(r.exception)
    (tmp_path / "barcode_index.csv").write_text("CB,index\nA-1,3\nB-1,4\nC-1,5\n")
    for extra, word in ((["--idents_1", "A", "--idents_2", "A"], "same"), (["--idents_1", "Z"], "'Z'"),
                        (["--idents_1", "A", "--idents_2", "Z"], "'Z'"), (["--idents_1", ""], "names no cluster"),
                        (["--idents_1", "A", "--n_perm", "0"], "n_perm"), (["--idents_1", "A", "--n_perm", "-3"], "n_perm"),
                        (["--idents_1", "A", "--seed", "-1"], "seed"),
                        (["--idents_1", "A", "--seed", str(1 << 64)], "seed"),
                        (["--idents_1", "ghost"], "has no cell"), (["--idents_1", "A", "--idents_2", "ghost"], "has no cell")):
        r = _run(_args(tmp_path, clu) + extra)
        assert isinstance(r.exception, ValueError) and word in str(r.exception), (extra, repr(r.exception))
    clu.write_text("index,group\n3,A\n4,A\n5,\n")                     # nobody left for "the rest"
    r = _run(_args(tmp_path, clu, id1="A"))
    assert isinstance(r.exception, ValueError) and "has no cell" in str(r.exception)
    r = _run(["diff_pa", "--output_dir", str(tmp_path), "--res_pkl_file", "res.gene.pkl", "--cell_cluster_file", str(clu)])
    assert r.exit_code == 2 and "--idents_1" in r.output
    r = _run(["diff_pa", "--output_dir", str(tmp_path), "--res_pkl_file", "res.gene.pkl", "--idents_1", "A"])
    assert r.exit_code == 2 and "--cell_cluster_file" in r.output
    assert sorted(os.listdir(tmp_path)) == ["barcode_index.csv", "groups.csv", "res.gene.pkl"]


# ---------------------------------------------------------------- GPU: golden cases
def _golden_rec_rows(cs, n_cols):
    """the reference's own matrix rows (tests/golden/fixture_report.npz), cut into records: a record's rows are its
    labels < K that have a read, in label order"""
    pas, dense = rc.dense_of_body(cs["mat_body"], n_cols)
    out, k = [], 0
    for rec in cs["records"]:
        lab = np.asarray(rec["label_arr"])
        n = len(np.unique(lab[lab < int(rec["K"])]))
        out.append((rec["gene_info_str"], [(pas[k + i], dense[k + i]) for i in range(n)]))
        k += n
    assert k == len(pas)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("c,j", rc.golden_perm_params())
def test_golden_case_and_cluster_file(c, j, tmp_path):
    """every golden case and cluster file that gives two non-empty populations: the first such cluster against the
    rest, 199 permutations; counts equal to the exact oracle's"""
    cs = rc.fixture_case(c)
    texts = rc.cluster_texts(cs)
    bc, paths = rc.write_case(cs, tmp_path)
    fn = cs["clu_files"][j]
    id1 = rc.golden_ident(bc, texts[fn])
    rec_rows = _golden_rec_rows(cs, len(rc.column_ids(bc)))
    check(tmp_path, paths[j], texts[fn], cs["res"], rec_rows, bc, id1, None, 199, 1, f"{cs['name']}/{fn}")


def test_golden_cases_are_used():
    ids = [p.id for p in rc.golden_perm_params()]
    assert len(ids) >= 30 and any(i.startswith("SCZ") for i in ids) and any(i.startswith("chain") for i in ids)


# ---------------------------------------------------------------- GPU: the synthetic directory
@functools.lru_cache(maxsize=None)
def _syn():
    records, bc, clu_text = rc.synthetic()
    return dict(records=records, bc=bc, clu=clu_text, rec_rows=rc.rec_rows_of(records, rc.column_ids(bc)))


def _sense(lines, n_perm, what):
    """planted records reach the smallest p-value, no null record does; on whatever `lines` holds (oracle or file)"""
    planted = {f"GENE{r}" for r in range(rc.N_PLANTED)}
    seen = set()
    for gene, ge in lines:
        name = gene.split(":")[1]
        if name in planted:
            seen.add(name)
            assert ge == 0, (what, gene, ge)
        else:
            assert ge > 0, (what, gene, ge)
    assert seen == planted, what


@pytest.mark.gpu
@pytest.mark.parametrize("id2", ["B", None], ids=["A_vs_B", "A_vs_rest"])
def test_synthetic_directory(id2, tmp_path):
    """999 permutations of 230 + 301 cells (with --idents_2; n = 531 is no multiple of 64) and of 230 + 341 (without):
    parity with the exact oracle, and sense: the planted records have gene_p_val = 1 / 1000, no other record has -
    asserted on the oracle, then on the file"""
    s = _syn()
    path = rc.write_synthetic(tmp_path)
    c1, c2 = populations(s["bc"], s["clu"], "A", id2)
    assert (len(c1), len(c2)) == ((230, 301) if id2 else (230, 341))
    text, lines = check(tmp_path, path, s["clu"], "res.gene.pkl", s["rec_rows"], s["bc"], "A", id2, 999, 1, f"syn/{id2}")
    genes = {ln["gene"].split(":")[1] for ln in lines}
    assert "GENE5" not in genes and "GENE6" not in genes                 # reads only in A; K = 1
    assert sum(ln["gene"].split(":")[1] == "GENE4" for ln in lines) == 2   # the row without a tested read is dropped
    assert sum(ln["gene"].split(":")[1] == f"GENE{len(s['records']) - 1}" for ln in lines) > 55   # the K = 63 record
    assert len(genes) >= 30
    _sense([(ln["gene"], ln["gene_ge"][0]) for ln in lines if ln["first"]], 999, "oracle")
    body = list(csv.reader(io.StringIO(text)))[1:]
    _sense(sorted({(r[0], int(r[12])) for r in body}), 999, "file")
    assert {r[13] for r in body if r[0].split(":")[1] in {"GENE0", "GENE1", "GENE2", "GENE3"}} == {repr(1 / 1000)}


@pytest.mark.gpu
@pytest.mark.parametrize("n_perm", [1, 255, 256, 257])
def test_tile_edges(n_perm, tmp_path):
    """a workgroup of the test kernel takes 256 permutations: one short of a tile, a full tile, one over, and one"""
    s = _syn()
    path = rc.write_synthetic(tmp_path, 12)
    check(tmp_path, path, s["clu"], "res.gene.pkl", s["rec_rows"][:12], s["bc"], "C", "A", n_perm, 5, f"tile/{n_perm}")


@pytest.mark.gpu
@pytest.mark.parametrize("n_cells,n_a", [(64, 1), (64, 63), (64, 32), (65, 1), (130, 129), (2, 1)],
                         ids=["64-1", "64-63", "64-32", "65-1", "130-129", "2-1"])
def test_small_and_lopsided_populations(n_cells, n_a, tmp_path):
    """populations of 1 cell and of n - 1 cells, n = 64 exactly, one over, and the smallest n"""
    path, clu_text, bc, records, ids = rc.small_dir(tmp_path, n_cells, n_a, 100 + n_cells + n_a)
    rec_rows = rc.rec_rows_of(records, ids)
    _text, lines = check(tmp_path, path, clu_text, "res.utr.pkl", rec_rows, bc, "A", None, 300, 9, f"small/{n_cells}/{n_a}")
    assert len(lines) >= 12


@pytest.mark.gpu
def test_seeds(tmp_path):
    """the same seed gives the same bytes, another seed other counts"""
    s = _syn()
    path = rc.write_synthetic(tmp_path)
    a = _command(tmp_path, path, "res.gene.pkl", "A", "B", 99, 1)
    b = _command(tmp_path, path, "res.gene.pkl", "A", "B", 99, 1)
    c = _command(tmp_path, path, "res.gene.pkl", "A", "B", 99, 2)
    assert a == b and a != c
    col = lambda text: [r[8] for r in csv.reader(io.StringIO(text))]
    assert col(a) != col(c) and len(col(a)) == len(col(c)) > 100


@pytest.mark.gpu
def test_batch_and_chunk_invariance(tmp_path, monkeypatch):
    """records split over several count batches and the permutations over several chunks: the same bytes"""
    from scape_amd import _lib, report
    s = _syn()
    path = rc.write_synthetic(tmp_path)
    big = _command(tmp_path, path, "res.gene.pkl", "A", None, 999, 1)
    lib = _lib.load_library()
    calls = {"masks": [], "test": 0}
    real_m, real_t = lib.scape_hip_report_perm_masks, lib.scape_hip_report_perm_test

    def masks(*a):
        calls["masks"].append((a[3], a[4]))
        return real_m(*a)

    def test(*a):
        calls["test"] += 1
        return real_t(*a)
    monkeypatch.setattr(lib, "scape_hip_report_perm_masks", masks)
    monkeypatch.setattr(lib, "scape_hip_report_perm_test", test)
    assert _command(tmp_path, path, "res.gene.pkl", "A", None, 999, 1) == big
    assert calls["masks"] == [(1, 999)] and calls["test"] == 1
    calls.update(masks=[], test=0)
    monkeypatch.setattr(report, "MAX_BATCH_BYTES", 1 << 16)             # a record of K = 8 alone takes 57 KB
    monkeypatch.setattr(report, "MAX_PERM_BYTES", 1 << 30)
    assert _command(tmp_path, path, "res.gene.pkl", "A", None, 999, 1) == big
    assert calls["masks"] == [(1, 999)] and calls["test"] > 5
    n_batches = calls["test"]
    calls.update(masks=[], test=0)
    monkeypatch.setattr(report, "MAX_PERM_BYTES", (9 + 1) * 8 * 300)     # 9 words of 64 positions, 1 key bound: 300 permutations
    assert _command(tmp_path, path, "res.gene.pkl", "A", None, 999, 1) == big
    assert calls["test"] == 4 * n_batches and calls["masks"][:4] == [(1, 300), (301, 300), (601, 300), (901, 99)]


# ---------------------------------------------------------------- GPU: the entry points
def _np_mix(z):
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def _np_members(seed, p, n1, n):
    """the selection in numpy (uint64 arithmetic wraps mod 2^64): boolean membership of permutation p"""
    with np.errstate(over="ignore"):
        base = _np_mix(np.uint64(seed) + np.uint64(G) * np.uint64(p))
        j = np.arange(n, dtype=np.uint64)
        keys = (_np_mix(base + np.uint64(G) * (j + np.uint64(1))) & ~np.uint64(0xFFFFFF)) | j
    m = np.zeros(n, dtype=bool)
    m[np.argsort(keys)[:n1]] = True
    return m


def test_numpy_selection_is_the_python_selection():
    for seed, p, n1, n in ((1, 1, 10, 50), (M64, 7, 1, 64), (12345, 400, 129, 130)):
        assert sorted(np.nonzero(_np_members(seed, p, n1, n))[0].tolist()) == sorted(members(seed, p, n1, n))


@pytest.mark.gpu
def test_entry_points():
    """scape_hip_report_perm_masks / _perm_test on a hand-made matrix: records of 2, 5, 70 and 150 rows (the last two
    are taken in groups of 64 rows), tested columns in front of 9 others; t, a0 and S(0) against numpy, the counts
    against a numpy restatement (every comparison at least 1e-9 away from a tie, asserted); one call with 300
    permutations equals three calls with 100, 156 and 44 that accumulate; then the error paths"""
    from scape_amd import _lib
    from scape_amd._lib import P_d, P_i64, check as chk, ptr
    n1, n2, n_cols, seed, n_perm, Ks, off, lab, cb, dense, rows, roff, rng = rc.entry_point_matrix()
    n = n1 + n2
    sub = dense[rows][:, :n]
    t_want, a0_want = sub.sum(axis=1), sub[:, :n1].sum(axis=1)
    member = np.stack([np.arange(n) < n1] + [_np_members(seed, p, n1, n) for p in range(1, n_perm + 1)])
    a = sub @ member.T.astype(np.int64)                                   # [row][labelling]
    site_want, gene_want, stat0_want = np.zeros(len(rows), np.int64), np.zeros(len(Ks), np.int64), np.zeros(len(Ks))
    for r in range(len(Ks)):
        sl = slice(roff[r], roff[r + 1])
        T, A = int(t_want[sl].sum()), a[sl].sum(axis=0)
        B = T - A
        N = (a[sl] * T - t_want[sl, None] * A[None, :]).astype(np.float64)
        ab = A.astype(np.float64) * B
        d = np.abs(N / ab)
        S = (N * N / (t_want[sl, None].astype(np.float64) * ab)).sum(axis=0)
        assert np.all(ab > 0)
        assert np.all(d[:, 0] > 0) and S[0] > 0
        rel = np.abs(d[:, 1:] - d[:, :1]) / d[:, :1]
        assert np.all((rel == 0) | (rel > 1e-9)) and np.all((S[1:] == S[0]) | (np.abs(S[1:] - S[0]) > 1e-9 * S[0]))
        site_want[sl] = (d[:, 1:] >= d[:, :1] * (1 - 2.0 ** -40)).sum(axis=1)
        gene_want[r] = (S[1:] >= S[0] * (1 - 2.0 ** -40)).sum()
        stat0_want[r] = S[0]
    ctx = _lib.default_context(None)
    lib = ctx.lib

    def counts():
        assert np.array_equal(rc.device_counts(ctx, Ks, off, lab, cb, n_cols), dense.sum(axis=1))

    def outs():
        return (np.full(len(rows), -1, np.int64), np.full(len(rows), -1, np.int64), np.zeros(len(rows), np.int64),
                np.full(len(Ks), -1.0), np.zeros(len(Ks), np.int64))

    def test(o, roff_=roff):
        return lib.scape_hip_report_perm_test(ctx.h, len(Ks), ptr(roff_, P_i64), ptr(rows, P_i64), ptr(o[0], P_i64),
                                              ptr(o[1], P_i64), ptr(o[2], P_i64), ptr(o[3], P_d), ptr(o[4], P_i64))
    try:
        counts()
        chk(lib.scape_hip_report_perm_masks(ctx.h, n1, n2, 1, n_perm, seed), "perm_masks")
        one = outs()
        chk(test(one), "perm_test")
        for got, want, name in ((one[0], t_want, "t"), (one[1], a0_want, "a0"), (one[2], site_want, "site_n_ge"),
                                (one[4], gene_want, "gene_n_ge")):
            print(name, "equal", np.array_equal(got, want))
            assert np.array_equal(got, want), name
        assert np.allclose(one[3], stat0_want, rtol=1e-12, atol=0)
        assert 0 < gene_want.min() and gene_want.max() < n_perm and site_want.min() < site_want.max()
        acc = outs()
        for p_first, p_count in ((1, 100), (101, 156), (257, 44)):
            chk(lib.scape_hip_report_perm_masks(ctx.h, n1, n2, p_first, p_count, seed), "perm_masks")
            chk(test(acc), "perm_test")
        assert np.array_equal(acc[2], site_want) and np.array_equal(acc[4], gene_want)
        assert np.array_equal(acc[3], one[3])
        chk(lib.scape_hip_report_perm_masks(ctx.h, n1, n2, 1, n_perm, seed + 1), "perm_masks")
        other = outs()
        chk(test(other), "perm_test")
        assert not np.array_equal(other[2], site_want) and np.array_equal(other[3], one[3])
        # error paths: each returns non-zero and leaves a message
        o = outs()
        bad_roff = roff.copy()
        bad_roff[1], bad_roff[2] = roff[2], roff[1]
        assert test(o, bad_roff) != 0 and "non-decreasing" in _lib.last_error()
        assert lib.scape_hip_report_perm_test(ctx.h, len(Ks), None, ptr(rows, P_i64), ptr(o[0], P_i64), ptr(o[1], P_i64),
                                              ptr(o[2], P_i64), ptr(o[3], P_d), ptr(o[4], P_i64)) != 0
        assert lib.scape_hip_report_perm_test(ctx.h, len(Ks), ptr(roff, P_i64), ptr(rows, P_i64), ptr(o[0], P_i64),
                                              ptr(o[1], P_i64), None, ptr(o[3], P_d), ptr(o[4], P_i64)) != 0
        assert _lib.last_error() != ""
        for args, word in (((1 << 24, 1, 1, 1, 0), "2^24"), ((1 << 23, 1 << 23, 1, 1, 0), "2^24"),
                           ((0, 5, 1, 1, 0), "at least one cell"), ((5, 0, 1, 1, 0), "at least one cell"),
                           ((5, 5, 0, 1, 0), "p_first"), ((5, 5, 1, 0, 0), "p_count")):
            assert lib.scape_hip_report_perm_masks(ctx.h, *args) != 0 and word in _lib.last_error(), args
        assert lib.scape_hip_report_perm_masks(None, 5, 5, 1, 1, 0) != 0
        assert test(outs()) == 0                                                   # a refused call keeps the earlier masks
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
