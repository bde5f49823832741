"""`scape boot_pa_usage_diff`: percentile bootstrap intervals of the difference of every pA site's usage between two
cell populations (scape_amd/report.py, section boot_pa_len_diff, boot_pa_usage_diff; kernel k_rep_boot_usage_diff and the
entry point scape_hip_report_boot_usage_diff of scape_amd/csrc/perm.inc).  The select on signed values, the refusals of
both new entry points and the helpers are in tests/test_report_bootlendiff.py.

The contract.  Populations, tested columns, cell[j], multiplicities and the rank rule as in that file.  Reported records
and lines are diff_pa's: two kept rows or more, reads in both populations, one line per kept row.  With c_ij the count of
kept row i at position j, m = 1 for b = 0:
    a_ig(b) = sum_{j in g} m(b, cell[j]) c_ij,   A_g(b) = sum_i a_ig(b)                                  g = 1, 2
    d_i(b) = (double)a_i1(b) / (double)A_1(b) - (double)a_i2(b) / (double)A_2(b),  +infinity when either A is 0
One series per kept row; the columns are stated at `oracle_lines`.  Two correctly rounded divisions and one subtraction
of exact integers: every comparison is by equality, bits or text."""
import csv
import functools
import io
import os

import numpy as np
import pytest

import report_cases as rc
from report_cases import no_gpu  # noqa: F401  (fixture)
from test_report_bootlen import _p, interval, level_bp, mult
from test_report_bootlendiff import (EP_CHUNKS, EP_KEPT, EP_POPS, EP_SEED, _boot_usage_diff, all_values, as_text,
                                     batch_chunk_and_seed_invariance, check_syn, diff_command, ep_case,
                                     help_and_import_path, in_chunks, prerequisites_and_argument_errors, same_bits,
                                     same_text, subtract, swapped_idents, two_populations)
from test_report_bootusage import _boot_usage, usage_values

HEADER = ["gene", "pa_info", "versus", "num_pa", "reads.1", "reads.2", "gene_reads.1", "gene_reads.2", "usage.1",
          "usage.2", "delta_usage", "delta_usage_lo", "delta_usage_hi", "n_empty", "n_boot", "level"]
SHARED = ["gene", "pa_info", "versus", "usage.1", "usage.2", "delta_usage"]       # diff_pa's text
CMD = "boot_pa_usage_diff"


# ---------------------------------------------------------------- the contract, restated
def usage_diff_values(sub, n1, M):
    """d_i(b) [kept rows, replicates] from the counts sub [kept rows, positions], population 1's n1 positions and the
    multiplicities M [replicates, positions]"""
    u, _a, _A = usage_values(sub, [0, n1, np.asarray(sub).shape[1]], M)
    return np.stack([subtract(u_i) for u_i in u])


def oracle_lines(records, bc, clu_text, id1, id2, n_boot, level, seed):
    """the file's lines as lists of text fields.  Columns: gene = gene_info_str; pa_info = diff_pa's; versus; num_pa =
    kept rows; reads.g = a_ig(0); gene_reads.g = A_g(0); usage.g = repr(a_ig(0) / A_g(0)); delta_usage = the integer
    a_i1 T - t_i A_1 over the f64 product A_1 A_2, one division (diff_pa's); delta_usage_lo / _hi = repr of lo / hi, empty
    when D = 0; n_empty = n_boot - D; n_boot; level = the option's text"""
    cell, n1, versus = two_populations(bc, clu_text, id1, id2)
    M = mult(seed, 1, n_boot, cell)
    L = level_bp(level)
    lines = []
    for rec, dense in zip(records, rc.dense_counts(records, rc.column_ids(bc))):
        sub = dense[:, cell]
        kept = [lb for lb in range(int(rec["K"])) if sub[lb].any()]
        a, b = sub[kept][:, :n1].sum(axis=1).tolist(), sub[kept][:, n1:].sum(axis=1).tolist()
        A, B = sum(a), sum(b)
        if len(kept) < 2 or A == 0 or B == 0:
            continue
        d = usage_diff_values(sub[kept], n1, M)
        for i, lb in enumerate(kept):
            lo, hi, D = interval(d[i], L)
            delta = float(a[i] * (A + B) - (a[i] + b[i]) * A) / (float(A) * float(B))
            lines.append([rec["gene_info_str"], rc.pa_info(rec, lb), versus, str(len(kept)), str(a[i]), str(b[i]), str(A),
                          str(B), repr(a[i] / A), repr(b[i] / B), repr(delta)] +
                         ([repr(lo), repr(hi)] if D else ["", ""]) + [str(n_boot - D), str(n_boot), level])
    return lines


# ---------------------------------------------------------------- CPU
def test_help_and_import_path():
    help_and_import_path(CMD, "BOOT_PA_USAGE_DIFF_HEADER", HEADER, "scape_hip_report_boot_usage_diff")


def test_prerequisites_and_argument_errors(tmp_path, no_gpu):
    prerequisites_and_argument_errors(CMD, tmp_path)


def test_purpose_on_the_oracle():
    """20 + 20 cells, two sites.  Where population 1 uses the second site and population 2 the first, the second site's
    interval lies wholly above 0 and the first site's is its mirror image; with the same table in both populations
    both contain 0"""
    rng = np.random.default_rng(2)
    n1 = n = 20
    M = mult(1, 1, 999, np.arange(2 * n))
    apart = np.zeros((2, 2 * n), dtype=np.int64)
    apart[1, :n1] = rng.integers(1, 5, n)
    apart[0, n1:] = rng.integers(1, 5, n)
    apart[0, :n1] = apart[1, n1:] = rng.random(n) < 0.2
    d = usage_diff_values(apart, n1, M)
    (lo0, hi0, D0), (lo1, hi1, D1) = interval(d[0], 9500), interval(d[1], 9500)
    print("apart", lo0, hi0, lo1, hi1)
    assert D0 == D1 == 999 and 0 < lo1 <= hi1 and lo0 <= hi0 < 0
    table = rng.integers(0, 4, (2, n))
    d = usage_diff_values(np.concatenate([table, table], axis=1), n1, M)
    for i in range(2):
        lo, hi, D = interval(d[i], 9500)
        print("same table", i, lo, hi)
        assert D == 999 and lo < 0 < hi


@functools.lru_cache(maxsize=None)
def _syn_lines(id1, id2, n_boot, level, seed, n_rec=None):
    records, bc, clu_text = rc.synthetic()
    return oracle_lines(records[:n_rec], bc, clu_text, id1, id2, n_boot, level, seed)


def _assert_purpose(lines):
    """GENE0..GENE3 of the synthetic directory (A uses its first site ten times as often as the other cells): the first
    site's interval of A minus B lies wholly above 0"""
    first = {}
    for ln in lines:
        first.setdefault(ln[0].split(":")[1], ln)
    for gene in ("GENE0", "GENE1", "GENE2", "GENE3"):
        print(gene, first[gene][10:13])
        assert 0 < float(first[gene][11]) <= float(first[gene][12]) and float(first[gene][10]) > 0, gene


def test_oracle_on_the_synthetic_directory():
    lines = _syn_lines("A", "B", 999, "95", 1)
    _assert_purpose(lines)
    assert max(int(ln[3]) for ln in lines) == 63 and len({ln[0] for ln in lines}) == 36
    assert len(lines) == 245 and all(ln[11] and float(ln[11]) <= float(ln[12]) for ln in lines)
    assert any(float(ln[12]) < 0 for ln in lines) and any(float(ln[11]) < 0 < float(ln[12]) for ln in lines)


# ---------------------------------------------------------------- GPU: the entry point
@pytest.mark.gpu
@pytest.mark.parametrize("sizes", EP_POPS, ids=["1+7", "5+5", "40+1"])
def test_boot_usage_diff(sizes):
    """scape_hip_report_boot_usage_diff on the hand-made matrix (records of 2, 3 and 8 kept rows take the kernel's
    register path, those of 9 and 63 its two walks), 270 replicates written in chunks of 150 and 120: t and a0 are
    exact, every value equals the oracle's bit for bit, and equals the numpy f64 difference of the two populations'
    values of a scape_hip_report_boot_usage call at G = 2 on the same rows"""
    from scape_amd import _lib
    m, cell, seg, M, t_want, a0_want = ep_case(sizes)
    n_boot, n_rows, n = sum(EP_CHUNKS), len(m["rows"]), sum(sizes)
    want = np.concatenate([usage_diff_values(m["dense"][m["roff"][r]:m["roff"][r + 1], :n], sizes[0], M)
                           for r in range(len(EP_KEPT))])
    ctx = _lib.default_context(None)
    try:
        rc.device_counts(ctx, m["Ks"], m["off"], m["lab"], m["cb"], m["n_cols"])
        _rc, t, a0 = in_chunks(ctx, cell, EP_SEED, EP_CHUNKS, lambda: _boot_usage_diff(ctx, m, 2, seg, n_boot))
        got = all_values(ctx, n_rows, n_boot)
        assert ctx.lib.scape_hip_report_boot_vals_get(ctx.h, n_rows, _p(np.zeros(n_boot))) != 0
        in_chunks(ctx, cell, EP_SEED, (n_boot,), lambda: _boot_usage(ctx, m, 2, seg, n_boot))
        parts = all_values(ctx, n_rows * 2, n_boot).reshape(n_rows, 2, n_boot)
    finally:
        ctx.lib.scape_hip_report_free(ctx.h)
    assert np.array_equal(t, t_want) and np.array_equal(a0, a0_want)
    same_bits(got, want, sizes)
    same_bits(got, np.stack([subtract(parts[k].T) for k in range(n_rows)]), sizes)
    fin = np.isfinite(want)
    one_sided = ((a0_want[:, 0] > 0) & (a0_want[:, 1] == 0)) | ((a0_want[:, 0] == 0) & (a0_want[:, 1] > 0))
    print(sizes, "defined", int(fin.sum()), "of", fin.size, "negative", int((want < 0).sum()))
    assert (want < 0).any() and ((want > 0) & fin).any() and fin[one_sided].any()
    assert 1 not in sizes or (fin.sum(axis=1) < n_boot).any()


# ---------------------------------------------------------------- GPU: the command
@pytest.mark.gpu
@pytest.mark.parametrize("id2", ["B", None], ids=["A_vs_B", "A_vs_rest"])
def test_synthetic_directory(id2, tmp_path):
    """999 replicates of 230 + 301 cells (with --idents_2) and of 230 + 341 (without): the whole file equals the
    oracle's text, the record of 63 kept rows included; read from the file, the planted sites' intervals lie above 0"""
    text, lines = check_syn(CMD, _syn_lines, HEADER, tmp_path, "A", id2, 999, "95", 1, f"syn/{id2}")
    assert max(int(ln[3]) for ln in lines) == 63 and len(lines) > 150
    _assert_purpose(list(csv.reader(io.StringIO(text)))[1:])
    assert os.path.exists(os.path.join(str(tmp_path), f"syn_groups.gene.A_vs_{id2 or 'rest'}.boot_pa_usage_diff.csv"))
    assert lines[0][2] == ("A_Vs_B" if id2 else "A") and lines[0][14:] == ["999", "95"]


@pytest.mark.gpu
def test_small_directory_utr(tmp_path):
    """res.utr.pkl, 15 + 25 cells, level 99.5 and the largest seed"""
    path, clu_text, bc, records, _ids = rc.small_dir(tmp_path, 40, 15, 6)
    text = diff_command(CMD, tmp_path, path, "res.utr.pkl", "B", "A", 299, "99.5", 2 ** 64 - 1)
    lines = oracle_lines(records, bc, clu_text, "B", "A", 299, "99.5", 2 ** 64 - 1)
    same_text(text, as_text(lines, HEADER), "small")
    assert len(lines) == sum(2 + r % 4 for r in range(8)) and lines[0][15] == "99.5"
    assert os.path.exists(os.path.join(str(tmp_path), "small.utr.B_vs_A.boot_pa_usage_diff.csv"))


@pytest.mark.gpu
@pytest.mark.parametrize("n_boot", [1, 255, 256, 257])
def test_tile_edges(n_boot, tmp_path):
    """a workgroup of k_rep_boot_usage_diff takes 256 replicates: one, one short of a tile, a full tile and one over"""
    _text, lines = check_syn(CMD, _syn_lines, HEADER, tmp_path, "C", "A", n_boot, "95", 5, f"tile/{n_boot}", n_rec=12)
    assert len(lines) > 25


@pytest.mark.gpu
def test_batch_chunk_and_seed_invariance(tmp_path, monkeypatch):
    """records split over several count batches, the record of 63 kept rows alone in its own, and the replicates over
    several chunks: the same bytes.  Another seed changes the two interval columns and n_empty only"""
    # the record of K = 63: 63 x 600 x 12 bytes of counts and 63 x 299 x 8 of values
    batch_chunk_and_seed_invariance(CMD, "scape_hip_report_boot_usage_diff", [11, 12], 13, tmp_path, monkeypatch, 1 << 19)


@pytest.mark.gpu
def test_swapped_idents(tmp_path):
    """B against A: lo' = -hi and hi' = -lo, as floats (the sign of a zero flips)"""
    assert swapped_idents(CMD, 11, [], [0, 1, 3, 13], tmp_path) > 150


@pytest.mark.gpu
@pytest.mark.parametrize("id2", ["B", None], ids=["A_vs_B", "A_vs_rest"])
def test_shared_columns_are_diff_pa_s(id2, tmp_path):
    """pa_info, versus, usage.1, usage.2 and delta_usage are diff_pa's text, line for line"""
    path = rc.write_synthetic(tmp_path)
    mine = list(csv.DictReader(io.StringIO(diff_command(CMD, tmp_path, path, "res.gene.pkl", "A", id2, 99, "95", 1))))
    theirs = list(csv.DictReader(io.StringIO(rc.perm_command("diff_pa", tmp_path, path, "res.gene.pkl", "A", id2, 9, 1))))
    assert len(mine) == len(theirs) > 150
    assert [[r[c] for c in SHARED] for r in mine] == [[r[c] for c in SHARED] for r in theirs]
