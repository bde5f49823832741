"""`scape boot_pa_usage`: percentile bootstrap intervals of every pA site's usage per cell population, by resampling the
cells (scape_amd/report.py, section boot_pa_usage; kernel k_rep_boot_usage and the entry point
scape_hip_report_boot_usage of scape_amd/csrc/perm.inc, behind boot_pa_len's k_rep_boot_mult and k_rep_boot_select).

The contract.  Options, populations, tested columns, cell[j] and the multiplicities m(b, c) are boot_pa_len's
(tests/test_report_bootlen.py): replicate b is the same resampled data set.  Kept rows of a record: the labels < K with
a read in a tested cell; reported when there are two or more (positions play no part: no span condition).  With c_ij the
count of kept row i at position j, m = 1 for b = 0:
    a_ig(b) = sum_{j in g} m(b, cell[j]) c_ij,   A_g(b) = sum_i a_ig(b)            exact integers, A <= 15 T < 2^31
    u_ig(b) = (double)a_ig(b) / (double)A_g(b),  +infinity when A_g(b) = 0
    D_g = #{b in 1..n_boot: A_g(b) > 0},   k = max(1, (D_g + 1)(10000 - L) // 20000),   L = the level in basis points
    lo = the k-th smallest of the n_boot values u_ig(1..n_boot),   hi = the (D_g + 1 - k)-th;   no interval when D_g = 0
One line per reported record, kept row and population with A_g(0) > 0: records in file order, kept rows by ascending
label, populations in their order; the columns are stated at `oracle_lines`.

Nothing rounds but the one division, so the numpy oracle below (integer matrix products, one f64 division, np.sort)
gives the device's values to the bit and the file as exact text: no test of this file has a tolerance."""
import csv
import functools
import io
import os

import numpy as np
import pytest

import report_cases as rc
from report_cases import no_gpu, run as _run  # noqa: F401  (no_gpu: fixture)
from test_report_bootlen import (_bits, _boot_len, _boot_mult, _p, _quantiles, _reads_of, _vals_get, interval, level_bp,
                                 mult)
from test_report_diffgroups import populations_all

HEADER = ["gene", "pa_info", "group", "num_pa", "reads", "gene_reads", "usage", "usage_lo", "usage_hi", "n_empty",
          "n_boot", "level"]
PLANTED = ("GENE0", "GENE1", "GENE2", "GENE3")


# ---------------------------------------------------------------- the contract, restated
def usage_values(sub, seg, M):
    """(u [kept rows, replicates, G] as f64, a [kept rows, replicates, G], A [replicates, G]) from the counts sub [kept
    rows, positions], the segment offsets and the multiplicities M [replicates, positions]: integer matrix products,
    then one division.  A is formed on its own, from the column sums, and must be the sum of the a"""
    sub, M = np.asarray(sub, dtype=np.int64), M.astype(np.int64)
    n, G = sub.shape[1], len(seg) - 1
    one = np.zeros((n, G), dtype=np.int64)
    for g in range(G):
        one[seg[g]:seg[g + 1], g] = 1
    a = np.stack([M @ (one * row[:, None]) for row in sub])
    A = M @ (one * sub.sum(axis=0)[:, None])
    assert np.array_equal(a.sum(axis=0), A) and A.max(initial=0) < 1 << 31
    with np.errstate(divide="ignore", invalid="ignore"):
        u = a.astype(np.float64) / A.astype(np.float64)[None]
    u[:, A == 0] = np.inf
    assert np.all((u[:, A > 0] >= 0) & (u[:, A > 0] <= 1))
    return u, a, A


def oracle_lines(records, bc, clu_text, idents, n_boot, level, seed):
    """the file's lines as lists of text fields.  Columns: gene = gene_info_str; pa_info = diff_pa's; group; num_pa =
    kept rows; reads = a_ig(0); gene_reads = A_g(0); usage = repr(a_ig(0) / A_g(0)); usage_lo / _hi = repr of lo / hi,
    empty when D_g = 0; n_empty = n_boot - D_g; n_boot; level = the option's text.  clu_text = None: one population
    all_cell of every column"""
    col_ids = rc.column_ids(bc)
    pops = [("all_cell", list(range(len(col_ids))))] if clu_text is None else populations_all(bc, clu_text, idents)
    cell = np.array([j for _n, cols in pops for j in cols], dtype=np.int64)
    seg = np.concatenate([[0], np.cumsum([len(cols) for _n, cols in pops])])
    M = mult(seed, 1, n_boot, cell)
    L = level_bp(level)
    lines = []
    for rec, dense in zip(records, rc.dense_counts(records, col_ids)):
        sub = dense[:, cell]
        kept = [lb for lb in range(int(rec["K"])) if sub[lb].any()]
        if len(kept) < 2:
            continue
        u, _a, _A = usage_values(sub[kept], seg, M)
        a0 = np.stack([sub[kept][:, seg[g]:seg[g + 1]].sum(axis=1) for g in range(len(pops))], axis=1)
        A0 = a0.sum(axis=0)
        for i, lb in enumerate(kept):
            for g, (name, _cols) in enumerate(pops):
                if A0[g] == 0:
                    continue
                lo, hi, D = interval(u[i, :, g], L)
                lines.append([rec["gene_info_str"], rc.pa_info(rec, lb), name, str(len(kept)), str(int(a0[i, g])),
                              str(int(A0[g])), repr(int(a0[i, g]) / int(A0[g]))] +
                             ([repr(lo), repr(hi)] if D else ["", ""]) + [str(n_boot - D), str(n_boot), level])
    return lines


def as_text(lines):
    out = io.StringIO()
    w = csv.writer(out, delimiter=',', quoting=csv.QUOTE_MINIMAL, lineterminator='\n')
    w.writerow(HEADER)
    w.writerows(lines)
    return out.getvalue()


# ---------------------------------------------------------------- the command
def _args(root, clu=None, res="res.gene.pkl", idents=(), n_boot=None, level=None, seed=None, cmd="boot_pa_usage"):
    a = [cmd, "--output_dir", str(root), "--res_pkl_file", res]
    if clu is not None:
        a += ["--cell_cluster_file", str(clu)]
    for i in idents:
        a += ["--idents", i]
    for opt, v in (("--n_boot", n_boot), ("--level", level), ("--seed", seed)):
        if v is not None:
            a += [opt, str(v)]
    return a


def _path(root, clu, res, idents=(), cmd="boot_pa_usage"):
    kind = res[len("res."):-len(".pkl")]
    if clu is None:
        return os.path.join(str(root), f"all_cell.{kind}.{cmd}.csv")
    stem = os.path.splitext(os.path.basename(str(clu)))[0]
    tag = "." + "+".join(idents) if idents else ""
    return os.path.join(str(root), f"{stem}.{kind}{tag}.{cmd}.csv")


def _command(root, clu, res, idents, n_boot, level, seed, what="", cmd="boot_pa_usage"):
    r = _run(_args(root, clu, res, idents, n_boot, level, seed, cmd))
    assert r.exit_code == 0, (what, r.output, repr(r.exception))
    assert not rc.parts_left(root)
    with open(_path(root, clu, res, idents, cmd), newline="") as fh:
        return fh.read()


# ---------------------------------------------------------------- CPU
def test_help_and_import_path():
    r = _run(["--help"])
    assert r.exit_code == 0 and "boot_pa_usage" in r.output
    r = _run(["boot_pa_usage", "--help"])
    assert r.exit_code == 0, r.output
    for o in ("--output_dir", "--res_pkl_file", "--cell_cluster_file", "--idents", "--n_boot", "--level", "--seed"):
        assert o in r.output
    assert "--strata_file" not in r.output and "--n_perm" not in r.output
    flat = " ".join(r.output.split())
    assert "[default: 9999]" in flat and "[default: 95]" in flat and "[default: 1]" in flat
    import scape.utils as su
    from scape_amd import _lib, report
    assert su.boot_pa_usage is report.boot_pa_usage
    assert "scape_hip_report_boot_usage" in _lib.SIGNATURES
    assert report.BOOT_PA_USAGE_HEADER == HEADER


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
    from scape_amd import report
    with pytest.raises(ValueError, match="idents needs a cell_cluster_file"):
        report._boot_pa_usage(str(tmp_path), "res.gene.pkl", None, ("A",))
    ids = list(range(100, 166))
    (tmp_path / "barcode_index.csv").write_text("CB,index\n" + "".join(f"C{i}-1,{i}\n" for i in ids))
    clu.write_text("index,group\n" + "".join(f"{i},g{i}\n" for i in ids[:65]))
    r = _run(_args(tmp_path, clu))
    assert isinstance(r.exception, ValueError) and "65 clusters: boot_pa_usage" in str(r.exception)
    assert "--idents" in str(r.exception)
    r = _run(_args(tmp_path, clu) + ["--strata_file", str(clu)])
    assert r.exit_code == 2 and "--strata_file" in r.output
    r = _run(["boot_pa_usage", "--res_pkl_file", "res.gene.pkl"])
    assert r.exit_code == 2 and "--output_dir" in r.output
    assert sorted(os.listdir(tmp_path)) == ["barcode_index.csv", "groups.csv", "res.gene.pkl"]


@functools.lru_cache(maxsize=None)
def _syn_lines(idents, n_boot, level, seed, all_cell=False, n_rec=None):
    records, bc, clu_text = rc.synthetic()
    return oracle_lines(records[:n_rec], bc, None if all_cell else clu_text, idents, n_boot, level, seed)


def _first_site_intervals(lines):
    """{(gene name, group): (lo, hi)} of the first kept row of every record, from lines of text fields"""
    out = {}
    for ln in lines:
        key = (ln[0].split(":")[1], ln[2])
        if key not in out:
            out[key] = (float(ln[7]), float(ln[8]))
    return out


def _assert_purpose(lines):
    """records 0..3 of the synthetic directory (A uses its first site ten times as often): cluster A's interval of the
    first site lies wholly above cluster B's"""
    first = _first_site_intervals(lines)
    for gene in PLANTED:
        (a_lo, a_hi), (b_lo, b_hi) = first[(gene, "A")], first[(gene, "B")]
        print(gene, "A", a_lo, a_hi, "B", b_lo, b_hi)
        assert b_lo <= b_hi < a_lo <= a_hi, gene


def test_oracle_on_the_synthetic_directory():
    """n_boot = 999, seed 1, level 95, all clusters: the shape of the file and its purpose (usage_values asserts that a
    record's a_ig(b) sum to A_g(b) in every replicate)"""
    lines = _syn_lines((), 999, "95", 1)
    _assert_purpose(lines)
    first = _first_site_intervals(lines)
    assert [round(v, 3) for v in first[("GENE0", "A")] + first[("GENE0", "B")]] == [0.480, 0.626, 0.032, 0.151]
    n_empty, no_read = sum(int(ln[9]) > 0 for ln in lines), sum(ln[4] == "0" for ln in lines)
    print("lines", len(lines), "n_empty > 0", n_empty, "reads = 0", no_read)
    assert n_empty >= 1 and no_read >= 1
    assert (len(lines), n_empty, no_read) == (739, 32, 22)
    assert max(int(ln[3]) for ln in lines) == 63
    for ln in lines:
        if ln[4] == "0":
            assert ln[6] == "0.0" and (ln[7] == "0.0" or ln[7] == "")


# ---------------------------------------------------------------- GPU: the entry points
EP_CHUNKS = (150, 120)                    # 270 replicates: one tile of 256 and a part, written in two chunks
EP_SEED = 77
EP_N = 150                                # tested columns, in front of 5 others that hold reads too
EP_KEPT = (2, 3, 5, 8, 9, 63)             # 8 and 9: the two sides of the kernel's one-walk limit of 8 kept rows
EP_FRONT = (0, 1, 3, 4, 5, 8, 9, 9, 4, 1)  # nonzeros of the first ten kept rows in the columns 0..8


def ep_sizes(G):
    """segments over the 150 tested columns: the columns 0..8 first (where the nonzeros per row are set by hand), then
    what the others leave, then one cell each (the last of them column 149)"""
    if G == 1:
        return [EP_N]
    if G == 2:
        return [9, EP_N - 9]
    return [9, EP_N - 9 - (G - 2)] + [1] * (G - 2)


@functools.lru_cache(maxsize=None)
def ep_matrix():
    """records of 2, 3, 5, 8, 9 and 63 kept rows over 150 tested columns.  In the columns 0..8 the first ten kept rows
    (records 0..2) have 0, 1, 3, 4, 5, 8, 9, 9, 4 and 1 nonzeros: both sides of the walk's unroll of 4; record 4 has no
    read there (with G >= 2 a population without a read: every value +infinity).  Records 0 and 1 have no read in
    column 149, the last single-cell population.  Record 0 has a label whose reads all lie in untested columns (not a
    kept row), and one count is above 2^16"""
    rng = np.random.default_rng(5)
    n_cols = EP_N + 5
    Ks = np.array([3, 3, 5, 8, 9, 63], dtype=np.int32)
    base = np.concatenate([[0], np.cumsum(Ks)])
    shape = (int(Ks.sum()), n_cols)
    dense = ((rng.random(shape) < 0.15) * rng.integers(1, 4, shape)).astype(np.int64)
    kept = [np.array([0, 2]) + base[0]] + [np.arange(K) + base[r] for r, K in enumerate(Ks.tolist()) if r]
    dense[base[0] + 1, :EP_N] = 0
    dense[base[0] + 1, EP_N:] = 2
    rows = np.concatenate(kept).astype(np.int64)
    roff = np.concatenate([[0], np.cumsum([len(k) for k in kept])]).astype(np.int64)
    assert tuple(np.diff(roff).tolist()) == EP_KEPT
    for k, c in enumerate(EP_FRONT):
        dense[rows[k], :9] = 0
        dense[rows[k], rng.permutation(9)[:c]] = rng.integers(1, 4, c)
    dense[rows[roff[4]:roff[5]], :9] = 0
    dense[base[5]:, :9] = (rng.random((63, 9)) < 0.3) * rng.integers(1, 4, (63, 9))
    dense[:base[2], EP_N - 1] = 0
    dense[base[2]:, EP_N - 1] = (rng.random(int(Ks.sum()) - base[2]) < 0.5) * 2
    dense[rows, 20 + np.arange(len(rows)) % 100] += 1                 # every kept row has a read
    dense[rows[3], 40] = 70000
    assert [int((dense[rows[k], :9] > 0).sum()) for k in range(10)] == list(EP_FRONT)
    off, lab, cb = _reads_of(dense, Ks)
    return dict(Ks=Ks, off=off, lab=lab, cb=cb, n_cols=n_cols, rows=rows, roff=roff, n=EP_N, dense=dense)


@functools.lru_cache(maxsize=None)
def ep_case(G, n_boot=sum(EP_CHUNKS), n_rec=len(EP_KEPT)):
    """(matrix, cell, seg, per record (u [rows, n_boot, G], t, a0)) of the first n_rec records"""
    m = ep_matrix()
    cell = (7 * np.arange(EP_N) + 3).astype(np.int32)
    seg = np.concatenate([[0], np.cumsum(ep_sizes(G))]).astype(np.int32)
    assert seg[-1] == EP_N
    M = mult(EP_SEED, 1, n_boot, cell)
    recs = []
    for r in range(n_rec):
        sub = m["dense"][m["rows"][m["roff"][r]:m["roff"][r + 1]], :EP_N]
        u, _a, _A = usage_values(sub, seg, M)
        a0 = np.stack([sub[:, seg[g]:seg[g + 1]].sum(axis=1) for g in range(G)], axis=1)
        recs.append((u, sub.sum(axis=1), a0))
    return m, cell, seg, recs


def _boot_usage(ctx, m, G, seg, n_boot, roff=None, rows=None):
    roff, rows = m["roff"] if roff is None else roff, m["rows"] if rows is None else rows
    t, a0 = np.full(len(rows), -1, np.int64), np.full((len(rows), G), -1, np.int64)
    rc_ = ctx.lib.scape_hip_report_boot_usage(ctx.h, len(roff) - 1, _p(roff), _p(rows), G, _p(seg), n_boot, _p(t),
                                              _p(a0))
    return rc_, t, a0


def _check_record_set(ctx, G, n_boot, recs, t, a0, levels):
    """t, a0, every value and the intervals at `levels` of the record set on the device against the oracle's"""
    n_rows = sum(len(r[1]) for r in recs)
    got = np.stack([_vals_get(ctx, k, n_boot) for k in range(n_rows * G)]).reshape(n_rows, G, n_boot)
    quant = {L: _quantiles(ctx, L, n_rows * G) for L in levels}
    assert np.array_equal(t, np.concatenate([r[1] for r in recs]))
    assert np.array_equal(a0, np.concatenate([r[2] for r in recs]))
    want = np.concatenate([r[0] for r in recs]).transpose(0, 2, 1)          # [row, G, n_boot]
    assert np.array_equal(_bits(got), _bits(want)), (G, n_boot, np.argwhere(_bits(got) != _bits(want))[:5])
    for L, (rc_, lo, hi, D) in quant.items():
        assert rc_ == 0
        for k in range(n_rows):
            for g in range(G):
                w = interval(want[k, g], L)
                s = k * G + g
                assert (_bits(lo[s:s + 1])[0], _bits(hi[s:s + 1])[0], int(D[s])) == \
                    (_bits([w[0]])[0], _bits([w[1]])[0], w[2]), (G, L, k, g)
    return want


@pytest.mark.gpu
@pytest.mark.parametrize("G", [1, 2, 3, 33, 64])
def test_boot_usage(G):
    """scape_hip_report_boot_usage on the hand-made matrix, 270 replicates written in chunks of 150 and 120: t and a0
    are exact, every series equals the oracle bit for bit, and so do lo, hi and D at 9500 and 5000 basis points.  The
    records of 2, 3, 5 and 8 kept rows take the kernel's one-walk path, those of 9 and 63 its two walks.  With
    two populations or more a record has a population without a read (every value +infinity, D = 0); with three or more
    there is a population of one cell (about 37 % of its replicates empty)"""
    from scape_amd import _lib
    m, cell, seg, recs = ep_case(G)
    n_boot = sum(EP_CHUNKS)
    ctx = _lib.default_context(None)
    try:
        rc.device_counts(ctx, m["Ks"], m["off"], m["lab"], m["cb"], m["n_cols"])
        first = 1
        for b_count in EP_CHUNKS:
            _lib.check(_boot_mult(ctx, cell, first, b_count, EP_SEED), "boot_mult")
            rc_, t, a0 = _boot_usage(ctx, m, G, seg, n_boot)
            _lib.check(rc_, "boot_usage")
            first += b_count
        want = _check_record_set(ctx, G, n_boot, recs, t, a0, (9500, 5000))
    finally:
        ctx.lib.scape_hip_report_free(ctx.h)
    D = np.isfinite(want).sum(axis=2)                                       # [row, G]
    one_cell = np.diff(seg) == 1
    seen = dict(empty=bool((D == 0).any()), zero_site=bool(((want == 0).all(axis=2) & (D > 0)).any()),
                one_cell=bool(((D[:, one_cell] > 0.5 * n_boot) & (D[:, one_cell] < 0.75 * n_boot)).any()))
    print(G, seen)
    assert G < 2 or seen["empty"]
    assert G < 3 or all(seen.values()), seen


@pytest.mark.gpu
@pytest.mark.parametrize("n_boot", [1, 255, 256, 257])
def test_tile_edges(n_boot):
    """a workgroup of k_rep_boot_usage takes 256 replicates: one, one short of a tile, a full tile and one over, on the
    two smallest records, in one chunk"""
    from scape_amd import _lib
    m, cell, seg, recs = ep_case(3, n_boot, 2)
    roff, rows = m["roff"][:3].copy(), m["rows"][:int(m["roff"][2])].copy()
    ctx = _lib.default_context(None)
    try:
        rc.device_counts(ctx, m["Ks"], m["off"], m["lab"], m["cb"], m["n_cols"])
        _lib.check(_boot_mult(ctx, cell, 1, n_boot, EP_SEED), "boot_mult")
        rc_, t, a0 = _boot_usage(ctx, m, 3, seg, n_boot, roff, rows)
        _lib.check(rc_, "boot_usage")
        _check_record_set(ctx, 3, n_boot, recs, t, a0, (9500, 5000))
    finally:
        ctx.lib.scape_hip_report_free(ctx.h)


def _ep_positions(m):
    return np.random.default_rng(3).integers(0, (1 << 22) + 1, len(m["rows"])).astype(np.int32)


@pytest.mark.gpu
def test_refusals():
    """each refused call returns non-zero with its entry point's name in the message, and the valid calls before and
    after it give the same outputs"""
    from scape_amd import _lib
    G, n_boot = 3, 270
    m, cell, seg, _recs = ep_case(G)
    q = _ep_positions(m)
    n_series = len(m["rows"]) * G
    ctx = _lib.default_context(None)
    lib = ctx.lib
    entry = "scape_hip_report_boot_usage"

    def build(b_first=1, b_count=n_boot):
        return _boot_mult(ctx, cell, b_first, b_count, EP_SEED)

    def good():
        _lib.check(build(), "boot_mult")
        rc_, t, a0 = _boot_usage(ctx, m, G, seg, n_boot)
        _lib.check(rc_, "boot_usage")
        rc_, lo, hi, D = _quantiles(ctx, 9500, n_series)
        _lib.check(rc_, "boot_quantiles")
        return [a.tobytes() for a in (t, a0, lo, hi, D, _vals_get(ctx, 4, n_boot),
                                      _vals_get(ctx, n_series - 1, n_boot))]

    def refused(rc_, name, word):
        assert rc_ != 0 and name in _lib.last_error() and word in _lib.last_error(), _lib.last_error()

    def changed(a, k, v):
        b = a.copy()
        b[k] = v
        return b
    try:
        refused(_boot_usage(ctx, m, G, seg, n_boot)[0], entry, "report_counts")
        rc.device_counts(ctx, m["Ks"], m["off"], m["lab"], m["cb"], m["n_cols"])
        refused(_boot_usage(ctx, m, G, seg, n_boot)[0], entry, "boot_mult has not been called")
        refused(_quantiles(ctx, 9500, n_series)[0], "scape_hip_report_boot_quantiles", "boot_len has not been called")
        first = good()
        refused(_boot_usage(ctx, m, 0, seg[:1].copy(), n_boot)[0], entry, "n_groups")
        seg65 = np.concatenate([np.arange(65), [m["n"]]]).astype(np.int32)
        refused(_boot_usage(ctx, m, 65, seg65, n_boot)[0], entry, "n_groups")
        refused(_boot_usage(ctx, m, G, changed(seg, 3, seg[3] - 1), n_boot)[0], entry, "seg_off")
        refused(_boot_usage(ctx, m, G, changed(seg, 2, seg[1] - 1), n_boot)[0], entry, "non-decreasing")
        refused(_boot_usage(ctx, m, G, changed(seg, 0, 1), n_boot)[0], entry, "seg_off must start at 0")
        refused(_boot_usage(ctx, m, G, seg, n_boot - 1)[0], entry, "n_boot")
        refused(_boot_usage(ctx, m, G, seg, n_boot, rows=changed(m["rows"], 5, int(m["Ks"].sum())))[0], entry,
                "row index out of range")
        refused(lib.scape_hip_report_boot_vals_get(ctx.h, n_series, _p(np.zeros(n_boot))),
                "scape_hip_report_boot_vals_get", "series")
        # a record of 2^27 reads, built from few large counts: the heaviest kept row, 2^27 / its reads times over
        t_rows = np.frombuffer(first[0], dtype=np.int64)
        heavy_row, reads = int(m["rows"][int(np.argmax(t_rows))]), int(t_rows.max())
        assert reads > 70000
        heavy = np.full(-(-(1 << 27) // reads), heavy_row, dtype=np.int64)
        rc_, _t, _a0 = _boot_usage(ctx, m, G, seg, n_boot, np.array([0, len(heavy)], np.int64), heavy)
        refused(rc_, entry, "2^27 or more reads")
        assert good() == first
        # quantiles before every column is written: a record set begun with 150 of the 270 replicates
        _lib.check(build(1, 150), "boot_mult")
        _lib.check(_boot_usage(ctx, m, G, seg, n_boot)[0], "boot_usage")
        refused(_quantiles(ctx, 9500, n_series)[0], "scape_hip_report_boot_quantiles", "replicate 151")
        _lib.check(build(151, 120), "boot_mult")
        refused(_boot_usage(ctx, m, G, seg, n_boot, m["roff"][:3].copy(), m["rows"][:int(m["roff"][2])].copy())[0],
                entry, "later chunk")
        # a boot_len chunk behind a boot_usage record set; one series per row there, so the numbers alone would pass
        one_each = np.arange(len(m["rows"]) + 1, dtype=np.int64)
        refused(_boot_len(ctx, m, G, seg, q, n_boot, one_each, m["rows"])[0], "scape_hip_report_boot_len",
                "later chunk")
        _lib.check(_boot_usage(ctx, m, G, seg, n_boot)[0], "boot_usage")
        rc_, lo, hi, D = _quantiles(ctx, 9500, n_series)
        assert rc_ == 0 and [a.tobytes() for a in (lo, hi, D)] == first[2:5]
        # and the reverse: a boot_usage chunk behind a boot_len record set of as many series
        _lib.check(build(1, 150), "boot_mult")
        _lib.check(_boot_len(ctx, m, G, seg, q, n_boot, one_each, m["rows"])[0], "boot_len")
        _lib.check(build(151, 120), "boot_mult")
        refused(_boot_usage(ctx, m, G, seg, n_boot)[0], entry, "later chunk")
        assert good() == first
    finally:
        lib.scape_hip_report_free(ctx.h)


@pytest.mark.gpu
def test_record_sets_share_and_reset_one_state():
    """the values' array, its written columns and the select are shared by boot_len and boot_usage: after a record set
    of the one, a fresh record set of the other returns what it returns in a context of its own"""
    from scape_amd import _lib
    G, n_boot = 3, 270
    m, cell, seg, recs = ep_case(G)
    q = _ep_positions(m)
    n_rec, n_rows = len(recs), len(m["rows"])

    def run(ctx, usage):
        _lib.check(_boot_mult(ctx, cell, 1, n_boot, EP_SEED), "boot_mult")
        rc_, t, a0 = _boot_usage(ctx, m, G, seg, n_boot) if usage else _boot_len(ctx, m, G, seg, q, n_boot)
        _lib.check(rc_, "boot_usage" if usage else "boot_len")
        n_series = (n_rows if usage else n_rec) * G
        rc_, lo, hi, D = _quantiles(ctx, 9500, n_series)
        _lib.check(rc_, "boot_quantiles")
        assert ctx.lib.scape_hip_report_boot_vals_get(ctx.h, n_series, _p(np.zeros(n_boot))) != 0
        return [a.tobytes() for a in (t, a0, lo, hi, D)] + \
            [_vals_get(ctx, k, n_boot).tobytes() for k in range(n_series)]
    alone = {}
    for usage in (False, True):
        ctx = _lib.default_context(None)
        try:
            rc.device_counts(ctx, m["Ks"], m["off"], m["lab"], m["cb"], m["n_cols"])
            alone[usage] = run(ctx, usage)
        finally:
            ctx.lib.scape_hip_report_free(ctx.h)
    assert alone[False] != alone[True]
    ctx = _lib.default_context(None)
    try:
        rc.device_counts(ctx, m["Ks"], m["off"], m["lab"], m["cb"], m["n_cols"])
        for usage in (True, False, True, False):
            assert run(ctx, usage) == alone[usage], usage
    finally:
        ctx.lib.scape_hip_report_free(ctx.h)


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
def test_synthetic_directory_all_clusters_idents_and_purpose(tmp_path):
    """999 replicates of 230 + 301 + 40 cells in the clusters A, B, C: the whole file equals the oracle's text; read
    from the file, cluster A's interval of the first site of GENE0..GENE3 lies above cluster B's.  With --idents C
    --idents A the file equals the oracle's too, carries .C+A in its name and C's line of a site first, and every line
    is, byte for byte, the line of that gene, site and cluster in the all-cluster file"""
    text, lines = _check_syn(tmp_path, (), 999, "95", 1, "syn/all")
    assert {ln[2] for ln in lines} == {"A", "B", "C"} and max(int(ln[3]) for ln in lines) == 63
    assert any(int(ln[9]) > 0 for ln in lines) and any(ln[4] == "0" for ln in lines)
    _assert_purpose(list(csv.reader(io.StringIO(text)))[1:])
    assert os.path.basename(_path(tmp_path, "syn_groups.csv", "res.gene.pkl")) == "syn_groups.gene.boot_pa_usage.csv"
    both = {tuple(ln.split(",")[:3]): ln for ln in text.split("\n")[1:-1]}
    assert len(both) == len(lines)
    two, two_lines = _check_syn(tmp_path, ("C", "A"), 999, "95", 1, "syn/C+A")
    assert os.path.exists(os.path.join(str(tmp_path), "syn_groups.gene.C+A.boot_pa_usage.csv"))
    assert [ln[2] for ln in two_lines[:2]] == ["C", "A"]
    mine = two.split("\n")[1:-1]
    assert len(mine) > 300 and all(both[tuple(ln.split(",")[:3])] == ln for ln in mine)


@pytest.mark.gpu
def test_synthetic_directory_all_cell(tmp_path):
    """no cluster file: one population all_cell of all 600 columns, the cells without a cluster included"""
    _text, lines = _check_syn(tmp_path, (), 299, "90.00", 1, "syn/all_cell", all_cell=True)
    assert {ln[2] for ln in lines} == {"all_cell"} and lines[0][11] == "90.00"
    assert os.path.exists(os.path.join(str(tmp_path), "all_cell.gene.boot_pa_usage.csv"))


@pytest.mark.gpu
def test_level_and_largest_seed(tmp_path):
    """--level 99.5 and --seed 2^64 - 1 on the first 8 records"""
    _text, lines = _check_syn(tmp_path, (), 299, "99.5", 2 ** 64 - 1, "syn/99.5", n_rec=8)
    assert len(lines) > 30 and lines[0][11] == "99.5"


@pytest.mark.gpu
def test_batch_and_chunk_invariance(tmp_path, monkeypatch):
    """records split over several count batches, the record of 63 kept rows alone in its own, and the replicates over
    several chunks: the same bytes"""
    from scape_amd import _lib, report
    path = rc.write_synthetic(tmp_path)
    big = _command(tmp_path, path, "res.gene.pkl", (), 299, "95", 1)
    assert big == as_text(_syn_lines((), 299, "95", 1))
    lib = _lib.load_library()
    calls = {"mult": [], "usage": []}
    real_m, real_u = lib.scape_hip_report_boot_mult, lib.scape_hip_report_boot_usage

    def make_mult(*a):
        calls["mult"].append((a[3], a[4]))
        return real_m(*a)

    def boot_usage(*a):
        calls["usage"].append((a[1], int(a[2][a[1]])))                    # records and kept rows of the call
        return real_u(*a)
    monkeypatch.setattr(lib, "scape_hip_report_boot_mult", make_mult)
    monkeypatch.setattr(lib, "scape_hip_report_boot_usage", boot_usage)
    # the record of K = 63: 63 x 600 x 12 bytes of counts and 63 x 3 x 299 x 8 of values, each above 450 KB
    monkeypatch.setattr(report, "MAX_BATCH_BYTES", 1 << 19)
    monkeypatch.setattr(report, "MAX_PERM_BYTES", 1 << 30)
    assert _command(tmp_path, path, "res.gene.pkl", (), 299, "95", 1) == big
    assert calls["mult"] == [(1, 299)] and len(calls["usage"]) > 3 and calls["usage"][-1] == (1, 63), calls
    n_batches = len(calls["usage"])
    calls.update(mult=[], usage=[])
    monkeypatch.setattr(report, "MAX_PERM_BYTES", 571 * 100)             # one byte per tested cell: 100 replicates
    assert _command(tmp_path, path, "res.gene.pkl", (), 299, "95", 1) == big
    assert len(calls["usage"]) == 3 * n_batches and calls["mult"][:3] == [(1, 100), (101, 100), (201, 99)]


@pytest.mark.gpu
def test_agreement_with_the_neighbours(tmp_path):
    """same seed and idents: usage is diff_pa's usage.1 / usage.2 as text for every line of diff_pa --idents_1 A
    --idents_2 B, and n_empty is boot_pa_len's for every (gene, group) that it reports"""
    path = rc.write_synthetic(tmp_path)
    mine = list(csv.reader(io.StringIO(_command(tmp_path, path, "res.gene.pkl", ("A", "B"), 299, "95", 1))))[1:]
    by = {(ln[0], ln[1], ln[2]): ln for ln in mine}
    theirs = rc.perm_command("diff_pa", tmp_path, path, "res.gene.pkl", "A", "B", 9, 1)
    theirs = list(csv.DictReader(io.StringIO(theirs)))
    assert len(theirs) > 90
    for row in theirs:
        assert by[(row["gene"], row["pa_info"], "A")][6] == row["usage.1"], row
        assert by[(row["gene"], row["pa_info"], "B")][6] == row["usage.2"], row
    lens = list(csv.reader(io.StringIO(_command(tmp_path, path, "res.gene.pkl", ("A", "B"), 299, "95", 1,
                                                cmd="boot_pa_len"))))[1:]
    assert len(lens) > 60
    empty = {}
    for ln in mine:
        empty.setdefault((ln[0], ln[2]), set()).add(ln[9])
    assert all(len(v) == 1 for v in empty.values())
    for ln in lens:
        assert empty[(ln[0], ln[1])] == {ln[10]}, ln
