"""`scape ex_pa_len_mat`: the gene x cell matrix of the expected pA length as a 10x-style directory <res>.len/
(matrix.mtx.gz, reads.mtx.gz, features.tsv.gz, barcodes.tsv.gz).

The yardstick is a plain-Python restatement of the definition: the weights c_l / T, the terms (c_l / T) * n_l, the order
of numpy's pairwise sum, and '%.6f' in exact integers.  It is pinned, without a GPU, to the REFERENCE's own per-cell
answers: golden cases fuzz7 and fuzz23 (tests/golden/fixture_report.npz) ran the reference's cal_exp_pa_len with a
cluster file that puts every cell in a cluster of its own (grp_per_cell.csv).  The GPU tests compare the decompressed
files byte for byte: with those lines on the two golden cases, with the restatement on hand-made records."""
import functools
import gzip
import io
import math
import os
import struct

import numpy as np
import pandas as pd
import pytest

import report_cases as rc
from report_cases import no_gpu, parts_left as _parts_left, run as _run  # noqa: F401  (no_gpu is a fixture)

REAL_BANNER = "%%MatrixMarket matrix coordinate real general\n"
INT_BANNER = "%%MatrixMarket matrix coordinate integer general\n"
FILES = ("matrix.mtx.gz", "reads.mtx.gz", "features.tsv.gz", "barcodes.tsv.gz")
PER_CELL = ("fuzz7", "fuzz23")
MAX_N = 2.0 ** 31 / 9


# ---------------------------------------------------------------- the definition, restated
def pairwise(p):
    """sum of the list p in the order of numpy's pairwise sum"""
    n = len(p)
    if n < 8:
        res = 0.0
        for x in p:
            res = res + x
        return res
    if n <= 128:
        r = list(p[:8])
        i = 8
        while i < n - n % 8:
            for j in range(8):
                r[j] = r[j] + p[i + j]
            i += 8
        res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
        while i < n:
            res = res + p[i]
            i += 1
        return res
    n2 = n // 2
    n2 -= n2 % 8
    return pairwise(p[:n2]) + pairwise(p[n2:])


def n_arr_of(rec):
    """n_arr of exp_pa_len (apa_core.py:1051), the reference's numpy expression; None for K == 1"""
    if int(rec["K"]) == 1:
        return None
    a_arr = np.asarray(rec["alpha_arr"])
    with np.errstate(all="ignore"):
        return (1.0 + 9.0 * (a_arr - a_arr[0]) / (a_arr[-1] - a_arr[0])).tolist()


def has_values(n_arr):
    return n_arr is None or all(math.isfinite(x) and abs(x) < MAX_N for x in n_arr)


def exp_len(counts, n_arr):
    """the value of a cell with the counts c_0 .. c_{K-1} (Python ints, their sum above 0)"""
    if n_arr is None:
        return 1.0
    T = float(sum(counts))
    return 0.0 + pairwise([(float(c) / T) * n for c, n in zip(counts, n_arr)])     # numpy starts from its initial 0.0


def fixed6(v):
    """'%.6f' % v in integers: v = +-m 2^e, q = m 10^6 2^e rounded half to even"""
    bits = struct.unpack("<Q", struct.pack("<d", v))[0]
    sign, ex, frac = bits >> 63, (bits >> 52) & 0x7ff, bits & ((1 << 52) - 1)
    m, e = (frac, -1074) if ex == 0 else (frac | (1 << 52), ex - 1075)
    x = m * 10 ** 6
    if e >= 0:
        q = x << e
    else:
        q, rem, half = x >> -e, x & ((1 << -e) - 1), 1 << (-e - 1)
        if rem > half or (rem == half and q & 1):
            q += 1
    d = str(q).rjust(7, "0")
    return ("-" if sign else "") + d[:-6] + "." + d[-6:]


def cells_of(records, col_ids):
    """per record [(column, counts c_0 .. c_{K-1})] of the columns with T > 0, ascending; [] for a record without
    values"""
    out = []
    for rec, m in zip(records, rc.dense_counts(records, col_ids)):
        cols = np.nonzero(m.sum(axis=0))[0] if has_values(n_arr_of(rec)) else []
        out.append([(int(c), m[:, c].tolist()) for c in cols])
    return out


def expected_texts(records, bc_csv, value_text=None):
    """the four files.  value_text(record number, column) overrides the restatement's text of a value"""
    cbs = pd.read_csv(io.StringIO(bc_csv), index_col="index")["CB"].tolist()
    vals, reads = [], []
    for r, (rec, cells) in enumerate(zip(records, cells_of(records, rc.column_ids(bc_csv)))):
        n_arr = n_arr_of(rec)
        for c, counts in cells:
            txt = value_text(r, c) if value_text else fixed6(exp_len(counts, n_arr))
            vals.append(f"{r + 1} {c + 1} {txt}\n")
            reads.append(f"{r + 1} {c + 1} {sum(counts)}\n")
    head = f"{len(records)} {len(cbs)} {len(vals)}\n"
    names = [":".join(rec["gene_info_str"].split(":")[1:3]) for rec in records]
    return {"matrix.mtx.gz": REAL_BANNER + head + "".join(vals), "reads.mtx.gz": INT_BANNER + head + "".join(reads),
            "features.tsv.gz": "".join(f"{s}\t{s}\tGene Expression\n" for s in names),
            "barcodes.tsv.gz": "".join(f"{b}\n" for b in cbs)}


# ---------------------------------------------------------------- the reference's per-cell lines
def _case(name):
    return next(cs for cs in rc.fixture_cases() if cs["name"] == name)


@functools.lru_cache(maxsize=None)
def reference_lines(name):
    """per record of a per-cell golden case {cell id: exp_length text of the reference ('' = nan)}: the reference writes
    one line per record and cluster present among the record's reads, the clusters ("cell<id>") in np.unique's order"""
    cs = _case(name)
    text = cs["len_texts"][cs["len_names"].index("grp_per_cell." + cs["res"][len("res."):-len(".pkl")] + ".pa.len.csv")]
    lines = text.split("\n")[1:-1]
    out, at = [], 0
    for rec in cs["records"]:
        ids = sorted(set(int(i) for i in rec["cb_id_arr"]), key=lambda i: f"cell{i}")
        gene = ":".join(rec["gene_info_str"].split(":")[1:3])
        got = {}
        for i in ids:
            g, cell, val, num_pa = lines[at].split(",")
            assert (g, cell, int(num_pa)) == (gene, f"cell{i}", int(rec["K"])), (name, at, lines[at])
            got[i] = val
            at += 1
        out.append(got)
    assert at == len(lines)
    return out


@pytest.mark.parametrize("name", PER_CELL)
def test_restatement_vs_reference_per_cell_lines(name):
    """every (record, cell) line of the reference with a finite exp_length and T > 0 is the restatement's double
    exactly; its nan lines, and the K == 1 lines of cells whose reads all have label >= K, are exactly the pairs the
    restatement gives no entry"""
    cs = _case(name)
    bc = rc.text(rc.fixture(), cs["barcode"])
    col_ids = rc.column_ids(bc)
    col_of = {i: j for j, i in enumerate(col_ids)}
    n_values = 0
    for rec, cells, ref in zip(cs["records"], cells_of(cs["records"], col_ids), reference_lines(name)):
        n_arr = n_arr_of(rec)
        mine = {c: exp_len(counts, n_arr) for c, counts in cells}
        omitted = {col_of[i] for i in ref} - set(mine)
        lab, cb = np.asarray(rec["label_arr"]), np.asarray(rec["cb_id_arr"])
        no_site = {col_of[int(i)] for i in set(cb.tolist())} - {col_of[int(i)] for i in set(cb[lab < rec["K"]].tolist())}
        want_omitted = {col_of[i] for i, val in ref.items() if val == "" or (int(rec["K"]) == 1 and col_of[i] in no_site)}
        assert omitted == want_omitted, (name, rec["gene_info_str"])
        for i, val in ref.items():
            if col_of[i] in mine:
                assert val != "" and struct.pack("<d", float(val)) == struct.pack("<d", mine[col_of[i]]), \
                    (name, rec["gene_info_str"], i, val, mine[col_of[i]])
                n_values += 1
        assert set(mine) <= {col_of[i] for i in ref}
    assert n_values > 300


def test_restatement_order_and_text():
    """the pairwise order against np.sum (1-D and row-wise) at every length where it changes its path, and the integer
    formatter against '%.6f' on signs, ties, subnormals and random bit patterns"""
    rng = np.random.default_rng(3)
    for K in list(range(2, 40)) + [63, 64, 65, 127, 128, 129, 135, 136, 137, 150, 255, 256, 257, 300, 1000]:
        for trial in range(4):
            c = rng.integers(1, 400, K) * (rng.random(K) < 0.6)
            c[rng.integers(0, K)] += 1
            a = rng.integers(0, 5000, K).astype(np.float64)
            a[-1] = a[0] + 1 + rng.integers(0, 900)
            n_arr = 1.0 + 9.0 * (a - a[0]) / (a[-1] - a[0])
            ws = np.zeros(K)
            ws[:] = c
            ws = ws / np.sum(ws)
            got = struct.pack("<d", exp_len(c.tolist(), n_arr.tolist()))
            assert got == struct.pack("<d", float(np.sum(ws * n_arr))), K
            assert got == struct.pack("<d", float(np.sum((ws * n_arr).reshape(1, K), axis=1)[0])), K
    special = [0.0, -0.0, 1.0, 10.0, -19.04, 1.0390625, 1.1171875, 0.0000005, 0.0000015, -0.0000005, 2.5e-7, 5e-324,
               -5e-324, 2.0 ** 31 - 1, -(2.0 ** 31) + 0.5, 123456.7890125, 0.1, 1e-7, 4.9999995, 9.9999995, 99.9999995]
    bits = rng.integers(0, 1 << 63, 20000, dtype=np.int64).astype(np.uint64) | (rng.integers(0, 2, 20000).astype(np.uint64) << 63)
    rand = [v for v in bits.view(np.float64).tolist() if v == v and abs(v) < 2.0 ** 31]
    ties = [(k + 0.5) / 2 ** s for s in (1, 6, 7, 12) for k in range(-40, 40)]
    for v in special + rand + ties + rng.uniform(-30, 30, 20000).tolist():
        assert fixed6(v) == "%.6f" % v, v.hex()
    assert fixed6(1.0390625) == "1.039062" and fixed6(1.1171875) == "1.117188" and fixed6(-1e-9) == "-0.000000"


# ---------------------------------------------------------------- CPU: the command's surface
def _args(root, res="res.gene.pkl"):
    return ["ex_pa_len_mat", "--output_dir", str(root), "--res_pkl_file", res]


def _len_dir(root, res="res.gene.pkl"):
    return os.path.join(str(root), res.replace(".pkl", ".len"))


def _read_dir(root, res="res.gene.pkl"):
    out = {}
    for name in FILES:
        with gzip.open(os.path.join(_len_dir(root, res), name), "rt", newline="") as fh:
            out[name] = fh.read()
    return out


def test_help_lists_the_command():
    r = _run(["--help"])
    assert r.exit_code == 0 and "ex_pa_len_mat" in r.output
    r = _run(["ex_pa_len_mat", "--help"])
    assert r.exit_code == 0, r.output
    assert "--output_dir" in r.output and "--res_pkl_file" in r.output


def test_utils_reexports_the_command():
    import inspect
    import scape.utils as su
    from scape_amd import report
    assert su.ex_pa_len_mat is report.ex_pa_len_mat
    assert list(inspect.signature(report._ex_pa_len_mat).parameters) == ["output_dir", "res_pkl_file", "device"]


def test_prerequisites(tmp_path, no_gpu):
    """ex_pa_cnt_mat's checks, messages and order, all before the GPU; the directory is untouched afterwards"""
    r = _run(_args(tmp_path / "nope"))
    assert r.exit_code != 0 and "Given output_dir folder does not exists." in str(r.exception)
    r = _run(_args(tmp_path))
    assert "Given res_pkl_file is not in output_dir." in str(r.exception)
    r = _run(["ex_pa_len_mat", "--output_dir", str(tmp_path)])                     # default "None"
    assert "Invalid file" in str(r.exception) and "None" in str(r.exception)
    (tmp_path / "res.gene.pkl").write_bytes(b"")
    r = _run(_args(tmp_path))
    assert isinstance(r.exception, FileNotFoundError) and "barcode_index.csv" in str(r.exception)
    (tmp_path / "barcode_index.csv").write_text("CB,index\n")
    r = _run(_args(tmp_path))
    assert isinstance(r.exception, ValueError) and "lists no barcode" in str(r.exception)
    (tmp_path / "barcode_index.csv").write_text('CB,index\nA-1,0\n"B\tX-1",1\n')
    r = _run(_args(tmp_path))
    assert isinstance(r.exception, ValueError) and "B\\tX-1" in str(r.exception)
    assert sorted(os.listdir(tmp_path)) == ["barcode_index.csv", "res.gene.pkl"] and not _parts_left(tmp_path)


# ---------------------------------------------------------------- GPU
def _shrink(monkeypatch, block=1 << 12):
    """batches, render blocks and gzip members small enough that a directory takes several of each"""
    from scape_amd import report
    monkeypatch.setattr(report, "MAX_BATCH_BYTES", 1 << 14)
    monkeypatch.setattr(report, "MAX_BLOCK_BYTES", block)
    monkeypatch.setattr(report, "GZIP_PART", 1 << 11)


def _check_mmread(root, res, want):
    """both matrices load, hold the written numbers and have identical sparsity"""
    import scipy.io
    import scipy.sparse
    m = [scipy.sparse.coo_matrix(scipy.io.mmread(os.path.join(_len_dir(root, res), name)))
         for name in ("matrix.mtx.gz", "reads.mtx.gz")]
    ent = [ln.split() for ln in want["matrix.mtx.gz"].split("\n")[2:-1]]
    assert m[0].shape == m[1].shape == tuple(int(v) for v in want["matrix.mtx.gz"].split("\n")[1].split()[:2])
    assert m[0].nnz == m[1].nnz == len(ent)
    assert np.array_equal(m[0].row, m[1].row) and np.array_equal(m[0].col, m[1].col)
    assert np.array_equal(m[0].row, [int(e[0]) - 1 for e in ent]) and np.array_equal(m[0].col, [int(e[1]) - 1 for e in ent])
    assert np.array_equal(m[0].data, [float(e[2]) for e in ent]) and (m[1].data >= 1).all()


@pytest.mark.gpu
@pytest.mark.parametrize("name", PER_CELL)
def test_golden_per_cell_cases(name, tmp_path, monkeypatch):
    """the values are '%.6f' of the reference's own per-cell doubles, the reads are dense_counts summed over labels"""
    cs = _case(name)
    if name == "fuzz23":
        _shrink(monkeypatch)
    bc, _paths = rc.write_case(cs, tmp_path, {})
    r = _run(_args(tmp_path, cs["res"]))
    assert r.exit_code == 0, (name, r.output, repr(r.exception))
    col_ids = rc.column_ids(bc)
    ref = reference_lines(name)
    want = expected_texts(cs["records"], bc, lambda rec_no, c: "%.6f" % float(ref[rec_no][col_ids[c]]))
    dense = rc.dense_counts(cs["records"], col_ids)
    reads = [ln.split() for ln in want["reads.mtx.gz"].split("\n")[2:-1]]
    assert all(int(t) == dense[int(a) - 1][:, int(b) - 1].sum() for a, b, t in reads) and len(reads) > 300
    got = _read_dir(tmp_path, cs["res"])
    for fn in FILES:
        assert got[fn] == want[fn], (name, fn)
    _check_mmread(tmp_path, cs["res"], want)
    assert sorted(os.listdir(_len_dir(tmp_path, cs["res"]))) == sorted(FILES)
    assert not _parts_left(tmp_path)


LADDER_K = (1, 2, 7, 8, 9, 15, 16, 17, 127, 128, 129, 136, 137, 300)
TIES = ((0, 5, 576), "1.039062"), ((0, 15, 576), "1.117188")


@functools.lru_cache(maxsize=None)
def ladder(n_cols):
    """hand-made records on n_cols barcodes (scrambled ids): (records, barcode_index.csv text, names of the records
    without values).  Records 0 .. 13 take K through LADDER_K with counts from 1 to the hundreds, reads of label K and
    K + 1 among them, alphas unsorted in every second one (values below 1, below 0 and above 10); then a record without
    reads, one whose reads all have label >= K, one where column 0 has only such reads beside columns with T > 0, a NaN
    alpha, alpha[-1] == alpha[0], the two exact decimal ties with counts (1, 1, 0) in one cell, and K == 1 again: 22
    records, so the row numbers cross 9 / 10"""
    rng = np.random.default_rng(100 + n_cols)
    ids = (np.arange(n_cols) * 7919 + 13) % 100003
    bc = "CB,index\n" + "".join(f"L{j:04d}-1,{i}\n" for j, i in enumerate(ids.tolist()))

    def reads(K, n_cells, heavy):
        """(labels, columns): n_cells columns with reads, `heavy` of them with hundreds per label"""
        cols = rng.choice(n_cols, size=min(n_cells, n_cols), replace=False)
        lab, col = [], []
        for j, c in enumerate(cols.tolist()):
            n = int(rng.integers(150, 900)) if j < heavy else int(rng.integers(1, 6))
            lab.append(rng.integers(0, K + 2, n) if j % 3 else rng.integers(0, K, n))
            col.append(np.full(n, c))
        return np.concatenate(lab).astype(np.int64), np.concatenate(col)

    def record(r, K, alpha, lab, col):
        return dict(gene_info_str=f"{1 + r % 4}:LG{r}:{1 + r % 3}:{1000 * r + 1}-{1000 * r + 9000}:{'+-'[r % 2]}", K=K,
                    alpha_arr=np.asarray(alpha), beta_arr=np.full(len(alpha), 10.0), label_arr=lab,
                    cb_id_arr=ids[col].astype(np.int64))
    recs = []
    for r, K in enumerate(LADDER_K):
        alpha = rng.choice(np.arange(5, 6000), K, replace=False)
        if r % 2 == 0:
            alpha = np.sort(alpha)
        recs.append(record(r, K, alpha, *reads(K, 1100 if K < 100 else 48, 3)))
    none = np.zeros(0, np.int64)
    recs.append(record(14, 5, [10, 20, 30, 40, 50], none, none))
    recs.append(record(15, 3, [10, 20, 30], rng.integers(3, 6, 40).astype(np.int64), rng.integers(0, n_cols, 40)))
    lab, col = reads(4, 300, 2)
    keep = col != 0
    recs.append(record(16, 4, [100, 10, 900, 110], np.concatenate([lab[keep], [4, 5, 4]]),      # n_arr 1, -80, 721, 10
                       np.concatenate([col[keep], [0, 0, 0]])))
    recs.append(record(17, 3, [10.0, float("nan"), 300.0], *reads(3, 50, 1)))
    recs.append(record(18, 3, [250, 20, 250], *reads(3, 50, 1)))
    for r, (alpha, _txt) in enumerate(TIES, start=19):
        recs.append(record(r, 3, alpha, np.array([0, 1, 3], np.int64), np.full(3, n_cols - 1)))
    recs.append(record(21, 1, [77], *reads(1, 1100, 2)))
    return recs, bc, ("LG17", "LG18")


@pytest.mark.gpu
@pytest.mark.parametrize("n_cols", [1, 255, 256, 257, 1030])
def test_boundary_ladder(n_cols, tmp_path):
    from scape.apa_core import Parameters
    recs, bc, skipped = ladder(n_cols)
    rc.write_dir(str(tmp_path), "res.gene.pkl", recs, bc, {}, Parameters)
    r = _run(_args(tmp_path))
    assert r.exit_code == 0, (r.output, repr(r.exception))
    want = expected_texts(recs, bc)
    got = _read_dir(tmp_path)
    for fn in FILES:
        assert got[fn] == want[fn], (n_cols, fn)
    for name in skipped:                                            # named on stderr, their rows kept and empty
        assert any(ln.endswith(": no entry") and f":{name}:" in ln for ln in r.output.splitlines()), r.output
    entries = [ln.split() for ln in got["matrix.mtx.gz"].split("\n")[2:-1]]
    rows = {int(e[0]) for e in entries}
    assert got["matrix.mtx.gz"].split("\n")[1].split()[0] == str(len(recs)) == "22"
    assert not rows & {15, 16, 18, 19} and {1, 9, 10, 14, 20, 21, 22} <= rows
    assert f"20 {n_cols} 1.039062\n" in got["matrix.mtx.gz"] and f"21 {n_cols} 1.117188\n" in got["matrix.mtx.gz"]
    assert f"20 {n_cols} 2\n" in got["reads.mtx.gz"]
    assert max(int(ln.split()[2]) for ln in got["reads.mtx.gz"].split("\n")[2:-1]) >= 150
    if n_cols > 1:                                                  # with one barcode, record 16 has no cell with T > 0
        vals = [float(e[2]) for e in entries]
        assert min(vals) < 0 and max(vals) > 10 and any(e[2].startswith("-") for e in entries)
        assert not any(e[0] == "17" and e[1] == "1" for e in entries) and any(e[0] == "17" for e in entries)
    if n_cols >= 1000:
        assert {len(e[1]) for e in entries} == {1, 2, 3, 4}


@pytest.mark.gpu
def test_batch_and_block_invariance(tmp_path, monkeypatch):
    """the ladder with the default sizes (one batch, one block per matrix), with one batch cut into the smallest
    blocks (the records without an entry form a block of no bytes), and with tiny batches and gzip members as well: the
    decompressed files are identical, and the small runs did split the work"""
    from scape.apa_core import Parameters
    from scape_amd import _lib, report
    recs, bc, _skipped = ladder(257)
    rc.write_dir(str(tmp_path), "res.utr.pkl", recs, bc, {}, Parameters)
    lib = _lib.load_library()
    real_render, real_counts, calls, batches = lib.scape_hip_report_render_len_mtx, lib.scape_hip_report_counts, [], []

    def render(*a):
        calls.append((a[2], a[9]))
        return real_render(*a)

    def counts(*a):
        batches.append(a[1])
        return real_counts(*a)
    monkeypatch.setattr(lib, "scape_hip_report_render_len_mtx", render)
    monkeypatch.setattr(lib, "scape_hip_report_counts", counts)

    def run_once():
        del calls[:], batches[:]
        r = _run(_args(tmp_path, "res.utr.pkl"))
        assert r.exit_code == 0, repr(r.exception)
        per_what = [[n_rec for n_rec, w in calls if w == what] for what in (0, 1)]
        assert per_what[0] == per_what[1] and sum(per_what[0]) == sum(batches) == len(recs)
        return _read_dir(tmp_path, "res.utr.pkl"), per_what[0]
    big, blocks = run_once()
    assert big == expected_texts(recs, bc) and blocks == batches == [len(recs)]
    monkeypatch.setattr(report, "MAX_BLOCK_BYTES", 1)
    got, blocks = run_once()
    assert got == big and batches == [len(recs)]
    assert len(blocks) >= len(recs) - 2 and blocks[14] == 2         # records 14 and 15, neither with an entry
    _shrink(monkeypatch, block=1)
    got, blocks = run_once()
    assert got == big and len(batches) > 10 and len(blocks) >= len(batches) and max(blocks) <= 2


@pytest.mark.gpu
def test_failed_run_leaves_nothing(tmp_path):
    """an unknown barcode id below K: KeyError, no .part file and no new directory; with a complete earlier output in
    place, that output stays as it was"""
    from scape.apa_core import Parameters
    rec = dict(gene_info_str="1:G:1:100-900:+", K=2, alpha_arr=np.array([10, 500]), beta_arr=np.array([5.0, 7.5]),
               label_arr=np.array([0, 1, 1, 1]), cb_id_arr=np.array([3, 4, 99, 4]))
    bc = "CB,index\nA-1,3\nB-1,4\n"
    rc.write_dir(str(tmp_path), "res.gene.pkl", [rec], bc, {}, Parameters)
    r = _run(_args(tmp_path))
    assert isinstance(r.exception, KeyError) and "99" in str(r.exception)
    assert not _parts_left(tmp_path) and not os.path.exists(_len_dir(tmp_path))

    good = dict(rec, label_arr=np.array([0, 1, 2, 1]))              # id 99 has label K: it is not looked up
    rc.write_dir(str(tmp_path), "res.gene.pkl", [good], bc, {}, Parameters)
    r = _run(_args(tmp_path))
    assert r.exit_code == 0, repr(r.exception)
    want = {"matrix.mtx.gz": REAL_BANNER + "1 2 2\n1 1 1.000000\n1 2 10.000000\n",
            "reads.mtx.gz": INT_BANNER + "1 2 2\n1 1 1\n1 2 2\n",
            "features.tsv.gz": "G:1\tG:1\tGene Expression\n", "barcodes.tsv.gz": "A-1\nB-1\n"}
    assert _read_dir(tmp_path) == want
    rc.write_dir(str(tmp_path), "res.gene.pkl", [rec], bc, {}, Parameters)
    r = _run(_args(tmp_path))
    assert isinstance(r.exception, KeyError) and "99" in str(r.exception)
    assert not _parts_left(tmp_path) and sorted(os.listdir(_len_dir(tmp_path))) == sorted(FILES)
    assert _read_dir(tmp_path) == want

    neg = dict(rec, label_arr=np.array([0, -1, 2, 1]))
    rc.write_dir(str(tmp_path / "neg"), "res.gene.pkl", [neg], bc, {}, Parameters)
    r = _run(_args(tmp_path / "neg"))
    assert isinstance(r.exception, ValueError) and "negative label" in str(r.exception)
    assert not _parts_left(tmp_path) and not os.path.exists(_len_dir(tmp_path / "neg"))


@pytest.mark.gpu
def test_entry_point_refusals():
    """before scape_hip_report_counts, a slot outside 0 / 1 and a `what` outside 0 / 1 are error returns; the same
    call with valid arguments then renders"""
    import ctypes
    from scape_amd import _lib
    from scape_amd._lib import P_i8, P_i32, P_i64, ptr
    ctx = _lib.default_context(None)
    lib = ctx.lib
    lib.scape_hip_report_free(ctx.h)
    row0, K, n_off, skip = np.zeros(1, np.int64), np.array([3], np.int32), np.zeros(1, np.int64), np.zeros(1, np.int8)
    n_arr = np.array([1.0, 5.5, 10.0])
    nbytes, nnz = ctypes.c_int64(-1), ctypes.c_int64(-1)

    def call(slot, what):
        return lib.scape_hip_report_render_len_mtx(ctx.h, slot, 1, ptr(row0, P_i64), ptr(K, P_i32), ptr(n_off, P_i64),
                                                   ptr(n_arr), ptr(skip, P_i8), 1, what, ctypes.byref(nbytes),
                                                   ctypes.byref(nnz))
    try:
        assert call(0, 0) != 0 and "scape_hip_report_counts has not been called" in _lib.last_error()
        lab, cb = np.array([0, 1, 1, 2, 3], np.int64), np.array([0, 0, 1, 1, 2], np.int64)
        rc.device_counts(ctx, K, np.array([0, 5], np.int64), lab, cb, 3)
        for slot, what in ((-1, 0), (2, 0), (0, -1), (0, 2), (1, 7)):
            assert call(slot, what) != 0, (slot, what)
            assert (nbytes.value, nnz.value) == (-1, -1)
        K[0] = 4                                                    # more rows than the counts hold
        assert call(0, 0) != 0
        K[0] = 3
        for what, text in ((0, "1 1 3.250000\n1 2 7.750000\n"), (1, "1 1 2\n1 2 2\n")):
            assert call(what, what) == 0, _lib.last_error()
            assert (nbytes.value, nnz.value) == (len(text), 2)
            hp, nb = ctypes.c_void_p(), ctypes.c_int64(0)
            assert lib.scape_hip_report_fetch(ctx.h, what, ctypes.byref(hp), ctypes.byref(nb)) == 0
            assert ctypes.string_at(hp.value, nb.value).decode() == text
    finally:
        lib.scape_hip_report_free(ctx.h)
