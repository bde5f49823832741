"""`scape ex_pa_usage_mat`: the per-cell usage (PSI) of every pA site as a 10x-style directory <res>.usage/
(matrix.mtx.gz, reads.mtx.gz, features.tsv.gz, barcodes.tsv.gz) on the rows and columns of `ex_pa_cnt_mat --format mtx`.

The yardstick is a plain restatement in Python ints: the rows are the labels < K with reads of rc.dense_counts, record by
record; T is a column's sum over the record's K rows; a value is fixed6(int(c) / int(T)) (Python's true division of
ints is the correctly rounded quotient, test_report_lenmat.fixed6 is '%.6f' in exact integers).  Without a GPU it is
pinned to the REFERENCE's own dense count matrices (tests/golden/fixture_report.npz, 46 cases): same rows, same
places, c / T from the reference's counts.  The GPU tests compare the decompressed files for equality."""
import functools
import gzip
import inspect
import io
import os
import struct

import numpy as np
import pandas as pd
import pytest

import report_cases as rc
import test_report_lenmat as tl
from report_cases import no_gpu, parts_left as _parts_left, run as _run  # noqa: F401  (no_gpu is a fixture)
from test_report_lenmat import fixed6

REAL_BANNER = "%%MatrixMarket matrix coordinate real general\n"
INT_BANNER = "%%MatrixMarket matrix coordinate integer general\n"
FILES = ("matrix.mtx.gz", "reads.mtx.gz", "features.tsv.gz", "barcodes.tsv.gz")


# ---------------------------------------------------------------- the definition, restated
def usage_entries(records, col_ids, min_reads=1):
    """(pa_info of every kept row, {(record, label): file row}, value entries [(file row, column, c, T)], reads entries
    [(file row, column, T)]), rows and columns 0-based and ascending.  A kept row is a label < K with reads, whatever
    min_reads is; a value entry needs c > 0 and T >= min_reads, a reads entry T >= min_reads"""
    feats, row_of, vals, reads = [], {}, [], []
    for r, (rec, m) in enumerate(zip(records, rc.dense_counts(records, col_ids))):
        T = m.sum(axis=0)
        cols = [int(c) for c in np.nonzero(T >= max(min_reads, 1))[0]]
        for lb in range(len(m)):
            if not m[lb].any():
                continue
            row = row_of[(r, lb)] = len(feats)
            feats.append(rc.pa_info(rec, lb))
            for c in cols:
                reads.append((row, c, int(T[c])))
                if m[lb, c] > 0:
                    vals.append((row, c, int(m[lb, c]), int(T[c])))
    return feats, row_of, vals, reads


def expected_texts(records, bc_csv, min_reads=1):
    """the four files of the restatement, and its {(record, label): file row}"""
    cbs = pd.read_csv(io.StringIO(bc_csv), index_col="index")["CB"].tolist()
    feats, row_of, vals, reads = usage_entries(records, rc.column_ids(bc_csv), min_reads)
    head = f"{len(feats)} {len(cbs)} "
    vtxt = "".join(f"{a + 1} {b + 1} {fixed6(c / T)}\n" for a, b, c, T in vals)
    rtxt = "".join(f"{a + 1} {b + 1} {T}\n" for a, b, T in reads)
    return {"matrix.mtx.gz": f"{REAL_BANNER}{head}{len(vals)}\n{vtxt}",
            "reads.mtx.gz": f"{INT_BANNER}{head}{len(reads)}\n{rtxt}",
            "features.tsv.gz": "".join(f"{p}\t{p}\tGene Expression\n" for p in feats),
            "barcodes.tsv.gz": "".join(f"{b}\n" for b in cbs)}, row_of


def test_restatement_vs_reference_count_matrices():
    """on every golden case: the restatement's rows are the reference's matrix rows (test_report_mtx's expected
    features text), at min_reads 1 its value entries sit where the reference's matrix body has its nonzeros, in that
    order, and every value is c / T with c read from that body; '%.6f' agrees with fixed6 and numpy's f64 quotient has
    the same bits.  The cases hold 0 to 4,288 entries with 0 < c < T each, T up to 37"""
    import test_report_mtx as tm
    n_frac, n_cases, t_max = 0, 0, 0
    for cs in rc.fixture_cases():
        bc = rc.text(rc.fixture(), cs["barcode"])
        ref_texts, dense = tm._expected_from_dense(cs["mat_body"], bc)
        want, _row_of = expected_texts(cs["records"], bc)
        assert want["features.tsv.gz"] == ref_texts["features.tsv.gz"], cs["name"]
        assert want["barcodes.tsv.gz"] == ref_texts["barcodes.tsv.gz"], cs["name"]
        _feats, _rows, vals, reads = usage_entries(cs["records"], rc.column_ids(bc))
        i, j = np.nonzero(dense)
        assert [(a, b) for a, b, _c, _T in vals] == list(zip(i.tolist(), j.tolist())), cs["name"]
        assert {(a, b) for a, b, _c, _T in vals} <= {(a, b) for a, b, _T in reads}
        lines = want["matrix.mtx.gz"].split("\n")[2:-1]
        assert len(lines) == len(vals)
        for (a, b, c, T), ln in zip(vals, lines):
            v = c / T
            assert c == dense[a, b] and 0 < c <= T and v == int(dense[a, b]) / T
            assert "%.6f" % v == fixed6(v) == ln.split()[2]
            assert struct.pack("<d", float(np.float64(c) / np.float64(T))) == struct.pack("<d", v)
            n_frac += c < T
            t_max = max(t_max, T)
        n_cases += 1
    assert n_cases == 46 and n_frac > 30000 and t_max >= 30


# ---------------------------------------------------------------- CPU: the command's surface
def _args(root, res="res.gene.pkl", min_reads=None):
    return ["ex_pa_usage_mat", "--output_dir", str(root), "--res_pkl_file", res] + \
        ([] if min_reads is None else ["--min_reads", str(min_reads)])


def _usage_dir(root, res="res.gene.pkl", min_reads=1):
    return os.path.join(str(root), res.replace(".pkl", ".usage" if min_reads == 1 else f".min{min_reads}.usage"))


def _read_files(path, names=FILES):
    out = {}
    for name in names:
        with gzip.open(os.path.join(path, name), "rt", newline="") as fh:
            out[name] = fh.read()
    return out


def test_help_lists_the_command():
    r = _run(["--help"])
    assert r.exit_code == 0 and "ex_pa_usage_mat" in r.output
    r = _run(["ex_pa_usage_mat", "--help"])
    assert r.exit_code == 0, r.output
    assert "--output_dir" in r.output and "--res_pkl_file" in r.output and "--min_reads" in r.output


def test_utils_reexports_the_command():
    import scape.utils as su
    from scape_amd import report
    assert su.ex_pa_usage_mat is report.ex_pa_usage_mat
    params = inspect.signature(report._ex_pa_usage_mat).parameters
    assert list(params) == ["output_dir", "res_pkl_file", "min_reads", "device"]
    assert params["min_reads"].default == 1 and params["device"].default is None


def test_prerequisites(tmp_path, no_gpu):
    """ex_pa_cnt_mat's checks, messages and order, all before the GPU; a --min_reads outside 1 .. 2^31 - 1 is refused
    by click; the directory is untouched afterwards"""
    r = _run(_args(tmp_path / "nope"))
    assert r.exit_code != 0 and "Given output_dir folder does not exists." in str(r.exception)
    r = _run(_args(tmp_path))
    assert "Given res_pkl_file is not in output_dir." in str(r.exception)
    r = _run(["ex_pa_usage_mat", "--output_dir", str(tmp_path)])                   # default "None"
    assert "Invalid file" in str(r.exception) and "None" in str(r.exception)
    (tmp_path / "res.gene.pkl").write_bytes(b"")
    r = _run(_args(tmp_path))
    assert isinstance(r.exception, FileNotFoundError) and "barcode_index.csv" in str(r.exception)
    (tmp_path / "barcode_index.csv").write_text("CB,index\n")
    r = _run(_args(tmp_path))
    assert isinstance(r.exception, ValueError) and "lists no barcode" in str(r.exception)
    (tmp_path / "barcode_index.csv").write_text('CB,index\nA-1,0\n"B\tX-1",1\n')
    r = _run(_args(tmp_path, min_reads=3))
    assert isinstance(r.exception, ValueError) and "B\\tX-1" in str(r.exception)
    (tmp_path / "barcode_index.csv").write_text("CB,index\nA-1,0\n")
    for bad in ("0", "-1", "x", str(2 ** 31)):
        r = _run(_args(tmp_path, min_reads=bad))
        assert r.exit_code == 2 and "--min_reads" in r.output, (bad, r.output)
    assert sorted(os.listdir(tmp_path)) == ["barcode_index.csv", "res.gene.pkl"] and not _parts_left(tmp_path)


def test_entry_refuses_min_reads_before_any_file(tmp_path, no_gpu):
    from scape_amd import report
    for bad in (0, -1, 2 ** 31, 1.5, "2", True):
        with pytest.raises(ValueError, match="min_reads"):
            report._ex_pa_usage_mat(str(tmp_path / "nope"), "res.gene.pkl", min_reads=bad)


# ---------------------------------------------------------------- GPU
def _mm(path, name):
    import scipy.io
    import scipy.sparse
    return scipy.sparse.coo_matrix(scipy.io.mmread(os.path.join(path, name)))


@pytest.mark.gpu
@pytest.mark.parametrize("c", rc.case_params())
def test_golden_cases(c, tmp_path, monkeypatch):
    """ex_pa_cnt_mat --format mtx and ex_pa_usage_mat in one directory: the same features and barcodes, all four files
    the restatement's, and the loaded matrices agree with the loaded count matrix"""
    import test_report_mtx as tm
    cs = rc.fixture_case(c)
    if cs["name"] == "fuzz23":
        tl._shrink(monkeypatch)
    bc, _paths = rc.write_case(cs, tmp_path, {})
    r = _run(tm._mtx_args(tmp_path, cs["res"]))
    assert r.exit_code == 0, (cs["name"], r.output, repr(r.exception))
    r = _run(_args(tmp_path, cs["res"]))
    assert r.exit_code == 0, (cs["name"], r.output, repr(r.exception))
    lines = r.output.splitlines()
    assert lines[0] == "Finish pA site usage for each cell" and lines[1].startswith("Finish ") and len(lines) == 2
    udir, cdir = _usage_dir(tmp_path, cs["res"]), tm._mtx_dir(tmp_path, cs["res"])
    got, cnt = _read_files(udir), _read_files(cdir, tm.FILES)
    assert got["features.tsv.gz"] == cnt["features.tsv.gz"] and got["barcodes.tsv.gz"] == cnt["barcodes.tsv.gz"]
    want, _row_of = expected_texts(cs["records"], bc)
    for name in FILES:
        assert got[name] == want[name], (cs["name"], name)
    assert sorted(os.listdir(udir)) == sorted(FILES) and not _parts_left(tmp_path)
    vm, rm, cm = _mm(udir, "matrix.mtx.gz"), _mm(udir, "reads.mtx.gz"), _mm(cdir, "matrix.mtx.gz")
    assert vm.shape == rm.shape == cm.shape
    assert np.array_equal(vm.row, cm.row) and np.array_equal(vm.col, cm.col)
    n_cols = vm.shape[1]
    assert np.isin(vm.row.astype(np.int64) * n_cols + vm.col, rm.row.astype(np.int64) * n_cols + rm.col).all()
    if vm.nnz:
        T = rm.toarray()[vm.row, vm.col]
        assert (T >= cm.data).all() and (cm.data >= 1).all()
        assert (np.abs(cm.data / T - vm.data) <= 0.5e-6 + 1e-12).all()


LADDER_K = (1, 2, 9, 10, 129, 300)


@functools.lru_cache(maxsize=None)
def ladder(n_cols):
    """hand-made records on n_cols barcodes (scrambled ids), built as test_report_lenmat.ladder builds its own: (records,
    barcode_index.csv text, {name: record number}).  Records 0 .. 5 take K through LADDER_K: about 1,100 cells with
    reads for K < 100 and 48 above, three of them with hundreds of reads per label and the rest with 1 to 5, reads of
    label K and K + 1 among them; with K >= 9 the first, one middle and the last label have no read at all, so file
    rows differ from count rows and a record's rows are not contiguous in the file.  Then "none" without reads, "above"
    whose reads all have label >= K, "col0" where column 0 has only such reads beside columns with T > 0, "ties" with
    the exact decimal ties (1, 127) in the last column and (3, 125) in the first (two records, "ties" and "ties2", when
    there is one column), "small" with cells of T = 1, 2, 4, 5, 6 in a K = 3 record and "two" with two reads in all"""
    rng = np.random.default_rng(200 + n_cols)
    ids = (np.arange(n_cols) * 7919 + 13) % 100003
    bc = "CB,index\n" + "".join(f"U{j:04d}-1,{i}\n" for j, i in enumerate(ids.tolist()))

    def reads(K, n_cells, heavy):
        """(labels, columns): n_cells columns with reads, `heavy` of them with hundreds per label"""
        empty = {0, K // 2, K - 1} if K >= 9 else set()
        site = np.array([lb for lb in range(K) if lb not in empty], dtype=np.int64)
        cols = rng.choice(n_cols, size=min(n_cells, n_cols), replace=False)
        lab, col = [], []
        for j, c in enumerate(cols.tolist()):
            n = len(site) * int(rng.integers(100, 400)) if j < heavy else int(rng.integers(1, 6))
            pool = np.concatenate([site, [K, K + 1]]) if j % 3 else site
            lab.append(pool[rng.integers(0, len(pool), n)])
            col.append(np.full(n, c))
        return np.concatenate(lab).astype(np.int64), np.concatenate(col)

    names, recs = {}, []

    def record(name, K, lab, col):
        r = names[name] = len(recs)
        recs.append(dict(gene_info_str=f"{1 + r % 4}:UG{r}:{1 + r % 3}:{1000 * r + 1}-{1000 * r + 9000}:{'+-'[r % 2]}",
                         K=K, alpha_arr=rng.choice(np.arange(5, 6000), K, replace=False).astype(np.int64),
                         beta_arr=rng.choice([5.0, 7.5, 10.0, 32.5], K), label_arr=np.asarray(lab, dtype=np.int64),
                         cb_id_arr=ids[np.asarray(col, dtype=np.int64)].astype(np.int64)))
    for K in LADDER_K:
        record(f"K{K}", K, *reads(K, 1100 if K < 100 else 48, 3))
    none = np.zeros(0, np.int64)
    record("none", 5, none, none)
    record("above", 3, rng.integers(3, 6, 40), rng.integers(0, n_cols, 40))
    lab, col = reads(4, 300, 2)
    keep = col != 0
    record("col0", 4, np.concatenate([lab[keep], [4, 5, 4]]), np.concatenate([col[keep], [0, 0, 0]]))
    last, first = [0] + [1] * 127, [0] * 3 + [1] * 125
    if n_cols == 1:
        record("ties", 2, last, [0] * 128)
        record("ties2", 2, first, [0] * 128)
    else:
        record("ties", 2, last + first, [n_cols - 1] * 128 + [0] * 128)
    cells = [(1, 0, 0), (1, 1, 0), (1, 0, 3), (2, 2, 1), (1, 2, 3)]                 # T = 1, 2, 4, 5, 6
    lab = [lb for cnt in cells for lb in range(3) for _ in range(cnt[lb])]
    col = [min(j + 1, n_cols - 1) for j, cnt in enumerate(cells) for _ in range(sum(cnt))]
    record("small", 3, lab, col)
    record("two", 2, [0, 1], [n_cols - 1] * 2)
    return recs, bc, names


def _ladder_runs(tmp_path, n_cols, Ns=(1, 2, 5)):
    from scape.apa_core import Parameters
    recs, bc, names = ladder(n_cols)
    rc.write_dir(str(tmp_path), "res.gene.pkl", recs, bc, {}, Parameters)
    got = {}
    for N in Ns:
        r = _run(_args(tmp_path, min_reads=None if N == 1 else N))
        assert r.exit_code == 0, (N, r.output, repr(r.exception))
        got[N] = _read_files(_usage_dir(tmp_path, min_reads=N))
    return recs, bc, names, got


@pytest.mark.gpu
@pytest.mark.parametrize("n_cols", [1, 255, 256, 257, 1030])
def test_boundary_ladder(n_cols, tmp_path):
    recs, bc, names, got = _ladder_runs(tmp_path, n_cols)
    assert sorted(d for d in os.listdir(tmp_path) if d.endswith(".usage")) == \
        ["res.gene.min2.usage", "res.gene.min5.usage", "res.gene.usage"]
    assert not _parts_left(tmp_path)
    for N in (1, 2, 5):
        want, row_of = expected_texts(recs, bc, N)
        for fn in FILES:
            assert got[N][fn] == want[fn], (n_cols, N, fn)
    assert got[1]["features.tsv.gz"] == got[2]["features.tsv.gz"] == got[5]["features.tsv.gz"]
    n_rows = got[1]["features.tsv.gz"].count("\n")
    assert n_rows > 100 and all(got[N][fn].split("\n")[1].split()[0] == str(n_rows)
                                for N in (1, 2, 5) for fn in ("matrix.mtx.gz", "reads.mtx.gz"))
    # the exact decimal ties round to even
    a, b = row_of[(names["ties"], 0)] + 1, row_of[(names["ties"], 1)] + 1
    for N in (1, 2, 5):
        text = got[N]["matrix.mtx.gz"]
        assert f"{a} {n_cols} 0.007812\n" in text and f"{b} {n_cols} 0.992188\n" in text
        first = names.get("ties2", names["ties"])
        a1, b1 = row_of[(first, 0)] + 1, row_of[(first, 1)] + 1
        assert f"{a1} 1 0.023438\n" in text and f"{b1} 1 0.976562\n" in text
        assert f"{a} {n_cols} 128\n" in got[N]["reads.mtx.gz"]
    # file rows are not count rows, and a record's rows are not contiguous there
    assert (names["K9"], 0) not in row_of and (names["K9"], 4) not in row_of and (names["K9"], 8) not in row_of
    assert (names["K300"], 150) not in row_of and row_of[(names["K300"], 151)] == row_of[(names["K300"], 149)] + 1
    assert not any(r in (names["none"], names["above"]) for r, _lb in row_of)
    # with N = 5 the rows of "two" keep their features lines and have no entry in either matrix
    two = {row_of[(names["two"], lb)] + 1 for lb in (0, 1)}
    for fn in ("matrix.mtx.gz", "reads.mtx.gz"):
        rows = [{int(ln.split()[0]) for ln in got[N][fn].split("\n")[2:-1]} for N in (1, 2, 5)]
        assert two <= rows[0] and two <= rows[1] and not two & rows[2], fn
    assert len(got[2]["matrix.mtx.gz"]) > len(got[5]["matrix.mtx.gz"])
    if n_cols > 1:                                                  # one barcode: a record has one cell, T = 1 only by chance
        assert len(got[1]["matrix.mtx.gz"]) > len(got[2]["matrix.mtx.gz"])
        col0 = {row_of[(names["col0"], lb)] + 1 for lb in range(4) if (names["col0"], lb) in row_of}
        ent = [ln.split() for ln in got[1]["reads.mtx.gz"].split("\n")[2:-1]]
        assert col0 and any(int(e[0]) in col0 for e in ent) and not any(int(e[0]) in col0 and e[1] == "1" for e in ent)
        small = row_of[(names["small"], 0)] + 1
        assert [e[2] for e in ent if int(e[0]) == small] == ["1", "2", "4", "5", "6"]
    if n_cols >= 1000:
        for fn in ("matrix.mtx.gz", "reads.mtx.gz"):
            assert {len(ln.split()[1]) for ln in got[1][fn].split("\n")[2:-1]} == {1, 2, 3, 4}, fn
        assert {len(ln.split()[2]) for ln in got[1]["reads.mtx.gz"].split("\n")[2:-1]} >= {1, 2, 3, 4}


@pytest.mark.gpu
def test_batch_and_block_invariance(tmp_path, monkeypatch):
    """the ladder at 257 columns with the default sizes (one batch, one block per matrix), with one batch cut into
    one-row blocks, and with tiny batches and gzip members as well: the decompressed files are identical, the small
    runs did split the work, and the totals were formed once per batch, not once per block"""
    from scape.apa_core import Parameters
    from scape_amd import _lib, report
    recs, bc, _names = ladder(257)
    rc.write_dir(str(tmp_path), "res.utr.pkl", recs, bc, {}, Parameters)
    lib = _lib.load_library()
    real = {n: getattr(lib, n) for n in ("scape_hip_report_render_usage_mtx", "scape_hip_report_usage_totals",
                                         "scape_hip_report_counts")}
    calls, totals, batches = [], [], []

    def render(*a):
        calls.append((a[2], a[7]))
        return real["scape_hip_report_render_usage_mtx"](*a)

    def tot(*a):
        totals.append(a[1])
        return real["scape_hip_report_usage_totals"](*a)

    def counts(*a):
        batches.append(a[1])
        return real["scape_hip_report_counts"](*a)
    monkeypatch.setattr(lib, "scape_hip_report_render_usage_mtx", render)
    monkeypatch.setattr(lib, "scape_hip_report_usage_totals", tot)
    monkeypatch.setattr(lib, "scape_hip_report_counts", counts)
    want, _row_of = expected_texts(recs, bc, 2)
    n_rows = want["features.tsv.gz"].count("\n")

    def run_once():
        del calls[:], totals[:], batches[:]
        r = _run(_args(tmp_path, "res.utr.pkl", 2))
        assert r.exit_code == 0, repr(r.exception)
        per_what = [[n for n, w in calls if w == what] for what in (0, 1)]
        assert sum(per_what[0]) == sum(per_what[1]) == n_rows and sum(batches) == len(recs)   # each matrix cuts its own blocks
        assert len(totals) <= len(batches) and set(totals) <= set(batches)
        return _read_files(_usage_dir(tmp_path, "res.utr.pkl", 2)), per_what
    big, blocks = run_once()
    assert big == want and blocks == [[n_rows], [n_rows]] and batches == totals == [len(recs)]
    monkeypatch.setattr(report, "MAX_BLOCK_BYTES", 1)
    got, blocks = run_once()
    assert got == big and batches == totals == [len(recs)] and blocks == [[1] * n_rows] * 2
    tl._shrink(monkeypatch, block=1)
    got, blocks = run_once()
    assert got == big and len(batches) > len(LADDER_K) and len(totals) >= len(LADDER_K)
    assert blocks == [[1] * n_rows] * 2 and n_rows > 10 * len(totals)


@pytest.mark.gpu
def test_failed_run_leaves_nothing(tmp_path):
    """an unknown barcode id below K: KeyError, no .part file and no new directory; with a complete earlier output in
    place, that output stays as it was; a negative label: ValueError, nothing left"""
    from scape.apa_core import Parameters
    rec = dict(gene_info_str="1:G:1:100-900:+", K=2, alpha_arr=np.array([10, 500]), beta_arr=np.array([5.0, 7.5]),
               label_arr=np.array([0, 1, 1, 1]), cb_id_arr=np.array([3, 4, 99, 4]))
    bc = "CB,index\nA-1,3\nB-1,4\n"
    rc.write_dir(str(tmp_path), "res.gene.pkl", [rec], bc, {}, Parameters)
    r = _run(_args(tmp_path))
    assert isinstance(r.exception, KeyError) and "99" in str(r.exception)
    assert not _parts_left(tmp_path) and not os.path.exists(_usage_dir(tmp_path))

    good = dict(rec, label_arr=np.array([0, 1, 2, 1]))              # id 99 has label K: it is not looked up
    rc.write_dir(str(tmp_path), "res.gene.pkl", [good], bc, {}, Parameters)
    r = _run(_args(tmp_path))
    assert r.exit_code == 0, repr(r.exception)
    want = {"matrix.mtx.gz": REAL_BANNER + "2 2 2\n1 1 1.000000\n2 2 1.000000\n",
            "reads.mtx.gz": INT_BANNER + "2 2 4\n1 1 1\n1 2 2\n2 1 1\n2 2 2\n",
            "features.tsv.gz": "1:110:5.0:+:1:G:1\t1:110:5.0:+:1:G:1\tGene Expression\n"
                               "1:600:7.5:+:2:G:1\t1:600:7.5:+:2:G:1\tGene Expression\n",
            "barcodes.tsv.gz": "A-1\nB-1\n"}
    assert _read_files(_usage_dir(tmp_path)) == want
    rc.write_dir(str(tmp_path), "res.gene.pkl", [rec], bc, {}, Parameters)
    r = _run(_args(tmp_path))
    assert isinstance(r.exception, KeyError) and "99" in str(r.exception)
    assert not _parts_left(tmp_path) and sorted(os.listdir(_usage_dir(tmp_path))) == sorted(FILES)
    assert _read_files(_usage_dir(tmp_path)) == want

    neg = dict(rec, label_arr=np.array([0, -1, 2, 1]))
    rc.write_dir(str(tmp_path / "neg"), "res.gene.pkl", [neg], bc, {}, Parameters)
    r = _run(_args(tmp_path / "neg", min_reads=3))
    assert isinstance(r.exception, ValueError) and "negative label" in str(r.exception)
    assert not _parts_left(tmp_path) and not os.path.exists(_usage_dir(tmp_path / "neg", min_reads=3))


@pytest.mark.gpu
def test_entry_point_refusals():
    """before scape_hip_report_counts, before the totals of these counts, a slot or `what` outside 0 / 1, min_reads
    below 1 and a row or record beyond what the counts hold are error returns that leave the output arguments alone;
    the same call with valid arguments then renders a 3-read, 2-column case into both slots"""
    import ctypes
    from scape_amd import _lib
    from scape_amd._lib import P_i32, P_i64, ptr
    ctx = _lib.default_context(None)
    lib = ctx.lib
    lib.scape_hip_report_free(ctx.h)
    K, row0 = np.array([2], np.int32), np.zeros(1, np.int64)
    nbytes, nnz = ctypes.c_int64(-1), ctypes.c_int64(-1)

    def totals():
        return lib.scape_hip_report_usage_totals(ctx.h, 1, ptr(row0, P_i64), ptr(K, P_i32))

    def call(slot=0, what=0, min_reads=1, rows=(0, 1), row_rec=(0, 0)):
        rows, row_rec = np.array(rows, np.int64), np.array(row_rec, np.int32)
        return lib.scape_hip_report_render_usage_mtx(ctx.h, slot, len(rows), ptr(rows, P_i64), ptr(row_rec, P_i32), 1,
                                                     min_reads, what, ctypes.byref(nbytes), ctypes.byref(nnz))

    def counts():                                                   # counts (1, 0) and (1, 1): T = (2, 1)
        rc.device_counts(ctx, K, np.array([0, 3], np.int64), np.array([0, 1, 1], np.int64),
                         np.array([0, 0, 1], np.int64), 2)
    try:
        assert totals() != 0 and "scape_hip_report_counts has not been called" in _lib.last_error()
        assert call() != 0 and "scape_hip_report_counts has not been called" in _lib.last_error()
        counts()
        assert call() != 0 and "scape_hip_report_usage_totals has not been called" in _lib.last_error()
        K[0] = 3                                                    # more rows than the counts hold
        assert totals() != 0
        K[0] = 2
        assert totals() == 0, _lib.last_error()
        for kw in (dict(slot=-1), dict(slot=2), dict(what=-1), dict(what=2), dict(min_reads=0), dict(min_reads=-3),
                   dict(rows=(0, 2)), dict(rows=(-1, 1)), dict(row_rec=(0, 1)), dict(row_rec=(-1, 0))):
            assert call(**kw) != 0, kw
            assert (nbytes.value, nnz.value) == (-1, -1), kw
        texts = {(0, 1): "1 1 0.500000\n2 1 0.500000\n2 2 1.000000\n", (1, 1): "1 1 2\n1 2 1\n2 1 2\n2 2 1\n",
                 (0, 2): "1 1 0.500000\n2 1 0.500000\n", (1, 2): "1 1 2\n2 1 2\n"}
        for (what, N), text in texts.items():
            assert call(slot=what, what=what, min_reads=N) == 0, _lib.last_error()
            assert (nbytes.value, nnz.value) == (len(text), text.count("\n"))
            hp, nb = ctypes.c_void_p(), ctypes.c_int64(0)
            assert lib.scape_hip_report_fetch(ctx.h, what, ctypes.byref(hp), ctypes.byref(nb)) == 0
            assert ctypes.string_at(hp.value, nb.value).decode() == text
        nbytes.value = nnz.value = -1
        counts()                                                    # new counts: the totals of the old ones are gone
        assert call() != 0 and "scape_hip_report_usage_totals has not been called" in _lib.last_error()
        assert (nbytes.value, nnz.value) == (-1, -1)
    finally:
        lib.scape_hip_report_free(ctx.h)
