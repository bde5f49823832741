"""`scape ex_pa_cnt_mat --format mtx`: the count matrix as a 10x-style Matrix Market directory <res>.cnt/
(matrix.mtx.gz, features.tsv.gz, barcodes.tsv.gz).

The expected texts of the golden cases (tests/golden/fixture_report.npz) come from the REFERENCE's own dense matrix
body: its rows are the matrix rows, its first field is pa_info, its nonzero fields are the entries.  A wide synthetic
stream is checked against an np.add.at restatement of the counts.  Every file is compared byte for byte after
decompression, and the matrix is also read back with scipy.io.mmread."""
import gzip
import io
import os

import numpy as np
import pandas as pd
import pytest

import report_cases as rc
from report_cases import no_gpu, parts_left as _parts_left, run as _run  # noqa: F401  (no_gpu is a fixture)

BANNER = "%%MatrixMarket matrix coordinate integer general\n"
FILES = ("matrix.mtx.gz", "features.tsv.gz", "barcodes.tsv.gz")


def _mtx_args(root, res="res.gene.pkl"):
    return ["ex_pa_cnt_mat", "--output_dir", str(root), "--res_pkl_file", res, "--format", "mtx"]


def _mtx_dir(root, res="res.gene.pkl"):
    return os.path.join(str(root), res.replace(".pkl", ".cnt"))


def _read_dir(root, res="res.gene.pkl"):
    out = {}
    for name in FILES:
        with gzip.open(os.path.join(_mtx_dir(root, res), name), "rt", newline="") as fh:
            out[name] = fh.read()
    return out


def _texts(pa_info, dense, barcodes):
    """the three files of a matrix: rows named pa_info, dense [rows, barcodes] integer counts"""
    i, j = np.nonzero(dense)                      # row-major: rows ascending, columns ascending within a row
    ent = "".join(f"{a + 1} {b + 1} {dense[a, b]}\n" for a, b in zip(i.tolist(), j.tolist()))
    return {"matrix.mtx.gz": f"{BANNER}{dense.shape[0]} {dense.shape[1]} {len(i)}\n{ent}",
            "features.tsv.gz": "".join(f"{p}\t{p}\tGene Expression\n" for p in pa_info),
            "barcodes.tsv.gz": "".join(f"{b}\n" for b in barcodes)}


def _barcodes(bc_csv):
    return pd.read_csv(io.StringIO(bc_csv), index_col="index")["CB"].tolist()


def _expected_from_dense(mat_body, bc_csv):
    """the three texts and the integer matrix that a dense body (rows '"pa_info","0.0","2",...') stands for"""
    cbs = _barcodes(bc_csv)
    pa_info, dense = rc.dense_of_body(mat_body, len(cbs))
    return _texts(pa_info, dense, cbs), dense


def _check_mmread(root, res, dense):
    import scipy.io
    import scipy.sparse
    m = scipy.sparse.coo_matrix(scipy.io.mmread(os.path.join(_mtx_dir(root, res), "matrix.mtx.gz")))
    assert m.shape == dense.shape
    assert np.array_equal(m.toarray(), dense)


# ---------------------------------------------------------------- CPU
def test_format_option():
    r = _run(["ex_pa_cnt_mat", "--help"])
    assert r.exit_code == 0, r.output
    assert "--format" in r.output and "[tsv|mtx]" in r.output
    r = _run(["ex_pa_cnt_mat", "--output_dir", ".", "--res_pkl_file", "res.gene.pkl", "--format", "csv"])
    assert r.exit_code == 2 and "--format" in r.output


def test_entry_point_format_argument(tmp_path):
    import inspect
    import scape.utils as su
    from scape_amd import report
    assert inspect.signature(report._ex_pa_cnt_mat).parameters["fmt"].default == "tsv"
    assert su.ex_pa_cnt_mat is report.ex_pa_cnt_mat
    with pytest.raises(ValueError, match="csv"):
        report._ex_pa_cnt_mat(str(tmp_path), "res.gene.pkl", fmt="csv")


def test_mtx_prerequisites(tmp_path, no_gpu):
    """the dense path's checks, messages and order, then the barcodes' own check, all before the GPU"""
    mtx = ["--format", "mtx"]
    r = _run(["ex_pa_cnt_mat", "--output_dir", str(tmp_path / "nope"), "--res_pkl_file", "res.gene.pkl"] + mtx)
    assert r.exit_code != 0 and "Given output_dir folder does not exists." in str(r.exception)
    r = _run(_mtx_args(tmp_path))
    assert "Given res_pkl_file is not in output_dir." in str(r.exception)
    r = _run(["ex_pa_cnt_mat", "--output_dir", str(tmp_path)] + mtx)              # default "None"
    assert "Invalid file" in str(r.exception) and "None" in str(r.exception)
    (tmp_path / "res.gene.pkl").write_bytes(b"")
    r = _run(_mtx_args(tmp_path))
    assert isinstance(r.exception, FileNotFoundError) and "barcode_index.csv" in str(r.exception)
    (tmp_path / "barcode_index.csv").write_text("CB,index\n")
    r = _run(_mtx_args(tmp_path))
    assert isinstance(r.exception, ValueError) and "lists no barcode" in str(r.exception)
    (tmp_path / "barcode_index.csv").write_text('CB,index\nA-1,0\n"B\tX-1",1\n')
    r = _run(_mtx_args(tmp_path))
    assert isinstance(r.exception, ValueError) and "B\\tX-1" in str(r.exception)
    assert not os.path.exists(_mtx_dir(tmp_path)) and not _parts_left(tmp_path)


# ---------------------------------------------------------------- GPU
def _shrink(monkeypatch, block=1 << 12):
    """batches, render blocks and gzip members small enough that a case takes several of each"""
    from scape_amd import report
    monkeypatch.setattr(report, "MAX_BATCH_BYTES", 1 << 14)
    monkeypatch.setattr(report, "MAX_BLOCK_BYTES", block)
    monkeypatch.setattr(report, "GZIP_PART", 1 << 11)


@pytest.mark.gpu
@pytest.mark.parametrize("c", rc.case_params())
def test_mtx_case_vs_reference_dense(c, tmp_path, monkeypatch):
    cs = rc.fixture_case(c)
    if cs["name"].startswith("fuzz"):
        _shrink(monkeypatch)
    bc, _paths = rc.write_case(cs, tmp_path, {})
    r = _run(_mtx_args(tmp_path, cs["res"]))
    assert r.exit_code == 0, (cs["name"], r.output, repr(r.exception))
    lines = r.output.splitlines()
    assert lines[0] == "Finish counting for each gene" and lines[1].startswith("Finish ") and len(lines) == 2
    want, dense = _expected_from_dense(cs["mat_body"], bc)
    got = _read_dir(tmp_path, cs["res"])
    for name in FILES:
        assert got[name] == want[name], (cs["name"], name)
    _check_mmread(tmp_path, cs["res"], dense)
    assert sorted(os.listdir(_mtx_dir(tmp_path, cs["res"]))) == sorted(FILES)
    assert not os.path.exists(os.path.join(str(tmp_path), cs["res"].replace(".pkl", ".cnt.tsv.gz")))
    assert not _parts_left(tmp_path)


@pytest.mark.gpu
def test_mtx_batch_and_block_invariance(tmp_path, monkeypatch):
    """the largest golden case with the default sizes and with one-row blocks, tiny batches and gzip members: the
    decompressed files are identical (and the tiny run did split the work)"""
    from scape_amd import _lib
    cs = max(rc.fixture_cases(), key=lambda x: x["mat_body"].count("\n"))      # the most matrix rows
    rc.write_case(cs, tmp_path, {})
    assert _run(_mtx_args(tmp_path, cs["res"])).exit_code == 0
    big = _read_dir(tmp_path, cs["res"])
    lib = _lib.load_library()
    real, calls = lib.scape_hip_report_render_mtx, []

    def counted(*a):
        calls.append(a[2])
        return real(*a)
    monkeypatch.setattr(lib, "scape_hip_report_render_mtx", counted)
    _shrink(monkeypatch, block=1)
    r = _run(_mtx_args(tmp_path, cs["res"]))
    assert r.exit_code == 0, repr(r.exception)
    assert _read_dir(tmp_path, cs["res"]) == big
    n_rows = int(big["matrix.mtx.gz"].split("\n")[1].split()[0])
    assert len(calls) == n_rows > 2 and set(calls) == {1}


@pytest.mark.gpu
@pytest.mark.parametrize("small", [False, True], ids=["default_sizes", "small_sizes"])
def test_mtx_wide_stream(small, tmp_path, monkeypatch):
    from scape.apa_core import Parameters
    recs, bc, pa_info, dense = rc.wide_stream()
    assert any(p["K"] > 63 for p in recs) and dense.max() >= 100 and dense.shape[1] >= 3000
    assert (dense[:, -1] > 0).any() and not (dense[:, 40] > 0).any()
    if small:
        _shrink(monkeypatch, block=1 << 15)
    rc.write_dir(str(tmp_path), "res.gene.pkl", recs, bc, {}, Parameters)
    r = _run(_mtx_args(tmp_path))
    assert r.exit_code == 0, repr(r.exception)
    assert _read_dir(tmp_path) == _texts(pa_info, dense, _barcodes(bc))
    _check_mmread(tmp_path, "res.gene.pkl", dense)


@pytest.mark.gpu
def test_mtx_errors_and_empty(tmp_path):
    """unknown cell id below K: KeyError, no .part left, the previous output untouched; the same id at label K is not
    looked up; a tab in a gene name: ValueError; no read below K: an empty 0 x n matrix"""
    from scape.apa_core import Parameters
    rec = dict(gene_info_str="1:G:1:100-900:+", K=2, alpha_arr=np.array([10, 500]), beta_arr=np.array([5.0, 7.5]),
               label_arr=np.array([0, 1, 2, 1]), cb_id_arr=np.array([3, 4, 99, 4]))
    bc = "CB,index\nA-1,3\nB-1,4\n"
    rc.write_dir(str(tmp_path), "res.gene.pkl", [rec], bc, {}, Parameters)
    r = _run(_mtx_args(tmp_path))
    assert r.exit_code == 0, repr(r.exception)                     # id 99 has label K
    want = {"matrix.mtx.gz": BANNER + "2 2 2\n1 1 1\n2 2 2\n",
            "features.tsv.gz": "1:110:5.0:+:1:G:1\t1:110:5.0:+:1:G:1\tGene Expression\n"
                               "1:600:7.5:+:2:G:1\t1:600:7.5:+:2:G:1\tGene Expression\n",
            "barcodes.tsv.gz": "A-1\nB-1\n"}
    assert _read_dir(tmp_path) == want

    rec["label_arr"] = np.array([0, 1, 1, 1])
    rc.write_dir(str(tmp_path), "res.gene.pkl", [rec], bc, {}, Parameters)
    r = _run(_mtx_args(tmp_path))
    assert isinstance(r.exception, KeyError) and "99" in str(r.exception)
    assert not _parts_left(tmp_path)
    assert _read_dir(tmp_path) == want                             # the complete earlier output stays as it was

    tab = tmp_path / "tab"
    rc.write_dir(str(tab), "res.gene.pkl", [dict(rec, gene_info_str="1:G\tX:1:100-900:+",
                                                 label_arr=np.array([0, 1, 2, 1]))], bc, {}, Parameters)
    r = _run(_mtx_args(tab))
    assert isinstance(r.exception, ValueError) and "pa_info" in str(r.exception) and "G\\tX" in str(r.exception)
    assert not _parts_left(tab) and not os.path.exists(_mtx_dir(tab))

    empty = tmp_path / "empty"
    rc.write_dir(str(empty), "res.gene.pkl", [dict(rec, label_arr=np.array([2, 2, 5, 3])),
                                              dict(rec, gene_info_str="1:H:1:100-900:-", K=1, alpha_arr=np.array([7]),
                                                   beta_arr=np.array([5.0]), label_arr=np.array([1, 1]),
                                                   cb_id_arr=np.array([3, 77]))], bc, {}, Parameters)
    r = _run(_mtx_args(empty))
    assert r.exit_code == 0, repr(r.exception)
    assert _read_dir(empty) == {"matrix.mtx.gz": BANNER + "0 2 0\n", "features.tsv.gz": "",
                                "barcodes.tsv.gz": "A-1\nB-1\n"}
    _check_mmread(empty, "res.gene.pkl", np.zeros((0, 2), dtype=np.int64))


@pytest.mark.gpu
def test_mtx_chain_both_formats(tmp_path):
    """infer_pa_all (GPU) -> merge_pa -> ex_pa_cnt_mat in both formats in one directory: the matrix equals the parsed
    dense output of the same run, the mtx run leaves the dense file alone, and a dense run after it writes the same
    bytes as the dense-only run before it"""
    import merge_chain_dir as mc
    from scape_amd.apa_core import infer_all
    from scape_amd.junction_handler import _merge_pa
    mc.write_inputs(str(tmp_path))
    infer_all(str(tmp_path), gpus=1, rng_mode="per_utr", seed=mc.SEED, re_run_mode=True, **mc.KW)
    _merge_pa(str(tmp_path), True)
    _merge_pa(str(tmp_path), False)
    bc = rc.chain_barcode_csv()
    (tmp_path / "barcode_index.csv").write_text(bc)
    byname = {cs["name"]: cs for cs in rc.fixture_cases()}
    for tag in ("gene", "utr"):
        res = f"res.{tag}.pkl"
        gz = tmp_path / f"res.{tag}.cnt.tsv.gz"
        dense_args = ["ex_pa_cnt_mat", "--output_dir", str(tmp_path), "--res_pkl_file", res]
        assert _run(dense_args).exit_code == 0
        dense_only = gz.read_bytes()
        r = _run(_mtx_args(tmp_path, res))
        assert r.exit_code == 0, repr(r.exception)
        assert gz.read_bytes() == dense_only
        assert _run(dense_args + ["--format", "tsv"]).exit_code == 0
        assert gz.read_bytes() == dense_only
        with gzip.open(gz, "rt", newline="") as fh:
            body = fh.read().split("\n", 1)[1]
        assert body == byname[f"chain/{tag}"]["mat_body"]
        want, dense = _expected_from_dense(body, bc)
        assert dense.shape[0] > 0 and _read_dir(tmp_path, res) == want
        _check_mmread(tmp_path, res, dense)
