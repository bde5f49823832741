"""`scape ex_pa_cnt_mat` and `scape cal_exp_pa_len` (reference utils.py:319-427, :438-553) against the REFERENCE's own
outputs on the golden cases of tests/golden/fixture_report.npz (generator: tests/golden/make_golden_report.py): both
example directories, ~40 fuzzed directories and the infer_pa -> merge_pa chain directory.  The matrix is compared
byte for byte after decompression, the .pa.len.csv files byte for byte.

The golden directories are small (at most 407 matrix rows, counts up to 37 in a dense body, 46 bitmap words of cluster
codes): the boundary shapes of the kernels underneath - more than 1,024 rows in a render block, 255 / 256 / 257 columns,
counts of up to seven digits, more than 8,192 cluster codes - are tested in tests/test_report_ladder.py against the
exact oracle of tests/report_ladder.py."""
import gzip
import os

import numpy as np
import pytest

import report_cases as rc
from report_cases import no_gpu, run as _run  # noqa: F401  (no_gpu is a fixture)


# ---------------------------------------------------------------- CPU
def test_help_lists_both_commands():
    r = _run(["--help"])
    assert r.exit_code == 0, r.output
    assert "cal_exp_pa_len" in r.output and "ex_pa_cnt_mat" in r.output


@pytest.mark.parametrize("cmd,opts", [("cal_exp_pa_len", ["--output_dir", "--cell_cluster_file", "--res_pkl_file"]),
                                      ("ex_pa_cnt_mat", ["--output_dir", "--res_pkl_file"])])
def test_command_help(cmd, opts):
    r = _run([cmd, "--help"])
    assert r.exit_code == 0, r.output
    for o in opts:
        assert o in r.output


def test_utils_import_path():
    import scape.utils as su
    from scape_amd import report
    assert su.cal_exp_pa_len is report.cal_exp_pa_len and su.ex_pa_cnt_mat is report.ex_pa_cnt_mat


def test_ex_pa_cnt_mat_prerequisites(tmp_path, no_gpu):
    r = _run(["ex_pa_cnt_mat", "--output_dir", str(tmp_path / "nope"), "--res_pkl_file", "res.gene.pkl"])
    assert r.exit_code != 0 and "Given output_dir folder does not exists." in str(r.exception)
    r = _run(["ex_pa_cnt_mat", "--output_dir", str(tmp_path), "--res_pkl_file", "res.gene.pkl"])
    assert "Given res_pkl_file is not in output_dir." in str(r.exception)
    r = _run(["ex_pa_cnt_mat", "--output_dir", str(tmp_path)])              # default "None"
    assert "Invalid file" in str(r.exception) and "None" in str(r.exception)
    (tmp_path / "res.gene.pkl").write_bytes(b"")
    r = _run(["ex_pa_cnt_mat", "--output_dir", str(tmp_path), "--res_pkl_file", "res.gene.pkl"])
    assert isinstance(r.exception, FileNotFoundError) and "barcode_index.csv" in str(r.exception)


def test_cal_exp_pa_len_prerequisites(tmp_path, no_gpu):
    d = str(tmp_path)
    args = ["cal_exp_pa_len", "--output_dir", d, "--res_pkl_file", "res.gene.pkl"]
    assert "stores res pickle files by infer_pa" in str(_run(args).exception)
    os.makedirs(tmp_path / "pkl_output")
    assert "stores res pickle files by prepare_input" in str(_run(args).exception)
    os.makedirs(tmp_path / "pkl_input")
    assert "Must run apajunction before apaexppalen" in str(_run(args).exception)
    assert "Must run apajunction before apaexppalen" in str(_run(args[:3]).exception)     # default "None"
    (tmp_path / "res.gene.pkl").write_bytes(b"")
    assert "Please use the same output directory as in prepare_input and infer_pa" in str(_run(args).exception)
    (tmp_path / "barcode_index.csv").write_text("CB,index\nAAA-1,0\n")
    r = _run(args + ["--cell_cluster_file", str(tmp_path / "missing.csv")])
    assert "Given cell_cluster_file file does not exists" in str(r.exception)


def test_fixture_decodes():
    f = rc.fixture()
    ids = rc.case_ids(f)
    assert len(ids) >= 46
    names = [rc.case(f, c)["name"] for c in ids]
    assert {"SCZ-nowa-scape/gene", "SCZ-nowa-scape/utr", "toy-example/gene", "toy-example/utr",
            "chain/gene", "chain/utr"} <= set(names)
    assert sum(n.startswith("fuzz") for n in names) >= 40
    ks = []
    for c in ids:
        cs = rc.case(f, c)
        bc = rc.text(f, cs["barcode"])
        assert rc.digest(rc.header_line(bc)) == cs["mat_header"]
        assert len(cs["len_texts"]) == 1 + len(cs["clusters"])
        for r in cs["records"]:
            assert len(r["label_arr"]) == len(r["cb_id_arr"]) and len(r["alpha_arr"]) == r["K"]
            ks.append(r["K"])
    assert min(ks) == 1 and max(ks) > 63


# ---------------------------------------------------------------- GPU
def _check_outputs(cs, bc, paths, root, read_with_pandas=False):
    r = _run(["ex_pa_cnt_mat", "--output_dir", str(root), "--res_pkl_file", cs["res"]])
    assert r.exit_code == 0, (cs["name"], r.output, repr(r.exception))
    gz = os.path.join(str(root), cs["res"].replace(".pkl", ".cnt.tsv.gz"))
    with gzip.open(gz, "rt", newline="") as fh:
        mat = fh.read()
    hdr = rc.header_line(bc)
    assert mat[:len(hdr)] == hdr, cs["name"]
    assert mat[len(hdr):] == cs["mat_body"], cs["name"]
    assert not os.path.exists(gz + ".part")
    if read_with_pandas:
        import pandas as pd
        df = pd.read_csv(gz)
        assert df.shape == (cs["mat_body"].count("\n"), hdr.count(",") + 1)
    for j, cf in enumerate(["None"] + paths):
        r = _run(["cal_exp_pa_len", "--output_dir", str(root), "--cell_cluster_file", cf, "--res_pkl_file", cs["res"]])
        assert r.exit_code == 0, (cs["name"], cf, r.output, repr(r.exception))
        out = os.path.join(str(root), cs["len_names"][j])
        with open(out) as fh:
            assert fh.read() == cs["len_texts"][j], (cs["name"], cf)


@pytest.mark.gpu
@pytest.mark.parametrize("c", rc.case_params())
def test_report_case_vs_reference(c, tmp_path, monkeypatch):
    """Every golden case.  The fuzzed ones run with a batch budget and a render block so small that records go to
    the device in several batches and rows are rendered a few at a time; the example directories run with the batch
    sized from free device memory."""
    from scape_amd import report
    cs = rc.fixture_case(c)
    if cs["name"].startswith("fuzz"):
        monkeypatch.setattr(report, "MAX_BATCH_BYTES", 1 << 14)
        monkeypatch.setattr(report, "MAX_BLOCK_BYTES", 1 << 12)
        monkeypatch.setattr(report, "GZIP_PART", 1 << 11)
    bc, paths = rc.write_case(cs, tmp_path)
    _check_outputs(cs, bc, paths, tmp_path, read_with_pandas=not cs["name"].startswith("fuzz"))


@pytest.mark.gpu
def test_unknown_barcode_and_cluster_ids_raise(tmp_path):
    """A read whose cell id is not in barcode_index.csv (matrix; label < K) or in the cluster file is a KeyError, as in
    the reference; a read of the uniform component with an unknown id is not looked up by the matrix."""
    from scape.apa_core import Parameters
    rec = dict(gene_info_str="1:G:1:100-900:+", K=2, alpha_arr=np.array([10, 500]), beta_arr=np.array([5.0, 7.5]),
               label_arr=np.array([0, 1, 2, 1]), cb_id_arr=np.array([3, 4, 99, 4]))
    bc = "CB,index\nA-1,3\nB-1,4\n"
    rc.write_dir(str(tmp_path), "res.gene.pkl", [rec], bc, {"g.csv": "index,group\n3,x\n"}, Parameters)
    r = _run(["ex_pa_cnt_mat", "--output_dir", str(tmp_path), "--res_pkl_file", "res.gene.pkl"])
    assert r.exit_code == 0, repr(r.exception)                       # id 99 has label K
    r = _run(["cal_exp_pa_len", "--output_dir", str(tmp_path), "--cell_cluster_file", str(tmp_path / "g.csv"),
              "--res_pkl_file", "res.gene.pkl"])
    assert isinstance(r.exception, KeyError)
    rec["label_arr"] = np.array([0, 1, 1, 1])
    rc.write_dir(str(tmp_path), "res.gene.pkl", [rec], bc, {}, Parameters)
    r = _run(["ex_pa_cnt_mat", "--output_dir", str(tmp_path), "--res_pkl_file", "res.gene.pkl"])
    assert isinstance(r.exception, KeyError)
    assert not os.path.exists(tmp_path / "res.gene.cnt.tsv.gz.part")


@pytest.mark.gpu
def test_chain_infer_merge_then_report_vs_reference(tmp_path):
    """The whole tutorial chain on this package: infer_pa_all (GPU, rng_mode per_utr) -> merge_pa (both modes) ->
    ex_pa_cnt_mat and cal_exp_pa_len, compared with the reference's two commands on the reference-merged records of the
    same directory (fixture_merge_chain.npz -> fixture_report.npz cases chain/gene, chain/utr)."""
    import merge_chain_dir as mc
    from scape_amd.apa_core import infer_all
    from scape_amd.junction_handler import _merge_pa
    mc.write_inputs(str(tmp_path))
    infer_all(str(tmp_path), gpus=1, rng_mode="per_utr", seed=mc.SEED, re_run_mode=True, **mc.KW)
    _merge_pa(str(tmp_path), True)
    _merge_pa(str(tmp_path), False)
    bc = rc.chain_barcode_csv()
    (tmp_path / "barcode_index.csv").write_text(bc)
    clu = tmp_path / "chain_groups.csv"
    clu.write_text(rc.chain_cluster_csv())
    byname = {cs["name"]: cs for cs in rc.fixture_cases()}
    for tag in ("gene", "utr"):
        cs = byname[f"chain/{tag}"]
        _check_outputs(cs, bc, [str(clu)], tmp_path, read_with_pandas=True)
