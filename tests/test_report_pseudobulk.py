"""`scape ex_pa_pseudobulk`: the pA x cell count matrix summed over cell groups (pseudo-replicates for DEXSeq and the
share of each population's cells with a read), three small csv files.

The expected texts are built here, in plain Python, from the REFERENCE's own dense matrix body of the golden cases
(tests/golden/fixture_report.npz) and the definitions of the command, restated below without importing anything from
scape_amd: clusters as text, populations in order of first appearance, R's split(cells, sort(1:n %% k)) chunks.
Everything is an exact integer or one float64 division printed with repr(), so every comparison is byte for byte.

Kernel check done once by hand (not committed), on an MI355X: with every segment started one column late, 95 of the
98 GPU tests fail; with `>= 0` for `> 0` in the nonzero count, the same 95 fail.  The three that pass cannot see the
kernel: the case without a row (fuzz15, twice) and the cluster file whose fields are all empty (fuzz6)."""
import csv
import glob
import io
import os

import numpy as np
import pytest

import report_cases as rc
from report_cases import (cluster_rows as _cluster_rows, column_ids as _column_ids, dense_of_body as _dense_of_body,
                          first_clusters as _first_clusters, fixture_case as _case, fixture_cases as _cases, no_gpu,
                          parts_left as _parts_left, run as _run)  # noqa: F401  (no_gpu is a fixture)

KINDS = ("cnt", "pct", "samples")


def _args(root, clu, res="res.gene.pkl", k=None, id1=None, id2=None):
    a = ["ex_pa_pseudobulk", "--output_dir", str(root), "--res_pkl_file", res, "--cell_cluster_file", str(clu)]
    if k is not None:
        a += ["--num_splits", str(k)]
    if id1 is not None:
        a += ["--idents_1", id1]
    if id2 is not None:
        a += ["--idents_2", id2]
    return a


def _paths(root, clu, res, id1=None, id2=None):
    tag = "" if id1 is None else f".{id1}_vs_{id2 if id2 is not None else 'rest'}"
    kind = res[len("res."):-len(".pkl")]
    stem = os.path.splitext(os.path.basename(str(clu)))[0]
    return [os.path.join(str(root), f"{stem}.{kind}{tag}.pseudobulk.{w}.csv") for w in KINDS]


def _read_out(root, clu, res, id1=None, id2=None):
    out = {}
    for w, p in zip(KINDS, _paths(root, clu, res, id1, id2)):
        with open(p, newline="") as fh:
            out[w] = fh.read()
    return out


# ---------------------------------------------------------------- the definitions, restated
def r_split_sizes(n, k):
    """chunk sizes of R's split(cells, sort(1:n %% k)), transcribed literally: build 1:n %% k, sort it, run-length it
    (split() makes one chunk per distinct value, in ascending order; values that do not occur make no chunk).  Derived
    from R's documented %%, sort and split, not run in R."""
    vals = sorted(i % k for i in range(1, n + 1))
    sizes = []
    for j, v in enumerate(vals):
        if j and v == vals[j - 1]:
            sizes[-1] += 1
        else:
            sizes.append(1)
    return sizes


def _csv_text(rows):
    out = io.StringIO()
    csv.writer(out, delimiter=",", quoting=csv.QUOTE_MINIMAL, lineterminator="\n").writerows(rows)
    return out.getvalue()


def expected(pa_info, dense, bc_csv, clu_csv, k=6, id1=None, id2=None):
    """the three texts for a dense integer matrix [rows, columns of bc_csv] with rows named pa_info"""
    last, order = {}, []
    for i, name in _cluster_rows(clu_csv):
        last[i] = name                                      # a repeated id keeps its last row
        if name != "" and name not in order:
            order.append(name)                              # first appearance in the file
    col_clu = [last.get(i, "") for i in _column_ids(bc_csv)]
    assert len(col_clu) == dense.shape[1]
    if id1 is None:
        pops = [(c, [j for j, x in enumerate(col_clu) if x == c]) for c in order]
    elif id2 is not None:
        pops = [("Population1", [j for j, x in enumerate(col_clu) if x == id1]),
                ("Population2", [j for j, x in enumerate(col_clu) if x == id2])]
    else:
        pops = [("Population1", [j for j, x in enumerate(col_clu) if x == id1]),
                ("Population2", [j for j, x in enumerate(col_clu) if x != "" and x != id1])]
    pops = [(name, cols) for name, cols in pops if cols]
    samples = []                                            # (sample, population, split, columns)
    for name, cols in pops:
        a = 0
        for i, n in enumerate(r_split_sizes(len(cols), k)):
            samples.append((f"{name}_{i + 1}", name, i + 1, cols[a:a + n]))
            a += n
        assert a == len(cols)
    cnt = [["pa_info"] + [s[0] for s in samples]]
    pct = [["pa_info"] + [name for name, _ in pops]]
    for r, pa in enumerate(pa_info):
        row = dense[r]
        cnt.append([pa] + [int(row[s[3]].sum()) for s in samples])
        pct.append([pa] + [repr(int((row[cols] > 0).sum()) / len(cols)) for _, cols in pops])
    smp = [["sample", "population", "split", "n_cells"]] + [[s[0], s[1], s[2], len(s[3])] for s in samples]
    return {"cnt": _csv_text(cnt), "pct": _csv_text(pct), "samples": _csv_text(smp)}


# ---------------------------------------------------------------- CPU
def test_help_lists_command_and_options():
    r = _run(["--help"])
    assert r.exit_code == 0 and "ex_pa_pseudobulk" in r.output
    r = _run(["ex_pa_pseudobulk", "--help"])
    assert r.exit_code == 0, r.output
    for o in ("--output_dir", "--res_pkl_file", "--cell_cluster_file", "--num_splits", "--idents_1", "--idents_2"):
        assert o in r.output
    assert "default: 6" in r.output


def test_utils_import_path():
    import scape.utils as su
    from scape_amd import report
    assert su.ex_pa_pseudobulk is report.ex_pa_pseudobulk


def test_prerequisites_and_argument_errors(tmp_path, no_gpu):
    clu = tmp_path / "groups.csv"
    r = _run(_args(tmp_path / "nope", clu))
    assert r.exit_code != 0 and "Given output_dir folder does not exists." in str(r.exception)
    r = _run(_args(tmp_path, clu))
    assert "Given res_pkl_file is not in output_dir." in str(r.exception)
    r = _run(["ex_pa_pseudobulk", "--output_dir", str(tmp_path), "--cell_cluster_file", str(clu)])   # default "None"
    assert "Invalid file" in str(r.exception) and "None" in str(r.exception)
    (tmp_path / "res.gene.pkl").write_bytes(b"")
    r = _run(_args(tmp_path, clu))
    assert "Given cell_cluster_file file does not exists" in str(r.exception)
    clu.write_text("index,group\n3,A\n4,B\n5,\n")
    r = _run(_args(tmp_path, clu))
    assert isinstance(r.exception, FileNotFoundError) and "barcode_index.csv" in str(r.exception)
    (tmp_path / "barcode_index.csv").write_text("CB,index\nA-1,3\nB-1,4\nC-1,5\n")
    for extra, word in ((["--num_splits", "0"], "num_splits"), (["--num_splits", "-2"], "num_splits"),
                        (["--idents_2", "B"], "idents_1"), (["--idents_1", "A", "--idents_2", "A"], "same"),
                        (["--idents_1", "Z"], "'Z'"), (["--idents_1", "A", "--idents_2", "Z"], "'Z'"),
                        (["--idents_1", ""], "names no cluster")):
        r = _run(_args(tmp_path, clu) + extra)
        assert isinstance(r.exception, ValueError) and word in str(r.exception), (extra, repr(r.exception))
    r = _run(["ex_pa_pseudobulk", "--output_dir", str(tmp_path), "--res_pkl_file", "res.gene.pkl"])
    assert r.exit_code == 2 and "--cell_cluster_file" in r.output
    assert sorted(os.listdir(tmp_path)) == ["barcode_index.csv", "groups.csv", "res.gene.pkl"]


def test_split_rule():
    from scape_amd import report
    assert r_split_sizes(7, 6) == [1, 2, 1, 1, 1, 1]
    assert r_split_sizes(3, 6) == [1, 1, 1]
    assert r_split_sizes(12, 6) == [2] * 6
    assert r_split_sizes(0, 6) == []
    for n, k, want in ((7, 6, [1, 2, 1, 1, 1, 1]), (3, 6, [1, 1, 1]), (12, 6, [2] * 6), (0, 6, [])):
        assert report._split_sizes(n, k) == want
    for n in range(0, 41):
        for k in range(1, 9):
            got = report._split_sizes(n, k)
            assert got == r_split_sizes(n, k), (n, k)
            assert sum(got) == n and all(c > 0 for c in got)


def test_grouping_of_hand_written_files(tmp_path):
    """scrambled id order, a repeated id (last row wins), ids on one side only, empty fields, a cluster named NA"""
    from scape_amd import report
    col_ids = np.array([40, 7, 12, 3, 99, 21, 5, 8], dtype=np.int64)          # column j = row j of barcode_index.csv
    clu = tmp_path / "c.csv"
    clu.write_text("index,group,other\n12,T,x\n7,NA,x\n500,ghost,x\n3,,x\n21,T,x\n40,B,x\n7,B,x\n5,NA,x\n99,007,x\n")
    ids, names = report._read_clusters(str(clu))
    assert ids.tolist() == [12, 7, 500, 3, 21, 40, 7, 5, 99]
    assert names == ["T", "NA", "ghost", "", "T", "B", "B", "NA", "007"]       # text as written: NA and 007 stay
    col_clu, order = report._column_clusters(col_ids, ids, names)
    assert col_clu == ["B", "B", "T", None, "007", "T", "NA", None]            # id 7: last row; id 3: empty; id 8: absent
    assert order == ["T", "NA", "ghost", "B", "007"]
    pops = report._populations(col_clu, order, None, None)
    assert [(n, c.tolist()) for n, c in pops] == [("T", [2, 5]), ("NA", [6]), ("B", [0, 1]), ("007", [4])]
    table, slot, seg_off, seg_pop = report._samples(pops, 6, len(col_ids))
    assert table == [["T_1", "T", 1, 1], ["T_2", "T", 2, 1], ["NA_1", "NA", 1, 1], ["B_1", "B", 1, 1],
                     ["B_2", "B", 2, 1], ["007_1", "007", 1, 1]]
    assert slot.tolist() == [3, 4, 0, 6, 5, 1, 2, 7] and seg_off.tolist() == [0, 1, 2, 3, 4, 5, 6]
    assert seg_pop.tolist() == [0, 0, 1, 2, 2, 3]
    table, slot, seg_off, _ = report._samples(pops, 1, len(col_ids))
    assert [t[0] for t in table] == ["T_1", "NA_1", "B_1", "007_1"] and seg_off.tolist() == [0, 2, 3, 5, 6]
    assert slot.tolist() == [3, 4, 0, 6, 5, 1, 2, 7]
    pops = report._populations(col_clu, order, "NA", None)
    assert [(n, c.tolist()) for n, c in pops] == [("Population1", [6]), ("Population2", [0, 1, 2, 4, 5])]
    pops = report._populations(col_clu, order, "B", "T")
    assert [(n, c.tolist()) for n, c in pops] == [("Population1", [0, 1]), ("Population2", [2, 5])]
    pops = report._populations(col_clu, order, "ghost", "T")                   # a cluster without a column: no table column
    assert [(n, c.tolist()) for n, c in pops] == [("Population2", [2, 5])]
    with pytest.raises(ValueError, match="names no cluster"):
        report._populations(col_clu, order, "nope", None)
    # the restatement of this file agrees on the same input
    bc = "CB,index\n" + "".join(f"X{j}-1,{i}\n" for j, i in enumerate(col_ids.tolist()))
    dense = np.arange(16, dtype=np.int64).reshape(2, 8) % 3
    want = expected(["p", "q"], dense, bc, clu.read_text(), 6)
    assert want["cnt"] == "pa_info,T_1,T_2,NA_1,B_1,B_2,007_1\np,2,2,0,0,1,1\nq,1,1,2,2,0,0\n"
    assert want["pct"] == "pa_info,T,NA,B,007\np,1.0,0.0,0.5,1.0\nq,1.0,1.0,0.5,0.0\n"


# ---------------------------------------------------------------- GPU
def _golden_params():
    out = []
    for c in rc.case_ids(rc.fixture()):
        cs = _case(c)
        for j, fn in enumerate(cs["clu_files"]):
            out.append(pytest.param(c, j, id=f"{cs['name'].replace('/', '-')}-{fn}"))
    return out


def _check(root, clu_path, clu_text, res, pa, dense, bc, k=None, id1=None, id2=None, what=""):
    r = _run(_args(root, clu_path, res, k, id1, id2))
    assert r.exit_code == 0, (what, r.output, repr(r.exception))
    lines = r.output.splitlines()
    assert len(lines) == 2 and lines[0].startswith("Finish pseudo-bulk") and lines[1].startswith("Finish ")
    want = expected(pa, dense, bc, clu_text, 6 if k is None else k, id1, id2)
    got = _read_out(root, clu_path, res, id1, id2)
    for w in KINDS:
        print(what, "k", k, w, "bytes", len(got[w]), "equal", got[w] == want[w])
        assert got[w] == want[w], (what, k, id1, id2, w)
    assert not _parts_left(root)
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("c,j", _golden_params())
def test_golden_case_and_cluster_file(c, j, tmp_path):
    """every golden case with each of its cluster files, num_splits default, 1 and 4"""
    cs = _case(c)
    texts = rc.cluster_texts(cs)
    bc, paths = rc.write_case(cs, tmp_path)
    fn = cs["clu_files"][j]
    pa, dense = _dense_of_body(cs["mat_body"], len(_column_ids(bc)))
    for k in (None, 1, 4):
        _check(tmp_path, paths[j], texts[fn], cs["res"], pa, dense, bc, k, what=f"{cs['name']}/{fn}")
    before = sorted(os.listdir(tmp_path))
    assert len([n for n in before if ".pseudobulk." in n]) == 3


def _own_cluster_files(col_ids):
    """cluster files written for any barcode list: partial coverage, reversed order, one cluster per cell, clusters
    of very unequal size (with 1,200 columns or more: 383 and 389 cells, which the default 6 splits cut into chunks
    of 63, 64 and 65 columns, beside one of all the rest; the last 7 columns in no group)"""
    n = len(col_ids)
    out = {"own_partial.csv": "index,group\n" + "".join(f"{i},c{j % 4}\n" for j, i in enumerate(col_ids) if j % 3 != 2),
           "own_reversed.csv": "group,index\n" + "".join(f"k{j % 5},{col_ids[j]}\n" for j in reversed(range(n))),
           "own_per_cell.csv": "index,group\n" + "".join(f"{i},cell{i}\n" for i in col_ids)}
    if n >= 1200:
        def name(j):
            return "" if j >= n - 7 else "s63" if 5 <= j < 388 else "s65" if 388 <= j < 777 else "big"
    else:
        def name(j):
            return "small" if j == n // 2 else "big"
    out["own_unequal.csv"] = "index,group\n" + "".join(f"{i},{name(j)}\n" for j, i in enumerate(col_ids))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("c", rc.case_params())
def test_golden_case_with_written_cluster_files(c, tmp_path):
    cs = _case(c)
    col_ids = _column_ids(rc.text(rc.fixture(), cs["barcode"]))
    texts = _own_cluster_files(col_ids)
    bc, paths = rc.write_case(cs, tmp_path, texts)
    pa, dense = _dense_of_body(cs["mat_body"], len(col_ids))
    for (fn, text), path in zip(texts.items(), paths):
        got = _check(tmp_path, path, text, cs["res"], pa, dense, bc, what=f"{cs['name']}/{fn}")
        sizes = [int(ln.rsplit(",", 1)[1]) for ln in got["samples"].splitlines()[1:]]
        if fn == "own_per_cell.csv":
            assert set(sizes) <= {1} and len(sizes) == len(col_ids)
        if fn == "own_unequal.csv" and len(col_ids) >= 1200:
            assert {63, 64, 65} <= set(sizes) and max(sizes) >= 100
        if fn == "own_unequal.csv" and len(col_ids) >= 30000:
            assert max(sizes) > 5000


def _ident_cases():
    names = ["SCZ-nowa-scape/gene", "fuzz0", "fuzz4", "fuzz21"]
    byname = {cs["name"]: c for c, cs in zip(rc.case_ids(rc.fixture()), _cases())}
    return [pytest.param(byname[n], id=n.replace("/", "-")) for n in names]


@pytest.mark.gpu
@pytest.mark.parametrize("c", _ident_cases())
def test_idents(c, tmp_path):
    """--idents_1 A --idents_2 B, and --idents_1 A alone (Population2 = every other cluster)"""
    cs = _case(c)
    texts = rc.cluster_texts(cs)
    bc, paths = rc.write_case(cs, tmp_path)
    pa, dense = _dense_of_body(cs["mat_body"], len(_column_ids(bc)))
    fn, path = cs["clu_files"][-1], paths[-1]
    order = _first_clusters(texts[fn])
    assert len(order) >= 3
    a, b = order[1], order[-1]
    for id1, id2, k in ((a, b, None), (b, a, 4), (a, None, None), (order[0], None, 1)):
        got = _check(tmp_path, path, texts[fn], cs["res"], pa, dense, bc, k, id1, id2, what=f"{cs['name']}/{fn}")
        assert got["pct"].startswith("pa_info,Population1,Population2\n")
    assert os.path.basename(_paths(tmp_path, path, cs["res"], a, None)[0]).count(f".{a}_vs_rest.pseudobulk.cnt.csv") == 1


@pytest.mark.gpu
def test_batch_invariance(tmp_path, monkeypatch):
    """the golden case with the most rows: a batch budget of 16 KiB gives the same bytes in several device calls"""
    from scape_amd import _lib, report
    cs = max(_cases(), key=lambda x: x["mat_body"].count("\n"))
    col_ids = _column_ids(rc.text(rc.fixture(), cs["barcode"]))
    texts = _own_cluster_files(col_ids)
    bc, paths = rc.write_case(cs, tmp_path, texts)
    pa, dense = _dense_of_body(cs["mat_body"], len(col_ids))
    path, text = paths[0], texts["own_partial.csv"]
    big = _check(tmp_path, path, text, cs["res"], pa, dense, bc, what="default budget")
    lib = _lib.load_library()
    real, calls = lib.scape_hip_report_group_sums, []

    def counted(*a):
        calls.append(a[3])
        return real(*a)
    monkeypatch.setattr(lib, "scape_hip_report_group_sums", counted)
    monkeypatch.setattr(report, "MAX_BATCH_BYTES", 1 << 14)
    small = _check(tmp_path, path, text, cs["res"], pa, dense, bc, what="16 KiB budget")
    assert small == big
    assert len(calls) > 3 and sum(calls) == len(pa)


@pytest.mark.gpu
@pytest.mark.parametrize("small", [False, True], ids=["default_sizes", "small_batches"])
def test_wide_stream_vs_add_at(small, tmp_path, monkeypatch):
    """3,100 barcodes with scrambled ids and a repeated id, K up to 70, counts in the hundreds: expected sums from the
    np.add.at restatement of the counts (report_cases.wide_stream)"""
    from scape.apa_core import Parameters
    from scape_amd import report
    recs, bc, pa, dense = rc.wide_stream()
    col_ids = _column_ids(bc)
    if small:
        monkeypatch.setattr(report, "MAX_BATCH_BYTES", 1 << 20)
    texts = _own_cluster_files(col_ids)
    texts["own_types.csv"] = "index,group\n" + "".join(f"{i},type{(i // 3) % 12}\n" for i in sorted(set(col_ids))[::-1])
    paths = rc.write_dir(str(tmp_path), "res.gene.pkl", recs, bc, texts, Parameters)
    for (fn, text), path in zip(texts.items(), paths):
        for k in (None, 3):
            _check(tmp_path, path, text, "res.gene.pkl", pa, dense, bc, k, what=fn)
    _check(tmp_path, paths[-1], texts["own_types.csv"], "res.gene.pkl", pa, dense, bc, None, "type3", what="idents")


@pytest.mark.gpu
def test_group_sums_entry_point():
    """the C entry point on its own: segments of 0, 1, 63, 64, 65 and 4,000 columns, columns before the first and
    behind the last segment, 70 rows of one record; sums and nonzero counts against numpy"""
    from scape_amd import _lib
    from scape_amd._lib import P_i32, P_i64, check, ptr
    rng = np.random.default_rng(3)
    lens = [0, 1, 63, 0, 64, 65, 4000, 2, 0, 129, 1, 1, 1, 300]
    lead, n_cols = 3, 3 + sum(lens) + 11
    seg_off = (lead + np.concatenate([[0], np.cumsum(lens)])).astype(np.int32)
    K, n = 70, 60000
    lab = rng.integers(0, K + 1, n).astype(np.int64)
    cb = (rng.integers(0, n_cols, n) ** 2 // n_cols).astype(np.int64)           # skewed: many empty columns
    off, Ks = np.array([0, n], dtype=np.int64), np.array([K], dtype=np.int32)
    want = np.zeros((K, n_cols), dtype=np.int64)
    np.add.at(want, (lab[lab < K], cb[lab < K]), 1)
    ctx = _lib.default_context(None)
    try:
        assert np.array_equal(rc.device_counts(ctx, Ks, off, lab, cb, n_cols), want.sum(axis=1))
        rows = np.arange(K, dtype=np.int64)[::-1].copy()
        n_seg = len(lens)
        sums, nz = np.full((K, n_seg), -1, np.int32), np.full((K, n_seg), -1, np.int32)
        check(ctx.lib.scape_hip_report_group_sums(ctx.h, n_seg, ptr(seg_off, P_i32), K, ptr(rows, P_i64),
                                                  ptr(sums, P_i32), ptr(nz, P_i32)), "group_sums")
        for s in range(n_seg):
            blk = want[rows][:, seg_off[s]:seg_off[s + 1]]
            assert np.array_equal(sums[:, s], blk.sum(axis=1)), s
            assert np.array_equal(nz[:, s], (blk > 0).sum(axis=1)), s
        bad_off = seg_off.copy()
        bad_off[-1] = n_cols + 1
        assert ctx.lib.scape_hip_report_group_sums(ctx.h, n_seg, ptr(bad_off, P_i32), K, ptr(rows, P_i64),
                                                   ptr(sums, P_i32), ptr(nz, P_i32)) != 0
        rows[0] = K
        assert ctx.lib.scape_hip_report_group_sums(ctx.h, n_seg, ptr(seg_off, P_i32), K, ptr(rows, P_i64),
                                                   ptr(sums, P_i32), ptr(nz, P_i32)) != 0
    finally:
        ctx.lib.scape_hip_report_free(ctx.h)


@pytest.mark.gpu
def test_chain_directory(tmp_path):
    """infer_pa_all (GPU) -> merge_pa -> ex_pa_cnt_mat -> ex_pa_pseudobulk in one directory: the tables are the sums
    of the dense file of the same run, which equals the reference's"""
    import gzip
    import merge_chain_dir as mc
    from scape_amd.apa_core import infer_all
    from scape_amd.junction_handler import _merge_pa
    mc.write_inputs(str(tmp_path))
    infer_all(str(tmp_path), gpus=1, rng_mode="per_utr", seed=mc.SEED, re_run_mode=True, **mc.KW)
    _merge_pa(str(tmp_path), True)
    _merge_pa(str(tmp_path), False)
    bc, clu_text = rc.chain_barcode_csv(), rc.chain_cluster_csv()
    (tmp_path / "barcode_index.csv").write_text(bc)
    clu = tmp_path / "chain_groups.csv"
    clu.write_text(clu_text)
    byname = {cs["name"]: cs for cs in _cases()}
    for tag in ("gene", "utr"):
        res = f"res.{tag}.pkl"
        assert _run(["ex_pa_cnt_mat", "--output_dir", str(tmp_path), "--res_pkl_file", res]).exit_code == 0
        with gzip.open(tmp_path / f"res.{tag}.cnt.tsv.gz", "rt", newline="") as fh:
            body = fh.read().split("\n", 1)[1]
        assert body == byname[f"chain/{tag}"]["mat_body"]
        pa, dense = _dense_of_body(body, 450)
        assert len(pa) > 0
        _check(tmp_path, clu, clu_text, res, pa, dense, bc, what=f"chain/{tag}")
        _check(tmp_path, clu, clu_text, res, pa, dense, bc, 2, "grp1", "grp3", what=f"chain/{tag} idents")


@pytest.mark.gpu
def test_unknown_cell_id(tmp_path):
    """a read below K whose cell id is not in barcode_index.csv: KeyError naming the record, nothing written, no
    .part left, earlier complete outputs untouched; the same id at label K is not looked up"""
    from scape.apa_core import Parameters
    rec = dict(gene_info_str="1:G:1:100-900:+", K=2, alpha_arr=np.array([10, 500]), beta_arr=np.array([5.0, 7.5]),
               label_arr=np.array([0, 1, 2, 1]), cb_id_arr=np.array([3, 4, 99, 4]))
    bc = "CB,index\nA-1,3\nB-1,4\nC-1,5\n"
    clu_text = "index,group\n4,x\n3,y\n"
    paths = rc.write_dir(str(tmp_path), "res.gene.pkl", [rec], bc, {"g.csv": clu_text}, Parameters)
    r = _run(_args(tmp_path, paths[0]))
    assert r.exit_code == 0, repr(r.exception)                     # id 99 has label K
    want = {"cnt": "pa_info,x_1,y_1\n1:110:5.0:+:1:G:1,0,1\n1:600:7.5:+:2:G:1,2,0\n",
            "pct": "pa_info,x,y\n1:110:5.0:+:1:G:1,0.0,1.0\n1:600:7.5:+:2:G:1,1.0,0.0\n",
            "samples": "sample,population,split,n_cells\nx_1,x,1,1\ny_1,y,1,1\n"}
    assert _read_out(tmp_path, paths[0], "res.gene.pkl") == want
    rec["label_arr"] = np.array([0, 1, 1, 1])
    rc.write_dir(str(tmp_path), "res.gene.pkl", [rec], bc, {"g.csv": clu_text, "h.csv": clu_text}, Parameters)
    for name in ("g.csv", "h.csv"):
        r = _run(_args(tmp_path, tmp_path / name))
        assert isinstance(r.exception, KeyError) and "99" in str(r.exception) and "1:G:1:100-900:+" in str(r.exception)
    assert not _parts_left(tmp_path)
    assert _read_out(tmp_path, paths[0], "res.gene.pkl") == want   # the complete earlier output stays as it was
    assert not glob.glob(os.path.join(str(tmp_path), "h.*"))[1:]   # h.csv itself and nothing else
    # a row whose reads all fall on cells of no group stays, with zeros; a cluster file without any group
    rec["cb_id_arr"] = np.array([5, 4, 5, 4])
    rc.write_dir(str(tmp_path), "res.gene.pkl", [rec], bc, {"g.csv": clu_text, "none.csv": "index,group\n3,\n"},
                 Parameters)
    assert _run(_args(tmp_path, paths[0])).exit_code == 0
    assert _read_out(tmp_path, paths[0], "res.gene.pkl")["cnt"] == \
        "pa_info,x_1,y_1\n1:110:5.0:+:1:G:1,0,0\n1:600:7.5:+:2:G:1,2,0\n"
    assert _run(_args(tmp_path, tmp_path / "none.csv")).exit_code == 0
    assert _read_out(tmp_path, tmp_path / "none.csv", "res.gene.pkl") == \
        {"cnt": "pa_info\n1:110:5.0:+:1:G:1\n1:600:7.5:+:2:G:1\n", "pct": "pa_info\n1:110:5.0:+:1:G:1\n1:600:7.5:+:2:G:1\n",
         "samples": "sample,population,split,n_cells\n"}
