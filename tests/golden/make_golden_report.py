"""Generator of tests/golden/fixture_report.npz: the REFERENCE's own `ex_pa_cnt_mat` and `cal_exp_pa_len`
(src/scape/utils.py:319-427, :438-553, current code - not the example directories' shipped .cnt.tsv.gz files, which
are stale) run through their click callbacks on

  * both example directories (res.gene.pkl / res.utr.pkl, without and with each shipped cluster file),
  * ~40 fuzzed directories (K 1..70, unsorted alphas, non-integer betas, labels == K, records without reads or without
    reads below K, complete multi-row pivots, barcode ids offset from row positions and never-seen barcodes, string /
    numeric / integer / NaN-mixed / all-NaN cluster groups, one cluster per cell, enough records for several batches),
  * the infer_pa -> merge_pa chain directory (tests/merge_chain_dir.py; records: the reference-merged ones of
    fixture_merge_chain.npz, barcode and cluster files: tests/report_cases.py).

The reference is imported as make_golden.load_reference does, with empty stand-ins for pybedtools and gffutils.
Run: python tests/golden/make_golden_report.py  (needs the reference checkout, CPU only)."""
import contextlib
import gzip
import io
import os
import shutil
import sys
import tempfile
import types
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import report_cases as rc  # noqa: E402
from make_golden import REF, load_reference  # noqa: E402

EXAMPLES = {"SCZ-nowa-scape": ["author_cell_type.csv", "author_cell_type_cond.csv"],
            "toy-example": ["cluster_wrt_CB.csv"]}


def load_reference_utils():
    load_reference()
    for name in ("pybedtools", "gffutils"):
        sys.modules.setdefault(name, types.ModuleType(name))
    import importlib
    with contextlib.redirect_stdout(io.StringIO()):
        return importlib.import_module("scape.utils")


def _u8(s):
    return rc.pack(s)


def run_reference(ut, records, barcode_csv, clusters, res_name):
    """(matrix text, [(output file name, .pa.len.csv text)]) of the reference on one directory"""
    Para = sys.modules["scape.apa_core"].Parameters
    root = tempfile.mkdtemp(prefix="report_case_")
    try:
        paths = rc.write_dir(root, res_name, records, barcode_csv, clusters, Para)
        with contextlib.redirect_stdout(io.StringIO()), warnings.catch_warnings(), np.errstate(all="ignore"):
            warnings.simplefilter("ignore")
            ut.ex_pa_cnt_mat.callback(output_dir=root, res_pkl_file=res_name)
            lens = []
            for cf in ["None"] + paths:
                before = set(os.listdir(root))
                ut.cal_exp_pa_len.callback(output_dir=root, cell_cluster_file=cf, res_pkl_file=res_name)
                new = sorted(set(os.listdir(root)) - before)
                assert len(new) == 1, new
                with open(os.path.join(root, new[0])) as fh:
                    lens.append((new[0], fh.read()))
        with gzip.open(os.path.join(root, res_name.replace(".pkl", ".cnt.tsv.gz")), "rt", newline="") as fh:
            mat = fh.read()
        return mat, lens
    finally:
        shutil.rmtree(root, ignore_errors=True)


class Store:
    def __init__(self):
        self.d = {}
        self.n = 0
        self.rec_keys = {}

    def blob(self, key, s):
        if "blob_" + key not in self.d:
            self.d["blob_" + key] = rc.pack_csv(s)
            assert rc.text(self.d, key) == s, key
        return key

    def recs(self, records):
        """record arrays under r<k>_, shared by cases with identical records"""
        import hashlib
        h = hashlib.sha256()
        for r in records:
            h.update(r["gene_info_str"].encode() + str(r["K"]).encode())
            for k in ("alpha_arr", "beta_arr", "label_arr", "cb_id_arr"):
                a = np.asarray(r[k])
                h.update(str(a.dtype).encode() + a.tobytes())
        key = h.hexdigest()
        if key in self.rec_keys:
            return self.rec_keys[key]
        k = len(self.rec_keys)
        self.rec_keys[key] = k
        p, d = f"r{k}_", self.d
        d[p + "rec_gene"] = np.array([r["gene_info_str"] for r in records]) if records else np.zeros(0, "<U1")
        d[p + "rec_K"] = np.array([r["K"] for r in records], dtype=np.int64)
        d[p + "rec_n"] = np.array([len(r["label_arr"]) for r in records], dtype=np.int64)
        d[p + "rec_na"] = np.array([len(r["alpha_arr"]) for r in records], dtype=np.int64)
        d[p + "alpha"] = np.concatenate([np.asarray(r["alpha_arr"]) for r in records]) if records else np.zeros(0, np.int64)
        d[p + "beta"] = np.concatenate([np.asarray(r["beta_arr"], dtype=np.float64) for r in records]) if records \
            else np.zeros(0)
        d[p + "label"] = np.concatenate([np.asarray(r["label_arr"], dtype=np.int64) for r in records]) if records \
            else np.zeros(0, np.int64)
        cb = np.concatenate([np.asarray(r["cb_id_arr"], dtype=np.int64) for r in records]) if records \
            else np.zeros(0, np.int64)
        assert len(cb) == 0 or (cb.min() >= -2 ** 31 and cb.max() < 2 ** 31)
        d[p + "cb"] = cb.astype(np.int32)
        return k

    def add(self, ut, name, records, barcode_key, clu, res_name):
        """clu: [(file name, blob key)]"""
        bc = rc.text(self.d, barcode_key)
        clusters = {fn: rc.text(self.d, k) for fn, k in clu}
        mat, lens = run_reference(ut, records, bc, clusters, res_name)
        hdr = rc.header_line(bc)
        assert mat.startswith(hdr), name
        c, p = self.n, f"c{self.n}_"
        d = self.d
        d[p + "name"] = np.array(name)
        d[p + "res"] = np.array(res_name)
        d[p + "barcode"] = np.array(barcode_key)
        d[p + "clu_files"] = np.array([fn for fn, _ in clu] or [""])[:len(clu)]
        d[p + "clu_keys"] = np.array([k for _, k in clu] or [""])[:len(clu)]
        d[p + "recs"] = np.array(self.recs(records))
        d[p + "mat_header"] = np.array(rc.digest(hdr))
        d[p + "mat_body"] = _u8(mat[len(hdr):])
        d[p + "len_names"] = np.array([n for n, _ in lens])
        for j, (_n, t) in enumerate(lens):
            d[p + f"len{j}"] = _u8(t)
        self.n += 1
        return c


# ---------------------------------------------------------------- cases
def example_cases(st, ut):
    from scape_amd import safe_pickle
    st.blob("bc_examples", open(os.path.join(REF, "examples", "SCZ-nowa-scape", "barcode_index.csv")).read())
    for ex, cfiles in EXAMPLES.items():
        clu = [(fn, st.blob(f"{ex}_{fn}", open(os.path.join(REF, "examples", ex, fn)).read())) for fn in cfiles]
        for mode in ("gene", "utr"):
            recs = []
            for p in safe_pickle.iter_pickles(os.path.join(REF, "examples", ex, f"res.{mode}.pkl")):
                recs.append(dict(gene_info_str=p.gene_info_str, K=int(p.K), alpha_arr=np.asarray(p.alpha_arr),
                                 beta_arr=np.asarray(p.beta_arr), label_arr=np.asarray(p.label_arr),
                                 cb_id_arr=np.asarray(p.cb_id_arr)))
            c = st.add(ut, f"{ex}/{mode}", recs, "bc_examples", clu, f"res.{mode}.pkl")
            print("case", c, ex, mode, len(recs), "records", flush=True)


def _cluster_text(rng, ids, kind, tag):
    vals = []
    for i in ids:
        if kind == "str":               # names that look numeric sort as strings: '10' < '2' < '9' < 'b'
            v = rng.choice(["10", "2", "9", "b", "a1"])
        elif kind == "float":
            v = rng.choice(["1.5", "2.0", "3", "0.25"])
        elif kind == "float_nan":
            v = rng.choice(["1.5", "2", "", "7"])
        elif kind == "int":
            v = str(rng.choice([3, 1, 2, 11]))
        elif kind == "str_nan":
            v = rng.choice(["T", "B", "", "NK cell"])
        elif kind == "all_nan":
            v = ""
        elif kind == "per_cell":
            v = f"cell{i}"
        else:
            raise ValueError(kind)
        vals.append(v)
    order = rng.permutation(len(ids))
    return "index,group\n" + "".join(f"{ids[j]},{vals[j]}\n" for j in order)


def fuzz_case(rng, ci):
    big = ci in (7, 23)                                           # one cluster per cell over many cells
    n_bc = int(rng.integers(800, 1500)) if big else int(rng.integers(3, 120))
    base = int(rng.choice([0, 0, 7, 1000, int(rng.integers(1, 50000))]))
    ids = base + np.sort(rng.choice(np.arange(n_bc * 3), n_bc, replace=False)) if rng.random() < 0.6 else \
        base + np.arange(n_bc)
    rows = rng.permutation(n_bc) if rng.random() < 0.5 else np.arange(n_bc)
    bc = "CB,index\n" + "".join(f"F{ci}_{ids[j]:06d}-1,{ids[j]}\n" for j in rows)
    n_rec = int(rng.integers(60, 120)) if ci in (3, 31) else int(rng.integers(1, 14))
    used = ids[: max(1, int(n_bc * rng.uniform(0.3, 1.0)))]       # barcodes after these never occur
    recs = []
    for r in range(n_rec):
        kk = rng.random()
        K = int(rng.integers(40, 71)) if kk < 0.08 else int(rng.integers(1, 4)) if kk < 0.6 else int(rng.integers(1, 9))
        alpha = rng.choice(np.arange(50, 4000), K, replace=False)
        if rng.random() < 0.6:
            alpha = np.sort(alpha)
        beta = rng.choice([5.0, 7.5, 10.0, 12.25, 30.0, 45.0, 17.0], K)
        shape = rng.random()
        if shape < 0.07:
            lab = np.zeros(0, np.int64)                          # no reads
        elif shape < 0.13:
            lab = np.full(int(rng.integers(1, 20)), K, np.int64)  # only the uniform component
        elif shape < 0.3:                                        # complete pivot: every cell in every chosen row
            labs = np.sort(rng.choice(K, int(rng.integers(1, min(K, 4) + 1)), replace=False))
            cells = rng.choice(used, int(rng.integers(1, min(len(used), 6) + 1)), replace=False)
            reps = rng.integers(1, 4, (len(labs), len(cells)))
            lab = np.repeat(np.repeat(labs, len(cells)), reps.ravel())
            cb = np.repeat(np.tile(cells, len(labs)), reps.ravel())
            if rng.random() < 0.5:                               # reads of the uniform component do not break it
                lab = np.concatenate([lab, [K, K]])
                cb = np.concatenate([cb, rng.choice(used, 2)])
            perm = rng.permutation(len(lab))
            lab, cb = lab[perm].astype(np.int64), cb[perm].astype(np.int64)
        else:
            n = int(rng.integers(1, 400 if not big else 3000))
            p = rng.dirichlet(np.ones(K + 1))
            lab = rng.choice(K + 1, n, p=p).astype(np.int64)
        if shape < 0.13 or shape >= 0.3:
            cb = rng.choice(used, len(lab)).astype(np.int64)
        st = int(rng.integers(1, 10 ** 7))
        strand = "-" if rng.random() < 0.4 else "+"
        recs.append(dict(gene_info_str=f"{rng.choice(['1', 'X', 'chr7'])}:GF{ci}.{r}:{int(rng.integers(1, 4))}:"
                                       f"{st}-{st + 5000}:{strand}",
                         K=K, alpha_arr=alpha.astype(np.int64), beta_arr=beta, label_arr=lab, cb_id_arr=cb))
    kinds = ["str", "float", "float_nan", "int", "str_nan", "all_nan"]
    if big:
        ck = ["per_cell"]
    else:
        ck = list(rng.choice(kinds, int(rng.integers(0, 3)), replace=False))
    return bc, recs, ids, ck


def fuzz_cases(st, ut, n=40, seed=20261016):
    rng = np.random.default_rng(seed)
    for ci in range(n):
        bc, recs, ids, kinds = fuzz_case(rng, ci)
        bkey = st.blob(f"fuzz{ci}_bc", bc)
        clu = [(f"grp_{k}.csv", st.blob(f"fuzz{ci}_{k}", _cluster_text(rng, ids, k, ci))) for k in kinds]
        res = "res.gene.pkl" if ci % 2 == 0 else "res.utr.pkl"
        c = st.add(ut, f"fuzz{ci}", recs, bkey, clu, res)
        print("case", c, f"fuzz{ci}", len(recs), "records", kinds, flush=True)


def chain_cases(st, ut):
    f = np.load(os.path.join(HERE, "fixture_merge_chain.npz"))
    bkey = st.blob("chain_bc", rc.chain_barcode_csv())
    clu = [("chain_groups.csv", st.blob("chain_groups", rc.chain_cluster_csv()))]
    for tag, res in (("gene", "res.gene.pkl"), ("utr", "res.utr.pkl")):
        recs = []
        for k in range(int(f[f"{tag}_n"])):
            p = f"{tag}{k}_"
            recs.append(dict(gene_info_str=str(f[p + "gene_info_str"]), K=int(f[p + "K"]), alpha_arr=f[p + "alpha_arr"],
                             beta_arr=f[p + "beta_arr"], label_arr=f[p + "label_arr"], cb_id_arr=f[p + "cb_id_arr"]))
        c = st.add(ut, f"chain/{tag}", recs, bkey, clu, res)
        print("case", c, "chain", tag, len(recs), "records", flush=True)


def main():
    ut = load_reference_utils()
    st = Store()
    example_cases(st, ut)
    fuzz_cases(st, ut)
    chain_cases(st, ut)
    st.d["case_ids"] = np.arange(st.n)
    path = os.path.join(HERE, "fixture_report.npz")
    np.savez_compressed(path, **st.d)
    print("wrote", path, os.path.getsize(path), "bytes,", st.n, "cases")


if __name__ == "__main__":
    main()
