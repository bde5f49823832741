"""Directories of the cal_exp_pa_len / ex_pa_cnt_mat golden cases (tests/golden/fixture_report.npz), shared by the
generator (tests/golden/make_golden_report.py, which runs the REFERENCE's two commands on them) and by
tests/test_report.py (which runs this build's).

A case is a result stream (records with gene_info_str, K, alpha_arr, beta_arr, label_arr, cb_id_arr), a
barcode_index.csv text, cluster file texts, and the reference's outputs: the decompressed count matrix (header kept as
a digest: it is the barcode list, stored once per barcode file) and one .pa.len.csv text per cluster file (None
first).  Texts are stored as uint8 arrays; cases name shared texts through `blob_<key>` entries."""
import hashlib
import os
import pickle

import numpy as np


def pack(s):
    """a text as lzma-compressed uint8 (the npz's own deflate leaves 20x more of the mostly-"0.0" matrix rows)"""
    import lzma
    return np.frombuffer(lzma.compress(s.encode(), preset=9), dtype=np.uint8)


def unpack(a):
    import lzma
    return lzma.decompress(a.tobytes()).decode()


def pack_csv(s):
    """a two-column csv whose `index` column counts 0, 1, ... in row order is kept as its other column only"""
    lines = s.split("\n")
    head = lines[0].split(",")
    body = lines[1:-1] if s.endswith("\n") else None
    if body is not None and len(head) == 2 and "index" in head:
        ip = head.index("index")
        vals = []
        for i, ln in enumerate(body):
            parts = ln.split(",")
            if len(parts) != 2 or parts[ip] != str(i):
                break
            vals.append(parts[1 - ip])
        else:
            return pack(f"seq{ip}\n{lines[0]}\n" + "\n".join(vals))
    return pack("raw\n" + s)


def text(f, key):
    """a text stored by pack_csv"""
    s = unpack(f["blob_" + key])
    kind, rest = s.split("\n", 1)
    if kind == "raw":
        return rest
    ip = int(kind[3:])
    head, vals = rest.split("\n", 1)
    vals = vals.split("\n")
    rows = [f"{i},{v}" if ip == 0 else f"{v},{i}" for i, v in enumerate(vals)]
    return head + "\n" + "".join(r + "\n" for r in rows)


def header_line(barcode_csv):
    """the matrix header the reference writes for a barcode_index.csv (csv QUOTE_ALL)"""
    import csv
    import io
    import pandas as pd
    cb = pd.read_csv(io.StringIO(barcode_csv), index_col="index")["CB"].tolist()
    out = io.StringIO()
    csv.writer(out, delimiter=',', quoting=csv.QUOTE_ALL, lineterminator='\n').writerow(["pa_info"] + cb)
    return out.getvalue()


def digest(s):
    return hashlib.sha256(s.encode()).hexdigest()


def case_ids(f):
    return [int(i) for i in f["case_ids"]]


def case(f, c):
    p, q = f"c{c}_", f"r{int(f[f'c{c}_recs'])}_"
    n, na = f[q + "rec_n"], f[q + "rec_na"]
    ro, ao = np.concatenate([[0], np.cumsum(n)]), np.concatenate([[0], np.cumsum(na)])
    recs = []
    for r in range(len(n)):
        recs.append(dict(gene_info_str=str(f[q + "rec_gene"][r]), K=int(f[q + "rec_K"][r]),
                         alpha_arr=f[q + "alpha"][ao[r]:ao[r + 1]], beta_arr=f[q + "beta"][ao[r]:ao[r + 1]],
                         label_arr=f[q + "label"][ro[r]:ro[r + 1]],
                         cb_id_arr=f[q + "cb"][ro[r]:ro[r + 1]].astype(np.int64)))
    clusters = [str(k) for k in f[p + "clu_keys"]]
    return dict(name=str(f[p + "name"]), res=str(f[p + "res"]), barcode=str(f[p + "barcode"]), records=recs,
                clusters=clusters, clu_files=[str(k) for k in f[p + "clu_files"]],
                mat_body=unpack(f[p + "mat_body"]), mat_header=str(f[p + "mat_header"]),
                len_names=[str(k) for k in f[p + "len_names"]],
                len_texts=[unpack(f[p + f"len{j}"]) for j in range(len(f[p + "len_names"]))])


def write_dir(root, res_name, records, barcode_csv, cluster_texts, para_cls):
    """output_dir layout of the reference: pkl_input/, pkl_output/, barcode_index.csv, the result stream and the
    cluster files {file name: text}; records pickled as para_cls objects the way merge_pa writes them"""
    os.makedirs(os.path.join(root, "pkl_input"), exist_ok=True)
    os.makedirs(os.path.join(root, "pkl_output"), exist_ok=True)
    with open(os.path.join(root, "barcode_index.csv"), "w") as fh:
        fh.write(barcode_csv)
    with open(os.path.join(root, res_name), "wb") as fh:
        for r in records:
            K = int(r["K"])
            p = para_cls(title="Final Result", alpha_arr=np.asarray(r["alpha_arr"]), beta_arr=np.asarray(r["beta_arr"]),
                         ws=np.full(K, 1.0 / max(K, 1)), L=0, cb_id_arr=np.asarray(r["cb_id_arr"]),
                         readID_arr=np.arange(len(r["cb_id_arr"]), dtype=np.int64))
            p.K = K
            p.label_arr = np.asarray(r["label_arr"])
            p.gene_info_str = r["gene_info_str"]
            pickle.dump(p, fh)
    paths = []
    for name, body in cluster_texts.items():
        path = os.path.join(root, name)
        with open(path, "w") as fh:
            fh.write(body)
        paths.append(path)
    return paths


# ---------------------------------------------------------------- the infer_pa -> merge_pa chain directory
def chain_barcode_csv(n_ids=450):
    """barcode_index.csv of the chain directory (tests/merge_chain_dir.py: cell ids 0..399): ids in a scrambled row
    order, 50 barcodes that no read carries"""
    rows = ["CB,index"] + [f"CHAIN-{(j * 7) % n_ids:04d}-1,{(j * 7) % n_ids}" for j in range(n_ids)]
    return "\n".join(rows) + "\n"


def chain_cluster_csv(n_ids=450):
    """cluster file of the chain directory: string groups mixed with NaN (empty fields)"""
    rows = ["index,group"] + [f"{i}," + ("" if i % 11 == 0 else f"grp{i % 4}") for i in range(n_ids)]
    return "\n".join(rows) + "\n"
