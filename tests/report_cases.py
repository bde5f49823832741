"""Directories of the cal_exp_pa_len / ex_pa_cnt_mat golden cases (tests/golden/fixture_report.npz), shared by the
generator (tests/golden/make_golden_report.py, which runs the REFERENCE's two commands on them) and by
tests/test_report*.py (which run this build's), and the scaffolding those test files share: the CLI runner, the case
loaders, the commands' definitions restated in plain Python and the common parts of the permutation tests' oracle.
Nothing below "the definitions, restated" imports from scape_amd.

A case is a result stream (records with gene_info_str, K, alpha_arr, beta_arr, label_arr, cb_id_arr), a
barcode_index.csv text, cluster file texts, and the reference's outputs: the decompressed count matrix (header kept as
a digest: it is the barcode list, stored once per barcode file) and one .pa.len.csv text per cluster file (None
first).  Texts are stored as uint8 arrays; cases name shared texts through `blob_<key>` entries."""
import csv
import functools
import glob
import hashlib
import io
import os
import pickle
from fractions import Fraction

import numpy as np
import pytest


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


# ---------------------------------------------------------------- running the commands
def run(args):
    from click.testing import CliRunner
    from scape.cli import cli
    return CliRunner().invoke(cli, args)


@pytest.fixture
def no_gpu(monkeypatch):
    from scape_amd import _lib

    def refuse(*a, **k):
        raise AssertionError("the GPU was touched before the prerequisite checks")
    monkeypatch.setattr(_lib, "default_context", refuse)
    monkeypatch.setattr(_lib, "Context", refuse)


def parts_left(root):
    return glob.glob(os.path.join(str(root), "**", "*.part"), recursive=True)


def perm_args(cmd, root, clu, res="res.gene.pkl", id1=None, id2=None, n_perm=None, seed=None):
    """command line of diff_pa / diff_pa_len"""
    a = [cmd, "--output_dir", str(root), "--res_pkl_file", res, "--cell_cluster_file", str(clu)]
    for opt, v in (("--idents_1", id1), ("--idents_2", id2), ("--n_perm", n_perm), ("--seed", seed)):
        if v is not None:
            a += [opt, str(v)]
    return a


def perm_path(cmd, root, clu, res, id1, id2):
    kind = res[len("res."):-len(".pkl")]
    stem = os.path.splitext(os.path.basename(str(clu)))[0]
    return os.path.join(str(root), f"{stem}.{kind}.{id1}_vs_{id2 if id2 is not None else 'rest'}.{cmd}.csv")


def perm_command(cmd, root, clu, res, id1, id2, n_perm, seed, what=""):
    """the text of the file that diff_pa / diff_pa_len writes"""
    r = run(perm_args(cmd, root, clu, res, id1, id2, n_perm, seed))
    assert r.exit_code == 0, (what, r.output, repr(r.exception))
    assert not parts_left(root)
    with open(perm_path(cmd, root, clu, res, id1, id2), newline="") as fh:
        return fh.read()


def device_counts(ctx, Ks, off, lab, cb, n_cols):
    """scape_hip_report_counts of records given as arrays, cell id = matrix column: the row totals"""
    from scape_amd._lib import P_i8, P_i32, P_i64, check, ptr
    table = np.arange(n_cols, dtype=np.int32)
    row_tot, complete, bad = np.zeros(int(Ks.sum()), np.int64), np.zeros(len(Ks), np.int8), np.zeros(2, np.int64)
    check(ctx.lib.scape_hip_report_counts(ctx.h, len(Ks), ptr(off, P_i64), ptr(Ks, P_i32), ptr(lab, P_i64),
                                          ptr(cb, P_i64), 0, n_cols, ptr(table, P_i32), n_cols, ptr(row_tot, P_i64),
                                          ptr(complete, P_i8), ptr(bad, P_i64)), "counts")
    return row_tot


def entry_point_matrix():
    """the hand-made matrix of the permutation entry points' tests: records of 2, 5, 70 and 150 rows (the last two are
    taken in groups of 64 rows), 70 + 91 tested columns in front of 9 others.  Returns (n1, n2, n_cols, seed, n_perm,
    Ks, read offsets, labels, cell ids, dense counts, kept count rows, their offsets per record, the generator)"""
    rng = np.random.default_rng(8)
    n1, n2, rest, seed, n_perm = 70, 91, 9, 77, 300
    n, n_cols = n1 + n2, n1 + n2 + rest
    Ks = np.array([2, 5, 70, 150], dtype=np.int32)
    lab, cb, off = [], [], [0]
    for K in Ks.tolist():
        m = 40 * K + 300
        lab.append(rng.integers(0, K + 1, m))
        cb.append((rng.integers(0, n_cols, m) ** 2) // n_cols)
        off.append(off[-1] + m)
    lab, cb, off = np.concatenate(lab).astype(np.int64), np.concatenate(cb).astype(np.int64), np.array(off, np.int64)
    rowbase = np.concatenate([[0], np.cumsum(Ks)])
    dense = np.zeros((int(Ks.sum()), n_cols), dtype=np.int64)
    for r, K in enumerate(Ks.tolist()):
        l, c = lab[off[r]:off[r + 1]], cb[off[r]:off[r + 1]]
        np.add.at(dense, (rowbase[r] + l[l < K], c[l < K]), 1)
    kept = [np.nonzero(dense[rowbase[r]:rowbase[r + 1], :n].sum(axis=1) > 0)[0] + rowbase[r] for r in range(len(Ks))]
    rows = np.concatenate(kept).astype(np.int64)
    roff = np.concatenate([[0], np.cumsum([len(k) for k in kept])]).astype(np.int64)
    assert len(kept[3]) > 128 and len(kept[2]) > 64
    return n1, n2, n_cols, seed, n_perm, Ks, off, lab, cb, dense, rows, roff, rng


# ---------------------------------------------------------------- the golden cases, loaded once
@functools.lru_cache(maxsize=None)
def fixture():
    from conftest import load_npz
    return load_npz("fixture_report.npz")


@functools.lru_cache(maxsize=None)
def fixture_case(c):
    return case(fixture(), c)


def fixture_cases():
    return [fixture_case(c) for c in case_ids(fixture())]


def case_params():
    return [pytest.param(c, id=fixture_case(c)["name"].replace("/", "-")) for c in case_ids(fixture())]


def cluster_texts(cs):
    """{cluster file name: text} of a golden case"""
    return {fn: text(fixture(), k) for fn, k in zip(cs["clu_files"], cs["clusters"])}


def write_case(cs, root, clusters=None):
    """the directory of a golden case with its own cluster files, or with the given {name: text}: (barcode_index.csv
    text, cluster file paths)"""
    from scape.apa_core import Parameters
    bc = text(fixture(), cs["barcode"])
    return bc, write_dir(str(root), cs["res"], cs["records"], bc, cluster_texts(cs) if clusters is None else clusters,
                         Parameters)


# ---------------------------------------------------------------- the definitions, restated
def column_ids(bc_csv):
    rows = list(csv.reader(io.StringIO(bc_csv)))
    ip = rows[0].index("index")
    return [int(r[ip]) for r in rows[1:]]


def cluster_rows(clu_csv):
    """(id, cluster text) of every row: index column by name, the first other column as written"""
    rows = list(csv.reader(io.StringIO(clu_csv)))
    ip = rows[0].index("index")
    other = [j for j in range(len(rows[0])) if j != ip][0]
    return [(int(r[ip]), r[other]) for r in rows[1:]]


def first_clusters(clu_csv):
    """cluster names in order of first appearance in the file"""
    order = []
    for _i, name in cluster_rows(clu_csv):
        if name != "" and name not in order:
            order.append(name)
    return order


def populations(bc_csv, clu_csv, id1, id2):
    """(columns of population 1, columns of population 2), ascending; clusters as text, a repeated id keeps its last
    row; without id2 population 2 is every other column that has a cluster"""
    last = {}
    for i, name in cluster_rows(clu_csv):
        last[i] = name
    col_clu = [last.get(i, "") for i in column_ids(bc_csv)]
    c1 = [j for j, x in enumerate(col_clu) if x == id1]
    c2 = [j for j, x in enumerate(col_clu) if (x == id2 if id2 is not None else x != "" and x != id1)]
    return c1, c2


def pa_info(rec, lab):
    """pa_info of the reference (utils.py:494-512), restated"""
    chrom, gene, utr, st_en, strand = rec["gene_info_str"].split(":")
    st, en = (int(v) for v in st_en.split("-"))
    a = int(rec["alpha_arr"][lab])
    loc = a + st if strand == "+" else en - a + 1
    return f"{chrom}:{loc}:{float(rec['beta_arr'][lab])!r}:{strand}:{lab + 1}:{gene}:{utr}"


def dense_counts(records, col_ids):
    """per record its [K, matrix column] read counts of the labels < K (np.add.at); a repeated id keeps its last
    column"""
    col_of = {int(i): j for j, i in enumerate(col_ids)}
    out = []
    for rec in records:
        K = int(rec["K"])
        m = np.zeros((K, len(col_ids)), dtype=np.int64)
        lab, cb = np.asarray(rec["label_arr"]), np.asarray(rec["cb_id_arr"])
        ok = lab < K
        np.add.at(m, (lab[ok], np.array([col_of[int(i)] for i in cb[ok]], dtype=np.int64)), 1)
        out.append(m)
    return out


def rec_rows_of(records, col_ids):
    """[(gene, [(pa_info, counts over the columns)])]: per record the labels < K with reads, in label order"""
    return [(rec["gene_info_str"], [(pa_info(rec, lb), m[lb]) for lb in range(len(m)) if m[lb].any()])
            for rec, m in zip(records, dense_counts(records, col_ids))]


def dense_of_body(mat_body, n_cols):
    """(pa_info of every row, integer matrix) that a dense body (rows '"pa_info","0.0","2",...') stands for"""
    rows = list(csv.reader(io.StringIO(mat_body)))
    dense = np.array([[int(float(v)) for v in r[1:]] for r in rows], dtype=np.int64).reshape(len(rows), n_cols)
    return [r[0] for r in rows], dense


# ---------------------------------------------------------------- the permutation tests: labellings and p-values
M64 = (1 << 64) - 1
G = 0x9E3779B97F4A7C15
RTOL = Fraction(1, 10 ** 12)


def mix(z):
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def key(seed, p, j):
    h = mix((mix((seed + G * p) & M64) + G * (j + 1)) & M64)
    return (h & ~0xFFFFFF & M64) | j


def members(seed, p, n1, n):
    """positions of population 1 under permutation p >= 1: the n1 smallest keys (a key's low 24 bits are its position)"""
    base = mix((seed + G * p) & M64)
    keys = sorted((mix((base + G * (j + 1)) & M64) & ~0xFFFFFF & M64) | j for j in range(n))
    return [k & 0xFFFFFF for k in keys[:n1]]


def bh(ps):
    """Benjamini-Hochberg on Fractions: adj_i = min(1, min over j with p_j >= p_i of m p_j / rank_j)"""
    m = len(ps)
    order = sorted(range(m), key=lambda i: ps[i])
    out, best = [None] * m, Fraction(1)
    for rank in range(m, 0, -1):
        i = order[rank - 1]
        best = min(best, ps[i] * m / rank)
        out[i] = best
    return out


def close(got_text, want):
    """a printed float is repr() of itself and within RTOL of the Fraction"""
    got = Fraction(float(got_text))
    assert repr(float(got_text)) == got_text
    return abs(got - want) <= RTOL * abs(want)


# ---------------------------------------------------------------- the permutation tests: directories
def golden_ident(bc, clu_text):
    """the first cluster (in order of first appearance) that has a column and leaves another column for the rest"""
    for name in first_clusters(clu_text):
        c1, c2 = populations(bc, clu_text, name, None)
        if c1 and c2:
            return name
    return None


def golden_perm_params():
    """every golden case and cluster file that gives two non-empty populations"""
    out = []
    for c in case_ids(fixture()):
        cs = fixture_case(c)
        bc = text(fixture(), cs["barcode"])
        for j, (fn, k) in enumerate(zip(cs["clu_files"], cs["clusters"])):
            if golden_ident(bc, text(fixture(), k)) is not None:
                out.append(pytest.param(c, j, id=f"{cs['name'].replace('/', '-')}-{fn}"))
    return out


SYN_SEED = 11
N_PLANTED = 4


@functools.lru_cache(maxsize=None)
def synthetic(gen_seed=SYN_SEED, n_cells=600):
    """about 40 records, K = 1..8 and one K = 63, 600 barcodes with scrambled ids: 230 cells of cluster A, 301 of B, 40
    of C, 29 without a cluster; 95 % of the (site, cell) counts are zero.  Records 0..3 have a planted usage shift in A
    (many reads, the first site ten times as likely there), record 4 a row with reads only in cells of no cluster,
    record 5 reads only in A, record 6 K = 1; some reads carry the label K (no site)."""
    rng = np.random.default_rng(gen_seed)
    ids = (np.arange(n_cells) * 7919 + 13) % 100003                      # distinct, scrambled
    clu = np.array(["A"] * 230 + ["B"] * 301 + ["C"] * 40 + [""] * (n_cells - 571), dtype=object)
    clu = clu[rng.permutation(n_cells)]
    bc = "CB,index\n" + "".join(f"CELL{j:04d}-1,{i}\n" for j, i in enumerate(ids.tolist()))
    order = rng.permutation(n_cells)
    clu_text = "index,group\n" + "".join(f"{ids[j]},{clu[j]}\n" for j in order.tolist() if not (clu[j] == "" and j % 2))
    is_a, no_clu = clu == "A", clu == ""
    records = []
    Ks = [2, 3, 4, 5, 3, 4, 1] + [int(k) for k in rng.integers(1, 9, 32)] + [63]
    for r, K in enumerate(Ks):
        planted = r < N_PLANTED
        dens = np.full((K, n_cells), 0.30 if planted else 0.05)
        if planted:
            dens[0, ~is_a] = 0.03
        if r == 4:
            dens[1, :] = 0.0
            dens[1, no_clu] = 0.5
        if r == 5:
            dens[:, ~is_a] = 0.0
        cnt = (rng.random((K, n_cells)) < dens) * rng.integers(1, 4, (K, n_cells))
        lab, cell = np.nonzero(cnt)
        rep = cnt[lab, cell]
        lab, cell = np.repeat(lab, rep), np.repeat(cell, rep)
        extra = rng.integers(0, n_cells, 5)                              # reads of no site
        lab, cell = np.concatenate([lab, np.full(5, K)]), np.concatenate([cell, extra])
        mixo = rng.permutation(len(lab))
        strand = "+-"[r % 2]
        records.append(dict(gene_info_str=f"{1 + r % 5}:GENE{r}:{1 + r % 3}:{1000 * r + 100}-{1000 * r + 900}:{strand}",
                            K=K, alpha_arr=np.sort(rng.choice(np.arange(5, 790), K, replace=False)),
                            beta_arr=rng.choice([5.0, 7.5, 10.0, 32.5], K), label_arr=lab[mixo].astype(np.int64),
                            cb_id_arr=ids[cell[mixo]].astype(np.int64)))
    return records, bc, clu_text


def write_synthetic(root, n_rec=None):
    """the synthetic directory (its first n_rec records): the path of its cluster file"""
    from scape.apa_core import Parameters
    records, bc, clu_text = synthetic()
    return write_dir(str(root), "res.gene.pkl", records[:n_rec], bc, {"syn_groups.csv": clu_text}, Parameters)[0]


def small_dir(root, n_cells, n_a, gen_seed):
    """8 records on n_cells barcodes, the first n_a of them in cluster A, the others in B: (cluster file path, its
    text, barcode_index.csv text, records, column ids)"""
    from scape.apa_core import Parameters
    rng = np.random.default_rng(gen_seed)
    ids = np.arange(n_cells) * 3 + 2
    bc = "CB,index\n" + "".join(f"S{j}-1,{i}\n" for j, i in enumerate(ids.tolist()))
    clu_text = "index,group\n" + "".join(f"{i},{'A' if j < n_a else 'B'}\n" for j, i in enumerate(ids.tolist()))
    records = []
    for r in range(8):
        K = 2 + r % 4
        n = 400
        records.append(dict(gene_info_str=f"2:SG{r}:1:{500 * r + 1}-{500 * r + 400}:+", K=K,
                            alpha_arr=np.arange(K) * 40 + 10, beta_arr=np.full(K, 10.0),
                            label_arr=rng.integers(0, K, n).astype(np.int64),
                            cb_id_arr=ids[rng.integers(0, n_cells, n)].astype(np.int64)))
    path = write_dir(str(root), "res.utr.pkl", records, bc, {"small.csv": clu_text}, Parameters)[0]
    return path, clu_text, bc, records, ids.tolist()


# ---------------------------------------------------------------- a wide stream
def wide_stream(seed=5):
    """3,100 barcodes (scrambled ids with gaps, one id on two rows), records with K > 63, counts in the hundreds,
    reads over every column, and records whose reads are all in the uniform component (label >= K): (records,
    barcode_index.csv text, pa_info of the matrix rows, the matrix from dense_counts)"""
    rng = np.random.default_rng(seed)
    n_cols = 3100
    ids = rng.permutation(np.arange(7, 7 + 3 * n_cols, 3)).astype(np.int64)
    ids[40] = ids[2000]                           # a repeated id keeps its last row: column 2001 gets its reads
    bc = "CB,index\n" + "".join(f"W{j:05d}-1,{ids[j]}\n" for j in range(n_cols))
    used = np.array(sorted(set(ids.tolist())), dtype=np.int64)
    # (K, reads, how many distinct cells, labels: "mixed" = 0..K with some >= K, "uniform" = all >= K)
    specs = [(70, 25000, n_cols, "mixed"), (3, 30000, 40, "mixed"), (2, 500, 300, "uniform"),
             (1, 16000, n_cols, "mixed"), (64, 4000, 900, "mixed"), (5, 0, 0, "mixed"), (1, 80, 20, "uniform")]
    specs += [(int(rng.integers(1, 9)), int(rng.integers(50, 3000)), int(rng.integers(1, n_cols)), "mixed")
              for _ in range(12)]
    recs = []
    for r, (K, n, n_cells, kind) in enumerate(specs):
        cells = rng.choice(used, size=min(max(n_cells, 1), len(used)), replace=False)
        cb = cells[rng.integers(0, len(cells), n)] if n else np.zeros(0, np.int64)
        lab = rng.integers(K, K + 3, n) if kind == "uniform" else rng.integers(0, K + 1, n)
        if K == 1 and n_cells == n_cols:
            cb[:len(used)] = used                 # a read below K in every column that owns an id, the last one included
            lab[:len(used)] = 0
        alpha = np.sort(rng.choice(np.arange(50, 5000), K, replace=False)).astype(np.int64)
        beta = rng.choice([5.0, 7.5, 30.0], K)
        gene_info = f"{1 + r % 3}:WIDE{r:03d}:{1 + r % 2}:{10000 * r + 1}-{10000 * r + 9000}:{'+-'[r % 2]}"
        recs.append(dict(gene_info_str=gene_info, K=K, alpha_arr=alpha, beta_arr=beta, label_arr=lab.astype(np.int64),
                         cb_id_arr=cb.astype(np.int64)))
    rows = [row for _gene, rec_rows in rec_rows_of(recs, ids.tolist()) for row in rec_rows]
    dense = np.array([m for _pa, m in rows], dtype=np.int64).reshape(len(rows), n_cols)
    return recs, bc, [pa for pa, _m in rows], dense
