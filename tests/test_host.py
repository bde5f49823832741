"""CPU tests of the product's host logic (no GPU compute): chunk reader, binning, coverage,
restart sampling stream, CLI error behaviour, and that libscape_hip.so loads and exports
every symbol include/scape_hip.h declares."""
import os
import pickle
import re

import numpy as np
import pandas as pd
import pytest

from conftest import ROOT, load_npz, trace_params, utr_df


# ---------------------------------------------------------------- C-ABI surface
def test_library_exports_every_declared_symbol():
    from scape_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "scape_hip.h")).read()
    declared = set(re.findall(r"\b(scape_hip_[a-z_0-9]+)\s*\(", hdr))
    assert declared, "no declarations parsed"
    lib = _lib.load_library()
    for name in declared:
        assert hasattr(lib, name), f"libscape_hip.so lacks {name}"
    assert declared == set(_lib.SIGNATURES), "ctypes table and header disagree"
    assert lib.scape_hip_abi_version() == 4


def test_host_library_exports_every_declared_symbol():
    from scape_amd import _hostlib
    hdr = open(os.path.join(ROOT, "include", "scape_host.h")).read()
    declared = set(re.findall(r"\b(scape_host_[a-z_0-9]+)\s*\(", hdr))
    assert declared, "no declarations parsed"
    lib = _hostlib.load_library()
    for name in declared:
        assert hasattr(lib, name), f"libscape_host.so lacks {name}"
    assert declared == set(_hostlib.SIGNATURES), "ctypes table and header disagree"


def test_no_product_import_of_oracle():
    """The product path must never route through the oracle."""
    for root, _dirs, files in os.walk(os.path.join(ROOT, "scape_amd")):
        for fn in files:
            if fn.endswith((".py", ".hip", ".h", ".cpp")):
                src = open(os.path.join(root, fn)).read()
                assert "oracle" not in src.replace("# oracle", ""), f"{fn} mentions the oracle"
    for fn in os.listdir(os.path.join(ROOT, "scape")):
        if fn.endswith(".py"):
            assert "oracle" not in open(os.path.join(ROOT, "scape", fn)).read()


# ---------------------------------------------------------------- chunk reader
def _chunk_bytes(utrs):
    out = b""
    for gene, df in utrs:
        out += pickle.dumps((gene, df), protocol=4)
    return out


def test_safe_pickle_reads_prepare_input_layout():
    from scape_amd import safe_pickle
    rng = np.random.default_rng(3)
    utrs = []
    for i in range(3):
        n = 50 + 10 * i
        df = pd.DataFrame({"x": rng.integers(0, 1500, n), "l": rng.integers(31, 133, n),
                           "r": np.full(n, np.nan), "pa": np.where(rng.random(n) < 0.1, 800.0, np.nan),
                           "cb_id": rng.integers(0, 9999, n), "read_id": np.arange(n),
                           "junction": rng.integers(0, 2, n), "seg1_en": np.full(n, np.nan),
                           "seg2_en": rng.random(n)})
        utrs.append((f"chr1:G{i}:1:10-2000:+", df))
    got = safe_pickle.load_all(_chunk_bytes(utrs))
    assert len(got) == 3
    for (g0, d0), (g1, d1) in zip(utrs, got):
        assert g0 == g1 and list(d0.columns) == list(d1.columns)
        for c in d0.columns:
            assert np.array_equal(d0[c].values, d1[c].values, equal_nan=True)
            assert d0[c].dtype == d1[c].dtype


def test_safe_pickle_refuses_code_execution(tmp_path):
    from scape_amd import safe_pickle

    class Evil:
        def __reduce__(self):
            return (os.system, ("touch " + str(tmp_path / "pwned"),))
    data = pickle.dumps(("g", Evil()))
    with pytest.raises(safe_pickle.UnsafePickleError):
        safe_pickle.load_all(data)
    assert not (tmp_path / "pwned").exists()


def test_parameters_pickles_under_reference_class_path():
    from scape.apa_core import Parameters
    from scape_amd import safe_pickle
    p = Parameters(title="Final Result", alpha_arr=np.array([623]), beta_arr=np.array([10.0]),
                   ws=np.array([0.9, 0.1]), L=2000, cb_id_arr=np.arange(3), readID_arr=np.arange(3))
    p.bic = np.float64(1.5)
    p.lb_arr = [np.float64(-3.0), np.float64(-2.0)]
    p.label_arr = np.array([0, 0, 1])
    p.gene_info_str = "chr1:G:1:1-2:+"
    blob = pickle.dumps(p)
    assert b"scape.apa_core" in blob and b"Parameters" in blob
    q = pickle.loads(blob)
    assert type(q) is Parameters and q.K == 1 and "K=1" in str(q)
    s = safe_pickle.load_all(blob)[0]
    assert s.gene_info_str == p.gene_info_str and np.array_equal(s.label_arr, p.label_arr)
    assert [float(v) for v in s.lb_arr] == [-3.0, -2.0]


# ---------------------------------------------------------------- binning / coverage / grids
def test_binning_matches_oracle_on_random_reads(oracle):
    from scape_amd.host import bin_reads
    rng = np.random.default_rng(5)
    for case in range(6):
        n = int(rng.integers(1, 3000))
        x = rng.integers(0, 2500, n).astype(float)
        l = rng.integers(31, 133, n).astype(float)
        r = np.full(n, np.nan)
        pa = np.full(n, np.nan)
        if case % 2:
            m = rng.random(n) < 0.2
            pa[m] = rng.integers(100, 2600, m.sum())
        if case >= 3:
            m = rng.random(n) < 0.3
            r[m] = rng.integers(1, 140, m.sum())
        got = bin_reads(x, l, r, pa)
        want = oracle.bin_reads(x, l, r, pa)
        for g, w in zip(got, want):
            assert np.array_equal(g, w, equal_nan=True)


def test_prepare_utr_matches_reference_trace():
    from scape_amd.host import coverage_profile, prepare_utr
    for name in ("synA", "synB", "chr19"):
        f = load_npz(f"trace_{name}.npz")
        p = trace_params(f)
        for i in range(int(f["n_utr"])):
            gene, df = utr_df(f, i)
            q = prepare_utr(df, gene_info_str=gene, **p)
            for k, v in (("x", q.x), ("l", q.l), ("r", q.r), ("pa", q.pa)):
                assert np.array_equal(v, f[f"u{i}_bin_{k}"], equal_nan=True)
            assert np.array_equal(q.cnt, f[f"u{i}_bin_cnt"]) and np.array_equal(q.idx, f[f"u{i}_bin_idx"])
            assert np.array_equal(q.theta, f[f"u{i}_all_theta"]) and np.array_equal(q.betas, f[f"u{i}_betas"])
            assert q.L == int(f[f"u{i}_L"]) and q.min_theta == float(f[f"u{i}_min_theta"])
            assert q.unif_ll == float(f[f"u{i}_unif_ll"])
            _, ys = coverage_profile(q.x, q.l, q.cnt, q.L, q.p["beta_step"])
            assert np.array_equal(ys, f[f"u{i}_cov_y"])         # bit-equal to ker_smooth's loops


def test_sampler_consumes_reference_stream():
    """init_para + gen_k_arr draws equal the reference's, call for call (first sweep of each UTR)."""
    from scape_amd.host import Sampler, prepare_utr
    for name in ("synA", "synB", "chr17"):
        f = load_npz(f"trace_{name}.npz")
        p = trace_params(f)
        for i in range(int(f["n_utr"])):
            gene, df = utr_df(f, i)
            q = prepare_utr(df, gene_info_str=gene, **p)
            rs = np.random.RandomState(0)
            st = ("MT19937", f[f"u{i}_rng_keys"], int(f[f"u{i}_rng_pos"]), 0, 0.0)
            rs.set_state(st)
            smp, c = Sampler(rs), 0
            for K in range(p["n_max_apa"], p["n_min_apa"] - 1, -1):
                for _ in range(10):
                    a, b, w, ka = smp.init_job(q, K)
                    assert np.array_equal(q.theta[a], f[f"u{i}_call_a0"][c, :K])
                    assert np.array_equal(q.betas[b], f[f"u{i}_call_b0"][c, :K])
                    assert np.array_equal(w, f[f"u{i}_call_w0"][c, :K + 1])
                    assert np.array_equal(ka, f[f"u{i}_call_k_arr"][c].astype(int))
                    c += 1


def test_native_sampler_equals_numpy_stream():
    """libscape_host.so draws the numbers numpy's legacy RandomState draws (both init_para branches:
    K <= #peaks -> choice with p, K > #peaks -> permutation(L)), and leaves the same generator state."""
    from scape_amd.host import FastSampler, Sampler, prepare_utr
    from scape_amd.synth import synth_chunk
    from scape_amd import _hostlib
    lib = _hostlib.load_library()
    st = np.zeros(625, dtype=np.uint32)
    for seed in (0, 1, 12345, 2 ** 32 - 1):
        lib.scape_host_mt_seed(seed, _hostlib.ptr(st, _hostlib.P_u32))
        ref = np.random.RandomState(seed)
        g = ref.get_state()
        assert np.array_equal(st[:624], g[1]) and st[624] == g[2]
        assert [lib.scape_host_mt_double(_hostlib.ptr(st, _hostlib.P_u32)) for _ in range(700)] == list(ref.random_sample(700))
    preps = [prepare_utr(df, g, n_max_apa=12, n_min_apa=1) for g, df in synth_chunk(10, 600, base_seed=5)]
    f = load_npz("trace_chr17.npz")
    preps.append(prepare_utr(utr_df(f, 0)[1], gene_info_str="chr17", **trace_params(f)))
    for u, q in enumerate(preps):
        r1, r2 = np.random.RandomState(100 + u), np.random.RandomState(100 + u)
        s1, s2 = Sampler(r1), FastSampler(r2)
        for K in list(range(14, 0, -1)) + [25]:
            for _ in range(3):
                for x, y in zip(s1.init_job(q, K), s2.init_job(q, K)):
                    assert np.array_equal(x, y) and x.dtype == y.dtype, (u, K)
            assert np.array_equal(s1.init_ws(K - 1, 0.15), s2.init_ws(K - 1, 0.15))
            assert np.array_equal(s1.k_arr(K - 1), s2.k_arr(K - 1))
        g1, g2 = r1.get_state(), s2.rs.get_state()
        assert np.array_equal(g1[1], g2[1]) and g1[2] == g2[2]
    # what numpy refuses, the native path declines and numpy then raises as usual
    q = preps[0]
    with pytest.raises(ValueError):
        FastSampler(np.random.RandomState(1)).init_job(q, q.L + len(q.peaks) + 5)


def test_native_sweep_equals_job_by_job_draws():
    """FastSampler.sweep (one native call per K sweep, the reference-stream fast path) == init_job per restart."""
    from scape_amd.host import FastSampler, Sampler, prepare_utr
    from scape_amd.synth import synth_chunk
    for u, (g, df) in enumerate(synth_chunk(6, 500, base_seed=21)):
        q = prepare_utr(df, g, n_max_apa=12, n_min_apa=1)
        r1, r2 = np.random.RandomState(9 + u), np.random.RandomState(9 + u)
        s1, s2 = Sampler(r1), FastSampler(r2)
        for n_max, n_min in ((12, 1), (5, 2), (14, 12), (3, 3)):
            jk, a, b, w, ka = s2.sweep(q, n_max, n_min)
            i = 0
            for K in range(n_max, n_min - 1, -1):
                for _ in range(10):
                    ea, eb, ew, eka = s1.init_job(q, K)
                    assert jk[i] == K and np.array_equal(a[i, :K], ea) and np.array_equal(b[i, :K], eb)
                    assert np.array_equal(w[i, :K + 1], ew) and np.array_equal(ka[i], eka)
                    assert not a[i, K:].any() and not w[i, K + 1:].any()
                    i += 1
            assert i == len(jk)
        g1, g2 = r1.get_state(), s2.rs.get_state()
        assert np.array_equal(g1[1], g2[1]) and g1[2] == g2[2]


def test_native_sweep_many_equals_single_sweeps():
    """The threaded batch call for the heads of several streams draws what the per-stream calls draw."""
    from scape_amd.host import FastSampler, prepare_utr
    from scape_amd.synth import synth_chunk
    preps = [prepare_utr(df, g, n_max_apa=10, n_min_apa=1) for g, df in synth_chunk(7, 400, base_seed=31)]
    one = [FastSampler(np.random.RandomState(40 + i)) for i in range(7)]
    many = [FastSampler(np.random.RandomState(40 + i)) for i in range(7)]
    a = [s.sweep(q, 10 - i % 3, 1 + i % 2) for i, (s, q) in enumerate(zip(one, preps))]
    b = FastSampler.sweep_many([(s, q, 10 - i % 3, 1 + i % 2) for i, (s, q) in enumerate(zip(many, preps))], n_threads=3)
    for x, y in zip(a, b):
        for u, v in zip(x, y):
            assert np.array_equal(u, v)
    for s, t in zip(one, many):
        assert np.array_equal(s.state, t.state)
    with pytest.raises(ValueError):
        FastSampler.sweep_many([(one[0], preps[0], 3, 1), (one[0], preps[1], 3, 1)])


def test_native_plan_equals_python_plan():
    """Engine.plan (scape_host_plan, threaded) == Engine.plan_python (numpy RandomState), table for table,
    for mixed K ranges and seeds at the 32-bit edge."""
    from scape_amd.engine import Engine
    from scape_amd.host import prepare_utr
    from scape_amd.synth import synth_chunk
    chunk = synth_chunk(12, 500, base_seed=9)
    preps = [prepare_utr(df, g, n_max_apa=(10 if i % 3 else 4), n_min_apa=(1 if i % 2 else 2))
             for i, (g, df) in enumerate(chunk)]
    seeds = [(2 ** 32 - 4 + i) % 2 ** 32 for i in range(len(preps))]
    P1 = Engine.plan_python(preps, seeds)
    for nt in (1, 3):
        P2 = Engine.plan(preps, seeds, n_threads=nt)
        for k in ("ju", "jk", "jf", "a", "b", "w", "ka"):
            assert np.array_equal(getattr(P1["main"], k), getattr(P2["main"], k)), k
        for k in ("spans", "states", "prune_w", "prune_ka", "prune_states"):
            assert np.array_equal(P1[k], P2[k]), k


def test_snap_to_grid_ties_go_up(oracle):
    from scape_amd.host import snap_to_grid
    grid = np.arange(31, 2000, 9) + 0.0
    vals = np.array([-5.0, 31.0, 35.5, 35.4, 35.6, 40.0, 1999.0, 5000.0, 44.5])
    assert np.array_equal(snap_to_grid(grid, vals), oracle.nearest_on_grid(grid, vals)[0])


def test_k_arr_rules():
    from scape_amd.host import Sampler
    s = Sampler(np.random.RandomState(4))
    st = s.rs.get_state()[2]
    assert np.array_equal(s.k_arr(1), np.zeros(50)) and np.array_equal(s.k_arr(0), np.zeros(50))
    assert s.rs.get_state()[2] == st                       # K <= 1 draws nothing (apa_core.py:671-672)
    ka = s.k_arr(4)
    for t0 in range(0, 48, 4):
        assert sorted(ka[t0:t0 + 4]) == [0, 1, 2, 3]


# ---------------------------------------------------------------- pre-binned columnar chunks
def test_binned_chunk_gives_identical_preps_and_detects_staleness(tmp_path):
    from scape_amd import binned
    from scape_amd.apa_core import load_preps
    from scape_amd.synth import synth_chunk
    f = load_npz("fixture_chr17.npz")
    utrs = [utr_df(f, i) for i in range(int(f["n_utr"]))] + synth_chunk(5, 400, base_seed=8, pa_rate=0.05)
    rng = np.random.default_rng(1)
    full = []
    for g, df in utrs:                                  # the three columns merge_pa reads besides read_id
        df = df.copy()
        n = len(df)
        df["junction"] = (rng.random(n) < 0.1).astype(np.int64)
        df["seg1_en"] = np.where(df["junction"] == 1, rng.integers(1000, 9000, n).astype(float), np.nan)
        df["seg2_en"] = np.where(df["junction"] == 1, rng.integers(1000, 9000, n).astype(float), np.nan)
        full.append((g, df))
    path = str(tmp_path / "c.100.1.1.input.pkl")
    with open(path, "wb") as fh:
        for it in full:
            pickle.dump(it, fh)
    kw = dict(n_max_apa=4, n_min_apa=1)
    want = load_preps(path, kw)                         # no binned file yet: decodes the pickle
    bp = binned.prebin_chunk(path)
    assert bp == str(tmp_path / "c.100.1.1.binned.npz") and binned.is_current(bp, path)
    with np.load(bp, allow_pickle=False) as z:          # plain arrays only
        assert int(z["version"]) == binned.VERSION and len(z["gene_info"]) == len(full)
    got = load_preps(path, kw)
    assert len(got) == len(want)
    for a, b in zip(got, want):
        for k in ("x", "l", "r", "pa", "cnt", "idx", "cb_id", "read_id", "theta", "betas", "peaks", "peak_w", "s_dis"):
            assert np.array_equal(getattr(a, k), getattr(b, k), equal_nan=True), k
        assert (a.gene_info_str, a.L, a.min_theta, a.unif_ll, a.p) == (b.gene_info_str, b.L, b.min_theta, b.unif_ll, b.p)
    for (g, b, cols), (g0, df) in zip(binned.read_binned(bp), full):
        assert g == g0 and np.array_equal(cols["junction"], df["junction"])
        assert np.array_equal(cols["seg1_en"], df["seg1_en"], equal_nan=True)
        assert np.array_equal(cols["seg2_en"], df["seg2_en"], equal_nan=True)
    with open(path, "ab") as fh:                        # the chunk changes -> the binned copy is stale
        pickle.dump(full[0], fh)
    assert not binned.is_current(bp, path)
    assert len(load_preps(path, kw)) == len(full) + 1


# ---------------------------------------------------------------- CLI behaviour (reference apa_core.py:78-132)
def test_cli_error_behaviour(tmp_path):
    from click.testing import CliRunner
    from scape.cli import cli
    out = tmp_path / "out"
    out.mkdir()
    run = CliRunner()
    # parameters.toml must exist (assert at apa_core.py:85)
    r = run.invoke(cli, ["infer_pa", "--pkl_input_file", str(tmp_path / "a.100.1.1.input.pkl"), "--output_dir", str(out)])
    assert isinstance(r.exception, AssertionError)
    (out / "parameters.toml").write_text("n_max_apa = 3\noutput_dir = \"x\"\n")
    r = run.invoke(cli, ["infer_pa", "--pkl_input_file", str(tmp_path / "missing.input.pkl"), "--output_dir", str(out)])
    assert "does not exists" in str(r.exception)
    tmp_in = tmp_path / "b.tmp.100.1.1.input.pkl"
    tmp_in.write_bytes(b"")
    r = run.invoke(cli, ["infer_pa", "--pkl_input_file", str(tmp_in), "--output_dir", str(out)])
    assert "incomplete" in str(r.exception)
    r = run.invoke(cli, ["infer_pa", "--pkl_input_file", str(tmp_in), "--output_dir", str(tmp_path / "nope")])
    assert isinstance(r.exception, AssertionError)


def test_infer_all_resume_skips_finished_chunks(tmp_path, monkeypatch):
    from scape_amd import apa_core
    d = tmp_path / "o"
    (d / "pkl_input").mkdir(parents=True)
    (d / "pkl_output").mkdir()
    for i in range(4):
        (d / "pkl_input" / f"c.100.4.{i + 1}.input.pkl").write_bytes(b"x")
    (d / "pkl_input" / "c.tmp.100.4.9.input.pkl").write_bytes(b"x")          # incomplete chunk: never processed
    (d / "pkl_output" / "c.100.4.2.res.pkl").write_bytes(b"y")                 # finished
    (d / "pkl_output" / "c.100.4.3.res.pkl").write_bytes(b"y")                 # older than its chunk -> redo
    os.utime(d / "pkl_output" / "c.100.4.3.res.pkl", (1, 1))
    seen = []
    monkeypatch.setattr(apa_core, "infer_files", lambda files, out, **kw: seen.append([os.path.basename(f) for f in files]))
    apa_core.infer_all(str(d), gpus=1, resume=True, n_max_apa=3)
    assert seen == [["c.100.4.1.input.pkl", "c.100.4.3.input.pkl", "c.100.4.4.input.pkl"]]
    apa_core.infer_all(str(d), gpus=1, n_max_apa=3)
    assert len(seen[1]) == 4


def test_wave_split_respects_budget(monkeypatch):
    from scape_amd import engine

    class Q:
        def __init__(self, N, T):
            self.N, self.T, self.betas, self.gene_info_str = N, T, np.zeros(13), "g"
    eng = engine.Engine.__new__(engine.Engine)
    eng.mem_fraction = 1.0
    preps = [Q(100, 218), Q(1000, 300), Q(50, 218), Q(1200, 400)]
    sizes = [engine.Engine.utr_bytes(q) for q in preps]
    monkeypatch.setattr(engine.Engine, "_budget", lambda self: sizes[1] + sizes[2])
    waves = eng.waves(preps[:3])
    assert waves == [[0], [1, 2]]
    with pytest.raises(Exception):
        eng.waves(preps)


# ---------------------------------------------------------------- exact-stream driver (host logic only, no GPU)
class _FakeBatch:
    """Stands in for HipBatch.em_packed in the stream-driver tests: every job's "fit" is a pure function of that job's
    own table row (as on the GPU, where a job's bits do not depend on what shares its call), made up so that sweeps end
    clean, pruned to various K' or at K = n_max (re-run).  For Engine.process it also carries the rest of what that calls:
    the lb rows of the last call stay fetchable, labels are a pure function of the model they are asked for."""
    calls = 0

    def __init__(self, preps=()):
        self.bin_off = np.zeros(len(preps) + 1, dtype=np.int64)
        np.cumsum([q.N for q in preps], out=self.bin_off[1:])
        self.seen = []                                     # (job tables, result arrays) of every call, in call order

    def build(self):
        pass

    def timing(self, which):
        return 0.0, 0

    def em_counters(self):
        return 0, 0, 0

    def em_fetch_lb(self, job_idx):
        return self.seen[-1][1][5][np.asarray(job_idx, dtype=np.int64)].copy()

    @staticmethod
    def fit_at(pj, out, i, lb_row=None):
        from scape_amd.engine import HipBatch
        return HipBatch.fit_at(pj, out, i, lb_row)

    @staticmethod
    def label_rule(n, K, a, b):
        return ((np.arange(n) * (1 + int(np.sum(a[:K])) + int(np.sum(b[:K])))) % (K + 1)).astype(np.int32)

    def labels_packed(self, su, sk, a, b, w):
        flat = np.full(int(self.bin_off[-1]), -1, dtype=np.int32)
        for i, u in enumerate(su):
            lo, hi = int(self.bin_off[u]), int(self.bin_off[u + 1])
            flat[lo:hi] = self.label_rule(hi - lo, int(sk[i]), a[i], b[i])
        return flat

    def em_packed(self, pj, reuse_buffers=False, want_lb=True):
        import zlib
        from scape_amd.host import N_ROUND
        type(self).calls += 1
        n, kmax = len(pj), pj.kmax
        ao, bo, wo = pj.a.copy(), pj.b.copy(), np.zeros_like(pj.w)
        bic, nlb, lb = np.zeros(n), np.full(n, 3, np.int32), np.zeros((n, N_ROUND))
        for i in range(n):
            K = int(pj.jk[i])
            h = zlib.crc32(pj.a[i, :K].tobytes() + pj.b[i, :K].tobytes() + pj.w[i, :K + 1].tobytes() + pj.ka[i].tobytes() +
                           bytes([K, int(pj.jf[i])]))          # (the row up to K: the padding width depends on the call)
            r = np.random.RandomState(h)
            w = r.dirichlet(np.full(K + 1, 0.6))
            w[0] += 0.06                                   # (one component always stays: rm_component needs K' >= 1)
            w /= w.sum()
            wo[i, :K + 1] = w
            bic[i] = 2.0 * abs(K - 2.3) + 30.0 * r.random_sample()
            lb[i, :3] = r.random_sample(3)
        self.seen.append((pj, (ao, bo, wo, bic, nlb, lb)))
        return ao, bo, wo, bic, nlb, (lb if want_lb else None)


def _stream_preps(n, base):
    from scape_amd.host import prepare_utr
    from scape_amd.synth import synth_utr
    return [prepare_utr(df, gene_info_str=g, n_max_apa=3, n_min_apa=1)
            for g, df, _ in (synth_utr(i, 150, k_cap=3, base_seed=base) for i in range(n))]


def _drive(chunks, depth, preds=None, seed=7):
    from scape_amd.engine import Engine, _Sweep
    from scape_amd.host import FastSampler
    streams, all_sw = [], []
    for ci, preps in enumerate(chunks):
        smp = FastSampler(np.random.RandomState(seed + ci))
        sws = [_Sweep(u, q, smp, True) for u, q in enumerate(preps)]
        if preds is not None:
            for sw, p in zip(sws, preds[ci]):
                sw.pred = p
        streams.append((smp, sws))
        all_sw.append(sws)
    deferred = []
    Engine._drive_streams(_FakeBatch(), streams, deferred, depth=depth)
    Engine._finish_deferred(_FakeBatch(), deferred)
    sig = [[(sw.best.K, sw.best.a_idx.tobytes(), sw.best.b_idx.tobytes(), sw.best.ws.tobytes(), sw.best.bic, sw.n_jobs)
            for sw in sws] for sws in all_sw]
    return sig, [smp.state.copy() for smp, _ in streams]


def test_stream_driver_results_do_not_depend_on_depth_or_predictions(monkeypatch):
    """Engine._drive_streams: several UTRs of a stream per EM call, drawn from the state their predecessors' PREDICTED
    outcome leaves.  Whatever the predictions say - right, wrong, absent, 'stop' - every UTR must get the fit, the job
    count and the generator state of the strictly serial loop (depth 1); also with the look-ahead draws on and off and in the
    two-halves schedule of many streams."""
    from scape_amd.engine import Engine
    chunks = [_stream_preps(14, 9100), _stream_preps(9, 9200), _stream_preps(5, 9300)]
    ref, ref_states = _drive(chunks, 1)
    outcomes = {(k, nj) for ch in ref for (k, *_rest, nj) in ch}
    assert len({nj for _k, nj in outcomes}) >= 3, outcomes          # clean (30 jobs), pruned (+1) and re-run sweeps all occur
    rs = np.random.RandomState(3)
    true_pred = [[("clean" if nj == 30 else ("prune", k) if nj == 31 else "stop") for (k, *_r, nj) in ch] for ch in ref]
    for trial in range(6):
        if trial == 0:
            preds = None                                              # no predictor: followers assume a clean end
        elif trial == 1:
            preds = true_pred                                         # an oracle predictor: (almost) nothing discarded
        else:                                                         # right, wrong and missing predictions mixed
            preds = [[p if rs.random_sample() < 0.6 else rs.choice(["clean", "stop", None, "p1", "p2"]) for p in ch]
                     for ch in true_pred]
            preds = [[("prune", int(p[1])) if isinstance(p, str) and p.startswith("p") else p for p in ch] for ch in preds]
        for depth, ahead, pp in ((3, True, 32), (8, True, 32), (8, False, 32), (4, True, 2)):
            monkeypatch.setattr(Engine, "draw_ahead", ahead)
            monkeypatch.setattr(Engine, "pingpong_min_streams", pp)
            before = dict(Engine.spec_stats)
            got, states = _drive(chunks, depth, preds)
            assert got == ref, (trial, depth, ahead, pp)
            for a, b in zip(states, ref_states):
                assert np.array_equal(a, b), (trial, depth, ahead, pp)
            if trial == 1 and pp == 32:
                assert Engine.spec_stats["utrs_kept"] - before["utrs_kept"] >= sum(len(c) for c in chunks)


def test_prediction_pass_failure_is_not_a_stream_failure():
    """Engine._predict_outcomes fits the wave from OTHER seeds; when that fit prunes every component of some UTR
    (the reference's IndexError, apa_core.py:838-839) or the library refuses its job tables, the real stream must go
    on without predictions and the measurement fields of the real sweeps must stay as they were."""
    from scape_amd import _lib
    from scape_amd.engine import Engine, _Sweep
    from scape_amd.host import FastSampler
    preps = _stream_preps(4, 9400)
    for exc in (IndexError("index 0 is out of bounds for axis 0 with size 0"), _lib.ScapeHipError("job table refused")):
        eng = Engine.__new__(Engine)              # no GPU: only the prediction wrapper is exercised
        eng.last_main_em_ms, eng.last_main_counters = 12.5, (1, 2, 3)

        def boom(*a, _e=exc, **k):
            eng.last_main_em_ms, eng.last_host_ms = -1.0, dict(x=1)      # what a half-finished process() leaves behind
            raise _e
        eng.plan = lambda preps, seeds: None
        eng.process = boom
        smp = FastSampler(np.random.RandomState(1))
        sweeps = [_Sweep(u, q, smp, True) for u, q in enumerate(preps)]
        for sw in sweeps:
            sw.pred = "clean"
        eng._predict_outcomes(None, preps, sweeps, True)
        assert all(sw.pred is None for sw in sweeps)
        assert eng.last_main_em_ms == 12.5 and eng.last_main_counters == (1, 2, 3)
        assert not hasattr(eng, "last_host_ms")


def _fit_sig(f):
    return (f.K, f.a_idx.tobytes(), f.b_idx.tobytes(), f.ws.tobytes(), np.float64(f.bic).tobytes(), f.lb.tobytes())


def test_process_equals_the_sweep_state_machine():
    """Engine.process (tables of a whole batch drawn up front, vectorised selection) and the _Sweep state machine are
    the same function of (UTR, seed): K, a_idx, b_idx, ws, bic and lb equal as bytes, and equal job counts, with the
    re-run rule on and off.  process's labels are those of the fit it returns."""
    from scape_amd.engine import Engine, _Sweep
    from scape_amd.host import FastSampler, N_TRIAL, prepare_utr
    from scape_amd.synth import synth_utr
    classes = dict(clean=0, pruned=0, rerun=0)
    for base, n_max, n_min in ((9100, 3, 1), (9500, 4, 2), (9700, 5, 1)):
        preps = [prepare_utr(df, gene_info_str=g, n_max_apa=n_max, n_min_apa=n_min)
                 for g, df, _ in (synth_utr(i, 150, k_cap=3, base_seed=base) for i in range(40))]
        seeds = [(2 ** 32 - 7 + 3 * i) % 2 ** 32 for i in range(len(preps))]
        n_sweep = (n_max - n_min + 1) * N_TRIAL
        for re_run in (True, False):
            eng = Engine.__new__(Engine)
            eng.sweep_lock = None
            batch = _FakeBatch(preps)
            got = eng.process(batch, preps, Engine.plan(preps, seeds), re_run)
            assert set(eng.last_host_ms) == {"build_em", "select_prune", "labels", "collect"}
            sweeps = [_Sweep(u, q, FastSampler(np.random.RandomState(sd)), re_run)
                      for u, (q, sd) in enumerate(zip(preps, seeds))]
            Engine._drive(_FakeBatch(preps), sweeps)
            for u, ((fit, lab, nj), sw) in enumerate(zip(got, sweeps)):
                assert _fit_sig(fit) == _fit_sig(sw.best), (base, re_run, u)
                assert nj == sw.n_jobs, (base, re_run, u)
                assert np.array_equal(lab, batch.label_rule(preps[u].N, fit.K, fit.a_idx, fit.b_idx)), (base, re_run, u)
                if re_run:
                    classes["clean" if nj == n_sweep else "pruned" if nj == n_sweep + 1 else "rerun"] += 1
    assert min(classes.values()) >= 5, classes


def test_traced_sweeps_equal_untraced_sweeps():
    """A traced sweep (keep_trace: every fit of the UTR is kept) takes the same draws and gives the same winner and job
    count as an untraced one - with one sampler per UTR (all UTRs advance together) and with one shared sampler driven
    one UTR at a time (the reference's stream) - and its trace is, in order, the fit of every row of that UTR the batch
    was handed."""
    from scape_amd.engine import Engine, _Sweep
    from scape_amd.host import FastSampler
    preps = _stream_preps(30, 9100)

    def run(shared, traced):
        batch = _FakeBatch(preps)
        one = FastSampler(np.random.RandomState(11)) if shared else None
        smps = [one if shared else FastSampler(np.random.RandomState(500 + u)) for u in range(len(preps))]
        sweeps = [_Sweep(u, q, smp, True, [] if traced else None) for u, (q, smp) in enumerate(zip(preps, smps))]
        if shared:
            deferred = []
            for sw in sweeps:
                Engine._drive(batch, [sw], deferred)
            Engine._finish_deferred(batch, deferred)
        else:
            Engine._drive(batch, sweeps)
        return batch, sweeps, [smp.state.copy() for smp in smps]

    for shared in (False, True):
        _b0, plain, plain_states = run(shared, False)
        batch, traced, states = run(shared, True)
        assert [(_fit_sig(sw.best), sw.n_jobs) for sw in traced] == [(_fit_sig(sw.best), sw.n_jobs) for sw in plain]
        for a, b in zip(states, plain_states):
            assert np.array_equal(a, b)
        rows = [[] for _ in preps]
        for pj, out in batch.seen:
            for i, u in enumerate(pj.ju):
                rows[u].append(_fit_sig(_FakeBatch.fit_at(pj, out, i)))
        for sw in traced:
            assert len(sw.trace) == sw.n_jobs and [_fit_sig(f) for f in sw.trace] == rows[sw.u], sw.u
        assert len({sw.n_jobs for sw in traced}) >= 3        # clean, pruned and re-run sweeps all occur


def test_sweep_winners_is_the_reference_float32_argmin():
    """engine.sweep_winners: first arg-min over the restarts of a K, then first arg-min over K, both on BICs rounded to
    float32 as in the reference's bic_arr - on uniform and on ragged spans."""
    import warnings
    from scape_amd.engine import sweep_winners
    from scape_amd.host import N_TRIAL

    def plain(bic, spans):
        win = []
        for lo, hi in zip(spans[:-1], spans[1:]):
            with np.errstate(over="ignore"):
                b32 = np.array(bic[lo:hi], dtype=np.float32)
            per_k = [k0 + int(np.argmin(b32[k0:k0 + N_TRIAL])) for k0 in range(0, hi - lo, N_TRIAL)]     # em_optim0 (:865)
            win.append(int(lo) + per_k[int(np.argmin(b32[per_k]))])                                       # run (:972)
        return win

    rs = np.random.RandomState(5)
    for nks in ([3] * 7, [3, 1, 4, 2, 2, 5, 1], [2]):
        spans = np.concatenate([[0], np.cumsum(np.array(nks) * N_TRIAL)]).astype(np.int64)
        bic = np.round(rs.normal(3000.0, 40.0, spans[-1]))          # rounded: plenty of exact ties
        assert sweep_winners(bic, spans).tolist() == plain(bic, spans), nks
        bic[rs.choice(len(bic), 3, replace=False)] = np.nan         # np.argmin takes the first NaN, as in the reference
        assert sweep_winners(bic, spans).tolist() == plain(bic, spans), nks
    one = np.array([0, 2 * N_TRIAL], dtype=np.int64)
    bic = np.full(2 * N_TRIAL, 50.0)
    bic[[3, 7]] = 10.0                                              # tie within a restart block: the first restart
    assert sweep_winners(bic, one).tolist() == [3]
    bic[N_TRIAL + 1] = 10.0                                         # tie across K blocks: the first block
    assert sweep_winners(bic, one).tolist() == [3]
    bic[N_TRIAL + 1] = 10.0 - 1e-9                                  # smaller in float64, the same float32: still a tie
    assert np.float32(bic[N_TRIAL + 1]) == np.float32(10.0) and sweep_winners(bic, one).tolist() == [3]
    bic[N_TRIAL + 1] = 9.0
    assert sweep_winners(bic, one).tolist() == [N_TRIAL + 1]
    bic[:] = 1e300                                                  # above the float32 maximum: inf, no warning
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert sweep_winners(bic, one).tolist() == [0]
        bic[N_TRIAL + 4] = 3e38
        assert sweep_winners(bic, one).tolist() == [N_TRIAL + 4]
        assert sweep_winners(bic, (N_TRIAL, 2 * N_TRIAL)).tolist() == [N_TRIAL + 4]     # one UTR's slice of a larger call


def test_wave_composition_round_robin():
    """engine.compose_wave: round-robin over the streams in flight with a per-stream cap and a byte budget; each stream's
    UTRs contiguous and in file order, streams in admission order; the first UTR is taken even over budget; a UTR
    larger than the device raises."""
    from scape_amd import _lib, engine

    class Q:
        def __init__(self, N=100, T=218):
            self.N, self.T, self.betas, self.gene_info_str = N, T, np.zeros(13), "g"
    b = engine.Engine.utr_bytes(Q())

    def streams(*sizes):
        return [engine._FileStream(tag, [Q() for _ in range(n)], None, [None] * n) for tag, n in enumerate(sizes)]

    def ids(wave):
        return [(st.tag, i) for st, i in wave]
    act = streams(5, 1, 3)
    assert ids(engine.compose_wave(act, 2, 100 * b, 1000 * b)) == [(0, 0), (0, 1), (1, 0), (2, 0), (2, 1)]
    assert [st.cursor for st in act] == [2, 1, 2]
    assert ids(engine.compose_wave(act, 2, 100 * b, 1000 * b)) == [(0, 2), (0, 3), (2, 2)]      # goes on from the cursors
    assert [st.cursor for st in act] == [4, 1, 3]
    act = streams(5, 1, 3)
    assert ids(engine.compose_wave(act, 2, 4 * b, 1000 * b)) == [(0, 0), (0, 1), (1, 0), (2, 0)]
    assert [st.cursor for st in act] == [2, 1, 1]
    act = streams(2, 2)
    big = Q(1000, 300)
    act[0].preps[0] = big
    assert engine.Engine.utr_bytes(big) > 4 * b
    assert ids(engine.compose_wave(act, 2, 4 * b, engine.Engine.utr_bytes(big))) == [(0, 0)]       # over budget, taken alone
    assert [st.cursor for st in act] == [1, 0]
    act[1].preps[0] = big
    with pytest.raises(_lib.ScapeHipError):
        engine.compose_wave(act, 2, 4 * b, engine.Engine.utr_bytes(big) - 1)


def test_find_peaks_equals_scipy():
    """scape_amd.host.find_peaks restates scipy.signal.find_peaks(x, distance=d) (apa_core.py:784) so that the CLI
    does not import scipy.signal; it must return exactly scipy's peaks - also with plateaus, ties between peak
    heights and peaks closer than the distance."""
    from scipy.signal import find_peaks as sp
    from scape_amd.host import find_peaks
    rs = np.random.RandomState(5)
    cases = []
    for trial in range(300):
        n = int(rs.randint(3, 400))
        kind = trial % 4
        if kind == 0:
            x = rs.random_sample(n)
        elif kind == 1:
            x = rs.randint(0, 4, n).astype(float)                     # plateaus and equal heights everywhere
        elif kind == 2:
            x = np.convolve(rs.poisson(2.0, n).astype(float), np.ones(7) / 7, mode="same")
        else:
            x = np.repeat(rs.randint(0, 6, n // 3 + 1), 3)[:n].astype(float)
        cases.append(x)
    cases += [np.zeros(5), np.array([0., 1, 0]), np.array([1., 1, 1]), np.array([0., 2, 2, 0, 2, 2, 2, 0]), np.arange(10.0)]
    for x in cases:
        for d in (1, 2, 3.5, 10, 100):
            want = sp(x, distance=d)[0]
            got = find_peaks(x, d)[0]
            assert np.array_equal(got, want), (x.tolist(), d, got, want)
    assert len(find_peaks(np.array([1.0, 2.0]), 5)[0]) == 0


def test_column_class_ladder_covers_every_dispatch_threshold():
    """tests/test_em_column_classes.py runs the EM and label kernels at the K values of its LADDER.  The column classes
    are read here from the class lists of scape_hip.hip: every class boundary (kmax + 1 <= C) must have its last K
    (C - 1) and the first K of the next class (C) on the ladder, and so must SCAPE_MAX_K - whoever adds a class has
    to extend the ladder."""
    from test_em_column_classes import FIXED_CAPS, LADDER, MIXED_CAPS
    src = open(os.path.join(ROOT, "scape_amd", "csrc", "scape_hip.hip")).read()
    hdr = open(os.path.join(ROOT, "include", "scape_hip.h")).read()
    max_k = int(re.search(r"#define\s+SCAPE_MAX_K\s+(\d+)", hdr).group(1))

    def class_list(name):
        found = re.findall(r"using %s = std::integer_sequence<int,([\d,\s]+)>;" % name, src)
        assert len(found) == 1 and len(re.findall(r"\b%s\b\s*=" % name, src)) == 1, (name, "defined exactly once")
        return [int(c) for c in found[0].split(",")]
    estep = class_list("EstepClasses")       # k2_estep and k2_estep_all_rounds share it
    fam = {"k2_estep": estep, "k2_estep_cs": class_list("WideClasses"), "k2_estep_all_rounds": estep,
           "k_labels": class_list("LabelClasses")}
    # each family's kernels are dispatched over its list and nowhere else: no launch macro is left, one dispatch per kernel
    assert "LAUNCH_" not in src
    for kernel, lst in (("k2_estep", "EstepClasses"), ("k2_estep_cs", "WideClasses"),
                        ("k2_estep_all_rounds", "EstepClasses"), ("k_labels", "LabelClasses")):
        assert len(re.findall(r"\b%s<" % kernel, src)) == 1, kernel
        assert re.search(r"with_column_class\(%s\{\}, kmax \+ 1, \[&\]\(auto cm\) \{\s*[^;]*\b%s<decltype\(cm\)::value>" % (lst, kernel), src), kernel
    # the wide E-step's cap is derived from its list, not a second literal
    cap_name = re.search(r"wide = .*kmax \+ 1 <= (\w+);", src).group(1)
    assert re.search(r"constexpr int %s = last_class\(WideClasses\{\}\);" % cap_name, src), cap_name
    wide_cap = fam["k2_estep_cs"][-1]
    assert max_k in LADDER and max(LADDER) == max_k and min(LADDER) == 1
    for name, classes in fam.items():
        assert len(classes) >= 4 and classes == sorted(set(classes)), (name, classes)
        top = wide_cap if name == "k2_estep_cs" else max_k + 1
        assert classes[-1] == top, (name, classes)          # the largest class holds the family's largest kmax
        for c in classes[:-1] + ([top] if top <= max_k else []):
            assert c - 1 in LADDER and c in LADDER, (name, c, "no K on both sides of kmax + 1 <= %d" % c)
    # calls with only fixed jobs: one kmax per class of k2_estep_all_rounds; mixed calls: the generic-body classes
    e = fam["k2_estep_all_rounds"]
    cls = lambda kmax: next(c for c in e if kmax + 1 <= c)      # noqa: E731
    assert sorted(cls(k) for k in FIXED_CAPS) == e and all(k in LADDER for k in FIXED_CAPS + MIXED_CAPS)
    generic = [c for c in fam["k2_estep"] if c > 16]            # ESTEP_DISPATCH: exact variants up to 16 columns
    assert "if constexpr (CM <= 16)" in open(os.path.join(ROOT, "scape_amd", "csrc", "em_lockstep.inc")).read()
    assert {cls(k) for k in MIXED_CAPS} == set(generic) and max_k in MIXED_CAPS


def test_tensor_ladder_covers_every_boundary_of_the_tensor_build():
    """tests/test_tensor_ladder.py runs Phase A and the three forms of Phase B on the batches of tests/tensor_ladder.py.
    The boundaries are read here from the sources - row pitch, wavefront / workgroup / launch widths, PA_TT, TILE_ROWS,
    PB_LOGCAP, PB_RING, PB_STEPS, the n_beta <= 16 of the form choice, the 8 of the XCD placement, the T_max cap - and
    the ladder must have a value on both sides of each (whoever moves one has to move the ladder).  The form each case
    expects is recomputed from those constants."""
    import tensor_ladder as tl
    src = open(os.path.join(ROOT, "scape_amd", "csrc", "scape_hip.hip")).read()
    inc = open(os.path.join(ROOT, "scape_amd", "csrc", "phase_b.inc")).read()

    def define(text, name):
        found = re.findall(r"#define\s+%s\s+(\d+)\b" % name, text)
        assert len(found) == 1, name
        return int(found[0])
    PITCH, TILE_ROWS, PA_TT = (define(src, n) for n in ("PITCH", "TILE_ROWS", "PA_TT"))
    LOGCAP, RING, STEPS = (define(inc, n) for n in ("PB_LOGCAP", "PB_RING", "PB_STEPS"))
    # the three places that hold it: batch_plan's walk, phase_b_choose, the load's allocation of the Phase B tables
    b_caps = [re.findall(r"bool slide = p\.n_beta <= (\d+);", src), re.findall(r"if \(B <= (\d+) && !v2 && \(split \|\| slide\)\)", src),
              re.findall(r"if \(p->n_beta <= (\d+)\) \{   // the three-kernel Phase B", src)]
    assert b_caps == [["16"]] * 3, b_caps
    b_cap = {16}
    cap = re.search(r"s\.pb_slide = slide && s\.W_max <= 4 \* PB_STEPS && s\.T_max <= (\d+);", src)
    assert cap and int(cap.group(1)) == 4096            # the cap exists; a 4097-point grid is not part of the ladder
    xcd = re.findall(r"\(slot / (?:T_max|blocks_max)\) \* (\d+) \+ \(id & (\d+)\)", src + inc)
    assert len(xcd) == 2 and set(xcd) == {("8", "7")}, xcd
    wave_bins, wg_bins = re.search(r"const int n0 = (\d+) \* bb \+ (\d+) \* wave", inc).groups()[::-1]
    wave_bins, wg_bins = int(wave_bins), int(wg_bins)
    pa_lanes = int(re.search(r"__launch_bounds__\((\d+)\) void k_phase_a\(", src).group(1))
    assert (wave_bins, wg_bins, pa_lanes) == (PITCH, 4 * PITCH, 256) and "(b.Np_max + 255) / 256, (b.T_max + PA_TT - 1) / PA_TT" in src

    cases = {c.name: c for c in tl.cases()}
    utrs = [q for c in cases.values() for q in c.preps]
    assert all(q.N <= 257 and q.T <= 130 for q in utrs)
    for q in utrs:
        assert np.all(np.diff(q.x) >= 0) and np.all(np.diff(q.theta) >= 0)
    # ---- N: one batch, a UTR on, below and above every bin-count boundary; unequal T, the largest not first
    nc = cases["N"]
    Ns, Ts = [q.N for q in nc.preps], [q.T for q in nc.preps]
    assert Ns == list(tl.N_LADDER) and 1 in Ns
    for b in (PITCH, wg_bins, pa_lanes):
        assert {b - 1, b, b + 1} <= set(Ns), b
    assert len(set(Ts)) == len(Ts) and Ts.index(max(Ts)) > 0
    # ---- T: PA_TT and the ring, the interior range
    all_T = {q.T for q in utrs}
    for b in (PA_TT, RING):
        assert {b - 1, b, b + 1} <= all_T, b
    assert {1, 2} <= all_T

    def interior(q):
        step = q.theta[1] - q.theta[0] if q.T > 1 else 0.0
        if not (step > 0 and np.all(np.floor(q.theta) == q.theta) and np.all(np.diff(q.theta) == step)):
            return None
        rmax = int(np.floor(3 * q.betas.max() / step)) + 1
        return (q.T - 2 - rmax) - (rmax + 1) + 1
    counts = {(c.name, q.T): interior(q) for c in cases.values() for q in c.preps}
    assert counts[("T46", 46)] == 0 and cases["T46"].form == 0
    assert [counts[("Tdef", t)] for t in tl.T_DEFAULT] == [1, 4, 5, 7] and cases["Tdef"].form == 2
    assert [counts[("T12", t)] for t in tl.T_BETAS12] == [1, 3, 4, 5, 59, 60, 61, 64] and cases["T12"].form == 2
    assert counts[("T12none", 1)] is None and counts[("T12none", 2)] < 1 and cases["T12none"].form == 0
    assert {v % 4 for v in counts.values() if v is not None and v >= 4} == {0, 1, 2, 3}

    def widest(q):
        lo = np.searchsorted(q.theta, q.theta - 3 * q.betas.max(), "left")
        hi = np.searchsorted(q.theta, q.theta + 3 * q.betas.max(), "right") - 1
        return int((hi - lo + 1).max())
    # ---- window width: the (PB_STEPS - 1)- and PB_STEPS-step instantiations, one grid too wide (demoted)
    w = {taps: widest(cases[f"W{taps}"].preps[0]) for taps in tl.WIDTHS}
    assert all(k == v for k, v in w.items()), w
    steps = {taps: (taps + 3) // 4 for taps in w}
    assert sorted(steps.values()) == [STEPS - 1, STEPS, STEPS, STEPS + 1]
    assert max(t for t in w if t <= 4 * STEPS) >= 4 * STEPS - 1 and min(t for t in w if t > 4 * STEPS) == 4 * STEPS + 1
    assert cases["W49"].form == 0 and all(cases[f"W{t}"].form == 2 for t in (43, 45, 47))
    rw = cases["ringwrap"].preps[0]
    assert rw.T > RING and widest(rw) >= 4 * (STEPS - 2) and cases["ringwrap"].form == 2
    # inclusive window ends: on the default grid theta_i -+ 3 beta is a grid point at beta = 15, 30, 45, 60
    q = cases["Tdef"].preps[-1]
    i = q.T // 2
    on = [b for b in q.betas if q.theta[i] - 3 * b in q.theta and q.theta[i] + 3 * b in q.theta]
    assert on == [15.0, 30.0, 45.0, 60.0]
    # ---- n_beta: both sides of the form choice, the guards below 16, tile crossings
    assert {1, 3, 4, 5, 13} <= set(tl.N_BETA) and {max(b_cap), max(b_cap) + 1} <= set(tl.N_BETA)
    for B in tl.N_BETA:
        c = cases[f"B{B}"]
        assert len(c.preps[0].betas) == B and c.form == (2 if B <= 16 else 0) and c.forms["split"] == (1 if B <= 16 else 0)
        crosses = [i for i in range(c.preps[0].T) if (i * B) % TILE_ROWS + B > TILE_ROWS]       # an alpha's rows lie in two tiles
        if B in (13, 16):
            assert bool(crosses) == (B == 13), (B, crosses)
    # ---- n_log: both sides of PB_LOGCAP, none, one, every bin; at n = 0, PITCH - 1, PITCH, N - 1; both kinds
    lg = [(q.N, np.flatnonzero(~np.isnan(q.pa) | ~np.isnan(q.r))) for q in cases["nlog"].preps]
    n_log = [len(b) for _, b in lg]
    assert {0, 1, LOGCAP, LOGCAP + 1} <= set(n_log) and any(len(b) == N for N, b in lg)
    singles = sorted(int(b[0]) for N, b in lg if len(b) == 1)
    assert singles == [0, PITCH - 1, PITCH, 99]
    for q in utrs:
        if q.N > PITCH:
            assert {0, PITCH - 1, PITCH, q.N - 1} <= set(np.flatnonzero(~np.isnan(q.pa) | ~np.isnan(q.r))) or any(q is p for p in cases["nlog"].preps)
    assert any((~np.isnan(q.pa)).any() and (~np.isnan(q.r)).any() for q in cases["nlog"].preps)
    # ---- n_utr: both sides of the XCD placement's 8, unequal T
    xcds = int(xcd[0][0])
    assert {1, xcds - 1, xcds, xcds + 1} <= set(tl.N_UTR)
    for n in tl.N_UTR:
        ps = cases[f"U{n}"].preps
        assert len(ps) == n and (n == 1 or len({q.T for q in ps}) > 1)
    # ---- grids
    fr, rp = cases["fractional"].preps[0].theta, cases["repeated"].preps[0].theta
    assert np.any(np.floor(fr) != fr) and len(set(np.diff(fr))) > 1 and np.all(fr * 4 == np.floor(fr * 4))
    assert np.any(np.diff(rp) == 0) and np.all(np.diff(rp) >= 0)
    assert cases["fractional"].form == 0 and cases["repeated"].form == 0 and cases["fractional"].forms["split"] == 1
    # ---- values
    for q in (cases["N"].preps[-1], cases["cut"].preps[0]):
        u = q.theta[None, :] - q.x[:, None]
        assert np.any(q.l[:, None] == u) and np.any(u < 0)
        assert np.any(np.isin(q.pa[~np.isnan(q.pa)], q.theta)) and not np.all(np.isin(q.pa[~np.isnan(q.pa)], q.theta))
    rs = np.concatenate([q.r[~np.isnan(q.r)] for q in utrs])
    s = tl.S_DIS
    assert rs.max() <= s.max() and np.any(rs < s[0]) and np.any(np.isin(rs, s)) and np.any(~np.isin(rs, s) & (rs > s[0]))
    assert cases["cut"].preps[0].p["sigma_f"] == 10
    # ---- the form every case expects, recomputed from the constants read above
    for c in cases.values():
        want = 2 if tl.expected_slide(c.preps, b_cap=max(b_cap), steps=STEPS, t_cap=int(cap.group(1))) else 0
        assert c.form == want, (c.name, c.form, want)
    assert {c.form for c in cases.values()} == {0, 2}


def test_mstep_ladder_covers_every_boundary_of_the_mstep_kernels():
    """tests/test_mstep_ladder.py runs k2_mstep, k3_mstep and k4_mstep on the cases of tests/mstep_ladder.py.  The
    boundaries are read here from the sources - MT_ROWS, MT_NC, MT_MAXJ, M3_CH, M4_TPW, EM_DEPTH, SCAPE_MAX_JOBS_PER_UTR,
    the ring-depth formulas, the jobs_per_pass values, the 1,024-entry rule of em_depth, the n_utr >= 8 split - and the
    ladder must have a case on both sides of each (whoever moves one has to move the ladder).  The ladder's restatement
    of the kernel-selection rule (em_wide, em_depth, em_choose) is pinned to the source here as well."""
    import mstep_ladder as ml
    csrc = os.path.join(ROOT, "scape_amd", "csrc")
    src = open(os.path.join(csrc, "scape_hip.hip")).read()
    em = open(os.path.join(csrc, "em_lockstep.inc")).read()      # the constants the E-step and the host share with the M-step
    frame = open(os.path.join(csrc, "mstep.inc")).read()         # what the three kernels share
    k2 = open(os.path.join(csrc, "mstep_staged.inc")).read()
    k3 = open(os.path.join(csrc, "mstep_ring.inc")).read()
    k4 = open(os.path.join(csrc, "mstep_multi.inc")).read()
    hdr = open(os.path.join(ROOT, "include", "scape_hip.h")).read()

    def define(text, name):
        found = re.findall(r"#define\s+%s\s+(\d+)\b" % name, text)
        assert len(found) == 1, name
        return int(found[0])
    MT_RB, MT_MAXJ, DEPTH = (define(em, n) for n in ("MT_RB", "MT_MAXJ", "EM_DEPTH"))
    MT_NC = define(k2, "MT_NC")
    assert "#define MT_ROWS (64 * MT_RB)" in em
    MT_ROWS = 64 * MT_RB
    M3_CH, M3_WPC, M4_TPW = define(frame, "M3_CH"), define(k3, "M3_WPC"), define(k4, "M4_TPW")
    assert not re.findall(r"#define\s+(MT_NC|M3_CH)\b", em + k3 + k4)              # one definition each, in the file read above
    MAX_JOBS = define(hdr, "SCAPE_MAX_JOBS_PER_UTR")
    # ---- the ladder's constants and its restatement of the selection rule
    assert (ml.ROWS, ml.HALF, ml.MT_MAXJ, ml.EM_DEPTH, ml.MAX_JOBS_PER_UTR) == (MT_ROWS, M3_CH, MT_MAXJ, DEPTH, MAX_JOBS)
    assert "const bool wide = n_jobs <= sw.wide_maxjobs && kmax + 1 <= WIDE_MAX_COLUMNS;" in src
    assert "constexpr int WIDE_MAX_COLUMNS = last_class(WideClasses{});" in src
    wide = [int(c) for c in re.findall(r"using WideClasses = std::integer_sequence<int,([\d,\s]+)>;", src)[0].split(",")]
    assert ml.WIDE_MAX_COLUMNS == wide[-1]
    assert "s.split_maxtiles = env_r ? atoi(env_r) : %d;" % ml.SPLIT_MAXTILES_DEFAULT in src
    assert "s.wide_maxjobs = env_w ? atoi(env_w) : %d;" % ml.WIDE_MAXJOBS_DEFAULT in src
    assert "s.depth = std::min(EM_DEPTH, std::max(1, env_d ? atoi(env_d) : EM_DEPTH));" in src
    assert "if (!any_m || em_wide(sw, n_jobs, kmax)) return 1;" in src
    entries = re.search(r"while \(depth > 1 && \(\(size_t\)max_jobs_utr \* depth > (\d+) \|\|", src)
    assert entries and int(entries.group(1)) == ml.LIST_ENTRIES and len(re.findall(r"off < %d\) s_all\[off\] = j;" % ml.LIST_ENTRIES, k2)) == 1
    assert "k.job_split = (long long)p.active.size() * p.tiles_max <= sw.split_maxtiles;" in src
    assert "k.multi_mstep = k.ring_mstep && !k.job_split && !sw.debug && p.pttot < ((size_t)1 << 31) && !sw.mstep_v3;" in src
    assert "const int jobs_per_pass = k.job_split ? 16 : MT_MAXJ;" in src
    assert "const unsigned psplit = k.job_split ? (unsigned)std::min(64, (p.max_cols_utr + 15) / 16) : 1u;" in src
    xcd = re.findall(r"if \(n_utr >= (\d+)\) \{", frame)                            # the grid rule: stated once, in mstep_block,
    assert xcd == [str(ml.XCD_UTRS)] and not re.findall(r"n_utr\s*[<>]=?\s*\d", k2 + k3 + k4), xcd   # and taken from there by all three
    for k in (k2, k3, k4):
        assert len(re.findall(r"if \(!mstep_block\(blockIdx\.x, n_utr, \w+, ul, \w+\)\) return;", k)) == 1
    # ---- ring depths, from the formulas
    assert "#define M3_AREA_BYTES (M3_WPC >= 3 ? 51 * 1024 : 78 * 1024)" in k3
    assert "constexpr int m3_rv(int G) { return (M3_WPC >= 3) ? (G <= 1 ? 3 : 2) : 3; }" in k3
    assert re.search(r"constexpr int m3_rt\(int G\) \{\s*return \(M3_AREA_BYTES - m3_rv\(G\) \* G \* 2048\) / 8192 > 10 \? 10 : "
                     r"\(M3_AREA_BYTES - m3_rv\(G\) \* G \* 2048\) / 8192;", k3)
    assert "#define M4_REC_BYTES (64 * 24)" in k4 and "#define M4_WPC M3_WPC" in k4
    assert "#define M4_TAIL_BYTES (4 * 64 * 12 + M4_TPW * (M4_REC_BYTES + 12 * 4) + 16 * 4 + 4 * 8)" in k4
    assert "#define M4_AREA_BYTES (((M4_WPC >= 3 ? 53760 : 81920) - M4_TAIL_BYTES) / 1024 * 1024)" in k4
    assert "constexpr int m4_rv(int G) { return M4_AREA_BYTES / (G * 2048 + 8192) < 2 ? 2 : M4_AREA_BYTES / (G * 2048 + 8192); }" in k4
    assert re.search(r"constexpr int m4_rt\(int G\) \{\s*return \(M4_AREA_BYTES - m4_rv\(G\) \* G \* 2048\) / 8192 > 10 \? 10 : "
                     r"\(M4_AREA_BYTES - m4_rv\(G\) \* G \* 2048\) / 8192;", k4)
    a3 = 51 * 1024 if M3_WPC >= 3 else 78 * 1024
    a4 = ((53760 if M3_WPC >= 3 else 81920) - (4 * 64 * 12 + M4_TPW * (64 * 24 + 12 * 4) + 16 * 4 + 4 * 8)) // 1024 * 1024
    m3_rv = lambda G: ((3 if G <= 1 else 2) if M3_WPC >= 3 else 3)                  # noqa: E731
    m3_rt = lambda G: min(10, (a3 - m3_rv(G) * G * 2048) // 8192)                   # noqa: E731
    m4_rv = lambda G: max(2, a4 // (G * 2048 + 8192))                               # noqa: E731
    m4_rt = lambda G: min(10, (a4 - m4_rv(G) * G * 2048) // 8192)                   # noqa: E731
    cases = {c.name: c for c in ml.cases()}
    ring = cases["ring"]
    halves = {(q.N + M3_CH - 1) // M3_CH for q in ring.preps}
    assert halves == set(ml.RING_HALVES) and all(q.N % M3_CH for q in ring.preps)   # Np padding in every one
    groups = {n // len(ring.preps) // 16 for n in ring.calls}
    assert groups == {1, 2, 3, 4} == set(range(1, MT_MAXJ // 16 + 1))
    for n in ring.calls:                                                            # 16 G columns on every UTR's tile
        per = np.bincount([j.u for j in ring.jobs[:n]])
        assert np.all(per == n // len(ring.preps)) and per[0] % 16 == 0
    for G in groups:
        for depth in (m3_rt(G), m3_rv(G), m4_rt(G), m4_rv(G)):
            assert {1, 2, depth - 1, depth, depth + 1} - {0} <= halves, (G, depth)
    tile = {j.a_idx[0] * 8 // MT_ROWS for j in ring.jobs} | {(j.a_idx[2] * 8 + 7) // MT_ROWS for j in ring.jobs}
    assert tile == {ml.RING_TILE} and len(ring.preps[0].betas) == 8                 # every window inside one tile
    # ---- bins: the 16-bin half-chunk, k2_mstep's MT_NC-bin chunk
    Ns = [q.N for q in cases["bins"].preps]
    for b in (M3_CH, MT_NC):
        assert {b - 1, b, b + 1} <= set(Ns), b
    assert 1 in Ns and Ns[:len(ml.N_LADDER)] == list(ml.N_LADDER)
    for N in ml.N_LADDER:
        dropped = {nb for (n_, nb) in ml.BIN_SEEDS if n_ == N}
        assert {0, N - 1} <= dropped and {b for b in (M3_CH - 1, M3_CH, MT_NC - 1, MT_NC) if b < N} <= dropped, N
    # ---- call shape: 1 UTR, one below / on / above the XCD split; the passes of 16 and of MT_MAXJ; the list limits
    per_call = [len({j.u for j in cases["bins"].jobs[:n]}) for n in cases["bins"].calls]
    assert per_call == list(ml.N_UTR_CALLS) and {1, ml.XCD_UTRS - 1, ml.XCD_UTRS, ml.XCD_UTRS + 1} <= set(per_call)
    cols = set(cases["columns"].calls)
    for b in (16, 32, 48, MT_MAXJ, 2 * MT_MAXJ):
        assert {b, b + 1} <= cols, b
    assert {1, 15} <= cols and all(j.K == 1 for j in cases["columns"].jobs)
    many = cases["many"]
    assert max(many.calls) == MAX_JOBS and all(j.K == 1 for j in many.jobs) and many.preps[0].N <= 17
    for d in range(2, DEPTH + 1):                                                   # em_depth: the largest job count that keeps depth d
        assert {ml.LIST_ENTRIES // d, ml.LIST_ENTRIES // d + 1} <= set(many.calls), d
    got = {n: [ml.selection(env, many.jobs[:n], many.preps)["depth"] for _f, env in ml.FORMS] for n in many.calls}
    assert got[341][1] == 3 and got[342][1] == 2 and got[512][1] == 2 and got[513][1] == 1 and got[1024][1] == 1
    # ---- every case runs all three kernels, split and whole passes, both E-steps
    for c in cases.values():
        for n in c.calls or (len(c.jobs),):
            sel = [ml.selection(env, c.jobs[:n], c.preps) for _f, env in ml.FORMS]
            assert {s["kernel"] for s in sel} == {"k2_mstep", "k3_mstep", "k4_mstep"}, (c.name, n)
            assert {(s["kernel"], s["job_split"]) for s in sel} >= {("k2_mstep", True), ("k2_mstep", False), ("k3_mstep", True),
                                                                    ("k3_mstep", False), ("k4_mstep", False)}, (c.name, n)
            assert sel[-1]["wide"] and not any(s["wide"] for s in sel[:-1]), (c.name, n)
    # ---- window rows: B = 13 reaches every residue; the three beta counts; a grid of another length
    w = cases["window"]
    assert len(w.preps[0].betas) == 13 and {len(c.preps[0].betas) for c in cases.values()} == {8, 13, 16}
    ends = {(e, r) for (e, r) in ml.WINDOW_ENDS}
    assert ends == {(e, r) for e in ("lo", "hi") for r in (0, 1, 15, 16, 17, MT_ROWS - 1)}
    assert set(ml.WINDOW_TILES) == {1, 2, 3} and M4_TPW == 2                          # k4_mstep takes tiles in pairs: the odd tile last
    assert all((q.T * len(q.betas)) % MT_ROWS for c in cases.values() for q in c.preps)   # the last tile is partial everywhere


def test_estep_ladder_covers_every_boundary_of_the_estep():
    """tests/test_estep_ladder.py runs estep_body through k2_estep, k2_estep_all_rounds and k2_estep_cs on the cases of
    tests/estep_ladder.py.  The boundaries are read here from the sources - the 64 lanes of the bin loop, the row pitch,
    the column classes and the exact-variant limit of ESTEP_DISPATCH, the liveness cut, the rescue constant, the series
    limit of log s2, EM_DEPTH - and the ladder must have a value on both sides of each (whoever moves one has to move the
    ladder).  The ladder's restatement of which E-step kernel a call runs is pinned to the source here as well."""
    import estep_ladder as el
    import mstep_ladder as ml
    csrc = os.path.join(ROOT, "scape_amd", "csrc")
    src = open(os.path.join(csrc, "scape_hip.hip")).read()
    k2 = open(os.path.join(csrc, "em_lockstep.inc")).read()
    # ---- lanes and pitch
    assert len(re.findall(r"for \(int n = lane; n < Np; n \+= (\d+)\)", k2)) == 1 and len(re.findall(r"for \(int n0 = 0; n0 < Np; n0 \+= (\d+), buf \^= 1\)", k2)) == 1
    assert {re.search(r"for \(int n = lane; n < Np; n \+= (\d+)\)", k2).group(1),
            re.search(r"for \(int n0 = 0; n0 < Np; n0 \+= (\d+), buf", k2).group(1)} == {str(el.LANES)}
    assert "fetch(n + %d, mnext, cnext);" % el.LANES in k2 and "__launch_bounds__(%d, (CMAX > 12 ? 2 : ESTEP_WPS)) void k2_estep(" % el.LANES in k2
    assert int(re.search(r"#define PITCH (\d+)\b", src).group(1)) == el.PITCH and "d.Np = round_up((int)N, PITCH);" in src
    Ns = set(el.N_BINS)
    for b in (el.PITCH, el.LANES, 2 * el.LANES):
        assert {b - 1, b, b + 1} <= Ns, b
    assert {1, 4 * el.LANES + 1} <= Ns and max(Ns) <= 257
    by = {c.name: c for c in el.cases()}
    assert [q.N for q in by["bins"].preps[:-1]] == list(el.N_BINS)
    # ---- column classes, the exact variants, the wide cap
    classes = [int(c) for c in re.findall(r"using EstepClasses = std::integer_sequence<int,([\d,\s]+)>;", src)[0].split(",")]
    wide = [int(c) for c in re.findall(r"using WideClasses = std::integer_sequence<int,([\d,\s]+)>;", src)[0].split(",")]
    assert tuple(classes) == el.CLASSES and wide == [c for c in classes if c <= ml.WIDE_MAX_COLUMNS] and wide[-1] == ml.WIDE_MAX_COLUMNS
    assert "if constexpr (CM <= %d)" % el.EXACT_MAX in k2 and el.EXACT_MAX in classes
    Ks = set(el.K_COLUMNS)
    for c in classes[:-1]:                                                      # kmax + 1 <= c: K = c - 1 and K = c
        assert {c - 1, c} <= Ks, c
    assert {0, 1, 2, 3, classes[-1] - 1} <= Ks
    assert [next(c for c in classes if k + 1 <= c) for k in el.MIXED_KMAX] == [24, 24, 32, 64] and set(classes) - {4, 8, 12, 16} == {24, 32, 64}
    cols = by["columns"]
    assert cols.calls[:len(el.K_COLUMNS)] == tuple((i,) for i in range(len(el.K_COLUMNS)))
    assert [max(cols.jobs[i].K for i in call) for call in cols.calls[len(el.K_COLUMNS):]] == list(el.MIXED_KMAX)
    assert all(min(cols.jobs[i].K for i in call) == 0 for call in cols.calls[len(el.K_COLUMNS):])
    # ---- the constants of the body
    assert len(re.findall(r"arg >= (-[\d.]+)\)", k2)) == 2 and set(re.findall(r"arg >= (-[\d.]+)\)", k2)) == {"%.1f" % el.EXP_CUT}
    assert "any_live |= arg[i] >= %.1f;" % el.EXP_CUT in k2 and mr_exp_zero() > el.EXP_CUT
    assert k2.count("t_sumk < 1e-8") == 2 and k2.count("if (mod) z[c] += 1e-8;") == 2 and el.RESCUE == 1e-8
    assert k2.count("if (__ballot(fabs(x2) >= 1e-5)) ls2 = (fabs(x2) < 1e-5) ? ls2 : log(s2);") == 2 and el.LS2_SERIES == 1e-5
    assert k2.count("if (wK > P.max_unif_ws) {") == 1
    assert int(re.search(r"#define EM_DEPTH (\d+)", k2).group(1)) == ml.EM_DEPTH
    # ---- which kernel a call runs
    assert re.search(r"if \(!p\.any_m\) \{.{0,400}?launch_estep\(c, k2_estep_all_rounds<decltype\(cm\)::value>.{0,300}?return 0;\s*\}", src, re.S)
    assert re.search(r"k\.wide \? with_column_class\(WideClasses\{\}, kmax \+ 1, \[&\]\(auto cm\) \{\s*launch_estep\(c, k2_estep_cs<", src)
    assert 's.shrink = !(env_s && atoi(env_s) == 0);' in src and "any_m = any_m || job_fixed[j] == 0;" in src
    for c in by.values():
        small = False
        for call in c.calls or (tuple(range(len(c.jobs))),):
            jobs = [c.jobs[i] for i in call]
            assert all(j.fixed for j in jobs) and not c.companion.fixed and c.companion.u == len(c.preps) - 1 and c.companion.K == 1
            assert all(j.u < len(c.preps) - 1 for j in jobs)                     # the companion's UTR is its own
            sel = [el.selection(env, jobs + ([c.companion] if comp else [])) for _n, comp, env in el.SHAPES]
            kmax = max(1, max(j.K for j in jobs))
            want_cs = kmax + 1 <= ml.WIDE_MAX_COLUMNS
            small = small or want_cs
            assert [s["kernel"] for s in sel] == ["k2_estep_all_rounds", "k2_estep", "k2_estep", "k2_estep_cs" if want_cs else "k2_estep", "k2_estep"]
            assert [s["depth"] for s in sel[1:3]] == [1, ml.EM_DEPTH] and len({s["cls"] for s in sel}) == 1
        assert small or c.name != "bins"
    # ---- every family is there, T is the ladder's usual, N stays small
    assert {c.family for c in by.values()} == set(range(1, 11))
    assert all(q.N <= 257 and 200 <= q.T <= 230 for c in by.values() for q in c.preps)
    assert {c.nround for c in by.values() if c.family == 10} == {2, 5, 10, 20}


def test_label_ladder_covers_every_boundary_of_the_label_kernel():
    """tests/test_label_ladder.py runs k_labels on the cases of tests/label_ladder.py.  The boundaries are read here from the
    sources - LabelClasses, the 256 threads of the launch bounds, of the launch and so of the stride loop, the 64 lanes of
    a wavefront, the 16-bin row pitch, the clamp of d_exp_nonpos, SCAPE_MAX_K - and the ladder must have a case on both
    sides of each (whoever moves one has to move the ladder).  The reference's restatement of the pitch and the block is
    pinned to the source here as well."""
    import label_ladder as ll
    from oracle import label_reference as lr
    src = open(os.path.join(ROOT, "scape_amd", "csrc", "scape_hip.hip")).read()
    hdr = open(os.path.join(ROOT, "include", "scape_hip.h")).read()
    # ---- the column classes
    classes = [int(c) for c in re.findall(r"using LabelClasses = std::integer_sequence<int,([\d,\s]+)>;", src)[0].split(",")]
    max_k = int(re.search(r"#define\s+SCAPE_MAX_K\s+(\d+)", hdr).group(1))
    assert tuple(classes) == ll.CLASSES and classes[-1] == max_k + 1 and ll.KMAX_PAD == max_k
    Ks = set(ll.K_CLASSES)
    for c in classes:                                             # kmax + 1 <= c: K = c - 2, c - 1 and (below the last) c
        assert {c - 2, c - 1} <= Ks and (c == classes[-1] or c in Ks), c
    assert {0, 1} <= Ks
    by = {c.name: c for c in ll.cases()}
    assert [m.K for m in by["classes"].models] == list(ll.K_CLASSES) and by["classes"].calls == tuple((i,) for i in range(len(Ks)))
    assert all(ll.pitches(by["classes"], call) == ((max(1, by["classes"].models[call[0]].K), max_k) if by["classes"].models[call[0]].K != max_k
                                                    else (max_k,)) for call in by["classes"].calls)
    edge = {c for _K, c0, c1 in ll.PLANT_PAIRS for c in (c0, c1)}
    for c in classes[:-1]:                                        # planted and tied pairs straddle every class edge: columns c - 1 and c
        assert {c - 1, c} <= edge and any((c0, c1) == (c - 1, c) for _K, c0, c1 in ll.PLANT_PAIRS), c
        assert any((c0, c1) == (c - 1, c) for _K, c0, c1 in ll.TIE_PAIRS), c
    assert (max_k, max_k - 1, max_k) in ll.PLANT_PAIRS and {K for K, _c0, c1 in ll.PLANT_PAIRS if c1 == K} >= {1, 7, 8, 16, 32, max_k}
    # ---- the 256 threads: launch bounds, launch, stride loop; the 64 lanes
    assert re.search(r"__global__ __launch_bounds__\((\d+)\) void k_labels\(", src).group(1) == str(ll.BLOCK)
    assert re.search(r"hipLaunchKernelGGL\(k_labels<decltype\(cm\)::value>, dim3\(n_sel\), dim3\((\d+)\)", src).group(1) == str(ll.BLOCK)
    body = src[src.index("void k_labels("):src.index("// host side")]
    assert "for (int n = threadIdx.x; n < d.N; n += blockDim.x) {" in body and "labels[d.bin_off + n] = best;" in body
    assert lr.BLOCK == ll.BLOCK and lr.PITCH == ll.PITCH
    Ns = set(ll.N_BINS)
    for b in (ll.PITCH, 64, ll.BLOCK):
        assert {b - 1, b, b + 1} <= Ns, b
    assert {1, 2 * ll.BLOCK + 1} <= Ns and max(Ns) == 2 * ll.BLOCK + 1
    assert ll.PLANT_BINS == (0, ll.BLOCK - 1, ll.BLOCK) and ll.PLANT_N == ll.BLOCK + 1
    assert {ll.BLOCK + 1, 2 * ll.BLOCK + 1} <= set(ll.CALL_N) and any(n % ll.PITCH == 0 for n in ll.CALL_N)
    # ---- the row pitch
    assert int(re.search(r"#define PITCH (\d+)\b", src).group(1)) == ll.PITCH and "d.Np = round_up((int)N, PITCH);" in src
    assert "* B + b_in[(size_t)sel * kmax + c]) * d.Np : 0;" in body and "d_logw(ws_in[(size_t)sel * (kmax + 1) + c])" in body
    assert any(n % ll.PITCH for n in Ns) and any(n % ll.PITCH == 0 for n in Ns)
    # ---- the clamp of d_exp_nonpos, the counts on both sides of it (tests/test_label_reference.py looks at the arguments)
    assert "x = fmax(x, %.1f);" % ll.EXP_CLAMP in src and "d_exp_nonpos((lz[c] - mx) * cn, s_exptab)" in body
    assert ll.COUNT_MAX == 1000 and by["counts"].preps[0].cnt.max() == ll.COUNT_MAX and by["counts"].preps[0].cnt[ll.COUNT_BIN] == ll.COUNT_MAX
    # ---- the first maximum, the zero weight, the refusal
    assert "if (c < C && (c == 0 || zc > bz)) {" in body and "return (w <= 0.0) ? SENT : log(w); }" in src
    assert 'return fail("labels: a UTR is named twice");' in src and "a UTR is named twice" in hdr
    # ---- every family is there, T is the ladder's usual, the tensors stay small
    assert list(by) == ["bins", "classes", "planted", "ties", "counts", "calls"]
    assert all(q.N <= 2 * ll.BLOCK + 1 and 200 <= q.T <= 230 and len(q.betas) == 13 for c in by.values() for q in c.preps)
    assert all(len({by[n].models[i].u for i in call}) == len(call) for n in by for call in by[n].calls)   # one model per UTR and call


def mr_exp_zero():
    from oracle import mstep_reference as mr
    return mr.EXP_ZERO


def test_report_ladder_covers_every_boundary_of_the_report_kernels():
    """tests/test_report_ladder.py runs the count, scan, render, segment-sum and histogram kernels of report.inc and the
    count rule of report_mtx.inc's entry walk on the cases of tests/report_ladder.py.  The boundaries are read here from the source - REP_THREADS (the column tile of the
    render kernels, the word tile of k_rep_groups), REP_SCAN_THREADS (the step of k_rep_scan), the 64 lanes that the block
    helpers hard-code, REP_ZERO_FIELD - and the ladder must have a value on both sides of each, and beyond the second
    step of the two loops that carry (whoever moves one has to move the ladder)."""
    import report_ladder as rl
    src = open(os.path.join(ROOT, "scape_amd", "csrc", "report.inc")).read()
    mtx = open(os.path.join(ROOT, "scape_amd", "csrc", "report_mtx.inc")).read()
    threads = int(re.search(r"#define REP_THREADS (\d+)\b", src).group(1))
    scan = int(re.search(r"#define REP_SCAN_THREADS (\d+)\b", src).group(1))
    zero = int(re.search(r"#define REP_ZERO_FIELD (\d+)\b", src).group(1))
    assert (threads, scan, zero) == (rl.THREADS, rl.SCAN, rl.ZERO_FIELD) and "#define REP_WAVES (REP_THREADS / 64)" in src
    # ---- the wavefront of 64 as the helpers hard-code it
    helpers = src[src.index("// ---- block helpers"):src.index("__device__ __forceinline__ int rep_digits(")]
    assert helpers.count("const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;") == 2 and rl.WAVE == 64
    assert "for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);" in helpers
    assert "for (int o = 1; o < 64; o <<= 1) {" in helpers and "if (lane >= o) x += y;" in helpers and "if (lane == 63) lds[w] = x;" in helpers
    # ---- the loops whose strides the ladder straddles
    tile_loop = "for (int base = 0; base < n_cols; base += REP_THREADS) {"
    # the dense render; the one Matrix Market walk and the length matrix's render, which is a kernel of its own
    assert (src.count(tile_loop), mtx.count(tile_loop)) == (1, 2)
    assert "for (int base = 0; base < n_words; base += REP_THREADS) {" in src and "carry += tile;" in src
    assert "for (int base = 0; base < n; base += REP_SCAN_THREADS) {" in src and "carry += tot;" in src
    assert (src.count("pos += tile;"), mtx.count("pos += tile;")) == (1, 2) and "for (int s = w; s < n_seg; s += REP_WAVES) {" in src
    by = {c.name: c for c in rl.cases()}
    cols, rows = {c.n_cols for c in by.values() if c.family == "a"}, {len(c.rows) for c in by.values() if c.family == "c"}
    assert cols == set(rl.COLS) and rows == set(rl.ROWS)
    for c in (rl.WAVE, threads):
        assert {c - 1, c, c + 1} <= cols, c
    assert {2 * threads, 2 * threads + 1} <= cols and 1 in cols
    assert {scan - 1, scan, scan + 1, 2 * scan, 2 * scan + 1} <= rows and 1 in rows
    # ---- field widths on both sides of the zero field, in both forms; the digit counts the ladder reaches
    widths = {len(rl.field(v, f)) for v in by["widths"].counts[0] for f in (True, False)}
    assert {zero - 1, zero, zero + 1} <= widths and {len(str(v)) for v in rl.WIDTH_COUNTS} == set(range(1, 8))
    assert all(p in rl.WIDTH_COUNTS for d in range(1, 7) for p in (10 ** d - 1, 10 ** d))
    assert {c for c, v in rl.WIDTH_COLS.items() if v >= 10} >= {0, rl.WAVE - 1, rl.WAVE, threads - 1, threads, threads + 1}
    assert by["widths"].n_cols == threads + 2
    # ---- prefixes around the stride of the prefix copy, records around the wavefront
    assert "for (int64_t k = threadIdx.x; k < plen; k += REP_THREADS) dst[k] = pre[p0 + k];" in src
    assert {0, 1, threads - 1, threads, threads + 1} <= set(rl.PREFIX_LENGTHS) and max(rl.PREFIX_LENGTHS) > 2 * threads
    assert {1, rl.WAVE - 1, rl.WAVE} <= set(rl.RECORD_KS) and max(rl.RECORD_KS) > rl.WAVE
    assert by["records_complete"].n_cols == threads + 1
    # ---- cluster codes: 32 per bitmap word, REP_THREADS words per step of k_rep_groups
    assert "atomicOr(&b[code >> 5], 1u << (code & 31));" in src and "const int32_t n_words = (n_codes + 31) / 32;" in src
    codes = {h.n_codes for h in rl.hist_cases()}
    assert {32 * threads - 1, 32 * threads, 32 * threads + 1} <= codes and {1, 31, 32, 33, 64, None} <= codes
    # ---- segments: four wavefronts per workgroup, lengths around the 64 lanes
    waves = threads // 64
    assert {waves - 1, waves, waves + 1, 2 * waves + 1, 1} <= set(rl.SEG_LENGTHS)
    assert {0, 1, rl.WAVE - 1, rl.WAVE, rl.WAVE + 1} <= {n for v in rl.SEG_LENGTHS.values() for n in v}
    assert max(n for v in rl.SEG_LENGTHS.values() for n in v) > 4 * rl.WAVE                  # beyond the unrolled four
    assert {"a", "b", "c", "d", "e", "g"} == {c.family for c in by.values()}
