"""EM run-ahead: a job's bits must not depend on how many of its rounds share a tensor pass.

With SCAPE_HIP_EM_DEPTH > 1 (the default is the library's EM_DEPTH) a job executes up to that many consecutive rounds
between two M-step launches - as long as the next round's component is neither equal nor adjacent to one whose grid
arg-max is still pending - and publishes one M-step column per round (em_lockstep.inc: k2_estep).
SCAPE_HIP_EM_DEPTH=1 is the one-round-per-pass schedule.  Every case runs the same job tables at depth 1 and at the
other depths, through the M-step kernels (k3_mstep: calls with few live tiles, the default for these small calls;
k4_mstep: wave-sized calls, selected with SCAPE_HIP_SPLIT_MAXTILES=0; k2_mstep: SCAPE_HIP_MSTEP=v2), and every output
must be bit-equal: alpha_idx, beta_idx, ws, bic, n_lb and all of lb_arr.  SCAPE_HIP_WIDE_MAXJOBS=0 keeps the calls on k2_estep (the
4-wavefront E-step of small calls runs one round per pass whatever the depth).
"""
import os

import numpy as np
import pandas as pd
import pytest

pytestmark = pytest.mark.gpu

NARROW = {"SCAPE_HIP_WIDE_MAXJOBS": "0"}
VARIANTS = (                                   # (name, environment on top of NARROW)
    ("default depth, k3_mstep", {}),
    ("default depth, k4_mstep", {"SCAPE_HIP_SPLIT_MAXTILES": "0"}),
    ("depth 2, k4_mstep", {"SCAPE_HIP_EM_DEPTH": "2", "SCAPE_HIP_SPLIT_MAXTILES": "0"}),
    ("default depth, k2_mstep", {"SCAPE_HIP_MSTEP": "v2"}),
)
LIB_DEPTH = 3                                  # EM_DEPTH of the library (em_lockstep.inc); test_host-style source check below


def passes(k_arr, K, n_rounds, depth, fixed=False):
    """The schedule rule restated: the rounds 0 .. n_rounds - 1 of a job grouped into passes over the tensor."""
    out, i = [], 0
    while i < n_rounds:
        grp, pend = [i], ({int(k_arr[i])} if k_arr[i] < K else set())
        i += 1
        while not fixed and len(grp) < depth and i < n_rounds:
            c = int(k_arr[i])
            if {c - 1, c, c + 1} & pend:
                break
            grp.append(i)
            if c < K:
                pend.add(c)
            i += 1
        out.append(grp)
    return out


def _one_bin_df():
    n = 120
    return pd.DataFrame({"x": np.full(n, 400, np.int64), "l": np.full(n, 98, np.int64), "r": np.full(n, np.nan),
                         "pa": np.full(n, np.nan), "cb_id": np.arange(n), "read_id": np.arange(n)})


class _Bench:
    """Four synthetic UTRs (300-500 reads; the last one a single bin, the degenerate input of the edge-case tests) on a
    library handle of its own."""

    def __init__(self, nround=None):
        from scape_amd import _lib, engine
        from scape_amd.host import Sampler, prepare_utr
        from scape_amd.synth import synth_utr
        self.engine = engine
        self.nround = engine.N_ROUND if nround is None else nround
        items = [synth_utr(i, 300 + 100 * i, k_cap=5, base_seed=4100, pa_rate=0.05, r_rate=0.05) for i in range(3)]
        dfs = [df for _, df, *_ in items] + [_one_bin_df()]
        names = [g for g, *_ in items] + ["syn:ONEBIN:1:1-2000:+"]
        self.preps = [prepare_utr(df, gene_info_str=g) for df, g in zip(dfs, names)]
        self.sampler = Sampler(np.random.RandomState(20261018))
        self.ctx = _lib.Context(0)
        old = engine.N_ROUND
        engine.N_ROUND = self.nround            # HipBatch takes the call's round cap from here
        try:
            self.batch = engine.HipBatch(self.ctx, self.preps)
            self.batch.build()
        finally:
            engine.N_ROUND = old

    def jobs(self, Ks, utrs=(0, 1, 2), restarts=3, fixed=False):
        out = []
        for u in utrs:
            for K in Ks:
                for _ in range(restarts):
                    a, b, w, ka = self.sampler.init_job(self.preps[u], K)
                    out.append(self.engine._Job(u, K, fixed, a, b, w, ka[:self.nround].copy()))
        return out

    def call(self, pj, env):
        old_n = self.engine.N_ROUND
        self.engine.N_ROUND = self.nround
        keys = set(NARROW) | set(env)
        saved = {k: os.environ.get(k) for k in keys}
        os.environ.update(NARROW)
        os.environ.update(env)
        try:
            out = [np.array(x).copy() for x in self.batch.em_packed(pj)]
            launches = self.batch.em_traffic()["launches"]
        finally:
            self.engine.N_ROUND = old_n
            for k, v in saved.items():
                if v is None:
                    os.environ.pop(k, None)
                else:
                    os.environ[k] = v
        return out, launches

    def pack(self, jobs):
        old_n = self.engine.N_ROUND
        self.engine.N_ROUND = self.nround
        try:
            return self.engine.pack_jobs(jobs)
        finally:
            self.engine.N_ROUND = old_n

    def compare(self, jobs, variants=VARIANTS):
        """Runs the jobs at depth 1 and in every variant; asserts bit equality; returns (depth-1 outputs, launches by name)."""
        pj = self.pack(jobs)
        base, n1 = self.call(pj, {"SCAPE_HIP_EM_DEPTH": "1"})
        ao, bo, wo, bic, nlb, lb = base
        assert np.all((nlb >= 1) & (nlb <= self.nround))
        for i, j in enumerate(jobs):                       # the depth-1 run is a sane fit, not garbage that happens to agree
            assert np.all((ao[i, :j.K] >= 0) & (ao[i, :j.K] < self.preps[j.u].T)) and np.isfinite(bic[i])
            assert abs(wo[i, :j.K + 1].sum() - 1.0) < 1e-9 and np.all(np.isfinite(lb[i, :nlb[i]]))
        launches = {"depth 1": n1}
        for name, env in variants:
            got, n = self.call(pj, env)
            launches[name] = n
            for what, x, y in zip(("alpha_idx", "beta_idx", "ws", "bic", "n_lb", "lb_arr"), base, got):
                same = x.tobytes() == y.tobytes()
                if not same:
                    rows = np.nonzero([x[i].tobytes() != y[i].tobytes() for i in range(len(x))])[0]
                    raise AssertionError(f"{name}: {what} differs from depth 1 in {len(rows)} of {len(x)} jobs, first rows "
                                         f"{rows[:8].tolist()} (K {[jobs[r].K for r in rows[:8]]}, n_lb {nlb[rows[:8]].tolist()})")
        print(f"[run-ahead] {len(jobs)} jobs, M-step launches: {launches}")
        return base, launches

    def close(self):
        self.batch.free()
        self.ctx.close()


@pytest.fixture(scope="module")
def bench():
    b = _Bench()
    yield b
    b.close()


def test_library_depth_matches_source():
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scape_amd", "csrc",
                            "em_lockstep.inc")).read()
    assert f"#define EM_DEPTH {LIB_DEPTH}\n" in src


def test_k1_k2_degenerate_to_one_round_per_pass(bench):
    """K = 1 and K = 2: every round depends on the one before (same or adjacent component), so the schedule is the
    depth-1 schedule and the call takes the same number of M-step launches."""
    jobs = bench.jobs((1, 2), restarts=4)
    for j in jobs:
        assert all(len(g) == 1 for g in passes(j.k_arr, j.K, bench.nround, LIB_DEPTH))
    _, launches = bench.compare(jobs)
    assert launches["default depth, k4_mstep"] == launches["depth 1"] == launches["default depth, k3_mstep"]


def test_k3(bench):
    """K = 3: components 0 and 2 are independent, 1 depends on both."""
    jobs = bench.jobs((3,), restarts=6)
    assert any(len(g) == 2 for j in jobs for g in passes(j.k_arr, 3, bench.nround, LIB_DEPTH))
    assert not any(len(g) > 2 for j in jobs for g in passes(j.k_arr, 3, bench.nround, LIB_DEPTH))
    bench.compare(jobs)


@pytest.mark.parametrize("K", (6, 10, 12))
def test_column_classes(bench, K):
    """K = 6, 10, 12: the 8-, 12- and 16-column classes.  K = 10 must also need fewer M-step launches than depth 1."""
    jobs = bench.jobs((K,), restarts=4)
    base, launches = bench.compare(jobs)
    nlb = base[4]
    need = {d: max(len(passes(j.k_arr, K, int(n), d)) for j, n in zip(jobs, nlb)) for d in (1, LIB_DEPTH)}
    print(f"[run-ahead] K = {K}: launches the slowest job needs: depth 1 {need[1]}, depth {LIB_DEPTH} {need[LIB_DEPTH]}")
    if K == 10:
        assert launches["default depth, k4_mstep"] < launches["depth 1"]
        assert launches["default depth, k3_mstep"] < launches["depth 1"]


def test_k20_generic_body(bench):
    """One call with K = 20: the generic body of the 24-column kernel."""
    bench.compare(bench.jobs((20,), utrs=(0, 1), restarts=3))


@pytest.mark.parametrize("nround", (7, 8))
def test_round_cap_inside_and_on_the_edge_of_a_group(nround):
    """nround 7 and 8 at depth 3: the round cap falls inside a run-ahead group and on its edge.  The jobs' component
    order is set by hand - (0, 2, 4 | 1, 3, 5 | 0, 2 ...): groups of three rounds - so that the cap's place is known."""
    b = _Bench(nround=nround)
    try:
        jobs = b.jobs((6,), restarts=4)
        order = np.array([0, 2, 4, 1, 3, 5, 0, 2, 4, 1], np.int8)[:nround]
        for j in jobs[::2]:
            j.k_arr = order.copy()
        groups = passes(order, 6, nround, LIB_DEPTH)
        assert [len(g) for g in groups] == ([3, 3, 1] if nround == 7 else [3, 3, 2])
        base, _ = b.compare(jobs)
        assert np.any(base[4][::2] == nround)          # some hand-ordered job runs into the cap
    finally:
        b.close()


def test_stop_in_the_middle_of_a_group(bench):
    """At least one job meets the stopping rule in a round that is not the last of its run-ahead group."""
    jobs = bench.jobs((5, 6), restarts=8)
    base, _ = bench.compare(jobs)
    mid = 0
    for j, n in zip(jobs, base[4]):
        if n < bench.nround:                            # stopped by the rule; the groups as they would have gone on
            grp = next(g for g in passes(j.k_arr, j.K, bench.nround, LIB_DEPTH) if n - 1 in g)
            mid += (n - 1) != grp[-1]
    print(f"[run-ahead] {mid} of {len(jobs)} jobs stop in the middle of a group")
    assert mid >= 1


def test_mixed_fixed_and_ordinary(bench):
    """Fixed-inference jobs (one round per pass, no column) beside ordinary ones."""
    jobs = bench.jobs((3, 6), restarts=3) + bench.jobs((3, 6), restarts=3, fixed=True)
    base, _ = bench.compare(jobs[::2] + jobs[1::2])
    assert np.all(base[4] >= 2)


def test_crowded_utr(bench):
    """One UTR carries 40 jobs of K = 5 that start from the same alphas and walk (0, 2, 4 | 1, 3 | ...): in the first
    pass the columns of components 0 and 2 of EVERY job cover the tile that holds alpha_1 - 80 columns, more than the
    64 of one M-step pass."""
    from scape_amd.engine import _Job
    u, K = 1, 5
    q = bench.preps[u]
    a0, _, _, _ = bench.sampler.init_job(q, K)
    jobs = []
    for _ in range(40):
        _, b, w, ka = bench.sampler.init_job(q, K)
        ka = ka.copy()
        ka[:5] = (0, 2, 4, 1, 3)
        jobs.append(_Job(u, K, False, a0.copy(), b, w, ka))
    B, rows = len(q.betas), 64
    cover = np.zeros((q.T * B + rows - 1) // rows, int)
    for j in jobs:
        first = passes(j.k_arr, K, bench.nround, LIB_DEPTH)[0]
        assert first == [0, 1, 2]
        for r in first:
            c = int(j.k_arr[r])
            lo = 0 if c == 0 else int(j.a_idx[c - 1])
            hi = q.T - 1 if c == K - 1 else int(j.a_idx[c + 1])
            cover[lo * B // rows:((hi + 1) * B - 1) // rows + 1] += 1
    assert cover.max() > 64, cover.max()
    bench.compare(jobs)


def test_rescue_job(bench):
    """The one-bin UTR: components that take no responsibility make `Z[:,k] += 1e-8` fire (apa_core.py:528-529)."""
    bench.compare(bench.jobs((3, 5), utrs=(3,), restarts=4) + bench.jobs((3,), utrs=(0,), restarts=2))
