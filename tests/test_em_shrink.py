"""EM shrink: late in a call the E-step job list, the M-step's UTR list and both grids are cut down to what is live.

At every fourth pass the host driver (em_rounds, scape_hip.hip) reads how many jobs are finalised and how many each UTR
has left; when few enough are live, k_em_shrink (em_lockstep.inc) compacts the job list (jobs at status 2 leave; a job
at status 1 stays until its finalising E-step has run) and the UTR list, and the later launches run over the shorter
lists, a smaller M-step grid and only the run-ahead slots the live jobs can use.  That is placement only, so every
case runs the same job tables with SCAPE_HIP_EM_SHRINK=0 and with SCAPE_HIP_EM_SHRINK_AT=100 (shrink at every probe
that finds anything finished), through k3_mstep (the default for these small calls), k4_mstep
(SCAPE_HIP_SPLIT_MAXTILES=0) and k2_mstep (SCAPE_HIP_MSTEP=v2), and asserts byte equality of alpha_idx, beta_idx, ws,
bic, n_lb and all of lb_arr, and equal M-step launch counts.  SCAPE_HIP_WIDE_MAXJOBS=0 keeps the calls on k2_estep.

The shrink events themselves are checked against a model: from the n_lb of the run without shrink and the schedule rule
(passes, as in test_em_run_ahead.py) follows the pass in which each job is finalised, hence what is live at each probe,
and the library's trace lines (SCAPE_HIP_ROUND_TRACE: pass, jobs listed -> live, UTRs listed -> live, slots) must say
the same.  So an identity is never a run in which nothing shrank.
"""
import os
import re

import numpy as np
import pandas as pd
import pytest

pytestmark = pytest.mark.gpu

NARROW = {"SCAPE_HIP_WIDE_MAXJOBS": "0"}
OFF = {"SCAPE_HIP_EM_SHRINK": "0"}
ON = {"SCAPE_HIP_EM_SHRINK_AT": "100", "SCAPE_HIP_ROUND_TRACE": "1"}
PATHS = (                                      # (name, environment on top of NARROW)
    ("k3_mstep", {}),
    ("k4_mstep", {"SCAPE_HIP_SPLIT_MAXTILES": "0"}),
    ("k2_mstep", {"SCAPE_HIP_MSTEP": "v2"}),
)
DEPTH = 3                                      # EM_DEPTH of the library (test_em_run_ahead.py checks it against the source)
PROBE = 4                                      # the driver probes after passes 3, 7, 11, ...
TRACE = re.compile(r"\[shrink\] pass (\d+) jobs (\d+) -> (\d+) utrs (\d+) -> (\d+) slots (\d+)")


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


def slots_needed(max_k, depth=DEPTH):
    """The slots rule restated (em_slots_needed): K <= 2 never runs ahead, K = 3 only over the pair (0, 2)."""
    return min(depth, 1 if max_k <= 2 else 2 if max_k == 3 else depth)


def expected_events(jobs, nlb, nround):
    """(pass, jobs listed, live, UTRs listed, live, slots) of every shrink at threshold 100, and per job the pass whose
    first E-step launch finalises it.  A job that ran n rounds ran them in passes 0 .. p - 1 and is finalised in pass p."""
    fin = np.array([len(passes(j.k_arr, j.K, int(n), DEPTH, j.fixed)) for j, n in zip(jobs, nlb)])
    listed_j, listed_u, events = len(jobs), len({j.u for j in jobs}), []
    for r in range(PROBE - 1, nround, PROBE):
        if not np.any(fin - 1 > r - PROBE):         # no round ran since the last probe: the call ends here
            break
        live = fin > r
        live_j, live_u = int(live.sum()), len({j.u for j, a in zip(jobs, live) if a})
        if live_j and (live_j < listed_j or live_u < listed_u):
            max_k = max([j.K for j, a in zip(jobs, live) if a and not j.fixed], default=0)
            events.append((r, listed_j, live_j, listed_u, live_u, slots_needed(max_k)))
            listed_j, listed_u = live_j, live_u
    return events, fin


def _one_bin_df():
    n = 120
    return pd.DataFrame({"x": np.full(n, 400, np.int64), "l": np.full(n, 98, np.int64), "r": np.full(n, np.nan),
                         "pa": np.full(n, np.nan), "cb_id": np.arange(n), "read_id": np.arange(n)})


class _Bench:
    """Synthetic UTRs of 300-500 reads and, last, a single-bin one, on a library handle of its own."""

    def __init__(self, n_syn=9, nround=None):
        from scape_amd import _lib, engine
        from scape_amd.host import Sampler, prepare_utr
        from scape_amd.synth import synth_utr
        self.engine = engine
        self.nround = engine.N_ROUND if nround is None else nround
        items = [synth_utr(i, 300 + (200 * i) // max(1, n_syn - 1), k_cap=5, base_seed=5200, pa_rate=0.05, r_rate=0.05)
                 for i in range(n_syn)]
        dfs = [df for _, df, *_ in items] + [_one_bin_df()]
        names = [g for g, *_ in items] + ["syn:ONEBIN:1:1-2000:+"]
        self.preps = [prepare_utr(df, gene_info_str=g) for df, g in zip(dfs, names)]
        self.one_bin = n_syn
        self.tiles = [(p.T * len(p.betas) + 63) // 64 for p in self.preps]
        self.Sampler = Sampler
        self.ctx = _lib.Context(0)
        old = engine.N_ROUND
        engine.N_ROUND = self.nround            # HipBatch takes the call's round cap from here
        try:
            self.batch = engine.HipBatch(self.ctx, self.preps)
            self.batch.build()
        finally:
            engine.N_ROUND = old

    def jobs(self, seed, Ks, utrs, restarts=3, fixed=False):
        """Jobs drawn from a sampler of their own, so that a test's jobs do not depend on which tests ran before it."""
        sampler, out = self.Sampler(np.random.RandomState(20261020 + seed)), []
        for u in utrs:
            for K in Ks:
                for _ in range(restarts):
                    a, b, w, ka = sampler.init_job(self.preps[u], K)
                    out.append(self.engine._Job(u, K, fixed, a, b, w, ka[:self.nround].copy()))
        return out

    def call(self, pj, env):
        old_n = self.engine.N_ROUND
        self.engine.N_ROUND = self.nround
        keys = set(NARROW) | set(OFF) | set(ON) | set(env)
        saved = {k: os.environ.get(k) for k in keys}
        for k in keys:
            os.environ.pop(k, None)
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

    def compare(self, jobs, capfd):
        """Runs the jobs without and with the shrink on the three M-step paths; asserts bit equality, equal launch counts
        and the modelled shrink events; returns (outputs, events, pass that finalises each job)."""
        pj = self.pack(jobs)
        first = None
        for name, env in PATHS:
            capfd.readouterr()
            base, n_off = self.call(pj, {**env, **OFF})
            assert not TRACE.search(capfd.readouterr().err), f"{name}: SCAPE_HIP_EM_SHRINK=0 still shrinks"
            got, n_on = self.call(pj, {**env, **ON})
            seen = [tuple(int(x) for x in m) for m in TRACE.findall(capfd.readouterr().err)]
            ao, bo, wo, bic, nlb, lb = base
            assert np.all((nlb >= 1) & (nlb <= self.nround))
            for i, j in enumerate(jobs):                   # a sane fit, not garbage that happens to agree
                assert np.all((ao[i, :j.K] >= 0) & (ao[i, :j.K] < self.preps[j.u].T)) and np.isfinite(bic[i])
                assert abs(wo[i, :j.K + 1].sum() - 1.0) < 1e-9 and np.all(np.isfinite(lb[i, :nlb[i]]))
            for what, x, y in zip(("alpha_idx", "beta_idx", "ws", "bic", "n_lb", "lb_arr"), base, got):
                if x.tobytes() != y.tobytes():
                    rows = np.nonzero([x[i].tobytes() != y[i].tobytes() for i in range(len(x))])[0]
                    raise AssertionError(f"{name}: {what} differs with the shrink in {len(rows)} of {len(x)} jobs, first rows "
                                         f"{rows[:8].tolist()} (K {[jobs[r].K for r in rows[:8]]}, n_lb {nlb[rows[:8]].tolist()})")
            assert n_on == n_off, f"{name}: {n_on} M-step launches with the shrink, {n_off} without"
            events, fin = expected_events(jobs, nlb, self.nround)
            print(f"[shrink] {name}: {len(jobs)} jobs, {n_on} M-step launches, events {seen}")
            assert seen == events, f"{name}: shrink events {seen}, the model says {events}"
            if first is None:
                first = (base, events, fin)
            else:                                          # the three M-step kernels give the same bits
                assert all(x.tobytes() == y.tobytes() for x, y in zip(first[0], base)), name
        return first

    def close(self):
        self.batch.free()
        self.ctx.close()


@pytest.fixture(scope="module")
def bench():
    b = _Bench()
    yield b
    b.close()


def test_jobs_finish_many_passes_apart(bench, capfd):
    """K = 1 beside K = 2 and K = 10 in one call: the shrink drops jobs and, in the end, UTRs while others run on."""
    jobs = bench.jobs(1, (1, 2, 10), utrs=(0, 1, 2), restarts=3)
    _, events, fin = bench.compare(jobs, capfd)
    assert fin.max() - fin.min() >= 2 * PROBE
    assert any(e[2] < e[1] for e in events) and any(e[4] < e[3] for e in events), events


def _leaves_first(bench, capfd, gone, rest):
    """UTR `gone` carries K = 1 jobs only, the UTRs of `rest` K = 2 (one round per pass: slow) and K = 9: `gone` leaves
    the list at the first probe after its last job is finalised, while jobs of `rest` run on."""
    jobs = bench.jobs(2, (1,), utrs=(gone,), restarts=3) + bench.jobs(3, (2, 9), utrs=rest, restarts=3)
    _, events, fin = bench.compare(jobs, capfd)
    last = {u: max(int(f) for j, f in zip(jobs, fin) if j.u == u) for u in (gone,) + tuple(rest)}
    drop = next(e for e in events if e[0] >= last[gone])
    assert drop[4] < drop[3] and drop[4] >= 1 and drop[2] >= 1, (last, events)
    assert any(last[u] > drop[0] + PROBE for u in rest), (last, events)     # the shrunken lists serve a probe interval or more


def test_utr_with_most_tiles_leaves_first(bench, capfd):
    """The M-step grid's second factor (tiles of the largest live UTR) must fall with it."""
    order = sorted(range(bench.one_bin), key=lambda u: bench.tiles[u])
    assert bench.tiles[order[-1]] > bench.tiles[order[-2]] and bench.tiles[order[-1]] > 1
    _leaves_first(bench, capfd, order[-1], (order[0], order[1]))


def test_smallest_utr_leaves_first(bench, capfd):
    order = sorted(range(bench.one_bin), key=lambda u: bench.tiles[u])
    _leaves_first(bench, capfd, order[0], (order[-1], order[-2]))


def test_one_bin_utr_leaves_first(bench, capfd):
    _leaves_first(bench, capfd, bench.one_bin, (0, 1))


def test_live_utrs_cross_eight(bench, capfd):
    """Ten UTRs listed, then fewer than eight: k4_mstep and k2_estep map blocks to XCDs differently on either side."""
    jobs = bench.jobs(4, (1,), utrs=(1, 3, 5, 7, bench.one_bin), restarts=2) + bench.jobs(5, (6, 9), utrs=(0, 2, 4, 6, 8), restarts=2)
    _, events, _ = bench.compare(jobs, capfd)
    assert events[0][3] == 10 and any(e[3] >= 8 and 0 < e[4] < 8 for e in events), events


def test_odd_live_counts_and_a_single_live_job(bench, capfd):
    """Live jobs that are no multiple of 8 (the E-step grid is rounded up to one), and exactly one live job.  Jobs do not
    influence one another, so a first call tells when each candidate is finalised; the case keeps the one that runs
    longest and those that are done by the last probe before its end."""
    cand = bench.jobs(6, (1, 2, 3, 5), utrs=(0, 1, 2), restarts=2) + bench.jobs(7, (12,), utrs=(3,), restarts=2)
    out, _ = bench.call(bench.pack(cand), OFF)
    _, fin = expected_events(cand, out[4], bench.nround)
    top = int(np.argmax(fin))
    probe = max(r for r in range(PROBE - 1, bench.nround, PROBE) if r < fin[top])
    jobs = [j for i, j in enumerate(cand) if i == top or fin[i] <= probe]
    assert len(jobs) >= 4, fin.tolist()
    _, events, _ = bench.compare(jobs, capfd)
    assert any(e[2] % 8 for e in events), events
    assert events[-1][0] <= probe and events[-1][2] == 1, events


def test_job_at_status_one_when_the_lists_shrink(bench, capfd):
    """A job whose last round ran in the pass of a shrinking probe is at status 1 then (its arg-max is pending, the next
    pass finalises it): it must stay listed.  The model counts it live; equal outputs show that it was finished."""
    jobs = bench.jobs(8, (1, 2, 3, 4, 5, 6), utrs=(0, 1, 2, 3), restarts=2)
    _, events, fin = bench.compare(jobs, capfd)
    at_probe = {e[0] for e in events}
    pending = [int(f) for f in fin if f - 1 in at_probe]
    print(f"[shrink] {len(pending)} jobs at status 1 at a shrink (finalised in passes {sorted(set(pending))})")
    assert pending, (events, fin.tolist())


def test_mixed_fixed_and_ordinary(bench, capfd):
    """Fixed-inference jobs (one round per pass, no column) beside ordinary ones."""
    jobs = bench.jobs(9, (1, 3, 6), utrs=(0, 1, 2), restarts=2) + bench.jobs(10, (3, 6), utrs=(0, 1, 4), restarts=2, fixed=True)
    _, events, _ = bench.compare(jobs[::2] + jobs[1::2], capfd)
    assert events, "nothing shrank"


def test_deep_tail_of_k1_k2_jobs_runs_one_slot(bench, capfd):
    """K = 6 jobs that walk (0, 2, 4 | 1, 3, 5) run three rounds per pass and are done early; the K <= 2 jobs left, one
    round per pass, need one k2_estep slot."""
    fast = bench.jobs(11, (6,), utrs=(0, 1), restarts=2)
    for j in fast:
        j.k_arr = np.resize(np.array([0, 2, 4, 1, 3, 5], np.int8), bench.nround)
    jobs = fast + bench.jobs(12, (1, 2), utrs=(0, 1, 2, 3), restarts=4)
    _, events, _ = bench.compare(jobs, capfd)
    assert events and events[0][5] == DEPTH and events[-1][5] == 1, events


@pytest.mark.parametrize("nround", (7, 8))
def test_round_cap_between_two_probes_and_on_one(nround, capfd):
    """nround 7: the cap lies between the probes after passes 3 and 7; nround 8: the last M-step pass is a probe pass."""
    b = _Bench(n_syn=3, nround=nround)
    try:
        jobs = b.jobs(13, (1,), utrs=(0, 3), restarts=3) + b.jobs(14, (2, 6), utrs=(1, 2), restarts=3)
        base, events, fin = b.compare(jobs, capfd)
        assert np.any(base[4] == nround)               # some job runs into the cap
        assert events, "nothing shrank"
    finally:
        b.close()
