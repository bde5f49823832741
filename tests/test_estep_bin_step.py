"""The E-step's bin step, round state and suffix sums of v at the edges of the bin loop and of the in-register scan.

estep_body (em_lockstep.inc) walks the bins of a lane 64 apart behind a one-bin software pipeline, takes the component
of the round through a scalar register, and builds the suffix sums of v at 16-bin boundaries group by group of 64
bins, 8 groups (512 bins) per read-back.  The cases below put the padded bin count Np on both sides of each of those
strides and of twice the lane stride (N is Np itself or a few bins less, so that padding bins exist), run
K = 1 .. 15 components (every column class up to 16, the exact-K variants of each) with the round's component at 0,
at K - 1 and in between, and add a job whose first round takes the 1e-8 rescue, a UTR that mixes r-known reads and
pA-site reads with plain ones, and a fixed-inference job.  All jobs are non-fixed unless named otherwise: every round
publishes a column, so the suffix sums are read by the M-step.

Per job, in every path:
  - alpha and beta indices and the round count are exactly the C oracle's (oracle.scape_oracle, so_em_algo on the
    device's own tensor);
  - ws, lb and bic lie within the bounds tests/test_estep_ladder.py uses for the same quantities - ws_bound, lb_bound,
    bic_bound of oracle/mstep_reference.py, evaluated on the device's tensor - of the oracle's values;
  - the paths return identical bits: k2_estep at run-ahead depth 3 and depth 1, k2_estep_cs (4 wavefronts per job), and
    k2_estep in front of the k2_mstep reader (SCAPE_HIP_MSTEP=v2) against the default M-step - the two readers of the
    suffix sums.
Every seeded job is the one of seed 0 (one of seed 1: RESEED): on the C oracle's tensor the long-double reference of
each has no comparison within rounding of its threshold and every grid arg-max decided (checked on the CPU when the
cases were written); both are asserted again on the device's tensor.  There the C oracle itself lies within 0.07 of the bounds of the reference.
"""
import numpy as np
import pytest

import estep_ladder as el
from estep_ladder import ml

pytestmark = pytest.mark.gpu

NROUND = 4
NP_EDGES = {16: 11, 48: 48, 64: 61, 80: 80, 128: 125, 512: 512, 528: 523, 1024: 1024, 1040: 1029}      # Np -> N
K_LIST = (1, 2, 3, 5, 8, 10, 12, 15)
CLASSES = (4, 8, 12, 16)                          # one call per column class: the jobs of at most that many columns
A_RANGE = (20, 180)
SEED = 0
RESEED = {(0, 12): 1}                             # (UTR, K) -> seed: with seed 0 the 11-bin UTR's K = 12 job has an exact tie in round 1
PATHS = (("k2_estep, depth 3", dict(ml.NARROW, SCAPE_HIP_EM_DEPTH="3")),
         ("k2_estep, depth 1", dict(ml.NARROW, SCAPE_HIP_EM_DEPTH="1")),
         ("k2_estep_cs", {}),
         ("k2_estep, k2_mstep", dict(ml.NARROW, SCAPE_HIP_EM_DEPTH="3", SCAPE_HIP_MSTEP="v2")))


def _utrs():
    B8 = ml.betas_for(8)
    preps = [ml.make_utr(f"BS{Np}", N, 2100 + Np, B8, cnt_max=3) for Np, N in NP_EDGES.items()]
    # the rescue: every read end right of both alphas, column 0 all sentinel (mstep_ladder.dead_job)
    preps.append(ml.make_utr("BSrescue", 17, 517, B8, xlo=700, xhi=1500, cnt_max=2))
    # r-known and pA-site reads between plain ones
    q = ml.make_utr("BSmix", 61, 2161, B8, cnt_max=3)
    q.r[1::3] = 30.0
    q.pa[2::3] = q.x[2::3] + 250.0
    preps.append(q)
    return preps


def _job(q, u, K, k, seed):
    j = ml.random_job(q, K, np.random.RandomState(seed), u, NROUND, k, A_RANGE)
    return el.EJob(u, K, j.a_idx, j.b_idx, j.ws, j.k_arr, fixed=False, note=f"{q.gene_info_str.split(':')[1]} K={K} k={k}")


def _plan():
    """[(u, K, first component)] of the seeded jobs: three K per UTR, every K of K_LIST on at least three UTRs, its first
    component 0 the first time, K - 1 the second, K // 2 the third."""
    n, seen, plan = len(NP_EDGES), {}, []
    for u in range(n):
        for j in range(3):
            K = K_LIST[(u + 3 * j) % len(K_LIST)]
            t = seen[K] = seen.get(K, -1) + 1
            plan.append((u, K, (0, K - 1, K // 2)[t % 3]))
    return plan + [(n + 1, 3, 1), (n + 1, 5, 4)]


def _jobs(preps):
    n = len(NP_EDGES)
    jobs = [_job(preps[u], u, K, k, RESEED.get((u, K), SEED)) for u, K, k in _plan()]
    d = ml.dead_job(preps[n], 40, 1, u=n)
    jobs.append(el.EJob(n, 2, d.a_idx, d.b_idx, d.ws, np.zeros(NROUND, np.int8), fixed=False, tie=True, note="rescue"))
    f = _job(preps[3], 3, 3, 1, SEED)
    jobs.append(el.EJob(3, 3, f.a_idx, f.b_idx, f.ws, f.k_arr, fixed=True, note="fixed inference"))
    return jobs


def _reference(q, M, job):
    return ml.run_reference(q, M, job, NROUND, fixed=job.fixed)


def _conditions(fit, job):
    """What makes the job's answer a matter of arithmetic, not of rounding: [] if all hold."""
    problems = []
    if fit.near:
        problems.append(("a comparison within rounding of its threshold", fit.near))
    for i, r in enumerate(fit.rounds):
        if r.row >= 0 and not r.decided:
            problems.append((f"round {i} undecided", r.ratio))
        if r.row >= 0 and not job.tie and len(r.ties) > 1:
            problems.append((f"round {i}: exact ties", len(r.ties)))
    if not (np.all(np.isfinite(fit.ws)) and np.all(np.isfinite(fit.lb)) and np.isfinite(fit.bic)):
        problems.append(("the reference is not finite",))
    return problems


@pytest.fixture(scope="module")
def loaded():
    from test_estep_ladder import _Loaded
    preps = _utrs()
    case = el.ECase("bin_step", 0, "bin loop, scalar round state, in-register scan", preps, _jobs(preps), nround=NROUND)
    ld = _Loaded(case)
    fits, oracles = [], []
    for job in case.jobs:                       # the references, once, on the device's tensor
        q, M = preps[job.u], ld.M[job.u]
        fits.append(_reference(q, M, job))
        oracles.append(ml.run_oracle(q, M, job, NROUND, fixed=job.fixed))
    yield case, ld, fits, oracles
    ld.close()


def test_case_covers_the_edges():
    preps = _utrs()
    jobs = _jobs(preps)
    assert sorted({-(-q.N // 16) * 16 for q in preps[:len(NP_EDGES)]}) == sorted(NP_EDGES)
    assert {j.K for j in jobs} >= set(K_LIST)
    for K in K_LIST[1:]:
        firsts = {int(j.k_arr[0]) for j in jobs if j.K == K}
        assert 0 in firsts and K - 1 in firsts, (K, firsts)
    assert any(0 < int(j.k_arr[0]) < j.K - 1 for j in jobs)


@pytest.mark.parametrize("cls", CLASSES)
def test_bin_step_against_oracle_and_across_paths(loaded, cls):
    from test_estep_ladder import _bits
    case, ld, fits, oracles = loaded
    idx = [i for i, j in enumerate(case.jobs) if j.K + 1 <= cls]
    jobs = [case.jobs[i] for i in idx]
    assert max(j.K for j in jobs) + 1 > (0 if cls == 4 else cls - 4)          # the call runs the kernel of this class
    problems, first, worst = [], {}, dict(ws=0.0, lb=0.0, bic=0.0)
    for i in idx:
        problems += [(case.jobs[i].note, "conditions on the device's tensor") + tuple(p) for p in _conditions(fits[i], case.jobs[i])]
    rescued = [bool(fits[i].rounds[0].rescue) for i in idx]
    if cls == 4:
        assert any(rescued), "no job of the call takes the 1e-8 rescue"
    for path, env in PATHS:
        sel = el.selection(env, jobs)
        assert sel["kernel"] == ("k2_estep_cs" if path == "k2_estep_cs" else "k2_estep"), (path, sel)
        pj, out = ld.call(jobs, env)
        ao, bo, wo, bic, nlb, lb = out
        for row, i in enumerate(idx):
            job, fit, orc, K = case.jobs[i], fits[i], oracles[i], case.jobs[i].K
            tag = (f"<{cls}>", path, job.note)
            bits = _bits(pj, out, row)
            if first.setdefault(i, (path, bits))[1] != bits:
                problems.append(tag + ("bits differ from", first[i][0]))
            if int(nlb[row]) != len(orc["lb"]):
                problems.append(tag + ("rounds", int(nlb[row]), len(orc["lb"])))
                continue
            if not (np.array_equal(ao[row, :K], orc["a"]) and np.array_equal(bo[row, :K], orc["b"])):
                problems.append(tag + ("alpha / beta", ao[row, :K].tolist(), bo[row, :K].tolist(), orc["a"].tolist(), orc["b"].tolist()))
                continue
            n = len(orc["lb"])
            obs = dict(ws=float(np.max(np.abs(wo[row, :K + 1] - orc["ws"]) / fit.ws_bound)),
                       lb=float(np.max(np.abs(lb[row, :n] - orc["lb"]) / fit.lb_bound[:n])),
                       bic=abs(float(bic[row]) - orc["bic"]) / fit.bic_bound)
            for qn, r in obs.items():
                worst[qn] = max(worst[qn], r)
                if not r <= 1:
                    problems.append(tag + (f"{qn} outside its bound of the oracle: observed / bound", r))
    print(f"\n[bin step] <{cls}>: {len(jobs)} jobs x {len(PATHS)} paths; worst |device - oracle| / bound: "
          + ", ".join(f"{qn} {r:.3g}" for qn, r in worst.items()))
    assert not problems, f"{len(problems)} mismatches\n" + "\n".join(repr(p) for p in problems[:40])
