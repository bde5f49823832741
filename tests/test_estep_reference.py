"""The E-step bounds of oracle/mstep_reference.py and the ladder of tests/estep_ladder.py, checked on the CPU.

On the C oracle's tensor every ladder job must meet the ladder's conditions (near == 0; every listed perturbation moves
ws, lb or bic by more than the two runs' bounds; outside the counts family the bounds stay under their caps), and the C
oracle's own so_em_algo - f64, library exp and log, true divisions, numpy's pairwise sums: an independent implementation
in another summation order - must lie within the new bounds on every job, with the same number of rounds.  Each named
wrong E-step is checked against a two-bin example worked out by hand.  tests/test_estep_ladder.py runs the same cases on
the GPU.

Printed by the run (measurements): the largest bounds outside the counts family are ws 2.8e-12 relative (weights >= 1e-4)
and 7.1e-17 absolute below, lb 3.9e-13, bic 3.4e-13 relative; the oracle's largest observed / bound is ws 0.16, lb 0.035,
bic 0.053.
"""
import numpy as np
import pytest

import estep_ladder as el
from oracle import mstep_reference as mr

CASES = el.cases()
BY_NAME = {c.name: c for c in CASES}
_WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _summary():
    yield
    if _WORST:
        cap = [v for k, v in _WORST.items() if BY_NAME[k].capped]
        print("\n[estep reference] largest bounds outside the counts family: ws %.2g relative, %.2g absolute below 1e-4, lb %.2g, bic %.2g"
              % tuple(max(v["bounds"][i] for v in cap) for i in range(4)))
        print("[estep reference] the C oracle's largest observed / bound: ws %.2g, lb %.2g, bic %.2g"
              % tuple(max(v["oracle"][i] for v in _WORST.values()) for i in range(3)))


@pytest.mark.parametrize("name", [c.name for c in CASES])
def test_ladder_case_meets_its_conditions_and_holds_the_c_oracle(oracle, name):
    case = BY_NAME[name]
    problems, bounds, seen = [], [0.0] * 4, [0.0] * 3
    for i, job in enumerate(case.jobs):
        q = case.preps[job.u]
        M = el.oracle_tensor(q)
        pr, fit = el.check_job(case, q, M, job)
        problems += [(name, i, job.note) + tuple(p) for p in pr]
        bounds = [max(a, b) for a, b in zip(bounds, el.rel_bounds(fit))]
        got = el.run_oracle(q, M, job, case.nround)
        assert np.array_equal(got["a"], job.a_idx[fit.order]) and np.array_equal(got["b"], job.b_idx[fit.order])    # fixed: nothing moves
        if len(got["lb"]) != len(fit.lb):
            problems.append((name, i, job.note, "rounds", len(got["lb"]), len(fit.lb)))
            continue
        obs = (float(np.max(np.abs(got["ws"][:job.K + 1] - fit.ws) / fit.ws_bound)),
               float(np.max(np.abs(got["lb"] - fit.lb) / fit.lb_bound)), abs(got["bic"] - fit.bic) / fit.bic_bound)
        seen = [max(a, b) for a, b in zip(seen, obs)]
        if not max(obs) <= 1:
            problems.append((name, i, job.note, "the C oracle outside the bound: ws, lb, bic observed / bound", obs))
    _WORST[name] = dict(bounds=bounds, oracle=seen)
    print(f"\n[estep ladder, CPU] {name}: {len(case.jobs)} jobs; largest bounds ws {bounds[0]:.2g} rel / {bounds[1]:.2g} abs, lb {bounds[2]:.2g}, "
          f"bic {bounds[3]:.2g}; C oracle observed / bound ws {seen[0]:.2g}, lb {seen[1]:.2g}, bic {seen[2]:.2g}")
    assert not problems, f"{len(problems)} problems\n" + "\n".join(repr(p) for p in problems[:30])


def _facts(name):
    case = BY_NAME[name]
    out = []
    for job in case.jobs:
        q = case.preps[job.u]
        M = el.oracle_tensor(q)
        fit = el.run_reference(q, M, job, case.nround)
        out.append((job, q, fit, el.facts(q, M, job, fit)))
    return out


def test_ladder_cases_sit_on_their_boundaries(oracle):
    """What the constructions promise: which bins and columns are live, where the rescue and the cap fire, which jobs stop."""
    # bins, tight, columns, rounds: plain E-steps - no rescue, every bin with a live component
    for name in ("bins", "tight", "columns", "rounds2", "rounds5", "rounds10", "rounds20"):
        for job, q, fit, f in _facts(name):
            assert not any(f["rescue"]) and (job.K == 0 or f["all_sent_bins"] == 0), (name, job.note)
    assert [q.N for q in BY_NAME["bins"].preps[:-1]] == list(el.N_BINS) and all(j.K == 2 for j in BY_NAME["bins"].jobs)
    for job, q, fit, f in _facts("bins"):
        assert {v for _n, v in job.perturb} == {b for b in (0, 63, 64, q.N - 1) if b < q.N}
    assert all(q.cnt.max() <= 2 for n in ("bins", "tight", "columns", "rounds20") for q in BY_NAME[n].preps)
    assert [j.K for j in BY_NAME["columns"].jobs] == list(el.K_COLUMNS)
    # liveness: finite (not sentinel) entries below the cut, group by group
    live = {job.note: (job, q, f) for job, q, _fit, f in _facts("liveness")}
    job, q, f = live["dead everywhere"]
    assert f["fin"][:, 1].sum() > 20 and not f["live"][:, 1].any() and f["n_groups"] == 2
    job, q, f = live["group 0 dead, bin 64 live"]
    assert f["dead_groups"][1] == [0] and f["live"][64, 1] and f["fin"][:64, 1].sum() > 10
    job, q, f = live["one lane live"]
    (n,) = np.nonzero(f["live"][:, 1])[0]
    assert n < 64 and f["fin"][:, 1].sum() > 20 and -745.0 < f["arg"][n, 1] < -700.0
    assert np.all(f["arg"][f["fin"][:, 1] & ~f["live"][:, 1], 1] < -760.0)
    job, q, f = live["last group dead"]
    assert f["dead_groups"][1] == [1] and f["fin"][64, 1] and f["live"][:64, 1].sum() > 5
    for job, q, f in live.values():                                  # none of the cut's neighbours: [-746, -745.13] holds no argument
        a = f["arg"][f["fin"]]
        assert not np.any((a >= -747.0) & (a <= -745.0)), job.note
    # rescue
    r = {job.note: (job, fit, f) for job, _q, fit, f in _facts("rescue")}
    assert r["all sentinel"][2]["rescue"] == [True, True] and not r["all sentinel"][2]["fin"][:, 0].any()
    job, fit, f = r["live, far below"]
    assert f["rescue"][0] and f["fin"][:, 1].all() and float(fit.rounds[0].v.sum()) < 1e-6 and abs(fit.lb[0]) < 1e6
    assert r["far above"][2]["rescue"] == [False, False] and all(len(x[1].lb) == 2 for x in r.values())
    # cap
    c = {job.note: (fit, f) for job, _q, fit, f in _facts("cap")}
    assert c["above"][1]["capped"] == [True] and c["above"][0].ws[-1] == 0.15 and not c["above"][1]["rescue"][0]
    assert c["below"][1]["capped"] == [False] and c["below"][0].ws[-1] < 0.1
    c = {job.note: (fit, f) for job, _q, fit, f in _facts("cap05")}
    assert c["above"][1]["capped"] == [True] and c["above"][0].ws[-1] == 0.5 and BY_NAME["cap05"].preps[0].p["max_unif_ws"] == 0.5
    fit, f = c["below 0.5, above 0.15"]
    assert f["capped"] == [False] and 0.2 < fit.ws[-1] < 0.45
    # zero weights: the column stays dead (or is rescued when it is the updated one)
    z = {job.note: (job, fit, f) for job, _q, fit, f in _facts("zero")}
    assert z["component"][1].ws[1] == 0.0 and not z["component"][2]["fin"][:, 1].any()
    assert z["uniform"][1].rounds[0].ws[-1] == 0.0 and z["uniform"][2]["all_sent_bins"] == 0
    assert z["updated"][2]["rescue"][0] and abs(z["updated"][1].lb[0]) > 1e29           # 1e-8 cnt (SENT + SENT)
    # sentinel rows
    for job, q, fit, f in _facts("sentinel"):
        assert f["all_sent_bins"] >= 5 and f["one_finite_bins"] >= 5, job.note
    # counts
    assert set(BY_NAME["counts1"].preps[0].cnt.tolist()) == set(el.COUNTS) and not BY_NAME["counts1"].capped
    # rounds: nround = 2, K + 2 and 20; one job stops at round 1, one early, one runs to the cap; no stop is near (condition 1)
    assert {(c.nround, j.K) for c in CASES if c.family == 10 for j in c.jobs} == {(2, 3), (2, 8), (5, 3), (10, 8), (20, 3), (20, 8), (20, 0)}
    n20 = {job.K: f["nlb"] for job, _q, _fit, f in _facts("rounds20")}
    assert n20[0] == 2 and 2 < n20[3] < 20 and n20[8] == 20, n20
    for name in ("rounds5", "rounds10"):
        for job, q, fit, f in _facts(name):
            assert f["nlb"] == job.K + 2 and list(job.k_arr[:job.K + 1]) == list(range(job.K)) + [0]
    # log s2: no ladder job leaves the series (|s2 - 1| < 1e-5) - the rescue moves s2 by 1e-8 and nothing else moves it
    x2 = max(r.x2 for c in CASES for _job, _q, fit, _f in _facts(c.name) for r in fit.rounds)
    assert 0.99e-8 < x2 < 1.01e-8 < el.LS2_SERIES
    # every named wrong E-step is some job's (cap_inclusive cannot move a value: at equality the cap is the identity)
    named = {p for c in CASES for j in c.jobs for p, _v in j.perturb}
    assert named == set(mr.E_PERTURBATIONS) - {"cap_inclusive"}, named ^ set(mr.E_PERTURBATIONS)


# ---------------------------------------------------------------------------------------------------------------------
# two bins, one component, by hand: M = [log 1/2, log 1/8], unif_ll = log 1/4, ws = (1/2, 1/2), cnt = (1, 2)
#   bin 0: z = (1/4, 1/8)       -> Z = (2/3, 1/3)          bin 1: z = (1/16, 1/8)^2 -> Z = (1/5, 4/5)
#   ws = (2/3 + 2/5, 1/3 + 8/5) / 3 = (16/45, 29/45)
def _hand(ws=(0.5, 0.5), k_arr=(1,), nround=1, cap=1.0, M=(0.5, 0.125), **kw):
    Mt = np.log(np.array(M, np.float64)).reshape(1, 1, 2)
    return mr.em_rounds(Mt, np.array([1.0, 2.0]), float(np.log(0.25)), np.array([100.0]), np.array([5.0]), 2000.0, 100.0, cap,
                        np.array([0]), np.array([0]), np.array(ws), np.array(k_arr), nround, fixed=True, **kw)


def _h(*p):
    p = np.array(p)
    return float(-(p * np.log(p)).sum())


def test_each_wrong_estep_does_what_its_name_says():
    lg = np.log
    base = _hand()
    ell = 2 / 3 * lg(1 / 4) + 1 / 3 * lg(1 / 8) + 2 * (1 / 5 * lg(1 / 16) + 4 / 5 * lg(1 / 8))
    ent = _h(2 / 3, 1 / 3) + 2 * _h(1 / 5, 4 / 5)
    assert np.allclose(base.ws, [16 / 45, 29 / 45], rtol=1e-14) and base.lb[0] == pytest.approx(ell + ent, rel=1e-14)
    assert base.bic == pytest.approx(-2 * ell + 4 * lg(2), rel=1e-14) and base.near == 0 and not base.rounds[0].capped
    assert np.all(base.ws_bound < 1e-14) and base.lb_bound[0] < 1e-13 and base.bic_bound < 1e-13
    # untempered: bin 1 without its count in the exponent, Z = (1/3, 2/3)
    f = _hand(untempered=True)
    assert np.allclose(f.ws, [(2 / 3 + 2 / 3) / 3, (1 / 3 + 4 / 3) / 3], rtol=1e-14)
    # e_drop_bin: bin 1 in no sum; the BIC's log N keeps N = 2
    f = _hand(e_drop_bin=1)
    e0 = 2 / 3 * lg(1 / 4) + 1 / 3 * lg(1 / 8)
    assert np.allclose(f.ws, [2 / 3, 1 / 3], rtol=1e-14) and f.lb[0] == pytest.approx(e0 + _h(2 / 3, 1 / 3), rel=1e-14)
    assert f.bic == pytest.approx(-2 * e0 + 4 * lg(2), rel=1e-14)
    # e_drop_col: the component takes no part, the uniform column takes every read
    f = _hand(e_drop_col=0)
    assert f.ws.tolist() == [0.0, 1.0] and f.lb[0] == pytest.approx(3 * lg(0.5 * 0.25), rel=1e-14)
    # the cap: 29/45 > 1/2
    f = _hand(cap=0.5)
    assert f.rounds[0].capped and f.ws.tolist() == [0.5, 0.5]
    f = _hand(cap=0.5, no_cap=True)
    assert not f.rounds[0].capped and np.allclose(f.ws, base.ws, rtol=0, atol=0)
    # cap_inclusive: equal columns give ws = (1/2, 1/2) exactly; > leaves it, >= caps it (to the same values)
    eq = dict(M=(0.25, 0.25), cap=0.5)
    f, g = _hand(**eq), _hand(cap_inclusive=True, **eq)
    assert f.ws.tolist() == [0.5, 0.5] == g.ws.tolist() and not f.rounds[0].capped and g.rounds[0].capped and f.near == 1
    # exp_zero: a cut at -1/2 kills log(1/2) (bin 0, the uniform column) and 2 log(1/2) (bin 1, the component)
    f = _hand(exp_zero=-0.5)
    assert np.allclose(f.ws, [1 / 3, 2 / 3], rtol=1e-14) and f.lb[0] == pytest.approx(lg(1 / 4) + 2 * lg(1 / 8), rel=1e-14)
    # zero_weight_as_tiny: a weight of 0 is the sentinel (Z = 0 exactly); as log 1e-300 it leaves exp(-690) in bin 0
    f, g = _hand(ws=(0.0, 1.0)), _hand(ws=(0.0, 1.0), zero_weight_as_tiny=True)
    assert f.ws.tolist() == [0.0, 1.0] and 0 < g.ws[0] == pytest.approx(1e-300 * 0.5 / 0.25 / 3, rel=1e-12)
    # the rescue: sum Z_0 ~ 1e-30 < 1e-8
    eps = 1e-8
    r = _hand(ws=(1e-30, 1.0), k_arr=(0,))
    assert r.rounds[0].rescue and r.ws[0] == pytest.approx(3 * eps / (3 + 3 * eps), rel=1e-9)
    f = _hand(ws=(1e-30, 1.0), k_arr=(0,), no_rescue=True)
    assert not f.rounds[0].rescue and f.ws[0] < 1e-29
    f = _hand(ws=(1e-30, 1.0), k_arr=(0,), rescue_once=True)
    assert f.rounds[0].rescue and f.ws[0] == r.ws[0] and r.lb[0] - f.lb[0] == pytest.approx(3 * eps * (1 - lg(eps)), rel=1e-3)
    f = _hand(ws=(1e-30, 1.0), k_arr=(0,), entropy_plain=True)
    assert f.ws[0] == r.ws[0] and r.lb[0] - f.lb[0] == pytest.approx(3 * eps, rel=1e-3)
    # fresh_columns: round 1 of (0, 0) sees the uniform column's log-weight of the init; refreshed, it is a first round from ws_1
    two, fresh = _hand(k_arr=(0, 0), nround=2), _hand(k_arr=(0, 0), nround=2, fresh_columns=True)
    again = _hand(ws=tuple(two.rounds[0].ws.astype(np.float64)), k_arr=(0,))
    assert two.lb[0] == fresh.lb[0] and fresh.lb[1] == pytest.approx(again.lb[0], rel=1e-14) and abs(two.lb[1] - fresh.lb[1]) > 1e-3


def test_bounds_follow_the_chain():
    """The bounds grow with what the chain says they grow with, and an input weight carries no error."""
    one = _hand()
    assert one.rounds[0].ws_bound.shape == (2,) and one.lb_bound.shape == (1,)
    capped = _hand(cap=0.5)
    assert capped.ws_bound[1] <= mr.U * 0.5 * 1.0001 + 1e-300          # the cap value: only the reference's own rounding
    assert capped.ws_bound[0] > one.ws_bound[0] * 0.5                   # the renormalised weight keeps its error
    two = _hand(k_arr=(0, 0), nround=2)
    assert two.lb_bound[1] > two.lb_bound[0] and np.all(two.ws_bound > two.rounds[0].ws_bound)
    # the output sort permutes the bound with the weights
    Mt = np.log(np.array([[[0.5, 0.125]], [[0.25, 0.25]]]))
    f = mr.em_rounds(Mt, np.array([1.0, 2.0]), float(np.log(0.25)), np.array([100.0, 109.0]), np.array([5.0]), 2000.0, 100.0, 0.9,
                     np.array([1, 0]), np.array([0, 0]), np.array([0.3, 0.3, 0.4]), np.array([0]), 1, fixed=True)
    assert f.order.tolist() == [1, 0] and np.array_equal(f.ws_bound[:2], f.rounds[0].ws_bound[:2][::-1])
    assert np.array_equal(f.ws[:2], f.rounds[0].ws[:2].astype(np.float64)[::-1])
    # near: an exp argument at the cut, a row maximum that is itself a sentinel
    assert _hand(M=(0.5, 0.25 * np.exp(mr.EXP_ZERO / 2))).near == 1
