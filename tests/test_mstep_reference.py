"""oracle/mstep_reference.py and the ladder of tests/mstep_ladder.py, checked on the CPU against the C oracle.

The long-double rounds must reproduce so_em_algo (alpha, beta and the number of rounds exactly; ws, bic, lb to the
project's per-call tolerances) at nround = 1, 2 and 3 on the ladder's UTRs, and the ladder must meet its conditions on
the oracle's tensor: every round of every ladder job decided (or an exact tie by design), every listed perturbation a
different, decided row, every case on the boundary it names.  tests/test_mstep_ladder.py runs the same cases on the GPU.

Printed by the run (a measurement): ladder jobs left out 0; random family 4 of 240 undecided (at most 12 may be); the
smallest decided gap / bound on the oracle's tensor 5.1e6.
"""
import numpy as np
import pytest

import mstep_ladder as ml
from oracle import mstep_reference as mr

CASES = ml.cases()
BY_NAME = {c.name: c for c in CASES}
WS_TOL, BIC_TOL, LB_TOL = dict(rtol=1e-6, atol=1e-10), 1e-9, 1e-9


def _tensors(case):
    return [ml.oracle_tensor(q) for q in case.preps]


def _longer(job, nround):
    """The job with its component order continued round-robin to `nround` rounds."""
    ka = np.array([job.k_arr[i] if i < len(job.k_arr) else (int(job.k_arr[-1]) + i - len(job.k_arr) + 1) % job.K
                   for i in range(nround)], np.int8)
    return ml.dataclass_replace(job, k_arr=ka)


@pytest.mark.parametrize("nround", (1, 2, 3))
def test_long_double_rounds_reproduce_the_c_oracle(oracle, nround):
    """Every ladder UTR, up to 40 jobs of each case: so_em_algo and the long-double rounds from the same init.  A job
    whose rounds are not all decided in the reference (an arg-max inside the rounding of f64) is counted, not compared."""
    problems, compared, skipped = [], 0, 0
    for case in CASES:
        Ms = _tensors(case)
        for i, job in enumerate(case.jobs[:40]):
            q, M, j = case.preps[job.u], Ms[job.u], _longer(job, nround)
            fit = ml.run_reference(q, M, j, nround)
            if fit.near or not all(r.decided for r in fit.rounds):
                skipped += 1
                continue
            got = ml.run_oracle(q, M, j, nround)
            compared += 1
            tag = (case.name, i, nround)
            if not (np.array_equal(got["a"], fit.a_idx) and np.array_equal(got["b"], fit.b_idx)):
                problems.append(tag + ("alpha / beta", got["a"].tolist(), fit.a_idx.tolist(), got["b"].tolist(), fit.b_idx.tolist()))
            if len(got["lb"]) != len(fit.lb):
                problems.append(tag + ("rounds", len(got["lb"]), len(fit.lb)))
                continue
            if not np.allclose(got["ws"][:job.K + 1], fit.ws, **WS_TOL):
                problems.append(tag + ("ws", float(np.max(np.abs(got["ws"][:job.K + 1] - fit.ws)))))
            if not abs(got["bic"] - fit.bic) <= BIC_TOL * abs(fit.bic):
                problems.append(tag + ("bic", got["bic"], fit.bic))
            if not np.allclose(got["lb"], fit.lb, rtol=LB_TOL):
                problems.append(tag + ("lb", got["lb"].tolist(), fit.lb.tolist()))
    print(f"\n[mstep reference] nround {nround}: {compared} jobs compared with so_em_algo, {skipped} with an undecided round left out")
    assert compared >= 250 and skipped <= compared // 10
    assert not problems, f"{len(problems)} mismatches\n" + "\n".join(repr(p) for p in problems[:30])


@pytest.mark.parametrize("name", [c.name for c in CASES if not c.random])
def test_ladder_case_meets_its_conditions(oracle, name):
    """Conditions 1 and 2 on the oracle's tensor, no job left out; the facts a job's note names (`key=value`, the
    kernels' view of its first M-step) hold; a case with cols_keep has a mover in every 16 jobs."""
    case = BY_NAME[name]
    Ms = _tensors(case)
    problems, worst, moved = [], np.inf, []
    for i, job in enumerate(case.jobs):
        q, M = case.preps[job.u], Ms[job.u]
        pr, ratio, fit = ml.check_job(q, M, job, case.nround)
        worst = min(worst, ratio)
        problems += [(name, i, job.note) + tuple(p) for p in pr]
        f = ml.facts(q, M, job, fit.rounds[0])
        k = int(job.k_arr[0])
        moved.append(fit.rounds[0].row != int(job.a_idx[k]) * len(q.betas) + int(job.b_idx[k]))
        if "=" in job.note and not job.note.startswith("N="):
            key, val = job.note.split("=")
            if f[key] != int(val):
                problems.append((name, i, job.note, "is", f[key]))
        if job.note.startswith(("hi_mod", "n_tiles", "first")) and not f["hi_clipped"]:
            problems.append((name, i, job.note, "the winner is not clipped at the upper end"))
        if job.note.startswith("lo_mod") and not f["lo_clipped"]:
            problems.append((name, i, job.note, "the winner is not clipped at the lower end"))
    print(f"\n[mstep ladder, CPU] {name}: {len(case.jobs)} jobs, 0 left out, smallest decided gap / bound {worst:.3g}")
    if case.cols_keep is not None:
        for lo in range(case.cols_keep, len(case.jobs), 16):
            assert any(moved[lo:lo + 16]), (name, "jobs", lo, "to", lo + 15, "all stay at their init: a dropped pass would pass")
    assert not problems, f"{len(problems)} problems\n" + "\n".join(repr(p) for p in problems[:30])


def test_ladder_cases_sit_on_their_boundaries(oracle):
    """What the constructions promise beyond the notes: the extents under one window, the tail and the no-tail branch,
    the tie sets and where they lie, the partial last tile, the windows of B rows, the run of the round cases."""
    def first_rounds(name):
        case = BY_NAME[name]
        Ms = _tensors(case)
        out = []
        for job in case.jobs:
            q, M = case.preps[job.u], Ms[job.u]
            fit = ml.run_reference(q, M, job, case.nround)
            out.append((job, q, M, fit, ml.facts(q, M, job, fit.rounds[0])))
        return out
    # extents: 0 (the low tiles of the bins UTRs), Np and strictly between under one K = 1 window
    bins = BY_NAME["bins"]
    exts = [ml.tile_extents(M) for M in _tensors(bins)]
    assert any(e[0] == 0 for e in exts) and all(e[-1] == (q.N + 15) // 16 * 16 for e, q in zip(exts, bins.preps))
    assert len({q.T for q in bins.preps}) > 1 and bins.preps[7].L > 2000          # unequal T: tiles_max above a UTR's own count
    e33 = ml.tile_extents(_tensors(BY_NAME["extent"])[0])
    assert sorted(set(e33.tolist())) == [16, 32, 48]
    for job, q, M, fit, f in first_rounds("extent"):
        v, r = fit.rounds[0].v.astype(np.float64), fit.rounds[0]
        tails = [t for t in range(f["first_tile"], f["last_tile"] + 1) if v[e33[t]:].sum() != 0]
        if job.note == "inside":
            assert not tails and not f["rescue"] and f["n_tiles"] >= 3
        elif job.note == "tail":
            assert tails and len({int(e33[t]) for t in tails}) >= 2
        else:
            assert f["tail"] and 0 < f["win_ext"] < 48, f
    # supports: disjoint ones, ends in three different half-chunks
    sup = [(f["n0"], f["n1"]) for *_x, f in first_rounds("support")[:len(ml.SUPPORT)]]
    assert any(a1 <= b0 for _a0, a1 in sup for b0, _b1 in sup) and len({(n1 - 1) // 16 for _n0, n1 in sup}) == 3
    # windows
    for job, q, M, fit, f in first_rounds("window"):
        if job.note == "one16":
            assert f["group16"] and f["rd_hi"] - f["rd_lo"] == len(q.betas)
        if job.note == "two16":
            assert not f["group16"] and f["rd_hi"] - f["rd_lo"] == len(q.betas)
        if job.note == "last_partial":
            assert f["last_partial"] and int(job.k_arr[0]) == job.K - 1 and f["rd_hi"] == q.T * len(q.betas)
        if job.note == "first":
            assert int(job.k_arr[0]) == 0 and f["rd_lo"] == 0
    # ties
    want = {"one tile": ([0], [0]), "two tiles of extent 0": ([0, 1], [0]), "three tiles": ([0, 1, 2], [0])}
    for job, q, M, fit, f in first_rounds("ties"):
        r = fit.rounds[0]
        assert f["rescue"] and r.row == 0 and len(r.ties) == len(r.rows) > 1, job.note
        if job.note in want:
            assert (f["tie_tiles"], f["tie_exts"]) == want[job.note], (job.note, f["tie_tiles"], f["tie_exts"])
        else:
            assert f["tie_exts"] == [0, 16] and f["tie_tiles"] == list(range(11)), (f["tie_tiles"], f["tie_exts"])
    # rounds
    (job, q, M, fit, f), = first_rounds("rounds3")
    assert len(fit.rounds) == 3 and [r.k for r in fit.rounds] == [0, 2, 4] and job.K == 5
    (job, q, M, fit, f), = first_rounds("rounds2")
    assert len(fit.rounds) == 2 and fit.rounds[0].row != fit.rounds[1].row and job.K == 1
    # every named perturbation is some job's
    named = {p for c in CASES for j in c.jobs for p, _v in j.perturb}
    assert named == set(mr.PERTURBATIONS), named ^ set(mr.PERTURBATIONS)


def test_random_family_leaves_out_at_most_one_job_in_twenty(oracle):
    """Condition 4: the random family may have undecided jobs, at most 1 in 20; the counts are printed."""
    case = BY_NAME["random"]
    Ms = _tensors(case)
    und, worst = [], np.inf
    for i, job in enumerate(case.jobs):
        pr, ratio, _fit = ml.check_job(case.preps[job.u], Ms[job.u], job, 1)
        if pr:
            und.append(i)
        else:
            worst = min(worst, ratio)
    print(f"\n[mstep ladder, CPU] random family: {len(case.jobs)} jobs, {len(und)} undecided {und}, smallest decided gap / bound {worst:.3g}")
    assert len(case.jobs) == 240 and len(und) * 20 <= len(case.jobs)
    assert [q.N for q in case.preps] == list(ml.RANDOM_N) and {j.K for j in case.jobs} == set(range(1, 9))


def test_each_perturbation_changes_the_reference(oracle):
    """A perturbation must be a different computation, not a flag that is ignored: on a case built for it the scores,
    the window or the winner change; without it the reference is the oracle's (the test above)."""
    w = BY_NAME["window"]
    Ms = _tensors(w)
    job = next(j for j in w.jobs if j.note == "hi_mod=0")
    q, M = w.preps[job.u], Ms[job.u]
    base = ml.run_reference(q, M, job, 1).rounds[0]
    B = len(q.betas)
    hi = ml.run_reference(q, M, job, 1, hi_exclusive=True).rounds[0]
    lo = ml.run_reference(q, M, job, 1, lo_exclusive=True).rounds[0]
    assert len(hi.rows) == len(lo.rows) == len(base.rows) - B
    assert hi.rows[-1] == base.rows[-1] - B and lo.rows[0] == base.rows[0] + B and hi.row != base.row
    cut = ml.run_reference(q, M, job, 1, rows_to=int(base.rows[0]) + 5).rounds[0]
    assert len(cut.rows) == 5 and cut.row < base.rows[0] + 5
    none = ml.run_reference(q, M, job, 1, rows_to=0)
    assert none.rounds[0].row == -1 and np.array_equal(none.a_idx, job.a_idx)
    e = BY_NAME["extent"]
    job = e.jobs[0]
    q, M = e.preps[0], _tensors(e)[0]
    base = ml.run_reference(q, M, job, 1).rounds[0]
    z = ml.run_reference(q, M, job, 1, sentinel_as_zero=True).rounds[0]
    assert z.row != base.row and float(np.max(z.score - base.score)) > 1e20
    d = ml.run_reference(q, M, job, 1, drop_bin=base.n0).rounds[0]
    assert not np.array_equal(d.score, base.score)
    t = BY_NAME["ties"]
    job = t.jobs[0]
    q, M = t.preps[0], _tensors(t)[0]
    base = ml.run_reference(q, M, job, 1).rounds[0]
    last = ml.run_reference(q, M, job, 1, last_max=True).rounds[0]
    assert base.row == base.ties[0] and last.row == base.ties[-1] != base.row
