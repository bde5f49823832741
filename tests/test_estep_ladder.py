"""The E-step's values on the GPU at their boundary shapes, against the long-double reference and its derived bounds.

Every case of tests/estep_ladder.py (tests/test_host.py checks the ladder against the constants of the sources,
tests/test_estep_reference.py its conditions and the bounds themselves on the CPU) is loaded on a handle of its own with
the case's nround and built; the DEVICE'S OWN tensor is fetched and oracle/mstep_reference.py evaluated on it, so that
the rounding of the tensor build is out of the comparison.  The case's conditions are asserted again on that tensor
(near == 0, every listed wrong E-step moves the answer by more than the bounds, the bounds under their caps).  Every
call of the case then runs in the five shapes of estep_ladder.SHAPES - only fixed jobs (k2_estep_all_rounds), mixed with
a non-fixed companion on another UTR at run-ahead depth 1 and 3 (k2_estep), with the 4-wavefront E-step where the call
has at most 16 columns (k2_estep_cs), and without the shrink - and per job:
  - nlb is the reference's exactly; alpha and beta come back as they went in;
  - every ws[c], every lb[i] and bic lie within fit.ws_bound / lb_bound / bic_bound (first order, MARGIN = 2);
  - all shapes, and all calls that hold the job, return identical bits.
Mismatches are collected and reported together.

Largest bounds of the ladder (tests/test_estep_reference.py prints them; the caps are 1e-10 / 1e-14 / 1e-12 / 1e-12):
ws 2.8e-12 relative for weights >= 1e-4 (rounds5, K = 3 after 5 rounds) and 7.1e-17 absolute below, lb 3.9e-13, bic
3.4e-13 relative (rounds20, K = 8); the counts family (cnt up to 1000) is held to its own bound and exempt from the caps.

Measured on an MI355X (printed by every run; measurements, not targets): worst observed / bound per column class, the
same in k2_estep, k2_estep_all_rounds and (up to 16 columns) k2_estep_cs, whose bits are equal:
    class    ws        lb        bic             class    ws        lb        bic
    < 4>     0.144     0.0202    0.0534          <24>     0.0643    0.00765   0.00573
    < 8>     0.0608    0.00552   0.00573         <32>     0.0643    0.00765   0.00573
    <12>     0.0643    0.00566   0.00545         <64>     0.0643    0.00765   0.00573
    <16>     0.0397    0.00176   0
The extended tests/test_mstep_ladder.py (non-fixed jobs, counts up to 60) reaches 0.275.  The module takes about 1.2 s.

What the bound can and cannot see.  Scratch builds with one change each (never committed), this module's 15 tests and
the 12 of test_mstep_ladder.py, failures and the largest observed / bound:
  `1.0 / 24` -> `1.0 / 23` in d_exp_nonpos            5 fail (bins, tight, columns; window, ring)     ws 2.3
  Lg3 of d_log_pos 2.857142...e-01 -> 2.857152...e-01  3 fail (bins, tight, zero), lb alone moves       lb 1.7
  d_rcp_mid with one Newton step instead of two       0 fail: invisible - bits change (<4>: lb 0.0202 -> 0.0511, bic 0.0534 -> 0.107),
                                                      but one step already brings v_rcp_f64 to within the 2 ulp the chain allows
  the rescue's `z[c] += 1e-8` -> `1.0000001e-8`        12 fail (rescue, cap05, zero; 9 of the M-step ladder)   lb, bic 1.2e7
  `arg >= -746.0` -> `arg >= -700.0`                   1 fail (liveness: "one lane live")               ws 2.7e6
  `- 0.5 * x2 * x2` dropped from ls2                  0 fail: invisible, as expected - x2 is 1e-8 with the rescue, the term 5e-17 pk
                                                      per bin against a bound of some 1e-11 on lb, and a few u squared without it
  the bins' `if (n < N)` widened to `n < Np`          13 fail (rescue, cap05, zero; 10 of the M-step ladder): the padding bins'
                                                      1 / C enters sum Z_k and the rescue no longer fires       lb 6e13
So the bound sees a wrong exp or log coefficient only in its tightest cases and at about twice the bound - the observed
error of a correct kernel is 1 / 7 of it at best - and sees every wrong constant, cut or loop end by orders of magnitude.
The `log(s2)` branch of estep_body (|s2 - 1| >= 1e-5) is not reached by any ladder job and cannot be by any input: s2 is
1 within (2 K + 3) u, or 1 + 1e-8 with the rescue (tests/test_estep_reference.py asserts the ladder's largest |s2 - 1|).
"""
import os

import numpy as np
import pytest

import estep_ladder as el

pytestmark = pytest.mark.gpu
CASES = el.cases()
BY_NAME = {c.name: c for c in CASES}
_WORST = {}                                       # (kernel, column class, quantity) -> worst observed / bound


class _Loaded:
    """One ladder case on a library handle of its own, loaded with the case's nround and built."""

    def __init__(self, case):
        from scape_amd import _lib, engine
        self.case, self.engine = case, engine
        self.ctx = _lib.Context(0)
        old = engine.N_ROUND
        engine.N_ROUND = case.nround              # HipBatch takes the call's round cap from here
        try:
            self.batch = engine.HipBatch(self.ctx, case.preps)
            self.batch.build()
        finally:
            engine.N_ROUND = old
        self.M = [self.batch.fetch_tensor(u) for u in range(len(case.preps))]

    def call(self, jobs, env):
        e = self.engine
        old_n, saved = e.N_ROUND, {k: os.environ.pop(k, None) for k in el.KNOBS}
        e.N_ROUND = self.case.nround
        os.environ.update(env)
        try:
            pj = e.pack_jobs([e._Job(j.u, j.K, j.fixed, j.a_idx, j.b_idx, j.ws, j.k_arr) for j in jobs])
            return pj, [np.array(x).copy() for x in self.batch.em_packed(pj)]
        finally:
            e.N_ROUND = old_n
            for k in el.KNOBS:
                os.environ.pop(k, None)
                if saved[k] is not None:
                    os.environ[k] = saved[k]

    def close(self):
        self.batch.free()
        self.ctx.close()


def _bits(pj, out, i):
    ao, bo, wo, bic, nlb, lb = out
    K, n = int(pj.jk[i]), int(nlb[i])
    return (ao[i, :K].tobytes(), bo[i, :K].tobytes(), wo[i, :K + 1].tobytes(), bic[i].tobytes(), n, lb[i, :n].tobytes())


@pytest.fixture(scope="module", autouse=True)
def _summary():
    yield
    if _WORST:
        print("\n[estep ladder] worst observed / bound per (kernel, column class): ws | lb | bic")
        for kernel, cls in sorted({k[:2] for k in _WORST}):
            print(f"  {kernel:<20s} <{cls:>2d}>  " + " | ".join(f"{_WORST.get((kernel, cls, qn), 0.0):.3g}" for qn in ("ws", "lb", "bic")))


@pytest.mark.parametrize("name", [c.name for c in CASES])
def test_estep_ladder_case(name):
    case = BY_NAME[name]
    ld = _Loaded(case)
    try:
        _run_case(case, ld)
    finally:
        ld.close()


def _run_case(case, ld):
    problems = []
    # ---- the reference on the device's tensor; the ladder's conditions again
    fits = []
    for i, job in enumerate(case.jobs):
        pr, fit = el.check_job(case, case.preps[job.u], ld.M[job.u], job)
        fits.append(fit)
        problems += [(case.name, "conditions on the device's tensor", i, job.note) + tuple(p) for p in pr]
    # ---- every call, every shape
    first_bits, kernels, worst = {}, set(), {}
    calls = case.calls or (tuple(range(len(case.jobs))),)
    for call in calls:
        for shape, with_companion, env in el.SHAPES:
            jobs = [case.jobs[i] for i in call] + ([case.companion] if with_companion else [])
            sel = el.selection(env, jobs)
            kernels.add(sel["kernel"])
            pj, out = ld.call(jobs, env)
            ao, bo, wo, bic, nlb, lb = out
            for row, i in enumerate(call):
                job, fit, K = case.jobs[i], fits[i], case.jobs[i].K
                tag = (case.name, f"call {list(call) if len(call) < 6 else len(call)}", shape, sel["kernel"], i, job.note)
                bits = _bits(pj, out, row)
                if first_bits.setdefault(i, (tag, bits))[1] != bits:
                    problems.append(tag + ("bits differ from", first_bits[i][0][1:4]))
                if not (np.array_equal(ao[row, :K], job.a_idx[fit.order]) and np.array_equal(bo[row, :K], job.b_idx[fit.order])):
                    problems.append(tag + ("alpha / beta of a fixed job moved", ao[row, :K].tolist(), bo[row, :K].tolist()))
                if int(nlb[row]) != len(fit.lb):
                    problems.append(tag + ("rounds", int(nlb[row]), len(fit.lb)))
                    continue
                obs = dict(ws=float(np.max(np.abs(wo[row, :K + 1] - fit.ws) / fit.ws_bound)),
                           lb=float(np.max(np.abs(lb[row, :len(fit.lb)] - fit.lb) / fit.lb_bound)),
                           bic=abs(float(bic[row]) - fit.bic) / fit.bic_bound)
                for qn, r in obs.items():
                    print_key = (sel["kernel"], sel["cls"], qn)
                    worst[print_key] = max(worst.get(print_key, 0.0), r)
                    if not r <= 1:
                        got = dict(ws=wo[row, :K + 1].tolist(), lb=lb[row, :len(fit.lb)].tolist(), bic=float(bic[row]))[qn]
                        want = dict(ws=fit.ws.tolist(), lb=fit.lb.tolist(), bic=fit.bic)[qn]
                        problems.append(tag + (f"{qn} outside its bound: observed / bound", r, got, want))
    for key, r in worst.items():
        _WORST[key] = max(_WORST.get(key, 0.0), r)
    print(f"\n[estep ladder] {case.name}: {len(case.jobs)} jobs, {len(calls)} calls x {len(el.SHAPES)} shapes; worst observed / bound "
          + ", ".join(f"{qn} {max(r for k, r in worst.items() if k[2] == qn):.3g}" for qn in ("ws", "lb", "bic")) + f"; kernels {sorted(kernels)}")
    small = any(max(1, max(case.jobs[i].K for i in call)) + 1 <= el.ml.WIDE_MAX_COLUMNS for call in calls)
    assert kernels == {"k2_estep", "k2_estep_all_rounds"} | ({"k2_estep_cs"} if small else set())
    assert not problems, f"{len(problems)} mismatches\n" + "\n".join(repr(p) for p in problems[:40])
