"""The grid arg-max M-step on the GPU at its boundary shapes, against the long-double reference.

Every case of tests/mstep_ladder.py (tests/test_host.py checks the ladder against the constants of the sources,
tests/test_mstep_reference.py its conditions on the CPU) is loaded with the case's nround - 1 almost everywhere: an EM
call then returns the arg-max of exactly one M-step launch - and built; the DEVICE'S OWN tensor is fetched and
oracle/mstep_reference.py evaluated on it, so that the rounding of the tensor build is out of the comparison.  The
case's conditions are asserted again on that tensor (every round decided or an exact tie by design; every listed
perturbation a different, decided row).  The job table then runs through every form of mstep_ladder.FORMS - k2_mstep,
k3_mstep and k4_mstep, a tile's columns cut into passes of 16 and kept whole, run-ahead depth 1 and 3 on k2_estep, and
once the 4-wavefront E-step - and per job:
  - the updated component's (alpha_idx, beta_idx) is the reference's winning row EXACTLY (the first of an exact tie);
    the other components are where they were;
  - in the random family an undecided job must return a row whose long-double score is within the two bounds of the maximum;
  - ws, bic, lb meet the per-call tolerances against the long-double values (ws rtol 1e-6 / atol 1e-10, bic 1e-9, lb 1e-9);
  - ws, bic, lb of the decided jobs lie within the reference's derived bounds (fit.ws_bound / lb_bound / bic_bound: the
    E-step chain of oracle/mstep_reference.py, some 1e5 times sharper than the tolerances; tests/test_estep_ladder.py);
  - all forms, and all calls that hold the job, return identical bits.
Mismatches are collected and reported together.

Measured on an MI355X (printed by every run; measurements, not targets): worst |device ws - reference| / tolerance
9.9e-8 in every form (the forms are bit-equal); smallest decided gap / bound on the device's tensors 5.08e6 (case
"bins"; the random family 1.39e7 with 4 of its 240 jobs undecided); worst observed / E-step bound over ws, lb and bic of
the decided jobs 0.275 (random family; 0.12 elsewhere); the module takes about 3.5 s.

What the ladder found: the tie case "tiles of extent 0 and 16" failed in all eleven forms before k2_estep's reduction
over the tiles learned the all-sentinel floor (em_lockstep.inc: rd_fl) - the rows of a dead component's window are tied
exactly, a tile below its finite extent summed the sentinel terms by the MFMA chain, a tile beyond it from the suffix
sums, the two rounded differently and the later tile won (alpha index 80 where the reference and the oracle give 0).
Scratch builds with one comparison or term changed (never committed) fail this module's 12 tests as follows:
`row < hi` -> `row < hi - B` in the epilogue (then written out in each kernel, now mstep_best_of_rows of mstep.inc):
3 (extent, window, random); the `SENT * tl` term dropped from c0 (mstep_c0): 8; `>` -> `>=` in the merge across
wavefronts (mstep_merge_waves): 1 (ties); rd_n1 published one bin short by k2_estep: 4 (bins,
columns, rounds2, random).
"""
import os

import numpy as np
import pytest

import mstep_ladder as ml

pytestmark = pytest.mark.gpu
CASES = ml.cases()
BY_NAME = {c.name: c for c in CASES}
WS_RTOL, WS_ATOL, BIC_TOL, LB_TOL = 1e-6, 1e-10, 1e-9, 1e-9
KNOBS = ("SCAPE_HIP_MSTEP", "SCAPE_HIP_SPLIT_MAXTILES", "SCAPE_HIP_EM_DEPTH", "SCAPE_HIP_WIDE_MAXJOBS")


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
        old_n, saved = e.N_ROUND, {k: os.environ.pop(k, None) for k in KNOBS}
        e.N_ROUND = self.case.nround
        os.environ.update(env)
        try:
            pj = e.pack_jobs([e._Job(j.u, j.K, False, j.a_idx, j.b_idx, j.ws, j.k_arr) for j in jobs])
            return pj, [np.array(x).copy() for x in self.batch.em_packed(pj)]
        finally:
            e.N_ROUND = old_n
            for k in KNOBS:
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


_MEASURED = {}


@pytest.fixture(scope="module", autouse=True)
def _summary():
    yield
    if _MEASURED:
        print("\n[mstep ladder] worst |device ws - reference| / tolerance per form, over all cases:")
        forms = sorted({f for d in _MEASURED.values() for f in d["ws"]})
        for f in forms:
            print(f"  {f:<36s} {max(d['ws'].get(f, 0.0) for d in _MEASURED.values()):.3g}")
        print(f"[mstep ladder] smallest decided gap / bound on the device's tensors: {min(d['ratio'] for d in _MEASURED.values()):.3g}")
        print(f"[mstep ladder] worst observed / E-step bound (ws, lb, bic of the decided jobs): {max(d['bound'] for d in _MEASURED.values()):.3g}")


@pytest.mark.parametrize("name", [c.name for c in CASES])
def test_mstep_ladder_case(name):
    case = BY_NAME[name]
    ld = _Loaded(case)
    try:
        _run_case(case, ld)
    finally:
        ld.close()


def _run_case(case, ld):
    problems, worst_ratio = [], np.inf
    # ---- the reference on the device's tensor; conditions 1 and 2 again
    fits, undecided = [], []
    for i, job in enumerate(case.jobs):
        q, M = case.preps[job.u], ld.M[job.u]
        pr, ratio, fit = ml.check_job(q, M, job, case.nround)
        fits.append(fit)
        if pr and case.random:
            undecided.append(i)
            continue
        problems += [(case.name, "conditions on the device's tensor", i, job.note) + tuple(p) for p in pr]
        worst_ratio = min(worst_ratio, ratio)
    if case.random:
        print(f"\n[mstep ladder] {case.name}: {len(undecided)} of {len(case.jobs)} jobs undecided on the device's tensor {undecided}")
        assert len(undecided) * 20 <= len(case.jobs)
    # ---- every call, every form
    ws_worst, first_bits, kernels, bound_worst = {}, {}, set(), 0.0
    for n in case.calls or (len(case.jobs),):
        jobs = case.jobs[:n]
        for form, env in ml.FORMS:
            sel = ml.selection(env, jobs, case.preps)
            kernels.add((sel["kernel"], sel["job_split"], sel["depth"], sel["wide"]))
            pj, out = ld.call(jobs, env)
            ao, bo, wo, bic, nlb, lb = out
            for i, job in enumerate(jobs):
                q, fit, K, tag = case.preps[job.u], fits[i], job.K, (case.name, f"call of {n}", form, i, job.note)
                bits = _bits(pj, out, i)
                if first_bits.setdefault(i, (tag, bits))[1] != bits:
                    problems.append(tag + ("bits differ from", first_bits[i][0][1:3]))
                a, b = ao[i, :K], bo[i, :K]
                if i in undecided:
                    r, k = fit.rounds[0], int(job.k_arr[0])
                    got_row = int(a[k]) * len(q.betas) + int(b[k])
                    rest = np.arange(K) != k
                    if not (r.within(got_row) and np.array_equal(a[rest], job.a_idx[rest]) and np.array_equal(b[rest], job.b_idx[rest])):
                        problems.append(tag + ("undecided job: row outside the bounds of the maximum", got_row, r.row))
                elif not (np.array_equal(a, fit.a_idx) and np.array_equal(b, fit.b_idx)):
                    problems.append(tag + ("alpha / beta", a.tolist(), fit.a_idx.tolist(), b.tolist(), fit.b_idx.tolist(),
                                           "ties", len(fit.rounds[0].ties)))
                elif case.nround == 1:
                    rest = np.arange(K) != int(job.k_arr[0])
                    if not (np.array_equal(a[rest], job.a_idx[rest]) and np.array_equal(b[rest], job.b_idx[rest])):
                        problems.append(tag + ("another component moved", a.tolist(), job.a_idx.tolist()))
                w = wo[i, :K + 1]
                dev = float(np.max(np.abs(w - fit.ws) / (WS_ATOL + WS_RTOL * np.abs(fit.ws))))
                ws_worst[form] = max(ws_worst.get(form, 0.0), dev)
                if not dev <= 1:
                    problems.append(tag + ("ws", float(np.max(np.abs(w - fit.ws)))))
                if int(nlb[i]) != len(fit.lb):
                    problems.append(tag + ("rounds", int(nlb[i]), len(fit.lb)))
                elif not np.allclose(lb[i, :nlb[i]], fit.lb, rtol=LB_TOL, atol=0):
                    problems.append(tag + ("lb", lb[i, :nlb[i]].tolist(), fit.lb.tolist()))
                if not abs(float(bic[i]) - fit.bic) <= BIC_TOL * abs(fit.bic):
                    problems.append(tag + ("bic", float(bic[i]), fit.bic))
                # the E-step's derived bounds (oracle/mstep_reference.py), where the reference's rows are the device's
                if i not in undecided and int(nlb[i]) == len(fit.lb):
                    obs = (float(np.max(np.abs(w - fit.ws) / fit.ws_bound)), float(np.max(np.abs(lb[i, :nlb[i]] - fit.lb) / fit.lb_bound)),
                           abs(float(bic[i]) - fit.bic) / fit.bic_bound)
                    bound_worst = max(bound_worst, max(obs))
                    if not max(obs) <= 1:
                        problems.append(tag + ("ws, lb, bic outside the E-step bounds: observed / bound", obs))
    _MEASURED[case.name] = dict(ws=ws_worst, ratio=worst_ratio, bound=bound_worst)
    print(f"\n[mstep ladder] {case.name}: {len(case.jobs)} jobs, calls {case.calls or (len(case.jobs),)}, {len(ml.FORMS)} forms; "
          f"smallest decided gap / bound {worst_ratio:.3g}; worst |ws - reference| / tolerance {max(ws_worst.values()):.3g}; "
          f"worst observed / E-step bound {bound_worst:.3g}; kernels {sorted(kernels)}")
    assert {k[0] for k in kernels} == {"k2_mstep", "k3_mstep", "k4_mstep"} and {k[3] for k in kernels} == {False, True}
    assert not problems, f"{len(problems)} mismatches\n" + "\n".join(repr(p) for p in problems[:40])
