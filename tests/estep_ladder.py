"""The ladder of tests/test_estep_ladder.py and tests/test_estep_reference.py: tiny UTRs and FIXED jobs (no M-step: the
E-step chain alone) that put the bin count, the column count, the liveness cut, the rescue, the cap, zero weights,
sentinel rows, the counts, the round count and the shape of the call on both sides of every boundary of estep_body
(em_lockstep.inc) and of the four kernels that run it.  tests/test_host.py reads the boundaries from the sources and
checks the ladder against them.

UTRs come from mstep_ladder.make_utr (N is exactly what a case says, T is about 219); where a case needs particular
counts they are set on the UtrPrep after it is made.  The read ranges, alphas and weights below were chosen on the CPU
against the C oracle's tensor so that every case meets the conditions which tests/test_estep_reference.py checks again
on every run and tests/test_estep_ladder.py once more on the device's own tensor:
  1. near == 0: no comparison the device makes in f64 lies within rounding of its threshold;
  2. every perturbation a job lists - the wrong E-step its boundary is about (oracle/mstep_reference.py:
     E_PERTURBATIONS) - moves ws, lb or bic by more than the sum of the two runs' bounds;
  3. outside the counts family every job's bounds are at most WS_CAP relative (weights >= 1e-4; WS_CAP_ABS below) and
     LB_CAP relative for lb and bic: 1e-4 and 1e-3 of the per-call tolerances of the oracle comparisons.
"""
from dataclasses import dataclass

import numpy as np

import mstep_ladder as ml
from mstep_ladder import Job, make_utr, oracle_tensor          # noqa: F401  (the ladder's own vocabulary)

LANES = 64                                        # bins of a lane group: pinned to the source by tests/test_host.py
PITCH = 16                                        # Np = N rounded up to this
CLASSES = (4, 8, 12, 16, 24, 32, 64)              # EstepClasses; WideClasses are those up to WIDE_MAX_COLUMNS
EXACT_MAX = 16                                    # ESTEP_DISPATCH: one variant per exact K + 1 up to here, the generic body above
EXP_CUT = -746.0                                  # the wave-uniform liveness ballot
RESCUE = 1e-8
LS2_SERIES = 1e-5                                 # |s2 - 1| below this: log s2 by its series
WS_CAP, WS_CAP_ABS, LB_CAP = 1e-10, 1e-14, 1e-12
P05 = dict(ml.P0, max_unif_ws=0.5)
PS10 = dict(ml.P0, sigma_f=10)

N_BINS = (1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 257)
N_TIGHT = (1, 9, 17)
K_COLUMNS = (0, 1, 2, 3, 4, 7, 8, 11, 12, 15, 16, 23, 24, 31, 32, 63)
MIXED_KMAX = (16, 23, 31, 63)
COUNTS = (1, 2, 64, 1000)
SEED = 0                                          # of every seeded job: the first seed met the conditions in each family


@dataclass
class EJob(Job):
    fixed: bool = True


@dataclass
class ECase:
    name: str
    family: int
    boundary: str
    preps: list                        # the last one is the companion's UTR
    jobs: list
    nround: int = 1
    calls: tuple = ()                  # tuples of job indices, one per EM call; () = one call with all jobs
    capped: bool = True                # condition 3 applies (the counts family is exempt)

    @property
    def companion(self):
        """A non-fixed K = 1 job on the last UTR: it makes the call a mixed one (k2_estep, k2_estep_cs) and leaves
        kmax where it was.  Its own result is not asserted."""
        u = len(self.preps) - 1
        rs = np.random.RandomState(7)
        return EJob(u, 1, np.array([rs.randint(20, 150)], np.int32), np.array([3], np.int32), np.array([0.9, 0.1]),
                    np.zeros(self.nround, np.int8), fixed=False)


def _companion_utr(betas):
    return make_utr("Ecomp", 17, 917, betas, cnt_max=2)


def ejob(q, K, seed, u=0, nround=1, k=None, a_range=None, perturb=(), note="", order=None):
    """A fixed job from a seeded random init; order: the component order (default: round-robin from a random first)."""
    rs = np.random.RandomState(seed)
    if K == 0:
        return EJob(u, 0, np.zeros(0, np.int32), np.zeros(0, np.int32), np.array([ml.P0["max_unif_ws"]]), np.zeros(nround, np.int8),
                    perturb=tuple(perturb), note=note)
    j = ml.random_job(q, K, rs, u, nround, k, a_range)
    ka = j.k_arr if order is None else np.asarray(order, np.int8)
    return EJob(u, K, j.a_idx, j.b_idx, j.ws, ka, perturb=tuple(perturb), note=note)


def hand_job(K_a, b, ws, k_arr, u=0, perturb=(), note=""):
    a = np.asarray(K_a, np.int32)
    return EJob(u, len(a), a, np.asarray(b, np.int32), np.asarray(ws, np.float64), np.asarray(k_arr, np.int8), perturb=tuple(perturb), note=note)


def run_reference(q, M, job, nround, **perturb):
    return ml.run_reference(q, M, job, nround, fixed=job.fixed, **perturb)


def run_oracle(q, M, job, nround):
    return ml.run_oracle(q, M, job, nround, fixed=job.fixed)


def moved(base, other):
    """Which of ws, lb, bic differ between two Fits by more than the sum of their bounds (nan counts as moved)."""
    out = []
    if not np.all(np.abs(base.ws - other.ws) <= base.ws_bound + other.ws_bound):
        out.append("ws")
    if len(base.lb) != len(other.lb) or not np.all(np.abs(base.lb - other.lb) <= base.lb_bound + other.lb_bound):
        out.append("lb")
    if not abs(base.bic - other.bic) <= base.bic_bound + other.bic_bound:
        out.append("bic")
    return out


def rel_bounds(fit):
    """(largest relative ws bound over the weights >= 1e-4, largest absolute one below, relative lb, relative bic)."""
    big = fit.ws >= 1e-4
    ws_rel = float(np.max(fit.ws_bound[big] / fit.ws[big])) if big.any() else 0.0
    ws_abs = float(np.max(fit.ws_bound[~big])) if (~big).any() else 0.0
    return ws_rel, ws_abs, float(np.max(fit.lb_bound / np.abs(fit.lb))), fit.bic_bound / abs(fit.bic)


def check_job(case, q, M, job):
    """Conditions 1 to 3 for one job: (problems, the unperturbed Fit)."""
    fit = run_reference(q, M, job, case.nround)
    problems = []
    if fit.near:
        problems.append(("a comparison within rounding of its threshold", fit.near))
    if not (np.all(np.isfinite(fit.ws)) and np.all(np.isfinite(fit.lb)) and np.isfinite(fit.bic)):
        problems.append(("the reference is not finite",))
    for name, val in job.perturb:
        p = run_reference(q, M, job, case.nround, **{name: val})
        mv = moved(fit, p)
        want = ("ws", "lb") if name == "e_drop_bin" else ()
        if not mv or not set(want) <= set(mv):
            problems.append((f"{name}={val} moves only", mv))
    if case.capped:
        ws_rel, ws_abs, lb_rel, bic_rel = rel_bounds(fit)
        if not (ws_rel <= WS_CAP and ws_abs <= WS_CAP_ABS and lb_rel <= LB_CAP and bic_rel <= LB_CAP):
            problems.append(("a bound above its cap", ws_rel, ws_abs, lb_rel, bic_rel))
    return problems, fit


def facts(q, M, job, fit):
    """What round 0 of a job looks like to estep_body, restated in f64 from the tensor and the init (not from the
    reference's internals): per (bin, column) sentinel / finite, the exp argument, and what follows from them."""
    K, C, N = job.K, job.K + 1, q.N
    w = np.asarray(job.ws, np.float64)
    lw = np.where(w > 0, np.log(np.where(w > 0, w, 1.0)), ml.SENT)
    lz = np.empty((N, C))
    fin = np.ones((N, C), bool)
    for c in range(K):
        row = M[job.a_idx[c], job.b_idx[c]]
        lz[:, c] = lw[c] + row
        fin[:, c] = (row != ml.SENT) & (w[c] > 0)
    lz[:, K] = lw[K] + q.unif_ll
    fin[:, K] = w[K] > 0
    arg = (lz - lz.max(axis=1, keepdims=True)) * q.cnt[:, None].astype(np.float64)
    live = fin & (arg >= EXP_CUT)
    grp = np.arange(N) // LANES
    dead_groups = {c: [int(g) for g in range(grp.max() + 1) if not live[grp == g, c].any()] for c in range(C)}
    return dict(arg=arg, fin=fin, live=live, dead_groups=dead_groups, n_groups=int(grp.max()) + 1,
                all_sent_bins=int((~fin[:, :K]).all(axis=1).sum()) if K else 0,
                one_finite_bins=int((fin[:, :K].sum(axis=1) == 1).sum()) if K else 0,
                rescue=[r.rescue for r in fit.rounds], capped=[r.capped for r in fit.rounds], nlb=len(fit.lb))


# ---------------------------------------------------------------------------------------------------------------------
def cases():
    B8 = ml.betas_for(8)
    comp = _companion_utr(B8)
    cs = []
    # ---- 1. bins
    preps = [make_utr(f"EN{N}", N, 1100 + N, B8, cnt_max=2, xlo=400, xhi=700) for N in N_BINS]
    jobs = []
    for u, N in enumerate(N_BINS):
        drops = sorted({b for b in (0, LANES - 1, LANES, N - 1) if b < N})
        jobs.append(ejob(preps[u], 2, SEED, u, a_range=(70, 110), perturb=[("e_drop_bin", b) for b in drops], note=f"N={N}"))
    cs.append(ECase("bins", 1, "N, Np = ceil(N / 16) 16 and the 64-bin lane stride on both sides of each other; K = 2", preps + [comp], jobs))
    # ---- 2. tight
    preps = [make_utr(f"ET{N}", N, 1200 + N, B8, cnt_max=2, xlo=400, xhi=700) for N in N_TIGHT]
    jobs = [ejob(preps[u], K, SEED, u, a_range=(70, 110), note=f"N={N} K={K}") for u, N in enumerate(N_TIGHT) for K in (1, 2, 3)]
    cs.append(ECase("tight", 2, "the smallest bounds of the ladder: 1, 9, 17 bins of 1 or 2 reads, K = 1..3, alphas next to the reads",
                    preps + [comp], jobs))
    # ---- 3. columns
    q = make_utr("EC17", 17, 1317, B8, cnt_max=2, xlo=300, xhi=1300)
    jobs = []
    for K in K_COLUMNS:
        pert = [("e_drop_col", K)] + ([("e_drop_col", K - 1)] if K else [])
        jobs.append(ejob(q, K, SEED, 0, a_range=(40, 190), perturb=pert, note=f"K={K}"))
    calls = tuple((i,) for i in range(len(jobs))) + tuple(tuple(i for i, j in enumerate(jobs) if j.K <= cap) for cap in MIXED_KMAX)
    cs.append(ECase("columns", 3, "K = 0 .. 63: every exact-K variant edge up to 16 columns alone in its call, and the generic 24 / 32 / "
                    "64-column bodies with small K under runtime predication", [q, comp], jobs, calls=calls))
    # ---- 4. liveness: sigma_f = 10, reads 28 apart, 3 reads per bin
    cs.append(ECase("liveness", 4, "a component below the -746 cut in every bin, in the whole first lane group, in all lanes of a group "
                    "but one, in the partial last group only",
                    [live_utr(B8, 0), live_utr(B8, 1), make_utr("Ecomp10", 17, 917, B8, cnt_max=2, p=PS10)], live_jobs()))
    # ---- 5. rescue
    q = make_utr("ER17", 17, 517, B8, xlo=700, xhi=1500, cnt_max=2)
    d = ml.dead_job(q, 40, 1)
    jobs = [EJob(0, 2, d.a_idx, d.b_idx, d.ws, np.zeros(2, np.int8), perturb=(("no_rescue", True),), note="all sentinel"),
            hand_job([150, 185], [3, 4], [0.85, 1e-30, 0.15], [1, 1],
                     perturb=(("no_rescue", True), ("rescue_once", True), ("entropy_plain", True)), note="live, far below"),
            hand_job([150, 185], [3, 4], [0.45, 0.4, 0.15], [1, 1], note="far above")]
    cs.append(ECase("rescue", 5, "column k all sentinel, live with sum Z_k far below 1e-8, and far above it; a second round refreshes "
                    "the rescued weight", [q, comp], jobs, nround=2))
    # ---- 6. cap
    q = make_utr("EP33", 33, 633, B8, cnt_max=2, xlo=400, xhi=700)
    jobs = [hand_job([71, 205], [1, 2], [0.45, 0.45, 0.1], [0], perturb=(("no_cap", True),), note="above"),
            hand_job([80, 100], [4, 4], [0.45, 0.45, 0.1], [0], note="below")]
    cs.append(ECase("cap", 6, "the uniform weight clearly above and clearly below max_unif_ws = 0.15", [q, comp], jobs))
    q = make_utr("EP33h", 33, 633, B8, cnt_max=2, xlo=400, xhi=700, p=P05)
    jobs = [hand_job([5, 205], [2, 2], [0.45, 0.45, 0.1], [0], perturb=(("no_cap", True),), note="above"),
            hand_job([71, 205], [1, 2], [0.45, 0.45, 0.1], [0], note="below 0.5, above 0.15")]
    cs.append(ECase("cap05", 6, "the same with max_unif_ws = 0.5", [q, make_utr("Ecomp05", 17, 917, B8, cnt_max=2, p=P05)], jobs))
    # ---- 7. zero weights
    q = make_utr("EZ17", 17, 717, B8, cnt_max=2, xlo=300, xhi=600)
    tiny = (("zero_weight_as_tiny", True),)
    jobs = [hand_job([60, 75, 90], [3, 3, 3], [0.5, 0.0, 0.35, 0.15], [0, 2], perturb=tiny, note="component"),
            hand_job([75, 90], [3, 3], [0.5, 0.5, 0.0], [0, 1], perturb=tiny, note="uniform"),
            hand_job([60, 75, 90], [3, 3, 3], [0.0, 0.5, 0.35, 0.15], [0, 1], perturb=tiny, note="updated")]
    cs.append(ECase("zero", 7, "an init weight of exactly 0 for a component, for the uniform column and for the updated column",
                    [q, comp], jobs, nround=2))
    # ---- 8. sentinel rows
    q = make_utr("ES33", 33, 833, B8, cnt_max=2)
    jobs = [hand_job([30, 60], [2, 5], [0.4, 0.45, 0.15], [1], perturb=(("e_drop_col", 2),), note="rows"),
            hand_job([30], [2], [0.85, 0.15], [0], perturb=(("e_drop_col", 1),), note="rows, K=1")]
    cs.append(ECase("sentinel", 8, "bins where every component column holds the sentinel and bins where exactly one is finite", [q, comp], jobs))
    # ---- 9. counts (held to its own bound, exempt from the caps)
    q = make_utr("EK33", 33, 933, B8, cnt_max=2)
    q.cnt = np.array(COUNTS, np.int64)[np.random.RandomState(9).randint(0, 4, size=33)]
    for nr in (1, 2):
        cs.append(ECase(f"counts{nr}", 9, f"cnt drawn from {COUNTS}, K = 3, nround = {nr}", [q, comp],
                        [ejob(q, 3, 2, nround=nr, perturb=(("untempered", True),), a_range=(20, 180))], nround=nr, capped=False))
    # ---- 10. rounds
    q = make_utr("ER33", 33, 1033, B8, cnt_max=2)
    for nr, Ks in ((2, (3, 8)), (5, (3,)), (10, (8,)), (20, (3, 8, 0))):
        jobs = []
        for K in Ks:
            fresh = (("fresh_columns", True),) if nr == K + 2 else ()
            order = [i % K for i in range(nr)] if K else None
            jobs.append(ejob(q, K, SEED, nround=nr, a_range=(20, 180), perturb=fresh, order=order, note=f"K={K}"))
        cs.append(ECase(f"rounds{nr}", 10, f"nround = {nr}: K = {Ks}", [q, comp], jobs, nround=nr))
    return cs


def live_utr(betas, which):
    """65 bins 28 apart, sigma_f = 10 (a row is finite on some 22 bins and falls to -600 at their left end), 3 reads per
    bin; UTR 0 has 2 reads in bins 40 and 64, UTR 1 has 60 in bin 64."""
    q = make_utr(f"EL65{'ab'[which]}", 65, 465, betas, cnt_max=3, xlo=60, lmin=50, lmax=51, p=PS10, spaced=28)
    q.cnt = np.full(65, 3, np.int64)
    if which == 0:
        q.cnt[[40, 64]] = 2
    else:
        q.cnt[64] = 60
    return q


# note -> (UTR, alphas, weights, perturbations); beta index 0, component 0 is updated, component 1 is the subject: its weight
# puts (lz_1 - mx) cnt where the note says (the row maximum is the uniform column's -22.1 wherever column 0 is a sentinel)
LIVE = {"dead everywhere": (0, [100, 150], [0.85, 1e-200, 0.15], ()),
        "group 0 dead, bin 64 live": (0, [100, 216], [0.85, 1e-130, 0.15], ()),
        "one lane live": (0, [100, 150], [0.85, 1e-160, 0.15], (("exp_zero", -700.0),)),
        "last group dead": (1, [100, 205], [0.45, 0.4, 0.15], ())}


def live_jobs():
    return [hand_job(a, [0, 0], w, [0], u=u, perturb=p, note=note) for note, (u, a, w, p) in LIVE.items()]


# ---------------------------------------------------------------------------------------------------------------------
# which E-step kernel a call runs (scape_hip.hip: em_rounds, em_wide, with_column_class) - no API reports it.
# tests/test_host.py pins this to the source.
SHAPES = (("fixed only", False, {}),
          ("mixed, depth 1", True, dict(ml.NARROW, SCAPE_HIP_EM_DEPTH="1")),
          ("mixed, depth 3", True, dict(ml.NARROW, SCAPE_HIP_EM_DEPTH="3")),
          ("mixed, 4 wavefronts", True, {}),
          ("mixed, no shrink", True, dict(ml.NARROW, SCAPE_HIP_EM_SHRINK="0")))
KNOBS = ("SCAPE_HIP_MSTEP", "SCAPE_HIP_SPLIT_MAXTILES", "SCAPE_HIP_EM_DEPTH", "SCAPE_HIP_WIDE_MAXJOBS", "SCAPE_HIP_EM_SHRINK")


def selection(env, jobs):
    """dict(kernel, column class, depth) of an EM call of `jobs` (EJob; companion included) under `env`."""
    kmax = max(1, max(j.K for j in jobs))
    cls = next(c for c in CLASSES if kmax + 1 <= c)
    if all(j.fixed for j in jobs):
        return dict(kernel="k2_estep_all_rounds", cls=cls, depth=1)
    wide = len(jobs) <= int(env.get("SCAPE_HIP_WIDE_MAXJOBS", ml.WIDE_MAXJOBS_DEFAULT)) and kmax + 1 <= ml.WIDE_MAX_COLUMNS
    if wide:
        return dict(kernel="k2_estep_cs", cls=cls, depth=1)
    return dict(kernel="k2_estep", cls=cls, depth=min(ml.EM_DEPTH, max(1, int(env.get("SCAPE_HIP_EM_DEPTH", ml.EM_DEPTH)))))


def variant(job, cls):
    """The estep_body instantiation a job runs in a call of column class `cls`: its exact column count up to 16, the
    class's generic body above."""
    return job.K + 1 if cls <= EXACT_MAX else 0
