"""The ladder of tests/test_tensor_ladder.py and tests/test_tensor_reference.py: small batches with a value on both
sides of every boundary of the tensor build (k_phase_a, k_phase_b, k_pb_tables, k_phase_b_lin, k_pb_logcol, k_pb_slide).
tests/test_host.py reads the boundaries from the sources and checks the ladder against them.

UtrPrep objects are built directly (not through prepare_utr), so that N, T, the grid and n_beta are exactly what a case
says.  All inputs are integers, or dyadic fractions where a case says so: theta - x, theta_i -+ 3 beta and the
comparisons made on them are then exact in f64 and in long double alike.

Every UTR carries the value edges: bins with l == theta_m - x exactly (every seventh bin), bins that start right of the
first grid points (theta - x < 0), pA sites on a grid value (pa == theta_m) and off the grid, r below s_dis[0], on a
value of s_dis, between two and on its maximum.
"""
from dataclasses import dataclass, field

import numpy as np

S_DIS = np.arange(20, 150, 10) + 0.0
PMF_S = np.repeat(1 / len(S_DIS), len(S_DIS))
P0 = dict(mu_f=300, sigma_f=50, max_unif_ws=0.15)
R_VALUES = (10.0, 50.0, 55.0, 140.0)             # below s_dis[0], on a grid value, in between, the maximum

BETAS_DEF = np.arange(5, 70, 5) + 0.0            # the default grid: step 9, betas 5..65, reach 22
BETAS_SMALL = np.array([5.0, 10.0, 15.0])        # reach 6: interior points from T = 15
BETAS_12 = np.array([1.0, 2.0])                  # reach 1: interior points from T = 5


def uniform_theta(T, step=9, start=None):
    start = (400 if T <= 9 else 31) if start is None else start
    return start + step * np.arange(T) + 0.0


def make_utr(name, N, theta, betas, log_bins=(), p=P0):
    """One UTR with N bins ascending in x.  log_bins: bin numbers that are pA-site (even places of the list) or
    r-known (odd places) bins."""
    from scape_amd.host import UtrPrep
    theta = np.asarray(theta, dtype=np.float64)
    T, k = len(theta), np.arange(N)
    span = max(float(theta[-1]) - 35 - 2, 0.0)
    x = 2 + np.floor(k * span / max(N - 1, 1))
    l = 31.0 + (7 * k) % 100
    for n in range(3, N, 7):                              # l == theta_m - x exactly
        m = int(np.searchsorted(theta, x[n] + 31))
        if m < T:
            l[n] = theta[m] - x[n]
    r, pa = np.full(N, np.nan), np.full(N, np.nan)
    for q, n in enumerate(log_bins):
        if q % 2 == 0:
            m = min(T - 1, int(np.searchsorted(theta, x[n] + l[n])) + 1 + q % 3)
            pa[n] = theta[m] if q % 4 == 0 else x[n] + l[n] + 37
        else:
            r[n] = R_VALUES[(q // 2) % 4]
    L = 2000
    return UtrPrep(gene_info_str=f"ladder:{name}:1:1-{L}:+", p=dict(p), x=x, l=l, r=r, pa=pa, cnt=(1 + k % 5).astype(np.int64),
                   idx=np.arange(N, dtype=np.int64), cb_id=np.arange(N), read_id=np.arange(N), L=L,
                   min_theta=float(theta[0]), theta=theta, betas=np.asarray(betas, dtype=np.float64), s_dis=S_DIS.copy(),
                   pmf_s=PMF_S.copy(), unif_ll=float(np.log((1 / L) * (1 / L) * (1 / 150))))


def edge_bins(N, extra=()):
    """Log-domain bins at n = 0, 15, 16 and N - 1 (where they exist)."""
    return sorted({n for n in (0, 15, 16, N - 1) + tuple(extra) if 0 <= n < N})


@dataclass
class Case:
    name: str
    preps: list
    form: int                    # Phase B form of the default build (0 one kernel, 2 sliding windows)
    axes: tuple                  # which axes of the ladder the case belongs to
    operator: bool = False       # also checked through get_loglik_marginal_tensor (every bin in the log domain)
    point_ops: bool = False      # also checked through the three point operators, one theta each
    note: str = ""
    forms: dict = field(init=False)

    def __post_init__(self):
        B = len(self.preps[0].betas)
        self.forms = {"v2": 0, "split": 1 if B <= 16 else 0, None: self.form}


N_LADDER = (1, 15, 16, 17, 63, 64, 65, 255, 256, 257)
N_LADDER_T = (17, 23, 16, 31, 19, 40, 15, 22, 18, 26)          # unequal, the largest not first
T_DEFAULT = (47, 50, 51, 53)                                   # 46 is a case of its own: no interior point
T_BETAS12 = (5, 7, 8, 9, 63, 64, 65, 68)                       # 1 and 2: no interior point
WIDTHS = {43: (9, 65.0), 45: (8, 60.0), 47: (8, 62.0), 49: (8, 65.0)}     # taps: (theta step, largest beta)
N_BETA = (1, 3, 4, 5, 13, 16, 17)
N_UTR = (1, 7, 8, 9)


def betas_for(B):
    """B betas whose widest window stays within 48 taps on the step-9 grid."""
    if B <= 13:
        return 5.0 * np.arange(1, B + 1)
    return (4.0 if B == 16 else 3.5) * np.arange(1, B + 1)       # 3.5 k: dyadic, 3 beta = 10.5 k exact


def n_log_utrs():
    """n_log = 0, 1 (at 0, 15, 16, N - 1 in turn), 4, 64, 65 and every bin."""
    th = uniform_theta(20)
    out = [make_utr("nlog0", 100, th, BETAS_SMALL)]
    out += [make_utr(f"nlog1at{n}", 100, th, BETAS_SMALL, [n]) for n in (0, 15, 16, 99)]
    out.append(make_utr("nlog4", 100, th, BETAS_SMALL, edge_bins(100)))
    out.append(make_utr("nlog64", 100, th, BETAS_SMALL, edge_bins(100, range(20, 80))))
    out.append(make_utr("nlog65", 100, th, BETAS_SMALL, edge_bins(100, range(20, 81))))
    out.append(make_utr("nlogall", 70, th, BETAS_SMALL, range(70)))
    return out


def cases():
    cs = []
    # ---- N: ten UTRs of one batch, unequal T
    cs.append(Case("N", [make_utr(f"N{n}", n, uniform_theta(t), BETAS_SMALL, edge_bins(n))
                         for n, t in zip(N_LADDER, N_LADDER_T)], 2, ("N", "n_utr"), operator=True, point_ops=True))
    # ---- T and the interior, default grid
    cs.append(Case("T46", [make_utr("T46", 33, uniform_theta(46), BETAS_DEF, edge_bins(33))], 0, ("T",),
                   note="no interior point: the batch is built by k_phase_b"))
    cs.append(Case("Tdef", [make_utr(f"T{t}", 33 - i, uniform_theta(t), BETAS_DEF, edge_bins(33 - i)) for i, t in enumerate(T_DEFAULT)],
                   2, ("T", "ends"), operator=True,
                   note="theta_i -+ 3 beta falls on grid points at beta = 15, 30, 45, 60: both inclusive ends"))
    cs.append(Case("T12none", [make_utr(f"T{t}", 18, uniform_theta(t), BETAS_12, edge_bins(18)) for t in (1, 2)], 0, ("T",)))
    cs.append(Case("T12", [make_utr(f"T{t}", 18, uniform_theta(t), BETAS_12, edge_bins(18)) for t in T_BETAS12], 2, ("T",),
                   operator=True))
    cs.append(Case("ringwrap", [make_utr("T70", 20, uniform_theta(70), BETAS_DEF, edge_bins(20))], 2, ("T", "ring"),
                   note="43-tap windows walk 70 grid points: the 64-row ring wraps"))
    # ---- window width
    for taps, (step, bmax) in WIDTHS.items():
        cs.append(Case(f"W{taps}", [make_utr(f"W{taps}", 20, uniform_theta(56, step), [5.0, 30.0, bmax], edge_bins(20))],
                       2 if taps <= 48 else 0, ("width",)))
    # ---- n_beta
    for B in N_BETA:
        cs.append(Case(f"B{B}", [make_utr(f"B{B}", 21, uniform_theta(49), betas_for(B), edge_bins(21))],
                       2 if B <= 16 else 0, ("n_beta",), operator=B in (13, 16, 17)))
    # ---- n_log
    cs.append(Case("nlog", n_log_utrs(), 2, ("n_log",)))
    # ---- n_utr
    for n in N_UTR:
        cs.append(Case(f"U{n}", [make_utr(f"U{n}_{u}", 20 + u, uniform_theta(15 + (5 * u) % 11), BETAS_SMALL, edge_bins(20 + u))
                                 for u in range(n)], 2, ("n_utr",)))
    # ---- grids
    th = uniform_theta(40)
    frac = np.unique(np.concatenate([th[:12], th[15:24] + 0.5, th[27:] + 0.25]))       # fixed_run style, dyadic fractions
    cs.append(Case("fractional", [make_utr("frac", 30, frac, BETAS_SMALL, edge_bins(30))], 0, ("grid",), operator=True))
    rep = np.sort(np.concatenate([th[:30], th[10:11], th[20:21]]))                       # ascending with repeated values
    cs.append(Case("repeated", [make_utr("rep", 30, rep, BETAS_SMALL, edge_bins(30))], 0, ("grid",), operator=True))
    # ---- values: sigma_f = 10 puts the v < 1e-300 cut inside the grid's reach (theta - x - 280 = 367 at s = 20)
    cs.append(Case("cut", [make_utr("cut", 120, uniform_theta(76), BETAS_SMALL, edge_bins(120, (40, 41, 77)),
                                    p=dict(P0, sigma_f=10))], 2, ("values",), point_ops=True))
    return cs


def expected_slide(preps, b_cap=16, steps=12, t_cap=4096):
    """The host's rule for the sliding-window form, restated: at most b_cap betas, every UTR has a uniform grid of integer values with at
    least one interior point, the widest window fits 4 * steps taps, no grid is longer than t_cap."""
    betas = preps[0].betas
    if len(betas) > b_cap:
        return False
    w_max = 1
    for q in preps:
        th, T = q.theta, q.T
        step = th[1] - th[0] if T > 1 else 0.0
        uni = step > 0 and np.all(np.floor(th) == th) and np.all(np.diff(th) == step)
        if not uni:
            return False
        rmax = int(np.floor(3 * betas.max() / step)) + 1
        if rmax + 1 > T - 2 - rmax:
            return False
        lo = np.searchsorted(th, th - 3 * betas.max(), "left")
        hi = np.searchsorted(th, th + 3 * betas.max(), "right") - 1
        w_max = max(w_max, int((hi - lo + 1).max()))
    return w_max <= 4 * steps and max(q.T for q in preps) <= t_cap


_REF = {}


def reference(case):
    """[(PhaseA, PhaseB)] per UTR of a case: the long-double values and bounds, computed once per process."""
    from oracle import tensor_reference as tr
    if case.name not in _REF:
        out = []
        for q in case.preps:
            a = tr.phase_a_ld(q.x, q.l, q.r, q.pa, q.theta, q.s_dis, q.pmf_s, q.p["mu_f"], q.p["sigma_f"])
            out.append((a, tr.phase_b_ld(q.theta, q.betas, pa_ref=a)))
        _REF[case.name] = out
    return _REF[case.name]
