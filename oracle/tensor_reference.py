"""Long-double reference of the tensor build (Phase A, Phase B) with a per-entry rounding bound.

TEST INFRASTRUCTURE ONLY, like ``scape_oracle.py``: written from the formulas of the reference's
``taichi_core.py:24-246`` and evaluated in ``np.longdouble`` (64-bit mantissa) from the f64 inputs, the r-known branch
included.  The constant ``PI_REF`` is the reference's f64 literal, not pi.

Beside every value the functions return a FIRST-ORDER BOUND on how far a correct f64 evaluation may lie from it.  The
bound is derived by counting the roundings of the device's sequence (scape_hip.hip, phase_b.inc); where the C
oracle's sequence differs it rounds less often or the same.  Unit: u = 2^-53, the relative error of one correctly
rounded f64 operation.  An error of e ulp of a library function is at most 2 e u relative.  The derived bound is
multiplied by MARGIN = 2 for the second-order terms and never by anything else.

Notation: e(q) is the relative error of a positive quantity q in units of u, E(q) the absolute error of a log-domain
quantity in units of u.  inx(q) is 1 when the long-double value of q is not an f64 number (the f64 operation rounds)
and 0 when it is one (the operation is exact: integer and dyadic inputs make most differences exact).

Phase A, r-unknown bins (d_point_r_unknown):  v = sum_j term_j,  A = log v.
    d_j   = x - ((theta + s_j) - mu_f)      e(d_j)  = (inx(m1)|m1| + inx(m2)|m2| + inx(d_j)|d_j|) / |d_j|
    z_j   = d_j * (1 / sigma_f)             e(z_j)  = e(d_j) + 2          (reciprocal, product)
    arg_j = -0.5 z_j^2                      e(arg)  = 2 e(z_j) + 1 = 5 + 2 e(d_j)
    exp(arg_j)                              1.2     (0.60 ulp, d_exp_nonpos)  +  e(arg) |arg_j|   <- the dominant term
    * (1 / sqrt(2 PI)) * (1 / sigma_f)      2 + 1 + 1 + 1   (sqrt, reciprocal, product; reciprocal, product)
    (1 / s_j) * pdf                         1 + 1
    * (1 / (theta - x))                     inx(theta - x) + 1 + 1
    * pmf_j                                 1
  so e(term_j) = (5 + 2 e(d_j)) |arg_j| + 11.2 + inx(theta - x), the sum of S positive terms in order adds S - 1,
    e(v) = sum_j term_j e(term_j) / v + (S - 1),       E(A) = e(v) + 1.66 |A|      (0.83 ulp, d_log_pos).
  Terms in the subnormal range carry an absolute error of 2^-1074 against v >= 1e-300 (the cut): 1e-23 relative,
  left out.  v < 1e-300 is set to 0 and gives the sentinel, as in the reference.

Phase A, pA-site bins (d_point_pa, library log: 1 ulp = 2 u):
    ll    = -log(theta - x)                 E(ll)   = inx(theta - x) + 2 |ll|
    z     = (pa - theta) / sigma_f          e(z)    = inx(pa - theta) + 1
    t1    = -0.5 z^2                        E(t1)   = (2 e(z) + 1) |t1|
    lp    = (t1 - log sigma_f) - 0.5 log(2 PI)      E(lp) = E(t1) + 2 |log sigma_f| + 2 |0.5 log(2 PI)| + |t2| + |lp|
    A     = ll + lp                         E(A)    = E(ll) + E(lp) + |A|
Phase A, r-known bins (d_point_r_known, two-pass logsumexp over the s_j >= r, library exp / log):
    t_j   = ((-log s_j + lp_j) + ll) + log pmf_j,   lp_j as above with z = (x - ((theta + s_j) - mu_f)) / sigma_f
    E(t_j) = 2 |log s_j| + E(lp_j) + E(ll) + 2 |log pmf_j| + |a1| + |a2| + |t_j|       (the three partial sums)
    p_j   = exp(t_j - mx)                   e(p_j)  = E(t_j) + |t_j - mx| + 2     (mx itself cancels: it is added back)
    sum   = sum_j p_j                       e(sum)  = sum_j p_j e(p_j) / sum + (S - 1)
    A     = (log sum + mx) - log(sum_j pmf_j)
    E(A)  = e(sum) + 2 |log sum| + |log sum + mx| + (S_kept - 1) + 2 |log tmpn| + |A|
  l > theta - x gives the sentinel in all three branches (SENT + anything of ordinary size is SENT in f64 and in long
  double alike).

Phase B, common part (k_phase_b / k_pb_tables, library exp / log):
    g_w   = log N(theta_w; theta_i, beta)   E(g_w)  = (2 (inx(theta_w - theta_i) + 1) + 1) |t1| + 2 |log beta|
                                                      + 2 |0.5 log(2 PI)| + |t2| + |g_w|
    G     = log sum_w exp(g_w)              E(G)    = sum_w exp(g_w) (E(g_w) + 2) / sum + (W - 1) + 2 |G|
Phase B, log-domain path (pA-site and r-known bins on the device; every bin in get_loglik_marginal_tensor and in
the C oracle):
    t_w   = (A_w + g_w) - G                 E(t_w)  = E(A_w) + E(g_w) + E(G) + |A_w + g_w| + |t_w|
    p_w   = exp(t_w - mx)                   e(p_w)  = E(t_w) + |t_w - mx| + 2
    M     = log(sum_w p_w) + mx             E(M)    = sum_w p_w e(p_w) / sum + (W - 1) + 2 |log sum| + |M|
Phase B, linear-domain path (r-unknown bins on the device: weights once, f64 MFMA window sum of at most 48 taps):
    q_w   = exp(g_w - G)                    e(q_w)  = E(g_w) + E(G) + |g_w - G| + 2
    acc   = sum_w q_w V_w                   e(acc)  = sum_w q_w V_w (e(q_w) + e(V_w)) / acc + (W + 1)
    M     = log acc                         E(M)    = e(acc) + 1.66 |M|
  (one rounding per tap of the FMA chain; taps of weight 0 add exactly 0; + 1 covers a separately rounded product).
Window ends and the comparisons l <= theta - x, s_j < r are made in f64 AND in long double; ``cmp_mismatch`` counts
the places where the two disagree (tests keep it at 0 by using integer / dyadic inputs).
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

LD = np.longdouble
U = 2.0 ** -53
MARGIN = 2.0
SENT = float(np.finfo("f").min)
PI_REF = 3.141592653589793              # taichi_core.py:9
V_CUT = 1e-300                          # taichi_core.py:154
EXP_DEV = 1.2                           # d_exp_nonpos: 0.60 ulp
LOG_DEV = 1.66                          # d_log_pos: 0.83 ulp
LIB = 2.0                               # library exp / log: 1 ulp


def _need_long_double():
    assert np.finfo(LD).nmant >= 63, "np.longdouble has no 64-bit mantissa here: this reference needs one"


def _ld(a):
    return np.asarray(a, dtype=np.float64).astype(LD)


def _inx(a):
    """1.0 where the long-double value is not an f64 number."""
    return (a != a.astype(np.float64).astype(LD)).astype(np.float64)


def _f(a):
    return np.asarray(a, dtype=np.float64)


def _abs(a):
    return np.abs(a).astype(np.float64)


@dataclass
class PhaseA:
    A: np.ndarray            # [N, T] long double; SENT at sentinel entries
    bound: np.ndarray        # [N, T] f64, absolute, margin included; 0 at sentinel entries
    sent: np.ndarray         # [N, T] bool
    E: np.ndarray            # [N, T] E(A) in u, without the margin (Phase B inherits it)
    V: np.ndarray            # [N, T] long double, linear domain, r-unknown bins (0 elsewhere)
    eV: np.ndarray           # [N, T] e(V) in u
    kind: np.ndarray         # [N] 0 r-unknown, 1 pA site, 2 r known
    cut_distance: float      # smallest |v / 1e-300 - 1| over the r-unknown entries
    v_cut_max: float         # the largest v that the cut removed (0: none)
    cmp_mismatch: int


def _logpdf(d, e_d, sigma):
    """log N with z = d / sigma: value and E in u.  e_d: relative error of d in u."""
    z = d / sigma
    t1 = LD(-0.5) * (z * z)
    lsig, c = np.log(LD(sigma)), LD(0.5) * np.log(LD(2) * LD(PI_REF))
    t2 = t1 - lsig
    lp = t2 - c
    E = (2 * (e_d + 1) + 1) * _abs(t1) + LIB * float(abs(lsig)) + LIB * float(abs(c)) + _abs(t2) + _abs(lp)
    return lp, E


def _shift_chain(th, sj, mu_f, x):
    """d = x - ((theta + s_j) - mu_f) and its relative error in u."""
    m1 = th + sj
    m2 = m1 - mu_f
    d = x - m2
    ad = _abs(d)
    e_abs = _inx(m1) * _abs(m1) + _inx(m2) * _abs(m2) + _inx(d) * ad
    with np.errstate(divide="ignore", invalid="ignore"):
        e_d = np.where(ad > 0, e_abs / np.where(ad > 0, ad, 1.0), 0.0)
    return d, e_d


def phase_a_ld(x, l, r, pa, all_theta, s_dis, pmf, mu_f, sigma_f):
    _need_long_double()
    x64, l64, th64 = _f(x), _f(l), _f(all_theta)
    r64, pa64 = _f(r), _f(pa)
    N, T, S = len(x64), len(th64), len(s_dis)
    X, L_, TH = _ld(x64)[:, None], _ld(l64)[:, None], _ld(th64)[None, :]
    s, pm = _ld(s_dis), _ld(pmf)
    mu, sg = LD(float(mu_f)), LD(float(sigma_f))
    kind = np.where(~np.isnan(pa64), 1, np.where(~np.isnan(r64), 2, 0))
    u0 = TH - X
    ok = L_ <= u0
    ok64 = l64[:, None] <= (th64[None, :] - x64[:, None])
    mism = int((ok != ok64).sum())
    inx_u0 = _inx(u0)
    u0s = np.where(ok, u0, LD(1))
    A = np.full((N, T), LD(SENT))
    E = np.zeros((N, T))
    V = np.zeros((N, T), dtype=LD)
    eV = np.zeros((N, T))
    cut_distance, v_cut_max = np.inf, 0.0
    with np.errstate(all="ignore"):
        ll = -np.log(u0s)
        E_ll = inx_u0 + LIB * _abs(ll)
        # ---- r-unknown
        ru = kind == 0
        if ru.any():
            Xr, okr, u0r = X[ru], ok[ru], u0s[ru]
            lk = np.where(okr, LD(1) / u0r, LD(0))
            v = np.zeros(lk.shape, dtype=LD)
            num = np.zeros(lk.shape)
            norm = np.sqrt(LD(2) * LD(PI_REF))
            for j in range(S):
                d, e_d = _shift_chain(TH, s[j], mu, Xr)
                z = d / sg
                arg = LD(-0.5) * (z * z)
                term = (LD(1) / s[j]) * (np.exp(arg) / norm / sg) * lk * pm[j]
                e_term = (5 + 2 * e_d) * _abs(arg) + (EXP_DEV + 10.0) + inx_u0[ru]
                v = v + term
                num = num + (term * e_term.astype(LD)).astype(LD)
            pos = v > 0
            cut_distance = float(np.min(np.abs(v[pos] / LD(V_CUT) - 1))) if pos.any() else np.inf
            keep = ~(v < LD(V_CUT))
            v_cut_max = float(np.max(np.where(keep, LD(0), v)))
            v = np.where(keep, v, LD(0))
            fin = v > 0
            vs = np.where(fin, v, LD(1))
            ev = np.where(fin, (num / vs).astype(np.float64) + (S - 1), 0.0)
            a = np.log(vs)
            A[ru] = np.where(fin, a, LD(SENT))
            E[ru] = np.where(fin, ev + LOG_DEV * _abs(a), 0.0)
            V[ru] = v
            eV[ru] = ev
        # ---- pA site
        ps = kind == 1
        if ps.any():
            dpa = _ld(pa64)[ps][:, None] - TH
            lp, E_lp = _logpdf(dpa, _inx(dpa), sg)
            a = ll[ps] + lp
            A[ps] = np.where(ok[ps], a, LD(SENT))
            E[ps] = np.where(ok[ps], E_ll[ps] + E_lp + _abs(a), 0.0)
        # ---- r known
        rk = kind == 2
        if rk.any():
            Xk, okk = X[rk], ok[rk]
            rr = _ld(r64)[rk][:, None]
            shape = (int(rk.sum()), T)
            t, Et = [], []
            keepj = []
            for j in range(S):
                kj = np.broadcast_to(~(s[j] < rr), shape)
                assert np.all(rr[kj[:, 0]] <= s[j])
                d, e_d = _shift_chain(TH, s[j], mu, Xk)
                lp, E_lp = _logpdf(d, e_d, sg)
                lrs, lpm = -np.log(s[j]), np.log(pm[j])
                a1 = lrs + lp
                a2 = a1 + ll[rk]
                tj = a2 + lpm
                t.append(tj)
                Et.append(LIB * float(abs(lrs)) + E_lp + E_ll[rk] + LIB * float(abs(lpm)) + _abs(a1) + _abs(a2) + _abs(tj))
                keepj.append(kj)
            t, Et, keepj = np.stack(t), np.stack(Et), np.stack(keepj)
            assert keepj.any(axis=0).all(), "r above every s_dis value: the reference is NaN there"
            mx = np.max(np.where(keepj, t, LD(-np.inf)), axis=0)
            aj = np.where(keepj, t - mx, LD(0))
            p = np.where(keepj, np.exp(aj), LD(0))
            sm = p.sum(axis=0)
            e_sum = ((p * (Et + _abs(aj) + LIB).astype(LD)).sum(axis=0) / sm).astype(np.float64) + (S - 1)
            ls = np.log(sm)
            r1 = ls + mx
            tmpn = np.zeros(shape, dtype=LD)
            for j in range(S):
                tmpn = tmpn + np.where(keepj[j], pm[j], LD(0))
            nk = keepj.sum(axis=0)
            ltn = np.log(tmpn)
            a = r1 - ltn
            Ea = e_sum + LIB * _abs(ls) + _abs(r1) + (nk - 1) + LIB * _abs(ltn) + _abs(a)
            A[rk] = np.where(okk, a, LD(SENT))
            E[rk] = np.where(okk, Ea, 0.0)
    sent = A == LD(SENT)
    return PhaseA(A=A, bound=MARGIN * U * E, sent=sent, E=E, V=V, eV=eV, kind=kind, cut_distance=cut_distance, v_cut_max=v_cut_max,
                  cmp_mismatch=mism)


@dataclass
class PhaseB:
    M: np.ndarray            # [T, B, N] long double; SENT at sentinel entries
    sent: np.ndarray         # [T, B, N] bool
    bound_log: np.ndarray    # [T, B, N] f64 absolute, margin included: every bin through the log-domain path
    bound_dev: np.ndarray    # the same with the r-unknown bins through the linear-domain path (the batched build)
    lo: np.ndarray           # [T, B] window ends (inclusive)
    hi: np.ndarray
    cmp_mismatch: int


def window_ends(th64, betas64):
    """[T, B] inclusive window ends by the reference's rule (taichi_core.py:221-222) in f64, and how many of them a
    long-double evaluation of theta_i -+ 3 beta would place elsewhere."""
    T, B = len(th64), len(betas64)
    lo, hi = np.zeros((T, B), np.int64), np.zeros((T, B), np.int64)
    thl = _ld(th64)
    mism = 0
    for j, b in enumerate(betas64):
        lo[:, j] = np.searchsorted(th64, th64 - 3 * b, "left")
        hi[:, j] = np.searchsorted(th64, th64 + 3 * b, "right") - 1
        lob, hib = thl - LD(3) * LD(b), thl + LD(3) * LD(b)
        lo_l = (thl[None, :] < lob[:, None]).sum(axis=1)
        hi_l = (thl[None, :] <= hib[:, None]).sum(axis=1) - 1
        mism += int((lo_l != lo[:, j]).sum() + (hi_l != hi[:, j]).sum())
    return lo, hi, mism


def phase_b_ld(all_theta, betas, pa_ref=None, A=None):
    """Phase B of a PhaseA result, or (A given: an f64 [N, T] input, E(A) = 0) of the operator
    get_loglik_marginal_tensor."""
    _need_long_double()
    th64, be64 = _f(all_theta), _f(betas)
    T, B = len(th64), len(be64)
    if pa_ref is None:
        A64 = _f(A)
        Al, sentA = A64.astype(LD), A64 == SENT
        EA, V, eV = np.zeros(A64.shape), None, None
        lin_bins = np.zeros(A64.shape[0], bool)
    else:
        Al, sentA, EA, V, eV = pa_ref.A, pa_ref.sent, pa_ref.E, pa_ref.V, pa_ref.eV
        lin_bins = pa_ref.kind == 0
    N = Al.shape[0]
    thl = _ld(th64)
    lo, hi, mism = window_ends(th64, be64)
    M = np.full((T, B, N), LD(SENT))
    Elog = np.zeros((T, B, N))
    Edev = np.zeros((T, B, N))
    c = LD(0.5) * np.log(LD(2) * LD(PI_REF))
    any_lin = bool(lin_bins.any())
    with np.errstate(all="ignore"):
        for j in range(B):
            b = LD(be64[j])
            lb = np.log(b)
            for i in range(T):
                a0, a1 = int(lo[i, j]), int(hi[i, j]) + 1
                W = a1 - a0
                dth = thl[a0:a1] - thl[i]
                z = dth / b
                t1 = LD(-0.5) * (z * z)
                t2 = t1 - lb
                g = t2 - c
                Eg = (2 * (_inx(dth) + 1) + 1) * _abs(t1) + LIB * float(abs(lb)) + LIB * float(abs(c)) + _abs(t2) + _abs(g)
                pg = np.exp(g)
                psum = pg.sum()
                G = np.log(psum)
                EG = float((pg * (Eg + LIB).astype(LD)).sum() / psum) + (W - 1) + LIB * float(abs(G))
                # log-domain path
                Aw, sw = Al[:, a0:a1], sentA[:, a0:a1]
                t0 = Aw + g[None, :]
                t = t0 - G
                Et = EA[:, a0:a1] + Eg[None, :] + EG + _abs(t0) + _abs(t)
                live = ~sw
                some = live.any(axis=1)
                mx = np.max(np.where(live, t, LD(-np.inf)), axis=1)
                mxs = np.where(some, mx, LD(0))
                a = np.where(live, t - mxs[:, None], LD(0))
                p = np.where(live, np.exp(a), LD(0))
                sm = p.sum(axis=1)
                sms = np.where(some, sm, LD(1))
                e_sum = ((p * (Et + _abs(a) + LIB).astype(LD)).sum(axis=1) / sms).astype(np.float64) + (W - 1)
                ls = np.log(sms)
                m = ls + mxs
                M[i, j] = np.where(some, m, LD(SENT))
                el = np.where(some, e_sum + LIB * _abs(ls) + _abs(m), 0.0)
                Elog[i, j] = el
                Edev[i, j] = el
                if any_lin:
                    q = g - G
                    pw = np.exp(q)
                    e_pw = Eg + EG + _abs(q) + LIB
                    Vw = V[lin_bins, a0:a1]
                    prod = Vw * pw[None, :]
                    acc = prod.sum(axis=1)
                    pos = acc > 0
                    accs = np.where(pos, acc, LD(1))
                    e_acc = ((prod * (e_pw[None, :] + eV[lin_bins, a0:a1]).astype(LD)).sum(axis=1) / accs).astype(np.float64) + (W + 1)
                    assert np.array_equal(pos, some[lin_bins])
                    Edev[i, j, lin_bins] = np.where(pos, e_acc + LOG_DEV * _abs(np.log(accs)), 0.0)
    sent = M == LD(SENT)
    return PhaseB(M=M, sent=sent, bound_log=MARGIN * U * Elog, bound_dev=MARGIN * U * Edev, lo=lo, hi=hi, cmp_mismatch=mism)


def compare(got, ref, bound, sent):
    """A computed f64 array against the reference: (sentinel pattern equal, worst |got - ref| / bound over the
    entries, number of entries that are not within their bound).  No entry is left out: an entry is a sentinel in both,
    or compared; a NaN, an infinity, or a sentinel on one side only is never within a bound (its ratio is inf)."""
    got = np.asarray(got, dtype=np.float64)
    wrong = (got == SENT) != sent                       # a sentinel on one side only: never within a bound either
    fin = ~sent & ~wrong
    ratio = np.zeros(got.shape)
    ratio[wrong] = np.inf
    with np.errstate(invalid="ignore"):
        err = np.abs(got[fin].astype(LD) - ref[fin]).astype(np.float64)
        rf = err / bound[fin]
    ratio[fin] = np.where(np.isfinite(got[fin]) & np.isfinite(rf), rf, np.inf)
    return not wrong.any(), float(ratio.max()) if ratio.size else 0.0, int((~(ratio <= 1)).sum())
