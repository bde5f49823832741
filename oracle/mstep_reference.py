"""Long-double restatement of em_algo rounds on a GIVEN f64 marginal tensor, with the M-step's arg-max laid open.

TEST INFRASTRUCTURE ONLY, like ``tensor_reference.py``: written from the reference's ``apa_core.py:473-573`` and
``:702-779`` (cal_z_k, norm_z, mstep, maximize_ws, max_alpha_beta, elbo, cal_bic, em_algo) and evaluated in
``np.longdouble`` (64-bit mantissa).  The tensor, ``cnt``, the grids and the init are f64 inputs; nothing is built here.

Each round, in the reference's order: the stale-column refresh (:731), the count-tempered norm_z (:490-495), the
``Z[:, k] += 1e-8`` rescue (:528-529), maximize_ws with its cap (:498-505) and, for every row (alpha, beta) of the
inclusive window [alpha_{k-1}, alpha_{k+1}] (min_theta / L at the ends, :511-513), the score
    S(row) = sum_n (log w_k + M[row, n]) v[n],        v[n] = Z[n, k] cnt[n].
Per round the function returns the winning row (first maximum), every row's score, the rows tied with the winner IN
EXACT ARITHMETIC - rows whose tensor values are bit-identical to the winner's on every bin with v != 0 - and a
first-order BOUND per row on how far a correct f64 evaluation by the device's sequence (em_lockstep.inc: estep_body;
mstep.inc and the three kernels built on it: mstep_staged.inc, mstep_ring.inc, mstep_multi.inc) may lie from S(row).  A round is DECIDED when the winner beats every row
outside its tie set by more than the two rows' bounds: then every correct f64 evaluation returns the same row, and a
test may demand it exactly.

Notation as in tensor_reference.py: u = 2^-53; e(q) the relative error of a positive quantity in units of u, E(q)
the absolute error of a log-domain quantity in units of u; a library or device function of e ulp costs 2 e u.  The
derived bound is multiplied by MARGIN = 2 for the second-order terms and by nothing else.  The tensor is an input: it
carries no error of its own.

E-step chain of v (estep_body), columns c = 0..K of bin n, mx the row maximum:
    lw_c  = log w_c                         E(lw_c) = 2 |lw_c|  (library log) + e(w_c) once w_c is a computed weight
    lz_c  = lw_c + M_c                      E(lz_c) = E(lw_c) + |lz_c|;   M_c a sentinel: z_c = 0 exactly, no error
    arg_c = (lz_c - mx) cnt                 E(arg)  = cnt (E(lz_c) + E(mx) + |lz_c - mx|) + |arg_c|;  0 for the maximum
    z_c   = exp(arg_c)                      e(z_c)  = E(arg_c) + 1.2        (d_exp_nonpos, 0.60 ulp)  <- |arg| amplifies
    s     = sum_c z_c                       e(s)    = sum_c z_c e(z_c) / s + K
    Z_c   = z_c (1 / s)                     e(Z_c)  = e(z_c) + e(s) + 2 + 1    (d_rcp_mid: z (1/s) within 2 ulp of z / s)
    v     = Z_k cnt                         e(v)    = e(Z_k) + 1  (+ 1 when the rescue adds 1e-8)
  d_log_pos (0.83 ulp) enters the entropy only, not v.
  w_c   = sum_n cnt Z_c / sum_c (..)        e(w_c)  = sum_n cnt Z_c (e(Z_c) + 1) / sum + (N - 1) + K + 1  (+ K + 2: the cap)
M-step score of one row (k2_mstep's epilogue; k3_mstep and k4_mstep run the same chain):
    sv    = sum_n v                         |d sv|  <= sum_n v e(v) + (N - 1) sv
    tl    = sum_{n >= n_ext} v (from the end) |d tl| <= sum_tail v e(v) + (n_tail - 1) tl
    c0    = lw_k sv + SENT tl               |d c0|  <= |lw_k| |d sv| + E(lw_k) sv + |lw_k sv| + |SENT| (|d tl| + tl) + |c0|
    acc   = sum_{n < n_ext} M[n] v[n]       one rounding per term of the ascending MFMA chain: sum_j |P_j|, P_j the partial
                                            sums, plus sum_n |M[n] v[n]| e(v[n])
    S     = c0 + acc                        + |S|
  Which sentinel entries lie beyond the tile's extent (tail) and which before it (chain) depends on the tile; the bound
  takes BOTH for every sentinel entry (the chain over all bins, the tail over all sentinel bins), so that it holds for
  every extent.  Loose by that much, never tight: a looser bound leaves fewer rounds decided, it cannot pass a wrong row.
Comparisons the reference makes in f64 (the rescue's sum < 1e-8, the cap's w_K > max_unif_ws, the stopping rule) are
made in long double; ``near`` counts the places where the value lies within 1e-9 relative of its threshold - tests keep
it at 0.  exp is taken as 0 below -745.13, where the f64 exp is: a v[n] of 5e-324 or 0 moves no score by a rounding,
it only moves the ends n0, n1 of the support by a bin.

Named perturbations - WRONG M-steps expressed in the reference, to show that a test case sits on the boundary it names:
    drop_bin=n        v[n] treated as 0 in the scores
    lo_exclusive      the window without its first alpha          hi_exclusive    ... without its last alpha
    sentinel_as_zero  sentinel entries add 0 instead of SENT v
    last_max          the last maximum among the exact ties instead of the first
    rows_to=r         rows at or above r are ignored (a partial last tile, a window cut at a tile edge)
A perturbation that leaves no row gives row -1.

Bounds on the E-step's own outputs (Round / Fit: ws_bound, lb_bound, bic_bound; absolute, MARGIN included).  They follow
estep_body's sequence and hold for ANY order of the sums (a sum of m terms t_i costs (m - 1) sum |t_i|).  The chain above
feeds the M-step bound through e(w) as it always did; the E-step bounds run the same chain a second time (suffix F in
the code) with the weight error carried in full from round to round:
    W_c   = sum_n cnt Z_c                   e(W_c)  = sum_n cnt Z_c (e(Z_c) + 1) / W_c + (N - 1)
    S     = sum_c W_c                       e(S)    = sum_c W_c e(W_c) / S + K
    w_c   = W_c / S                         e(w_c)  = e(W_c) + e(S) + 1;  W_c = 0: w_c = 0 exactly
    cap:  sk = sum_{c < K} w_c              e(sk)   = sum_c w_c e(w_c) / sk + (K - 1)
          w_c = ((1 - m) w_c) / sk          e(w_c) += e(sk) + 3;   w_K = m = max_unif_ws is an input: no error
  ws_bound = u (MARGIN e(w_c) + 1) w_c + (sum cnt + 1) 2^-1074: the 1 is the reference's own rounding to f64, the last term
  the absolute rounding of values below the normal range (an exp result of 1e-310 has no relative accuracy).  The output
  sort permutes the bound with the weights.  A weight that was never computed (the init, the cap value) has e = 0.
ell = sum_{n, c: Z != 0} t,  t = (Z_c cnt) lz_c:
    |d t|  <= |t| (e(Z_c) + 2) + Z_c cnt E(lz_c)        (two products; E(lz_c) = |lz_c| on a sentinel entry that the
                                                         rescue made non-zero: the one rounding of log w + SENT)
    |d ell| <= sum |d t| + (terms - 1) sum |t|
  bic = -2 ell + (3 K + 1) log N:           |d bic| <= 2 |d ell| + 3 pen + |bic|     (library log, product, sum)
ent = sum_n cnt sum_c -pk_c L_c over the columns with pk_c > 0; s2 = sum_c Z_c, x2 = s2 - 1, X2 = 2 K + 3 (+ 1 with the
rescue) bounds |s2 - its exact value| / u: K roundings each of s and s2 and the 3 u of Z_c = z_c rcp(s) - the rounding of
Z_c that the closed form below does not see is inside X2:
    pk_c  = Z_c rcp(s2)                     e(pk)   = e(Z_c) + X2 + 2 + 1
    ls    = d_log_pos(s)  (0.83 ulp)        E(ls)   = e(s) + 1.66 |ls|
    ls2   = x2 - x2^2 / 2                   E(ls2)  = X2 (+ 3 |x2| + |x2|^3 / (3 u) with the rescue: roundings, the series' tail)
    L_c   = (arg_c - ls) - ls2              E(L_c)  = E(arg_c) + E(ls) + E(ls2) + |arg_c - ls| + |L_c|
    L_k   = log(zk) - ls2  (rescue)         E(L_k)  = e(Z_k) + 2 |log zk| + E(ls2) + |L_k|      zk = Z_k + 1e-8
    |d ent| <= sum cnt pk (|L| (e(pk) + 2) + E(L)) + (terms - 1) sum cnt pk |L|
  Without the rescue the exact s2 is 1 and the whole of ls2 counts as error.
lb = ell + ent:                             |d lb|  <= |d ell| + |d ent| + |lb|
Every bound gets one more u |value| for the reference's own rounding to f64.  The liveness test (lz_c - mx) cnt >= -746
of estep_body is one more f64 comparison: between -746 and -745.13 exp gives 0 or a subnormal, which the reference takes
as 0; an argument within 1e-9 relative of -745.13 counts as ``near``, and so does a bin whose row maximum is itself a
sentinel (log 0 + M), where f64 absorbs what long double keeps.

Named wrong E-steps (E_PERTURBATIONS), used like the M-step ones:
    e_drop_bin=n      bin n is in no sum (log N of the BIC keeps N)       e_drop_col=c    column c takes no part
    no_rescue         Z[:, k] is never lifted by 1e-8                     rescue_once     ... lifted, but the entropy is the un-rescued Z's
    no_cap            the uniform weight is not capped                    cap_inclusive   >= instead of > in the cap
    fresh_columns     every column's log-weight is refreshed every round, not only column k's
    untempered        the counts are not in the exponent                  exp_zero=x      exp is cut to 0 below x instead of -745.13
    entropy_plain     the entropy is -sum Z log Z, not re-normalised by s2
    zero_weight_as_tiny   log 0 is log 1e-300, not the sentinel
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

LD = np.longdouble
U = 2.0 ** -53
MARGIN = 2.0
SENT = float(np.finfo("f").min)
EXP_DEV = 1.2                           # d_exp_nonpos: 0.60 ulp
LIB = 2.0                               # library log: 1 ulp
RCP = 2.0                               # z * d_rcp_mid(s) against z / s
EXP_ZERO = -745.13                      # exp(x) is 0 in f64 below this
PERTURBATIONS = ("drop_bin", "lo_exclusive", "hi_exclusive", "sentinel_as_zero", "last_max", "rows_to")
E_PERTURBATIONS = ("e_drop_bin", "e_drop_col", "no_rescue", "rescue_once", "no_cap", "cap_inclusive", "fresh_columns",
                   "untempered", "exp_zero", "entropy_plain", "zero_weight_as_tiny")
LOG_DEV = 1.66                          # d_log_pos: 0.83 ulp
TINY = 2.0 ** -1074                     # the spacing of f64 below the normal range


def _need_long_double():
    assert np.finfo(LD).nmant >= 63, "np.longdouble has no 64-bit mantissa here: this reference needs one"


@dataclass
class Round:
    k: int
    rescue: bool
    v: np.ndarray               # [N] long double, Z[:, k] cnt (after the rescue)
    n0: int                     # bins [n0, n1) outside which v is exactly 0 (0, 0: v is 0 everywhere)
    n1: int
    lw: float                   # log w_k of the new weights
    rows: np.ndarray            # rows a * B + b of the window, ascending (after the perturbations)
    score: np.ndarray           # long double, per row of `rows`
    bound: np.ndarray           # f64 absolute, margin included, per row of `rows`
    row: int                    # the winner: first maximum (last_max: the last of its exact ties); -1 without a row
    ties: np.ndarray            # rows tied with the winner in exact arithmetic, the winner included, ascending
    ratio: float                # min over the rows outside `ties` of gap / (bound_w + bound_r); inf when there is none
    ws: np.ndarray              # [K + 1] long double, after maximize_ws
    lb: float
    near: int
    ws_bound: np.ndarray = None # f64 [K + 1] absolute, in the order of `ws`
    lb_bound: float = 0.0
    bic_bound: float = 0.0      # of the BIC a job that ends with this round returns
    capped: bool = False
    x2: float = 0.0             # largest |s2 - 1| over the bins: 1e-8 with the rescue, 0 without (estep_body's series is for < 1e-5)

    @property
    def decided(self):
        return self.ratio > 1.0

    def within(self, row):
        """Is `row` one a correct f64 evaluation may return: its score within the two bounds of the maximum?"""
        i, w = np.searchsorted(self.rows, row), np.searchsorted(self.rows, self.row)
        if i >= len(self.rows) or self.rows[i] != row:
            return False
        return bool(self.score[w] - self.score[i] <= LD(self.bound[w] + self.bound[i]))


@dataclass
class Fit:
    rounds: list
    a_idx: np.ndarray           # sorted by alpha (stable), as em_algo returns them (:768-772)
    b_idx: np.ndarray
    ws: np.ndarray              # f64 [K + 1]
    bic: float
    lb: np.ndarray              # f64 [n_lb]
    near: int = 0
    order: np.ndarray = field(default=None)     # the argsort that was applied
    ws_bound: np.ndarray = field(default=None)  # f64 [K + 1] absolute, in the order of `ws`
    lb_bound: np.ndarray = field(default=None)  # f64 [n_lb] absolute
    bic_bound: float = 0.0


def _log_w(w):
    return LD(SENT) if w <= 0 else np.log(w)


def _column(M, a, b, lw, sent_out):
    """log w + M[a, b, :] and where it is a sentinel (z = 0 exactly).  A weight of 0 makes log w the sentinel (:478); on a
    sentinel entry the sum is then 2 SENT, as in f64 (exp_log_lik sees it when the rescue makes Z non-zero there)."""
    row = M[a, b]
    sent_out[:] = (row == SENT) | (lw == LD(SENT))
    return lw + row.astype(LD)


def em_rounds(M, cnt, unif_ll, theta, betas, L, min_theta, max_unif_ws, a_idx, b_idx, ws, k_arr, nround, fixed=False,
              drop_bin=None, lo_exclusive=False, hi_exclusive=False, sentinel_as_zero=False, last_max=False, rows_to=None,
              e_drop_bin=None, e_drop_col=None, no_rescue=False, rescue_once=False, no_cap=False, cap_inclusive=False,
              fresh_columns=False, untempered=False, exp_zero=None, entropy_plain=False, zero_weight_as_tiny=False):
    """em_algo (:714-779) from a given init on the f64 tensor M [T, B, N]: `nround` rounds at most, the stopping rule
    included.  Returns a Fit; Fit.rounds[i] describes the M-step of round i."""
    _need_long_double()
    M = np.asarray(M, dtype=np.float64)
    n_bic = M.shape[2]
    cnt = np.asarray(cnt, dtype=np.float64)
    if e_drop_bin is not None and 0 <= e_drop_bin < n_bic:
        keep = np.arange(n_bic) != e_drop_bin
        M, cnt = M[:, :, keep], cnt[keep]
    T, B, N = M.shape
    theta, betas = np.asarray(theta, np.float64), np.asarray(betas, np.float64)
    cn = np.asarray(cnt, dtype=np.float64).astype(LD)
    cn64 = cn.astype(np.float64)
    ce, ce64 = (np.ones(N, LD), np.ones(N)) if untempered else (cn, cn64)      # the counts as the exponent has them
    cut = LD(EXP_ZERO if exp_zero is None else exp_zero)
    log_w = (lambda x: np.log(LD(1e-300)) if x <= 0 else np.log(x)) if zero_weight_as_tiny else _log_w
    a = np.array(a_idx, dtype=np.int64)
    b = np.array(b_idx, dtype=np.int64)
    K = len(a)
    C = K + 1
    w = np.asarray(ws, dtype=np.float64)[:C].astype(LD)
    Ew = np.zeros(C)                                     # e(w_c): the init is an input
    logz = np.zeros((N, C), dtype=LD)
    sent = np.zeros((N, C), dtype=bool)
    Elw = np.zeros(C)                                    # E(lw_c) of the column as it stands in logz
    EwF, ElwF = np.zeros(C), np.zeros(C)                 # the same two for the E-step bounds: e(w_c) carried in full

    def refresh(c):
        lw = log_w(w[c])
        Elw[c] = LIB * abs(float(lw)) + Ew[c]
        ElwF[c] = LIB * abs(float(lw)) + EwF[c]
        if c < K:
            logz[:, c] = _column(M, a[c], b[c], lw, sent[:, c])
        else:
            logz[:, c] = lw + LD(unif_ll)
            sent[:, c] = False
        if e_drop_col is not None and c == e_drop_col:
            logz[:, c] = LD(SENT)
            sent[:, c] = True
    for c in range(C):
        refresh(c)
    rounds, lbs, near_all = [], [], 0
    lb_prev = LD(SENT)
    Z = None
    ell_new = d_ell = LD(0)
    with np.errstate(all="ignore"):
        for it in range(nround):
            k = int(k_arr[it])
            near = 0
            for c in (range(C) if fresh_columns else (k,)):
                refresh(c)
            # ---- norm_z (:490-495)
            mx = logz.max(axis=1)
            amx = logz.argmax(axis=1)
            d = logz - mx[:, None]
            arg = d * ce[:, None]
            live = ~sent & (arg >= cut)
            z = np.where(live, np.exp(np.where(live, arg, LD(0))), LD(0))
            s = z.sum(axis=1)
            Zc = z / s[:, None]
            near += int((~sent & (np.abs(arg.astype(np.float64) / EXP_ZERO - 1) < 1e-9)).sum()) + int((mx < LD(SENT) / 2).sum())
            # e(z_c), e(s), e(Z_c) in u
            a_lz = np.abs(logz).astype(np.float64)
            is_mx = np.arange(C)[None, :] == amx[:, None]

            def chain(Elw):
                E_lz = np.where(sent, 0.0, Elw[None, :] + a_lz)
                E_mx = E_lz[np.arange(N), amx]
                E_arg = ce64[:, None] * (E_lz + E_mx[:, None] + np.abs(d).astype(np.float64)) + np.abs(arg).astype(np.float64)
                e_z = np.where(live & ~is_mx, E_arg + EXP_DEV, 0.0)
                e_s = (z * e_z.astype(LD)).sum(axis=1).astype(np.float64) / s.astype(np.float64) + K
                e_Z = np.where(live, e_z + e_s[:, None] + RCP + 1, 0.0)
                return E_lz, E_arg, e_s, e_Z
            _E_lz, _E_arg, _e_s, e_Z = chain(Elw)
            E_lzF, E_argF, e_sF, e_ZF = chain(ElwF)
            # ---- mstep (:525-533): rescue, maximize_ws
            sumk = Zc[:, k].sum()
            near += int(abs(float(sumk) / 1e-8 - 1) < 1e-9)
            rescue = bool(sumk < LD(1e-8)) and not no_rescue
            Z = Zc.copy()
            if rescue:
                Z[:, k] = Z[:, k] + LD(1e-8)
                e_Z[:, k] = e_Z[:, k] + 1
                e_ZF[:, k] = e_ZF[:, k] + 1
            wn = (cn[:, None] * Z).sum(axis=0)
            cz = (cn[:, None] * Z)
            e_w = (cz * (e_Z + 1).astype(LD)).sum(axis=0).astype(np.float64) / np.where(wn > 0, wn, LD(1)).astype(np.float64) + (N - 1) + K + 1
            # the same in full: numerators, their sum, the quotient
            wn64 = wn.astype(np.float64)
            e_WF = (cz * (e_ZF + 1).astype(LD)).sum(axis=0).astype(np.float64) / np.where(wn64 > 0, wn64, 1.0) + (N - 1)
            e_wF = np.where(wn64 > 0, e_WF + float((wn64 * e_WF).sum() / wn64.sum()) + K + 1, 0.0)
            wn = wn / wn.sum()
            near += int(abs(float(wn[K]) / max_unif_ws - 1) < 1e-9)
            capped = bool(wn[K] >= LD(max_unif_ws) if cap_inclusive else wn[K] > LD(max_unif_ws)) and not no_cap
            if capped:
                wk64 = wn[:K].astype(np.float64)
                e_sk = float((wk64 * e_wF[:K]).sum() / wk64.sum()) + max(K - 1, 0) if K else 0.0
                e_wF = np.where(wn64 > 0, e_wF + e_sk + 3, 0.0)
                e_wF[K] = 0.0
                wn[:K] = (LD(1) - LD(max_unif_ws)) * wn[:K] / wn[:K].sum()
                wn[K] = LD(max_unif_ws)
                e_w = e_w + K + 2
            w, Ew, EwF = wn, e_w, e_wF
            v = Z[:, k] * cn
            e_v = e_Z[:, k] + 1
            nz = np.nonzero(v != 0)[0]
            n0, n1 = (int(nz[0]), int(nz[-1]) + 1) if len(nz) else (0, 0)
            rnd = Round(k=k, rescue=rescue, v=v, n0=n0, n1=n1, lw=float(_log_w(w[k])) if k < K else 0.0, rows=np.zeros(0, np.int64),
                        score=np.zeros(0, LD), bound=np.zeros(0), row=-1, ties=np.zeros(0, np.int64), ratio=np.inf, ws=w.copy(),
                        lb=0.0, near=0)
            if not fixed and k < K:
                lo = min_theta if k == 0 else theta[a[k - 1]]
                hi = L if k == K - 1 else theta[a[k + 1]]
                al = np.nonzero((theta >= lo) & (theta <= hi))[0]
                if lo_exclusive:
                    al = al[1:]
                if hi_exclusive:
                    al = al[:-1]
                rows = (al[:, None] * B + np.arange(B)[None, :]).reshape(-1)
                if rows_to is not None:
                    rows = rows[rows < rows_to]
                vs = v.copy()
                if drop_bin is not None and 0 <= drop_bin < N:
                    vs[drop_bin] = LD(0)
                _score_rows(rnd, M.reshape(T * B, N), rows, vs, e_v, _log_w(w[k]), LIB * abs(float(_log_w(w[k]))) + Ew[k],
                            sentinel_as_zero, last_max)
                if rnd.row >= 0:
                    a[k], b[k] = rnd.row // B, rnd.row % B
            # ---- elbo (:559-561) on the logz of this round and the Z the rescue may have changed
            ell_new = _exp_log_lik(logz, Z, cn)
            Zent = Zc if rescue_once else Z
            lb_new = ell_new + _entropy(Zent, cn, entropy_plain)
            rnd.lb, rnd.near = float(lb_new), near
            # ---- the bounds of this round's outputs (module docstring)
            w64, lb64 = w.astype(np.float64), abs(float(lb_new))
            rnd.capped = capped
            rnd.x2 = float(np.max(np.abs(Zent.sum(axis=1) - 1))) if N else 0.0
            rnd.ws_bound = U * (MARGIN * EwF + 1) * w64 + (float(cn64.sum()) + 1) * TINY
            d_ell = _ell_error(logz, Z, cn64, sent, E_lzF, e_ZF)
            d_ent = _entropy_error(Zent, s, arg, is_mx, cn64, K, rescue and not rescue_once, k, E_argF, e_sF, e_ZF)
            rnd.lb_bound = U * (MARGIN * (d_ell + d_ent + lb64) + lb64)
            rnd.bic_bound = _bic_bound(float(ell_new), d_ell, K, n_bic)
            near_all += near
            rounds.append(rnd)
            lbs.append(float(lb_new))
            gap, thr = np.abs(lb_new - lb_prev), np.abs(LD(1e-6) * lb_prev)
            near_all += int(abs(float(gap / thr) - 1) < 1e-9)
            if gap < thr:
                break
            lb_prev = lb_new
        bic = LD(-2) * _exp_log_lik(logz, Z, cn) + LD(3 * K + 1) * np.log(LD(n_bic))
    order = np.argsort(theta[a], kind="stable")
    wout = w.astype(np.float64)
    wout[:K] = wout[:K][order]
    wb = rounds[-1].ws_bound.copy()
    wb[:K] = wb[:K][order]
    return Fit(rounds=rounds, a_idx=a[order], b_idx=b[order], ws=wout, bic=float(bic), lb=np.array(lbs), near=near_all, order=order,
               ws_bound=wb, lb_bound=np.array([r.lb_bound for r in rounds]), bic_bound=rounds[-1].bic_bound)


def _exp_log_lik(logz, Z, cn):
    nzm = Z != 0
    return np.where(nzm, (Z * cn[:, None]) * np.where(nzm, logz, LD(0)), LD(0)).sum()


def _entropy(Z, cn, plain=False):
    pk = Z if plain else Z / Z.sum(axis=1, keepdims=True)
    pos = pk > 0
    return (cn * np.where(pos, -pk * np.log(np.where(pos, pk, LD(1))), LD(0)).sum(axis=1)).sum()


def _ell_error(logz, Z, cn64, sent, E_lz, e_Z):
    """|d ell| in u (module docstring): the terms' own errors and (terms - 1) sum |t| for the additions."""
    nzm = Z != 0
    zc = np.where(nzm, Z, LD(0)).astype(np.float64) * cn64[:, None]
    a_lz = np.where(nzm, np.abs(logz), LD(0)).astype(np.float64)
    at = zc * a_lz
    E = np.where(sent, a_lz, E_lz)
    return float((at * (e_Z + 2)).sum() + (zc * E).sum() + max(int(nzm.sum()) - 1, 0) * at.sum())


def _entropy_error(Z, s, arg, is_mx, cn64, K, rescue, k, E_arg, e_s, e_Z):
    """|d ent| in u (module docstring), for the closed form of estep_body on the row sums s and s2."""
    s2 = Z.sum(axis=1)
    x2 = np.abs(s2 - 1).astype(np.float64)
    pk = Z / s2[:, None]
    pos = pk > 0
    L = np.abs(np.log(np.where(pos, pk, LD(1)))).astype(np.float64)
    ls = np.abs(np.log(s)).astype(np.float64)
    X2 = 2 * K + RCP + 1 + (1 if rescue else 0)
    E_ls2 = X2 + ((3 * x2 + x2 ** 3 / (3 * U)) if rescue else 0.0)
    a_arg = np.where(pos, np.abs(arg), LD(0)).astype(np.float64)
    E_L = np.where(is_mx, 0.0, E_arg) + (e_s + LOG_DEV * ls + E_ls2)[:, None] + (a_arg + ls[:, None]) + L
    if rescue:
        zk = np.abs(np.log(np.where(Z[:, k] > 0, Z[:, k], LD(1)))).astype(np.float64)
        E_L[:, k] = e_Z[:, k] + LIB * zk + E_ls2 + L[:, k]
    e_pk = e_Z + X2 + RCP + 1
    p64 = np.where(pos, pk, LD(0)).astype(np.float64) * cn64[:, None]
    t = p64 * L
    return float((t * (e_pk + 2)).sum() + (p64 * np.where(pos, E_L, 0.0)).sum() + max(int(pos.sum()) - 1, 0) * t.sum())


def _bic_bound(ell, d_ell, K, N):
    pen = (3 * K + 1) * float(np.log(float(N)))
    bic = abs(-2 * ell + pen)
    return U * (MARGIN * (2 * d_ell + (LIB + 1) * pen + bic) + bic)


def _score_rows(rnd, M2, rows, v, e_v, lw, E_lw, sentinel_as_zero, last_max):
    """Scores, bounds, winner, tie set and decision ratio of one M-step into `rnd`."""
    rnd.rows = rows
    if len(rows) == 0:
        return
    sup = np.nonzero(v != 0)[0]                          # terms with v == 0 add exactly 0 on the device and here
    Mw = M2[rows][:, sup]                                # f64 [R, n_sup]
    vs, ev = v[sup], e_v[sup]
    sm = Mw == SENT
    if sentinel_as_zero:
        Ml = np.where(sm, LD(0), Mw.astype(LD))
    else:
        Ml = Mw.astype(LD)
    mv = Ml * vs[None, :]
    sv = vs.sum()
    score = lw * sv + mv.sum(axis=1)
    # ---- the bound (module docstring), f64 arithmetic is enough for it
    amv = np.abs(mv).astype(np.float64)
    v64, sv64, alw = vs.astype(np.float64), float(sv), abs(float(lw))
    n = len(sup)
    d_sv = float((v64 * ev).sum()) + (n - 1) * sv64
    tl = np.where(sm & (not sentinel_as_zero), v64[None, :], 0.0)
    tl_sum = tl.sum(axis=1)
    d_tl = (tl * ev[None, :]).sum(axis=1) + np.maximum(sm.sum(axis=1) - 1, 0) * tl_sum
    c0 = np.abs(float(lw * sv) + SENT * tl_sum)
    b_c0 = alw * d_sv + E_lw * sv64 + alw * sv64 + abs(SENT) * (d_tl + tl_sum) + c0
    b_acc = np.abs(np.cumsum(mv.astype(np.float64), axis=1)).sum(axis=1) + (amv * ev[None, :]).sum(axis=1)
    bound = MARGIN * U * (b_c0 + b_acc + np.abs(score).astype(np.float64))
    rnd.score, rnd.bound = score, bound
    first = int(np.argmax(score))                        # np.argmax: the first maximum
    same = np.all(Mw == Mw[first][None, :], axis=1)      # bit-identical on the support of v: tied in exact arithmetic
    ties = rows[same]
    win = int(np.nonzero(same)[0][-1]) if last_max else first
    rnd.row, rnd.ties = int(rows[win]), ties
    rest = ~same
    if rest.any():
        gap = (score[first] - score[rest]).astype(np.float64)
        rnd.ratio = float(np.min(gap / (bound[first] + bound[rest])))
    else:
        rnd.ratio = np.inf
