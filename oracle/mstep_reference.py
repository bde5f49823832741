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
first-order BOUND per row on how far a correct f64 evaluation by the device's sequence (em_lockstep.inc: estep_body,
k2_mstep; mstep_ring.inc; mstep_multi.inc) may lie from S(row).  A round is DECIDED when the winner beats every row
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


def _log_w(w):
    return LD(SENT) if w <= 0 else np.log(w)


def _column(M, a, b, lw, sent_out):
    """log w + M[a, b, :] and where it is a sentinel (z = 0 exactly).  A weight of 0 makes log w the sentinel (:478); on a
    sentinel entry the sum is then 2 SENT, as in f64 (exp_log_lik sees it when the rescue makes Z non-zero there)."""
    row = M[a, b]
    sent_out[:] = (row == SENT) | (lw == LD(SENT))
    return lw + row.astype(LD)


def em_rounds(M, cnt, unif_ll, theta, betas, L, min_theta, max_unif_ws, a_idx, b_idx, ws, k_arr, nround, fixed=False,
              drop_bin=None, lo_exclusive=False, hi_exclusive=False, sentinel_as_zero=False, last_max=False, rows_to=None):
    """em_algo (:714-779) from a given init on the f64 tensor M [T, B, N]: `nround` rounds at most, the stopping rule
    included.  Returns a Fit; Fit.rounds[i] describes the M-step of round i."""
    _need_long_double()
    M = np.asarray(M, dtype=np.float64)
    T, B, N = M.shape
    theta, betas = np.asarray(theta, np.float64), np.asarray(betas, np.float64)
    cn = np.asarray(cnt, dtype=np.float64).astype(LD)
    cn64 = cn.astype(np.float64)
    a = np.array(a_idx, dtype=np.int64)
    b = np.array(b_idx, dtype=np.int64)
    K = len(a)
    C = K + 1
    w = np.asarray(ws, dtype=np.float64)[:C].astype(LD)
    Ew = np.zeros(C)                                     # e(w_c): the init is an input
    logz = np.zeros((N, C), dtype=LD)
    sent = np.zeros((N, C), dtype=bool)
    Elw = np.zeros(C)                                    # E(lw_c) of the column as it stands in logz

    def refresh(c):
        lw = _log_w(w[c])
        Elw[c] = LIB * abs(float(lw)) + Ew[c]
        if c < K:
            logz[:, c] = _column(M, a[c], b[c], lw, sent[:, c])
        else:
            logz[:, c] = lw + LD(unif_ll)
            sent[:, c] = False
    for c in range(C):
        refresh(c)
    rounds, lbs, near_all = [], [], 0
    lb_prev = LD(SENT)
    Z = None
    with np.errstate(all="ignore"):
        for it in range(nround):
            k = int(k_arr[it])
            near = 0
            refresh(k)
            # ---- norm_z (:490-495)
            mx = logz.max(axis=1)
            amx = logz.argmax(axis=1)
            d = logz - mx[:, None]
            arg = d * cn[:, None]
            live = ~sent & (arg >= LD(EXP_ZERO))
            z = np.where(live, np.exp(np.where(live, arg, LD(0))), LD(0))
            s = z.sum(axis=1)
            Zc = z / s[:, None]
            # e(z_c), e(s), e(Z_c) in u
            a_lz = np.abs(logz).astype(np.float64)
            E_lz = np.where(sent, 0.0, Elw[None, :] + a_lz)
            E_mx = E_lz[np.arange(N), amx]
            is_mx = np.arange(C)[None, :] == amx[:, None]
            E_arg = cn64[:, None] * (E_lz + E_mx[:, None] + np.abs(d).astype(np.float64)) + np.abs(arg).astype(np.float64)
            e_z = np.where(live & ~is_mx, E_arg + EXP_DEV, 0.0)
            e_s = (z * e_z.astype(LD)).sum(axis=1).astype(np.float64) / s.astype(np.float64) + K
            e_Z = np.where(live, e_z + e_s[:, None] + RCP + 1, 0.0)
            # ---- mstep (:525-533): rescue, maximize_ws
            sumk = Zc[:, k].sum()
            near += int(abs(float(sumk) / 1e-8 - 1) < 1e-9)
            rescue = bool(sumk < LD(1e-8))
            Z = Zc.copy()
            if rescue:
                Z[:, k] = Z[:, k] + LD(1e-8)
                e_Z[:, k] = e_Z[:, k] + 1
            wn = (cn[:, None] * Z).sum(axis=0)
            cz = (cn[:, None] * Z)
            e_w = (cz * (e_Z + 1).astype(LD)).sum(axis=0).astype(np.float64) / np.where(wn > 0, wn, LD(1)).astype(np.float64) + (N - 1) + K + 1
            wn = wn / wn.sum()
            near += int(abs(float(wn[K]) / max_unif_ws - 1) < 1e-9)
            if wn[K] > LD(max_unif_ws):
                wn[:K] = (LD(1) - LD(max_unif_ws)) * wn[:K] / wn[:K].sum()
                wn[K] = LD(max_unif_ws)
                e_w = e_w + K + 2
            w, Ew = wn, e_w
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
            lb_new = _exp_log_lik(logz, Z, cn) + _entropy(Z, cn)
            rnd.lb, rnd.near = float(lb_new), near
            near_all += near
            rounds.append(rnd)
            lbs.append(float(lb_new))
            gap, thr = np.abs(lb_new - lb_prev), np.abs(LD(1e-6) * lb_prev)
            near_all += int(abs(float(gap / thr) - 1) < 1e-9)
            if gap < thr:
                break
            lb_prev = lb_new
        bic = LD(-2) * _exp_log_lik(logz, Z, cn) + LD(3 * K + 1) * np.log(LD(N))
    order = np.argsort(theta[a], kind="stable")
    wout = w.astype(np.float64)
    wout[:K] = wout[:K][order]
    return Fit(rounds=rounds, a_idx=a[order], b_idx=b[order], ws=wout, bic=float(bic), lb=np.array(lbs), near=near_all, order=order)


def _exp_log_lik(logz, Z, cn):
    nzm = Z != 0
    return np.where(nzm, (Z * cn[:, None]) * np.where(nzm, logz, LD(0)), LD(0)).sum()


def _entropy(Z, cn):
    pk = Z / Z.sum(axis=1, keepdims=True)
    pos = pk > 0
    return (cn * np.where(pos, -pk * np.log(np.where(pos, pk, LD(1))), LD(0)).sum(axis=1)).sum()


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
