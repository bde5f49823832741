"""Long-double restatement of get_label on a GIVEN f64 marginal tensor, with the per-bin arg-max laid open.

TEST INFRASTRUCTURE ONLY, like ``mstep_reference.py``: written from the reference's ``apa_core.py:473-495`` and
``:873-881`` (cal_z_k, norm_z, get_label) and evaluated in ``np.longdouble`` (64-bit mantissa).  The tensor, ``cnt``,
``unif_ll`` and the model tables are f64 inputs; nothing is built here.

Decision variables of bin n, columns c = 0..K of the model (K, a, b, ws):
    lz[n, c] = log(ws[c]) + M[a_c, b_c, n]   (c < K)          lz[n, K] = log(ws[K]) + unif_ll
with the sentinel SENT in place of the log where ws[c] <= 0 (d_logw).  The label is the arg-max of Z = z / sum z,
z = exp((lz - max lz) cnt), the FIRST maximum (np.argmax, :880): a monotone image of lz, so the label is the first
arg-max of lz wherever the f64 evaluation keeps the order of the two best columns.

Sentinel-class columns.  A column with lz <= SENT / 2 (the bin outside the component's window, a weight of 0, or both)
is evaluated in f64, as the device and numpy do: log w + SENT rounds to SENT, SENT + SENT is 2 SENT, and among equal
f64 values the first column wins.  Long double must not separate what f64 cannot; such a value carries no error here.

The bound.  Notation of mstep_reference.py: u = 2^-53; E(q) the absolute error of a log-domain quantity, e(q) the
relative error of a positive one, both in units of u; a library or device function of e ulp costs 2 e u.  The device's
sequence (k_labels), for a column c of a bin with count cnt and mx the computed row maximum:
    lw_c  = log w_c  (d_logw: library log)    E(lw_c)  = LIB |lw_c|                       the weight is an input
    lz_c  = lw_c + M_c                        E(lz_c)  = E(lw_c) + |lz_c|                 one rounding
    d_c   = lz_c - mx                         E(d_c)   = E(lz_c) + |d_c|                  mx is ONE f64 number, subtracted from
                                                                                          every column: its own error moves no order
    arg_c = d_c cnt                           E(arg_c) = cnt E(d_c) + |arg_c|
    z_c   = d_exp_nonpos(arg_c)               e(z_c)   = E(arg_c) + EXP_DEV
    Z_c   = z_c / s                           e(Z_c)   = e(z_c) + 1                       the divisor s is the same for every
                                                                                          column: it cannot reorder, only its
                                                                                          rounding can merge values within an ulp
The computed Z_c and Z_d keep the order of lz_c > lz_d, strictly, when cnt (lz_c - lz_d) > u (e(Z_c) + e(Z_d)), that is when
    lz_c - lz_d  >  u [E(lz_c) + E(lz_d) + 2 |d_c| + 2 |d_d| + (2 EXP_DEV + 2) / cnt]
(|arg| / cnt = |d|).  The right-hand side times MARGIN = 2, for the second-order terms, is bound(c, d); for the best
column d_c = 0.  A loser whose argument falls below the clamp of d_exp_nonpos has z = 0 exactly against the winner's 1:
the first-order chain does not apply there and is not needed.  For orientation: |lz| is 20 to 40 and |lw| below 3 on the
ladder, so the bound of a pair is about 1.5e-14 at cnt = 1.

Every bin is one of three kinds:
    DECIDED  the best column beats every column outside its tie set by more than bound(best, d): the label is the arg-max
    TIE      the same, and the tie set has more than one column - columns IDENTICAL BY CONSTRUCTION: the same tensor value
             at the bin with the same weight bits, or sentinel-class and equal in f64.  The label is the first of them
    NEAR     some other column lies within its bound of the best: either is acceptable (``accept``).  The ladder of
             tests/label_ladder.py holds no such bin; the kind exists to report a broken case honestly.

Named perturbations (PERTURBATIONS) - WRONG labellings expressed in the reference, to show that a ladder case sits on the
boundary it names.  The model is read from the call's padded tables (a, b: [n_sel, kmax]; w: [n_sel, kmax + 1]) at row sel:
    last_max              >= in place of >: the last of the tied maxima
    pitch_N               the tensor's rows read at pitch N in place of Np = N rounded up to PITCH (padding bins hold SENT)
    drop_b                row a B in place of a B + b
    uniform_as_component  column K read from the tensor's row 0 (c < K -> c <= K with roff = 0), not from unif_ll
    k_pitch_plus1         a and b read at pitch kmax + 1                w_pitch_k       the weights read at pitch kmax
                          (an entry beyond the table reads as 0; an alpha beyond the UTR's grid as its last)
    drop_last_bin         the bin loop ends at N - 1                    first_block_only   no stride beyond bin BLOCK - 1
                          (bins without a label keep the caller's -1)
    zero_weight_as_one    a weight of 0 gives log w = 0, not the sentinel
    sentinel_as_zero      a sentinel entry of the tensor read as 0
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from .mstep_reference import EXP_DEV, LD, LIB, MARGIN, SENT, U, _need_long_double

PITCH = 16                              # row pitch of the device tensor: pinned to the source by tests/test_host.py
BLOCK = 256                             # threads of k_labels: pinned likewise
PERTURBATIONS = ("last_max", "pitch_N", "drop_b", "uniform_as_component", "k_pitch_plus1", "w_pitch_k", "drop_last_bin",
                 "first_block_only", "zero_weight_as_one", "sentinel_as_zero")
DECIDED, TIE, NEAR = 0, 1, 2


@dataclass
class Labels:
    label: np.ndarray           # int64 [N]; -1 where a perturbation leaves the bin without a label
    kind: np.ndarray            # uint8 [N]: DECIDED / TIE / NEAR
    accept: np.ndarray          # bool [N, K + 1]: the labels a correct f64 evaluation may return (one per bin unless NEAR)
    second: np.ndarray          # int64 [N]: the column outside the tie set with the smallest gap / bound; -1 without one
    gap: np.ndarray             # f64 [N]: lz[best] - lz[second]; inf without one
    bound: np.ndarray           # f64 [N]: bound(best, second), MARGIN included; 0 without one
    lz: np.ndarray              # long double [N, K + 1] (sentinel-class entries: their f64 value)
    arg: np.ndarray             # f64 [N, K + 1]: (lz - max lz) cnt, what d_exp_nonpos is given

    @property
    def near(self):
        return int((self.kind == NEAR).sum())

    @property
    def ratio(self):
        """Smallest gap / bound over the bins (inf where no bin has a second column)."""
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(self.second >= 0, self.gap / np.where(self.bound > 0, self.bound, 1.0), np.inf)
        return float(r.min()) if len(r) else np.inf


def _entry(flat, i):
    return flat[i] if 0 <= i < len(flat) else flat.dtype.type(0)


def label_call(M, cnt, unif_ll, sel, sel_K, a, b, w, perturb=None):
    """get_label for row `sel` of a call's padded model tables on the f64 tensor M [T, B, N] of that row's UTR."""
    _need_long_double()
    assert perturb is None or perturb in PERTURBATIONS, perturb
    M = np.asarray(M, dtype=np.float64)
    T, B, N = M.shape
    M2 = M.reshape(T * B, N)
    cn = np.asarray(cnt, dtype=np.float64)
    a, b, w = np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64), np.asarray(w, dtype=np.float64)
    kmax = a.shape[1]
    assert a.shape == b.shape and w.shape == (a.shape[0], kmax + 1)
    K = int(np.asarray(sel_K)[sel])
    C = K + 1
    pk = kmax + 1 if perturb == "k_pitch_plus1" else kmax
    pw = kmax if perturb == "w_pitch_k" else kmax + 1
    ai = [min(max(int(_entry(a.reshape(-1), sel * pk + c)), 0), T - 1) for c in range(K)]
    bi = [min(max(int(_entry(b.reshape(-1), sel * pk + c)), 0), B - 1) for c in range(K)]
    ws = np.array([float(_entry(w.reshape(-1), sel * pw + c)) for c in range(C)])
    # ---- the tensor value each column reads at each bin
    if perturb == "pitch_N":
        Np = (N + PITCH - 1) // PITCH * PITCH
        pad = np.full((T * B, Np), SENT)
        pad[:, :N] = M2
        flat = pad.reshape(-1)
        read = lambda row: flat[row * N + np.arange(N)]             # noqa: E731
    else:
        read = lambda row: M2[row]                                   # noqa: E731
    data = np.empty((N, C))
    for c in range(K):
        data[:, c] = read(ai[c] * B + (0 if perturb == "drop_b" else bi[c]))
    data[:, K] = read(0) if perturb == "uniform_as_component" else unif_ll
    if perturb == "sentinel_as_zero":
        data = np.where(data == SENT, 0.0, data)
    # ---- lz in long double; sentinel-class entries in f64
    zero_lw = 0.0 if perturb == "zero_weight_as_one" else SENT
    with np.errstate(all="ignore"):
        lw64 = np.array([zero_lw if x <= 0 else float(np.log(x)) for x in ws])
        lwl = np.array([LD(zero_lw) if x <= 0 else np.log(LD(x)) for x in ws], dtype=LD)
        lz64 = lw64[None, :] + data
        lz = lwl[None, :] + data.astype(LD)
        sc = lz <= LD(SENT) / 2
        lz = np.where(sc, lz64.astype(LD), lz)
    best = np.argmax(lz, axis=1) if N else np.zeros(0, np.int64)        # the first maximum
    rows = np.arange(N)
    mx = lz[rows, best]
    d = lz - mx[:, None]
    # identical by construction: the same value read with the same weight, or sentinel-class and equal in f64
    same = ((data == data[rows, best][:, None]) & (ws[None, :] == ws[best][:, None])) | (sc & sc[rows, best][:, None] & (d == 0))
    # ---- the bound of every column against the best (module docstring), f64 is enough for it
    E_lz = np.where(sc, 0.0, LIB * np.abs(lw64)[None, :] + np.abs(lz).astype(np.float64))
    ad = np.abs(d).astype(np.float64)
    with np.errstate(over="ignore"):
        bound = MARGIN * U * (E_lz + E_lz[rows, best][:, None] + 2 * ad + (2 * EXP_DEV + 2) / cn[:, None])
    gap = ad
    rest = ~same
    within = rest & (gap <= bound)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(rest, gap / bound, np.inf)
    second = np.where(rest.any(axis=1), np.argmin(r, axis=1), -1) if N else np.zeros(0, np.int64)
    has = second >= 0
    s_ix = np.where(has, second, 0)
    kind = np.where(within.any(axis=1), NEAR, np.where(same.sum(axis=1) > 1, TIE, DECIDED)).astype(np.uint8)
    label = best.astype(np.int64).copy()
    if perturb == "last_max":
        label = (C - 1 - np.argmax(same[:, ::-1], axis=1)).astype(np.int64)
    accept = within.copy()
    accept[rows, label] = True
    if perturb == "drop_last_bin" and N:
        label[N - 1] = -1
    if perturb == "first_block_only":
        label[BLOCK:] = -1
    with np.errstate(over="ignore", invalid="ignore"):
        arg = (d.astype(np.float64)) * cn[:, None]
    return Labels(label=label, kind=kind, accept=accept, second=second.astype(np.int64),
                  gap=np.where(has, gap[rows, s_ix], np.inf), bound=np.where(has, bound[rows, s_ix], 0.0), lz=lz, arg=arg)


def label_model(M, cnt, unif_ll, K, a_idx, b_idx, ws, perturb=None):
    """get_label for one model given alone: a one-row table of pitch max(1, K)."""
    kmax = max(1, int(K))
    a, b, w = np.zeros((1, kmax), np.int64), np.zeros((1, kmax), np.int64), np.zeros((1, kmax + 1))
    a[0, :K], b[0, :K], w[0, :K + 1] = np.asarray(a_idx)[:K], np.asarray(b_idx)[:K], np.asarray(ws)[:K + 1]
    return label_call(M, cnt, unif_ll, 0, [K], a, b, w, perturb)
