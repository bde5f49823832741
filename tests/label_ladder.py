"""The ladder of tests/test_label_ladder.py and tests/test_label_reference.py: small batches of UTRs, models and label
calls that put the bin count, the column count, the table pitch, the gap between the two best columns, exact ties, zero
and tiny weights, the counts and the shape of the call on both sides of every boundary of k_labels (scape_hip.hip) and
of the copy-back in scape_hip_batch_labels.  tests/test_host.py reads the boundaries from the sources and checks the
ladder against them.

UTRs come from mstep_ladder.make_utr (UtrPrep objects built directly: N is exactly what a case says, T is about 219,
B = 13); where a case needs particular counts they are set on the UtrPrep after it is made (the tensor does not depend
on them).  Every seed and hand-placed index in the tables below was searched for on the CPU against the C oracle's
tensor (find_seed, find_rows) so that every case meets the conditions which tests/test_label_reference.py checks again
on every run and tests/test_label_ladder.py once more on the device's own tensor:
  (a) no NEAR bin anywhere (oracle/label_reference.py): every bin of every model is DECIDED or an exact TIE by
      construction - a condition on the inputs, not a tolerance;
  (b) every perturbation a model lists - the wrong labelling its boundary is about - changes the label of at least one
      bin that is not NEAR with or without it, in at least one of the calls that hold the model;
  (c) each planted bin's two signs give two different labels: c0 for +g, c1 for -g.

The planted family is the sharp one.  For a bin n*, two columns c0 < c1 finite there and a sign, plant_weights()
computes the weights in long double FROM THE TENSOR THE TEST IS JUDGED ON, so that lz[n*, c0] - lz[n*, c1] = +-g with
g = TIGHT x the bin's margined bound and every other column at least 3 below.  The CPU half feeds it the oracle's tensor,
the GPU half the device's own: the two tensors differ by about 1e-13 relative, far more than g.

TIGHT = 2: the smallest power of two for which the C oracle (plain f64, library exp and log, so_get_label) returns the
planted label on every planted bin of the ladder on the CPU AND the bins are decided.  The evidence, on the oracle's
tensor, over the 148 planted bins (144 of the planted family, 4 of the counts family; tests/test_label_reference.py
measures it again on every run and prints it): the oracle's wrong labels at TIGHT = 2, 1, 1/2, 1/4, 1/8 are 0, 0, 0, 13,
36.  Plain f64 holds down to half the margined bound - the first-order bound is honest, and loose by the factor of four
that MARGIN and worst-case signs make - but a planted bin is DECIDED only when its gap EXCEEDS its bound (condition (a)),
which no TIGHT <= 1 gives: at 1 the gap is the bound up to the rounding of a weight and the bins come out NEAR.  So 2 it
is.  A device label that disagrees at this TIGHT is a finding about k_labels, not grounds to raise it.
"""
from dataclasses import dataclass, field

import numpy as np

import mstep_ladder as ml
from mstep_ladder import betas_for, make_utr, oracle_tensor          # noqa: F401  (the ladder's own vocabulary)

CLASSES = (8, 16, 32, 64)                         # LabelClasses: pinned to the source by tests/test_host.py
BLOCK = 256                                       # threads of k_labels (launch bounds and launch)
PITCH = 16                                        # Np = N rounded up to this
EXP_CLAMP = -750.0                                # d_exp_nonpos: arguments below give exactly 0
CLASS_A_HI = 120                                  # classes: alphas below this index, so that the last bins lie beyond every window and go to the uniform column
KMAX_PAD = 63                                     # the padded table pitch: SCAPE_MAX_K
TIGHT = 2.0
OTHERS_BELOW = 3.0                                # planted bins: every other column at least this far below the pair

N_BINS = (1, 15, 16, 17, 63, 64, 65, 255, 256, 257, 513)
K_CLASSES = (0, 1, 6, 7, 8, 14, 15, 16, 30, 31, 32, 62, 63)
# (K, c0, c1): two components at K = c1 + 1, and (K - 1, K) - a component against the uniform column
PLANT_PAIRS = ((2, 0, 1), (8, 6, 7), (9, 7, 8), (17, 15, 16), (33, 31, 32), (63, 61, 62),
               (1, 0, 1), (7, 6, 7), (8, 7, 8), (16, 15, 16), (32, 31, 32), (63, 62, 63))
PLANT_N = 257
PLANT_BINS = (0, 255, 256)                        # 0, the last of the first trip, the first of the second = N - 1
PLANT_COUNTS = (1, 60)                            # 60: make_utr's largest count
COUNT_MAX = 1000
COUNT_BIN = 100
TIE_PAIRS = ((2, 0, 1), (8, 6, 7), (9, 7, 8), (17, 15, 16), (33, 31, 32), (63, 61, 62))
CALL_N = (17, 257, 64, 513)
CALL_K = ((1, 7, 16, 63), (8, 0, 33, 15))         # model sets A and B: K per UTR

# ---- the tables (found with find_seed / find_rows against the C oracle's tensor; checked again by every test run)
BIN_SEEDS = {1: 3, 15: 0, 16: 0, 17: 2, 63: 0, 64: 0, 65: 0, 255: 0, 256: 0, 257: 0, 513: 0}
CLASS_SEEDS = {0: 0, 1: 0, 6: 0, 7: 0, 8: 0, 14: 0, 15: 0, 16: 0, 30: 0, 31: 0, 32: 0, 62: 0, 63: 0}
# rows (alpha index, beta index), a > 0 and b > 0, well inside their window at the bin (M > -40): the planted pair's columns
PLANT_ROWS = {0: ((30, 12), (55, 6)), 255: ((160, 11), (187, 11)), 256: ((161, 9), (188, 7)), COUNT_BIN: ((90, 7), (116, 3))}
TIE_ROW = (127, 12)                               # the row the tied columns share: finite on many bins
DEAD_ROWS = ((2, 8), (4, 7))                      # rows whose window misses bin 0 (the tensor holds the sentinel there)
ZERO_ROWS = ((127, 12), (160, 11))                 # (the row that would win with a weight, a weaker one)
TINY_ROWS = ((145, 3), (25, 3))                   # (the 1e-300 row, a row that is a sentinel on some bins where the first is finite)
COUNT_SEED = 0
CALL_SEEDS = ((0, 0, 0, 0), (0, 0, 0, 0))


@dataclass(eq=False)
class Model:
    u: int
    K: int
    a_idx: np.ndarray
    b_idx: np.ndarray
    ws: np.ndarray                     # planted models: the base weights plant_weights() starts from
    perturb: tuple = ()                # names of oracle/label_reference.py: PERTURBATIONS
    plant: tuple = None                # (bin, c0, c1, sign)
    note: str = ""


@dataclass
class Case:
    name: str
    boundary: str
    preps: list
    models: list
    calls: tuple                       # tuples of model indices in sel order, run in this order on one handle
    facts: dict = field(default_factory=dict)


def random_model(q, K, seed, u=0, perturb=(), note="", a_hi=None):
    """K distinct alphas in [1, a_hi) (ascending; a_hi: the grid's end), betas > 0, random weights: with a > 0 and b > 0 a
    wrong row pitch and a dropped beta index read other rows."""
    rs = np.random.RandomState(seed)
    if K == 0:
        return Model(u, 0, np.zeros(0, np.int32), np.zeros(0, np.int32), np.array([ml.P0["max_unif_ws"]]), tuple(perturb), None, note)
    a = np.sort(rs.choice(np.arange(1, q.T if a_hi is None else a_hi), size=K, replace=False)).astype(np.int32)
    b = rs.randint(1, len(q.betas), size=K).astype(np.int32)
    return Model(u, K, a, b, ml.random_ws(K, rs), tuple(perturb), None, note)


def planted_model(q, K, c0, c1, n, sign, u=0, note=""):
    """A random model whose columns c0 and c1 sit on the bin's PLANT_ROWS; the weights come from plant_weights()."""
    m = random_model(q, K, 7000 + 100 * K + n, u, note=note or f"K={K} ({c0}, {c1}) bin {n} {'+' if sign > 0 else '-'}g")
    for c, (a, b) in zip((c0, c1), PLANT_ROWS[n]):
        if c < K:
            m.a_idx[c], m.b_idx[c] = a, b
    m.plant = (n, c0, c1, sign)
    return m


def plant_weights(M, cnt, unif_ll, m, tight=None):
    """The weights of a planted model on the tensor M: lz[n, c0] - lz[n, c1] = sign * tight * bound(c0, c1) in long double
    (up to the rounding of the weight to f64: 1e-16), every other column at least OTHERS_BELOW under lz[n, c1]."""
    from oracle import label_reference as lr
    LD = lr.LD
    tight = TIGHT if tight is None else tight
    n, c0, c1, sign = m.plant
    K = m.K
    dat = np.array([M[m.a_idx[c], m.b_idx[c], n] for c in range(K)] + [unif_ll], dtype=np.float64)
    assert dat[c0] > -60 and dat[c1] > -60, (m.note, "a planted column is not inside its window at the bin")
    w = np.asarray(m.ws, dtype=np.float64).copy()
    lz1 = np.log(LD(w[c1])) + LD(dat[c1])
    rest = [c for c in range(K + 1) if c not in (c0, c1)]
    if rest:
        top = max(np.log(LD(w[c])) + LD(dat[c]) for c in rest)
        w[rest] = w[rest] * float(np.exp(min(LD(0), lz1 - LD(OTHERS_BELOW) - top)))
    w[c0] = float(np.exp(lz1 - LD(dat[c0])))                        # gap 0: the bound of the pair at these weights
    r = lr.label_model(M, cnt, unif_ll, K, m.a_idx, m.b_idx, w)
    assert int(r.second[n]) in (c0, c1) and r.bound[n] > 0, (m.note, int(r.second[n]))
    g = LD(tight) * LD(r.bound[n])
    w[c0] = float(np.exp(lz1 + LD(sign) * g - LD(dat[c0])))
    return w


def resolve(case, Ms, tight=None):
    """The weights of every model of the case on the tensors Ms (one per UTR)."""
    return [plant_weights(Ms[m.u], case.preps[m.u].cnt, case.preps[m.u].unif_ll, m, tight) if m.plant else np.asarray(m.ws, np.float64)
            for m in case.models]


def pitches(case, call):
    """The table pitches a call runs at: its own (kmax = max(1, K)) and the padded one."""
    own = max(1, max(case.models[i].K for i in call))
    return (own, KMAX_PAD) if own != KMAX_PAD else (own,)


def pack(case, call, kmax, ws):
    """The call's tables at pitch kmax: (sel_utr, sel_K, a, b, w).  What lies beyond a model's K is junk a kernel must
    not read: in-range indices, not zeros, and weights large enough to win."""
    rs = np.random.RandomState(1000 * kmax + 10 * len(call) + call[0])
    n, B = len(call), len(case.preps[0].betas)
    a = rs.randint(1, min(q.T for q in case.preps), size=(n, kmax)).astype(np.int32)
    b = rs.randint(1, B, size=(n, kmax)).astype(np.int32)
    w = rs.uniform(0.5, 5.0, size=(n, kmax + 1))
    for i, mi in enumerate(call):
        m = case.models[mi]
        a[i, :m.K], b[i, :m.K], w[i, :m.K + 1] = m.a_idx, m.b_idx, ws[mi]
    return (np.array([case.models[i].u for i in call], np.int32), np.array([case.models[i].K for i in call], np.int32), a, b, w)


def reference(case, Ms, ws, mi, perturb=None, call=None, kmax=None):
    """The reference's labels of model mi: alone, or as a row of `call` packed at pitch kmax."""
    from oracle import label_reference as lr
    m = case.models[mi]
    q = case.preps[m.u]
    if call is None:
        return lr.label_model(Ms[m.u], q.cnt, q.unif_ll, m.K, m.a_idx, m.b_idx, ws[mi], perturb)
    _su, sk, a, b, w = pack(case, call, kmax, ws)
    return lr.label_call(Ms[m.u], q.cnt, q.unif_ll, list(call).index(mi), sk, a, b, w, perturb)


def bites(case, Ms, ws, mi, base, name):
    """Condition (b) for one model and one perturbation."""
    from oracle import label_reference as lr
    for call in case.calls:
        if mi in call:
            for kmax in pitches(case, call):
                p = reference(case, Ms, ws, mi, name, call, kmax)
                if np.any((base.kind != lr.NEAR) & (p.kind != lr.NEAR) & (p.label != base.label)):
                    return True
    return False


def check_case(case, Ms, tight=None):
    """Conditions (a) to (c) on the tensors Ms: (problems, the weights, the unperturbed Labels per model, statistics)."""
    from oracle import label_reference as lr
    ws = resolve(case, Ms, tight)
    problems, refs = [], []
    stat = dict(bins=0, near=0, tie=0, bound=0.0, ratio=np.inf)
    for mi, m in enumerate(case.models):
        r = reference(case, Ms, ws, mi)
        refs.append(r)
        stat["bins"] += len(r.label)
        stat["near"] += r.near
        stat["tie"] += int((r.kind == lr.TIE).sum())
        fin = r.second >= 0
        if fin.any():
            stat["bound"] = max(stat["bound"], float(r.bound[fin & (r.gap < 1e30)].max(initial=0.0)))
            stat["ratio"] = min(stat["ratio"], r.ratio)
        if r.near:
            problems.append((case.name, mi, m.note, "near bins", np.nonzero(r.kind == lr.NEAR)[0][:5].tolist()))
        if m.plant:
            n, c0, c1, sign = m.plant
            want = c0 if sign > 0 else c1
            lo = min(float(r.lz[n, want] - r.lz[n, c]) for c in range(m.K + 1) if c not in (c0, c1)) if m.K + 1 > 2 else np.inf
            if int(r.label[n]) != want or r.kind[n] != lr.DECIDED or int(r.second[n]) != c0 + c1 - want or lo < OTHERS_BELOW - 1e-6:
                problems.append((case.name, mi, m.note, "the planted bin", int(r.label[n]), int(r.kind[n]), int(r.second[n]), lo))
        for name in m.perturb:
            if not bites(case, Ms, ws, mi, r, name):
                problems.append((case.name, mi, m.note, f"{name} changes no bin"))
    return problems, ws, refs, stat


def oracle_labels(q, M, m, ws):
    """so_get_label (plain f64) for one model on the tensor M."""
    import ctypes
    from oracle import scape_oracle as so
    lab = np.zeros(q.N, dtype=np.int64)
    f = lambda v: np.ascontiguousarray(v, dtype=np.float64)           # noqa: E731
    th, be, cnt, Mc = f(q.theta), f(q.betas), f(q.cnt), f(M)
    al, bt, w = f(q.theta[m.a_idx]), f(q.betas[m.b_idx]), f(ws)
    so.lib().so_get_label(so._p(Mc), ctypes.c_int(q.T), ctypes.c_int(len(be)), ctypes.c_int(q.N), so._p(th), so._p(be), so._p(cnt),
                          ctypes.c_double(q.unif_ll), ctypes.c_int(m.K), so._p(al), so._p(bt), so._p(w), so._p(lab, so._I64))
    return lab


# ---------------------------------------------------------------------------------------------------------------------
# the searches that filled the tables
def find_seed(q, M, K, perturb, seeds=range(400), want=None, a_hi=None):
    """The first seed whose random model has no NEAR bin, is bitten by every perturbation (alone and padded) and meets `want`."""
    for seed in seeds:
        case = Case("search", "", [q], [random_model(q, K, seed, 0, perturb, a_hi=a_hi)], ((0,),))
        pr, _ws, refs, _st = check_case(case, [M])
        if not pr and (want is None or want(refs[0])):
            return seed
    raise LookupError(f"no seed for N={q.N} K={K} {perturb}")


def find_rows(M, n, lo=-40.0, count=2, finite=True):
    """Rows (a, b), a > 0 and b > 0, spread over the grid, with M[a, b, n] > lo (finite) or the sentinel there (not finite)."""
    T, B, _N = M.shape
    ok = (M[:, :, n] > lo) if finite else (M[:, :, n] == ml.SENT)
    ok[0, :] = ok[:, 0] = False
    rows = np.argwhere(ok)
    assert len(rows) >= count, (n, len(rows))
    pick = rows[np.linspace(0, len(rows) - 1, count + 2).astype(int)[1:-1]]
    return tuple((int(a), int(b)) for a, b in pick)


def lab_utr(N, cnt_max=60):
    return make_utr(f"lab{N}" if cnt_max == 60 else f"lab{N}c{cnt_max}", N, 100 + N, betas_for(13), cnt_max=cnt_max)


def _with_counts(q, bins, value):
    q.cnt = q.cnt.copy()
    q.cnt[list(bins)] = value
    return q


def _bins_perturb(N):
    """(One bin cannot show both a changed component row and a changed uniform column: N = 1 leaves the second out.)"""
    return (("drop_b", "drop_last_bin", "sentinel_as_zero") + (("uniform_as_component",) if N > 1 else ()) + (("pitch_N",) if N % PITCH else ())
            + (("first_block_only",) if N > BLOCK else ()))


def cases():
    cs = []
    # ---- bins: the stride loop on both sides of one and two trips, one wavefront and a partial last one, Np != N
    preps = [lab_utr(N) for N in N_BINS]
    models = [random_model(q, 3, BIN_SEEDS[q.N], u, _bins_perturb(q.N), f"N={q.N}") for u, q in enumerate(preps)]
    cs.append(Case("bins", "N = 1 .. 513 around the 16-bin pitch, the 64 lanes and the 256 threads of one trip; alone and all in one call",
                   preps, models, tuple((u,) for u in range(len(preps))) + (tuple(range(len(preps))),)))
    # ---- classes: K + 1 on both sides of every entry of LabelClasses, alone and padded
    q = lab_utr(65)
    models = [random_model(q, K, CLASS_SEEDS[K], 0, ("drop_b", "uniform_as_component") if K else (), f"K={K}", CLASS_A_HI) for K in K_CLASSES]
    cs.append(Case("classes", "K = 0 .. 63 with K + 1 on both sides of 8, 16, 32, 64; each at its own pitch and at pitch 63 with junk beyond K",
                   [q], models, tuple((i,) for i in range(len(models)))))
    # ---- planted: gaps of TIGHT bounds, both signs
    preps = [_with_counts(lab_utr(PLANT_N), PLANT_BINS, c) for c in PLANT_COUNTS]
    models = [planted_model(preps[u], K, c0, c1, n, sign, u) for u in range(len(preps)) for (K, c0, c1) in PLANT_PAIRS
              for n in PLANT_BINS for sign in (1, -1)]
    cs.append(Case("planted", "the two best columns TIGHT bounds apart, both signs, at the class edges, bins 0, 255, 256 = N - 1, cnt 1 and 60",
                   preps, models, tuple((i,) for i in range(len(models)))))
    # ---- ties, sentinel rows, zero and tiny weights
    q = lab_utr(PLANT_N)
    models = []
    for K, c0, c1 in TIE_PAIRS:
        m = random_model(q, K, 8000 + K, 0, ("last_max",), f"tie ({c0}, {c1}) of K={K}")
        m.ws = m.ws * 0.2 / m.ws.sum()
        for c in (c0, c1):
            m.a_idx[c], m.b_idx[c], m.ws[c] = TIE_ROW[0], TIE_ROW[1], 0.4
        models.append(m)
    one = np.int32
    models.append(Model(0, 3, np.full(3, TIE_ROW[0], one), np.full(3, TIE_ROW[1], one), np.array([0.3, 0.3, 0.3, 0.1]), ("last_max",), None, "three-way tie"))
    (a0, b0), (a1, b1) = DEAD_ROWS
    models.append(Model(0, 2, np.array([a0, a1], one), np.array([b0, b1], one), np.array([0.3, 0.7, 0.0]),
                        ("sentinel_as_zero", "zero_weight_as_one", "last_max"), None, "every column sentinel-class at bin 0"))
    (a0, b0), (a1, b1) = ZERO_ROWS
    models.append(Model(0, 2, np.array([a0, a1], one), np.array([b0, b1], one), np.array([0.0, 0.05, 0.15]), ("zero_weight_as_one",), None,
                        "weight exactly 0 on the column that would win"))
    (a0, b0), (a1, b1) = TINY_ROWS
    models.append(Model(0, 2, np.array([a0, a1], one), np.array([b0, b1], one), np.array([1e-300, 0.5, 0.0]), ("zero_weight_as_one",), None,
                        "weight 1e-300"))
    cs.append(Case("ties", "exact ties at the class edges and three-way; all columns sentinel-class; weights 0 and 1e-300",
                   [q], models, tuple((i,) for i in range(len(models)))))
    # ---- counts
    q = _with_counts(lab_utr(PLANT_N, COUNT_MAX), (COUNT_BIN,), COUNT_MAX)
    models = [planted_model(q, K, c0, c1, COUNT_BIN, sign) for (K, c0, c1) in ((8, 6, 7), (7, 6, 7)) for sign in (1, -1)]
    models.append(random_model(q, 3, COUNT_SEED, 0, ("drop_b",), "losers underflow"))
    cs.append(Case("counts", "cnt up to 1000: a planted bin at cnt = 1000; bins where every losing column falls below the exp clamp",
                   [q], models, tuple((i,) for i in range(len(models)))))
    # ---- calls: selections, orders and repeats on one handle
    preps = [lab_utr(N) for N in CALL_N]
    pitch = ("k_pitch_plus1", "w_pitch_k")
    models = [random_model(preps[u], K, CALL_SEEDS[s][u], u, pitch if (s, u) in ((0, 2), (0, 3), (1, 0), (1, 2), (1, 3)) else (),
                           f"set {'AB'[s]} UTR {u} K={K}") for s in (0, 1) for u, K in enumerate(CALL_K[s])]
    calls = ((0,), (7, 4), (0, 2, 3), (4, 5, 6, 7), (4, 6, 7), (4,), (0, 1, 2, 3), (3, 0))
    cs.append(Case("calls", "sel_utr = [0], [3, 0], [0, 2, 3], all four; models of different K per call; the same selections again "
                   "with the other model set", preps, models, calls))
    return cs
