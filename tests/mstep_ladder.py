"""The ladder of tests/test_mstep_ladder.py and tests/test_mstep_reference.py: tiny UTRs and job tables that put the
bin count, the support of v, the finite extent of a tile, the window rows, the columns of a tile and the shape of the
call on both sides of every boundary of the M-step kernels (k2_mstep, k3_mstep, k4_mstep: mstep_staged.inc,
mstep_ring.inc, mstep_multi.inc on the frame of mstep.inc) and of the E-step code that feeds them (em_lockstep.inc,
k2_estep: rd_lo / rd_hi / rd_n0 / rd_n1, the suffix sums, the reduction across tiles).
tests/test_host.py reads the boundaries from the sources and checks the ladder against them.

UtrPrep objects are built directly (not through prepare_utr), so that N is exactly what a case says; the theta grid is
prepare_utr's (int(min l) .. L in steps of 9, L >= 2000: T is about 219, 28 to 55 tiles of 64 rows, the last one
partial).  Inputs are drawn from seeded families; every seed and every hand-placed alpha in the tables below was
searched for on the CPU (against the C oracle's tensor) so that the case meets the conditions which
tests/test_mstep_reference.py checks again on every run and tests/test_mstep_ladder.py once more on the device's own
tensor:
  1. every round of every ladder job is DECIDED (oracle/mstep_reference.py), or an exact tie by design;
  2. every perturbation a case lists - the wrong M-step its boundary is about - gives a different row, decided too.
"""
from dataclasses import dataclass

import numpy as np

S_DIS = np.arange(20, 150, 10) + 0.0
PMF_S = np.repeat(1 / len(S_DIS), len(S_DIS))
P0 = dict(mu_f=300, sigma_f=50, max_unif_ws=0.15)
THETA_STEP = 9
ROWS = 64                                         # MT_ROWS: pinned to the source by tests/test_host.py
HALF = 16                                         # M3_CH


def betas_for(B):
    """The model's beta grid np.arange(5, max_beta, 5): max_beta = 45 / 70 / 85 give B = 8 / 13 / 16."""
    max_beta = {8: 45, 13: 70, 16: 85}[B]
    out = np.arange(5, max_beta, 5) + 0.0
    assert len(out) == B
    return out


def make_utr(name, N, seed, betas, xlo=60, xhi=1300, L=2000, cnt_max=60, lmin=40, lmax=140, p=P0, spaced=None):
    """One UTR of N r-unknown bins, ascending in x: x, l and the read counts drawn from RandomState(seed).
    spaced: x = xlo + spaced * n instead of a random draw."""
    from scape_amd.host import UtrPrep
    rs = np.random.RandomState(seed)
    x = np.sort(rs.choice(np.arange(xlo, xhi), size=N, replace=False)).astype(np.float64)
    if spaced is not None:
        x = xlo + float(spaced) * np.arange(N)
    l = rs.randint(lmin, lmax, size=N).astype(np.float64)
    cnt = rs.randint(1, cnt_max + 1, size=N).astype(np.int64)
    min_theta = float(int(l.min()))
    theta = np.arange(int(min_theta), int(L), THETA_STEP) + 0.0
    return UtrPrep(gene_info_str=f"mstep:{name}:1:1-{L}:+", p=dict(p), x=x, l=l, r=np.full(N, np.nan), pa=np.full(N, np.nan),
                   cnt=cnt, idx=np.arange(N, dtype=np.int64), cb_id=np.arange(N), read_id=np.arange(N), L=int(L),
                   min_theta=min_theta, theta=theta, betas=np.asarray(betas, dtype=np.float64), s_dis=S_DIS.copy(),
                   pmf_s=PMF_S.copy(), unif_ll=float(np.log((1 / L) * (1 / L) * (1 / 150))))


_TENSOR = {}


def oracle_tensor(q):
    """The C oracle's marginal tensor [T, B, N] of a UTR (cached by name)."""
    from oracle import scape_oracle as so
    if q.gene_info_str not in _TENSOR:
        A = so.phase_a(q.x, q.l, q.r, q.pa, q.theta, q.s_dis, q.pmf_s, q.p["mu_f"], q.p["sigma_f"])
        _TENSOR[q.gene_info_str] = so.get_loglik_marginal_tensor(q.theta, q.betas, A)
    return _TENSOR[q.gene_info_str]


SENT = float(np.finfo("f").min)


_EXTENT = {}


def tile_extents(M):
    """tile_nend restated (k_tile_extent): per 64-row tile the bin count, rounded up to 16, beyond which every row
    holds the sentinel."""
    key = (id(M), M.shape)
    if key not in _EXTENT:
        _EXTENT[key] = (M, _tile_extents(M))            # (the tensor is kept, so that its id stays its own)
    return _EXTENT[key][1]


def _tile_extents(M):
    T, B, N = M.shape
    fin = (M.reshape(T * B, N) != SENT)
    Np = (N + 15) // 16 * 16
    out = []
    for r0 in range(0, T * B, ROWS):
        cols = np.nonzero(fin[r0:r0 + ROWS].any(axis=0))[0]
        out.append(min(Np, (int(cols[-1]) + 1 + 15) // 16 * 16) if len(cols) else 0)
    return np.array(out)


@dataclass
class Job:
    u: int
    K: int
    a_idx: np.ndarray
    b_idx: np.ndarray
    ws: np.ndarray
    k_arr: np.ndarray                  # the component order, as long as the case's nround
    perturb: tuple = ()                # ((name, value), ...): wrong M-steps that must change this job's answer (round 0)
    tie: bool = False                  # the winner has exact ties by design (the first of them is the answer)
    note: str = ""


def random_ws(K, rs, cap=P0["max_unif_ws"]):
    ws = rs.uniform(size=K + 1)
    ws = ws / ws.sum()
    if ws[-1] > cap:
        ws[:-1] = ws[:-1] * (1 - cap)
        ws[-1] = cap
    return ws


def random_job(q, K, rs, u=0, nround=1, k=None, a_range=None):
    """A job from a random init: K distinct alphas on the grid (ascending), random betas and weights, a random
    component first."""
    lo, hi = a_range if a_range is not None else (0, q.T)
    a = np.sort(rs.choice(np.arange(lo, hi), size=K, replace=False)).astype(np.int32)
    b = rs.randint(0, len(q.betas), size=K).astype(np.int32)
    order = np.array([(i + (rs.randint(K) if k is None else k)) % K for i in range(nround)], np.int8)
    return Job(u, K, a, b, random_ws(K, rs), order)


def run_reference(q, M, job, nround, **perturb):
    from oracle import mstep_reference as mr
    return mr.em_rounds(M, q.cnt, q.unif_ll, q.theta, q.betas, float(q.L), q.min_theta, q.p["max_unif_ws"], job.a_idx, job.b_idx,
                        job.ws, job.k_arr, nround, **perturb)


def run_oracle(q, M, job, nround, fixed=False):
    """so_em_algo from the job's init: dict(a, b: grid indices, ws, bic, lb).  fixed: no M-step (mstep_fixed)."""
    import ctypes
    from oracle import scape_oracle as so
    a, b = q.theta[job.a_idx].copy(), q.betas[job.b_idx].copy()
    w = np.asarray(job.ws, dtype=np.float64).copy()
    ka = np.ascontiguousarray(job.k_arr[:nround], dtype=np.int64)
    bic, lb = ctypes.c_double(0), np.zeros(nround)
    th, be, cnt = (np.ascontiguousarray(v, dtype=np.float64) for v in (q.theta, q.betas, q.cnt))
    Mc = np.ascontiguousarray(M)
    n = so.lib().so_em_algo(so._p(Mc), ctypes.c_int(q.T), ctypes.c_int(len(be)), ctypes.c_int(q.N), so._p(th), so._p(be), so._p(cnt),
                            ctypes.c_double(q.unif_ll), ctypes.c_double(q.L), ctypes.c_double(q.min_theta),
                            ctypes.c_double(q.p["max_unif_ws"]), ctypes.c_int(job.K), so._p(a), so._p(b), so._p(w),
                            so._p(ka, so._I64), ctypes.c_int(nround), ctypes.c_int(int(fixed)), ctypes.byref(bic), so._p(lb))
    return dict(a=np.searchsorted(q.theta, a), b=np.searchsorted(q.betas, b), ws=w, bic=bic.value, lb=lb[:n].copy())


# ---------------------------------------------------------------------------------------------------------------------
# what a job's first M-step looks like to the kernels
def facts(q, M, job, rnd):
    """The quantities of round 0 that the kernels branch on, restated from the job and the reference's round."""
    B, T, k, K = len(q.betas), q.T, int(job.k_arr[0]), job.K
    rd_lo = 0 if k == 0 else int(job.a_idx[k - 1]) * B
    rd_hi = (T if k == K - 1 else int(job.a_idx[k + 1]) + 1) * B
    ext = tile_extents(M)
    wt = rnd.row // ROWS
    v = rnd.v.astype(np.float64)
    n_lo = rnd.n0 & ~(HALF - 1)
    n_hi = min((rnd.n1 + HALF - 1) // HALF * HALF, int(ext[wt]))
    return dict(rd_lo=rd_lo, rd_hi=rd_hi, lo_mod=rd_lo % ROWS, hi_mod=rd_hi % ROWS, n_tiles=(rd_hi - 1) // ROWS - rd_lo // ROWS + 1,
                first_tile=rd_lo // ROWS, last_tile=(rd_hi - 1) // ROWS, win_tile=wt, win_ext=int(ext[wt]), n0=rnd.n0, n1=rnd.n1,
                rescue=rnd.rescue, tail=bool(v[int(ext[wt]):].sum() != 0), halves=max(0, n_hi - n_lo) // HALF,
                lo_clipped=rnd.row // B == rd_lo // B, hi_clipped=rnd.row // B == rd_hi // B - 1, n_ties=len(rnd.ties),
                tie_tiles=sorted({int(r) // ROWS for r in rnd.ties}), tie_exts=sorted({int(ext[int(r) // ROWS]) for r in rnd.ties}),
                last_partial=(T * B) % ROWS != 0 and wt == (T * B - 1) // ROWS, group16=(rd_lo // 16 == (rd_hi - 1) // 16))


def check_job(q, M, job, nround=1):
    """Conditions 1 and 2 for one job: (problems, smallest decision ratio, the unperturbed Fit)."""
    fit = run_reference(q, M, job, nround)
    problems, worst = [], np.inf
    if fit.near:
        problems.append(("a comparison within rounding of its threshold", fit.near))
    for i, r in enumerate(fit.rounds):
        worst = min(worst, r.ratio)
        if not r.decided:
            problems.append((f"round {i} undecided", r.ratio))
        if i == 0 and job.tie != (len(r.ties) > 1):
            problems.append(("exact ties", len(r.ties), "by design" if job.tie else "not by design"))
    for name, val in job.perturb:
        p = run_reference(q, M, job, 1, **{name: val}).rounds[0]
        if p.row == fit.rounds[0].row:
            problems.append((f"{name}={val} leaves the answer at row {p.row}",))
        elif p.row >= 0 and not p.decided:
            problems.append((f"{name}={val} undecided", p.ratio))
        if p.row >= 0:
            worst = min(worst, p.ratio)
    return problems, worst, fit


@dataclass
class Case:
    name: str
    boundary: str
    preps: list
    jobs: list
    nround: int = 1
    calls: tuple = ()                  # job counts of the EM calls (prefixes of `jobs`); () = one call with all jobs
    random: bool = False               # the random family: undecided jobs are counted and may be left out (1 in 20)
    cols_keep: int = None              # the perturbation cols_keep=m (a dropped pass or column group leaves the jobs from m on at
                                       # their init): every job from this index on must move away from its init


def job_from_seed(q, seed, u=0, kind="rand", K=None, k=None, a_lo=None, a_hi=None, nround=1, perturb=(), tie=False, note=""):
    """The seeded job families.  rand: K (1 + seed % 3 unless given) random alphas; window: K = 3, component 1 between
    alphas a_lo and a_hi; first: K = 2, component 0 below a_hi; last: K = 2, component 1 above a_lo."""
    rs = np.random.RandomState(seed)
    nb = len(q.betas)
    if kind == "rand":
        j = random_job(q, K if K is not None else 1 + seed % 3, rs, u, nround, k)
    else:
        if kind == "window":
            a = np.array([a_lo, rs.randint(a_lo, a_hi + 1), a_hi], np.int32)
            kk = 1
        elif kind == "first":
            a = np.array([rs.randint(0, a_hi + 1), a_hi], np.int32)
            kk = 0
        else:
            a = np.array([a_lo, rs.randint(a_lo, q.T)], np.int32)
            kk = 1
        j = Job(u, len(a), a, rs.randint(0, nb, size=len(a)).astype(np.int32), random_ws(len(a), rs), np.full(nround, kk, np.int8))
    j.perturb, j.tie, j.note = tuple(perturb), tie, note
    return j


def search(q, M, want, make, seeds=range(4000), nround=1):
    """The first seed whose job meets conditions 1 and 2 and whose facts contain `want` (values, or predicates)."""
    for seed in seeds:
        job = make(seed)
        problems, _ratio, fit = check_job(q, M, job, nround)
        if problems:
            continue
        f = facts(q, M, job, fit.rounds[0])
        if all(v(f[key]) if callable(v) else f[key] == v for key, v in want.items()):
            return seed
    raise LookupError(f"no seed gives {want}")


# ---------------------------------------------------------------------------------------------------------------------
# the tables (found with search() / by enumeration against the C oracle's tensor; checked again by every test run)
N_LADDER = (1, 15, 16, 17, 31, 32, 33)
# (N, bin) -> seed of a rand-family job whose answer changes when that bin is dropped from v
BIN_SEEDS = {(1, 0): 0, (15, 0): 22, (15, 14): 0, (16, 0): 26, (16, 14): 6, (16, 15): 0, (17, 0): 5, (17, 14): 6, (17, 15): 12,
             (17, 16): 0, (31, 0): 26, (31, 14): 4, (31, 15): 12, (31, 16): 12, (31, 17): 12, (31, 30): 6, (32, 0): 7, (32, 14): 11,
             (32, 15): 4, (32, 16): 24, (32, 17): 4, (32, 30): 28, (32, 31): 0, (33, 0): 26, (33, 14): 4, (33, 15): 11, (33, 16): 4,
             (33, 17): 24, (33, 30): 12, (33, 31): 12, (33, 32): 6}
N_UTR_CALLS = (1, 7, 8, 9)                        # active UTRs of the calls of the "bins" case
# support of v on the spaced UTR (sigma_f = 10: the 1e-300 cut and l <= theta - x bound the finite bins of a row on both
# sides): what is pinned -> (alpha index, beta index, bin whose loss changes the answer or None)
SUPPORT = {("n0", 0): (73, 11, 15), ("n0", 15): (130, 0, None), ("n0", 16): (156, 9, 31), ("n0", 17): (163, 4, 31),
           ("n1", 16): (61, 12, 12), ("n1", 17): (66, 12, None), ("n1", 32): (141, 12, 22), ("n1", 33): (146, 12, 32),
           ("n1", 40): (192, 12, 39)}
SUPPORT_FILL = 24                                 # further K = 1 jobs on the same tiles: 33 columns, three column groups
# window ends, B = 13: (end, rd mod 64) -> (alpha_{k-1}, alpha_{k+1}, seed); the winner is clipped at that end
WINDOW_ENDS = {("hi", 0): (107, 127, 0), ("lo", 0): (64, 84, 0), ("hi", 1): (112, 132, 13), ("lo", 1): (69, 89, 0),
               ("hi", 15): (118, 138, 13), ("lo", 15): (75, 95, 0), ("hi", 16): (123, 143, 13), ("lo", 16): (80, 100, 0),
               ("hi", 17): (128, 148, 13), ("lo", 17): (85, 105, 0), ("hi", 63): (166, 186, 13), ("lo", 63): (123, 143, 0)}
WINDOW_TILES = {1: (138, 140, 1), 2: (133, 140, 0), 3: (128, 140, 0)}      # tiles spanned -> (alpha_{k-1}, alpha_{k+1}, seed)
WINDOW_B = {"one16": (144, 0), "two16": (131, 0)}                          # a window of exactly B rows -> (alpha, seed)
WINDOW_LAST = (150, 5)                            # k = K - 1 on the UTR whose reads end at L: (alpha_{k-1}, seed)
WINDOW_FIRST = (120, 3)                           # k = 0, clipped at alpha_1: (alpha_1, seed)
EXTENT = {"tail": 0, "inside": 2, "win_tail": 46}                          # seeds on E33 (win_tail: K = 2 + seed % 2)
COLUMN_CALLS = (1, 15, 16, 17, 32, 33, 48, 49, 64, 65, 128, 129)
MANY_CALLS = (341, 342, 512, 513, 1024)
ROUNDS3_SEED, ROUNDS2_SEED = 0, 0
TIE_AHI = {"one tile": 5, "two tiles of extent 0": 12, "three tiles": 20, "tiles of extent 0 and 16": 80}
RING_HALVES = (1, 2, 3, 4, 5, 6)                  # streamed half-chunks: 1, 2 and depth - 1, depth, depth + 1 of every ring (test_host.py)
RING_CALLS = (96, 192, 288, 384)                  # 16, 32, 48, 64 columns on the tile: G = 1 .. 4 column groups where passes are not split
RING_TILE = 20                                    # alphas 160 .. 167 (B = 8): right of every read end, the extent is Np
RANDOM_N = (40, 47, 52, 58, 64, 65, 73, 81)
RANDOM_JOBS = 30


def dead_job(q, a_hi, seed, u=0):
    """K = 2, component 0 first, both alphas left of every read end: column 0 is all sentinel, the rescue fires, every
    row of the window [theta_0, alpha_1] is all sentinel on the support of v - an exact tie, the first row wins."""
    rs = np.random.RandomState(seed)
    return Job(u, 2, np.array([0, a_hi], np.int32), rs.randint(0, len(q.betas), size=2).astype(np.int32), random_ws(2, rs),
               np.zeros(1, np.int8), perturb=(("last_max", True),), tie=True)


def cases():
    B8, B13, B16 = betas_for(8), betas_for(13), betas_for(16)
    cs = []
    # ---- bins: N on both sides of 16 and 32; 1, 7, 8, 9 active UTRs; unequal T (utr_length 2600)
    preps = [make_utr(f"N{N}", N, 100 + N, B8) for N in N_LADDER]
    preps += [make_utr("N20L", 20, 120, B8, L=2600, xhi=1900), make_utr("N9", 9, 109, B8)]
    jobs = []
    for u, N in enumerate(N_LADDER):
        for (n_, nb), seed in BIN_SEEDS.items():
            if n_ == N:
                jobs.append(job_from_seed(preps[u], seed, u, perturb=(("drop_bin", nb),), note=f"N={N}: bin {nb}"))
    jobs += [job_from_seed(preps[u], seed, u) for u in (7, 8) for seed in (0, 1, 2)]
    ends = [max(i for i, j in enumerate(jobs) if j.u < n) + 1 for n in N_UTR_CALLS]
    cs.append(Case("bins", "N = 1 .. 33 around the 16-bin half-chunk and the 32-bin chunk; 1, 7, 8, 9 active UTRs; unequal T",
                   preps, jobs, calls=tuple(ends)))
    # ---- support of v
    q = make_utr("S40", 40, 7, B13, cnt_max=3, xlo=60, lmin=50, lmax=51, p=dict(P0, sigma_f=10), spaced=45)
    jobs = []
    for (key, want), (a, b, nb) in SUPPORT.items():
        jobs.append(Job(0, 1, np.array([a], np.int32), np.array([b], np.int32), np.array([0.85, 0.15]), np.zeros(1, np.int8),
                        perturb=(("drop_bin", nb),) if nb is not None else (), note=f"{key}={want}"))
    jobs += [job_from_seed(q, seed, 0, K=1) for seed in range(SUPPORT_FILL)]
    cs.append(Case("support", "rd_n0 at 0, 15, 16, 17 and rd_n1 at 16, 17, 32, 33, N; supports that end in different half-chunks, disjoint ones",
                   [q], jobs))
    # ---- finite extent
    q = make_utr("E33", 33, 133, B8)
    jobs = [job_from_seed(q, EXTENT["tail"], 0, perturb=(("sentinel_as_zero", True),), note="tail"),
            job_from_seed(q, EXTENT["inside"], 0, note="inside"),
            job_from_seed(q, EXTENT["win_tail"], 0, K=2 + EXTENT["win_tail"] % 2, perturb=(("sentinel_as_zero", True),), note="win_tail")]
    cs.append(Case("extent", "tiles of extent 16, 32 and Np under one window; v with mass beyond the extent and all inside it", [q], jobs))
    # ---- window rows (B = 13: rd_lo and rd_hi take every residue mod 64)
    qr = make_utr("Wright", 24, 31, B13, xlo=1000, xhi=1750, cnt_max=30)
    ql = make_utr("Wleft", 24, 32, B13, xlo=60, xhi=420, cnt_max=30)
    qe = make_utr("Wend", 12, 33, B13, xlo=1500, xhi=1900, lmin=60, lmax=99, cnt_max=30)
    jobs = []
    for (end, r), (a_lo, a_hi, seed) in WINDOW_ENDS.items():
        if end == "hi":
            pert = (("hi_exclusive", True), ("rows_to", ((a_hi + 1) * 13 - 1) // ROWS * ROWS))
            jobs.append(job_from_seed(qr, seed, 0, "window", a_lo=a_lo, a_hi=a_hi, perturb=pert, note=f"hi_mod={r}"))
        else:
            jobs.append(job_from_seed(ql, seed, 1, "window", a_lo=a_lo, a_hi=a_hi, perturb=(("lo_exclusive", True),), note=f"lo_mod={r}"))
    for n, (a_lo, a_hi, seed) in WINDOW_TILES.items():
        jobs.append(job_from_seed(qr, seed, 0, "window", a_lo=a_lo, a_hi=a_hi, perturb=(("hi_exclusive", True),), note=f"n_tiles={n}"))
    for name, (a, seed) in WINDOW_B.items():
        jobs.append(job_from_seed(qr, seed, 0, "window", a_lo=a, a_hi=a, note=name))
    last0 = (qe.T * 13 - 1) // ROWS * ROWS
    jobs.append(job_from_seed(qe, WINDOW_LAST[1], 2, "last", a_lo=WINDOW_LAST[0], perturb=(("rows_to", last0),), note="last_partial"))
    jobs.append(job_from_seed(qr, WINDOW_FIRST[1], 0, "first", a_hi=WINDOW_FIRST[0], perturb=(("hi_exclusive", True),), note="first"))
    cs.append(Case("window", "rd_lo, rd_hi mod 64 in {0, 1, 15, 16, 17, 63} with the winner clipped at that end; windows of B rows, of 1, 2, 3 "
                   "tiles, into the partial last tile; k = 0 and k = K - 1", [qr, ql, qe], jobs))
    # ---- columns per tile
    q = make_utr("C17", 17, 217, B8)
    cs.append(Case("columns", "1 .. 129 live columns on every tile (K = 1: the window is the whole grid)", [q],
                   [job_from_seed(q, seed, 0, K=1) for seed in range(max(COLUMN_CALLS))], calls=COLUMN_CALLS, cols_keep=0))
    q = make_utr("J13", 13, 313, B8)
    cs.append(Case("many", "341 .. 1,024 non-fixed jobs on one UTR: em_depth's 1,024-entry rule, SCAPE_MAX_JOBS_PER_UTR", [q],
                   [job_from_seed(q, seed, 0, K=1) for seed in range(max(MANY_CALLS))], calls=MANY_CALLS, cols_keep=0))
    # ---- ring depths: h half-chunks streamed (v is nowhere 0: counts of 1 or 2 reads never underflow) for G column groups
    preps = [make_utr(f"H{h}", 16 * h - 2, 800 + h, B8, xlo=600, xhi=1100, cnt_max=2) for h in RING_HALVES]
    a0 = RING_TILE * ROWS // 8
    jobs = [job_from_seed(preps[u], 100 * u + 16 * g + i, u, "window", a_lo=a0 + (i % 3), a_hi=a0 + 7 - (i % 2), note=f"halves={h}")
            for g in range(4) for u, h in enumerate(RING_HALVES) for i in range(16)]
    cs.append(Case("ring", "1 .. 6 half-chunks streamed by 1 .. 4 column groups: below, at and above the depth of every LDS-DMA ring",
                   preps, jobs, calls=RING_CALLS, cols_keep=0))
    # ---- rounds
    q = make_utr("R33", 33, 433, B8)
    j = random_job(q, 5, np.random.RandomState(ROUNDS3_SEED), nround=3)
    j.k_arr = np.array([0, 2, 4], np.int8)
    cs.append(Case("rounds3", "nround = 3, K = 5, order 0, 2, 4: three columns of one job in one launch at depth 3", [q], [j], nround=3))
    cs.append(Case("rounds2", "nround = 2, K = 1: the arg-max feeds the next round's column refresh", [q],
                   [job_from_seed(q, ROUNDS2_SEED, 0, K=1, nround=2)], nround=2))
    # ---- ties
    q = make_utr("T17", 17, 517, B8, xlo=700, xhi=1500)
    cs.append(Case("ties", "dead components: all-sentinel windows in one tile, over tiles of equal extent, over tiles of extent 0 and 16",
                   [q], [dataclass_replace(dead_job(q, a_hi, 1), note=name) for name, a_hi in TIE_AHI.items()]))
    # ---- B = 16 (T * B = 3,504 rows: 55 tiles) and the random family
    q = make_utr("B16", 21, 716, B16)
    cs.append(Case("beta16", "B = 16: 55 tiles, rows of a tile are four whole alphas", [q], [job_from_seed(q, seed, 0) for seed in range(12)]))
    preps = [make_utr(f"R{N}", N, 600 + u, B13, xhi=1700) for u, N in enumerate(RANDOM_N)]
    jobs = [job_from_seed(preps[u], 1000 * u + i, u, K=1 + i % 8) for u in range(len(preps)) for i in range(RANDOM_JOBS)]
    cs.append(Case("random", "8 UTRs of 40 to 81 bins, 30 jobs each, K = 1 .. 8, random component", preps, jobs, random=True))
    return cs


def dataclass_replace(obj, **kw):
    import dataclasses
    return dataclasses.replace(obj, **kw)


# ---------------------------------------------------------------------------------------------------------------------
# the host's kernel selection restated (scape_hip.hip: em_switches, em_wide, em_depth, em_choose, em_rounds) - no API
# reports which M-step kernel a call ran.  tests/test_host.py pins these constants to the source.
EM_DEPTH = 3
WIDE_MAX_COLUMNS = 16
WIDE_MAXJOBS_DEFAULT = 1024
SPLIT_MAXTILES_DEFAULT = 1024
LIST_ENTRIES = 1024                               # list entries per UTR of k2_mstep / k3_mstep
MAX_JOBS_PER_UTR = 1024
MT_MAXJ = 64
XCD_UTRS = 8                                      # n_utr >= 8: a UTR's tiles go to one XCD


def selection(env, jobs, preps):
    """dict(wide, depth, kernel, job_split, jobs_per_pass, grid_y) of an EM call with the environment `env`."""
    n_jobs, kmax = len(jobs), max(j.K for j in jobs)
    wide_max = int(env.get("SCAPE_HIP_WIDE_MAXJOBS", WIDE_MAXJOBS_DEFAULT))
    split_max = int(env.get("SCAPE_HIP_SPLIT_MAXTILES", SPLIT_MAXTILES_DEFAULT))
    depth = min(EM_DEPTH, max(1, int(env.get("SCAPE_HIP_EM_DEPTH", EM_DEPTH))))
    wide = n_jobs <= wide_max and kmax + 1 <= WIDE_MAX_COLUMNS
    per_utr = {}
    for j in jobs:
        per_utr[j.u] = per_utr.get(j.u, 0) + 1
    if wide:
        depth = 1
    while depth > 1 and max(per_utr.values()) * depth > LIST_ENTRIES:
        depth -= 1
    B = len(preps[0].betas)
    tiles_max = max((preps[u].T * B + ROWS - 1) // ROWS for u in per_utr)
    job_split = len(per_utr) * tiles_max <= split_max
    mode = env.get("SCAPE_HIP_MSTEP")
    kernel = "k2_mstep" if mode == "v2" else ("k3_mstep" if job_split or mode == "v3" else "k4_mstep")
    return dict(wide=wide, depth=depth, kernel=kernel, job_split=job_split, jobs_per_pass=16 if job_split else MT_MAXJ,
                grid_y=min(64, (max(per_utr.values()) * depth + 15) // 16) if job_split else 1, n_active=len(per_utr))


NARROW = {"SCAPE_HIP_WIDE_MAXJOBS": "0"}
FORMS = tuple((f"{name}, depth {d}", dict(NARROW, SCAPE_HIP_EM_DEPTH=str(d), **env)) for name, env in (
    ("k2_mstep, passes split", {"SCAPE_HIP_MSTEP": "v2"}),
    ("k2_mstep, passes whole", {"SCAPE_HIP_MSTEP": "v2", "SCAPE_HIP_SPLIT_MAXTILES": "0"}),
    ("k3_mstep, passes split", {}),
    ("k3_mstep, passes whole", {"SCAPE_HIP_MSTEP": "v3", "SCAPE_HIP_SPLIT_MAXTILES": "0"}),
    ("k4_mstep", {"SCAPE_HIP_SPLIT_MAXTILES": "0"})) for d in (1, 3)) + (("4-wavefront E-step", {}),)
