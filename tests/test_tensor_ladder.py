"""The tensor build on the GPU at its boundary shapes, against the long-double reference and its per-entry bound.

Every batch of the ladder (tests/tensor_ladder.py; tests/test_host.py checks it against the constants of the sources) is
built by k_phase_a and by each form of Phase B - k_phase_b (SCAPE_HIP_PHASE_B=v2), k_pb_tables + k_phase_b_lin (split)
and the default, k_pb_tables + k_pb_logcol + k_pb_slide where the batch is eligible.  The form a build took is asserted,
demotions included; the sentinel pattern must equal the reference's; every finite entry must lie within the bound that
oracle/tensor_reference.py derives for it (first order, from the roundings of the device's own sequence, times a fixed
margin of 2); forms must agree bit for bit.  The operator seam (three point operators, get_loglik_marginal_tensor:
every bin through k_phase_b's log-domain path) is held to the same bounds.  tests/test_tensor_reference.py validates
reference and bound on the CPU against the C oracle.

The last test takes UTRs with exactly N = 15 ... 257 bins through prepare_utr, Phase B's tile extents and the M-step's
sentinel tails: em_algo calls against the oracle's records, the same bits under every M-step kernel and Phase B form.

Measured on an MI355X (printed by every run as "[tensor ladder] worst observed / bound"; a measurement, not a target) -
worst observed error / bound over the ladder:
    Phase A (k_phase_a)           r-unknown bins 0.274, pA-site bins 0.270, r-known bins 0.154
    Phase B form 0, 1 and 2       linear-domain bins 0.272, log-domain bins 0.253 (the forms are bit-equal)
    get_loglik_marginal_tensor    0.226
    point operators               pa 0.252, r_known 0.119, r_unknown 0.196
(the C oracle, on the CPU: A 0.270, M 0.253).  The module takes about 4 s, the reference about 3 s of it.

What the bound can and cannot see.  The smallest bounds of the ladder are about 60 u (u = 2^-53): a dozen roundings
follow the exp, 1.66 |value| u comes with the log, the margin doubles both.  Arithmetic perturbations of scratch builds
(never committed): 1.0 / 24 -> 1.0 / 23 in d_exp_nonpos (up to 870 u on exp) and Lg5 with its fifth digit changed in
d_log_pos (up to 340 u absolute) fail every Phase A, Phase B and operator test, at up to 5.1 and 3.3 times the bound; a
lower window end made exclusive (`th[a] <= lob` together with `th[a - 1] > lob`) fails 27 tests.  1.0 / 120 -> 1.0 / 100
changes exp by at most r^5 / 600 = 2.2 u (|r| <= ln2 / 256) and Lg7's fifth digit changes log by at most s^15 1e-5 =
0.3 u absolute (s <= 0.1716): both lie below what ANY correct evaluation may deviate, no test against a rounding bound
can tell them from a correct kernel.  `th[a] < lob` -> `th[a] <= lob` alone changes nothing: the walk back
(`th[a - 1] >= lob`) undoes the extra step.
"""
import copy
import os

import numpy as np
import pandas as pd
import pytest

import tensor_ladder as tl

pytestmark = pytest.mark.gpu
SENT = float(np.finfo("f").min)
CASES = tl.cases()
BY_NAME = {c.name: c for c in CASES}
MODES = ("v2", "split", None)
FORM_NAME = {0: "Phase B form 0 (k_phase_b)", 1: "Phase B form 1 (k_pb_tables + k_phase_b_lin)",
             2: "Phase B form 2 (k_pb_tables + k_pb_logcol + k_pb_slide)"}
SEED = 20261019
RESEED = {}          # (N, K) -> seeds further; the rule of test_em_column_classes.RESEED.  None was needed.


class _Worst:
    def __init__(self):
        self.tab = {}

    def add(self, key, ratio):
        assert ratio == ratio, key                      # never a NaN: compare() reports those as inf
        self.tab[key] = max(self.tab.get(key, 0.0), ratio)

    def show(self):
        print("\n[tensor ladder] worst observed / bound (bound = first-order rounding count x 2):")
        for key in sorted(self.tab):
            print(f"  {key:<78s} {self.tab[key]:.3f}")


class _Builds:
    """The ladder's batches built on the GPU, each (case, Phase B mode) once per module."""

    def __init__(self, ctx):
        self.ctx, self.got, self.worst = ctx, {}, _Worst()

    def get(self, case, mode):
        from scape_amd.engine import HipBatch
        if (case.name, mode) not in self.got:
            old = os.environ.pop("SCAPE_HIP_PHASE_B", None)
            try:
                if mode is not None:
                    os.environ["SCAPE_HIP_PHASE_B"] = mode
                batch = HipBatch(self.ctx, case.preps)
                batch.build()
                form = batch.phase_b_form()
                A = [batch.fetch_loglik(u) for u in range(len(case.preps))]
                M = [batch.fetch_tensor(u) for u in range(len(case.preps))]
                batch.free()
            finally:
                os.environ.pop("SCAPE_HIP_PHASE_B", None)
                if old is not None:
                    os.environ["SCAPE_HIP_PHASE_B"] = old
            self.got[(case.name, mode)] = (form, A, M)
        return self.got[(case.name, mode)]


@pytest.fixture(scope="module")
def builds(hip_ctx):
    b = _Builds(hip_ctx)
    yield b
    b.worst.show()


def _check(problems, tag, got, ref, bound, sent):
    from oracle import tensor_reference as tr
    same, ratio, n_out = tr.compare(got, ref, bound, sent)
    if not same:
        problems.append(tag + ("sentinel pattern", int(((got == SENT) != sent).sum())))
    if n_out:
        problems.append(tag + ("beyond the bound", n_out, f"worst observed / bound {ratio:.2f}"))
    return ratio


def _report(problems):
    assert not problems, f"{len(problems)} mismatches\n" + "\n".join(repr(p) for p in problems[:40])


# ---------------------------------------------------------------- Phase A
@pytest.mark.parametrize("name", [c.name for c in CASES])
def test_phase_a_within_bound(builds, name):
    """k_phase_a on every ladder batch: sentinel pattern equal, every finite entry within its bound."""
    case, problems, worst = BY_NAME[name], [], 0.0
    _form, A, _M = builds.get(case, None)
    for u, (q, (a, _b)) in enumerate(zip(case.preps, tl.reference(case))):
        assert A[u].shape == (q.N, q.T)
        for kind, what in enumerate(("r-unknown bins", "pA-site bins", "r-known bins")):
            rows = a.kind == kind
            if rows.any():
                ratio = _check(problems, (name, u, "A", what), A[u][rows], a.A[rows], a.bound[rows], a.sent[rows])
                builds.worst.add(f"Phase A (k_phase_a), {what}", ratio)
                worst = max(worst, ratio)
    print(f"\n[{name}] Phase A worst observed / bound {worst:.3f}")
    _report(problems)


@pytest.mark.parametrize("name", [c.name for c in CASES if c.point_ops])
def test_point_operators_within_bound(builds, name):
    """The three operator entry points with one theta each, on all N bins of every UTR of the N ladder and of the
    value edges (pa == theta on the even bins, r on and around the s_dis grid)."""
    from oracle import tensor_reference as tr
    from scape import taichi_core as tc
    case, problems, worst = BY_NAME[name], [], {"pa": 0.0, "r_known": 0.0, "r_unknown": 0.0}
    for u, q in enumerate(case.preps):
        theta = float(q.theta[q.T // 2])
        mu_f, sigma_f, nan = q.p["mu_f"], q.p["sigma_f"], np.full(q.N, np.nan)
        k = np.arange(q.N)
        pa_all = np.where(k % 2 == 0, theta, q.x + q.l + 37)
        r_all = np.array(tl.R_VALUES)[k % 4]
        for kind, r, pa, call in (
                ("r_unknown", nan, nan, lambda: tc.loglik_xlr_t_r_unknown(q.x, q.l, nan, q.s_dis, q.pmf_s, theta, mu_f, sigma_f)),
                ("pa", nan, pa_all, lambda: tc.loglik_xlr_t_pa(q.x, q.l, pa_all, theta, sigma_f)),
                ("r_known", r_all, nan, lambda: tc.loglik_xlr_t_r_known(q.x, q.l, r_all, q.s_dis, q.pmf_s, theta, mu_f, sigma_f))):
            ref = tr.phase_a_ld(q.x, q.l, r, pa, [theta], q.s_dis, q.pmf_s, mu_f, sigma_f)
            assert ref.cmp_mismatch == 0 and ref.cut_distance > 1e-6
            got = np.asarray(call())
            assert got.shape == (q.N,)
            worst[kind] = max(worst[kind], _check(problems, (name, u, kind), got[:, None], ref.A, ref.bound, ref.sent))
    print(f"\n[{name}] point operators worst observed / bound " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    for k, v in worst.items():
        builds.worst.add(f"point operator loglik_xlr_t_{k}", v)
    _report(problems)


# ---------------------------------------------------------------- Phase B
@pytest.mark.parametrize("name", [c.name for c in CASES])
def test_phase_b_forms_within_bound_and_bit_equal(builds, name):
    """fetch_tensor under SCAPE_HIP_PHASE_B=v2, split and the default: the form the ladder says, the reference's
    sentinel pattern (hence count), every finite entry within its full-chain bound, all forms the same bits."""
    case, problems = BY_NAME[name], []
    ref = tl.reference(case)
    first = None
    for mode in MODES:
        form, _A, M = builds.get(case, mode)
        assert form == case.forms[mode], (name, mode, form, case.forms[mode])
        worst = 0.0
        for u, (q, (_a, b)) in enumerate(zip(case.preps, ref)):
            assert M[u].shape == (q.T, len(q.betas), q.N)
            assert int((M[u] == SENT).sum()) == int(b.sent.sum()), (name, mode, u)
            for lin, what in ((True, "linear-domain bins"), (False, "log-domain bins")):
                cols = (_a.kind == 0) == lin
                if cols.any():
                    ratio = _check(problems, (name, mode, u, "M", what), M[u][:, :, cols], b.M[:, :, cols], b.bound_dev[:, :, cols],
                                   b.sent[:, :, cols])
                    builds.worst.add(f"{FORM_NAME[form]}, {what}", ratio)
                    worst = max(worst, ratio)
        print(f"\n[{name}] mode {mode}: form {form}, worst observed / bound {worst:.3f}")
        if first is None:
            first = M
        else:
            for u, (x, y) in enumerate(zip(first, M)):
                if not np.array_equal(x, y):
                    problems.append((name, mode, u, "bits differ from the v2 build", int((x != y).sum())))
    _report(problems)


@pytest.mark.parametrize("name", [c.name for c in CASES if c.operator])
def test_marginal_tensor_operator_within_bound(builds, name):
    """get_loglik_marginal_tensor - every bin through the log-domain path of k_phase_b - on the N, T, n_beta and grid
    axes; its input is the reference's A rounded to f64, so the bound has no Phase A share."""
    from oracle import tensor_reference as tr
    from scape import taichi_core as tc
    case, problems, worst = BY_NAME[name], [], 0.0
    for u, (q, (a, _b)) in enumerate(zip(case.preps, tl.reference(case))):
        A64 = np.where(a.sent, SENT, a.A.astype(np.float64))
        ref = tr.phase_b_ld(q.theta, q.betas, A=A64)
        assert ref.cmp_mismatch == 0
        got = tc.get_loglik_marginal_tensor(q.theta, q.betas, A64)
        assert got.shape == (q.T, len(q.betas), q.N)
        worst = max(worst, _check(problems, (name, u, "operator"), got, ref.M, ref.bound_log, ref.sent))
    builds.worst.add("get_loglik_marginal_tensor (k_phase_b, all bins log-domain)", worst)
    print(f"\n[{name}] get_loglik_marginal_tensor worst observed / bound {worst:.3f}")
    _report(problems)


# ---------------------------------------------------------------- tile extents and the M-step's sentinel tails
EXTENT_N = (15, 16, 17, 63, 64, 65, 255, 256, 257)


def _sites_df(N):
    """Exactly N bins (x = 5 k + 2, l = 98: one bin per k), read counts shaped into two clear sites (three from N = 63)."""
    k = np.arange(N)
    centres = (0.2, 0.75) if N < 63 else (0.15, 0.5, 0.85)
    w = max(1.5, N / 24)
    cnt = 1 + sum(np.rint(40 * np.exp(-0.5 * ((k - c * N) / w) ** 2)).astype(int) for c in centres)
    x = np.repeat(5 * k + 2, cnt)
    n = len(x)
    return pd.DataFrame({"x": x.astype(np.int64), "l": np.full(n, 98, np.int64), "r": np.full(n, np.nan),
                         "pa": np.full(n, np.nan), "cb_id": np.arange(n), "read_id": np.arange(n)})


def test_tile_extents_and_mstep_tails_at_bin_count_boundaries(hip_ctx, oracle, monkeypatch):
    """UTRs of exactly N = 15 ... 257 bins (row pitch 16: N on, one below and one above a multiple of 16, of 64, of
    256) through prepare_utr.  K = 1, 2, 3 from Model.init_para(K), non-fixed and fixed: alpha, beta, rounds exact and
    ws / bic / lb to the tolerances of test_em_column_classes.py against the oracle's em_algo records; the same bits
    under SCAPE_HIP_MSTEP=v2, v3 and the default, on the tile extents of every Phase B form."""
    from test_em_column_classes import _bits, _bits_differ, _Dev, _LJob, _oracle_model, _vs_oracle
    from test_em_column_classes import _report as report_em
    from scape_amd.engine import HipBatch, pack_jobs
    from scape_amd.host import prepare_utr
    dfs = [_sites_df(N) for N in EXTENT_N]
    preps = [prepare_utr(df, gene_info_str=f"syn:EXT{N}:1:1-2000:+") for df, N in zip(dfs, EXTENT_N)]
    models = [_oracle_model(oracle, df) for df in dfs]
    jobs = []
    for u, (q, m, N) in enumerate(zip(preps, models, EXTENT_N)):
        assert q.N == N == m.N and np.array_equal(q.theta, m.all_theta) and np.array_equal(q.betas, m.betas)
        assert np.array_equal(q.cnt, m.cnt) and q.L == m.L and q.unif_ll == m.unif_ll
        for K in (1, 2, 3):
            np.random.seed((SEED + 1000 * N + K + 10 * RESEED.get((N, K), 0)) % 2 ** 32)
            p0 = m.init_para(K)
            m.em_algo(copy.deepcopy(p0))
            m.em_algo(copy.deepcopy(p0), fixed=True)
            jobs.append(_LJob(u, K, 0, q, m.calls[-2], m.calls[-1]))
    pairs = [(j, False) for j in jobs] + [(j, True) for j in jobs]
    pj = pack_jobs([j.job(fixed) for j, fixed in pairs])
    problems, dev, ref_bits = [], _Dev(), None
    for pb in MODES:
        if pb is None:
            monkeypatch.delenv("SCAPE_HIP_PHASE_B", raising=False)
        else:
            monkeypatch.setenv("SCAPE_HIP_PHASE_B", pb)
        batch = HipBatch(hip_ctx, preps)
        batch.build()
        assert batch.phase_b_form() == {"v2": 0, "split": 1, None: 2}[pb]
        for ms in ("v2", "v3", None):
            if ms is None:
                monkeypatch.delenv("SCAPE_HIP_MSTEP", raising=False)
            else:
                monkeypatch.setenv("SCAPE_HIP_MSTEP", ms)
            out = [np.array(x).copy() for x in batch.em_packed(pj)]
            bits = [_bits(pj, out, i) for i in range(len(pairs))]
            if ref_bits is None:
                ref_bits = bits
                for i, (j, fixed) in enumerate(pairs):
                    tag = (f"N={EXTENT_N[j.u]}", "fixed" if fixed else "non-fixed", j.K)
                    _vs_oracle(j.prep, pj, out, i, j.rec[fixed], dev, ("N boundary", 4), tag, problems)
            for (j, fixed), a, b in zip(pairs, ref_bits, bits):
                if _bits_differ(a, b):
                    problems.append((f"Phase B {pb}, M-step {ms}", EXTENT_N[j.u], j.K, fixed, _bits_differ(a, b)))
        batch.free()
    monkeypatch.delenv("SCAPE_HIP_MSTEP", raising=False)
    monkeypatch.delenv("SCAPE_HIP_PHASE_B", raising=False)
    dev.show("N boundaries")
    report_em(problems, "tile extents / M-step tails")
