"""The long-double reference of the tensor build (oracle/tensor_reference.py) and its per-entry rounding bound, validated
on the CPU with an independent f64 implementation - the C oracle - on every input of the ladder (tests/tensor_ladder.py),
before any GPU is involved.  tests/test_tensor_ladder.py then holds the HIP kernels to the same bound.
"""
import numpy as np
import pytest

import tensor_ladder as tl

SENT = float(np.finfo("f").min)
FLAT_RTOL = 1e-13            # what test_phase_a_b_vs_reference_trace and its like allow on a log-domain value


@pytest.fixture(scope="module")
def ladder():
    return tl.cases()


def test_long_double_has_a_64_bit_mantissa():
    assert np.finfo(np.longdouble).nmant >= 63


def test_comparisons_are_exact_and_no_entry_sits_on_the_cut(ladder):
    """Integer / dyadic inputs: l <= theta - x and the window ends come out the same in f64 and in long double, and no
    r-unknown entry lies within a relative 1e-6 of the v < 1e-300 cut - the sentinel pattern is then a matter of the
    formulas alone.  The 'cut' case has entries within two decades of the cut on either side: a cut constant that is off
    by more changes its sentinel pattern."""
    for c in ladder:
        for q, (a, b) in zip(c.preps, tl.reference(c)):
            assert a.cmp_mismatch == 0 and b.cmp_mismatch == 0, (c.name, q.gene_info_str)
            assert a.cut_distance > 1e-6, (c.name, q.gene_info_str, a.cut_distance)
    cut = next(c for c in ladder if c.name == "cut")
    q, (a, _b) = cut.preps[0], tl.reference(cut)[0]
    ru = a.kind == 0
    kept = a.V[ru][a.V[ru] > 0].astype(np.float64)
    assert 1e-300 <= kept.min() < 1e-298, kept.min()                # just above the cut
    assert 1e-302 < a.v_cut_max < 1e-300, a.v_cut_max               # just below it
    assert (a.sent[ru] & (q.l[ru][:, None] <= q.theta[None, :] - q.x[ru][:, None])).any()      # cut, not infeasible


def test_c_oracle_lies_within_the_bound_on_every_ladder_input(ladder, oracle):
    """oracle.phase_a and oracle.get_loglik_marginal_tensor (plain f64, library exp / log, divisions) against the
    long-double values: the same sentinel pattern, every finite entry within its bound (the C code takes every bin
    through the log-domain path: bound_log).  Also the f64 numpy twin phase_a_np on the smaller UTRs."""
    from oracle import tensor_reference as tr
    worst = {"A": 0.0, "M": 0.0}
    problems = []
    for c in ladder:
        for q, (a, b) in zip(c.preps, tl.reference(c)):
            A = oracle.phase_a(q.x, q.l, q.r, q.pa, q.theta, q.s_dis, q.pmf_s, q.p["mu_f"], q.p["sigma_f"])
            same, ratio, n_out = tr.compare(A, a.A, a.bound, a.sent)
            worst["A"] = max(worst["A"], ratio)
            if not same or n_out:
                problems.append((c.name, q.gene_info_str, "A", same, ratio, n_out))
            M = oracle.get_loglik_marginal_tensor(q.theta, q.betas, A)
            same, ratio, n_out = tr.compare(M, b.M, b.bound_log, b.sent)
            worst["M"] = max(worst["M"], ratio)
            if not same or n_out:
                problems.append((c.name, q.gene_info_str, "M", same, ratio, n_out))
            if q.N * q.T <= 2000:
                An = oracle.phase_a_np(q.x, q.l, q.r, q.pa, q.theta, q.s_dis, q.pmf_s, q.p["mu_f"], q.p["sigma_f"])
                same, ratio, n_out = tr.compare(An, a.A, a.bound, a.sent)
                if not same or n_out:
                    problems.append((c.name, q.gene_info_str, "A numpy twin", same, ratio, n_out))
    print(f"\n[C oracle against long double] worst observed / bound: A {worst['A']:.3f}, M {worst['M']:.3f}")
    assert not problems, problems[:20]


def test_bound_is_sharp(ladder):
    """Over the finite entries of the ladder the median bound is at most 1/20 of the flat tolerance
    (1e-13 |value|) at the same entries - for A, for M through the log-domain path and for M as the batched build
    computes it."""
    ba, fa, bl, bd, fm = [], [], [], [], []
    for c in ladder:
        for a, b in tl.reference(c):
            fin = ~a.sent
            ba.append(a.bound[fin])
            fa.append(FLAT_RTOL * np.abs(a.A[fin]).astype(np.float64))
            fin = ~b.sent
            bl.append(b.bound_log[fin])
            bd.append(b.bound_dev[fin])
            fm.append(FLAT_RTOL * np.abs(b.M[fin]).astype(np.float64))
    ba, fa, bl, bd, fm = map(np.concatenate, (ba, fa, bl, bd, fm))
    assert len(ba) > 10000 and len(fm) > 100000
    assert np.all(ba > 0) and np.all(bl > 0) and np.all(bd > 0)
    u = 2.0 ** -53
    print(f"\n[bound] median in u: A {np.median(ba) / u:.0f} (flat {np.median(fa) / u:.0f}), M log path {np.median(bl) / u:.0f}, "
          f"M batched build {np.median(bd) / u:.0f} (flat {np.median(fm) / u:.0f})")
    assert np.median(ba) <= np.median(fa) / 20
    assert np.median(bl) <= np.median(fm) / 20
    assert np.median(bd) <= np.median(fm) / 20


def test_operator_reference_takes_an_f64_input(ladder):
    """phase_b_ld(A=...) - the reference of get_loglik_marginal_tensor, whose input is an f64 A - against the chained
    reference: the same sentinel pattern, values within the chained bound of each other (they differ by the rounding of A
    to f64), and a bound that is never larger (it has no Phase A share)."""
    from oracle import tensor_reference as tr
    c = next(c for c in ladder if c.name == "N")
    for q, (a, b) in list(zip(c.preps, tl.reference(c)))[:4]:
        A64 = np.where(a.sent, SENT, a.A.astype(np.float64))
        op = tr.phase_b_ld(q.theta, q.betas, A=A64)
        assert np.array_equal(op.sent, b.sent)
        fin = ~b.sent
        assert np.all(np.abs(op.M[fin] - b.M[fin]).astype(np.float64) <= b.bound_log[fin])
        assert np.all(op.bound_log[fin] <= b.bound_log[fin])


def test_compare_reports_nan_and_inf_as_beyond_the_bound():
    """A NaN or an infinity at a non-sentinel entry is neither a sentinel nor within any bound; a sentinel where the
    reference has a value (and the reverse) breaks the pattern."""
    from oracle import tensor_reference as tr
    ref = np.array([[-5.0, -6.0, SENT]], dtype=np.longdouble)
    bound, sent = np.array([[1e-13, 1e-13, 0.0]]), np.array([[False, False, True]])
    assert tr.compare([[-5.0, -6.0, SENT]], ref, bound, sent) == (True, 0.0, 0)
    for bad in (np.nan, np.inf, -np.inf):
        same, ratio, n_out = tr.compare([[bad, -6.0, SENT]], ref, bound, sent)
        assert same and ratio == np.inf and n_out == 1, bad
    same, ratio, n_out = tr.compare([[-5.0, -6.0 - 3e-13, SENT]], ref, bound, sent)
    assert same and 2.9 < ratio < 3.1 and n_out == 1
    assert not tr.compare([[-5.0, SENT, SENT]], ref, bound, sent)[0]
    assert not tr.compare([[-5.0, -6.0, -7.0]], ref, np.array([[1e-13, 1e-13, 1e-13]]), sent)[0]
    same, ratio, n_out = tr.compare([[-5.0, -6.0, np.nan]], ref, bound, sent)      # NaN where the reference has the sentinel
    assert not same and ratio == np.inf and n_out == 1
