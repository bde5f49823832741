"""oracle/label_reference.py and the ladder of tests/label_ladder.py, checked on the CPU.

On the C oracle's tensor every ladder case must meet the ladder's conditions (no NEAR bin; every listed perturbation
changes a bin that is not NEAR; each planted bin's two signs give c0 and c1), and the C oracle's own so_get_label - plain
f64, library exp and log, true divisions: an independent implementation - must return the reference's label on every
DECIDED and TIE bin of the ladder and on a few thousand bins of random models.  Each named wrong labelling is checked
against a small example worked out by hand.  tests/test_label_ladder.py runs the same cases on the GPU.

Printed by the run (measurements on the oracle's tensor): TIGHT = 2; 44,932 bins of 191 models, near = 0, 1,108 exact
ties; the largest bound of a runner-up column is 9.0e-13 (a far runner-up in the ties family: the bound grows with the
gap), below 2e-13 on every planted pair; the smallest gap / bound of a decided bin is 1.99 - the planted bins, by
construction - and 1.7e10 outside the planted and counts families, which is how blunt random models are (3.1e9 over the
7,668 bins of the random models below).  Of the 148 planted bins the C oracle labels 0, 0, 0, 13, 36 wrongly at
TIGHT = 2, 1, 1/2, 1/4, 1/8.
"""
import numpy as np
import pytest

import label_ladder as ll
from oracle import label_reference as lr

CASES = ll.cases()
BY_NAME = {c.name: c for c in CASES}
_STAT = {}


def _tensors(case):
    return [ll.oracle_tensor(q) for q in case.preps]


@pytest.fixture(scope="module", autouse=True)
def _summary():
    yield
    if len(_STAT) == len(CASES):
        s = list(_STAT.values())
        print(f"\n[label reference] TIGHT = {ll.TIGHT:g}; {sum(x['bins'] for x in s)} bins of {sum(x['models'] for x in s)} models, "
              f"near = {sum(x['near'] for x in s)}, exact ties {sum(x['tie'] for x in s)}; largest bound {max(x['bound'] for x in s):.2g}; "
              f"smallest decided gap / bound {min(x['ratio'] for x in s):.3g} "
              f"(outside planted and counts {min(x['ratio'] for k, x in _STAT.items() if k not in ('planted', 'counts')):.2g})")


@pytest.mark.parametrize("name", [c.name for c in CASES])
def test_ladder_case_meets_its_conditions_and_agrees_with_the_c_oracle(oracle, name):
    case = BY_NAME[name]
    Ms = _tensors(case)
    problems, ws, refs, stat = ll.check_case(case, Ms)
    for mi, (m, r) in enumerate(zip(case.models, refs)):
        got = ll.oracle_labels(case.preps[m.u], Ms[m.u], m, ws[mi])
        sure = r.kind != lr.NEAR
        bad = np.nonzero(sure & (got != r.label))[0]
        if len(bad):
            problems.append((name, mi, m.note, "the C oracle disagrees on decided / tie bins", bad[:5].tolist(), got[bad[:5]].tolist(),
                             r.label[bad[:5]].tolist()))
        if not np.all(r.accept[np.arange(len(got)), got]):
            problems.append((name, mi, m.note, "the C oracle returns a label outside the accepted ones"))
        # a model's labels do not depend on the call it is part of
        for call in case.calls:
            if mi in call and len(call) > 1:
                for kmax in ll.pitches(case, call):
                    assert np.array_equal(ll.reference(case, Ms, ws, mi, None, call, kmax).label, r.label), (name, mi, call, kmax)
    stat["models"] = len(case.models)
    _STAT[name] = stat
    print(f"\n[label ladder, CPU] {name}: {len(case.models)} models, {stat['bins']} bins, near {stat['near']}, ties {stat['tie']}, "
          f"largest bound {stat['bound']:.2g}, smallest gap / bound {stat['ratio']:.3g}")
    assert stat["near"] == 0
    assert not problems, f"{len(problems)} problems\n" + "\n".join(repr(p) for p in problems[:30])


def _planted():
    return [(c, mi) for c in CASES for mi, m in enumerate(c.models) if m.plant]


def test_tight_is_the_smallest_power_of_two_that_decides_and_the_c_oracle_holds(oracle):
    """The C oracle's label on every planted bin at TIGHT and at the powers of two below it.  A planted bin is DECIDED only
    when its gap exceeds its bound, so TIGHT > 1: 2 is the smallest power of two the conditions allow, and the C oracle must
    be right on every planted bin there (condition (c) with it: the two signs give c0 and c1).  Below - where the reference
    calls the bins NEAR - the oracle's wrong labels are counted and printed: they show where plain f64 stops resolving."""
    wrong = {}
    for tight in (ll.TIGHT, 1.0, 0.5, 0.25, 0.125):
        wrong[tight] = 0
        for case in {c.name: c for c, _mi in _planted()}.values():
            Ms = _tensors(case)
            ws = ll.resolve(case, Ms, tight)
            for mi, m in enumerate(case.models):
                if m.plant:
                    n, c0, c1, sign = m.plant
                    got = ll.oracle_labels(case.preps[m.u], Ms[m.u], m, ws[mi])
                    wrong[tight] += int(got[n] != (c0 if sign > 0 else c1))
    n_planted = len(_planted())
    print(f"\n[label reference] planted bins: {n_planted}; the C oracle's wrong labels at TIGHT = "
          + ", ".join(f"{t:g}: {w}" for t, w in wrong.items()))
    assert n_planted == 2 * (len(ll.PLANT_PAIRS) * len(ll.PLANT_BINS) * len(ll.PLANT_COUNTS) + 2)
    assert ll.TIGHT == 2.0 and wrong[ll.TIGHT] == 0 and wrong[0.125] > 0, wrong
    for tight in (1.0,):                                          # at the bound itself the planted bins are not decided
        case = BY_NAME["counts"]
        assert ll.check_case(case, _tensors(case), tight)[3]["near"] > 0


def test_random_models_agree_with_the_c_oracle(oracle):
    """A few thousand bins of random models, K = 1 .. 63, on UTRs of the ladder: equal wherever the reference is sure, and
    it is sure everywhere (random bins have ten orders of magnitude of room)."""
    bins = near = 0
    worst = np.inf
    for N in (17, 65, 257, 513):
        q = ll.lab_utr(N)
        M = ll.oracle_tensor(q)
        for i, K in enumerate((1, 2, 3, 5, 8, 13, 21, 34, 63)):
            m = ll.random_model(q, K, 500 + 10 * N + i)
            r = lr.label_model(M, q.cnt, q.unif_ll, K, m.a_idx, m.b_idx, m.ws)
            got = ll.oracle_labels(q, M, m, m.ws)
            sure = r.kind != lr.NEAR
            assert np.array_equal(got[sure], r.label[sure]), (N, K)
            bins, near, worst = bins + N, near + r.near, min(worst, r.ratio)
    print(f"\n[label reference] random models: {bins} bins, near {near}, smallest gap / bound {worst:.3g}")
    assert bins > 5000 and near == 0 and worst > 1e6


def test_ladder_cases_sit_on_their_boundaries(oracle):
    """What the constructions promise."""
    by = BY_NAME
    # bins, classes: the tables as the module states them; a > 0 and b > 0 everywhere
    assert [q.N for q in by["bins"].preps] == list(ll.N_BINS) and [m.K for m in by["classes"].models] == list(ll.K_CLASSES)
    assert all(m.a_idx.min() > 0 and m.b_idx.min() > 0 for n in ("bins", "classes", "calls") for m in by[n].models if m.K)
    assert by["bins"].calls[-1] == tuple(range(len(ll.N_BINS)))
    c = by["classes"]
    Ms = _tensors(c)
    refs = ll.check_case(c, Ms)[2]
    top = refs[list(ll.K_CLASSES).index(63)].label
    assert top.max() > 31 and np.any(top == 63)                   # high columns win bins, and so does the uniform column
    for m, r in zip(c.models, refs):
        assert np.any(r.label == m.K), m.note                     # ... in every model: a kernel that reads beyond K has something to lose
    # planted: every pair, bin, sign and count; the gap is TIGHT bounds, the others 3 below
    c = by["planted"]
    assert {(m.K,) + m.plant[1:3] for m in c.models} == set(ll.PLANT_PAIRS) and {m.plant[0] for m in c.models} == set(ll.PLANT_BINS)
    assert [int(q.cnt[n]) for q in c.preps for n in ll.PLANT_BINS] == [cv for cv in ll.PLANT_COUNTS for _n in ll.PLANT_BINS]
    assert ll.PLANT_BINS == (0, ll.BLOCK - 1, ll.BLOCK) and ll.PLANT_N == ll.BLOCK + 1 and max(ll.PLANT_COUNTS) == c.preps[0].cnt.max()
    Ms = _tensors(c)
    _pr, ws, refs, _st = ll.check_case(c, Ms)
    for m, r in zip(c.models, refs):
        n = m.plant[0]
        assert 0.99 * ll.TIGHT < r.gap[n] / r.bound[n] < 1.01 * ll.TIGHT, (m.note, r.gap[n] / r.bound[n])
        assert r.bound[n] < 2e-13 and r.gap[n] < 4e-13
    by_bin = {}
    for m, r in zip(c.models, refs):
        by_bin.setdefault((m.u, m.K) + m.plant[:3], set()).add(int(r.label[m.plant[0]]))
    assert all(len(v) == 2 for v in by_bin.values())              # (c): the two signs, two labels
    # ties
    c = by["ties"]
    Ms = _tensors(c)
    _pr, ws, refs, _st = ll.check_case(c, Ms)
    for (K, c0, c1), r in zip(ll.TIE_PAIRS, refs):
        t = r.kind == lr.TIE
        assert t.sum() > 50 and np.all(r.label[t] == c0) and not np.any(r.label == c1), (K, c0, c1)
    notes = {m.note: (m, r) for m, r in zip(c.models, refs)}
    m, r = notes["three-way tie"]
    assert np.all(r.label[r.kind == lr.TIE] == 0) and (r.kind == lr.TIE).sum() > 50 and r.accept[r.kind == lr.TIE].sum(axis=1).max() == 1
    m, r = notes["every column sentinel-class at bin 0"]
    assert r.label[0] == 0 and r.kind[0] == lr.TIE and np.all(r.lz[0] == lr.SENT) and m.ws[-1] == 0.0
    assert np.all(Ms[0][m.a_idx, m.b_idx, 0] == lr.SENT)
    m, r = notes["weight exactly 0 on the column that would win"]
    assert not np.any(r.label == 0) and np.sum(ll.reference(c, Ms, ws, c.models.index(m), "zero_weight_as_one").label == 0) > 100
    m, r = notes["weight 1e-300"]
    only = (Ms[0][m.a_idx[0], m.b_idx[0]] != lr.SENT) & (Ms[0][m.a_idx[1], m.b_idx[1]] == lr.SENT)
    assert only.sum() > 100 and np.all(r.label[only] == 0) and np.all(r.lz[only, 0] < -690) and np.all(r.kind[only] == lr.DECIDED)
    # counts: the planted bin at cnt = 1000; bins where every losing column, finite ones included, falls below the clamp
    c = by["counts"]
    q = c.preps[0]
    assert q.cnt[ll.COUNT_BIN] == ll.COUNT_MAX == 1000 and q.cnt.max() == 1000 and all(m.plant[0] == ll.COUNT_BIN for m in c.models[:-1])
    Ms = _tensors(c)
    refs = ll.check_case(c, Ms)[2]
    r = refs[-1]
    los = np.ones(r.arg.shape, bool)
    los[np.arange(q.N), r.label] = False
    under = np.all(np.where(los, r.arg, -np.inf) < ll.EXP_CLAMP, axis=1) & np.any(los & (r.lz > lr.SENT / 2), axis=1)
    alive = np.any(los & (r.arg > ll.EXP_CLAMP) & (r.arg < 0), axis=1)
    assert under.sum() >= 5 and alive.sum() >= 5                  # both sides of the clamp
    assert not np.any((r.arg > ll.EXP_CLAMP - 5) & (r.arg < ll.EXP_CLAMP + 5))
    # calls: the selections, and the two model sets differ on most bins of every UTR (a stale label buffer would show)
    c = by["calls"]
    sel = [[c.models[i].u for i in call] for call in c.calls]
    assert sel == [[0], [3, 0], [0, 2, 3], [0, 1, 2, 3], [0, 2, 3], [0], [0, 1, 2, 3], [3, 0]]
    sets = [{i // 4 for i in call} for call in c.calls]
    assert all(len(s) == 1 for s in sets) and [s.pop() for s in sets] == [0, 1, 0, 1, 1, 1, 0, 0]
    assert [q.N for q in c.preps] == list(ll.CALL_N) and all(len({c.models[i].K for i in call}) == len(call) for call in c.calls)
    Ms = _tensors(c)
    refs = ll.check_case(c, Ms)[2]
    for u in range(4):
        assert np.mean(refs[u].label != refs[4 + u].label) > 0.8, u
    # every named wrong labelling is some model's
    named = {p for cs in CASES for m in cs.models for p in m.perturb}
    assert named == set(lr.PERTURBATIONS), named ^ set(lr.PERTURBATIONS)


# ---------------------------------------------------------------------------------------------------------------------
# by hand: T = 2, B = 2, N = 3 (Np = 16); rows (a, b) -> 2 a + b; unif_ll = log 1/8; cnt = (1, 2, 3)
#   row 0 = sentinel everywhere; row 1 = log (1/2, 1/4, S); row 2 = log (1/4, 1/2, 1/2); row 3 = log (1/16, 1/4, S)   (S: sentinel)
#   model K = 2: columns (a, b) = (1, 1) -> row 3 and (1, 0) -> row 2, ws = (1/2, 1/4, 1/4)
#   bin 0: (1/32, 1/16, 1/32) -> 1      bin 1: (1/8, 1/8, 1/32) -> a plain f64 near-tie: log 1/2 + log 1/4 against log 1/4 + log 1/2
#   bin 2: (S, 1/8, 1/32) -> 1
def _hand(perturb=None, ws=(0.5, 0.25, 0.25), ab=((1, 1), (1, 0)), sel=0, tables=None):
    S = lr.SENT
    with np.errstate(divide="ignore"):
        M = np.log(np.array([[[0, 0, 0], [0.5, 0.25, 0]], [[0.25, 0.5, 0.5], [1 / 16, 0.25, 0]]]))
    M[np.isinf(M)] = S
    cnt, ul = np.array([1.0, 2.0, 3.0]), float(np.log(0.125))
    if tables is not None:
        return lr.label_call(M, cnt, ul, sel, *tables, perturb)
    return lr.label_model(M, cnt, ul, len(ab), [x[0] for x in ab], [x[1] for x in ab], ws, perturb)


def test_each_wrong_labelling_does_what_its_name_says():
    base = _hand()
    assert base.label.tolist() == [1, 0, 1] and base.kind.tolist() == [lr.DECIDED, lr.NEAR, lr.DECIDED]
    assert base.accept[1].tolist() == [True, True, False] and base.gap[1] < 1e-15 and 1e-16 < base.bound[1] < 1e-14
    assert base.lz[2, 0] == lr.SENT and base.gap[0] == pytest.approx(np.log(2), rel=1e-15)
    assert base.arg[0].tolist() == pytest.approx([-np.log(2), 0, -np.log(2)]) and base.arg[2, 2] == pytest.approx(-3 * np.log(4))
    # exact ties: the same row with the same weight; the first wins, last_max takes the last
    tie = _hand(ab=((1, 0), (1, 0)), ws=(0.25, 0.25, 0.25))
    assert tie.label.tolist() == [0, 0, 0] and tie.kind.tolist() == [lr.TIE] * 3 and tie.accept.sum() == 3
    assert _hand("last_max", ab=((1, 0), (1, 0)), ws=(0.25, 0.25, 0.25)).label.tolist() == [1, 1, 1]
    # drop_b: column 0 reads row 2 like column 1, with the larger weight
    assert _hand("drop_b").label.tolist() == [0, 0, 0]
    # pitch_N: row r of bin n is read at flat r * 3 + n of the [4, 16] buffer: rows 2 and 3 become row 0's bins 6 .. 11 - all sentinel
    p = _hand("pitch_N")
    assert p.label.tolist() == [2, 2, 2] and np.all(p.lz[:, :2] == lr.SENT)
    # uniform_as_component: column K reads row 0 (sentinel)
    assert np.all(_hand("uniform_as_component").lz[:, 2] == lr.SENT)
    assert _hand("uniform_as_component", ws=(0.5, 0.25, 0.9)).label.tolist() == [1, 0, 1] != _hand(ws=(0.5, 0.25, 0.9)).label.tolist()
    # drop_last_bin, first_block_only: bins without a label keep -1
    assert _hand("drop_last_bin").label.tolist() == [1, 0, -1] and _hand("first_block_only").label.tolist() == [1, 0, 1]
    # zero weights: the sentinel; as log 0 = 0 the column wins
    z = _hand(ws=(0.5, 0.0, 0.125))
    assert z.label.tolist() == [0, 0, 2] and np.all(z.lz[:, 1] == lr.SENT) and z.lz[2, 0] == lr.SENT and z.near == 0
    assert _hand("zero_weight_as_one", ws=(0.5, 0.0, 0.125)).label.tolist() == [1, 1, 1]
    both = _hand(ws=(0.0, 0.0, 0.0))                              # every column sentinel-class: 2 SENT, SENT, SENT at bin 2 - and SENT wins
    assert both.lz[2].tolist() == [2 * lr.SENT, lr.SENT, lr.SENT] and both.label.tolist() == [0, 0, 1] and both.kind.tolist() == [lr.TIE] * 3
    # sentinel_as_zero: column 0 of bin 2 reads 0
    assert _hand("sentinel_as_zero").label.tolist() == [1, 0, 0]
    # the table pitches: two rows at kmax = 2; row 1 read at pitch 3 / its weights at pitch 2
    a, b = np.array([[1, 1], [1, 1]]), np.array([[1, 0], [0, 1]])
    w = np.array([[0.5, 0.25, 0.25], [0.25, 0.125, 0.25]])
    t = ([2, 2], a, b, w)
    assert _hand(tables=t, sel=0).label.tolist() == [1, 0, 1] and _hand(tables=t, sel=1).label.tolist() == [0, 0, 0]
    assert _hand("k_pitch_plus1", tables=t, sel=0).label.tolist() == [1, 0, 1]
    kp = _hand("k_pitch_plus1", tables=t, sel=1)                  # a = (1, 0 beyond the table), b = (1, 0): rows 3 and 0
    assert np.all(kp.lz[:, 1] == lr.SENT) and kp.label.tolist() == [2, 0, 2]
    wp = _hand("w_pitch_k", tables=t, sel=1)                      # weights (0.25, 0.25, 0.125) from flat 2 ..
    assert wp.label.tolist() == [0, 0, 0] and wp.lz[0, 2] == pytest.approx(np.log(0.125 / 8))
    with pytest.raises(AssertionError):
        _hand("no_such_labelling")


def test_the_bound_follows_the_chain():
    """bound(best, d) = MARGIN u [E(lz_best) + E(lz_d) + 2 |d_d| + (2 EXP_DEV + 2) / cnt] on the hand example."""
    r = _hand()
    u, lg = lr.U, np.log
    E = lambda w, lz: lr.LIB * abs(lg(w)) + abs(lz)                # noqa: E731
    want0 = lr.MARGIN * u * (E(0.25, lg(1 / 16)) + E(0.5, lg(1 / 32)) + 2 * lg(2) + (2 * lr.EXP_DEV + 2) / 1.0)
    assert r.second[0] in (0, 2) and r.bound[0] == pytest.approx(want0, rel=1e-12) or r.bound[0] == pytest.approx(
        lr.MARGIN * u * (E(0.25, lg(1 / 16)) + E(0.25, lg(1 / 32)) + 2 * lg(2) + (2 * lr.EXP_DEV + 2)), rel=1e-12)
    want1 = lr.MARGIN * u * (E(0.5, lg(1 / 8)) + E(0.25, lg(1 / 8)) + 2 * float(r.gap[1]) + (2 * lr.EXP_DEV + 2) / 2.0)
    assert r.bound[1] == pytest.approx(want1, rel=1e-12)
    # a sentinel-class runner-up carries no error of its own; the counts shrink only the exp and division terms
    assert r.second[2] == 2 and lr.MARGIN == 2 and lr.EXP_DEV == 1.2 and lr.LIB == 2
