"""k_labels on the GPU at its boundary shapes, against the long-double reference of oracle/label_reference.py.

Every case of tests/label_ladder.py (tests/test_host.py checks the ladder against the constants of the sources,
tests/test_label_reference.py its conditions and the reference itself on the CPU) is loaded on a handle of its own and
built; the DEVICE'S OWN tensor is fetched and the reference evaluated on it, so that the rounding of the tensor build is
out of the comparison - the planted family's weights are computed from that tensor too.  The case's conditions are
asserted again on it (no NEAR bin, every listed wrong labelling changes a bin, the planted signs give c0 and c1).  Every
call of the case then runs, in the case's order on the one handle, at its own table pitch (kmax = max(1, K)) and padded
to kmax = 63 with junk beyond each model's K, and per call:
  - every bin of a selected UTR carries the reference's label (DECIDED and TIE bins: exactly that one);
  - every bin of an unselected UTR keeps the caller's -1;
  - every (UTR, model) returns identical labels in every call and at every pitch that holds it.
Mismatches are collected and reported together.  The column classes reached (kmax + 1 against LabelClasses, as
with_column_class dispatches them) must be all four.  A call that names a UTR twice is refused, and the handle works
afterwards.

Measured on an MI355X (printed by every run; measurements, not targets): 355 label calls, 89,007 bins compared, zero
mismatches, classes <8>, <16>, <32>, <64> reached; on the device's tensor near = 0, 1,108 exact ties, smallest gap / bound
1.99 (the planted bins).  The module takes about 0.5 s - its slowest case, bins, 0.3 s - next to the 1.2 s of
tests/test_estep_ladder.py.

What the ladder can and cannot see.  The scratch builds of k_labels with one change each were NOT run on a GPU: the
table below is what the reference's named wrong labellings (condition (b), asserted on the device's tensor by every run)
say each change does to the ladder, and is still to be confirmed by such builds:
  `zc > bz` -> `>=`                      last_max: the 7 tie models and the all-sentinel bin of "ties" (1,108 tie bins)
  `d.Np` -> `d.N` in roff                pitch_N: every model of "bins" with N % 16 != 0 (8 of 11)
  `+ b_in[...]` dropped                  drop_b: every model of "bins", of "classes" with K >= 1, "losers underflow" of "counts"
  `c < K` -> `c <= K` in the lz line     uniform_as_component: "bins" (N > 1) and "classes" (K >= 1) - row 0 of the tensor is all
                                         sentinel on these UTRs, so the bins that go to the uniform column lose it
  d_logw -> log without `w <= 0`         NOT covered by a named labelling: log 0 = -inf behaves like the sentinel in every sum
                                         (zero_weight_as_one, log 0 = 0, is the wrong reading the ties family lists); expected
                                         invisible except where every column is sentinel-class (-inf - -inf is a NaN)
  a float-rounded slw                    the planted family's target: log w moves by up to 6e-8 |log w|, some 1e6 planted gaps
  `slw + Mu` as __builtin_fma(1.0, ..)   expected invisible and harmless: fma(1, a, b) is the one rounding of a + b
  `* cn` dropped                         expected invisible and harmless: a positive factor cannot reorder columns, and with
                                         |lz| >= 1 a non-zero f64 gap of lz survives the exp (1 - 1e-16 |lz| is not 1)
"""
import time

import numpy as np
import pytest

import label_ladder as ll

pytestmark = pytest.mark.gpu
CASES = ll.cases()
BY_NAME = {c.name: c for c in CASES}
_CLASSES = set()
_T0 = time.perf_counter()
_DONE = []


class _Loaded:
    """One ladder case on a library handle of its own, built."""

    def __init__(self, case):
        from scape_amd import _lib, engine
        self.ctx = _lib.Context(0)
        self.batch = engine.HipBatch(self.ctx, case.preps)
        self.batch.build()
        self.M = [self.batch.fetch_tensor(u) for u in range(len(case.preps))]

    def close(self):
        self.batch.free()
        self.ctx.close()


@pytest.fixture(scope="module", autouse=True)
def _summary():
    yield
    if len(_DONE) == len(CASES):
        print(f"\n[label ladder] column classes reached: {sorted(_CLASSES)}; {sum(d[0] for d in _DONE)} label calls, "
              f"{sum(d[1] for d in _DONE)} bins compared; the module took {time.perf_counter() - _T0:.2f} s from its import")


@pytest.mark.parametrize("name", [c.name for c in CASES])
def test_label_ladder_case(name):
    case = BY_NAME[name]
    ld = _Loaded(case)
    try:
        _run_case(case, ld)
    finally:
        ld.close()


def _run_case(case, ld):
    # ---- the reference on the device's tensor; the ladder's conditions again
    problems, ws, refs, stat = ll.check_case(case, ld.M)
    problems = [p[:3] + ("conditions on the device's tensor",) + p[3:] for p in problems]
    off = ld.batch.bin_off
    first, n_calls, n_bins = {}, 0, 0
    for ci, call in enumerate(case.calls):
        for kmax in ll.pitches(case, call):
            su, sk, a, b, w = ll.pack(case, call, kmax, ws)
            flat = ld.batch.labels_packed(su, sk, a, b, w)
            _CLASSES.add(next(c for c in ll.CLASSES if kmax + 1 <= c))
            n_calls += 1
            rest = np.ones(len(flat), bool)
            for mi in call:
                m, r = case.models[mi], refs[mi]
                tag = (case.name, f"call {ci} {list(call) if len(call) < 6 else len(call)}", f"kmax={kmax}", mi, m.note)
                got = flat[off[m.u]:off[m.u + 1]].astype(np.int64)
                rest[off[m.u]:off[m.u + 1]] = False
                n_bins += len(got)
                inside = (got >= 0) & (got <= m.K)
                ok = inside & r.accept[np.arange(len(got)), np.clip(got, 0, m.K)]
                if not ok.all():
                    bad = np.nonzero(~ok)[0]
                    problems.append(tag + (f"{len(bad)} wrong labels: bins, got, want, gap / bound", bad[:6].tolist(), got[bad[:6]].tolist(),
                                           r.label[bad[:6]].tolist(), (r.gap[bad[:6]] / np.maximum(r.bound[bad[:6]], 1e-300)).tolist()))
                if first.setdefault(mi, (tag, got))[1].tobytes() != got.tobytes():
                    problems.append(tag + ("labels differ from", first[mi][0][1:3], int((first[mi][1] != got).sum())))
            if not np.all(flat[rest] == -1):
                problems.append((case.name, f"call {ci}", f"kmax={kmax}", "bins of unselected UTRs were written", int((flat[rest] != -1).sum())))
    _DONE.append((n_calls, n_bins))
    print(f"\n[label ladder] {case.name}: {len(case.models)} models, {n_calls} calls, {n_bins} bins compared; on the device's tensor near "
          f"{stat['near']}, ties {stat['tie']}, largest bound {stat['bound']:.2g}, smallest gap / bound {stat['ratio']:.3g}")
    assert stat["near"] == 0
    assert not problems, f"{len(problems)} mismatches\n" + "\n".join(repr(p) for p in problems[:40])


def test_a_utr_named_twice_is_refused_and_the_handle_works_afterwards():
    """The output holds one label per bin: two models of one UTR in one call would be two workgroups writing the same bins.
    labels_check refuses the call before anything is queued."""
    from scape_amd import _lib
    case = BY_NAME["calls"]
    ld = _Loaded(case)
    try:
        _pr, ws, refs, _st = ll.check_case(case, ld.M)
        off = ld.batch.bin_off
        su, sk, a, b, w = ll.pack(case, (0, 2, 3), ll.KMAX_PAD, ws)
        want = ld.batch.labels_packed(su, sk, a, b, w)
        for twice in ([0, 2, 0], [3, 3, 2], [2, 2, 2]):
            with pytest.raises(_lib.ScapeHipError, match="labels: a UTR is named twice"):
                ld.batch.labels_packed(twice, sk, a, b, w)
        with pytest.raises(_lib.ScapeHipError, match="labels: a UTR is named twice"):
            ld.batch.labels_packed([1, 1], [1, 0], a[:2, :1], b[:2, :1], np.full((2, 2), 0.5))
        got = ld.batch.labels_packed(su, sk, a, b, w)
        assert np.array_equal(got, want) and np.all(got[off[1]:off[2]] == -1)
        for mi in (0, 2, 3):
            u = case.models[mi].u
            assert np.array_equal(got[off[u]:off[u + 1]], refs[mi].label)
    finally:
        ld.close()


def test_every_label_class_is_reached():
    """k_labels<8>, <16>, <32> and <64>: the classes of the pitches the ladder's calls run at (no API reports the kernel a call
    ran; with_column_class takes the first class that holds kmax + 1, and tests/test_host.py pins ll.CLASSES to LabelClasses).
    Each class is reached by a call at its own pitch whose largest K + 1 is the class's first and last column count."""
    cls = lambda kmax: next(c for c in ll.CLASSES if kmax + 1 <= c)          # noqa: E731
    own = {}
    for case in CASES:
        for call in case.calls:
            kmax = ll.pitches(case, call)[0]
            own.setdefault(cls(kmax), set()).add(kmax + 1)
    assert set(own) == set(ll.CLASSES)
    lo = 2
    for c in ll.CLASSES:
        assert {lo, c} <= own[c], (c, sorted(own[c]))
        lo = c + 1
    assert not _DONE or len(_DONE) < len(CASES) or _CLASSES == set(ll.CLASSES)
