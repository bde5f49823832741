"""The host frame of the permutation tests' entry points (perm.inc): a refused call leaves the handle as it was, and
scape_hip_report_free followed by the same calls gives the same outputs.

The matrix is rc.entry_point_matrix(): 4 records of 2, 5, 70 and 150 rows, 161 tested columns, 300 permutations, the
smallest shapes that cross the 64-row LDS class and the 256-permutation tile.

Every refusal used here is an argument refusal that fires ahead of the first queueing.  The entry points refuse after
rep_perm_prepare has queued work in three places only, and none can be reached on this matrix: a record of 2^31 or more
reads, reads x largest position of 2^48 or more in scape_hip_report_perm_len_trend (positions end at 2^22, so a record
of 2^26 reads), and more than 2^39 rows x groups in scape_hip_report_perm_pairs.
"""
import functools

import numpy as np
import pytest

import report_cases as rc

SIZES = np.array([50, 60, 51], dtype=np.int32)                  # three groups of the 161 tested columns
SEG = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int32)
PAIR_G, PAIR_H = np.array([0, 0, 1], dtype=np.int32), np.array([1, 2, 2], dtype=np.int32)
G = len(SIZES)


@functools.lru_cache(maxsize=None)
def matrix():
    n1, n2, n_cols, seed, n_perm, Ks, off, lab, cb, _dense, rows, roff, _rng = rc.entry_point_matrix()
    rng = np.random.default_rng(21)
    n_rows, n_rec = len(rows), len(Ks)
    return dict(n1=n1, n2=n2, n=n1 + n2, n_cols=n_cols, seed=seed, n_perm=n_perm, Ks=Ks, off=off, lab=lab, cb=cb,
                rows=rows, roff=roff, n_rows=n_rows, n_rec=n_rec,
                w=rng.integers(0, 2000, n_rows).astype(np.float64), tol=np.full(n_rec, 1e-9),
                x=rng.integers(0, 2000, n_rows).astype(np.int32),
                q=rng.integers(0, 60, n1 + n2).astype(np.uint16), rank=np.arange(n1 + n2, dtype=np.int32))


def _p(a):
    from scape_amd._lib import P_d, P_i32, P_i64, P_u16, ptr
    return ptr(a, {np.dtype(np.float64): P_d, np.dtype(np.int32): P_i32, np.dtype(np.int64): P_i64,
                   np.dtype(np.uint16): P_u16}[a.dtype])


def _outs(*spec):
    """fresh outputs: (length, dtype) each; the counters start at 0, everything else at -1"""
    return [np.zeros(n, np.int64) if dt == "counter" else np.full(n, -1, dt) for n, dt in spec]


def _builder(ctx, name):
    m, lib, h = matrix(), ctx.lib, ctx.h
    tail = (1, m["n_perm"], m["seed"])
    if name in ("perm_test", "perm_len"):
        return lib.scape_hip_report_perm_masks(h, m["n1"], m["n2"], *tail)
    if name in ("perm_groups", "perm_len_groups"):
        return lib.scape_hip_report_perm_labels(h, G, _p(SIZES), *tail)
    if name == "perm_pairs":
        return lib.scape_hip_report_perm_pair_masks(h, G, _p(SIZES), len(PAIR_G), _p(PAIR_G), _p(PAIR_H), *tail)
    if name == "perm_markers":
        return lib.scape_hip_report_perm_marker_masks(h, G - 1, _p(SIZES), int(SIZES[-1]), _p(m["rank"]), *tail)
    return lib.scape_hip_report_perm_scores(h, m["n"], _p(m["q"]), *tail)


def _call(ctx, name, bad=False):
    """one call of the test entry point `name` on the matrix, or (bad) the same call with one argument that it refuses;
    returns (rc, outputs)"""
    m, lib, h = matrix(), ctx.lib, ctx.h
    roff, rows, n_rec, R = m["roff"], m["rows"], m["n_rec"], m["n_rows"]
    i64, f64, cnt = np.int64, np.float64, "counter"
    if bad and name in ("perm_groups", "perm_trend"):           # one record of more rows than the entry point takes
        R, n_rec = (3999, 1) if name == "perm_groups" else (4001, 1)
        rows, roff = np.resize(rows, R).astype(np.int64), np.array([0, R], np.int64)
    head = (h, n_rec, _p(roff), _p(rows))
    if name == "perm_test":
        if bad:
            rows = rows.copy()
            rows[5] = int(m["Ks"].sum())                        # one past the last count row
            head = (h, n_rec, _p(roff), _p(rows))
        o = _outs((R, i64), (R, i64), (R, cnt), (n_rec, f64), (n_rec, cnt))
        return lib.scape_hip_report_perm_test(*head, *map(_p, o)), o
    if name == "perm_len":
        tol = m["tol"].copy()
        if bad:
            tol[1] = np.inf
        o = _outs((R, i64), (R, i64), (n_rec, f64), (n_rec, cnt))
        return lib.scape_hip_report_perm_len(*head, _p(m["w"]), _p(tol), *map(_p, o)), o
    if name == "perm_groups":
        o = _outs((R, i64), (R * G, i64), (R, cnt), (n_rec, f64), (R, f64), (n_rec, cnt))
        return lib.scape_hip_report_perm_groups(*head, G, _p(SEG), *map(_p, o)), o
    if name == "perm_len_groups":
        x = m["x"].copy()
        if bad:
            x[3] = -1
        o = _outs((R, i64), (R * G, i64), (n_rec, f64), (n_rec * G, f64), (n_rec, cnt), (n_rec * G, cnt))
        return lib.scape_hip_report_perm_len_groups(*head, G, _p(SEG), _p(x), _p(m["tol"]), _p(m["tol"]), *map(_p, o)), o
    if name in ("perm_pairs", "perm_markers"):
        n_items = len(PAIR_G) if name == "perm_pairs" else G - 1
        first = 1 if bad else 0                                 # the range then ends one past the last item
        o = _outs((R, i64), (R * G, i64), (n_items * R, cnt), (n_items * n_rec, f64), (n_items * n_rec, cnt))
        f = lib.scape_hip_report_perm_pairs if name == "perm_pairs" else lib.scape_hip_report_perm_markers
        return f(*head, G, _p(SEG), first, n_items, *map(_p, o)), o
    if name == "perm_trend":
        o = _outs((R, i64), (R, i64), (R, i64), (R, cnt), (R, f64), (n_rec, f64), (n_rec, cnt))
        return lib.scape_hip_report_perm_trend(*head, *map(_p, o)), o
    assert name == "perm_len_trend"
    x = m["x"].copy()
    if bad:
        x[0] = (1 << 22) + 1
    o = _outs((R, i64), (R, i64), (R, i64), (2 * n_rec, i64), (n_rec, cnt))
    return lib.scape_hip_report_perm_len_trend(*head, _p(x), *map(_p, o)), o


# entry point -> a word of the message of its refused call
ENTRY_POINTS = {"perm_test": "row index out of range", "perm_len": "tolerances", "perm_groups": "rounding bound",
                "perm_len_groups": "2^22", "perm_pairs": "must name pairs", "perm_markers": "must name markers",
                "perm_trend": "more than 4000 rows", "perm_len_trend": "2^22"}


def _counts(ctx):
    m = matrix()
    rc.device_counts(ctx, m["Ks"], m["off"], m["lab"], m["cb"], m["n_cols"])


def _good(ctx, name):
    from scape_amd._lib import check
    rc_, o = _call(ctx, name)
    check(rc_, name)
    assert np.all(o[0] >= 0), name                                              # written
    return [a.tobytes() for a in o]


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(ENTRY_POINTS))
def test_refused_call_leaves_the_handle_usable(name):
    """a valid call, a refused one (rc != 0 and its message), the valid call again: the two valid calls' outputs are equal
    to the bit"""
    from scape_amd import _lib
    ctx = _lib.default_context(None)
    try:
        _counts(ctx)
        _lib.check(_builder(ctx, name), "builder of " + name)
        first = _good(ctx, name)
        rc_, _o = _call(ctx, name, bad=True)
        assert rc_ != 0 and ENTRY_POINTS[name] in _lib.last_error(), _lib.last_error()
        assert _good(ctx, name) == first
    finally:
        ctx.lib.scape_hip_report_free(ctx.h)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(ENTRY_POINTS))
def test_free_and_reuse(name):
    """counts, builder and test, scape_hip_report_free, and the three again: the same outputs; a second free in a row
    returns 0"""
    from scape_amd import _lib
    ctx = _lib.default_context(None)
    runs = []
    try:
        for _ in range(2):
            _counts(ctx)
            _lib.check(_builder(ctx, name), "builder of " + name)
            runs.append(_good(ctx, name))
            assert ctx.lib.scape_hip_report_free(ctx.h) == 0
        assert ctx.lib.scape_hip_report_free(ctx.h) == 0
        rc_, _o = _call(ctx, name)
        assert rc_ != 0 and "report_counts" in _lib.last_error()                # nothing is left of the counts
    finally:
        ctx.lib.scape_hip_report_free(ctx.h)
    assert runs[0] == runs[1]
