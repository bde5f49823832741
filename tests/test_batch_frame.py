"""The host frame of the batch handle (scape_hip_batch_load / _build / _em / _em_fetch_lb / _labels / _free): the batch
state is freed as one and a freed handle starts over, a refused call leaves the batch as it was, and
scape_hip_batch_phase_b_form answers only for a batch that has been built.

The batch is smoke()'s: 3 UTRs of 300 reads with K <= 3, which has log-domain bins and uniform theta grids, so its build
takes Phase B form 2; "another shape" is one UTR from the same generator.  Every test works on a handle of its own.

Every refusal used here fires ahead of the first queueing.
"""
import copy
import ctypes
import functools

import numpy as np
import pytest


@functools.lru_cache(maxsize=None)
def case():
    """(preps, main sweep's packed jobs) of the batch and of the one-UTR batch"""
    from scape_amd.engine import Engine
    from scape_amd.host import prepare_utr
    from scape_amd.synth import synth_chunk
    kw = dict(n_max_apa=3, n_min_apa=1)
    out = []
    for n_utr, seed in ((3, 11), (1, 12)):
        preps = [prepare_utr(df, gene_info_str=g, **kw) for g, df in synth_chunk(n_utr, 300, k_cap=3, base_seed=seed, pa_rate=0.05)]
        out.append((preps, Engine.plan(preps, [100 + i for i in range(n_utr)])["main"]))
    return out


def _handle():
    from scape_amd import _lib
    return _lib.Context(_lib.default_context(None).device)


def _best_rows(pj, bic):
    """per UTR the job of lowest BIC (the first of them)"""
    return np.array([np.flatnonzero(pj.ju == u)[np.argmin(bic[pj.ju == u])] for u in np.unique(pj.ju)], dtype=np.int32)


def _em_and_labels(batch, pj):
    """em_packed -> em_fetch_lb and labels_packed of every UTR's best job; the defined part of every output, as bytes"""
    ao, bo, wo, bic, nlb, lb = batch.em_packed(pj, want_lb=False)
    assert lb is None
    out = [bic.tobytes(), nlb.tobytes()]
    for i, K in enumerate(pj.jk):
        out += [ao[i, :K].tobytes(), bo[i, :K].tobytes(), wo[i, :K + 1].tobytes()]
    rows = _best_rows(pj, bic)
    lbs = batch.em_fetch_lb(rows)
    out += [lbs[k, :nlb[i]].tobytes() for k, i in enumerate(rows)]
    flat = batch.labels_packed(pj.ju[rows], pj.jk[rows], ao[rows], bo[rows], wo[rows])
    assert flat.min() >= 0
    return out + [flat.tobytes()]


def _whole_run(ctx, preps, pj):
    """load -> build -> em_packed -> em_fetch_lb -> labels_packed -> fetch_tensor of UTR 0"""
    from scape_amd.engine import HipBatch
    batch = HipBatch(ctx, preps)
    batch.build()
    return batch, _em_and_labels(batch, pj) + [batch.fetch_tensor(0).tobytes()]


@pytest.mark.gpu
def test_free_and_reuse():
    """the whole run, free, the run again, the other shape, the first once more: the three runs of the first batch are
    equal to the bit, and to a fresh handle's; a freed handle refuses every batch call"""
    from scape_amd._lib import ScapeHipError
    (preps, pj), (preps1, pj1) = case()
    ctx, fresh = _handle(), _handle()
    try:
        batch, first = _whole_run(ctx, preps, pj)
        batch.free()
        rows = np.zeros(1, np.int32)
        for call, message in ((lambda: batch.em_fetch_lb(rows), "no completed scape_hip_batch_em call"),
                              (lambda: batch.em_packed(pj), "batch_build has not run"),
                              (lambda: batch.labels_packed(pj.ju[:1], pj.jk[:1], pj.a[:1], pj.b[:1], pj.w[:1]), "batch_build has not run"),
                              (lambda: batch.fetch_tensor(0), "batch_build has not run"),
                              (batch.build, "no batch loaded")):
            with pytest.raises(ScapeHipError, match=message):
                call()
        batch.free()                                                            # a second free in a row is fine
        _batch, second = _whole_run(ctx, preps, pj)
        _batch, other = _whole_run(ctx, preps1, pj1)                           # no free in between: the buffers are reused
        _batch, third = _whole_run(ctx, preps, pj)
        _batch, want = _whole_run(fresh, preps, pj)
        _batch, want_other = _whole_run(fresh, preps1, pj1)
        assert first == want and second == want and third == want
        assert other == want_other
    finally:
        ctx.close()
        fresh.close()


@pytest.mark.gpu
def test_refused_call_leaves_the_batch():
    """with the batch built and a good EM result in hand: a refused call (its message), then the good EM and labels
    calls again give the same bits; a load refused for its arrays leaves its handle unloaded"""
    from scape_amd._lib import ScapeHipError, last_error
    from scape_amd.engine import HipBatch, PackedJobs
    (preps, pj), _other = case()
    ctx, ctx2 = _handle(), _handle()
    try:
        batch, _run = _whole_run(ctx, preps, pj)
        good = _em_and_labels(batch, pj)
        n, kmax = len(pj), pj.kmax
        j = int(np.flatnonzero(pj.jk >= 1)[0])                                  # a job that has an alpha index to spoil

        def em_with(**changed):
            t = {k: getattr(pj, k).copy() for k in ("ju", "jk", "jf", "a", "b", "w", "ka")}
            for k, (at, v) in changed.items():
                t[k][at] = v
            return lambda: batch.em_packed(PackedJobs(**t))
        no_columns = PackedJobs(pj.ju, pj.jk, pj.jf, np.zeros((n, 0), np.int32), np.zeros((n, 0), np.int32), np.zeros((n, 1)), pj.ka)
        refused = ((em_with(ju=(0, len(preps))), "bad UTR index"),
                   (em_with(a=((j, 0), preps[pj.ju[j]].T)), "alpha/beta index out of range"),
                   (lambda: batch.em_packed(no_columns), "kmax out of range"),
                   (lambda: batch.labels_packed(pj.ju[:1], [kmax + 1], pj.a[:1], pj.b[:1], pj.w[:1]), "labels: K out of range"),
                   (lambda: batch.em_fetch_lb([n]), "fetch_lb: job index out of range"))
        for call, message in refused:
            with pytest.raises(ScapeHipError, match=message):
                call()
            assert _em_and_labels(batch, pj) == good, message
        # the second handle: a good load, then one whose second UTR's theta grid descends
        HipBatch(ctx2, preps)
        bad = [copy.copy(q) for q in preps]
        bad[1].theta = preps[1].theta[::-1].copy()
        with pytest.raises(ScapeHipError, match="UTR 1: all_theta must be ascending"):
            HipBatch(ctx2, bad)
        assert ctx2.lib.scape_hip_batch_build(ctx2.h) != 0 and "no batch loaded" in last_error()
        _batch, again = _whole_run(ctx2, preps, pj)                             # and the handle loads again
        assert again[:-1] == good
    finally:
        ctx.close()
        ctx2.close()


@pytest.mark.gpu
def test_phase_b_form_needs_a_build():
    """scape_hip_batch_phase_b_form on a fresh handle and on a loaded, unbuilt one is an error; after build() it is 2"""
    from scape_amd._lib import ScapeHipError, check
    from scape_amd.engine import HipBatch
    (preps, _pj), _other = case()
    ctx = _handle()
    try:
        form = ctypes.c_int32(-1)
        with pytest.raises(ScapeHipError, match="batch_build has not run"):
            check(ctx.lib.scape_hip_batch_phase_b_form(ctx.h, ctypes.byref(form)), "batch_phase_b_form")
        batch = HipBatch(ctx, preps)
        with pytest.raises(ScapeHipError, match="batch_build has not run"):
            batch.phase_b_form()
        batch.build()
        assert batch.phase_b_form() == 2
        HipBatch(ctx, preps)                                                    # loaded again: that batch has no build yet
        with pytest.raises(ScapeHipError, match="batch_build has not run"):
            batch.phase_b_form()
    finally:
        ctx.close()
