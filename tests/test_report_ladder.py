"""The count, scan, render, segment-sum and histogram kernels of scape_amd/csrc/report.inc at their boundary shapes,
against the exact oracle of tests/report_ladder.py (Python ints, str and bytes; no tolerance appears anywhere).

Where the boundary shapes of the report kernels are tested: here.  tests/test_report*.py compare whole commands with
the reference's files on the golden directories, whose shapes are narrower than a real run's (at most 407 rows per
render block, counts up to 37 in a dense body, no column count at a tile edge, 46 bitmap words of cluster codes).

CPU: the oracle's dense text of every golden case of tests/golden/fixture_report.npz, with the oracle's OWN
pivot-complete flag, is the reference's recorded matrix body - which ties the oracle, and the completeness rule in
particular, to the reference's pandas output and not to the device; hand-worked rows and a hand-worked histogram; the
stated matrix of every case is what its reads count to; the command directory has no near tie for diff_pa.

GPU, through the C entry points by ctypes, so that a case's shape is exactly what reaches the kernel:
  families a-e, g  scape_hip_report_counts: row totals, complete flags and bad-read indices; scape_hip_report_render +
                   _fetch: bytes_out and the bytes, every row once with is_int 0 and once with 1 (alternating per row,
                   then the complement); scape_hip_report_render_mtx: bytes and nnz_out with row_no0 = 1, 9, 10 and
                   99,999, so that the row-number width changes inside a block
  family f         scape_hip_report_hist + _hist_fetch: groups per record, codes, histograms
  family g         scape_hip_report_group_sums: sums and nonzero counts per row and segment
  slots            five blocks of unequal size alternately in slots 0 and 1, each slot regrowing its pinned buffer,
                   fetched in order.  What the code states, asserted: a render into a slot that has not been fetched
                   WAITS for that slot's copy and then takes the slot over (the earlier block is gone, one fetch gives
                   the later one, a second fetch is refused); scape_hip_report_counts while a slot is pending waits for
                   the slot, which can still be fetched afterwards with the text of the earlier counts
  commands         one directory of 5 barcodes and 1,400 records of K = 2..3, no size monkeypatched: ex_pa_cnt_mat (tsv)
                   against this oracle, --format mtx against test_report_mtx._texts, ex_pa_len_mat against
                   test_report_lenmat.expected_texts, cal_exp_pa_len with a two-cluster file against an exact histogram
                   and test_report_bootlen.exp_len, diff_pa with 19 permutations against test_report_diffpa.oracle.
                   Every caller of k_rep_scan sees n > 1024 there.
Mismatches of a case are collected and reported together.

Measured on an MI355X (printed by every run; a measurement, not a target): the 42 GPU tests of the module take 3.4 s of
wall time, 2.9 s of it the five commands; family b's 2.2 M reads (36 MB of upload) are counted in 0.07 s, so the
999,999 / 1,000,000 pair stays.

What the ladder found: nothing - every case passed on the first run, no kernel changed.  That it can fail was checked
once by hand (never committed) with scratch builds of the library that differ from the source in one statement, every
device buffer of those builds padded so that a wrong offset stays inside its allocation.  Of the 42 GPU tests fail:
  `carry += tot` dropped in k_rep_scan                  31: roff[n] is the carry, so every block is "empty": all 26
                                                         count-and-render cases, the slots, and the four commands that
                                                         render or compact rows (hists and segment sums pass)
  `pos += tile` dropped in k_rep_render                 28: the row's newline lands at `pos` too, so all 26
                                                         count-and-render cases, the slots and the dense command (the
                                                         Matrix Market kernels have their own)
  `lane >= o` -> `lane > o` in rep_block_excl           41: everything but the segment sums, which do not scan
  rep_digits one digit short from 1000 on               2: "widths" and "segments" (counts of 3000)
  `code & 31` -> `code & 15` in k_rep_hist's mask       7: every histogram case with a code on bit 16 or above of a
                                                         word (codes1 and the NULL map have none)
  `n_rows += s > 0` -> `n_rows += 1` in k_rep_complete  10: "records_complete", cols1 and the row cases (complete
                                                         records with a row without reads), the slots, the dense command
"""
import ctypes
import functools
import gzip
import os
import time

import numpy as np
import pytest

import report_cases as rc
import report_ladder as rl

CASES = {c.name: c for c in rl.cases()}
HIST_CASES = {c.name: c for c in rl.hist_cases()}


def _csv_field(s):
    return ('"' + s.replace('"', '""') + '"').encode()


def _dense_body(records, col_ids):
    """the dense matrix body of a result stream by the oracle: the rows with reads of every record, in the form its
    own pivot-complete flag gives"""
    out = []
    for rec, m in zip(records, rc.dense_counts(records, col_ids)):
        rows = m.tolist()
        flag = rl.complete(rows)
        out += [rl.dense_row(_csv_field(rc.pa_info(rec, lb)), row, flag) for lb, row in enumerate(rows) if any(row)]
    return b"".join(out)


# ---------------------------------------------------------------- CPU
@pytest.mark.parametrize("c", rc.case_params())
def test_oracle_dense_text_is_the_reference_body(c):
    cs = rc.fixture_case(c)
    col_ids = rc.column_ids(rc.text(rc.fixture(), cs["barcode"]))
    assert _dense_body(cs["records"], col_ids) == cs["mat_body"].encode(), cs["name"]


def test_golden_cases_hold_both_forms():
    """the pin above sees complete and incomplete records, so it can tell the two rules apart"""
    flags = set()
    for cs in rc.fixture_cases():
        col_ids = rc.column_ids(rc.text(rc.fixture(), cs["barcode"]))
        flags |= {rl.complete(m.tolist()) for m in rc.dense_counts(cs["records"], col_ids) if m.any()}
    assert flags == {True, False}


def test_hand_worked_rows():
    assert rl.dense_row(b'"p"', [0, 7, 12, 0], True) == b'"p","0.0","7","12","0.0"\n'
    assert rl.dense_row(b'"p"', [0, 7, 12, 0], False) == b'"p","0.0","7.0","12.0","0.0"\n'
    assert rl.dense_row(b"", [0], True) == b',"0.0"\n' and rl.dense_row(b"x", [1000], False) == b'x,"1000.0"\n'
    assert len(rl.field(0, True)) == len(rl.field(0, False)) == rl.ZERO_FIELD
    assert rl.mtx_row(10, [0, 3, 0, 120]) == b"10 2 3\n10 4 120\n" and rl.mtx_row(1, [0, 0]) == b""
    assert rl.row_total([0, 3, 0, 120]) == 123
    assert rl.seg_sums([9, 1, 0, 2, 5, 9], [1, 1, 4, 5]) == ([0, 3, 5], [0, 2, 1])
    # complete: columns 0 and 2 have reads, in both rows with reads; the empty row is no row of the pivot
    assert rl.complete([[1, 0, 2], [0, 0, 0], [3, 0, 1]]) and rl.complete([[0, 0]]) and rl.complete([[0, 4]])
    assert not rl.complete([[1, 0, 2], [3, 0, 0]]) and not rl.complete([[1, 0], [0, 1]])


def test_hand_worked_histogram():
    # K = 2: codes 5 and 2 present; label 2 and 7 share slot K; code 9 has a read of no site only
    present, hist = rl.histogram(2, [0, 1, 1, 2, 7, 0, 3], [5, 5, 2, 2, 2, 5, 9])
    assert present == [2, 5, 9] and hist == [[0, 1, 2], [2, 1, 0], [0, 0, 1]]
    assert rl.histogram(1, [], []) == ([], [])


def test_cases_state_what_their_reads_count_to():
    """the generator: np.add.at over every case's reads (label < K, known cell) is the stated matrix; the families hold
    what their notes say"""
    for c in rl.cases():
        K, off, lab, cb, id_min, table = c.reads
        got = np.zeros((sum(c.Ks), c.n_cols), dtype=np.int64)
        base = np.concatenate([[0], np.cumsum(c.Ks)])
        for r in range(len(c.Ks)):
            l, i = lab[off[r]:off[r + 1]], cb[off[r]:off[r + 1]]
            d = i - id_min
            ok = (l >= 0) & (l < c.Ks[r]) & (d >= 0) & (d < len(table))
            col = table[np.where(ok, d, 0)]
            ok &= col >= 0
            np.add.at(got, (base[r] + l[ok], col[ok]), 1)
        assert got.tolist() == c.counts, c.name
        assert c.note and id_min == c.ids.min()
        if c.want_complete is not None:
            assert c.complete == c.want_complete, c.name
    by = CASES
    for n in rl.COLS:
        c = by[f"cols{n}"]
        m = np.array(c.counts)
        assert c.Ks == [1, 3, 5] and 0.3 < (m > 0).mean() < 0.5 or n == 1
        assert all((m[:, e] > 0).any() for e in (0, 63, 64, 255, 256, n - 1) if e < n)
        assert m[-1, -1] > 0 and not m[-1, :-1].any()
    w = by["widths"]
    assert sorted(v for v in w.counts[0] if v) == sorted(rl.WIDTH_COUNTS) and max(w.counts[1]) < 10
    assert all(w.counts[0][e] >= 10 for e in (0, 63, 64, 255, 256, 257)) and w.n_cols == 258 and w.Ks == [2]
    for n in rl.ROWS:
        c = by[f"rows{n}"]
        assert len(c.rows) == n and c.n_cols == 3 and set(c.Ks) <= {1, 2, 3}
        assert len({len(c.dense_text([0] * n, i, i + 1)) for i in range(min(n, 8))}) > 1 or n == 1
    p = by[f"rows{rl.ROWS[-1]}_permuted"]
    assert len(p.rows) == rl.ROWS[-1] and len(set(p.rows)) == rl.ROWS[-1] - 1 and p.rows != sorted(p.rows)
    assert by["prefixes"].pre_len == list(rl.PREFIX_LENGTHS)
    assert by["records_K"].Ks[:4] == list(rl.RECORD_KS) and by["records_K"].row_tot[-5:] == [0] * 5
    assert by["records_complete"].complete == [1, 0, 0, 1, 1]
    assert by["unknown_id_no_site"].bad == [-1, -1]
    assert by["unknown_id_site"].bad[0] >= 0 and by["unknown_id_site"].bad[1] == -1
    assert by["negative_label"].bad[0] == -1 and by["negative_label"].bad[1] >= 0
    assert min(by["unknown_and_negative"].bad) >= 0
    s = by["segments"]
    assert [len(o) - 1 for o in s.segs] == [1, 3, 4, 5, 9] and sorted(s.rows) == list(range(9)) and s.rows != sorted(s.rows)
    assert all(o[0] == rl.SEG_FIRST > 0 and o[-1] < s.n_cols for o in s.segs)
    assert {b - a for o in s.segs for a, b in zip(o[:-1], o[1:])} == {0, 1, 63, 64, 65, 300}
    for h in rl.hist_cases():
        n_groups, codes, hist = h.expected
        assert len(codes) == sum(n_groups) and sum(hist) == len(h.reads[2]), h.name
        if h.n_codes:
            assert n_groups[3] == n_groups[7] == 0 and codes[:n_groups[0]] == sorted({0, h.n_codes - 1}), h.name
            assert codes[n_groups[0]:n_groups[0] + n_groups[1]] == [c for c in range(h.n_codes) if c % 32 in (0, 31)]


@functools.lru_cache(maxsize=None)
def _command_case():
    records, bc, clu = rl.command_records()
    col_ids = rc.column_ids(bc)
    rec_rows = rc.rec_rows_of(records, col_ids)
    return dict(records=records, bc=bc, clu=clu, col_ids=col_ids, rec_rows=rec_rows)


def test_command_directory_shape_and_no_near_tie():
    """more than 2,048 matrix rows, more than 1,024 records with two kept rows, and - on the oracle alone, as
    tests/test_report_diffpa.py demands - no permutation within 2^-39 of an observed statistic"""
    import test_report_diffpa as td
    s = _command_case()
    assert sum(len(rows) for _g, rows in s["rec_rows"]) > 2 * rl.SCAN
    c1, c2 = rc.populations(s["bc"], s["clu"], "A", "B")
    assert (len(c1), len(c2)) == (2, 3)
    lines = td.oracle(s["rec_rows"], c1, c2, 19, 1)
    td.assert_no_near_tie(lines, "ladder directory")
    assert sum(ln["first"] for ln in lines) > rl.SCAN and len(lines) > 2 * rl.SCAN
    assert {rl.complete(m.tolist()) for m in rc.dense_counts(s["records"], s["col_ids"])} == {True, False}


# ---------------------------------------------------------------- GPU: the entry points
_T = {}


@pytest.fixture(scope="module")
def dev():
    from scape_amd import _lib
    ctx = _lib.default_context(None)
    t0 = time.perf_counter()
    try:
        yield ctx
    finally:
        ctx.lib.scape_hip_report_free(ctx.h)
        print(f"\n[report ladder] GPU tests of the module: {time.perf_counter() - t0:.2f} s wall; "
              + ", ".join(f"{k} {v:.2f} s" for k, v in _T.items()))


def _diff(got, want):
    """where two byte strings part, with both sides' bytes around it"""
    if got == want:
        return None
    n = min(len(got), len(want))
    at = next((i for i in range(n) if got[i] != want[i]), n)
    line = want.count(b"\n", 0, at)
    return (f"lengths {len(got)} / {len(want)}, first difference at byte {at} (after {line} newlines of the expected "
            f"text): got {got[max(0, at - 12):at + 12]!r}, expected {want[max(0, at - 12):at + 12]!r}")


def _counts(ctx, case):
    from scape_amd._lib import P_i8, P_i32, P_i64, check, ptr
    K, off, lab, cb, id_min, table = case.reads
    row_tot, flags, bad = np.full(int(K.sum()), -1, np.int64), np.full(len(K), -1, np.int8), np.full(2, -5, np.int64)
    check(ctx.lib.scape_hip_report_counts(ctx.h, len(K), ptr(off, P_i64), ptr(K, P_i32), ptr(lab, P_i64), ptr(cb, P_i64),
                                          id_min, len(table), ptr(table, P_i32), case.n_cols, ptr(row_tot, P_i64),
                                          ptr(flags, P_i8), ptr(bad, P_i64)), "report_counts")
    return row_tot.tolist(), flags.tolist(), bad.tolist()


def _render(ctx, slot, rows, is_int, prefixes):
    from scape_amd._lib import P_i8, P_i64, ptr
    rows, is_int = np.asarray(rows, dtype=np.int64), np.asarray(is_int, dtype=np.int8)
    poff = np.zeros(len(rows) + 1, dtype=np.int64)
    np.cumsum([len(p) for p in prefixes], out=poff[1:])
    nbytes = ctypes.c_int64(-1)
    rcode = ctx.lib.scape_hip_report_render(ctx.h, slot, len(rows), ptr(rows, P_i64), ptr(is_int, P_i8), ptr(poff, P_i64),
                                            b"".join(prefixes), ctypes.byref(nbytes))
    return rcode, nbytes.value


def _render_mtx(ctx, slot, rows, row_no0):
    from scape_amd._lib import P_i64, ptr
    rows = np.asarray(rows, dtype=np.int64)
    nbytes, nnz = ctypes.c_int64(-1), ctypes.c_int64(-1)
    rcode = ctx.lib.scape_hip_report_render_mtx(ctx.h, slot, len(rows), ptr(rows, P_i64), row_no0, ctypes.byref(nbytes),
                                                ctypes.byref(nnz))
    return rcode, nbytes.value, nnz.value


def _fetch(ctx, slot):
    hp, nb = ctypes.c_void_p(), ctypes.c_int64(-1)
    rcode = ctx.lib.scape_hip_report_fetch(ctx.h, slot, ctypes.byref(hp), ctypes.byref(nb))
    return rcode, (ctypes.string_at(hp.value, nb.value) if rcode == 0 and nb.value > 0 else b"")


def _check_counts(ctx, case, problems):
    t0 = time.perf_counter()
    tot, flags, bad = _counts(ctx, case)
    _T[f"counts of {case.name}"] = time.perf_counter() - t0
    if tot != case.row_tot:
        wrong = [i for i, (a, b) in enumerate(zip(tot, case.row_tot)) if a != b]
        problems.append((case.name, "row totals", len(wrong), "rows differ, first", wrong[0], tot[wrong[0]], case.row_tot[wrong[0]]))
    if flags != case.complete:
        problems.append((case.name, "complete flags", flags, case.complete))
    if bad != case.bad:
        problems.append((case.name, "bad reads", bad, case.bad))


@pytest.mark.gpu
@pytest.mark.parametrize("name", [c.name for c in rl.cases()])
def test_counts_and_render(name, dev):
    case, problems = CASES[name], []
    _check_counts(dev, case, problems)
    n, pre = len(case.rows), case.prefixes()
    for flip in (0, 1):
        is_int = [(i + flip) % 2 for i in range(n)]
        want = case.dense_text(is_int)
        rcode, nbytes = _render(dev, flip, case.rows, is_int, pre)
        frc, got = _fetch(dev, flip)
        if rcode or frc or nbytes != len(want):
            problems.append((name, "render", flip, "return codes", rcode, frc, "bytes_out", nbytes, len(want)))
        d = _diff(got, want)
        if d:
            problems.append((name, "dense text, is_int = (row + %d) %% 2" % flip, d))
    for row_no0 in rl.ROW_NO0:
        want, want_nnz = case.mtx_text(row_no0)
        rcode, nbytes, nnz = _render_mtx(dev, row_no0 % 2, case.rows, row_no0)
        frc, got = _fetch(dev, row_no0 % 2)
        if rcode or frc or nbytes != len(want) or nnz != want_nnz:
            problems.append((name, "render_mtx", row_no0, "return codes", rcode, frc, "bytes_out", nbytes, len(want),
                             "nnz_out", nnz, want_nnz))
        d = _diff(got, want)
        if d:
            problems.append((name, f"Matrix Market text, row_no0 = {row_no0}", d))
    assert not problems, f"{len(problems)} mismatches\n" + "\n".join(repr(p) for p in problems[:40])


@pytest.mark.gpu
def test_segment_sums(dev):
    from scape_amd._lib import P_i32, P_i64, check, ptr
    case, problems = CASES["segments"], []
    _check_counts(dev, case, problems)
    rows = np.asarray(case.rows, dtype=np.int64)
    for seg_off in case.segs:
        n_seg = len(seg_off) - 1
        off = np.asarray(seg_off, dtype=np.int32)
        sums, nz = np.full((len(rows), n_seg), -1, np.int32), np.full((len(rows), n_seg), -1, np.int32)
        check(dev.lib.scape_hip_report_group_sums(dev.h, n_seg, ptr(off, P_i32), len(rows), ptr(rows, P_i64),
                                                  ptr(sums, P_i32), ptr(nz, P_i32)), "report_group_sums")
        want = [rl.seg_sums(case.counts[r], seg_off) for r in case.rows]
        if sums.tolist() != [w[0] for w in want]:
            problems.append((n_seg, "sums", sums.tolist(), [w[0] for w in want]))
        if nz.tolist() != [w[1] for w in want]:
            problems.append((n_seg, "nonzero counts", nz.tolist(), [w[1] for w in want]))
    assert not problems, f"{len(problems)} mismatches\n" + "\n".join(repr(p) for p in problems[:40])


@pytest.mark.gpu
@pytest.mark.parametrize("name", [c.name for c in rl.hist_cases()])
def test_histograms(name, dev):
    from scape_amd._lib import P_i32, P_i64, check, ptr
    case, problems = HIST_CASES[name], []
    K, off, lab, cb, id_min, table = case.reads
    want_groups, want_codes, want_hist = case.expected
    n_groups, bad = np.full(len(K), -1, np.int64), np.full(2, -5, np.int64)
    check(dev.lib.scape_hip_report_hist(dev.h, len(K), ptr(off, P_i64), ptr(K, P_i32), ptr(lab, P_i64), ptr(cb, P_i64),
                                        id_min, len(table) if table is not None else 0,
                                        ptr(table, P_i32) if table is not None else None, case.n_codes or 1,
                                        ptr(n_groups, P_i64), ptr(bad, P_i64)), "report_hist")
    assert bad.tolist() == [-1, -1], (name, bad)
    if n_groups.tolist() != want_groups:
        problems.append((name, "groups per record", n_groups.tolist(), want_groups))
    G, H = int(n_groups.sum()), int(np.sum(n_groups * (K.astype(np.int64) + 1)))
    codes, hist = np.full(max(G, 1), -1, np.int32), np.full(max(H, 1), -1, np.int32)
    check(dev.lib.scape_hip_report_hist_fetch(dev.h, G, ptr(codes, P_i32), H, ptr(hist, P_i32)), "report_hist_fetch")
    codes, hist = codes[:G].tolist(), hist[:H].tolist()
    if codes != want_codes:
        wrong = [i for i, (a, b) in enumerate(zip(codes, want_codes)) if a != b]
        problems.append((name, "codes", len(codes), len(want_codes), "first difference", wrong[:1],
                         [(codes[i], want_codes[i]) for i in wrong[:5]]))
    if hist != want_hist:
        wrong = [i for i, (a, b) in enumerate(zip(hist, want_hist)) if a != b]
        problems.append((name, "histogram", len(hist), len(want_hist), "differing slots", len(wrong), wrong[:5],
                         [(hist[i], want_hist[i]) for i in wrong[:5]]))
    assert not problems, f"{len(problems)} mismatches\n" + "\n".join(repr(p) for p in problems[:40])


@pytest.mark.gpu
def test_slots(dev):
    from scape_amd import _lib
    case, other = CASES[f"rows{rl.ROWS[-1]}"], CASES["cols65"]
    problems = []
    dev.lib.scape_hip_report_free(dev.h)            # fresh slots: every growth of a pinned buffer happens below
    _check_counts(dev, case, problems)
    n, pre = len(case.rows), case.prefixes()
    is_int = [i % 2 for i in range(n)]
    cuts = [0, 5, 40, 300, 1100, n]
    blocks = list(zip(cuts[:-1], cuts[1:]))
    assert [b - a for a, b in blocks[0::2]] == sorted(b - a for a, b in blocks[0::2])     # each slot's blocks grow
    assert [b - a for a, b in blocks[1::2]] == sorted(b - a for a, b in blocks[1::2])

    def render(slot, blk):
        a, b = blocks[blk]
        rcode, nbytes = _render(dev, slot, case.rows[a:b], is_int[a:b], pre[a:b])
        assert rcode == 0 and nbytes == len(case.dense_text(is_int, a, b)), (blk, rcode, nbytes, _lib.last_error())

    def fetched(slot, blk, what):
        frc, got = _fetch(dev, slot)
        d = _diff(got, case.dense_text(is_int, *blocks[blk]))
        if frc or d:
            problems.append((what, "slot", slot, "block", blk, frc, d))

    assert _fetch(dev, 0)[0] != 0 and "nothing rendered" in _lib.last_error()
    for blk in range(len(blocks)):                # block n is rendered behind block n - 1, which is then fetched
        render(blk % 2, blk)
        if blk:
            fetched((blk - 1) % 2, blk - 1, "in order")
    fetched((len(blocks) - 1) % 2, len(blocks) - 1, "in order")
    assert _fetch(dev, 0)[0] != 0 and _fetch(dev, 1)[0] != 0
    # a second render into a slot that has not been fetched waits for the slot and takes it over
    render(0, 1)
    render(0, 2)
    fetched(0, 2, "second render into an unfetched slot")
    assert _fetch(dev, 0)[0] != 0 and "nothing rendered" in _lib.last_error()
    # counts while a slot is pending: the slot is finished first and can still be fetched
    render(1, 3)
    _check_counts(dev, other, problems)
    fetched(1, 3, "fetched after the next counts call")
    rcode, nbytes = _render(dev, 0, other.rows, [1] * len(other.rows), other.prefixes())
    frc, got = _fetch(dev, 0)
    d = _diff(got, other.dense_text([1] * len(other.rows)))
    if rcode or frc or d:
        problems.append(("render of the next counts", rcode, frc, d))
    assert not problems, f"{len(problems)} mismatches\n" + "\n".join(repr(p) for p in problems[:40])


# ---------------------------------------------------------------- GPU: the commands, production block sizes
@pytest.fixture(scope="module")
def ladder_dir(tmp_path_factory):
    from scape.apa_core import Parameters
    s = _command_case()
    root = tmp_path_factory.mktemp("report_ladder")
    clu_path = rc.write_dir(str(root), "res.gene.pkl", s["records"], s["bc"], {"ladder_groups.csv": s["clu"]}, Parameters)[0]
    return root, clu_path


def _scan_sizes(monkeypatch, name, arg=2):
    """the n_rows / n_rec argument (argument number `arg`) of every call of an entry point during the test"""
    from scape_amd import _lib
    lib, seen = _lib.load_library(), []
    real = getattr(lib, name)
    monkeypatch.setattr(lib, name, lambda *a: (seen.append(a[arg]), real(*a))[1])
    return seen


@pytest.mark.gpu
def test_command_dense_matrix(ladder_dir, monkeypatch):
    from scape_amd import report
    root, _clu = ladder_dir
    s = _command_case()
    assert report.MAX_BATCH_BYTES is None and report.MAX_BLOCK_BYTES == 256 << 20
    seen = _scan_sizes(monkeypatch, "scape_hip_report_render")
    r = rc.run(["ex_pa_cnt_mat", "--output_dir", str(root), "--res_pkl_file", "res.gene.pkl"])
    assert r.exit_code == 0, (r.output, repr(r.exception))
    with gzip.open(os.path.join(str(root), "res.gene.cnt.tsv.gz"), "rb") as fh:
        got = fh.read()
    want = rc.header_line(s["bc"]).encode() + _dense_body(s["records"], s["col_ids"])
    assert max(seen) > 2 * rl.SCAN
    assert _diff(got, want) is None, _diff(got, want)


@pytest.mark.gpu
def test_command_matrix_market(ladder_dir, monkeypatch):
    import test_report_mtx as tm
    root, _clu = ladder_dir
    s = _command_case()
    seen = _scan_sizes(monkeypatch, "scape_hip_report_render_mtx")
    r = rc.run(["ex_pa_cnt_mat", "--output_dir", str(root), "--res_pkl_file", "res.gene.pkl", "--format", "mtx"])
    assert r.exit_code == 0, (r.output, repr(r.exception))
    rows = [row for _g, rec_rows in s["rec_rows"] for row in rec_rows]
    dense = np.array([m for _pa, m in rows], dtype=np.int64).reshape(len(rows), len(s["col_ids"]))
    want = tm._texts([pa for pa, _m in rows], dense, tm._barcodes(s["bc"]))
    got = tm._read_dir(root)
    assert max(seen) > 2 * rl.SCAN
    for name in tm.FILES:
        assert got[name] == want[name], (name, _diff(got[name].encode(), want[name].encode()))


@pytest.mark.gpu
def test_command_length_matrix(ladder_dir, monkeypatch):
    import test_report_lenmat as tl
    root, _clu = ladder_dir
    s = _command_case()
    seen = _scan_sizes(monkeypatch, "scape_hip_report_render_len_mtx")
    r = rc.run(["ex_pa_len_mat", "--output_dir", str(root), "--res_pkl_file", "res.gene.pkl"])
    assert r.exit_code == 0, (r.output, repr(r.exception))
    want, got = tl.expected_texts(s["records"], s["bc"]), tl._read_dir(root)
    assert max(seen) > rl.SCAN
    for name in tl.FILES:
        assert got[name] == want[name], (name, _diff(got[name].encode(), want[name].encode()))


@pytest.mark.gpu
def test_command_expected_length(ladder_dir):
    """cal_exp_pa_len with the two-cluster file: per record the clusters among its reads (label >= K included) in
    np.unique's order, exp_pa_len of the cluster's exact label histogram"""
    import pandas as pd
    import test_report_bootlen as bl
    root, clu_path = ladder_dir
    s = _command_case()
    r = rc.run(["cal_exp_pa_len", "--output_dir", str(root), "--cell_cluster_file", clu_path, "--res_pkl_file", "res.gene.pkl"])
    assert r.exit_code == 0, (r.output, repr(r.exception))
    clu_of = dict(rc.cluster_rows(s["clu"]))
    lines = []
    for rec in s["records"]:
        _chrom, gene, utr, _st_en, _strand = rec["gene_info_str"].split(":")
        K, lab = int(rec["K"]), rec["label_arr"].tolist()
        names = [clu_of[int(i)] for i in rec["cb_id_arr"].tolist()]
        for name in sorted(set(names)):
            cnt = np.array([sum(1 for l, x in zip(lab, names) if x == name and l == k) for k in range(K)], dtype=np.int64)
            lines.append([gene + ":" + utr, name, bl.exp_len(np.asarray(rec["alpha_arr"]), cnt), K])
    want = pd.DataFrame(lines, columns=["gene_id", "cell_cluster", "exp_length", "num_pa"]).to_csv(header=True, index=False)
    with open(os.path.join(str(root), "ladder_groups.gene.pa.len.csv")) as fh:
        got = fh.read()
    assert len(lines) > 2 * rl.SCAN and any(ln[2] != ln[2] for ln in lines)          # a cluster with reads of no site: nan
    assert _diff(got.encode(), want.encode()) is None, _diff(got.encode(), want.encode())


@pytest.mark.gpu
def test_command_diff_pa(ladder_dir, monkeypatch):
    import test_report_diffpa as td
    root, clu_path = ladder_dir
    s = _command_case()
    seen = _scan_sizes(monkeypatch, "scape_hip_report_group_sums", 3)
    _text, lines = td.check(root, clu_path, s["clu"], "res.gene.pkl", s["rec_rows"], s["bc"], "A", "B", 19, 1, "ladder directory")
    assert len(lines) > 2 * rl.SCAN and sum(ln["first"] for ln in lines) > rl.SCAN
    assert max(seen) > 2 * rl.SCAN                            # the kept rows that rep_perm_prepare scans
