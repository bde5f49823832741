#!/usr/bin/env python3
"""Timing of `scape diff_pa_markers` (scape_amd/report.py) against the loop of `scape diff_pa --idents_1 X` commands it
replaces, on the synthetic directory of tools/diff_pa_timing.py: by default 2,000 records (K = 2..8 pA sites, about
10,000 count rows) x 20,000 cells x 9,999 permutations, 95 % of the (site, cell) counts zero, the cells cut into G = 12
equal-sized clusters (cell i in cluster i * G // cells).  In one process and session: a warm-up run of each command with
255 permutations, then --repeats times the timed `diff_pa_markers` run and the timed loop of the G `diff_pa` runs, one
per cluster against the rest, in the order of the markers file's blocks.  One JSON line holds, per repeat, both wall
times, the stage times (report.LAST_TIMES; for the loop their sums over its runs), the seconds inside the library's
mask and test calls (`calls_s`: the marker masks call against the G masks calls, the markers call against the G test
calls; a masks call is its one launch and the wait for it, a test call also compacts the kept rows), and
`blocks_equal_diff_pa`: whether every block of the markers file equals the file of the loop's run on that cluster in
every shared column but the two adjusted p-values, compared as text.  Kernel times come from a second process,

    rocprofv3 --kernel-trace --output-format csv -d P -- python tools/diff_pa_markers_timing.py --dir <made before>
    python tools/diff_pa_markers_timing.py --kernel_trace P

whose second command cuts the trace's launches into the warm-up and the repeats by their order and prints, per repeat,
the milliseconds of the marker kernels beside the sums over the loop's launches of diff_pa's kernels, and the spread of
those sums.

    python tools/diff_pa_markers_timing.py [--records N] [--cells N] [--n_perm N] [--dir D] [--groups G] [--repeats R]
"""
import argparse
import contextlib
import csv
import glob
import io
import json
import os
import re
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from diff_pa_groups_timing import make_groups  # noqa: E402
from diff_pa_timing import make_dir  # noqa: E402

# (the command's kernel, the loop's kernel that does the same work)
KERNELS = (("k_rep_perm_marker_masks", "k_rep_perm_mask_strata"), ("k_rep_perm_markers", "k_rep_perm_test"))
CALLS = {"masks": ("scape_hip_report_perm_marker_masks", "scape_hip_report_perm_masks"),
         "test": ("scape_hip_report_perm_markers", "scape_hip_report_perm_test")}


def quiet(fn, *args):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*args)


def body(path):
    with open(path, newline="") as fh:
        return list(csv.reader(fh))[1:]


class CallClock:
    """seconds spent inside some of the library's entry points, by name"""

    def __init__(self, lib, names):
        self.s = dict.fromkeys(names, 0.0)
        for name in names:
            setattr(lib, name, self._timed(name, getattr(lib, name)))

    def _timed(self, name, fn):
        def call(*a):
            t0 = time.perf_counter()
            try:
                return fn(*a)
            finally:
                self.s[name] += time.perf_counter() - t0
        return call

    def take(self):
        out, self.s = self.s, dict.fromkeys(self.s, 0.0)
        return out


def kernel_trace(root, repeats, G):
    """per repeat the ms of KERNELS in a rocprofv3 kernel trace of this script: a command's kernel has as many launches
    in the warm-up as in every repeat, the loop's kernel one run's in the warm-up and G runs' in every repeat"""
    launches = {}
    for f in sorted(glob.glob(os.path.join(root, "**", "*kernel_trace.csv"), recursive=True)):
        with open(f, newline="") as fh:
            for r in csv.DictReader(fh):
                name = re.sub(r"\s*\[clone.*", "", re.sub(r"\(.*", "", r["Kernel_Name"]).strip())
                launches.setdefault(name, []).append((int(r["Start_Timestamp"]), int(r["End_Timestamp"])))
    out = {}
    for pair in KERNELS:
        for name, runs in zip(pair, (1, G)):
            ms = [(e - s) / 1e6 for s, e in sorted(launches.get(name, []))]
            per_run, rest = divmod(len(ms), 1 + runs * repeats)
            if not ms or rest:
                raise SystemExit(f"{name}: {len(ms)} launches do not fit a warm-up and {repeats} repeats of {runs} runs")
            ms = ms[per_run:]                                        # the warm-up run
            step = per_run * runs
            out[name] = {"launches_per_repeat": step,
                         "ms": [sum(ms[k * step:(k + 1) * step]) for k in range(repeats)]}
    for ours, theirs in KERNELS:
        a, b = out[ours]["ms"], out[theirs]["ms"]
        out[f"{ours}_over_{theirs}"] = {"per_repeat": [x / y for x, y in zip(a, b)],
                                        "spread_of_the_loop_sum": (max(b) - min(b)) / min(b)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=2000)
    ap.add_argument("--cells", type=int, default=20000)
    ap.add_argument("--n_perm", type=int, default=9999)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--dir", default=None, help="directory to make the inputs in, or to reuse if it holds them")
    ap.add_argument("--groups", type=int, default=12, help="number of equal-sized clusters")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--kernel_trace", default=None,
                    help="summarise the rocprofv3 kernel trace under this directory (of a run with the same --groups and "
                         "--repeats) and do nothing else")
    a = ap.parse_args()
    G = a.groups
    if a.kernel_trace is not None:
        print(json.dumps(kernel_trace(a.kernel_trace, a.repeats, G)))
        return
    from scape_amd import _lib, report
    root = a.dir or tempfile.mkdtemp(prefix="diff_pa_markers_timing_")
    names = [f"g{g}" for g in range(G)]
    out = {"records": a.records, "cells": a.cells, "n_perm": a.n_perm, "groups": G, "repeats": []}
    try:
        if not os.path.exists(os.path.join(root, "nz.npz")):
            os.makedirs(root, exist_ok=True)
            make_dir(root, a.records, a.cells)
        z = np.load(os.path.join(root, "nz.npz"))
        clu = make_groups(root, int(z["n_cells"]), G)
        out.update(rows=int(z["rec_rows"][-1]), nonzeros=int(z["row_off"][-1]), device=_lib.default_context().name())
        quiet(report._diff_pa_markers, root, "res.gene.pkl", clu, (), 255, a.seed)
        quiet(report._diff_pa, root, "res.gene.pkl", clu, names[0], None, 255, a.seed)
        clock = CallClock(_lib.load_library(), [n for pair in CALLS.values() for n in pair])
        for _ in range(a.repeats):
            rep = {}
            t0 = time.perf_counter()
            markers_path = quiet(report._diff_pa_markers, root, "res.gene.pkl", clu, (), a.n_perm, a.seed)
            rep["diff_pa_markers"] = {"wall_s": time.perf_counter() - t0, "stages_s": dict(report.LAST_TIMES)}
            calls = clock.take()
            stages, paths = {}, []
            t0 = time.perf_counter()
            for name in names:
                paths.append(quiet(report._diff_pa, root, "res.gene.pkl", clu, name, None, a.n_perm, a.seed))
                for k, v in report.LAST_TIMES.items():
                    stages[k] = stages.get(k, 0.0) + v
            rep["diff_pa_loop"] = {"wall_s": time.perf_counter() - t0, "stages_s": stages}
            rep["loop_over_markers"] = rep["diff_pa_loop"]["wall_s"] / rep["diff_pa_markers"]["wall_s"]
            calls.update({k: v for k, v in clock.take().items() if v})
            rep["calls_s"] = {what: {"diff_pa_markers": calls[ours], "diff_pa_loop": calls[theirs]}
                              for what, (ours, theirs) in CALLS.items()}
            out["repeats"].append(rep)
        got = body(markers_path)
        out["lines"] = len(got)
        want = [r[:2] + [name] + r[2:] for name, path in zip(names, paths) for r in body(path)]
        adj = (report.DIFF_PA_MARKERS_HEADER.index("p_val_adj"), report.DIFF_PA_MARKERS_HEADER.index("gene_p_val_adj"))
        strip = lambda rows: [[v for j, v in enumerate(r) if j not in adj] for r in rows]
        out["blocks_equal_diff_pa"] = strip(got) == strip(want)
    finally:
        if a.dir is None:
            shutil.rmtree(root, ignore_errors=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
