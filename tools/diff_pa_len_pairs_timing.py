#!/usr/bin/env python3
"""Timing of `scape diff_pa_len_pairs` (scape_amd/report.py) against the loop of `scape diff_pa_len` commands it
replaces, and with --markers of `scape diff_pa_len_markers` against the loop of `scape diff_pa_len --idents_1 X`, on the
synthetic directory of tools/diff_pa_timing.py: by default 2,000 records (K = 2..8 pA sites, about 10,000 count rows) x
20,000 cells x 9,999 permutations, 95 % of the (site, cell) counts zero, the cells cut into G = 12 equal-sized clusters
(cell i in cluster i * G // cells).  In one process and session: a warm-up run of each command with 255 permutations,
then the timed one-run command and the timed loop of the G (G - 1) / 2 (or G) `diff_pa_len` runs, one per block in the
order of the one-run file's blocks.  One JSON line holds both wall times, the stage times (report.LAST_TIMES; for the
loop their sums over its runs) and `blocks_equal_diff_pa_len`: whether every block of the one-run file equals the file
of the loop's run on that pair or marker in every shared column but p_val_adj, compared as text.  Kernel times come from
a second process, each step under a time limit of its own:

    timeout -k 10 900 python tools/diff_pa_len_pairs_timing.py --dir D [--markers]
    timeout -k 10 900 rocprofv3 --kernel-trace --stats --output-format csv -d P -- \\
        python tools/diff_pa_len_pairs_timing.py --dir D [--markers]
    python tools/diff_pa_len_pairs_timing.py --kernel_trace P [--markers]

whose last command cuts the trace's launches into the warm-up and the timed runs by their order and prints the
milliseconds of every kernel of the timed one-run command beside the sums over the loop's launches.

    python tools/diff_pa_len_pairs_timing.py [--records N] [--cells N] [--n_perm N] [--dir D] [--groups G] [--markers]
"""
import argparse
import csv
import glob
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
from diff_pa_pairs_timing import body, quiet  # noqa: E402
from diff_pa_timing import make_dir  # noqa: E402

# the kernels only the one-run command launches, and those only the loop launches
OURS = {False: ("k_rep_perm_pair_masks", "k_rep_perm_len_pairs", "k_rep_pair_segidx", "k_rep_groups_rowstat"),
        True: ("k_rep_perm_marker_masks", "k_rep_perm_len_markers", "k_rep_groups_rowstat")}
THEIRS = ("k_rep_perm_mask_strata", "k_rep_perm_len", "k_rep_perm_rowstat")
SHARED = ("k_rep_perm_fill", "k_rep_scan", "k_rep_segsum", "k_rep_count", "k_rep_complete")


def kernel_trace(root, runs, markers):
    """the ms and launches of the timed one-run command and of the timed loop of `runs` runs in a rocprofv3 kernel trace
    of this script: the one-run command's own kernels have as many launches in its warm-up as in its timed run, the
    loop's own kernels one run's in the warm-up and `runs` runs' when timed, and a shared kernel follows the order
    warm-up of ours, warm-up of theirs, ours, the loop"""
    launches = {}
    for f in sorted(glob.glob(os.path.join(root, "**", "*kernel_trace.csv"), recursive=True)):
        with open(f, newline="") as fh:
            for r in csv.DictReader(fh):
                name = re.sub(r"\s*\[clone.*", "", re.sub(r"\(.*", "", r["Kernel_Name"]).strip())
                launches.setdefault(name, []).append((int(r["Start_Timestamp"]), int(r["End_Timestamp"])))
    ms = {name: [(e - s) / 1e6 for s, e in sorted(v)] for name, v in launches.items()}

    def part(name, v):
        return {"ms": sum(v), "launches": len(v), "each_ms": [min(v), max(v)] if v else []}
    out = {"one_run": {}, "loop": {}}
    for name in OURS[markers]:
        v = ms.get(name, [])
        if not v or len(v) % 2:
            raise SystemExit(f"{name}: {len(v)} launches do not fit a warm-up and a timed run")
        out["one_run"][name] = part(name, v[len(v) // 2:])
    for name in THEIRS:
        v = ms.get(name, [])
        per_run, rest = divmod(len(v), 1 + runs)
        if not v or rest:
            raise SystemExit(f"{name}: {len(v)} launches do not fit a warm-up and {runs} runs")
        out["loop"][name] = part(name, v[per_run:])
    for name in SHARED:
        v = ms.get(name, [])
        per_run, rest = divmod(len(v), 3 + runs)
        if not v or rest:
            raise SystemExit(f"{name}: {len(v)} launches do not fit two warm-ups, a timed run and {runs} runs")
        out["one_run"][name] = part(name, v[2 * per_run:3 * per_run])
        out["loop"][name] = part(name, v[3 * per_run:])
    ours = "k_rep_perm_len_markers" if markers else "k_rep_perm_len_pairs"
    out[f"{ours}_over_k_rep_perm_len"] = out["one_run"][ours]["ms"] / out["loop"]["k_rep_perm_len"]["ms"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=2000)
    ap.add_argument("--cells", type=int, default=20000)
    ap.add_argument("--n_perm", type=int, default=9999)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--dir", default=None, help="directory to make the inputs in, or to reuse if it holds them")
    ap.add_argument("--groups", type=int, default=12, help="number of equal-sized clusters")
    ap.add_argument("--markers", action="store_true",
                    help="time diff_pa_len_markers against the loop of the G `diff_pa_len --idents_1 X` runs")
    ap.add_argument("--kernel_trace", default=None,
                    help="summarise the rocprofv3 kernel trace under this directory (of a run with the same --groups and "
                         "--markers) and do nothing else")
    a = ap.parse_args()
    G = a.groups
    if a.markers:
        items = [((f"g{g}",), f"g{g}", None) for g in range(G)]
    else:
        items = [((f"g{g}", f"g{h}"), f"g{g}", f"g{h}") for g in range(G) for h in range(g + 1, G)]
    if a.kernel_trace is not None:
        print(json.dumps(kernel_trace(a.kernel_trace, len(items), a.markers)))
        return
    from scape_amd import _lib, report
    one_run = report._diff_pa_len_markers if a.markers else report._diff_pa_len_pairs
    ours, theirs = ("diff_pa_len_markers" if a.markers else "diff_pa_len_pairs"), "diff_pa_len_loop"
    root = a.dir or tempfile.mkdtemp(prefix="diff_pa_len_pairs_timing_")
    out = {"records": a.records, "cells": a.cells, "n_perm": a.n_perm, "groups": G, "blocks": len(items)}
    try:
        if not os.path.exists(os.path.join(root, "nz.npz")):
            os.makedirs(root, exist_ok=True)
            make_dir(root, a.records, a.cells)
        z = np.load(os.path.join(root, "nz.npz"))
        clu = make_groups(root, int(z["n_cells"]), G)
        out.update(rows=int(z["rec_rows"][-1]), nonzeros=int(z["row_off"][-1]), device=_lib.default_context().name())
        quiet(one_run, root, "res.gene.pkl", clu, (), 255, a.seed)
        quiet(report._diff_pa_len, root, "res.gene.pkl", clu, *items[0][1:], 255, a.seed)

        t0 = time.perf_counter()
        one_path = quiet(one_run, root, "res.gene.pkl", clu, (), a.n_perm, a.seed)
        out[ours] = {"wall_s": time.perf_counter() - t0, "stages_s": dict(report.LAST_TIMES)}

        stages, paths = {}, []
        t0 = time.perf_counter()
        for _groups, id1, id2 in items:
            paths.append(quiet(report._diff_pa_len, root, "res.gene.pkl", clu, id1, id2, a.n_perm, a.seed))
            for k, v in report.LAST_TIMES.items():
                stages[k] = stages.get(k, 0.0) + v
        out[theirs] = {"wall_s": time.perf_counter() - t0, "stages_s": stages}
        out["loop_over_one_run"] = out[theirs]["wall_s"] / out[ours]["wall_s"]

        got = body(one_path)
        out[ours]["lines"] = len(got)
        want = [r[:1] + list(groups) + r[1:] for (groups, _id1, _id2), path in zip(items, paths) for r in body(path)]
        header = report.DIFF_PA_LEN_MARKERS_HEADER if a.markers else report.DIFF_PA_LEN_PAIRS_HEADER
        adj = header.index("p_val_adj")
        strip = lambda rows: [r[:adj] + r[adj + 1:] for r in rows]
        out["blocks_equal_diff_pa_len"] = strip(got) == strip(want)
        out["wall_gate_passed"] = out[ours]["wall_s"] < out[theirs]["wall_s"]
    finally:
        if a.dir is None:
            shutil.rmtree(root, ignore_errors=True)
    print(json.dumps(out))
    if not (out.get("blocks_equal_diff_pa_len") and out.get("wall_gate_passed")):
        raise SystemExit("the one-run file differs from the loop's files, or took longer than the loop")


if __name__ == "__main__":
    main()
