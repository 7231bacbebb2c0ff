#!/usr/bin/env python3
"""nemo_lineage_repair_sets beside nemo_lineage_cuts on the C3-shaped graph (run 0's post graph of a 12-run corpus): for
several absent sets (the first n sink goals of a fixed shuffle, every one a candidate) and max_size, the sets each level
evaluates, the wall time of the blocking call (median of --steps after --warmup) and, from a second set of calls with
event timing on, the time of the groups and of the persistent kernels (nemo_timings), from which the time per chunk of
64 sets follows: k_lrep_lds over its chunks (the status launch counts as one) and k_lin_lds over its own, the same list
as candidates on the same graph.  The two searches' frontiers differ, so the chunk counts are printed beside the times.
One JSON line per (absent sinks, max_size).

  python tools/lineage_repair_bench.py --steps 5 --warmup 1 --absent 16,64,256 --sizes 2,3,4
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from nemo_amd import engine as E  # noqa: E402
from tools import synth  # noqa: E402

GROUPS = ["k_lrepair", "k_lrep_lds", "k_lrep_glob", "k_lineage", "k_lin_lds", "k_lin_glob", "k_lin_filter", "k_lin_rehash"]


def timed(eng, call, steps, warmup):
    for _ in range(warmup):
        call()
    wall = []
    for _ in range(steps):
        t0 = time.perf_counter()
        call()
        wall.append(1e3 * (time.perf_counter() - t0))
    eng.set_timing(True)
    eng.set_timing_groups(GROUPS)
    eng.reset_timings()
    for _ in range(steps):
        call()
    eng.synchronize()
    t = eng.timings()
    eng.set_timing(False)
    out = {"wall_ms": round(statistics.median(wall), 4), "wall_ms_min_max": [round(min(wall), 4), round(max(wall), 4)]}
    for g in GROUPS:
        if g in t and t[g]["launches"]:
            out[g] = round(t[g]["ms"] / steps, 4)
            out[g + "_launches"] = t[g]["launches"] // steps
    return out


def chunks(levels):
    return int(sum((int(n) + 63) // 64 for n in levels))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--absent", default="16,64,256")
    ap.add_argument("--sizes", default="2,3,4")
    ap.add_argument("--lds", type=int, default=-1, help="option wit_lds_max (-1: the default, 0: the global tier)")
    ap.add_argument("--grid", type=int, default=0, help="option kl_grid (1: one workgroup walks every chunk of a level)")
    a = ap.parse_args()
    corpus, _ = synth.generate(12, p_fault=0.55, prepend_run0=True, **synth.CONFIGS["c3"])
    it = int(corpus.iteration[0])
    g = 2 * corpus.run_index(it) + 1
    n0, n1 = int(corpus.node_off[g]), int(corpus.node_off[g + 1])
    e0, e1 = int(corpus.edge_off[g]), int(corpus.edge_off[g + 1])
    has_child = np.zeros(n1 - n0, bool)
    has_child[corpus.edge_src[e0:e1]] = True
    rule = (corpus.node_word[n0:n1] & np.uint32(0x80000000)) != 0
    sinks = np.flatnonzero(~rule & ~has_child)
    sinks = sinks[np.random.default_rng(7).permutation(len(sinks))]
    eng = E.Engine(0)
    kernel = "k_lrep_lds" if a.lds else "k_lrep_glob"
    twin = "k_lin_lds" if a.lds else "k_lin_glob"
    try:
        eng.set_option("wit_lds_max", a.lds)
        eng.set_option("kl_grid", a.grid)
        eng.load(corpus)
        for n in [int(x) for x in a.absent.split(",")]:
            A = [int(v) for v in sinks[:n]]
            for size in [int(x) for x in a.sizes.split(",")]:
                row = {"V": n1 - n0, "E": e1 - e0, "sinks": len(sinks), "absent": len(A), "max_size": size, "kl_grid": a.grid}
                try:
                    rows = eng.lineage_repair_sets(it, 1, A, None, size)
                    status, _, st = eng.lineage_repair_stats()
                    row.update(status=status, rows=len(rows), sets_per_level=[int(x) for x in st[:size + 1, 0]])
                    row["chunks"] = chunks(st[:size + 1, 0]) + 1
                    row["lineage_repair_sets"] = timed(eng, lambda: eng.lineage_repair_sets(it, 1, A, None, size), a.steps, a.warmup)
                    if kernel in row["lineage_repair_sets"]:
                        row["us_per_chunk"] = round(1e3 * row["lineage_repair_sets"][kernel] / row["chunks"], 3)
                    cuts = eng.lineage_cuts(it, 1, A, size)
                    cst = eng.lineage_cut_stats()
                    row.update(cut_rows=len(cuts), cut_sets_per_level=[int(x) for x in cst[:size + 1, 0]], cut_chunks=chunks(cst[:size + 1, 0]))
                    row["lineage_cuts"] = timed(eng, lambda: eng.lineage_cuts(it, 1, A, size), a.steps, a.warmup)
                    if twin in row["lineage_cuts"] and row["cut_chunks"]:
                        row["cut_us_per_chunk"] = round(1e3 * row["lineage_cuts"][twin] / row["cut_chunks"], 3)
                    if "us_per_chunk" in row and "cut_us_per_chunk" in row:
                        row["ratio"] = round(row["us_per_chunk"] / row["cut_us_per_chunk"], 3)
                except E.NemoError as e:  # a level past lineage_children_max: reported, not timed
                    row["error"] = e.msg
                print(json.dumps(row), flush=True)
    finally:
        eng.close()


if __name__ == "__main__":
    main()
