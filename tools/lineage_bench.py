#!/usr/bin/env python3
"""nemo_lineage_cuts beside nemo_min_cuts on the C3-shaped graph (run 0's post graph of a 12-run corpus, every sink
goal a candidate): per max_size the sets each level evaluates, the hypotheses each round of nemo_min_cuts evaluates
(max_size 2 and 3; the exhaustive search stops there), both calls' wall time (a host clock around the blocking call,
median of --steps after --warmup) and, from a second set of calls with event timing on, the time of the groups and of
the new kernels (nemo_timings).  One JSON line per max_size.

  python tools/lineage_bench.py --steps 10 --warmup 2 --sizes 2,3,4,5,6
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from nemo_amd import engine as E  # noqa: E402
from tools import synth  # noqa: E402

GROUPS = ["k_lineage", "k_lin_lds", "k_lin_glob", "k_lin_filter", "k_lin_rehash", "k_cuts", "k_cut_lds", "k_cut_glob"]


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
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sizes", default="2,3,4,5,6")
    ap.add_argument("--min-cuts-max", type=int, default=2,
                    help="largest max_size nemo_min_cuts is run at (round 3 over thousands of live candidates is billions of "
                         "hypotheses: past this size its count is given by the formula C(K1, 3) and no time is taken)")
    a = ap.parse_args()
    corpus, _ = synth.generate(12, p_fault=0.55, prepend_run0=True, **synth.CONFIGS["c3"])
    it = int(corpus.iteration[0])
    g = 2 * corpus.run_index(it) + 1
    eng = E.Engine(0)
    try:
        eng.load(corpus)
        for size in [int(x) for x in a.sizes.split(",")]:
            row = {"V": corpus.graph_size(g), "max_size": size}
            try:
                rows = eng.lineage_cuts(it, 1, None, size)
            except E.NemoError as e:  # a level past lineage_children_max: reported, not timed
                row["error"] = e.msg
                print(json.dumps(row), flush=True)
                continue
            st = eng.lineage_cut_stats()
            row["rows"] = len(rows)
            row["sets_per_level"] = [int(x) for x in st[:size + 1, 0]]
            row["cuts_per_level"] = [int(x) for x in st[:size + 1, 1]]
            row["lineage_cuts"] = timed(eng, lambda: eng.lineage_cuts(it, 1, None, size), a.steps, a.warmup)
            if size <= min(a.min_cuts_max, 3):
                ref = eng.min_cuts(it, 1, None, size)
                assert len(ref) == len(rows) and all(int(x["size"]) == int(y["size"]) and
                                                     list(x["node"][:3]) == list(y["node"][:3]) for x, y in zip(ref, rows))
                row["min_cuts_hypotheses"] = [int(x) for x in eng.min_cut_stats()[:size, 1]]
                row["min_cuts"] = timed(eng, lambda: eng.min_cuts(it, 1, None, size), max(1, a.steps // (5 if size == 3 else 1)), 1)
            elif size == 3:
                eng.min_cuts(it, 1, None, 2)
                k, k1 = int(eng.min_cut_stats()[0, 1]), int(eng.min_cut_stats()[1, 0])
                row["min_cuts_hypotheses_by_formula"] = [k, k1 * (k1 - 1) // 2, k1 * (k1 - 1) * (k1 - 2) // 6]
            print(json.dumps(row), flush=True)
    finally:
        eng.close()


if __name__ == "__main__":
    main()
