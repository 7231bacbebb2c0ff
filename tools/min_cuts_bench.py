#!/usr/bin/env python3
"""Time nemo_min_cuts on the bench's C3 corpus, next to the same pair hypotheses through nemo_knockout_sets.

The corpus is bench.py's C3 corpus (`--runs` runs of ~5k-node graphs, run 0 prepended).  The subject is run 0's post
graph with all its sink goals as candidates and max_size 2: K singles, then C(K1,2) pairs of the live ones.  The
second path enumerates the same pairs on the host in colex order and passes them as explicit sets, without masks.
Before anything is timed the two are compared: the pairs that sets mode reports lost, minus those that hold a
size-1 cut, must be exactly the size-2 rows of the cut call, in order.  Reported for both paths:
  wall_ms        host clock around the call (both block until their rows are on the host), median of `--steps`
                 calls after `--warmup` calls, timing events off
  kernel_ms      HIP-event time per call of the sweep kernel (k_cut_lds / k_cut_glob: all rounds; k_ko_lds /
                 k_ko_glob), and of the whole group (k_cuts, k_knock), from a second set of calls
  us_per_chunk   the sweep kernel's time per chunk of 64 hypotheses
With a library that has no nemo_min_cuts (an older build), only the sets path runs, so the same file measures the
yardstick on it.  One JSON line.  Needs a GPU (no fallback).

--repairs times the dual search instead of the sets path, beside nemo_min_cuts on the same graph: nemo_min_repair_sets
with every sink goal of run 0's post graph absent and a candidate (K singles, C(K1,2) pairs: nemo_min_cuts' hypothesis
counts where no single sink is a cut or a repair), kernels k_repair_lds / k_repair_glob, group k_repair; and the pair
form nemo_min_repairs of run 0 against the first failed run, whose absent sinks are few.
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


def pairs_colex(k):
    """(a, b) of every pair of positions < k in colex order: b outermost, a < b"""
    b = np.repeat(np.arange(k, dtype=np.int64), np.arange(k, dtype=np.int64))
    a = np.arange(len(b), dtype=np.int64) - b * (b - 1) // 2
    return a, b


def timed_calls(eng, call, groups, steps, warmup):
    for _ in range(warmup):
        call()
    wall = []
    for _ in range(steps):
        t0 = time.perf_counter()
        call()
        wall.append(1e3 * (time.perf_counter() - t0))
    eng.set_timing(True)
    eng.set_timing_groups(groups)
    eng.reset_timings()
    for _ in range(steps):
        call()
    eng.synchronize()
    t = eng.timings()
    eng.set_timing(False)
    return wall, {g: t[g]["ms"] / steps for g in groups if g in t and t[g]["launches"]}


def report(wall, ms, group, kernels, chunks):
    kern = sum(ms.get(k, 0.0) for k in kernels)
    return {"wall_ms": round(statistics.median(wall), 3), "wall_ms_min_max": [round(min(wall), 3), round(max(wall), 3)],
            "group_ms": round(ms.get(group, 0.0), 4), "kernel": [k for k in kernels if k in ms], "kernel_ms": round(kern, 4),
            "chunks": int(chunks), "us_per_chunk": round(1e3 * kern / max(int(chunks), 1), 5)}


def repairs_mode(eng, corpus, it, a, out):
    """nemo_min_cuts and nemo_min_repair_sets over all sink goals of run 0's post graph, max_size 2, and the pair form"""
    cand = eng.knockout_leaves([it], 1)["node"].astype(np.uint32).copy()
    eng.min_cuts(it, 1, None, 2)
    cs = eng.min_cut_stats()
    chunks = sum((int(cs[s][1]) + 63) // 64 for s in range(2))
    wall, ms = timed_calls(eng, lambda: eng._chk(eng.L.nemo_min_cuts(eng.h, it, 1, None, 0, 2, 0)),
                           ["k_cuts", "k_cut_lds", "k_cut_glob"], a.steps, a.warmup)
    out["min_cuts"] = report(wall, ms, "k_cuts", ["k_cut_lds", "k_cut_glob"], chunks)
    out["min_cuts"]["hypotheses"] = [int(cs[0][1]), int(cs[1][1])]
    rows = eng.min_repair_sets(it, 1, cand, None, 2)
    status, n_absent, rs, _ = eng.min_repair_stats()
    chunks = 1 + sum((int(rs[s][1]) + 63) // 64 for s in range(2))  # round 0 is one chunk
    wall, ms = timed_calls(eng, lambda: eng._chk(eng.L.nemo_min_repair_sets(eng.h, it, 1, cand.ctypes.data, len(cand), None, 0, 2, 0)),
                           ["k_repair", "k_repair_lds", "k_repair_glob"], a.steps, a.warmup)
    out["min_repair_sets"] = report(wall, ms, "k_repair", ["k_repair_lds", "k_repair_glob"], chunks)
    out["min_repair_sets"].update({"status": status, "absent": n_absent, "rows": len(rows), "hypotheses": [int(rs[0][1]), int(rs[1][1])]})
    if out["min_cuts"]["us_per_chunk"]:
        out["repair_over_cut_per_chunk"] = round(out["min_repair_sets"]["us_per_chunk"] / out["min_cuts"]["us_per_chunk"], 4)
    failed = corpus.failed_iters()
    if failed:
        eng.mark()
        f = failed[0]
        rows = eng.min_repairs(it, f, 2)
        status, n_absent, rs, _ = eng.min_repair_stats()
        wall, ms = timed_calls(eng, lambda: eng._chk(eng.L.nemo_min_repairs(eng.h, it, f, 2, 0)),
                               ["k_repair", "k_repair_lds", "k_repair_glob", "k_repair_absent", "k_lab_hash"], a.steps, a.warmup)
        out["min_repairs"] = {"other": f, "status": status, "absent": n_absent, "rows": len(rows),
                              "wall_ms": round(statistics.median(wall), 3), "ms": {k: round(v, 4) for k, v in ms.items()}}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=10000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--lds-max", type=int, default=-1, help="option knock_lds_max (0: the global tier)")
    ap.add_argument("--repairs", action="store_true", help="nemo_min_repair_sets / nemo_min_repairs beside nemo_min_cuts")
    a = ap.parse_args()
    have_cuts = hasattr(E.Engine, "min_cuts")
    corpus, _ = synth.generate(a.runs, prepend_run0=True, threads=min(16, os.cpu_count() or 1), **synth.CONFIGS["c3"])
    it = int(corpus.iteration[0])
    eng = E.Engine(0)
    out = {"runs": corpus.n_runs, "steps": a.steps, "lds_max": a.lds_max, "has_min_cuts": have_cuts}
    try:
        eng.set_option("knock_lds_max", a.lds_max)
        eng.load(corpus)
        if a.repairs:
            repairs_mode(eng, corpus, it, a, out)
            print(json.dumps(out))
            return
        leaves = eng.knockout_leaves([it], 1).copy()
        cand = leaves["node"].astype(np.uint32)
        single = (leaves["n_roots"] > 0) & (leaves["roots_dead"] == leaves["n_roots"])
        K = len(cand)
        pa, pb = pairs_colex(K)
        H = len(pa)
        nodes = np.empty(2 * H, np.uint32)
        nodes[0::2], nodes[1::2] = cand[pa], cand[pb]
        off = np.arange(H + 1, dtype=np.uint64) * 2
        sets = eng.knockout_sets_raw(it, 1, off, nodes, H)
        lost = (sets["n_roots"] > 0) & (sets["roots_dead"] == sets["n_roots"])
        minimal = lost & ~single[pa] & ~single[pb]
        out.update({"candidates": K, "pairs": H, "size1_cuts": int(single.sum()), "pairs_lost": int(lost.sum()),
                    "pairs_minimal": int(minimal.sum())})
        if have_cuts:
            rows = eng.min_cuts(it, 1, None, 2)
            stats = eng.min_cut_stats()
            two = rows[rows["size"] == 2]["node"][:, :2].astype(np.int64)
            one = rows[rows["size"] == 1]["node"][:, 0].astype(np.int64)
            # every pair of live candidates keeps its colex order among all pairs, so the rows are the minimal pairs in order
            want = np.column_stack([cand[pa[minimal]], cand[pb[minimal]]]).astype(np.int64)
            assert np.array_equal(one, cand[single].astype(np.int64)), "size-1 cuts differ from knockout_leaves"
            assert np.array_equal(two, want), "size-2 cuts differ from the lost pairs of knockout_sets"
            assert int(stats[0][1]) == K and int(stats[1][2]) == len(want)
            chunks = sum((int(stats[s][1]) + 63) // 64 for s in range(2))
            wall, ms = timed_calls(eng, lambda: eng._chk(eng.L.nemo_min_cuts(eng.h, it, 1, None, 0, 2, 0)),
                                   ["k_cuts", "k_cut_lds", "k_cut_glob"], a.steps, a.warmup)
            out["min_cuts"] = report(wall, ms, "k_cuts", ["k_cut_lds", "k_cut_glob"], chunks)
            out["live"] = int(stats[1][0])
        wall, ms = timed_calls(eng, lambda: eng._chk(eng.L.nemo_knockout_sets(eng.h, it, 1, off.ctypes.data, nodes.ctypes.data, H, 0)),
                               ["k_knock", "k_ko_lds", "k_ko_glob"], a.steps, a.warmup)
        out["knockout_sets"] = report(wall, ms, "k_knock", ["k_ko_lds", "k_ko_glob"], (H + 63) // 64)
    finally:
        eng.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
