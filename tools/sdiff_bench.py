#!/usr/bin/env python3
"""Time nemo_diffprov_symmetric (k_sdiff) on a role-exchanged C3 corpus, next to the two existing
per-graph LDS kernels of the same form (stage a graph, sweep its levels): k_marksimp and k_proto.

The generator's failed runs derive a subset of run 0's labels, so the corpus is loaded with one
failed (sparse) run as iteration 0 and every successful run as an entry: each entry then has a
non-empty S.  3 warm-up calls, then `--steps` timed calls with the k_sdiff / k_marksimp / k_proto
timing groups (HIP events around the launches).  Prints one JSON line: milliseconds per call,
algorithmic bytes (DESIGN.md §Symmetric diff), the fraction of HBM peak as bench.py computes it
(bytes / time / 8000 GB/s), and the time per graph of the three kernels.

--pairs: instead, three legs on the same corpus and entries, in one process and with the same method
(HIP events around the launches of the k_lab_hash and k_sdiff groups): (a) nemo_diffprov_symmetric,
(b) nemo_diffprov_pairs with every `other` = iteration 0 (the load's shared table, nothing built),
(c) nemo_diffprov_pairs with a distinct good `other` per entry (one table per entry).  The legs
alternate `--rounds` times; prints one JSON line with every round's milliseconds per call and the
table memory of (c).

Reads nothing but the synthetic generator's output; needs a GPU (no fallback).
"""
import argparse
import dataclasses
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from nemo_amd import engine as E  # noqa: E402
from tools import synth  # noqa: E402

HBM_PEAK_GBS = 8000.0  # as bench.py


def role_exchanged(corpus):
    it = corpus.iteration.astype(np.int64).copy()
    r0 = corpus.run_index(0)
    rf = next(r for r in range(corpus.n_runs) if corpus.status[r] != "success")
    it[r0], it[rf] = it[rf], 0
    ex = dataclasses.replace(corpus, iteration=np.ascontiguousarray(it, dtype=np.uint32))
    return ex, [int(it[r]) for r in range(corpus.n_runs) if corpus.status[r] == "success"]


def pairs_legs(ex, entries, steps, warmup, rounds):
    """The three legs of --pairs, alternating; per leg and round the groups' ms per call."""
    n = len(entries)
    distinct = entries[1:] + entries[:1]  # entry e against the next good run: n distinct `other` runs
    legs = {"a_symmetric": lambda eng: eng.diffprov_symmetric(entries),
            "b_pairs_shared": lambda eng: eng.diffprov_pairs(entries, [0] * n),
            "c_pairs_distinct": lambda eng: eng.diffprov_pairs(entries, distinct)}
    # the region of (c): one table per entry, the smallest power of two >= twice the other graph's nodes (>= 16)
    slots = 0
    for it in distinct:
        v, cap = ex.graph_size(2 * ex.run_index(it) + 1), 16
        while cap < 2 * v:
            cap *= 2
        slots += cap
    out = {"runs": ex.n_runs, "entries": n, "steps": steps, "rounds": rounds, "c_tables": n,
           "c_table_bytes": 4 * slots, "legs": {k: [] for k in legs}}
    eng = E.Engine(0)
    try:
        eng.load(ex)
        eng.mark()
        ref = None
        for name, call in legs.items():
            for _ in range(warmup):
                call(eng)
            eng.synchronize()
            masks = eng.sdiff_masks()
            if name == "a_symmetric":
                ref = masks
                out["entries_nonempty"] = sum(1 for m in masks if m.any())
            elif name == "b_pairs_shared":
                out["b_equals_a"] = all(np.array_equal(x, y) for x, y in zip(ref, masks))
            else:
                out["c_entries_nonempty"] = sum(1 for m in masks if m.any())
        eng.set_timing(True)
        eng.set_timing_groups(["k_lab_hash", "k_sdiff"])
        for _ in range(rounds):
            for name, call in legs.items():
                eng.reset_timings()
                for _ in range(steps):
                    call(eng)
                eng.synchronize()
                t = eng.timings()
                row = {}
                for g in ("k_lab_hash", "k_sdiff"):
                    if g in t and t[g]["launches"]:
                        ms = t[g]["ms"] / t[g]["launches"]
                        gb = t[g]["bytes"] / t[g]["launches"]
                        row[g] = {"ms_per_call": round(ms, 4), "bytes": gb, "gbs": round(gb / ms / 1e6, 1)}
                out["legs"][name].append(row)
    finally:
        eng.close()
    print(json.dumps(out))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=10000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--pairs", action="store_true", help="time symmetric / pairs-shared / pairs-distinct instead")
    ap.add_argument("--rounds", type=int, default=3, help="--pairs: alternations of the three legs")
    a = ap.parse_args()
    corpus, _ = synth.generate(a.runs, **synth.CONFIGS["c3"])
    ex, entries = role_exchanged(corpus)
    if a.pairs:
        pairs_legs(ex, entries, a.steps, a.warmup, a.rounds)
        return
    success = list(entries)
    eng = E.Engine(0)
    try:
        eng.load(ex)
        eng.mark()
        for _ in range(a.warmup):
            eng.mark()  # k_marksimp takes the mark this call defers, as in a bench step
            eng.simplify()
            eng.protos_partial(success, 0)
            eng.diffprov_symmetric(entries)
        eng.synchronize()
        nonempty = sum(1 for m in eng.sdiff_masks() if m.any())
        eng.set_timing(True)
        eng.set_timing_groups(["k_sdiff", "k_marksimp", "k_proto"])
        eng.reset_timings()
        for _ in range(a.steps):
            eng.mark()
            eng.simplify()
            eng.protos_partial(success, 0)
            eng.diffprov_symmetric(entries)
        eng.synchronize()
        t = eng.timings()
    finally:
        eng.close()
    out = {"runs": ex.n_runs, "entries": len(entries), "entries_nonempty": nonempty, "steps": a.steps}
    per_graph = {}
    for name, graphs in (("k_sdiff", len(entries)), ("k_marksimp", ex.n_graphs), ("k_proto", ex.n_runs)):
        g = t.get(name)
        if not g or not g["launches"]:
            out[name] = None
            continue
        ms = g["ms"] / g["launches"]
        gb = g["bytes"] / g["launches"]
        out[name] = {"ms_per_call": round(ms, 4), "bytes": gb, "gbs": round(gb / ms / 1e6, 1),
                     "hbm_frac": round(gb / ms / 1e6 / HBM_PEAK_GBS, 4), "graphs": graphs,
                     "us_per_graph": round(1e3 * ms / graphs, 4)}
        per_graph[name] = 1e3 * ms / graphs
    if "k_sdiff" in per_graph and len(per_graph) == 3:
        slower = max(per_graph["k_marksimp"], per_graph["k_proto"])
        out["ratio_to_slower_yardstick"] = round(per_graph["k_sdiff"] / slower, 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
