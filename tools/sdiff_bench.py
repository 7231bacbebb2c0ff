#!/usr/bin/env python3
"""Time nemo_diffprov_symmetric (k_sdiff) on a role-exchanged C3 corpus, next to the two existing
per-graph LDS kernels of the same form (stage a graph, sweep its levels): k_marksimp and k_proto.

The generator's failed runs derive a subset of run 0's labels, so the corpus is loaded with one
failed (sparse) run as iteration 0 and every successful run as an entry: each entry then has a
non-empty S.  3 warm-up calls, then `--steps` timed calls with the k_sdiff / k_marksimp / k_proto
timing groups (HIP events around the launches).  Prints one JSON line: milliseconds per call,
algorithmic bytes (DESIGN.md §Symmetric diff), the fraction of HBM peak as bench.py computes it
(bytes / time / 8000 GB/s), and the time per graph of the three kernels.

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


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=10000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    corpus, _ = synth.generate(a.runs, **synth.CONFIGS["c3"])
    ex, entries = role_exchanged(corpus)
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
