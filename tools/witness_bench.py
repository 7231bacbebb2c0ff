#!/usr/bin/env python3
"""Time nemo_witness_sets / nemo_witness_labels on the bench's C3 corpus against the knock-out calls on the same sets.

The corpus is bench.py's C3 corpus (`--runs` runs of ~5k-node graphs, run 0 prepended).  The hypotheses are run 0's
sink goals as singleton sets: as nodes on run 0's post graph (nemo_witness_sets against nemo_knockout_sets, no
masks) and as labels, sink goals only, on every good run's post graph (nemo_witness_labels against
nemo_knockout_labels).  Before anything is timed the device rows are compared where the calls overlap: roots_alive
against n_roots - roots_dead, and roots_alive == 0 < n_roots against the label form's lost bits.  Then, for every
value of `--lds-max` (option wit_lds_max; the knock-out calls keep their own tier), `--rounds` rounds alternate
the yardstick and the new call, `--steps` calls each after `--warmup`:
  wall_ms            host clock around the call (it blocks until the rows are on the host), median
  k_witness / k_wit_lds / k_wit_glob / k_knock / k_ko_lds / k_klabel / k_kl_lds
                     HIP-event time per call from a second set of calls with timing on
  us_per_graph_chunk the sweep kernel's time per (listed graph, chunk of 64 sets)
One JSON line per (lds_max, round).  Needs a GPU (no fallback).
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
from nemo_amd.corpus import NODE_RULE  # noqa: E402
from tools import synth  # noqa: E402

GROUPS = ["k_witness", "k_wit_lds", "k_wit_glob", "k_wit_table", "k_knock", "k_ko_lds", "k_ko_glob", "k_klabel", "k_kl_lds", "k_kl_glob"]


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
    ap.add_argument("--runs", type=int, default=1000)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--lds-max", default="159744,81920,0", help="values of option wit_lds_max, in turn")
    a = ap.parse_args()
    corpus, _ = synth.generate(a.runs, prepend_run0=True, threads=min(16, os.cpu_count() or 1), **synth.CONFIGS["c3"])
    good = corpus.success_iters()
    g0 = 2 * corpus.run_index(0) + 1
    n0, n1, e0, e1 = int(corpus.node_off[g0]), int(corpus.node_off[g0 + 1]), int(corpus.edge_off[g0]), int(corpus.edge_off[g0 + 1])
    has_child = np.zeros(n1 - n0, bool)
    has_child[corpus.edge_src[e0:e1]] = True
    leaves = np.flatnonzero(~has_child & ((corpus.node_word[n0:n1] & np.uint32(NODE_RULE)) == 0))
    sets = [[int(v)] for v in leaves]
    lsets = [[int(corpus.label[n0 + v])] for v in leaves]
    chunks = (len(sets) + 63) // 64
    eng = E.Engine(0)
    try:
        eng.load(corpus)
        # the rows where the calls overlap
        ko = eng.knockout_sets(0, 1, sets).copy()
        wt = eng.witness_sets(0, 1, sets).copy()
        assert np.array_equal(wt["roots_alive"], ko["n_roots"] - ko["roots_dead"]) and np.array_equal(wt["n_roots"], ko["n_roots"])
        lost, _ = eng.knockout_labels(good, 1, lsets, sinks_only=True)
        wl = eng.witness_labels(good, 1, lsets, sinks_only=True).reshape(len(good), len(sets))
        bits = ((lost[:, :, None] >> np.arange(64, dtype=np.uint64)[None, None, :]) & np.uint64(1)).reshape(len(good), -1)[:, :len(sets)]
        assert np.array_equal(bits.astype(bool), (wl["roots_alive"] == 0) & (wl["n_roots"] > 0)), "lost bits and roots_alive differ"
        head = {"runs": corpus.n_runs, "good": len(good), "sets": len(sets), "chunks": chunks, "V0": n1 - n0, "E0": e1 - e0,
                "n_nodes_mean": round(float(wt["n_nodes"].mean()), 1), "n_sinks_mean": round(float(wt["n_sinks"].mean()), 1)}
        for lds in [int(x) for x in a.lds_max.split(",")]:
            eng.set_option("wit_lds_max", lds)
            for rnd in range(a.rounds):
                row = dict(head, wit_lds_max=lds, round=rnd)
                row["knockout_sets"] = timed(eng, lambda: eng.knockout_sets(0, 1, sets), a.steps, a.warmup)
                row["witness_sets"] = timed(eng, lambda: eng.witness_sets(0, 1, sets), a.steps, a.warmup)
                row["witness_sets_all"] = timed(eng, lambda: eng.witness_sets(0, 1, sets, all=True), a.steps, a.warmup)
                row["knockout_labels"] = timed(eng, lambda: eng.knockout_labels(good, 1, lsets, sinks_only=True), a.steps, a.warmup)
                row["witness_labels"] = timed(eng, lambda: eng.witness_labels(good, 1, lsets, sinks_only=True), a.steps, a.warmup)
                for name, n_graphs in (("witness_sets", 1), ("witness_labels", len(good)), ("knockout_sets", 1), ("knockout_labels", len(good))):
                    ms = sum(row[name].get(k, 0.0) for k in ("k_wit_lds", "k_wit_glob", "k_ko_lds", "k_ko_glob", "k_kl_lds", "k_kl_glob"))
                    row[name]["us_per_graph_chunk"] = round(1e3 * ms / (n_graphs * chunks), 4)
                row["ratio_sets_wall"] = round(row["witness_sets"]["wall_ms"] / row["knockout_sets"]["wall_ms"], 3)
                row["ratio_labels_wall"] = round(row["witness_labels"]["wall_ms"] / row["knockout_labels"]["wall_ms"], 3)
                print(json.dumps(row), flush=True)
    finally:
        eng.close()


if __name__ == "__main__":
    main()
