#!/usr/bin/env python3
"""Time nemo_min_label_cuts on the bench's C3 corpus, next to what a caller had before it: the host enumerates a
round's label sets, uploads them through nemo_knockout_labels, downloads the words and counts, and applies q and the
minimality filter on the host.

The corpus is bench.py's C3 corpus (`--runs` runs of ~5k-node graphs, run 0 prepended).  The run list is the post
graph of every good run; the candidates are `--cands` of run 0's sink labels, so that round 2 has a few thousand chunks
of 64 pairs (700 candidates: 244,650 pairs, 3,823 chunks if all are live).  max_size is 2 and q is `--min-runs`.  The
tool first checks that both paths give the same rows and n_lost, then times them alternately, `--rounds` times, in one
session, and prints one JSON line:
  wall_ms        host clock around one whole answer (both rounds), median of `--steps` per alternation, timing events off
  sweep_ms       the sweep kernels' event time per answer (k_lc_lds + k_lc_glob, or k_kl_lds + k_kl_glob)
  us_per_graph_chunk   sweep_ms over (list positions x chunks of both rounds)
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nemo_amd import engine as E  # noqa: E402
from tools import synth  # noqa: E402


def host_loop(eng, its, cand, q, sinks):
    """the parent commit's path: (rows [(size, labels)], n_lost, chunks evaluated)"""
    n = len(its)
    q = q or n
    singles = (np.arange(len(cand) + 1, dtype=np.uint64), cand)
    eng.knockout_labels(its, 1, singles, sinks_only=sinks)
    n_lost, n_hit = eng.knockout_label_counts()
    rows = [((int(cand[p]),), int(n_lost[p])) for p in np.flatnonzero(n_lost >= q)]
    live = cand[(n_lost < q) & (n_hit > 0)]
    chunks = (len(cand) + 63) // 64
    k1 = len(live)
    if k1 >= 2:
        hi, lo = np.tril_indices(k1, -1)  # row hi, columns lo < hi: the colex order, all pairs below position hi first
        labels = np.empty(2 * len(lo), np.uint32)
        labels[0::2], labels[1::2] = live[lo], live[hi]
        off = np.arange(len(lo) + 1, dtype=np.uint64) * 2
        eng.knockout_labels(its, 1, (off, labels), sinks_only=sinks)
        n_lost, _ = eng.knockout_label_counts()
        rows += [((int(live[lo[s]]), int(live[hi[s]])), int(n_lost[s])) for s in np.flatnonzero(n_lost >= q)]
        chunks += (len(lo) + 63) // 64
    return rows, chunks


def device_call(eng, its, cand, q, sinks):
    rows, n_lost = eng.min_label_cuts(its, 1, cand, 2, q, sinks_only=sinks)
    return [(tuple(int(x) for x in r["label"][:int(r["size"])]), int(c)) for r, c in zip(rows, n_lost)]


def timed_sweeps(eng, fn, groups, steps):
    eng.set_timing(True)
    eng.set_timing_groups(groups)
    eng.reset_timings()
    for _ in range(steps):
        fn()
    eng.synchronize()
    t = eng.timings()
    eng.set_timing(False)
    return {g: round(t[g]["ms"] / steps, 4) for g in groups if g in t and t[g]["launches"]}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=64)
    ap.add_argument("--cands", type=int, default=700)
    ap.add_argument("--min-runs", type=int, default=0)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=3, help="alternations of the two paths")
    ap.add_argument("--sinks", action="store_true", help="NEMO_KL_SINKS")
    a = ap.parse_args()
    corpus, _ = synth.generate(a.runs, prepend_run0=True, threads=min(16, os.cpu_count() or 1), **synth.CONFIGS["c3"])
    its = [int(x) for x in corpus.success_iters()]
    it0 = int(corpus.iteration[0])
    eng = E.Engine(0)
    out = {"runs": corpus.n_runs, "graphs": len(its), "steps": a.steps, "rounds": a.rounds, "sinks": bool(a.sinks), "min_runs": a.min_runs}
    try:
        eng.load(corpus)
        leaves = eng.knockout_leaves([it0], 1).copy()
        n0 = int(corpus.node_off[2 * corpus.run_index(it0) + 1])
        labels = corpus.label[n0 + leaves["node"].astype(np.int64)]
        cand = np.ascontiguousarray(list(dict.fromkeys(labels.tolist()))[:a.cands], dtype=np.uint32)
        want, chunks = host_loop(eng, its, cand, a.min_runs, a.sinks)
        got = device_call(eng, its, cand, a.min_runs, a.sinks)
        assert got == want, "the two paths' rows differ"  # parity before any timing
        stats = eng.min_label_cut_stats().reshape(-1).tolist()
        out.update({"cands": len(cand), "rows": len(got), "stats": stats, "graph_chunks": len(its) * chunks})
        paths = {"host_loop": (lambda: host_loop(eng, its, cand, a.min_runs, a.sinks), ["k_klabel", "k_kl_lds", "k_kl_glob"]),
                 "min_label_cuts": (lambda: device_call(eng, its, cand, a.min_runs, a.sinks),
                                    ["k_lcuts", "k_lc_lds", "k_lc_glob", "k_lc_reduce", "k_lc_support"])}
        res = {name: {"wall_ms": [], "sweep_ms": []} for name in paths}
        for _ in range(a.rounds):
            for name, (fn, groups) in paths.items():
                for _ in range(a.warmup):
                    fn()
                wall = []
                for _ in range(a.steps):
                    t0 = time.perf_counter()
                    fn()
                    wall.append(1e3 * (time.perf_counter() - t0))
                ms = timed_sweeps(eng, fn, groups, a.steps)
                res[name]["wall_ms"].append(round(statistics.median(wall), 3))
                res[name]["sweep_ms"].append(round(sum(v for k, v in ms.items() if k.endswith("_lds") or k.endswith("_glob")), 4))
                res[name]["kernels_ms"] = ms
        for name, r in res.items():
            r["us_per_graph_chunk"] = [round(1e3 * s / (len(its) * chunks), 5) for s in r["sweep_ms"]]
        out.update(res)
    finally:
        eng.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
