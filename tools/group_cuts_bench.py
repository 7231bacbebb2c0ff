#!/usr/bin/env python3
"""Time nemo_min_group_cuts on the bench's C3 corpus, next to what a caller had before it: the host enumerates a
round's sets of groups, writes each set's union of labels out, uploads the unions through nemo_knockout_labels,
downloads the counts, and applies q and the minimality filter on the host.

The corpus is bench.py's C3 corpus (`--runs` runs of ~5k-node graphs, run 0 prepended).  The run list is the post
graph of every good run.  The candidates are fault events over run 0's sink labels in node order: the first `--cands`
labels as omission groups of one label each, and crash-like groups over the first `--crash-labels` labels: label k
has location k % `--locs` and time (k // `--locs`) scaled to 1 .. `--times`; the crash group (location, t) unites the
labels of that location with time >= t, so the groups of one location nest and hold tens to hundreds of labels.
max_size is 2 and q is `--min-runs`.  The tool first checks that both paths give the same rows and n_lost, then times
them alternately, `--rounds` times, in one session, and prints one JSON line:
  wall_ms        host clock around one whole answer (both rounds), median of `--steps` per alternation, timing events off
  sweep_ms       the sweep kernels' event time per answer (k_gc_lds + k_gc_glob, or k_kl_lds + k_kl_glob)
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


def make_groups(labels, cands, crash_labels, locs, times):
    groups = [np.array([x], np.uint32) for x in labels[:cands]]
    pool = labels[:crash_labels]
    k = np.arange(len(pool))
    loc, t = k % locs, 1 + (k // locs) * times // max(1, (len(pool) + locs - 1) // locs)
    for a in range(locs):
        for ct in range(1, times + 1):
            groups.append(np.ascontiguousarray(pool[(loc == a) & (t >= ct)], dtype=np.uint32))
    return groups


def unions(groups, sets):
    """(set_off, set_labels) of the sets' unions: the groups' labels one after the other (a label named twice in a
    set counts once, so no duplicate is removed)"""
    parts = [groups[p] for c in sets for p in c]
    lens = np.array([sum(len(groups[p]) for p in c) for c in sets], np.uint64)
    off = np.zeros(len(sets) + 1, np.uint64)
    off[1:] = np.cumsum(lens, dtype=np.uint64)
    return off, (np.concatenate(parts) if parts else np.zeros(0, np.uint32))


def host_loop(eng, its, groups, q, sinks):
    """the parent commit's path: (rows [(positions, n_lost)], chunks evaluated)"""
    n = len(its)
    q = q or n
    K = len(groups)
    eng.knockout_labels(its, 1, unions(groups, [(p,) for p in range(K)]), sinks_only=sinks)
    n_lost, n_hit = eng.knockout_label_counts()
    rows = [((int(p),), int(n_lost[p])) for p in np.flatnonzero(n_lost >= q)]
    live = np.flatnonzero((n_lost < q) & (n_hit > 0))
    chunks = (K + 63) // 64
    k1 = len(live)
    if k1 >= 2:
        hi, lo = np.tril_indices(k1, -1)  # row hi, columns lo < hi: the colex order, all pairs below position hi first
        pairs = list(zip(live[lo].tolist(), live[hi].tolist()))
        eng.knockout_labels(its, 1, unions(groups, pairs), sinks_only=sinks)
        n_lost, _ = eng.knockout_label_counts()
        rows += [(pairs[s], int(n_lost[s])) for s in np.flatnonzero(n_lost >= q)]
        chunks += (len(lo) + 63) // 64
    return rows, chunks


def device_call(eng, its, packed, q, sinks):
    rows, n_lost = eng.min_group_cuts(its, 1, packed, 2, q, sinks_only=sinks)
    return [(tuple(int(x) for x in r["group"][:int(r["size"])]), int(c)) for r, c in zip(rows, n_lost)]


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
    ap.add_argument("--cands", type=int, default=300, help="omission groups")
    ap.add_argument("--crash-labels", type=int, default=2000)
    ap.add_argument("--locs", type=int, default=8)
    ap.add_argument("--times", type=int, default=12)
    ap.add_argument("--min-runs", type=int, default=0)
    ap.add_argument("--steps", type=int, default=3)
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
        labels = np.ascontiguousarray(list(dict.fromkeys(labels.tolist())), dtype=np.uint32)
        groups = make_groups(labels, a.cands, a.crash_labels, a.locs, a.times)
        packed = unions(groups, [(p,) for p in range(len(groups))])
        want, chunks = host_loop(eng, its, groups, a.min_runs, a.sinks)
        got = device_call(eng, its, packed, a.min_runs, a.sinks)
        assert got == want, "the two paths' rows differ"  # parity before any timing
        stats = eng.min_group_cut_stats().reshape(-1).tolist()
        sizes = sorted(len(g) for g in groups[a.cands:])
        out.update({"groups": len(groups), "labels_named": int(packed[0][-1]), "crash_group_sizes": [sizes[0], sizes[len(sizes) // 2], sizes[-1]],
                    "rows": len(got), "stats": stats, "graph_chunks": len(its) * chunks})
        paths = {"host_loop": (lambda: host_loop(eng, its, groups, a.min_runs, a.sinks), ["k_klabel", "k_kl_lds", "k_kl_glob"]),
                 "min_group_cuts": (lambda: device_call(eng, its, packed, a.min_runs, a.sinks),
                                    ["k_gcuts", "k_gc_table", "k_gc_rows", "k_gc_lds", "k_gc_glob", "k_lc_reduce", "k_lc_support"])}
        res = {name: {"wall_ms": [], "sweep_ms": []} for name in paths}
        for _ in range(a.rounds):
            for name, (fn, tgroups) in paths.items():
                for _ in range(a.warmup):
                    fn()
                wall = []
                for _ in range(a.steps):
                    t0 = time.perf_counter()
                    fn()
                    wall.append(1e3 * (time.perf_counter() - t0))
                ms = timed_sweeps(eng, fn, tgroups, a.steps)
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
