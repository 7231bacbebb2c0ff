#!/usr/bin/env python3
"""Time nemo_knockout_labels on the bench's C3 corpus, next to what a caller had before it: the same hypotheses
translated to node indices on the host and sent through nemo_knockout_sets, one blocking call per graph.

The corpus is bench.py's C3 corpus (`--runs` runs of ~5k-node graphs, run 0 prepended).  The hypotheses are the
labels of run 0's sink goals, one single-label set each (2,953 sets, 47 chunks at the default shape), evaluated on the
post graph of every good run in one call.  The per-graph path runs on a sample of `--sample` graphs spread over the
list and is scaled by graphs; its time is reported with and without the host translation.  `--no-hitlist` times the
new call under option kl_hitlist 0 (no hit list, every chunk probes with every node's label) and skips the yardstick.
Before anything is timed the sample's lost bits from nemo_knockout_sets are compared with the new call's.  Reported:
  wall_ms        host clock around the call(s), median of `--steps` calls after `--warmup` calls, timing events off
  kernel_ms      HIP-event time per call of the sweep kernels (k_kl_lds / k_kl_glob; k_ko_lds / k_ko_glob) and of
                 the whole group (k_klabel, k_knock), from a second set of calls
  us_per_chunk   the sweep kernels' time per (graph, chunk of 64 sets)
With a library that has no nemo_knockout_labels (an older build), only the per-graph path runs, so the same file
measures the yardstick on it.  One JSON line.  Needs a GPU (no fallback).
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


def translate(corpus, g, labels):
    """single-label sets -> (set_off u64, set_nodes u32) on graph g: every node that carries the set's label"""
    n0, n1 = int(corpus.node_off[g]), int(corpus.node_off[g + 1])
    lab = corpus.label[n0:n1]
    order = np.argsort(lab, kind="stable")
    sl = lab[order]
    lo, hi = np.searchsorted(sl, labels, "left"), np.searchsorted(sl, labels, "right")
    cnt = (hi - lo).astype(np.int64)
    off = np.zeros(len(labels) + 1, np.uint64)
    off[1:] = np.cumsum(cnt)
    idx = np.repeat(lo - np.concatenate([[0], np.cumsum(cnt)[:-1]]), cnt) + np.arange(int(cnt.sum()))
    return off, np.ascontiguousarray(order[idx], dtype=np.uint32)


def med(x):
    return round(statistics.median(x), 3)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=10000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sample", type=int, default=32, help="graphs of the per-graph path")
    ap.add_argument("--lds-max", type=int, default=-1, help="option knock_lds_max (0: the global tier)")
    ap.add_argument("--sinks", action="store_true", help="NEMO_KL_SINKS")
    ap.add_argument("--no-hitlist", action="store_true", help="option kl_hitlist 0: V probes per chunk (the new call alone is timed)")
    a = ap.parse_args()
    have = hasattr(E.Engine, "knockout_labels")
    corpus, _ = synth.generate(a.runs, prepend_run0=True, threads=min(16, os.cpu_count() or 1), **synth.CONFIGS["c3"])
    its = [int(x) for x in corpus.success_iters()]
    it0 = int(corpus.iteration[0])
    eng = E.Engine(0)
    out = {"runs": corpus.n_runs, "graphs": len(its), "steps": a.steps, "lds_max": a.lds_max, "has_knockout_labels": have,
           "sinks": bool(a.sinks), "hitlist": not a.no_hitlist}
    try:
        eng.set_option("knock_lds_max", a.lds_max)
        if a.no_hitlist:
            eng.set_option("kl_hitlist", 0)
        eng.load(corpus)
        leaves = eng.knockout_leaves([it0], 1).copy()
        n0 = int(corpus.node_off[2 * corpus.run_index(it0) + 1])
        labels = np.unique(corpus.label[n0 + leaves["node"].astype(np.int64)]).astype(np.uint32)
        n_sets = len(labels)
        ck = (n_sets + 63) // 64
        set_off = np.arange(n_sets + 1, dtype=np.uint64)
        it_arr = np.ascontiguousarray(its, dtype=np.uint32)
        sample = [its[k * len(its) // a.sample] for k in range(min(a.sample, len(its)))]
        out.update({"sets": n_sets, "chunks": ck, "sample": len(sample)})

        def per_graph(keep=None, timing=None):
            t_tr = t_call = 0.0
            for k, it in enumerate(sample):
                t0 = time.perf_counter()
                off, nodes = translate(corpus, 2 * corpus.run_index(it) + 1, labels)
                t1 = time.perf_counter()
                eng._chk(eng.L.nemo_knockout_sets(eng.h, it, 1, off.ctypes.data, nodes.ctypes.data if len(nodes) else None, n_sets, 0))
                t2 = time.perf_counter()
                t_tr, t_call = t_tr + (t1 - t0), t_call + (t2 - t1)
                if keep is not None:
                    r = eng.knockout_rows()
                    keep.append((r["n_roots"] > 0) & (r["roots_dead"] == r["n_roots"]))
            if timing is not None:
                timing.append((1e3 * t_tr, 1e3 * t_call))

        if not a.sinks:
            lost_sets = []
            per_graph(keep=lost_sets)
        if have:
            lost, hit = eng.knockout_labels(its, 1, (set_off, labels), sinks_only=a.sinks)
            n_lost, n_hit = eng.knockout_label_counts()
            out.update({"lost_bits": int(n_lost.sum()), "hit_bits": int(n_hit.sum()), "sets_lost_somewhere": int((n_lost > 0).sum())})
            if not a.sinks:
                for it, want in zip(sample, lost_sets):
                    row = lost[its.index(it)]
                    got = np.unpackbits(row.view(np.uint8), bitorder="little")[:n_sets].astype(bool)
                    assert np.array_equal(got, want), f"lost bits of run {it} differ from nemo_knockout_sets"

            def call():
                eng._chk(eng.L.nemo_knockout_labels(eng.h, it_arr.ctypes.data, len(its), 1, set_off.ctypes.data, labels.ctypes.data,
                                                    n_sets, E.KL_SINKS if a.sinks else 0))

            for _ in range(a.warmup):
                call()
            wall = []
            for _ in range(a.steps):
                t0 = time.perf_counter()
                call()
                wall.append(1e3 * (time.perf_counter() - t0))
            groups = ["k_klabel", "k_kl_tables", "k_kl_lds", "k_kl_glob", "k_kl_count"]
            eng.set_timing(True)
            eng.set_timing_groups(groups)
            eng.reset_timings()
            for _ in range(a.steps):
                call()
            eng.synchronize()
            t = eng.timings()
            eng.set_timing(False)
            ms = {g: t[g]["ms"] / a.steps for g in groups if g in t and t[g]["launches"]}
            sweep = ms.get("k_kl_lds", 0.0) + ms.get("k_kl_glob", 0.0)
            out["knockout_labels"] = {"wall_ms": med(wall), "wall_ms_min_max": [round(min(wall), 3), round(max(wall), 3)],
                                      "group_ms": round(ms.get("k_klabel", 0.0), 4), "kernels_ms": {k: round(v, 4) for k, v in ms.items()},
                                      "sweep_ms": round(sweep, 4), "graph_chunks": len(its) * ck,
                                      "us_per_graph_chunk": round(1e3 * sweep / (len(its) * ck), 5)}
        if not a.sinks and not a.no_hitlist:
            for _ in range(a.warmup):
                per_graph()
            tm = []
            for _ in range(a.steps):
                per_graph(timing=tm)
            groups = ["k_knock", "k_ko_lds", "k_ko_glob"]
            eng.set_timing(True)
            eng.set_timing_groups(groups)
            eng.reset_timings()
            for _ in range(a.steps):
                per_graph()
            eng.synchronize()
            t = eng.timings()
            eng.set_timing(False)
            ms = {g: t[g]["ms"] / a.steps for g in groups if g in t and t[g]["launches"]}
            sweep = ms.get("k_ko_lds", 0.0) + ms.get("k_ko_glob", 0.0)
            scale = len(its) / len(sample)
            calls = [c for _, c in tm]
            trans = [x for x, _ in tm]
            out["knockout_sets_per_graph"] = {
                "sample_call_wall_ms": med(calls), "sample_call_wall_ms_min_max": [round(min(calls), 3), round(max(calls), 3)],
                "sample_translate_ms": med(trans), "scaled_call_wall_ms": round(statistics.median(calls) * scale, 1),
                "scaled_wall_with_translation_ms": round((statistics.median(calls) + statistics.median(trans)) * scale, 1),
                "sample_group_ms": round(ms.get("k_knock", 0.0), 4), "sample_sweep_ms": round(sweep, 4),
                "scaled_sweep_ms": round(sweep * scale, 2), "graph_chunks": len(sample) * ck,
                "us_per_graph_chunk": round(1e3 * sweep / (len(sample) * ck), 5)}
    finally:
        eng.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
