#!/usr/bin/env python3
"""Time nemo_knockout_leaves on the bench's C3 corpus, next to a host baseline in the same process.

The corpus is bench.py's C3 corpus (`--runs` runs of ~5k-node graphs, run 0 prepended); the call knocks out every
sink goal of every good run's post graph, one at a time, without masks.  Reported:
  leaves         sink goals per listed graph: min, mean, max (everything else scales with it), hypotheses, chunks
  wall_ms        host clock around the call (it blocks until the rows are on the host), median of `--steps` calls
                 after `--warmup` calls, timing events off
  k_ko_*         HIP-event time per call of every kernel of the group (k_ko_leaves: both launches; k_knock is the
                 whole sequence between one pair of events, the host's round trip for the counts included) from a
                 second set of calls, with the byte / op model of DESIGN.md §Knock-out: GB/s against the 8 TB/s
                 HBM peak as bench.py computes it, folded child words per second, and k_ko_lds per (graph, chunk)
  k_proto        k_proto per graph from one analysis step in the same process, for scale (a kernel with one
                 workgroup per post graph and a Kahn-level loop of its own)
  host_ms        the baseline: tools/knockout_host_base.c on one thread (the same bit-parallel sweep, 64
                 hypotheses per word) over the first `--host-graphs` listed graphs; host_ms_all is its sweep time
                 scaled to all listed graphs by their hypotheses x edges
  ratio          host_ms_all / wall_ms
The device rows of those graphs are compared with the baseline's before anything is printed.  One JSON line.
Needs a GPU (no fallback).
"""
import argparse
import ctypes
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

HBM_PEAK_GBS = 8000.0  # as bench.py
GROUPS = ["k_knock", "k_ko_leaves", "k_ko_lds", "k_ko_glob"]


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=10000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-graphs", type=int, default=32)
    ap.add_argument("--lds-max", type=int, default=-1, help="option knock_lds_max (0: the global tier)")
    a = ap.parse_args()
    base = ctypes.CDLL(os.path.join(ROOT, "tools", "libknockbase.so"))
    vp, u64 = ctypes.c_void_p, ctypes.c_uint64
    base.knockout_host_rows.argtypes = [vp, vp, vp, vp, vp, vp, u64, vp, u64, vp, vp]
    base.knockout_host_rows.restype = ctypes.c_int
    corpus, _ = synth.generate(a.runs, prepend_run0=True, threads=min(16, os.cpu_count() or 1), **synth.CONFIGS["c3"])
    good = corpus.success_iters()
    graphs = np.ascontiguousarray([2 * corpus.run_index(x) + 1 for x in good], np.uint32)
    it = np.ascontiguousarray(good, np.uint32)
    eng = E.Engine(0)
    try:
        eng.set_option("knock_lds_max", a.lds_max)
        eng.load(corpus)
        # one analysis step, for k_proto per graph from the same process
        eng.set_timing(True)
        eng.set_timing_groups(["k_proto"])
        eng.mark()
        eng.simplify()
        eng.protos_partial(good, 0)
        eng.synchronize()
        proto = eng.timings().get("k_proto")
        eng.set_timing(False)
        for _ in range(a.warmup):
            rows = eng.knockout_leaves(good, 1)
        first, count = eng.knockout_ranges()
        wall = []
        for _ in range(a.steps):
            t0 = time.perf_counter()
            eng._chk(eng.L.nemo_knockout_leaves(eng.h, it.ctypes.data, len(it), 1, 0))
            wall.append(1e3 * (time.perf_counter() - t0))
        eng.set_timing(True)
        eng.set_timing_groups(GROUPS)
        eng.reset_timings()
        for _ in range(a.steps):
            eng._chk(eng.L.nemo_knockout_leaves(eng.h, it.ctypes.data, len(it), 1, 0))
        eng.synchronize()
        t = eng.timings()
        eng.set_timing(False)
    finally:
        eng.close()
    hg = min(a.host_graphs, len(graphs))
    n_host = int(count[:hg].sum())
    host_rows = np.zeros(max(n_host, 1), E.KNOCK_DTYPE)
    n_rows, secs = ctypes.c_uint64(), (ctypes.c_double * 2)()
    rc = base.knockout_host_rows(corpus.node_off.ctypes.data, corpus.edge_off.ctypes.data, corpus.node_word.ctypes.data,
                                 corpus.edge_src.ctypes.data, corpus.edge_dst.ctypes.data, graphs.ctypes.data, hg,
                                 host_rows.ctypes.data, n_host, ctypes.byref(n_rows), secs)
    assert rc == 0 and n_rows.value == n_host, (rc, n_rows.value, n_host)
    assert np.array_equal(host_rows[:n_host], rows[:n_host]), "host baseline and device rows differ"
    ne = (corpus.edge_off[graphs + 1] - corpus.edge_off[graphs]).astype(np.float64)
    chunks = (count.astype(np.int64) + 63) // 64
    work = chunks * ne  # a graph's sweep work: chunks x edges
    host_ms = 1e3 * (secs[0] + secs[1])
    host_all = 1e3 * (secs[1] * work.sum() / max(work[:hg].sum(), 1.0) + secs[0] * len(graphs) / max(hg, 1))
    wall_ms = statistics.median(wall)
    out = {"runs": corpus.n_runs, "graphs": len(graphs), "leaves_min_mean_max": [int(count.min()), round(float(count.mean()), 1),
                                                                                   int(count.max())],
           "hypotheses": int(count.sum()), "chunks": int(chunks.sum()), "lost": int(((rows["roots_dead"] == rows["n_roots"]) &
                                                                                     (rows["n_roots"] > 0)).sum()),
           "n_dead_mean": round(float(rows["n_dead"].astype(np.float64).mean()), 2), "steps": a.steps,
           "wall_ms": round(wall_ms, 3), "wall_ms_min_max": [round(min(wall), 3), round(max(wall), 3)],
           "host_graphs": hg, "host_ms": round(host_ms, 2), "host_sweep_ms": round(1e3 * secs[1], 2),
           "host_ms_all": round(host_all, 1), "ratio_host_over_wall": round(host_all / wall_ms, 1)}
    if proto and proto["launches"]:
        ms = proto["ms"] / proto["launches"]
        out["k_proto"] = {"ms": round(ms, 4), "us_per_graph": round(1e3 * ms / corpus.n_runs, 4)}
    for g in GROUPS:
        if g not in t or not t[g]["launches"]:
            continue
        ms, gb, ops = t[g]["ms"] / a.steps, t[g]["bytes"] / a.steps, t[g]["edges"] / a.steps
        row = {"ms_per_call": round(ms, 4), "bytes": gb, "gbs": round(gb / ms / 1e6, 1),
               "hbm_frac": round(gb / ms / 1e6 / HBM_PEAK_GBS, 4)}
        if ops:
            row["child_words_per_s"] = round(ops / ms * 1e3, 0)
        if g == "k_ko_lds":
            row["us_per_graph_chunk"] = round(1e3 * ms / max(int(chunks.sum()), 1), 4)
        out[g] = row
    print(json.dumps(out))


if __name__ == "__main__":
    main()
