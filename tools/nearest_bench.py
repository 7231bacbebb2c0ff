#!/usr/bin/env python3
"""Time nemo_nearest_runs on the bench's C3 corpus, next to a host baseline in the same process.

The corpus is bench.py's C3 corpus (`--runs` runs of ~5k-node graphs, run 0 prepended); the failed runs are the
queries and the good runs the candidates.  Reported, per nemo_nearest_runs call:
  wall_ms        host clock around the call (it blocks until the rows are on the host), median of `--steps`
                 calls after `--warmup` calls, timing events off
  k_near*        HIP-event time per call of every kernel of the group (k_near_bits, k_near_isect, k_near_pick;
                 k_near is the whole sequence between one pair of events) from a second set of calls, with the
                 byte / op model of DESIGN.md §Nearest runs: GB/s against the 8 TB/s HBM peak as bench.py
                 computes it, and word pairs per second for k_near_isect.  k_near_lmax runs once per load and
                 is reported from the first call.
  host_ms        the baseline: tools/nearest_host_base.c on one thread (sorted distinct label lists per run, a
                 merge per pair, the argmin) for the first `--host-queries` queries against every candidate; one
                 call (it takes seconds); host_ms_all is that time scaled to all queries (the work is linear in
                 them: the per-run lists are built once and are under 1 % of it)
  ratio          host_ms_all / wall_ms
The device rows of those queries are compared with the baseline's before anything is printed.  --deep: a deep
corpus instead (few runs, long rows are made by spreading the label ids up to --spread).  One JSON line.
Needs a GPU (no fallback).
"""
import argparse
import ctypes
import dataclasses
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
GROUPS = ["k_near", "k_near_lmax", "k_near_bits", "k_near_isect", "k_near_pick"]


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=10000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-queries", type=int, default=32)
    ap.add_argument("--spread", type=int, default=0, help="move the label ids through l -> l * k so that the largest is about this")
    a = ap.parse_args()
    base = ctypes.CDLL(os.path.join(ROOT, "tools", "libnearbase.so"))
    base.nearest_host_rows.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p,
                                       ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p]
    base.nearest_host_rows.restype = ctypes.c_int
    corpus, _ = synth.generate(a.runs, prepend_run0=True, threads=min(16, os.cpu_count() or 1), **synth.CONFIGS["c3"])
    if a.spread:
        k = max(1, a.spread // (int(corpus.label.max()) + 1))
        corpus = dataclasses.replace(corpus, label=np.ascontiguousarray(corpus.label * np.uint32(k), dtype=np.uint32))
    queries, cands = corpus.failed_iters(), corpus.success_iters()
    goal = (corpus.node_word & np.uint32(0x80000000)) == 0
    post = np.zeros(len(goal), bool)
    for r in range(corpus.n_runs):
        post[int(corpus.node_off[2 * r + 1]):int(corpus.node_off[2 * r + 2])] = True
    lmax = int(corpus.label[goal & post].max())
    W = 2 * ((lmax + 1 + 127) // 128)
    n_q, n_c = len(queries), len(cands)
    eng = E.Engine(0)
    try:
        eng.load(corpus)
        eng.set_timing(True)
        eng.set_timing_groups(["k_near_lmax"])
        rows = eng.nearest_runs(queries, cands)  # the load's first call: k_near_lmax
        first = eng.timings().get("k_near_lmax")
        eng.set_timing(False)
        for _ in range(a.warmup):
            rows = eng.nearest_runs(queries, cands)
        qa, ca = np.ascontiguousarray(queries, np.uint32), np.ascontiguousarray(cands, np.uint32)
        wall = []
        for _ in range(a.steps):
            t0 = time.perf_counter()
            eng._chk(eng.L.nemo_nearest_runs(eng.h, qa.ctypes.data, n_q, ca.ctypes.data, n_c))
            wall.append(1e3 * (time.perf_counter() - t0))
        eng.set_timing(True)
        eng.set_timing_groups(GROUPS)
        eng.reset_timings()
        for _ in range(a.steps):
            eng._chk(eng.L.nemo_nearest_runs(eng.h, qa.ctypes.data, n_q, ca.ctypes.data, n_c))
        eng.synchronize()
        t = eng.timings()
        eng.set_timing(False)
    finally:
        eng.close()
    hq = min(a.host_queries, n_q)
    q_run = np.ascontiguousarray([corpus.run_index(x) for x in queries[:hq]], np.uint32)
    c_run = np.ascontiguousarray([corpus.run_index(x) for x in cands], np.uint32)
    host_rows = np.zeros(max(hq, 1), E.NEAREST_DTYPE)
    t0 = time.perf_counter()
    rc = base.nearest_host_rows(corpus.node_off.ctypes.data, corpus.node_word.ctypes.data, corpus.label.ctypes.data,
                                corpus.n_runs, q_run.ctypes.data, hq, c_run.ctypes.data, n_c, host_rows.ctypes.data)
    host_ms = 1e3 * (time.perf_counter() - t0)
    assert rc == 0 and np.array_equal(host_rows[:hq], rows[:hq]), "host baseline and device rows differ"
    wall_ms = statistics.median(wall)
    host_all = host_ms * n_q / max(hq, 1)
    rows_n = len(set(queries) | set(cands))
    out = {"runs": corpus.n_runs, "queries": n_q, "candidates": n_c, "lmax": lmax, "W": W,
           "bit_matrix_bytes": rows_n * W * 8, "matrix_bytes": 4 * n_q * n_c, "word_pairs": n_q * n_c * W,
           "steps": a.steps, "wall_ms": round(wall_ms, 4), "wall_ms_min_max": [round(min(wall), 4), round(max(wall), 4)],
           "host_queries": hq, "host_ms": round(host_ms, 2), "host_ms_all": round(host_all, 1),
           "ratio_host_over_wall": round(host_all / wall_ms, 1),
           "dist_mean": float(rows["dist"].astype(np.float64).mean()), "dist_zero": int((rows["dist"] == 0).sum())}
    if first and first["launches"]:
        ms, gb = first["ms"] / first["launches"], first["bytes"] / first["launches"]
        out["k_near_lmax"] = {"ms": round(ms, 4), "bytes": gb, "gbs": round(gb / ms / 1e6, 1)}
    for g in GROUPS:
        if g == "k_near_lmax" or g not in t or not t[g]["launches"]:
            continue
        ms, gb, ops = t[g]["ms"] / a.steps, t[g]["bytes"] / a.steps, t[g]["edges"] / a.steps
        row = {"ms_per_call": round(ms, 4), "bytes": gb, "gbs": round(gb / ms / 1e6, 1),
               "hbm_frac": round(gb / ms / 1e6 / HBM_PEAK_GBS, 4)}
        if ops:
            row["word_pairs_per_s"] = round(ops / ms * 1e3, 0)
        out[g] = row
    print(json.dumps(out))


if __name__ == "__main__":
    main()
