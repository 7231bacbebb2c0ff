#!/usr/bin/env python3
"""Time nemo_diff_classes on the bench's C3 corpus in per-run mode, next to a host baseline in the same
process.

The corpus is bench.py's C3 corpus (`--runs` runs of ~5k-node graphs, run 0 prepended); every failed run is
one entry of one per-run nemo_diffprov.  Reported, per nemo_diff_classes call:
  wall_ms        host clock around the call (it blocks until the classes are known), median of `--steps`
                 calls after `--warmup` calls, timing events off
  k_dclass_ms    HIP-event time of the k_dclass group (hash + compare launches) from a second set of calls
  host_ms        the baseline: the same partition computed on one host thread from nemo_diff_masks_view
                 (the pinned masks nemo_diffprov already copied) by tools/dclass_host_base.c, hash buckets
                 and memcmp; median of the same number of calls.  The D2H copy of the masks is not in it.
  ratio          host_ms / wall_ms
The two partitions are compared before anything is printed.  One JSON line.  Needs a GPU (no fallback).
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
from nemo_amd.corpus import DIFF_PER_RUN  # noqa: E402
from tools import synth  # noqa: E402

HBM_PEAK_GBS = 8000.0  # as bench.py


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=10000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    base = ctypes.CDLL(os.path.join(ROOT, "tools", "libdclassbase.so"))
    base.dclass_host_partition.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_void_p]
    base.dclass_host_partition.restype = ctypes.c_uint32
    corpus, _ = synth.generate(a.runs, prepend_run0=True, threads=min(16, os.cpu_count() or 1), **synth.CONFIGS["c3"])
    failed = corpus.failed_iters()
    eng = E.Engine(0)
    try:
        eng.load(corpus)
        eng.mark()
        eng.diffprov(failed, DIFF_PER_RUN)
        masks = eng.diff_masks_view()  # waits for the diff and its mask copy
        n, v0 = masks.shape
        for _ in range(a.warmup):
            class_of, classes = eng.diff_classes()
        wall = []
        for _ in range(a.steps):
            t0 = time.perf_counter()
            eng._chk(eng.L.nemo_diff_classes(eng.h))
            wall.append(1e3 * (time.perf_counter() - t0))
        eng.set_timing(True)
        eng.set_timing_groups(["k_dclass"])
        eng.reset_timings()
        for _ in range(a.steps):
            eng._chk(eng.L.nemo_diff_classes(eng.h))
        eng.synchronize()
        t = eng.timings().get("k_dclass")
        eng.set_timing(False)
        host_of = np.zeros(max(n, 1), np.uint32)
        host = []
        for _ in range(a.warmup + a.steps):
            t0 = time.perf_counter()
            k = base.dclass_host_partition(masks.ctypes.data, n, v0, host_of.ctypes.data)
            host.append(1e3 * (time.perf_counter() - t0))
        host = host[a.warmup:]
        assert k == len(classes) and np.array_equal(host_of[:n], class_of), "host baseline and device classes differ"
    finally:
        eng.close()
    wall_ms, host_ms = statistics.median(wall), statistics.median(host)
    out = {"runs": corpus.n_runs, "entries": int(n), "v0": int(v0), "mask_bytes": int(n) * int(v0),
           "classes": int(len(classes)), "largest_class": int(classes[:, 1].max()) if len(classes) else 0,
           "steps": a.steps, "wall_ms": round(wall_ms, 4), "wall_ms_min_max": [round(min(wall), 4), round(max(wall), 4)],
           "host_ms": round(host_ms, 4), "host_ms_min_max": [round(min(host), 4), round(max(host), 4)],
           "ratio_host_over_wall": round(host_ms / wall_ms, 2)}
    if t and t["launches"]:
        calls = a.steps
        ms, gb = t["ms"] / calls, t["bytes"] / calls
        out["k_dclass"] = {"ms_per_call": round(ms, 4), "launches_per_call": t["launches"] / calls, "bytes": gb,
                           "gbs": round(gb / ms / 1e6, 1), "hbm_frac": round(gb / ms / 1e6 / HBM_PEAK_GBS, 4)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
