#!/usr/bin/env python3
"""nemo_lineage_group_cuts beside nemo_min_group_cuts, on two inputs: the good runs of the 12-run C3-shaped corpus with
tools/group_cuts_bench.py's fault events over run 0's sink labels (omission groups of one label, nested crash-like
groups per location), and one case-study fixture with nemo_amd.faults.fault_events over its clock labels.  Per input
and max_size: the rows, the sets each level evaluates and the cuts it finds, both calls' wall time (a host clock around
the blocking call, median of --steps after --warmup) and, from a second set of calls with event timing on, the time of
the groups and of the kernels (nemo_timings).  The exhaustive call is run up to max_size 3 and must return the same
rows.  A level that ends in NEMO_ERR_LIMIT is recorded as it is.  One JSON line per (input, max_size).

  python tools/lineage_group_bench.py --steps 10 --warmup 2 --sizes 3,4,5,6
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from nemo_amd import engine as E  # noqa: E402
from nemo_amd.corpus import load_molly  # noqa: E402
from nemo_amd.faults import fault_events  # noqa: E402
from tools import synth  # noqa: E402
from tools.group_cuts_bench import make_groups  # noqa: E402

GROUPS = ["k_lgcuts", "k_lgc_lds", "k_lgc_glob", "k_lgc_cuts", "k_lin_filter", "k_lin_rehash", "k_gc_table", "k_gc_rows", "k_gcuts", "k_gc_lds",
          "k_gc_glob", "k_lc_reduce"]


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


def rows_of(rows):
    return [(int(r["size"]),) + tuple(int(x) for x in r["group"][:int(r["size"])]) for r in rows]


def measure(eng, name, its, groups, min_runs, sizes, steps, warmup):
    packed = (np.cumsum([0] + [len(g) for g in groups]).astype(np.uint64),
              np.ascontiguousarray([x for g in groups for x in g], dtype=np.uint32))
    for size in sizes:
        row = {"input": name, "runs_listed": len(its), "groups": len(groups), "labels_named": int(packed[0][-1]), "min_runs": min_runs,
               "max_size": size}
        try:
            rows, n_lost = eng.lineage_group_cuts(its, 1, packed, size, min_runs)
        except E.NemoError as e:  # a level past lineage_children_max: recorded, not worked round
            row["error"] = e.msg
            print(json.dumps(row), flush=True)
            continue
        st = eng.lineage_group_cut_stats()
        row["rows"] = len(rows)
        row["sets_per_level"] = [int(x) for x in st[:size + 1, 0]]
        row["cuts_per_level"] = [int(x) for x in st[:size + 1, 1]]
        row["lineage_group_cuts"] = timed(eng, lambda: eng.lineage_group_cuts(its, 1, packed, size, min_runs), steps, warmup)
        if size <= 3:
            ref, ref_lost = eng.min_group_cuts(its, 1, packed, size, min_runs)
            assert rows_of(ref) == rows_of(rows) and ref_lost.tolist() == n_lost.tolist(), "the two searches' rows differ"
            row["min_group_cuts_hypotheses"] = [int(x) for x in eng.min_group_cut_stats()[:size, 1]]
            row["min_group_cuts"] = timed(eng, lambda: eng.min_group_cuts(its, 1, packed, size, min_runs), steps, warmup)
        print(json.dumps(row), flush=True)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sizes", default="3,4,5,6")
    ap.add_argument("--min-runs", type=int, default=0, help="q (0: every listed run)")
    ap.add_argument("--cands", type=int, default=60, help="C3: omission groups of one label")
    ap.add_argument("--crash-labels", type=int, default=600)
    ap.add_argument("--locs", type=int, default=4)
    ap.add_argument("--times", type=int, default=5)
    ap.add_argument("--case", default="cs_pb_asynchronous", help="fixture under tests/golden")
    a = ap.parse_args()
    sizes = [int(x) for x in a.sizes.split(",")]
    eng = E.Engine(0)
    try:
        corpus, _ = synth.generate(12, prepend_run0=True, threads=min(16, os.cpu_count() or 1), **synth.CONFIGS["c3"])
        its = [int(x) for x in corpus.success_iters()]
        it0 = int(corpus.iteration[0])
        eng.load(corpus)
        leaves = eng.knockout_leaves([it0], 1).copy()
        n0 = int(corpus.node_off[2 * corpus.run_index(it0) + 1])
        labels = corpus.label[n0 + leaves["node"].astype(np.int64)]
        labels = np.ascontiguousarray(list(dict.fromkeys(labels.tolist())), dtype=np.uint32)
        groups = [g.tolist() for g in make_groups(labels, a.cands, a.crash_labels, a.locs, a.times)]
        for q in sorted({a.min_runs, 1}):
            measure(eng, "c3", its, groups, q, sizes, a.steps, a.warmup)
        d = os.path.join(ROOT, "tests", "golden", a.case)
        corpus = load_molly(d)
        runs = json.load(open(os.path.join(d, "runs.json")))
        spec = runs[0]["failureSpec"]
        good = [int(r["iteration"]) for r in runs if r["status"] == "success"]
        _, groups = fault_events(corpus.labels, spec["eot"], spec["eff"])
        eng.load(corpus)
        for q in sorted({a.min_runs, 1}):
            measure(eng, a.case, good, [list(g) for g in groups], q, sizes, a.steps, a.warmup)
    finally:
        eng.close()


if __name__ == "__main__":
    main()
