"""The hand-over's timeline from a rocprofv3 run with --kernel-trace --memory-copy-trace (csv): for every
step of the trace (from one k_build launch to the next), the start and end of the hand-over's kernels and
copies and of the last analysis kernel relative to k_build's start, the copies' rates, and the link's idle
time between the first hand-over copy's start and the last one's end.  Then the whole merged timeline of
the second-to-last step, and the per-launch durations of the kernels that run beside the copies.
The runtime's D2H copies to pinned memory show up as its blit kernel (__amd_rocclr_copyBuffer) in the kernel
trace, not in the copy trace: launches of it of at least MIN_US count as the bulk copies, as many of them as the
step has k_pack_state launches as the node state's, the rest as the pairs'; given the two byte counts, each
half's rate is printed.
usage: python tools/handover_timeline.py DIR [STATE_BYTES PAIRS_BYTES [MIN_US]]"""
import csv
import glob
import os
import statistics
import sys

d = sys.argv[1]
state_bytes = int(sys.argv[2]) if len(sys.argv) > 3 else 0
pairs_bytes = int(sys.argv[3]) if len(sys.argv) > 3 else 0
min_us = float(sys.argv[4]) if len(sys.argv) > 4 else 20.0
min_bytes = 1 << 20


def find(suffix):
    hits = sorted(glob.glob(os.path.join(d, "**", "*" + suffix), recursive=True))
    if not hits:
        sys.exit(f"no *{suffix} under {d}")
    return hits[-1]


ev = []  # (start, end, kind, name, bytes, queue)
for r in csv.DictReader(open(find("kernel_trace.csv"))):
    name = r["Kernel_Name"].split("(")[0].replace("void ", "").replace("nemo::", "")
    ev.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), "k", name, 0, r.get("Queue_Id", "")))
for r in csv.DictReader(open(find("memory_copy_trace.csv"))):
    ev.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), "c", r.get("Direction", "copy"),
               int(r.get("Size", 0) or 0), ""))
ev.sort()
builds = [i for i, e in enumerate(ev) if e[2] == "k" and e[3].startswith("k_build")]
if len(builds) < 3:
    sys.exit("fewer than three k_build launches in the trace")

HAND = ("k_pack_state", "k_scan64", "k_chain_pairs")
BESIDE = ("k_proto_lds", "k_chains", "k_pull_lds")


def is_bulk(e):  # a hand-over copy: the blit kernel, or a traced copy device to host of at least min_bytes
    if e[2] == "k":
        return "copyBuffer" in e[3] and e[1] - e[0] >= min_us * 1e3
    return e[4] >= min_bytes and "HOST" in e[3].upper().split("TO")[-1]


def us(x):
    return x / 1e3


print("per step, us from k_build's start: first start / last end (launches or copies)")
print(f"{'step':>4} {'len':>7} | {'pack_state':>18} | {'scan64':>16} | {'chain_pairs':>18} | {'bulk D2H':>18} "
      f"| {'GB/s each':>22} | {'idle':>6} | last analysis kernel")
idles, lens, rate_log = [], [], []
beside = {k: [] for k in BESIDE}
for n, (a, b) in enumerate(zip(builds[:-1], builds[1:])):
    t0 = ev[a][0]
    step = ev[a:b]
    cols = []
    for h in HAND:
        xs = [e for e in step if e[2] == "k" and e[3].startswith(h)]
        cols.append(f"{us(xs[0][0] - t0):7.1f}/{us(max(e[1] for e in xs) - t0):7.1f} ({len(xs)})" if xs else "-")
    cp = [e for e in step if is_bulk(e)]
    if cp:
        first, last = cp[0][0], max(e[1] for e in cp)
        busy, edge = 0, first
        for e in cp:  # the union of the copies' intervals
            if e[1] > edge:
                busy += e[1] - max(e[0], edge)
                edge = e[1]
        idle = us(last - first - busy)
        idles.append(idle)
        half = sum(1 for e in step if e[2] == "k" and e[3].startswith("k_pack_state"))  # one state copy per launch
        # GB/s of the state's copies, then of the pairs': bytes over the copies' own durations
        if state_bytes and 0 < half < len(cp):
            rates = (f"{state_bytes / sum(e[1] - e[0] for e in cp[:half]):.1f} "
                     f"{pairs_bytes / sum(e[1] - e[0] for e in cp[half:]):.1f}")
            rate_log.append((state_bytes / sum(e[1] - e[0] for e in cp[:half]),
                             pairs_bytes / sum(e[1] - e[0] for e in cp[half:])))
        else:
            rates = " ".join(f"{e[4] / max(e[1] - e[0], 1):.1f}" for e in cp[:8] if e[4]) or "-"
        ccol = f"{us(first - t0):7.1f}/{us(last - t0):7.1f} ({len(cp)})"
    else:
        idle, rates, ccol = 0.0, "-", "-"
    ana = [e for e in step if e[2] == "k" and not e[3].startswith(HAND) and "to_host" not in e[3]
           and "copyBuffer" not in e[3] and not e[3].startswith("k_zero")]
    la = max(ana, key=lambda e: e[1])
    lens.append(us(ev[b][0] - t0))
    print(f"{n:4d} {lens[-1]:7.1f} | {cols[0]:>18} | {cols[1]:>16} | {cols[2]:>18} | {ccol:>18} | {rates:>22} | "
          f"{idle:6.1f} | {la[3][:24]} ends {us(la[1] - t0):.1f}")
    if not cp:
        continue  # a step without a hand-over (the load's)
    for k in BESIDE:  # the step's longest launch of each: the LDS-tier k_chains, the simplified pull
        xs = [us(e[1] - e[0]) for e in step if e[2] == "k" and e[3].startswith(k)]
        if xs:
            beside[k].append(max(xs))
print(f"median step {statistics.median(lens):.1f} us, median link idle inside the hand-over "
      f"{statistics.median(idles) if idles else 0:.1f} us")
if rate_log:
    print(f"median GB/s of the copies' own durations: state {statistics.median(r[0] for r in rate_log):.1f}, "
          f"pairs {statistics.median(r[1] for r in rate_log):.1f}")
for k, v in beside.items():
    if v:
        print(f"{k} (the step's longest launch): {len(v)} steps, median {statistics.median(v):.1f} us, "
              f"mean {statistics.mean(v):.1f} us, max {max(v):.1f} us")

a, b = builds[-3], builds[-2]
t0 = ev[a][0]
print(f"\nthe second-to-last step, every kernel and copy (start us, duration us, queue, name, bytes)")
for e in ev[a:b]:
    print(f"{us(e[0] - t0):9.1f} {us(e[1] - e[0]):9.1f} {e[5]:>3} {e[3][:60]}{'  %d B' % e[4] if e[2] == 'c' else ''}")
