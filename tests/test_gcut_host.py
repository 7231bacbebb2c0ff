"""Host-side checks of the minimal cut sets over fault events (no GPU): the C ABI declares and exports
nemo_min_group_cuts and its two fetches, the Python and Go bindings call them as declared, the semantics, the error
codes and the limits are documented, the host arithmetic (nemo_amd/csrc/gcut_host.h: the group check, the distinct
labels, the table and region sizes) passes its stand-alone check program under the host sanitizers, and
nemo_amd.faults.fault_events turns clock labels into Molly's fault events and their label groups."""
import ctypes
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from nemo_amd import engine as E
from nemo_amd.faults import fault_events, parse_clock
from tests.test_go_binding import go_calls, header_decls

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GO = os.path.join(ROOT, "go", "graphing", "nemohip.go")
CALLS = {"nemo_min_group_cuts": 10, "nemo_fetch_min_group_cuts": 5, "nemo_fetch_min_group_cut_stats": 2}


def test_header_declares_the_calls():
    funcs, defines, _, _ = header_decls()
    for name, arity in CALLS.items():
        assert name in E.header_symbols()
        assert funcs[name] == arity, name
    txt = open(E.HEADER).read()
    assert "#define NEMOHIP_ABI_VERSION 1" in txt  # additive
    start = txt.index("minimal cut sets over fault events: groups of labels as candidates")
    assert txt.index("int nemo_fetch_min_label_cut_stats") < start < txt.index("corrections / extensions on run 0")
    doc = txt[start:txt.index("int nemo_fetch_min_group_cut_stats")]
    for name in ("NEMO_ERR_NOTFOUND", "NEMO_ERR_STATE", "NEMO_ERR_LIMIT", "NEMO_ERR_INVALID", "roots_dead == n_roots > 0",
                 "NEMO_KL_SINKS", "listed twice", "shorten\n * the group list or the run list", "UINT32_MAX", "2^28", "2^32 - 2",
                 "2^32 - 1 labels", "2^24 labels in one group", "D + 1 + V <= 2^32 - 1", "min_runs", "0\n * means n",
                 "max_size must be 1, 2 or 3", "no implicit event list", "live list",
                 "group_labels[group_off[k] .. group_off[k+1])", "union of G_k", "goal or rule", "only sink goals",
                 "over candidate positions, not over label sets", "equal or nested groups are different candidates",
                 "each is a row", "pair of nested groups is never a minimal cut", "follows from monotonicity",
                 "empty group is legal", "named twice in a group counts once", "no listed node\n * carries matches nothing",
                 "hit at least one listed\n * graph", "C(K1,2)", "C(K1,3)", "colex rank", "(size, rank)", "n_lost[k]",
                 "candidate positions", "ascending", "without roots is never lost", "n == 0 or n_groups == 0",
                 "before that round's launch", "leaves no results", "blocks until\n * the rows are on the host", "knock_lds_max",
                 "kl_grid", "cond outside\n * 0 / 1", "unknown flags", "decreasing group_off", "group_off == NULL",
                 "group_labels == NULL", "node context", "without a loaded corpus", "before anything is uploaded",
                 "next nemo_min_group_cuts or nemo_load_corpus", "in both directions"):
        assert name in doc, name
    struct = re.search(r"typedef struct nemo_group_cut \{(.*?)\} nemo_group_cut;", txt, flags=re.S)
    assert struct and "uint32_t size;" in struct.group(1) and "uint32_t group[3];" in struct.group(1)
    opts = txt[txt.index("Tuning / test knobs"):txt.index("int nemo_set_option")]
    assert opts.count("nemo_min_group_cuts") >= 2  # under knock_lds_max and under kl_grid
    assert E.GROUP_CUT_DTYPE.itemsize == 16 and E.GROUP_CUT_DTYPE.names == ("size", "group")


def test_library_exports_the_calls():
    if not os.path.exists(E.LIB_PATH):
        subprocess.run(["make", "-s", "-C", ROOT, "nemo_amd/libnemohip.so"], check=True)
    L = ctypes.CDLL(E.LIB_PATH)
    for name in CALLS:
        assert hasattr(L, name), name
    assert L.nemo_abi_version() == 1
    vp, u32, u64, sz = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_size_t
    L.nemo_min_group_cuts.argtypes = [vp, vp, sz, ctypes.c_int, vp, vp, sz, u32, u32, u32]
    assert L.nemo_min_group_cuts(None, None, 0, 1, None, None, 0, 2, 0, 0) == 1  # NEMO_ERR_INVALID: a null context, no device
    L.nemo_fetch_min_group_cuts.argtypes = [vp, vp, vp, u64, vp]
    assert L.nemo_fetch_min_group_cuts(None, None, None, 0, None) == 1
    L.nemo_fetch_min_group_cut_stats.argtypes = [vp, vp]
    out = np.zeros(9, np.uint64)
    assert L.nemo_fetch_min_group_cut_stats(None, out.ctypes.data) == 1


def test_engine_binds_the_calls():
    for name, arity in CALLS.items():
        fn = getattr(E.lib(), name)
        assert len(fn.argtypes) == arity and fn.restype is ctypes.c_int, name
    sig = inspect.signature(E.Engine.min_group_cuts)
    assert list(sig.parameters) == ["self", "iters", "cond", "groups", "max_size", "min_runs", "sinks_only"]
    assert sig.parameters["max_size"].default == 2 and sig.parameters["min_runs"].default == 0
    assert sig.parameters["sinks_only"].default is False
    assert list(inspect.signature(E.Engine.min_group_cut_rows).parameters) == ["self"]
    assert list(inspect.signature(E.Engine.min_group_cut_stats).parameters) == ["self"]


def test_go_binding_calls_them_as_declared():
    src = open(GO).read()
    funcs, defines, _, _ = header_decls()
    calls = {}
    for name, n in go_calls(src):
        calls.setdefault(name, set()).add(n)
    for name in CALLS:
        assert f"C.{name}(" in src, name
        assert calls[name] == {funcs[name]} == {CALLS[name]}, name
    m = re.search(r"func \(n \*Neo4J\) MinGroupCuts\(.*?\n}\n", src, flags=re.S)
    assert m, "no MinGroupCuts helper"
    for name in CALLS:
        assert f"C.{name}(" in m.group(0), name
    assert "C.NEMO_KL_SINKS" in m.group(0) and "C.nemo_group_cut" in m.group(0)


def test_host_check_program_passes_under_the_host_sanitizers(tmp_path):
    src = os.path.join(ROOT, "tools", "gcut_host_check.cpp")
    text = open(src).read()
    assert "int main()" in text and '#include "../nemo_amd/csrc/gcut_host.h"' in text
    hdr = open(os.path.join(ROOT, "nemo_amd", "csrc", "gcut_host.h")).read()
    assert "hip_runtime" not in hdr  # pure host functions
    for inc in ('#include "cut_host.h"', '#include "klabel_host.h"', '#include "lcut_host.h"'):  # reused, not copied
        assert inc in hdr, inc
    assert "klabel::check_offsets" in hdr and "klabel::table_slots" in hdr and "lcuts::region_words" in hdr
    mk = open(os.path.join(ROOT, "tools", "Makefile")).read()
    assert "-fsanitize=address,undefined" in mk and "gcut_host_check.cpp" in mk
    if shutil.which("g++") is None and shutil.which("c++") is None:
        pytest.fail("no host C++ compiler to build tools/gcut_host_check.cpp")
    exe = str(tmp_path / "gcut_host_check")
    # tools/Makefile's rule, the binary in the test's own folder; the sanitizer runtimes are linked into the
    # program itself: it runs as it is, whatever else the loader brings
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tools"), "-B", "gcut_host_check", f"GCUT_CHECK={exe}"], check=True)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    assert run.stdout.rstrip().endswith("gcut_host_check OK")


def test_fault_events_on_a_hand_written_label_list():
    """two nodes a and b, eot 3, eff 2: a message on either side of eff, a self-send, a wildcard clock, a non-clock"""
    labels = ["clock(a, b, 1, 2)",            # 0: an omission (1 < eff)
              "clock(a, a, 2, __WILDCARD__)",  # 1: a's own clock at 2: sender only
              "clock(b, a, 2, 3)",            # 2: at eff: no omission
              "log(b, hello)",                # 3: no clock goal
              "clock(b, b, 1, 2)",            # 4: a self-send: no omission; b sends at 1 and receives at 2
              "clock(b, a, 1, 2)"]            # 5: an omission
    assert parse_clock(labels[0]) == ("a", "b", 1, False) and parse_clock(labels[1]) == ("a", "a", 2, True)
    assert parse_clock(labels[3]) is None and parse_clock("clock(a, b, x, 2)") is None and parse_clock("clock(a, b, 1)") is None
    events, groups = fault_events(labels, 3, 2)
    assert events == [("omit", "a", "b", 1), ("omit", "b", "a", 1),
                      ("crash", "a", None, 1), ("crash", "a", None, 2), ("crash", "a", None, 3),
                      ("crash", "b", None, 1), ("crash", "b", None, 2), ("crash", "b", None, 3)]
    assert groups == [[0], [5],
                      [0, 1, 2, 5],  # a from 1 on: sends 0 (at 1) and 1 (at 2); receives 2 (sent at 2) and 5 (sent at 1, arrives at 2)
                      [1, 2, 5],     # a from 2 on: sends 1; receives 2 and 5 (5 arrives at 2); no longer sends 0
                      [2],           # a from 3 on: receives 2 (arrives at 3)
                      [0, 2, 4, 5],  # b from 1 on: sends 2, 4, 5; receives 0 and 4
                      [0, 2, 4],     # b from 2 on: sends 2; receives 0 and 4 (both arrive at 2)
                      []]            # b from 3 on: nothing left; the event keeps its position
    # the order does not depend on the labels' order, the ids do
    ev2, gr2 = fault_events(labels[::-1], 3, 2)
    assert ev2 == events and gr2 == [sorted(5 - x for x in g) for g in groups]
    assert fault_events([], 3, 2) == ([], []) and fault_events(["log(a)"], 3, 2) == ([], [])
    doc = fault_events.__doc__
    assert "caller's filter" in doc and "every subset of a set within\n    the budget is within the budget" in doc
