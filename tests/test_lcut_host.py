"""Host-side checks of the minimal cut sets by label (no GPU): the C ABI declares and exports nemo_min_label_cuts and
its two fetches, the Python and Go bindings call them as declared, the semantics, the error codes and the limits are
documented, and the host arithmetic (nemo_amd/csrc/lcut_host.h: the candidate check, the min_runs rule, the rounds'
limits, the live list, the table and region sizes) passes its stand-alone check program under the host sanitizers."""
import ctypes
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from nemo_amd import engine as E
from tests.test_go_binding import go_calls, header_decls

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GO = os.path.join(ROOT, "go", "graphing", "nemohip.go")
CALLS = {"nemo_min_label_cuts": 9, "nemo_fetch_min_label_cuts": 5, "nemo_fetch_min_label_cut_stats": 2}


def test_header_declares_the_calls():
    funcs, defines, _, _ = header_decls()
    for name, arity in CALLS.items():
        assert name in E.header_symbols()
        assert funcs[name] == arity, name
    txt = open(E.HEADER).read()
    assert "#define NEMOHIP_ABI_VERSION 1" in txt  # additive
    start = txt.index("minimal cut sets by label: the smallest fault sets that defeat every listed run")
    assert txt.index("int nemo_fetch_knockout_label_counts") < start < txt.index("corrections / extensions on run 0")
    doc = txt[start:txt.index("int nemo_fetch_min_label_cut_stats")]
    for name in ("NEMO_ERR_NOTFOUND", "NEMO_ERR_STATE", "NEMO_ERR_LIMIT", "NEMO_ERR_INVALID", "roots_dead == n_roots > 0",
                 "NEMO_KL_SINKS", "listed twice", "shorten the candidate list or the run list", "UINT32_MAX", "2^28", "2^32 - 2",
                 "min_runs", "0\n * means n", "max_size must be 1, 2 or 3", "no implicit list", "distinct", "live list",
                 "hit at least one listed graph", "C(K1,2)", "C(K1,3)", "colex rank", "(size, rank)", "n_lost[k]",
                 "without roots is never lost", "n == 0 or n_cand == 0", "before that round's launch", "leaves no results",
                 "blocks until the rows are on the host", "knock_lds_max", "kl_grid", "cond outside 0 / 1", "unknown flags",
                 "node context", "without a loaded corpus"):
        assert name in doc, name
    struct = re.search(r"typedef struct nemo_label_cut \{(.*?)\} nemo_label_cut;", txt, flags=re.S)
    assert struct and "uint32_t size;" in struct.group(1) and "uint32_t label[3];" in struct.group(1)
    opts = txt[txt.index("Tuning / test knobs"):txt.index("int nemo_set_option")]
    assert opts.count("nemo_min_label_cuts") >= 2  # under knock_lds_max and under kl_grid
    assert E.LABEL_CUT_DTYPE.itemsize == 16 and E.LABEL_CUT_DTYPE.names == ("size", "label")


def test_library_exports_the_calls():
    if not os.path.exists(E.LIB_PATH):
        subprocess.run(["make", "-s", "-C", ROOT, "nemo_amd/libnemohip.so"], check=True)
    L = ctypes.CDLL(E.LIB_PATH)
    for name in CALLS:
        assert hasattr(L, name), name
    assert L.nemo_abi_version() == 1
    vp, u32, u64, sz = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_size_t
    L.nemo_min_label_cuts.argtypes = [vp, vp, sz, ctypes.c_int, vp, sz, u32, u32, u32]
    assert L.nemo_min_label_cuts(None, None, 0, 1, None, 0, 2, 0, 0) == 1  # NEMO_ERR_INVALID: a null context, no device
    L.nemo_fetch_min_label_cuts.argtypes = [vp, vp, vp, u64, vp]
    assert L.nemo_fetch_min_label_cuts(None, None, None, 0, None) == 1
    L.nemo_fetch_min_label_cut_stats.argtypes = [vp, vp]
    out = np.zeros(9, np.uint64)
    assert L.nemo_fetch_min_label_cut_stats(None, out.ctypes.data) == 1


def test_engine_binds_the_calls():
    for name, arity in CALLS.items():
        fn = getattr(E.lib(), name)
        assert len(fn.argtypes) == arity and fn.restype is ctypes.c_int, name
    sig = inspect.signature(E.Engine.min_label_cuts)
    assert list(sig.parameters) == ["self", "iters", "cond", "cand_labels", "max_size", "min_runs", "sinks_only"]
    assert sig.parameters["max_size"].default == 2 and sig.parameters["min_runs"].default == 0
    assert sig.parameters["sinks_only"].default is False
    assert list(inspect.signature(E.Engine.min_label_cut_rows).parameters) == ["self"]
    assert list(inspect.signature(E.Engine.min_label_cut_stats).parameters) == ["self"]


def test_go_binding_calls_them_as_declared():
    src = open(GO).read()
    funcs, defines, _, _ = header_decls()
    calls = {}
    for name, n in go_calls(src):
        calls.setdefault(name, set()).add(n)
    for name in CALLS:
        assert f"C.{name}(" in src, name
        assert calls[name] == {funcs[name]} == {CALLS[name]}, name
    m = re.search(r"func \(n \*Neo4J\) MinLabelCuts\(.*?\n}\n", src, flags=re.S)
    assert m, "no MinLabelCuts helper"
    for name in CALLS:
        assert f"C.{name}(" in m.group(0), name
    assert "C.NEMO_KL_SINKS" in m.group(0) and "C.nemo_label_cut" in m.group(0)


def test_host_check_program_passes_under_the_host_sanitizers(tmp_path):
    src = os.path.join(ROOT, "tools", "lcut_host_check.cpp")
    text = open(src).read()
    assert "int main()" in text and '#include "../nemo_amd/csrc/lcut_host.h"' in text
    hdr = open(os.path.join(ROOT, "nemo_amd", "csrc", "lcut_host.h")).read()
    assert "hip_runtime" not in hdr  # pure host functions
    assert '#include "cut_host.h"' in hdr and '#include "klabel_host.h"' in hdr  # reused, not copied
    assert "cuts::check_cands" in hdr and "cuts::round_hyps" in hdr and "klabel::table_slots" in hdr
    mk = open(os.path.join(ROOT, "tools", "Makefile")).read()
    assert "-fsanitize=address,undefined" in mk and "lcut_host_check.cpp" in mk
    if shutil.which("g++") is None and shutil.which("c++") is None:
        pytest.fail("no host C++ compiler to build tools/lcut_host_check.cpp")
    exe = str(tmp_path / "lcut_host_check")
    # tools/Makefile's rule, the binary in the test's own folder; the sanitizer runtimes are linked into the
    # program itself: it runs as it is, whatever else the loader brings
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tools"), "-B", "lcut_host_check", f"LCUT_CHECK={exe}"], check=True)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    assert run.stdout.rstrip().endswith("lcut_host_check OK")
