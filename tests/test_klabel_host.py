"""Host-side checks of the knock-out by label (no GPU): the C ABI declares and exports nemo_knockout_labels and its
two fetches, the Python and Go bindings call them as declared, the option and the error codes are documented, and
the host arithmetic (nemo_amd/csrc/klabel_host.h: the validation and the two limits, the table sizes and offsets, the
hash, the work items and the grid) passes its stand-alone check program under the host sanitizers."""
import ctypes
import inspect
import os
import re
import shutil
import subprocess

import pytest

from nemo_amd import engine as E
from tests.test_go_binding import go_calls, header_decls

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GO = os.path.join(ROOT, "go", "graphing", "nemohip.go")
CALLS = {"nemo_knockout_labels": 8, "nemo_fetch_knockout_labels": 4, "nemo_fetch_knockout_label_counts": 4}


def test_header_declares_the_calls():
    funcs, defines, _, _ = header_decls()
    for name, arity in CALLS.items():
        assert name in E.header_symbols()
        assert funcs[name] == arity, name
    assert "NEMO_KL_SINKS" in defines
    txt = open(E.HEADER).read()
    assert "#define NEMOHIP_ABI_VERSION 1" in txt  # additive
    assert "#define NEMO_KL_SINKS 1u" in txt
    start = txt.index("knock-out by label: fault sets tested against every listed run")
    assert txt.index("int nemo_fetch_min_cut_stats") < start  # after the minimal-cut block
    doc = txt[start:txt.index("int nemo_fetch_knockout_label_counts")]
    for name in ("NEMO_ERR_NOTFOUND", "NEMO_ERR_STATE", "NEMO_ERR_LIMIT", "NEMO_ERR_INVALID", "roots_dead == n_roots > 0",
                 "NEMO_KL_SINKS", "listed twice", "tile the", "UINT32_MAX", "decreasing set_off", "2^28", "2^32 - 1",
                 "named twice", "non-empty", "ceil(n_sets / 64)", "sink goals"):
        assert name in doc, name
    opts = txt[txt.index("Tuning / test knobs"):txt.index("int nemo_set_option")]
    assert '"kl_grid"' in opts and '"cut_grid"' in opts and '"kl_hitlist"' in opts
    assert "more than 2^32 - 1 sets" in doc


def test_library_exports_the_calls():
    if not os.path.exists(E.LIB_PATH):
        subprocess.run(["make", "-s", "-C", ROOT, "nemo_amd/libnemohip.so"], check=True)
    L = ctypes.CDLL(E.LIB_PATH)
    for name in CALLS:
        assert hasattr(L, name), name
    assert L.nemo_abi_version() == 1
    vp, u32, u64, sz = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_size_t
    L.nemo_knockout_labels.argtypes = [vp, vp, sz, ctypes.c_int, vp, vp, sz, u32]
    assert L.nemo_knockout_labels(None, None, 0, 1, None, None, 0, 0) == 1  # NEMO_ERR_INVALID: a null context, no device
    L.nemo_fetch_knockout_labels.argtypes = [vp, vp, vp, u64]
    assert L.nemo_fetch_knockout_labels(None, None, None, 0) == 1
    L.nemo_fetch_knockout_label_counts.argtypes = [vp, vp, vp, u64]
    assert L.nemo_fetch_knockout_label_counts(None, None, None, 0) == 1


def test_engine_binds_the_calls():
    for name, arity in CALLS.items():
        fn = getattr(E.lib(), name)
        assert len(fn.argtypes) == arity and fn.restype is ctypes.c_int, name
    sig = inspect.signature(E.Engine.knockout_labels)
    assert list(sig.parameters) == ["self", "iters", "cond", "sets", "sinks_only"]
    assert sig.parameters["sinks_only"].default is False
    assert list(inspect.signature(E.Engine.knockout_label_counts).parameters) == ["self"]
    assert E.KL_SINKS == 1


def test_go_binding_calls_them_as_declared():
    src = open(GO).read()
    funcs, defines, _, _ = header_decls()
    calls = {}
    for name, n in go_calls(src):
        calls.setdefault(name, set()).add(n)
    for name in CALLS:
        assert f"C.{name}(" in src, name
        assert calls[name] == {funcs[name]} == {CALLS[name]}, name
    m = re.search(r"func \(n \*Neo4J\) KnockoutLabels\(.*?\n}\n", src, flags=re.S)
    assert m, "no KnockoutLabels helper"
    for name in CALLS:
        assert f"C.{name}(" in m.group(0), name
    assert "C.NEMO_KL_SINKS" in m.group(0) and "NEMO_KL_SINKS" in defines


def test_host_check_program_passes_under_the_host_sanitizers(tmp_path):
    src = os.path.join(ROOT, "tools", "klabel_host_check.cpp")
    text = open(src).read()
    assert "int main()" in text and '#include "../nemo_amd/csrc/klabel_host.h"' in text
    hdr = open(os.path.join(ROOT, "nemo_amd", "csrc", "klabel_host.h")).read()
    assert "hip_runtime" not in hdr  # pure host functions
    mk = open(os.path.join(ROOT, "tools", "Makefile")).read()
    assert "-fsanitize=address,undefined" in mk and "klabel_host_check.cpp" in mk
    if shutil.which("g++") is None and shutil.which("c++") is None:
        pytest.fail("no host C++ compiler to build tools/klabel_host_check.cpp")
    exe = str(tmp_path / "klabel_host_check")
    # tools/Makefile's rule, the binary in the test's own folder; the sanitizer runtimes are linked into the
    # program itself: it runs as it is, whatever else the loader brings
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tools"), "-B", "klabel_host_check", f"KLABEL_CHECK={exe}"], check=True)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    assert run.stdout.rstrip().endswith("klabel_host_check OK")
