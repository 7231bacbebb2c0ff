"""Host-side checks of the minimal cut sets (no GPU): the C ABI declares and exports nemo_min_cuts and its two
fetches, the Python and Go bindings call them as declared, the option is documented, and the host arithmetic
(nemo_amd/csrc/cut_host.h: colex rank and unrank, the per-round limit, the candidate validation, the live list,
the chunk and grid counts) passes its stand-alone check program under the host sanitizers."""
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
CALLS = {"nemo_min_cuts": 7, "nemo_fetch_min_cuts": 4, "nemo_fetch_min_cut_stats": 2}


def test_header_declares_the_calls():
    funcs, _, types, fields = header_decls()
    for name, arity in CALLS.items():
        assert name in E.header_symbols()
        assert funcs[name] == arity, name
    assert "nemo_cut" in types and fields["nemo_cut"] == {"size", "node"}
    txt = open(E.HEADER).read()
    assert "#define NEMOHIP_ABI_VERSION 1" in txt  # additive
    assert "uint32_t node[3];" in txt
    doc = txt[txt.index("minimal cut sets: the smallest fault sets"):txt.index("typedef struct nemo_cut")]
    assert txt.index("typedef struct nemo_knock") < txt.index("minimal cut sets: the smallest fault sets")  # beside it
    for name in ("NEMO_ERR_NOTFOUND", "NEMO_ERR_STATE", "NEMO_ERR_LIMIT", "NEMO_ERR_INVALID", "roots_dead == n_roots",
                 "C(c,3) + C(b,2) + a", "cand == NULL", "listed twice", "shorten the", "(size, rank)", "live list",
                 "max_size must be 1, 2 or 3"):
        assert name in doc, name
    opts = txt[txt.index("Tuning / test knobs"):txt.index("int nemo_set_option")]
    assert '"cut_grid"' in opts


def test_library_exports_the_calls():
    if not os.path.exists(E.LIB_PATH):
        subprocess.run(["make", "-s", "-C", ROOT, "nemo_amd/libnemohip.so"], check=True)
    L = ctypes.CDLL(E.LIB_PATH)
    for name in CALLS:
        assert hasattr(L, name), name
    assert L.nemo_abi_version() == 1
    vp, u32, u64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64
    L.nemo_min_cuts.argtypes = [vp, u32, ctypes.c_int, vp, ctypes.c_size_t, u32, u32]
    assert L.nemo_min_cuts(None, 0, 1, None, 0, 2, 0) == 1  # NEMO_ERR_INVALID: a null context, without a device
    L.nemo_fetch_min_cuts.argtypes = [vp, vp, u64, vp]
    assert L.nemo_fetch_min_cuts(None, None, 0, None) == 1
    L.nemo_fetch_min_cut_stats.argtypes = [vp, vp]
    assert L.nemo_fetch_min_cut_stats(None, None) == 1


def test_engine_binds_the_calls():
    for name, arity in CALLS.items():
        fn = getattr(E.lib(), name)
        assert len(fn.argtypes) == arity and fn.restype is ctypes.c_int, name
    sig = inspect.signature(E.Engine.min_cuts)
    assert list(sig.parameters) == ["self", "iteration", "cond", "candidates", "max_size"]
    assert sig.parameters["candidates"].default is None and sig.parameters["max_size"].default == 2
    assert callable(E.Engine.min_cut_stats) and callable(E.Engine.min_cut_rows)
    assert E.CUT_DTYPE.names == ("size", "node") and E.CUT_DTYPE.itemsize == 16
    assert E.CUT_DTYPE["node"].shape == (3,)


def test_go_binding_calls_them_as_declared():
    src = open(GO).read()
    funcs, _, _, fields = header_decls()
    calls = {}
    for name, n in go_calls(src):
        calls.setdefault(name, set()).add(n)
    for name in CALLS:
        assert f"C.{name}(" in src, name
        assert calls[name] == {funcs[name]} == {CALLS[name]}, name
    m = re.search(r"func \(n \*Neo4J\) MinCuts\(.*?\n}\n", src, flags=re.S)
    assert m, "no MinCuts helper"
    for f in set(re.findall(r"\bcut\.(\w+)", m.group(0))):
        assert f in fields["nemo_cut"], f
    assert "C.nemo_cut" in src


def test_host_check_program_passes_under_the_host_sanitizers(tmp_path):
    src = os.path.join(ROOT, "tools", "cut_host_check.cpp")
    text = open(src).read()
    assert "int main()" in text and '#include "../nemo_amd/csrc/cut_host.h"' in text
    hdr = open(os.path.join(ROOT, "nemo_amd", "csrc", "cut_host.h")).read()
    assert "hip_runtime" not in hdr  # pure host functions
    mk = open(os.path.join(ROOT, "tools", "Makefile")).read()
    assert "-fsanitize=address,undefined" in mk and "cut_host_check.cpp" in mk
    if shutil.which("g++") is None and shutil.which("c++") is None:
        pytest.fail("no host C++ compiler to build tools/cut_host_check.cpp")
    exe = str(tmp_path / "cut_host_check")
    # tools/Makefile's rule, the binary in the test's own folder; the sanitizer runtimes are linked into the
    # program itself: it runs as it is, whatever else the loader brings
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tools"), "-B", "cut_host_check", f"CUT_CHECK={exe}"], check=True)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    assert run.stdout.rstrip().endswith("cut_host_check OK")
