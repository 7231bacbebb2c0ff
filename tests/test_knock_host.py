"""Host-side checks of the knock-out analysis (no GPU): the C ABI declares and exports nemo_knockout_leaves,
nemo_knockout_sets and the three fetches, the Python and Go bindings call them as declared, the option is
documented, and the host arithmetic (nemo_amd/csrc/knock_host.h: the LDS tier, the chunk table, the limits, the
validation of explicit sets) passes its stand-alone check program under the host sanitizers."""
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
CALLS = {"nemo_knockout_leaves": 5, "nemo_knockout_sets": 7, "nemo_fetch_knockout": 4, "nemo_fetch_knockout_ranges": 4,
         "nemo_fetch_knockout_mask": 4}
FIELDS = ("graph", "node", "n_dead", "roots_dead", "n_roots")


def test_header_declares_the_calls():
    funcs, defines, types, fields = header_decls()
    for name, arity in CALLS.items():
        assert name in E.header_symbols()
        assert funcs[name] == arity, name
    assert "nemo_knock" in types and fields["nemo_knock"] == set(FIELDS)
    assert "NEMO_KO_MASKS" in defines
    txt = open(E.HEADER).read()
    assert "#define NEMOHIP_ABI_VERSION 1" in txt  # additive
    doc = txt[txt.index("knock-out analysis: which events"):txt.index("typedef struct nemo_knock")]
    for name in ("NEMO_ERR_NOTFOUND", "NEMO_ERR_STATE", "NEMO_ERR_LIMIT", "NEMO_ERR_INVALID", "NEMO_NODE_RULE",
                 "roots_dead == n_roots", "tile the call", "counts once", "node-index order"):
        assert name in doc, name
    opts = txt[txt.index("Tuning / test knobs"):txt.index("int nemo_set_option")]
    assert '"knock_lds_max"' in opts and "0 = every graph in device memory" in opts


def test_library_exports_the_calls():
    if not os.path.exists(E.LIB_PATH):
        subprocess.run(["make", "-s", "-C", ROOT, "nemo_amd/libnemohip.so"], check=True)
    L = ctypes.CDLL(E.LIB_PATH)
    for name in CALLS:
        assert hasattr(L, name), name
    assert L.nemo_abi_version() == 1
    vp, u32, u64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64
    L.nemo_knockout_leaves.argtypes = [vp, vp, ctypes.c_size_t, ctypes.c_int, u32]
    assert L.nemo_knockout_leaves(None, None, 0, 1, 0) == 1  # NEMO_ERR_INVALID: a null context, without a device
    L.nemo_knockout_sets.argtypes = [vp, u32, ctypes.c_int, vp, vp, ctypes.c_size_t, u32]
    assert L.nemo_knockout_sets(None, 0, 1, None, None, 0, 0) == 1
    L.nemo_fetch_knockout.argtypes = [vp, vp, u64, vp]
    assert L.nemo_fetch_knockout(None, None, 0, None) == 1
    L.nemo_fetch_knockout_ranges.argtypes = [vp, vp, vp, u64]
    assert L.nemo_fetch_knockout_ranges(None, None, None, 0) == 1
    L.nemo_fetch_knockout_mask.argtypes = [vp, u64, vp, u64]
    assert L.nemo_fetch_knockout_mask(None, 0, None, 0) == 1


def test_engine_binds_the_calls():
    for name, arity in CALLS.items():
        fn = getattr(E.lib(), name)
        assert len(fn.argtypes) == arity and fn.restype is ctypes.c_int, name
    assert list(inspect.signature(E.Engine.knockout_leaves).parameters) == ["self", "iters", "cond", "masks"]
    assert list(inspect.signature(E.Engine.knockout_sets).parameters) == ["self", "iteration", "cond", "sets", "masks"]
    for name in ("knockout_rows", "knockout_ranges", "knockout_mask"):
        assert callable(getattr(E.Engine, name)), name
    assert E.KNOCK_DTYPE.names == FIELDS and E.KNOCK_DTYPE.itemsize == 20 and E.KO_MASKS == 1


def test_go_binding_calls_them_as_declared():
    src = open(GO).read()
    funcs, _, _, _ = header_decls()
    calls = dict(go_calls(src))
    for name in CALLS:
        assert f"C.{name}(" in src, name
        assert calls[name] == funcs[name] == CALLS[name], name
    for method in ("KnockOutLeaves", "KnockOutSets"):
        assert re.search(r"func \(n \*Neo4J\) %s\(" % method, src), method
    m = re.search(r"func \(n \*Neo4J\) knockOut\(k C\.nemo_knock\).*?\n}\n", src, flags=re.S)
    assert m, "no knockOut conversion"
    for f in set(re.findall(r"\bk\.(\w+)", m.group(0))):
        assert f in FIELDS, f
    assert "C.NEMO_KO_MASKS" in src


def test_graphing_has_critical_leaves():
    from nemo_amd import graphing as GR
    assert list(inspect.signature(GR.Neo4J.CriticalLeaves).parameters) == ["self", "run", "cond"]
    doc = GR.Neo4J.CriticalLeaves.__doc__
    assert "no reference counterpart" in doc and "nemo_knockout_leaves" in doc


def test_host_check_program_passes_under_the_host_sanitizers(tmp_path):
    src = os.path.join(ROOT, "tools", "knock_host_check.cpp")
    text = open(src).read()
    assert "int main()" in text and '#include "../nemo_amd/csrc/knock_host.h"' in text
    hdr = open(os.path.join(ROOT, "nemo_amd", "csrc", "knock_host.h")).read()
    assert "hip_runtime" not in hdr  # pure host functions
    mk = open(os.path.join(ROOT, "tools", "Makefile")).read()
    assert "-fsanitize=address,undefined" in mk and "knock_host_check.cpp" in mk
    if shutil.which("g++") is None and shutil.which("c++") is None:
        pytest.fail("no host C++ compiler to build tools/knock_host_check.cpp")
    exe = str(tmp_path / "knock_host_check")
    # tools/Makefile's rule, the binary in the test's own folder; the sanitizer runtimes are linked into the
    # program itself: it runs as it is, whatever else the loader brings
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tools"), "-B", "knock_host_check", f"KNOCK_CHECK={exe}"],
                   check=True)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    assert run.stdout.rstrip().endswith("knock_host_check OK")
