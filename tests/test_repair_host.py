"""Host-side checks of the minimal repair sets (no GPU): the C ABI declares and exports nemo_min_repair_sets,
nemo_min_repairs and their three fetches, the Python and Go bindings call them as declared, and the host arithmetic
(nemo_amd/csrc/repair_host.h: the validation of the two lists, the absent bitmap, the LDS image and its tier, the status
from round 0's word) passes its stand-alone check program under the host sanitizers."""
import ctypes
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from nemo_amd import engine as E
from nemo_amd.corpus import Corpus
from tests.test_go_binding import go_calls, header_decls

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GO = os.path.join(ROOT, "go", "graphing", "nemohip.go")
CALLS = {"nemo_min_repair_sets": 9, "nemo_min_repairs": 5, "nemo_fetch_min_repairs": 4, "nemo_fetch_min_repair_stats": 2,
         "nemo_fetch_min_repair_cands": 4}


def test_header_declares_the_calls():
    funcs, defines, types, fields = header_decls()
    for name, arity in CALLS.items():
        assert name in E.header_symbols()
        assert funcs[name] == arity, name
    assert "nemo_repair" in types and fields["nemo_repair"] == fields["nemo_cut"] == {"size", "node"}
    assert {"NEMO_REPAIR_HOLDS", "NEMO_REPAIR_SEARCHED", "NEMO_REPAIR_BEYOND"} <= defines
    txt = open(E.HEADER).read()
    assert "#define NEMOHIP_ABI_VERSION 1" in txt  # additive
    for line in ("#define NEMO_REPAIR_HOLDS 0", "#define NEMO_REPAIR_SEARCHED 1", "#define NEMO_REPAIR_BEYOND 2"):
        assert line in txt
    doc = txt[txt.index("minimal repair sets: the fewest missing events"):txt.index("typedef struct nemo_repair")]
    assert txt.index("typedef struct nemo_cut") < txt.index("minimal repair sets: the fewest missing events")  # beside it
    for name in ("NEMO_ERR_NOTFOUND", "NEMO_ERR_STATE", "NEMO_ERR_LIMIT", "NEMO_ERR_INVALID", "F = A \\ S", "S = {} and S = cand",
                 "C(c,3) + C(b,2) + a", "cand == NULL", "listed twice", "not in absent", "shorten the", "(size, rank)", "live list",
                 "max_size must be 1, 2 or 3", "nemo_diffprov_pairs", "sink goals", "node-index order"):
        assert name in doc, name


def test_library_exports_the_calls():
    if not os.path.exists(E.LIB_PATH):
        subprocess.run(["make", "-s", "-C", ROOT, "nemo_amd/libnemohip.so"], check=True)
    L = ctypes.CDLL(E.LIB_PATH)
    for name in CALLS:
        assert hasattr(L, name), name
    assert L.nemo_abi_version() == 1
    vp, u32, u64, sz = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_size_t
    L.nemo_min_repair_sets.argtypes = [vp, u32, ctypes.c_int, vp, sz, vp, sz, u32, u32]
    assert L.nemo_min_repair_sets(None, 0, 1, None, 0, None, 0, 2, 0) == 1  # NEMO_ERR_INVALID: a null context, without a device
    L.nemo_min_repairs.argtypes = [vp, u32, u32, u32, u32]
    assert L.nemo_min_repairs(None, 0, 1, 2, 0) == 1
    L.nemo_fetch_min_repairs.argtypes = [vp, vp, u64, vp]
    assert L.nemo_fetch_min_repairs(None, None, 0, None) == 1
    L.nemo_fetch_min_repair_stats.argtypes = [vp, vp]
    assert L.nemo_fetch_min_repair_stats(None, None) == 1
    L.nemo_fetch_min_repair_cands.argtypes = [vp, vp, u64, vp]
    assert L.nemo_fetch_min_repair_cands(None, None, 0, None) == 1


def test_engine_binds_the_calls():
    for name, arity in CALLS.items():
        fn = getattr(E.lib(), name)
        assert len(fn.argtypes) == arity and fn.restype is ctypes.c_int, name
    sig = inspect.signature(E.Engine.min_repairs)
    assert list(sig.parameters) == ["self", "base", "other", "max_size"] and sig.parameters["max_size"].default == 2
    sig = inspect.signature(E.Engine.min_repair_sets)
    assert list(sig.parameters) == ["self", "iteration", "cond", "absent", "candidates", "max_size"]
    assert sig.parameters["candidates"].default is None and sig.parameters["max_size"].default == 2
    assert callable(E.Engine.min_repair_rows) and callable(E.Engine.min_repair_stats)
    assert (E.REPAIR_HOLDS, E.REPAIR_SEARCHED, E.REPAIR_BEYOND) == (0, 1, 2)


def test_repair_labels_names_the_rows():
    u32 = lambda x: np.ascontiguousarray(x, dtype=np.uint32)
    # run 0: a pre graph of one node, a post graph of four; the labels of the post graph's nodes are 1..4
    corpus = Corpus(iteration=u32([0]), node_off=np.ascontiguousarray([0, 1, 5], dtype=np.uint64),
                    edge_off=np.ascontiguousarray([0, 0, 0], dtype=np.uint64), node_word=u32([0, 2, 2, 2, 2]),
                    label=u32([0, 1, 2, 3, 9]), edge_src=u32([]), edge_dst=u32([]), n_tables=3, table_pre=0, table_post=1,
                    status=["success"], labels=["pre", "a(1)", "b(2)", "c(3)"])
    rows = u32([[1, 2, 0xFFFFFFFF, 0xFFFFFFFF], [3, 0, 1, 3]])
    assert E.repair_labels(corpus, 1, rows) == [["c(3)"], ["a(1)", "b(2)", "9"]]  # label 9 has no string: its id
    assert E.repair_labels(corpus, 1, u32([]).reshape(0, 4)) == []


def test_go_binding_calls_them_as_declared():
    src = open(GO).read()
    funcs, defines, _, fields = header_decls()
    calls = {}
    for name, n in go_calls(src):
        calls.setdefault(name, set()).add(n)
    for name in ("nemo_min_repairs", "nemo_fetch_min_repairs", "nemo_fetch_min_repair_stats", "nemo_fetch_min_repair_cands"):
        assert f"C.{name}(" in src, name
        assert calls[name] == {funcs[name]} == {CALLS[name]}, name
    for name, ns in calls.items():  # ... and whichever of the five it calls beside them
        if name in CALLS:
            assert ns == {CALLS[name]}, name
    m = re.search(r"func \(n \*Neo4J\) MinRepairs\(base, other uint, maxSize uint\).*?\n}\n", src, flags=re.S)
    assert m, "no MinRepairs(base, other uint, maxSize uint) helper"
    for f in set(re.findall(r"\brep\.(\w+)", m.group(0))):
        assert f in fields["nemo_repair"], f
    assert "C.nemo_repair" in src
    for c in set(re.findall(r"\bC\.(NEMO_REPAIR_\w+)", src)):
        assert c in defines, c


def test_host_check_program_passes_under_the_host_sanitizers(tmp_path):
    src = os.path.join(ROOT, "tools", "repair_host_check.cpp")
    text = open(src).read()
    assert "int main()" in text and '#include "../nemo_amd/csrc/repair_host.h"' in text
    hdr = open(os.path.join(ROOT, "nemo_amd", "csrc", "repair_host.h")).read()
    assert "hip_runtime" not in hdr  # pure host functions
    mk = open(os.path.join(ROOT, "tools", "Makefile")).read()
    assert "-fsanitize=address,undefined" in mk and "repair_host_check.cpp" in mk
    if shutil.which("g++") is None and shutil.which("c++") is None:
        pytest.fail("no host C++ compiler to build tools/repair_host_check.cpp")
    exe = str(tmp_path / "repair_host_check")
    # tools/Makefile's rule, the binary in the test's own folder; the sanitizer runtimes are linked into the
    # program itself: it runs as it is, whatever else the loader brings
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tools"), "-B", "repair_host_check", f"REPAIR_CHECK={exe}"], check=True)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    assert run.stdout.rstrip().endswith("repair_host_check OK")
