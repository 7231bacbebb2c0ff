"""Host-side checks of the nearest-run search (no GPU): the C ABI declares and exports nemo_nearest_runs and its two
fetches, the Python and Go bindings call them as declared, both options are documented, and the host arithmetic
(nemo_amd/csrc/nearest_host.h: distinct runs, rows of the list positions, words per row, the limits, the tile and
split-K grid) passes its stand-alone check program under the host sanitizers."""
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
CALLS = {"nemo_nearest_runs": 5, "nemo_fetch_nearest": 4, "nemo_fetch_label_distances": 5}


def test_header_declares_the_calls():
    funcs, _, types, fields = header_decls()
    for name, arity in CALLS.items():
        assert name in E.header_symbols()
        assert funcs[name] == arity, name
    assert "nemo_nearest" in types
    assert fields["nemo_nearest"] == {"cand", "dist", "only_query", "only_cand"}
    txt = open(E.HEADER).read()
    assert "#define NEMOHIP_ABI_VERSION 1" in txt  # additive
    doc = txt[txt.index("nearest runs by post-goal label sets"):txt.index("int nemo_nearest_runs(")]
    for name in ("NEMO_ERR_NOTFOUND", "NEMO_ERR_STATE", "NEMO_ERR_LIMIT", "UINT32_MAX", "nemo_diffprov_pairs"):
        assert name in doc, name
    assert "ties go to the smallest j" in doc  # the tie rule
    assert "a run is not its own neighbour" in doc  # the self-exclusion
    assert "tile\n * the queries" in doc or "tile the queries" in doc
    opts = txt[txt.index("Tuning / test knobs"):txt.index("int nemo_set_option")]
    assert '"near_bits_lds_max"' in opts and "0 = every row in place" in opts
    assert '"near_ksplit"' in opts


def test_library_exports_the_calls():
    if not os.path.exists(E.LIB_PATH):
        subprocess.run(["make", "-s", "-C", ROOT, "nemo_amd/libnemohip.so"], check=True)
    L = ctypes.CDLL(E.LIB_PATH)
    for name in CALLS:
        assert hasattr(L, name), name
    assert L.nemo_abi_version() == 1
    L.nemo_nearest_runs.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t]
    assert L.nemo_nearest_runs(None, None, 0, None, 0) == 1  # NEMO_ERR_INVALID: a null context, without a device
    L.nemo_fetch_nearest.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p]
    assert L.nemo_fetch_nearest(None, None, 0, None) == 1
    L.nemo_fetch_label_distances.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p,
                                             ctypes.c_uint64]
    assert L.nemo_fetch_label_distances(None, 0, 0, None, 0) == 1


def test_engine_binds_the_calls():
    for name, arity in CALLS.items():
        fn = getattr(E.lib(), name)
        assert len(fn.argtypes) == arity and fn.restype is ctypes.c_int, name
    assert list(inspect.signature(E.Engine.nearest_runs).parameters) == ["self", "queries", "candidates"]
    assert list(inspect.signature(E.Engine.label_distances).parameters) == ["self", "q_lo", "q_hi"]
    assert E.NEAREST_DTYPE.names == ("cand", "dist", "only_query", "only_cand") and E.NEAREST_DTYPE.itemsize == 16


def test_go_binding_calls_them_as_declared():
    src = open(GO).read()
    funcs, _, _, _ = header_decls()
    m = re.search(r"func \(n \*Neo4J\) NearestRuns\(.*?\n}\n", src, flags=re.S)
    assert m, "no NearestRuns method on *Neo4J"
    body = m.group(0)
    calls = dict(go_calls(body))
    for name in ("nemo_nearest_runs", "nemo_fetch_nearest"):
        assert f"C.{name}(" in body, name
        assert calls[name] == funcs[name] == CALLS[name], name
    for f in set(re.findall(r"\bnear\[i\]\.(\w+)", body)):
        assert f in {"cand", "dist", "only_query", "only_cand"}, f


def test_graphing_has_nearest_runs():
    from nemo_amd import graphing as GR
    assert list(inspect.signature(GR.Neo4J.NearestRuns).parameters) == ["self", "queries", "candidates"]
    doc = GR.Neo4J.NearestRuns.__doc__
    assert "no reference counterpart" in doc and "PairDiffProv" in doc and "`pairs`" in doc


def test_host_check_program_passes_under_the_host_sanitizers(tmp_path):
    src = os.path.join(ROOT, "tools", "nearest_host_check.cpp")
    text = open(src).read()
    assert "int main()" in text and '#include "../nemo_amd/csrc/nearest_host.h"' in text
    hdr = open(os.path.join(ROOT, "nemo_amd", "csrc", "nearest_host.h")).read()
    assert "hip_runtime" not in hdr  # pure host functions
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("no host C++ compiler to build tools/nearest_host_check.cpp")
    exe = str(tmp_path / "nearest_host_check")
    # the sanitizer runtimes linked into the program itself: it runs as it is, whatever else the loader brings
    subprocess.run([cxx, "-std=c++17", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", src, "-o", exe],
                   check=True, cwd=ROOT)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    assert run.stdout.rstrip().endswith("nearest_host_check OK")
