"""Host-side checks of the pair diff (no GPU): the C ABI declares and exports nemo_diffprov_pairs, the Python and
Go bindings call it as declared, the option is documented, and the host arithmetic of the label tables
(nemo_amd/csrc/pairs_host.h: distinct `other` runs, capacities, placement in the region) passes its stand-alone
check program under the host sanitizers."""
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


def test_header_declares_the_call():
    assert "nemo_diffprov_pairs" in E.header_symbols()
    funcs, _, _, _ = header_decls()
    assert funcs["nemo_diffprov_pairs"] == 4
    txt = open(E.HEADER).read()
    assert "#define NEMOHIP_ABI_VERSION 1" in txt  # additive
    doc = txt[txt.index("differential provenance between arbitrary pairs"):txt.index("int nemo_diffprov_pairs(")]
    # the reference lines it mirrors, which graph `rule` is local to, and whose results it replaces
    assert "differential-provenance.go:22-28" in doc and ":82-98" in doc
    assert "local to the entry's base run's post graph" in doc
    for name in ("nemo_fetch_sdiff_masks", "nemo_fetch_surplus", "nemo_pull_edges(ctx, 3)", "nemo_mark_holds",
                 "NEMO_ERR_STATE", "NEMO_ERR_NOTFOUND"):
        assert name in doc, name
    opts = txt[txt.index("Tuning / test knobs"):txt.index("int nemo_set_option")]
    assert '"pair_hash_lds_max"' in opts and "0 = every table in place" in opts


def test_library_exports_the_call():
    if not os.path.exists(E.LIB_PATH):
        subprocess.run(["make", "-s", "-C", ROOT, "nemo_amd/libnemohip.so"], check=True)
    L = ctypes.CDLL(E.LIB_PATH)
    assert hasattr(L, "nemo_diffprov_pairs")
    assert L.nemo_abi_version() == 1
    L.nemo_diffprov_pairs.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]
    assert L.nemo_diffprov_pairs(None, None, None, 0) == 1  # NEMO_ERR_INVALID: a null context, without a device


def test_engine_binds_the_call():
    fn = E.lib().nemo_diffprov_pairs
    assert len(fn.argtypes) == 4 and fn.restype is ctypes.c_int
    assert list(inspect.signature(E.Engine.diffprov_pairs).parameters) == ["self", "base", "other"]


def test_go_binding_calls_it_as_declared():
    src = open(GO).read()
    funcs, _, _, _ = header_decls()
    calls = dict(go_calls(src))
    assert calls.get("nemo_diffprov_pairs") == funcs["nemo_diffprov_pairs"] == 4
    m = re.search(r"func \(n \*Neo4J\) PairDiffProv\(.*?\n}\n", src, flags=re.S)
    assert m, "no PairDiffProv method on *Neo4J"
    body = m.group(0)
    for name in ("nemo_diffprov_pairs", "nemo_fetch_sdiff_masks", "nemo_fetch_surplus", "nemo_pull_edges"):
        assert f"C.{name}(" in body, name


def test_graphing_has_pair_diffprov():
    from nemo_amd import graphing as GR
    assert list(inspect.signature(GR.Neo4J.PairDiffProv).parameters) == ["self", "pairs"]
    assert "no reference counterpart" in GR.Neo4J.PairDiffProv.__doc__


def test_host_check_program_passes_under_the_host_sanitizers(tmp_path):
    src = os.path.join(ROOT, "tools", "pairs_host_check.cpp")
    text = open(src).read()
    assert "int main()" in text and '#include "../nemo_amd/csrc/pairs_host.h"' in text
    hdr = open(os.path.join(ROOT, "nemo_amd", "csrc", "pairs_host.h")).read()
    assert "hip_runtime" not in hdr  # pure host functions
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("no host C++ compiler to build tools/pairs_host_check.cpp")
    exe = str(tmp_path / "pairs_host_check")
    # the sanitizer runtimes linked into the program itself: it runs as it is, whatever else the loader brings
    subprocess.run([cxx, "-std=c++17", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", src, "-o", exe],
                   check=True, cwd=ROOT)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    assert run.stdout.rstrip().endswith("pairs_host_check OK")
