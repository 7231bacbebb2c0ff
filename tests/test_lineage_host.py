"""Host-side checks of the lineage-driven cut search (no GPU): the C ABI declares and exports nemo_lineage_cuts and its
two fetches and the struct; the Python and Go bindings call them as declared; the semantics, the row order, the search,
the error codes, the limits and the option are documented; nemo_amd/csrc/lin_host.h reuses cut_host.h and passes its
stand-alone check program under the host sanitizers; and the need pass lives in a header both kernels include."""
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
CSRC = os.path.join(ROOT, "nemo_amd", "csrc")
CALLS = {"nemo_lineage_cuts": 7, "nemo_fetch_lineage_cuts": 4, "nemo_fetch_lineage_cut_stats": 2}


def test_header_declares_the_calls():
    funcs, _, types, fields = header_decls()
    for name, arity in CALLS.items():
        assert name in E.header_symbols()
        assert funcs[name] == arity, name
    assert "nemo_lineage_cut" in types and fields["nemo_lineage_cut"] == {"size", "node"}
    txt = open(E.HEADER).read()
    assert "#define NEMOHIP_ABI_VERSION 1" in txt  # additive
    assert "uint32_t node[8];" in txt and "uint64_t out[18]" in txt
    start = txt.index("lineage-driven cut search: minimal cuts up to size 8")
    assert txt.index("int nemo_fetch_min_cut_stats") < start < txt.index("knock-out by label: fault sets tested")  # beside nemo_min_cuts
    doc = txt[start:txt.index("int nemo_fetch_lineage_cut_stats")]
    for name in ("nemo_min_cuts'\n * definitions above, unchanged", "cand == NULL means every sink goal", "goals, rules or inner nodes",
                 "listed twice", "checked on the host before\n * anything is uploaded", "max_size must be 1..8", "flags 0",
                 "More than 65535 candidates", "eight u16 candidate positions", "all minimal cuts of size <= max_size",
                 "largest position first", "nemo_min_cuts' row order", "ascend by candidate position", "UINT32_MAX",
                 "Level 0 evaluates the empty set", "frontier of distinct sets of size d", "is not expanded",
                 "nemo_witness_sets' single derivation", "smallest node index", "not NEMO_WIT_ALL", "every candidate e that is in W_F",
                 "no\n * proper subset among the cuts of sizes <= d", "stops after level\n * max_size", "frontier is empty",
                 "Every minimal cut is reached", "n_cand == 0 with a list", "graph without roots", "every stat is 0",
                 "NEMO_ERR_NOTFOUND", "cond outside 0 / 1", "NEMO_ERR_STATE", "node context", "2^32 - 2 sets",
                 "counted before duplicates\n * are removed", '"lineage_children_max"', "NEMO_ERR_LIMIT", "leaves no results",
                 "runs again, once", "blocks until the rows are on the host", "next nemo_lineage_cuts or nemo_load_corpus",
                 "both directions", '"wit_lds_max"', '"kl_grid"', "sets evaluated at size d"):
        assert name in doc, name
    opts = txt[txt.index("Tuning / test knobs"):txt.index("int nemo_set_option")]
    for name in ('"lineage_children_max"', "2^24", "256 MiB", "a memory bound", "at least 64", "-1 = the", "nemo_lineage_cuts takes its tier"):
        assert name in opts, name
    assert E.LINEAGE_CUT_DTYPE.itemsize == 36 and E.LINEAGE_CUT_DTYPE.names == ("size", "node")
    assert E.LINEAGE_CUT_DTYPE["node"].shape == (8,)


def test_library_exports_the_calls():
    if not os.path.exists(E.LIB_PATH):
        subprocess.run(["make", "-s", "-C", ROOT, "nemo_amd/libnemohip.so"], check=True)
    L = ctypes.CDLL(E.LIB_PATH)
    for name in CALLS:
        assert hasattr(L, name), name
    assert L.nemo_abi_version() == 1
    vp, u32, u64, sz = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_size_t
    L.nemo_lineage_cuts.argtypes = [vp, u32, ctypes.c_int, vp, sz, u32, u32]
    assert L.nemo_lineage_cuts(None, 0, 1, None, 0, 3, 0) == 1  # NEMO_ERR_INVALID: a null context, no device
    L.nemo_fetch_lineage_cuts.argtypes = [vp, vp, u64, vp]
    assert L.nemo_fetch_lineage_cuts(None, None, 0, None) == 1
    L.nemo_fetch_lineage_cut_stats.argtypes = [vp, vp]
    assert L.nemo_fetch_lineage_cut_stats(None, None) == 1


def test_engine_binds_the_calls():
    for name, arity in CALLS.items():
        fn = getattr(E.lib(), name)
        assert len(fn.argtypes) == arity and fn.restype is ctypes.c_int, name
    sig = inspect.signature(E.Engine.lineage_cuts)
    assert list(sig.parameters) == ["self", "iteration", "cond", "candidates", "max_size"]
    assert sig.parameters["candidates"].default is None and sig.parameters["max_size"].default == 3
    assert list(inspect.signature(E.Engine.lineage_cut_rows).parameters) == ["self"]
    assert list(inspect.signature(E.Engine.lineage_cut_stats).parameters) == ["self"]
    assert "reshape(9, 2)" in inspect.getsource(E.Engine.lineage_cut_stats)


def test_go_binding_calls_them_as_declared():
    src = open(GO).read()
    funcs, _, _, fields = header_decls()
    calls = {}
    for name, n in go_calls(src):
        calls.setdefault(name, set()).add(n)
    for name in CALLS:
        assert f"C.{name}(" in src, name
        assert calls[name] == {funcs[name]} == {CALLS[name]}, name
    fn = re.search(r"func \(n \*Neo4J\) LineageCuts\(.*?\n}\n", src, flags=re.S)
    assert fn and all(f"C.{name}(" in fn.group(0) for name in CALLS) and "C.nemo_lineage_cut" in fn.group(0)
    assert "[18]uint64" in fn.group(0)
    for f in set(re.findall(r"\bcut\.(\w+)", fn.group(0))):
        assert f in fields["nemo_lineage_cut"], f"cut.{f} is not a field of nemo_lineage_cut"


def test_host_header_reuses_and_kernels_share_the_need_pass():
    hdr = open(os.path.join(CSRC, "lin_host.h")).read()
    assert "hip_runtime" not in hdr  # pure host functions
    assert '#include "cut_host.h"' in hdr and "cuts::check_cands" in hdr and "cuts::chunks" in hdr and "cuts::grid" in hdr
    assert "std::sort" not in hdr  # the candidate check is not restated
    down = open(os.path.join(CSRC, "wit_down.h")).read()
    assert "void wit_down(" in down and "wit_need(" in down and "void wit_or(" in down
    for k in ("k_witness.hip", "k_lineage.hip"):
        src = open(os.path.join(CSRC, k)).read()
        assert '#include "wit_down.h"' in src and "void wit_down(" not in src, k
    lin = open(os.path.join(CSRC, "k_lineage.hip")).read()
    assert "ko_sweep<LDS>(g)" in lin and "wit_down<LDS>(g, need, n, false)" in lin
    for name in ("k_lin_lds", "k_lin_glob", "k_lin_filter"):
        assert f"void {name}(" in lin, name
    api = open(os.path.join(CSRC, "api_lineage.hip")).read()
    assert '#include "knock_api.h"' in api and 'GroupTimer timer(c, "k_lineage")' in api and "ensure_nlev(" in api
    # the tier choice, the level loop and the rows are the shared tail's: the call names its tier functions and kernels
    tail = open(os.path.join(CSRC, "lin_api.h")).read()
    assert '#include "lin_api.h"' in api and "lin_node_search(c, ls," in api and "wit::lds_fits, wit::wit_lds_bytes, wit::glob_words" in api
    assert '"k_lin_lds"' in api and '"k_lin_glob"' in api and "ls.glob_node_bytes = 32.0" in api
    for name in ("ko_lds_total(", "c->opt.wit_lds_max", "c->opt.kl_grid", "lin_levels(", "lin_sorted_keys(", "lin::key_unpack("):
        assert tail.count(name) == 1 + (name in ("lin_levels(", "lin_sorted_keys(")), name  # once (the two: defined, and called once)
        assert name not in api, name
    assert "std::function" not in api and "std::function" not in tail
    assert "NEMO_WIT_MASKS" not in api and "nemo_witness_sets(" not in api  # fused: no witness call and a reader


def test_host_check_program_passes_under_the_host_sanitizers(tmp_path):
    src = os.path.join(ROOT, "tools", "lin_host_check.cpp")
    text = open(src).read()
    assert "int main()" in text and '#include "../nemo_amd/csrc/lin_host.h"' in text
    mk = open(os.path.join(ROOT, "tools", "Makefile")).read()
    assert "-fsanitize=address,undefined" in mk and "lin_host_check.cpp" in mk
    if shutil.which("g++") is None and shutil.which("c++") is None:
        pytest.fail("no host C++ compiler to build tools/lin_host_check.cpp")
    exe = str(tmp_path / "lin_host_check")
    # tools/Makefile's rule, the binary in the test's own folder; the sanitizer runtimes are linked into the
    # program itself: it runs as it is, whatever else the loader brings
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tools"), "-B", "lin_host_check", f"LIN_CHECK={exe}"], check=True)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    assert run.stdout.rstrip().endswith("lin_host_check OK")
