"""Host-side checks of the lineage cut search over fault events (no GPU): the C ABI declares and exports
nemo_lineage_group_cuts, its two fetches and the struct; the Python and Go bindings call them as declared; the header
states the definitions it takes over, the search, the completeness argument, the emission rule, the errors and the
limits; nemo_amd/csrc/lgc_host.h reuses the parent calls' host headers and passes its stand-alone check program (a host
model of the whole search against brute force) under the host sanitizers; and the kernels share the parents' device
code instead of restating it."""
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
CALLS = {"nemo_lineage_group_cuts": 10, "nemo_fetch_lineage_group_cuts": 5, "nemo_fetch_lineage_group_cut_stats": 2}


def test_header_declares_the_calls():
    funcs, _, types, fields = header_decls()
    for name, arity in CALLS.items():
        assert name in E.header_symbols()
        assert funcs[name] == arity, name
    assert "nemo_lineage_group_cut" in types and fields["nemo_lineage_group_cut"] == {"size", "group"}
    txt = open(E.HEADER).read()
    assert "#define NEMOHIP_ABI_VERSION 1" in txt  # additive
    assert "uint32_t group[8];" in txt
    start = txt.index("lineage cut search over fault events")
    assert txt.index("int nemo_fetch_min_group_cut_stats") < start < txt.index("surviving derivations: why")  # beside nemo_min_group_cuts
    doc = re.sub(r"\s*\n \* ", " ", txt[start:txt.index("int nemo_fetch_lineage_group_cut_stats")])
    for name in ("nemo_min_group_cuts' definitions above, unchanged", "a run listed twice", "all minimal cuts of size <= max_size",
                 "colex order of the candidate positions", "UINT32_MAX", "n_lost[k] is row k's lost_count",
                 "nemo_min_group_cuts' own, in its order", "its live list keeps candidate order",
                 "level 0 evaluates the empty set", "lost_count >= q is a minimal cut of size d", "not expanded",
                 "nemo_witness_labels' single derivation", "smallest node index", "not NEMO_WIT_ALL", "only sink goals of W_F^i count",
                 "no proper subset among the cuts of sizes <= d", "stops after level max_size or at an empty frontier",
                 "Every minimal cut is reached", "lost_count(F) < q <= lost_count(C)", "lost under C and not under F",
                 "an alive root among them", "is not in F", "a child of F lies in C", "filtered before it was evaluated",
                 "whether or not the cross-run count later makes the set a cut", "the subset filter drops them", "one fused pass",
                 "costs nothing under q = n", "before duplicates are removed", "decreasing group_off", "max_size must be 1..8",
                 "min_runs > n", "cond outside 0 / 1", "unknown flags", "more than 65535 groups", "eight u16 candidate positions",
                 "2^24 in one group", "> 2^28 lost words", "2^32 - 2 sets", '"lineage_children_max"', "leaves no results",
                 "runs again, once", "does not append its cuts twice", "every listed graph empty", "nothing is evaluated",
                 "NEMO_ERR_NOTFOUND", "NEMO_ERR_STATE", "node context", "next nemo_lineage_group_cuts or nemo_load_corpus",
                 "both directions", '"wit_lds_max"', '"kl_grid"'):
        assert name in doc, name
    assert E.LINEAGE_GROUP_CUT_DTYPE.itemsize == 36 and E.LINEAGE_GROUP_CUT_DTYPE.names == ("size", "group")
    assert E.LINEAGE_GROUP_CUT_DTYPE["group"].shape == (8,)


def test_library_exports_the_calls():
    if not os.path.exists(E.LIB_PATH):
        subprocess.run(["make", "-s", "-C", ROOT, "nemo_amd/libnemohip.so"], check=True)
    L = ctypes.CDLL(E.LIB_PATH)
    for name in CALLS:
        assert hasattr(L, name), name
    assert L.nemo_abi_version() == 1
    vp, u32, u64, sz = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_size_t
    L.nemo_lineage_group_cuts.argtypes = [vp, vp, sz, ctypes.c_int, vp, vp, sz, u32, u32, u32]
    assert L.nemo_lineage_group_cuts(None, None, 0, 1, None, None, 0, 3, 0, 0) == 1  # NEMO_ERR_INVALID: a null context, no device
    L.nemo_fetch_lineage_group_cuts.argtypes = [vp, vp, vp, u64, vp]
    assert L.nemo_fetch_lineage_group_cuts(None, None, None, 0, None) == 1
    L.nemo_fetch_lineage_group_cut_stats.argtypes = [vp, vp]
    assert L.nemo_fetch_lineage_group_cut_stats(None, None) == 1


def test_engine_binds_the_calls():
    for name, arity in CALLS.items():
        fn = getattr(E.lib(), name)
        assert len(fn.argtypes) == arity and fn.restype is ctypes.c_int, name
    sig = inspect.signature(E.Engine.lineage_group_cuts)
    assert list(sig.parameters) == ["self", "iters", "cond", "groups", "max_size", "min_runs", "sinks_only"]
    assert sig.parameters["min_runs"].default == 0 and sig.parameters["sinks_only"].default is False
    assert list(inspect.signature(E.Engine.lineage_group_cut_rows).parameters) == ["self"]
    assert "reshape(9, 2)" in inspect.getsource(E.Engine.lineage_group_cut_stats)


def test_go_binding_calls_them_as_declared():
    src = open(GO).read()
    funcs, _, _, fields = header_decls()
    calls = {}
    for name, n in go_calls(src):
        calls.setdefault(name, set()).add(n)
    for name in CALLS:
        assert f"C.{name}(" in src, name
        assert calls[name] == {funcs[name]} == {CALLS[name]}, name
    fn = re.search(r"func \(n \*Neo4J\) LineageGroupCuts\(.*?\n}\n", src, flags=re.S)
    assert fn and all(f"C.{name}(" in fn.group(0) for name in CALLS) and "C.nemo_lineage_group_cut" in fn.group(0)
    assert "[18]uint64" in fn.group(0) and src.index("func (n *Neo4J) MinGroupCuts(") < fn.start()
    for f in set(re.findall(r"\bgc\.(\w+)", fn.group(0))):
        assert f in fields["nemo_lineage_group_cut"], f"gc.{f} is not a field of nemo_lineage_group_cut"


def test_host_header_reuses_and_kernels_share():
    hdr = open(os.path.join(CSRC, "lgc_host.h")).read()
    assert "hip_runtime" not in hdr  # pure host functions
    for name in ('#include "gcut_host.h"', '#include "lin_host.h"', '#include "wit_host.h"', "lin::front_fits", "klabel::words_fit",
                 "gcuts::list_entries", "lin::emit_bound"):
        assert name in hdr, name
    k = open(os.path.join(CSRC, "k_lgcuts.hip")).read()
    for name in ('#include "hit_list.h"', '#include "ko_sweep.h"', '#include "wit_down.h"', '#include "lin_dev.h"', "hit_list_build(",
                 "ko_sweep<LDS>(g)", "wit_down<LDS>(g, need, n, false)", "lin_stage_keys(", "lin_emit(", "lin_cut_insert(", "lgc::lost_count(",
                 "uint64_t lgc_wave_or(", "uint64_t lgc_range_or(", "void k_lgc_lds(", "void k_lgc_glob(", "void k_lgc_cuts("):
        assert name in k, name
    assert "void wit_down(" not in k and "void ko_sweep(" not in k and "void k_lin_filter(" not in k
    lin = open(os.path.join(CSRC, "k_lineage.hip")).read()
    assert '#include "lin_dev.h"' in lin and "lin::Key lin_load(" not in lin  # moved, not copied
    assert "lin_stage_keys(" in lin and "lin_emit(" in lin
    dev = open(os.path.join(CSRC, "lin_dev.h")).read()
    for name in ("lin::Key lin_load(", "void lin_store(", "uint32_t lin_wave_scan(", "void lin_cut_insert(", "void lin_stage_keys(",
                 "void lin_emit(", "lin::key_insert("):
        assert name in dev, name
    # the emission tail is lin_dev.h's alone: one scan, one claim on the children's cursor in the whole tree
    assert "lin_wave_scan(" not in k and "lin_wave_scan(" not in lin and "lin::key_insert(" not in k and "lin::key_insert(" not in lin
    claims = [f for f in sorted(os.listdir(CSRC)) if "ctr + 1," in open(os.path.join(CSRC, f)).read()]
    assert claims == ["lin_dev.h"] and dev.count("atomicAdd(l.ctr + 1,") == 1
    api = open(os.path.join(CSRC, "api_lgcuts.hip")).read()
    api_lin = open(os.path.join(CSRC, "api_lineage.hip")).read()
    api_lrep = open(os.path.join(CSRC, "api_lrepair.hip")).read()
    for name in ('GroupTimer timer(c, "k_lgcuts")', "launch_gc_table(", "launch_gc_rows(", "grow_drop(", "ko_lds_total(", "wit::lds_fits(",
                 '#include "lin_api.h"', "lin_levels(", "lin_sorted_keys("):
        assert name in api, name
    # the level loop, its buffers' growth and the overflow rule are lin_api.h's, once, for all three searches
    drv = open(os.path.join(CSRC, "lin_api.h")).read()
    assert '#include "knock_api.h"' in drv
    for name in ("launch_lin_filter(", "launch_lin_rehash(", "grow_keep(", "lin::cuts_grown(", "lin::emit_grown(", "lin::level_end("):
        assert name in drv, name
        assert name not in api and name not in api_lin and name not in api_lrep, name
    assert "static int lin_levels(" in drv and drv.count("int lin_levels(") == 1
    # ... and so is the tail of the two searches over one graph, from the tier choice to the rows: its callers name
    # what differs and neither the level loop nor the keys' way to the host
    assert "static int lin_node_search(" in drv and drv.count("int lin_node_search(") == 1
    assert drv.count("lin_levels(c, who,") == 1 and drv.count("lin_sorted_keys(c, b, nullptr,") == 1
    for src in (api_lin, api_lrep):
        assert '#include "lin_api.h"' in src and src.count("lin_node_search(c, ls,") == 1
        assert "lin_levels(" not in src and "lin_sorted_keys(" not in src and "lin::key_unpack(" not in src
    users = [f for f in sorted(os.listdir(CSRC)) if '#include "lin_api.h"' in open(os.path.join(CSRC, f)).read()]
    assert users == ["api_lgcuts.hip", "api_lineage.hip", "api_lrepair.hip"]
    host = open(os.path.join(CSRC, "lin_host.h")).read()
    assert "LevelEnd level_end(" in host and "level_end(" not in hdr  # moved, not copied
    ctx = open(os.path.join(CSRC, "ctx.h")).read()
    assert "struct LinBufs {" in ctx and "LinBufs d_ln;" in ctx and "LinBufs d_lg;" in ctx
    shared = open(os.path.join(CSRC, "knock_api.h")).read()
    assert "int grow_keep(" in shared and "int grow_drop(" in shared
    assert "int grow_keep(" not in api_lin


def test_host_check_program_passes_under_the_host_sanitizers(tmp_path):
    src = os.path.join(ROOT, "tools", "lgc_host_check.cpp")
    text = open(src).read()
    assert "int main()" in text and '#include "../nemo_amd/csrc/lgc_host.h"' in text
    mk = open(os.path.join(ROOT, "tools", "Makefile")).read()
    assert "-fsanitize=address,undefined" in mk and "lgc_host_check.cpp" in mk
    if shutil.which("g++") is None and shutil.which("c++") is None:
        pytest.fail("no host C++ compiler to build tools/lgc_host_check.cpp")
    exe = str(tmp_path / "lgc_host_check")
    # tools/Makefile's rule, the binary in the test's own folder; the sanitizer runtimes are linked into the
    # program itself: it runs as it is, whatever else the loader brings
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tools"), "-B", "lgc_host_check", f"LGC_CHECK={exe}"], check=True)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    assert run.stdout.rstrip().endswith("lgc_host_check OK")
