"""Host-side checks of the lineage repair search (no GPU): the C ABI declares and exports nemo_lineage_repair_sets,
nemo_lineage_repairs and their three fetches and the struct; the Python and Go bindings call them as declared; the
definitions, the lemma, the search, the checks' order, the limits and the options are documented;
nemo_amd/csrc/lrep_host.h reuses lin_host.h, repair_host.h and wit_host.h and passes its stand-alone check program under
the host sanitizers; and the blame pass lives in a header both kernels include, beside an unchanged wit_down.h."""
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
CALLS = {"nemo_lineage_repair_sets": 9, "nemo_lineage_repairs": 5, "nemo_fetch_lineage_repairs": 4,
         "nemo_fetch_lineage_repair_stats": 2, "nemo_fetch_lineage_repair_cands": 4}


def test_header_declares_the_calls():
    funcs, _, types, fields = header_decls()
    for name, arity in CALLS.items():
        assert name in E.header_symbols()
        assert funcs[name] == arity, name
    assert "nemo_lineage_repair" in types and fields["nemo_lineage_repair"] == {"size", "node"}
    txt = open(E.HEADER).read()
    assert "#define NEMOHIP_ABI_VERSION 1" in txt  # additive
    assert "uint64_t out[20]" in txt
    start = txt.index("lineage repair search: minimal repairs up to size 8 from blockers")
    assert txt.index("int nemo_fetch_min_repair_cands") < start < txt.index("lineage-driven cut search: minimal cuts")  # beside the repairs
    doc = re.sub(r"\s*\n \* ", " ", txt[start:txt.index("int nemo_fetch_lineage_repair_stats")])
    for name in ("nemo_min_repair_sets' definitions above, unchanged", "Blocker.", "every root is blamed", "that is in F blames nothing further",
                 "its dead child of smallest node index", "the forward rows ascend", "blames every child", "every blamed node is dead under F",
                 "Lemma.", "the outcome is lost under F'", "must restore a node of the blocker", "all minimal repairs of size <= max_size",
                 "largest position first", "ascend by candidate position", "UINT32_MAX", "For max_size <= 3 the rows",
                 "nemo_min_repair_sets' / nemo_min_repairs' own, in their order", "decided as round 0 of nemo_min_repair_sets decides it",
                 "every level stat is 0", "level 0 reports 1 set evaluated and 0 found", "Level 0 evaluates S = {}",
                 "frontier of distinct sets of d candidate positions", "is not expanded", "every candidate e in B_{A \\ S} with e not in S",
                 "no proper subset among the repairs of sizes <= d", "stops after level max_size, or at an empty frontier",
                 "Every minimal repair is reached", "has no children: nothing above it is a repair", "checked on the host in this order",
                 "cond outside 0 / 1; max_size outside 1..8 or flags != 0", "max_size must be 1..8", "an absent node >= V_g; an absent node listed twice; "
                 "a candidate listed twice; a candidate that is not in absent", "cand == NULL means cand = absent", "More than 65535 candidates",
                 "eight u16 candidate positions", "the implicit list", "device-made list once its count is known", "NEMO_ERR_STATE before nemo_mark_holds",
                 "a graph without roots and (x, x) give NEMO_REPAIR_HOLDS", "NEMO_ERR_NOTFOUND", "node context", "2^32 - 2 sets",
                 '"lineage_children_max"', "runs again, once", "not appended twice", "block until the rows are on the host",
                 "the next of them or nemo_load_corpus", "both directions", "nemo_lineage_cuts' and the exhaustive repair calls' included",
                 '"wit_lds_max"', '"kl_grid"', "a third u64 word per node and the absent bitmap"):
        assert name in doc, name
    opts = txt[txt.index("Tuning / test knobs"):txt.index("int nemo_set_option")]
    for name in ("the lineage repair calls too", "lineage repair searches' sweeps as well", "lineage repair calls' levels are held to the same limit"):
        assert name in opts, name
    assert E.LINEAGE_REPAIR_DTYPE.itemsize == 36 and E.LINEAGE_REPAIR_DTYPE.names == ("size", "node")
    assert E.LINEAGE_REPAIR_DTYPE["node"].shape == (8,)


def test_library_exports_the_calls():
    if not os.path.exists(E.LIB_PATH):
        subprocess.run(["make", "-s", "-C", ROOT, "nemo_amd/libnemohip.so"], check=True)
    L = ctypes.CDLL(E.LIB_PATH)
    for name in CALLS:
        assert hasattr(L, name), name
    assert L.nemo_abi_version() == 1
    vp, u32, u64, sz = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_size_t
    L.nemo_lineage_repair_sets.argtypes = [vp, u32, ctypes.c_int, vp, sz, vp, sz, u32, u32]
    assert L.nemo_lineage_repair_sets(None, 0, 1, None, 0, None, 0, 3, 0) == 1  # NEMO_ERR_INVALID: a null context, no device
    L.nemo_lineage_repairs.argtypes = [vp, u32, u32, u32, u32]
    assert L.nemo_lineage_repairs(None, 0, 1, 3, 0) == 1
    L.nemo_fetch_lineage_repairs.argtypes = [vp, vp, u64, vp]
    assert L.nemo_fetch_lineage_repairs(None, None, 0, None) == 1
    L.nemo_fetch_lineage_repair_stats.argtypes = [vp, vp]
    assert L.nemo_fetch_lineage_repair_stats(None, None) == 1
    L.nemo_fetch_lineage_repair_cands.argtypes = [vp, vp, u64, vp]
    assert L.nemo_fetch_lineage_repair_cands(None, None, 0, None) == 1


def test_engine_binds_the_calls():
    for name, arity in CALLS.items():
        fn = getattr(E.lib(), name)
        assert len(fn.argtypes) == arity and fn.restype is ctypes.c_int, name
    sig = inspect.signature(E.Engine.lineage_repair_sets)
    assert list(sig.parameters) == ["self", "iteration", "cond", "absent", "candidates", "max_size"]
    assert sig.parameters["candidates"].default is None and sig.parameters["max_size"].default == 3
    assert list(inspect.signature(E.Engine.lineage_repairs).parameters) == ["self", "base", "other", "max_size"]
    for name in ("lineage_repair_rows", "lineage_repair_stats", "lineage_repair_cands"):
        assert list(inspect.signature(getattr(E.Engine, name)).parameters) == ["self"], name
    assert "reshape(9, 2)" in inspect.getsource(E.Engine.lineage_repair_stats)


def test_go_binding_calls_them_as_declared():
    src = open(GO).read()
    funcs, _, _, fields = header_decls()
    calls = {}
    for name, n in go_calls(src):
        calls.setdefault(name, set()).add(n)
    for name in CALLS:
        assert f"C.{name}(" in src, name
        assert calls[name] == {funcs[name]} == {CALLS[name]}, name
    for fn_name, call in (("LineageRepairs", "nemo_lineage_repairs"), ("LineageRepairSets", "nemo_lineage_repair_sets")):
        fn = re.search(r"func \(n \*Neo4J\) %s\(.*?\n}\n" % fn_name, src, flags=re.S)
        assert fn and f"C.{call}(" in fn.group(0) and "n.lineageRepairResult(" in fn.group(0), fn_name
    fetch = re.search(r"func \(n \*Neo4J\) lineageRepairResult\(.*?\n}\n", src, flags=re.S)
    assert fetch and all(f"C.{name}(" in fetch.group(0) for name in CALLS if name.startswith("nemo_fetch"))
    assert "C.nemo_lineage_repair" in fetch.group(0) and "[20]uint64" in fetch.group(0)
    for f in set(re.findall(r"\brep\.(\w+)", fetch.group(0))):
        assert f in fields["nemo_lineage_repair"], f"rep.{f} is not a field of nemo_lineage_repair"


def test_host_header_reuses_and_kernels_share_the_blame_pass():
    hdr = open(os.path.join(CSRC, "lrep_host.h")).read()
    assert "hip_runtime" not in hdr  # pure host functions
    for inc in ('#include "lin_host.h"', '#include "repair_host.h"', '#include "wit_host.h"'):
        assert inc in hdr, inc
    assert "wit::wit_lds_bytes" in hdr and "repair::bitmap_words" in hdr and "repair::status" in hdr
    assert "std::sort" not in hdr and "struct Key" not in hdr  # neither the list checks nor the keys are restated
    down = open(os.path.join(CSRC, "blame_down.h")).read()
    assert "void blame_down(" in down and '#include "wit_down.h"' in down and "wit_or(" in down and "wit_need<LDS>(" in down
    wit = open(os.path.join(CSRC, "wit_down.h")).read()
    assert "blame" not in wit and "void wit_down(const KoImg<LDS> &g, uint64_t *need, uint32_t n, bool all)" in wit  # as it was
    k = open(os.path.join(CSRC, "k_lrepair.hip")).read()
    assert '#include "blame_down.h"' in k and "void blame_down(" not in k
    for name in ("k_lrep_lds", "k_lrep_glob"):
        assert f"void {name}(" in k, name
    assert "lrep_chunk<true>(" in k and "lrep_chunk<false>(" in k and k.count("blame_down<LDS>(g, blame, removed, lost)") == 1
    assert "ko_sweep<LDS>(g)" in k and "lin_emit(a, s_key, k, w)" in k and "lin_cut_insert(a, i, k)" in k and "!a.redo" in k
    assert "k_lin_filter" not in k.split("namespace nemo {")[1]  # the filter and the rehash are used as they are
    api = open(os.path.join(CSRC, "api_lrepair.hip")).read()
    # the level loop and the search's tail are lin_api.h's, included directly: no detour through a second header, no
    # type-erased hook on a per-level path
    tail = open(os.path.join(CSRC, "lin_api.h")).read()
    assert '#include "lin_api.h"' in api and "lin_node_search(c, ls," in api and not os.path.exists(os.path.join(CSRC, "lin_run.h"))
    assert all("lin_run" not in open(os.path.join(CSRC, f)).read() for f in os.listdir(CSRC))
    assert "std::function" not in api and "std::function" not in tail
    assert "lin::level_end(" not in api and "launch_lin_filter(" not in api  # ... once
    assert 'GroupTimer timer(c, "k_lrepair")' in api and "lrep::lds_fits, lrep::lrep_lds_bytes, lrep::glob_words" in api
    assert '"k_lrep_lds"' in api and '"k_lrep_glob"' in api and "ls.glob_node_bytes = 48.0" in api
    for name in ("ko_lds_total(", "c->opt.wit_lds_max", "c->opt.kl_grid"):  # the tier code, once, in the tail
        assert tail.count(name) == 1 and name not in api, name
    # the absent-set front end is repair_api.h's, once, for the four repair calls, each family on its own state
    front = open(os.path.join(CSRC, "repair_api.h")).read()
    api_rep = open(os.path.join(CSRC, "api_repair.hip")).read()
    for name in ("repair::check_lists(", "repair::bitmap(", "launch_repair_absent(", "launch_lab_hash(", "pairs::plan("):
        assert front.count(name) == 1 and name not in api and name not in api_rep, name
    users = [f for f in sorted(os.listdir(CSRC)) if '#include "repair_api.h"' in open(os.path.join(CSRC, f)).read()]
    assert users == ["api_lrepair.hip", "api_repair.hip"]
    for src, own in ((api, "cs.lr_abs, cs.d_lrcand, "), (api_rep, "cs.rp_abs, cs.rp.cand, ")):
        assert src.count("absent_check(c, who,") == 1 and src.count("absent_queue(c, " + own) == 1 and src.count("absent_pair(c, who, " + own) == 1
    assert "lrep::status_of_lost(" in api and "cs.rp" not in api and "d_ln" not in api and "lr_abs" not in api_rep and "d_lr" not in api_rep  # its own state
    ctx = open(os.path.join(CSRC, "ctx.h")).read()
    assert "LinBufs d_lr;" in ctx and "ev_lrep" in ctx and "h_lrep" in ctx
    assert ctx.count("struct AbsentSet {") == 1 and "AbsentSet rp_abs;" in ctx and "AbsentSet lr_abs;" in ctx
    for name in ("rp_bits", "lr_bits", "d_rpcnt", "d_lrcnt", "d_rptab", "d_lrtab", "d_rphreg", "d_lrhreg", "d_rpbits", "d_lrbits"):
        assert name not in ctx, name
    # the fetches' copy and its messages: knock_api.h's, once
    shared = open(os.path.join(CSRC, "knock_api.h")).read()
    assert shared.count("static inline int fetch_result(") == 1 and shared.count("(or after a later nemo_load_corpus)") == 1
    assert shared.count('"capacity too small"') == 1
    for f in ("api_cuts.hip", "api_repair.hip", "api_lineage.hip", "api_lgcuts.hip", "api_lrepair.hip", "cut_api.h", "lin_api.h", "repair_api.h"):
        src = open(os.path.join(CSRC, f)).read()
        assert "capacity too small" not in src and "after a later nemo_load_corpus" not in src, f
        assert ("fetch_result(c, " in src) == f.startswith("api_"), f


def test_host_check_program_passes_under_the_host_sanitizers(tmp_path):
    src = os.path.join(ROOT, "tools", "lrepair_host_check.cpp")
    text = open(src).read()
    assert "int main()" in text and '#include "../nemo_amd/csrc/lrep_host.h"' in text
    mk = open(os.path.join(ROOT, "tools", "Makefile")).read()
    assert "-fsanitize=address,undefined" in mk and "lrepair_host_check.cpp" in mk
    if shutil.which("g++") is None and shutil.which("c++") is None:
        pytest.fail("no host C++ compiler to build tools/lrepair_host_check.cpp")
    exe = str(tmp_path / "lrepair_host_check")
    # tools/Makefile's rule, the binary in the test's own folder; the sanitizer runtimes are linked into the
    # program itself: it runs as it is, whatever else the loader brings
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tools"), "-B", "lrepair_host_check", f"LREPAIR_CHECK={exe}"], check=True)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    assert run.stdout.rstrip().endswith("lrepair_host_check OK")
