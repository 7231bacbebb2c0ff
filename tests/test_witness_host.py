"""Host-side checks of the surviving derivations (no GPU): the C ABI declares and exports nemo_witness_sets,
nemo_witness_labels and their two fetches, the struct and the three flags; the Python and Go bindings call them as
declared; the semantics, the error codes, the limits and the option are documented; the host arithmetic
(nemo_amd/csrc/wit_host.h) passes its stand-alone check program under the host sanitizers; and witness_edges /
witness_support / witness_dot turn a hand-written mask into the witness's edges, base events and drawing."""
import ctypes
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from nemo_amd import engine as E
from nemo_amd.corpus import NODE_RULE, Corpus
from nemo_amd.dot import read_dot
from tests.test_go_binding import go_calls, header_decls

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GO = os.path.join(ROOT, "go", "graphing", "nemohip.go")
CALLS = {"nemo_witness_sets": 7, "nemo_witness_labels": 8, "nemo_fetch_witness": 4, "nemo_fetch_witness_mask": 4}
FIELDS = ("graph", "n_roots", "roots_alive", "n_nodes", "n_sinks")


def test_header_declares_the_calls():
    funcs, defines, types, fields = header_decls()
    for name, arity in CALLS.items():
        assert name in E.header_symbols()
        assert funcs[name] == arity, name
    assert "nemo_witness" in types and fields["nemo_witness"] == set(FIELDS)
    assert {"NEMO_WIT_ALL", "NEMO_WIT_MASKS", "NEMO_WIT_SINKS"} <= defines
    txt = open(E.HEADER).read()
    assert "#define NEMOHIP_ABI_VERSION 1" in txt  # additive
    for line in ("#define NEMO_WIT_ALL 1u", "#define NEMO_WIT_MASKS 2u", "#define NEMO_WIT_SINKS 4u"):
        assert line in txt, line
    start = txt.index("surviving derivations: why a run's outcome withstands a fault set")
    assert txt.index("int nemo_fetch_knockout_mask") < start < txt.index("corrections / extensions on run 0")
    doc = txt[start:txt.index("int nemo_fetch_witness_mask")]
    for name in ("alive = not dead", "an alive rule has only alive\n * children", "at least one alive child", "roots first",
                 "a root is needed iff it is alive", "a needed rule needs every child", "smallest node index", "NEMO_WIT_ALL",
                 "needs every alive child", "needs nothing further", "node's own kind", "union of all remaining derivations",
                 "first alive child\n * in row order", "nemo_knockout_sets'", "nemo_knockout_labels'", "i * n_sets + s",
                 "NEMO_WIT_SINKS is NEMO_ERR_INVALID here", "2^32 - 2", "2^28", "2^36 bytes", "tile the call", "empty set",
                 "graph without roots", "every root\n * dead", "named twice", "no listed node carries", "listed twice",
                 "n_sets == 0 or\n * n == 0", "NEMO_ERR_NOTFOUND", "NEMO_ERR_STATE", "NEMO_ERR_LIMIT", "node context",
                 "next witness call or nemo_load_corpus", "both directions", "wit_lds_max", "1 = in W_h"):
        assert name in doc, name
    opts = txt[txt.index("Tuning / test knobs"):txt.index("int nemo_set_option")]
    assert '"wit_lds_max"' in opts and "nemo_witness_sets" in opts and "second u64 word per node" in opts
    assert E.WITNESS_DTYPE.itemsize == 20 and E.WITNESS_DTYPE.names == FIELDS
    assert (E.WIT_ALL, E.WIT_MASKS, E.WIT_SINKS) == (1, 2, 4)


def test_library_exports_the_calls():
    if not os.path.exists(E.LIB_PATH):
        subprocess.run(["make", "-s", "-C", ROOT, "nemo_amd/libnemohip.so"], check=True)
    L = ctypes.CDLL(E.LIB_PATH)
    for name in CALLS:
        assert hasattr(L, name), name
    assert L.nemo_abi_version() == 1
    vp, u32, u64, sz = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_size_t
    L.nemo_witness_sets.argtypes = [vp, u32, ctypes.c_int, vp, vp, sz, u32]
    assert L.nemo_witness_sets(None, 0, 1, None, None, 0, 0) == 1  # NEMO_ERR_INVALID: a null context, no device
    L.nemo_witness_labels.argtypes = [vp, vp, sz, ctypes.c_int, vp, vp, sz, u32]
    assert L.nemo_witness_labels(None, None, 0, 1, None, None, 0, 0) == 1
    L.nemo_fetch_witness.argtypes = [vp, vp, u64, vp]
    assert L.nemo_fetch_witness(None, None, 0, None) == 1
    L.nemo_fetch_witness_mask.argtypes = [vp, u64, vp, u64]
    assert L.nemo_fetch_witness_mask(None, 0, None, 0) == 1


def test_engine_binds_the_calls():
    for name, arity in CALLS.items():
        fn = getattr(E.lib(), name)
        assert len(fn.argtypes) == arity and fn.restype is ctypes.c_int, name
    sig = inspect.signature(E.Engine.witness_sets)
    assert list(sig.parameters) == ["self", "iteration", "cond", "sets", "all", "masks"]
    sig = inspect.signature(E.Engine.witness_labels)
    assert list(sig.parameters) == ["self", "iters", "cond", "sets", "all", "masks", "sinks_only"]
    assert all(sig.parameters[k].default is False for k in ("all", "masks", "sinks_only"))
    assert list(inspect.signature(E.Engine.witness_rows).parameters) == ["self"]
    assert list(inspect.signature(E.Engine.witness_mask).parameters) == ["self", "hyp", "n_nodes"]
    assert list(inspect.signature(E.witness_edges).parameters) == ["corpus", "g", "mask", "all"]


def test_go_binding_calls_them_as_declared():
    src = open(GO).read()
    funcs, _, _, fields = header_decls()
    calls = {}
    for name, n in go_calls(src):
        calls.setdefault(name, set()).add(n)
    for name in CALLS:
        assert f"C.{name}(" in src, name
        assert calls[name] == {funcs[name]} == {CALLS[name]}, name
    sets = re.search(r"func \(n \*Neo4J\) WitnessSets\(.*?\n}\n", src, flags=re.S)
    labels = re.search(r"func \(n \*Neo4J\) WitnessLabels\(.*?\n}\n", src, flags=re.S)
    rows = re.search(r"func \(n \*Neo4J\) witnessRows\(.*?\n}\n", src, flags=re.S)
    assert sets and labels and rows
    assert "C.nemo_witness_sets(" in sets.group(0) and "C.nemo_witness_labels(" in labels.group(0)
    assert "C.NEMO_WIT_SINKS" in labels.group(0) and "C.NEMO_WIT_ALL" in src and "C.NEMO_WIT_MASKS" in src
    assert "C.nemo_fetch_witness(" in rows.group(0) and "C.nemo_fetch_witness_mask(" in rows.group(0) and "C.nemo_witness" in rows.group(0)
    for f in set(re.findall(r"\bw\.(\w+)", rows.group(0))):
        assert f in fields["nemo_witness"], f"w.{f} is not a field of nemo_witness"


def test_host_check_program_passes_under_the_host_sanitizers(tmp_path):
    src = os.path.join(ROOT, "tools", "wit_host_check.cpp")
    text = open(src).read()
    assert "int main()" in text and '#include "../nemo_amd/csrc/wit_host.h"' in text
    hdr = open(os.path.join(ROOT, "nemo_amd", "csrc", "wit_host.h")).read()
    assert "hip_runtime" not in hdr  # pure host functions
    for inc in ('#include "klabel_host.h"', '#include "knock_host.h"', '#include "lcut_host.h"'):  # reused, not copied
        assert inc in hdr, inc
    assert "knock::knock_lds_bytes" in hdr and "lcuts::region_words" in hdr and "KO_MAX_HYPS" in hdr
    mk = open(os.path.join(ROOT, "tools", "Makefile")).read()
    assert "-fsanitize=address,undefined" in mk and "wit_host_check.cpp" in mk
    if shutil.which("g++") is None and shutil.which("c++") is None:
        pytest.fail("no host C++ compiler to build tools/wit_host_check.cpp")
    exe = str(tmp_path / "wit_host_check")
    # tools/Makefile's rule, the binary in the test's own folder; the sanitizer runtimes are linked into the
    # program itself: it runs as it is, whatever else the loader brings
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tools"), "-B", "wit_host_check", f"WIT_CHECK={exe}"], check=True)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    assert run.stdout.rstrip().endswith("wit_host_check OK")


def test_edges_and_support_of_a_hand_written_mask():
    """pre graph: one goal.  post graph: goal 0 <- rules 1, 2; rule 1 <- leaves 3, 4; rule 2 <- leaves 4, 5; goal 6 <-
    rule 7 (no children).  Edges are given out of order: the helpers go by child index, not by edge order."""
    kinds = "grrggggr"
    edges = [(2, 5), (0, 2), (1, 4), (0, 1), (2, 4), (1, 3), (6, 7)]
    word = [0] + [(NODE_RULE | 2) if k == "r" else 2 for k in kinds]
    u32 = lambda x: np.ascontiguousarray(x, dtype=np.uint32)
    corpus = Corpus(iteration=u32([0]), node_off=np.array([0, 1, 9], np.uint64), edge_off=np.array([0, 0, 7], np.uint64),
                    node_word=u32(word), label=u32([9, 10, 11, 12, 13, 14, 15, 16, 17]), edge_src=u32([a for a, _ in edges]),
                    edge_dst=u32([b for _, b in edges]), n_tables=3, table_pre=0, table_post=1, status=["success"])
    one = np.array([1, 1, 0, 1, 1, 0, 1, 1], np.uint8)  # the derivation through rule 1, and the second root's
    assert E.witness_edges(corpus, 1, one).tolist() == [[0, 1], [1, 3], [1, 4], [6, 7]]
    assert E.witness_support(corpus, 1, one) == [(3, 13, None), (4, 14, None)]
    every = np.array([1, 1, 1, 1, 1, 1, 1, 1], np.uint8)
    assert E.witness_edges(corpus, 1, every).tolist() == [[0, 1], [1, 3], [1, 4], [2, 4], [2, 5], [6, 7]]  # a goal keeps one edge
    assert E.witness_edges(corpus, 1, every, all=True).tolist() == [[0, 1], [0, 2], [1, 3], [1, 4], [2, 4], [2, 5], [6, 7]]
    assert [v for v, _, _ in E.witness_support(corpus, 1, every)] == [3, 4, 5]
    through2 = np.array([1, 0, 1, 0, 1, 1, 0, 0], np.uint8)  # rule 1 dead: the goal's smallest child in W is rule 2
    assert E.witness_edges(corpus, 1, through2).tolist() == [[0, 2], [2, 4], [2, 5]]
    none = np.zeros(8, np.uint8)
    assert E.witness_edges(corpus, 1, none).shape == (0, 2) and E.witness_support(corpus, 1, none) == []
    assert E.witness_edges(corpus, 0, np.ones(1, np.uint8)).shape == (0, 2) and E.witness_support(corpus, 0, np.ones(1, np.uint8)) == [(0, 9, None)]
    back = read_dot(str(E.witness_dot(corpus, 1, one)))
    assert len(back.edges) == 4
