"""ctypes binding of libnemohip (include/nemohip.h) and a phase-level engine.

This is the Python equivalent of the cgo stub in INTEGRATION.md: it only moves
interned arrays across the C ABI and calls the gfx950 kernels.  There is no
fallback: if libnemohip.so is missing or no HIP device is present, every entry
point raises.
"""
from __future__ import annotations

import ctypes
import os
import re
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence

import numpy as np

from .corpus import CChain, CMissing, Corpus

_HERE = os.path.dirname(os.path.abspath(__file__))
# NEMO_LIB: a variant build of the same library (A/B kernel experiments: tools/variants.sh)
LIB_PATH = os.environ.get("NEMO_LIB") or os.path.join(_HERE, "libnemohip.so")
HEADER = os.path.join(os.path.dirname(_HERE), "include", "nemohip.h")
_LIB = None


class NemoError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"[nemo {code}] {msg}")
        self.code = code
        self.msg = msg


class CTiming(ctypes.Structure):
    _fields_ = [("name", ctypes.c_char * 32), ("launches", ctypes.c_uint64), ("ms", ctypes.c_double),
                ("bytes", ctypes.c_double), ("edges", ctypes.c_double)]


# struct nemo_nearest (nemo_fetch_nearest)
NEAREST_DTYPE = np.dtype([("cand", np.uint32), ("dist", np.uint32), ("only_query", np.uint32), ("only_cand", np.uint32)])
# struct nemo_knock (nemo_fetch_knockout)
KNOCK_DTYPE = np.dtype([("graph", np.uint32), ("node", np.uint32), ("n_dead", np.uint32), ("roots_dead", np.uint32),
                        ("n_roots", np.uint32)])
KO_MASKS = 1  # NEMO_KO_MASKS
# nemo_fetch_min_repair_stats' out[0] (NEMO_REPAIR_*)
REPAIR_HOLDS, REPAIR_SEARCHED, REPAIR_BEYOND = 0, 1, 2
# struct nemo_cut (nemo_fetch_min_cuts)
CUT_DTYPE = np.dtype([("size", np.uint32), ("node", np.uint32, (3,))])
KL_SINKS = 1  # NEMO_KL_SINKS
# struct nemo_label_cut (nemo_fetch_min_label_cuts)
LABEL_CUT_DTYPE = np.dtype([("size", np.uint32), ("label", np.uint32, (3,))])
# struct nemo_group_cut (nemo_fetch_min_group_cuts)
GROUP_CUT_DTYPE = np.dtype([("size", np.uint32), ("group", np.uint32, (3,))])
# struct nemo_witness (nemo_fetch_witness)
WITNESS_DTYPE = np.dtype([("graph", np.uint32), ("n_roots", np.uint32), ("roots_alive", np.uint32), ("n_nodes", np.uint32),
                          ("n_sinks", np.uint32)])
WIT_ALL, WIT_MASKS, WIT_SINKS = 1, 2, 4  # NEMO_WIT_ALL, NEMO_WIT_MASKS, NEMO_WIT_SINKS
# struct nemo_lineage_cut (nemo_fetch_lineage_cuts)
LINEAGE_CUT_DTYPE = np.dtype([("size", np.uint32), ("node", np.uint32, (8,))])
# struct nemo_lineage_repair (nemo_fetch_lineage_repairs): nemo_lineage_cut's layout
LINEAGE_REPAIR_DTYPE = np.dtype([("size", np.uint32), ("node", np.uint32, (8,))])
# struct nemo_lineage_group_cut (nemo_fetch_lineage_group_cuts)
LINEAGE_GROUP_CUT_DTYPE = np.dtype([("size", np.uint32), ("group", np.uint32, (8,))])


def header_symbols() -> List[str]:
    """Every function the C ABI header declares."""
    txt = open(HEADER).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(nemo_[a-z0-9_]+)\s*\(", txt)))


def lib():
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"libnemohip.so not built ({LIB_PATH}); run `make` or __graft_entry__.build()")
        # One HIP runtime per process: PyTorch-ROCm ships its own libamdhip64 under another file name,
        # so loading libnemohip (which resolves /opt/rocm's libamdhip64.so.7) before torch would leave
        # torch with a second runtime that cannot open the device ("No HIP GPUs are available").
        # Loading torch first makes libnemohip bind to the runtime torch already holds (same soname).
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        L = ctypes.CDLL(LIB_PATH)
        vp, u32, u64, sz, i32 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_size_t, ctypes.c_int
        P = ctypes.POINTER
        sig = {
            "nemo_abi_version": ([], i32),
            "nemo_partition_runs": ([vp, u32, vp], i32),
            "nemo_ctx_create": ([i32, P(vp)], i32),
            "nemo_ctx_create_node": ([i32, vp, P(vp)], i32),
            "nemo_node_devices": ([vp, vp, i32], i32),
            "nemo_ctx_destroy": ([vp], None),
            "nemo_last_error": ([vp], ctypes.c_char_p),
            "nemo_set_stream": ([vp, vp], i32),
            "nemo_set_timing": ([vp, i32], i32),
            "nemo_set_timing_groups": ([vp, ctypes.c_char_p], i32),
            "nemo_set_option": ([vp, ctypes.c_char_p, ctypes.c_int64], i32),
            "nemo_load_corpus": ([vp, vp], i32),
            "nemo_host_register": ([vp, u64], i32),
            "nemo_host_unregister": ([vp], i32),
            "nemo_rebuild": ([vp], i32),
            "nemo_num_nodes": ([vp], u64),
            "nemo_num_edges": ([vp], u64),
            "nemo_mark_holds": ([vp], i32),
            "nemo_simplify": ([vp], i32),
            "nemo_reduce_len": ([vp], sz),
            "nemo_protos_partial": ([vp, vp, sz, vp], i32),
            "nemo_protos_stage": ([vp, vp], i32),
            "nemo_protos_finalize": ([vp, vp, P(u32), vp, P(u32), vp, P(u32), P(u64), P(u32)], i32),
            "nemo_fetch_reduce": ([vp, vp, u64], i32),
            "nemo_prototypes": ([vp, vp, sz, P(u32), vp, P(u32), vp, P(u32)], i32),
            "nemo_missing_from": ([vp, u32, vp, u32, vp, P(u32)], i32),
            "nemo_diffprov": ([vp, vp, sz, i32], i32),
            "nemo_diffprov_labels": ([vp, vp, sz, vp, u64], i32),
            "nemo_diffprov_host_labels": ([vp, vp, sz, vp, u64], i32),
            "nemo_goal_labels": ([vp, u32, i32, vp, u64], i32),
            "nemo_fetch_diff_mask": ([vp, u32, vp, u64], i32),
            "nemo_fetch_missing": ([vp, vp, u64, P(u64)], i32),
            "nemo_fetch_diff_masks": ([vp, vp, u64], i32),
            "nemo_diff_masks_view": ([vp, vp, vp, vp], i32),
            "nemo_diff_classes": ([vp], i32),
            "nemo_fetch_diff_classes": ([vp, vp, vp, u64, P(u64)], i32),
            "nemo_fetch_diff_support": ([vp, vp, u64], i32),
            "nemo_diffprov_symmetric": ([vp, vp, sz], i32),
            "nemo_diffprov_pairs": ([vp, vp, vp, sz], i32),
            "nemo_fetch_sdiff_masks": ([vp, vp, vp, u64, P(u64)], i32),
            "nemo_fetch_surplus": ([vp, vp, u64, P(u64)], i32),
            "nemo_nearest_runs": ([vp, vp, sz, vp, sz], i32),
            "nemo_fetch_nearest": ([vp, vp, u64, P(u64)], i32),
            "nemo_fetch_label_distances": ([vp, u32, u32, vp, u64], i32),
            "nemo_knockout_leaves": ([vp, vp, sz, i32, u32], i32),
            "nemo_knockout_sets": ([vp, u32, i32, vp, vp, sz, u32], i32),
            "nemo_fetch_knockout": ([vp, vp, u64, P(u64)], i32),
            "nemo_fetch_knockout_ranges": ([vp, vp, vp, u64], i32),
            "nemo_fetch_knockout_mask": ([vp, u64, vp, u64], i32),
            "nemo_min_cuts": ([vp, u32, i32, vp, sz, u32, u32], i32),
            "nemo_fetch_min_cuts": ([vp, vp, u64, P(u64)], i32),
            "nemo_fetch_min_cut_stats": ([vp, vp], i32),
            "nemo_min_repair_sets": ([vp, u32, i32, vp, sz, vp, sz, u32, u32], i32),
            "nemo_min_repairs": ([vp, u32, u32, u32, u32], i32),
            "nemo_fetch_min_repairs": ([vp, vp, u64, P(u64)], i32),
            "nemo_fetch_min_repair_stats": ([vp, vp], i32),
            "nemo_fetch_min_repair_cands": ([vp, vp, u64, P(u64)], i32),
            "nemo_lineage_repair_sets": ([vp, u32, i32, vp, sz, vp, sz, u32, u32], i32),
            "nemo_lineage_repairs": ([vp, u32, u32, u32, u32], i32),
            "nemo_fetch_lineage_repairs": ([vp, vp, u64, P(u64)], i32),
            "nemo_fetch_lineage_repair_stats": ([vp, vp], i32),
            "nemo_fetch_lineage_repair_cands": ([vp, vp, u64, P(u64)], i32),
            "nemo_lineage_cuts": ([vp, u32, i32, vp, sz, u32, u32], i32),
            "nemo_fetch_lineage_cuts": ([vp, vp, u64, P(u64)], i32),
            "nemo_fetch_lineage_cut_stats": ([vp, vp], i32),
            "nemo_knockout_labels": ([vp, vp, sz, i32, vp, vp, sz, u32], i32),
            "nemo_fetch_knockout_labels": ([vp, vp, vp, u64], i32),
            "nemo_fetch_knockout_label_counts": ([vp, vp, vp, u64], i32),
            "nemo_min_label_cuts": ([vp, vp, sz, i32, vp, sz, u32, u32, u32], i32),
            "nemo_fetch_min_label_cuts": ([vp, vp, vp, u64, P(u64)], i32),
            "nemo_fetch_min_label_cut_stats": ([vp, vp], i32),
            "nemo_min_group_cuts": ([vp, vp, sz, i32, vp, vp, sz, u32, u32, u32], i32),
            "nemo_fetch_min_group_cuts": ([vp, vp, vp, u64, P(u64)], i32),
            "nemo_fetch_min_group_cut_stats": ([vp, vp], i32),
            "nemo_lineage_group_cuts": ([vp, vp, sz, i32, vp, vp, sz, u32, u32, u32], i32),
            "nemo_fetch_lineage_group_cuts": ([vp, vp, vp, u64, P(u64)], i32),
            "nemo_fetch_lineage_group_cut_stats": ([vp, vp], i32),
            "nemo_witness_sets": ([vp, u32, i32, vp, vp, sz, u32], i32),
            "nemo_witness_labels": ([vp, vp, sz, i32, vp, vp, sz, u32], i32),
            "nemo_fetch_witness": ([vp, vp, u64, P(u64)], i32),
            "nemo_fetch_witness_mask": ([vp, u64, vp, u64], i32),
            "nemo_triggers": ([vp], i32),
            "nemo_fetch_triggers": ([vp, vp, u64, P(u64), vp, u64, P(u64), vp, u64, P(u64)], i32),
            "nemo_fetch_node_flags": ([vp, u32, u32, vp, u64], i32),
            "nemo_fetch_chains": ([vp, vp, u64, P(u64)], i32),
            "nemo_stage_simplified": ([vp], i32),
            "nemo_simplified_view": ([vp, P(vp), P(vp), P(vp), P(u64)], i32),
            "nemo_fetch_run_tables": ([vp, i32, vp, u64], i32),
            "nemo_pull_edges": ([vp, i32], i32),
            "nemo_reduce_interpret": ([vp, u32, u32, P(u32), vp, P(u32), vp, P(u32)], i32),
            "nemo_pulled_count": ([vp, u32], u64),
            "nemo_fetch_pulled": ([vp, u32, vp, vp, u64, P(u64)], i32),
            "nemo_fetch_pulled_all": ([vp, vp, vp, vp, vp, u64, P(u64)], i32),
            "nemo_timings": ([vp, vp, u32, P(u32)], i32),
            "nemo_reset_timings": ([vp], i32),
            "nemo_synchronize": ([vp], i32),
            "nemo_debug_copy": ([vp, ctypes.c_char_p, vp, u64, u64], i32),
        }
        for name, (args, res) in sig.items():
            fn = getattr(L, name)
            fn.argtypes = args
            fn.restype = res
        _LIB = L
    return _LIB


def _p(a: Optional[np.ndarray]):
    return None if a is None or a.size == 0 else a.ctypes.data


PIN_FIELDS = ("node_word", "label", "edge_src", "edge_dst", "id_rank")


def pin_corpus(corpus: Corpus) -> list:
    """Page-lock a corpus' large host arrays (nemo_host_register) so that every nemo_load_corpus of it
    uploads by DMA; returns the registered arrays for unpin_corpus."""
    L = lib()
    pinned = []
    for k in PIN_FIELDS:
        a = getattr(corpus, k, None)
        if a is None or a.size == 0 or not a.flags["C_CONTIGUOUS"]:
            continue
        if L.nemo_host_register(a.ctypes.data, a.nbytes) == 0:
            pinned.append(a)
    return pinned


def unpin_corpus(pinned: list) -> None:
    L = lib()
    for a in pinned:
        L.nemo_host_unregister(a.ctypes.data)


def _graph_rows(corpus: Corpus, g: int):
    """(is_rule [V], children per node in ascending order) of graph g, from the host arrays"""
    n0, n1 = int(corpus.node_off[g]), int(corpus.node_off[g + 1])
    e0, e1 = int(corpus.edge_off[g]), int(corpus.edge_off[g + 1])
    rule = (corpus.node_word[n0:n1] & np.uint32(0x80000000)) != 0
    ch: List[List[int]] = [[] for _ in range(n1 - n0)]
    for s, d in zip(corpus.edge_src[e0:e1].tolist(), corpus.edge_dst[e0:e1].tolist()):
        ch[s].append(d)
    for row in ch:
        row.sort()
    return rule, ch


def witness_edges(corpus: Corpus, g: int, mask: np.ndarray, all: bool = False) -> np.ndarray:
    """The edges of a witness W of graph g (mask: Engine.witness_mask's bytes), as [k, 2] local (source, target)
    pairs sorted by (source, target): a rule in W keeps every forward edge, a goal in W the edge to its
    smallest-index child in W, or under `all` (a mask of a NEMO_WIT_ALL call) every edge to a child in W.
    witness_dot() turns them into a graph of nemo_amd.dot."""
    rule, ch = _graph_rows(corpus, g)
    out = []
    for v in np.flatnonzero(np.asarray(mask[:len(ch)])).tolist():
        if rule[v]:
            out += [(v, c) for c in ch[v]]
        else:
            kept = [c for c in ch[v] if mask[c]]
            out += [(v, c) for c in (kept if all else kept[:1])]
    return np.asarray(out, dtype=np.uint32).reshape(-1, 2)


def witness_support(corpus: Corpus, g: int, mask: np.ndarray):
    """The base events a witness rests on: [(local node, label id, label string or None)] of the sink goals (goals
    without children) of graph g that are in W, in node-index order."""
    rule, ch = _graph_rows(corpus, g)
    n0 = int(corpus.node_off[g])
    out = []
    for v in np.flatnonzero(np.asarray(mask[:len(ch)])).tolist():
        if not rule[v] and not ch[v]:
            lab = int(corpus.label[n0 + v])
            out.append((v, lab, corpus.labels[lab] if corpus.labels is not None and lab < len(corpus.labels) else None))
    return out


def repair_labels(corpus: Corpus, g: int, rows: np.ndarray) -> List[List[str]]:
    """The rows of Engine.min_repairs / min_repair_sets on graph g as label strings, for a report: per row the labels
    of its nodes in row order (the label id as a string where the corpus keeps no string table)."""
    n0 = int(corpus.node_off[g])
    out = []
    for row in np.asarray(rows, dtype=np.uint32).reshape(-1, 4).tolist():
        labs = []
        for v in row[1:1 + row[0]]:
            lab = int(corpus.label[n0 + v])
            labs.append(corpus.labels[lab] if corpus.labels is not None and lab < len(corpus.labels) else str(lab))
        out.append(labs)
    return out


def witness_dot(corpus: Corpus, g: int, mask: np.ndarray, all: bool = False):
    """witness_edges as a nemo_amd.dot.DotGraph (create_dot's drawing of a pre / post graph), to stand beside the
    diff graphs in a report."""
    from .dot import ProvNode, create_dot
    n0 = int(corpus.node_off[g])
    cache: Dict[int, object] = {}

    def node(i: int):
        if i not in cache:
            w = int(corpus.node_word[n0 + i])
            is_rule = bool(w & 0x80000000)
            lab = int(corpus.label[n0 + i])
            label = corpus.labels[lab] if corpus.labels is not None and lab < len(corpus.labels) else str(lab)
            table = corpus.tables[w & 0x00FFFFFF] if corpus.tables is not None else str(w & 0x00FFFFFF)
            id_ = corpus.node_ids[n0 + i] if corpus.node_ids is not None else f"g{g}_n{i}"
            typ = corpus.node_types[n0 + i] if is_rule and corpus.node_types is not None else None
            cache[i] = ProvNode(id_, label, table, typ, None, is_rule)
        return cache[i]

    return create_dot([(node(int(s)), node(int(d))) for s, d in witness_edges(corpus, g, mask, all)], "pre" if g % 2 == 0 else "post")


class Engine:
    """One libnemohip context bound to one HIP device."""

    def __init__(self, device: int = 0, devices: Optional[Sequence[int]] = None):
        """devices: a node context over these devices (nemo_ctx_create_node; repeats allowed)."""
        self.L = lib()
        h = ctypes.c_void_p()
        if devices is None:
            rc = self.L.nemo_ctx_create(device, ctypes.byref(h))
        else:
            d = np.ascontiguousarray(devices, dtype=np.int32)
            rc = self.L.nemo_ctx_create_node(len(d), d.ctypes.data, ctypes.byref(h))
        if rc != 0:
            raise NemoError(rc, "context creation failed (no HIP device?)")
        self.h = h
        self.corpus: Optional[Corpus] = None
        self._n_sym = 0  # entries of the last diffprov_symmetric

    def devices(self) -> List[int]:
        out = np.zeros(64, np.int32)
        n = self.L.nemo_node_devices(self.h, out.ctypes.data, 64)
        return out[:n].tolist()

    def close(self) -> None:
        if self.h:
            self.L.nemo_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc: int) -> None:
        if rc != 0:
            raise NemoError(rc, self.L.nemo_last_error(self.h).decode())

    # ---- phases -------------------------------------------------------------------
    def set_stream(self, stream_handle: int) -> None:
        self._chk(self.L.nemo_set_stream(self.h, ctypes.c_void_p(stream_handle)))

    def set_option(self, name: str, value: int) -> None:
        self._chk(self.L.nemo_set_option(self.h, name.encode(), int(value)))

    def set_timing(self, on: bool = True) -> None:
        self._chk(self.L.nemo_set_timing(self.h, int(on)))

    def set_timing_groups(self, groups: Sequence[str] = ()) -> None:
        """Time only these groups (empty: every group)."""
        self._chk(self.L.nemo_set_timing_groups(self.h, ",".join(groups).encode()))

    def load(self, corpus: Corpus) -> None:
        cs = corpus.c_struct()
        self._chk(self.L.nemo_load_corpus(self.h, ctypes.byref(cs)))
        self.corpus = corpus

    def rebuild(self) -> None:
        self._chk(self.L.nemo_rebuild(self.h))

    def mark(self) -> None:
        self._chk(self.L.nemo_mark_holds(self.h))

    def simplify(self) -> None:
        self._chk(self.L.nemo_simplify(self.h))

    def reduce_len(self) -> int:
        return int(self.L.nemo_reduce_len(self.h))

    def protos_partial(self, success: Sequence[int], d_reduce_ptr: int) -> None:
        s = np.ascontiguousarray(success, dtype=np.uint32)
        self._chk(self.L.nemo_protos_partial(self.h, _p(s), len(s), ctypes.c_void_p(d_reduce_ptr)))

    def reduce_vector(self) -> np.ndarray:
        """nemo_fetch_reduce: the context's own reduction vector (after protos_partial(.., 0))."""
        n = self.reduce_len()
        out = np.zeros(n, np.uint32)
        self._chk(self.L.nemo_fetch_reduce(self.h, _p(out), n))
        return out

    def protos_stage(self, d_reduce_ptr: int) -> None:
        """nemo_protos_stage: queue the (reduced) vector's D2H now; protos_finalize then only waits."""
        self._chk(self.L.nemo_protos_stage(self.h, ctypes.c_void_p(d_reduce_ptr)))

    def protos_finalize(self, d_reduce_ptr: int):
        T = self.corpus.n_tables
        inter = np.zeros(T + 1, np.uint32)
        uni = np.zeros(T + 1, np.uint32)
        a, ni, nu, nr = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32()
        ph = ctypes.c_uint64()
        self._chk(self.L.nemo_protos_finalize(self.h, ctypes.c_void_p(d_reduce_ptr), ctypes.byref(a), _p(inter),
                                              ctypes.byref(ni), _p(uni), ctypes.byref(nu), ctypes.byref(ph),
                                              ctypes.byref(nr)))
        return {"achieved": a.value, "inter": inter[:ni.value].tolist(), "union": uni[:nu.value].tolist(),
                "pre_holds": ph.value, "n_runs": nr.value}

    def prototypes(self, success: Sequence[int]):
        s = np.ascontiguousarray(success, dtype=np.uint32)
        T = self.corpus.n_tables
        inter = np.zeros(T + 1, np.uint32)
        uni = np.zeros(T + 1, np.uint32)
        a, ni, nu = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32()
        self._chk(self.L.nemo_prototypes(self.h, _p(s), len(s), ctypes.byref(a), _p(inter), ctypes.byref(ni),
                                         _p(uni), ctypes.byref(nu)))
        return a.value, inter[:ni.value].tolist(), uni[:nu.value].tolist()

    def missing_from(self, failed_iter: int, proto: Sequence[int]) -> List[int]:
        p = np.ascontiguousarray(proto, dtype=np.uint32)
        out = np.zeros(len(p) + 1, np.uint32)
        n = ctypes.c_uint32()
        self._chk(self.L.nemo_missing_from(self.h, failed_iter, _p(p), len(p), _p(out), ctypes.byref(n)))
        return out[:n.value].tolist()

    def diffprov(self, failed: Sequence[int], mode: int = 0) -> None:
        f = np.ascontiguousarray(failed, dtype=np.uint32)
        self._chk(self.L.nemo_diffprov(self.h, _p(f), len(f), mode))

    def diffprov_symmetric(self, failed: Sequence[int]) -> None:
        """nemo_diffprov_symmetric: for every entry, the part of its failed run's post provenance
        that run 0 lacks (S masks, surplus events; pull(3) for the induced edges)."""
        f = np.ascontiguousarray(failed, dtype=np.uint32)
        self._chk(self.L.nemo_diffprov_symmetric(self.h, _p(f), len(f)))
        self._n_sym = len(f) if 0 in set(int(x) for x in self.corpus.iteration) else 0

    def diffprov_pairs(self, base: Sequence[int], other: Sequence[int]) -> None:
        """nemo_diffprov_pairs: for every pair (base[e], other[e]) of loaded runs, the part of the base
        run's post provenance that the other run lacks.  sdiff_masks(), surplus() and pull(3) then
        return its results, slot = entry, over the base run's post graph."""
        b = np.ascontiguousarray(base, dtype=np.uint32)
        o = np.ascontiguousarray(other, dtype=np.uint32)
        if len(b) != len(o):
            raise ValueError("diffprov_pairs: base and other differ in length")
        self._n_sym = 0
        self._chk(self.L.nemo_diffprov_pairs(self.h, _p(b), _p(o), len(b)))
        self._n_sym = len(b)

    def nearest_runs(self, queries: Sequence[int], candidates: Sequence[int]) -> np.ndarray:
        """nemo_nearest_runs: for every query iteration, the position in `candidates` of the run whose
        post-goal label set is nearest to its own (ties to the smallest position, the query's own run
        skipped).  Returns the rows as a structured array (NEAREST_DTYPE: cand, dist, only_query,
        only_cand; all UINT32_MAX where no candidate is left)."""
        q = np.ascontiguousarray(queries, dtype=np.uint32)
        c = np.ascontiguousarray(candidates, dtype=np.uint32)
        self._near = (0, 0)
        self._chk(self.L.nemo_nearest_runs(self.h, _p(q), len(q), _p(c), len(c)))
        self._near = (len(q), len(c))
        n = ctypes.c_uint64()
        self._chk(self.L.nemo_fetch_nearest(self.h, None, 0, ctypes.byref(n)))
        out = np.zeros(n.value, NEAREST_DTYPE)
        self._chk(self.L.nemo_fetch_nearest(self.h, _p(out), len(out), ctypes.byref(n)))
        return out

    def label_distances(self, q_lo: int = 0, q_hi: Optional[int] = None) -> np.ndarray:
        """nemo_fetch_label_distances: rows [q_lo, q_hi) of the last nearest_runs call's distance matrix,
        [q_hi - q_lo, n_candidates] u32 (self-pairs carry their true distance 0)."""
        n_q, n_c = getattr(self, "_near", (0, 0))
        q_hi = n_q if q_hi is None else q_hi
        out = np.zeros((max(q_hi - q_lo, 0), n_c), np.uint32)
        self._chk(self.L.nemo_fetch_label_distances(self.h, q_lo, q_hi, _p(out), out.size))
        return out

    def knockout_leaves(self, iters: Sequence[int], cond: int = 1, masks: bool = False) -> np.ndarray:
        """nemo_knockout_leaves: one hypothesis per sink goal (a goal without children) of every listed run's
        pre (cond 0) or post (cond 1) graph, knocked out alone.  Returns the rows as a structured array
        (KNOCK_DTYPE: graph, node, n_dead, roots_dead, n_roots), graphs in list order, a graph's sink goals in
        node-index order; knockout_ranges() locates each listed graph's rows.  masks: keep the dead masks for
        knockout_mask()."""
        it = np.ascontiguousarray(iters, dtype=np.uint32)
        self._ko_ranges = 0
        self._chk(self.L.nemo_knockout_leaves(self.h, _p(it), len(it), int(cond), KO_MASKS if masks else 0))
        self._ko_ranges = len(it)
        return self.knockout_rows()

    def knockout_sets(self, iteration: int, cond: int, sets: Sequence[Sequence[int]], masks: bool = False) -> np.ndarray:
        """nemo_knockout_sets: explicit hypotheses on one graph, each a set of local node indices removed by
        assumption (the empty set is legal).  Returns one KNOCK_DTYPE row per set (node = UINT32_MAX)."""
        off = np.zeros(len(sets) + 1, np.uint64)
        off[1:] = np.cumsum([len(x) for x in sets], dtype=np.uint64)
        nodes = np.ascontiguousarray([v for x in sets for v in x], dtype=np.uint32)
        return self.knockout_sets_raw(iteration, cond, off, nodes, len(sets), masks)

    def knockout_sets_raw(self, iteration: int, cond: int, set_off: np.ndarray, set_nodes: np.ndarray, n_sets: int,
                          masks: bool = False) -> np.ndarray:
        """nemo_knockout_sets with the caller's own offsets (u64 [n_sets + 1]) and node array (u32)."""
        off = np.ascontiguousarray(set_off, dtype=np.uint64)
        nodes = np.ascontiguousarray(set_nodes, dtype=np.uint32)
        self._ko_ranges = 0
        self._chk(self.L.nemo_knockout_sets(self.h, int(iteration), int(cond), off.ctypes.data, _p(nodes), int(n_sets),
                                            KO_MASKS if masks else 0))
        self._ko_ranges = 1 if n_sets else 0
        return self.knockout_rows()

    def knockout_rows(self) -> np.ndarray:
        """nemo_fetch_knockout: the rows of the last knock-out call."""
        n = ctypes.c_uint64()
        self._chk(self.L.nemo_fetch_knockout(self.h, None, 0, ctypes.byref(n)))
        out = np.zeros(n.value, KNOCK_DTYPE)
        self._chk(self.L.nemo_fetch_knockout(self.h, _p(out), len(out), ctypes.byref(n)))
        return out

    def knockout_ranges(self):
        """nemo_fetch_knockout_ranges: (first hypothesis u64, count u32) per listed graph of the last leaves
        call, or of the one graph of the last sets call."""
        n = getattr(self, "_ko_ranges", 0)
        first, count = np.zeros(n, np.uint64), np.zeros(n, np.uint32)
        self._chk(self.L.nemo_fetch_knockout_ranges(self.h, _p(first), _p(count), n))
        return first, count

    def knockout_mask(self, hyp: int, n_nodes: int) -> np.ndarray:
        """nemo_fetch_knockout_mask: one byte per node of hypothesis `hyp`'s graph (n_nodes of them), 1 = dead;
        needs a call with masks=True."""
        out = np.zeros(n_nodes, np.uint8)
        self._chk(self.L.nemo_fetch_knockout_mask(self.h, int(hyp), _p(out), len(out)))
        return out

    def min_cuts(self, iteration: int, cond: int, candidates: Optional[Sequence[int]] = None, max_size: int = 2) -> np.ndarray:
        """nemo_min_cuts: all minimal cuts of size <= max_size (1..3) of a run's pre (cond 0) or post (cond 1) graph
        among `candidates` (graph-local node indices of any kind; None: every sink goal in node-index order).
        Returns the rows as a structured array (CUT_DTYPE: size, node[3] in candidate-list order, unused entries
        UINT32_MAX), sorted by (size, colex rank of the live positions); min_cut_stats() has the rounds' counts."""
        if candidates is None:
            self._chk(self.L.nemo_min_cuts(self.h, int(iteration), int(cond), None, 0, int(max_size), 0))
        else:
            cand = np.ascontiguousarray(candidates, dtype=np.uint32)
            keep = cand if len(cand) else np.zeros(1, np.uint32)  # an empty list is a list: never NULL
            self._chk(self.L.nemo_min_cuts(self.h, int(iteration), int(cond), _p(keep), len(cand), int(max_size), 0))
        return self.min_cut_rows()

    def min_cut_rows(self) -> np.ndarray:
        """nemo_fetch_min_cuts: the rows of the last min_cuts call."""
        n = ctypes.c_uint64()
        self._chk(self.L.nemo_fetch_min_cuts(self.h, None, 0, ctypes.byref(n)))
        out = np.zeros(n.value, CUT_DTYPE)
        self._chk(self.L.nemo_fetch_min_cuts(self.h, _p(out), len(out), ctypes.byref(n)))
        return out

    def min_cut_stats(self) -> np.ndarray:
        """nemo_fetch_min_cut_stats: a 3 x 3 u64 array, row s - 1 = (live candidates entering round s, hypotheses
        evaluated, minimal cuts found)."""
        out = np.zeros(9, np.uint64)
        self._chk(self.L.nemo_fetch_min_cut_stats(self.h, _p(out)))
        return out.reshape(3, 3)

    def min_repairs(self, base: int, other: int, max_size: int = 2) -> np.ndarray:
        """nemo_min_repairs: all minimal repairs of size <= max_size (1..3) of run `base`'s post graph, where the absent
        set and the candidates are its sink goals whose label is no goal label of run `other`'s post graph (made on the
        device; min_repair_stats() returns the list).  Returns the rows as an (n, 4) u32 array: size, then the nodes in
        candidate-list order, unused entries UINT32_MAX, sorted by (size, colex rank of the live positions)."""
        self._chk(self.L.nemo_min_repairs(self.h, int(base), int(other), int(max_size), 0))
        return self.min_repair_rows()

    def min_repair_sets(self, iteration: int, cond: int, absent: Sequence[int], candidates: Optional[Sequence[int]] = None,
                        max_size: int = 2) -> np.ndarray:
        """nemo_min_repair_sets: the same over an absent set and candidates the caller names (graph-local node indices
        of any kind; candidates None: the absent list, in its order).  A repair is a set S of candidates such that
        the outcome is not lost under absent \\ S."""
        ab = np.ascontiguousarray(absent, dtype=np.uint32)
        keep_a = ab if len(ab) else np.zeros(1, np.uint32)  # an empty list is a list: never NULL
        if candidates is None:
            self._chk(self.L.nemo_min_repair_sets(self.h, int(iteration), int(cond), _p(keep_a), len(ab), None, 0, int(max_size), 0))
        else:
            cand = np.ascontiguousarray(candidates, dtype=np.uint32)
            keep_c = cand if len(cand) else np.zeros(1, np.uint32)
            self._chk(self.L.nemo_min_repair_sets(self.h, int(iteration), int(cond), _p(keep_a), len(ab), _p(keep_c), len(cand),
                                                  int(max_size), 0))
        return self.min_repair_rows()

    def min_repair_rows(self) -> np.ndarray:
        """nemo_fetch_min_repairs: the rows of the last min_repairs / min_repair_sets call, (n, 4) u32."""
        n = ctypes.c_uint64()
        self._chk(self.L.nemo_fetch_min_repairs(self.h, None, 0, ctypes.byref(n)))
        out = np.zeros((n.value, 4), np.uint32)
        self._chk(self.L.nemo_fetch_min_repairs(self.h, _p(out), len(out), ctypes.byref(n)))
        return out

    def min_repair_stats(self):
        """nemo_fetch_min_repair_stats and nemo_fetch_min_repair_cands: (status, |A|, a 3 x 3 u64 array whose row s - 1 is
        (live candidates entering round s, hypotheses evaluated, minimal repairs found), the candidate list the call
        used as a u32 array).  status is REPAIR_HOLDS, REPAIR_SEARCHED or REPAIR_BEYOND."""
        st = np.zeros(11, np.uint64)
        self._chk(self.L.nemo_fetch_min_repair_stats(self.h, _p(st)))
        n = ctypes.c_uint64()
        self._chk(self.L.nemo_fetch_min_repair_cands(self.h, None, 0, ctypes.byref(n)))
        cand = np.zeros(n.value, np.uint32)
        self._chk(self.L.nemo_fetch_min_repair_cands(self.h, _p(cand), len(cand), ctypes.byref(n)))
        return int(st[0]), int(st[1]), st[2:].reshape(3, 3), cand

    def lineage_repairs(self, base: int, other: int, max_size: int = 3) -> np.ndarray:
        """nemo_lineage_repairs: all minimal repairs of size <= max_size (1..8) of run `base`'s post graph, where the
        absent set and the candidates are its sink goals whose label is no goal label of run `other`'s post graph (as
        min_repairs makes them; at most 65535), found by the lineage repair search: a restore set that does not bring
        the outcome back is extended only by candidates that lie in its blocker.  Returns the rows as a structured array
        (LINEAGE_REPAIR_DTYPE: size, node[8] ascending by candidate position, unused entries UINT32_MAX), sorted by
        (size, colex order of the candidate positions); lineage_repair_stats() has the status and the levels' counts."""
        self._chk(self.L.nemo_lineage_repairs(self.h, int(base), int(other), int(max_size), 0))
        return self.lineage_repair_rows()

    def lineage_repair_sets(self, iteration: int, cond: int, absent: Sequence[int], candidates: Optional[Sequence[int]] = None,
                            max_size: int = 3) -> np.ndarray:
        """nemo_lineage_repair_sets: the same over an absent set and candidates the caller names (as min_repair_sets
        takes them; candidates None: the absent list, in its order)."""
        ab = np.ascontiguousarray(absent, dtype=np.uint32)
        keep_a = ab if len(ab) else np.zeros(1, np.uint32)  # an empty list is a list: never NULL
        if candidates is None:
            self._chk(self.L.nemo_lineage_repair_sets(self.h, int(iteration), int(cond), _p(keep_a), len(ab), None, 0, int(max_size), 0))
        else:
            cand = np.ascontiguousarray(candidates, dtype=np.uint32)
            keep_c = cand if len(cand) else np.zeros(1, np.uint32)
            self._chk(self.L.nemo_lineage_repair_sets(self.h, int(iteration), int(cond), _p(keep_a), len(ab), _p(keep_c), len(cand),
                                                      int(max_size), 0))
        return self.lineage_repair_rows()

    def lineage_repair_rows(self) -> np.ndarray:
        """nemo_fetch_lineage_repairs: the rows of the last lineage_repairs / lineage_repair_sets call."""
        n = ctypes.c_uint64()
        self._chk(self.L.nemo_fetch_lineage_repairs(self.h, None, 0, ctypes.byref(n)))
        out = np.zeros(n.value, LINEAGE_REPAIR_DTYPE)
        self._chk(self.L.nemo_fetch_lineage_repairs(self.h, _p(out), len(out), ctypes.byref(n)))
        return out

    def lineage_repair_stats(self):
        """nemo_fetch_lineage_repair_stats: (status, |A|, a 9 x 2 u64 array, row d = (sets evaluated at size d, minimal
        repairs found of size d), d = 0..8).  status is REPAIR_HOLDS, REPAIR_SEARCHED or REPAIR_BEYOND."""
        st = np.zeros(20, np.uint64)
        self._chk(self.L.nemo_fetch_lineage_repair_stats(self.h, _p(st)))
        return int(st[0]), int(st[1]), st[2:].reshape(9, 2)

    def lineage_repair_cands(self) -> np.ndarray:
        """nemo_fetch_lineage_repair_cands: the candidate list the last call used (position -> node), a u32 array."""
        n = ctypes.c_uint64()
        self._chk(self.L.nemo_fetch_lineage_repair_cands(self.h, None, 0, ctypes.byref(n)))
        cand = np.zeros(n.value, np.uint32)
        self._chk(self.L.nemo_fetch_lineage_repair_cands(self.h, _p(cand), len(cand), ctypes.byref(n)))
        return cand

    def lineage_cuts(self, iteration: int, cond: int, candidates: Optional[Sequence[int]] = None, max_size: int = 3) -> np.ndarray:
        """nemo_lineage_cuts: all minimal cuts of size <= max_size (1..8) of a run's pre (cond 0) or post (cond 1) graph
        among `candidates` (as min_cuts takes them; at most 65535), found by the lineage-driven search: a fault set
        that is no cut is extended only by candidates that lie in the derivation it leaves.  Returns the rows as a
        structured array (LINEAGE_CUT_DTYPE: size, node[8] ascending by candidate position, unused entries UINT32_MAX),
        sorted by (size, colex order of the candidate positions); lineage_cut_stats() has the levels' counts."""
        if candidates is None:
            self._chk(self.L.nemo_lineage_cuts(self.h, int(iteration), int(cond), None, 0, int(max_size), 0))
        else:
            cand = np.ascontiguousarray(candidates, dtype=np.uint32)
            keep = cand if len(cand) else np.zeros(1, np.uint32)  # an empty list is a list: never NULL
            self._chk(self.L.nemo_lineage_cuts(self.h, int(iteration), int(cond), _p(keep), len(cand), int(max_size), 0))
        return self.lineage_cut_rows()

    def lineage_cut_rows(self) -> np.ndarray:
        """nemo_fetch_lineage_cuts: the rows of the last lineage_cuts call."""
        n = ctypes.c_uint64()
        self._chk(self.L.nemo_fetch_lineage_cuts(self.h, None, 0, ctypes.byref(n)))
        out = np.zeros(n.value, LINEAGE_CUT_DTYPE)
        self._chk(self.L.nemo_fetch_lineage_cuts(self.h, _p(out), len(out), ctypes.byref(n)))
        return out

    def lineage_cut_stats(self) -> np.ndarray:
        """nemo_fetch_lineage_cut_stats: a 9 x 2 u64 array, row d = (sets evaluated at size d, minimal cuts found of
        size d), d = 0..8."""
        out = np.zeros(18, np.uint64)
        self._chk(self.L.nemo_fetch_lineage_cut_stats(self.h, _p(out)))
        return out.reshape(9, 2)

    def knockout_labels(self, iters: Sequence[int], cond: int, sets, sinks_only: bool = False):
        """nemo_knockout_labels: hypotheses that name interned labels, tested on every listed run's pre (cond 0) or
        post (cond 1) graph in one call.  sets: a list of label lists, or a pair (set_off u64 [n_sets + 1],
        set_labels u32).  A set removes every node of a graph whose label it names (sinks_only: every sink goal).
        Returns (lost, hit), uint64 arrays of shape (n, n_chunks), n_chunks = ceil(n_sets / 64): bit s & 63 of
        word [i, s // 64] is set s on list position i; knockout_label_counts() has the per-set counts."""
        if isinstance(sets, tuple) and len(sets) == 2 and isinstance(sets[0], np.ndarray):
            off = np.ascontiguousarray(sets[0], dtype=np.uint64)
            labels = np.ascontiguousarray(sets[1], dtype=np.uint32)
            n_sets = max(len(off) - 1, 0)
        else:
            n_sets = len(sets)
            off = np.zeros(n_sets + 1, np.uint64)
            off[1:] = np.cumsum([len(x) for x in sets], dtype=np.uint64)
            labels = np.ascontiguousarray([v for x in sets for v in x], dtype=np.uint32)
        it = np.ascontiguousarray(iters, dtype=np.uint32)
        self._kl_shape = (0, 0, 0)
        self._chk(self.L.nemo_knockout_labels(self.h, _p(it), len(it), int(cond), off.ctypes.data, _p(labels), n_sets,
                                              KL_SINKS if sinks_only else 0))
        n_chunks = (n_sets + 63) // 64
        self._kl_shape = (len(it), n_chunks, n_sets)
        lost, hit = np.zeros((len(it), n_chunks), np.uint64), np.zeros((len(it), n_chunks), np.uint64)
        self._chk(self.L.nemo_fetch_knockout_labels(self.h, _p(lost), _p(hit), lost.size))
        return lost, hit

    def knockout_label_counts(self):
        """nemo_fetch_knockout_label_counts: (n_lost, n_hit) of the last knockout_labels call, per set the list
        positions on which it is lost / hits a node (a run listed twice counts twice)."""
        n_sets = getattr(self, "_kl_shape", (0, 0, 0))[2]
        n_lost, n_hit = np.zeros(n_sets, np.uint32), np.zeros(n_sets, np.uint32)
        self._chk(self.L.nemo_fetch_knockout_label_counts(self.h, _p(n_lost), _p(n_hit), n_sets))
        return n_lost, n_hit

    def min_label_cuts(self, iters: Sequence[int], cond: int, cand_labels: Sequence[int], max_size: int = 2, min_runs: int = 0,
                       sinks_only: bool = False):
        """nemo_min_label_cuts: all minimal sets of <= max_size (1..3) of the candidate labels whose loss defeats the
        outcome on at least min_runs of the listed runs' pre (cond 0) or post (cond 1) graphs (0: on every list
        position).  A set removes every node of a graph whose label it names (sinks_only: every sink goal).
        Returns (rows, n_lost): rows a structured array (LABEL_CUT_DTYPE: size, label[3] in candidate-list order,
        unused entries UINT32_MAX) sorted by (size, colex rank of the live positions), n_lost[k] the list positions
        on which row k is lost; min_label_cut_stats() has the rounds' counts."""
        it = np.ascontiguousarray(iters, dtype=np.uint32)
        cand = np.ascontiguousarray(cand_labels, dtype=np.uint32)
        keep = cand if len(cand) else np.zeros(1, np.uint32)  # an empty list is a list: never NULL
        self._chk(self.L.nemo_min_label_cuts(self.h, _p(it), len(it), int(cond), _p(keep), len(cand), int(max_size), int(min_runs),
                                             KL_SINKS if sinks_only else 0))
        return self.min_label_cut_rows()

    def min_label_cut_rows(self):
        """nemo_fetch_min_label_cuts: (rows, n_lost) of the last min_label_cuts call."""
        n = ctypes.c_uint64()
        self._chk(self.L.nemo_fetch_min_label_cuts(self.h, None, None, 0, ctypes.byref(n)))
        out, n_lost = np.zeros(n.value, LABEL_CUT_DTYPE), np.zeros(n.value, np.uint32)
        self._chk(self.L.nemo_fetch_min_label_cuts(self.h, _p(out), _p(n_lost), len(out), ctypes.byref(n)))
        return out, n_lost

    def min_label_cut_stats(self) -> np.ndarray:
        """nemo_fetch_min_label_cut_stats: a 3 x 3 u64 array, row s - 1 = (live candidates entering round s,
        hypotheses evaluated, minimal cuts found)."""
        out = np.zeros(9, np.uint64)
        self._chk(self.L.nemo_fetch_min_label_cut_stats(self.h, _p(out)))
        return out.reshape(3, 3)

    def min_group_cuts(self, iters: Sequence[int], cond: int, groups, max_size: int = 2, min_runs: int = 0,
                       sinks_only: bool = False):
        """nemo_min_group_cuts: min_label_cuts with groups of labels as candidates (a fault event that removes many
        labels at once, nemo_amd.faults.fault_events): all minimal sets of <= max_size (1..3) candidates whose loss
        together defeats the outcome on at least min_runs of the listed runs' pre (cond 0) or post (cond 1) graphs
        (0: on every list position).  groups: a list of label lists, or a pair (group_off u64 [n_groups + 1],
        group_labels u32), as knockout_labels takes its sets.  A set removes every node of a graph whose label one
        of its groups names (sinks_only: every sink goal).  Returns (rows, n_lost): rows a structured array
        (GROUP_CUT_DTYPE: size, group[3] the candidate positions, ascending, unused entries UINT32_MAX) sorted by
        (size, colex rank of the live positions), n_lost[k] the list positions on which row k is lost;
        min_group_cut_stats() has the rounds' counts."""
        if isinstance(groups, tuple) and len(groups) == 2 and isinstance(groups[0], np.ndarray):
            off = np.ascontiguousarray(groups[0], dtype=np.uint64)
            labels = np.ascontiguousarray(groups[1], dtype=np.uint32)
            n_groups = max(len(off) - 1, 0)
        else:
            n_groups = len(groups)
            off = np.zeros(n_groups + 1, np.uint64)
            off[1:] = np.cumsum([len(x) for x in groups], dtype=np.uint64)
            labels = np.ascontiguousarray([v for x in groups for v in x], dtype=np.uint32)
        it = np.ascontiguousarray(iters, dtype=np.uint32)
        keep = labels if len(labels) else np.zeros(1, np.uint32)  # an empty list is a list: never NULL
        self._chk(self.L.nemo_min_group_cuts(self.h, _p(it), len(it), int(cond), off.ctypes.data, _p(keep), n_groups, int(max_size),
                                             int(min_runs), KL_SINKS if sinks_only else 0))
        return self.min_group_cut_rows()

    def min_group_cut_rows(self):
        """nemo_fetch_min_group_cuts: (rows, n_lost) of the last min_group_cuts call."""
        n = ctypes.c_uint64()
        self._chk(self.L.nemo_fetch_min_group_cuts(self.h, None, None, 0, ctypes.byref(n)))
        out, n_lost = np.zeros(n.value, GROUP_CUT_DTYPE), np.zeros(n.value, np.uint32)
        self._chk(self.L.nemo_fetch_min_group_cuts(self.h, _p(out), _p(n_lost), len(out), ctypes.byref(n)))
        return out, n_lost

    def min_group_cut_stats(self) -> np.ndarray:
        """nemo_fetch_min_group_cut_stats: a 3 x 3 u64 array, row s - 1 = (live candidates entering round s,
        hypotheses evaluated, minimal cuts found)."""
        out = np.zeros(9, np.uint64)
        self._chk(self.L.nemo_fetch_min_group_cut_stats(self.h, _p(out)))
        return out.reshape(3, 3)

    def lineage_group_cuts(self, iters: Sequence[int], cond: int, groups, max_size: int = 3, min_runs: int = 0,
                           sinks_only: bool = False):
        """nemo_lineage_group_cuts: min_group_cuts' question for sets of up to eight fault events, answered by the
        lineage-driven search: all minimal sets of <= max_size (1..8) candidates whose loss together defeats the
        outcome on at least min_runs of the listed runs' pre (cond 0) or post (cond 1) graphs (0: on every list
        position); a set that is no cut is extended only by events that some surviving derivation rests on.  groups:
        as min_group_cuts takes them (at most 65535).  Returns (rows, n_lost): rows a structured array
        (LINEAGE_GROUP_CUT_DTYPE: size, group[8] the candidate positions, ascending, unused entries UINT32_MAX) sorted
        by (size, colex order of the candidate positions), n_lost[k] the list positions on which row k is lost;
        lineage_group_cut_stats() has the levels' counts."""
        if isinstance(groups, tuple) and len(groups) == 2 and isinstance(groups[0], np.ndarray):
            off = np.ascontiguousarray(groups[0], dtype=np.uint64)
            labels = np.ascontiguousarray(groups[1], dtype=np.uint32)
            n_groups = max(len(off) - 1, 0)
        else:
            n_groups = len(groups)
            off = np.zeros(n_groups + 1, np.uint64)
            off[1:] = np.cumsum([len(x) for x in groups], dtype=np.uint64)
            labels = np.ascontiguousarray([v for x in groups for v in x], dtype=np.uint32)
        it = np.ascontiguousarray(iters, dtype=np.uint32)
        keep = labels if len(labels) else np.zeros(1, np.uint32)  # an empty list is a list: never NULL
        self._chk(self.L.nemo_lineage_group_cuts(self.h, _p(it), len(it), int(cond), off.ctypes.data, _p(keep), n_groups,
                                                 int(max_size), int(min_runs), KL_SINKS if sinks_only else 0))
        return self.lineage_group_cut_rows()

    def lineage_group_cut_rows(self):
        """nemo_fetch_lineage_group_cuts: (rows, n_lost) of the last lineage_group_cuts call."""
        n = ctypes.c_uint64()
        self._chk(self.L.nemo_fetch_lineage_group_cuts(self.h, None, None, 0, ctypes.byref(n)))
        out, n_lost = np.zeros(n.value, LINEAGE_GROUP_CUT_DTYPE), np.zeros(n.value, np.uint32)
        self._chk(self.L.nemo_fetch_lineage_group_cuts(self.h, _p(out), _p(n_lost), len(out), ctypes.byref(n)))
        return out, n_lost

    def lineage_group_cut_stats(self) -> np.ndarray:
        """nemo_fetch_lineage_group_cut_stats: a 9 x 2 u64 array, row d = (sets evaluated at size d, minimal cuts found
        of size d), d = 0..8."""
        out = np.zeros(18, np.uint64)
        self._chk(self.L.nemo_fetch_lineage_group_cut_stats(self.h, _p(out)))
        return out.reshape(9, 2)

    def witness_sets(self, iteration: int, cond: int, sets: Sequence[Sequence[int]], all: bool = False, masks: bool = False) -> np.ndarray:
        """nemo_witness_sets: the surviving derivation of one graph under explicit hypotheses, each a set of local
        node indices removed by assumption (the empty set is legal).  Returns one WITNESS_DTYPE row per set (graph,
        n_roots, roots_alive, n_nodes = |W|, n_sinks = the base events W rests on).  all: every surviving derivation
        (NEMO_WIT_ALL), not the one that takes each goal's smallest alive child; masks: keep W for witness_mask()."""
        off = np.zeros(len(sets) + 1, np.uint64)
        off[1:] = np.cumsum([len(x) for x in sets], dtype=np.uint64)
        nodes = np.ascontiguousarray([v for x in sets for v in x], dtype=np.uint32)
        self._chk(self.L.nemo_witness_sets(self.h, int(iteration), int(cond), off.ctypes.data, _p(nodes), len(sets),
                                           (WIT_ALL if all else 0) | (WIT_MASKS if masks else 0)))
        return self.witness_rows()

    def witness_labels(self, iters: Sequence[int], cond: int, sets, all: bool = False, masks: bool = False,
                       sinks_only: bool = False) -> np.ndarray:
        """nemo_witness_labels: the surviving derivations of every listed run's pre (cond 0) or post (cond 1) graph
        under hypotheses that name interned labels (sets: as knockout_labels takes them; sinks_only: only sink goals
        match a label).  Returns the WITNESS_DTYPE rows, row i * n_sets + s = set s on list position i."""
        if isinstance(sets, tuple) and len(sets) == 2 and isinstance(sets[0], np.ndarray):
            off = np.ascontiguousarray(sets[0], dtype=np.uint64)
            labels = np.ascontiguousarray(sets[1], dtype=np.uint32)
            n_sets = max(len(off) - 1, 0)
        else:
            n_sets = len(sets)
            off = np.zeros(n_sets + 1, np.uint64)
            off[1:] = np.cumsum([len(x) for x in sets], dtype=np.uint64)
            labels = np.ascontiguousarray([v for x in sets for v in x], dtype=np.uint32)
        it = np.ascontiguousarray(iters, dtype=np.uint32)
        self._chk(self.L.nemo_witness_labels(self.h, _p(it), len(it), int(cond), off.ctypes.data, _p(labels), n_sets,
                                             (WIT_ALL if all else 0) | (WIT_MASKS if masks else 0) | (WIT_SINKS if sinks_only else 0)))
        return self.witness_rows()

    def witness_rows(self) -> np.ndarray:
        """nemo_fetch_witness: the rows of the last witness call."""
        n = ctypes.c_uint64()
        self._chk(self.L.nemo_fetch_witness(self.h, None, 0, ctypes.byref(n)))
        out = np.zeros(n.value, WITNESS_DTYPE)
        self._chk(self.L.nemo_fetch_witness(self.h, _p(out), len(out), ctypes.byref(n)))
        return out

    def witness_mask(self, hyp: int, n_nodes: int) -> np.ndarray:
        """nemo_fetch_witness_mask: one byte per node of hypothesis `hyp`'s graph (n_nodes of them), 1 = in W;
        needs a call with masks=True."""
        out = np.zeros(n_nodes, np.uint8)
        self._chk(self.L.nemo_fetch_witness_mask(self.h, int(hyp), _p(out), len(out)))
        return out

    def goal_labels(self, iteration: int, cond: int, d_out_ptr: int, cap: int) -> None:
        """nemo_goal_labels: [n, label...] of a run's goal labels into device memory."""
        self._chk(self.L.nemo_goal_labels(self.h, iteration, cond, ctypes.c_void_p(d_out_ptr), cap))

    def diffprov_labels(self, failed: Sequence[int], d_labels_ptr: int, cap: int) -> None:
        """nemo_diffprov_labels: reference-mode diff with a (broadcast) device label set."""
        f = np.ascontiguousarray(failed, dtype=np.uint32)
        self._chk(self.L.nemo_diffprov_labels(self.h, _p(f), len(f), ctypes.c_void_p(d_labels_ptr), cap))

    def diffprov_host_labels(self, failed: Sequence[int], labels: Sequence[int]) -> None:
        """nemo_diffprov_host_labels: reference-mode diff with a host label set."""
        f = np.ascontiguousarray(failed, dtype=np.uint32)
        lab = np.ascontiguousarray(labels, dtype=np.uint32)
        self._chk(self.L.nemo_diffprov_host_labels(self.h, _p(f), len(f), _p(lab), len(lab)))

    def triggers(self) -> None:
        self._chk(self.L.nemo_triggers(self.h))

    def pull(self, which: int) -> None:
        self._chk(self.L.nemo_pull_edges(self.h, which))

    def synchronize(self) -> None:
        self._chk(self.L.nemo_synchronize(self.h))

    # ---- fetches ------------------------------------------------------------------
    def flags(self, g_lo: int = 0, g_hi: Optional[int] = None) -> np.ndarray:
        c = self.corpus
        g_hi = c.n_graphs if g_hi is None else g_hi
        n = int(c.node_off[g_hi] - c.node_off[g_lo])
        out = np.zeros(max(n, 1), np.uint8)
        self._chk(self.L.nemo_fetch_node_flags(self.h, g_lo, g_hi, _p(out), n))
        return out[:n]

    def stage_simplified(self) -> None:
        """nemo_stage_simplified: async D2H of flags + chain (head, tail) pairs."""
        self._chk(self.L.nemo_stage_simplified(self.h))

    def simplified_view(self):
        """Zero-copy views of the staged results: (state[ceil(V/4)] u8 with 2 bits
        per node (NEMO_STATE_ALIVE | NEMO_STATE_HOLDS << 1), chain_off[G+1] u64,
        chain_ht[n, 2] u16 (or u32 when a graph has >= 65536 nodes)), valid until
        the next stage_simplified()."""
        vp = ctypes.c_void_p
        f, o, h, n, w = vp(), vp(), vp(), ctypes.c_uint64(), ctypes.c_int32()
        self._chk(self.L.nemo_simplified_view(self.h, ctypes.byref(f), ctypes.byref(o), ctypes.byref(h),
                                              ctypes.byref(n), ctypes.byref(w)))
        c = self.corpus
        V, G = int(c.node_off[-1]), c.n_graphs

        def view(ptr, ctype, count, dtype):
            if count == 0 or not ptr.value:
                return np.zeros(0, dtype)
            return np.ctypeslib.as_array(ctypes.cast(ptr, ctypes.POINTER(ctype)), shape=(count,))

        state = view(f, ctypes.c_uint8, (V + 3) // 4, np.uint8)
        off = view(o, ctypes.c_uint64, G + 1, np.uint64)
        if w.value:
            ht = view(h, ctypes.c_uint32, 2 * n.value, np.uint32).reshape(-1, 2)
        else:
            ht = view(h, ctypes.c_uint16, 2 * n.value, np.uint16).reshape(-1, 2)
        return state, off, ht

    @staticmethod
    def unpack_state(state: np.ndarray, V: int):
        """(alive, holds) bool arrays of length V from the 2-bit staged node state."""
        bits = np.unpackbits(state, bitorder="little")[:2 * V].reshape(V, 2)
        return bits[:, 0].astype(bool), bits[:, 1].astype(bool)

    def chains(self) -> np.ndarray:
        n = ctypes.c_uint64()
        self._chk(self.L.nemo_fetch_chains(self.h, None, 0, ctypes.byref(n)))
        buf = (CChain * max(n.value, 1))()
        self._chk(self.L.nemo_fetch_chains(self.h, buf, n.value, ctypes.byref(n)))
        arr = np.frombuffer(buf, dtype=np.uint32).reshape(-1, 5)
        return arr[:n.value].copy()

    def run_tables(self, which: int) -> np.ndarray:
        c = self.corpus
        W = (c.n_tables + 31) // 32
        out = np.zeros(c.n_runs * W + 1, np.uint32)
        self._chk(self.L.nemo_fetch_run_tables(self.h, which, _p(out), c.n_runs * W))
        return out[:c.n_runs * W].reshape(c.n_runs, W)

    def diff_mask(self, entry: int) -> np.ndarray:
        c = self.corpus
        r0 = c.run_index(0)
        V0 = c.graph_size(2 * r0 + 1)
        out = np.zeros(max(V0, 1), np.uint8)
        self._chk(self.L.nemo_fetch_diff_mask(self.h, entry, _p(out), V0))
        return out[:V0]

    def diff_masks(self, n_entries: int) -> np.ndarray:
        c = self.corpus
        V0 = c.graph_size(2 * c.run_index(0) + 1)
        out = np.zeros(max(n_entries * V0, 1), np.uint8)
        self._chk(self.L.nemo_fetch_diff_masks(self.h, _p(out), n_entries * V0))
        return out[:n_entries * V0].reshape(n_entries, V0)

    def diff_masks_view(self) -> np.ndarray:
        """Zero-copy (n_entries, V0) view of the D masks in library-owned pinned memory
        (valid until the next diffprov)."""
        p, ne, v0 = ctypes.c_void_p(), ctypes.c_uint64(), ctypes.c_uint64()
        self._chk(self.L.nemo_diff_masks_view(self.h, ctypes.byref(p), ctypes.byref(ne), ctypes.byref(v0)))
        n = ne.value * v0.value
        if n == 0 or not p.value:
            return np.zeros((ne.value, v0.value), np.uint8)
        buf = (ctypes.c_uint8 * n).from_address(p.value)
        return np.frombuffer(buf, np.uint8).reshape(ne.value, v0.value)

    def missing(self) -> np.ndarray:
        n = ctypes.c_uint64()
        self._chk(self.L.nemo_fetch_missing(self.h, None, 0, ctypes.byref(n)))
        buf = (CMissing * max(n.value, 1))()
        self._chk(self.L.nemo_fetch_missing(self.h, buf, n.value, ctypes.byref(n)))
        return np.frombuffer(buf, dtype=np.uint32).reshape(-1, 2)[:n.value].copy()

    def diff_classes(self):
        """nemo_diff_classes + nemo_fetch_diff_classes: the entries of the last diffprov grouped by
        identical D mask.  Returns (class_of[n_entries], classes[n_classes, 3]) as uint32 arrays;
        a classes row is (representative entry, member entries, |D|), classes are numbered by
        their smallest entry."""
        self._chk(self.L.nemo_diff_classes(self.h))
        n = ctypes.c_uint64()
        self._chk(self.L.nemo_fetch_diff_classes(self.h, None, None, 0, ctypes.byref(n)))
        classes = np.zeros((max(n.value, 1), 3), np.uint32)
        self._chk(self.L.nemo_fetch_diff_classes(self.h, None, classes.ctypes.data, n.value, ctypes.byref(n)))
        classes = classes[:n.value]
        class_of = np.zeros(max(int(classes[:, 1].sum()), 1), np.uint32)  # the sizes add up to the entries
        self._chk(self.L.nemo_fetch_diff_classes(self.h, class_of.ctypes.data, None, 0, ctypes.byref(n)))
        return class_of[:int(classes[:, 1].sum())], classes

    def diff_support(self) -> np.ndarray:
        """nemo_fetch_diff_support (after diff_classes): per node of run 0's post graph, the entries
        whose D holds it."""
        c = self.corpus
        has0 = 0 in set(int(x) for x in c.iteration)
        V0 = c.graph_size(2 * c.run_index(0) + 1) if has0 else 0
        out = np.zeros(max(V0, 1), np.uint32)
        self._chk(self.L.nemo_fetch_diff_support(self.h, out.ctypes.data, V0))
        return out[:V0]

    def sdiff_masks(self) -> List[np.ndarray]:
        """S mask of every symmetric-diff entry: one uint8 array per entry, over the nodes of the
        entry's own failed post graph."""
        n = ctypes.c_uint64()
        ne = self._n_sym
        off = np.zeros(ne + 1, np.uint64)
        self._chk(self.L.nemo_fetch_sdiff_masks(self.h, off.ctypes.data, None, 0, ctypes.byref(n)))
        out = np.zeros(max(n.value, 1), np.uint8)
        self._chk(self.L.nemo_fetch_sdiff_masks(self.h, None, _p(out), n.value, ctypes.byref(n)))
        return [out[int(off[e]):int(off[e + 1])].copy() for e in range(ne)]

    def surplus(self) -> np.ndarray:
        """Surplus events of the symmetric diff as rows (entry, rule local to the entry's failed post graph)."""
        n = ctypes.c_uint64()
        self._chk(self.L.nemo_fetch_surplus(self.h, None, 0, ctypes.byref(n)))
        buf = (CMissing * max(n.value, 1))()
        self._chk(self.L.nemo_fetch_surplus(self.h, buf, n.value, ctypes.byref(n)))
        return np.frombuffer(buf, dtype=np.uint32).reshape(-1, 2)[:n.value].copy()

    def trigger_rows(self):
        npre, npost, nasync = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
        self._chk(self.L.nemo_fetch_triggers(self.h, None, 0, ctypes.byref(npre), None, 0, ctypes.byref(npost), None,
                                             0, ctypes.byref(nasync)))
        pre = np.zeros(3 * npre.value + 1, np.uint32)
        post = np.zeros(2 * npost.value + 1, np.uint32)
        asy = np.zeros(nasync.value + 1, np.uint32)
        self._chk(self.L.nemo_fetch_triggers(self.h, _p(pre), npre.value, ctypes.byref(npre), _p(post), npost.value,
                                             ctypes.byref(npost), _p(asy), nasync.value, ctypes.byref(nasync)))
        return (pre[:3 * npre.value].reshape(-1, 3), post[:2 * npost.value].reshape(-1, 2), asy[:nasync.value])

    def pulled(self, slot: int):
        n = ctypes.c_uint64()
        self._chk(self.L.nemo_fetch_pulled(self.h, slot, None, None, 0, ctypes.byref(n)))
        s = np.zeros(n.value + 1, np.uint32)
        d = np.zeros(n.value + 1, np.uint32)
        self._chk(self.L.nemo_fetch_pulled(self.h, slot, _p(s), _p(d), n.value, ctypes.byref(n)))
        return s[:n.value], d[:n.value]

    def pulled_all(self, n_slots: int):
        """(off[n_slots], cnt[n_slots], src, dst) of the last pull in one call (nemo_fetch_pulled_all)."""
        off = np.zeros(max(n_slots, 1), np.uint64)
        cnt = np.zeros(max(n_slots, 1), np.uint32)
        n = ctypes.c_uint64()
        self._chk(self.L.nemo_fetch_pulled_all(self.h, _p(off), _p(cnt), None, None, 0, ctypes.byref(n)))
        src = np.zeros(max(n.value, 1), np.uint32)
        dst = np.zeros(max(n.value, 1), np.uint32)
        self._chk(self.L.nemo_fetch_pulled_all(self.h, None, None, _p(src), _p(dst), n.value, ctypes.byref(n)))
        return off[:n_slots], cnt[:n_slots], src[:n.value], dst[:n.value]

    def debug_copy(self, name: str, offset: int, nbytes: int) -> np.ndarray:
        out = np.zeros(max(nbytes, 1), np.uint8)
        self._chk(self.L.nemo_debug_copy(self.h, name.encode(), _p(out), offset, nbytes))
        return out[:nbytes]

    def timings(self) -> Dict[str, dict]:
        n = ctypes.c_uint32()
        self._chk(self.L.nemo_timings(self.h, None, 0, ctypes.byref(n)))
        buf = (CTiming * max(n.value, 1))()
        self._chk(self.L.nemo_timings(self.h, buf, n.value, ctypes.byref(n)))
        return {buf[i].name.decode(): {"launches": buf[i].launches, "ms": buf[i].ms, "bytes": buf[i].bytes,
                                       "edges": buf[i].edges} for i in range(n.value)}

    def reset_timings(self) -> None:
        self._chk(self.L.nemo_reset_timings(self.h))


def reduce_interpret(vec: np.ndarray, n_tables: int, table_post: int):
    """nemo_reduce_interpret: inter/union/achvdCond from a (reduced) host vector; no device needed."""
    v = np.ascontiguousarray(vec, dtype=np.uint32)
    inter = np.zeros(n_tables + 1, np.uint32)
    uni = np.zeros(n_tables + 1, np.uint32)
    a, ni, nu = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32()
    rc = lib().nemo_reduce_interpret(v.ctypes.data, n_tables, table_post, ctypes.byref(a), inter.ctypes.data,
                                     ctypes.byref(ni), uni.ctypes.data, ctypes.byref(nu))
    if rc != 0:
        raise NemoError(rc, "nemo_reduce_interpret")
    return a.value, inter[:ni.value].tolist(), uni[:nu.value].tolist()


@dataclass
class EngineResult:
    """The engine's results in the oracle's result layout (tests compare the two)."""

    flags: np.ndarray
    chains: np.ndarray
    proto_bits: np.ndarray
    graph_tables: np.ndarray
    achieved: int
    inter: List[int]
    union: List[int]
    diff_mask: np.ndarray
    missing: np.ndarray
    pre_rows: np.ndarray
    post_rows: np.ndarray
    async_rules: np.ndarray
    pulled: Optional[List[tuple]]


def analyze(corpus: Corpus, success: Sequence[int], failed: Sequence[int], diff_mode: int = 0,
            engine: Optional[Engine] = None, pulls: bool = True) -> EngineResult:
    """main.go:106-177's graph calls, in order, on the GPU."""
    eng = engine or Engine(0)
    eng.load(corpus)
    eng.mark()
    eng.simplify()
    achieved, inter, uni = eng.prototypes(success) if len(success) else (0, [], [])
    eng.diffprov(failed, diff_mode)
    eng.triggers()
    pulled = None
    if pulls:
        eng.pull(1)
        off, cnt, src, dst = eng.pulled_all(corpus.n_graphs)
        pulled = [(src[int(a):int(a) + int(n)], dst[int(a):int(a) + int(n)]) for a, n in zip(off, cnt)]
    has0 = 0 in set(int(x) for x in corpus.iteration)
    masks = np.stack([eng.diff_mask(e) for e in range(len(failed))]) if (has0 and len(failed)) else np.zeros((0, 0))
    pre, post, asy = eng.trigger_rows()
    res = EngineResult(flags=eng.flags(), chains=eng.chains(),
                       proto_bits=eng.run_tables(0) if len(success) else None,
                       graph_tables=eng.run_tables(1) if len(success) else None,
                       achieved=achieved, inter=inter, union=uni, diff_mask=masks, missing=eng.missing(),
                       pre_rows=pre, post_rows=post, async_rules=asy, pulled=pulled)
    return res
