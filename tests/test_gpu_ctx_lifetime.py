"""Lifetime of a context's per-corpus state (nemo_amd/csrc/ctx.h CorpusState): one Engine takes a corpus with
run 0 and failed runs, then the same corpus without run 0 and with fewer runs, then a load that fails its
validation, then the first corpus again.  Nothing computed for one corpus may be handed out for another, and
the second pass over the first corpus is identical to the first and to a fresh Engine's.

The expected status of every call after the smaller load and after the failed load is what the library
returned for this sequence before CorpusState existed (recorded from that build, call by call): without run 0
the diff, the symmetric diff and the triggers succeed with zero entries / rows ("MATCH on run 0 finds
nothing", differential-provenance.go:22), and the fetches report those zero counts; after a failed load the
fetches fail with NEMO_ERR_STATE, or report zero entries where they have no state check.  One thing differs
from that build on purpose: after a failed load the size queries (nemo_num_nodes, nemo_num_edges,
nemo_reduce_len, nemo_diff_masks_view's v0) report no corpus, where they used to report the previous corpus's
sizes (a load failing its first checks) or the rejected one's (a later check).
"""
import ctypes
import dataclasses

import numpy as np
import pytest

from nemo_amd import engine as E
from nemo_amd.corpus import DIFF_PER_RUN
from oracle import oracle as O
from tests.compare import _edge_multiset
from tools import synth

pytestmark = pytest.mark.gpu

OK, INVALID, STATE = 0, 1, 5  # NEMO_OK, NEMO_ERR_INVALID, NEMO_ERR_STATE (include/nemohip.h)


def _slots(n_slots, off, cnt, src, dst):
    """The pulled edges as sorted (slot, src, dst) rows: regions land in any order on the device."""
    slot = np.concatenate([np.full(int(cnt[k]), k, np.int64) for k in range(n_slots)] + [np.zeros(0, np.int64)])
    idx = np.concatenate([np.arange(int(off[k]), int(off[k]) + int(cnt[k])) for k in range(n_slots)] +
                         [np.zeros(0, np.int64)]).astype(np.int64)
    return _edge_multiset(slot, src[idx], dst[idx])


def _everything(eng, corpus):
    """Step 1: every analysis on `corpus`, as a dict of arrays in a canonical order."""
    s, f = corpus.success_iters(), corpus.failed_iters()
    G = corpus.n_graphs
    out = {}
    eng.load(corpus)
    eng.mark()
    eng.simplify()
    out["flags"], out["chains"] = eng.flags(), eng.chains()
    out["protos"] = np.array(sum((list(np.atleast_1d(x)) + [-1] for x in eng.prototypes(s)), []), np.int64)
    out["proto_bits"], out["graph_tables"] = eng.run_tables(0), eng.run_tables(1)
    eng.diffprov(f, DIFF_PER_RUN)
    out["dmask"], out["missing"] = eng.diff_masks(len(f)), eng.missing()
    eng.diffprov_symmetric(f)
    out["smask"], out["surplus"] = np.concatenate(eng.sdiff_masks()), eng.surplus()
    for which, n in ((1, G), (2, len(f)), (3, len(f))):
        eng.pull(which)
        out[f"pull{which}"] = _slots(n, *eng.pulled_all(n))
    eng.triggers()
    out["pre"], out["post"], out["async"] = eng.trigger_rows()
    eng.stage_simplified()
    state, off, ht = eng.simplified_view()
    out["state"], out["chain_off"] = state.copy(), off.copy()
    seg = np.repeat(np.arange(G, dtype=np.int64), np.diff(off.astype(np.int64)))
    out["chain_ht"] = _edge_multiset(seg, ht[:, 0], ht[:, 1])
    return out


def _same(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        assert a[k].shape == b[k].shape and np.array_equal(a[k], b[k]), f"{what}: {k} differs"


def _fetches(eng):
    """Status (and counts) of every fetch, through the C ABI: the Engine wrappers index the Python corpus."""
    L, h = eng.L, eng.h
    u64, vp = ctypes.c_uint64, ctypes.c_void_p
    n, a, b, c = u64(), u64(), u64(), u64()
    r = {}
    r["fetch_missing"] = [L.nemo_fetch_missing(h, None, 0, ctypes.byref(n)), n.value]
    n = u64()
    r["fetch_surplus"] = [L.nemo_fetch_surplus(h, None, 0, ctypes.byref(n)), n.value]
    p, ne, v0 = vp(), u64(), u64()
    r["diff_masks_view"] = [L.nemo_diff_masks_view(h, ctypes.byref(p), ctypes.byref(ne), ctypes.byref(v0)),
                            ne.value, v0.value, int(bool(p.value))]
    n = u64()
    r["fetch_sdiff_masks"] = [L.nemo_fetch_sdiff_masks(h, None, None, 0, ctypes.byref(n)), n.value]
    r["fetch_triggers"] = [L.nemo_fetch_triggers(h, None, 0, ctypes.byref(a), None, 0, ctypes.byref(b), None, 0,
                                                 ctypes.byref(c)), a.value, b.value, c.value]
    n = u64()
    r["fetch_pulled_all"] = [L.nemo_fetch_pulled_all(h, None, None, None, None, 0, ctypes.byref(n)), n.value]
    n = u64()
    r["fetch_chains"] = [L.nemo_fetch_chains(h, None, 0, ctypes.byref(n)), n.value]
    one = np.zeros(8, np.uint8)
    r["fetch_node_flags"] = [L.nemo_fetch_node_flags(h, 0, 0, one.ctypes.data, 8)]
    f, o, t, w = vp(), vp(), vp(), ctypes.c_int32()
    n = u64()
    r["simplified_view"] = [L.nemo_simplified_view(h, ctypes.byref(f), ctypes.byref(o), ctypes.byref(t),
                                                   ctypes.byref(n), ctypes.byref(w))]
    big = np.zeros(4096, np.uint32)
    r["fetch_run_tables"] = [L.nemo_fetch_run_tables(h, 0, big.ctypes.data, 4096)]
    r["fetch_reduce"] = [L.nemo_fetch_reduce(h, big.ctypes.data, 4096)]
    return r


def _sizes(eng):
    """[nemo_num_nodes, nemo_num_edges, nemo_reduce_len]: with no corpus loaded, 0, 0 and 2 * 0 + 4."""
    return [int(eng.L.nemo_num_nodes(eng.h)), int(eng.L.nemo_num_edges(eng.h)), int(eng.L.nemo_reduce_len(eng.h))]


def _no_run0_calls(eng, failed):
    """Step 2's calls that need run 0, on a loaded and marked corpus without one."""
    L, h = eng.L, eng.h
    f = np.ascontiguousarray(failed, np.uint32)
    r = {}
    r["diffprov"] = [L.nemo_diffprov(h, f.ctypes.data, len(f), DIFF_PER_RUN)]
    r["diffprov_symmetric"] = [L.nemo_diffprov_symmetric(h, f.ctypes.data, len(f))]
    r["triggers"] = [L.nemo_triggers(h)]
    for k in ("fetch_missing", "fetch_surplus", "diff_masks_view", "fetch_sdiff_masks", "fetch_triggers"):
        r[k] = _fetches(eng)[k]
    for which in (2, 3):
        n = ctypes.c_uint64()
        r[f"pull_edges({which})"] = [L.nemo_pull_edges(h, which),
                                     L.nemo_fetch_pulled_all(h, None, None, None, None, 0, ctypes.byref(n)), n.value]
    return r


# what the library returned before CorpusState (see the module docstring): [status, counts...]
WANT_NO_RUN0 = {
    "diffprov": [OK],
    "diffprov_symmetric": [OK],
    "triggers": [OK],
    "fetch_missing": [OK, 0],
    "fetch_surplus": [OK, 0],
    "diff_masks_view": [OK, 0, 0, 0],
    "fetch_sdiff_masks": [OK, 0],
    "fetch_triggers": [OK, 0, 0, 0],
    "pull_edges(2)": [OK, OK, 0],
    "pull_edges(3)": [OK, OK, 0],
}
WANT_FAILED_LOAD = {
    "fetch_missing": [OK, 0],
    "fetch_surplus": [STATE, 0],
    "diff_masks_view": [OK, 0, 0, 0],
    "fetch_sdiff_masks": [STATE, 0],
    "fetch_triggers": [STATE, 0, 0, 0],
    "fetch_pulled_all": [STATE, 0],
    "fetch_chains": [STATE, 0],
    "fetch_node_flags": [STATE],
    "simplified_view": [STATE],
    "fetch_run_tables": [STATE],
    "fetch_reduce": [STATE],
}


def test_corpus_state_does_not_outlive_its_corpus():
    A, _ = synth.generate(12, target_nodes=300, p_fault=0.5, prepend_run0=True)
    fa = A.failed_iters()
    assert fa and 0 in set(int(x) for x in A.iteration)
    keep = [r for r in range(A.n_runs) if int(A.iteration[r]) != 0][:7]
    B = A.subset(keep)
    fb = B.failed_iters()
    assert fb and len(fb) < len(fa)
    dup = dataclasses.replace(A, iteration=np.ascontiguousarray([A.iteration[0]] + list(A.iteration[:-1]), np.uint32))

    fresh = E.Engine(0)
    try:
        want = _everything(fresh, A)
    finally:
        fresh.close()
    eng = E.Engine(0)
    try:
        first = _everything(eng, A)
        _same(first, want, "first pass")
        assert len(first["missing"]) or len(first["surplus"]) or first["dmask"].any()  # A's diff is not empty

        # a load that fails its first check (too many tables) leaves none of A's sizes behind: before
        # CorpusState these four reported A's node, edge and table counts and run 0's post graph size
        assert _sizes(eng) == [int(A.node_off[-1]), int(A.edge_off[-1]), 2 * A.n_tables + 4]
        with pytest.raises(E.NemoError) as ei:
            eng.load(dataclasses.replace(A, n_tables=16384 + 1))  # NEMO_MAX_TABLES + 1
        assert "NEMO_MAX_TABLES" in str(ei.value)
        assert _sizes(eng) == [0, 0, 4]
        assert _fetches(eng)["diff_masks_view"] == [OK, 0, 0, 0]

        # 2. the smaller corpus without run 0
        eng.load(B)
        eng.mark()
        eng.simplify()
        orc = O.analyze(B, B.success_iters(), fb, diff_mode=DIFF_PER_RUN)
        assert np.array_equal(eng.flags(), orc.flags) and np.array_equal(eng.chains(), orc.chains)
        eng.pull(1)
        off, cnt, src, dst = eng.pulled_all(B.n_graphs)
        po = orc.pulled_off.astype(np.int64)
        og = np.repeat(np.arange(B.n_graphs, dtype=np.int64), np.diff(po))
        assert np.array_equal(_slots(B.n_graphs, off, cnt, src, dst), _edge_multiset(og, orc.pulled_src, orc.pulled_dst))
        got = _no_run0_calls(eng, fb)
        print("no run 0:", got)
        assert got == WANT_NO_RUN0

        # 3. a load that fails its validation leaves no corpus
        with pytest.raises(E.NemoError) as ei:
            eng.load(dup)
        assert "duplicate run iteration" in str(ei.value)
        got = _fetches(eng)
        print("failed load:", got)
        assert got == WANT_FAILED_LOAD
        assert _sizes(eng) == [0, 0, 4]  # nor the rejected corpus's sizes
        with pytest.raises(E.NemoError) as ei:
            eng.mark()
        assert ei.value.code == STATE

        # 4. the first corpus again
        _same(_everything(eng, A), want, "second pass")
    finally:
        eng.close()
