"""The sliced hand-over (options stage_slices, stage_pair_slices, stage_slice_ratio): nemo_stage_simplified packs and
copies the 2-bit node state and the chain pairs in K slices (the state's growing by the ratio, 4 by default), the
pairs ordered behind the end of nemo_simplify rather than behind whatever was queued since.  Every case runs load,
mark, simplify, stage_simplified, simplified_view and compares the state words, chain_off and the pairs with a fresh
engine's at one slice of each, and with the oracle's flags and chains.

A load resets the pair-count hint, so the first stage after it counts the pairs first and issues them in one slice;
the slices of the pairs run from the second stage of a load on.  Each case therefore stages twice."""
import functools

import numpy as np
import pytest

from nemo_amd import engine as E
from nemo_amd.corpus import DIFF_PER_RUN, F_DELETED, F_HOLDS, F_KEPT
from oracle import oracle as O
from tests.compare import assert_same
from tests.small import random_corpus

pytestmark = pytest.mark.gpu

KS = [1, 2, 3, 8]


@pytest.fixture(scope="module")
def eng():
    e = E.Engine(0)
    yield e
    e.close()


def _synth(n_runs, **kw):
    """A synthetic corpus whose node count is no multiple of 16 (the state's tail word is partial)."""
    from tools import synth
    for extra in range(16):
        corpus, _ = synth.generate(n_runs + extra, **kw)
        if int(corpus.node_off[-1]) % 16:
            return corpus
    raise AssertionError("no corpus with V % 16 != 0")


@functools.lru_cache(maxsize=None)
def _case(name):
    """(corpus, oracle result), computed once and left unchanged."""
    if name == "odd":  # tens of runs of graphs of a few hundred nodes, V % 16 != 0
        corpus = _synth(20, target_nodes=300)
    elif name == "hand":  # a handful of graphs: with three slices some graph's pairs straddle a boundary
        corpus = _synth(2, target_nodes=400)
    elif name == "big":  # more chains than "hand"
        corpus = _synth(30, target_nodes=600, p_fault=0.4)
    elif name == "wide":  # a graph of >= 65536 nodes: (head, tail) as two u32
        corpus = _synth(1, target_nodes=80000, eot=200)
        assert max(corpus.graph_size(g) for g in range(corpus.n_graphs)) >= 65536
    elif name in ("tiny", "nochain", "few"):
        # tiny: V < 16 K for K = 3 and 8 (some state slices empty); nochain: no chain at all; few: 1..2 chains
        # (more slices than pairs)
        for seed in range(400):
            corpus, _ = random_corpus(7000 + seed, n_runs=1, max_nodes=12)
            V = int(corpus.node_off[-1])
            orc = O.analyze(corpus, corpus.success_iters(), corpus.failed_iters(), skip_pulls=True)
            n = len(orc.chains)
            if V % 16 and V < 32 and ((name == "tiny" and n) or (name == "nochain" and n == 0) or
                                       (name == "few" and 1 <= n <= 2)):
                return corpus, orc
        raise AssertionError(f"no {name} corpus among the seeds")
    else:
        raise KeyError(name)
    s, f = corpus.success_iters(), corpus.failed_iters()
    return corpus, O.analyze(corpus, s, f, diff_mode=DIFF_PER_RUN, skip_pulls=name == "wide")


def _slices(eng, K):
    """K slices of the node state and of the chain pairs (-1: the defaults)."""
    eng.set_option("stage_slices", K)
    eng.set_option("stage_pair_slices", K)


def _view(eng):
    state, off, ht = eng.simplified_view()
    return state.copy(), off.copy(), ht.copy()


def _pass(eng, between=None):
    eng.mark()
    eng.simplify()
    if between:
        between()
    eng.stage_simplified()
    return _view(eng)


def _assert_oracle(corpus, orc, view):
    state, off, ht = view
    alive, holds = E.Engine.unpack_state(state, len(orc.flags))
    assert np.array_equal(alive, (orc.flags & (F_KEPT | F_DELETED)) == F_KEPT)
    assert np.array_equal(holds, (orc.flags & F_HOLDS) != 0)
    G = corpus.n_graphs
    assert len(off) == G + 1 and int(off[-1]) == len(ht) == len(orc.chains)
    g = np.repeat(np.arange(G), np.diff(off.astype(np.int64)))
    k = np.arange(len(ht)) - off[g].astype(np.int64)
    got = np.stack([g, k, ht[:, 0].astype(np.int64), ht[:, 1].astype(np.int64)], 1).reshape(-1, 4)
    assert np.array_equal(got, orc.chains[:, :4].astype(np.int64).reshape(-1, 4))


def _assert_same_view(a, b):
    for x, y, what in zip(a, b, ("state", "chain_off", "pairs")):
        assert x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x, y), what


@functools.lru_cache(maxsize=None)
def _one_slice(name):
    """The case's view from a fresh engine at stage_slices=1 (second stage of the load: the hinted path)."""
    corpus, _ = _case(name)
    e = E.Engine(0)
    try:
        _slices(e, 1)
        e.load(corpus)
        _pass(e)
        e.rebuild()
        return _pass(e)
    finally:
        e.close()


def _staged_twice(eng, name, K, **opts):
    """Load the case at K slices (and `opts`), stage twice (counted, then hinted): both views against the one-slice
    engine's and the oracle's."""
    corpus, orc = _case(name)
    for o, v in opts.items():
        eng.set_option(o, v)
    _slices(eng, K)
    try:
        eng.load(corpus)
        first = _pass(eng)
        eng.rebuild()
        second = _pass(eng)
    finally:
        _slices(eng, -1)
        for o in opts:
            eng.set_option(o, -1)
    ref = _one_slice(name)
    for v in (first, second):
        _assert_same_view(v, ref)
        _assert_oracle(corpus, orc, v)
    return second


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("name", ["odd", "tiny", "nochain", "few"])
def test_slices_equal_one_slice_and_the_oracle(eng, name, K):
    corpus, orc = _case(name)
    V = int(corpus.node_off[-1])
    assert V % 16 != 0
    if name == "tiny":
        assert (V + 15) // 16 < 3  # fewer state words than slices at K = 3 and 8
    if name == "nochain":
        assert len(orc.chains) == 0
    if name == "few":
        assert 1 <= len(orc.chains) < 3  # fewer pairs than slices at K = 3 and 8
    _staged_twice(eng, name, K)


def test_a_graphs_pairs_straddle_a_slice_boundary(eng):
    state, off, ht = _staged_twice(eng, "hand", 3)
    n = int(off[-1])
    assert n >= 3
    off = off.astype(np.int64)
    bounds = [k * n // 3 for k in (1, 2)]
    assert any(off[g] < b < off[g + 1] for b in bounds for g in range(len(off) - 1)), (off.tolist(), bounds)


@pytest.mark.parametrize("K", [2, 8])
def test_wide_pairs(eng, K):
    second = _staged_twice(eng, "wide", K)
    assert second[2].dtype == np.uint32 and len(second[2]) > 8


@pytest.mark.parametrize("K", [1, 3])
def test_short_hint_and_first_stage_after_a_load(eng, K):
    """A corpus is staged (twice: its count becomes the hint), then one with more chains is loaded into the same
    context: the very first stage after that load has no hint, and the view comes out right."""
    small, small_orc = _case("hand")
    big, big_orc = _case("big")
    assert len(big_orc.chains) > len(small_orc.chains)
    _slices(eng, K)
    try:
        eng.load(small)
        _pass(eng)
        eng.rebuild()
        _assert_oracle(small, small_orc, _pass(eng))
        eng.load(big)
        v = _pass(eng)
        _assert_oracle(big, big_orc, v)
        _assert_same_view(v, _one_slice("big"))
        eng.rebuild()
        _assert_same_view(_pass(eng), _one_slice("big"))
    finally:
        _slices(eng, -1)


@pytest.mark.parametrize("K", [1, 3])
def test_flags_and_chains_rewritten_before_the_stage(eng, K):
    """mark or simplify called again between simplify and stage_simplified (chains_final / flags_final cleared and
    set again), and stage_simplified twice in a row: the view equals a fresh engine's."""
    corpus, orc = _case("odd")
    ref = _one_slice("odd")
    _slices(eng, K)
    try:
        eng.load(corpus)
        _pass(eng)  # the hint
        eng.rebuild()
        eng.mark()
        eng.simplify()
        eng.mark()  # rewrites the flags: nothing is final
        eng.simplify()
        eng.stage_simplified()
        _assert_same_view(_view(eng), ref)
        eng.simplify()  # again, without a mark
        eng.stage_simplified()
        eng.stage_simplified()  # twice in a row: the second waits for the first's copies and reuses the buffers
        v = _view(eng)
        _assert_same_view(v, ref)
        _assert_oracle(corpus, orc, v)
        _slices(eng, K)  # an option change between simplify and the stage: behind the stream again
        eng.stage_simplified()
        _assert_same_view(_view(eng), ref)
    finally:
        _slices(eng, -1)


@pytest.mark.parametrize("opt,value", [("stage_aux", 0), ("graph_dedup", 0), ("stage_blocks", 64),
                                       ("stage_slice_ratio", 1), ("stage_slice_ratio", 8)])
def test_slices_with_the_other_staging_options(eng, opt, value):
    _staged_twice(eng, "odd", 3, **{opt: value})


@pytest.mark.parametrize("K", [1, 4])
def test_protos_and_pulls_queued_before_the_stage(eng, K):
    """The benchmark's order: the diff after mark, protos_partial between simplify and stage_simplified, the
    triggers and the simplified pull behind it.  The pairs now start at the end of nemo_simplify, beside the protos:
    every result still equals the oracle's."""
    from tools import synth
    corpus, _ = synth.generate(24, target_nodes=1500, p_fault=0.4)
    s, f = corpus.success_iters(), corpus.failed_iters()
    assert len(s) and len(f)
    orc = O.analyze(corpus, s, f, diff_mode=DIFF_PER_RUN)
    _slices(eng, K)
    try:
        eng.load(corpus)
        for _ in range(2):  # the second pass stages at the hint, in K slices
            eng.rebuild()
            eng.mark()
            eng.diffprov(f, DIFF_PER_RUN)
            eng.simplify()
            eng.protos_partial(s, 0)
            eng.stage_simplified()
            eng.protos_stage(0)
            eng.triggers()
            eng.pull(1)
            pr = eng.protos_finalize(0)
            off, cnt, src, dst = eng.pulled_all(corpus.n_graphs)
            pulled = [(src[int(a):int(a) + int(n)], dst[int(a):int(a) + int(n)]) for a, n in zip(off, cnt)]
            masks = np.stack([eng.diff_mask(e) for e in range(len(f))])
            pre, post, asy = eng.trigger_rows()
            view = _view(eng)
            res = E.EngineResult(flags=eng.flags(), chains=eng.chains(), proto_bits=eng.run_tables(0),
                                 graph_tables=eng.run_tables(1), achieved=pr["achieved"], inter=pr["inter"],
                                 union=pr["union"], diff_mask=masks, missing=eng.missing(), pre_rows=pre,
                                 post_rows=post, async_rules=asy, pulled=pulled)
            assert_same(corpus, res, orc, len(f))
            _assert_oracle(corpus, orc, view)
    finally:
        _slices(eng, -1)
