"""GPU parity over the table-id universe up to NEMO_MAX_TABLES = 16384 (512 words of per-run bitset), on
every tier that keeps a table bitset or a table field: the u16 node word of the LDS tiers (14-bit table
field), markConditionHolds' Tq in k_marksimp / k_mark / k_mw_mark_*, the proto and graph-table bitsets of
k_proto_lds / k_pg_*, k_reduce on both sides of RED_LDS_TABLES and across workgroups, the tier sizing with
4 KB of bitsets in every image, and the host half (nemo_missing_from, nemo_fetch_run_tables,
nemo_fetch_reduce, the node context's shard merge).

The corpora are synthetic ones moved through tests/tables.py; every case first asserts from the oracle's
result that its corpus really uses the ids it is about (a case that cannot meet that fails, it does not
skip), then compares libnemohip with the oracle bit for bit.
"""
import functools

import numpy as np
import pytest

from nemo_amd import engine as E
from nemo_amd.corpus import DIFF_PER_RUN, DIFF_REFERENCE, F_HOLDS, TABLE_MASK
from oracle import oracle as O
from tests import tables as TB
from tests.compare import assert_same

pytestmark = pytest.mark.gpu

T_MAX = TB.MAX_TABLES
SWAPPED = ((T_MAX - 1) & ~31, T_MAX - 1)  # last_word_placement(16384), pre and post exchanged
FAR = (T_MAX - 1, 0)                      # the condition tables in the last and in the first word
GLOBAL_TIER = (("graph_lds_max", 0), ("build_lds_max", 0))


@pytest.fixture(scope="module")
def eng():
    e = E.Engine(0)
    yield e
    e.close()


@functools.lru_cache(maxsize=None)
def _split(base, T, placement=None, mode=DIFF_PER_RUN):
    """(corpus, oracle result) of a split fixture, computed once and shared (never written to)."""
    corpus = {"base": TB.base_corpus, "big": TB.big_corpus, "many": TB.many_runs_corpus}[base]()
    pre, post = placement or TB.last_word_placement(T)
    x = TB.split_fixture(corpus, T, pre=pre, post=post)
    assert (x.table_pre, x.table_post) == (pre, post)
    return x, O.analyze(x, x.success_iters(), x.failed_iters(), diff_mode=mode)


def _missing_from(eng, corpus, orc):
    """nemo_missing_from for every failed run against set arithmetic on the oracle's graph tables: the
    union and inter protos, and every id of the universe (the complement of the run's table set)."""
    T = corpus.n_tables
    have = TB.unpack_bits(orc.graph_tables, T)
    for f in corpus.failed_iters():
        row = have[corpus.run_index(f)]
        for proto in ([int(t) for t in orc.union], [int(t) for t in orc.inter], list(range(T))):
            assert eng.missing_from(f, proto) == [t for t in proto if not row[t]], (f, len(proto))


def _compare(eng, corpus, orc, mode=DIFF_PER_RUN):
    s, f = corpus.success_iters(), corpus.failed_iters()
    res = E.analyze(corpus, s, f, diff_mode=mode, engine=eng, pulls=True)
    assert_same(corpus, res, orc, len(f))
    _missing_from(eng, corpus, orc)
    return res


def _options(eng, opts):
    for k, v in opts:
        eng.set_option(k, v)


def _restore(eng, opts):
    for k, _ in opts:
        eng.set_option(k, -1)


# ---- universe edges, default tiers (k_build, k_marksimp, k_proto_lds) ------------------------------

@pytest.mark.parametrize("T", [33, 64, 4096, 4097])
def test_universe_edges(eng, T):
    corpus, orc = _split("base", T)
    TB.assert_nonvacuous(corpus, orc, T)
    _compare(eng, corpus, orc)


@pytest.mark.parametrize("placement", [None, SWAPPED, FAR], ids=["last_word", "swapped", "far"])
def test_full_universe(eng, placement):
    corpus, orc = _split("base", T_MAX, placement)
    TB.assert_nonvacuous(corpus, orc, T_MAX)
    _compare(eng, corpus, orc)


def _assert_high(corpus, orc):
    assert int((corpus.node_word & np.uint32(TABLE_MASK)).min()) >= 8192
    assert min(corpus.table_pre, corpus.table_post) >= 8192
    assert ((orc.flags & F_HOLDS) != 0).any() and len(orc.inter) > 0 and min(int(t) for t in orc.union) >= 8192


def test_full_universe_every_id_high(eng):
    """A pure renaming with every id in use at 8192 and above: the top bit of the 14-bit table field."""
    corpus, _ = TB.high_relabel_fixture(TB.base_corpus())
    orc = O.analyze(corpus, corpus.success_iters(), corpus.failed_iters(), diff_mode=DIFF_PER_RUN)
    _assert_high(corpus, orc)
    _compare(eng, corpus, orc)


# ---- global tier: k_mark, k_simplify_flags, k_pg_* --------------------------------------------------

@pytest.mark.parametrize("T", [64, 4097, T_MAX])
def test_global_tier(eng, T):
    corpus, orc = _split("base", T)
    TB.assert_nonvacuous(corpus, orc, T)
    _options(eng, GLOBAL_TIER)
    try:
        _compare(eng, corpus, orc)
    finally:
        _restore(eng, GLOBAL_TIER)


# ---- graphs of NEMO_CSR_BIG nodes and more: k_mw_mark_z/a/b ------------------------------------------

@pytest.mark.parametrize("tiers", ["default", "global"])
def test_multi_workgroup_tier(eng, tiers):
    """With the LDS graph tiers off, every graph of 8192 nodes and more is marked by k_mw_mark_*, whose
    Tq (W + 1 words in the graph's slice of scratch) here has bits in word 0 and in word 511; with the
    default tiers k_marksimp takes the same graphs (16384 nodes at most) at the same universe."""
    corpus, orc = _split("big", T_MAX, FAR)
    TB.assert_big_fixture(corpus, orc)
    opts = GLOBAL_TIER[:1] if tiers == "global" else ()
    _options(eng, opts)
    try:
        _compare(eng, corpus, orc)
    finally:
        _restore(eng, opts)


# ---- k_build's fused tail ------------------------------------------------------------------------

def test_build_marksimp_tail_full_universe(eng):
    """Option build_marksimp 1: k_build's tail carves marksimp_bytes(V, 512) out of k_build's own LDS
    image.  The tail must really have run at this universe (4 KB of Tq in an image of some 11 KB): right
    after the load, before any mark or simplify call, the device's flags already hold the oracle's
    HOLDS bits."""
    corpus, orc = _split("base", T_MAX)
    TB.assert_nonvacuous(corpus, orc, T_MAX)
    opts = (("build_marksimp", 1),)
    other, _ = _split("base", 64)  # another corpus' flags in the buffer first
    eng.load(other)
    eng.mark()
    eng.simplify()
    _options(eng, opts)
    try:
        eng.load(corpus)
        raw = eng.debug_copy("flags", 0, len(orc.flags))
        assert np.array_equal(raw & F_HOLDS, orc.flags & F_HOLDS), "k_build's tail did not run on every graph"
        _compare(eng, corpus, orc)
    finally:
        _restore(eng, opts)


# ---- k_reduce across workgroups, on both sides of RED_LDS_TABLES ---------------------------------

@pytest.mark.parametrize("T", [4096, 4097])
def test_reduce_across_workgroups(eng, T):
    corpus, orc = _split("many", T)
    TB.assert_many_runs_fixture(corpus, orc)
    _compare(eng, corpus, orc)
    want = TB.reduce_vector(corpus, orc.proto_bits, orc.flags, corpus.success_iters())
    got = eng.reduce_vector()
    assert got.shape == want.shape == (2 * T + 4,)
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, f"reduce vector differs at {bad[:8].tolist()}: {got[bad[:8]].tolist()} vs {want[bad[:8]].tolist()}"


# ---- node context: shard merge of the 2T + 4 vector, node_fetch_run_tables at W = 512 --------------

def test_node_context_full_universe():
    e = E.Engine(devices=[0, 0, 0])
    try:
        assert e.devices() == [0, 0, 0]
        for mode in (DIFF_REFERENCE, DIFF_PER_RUN):
            x, orc = _split("base", T_MAX, None, mode)
            TB.assert_nonvacuous(x, orc, T_MAX)
            _compare(e, x, orc, mode)
        assert e.reduce_len() == 2 * T_MAX + 4
    finally:
        e.close()


# ---- reload across universes on one context -------------------------------------------------------

def test_reload_across_universes(eng):
    """16384, then 33, then 4097 tables on one context: every bitset cleared and every host buffer sized
    for the corpus at hand, not for the one before."""
    for T in (T_MAX, 33, 4097):
        corpus, orc = _split("base", T)
        TB.assert_nonvacuous(corpus, orc, T)
        res = _compare(eng, corpus, orc)
        assert res.proto_bits.shape == (corpus.n_runs, TB.words_of(T))
        assert eng.reduce_len() == 2 * T + 4


# ---- metamorphic, on the device alone -------------------------------------------------------------

def test_relabel_is_a_renaming_on_the_device(eng):
    """The device's own results on a corpus and on its renaming into [8192, 16384): everything but the
    table sets identical, the table sets permuted."""
    base = TB.base_corpus()
    corpus, pi = TB.high_relabel_fixture(base)
    s, f = base.success_iters(), base.failed_iters()
    a = E.analyze(base, s, f, diff_mode=DIFF_PER_RUN, engine=eng, pulls=False)
    b = E.analyze(corpus, s, f, diff_mode=DIFF_PER_RUN, engine=eng, pulls=False)
    assert ((a.flags & F_HOLDS) != 0).any() and a.proto_bits.any() and len(f) > 0 and a.diff_mask.any()
    for k in ("flags", "chains", "diff_mask", "missing", "pre_rows", "post_rows"):
        assert np.array_equal(getattr(a, k), getattr(b, k)), k
    assert np.array_equal(np.sort(a.async_rules), np.sort(b.async_rules))
    assert a.achieved == b.achieved
    assert np.array_equal(b.proto_bits, TB.image_bits(a.proto_bits, pi, T_MAX))
    assert np.array_equal(b.graph_tables, TB.image_bits(a.graph_tables, pi, T_MAX))
    assert sorted(b.inter) == sorted(pi[t] for t in a.inter) and sorted(b.union) == sorted(pi[t] for t in a.union)
