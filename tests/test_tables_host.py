"""The table-id universe up to NEMO_MAX_TABLES = 16384, host side (no GPU): the oracle under the two
corpus transforms of tests/tables.py, the conditions the split fixtures must meet before a GPU comparison
on them means anything, and nemo_reduce_interpret at T = 16384 against a numpy restatement of
prototype.go:80-130.
"""
import numpy as np
import pytest

from nemo_amd import engine as E
from nemo_amd.corpus import DIFF_PER_RUN, F_HOLDS, TABLE_MASK
from oracle import oracle as O
from tests import tables as TB
from tests.compare import _edge_multiset
from tests.small import random_corpus

UNIVERSES = (33, 64, 4096, 4097, 16384)


def _oracle(corpus, mode=DIFF_PER_RUN):
    return O.analyze(corpus, corpus.success_iters(), corpus.failed_iters(), diff_mode=mode)


def _assert_renamed(corpus, a, b, pi, T):
    """b = the oracle on relabel_tables(corpus, T, pi), a = on corpus: a pure renaming."""
    for k in ("flags", "chains", "diff_mask", "missing", "pre_rows", "post_rows", "pulled_off", "pulled_src",
              "pulled_dst"):
        assert np.array_equal(getattr(a, k), getattr(b, k)), k
    assert np.array_equal(np.sort(a.async_rules), np.sort(b.async_rules))
    assert a.achieved == b.achieved and a.run0 == b.run0 and a.v0 == b.v0
    assert np.array_equal(b.proto_bits, TB.image_bits(a.proto_bits, pi, T))
    assert np.array_equal(b.graph_tables, TB.image_bits(a.graph_tables, pi, T))
    assert sorted(int(t) for t in b.inter) == sorted(pi[int(t)] for t in a.inter)
    assert sorted(int(t) for t in b.union) == sorted(pi[int(t)] for t in a.union)


@pytest.mark.parametrize("seed", range(40))
def test_oracle_invariant_under_relabel_random(seed):
    corpus, _ = random_corpus(seed, n_runs=4, max_nodes=16)
    a = _oracle(corpus)
    for T in UNIVERSES:
        pi = TB.random_pi(corpus, T, 100 * seed + T)
        x = TB.relabel_tables(corpus, T, pi)
        assert x.n_tables == T and len(x.tables) == T and x.tables[x.table_pre] == "pre"
        _assert_renamed(corpus, a, _oracle(x), pi, T)


# the synthetic corpus uses 35 ids: no injective map into 33
@pytest.mark.parametrize("T", [t for t in UNIVERSES if t >= 35])
def test_oracle_invariant_under_relabel_synth(T):
    corpus = TB.base_corpus()
    assert len(TB.used_tables(corpus)) == 35
    pi = TB.random_pi(corpus, T, T)
    _assert_renamed(corpus, _oracle(corpus), _oracle(TB.relabel_tables(corpus, T, pi)), pi, T)


def test_transforms_touch_only_the_table_fields():
    corpus = TB.base_corpus()
    for x in (TB.split_fixture(corpus, 16384), TB.high_relabel_fixture(corpus)[0]):
        assert np.array_equal(x.node_word & ~np.uint32(TABLE_MASK), corpus.node_word & ~np.uint32(TABLE_MASK))
        assert int((x.node_word & np.uint32(TABLE_MASK)).max()) < x.n_tables == len(x.tables) == 16384
        for k in ("iteration", "node_off", "edge_off", "label", "edge_src", "edge_dst"):
            assert getattr(x, k) is getattr(corpus, k)
        assert x.status == corpus.status and x.tables[x.table_pre] == "pre" and x.tables[x.table_post] == "post"
    # the split keeps pre, post and the kept tables whole and the blocks of the others apart
    x = TB.split_fixture(corpus, 16384)
    old, new = corpus.node_word & np.uint32(TABLE_MASK), x.node_word & np.uint32(TABLE_MASK)
    owner = {}
    for o, n in set(zip(old.tolist(), new.tolist())):
        assert owner.setdefault(n, o) == o, f"id {n} drawn by tables {owner[n]} and {o}"
    keep = TB.keep_map(corpus, 16384, *TB.last_word_placement(16384))
    for o, n in list(keep.items()) + [(corpus.table_pre, x.table_pre), (corpus.table_post, x.table_post)]:
        assert set(new[old == o].tolist()) == {n}


@pytest.mark.parametrize("T", UNIVERSES)
def test_split_fixture_not_vacuous(T):
    x = TB.split_fixture(TB.base_corpus(), T)
    pre, post = TB.last_word_placement(T)
    assert (x.table_pre, x.table_post) == (pre, post) and pre != post
    assert pre >> 5 >= TB.words_of(T) - 2 and post >> 5 >= TB.words_of(T) - 2
    TB.assert_nonvacuous(x, _oracle(x), T)


@pytest.mark.parametrize("pre,post", [((16383) & ~31, 16383), (16383, 0)])
def test_split_fixture_other_placements_not_vacuous(pre, post):
    x = TB.split_fixture(TB.base_corpus(), 16384, pre=pre, post=post)
    TB.assert_nonvacuous(x, _oracle(x), 16384)


def test_split_changes_holds():
    """The split moves HOLDS (Tq depends on the new ids), so a comparison on it tests Tq at those ids."""
    corpus = TB.base_corpus()
    a, b = _oracle(corpus), _oracle(TB.split_fixture(corpus, 16384))
    ha, hb = int(((a.flags & F_HOLDS) != 0).sum()), int(((b.flags & F_HOLDS) != 0).sum())
    assert 0 < hb < ha, (ha, hb)


def test_high_relabel_fixture():
    x, pi = TB.high_relabel_fixture(TB.base_corpus())
    assert int((x.node_word & np.uint32(TABLE_MASK)).min()) >= 8192 and min(x.table_pre, x.table_post) >= 8192
    _assert_renamed(TB.base_corpus(), _oracle(TB.base_corpus()), _oracle(x), pi, 16384)


def test_big_fixture_uses_tq_word_0_and_511():
    """The multi-workgroup mark kernels' fixture: graphs of 8192 nodes and more whose Tq has bits in
    its first and in its last word (a holding goal of a table other than the condition's is in Tq)."""
    x = TB.split_fixture(TB.big_corpus(), 16384, pre=16383, post=0)
    TB.assert_big_fixture(x, O.analyze(x, x.success_iters(), x.failed_iters(), skip_pulls=True))


@pytest.mark.parametrize("T", [4096, 4097])
def test_many_runs_fixture(T):
    x = TB.split_fixture(TB.many_runs_corpus(), T)
    TB.assert_many_runs_fixture(x, O.analyze(x, x.success_iters(), x.failed_iters(), skip_pulls=True))


def test_oracle_reduce_vector_is_the_restated_one():
    """tests/tables.py reduce_vector (from proto bits and flags) equals the oracle's own vector."""
    for x in (TB.split_fixture(TB.base_corpus(), 16384), TB.split_fixture(TB.many_runs_corpus(), 4097)):
        orc = O.analyze(x, x.success_iters(), x.failed_iters(), skip_pulls=True)
        assert np.array_equal(TB.reduce_vector(x, orc.proto_bits, orc.flags, x.success_iters()), orc.reduce)


# ---- nemo_reduce_interpret (host function of libnemohip: loads without a device) --------------------

def _interpret_numpy(red, T, table_post):
    """prototype.go:80-130 on the reduction vector: `longest` (and with it the union) stays 0 when the
    first success run's list is empty; a label is in the intersection iff it is in that first list and
    found in every run that achieved the condition; the condition's own table is in neither."""
    cnt, first, achieved, first_nonempty = red[:T], red[T:2 * T], int(red[2 * T]), int(red[2 * T + 1])
    if not first_nonempty:
        return achieved, [], []
    other = np.arange(T) != table_post
    inter = np.nonzero((first != 0) & (cnt == achieved) & other)[0]
    union = np.nonzero((cnt > 0) & other)[0]
    return achieved, inter.tolist(), union.tolist()


@pytest.mark.parametrize("table_post", [0, 16383, 8192, 8191, 31, 32])
@pytest.mark.parametrize("kind", ["dense", "sparse", "first_empty"])
def test_reduce_interpret_full_universe(table_post, kind):
    T = 16384
    rng = np.random.default_rng(table_post + 7 * len(kind))
    achieved = 5
    red = np.zeros(2 * T + 4, np.uint32)
    p = 0.6 if kind == "dense" else 0.01
    red[:T] = rng.integers(0, achieved + 1, T) * (rng.random(T) < p)
    red[T:2 * T] = (red[:T] > 0) & (rng.random(T) < 0.7)
    # the edges: first and last id, both sides of a word boundary and of id 8192, and the condition's table
    for t in (0, 31, 32, 8191, 8192, T - 2, T - 1, table_post):
        red[t], red[T + t] = achieved, 1
    red[2 * T] = achieved
    red[2 * T + 1] = 0 if kind == "first_empty" else 1
    want = _interpret_numpy(red, T, table_post)
    got = E.reduce_interpret(red, T, table_post)
    assert got == want
    if kind != "first_empty":
        edge = {0, 31, 32, 8191, 8192, T - 2, T - 1} - {table_post}
        assert edge <= set(got[1]) and edge <= set(got[2]) and table_post not in got[1] + got[2]
    else:
        assert got == (achieved, [], [])


def test_reduce_interpret_matches_oracle_at_full_universe():
    x = TB.split_fixture(TB.base_corpus(), 16384)
    orc = O.analyze(x, x.success_iters(), x.failed_iters(), skip_pulls=True)
    a, inter, union = E.reduce_interpret(orc.reduce, x.n_tables, x.table_post)
    assert (a, inter, union) == (orc.achieved, [int(t) for t in orc.inter], [int(t) for t in orc.union])
