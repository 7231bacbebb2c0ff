"""The plain load reference (tests/load_reference.py) against itself and the edge lists, without a device:
its two level forms agree, its rows are the edge list, and relationships-created equals E on every graph
the host layer builds."""
import numpy as np
import pytest

from nemo_amd.corpus import corpus_from_graphs
from tests import load_cases as C
from tests import load_reference as R
from tests.small import random_corpus


def _check(corpus):
    for g in range(corpus.n_graphs):
        ref = R.graph_reference(corpus, g)  # asserts that peeling and the longest-path recursion agree
        V, src, dst, _ = R.graph_edges(corpus, g)
        assert ref["created"] == ref["E"] == len(src)
        assert ref["fp"][0] == 0 and ref["fp"][-1] == len(src) and len(ref["fp"]) == V + 1
        assert ref["rp"][0] == 0 and ref["rp"][-1] == len(src) and len(ref["rp"]) == V + 1
        edges = set(zip(src.tolist(), dst.tolist()))
        fwd = {(v, int(t)) for v in range(V) for t in ref["fc"][ref["fp"][v]:ref["fp"][v + 1]]}
        rev = {(int(s), v) for v in range(V) for s in ref["rc"][ref["rp"][v]:ref["rp"][v + 1]]}
        assert fwd == edges and rev == edges and len(edges) == len(src)
        # a level is one past the deepest parent, so every edge goes to a strictly deeper level
        assert np.all(ref["nlv"][dst] > ref["nlv"][src])
        assert ref["lvl"][-1] == V and len(ref["lvl"]) == ref["nlev"] + 1


@pytest.mark.parametrize("seed", range(12))
def test_reference_on_random_corpora(seed):
    corpus, _ = random_corpus(seed, max_nodes=40)
    _check(corpus)


def test_reference_on_ladder_graphs():
    corpus = corpus_from_graphs(C.ladder_runs())
    _check(corpus)
    for r, (n, mix8, order) in enumerate(C.LADDER_VARIANTS):
        ref = R.graph_reference(corpus, 2 * r + 1)
        _, _, _, role = C.ladder_index(n, mix8, order)
        fdeg, rdeg = np.diff(ref["fp"]), np.diff(ref["rp"])
        assert fdeg[role["a"]] == fdeg[role["b"]] == rdeg[role["c"]] == rdeg[role["d"]] == n
        assert ref["fc"][ref["fp"][role["a"] + 1] - 1] == ref["V"] - 1  # node V - 1 ends a's row
        for v in role.values():  # the long rows' waves: other rows of at most one entry, or of FILL with mix8
            w = slice(64 * (v // 64), 64 * (v // 64) + 64)
            other = sorted(set(fdeg[w].tolist() + rdeg[w].tolist()) - {n})
            assert (C.FILL in other) == mix8 and all(x <= 1 or x == C.FILL for x in other)


@pytest.mark.parametrize("L,V", [(6, 48), (9, 48), (253, 4100), (256, 4100)])
@pytest.mark.parametrize("order", ["asc", "desc"])
def test_reference_level_counts(L, V, order):
    corpus = corpus_from_graphs([(0, "success", C.small_path(5), C.levels(L, V, order))])
    ref = R.graph_reference(corpus, 1)
    assert ref["V"] == V and ref["nlev"] == L
    _check(corpus)


@pytest.mark.parametrize("kind", ["goal", "rule"])
def test_reference_indegree(kind):
    corpus = corpus_from_graphs([(0, "success", C.small_path(5), C.indegree(256, kind))])
    assert int(np.diff(R.graph_reference(corpus, 1)["rp"]).max()) == 256
    _check(corpus)


def test_e2_reference_statement():
    corpus = corpus_from_graphs([(0, "success", C.small_path(5), C.ladder(5, True, "shuf"))])
    ref = R.graph_reference(corpus, 1)
    topo = np.argsort(ref["nlv"], kind="stable")  # some Kahn order
    posoff, e2 = R.e2_reference(ref, topo)
    assert sorted((int(x) >> 16, int(x) & 0xFFFF) for x in e2) == sorted(zip(*[a.tolist() for a in R.graph_edges(corpus, 1)[1:3]]))
    assert np.all(np.diff(posoff) >= 0) and posoff[0] == 0
    assert np.array_equal(e2 >> 16, np.repeat(topo, np.diff(ref["fp"])[topo]))
