"""k_build's input phase: every edge and node-word load is a 16-byte load at an index clamped to the
graph's end, issued before the first use of any.  The cases are the shapes at which that can go wrong:
edge counts of every residue mod 4 and an edgeless or one-node graph in the corpus' last position (the
loads past the graph's end read the arrays' padding there, and the next graph's entries elsewhere), and
graphs of more nodes than one batch of word loads covers (2048), so that the later batches run.  Every
corpus is checked against the oracle, and k_build's device arrays against the global tier's."""
import numpy as np
import pytest

from nemo_amd import engine as E
from nemo_amd.corpus import DIFF_REFERENCE, corpus_from_graphs
from oracle import oracle as O
from tests.compare import assert_same

pytestmark = pytest.mark.gpu

WORD_BATCH = 2048  # nodes per batch of node-word loads (BLD_NW * 4 * BLD_BLOCK in k_load.hip)


@pytest.fixture(scope="module")
def eng():
    e = E.Engine(0)
    yield e
    e.close()


def _path(n, tag):
    """goal0 -> rule0 -> goal1 -> ... with a side goal every seventh step: 2n + ceil(n / 7) edges."""
    goals = [{"id": f"goal{i}", "label": f"log(a, {i}, {tag})", "table": "log" if i else "post", "time": str(n - i)}
             for i in range(n + 1)]
    goals += [{"id": f"goals{i}", "label": f"ack(a, {i})", "table": "ack", "time": "1"} for i in range(0, n, 7)]
    rules = [{"id": f"rule{i}", "label": "log", "table": "log", "type": "next" if i % 5 else "single"} for i in range(n)]
    edges = []
    for i in range(n):
        edges += [{"from": f"goal{i}", "to": f"rule{i}"}, {"from": f"rule{i}", "to": f"goal{i + 1}"}]
        if i % 7 == 0:
            edges.append({"from": f"rule{i}", "to": f"goals{i}"})
    return {"goals": goals, "rules": rules, "edges": edges}


EMPTY = {"goals": [], "rules": [], "edges": []}
ONE = {"goals": [{"id": "goal0", "label": "post(a)", "table": "post", "time": "1"}], "rules": [], "edges": []}


def _check(eng, corpus):
    s, f = corpus.success_iters(), corpus.failed_iters()
    orc = O.analyze(corpus, s, f, diff_mode=DIFF_REFERENCE)
    res = E.analyze(corpus, s, f, diff_mode=DIFF_REFERENCE, engine=eng, pulls=True)
    assert_same(corpus, res, orc, len(f), check_pulls=True)


def _tiers_identical(eng, corpus):
    """k_build's CSR rows, level offsets and per-node levels against the global tier's (build_lds_max 0)."""
    V, Ed, G = int(corpus.node_off[-1]), int(corpus.edge_off[-1]), corpus.n_graphs
    sizes = {"lvl": 4 * (V + G), "nlev": 4 * G, "fp": 4 * (V + G), "fc": 4 * Ed, "rp": 4 * (V + G), "rc": 4 * Ed,
             "nlv": 4 * V}
    got = {}
    for key, build_max in (("global", 0), ("build", -1)):
        eng.set_option("build_lds_max", build_max)
        try:
            eng.load(corpus)
            got[key] = {k: eng.debug_copy(k, 0, n).view(np.uint32) for k, n in sizes.items() if n}
        finally:
            eng.set_option("build_lds_max", -1)
    nlev = got["build"]["nlev"]
    for k in got["build"]:
        if k == "lvl":  # the entries past a graph's nlev + 1 offsets are not written
            for g in range(G):
                a = int(corpus.node_off[g]) + g
                n = int(nlev[g]) + 1
                assert np.array_equal(got["build"][k][a:a + n], got["global"][k][a:a + n]), (k, g)
        else:
            assert np.array_equal(got["build"][k], got["global"][k]), k


@pytest.mark.parametrize("n,edges", [(1, 3), (2, 5), (8, 18), (9, 20)])
def test_last_graph_edge_residues(eng, n, edges):
    last = _path(n, 1)
    assert len(last["edges"]) == edges  # residues 3, 1, 2 and 0 mod 4
    corpus = corpus_from_graphs([(0, "success", _path(5, 0), _path(6, 0)), (1, "failure", _path(3, 1), last)])
    assert int(corpus.edge_off[-1] - corpus.edge_off[-2]) == edges
    _check(eng, corpus)
    _tiers_identical(eng, corpus)


@pytest.mark.parametrize("last", ["empty", "one_node"])
def test_last_graph_without_edges(eng, last):
    g = EMPTY if last == "empty" else ONE
    corpus = corpus_from_graphs([(0, "success", _path(5, 0), _path(6, 0)), (1, "failure", g, g)])
    _check(eng, corpus)
    _tiers_identical(eng, corpus)


def test_edgeless_graphs_between_others(eng):
    # a graph whose loads all land on its neighbour's entries, in the middle of the corpus
    corpus = corpus_from_graphs([(0, "success", _path(9, 0), EMPTY), (1, "failure", ONE, _path(8, 1)),
                                 (2, "success", EMPTY, _path(2, 0))])
    _check(eng, corpus)
    _tiers_identical(eng, corpus)


@pytest.mark.parametrize("target", [2500, 4500])
def test_graphs_past_one_word_batch(eng, target):
    from tools import synth
    corpus, _ = synth.generate(4, target_nodes=target)
    sizes = np.diff(corpus.node_off.astype(np.int64))
    assert sizes.max() > (target // WORD_BATCH) * WORD_BATCH  # two and three batches of word loads
    _check(eng, corpus)
    _tiers_identical(eng, corpus)


def test_invalid_endpoint_in_last_group(eng):
    # an out-of-range endpoint in the partial last 16-byte group of the last graph is still refused,
    # and the entries past the graph's end (here the padding) are not taken for edges
    corpus = corpus_from_graphs([(0, "success", _path(5, 0), _path(2, 0))])
    src = corpus.edge_src.copy()
    src[-1] = 60000
    corpus.edge_src = src
    with pytest.raises(E.NemoError) as ei:
        eng.load(corpus)
    assert "edge references a node index out of range" in str(ei.value)
    corpus = corpus_from_graphs([(0, "success", _path(5, 0), _path(2, 0))])
    _check(eng, corpus)
