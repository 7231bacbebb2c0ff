"""The four knock-out calls keep their results apart (api_knock.hip, api_cuts.hip, api_klabel.hip, api_lcuts.hip
share knock_api.h's host code, each with its own event, pinned buffer and state): nemo_knockout_leaves,
nemo_min_cuts, nemo_knockout_labels and nemo_min_label_cuts back to back on one context, then every fetch in reverse
order, against the fetch made right after the same call on a context that ran nothing else.  Device against device:
what the calls compute is checked against plain-Python references in test_gpu_knockout.py, test_gpu_min_cuts.py,
test_gpu_knockout_labels.py and test_gpu_label_cuts.py.  Both tiers: knock_lds_max default and 0.
"""
import numpy as np
import pytest

from nemo_amd import engine as E
from tests.small import random_corpus
from tests.test_gpu_knockout_labels import Ref

pytestmark = pytest.mark.gpu
NO_LABEL = 0xFFFFFFFF


@pytest.fixture(scope="module")
def inputs():
    """three runs of at most 12 nodes a graph; at most 8 candidates and 8 sets (seed 5: every call returns rows, the
    two cut searches in rounds 2 and 3 as well)"""
    corpus, _ = random_corpus(5, n_runs=3, max_nodes=12)
    iters = [int(x) for x in corpus.iteration]
    ref = Ref(corpus)
    graphs = [ref.graph(2 * corpus.run_index(it) + 1) for it in iters]
    g0 = graphs[0]
    cand = (list(g0.leaves) + [v for v in g0.roots if v not in g0.leaves])[:8]
    labels = [g.label[v] for g in graphs for v in list(g.roots) + list(g.leaves) if g.label[v] != NO_LABEL]
    labels = [int(x) for x in dict.fromkeys(labels)][:8]
    sets = [[x] for x in labels[:6]] + [labels[:2], labels[2:5]]
    return {"corpus": corpus, "iters": iters, "cand": cand, "labels": labels, "sets": sets}


def call(eng, inp, which):
    if which == "leaves":
        eng.knockout_leaves(inp["iters"], 1)
    elif which == "cuts":
        eng.min_cuts(inp["iters"][0], 1, inp["cand"], 3)
    elif which == "labels":
        eng.knockout_labels(inp["iters"], 1, inp["sets"])
    else:
        eng.min_label_cuts(inp["iters"], 1, inp["labels"], 3, min_runs=1)


def fetch(eng, inp, which):
    """everything the call's fetches return, as bytes and lists"""
    if which == "leaves":
        first, count = eng.knockout_ranges()
        return eng.knockout_rows().tobytes(), first.tolist(), count.tolist()
    if which == "cuts":
        return eng.min_cut_rows().tobytes(), eng.min_cut_stats().tolist()
    if which == "labels":
        n, ck = len(inp["iters"]), (len(inp["sets"]) + 63) // 64
        lost, hit = np.zeros((n, ck), np.uint64), np.zeros((n, ck), np.uint64)
        eng._chk(eng.L.nemo_fetch_knockout_labels(eng.h, lost.ctypes.data, hit.ctypes.data, lost.size))
        n_lost, n_hit = eng.knockout_label_counts()
        return lost.tobytes(), hit.tobytes(), n_lost.tolist(), n_hit.tolist()
    rows, n_lost = eng.min_label_cut_rows()
    return rows.tobytes(), n_lost.tolist(), eng.min_label_cut_stats().tolist()


ORDER = ("leaves", "cuts", "labels", "lcuts")


@pytest.mark.parametrize("lds", [-1, 0], ids=["lds-tier", "global-tier"])
def test_the_four_calls_keep_their_results_apart(inputs, lds):
    want = {}
    for which in ORDER:  # the call alone on a fresh context, its fetch right behind it
        eng = E.Engine(0)
        try:
            eng.load(inputs["corpus"])
            eng.set_option("knock_lds_max", lds)
            call(eng, inputs, which)
            want[which] = fetch(eng, inputs, which)
        finally:
            eng.close()
    assert len(want["leaves"][0]) and len(want["cuts"][0]) and len(want["lcuts"][0]), "every call returns a row"
    assert any(want["labels"][0]) and any(want["labels"][1]), "some set is lost and some hits"
    eng = E.Engine(0)
    try:
        eng.load(inputs["corpus"])
        eng.set_option("knock_lds_max", lds)
        for which in ORDER:
            call(eng, inputs, which)
        for which in reversed(ORDER):
            assert fetch(eng, inputs, which) == want[which], f"{which}: the fetch after the other three calls differs"
        for which in reversed(ORDER):  # and each call again behind the others: the same rows once more
            call(eng, inputs, which)
        for which in ORDER:
            assert fetch(eng, inputs, which) == want[which], f"{which}: the fetch after a second round of calls differs"
    finally:
        eng.close()
