"""GPU checks of the nearest-run search (nemo_nearest_runs; k_near_lmax, k_near_bits, k_near_isect and k_near_pick
in nemo_amd/csrc/k_near.hip): the whole distance matrix and every result row, exact.

Reference.  There is no reference code for this call (include/nemohip.h fixes the semantics), so the reference is
the definition, computed here with Python sets: L(r) = the distinct labels of the goal nodes of run r's raw post
graph, read from the Corpus arrays; dist = |L(q) ^ L(c)|, only_query = |L(q) - L(c)|, only_cand = |L(c) - L(q)|;
the row of a query is the candidate position of least dist, ties to the smallest position, candidates of the
query's own iteration skipped, UINT32_MAX everywhere when none is left.  It never calls the library.  The link to
the pair diff (only_query == 0 exactly when the S mask is all zero) is checked device against device.

Label values a tiny graph cannot produce are reached by moving a corpus' `label` array through an injective map
(as tests/tables.py does for table ids): the call reads labels as numbers only.
"""
import dataclasses

import numpy as np
import pytest

from nemo_amd import engine as E
from nemo_amd.corpus import NODE_RULE, Corpus, corpus_from_graphs
from tests.small import random_corpus
from tests.test_gpu_sdiff import _with_iterations
from tools import synth

pytestmark = pytest.mark.gpu
NONE = 0xFFFFFFFF
SLAB_BITS = 16 * 64  # k_near_isect stages 16 u64 words of a row per K-slab


@pytest.fixture(scope="module")
def eng():
    e = E.Engine(0)
    yield e
    e.close()


# ---- the reference ----------------------------------------------------------------------------------------------
def label_sets(corpus: Corpus):
    """{iteration: L(r)} from the corpus arrays."""
    out = {}
    for r in range(corpus.n_runs):
        n0, n1 = int(corpus.node_off[2 * r + 1]), int(corpus.node_off[2 * r + 2])
        goal = (corpus.node_word[n0:n1] & np.uint32(NODE_RULE)) == 0
        out.setdefault(int(corpus.iteration[r]), set(int(x) for x in corpus.label[n0:n1][goal]))
    return out


def reference(sets, queries, cands):
    """(distance matrix [n_q, n_c], rows [(cand, dist, only_query, only_cand)])."""
    mat = np.zeros((len(queries), len(cands)), np.uint32)
    rows = []
    for i, q in enumerate(queries):
        best = None
        for j, c in enumerate(cands):
            mat[i, j] = len(sets[q] ^ sets[c])
            if c != q and (best is None or int(mat[i, j]) < best[1]):  # the first of the least: ties to the smallest j
                best = (j, int(mat[i, j]), len(sets[q] - sets[c]), len(sets[c] - sets[q]))
        rows.append(best if best is not None else (NONE, NONE, NONE, NONE))
    return mat, rows


def check(eng, sets, queries, cands, what=""):
    queries, cands = [int(x) for x in queries], [int(x) for x in cands]
    mat, rows = reference(sets, queries, cands)
    got = eng.nearest_runs(queries, cands)
    assert got.dtype == E.NEAREST_DTYPE and len(got) == len(queries), what
    got_rows = [tuple(int(x) for x in r) for r in got.tolist()]
    bad = [i for i in range(len(queries)) if got_rows[i] != tuple(rows[i])]
    assert not bad, f"{what}: rows {bad[:6]} differ: got {[got_rows[i] for i in bad[:6]]}, want {[rows[i] for i in bad[:6]]}"
    d = eng.label_distances()
    assert d.shape == mat.shape, what
    assert np.array_equal(d, mat), f"{what}: {int((d != mat).sum())} of {mat.size} distances differ"
    if len(queries) >= 2:  # a slice of the matrix
        lo, hi = len(queries) // 3, len(queries) - 1
        assert np.array_equal(eng.label_distances(lo, hi), mat[lo:hi]), what
    return got_rows, mat


def all_paths(eng, sets, queries, cands, what=""):
    """Rows built in LDS and in place (near_bits_lds_max -1 / 0), one K range or the automatic choice and three."""
    try:
        for lds in (-1, 0):
            eng.set_option("near_bits_lds_max", lds)
            for ks in (0, 3):
                eng.set_option("near_ksplit", ks)
                out = check(eng, sets, queries, cands, f"{what} lds {lds} ksplit {ks}")
    finally:
        eng.set_option("near_bits_lds_max", -1)
        eng.set_option("near_ksplit", -1)
    return out


def relabel(corpus: Corpus, new_of_old) -> Corpus:
    """The corpus with label id l replaced by new_of_old[l] (injective)."""
    m = np.asarray(new_of_old, np.uint32)
    assert len(np.unique(m)) == len(m) and int(corpus.label.max()) < len(m)
    return dataclasses.replace(corpus, label=np.ascontiguousarray(m[corpus.label], dtype=np.uint32))


# ---- 1. random corpora: every run a query and a candidate ---------------------------------------------------------
@pytest.mark.parametrize("seed", range(4))
def test_random_corpora_every_run_both_ways(eng, seed):
    seen_nonzero = False
    for k, n_runs in enumerate((5, 6, 8)):
        corpus = random_corpus(7000 * seed + 31 * k + 1, n_runs=n_runs, max_nodes=40)[0]
        sets = label_sets(corpus)
        its = [int(x) for x in corpus.iteration]
        eng.load(corpus)
        _, mat = all_paths(eng, sets, its, its, f"seed {seed} corpus {k}")
        assert all(mat[i, i] == 0 for i in range(len(its))), "a self-pair carries its true distance 0"
        seen_nonzero = seen_nonzero or bool(mat.any())
    assert seen_nonzero, "the corpora must hold runs with different label sets"


# ---- 2. hand-built label sets ---------------------------------------------------------------------------------------
def _goal(i, label):
    return {"id": f"goal{i}", "label": label, "table": "t1", "time": "1"}


def _lab(k):
    return f"t1(a, {k})"


def _flat(keys):
    return {"goals": [_goal(i, _lab(k)) for i, k in enumerate(keys)], "rules": [], "edges": []}


PRE = {"goals": [{"id": "goal0", "label": "pre(a)", "table": "pre", "time": "1"}], "rules": [], "edges": []}
# the label values the keys 0..11 are mapped to: word edges, and both sides of the first two K-slab edges
VALUES = [0, 63, 64, 127, 128, SLAB_BITS - 1, SLAB_BITS, 2 * SLAB_BITS - 1, 2 * SLAB_BITS, 5, 700, 1500]
EMPTY, REPEATED, TIE_Q, TIE_A, TIE_B, FAR = 1, 2, 3, 4, 5, 6
HAND = {0: [0, 1, 2, 3, 4, 5, 6, 7, 8],       # every edge value
        EMPTY: [],                             # no goal
        REPEATED: [1, 1, 1, 4, 4, 9],          # one label on several goals: |L| = 3
        TIE_Q: [0, 2, 5, 6],
        TIE_A: [0, 2, 5, 7],                   # dist(TIE_Q, TIE_A) = 2 ...
        TIE_B: [0, 2, 6, 8],                   # ... = dist(TIE_Q, TIE_B)
        FAR: [3, 7, 8, 9, 10, 11],
        7: [0, 2, 5, 6]}                       # the same set as TIE_Q: distance 0 between two runs


@pytest.fixture(scope="module")
def hand():
    runs = []
    for it, keys in HAND.items():
        post = _flat(keys) if keys else {"goals": [], "rules": [{"id": "rule0", "label": "t1", "table": "t1",
                                                                 "type": "single"}], "edges": []}
        runs.append((it, "success" if it in (0, TIE_A, TIE_B, 7) else "fail", PRE, post))
    corpus = corpus_from_graphs(runs)
    # keys -> VALUES; every other label id (the pre goal's, the rule's) goes past them
    new_of_old, spare = [], 3 * SLAB_BITS
    by_name = {_lab(k): v for k, v in enumerate(VALUES)}
    for name in corpus.labels:
        if name in by_name:
            new_of_old.append(by_name[name])
        else:
            new_of_old.append(spare)
            spare += 1
    corpus = relabel(corpus, new_of_old)
    sets = label_sets(corpus)
    assert sets[0] == set(VALUES[:9]) and sets[EMPTY] == set() and sets[REPEATED] == {63, 128, 5}
    return corpus, sets


def test_hand_built_sets(eng, hand):
    corpus, sets = hand
    its = [int(x) for x in corpus.iteration]
    eng.load(corpus)
    rows, mat = all_paths(eng, sets, its, its, "hand")
    q = its.index(TIE_Q)
    assert mat[q, its.index(TIE_A)] == mat[q, its.index(TIE_B)] == 2
    assert rows[its.index(EMPTY)][2] == 0 and rows[its.index(REPEATED)][2] <= 3
    # TIE_Q's nearest is run 7 (the same set); without it two candidates tie at 2 and the lower position wins
    assert rows[q] == (its.index(7), 0, 0, 0)
    for cands in ([TIE_B, TIE_A, FAR], [FAR, TIE_A, TIE_B], [TIE_Q, TIE_B, TIE_Q, TIE_A]):
        got, _ = all_paths(eng, sets, [TIE_Q], cands, f"tie {cands}")
        first = min(j for j, c in enumerate(cands) if c in (TIE_A, TIE_B))
        assert got[0] == (first, 2, 1, 1)


def test_no_candidate_left_duplicates_and_empty_lists(eng, hand):
    corpus, sets = hand
    eng.load(corpus)
    got, mat = all_paths(eng, sets, [FAR, TIE_Q], [FAR, FAR], "only the query itself")
    assert got[0] == (NONE, NONE, NONE, NONE) and got[1][0] == 0 and mat[0, 0] == 0
    all_paths(eng, sets, [TIE_Q, FAR, TIE_Q, 0, 0, EMPTY], [TIE_A, TIE_A, 0, FAR, EMPTY, TIE_A, 0], "duplicates")
    got, mat = check(eng, sets, [0, FAR, EMPTY], [], "no candidate")
    assert got == [(NONE, NONE, NONE, NONE)] * 3 and mat.shape == (3, 0)
    got, mat = check(eng, sets, [], [0, FAR], "no query")
    assert got == [] and mat.shape == (0, 2)
    check(eng, sets, [], [], "neither")


def test_errors(eng, hand):
    corpus, sets = hand
    eng.load(corpus)
    check(eng, sets, [0], [FAR])
    for q, c in (([0, 4242], [FAR]), ([0], [FAR, 4242])):
        with pytest.raises(E.NemoError) as ei:
            eng.nearest_runs(q, c)
        assert ei.value.code == 7 and "unknown run iteration 4242" in ei.value.msg
        with pytest.raises(E.NemoError) as ei:  # the failed call left no result
            eng.label_distances(0, 0)
        assert ei.value.code == 5
        assert eng.L.nemo_fetch_nearest(eng.h, None, 0, None) == 5
    check(eng, sets, [0], [FAR])
    with pytest.raises(E.NemoError) as ei:
        eng.label_distances(0, 2)
    assert ei.value.code == 1


def test_run_0_need_not_be_loaded(eng, hand):
    corpus, sets = hand
    no0 = _with_iterations(corpus, corpus.iteration + np.uint32(1))
    sets1 = {it + 1: s for it, s in sets.items()}
    its = [int(x) for x in no0.iteration]
    assert 0 not in its
    eng.load(no0)
    all_paths(eng, sets1, its, its, "no run 0")


def test_node_context_refuses(hand):
    corpus, _ = hand
    node = E.Engine(devices=[0])
    try:
        node.load(corpus)
        with pytest.raises(E.NemoError) as ei:
            node.nearest_runs([0], [FAR])
        assert ei.value.code == 5 and "single-device contexts only" in ei.value.msg
    finally:
        node.close()


# ---- 3. tile edges: 64 x 64 tiles of list positions ----------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny130():
    corpus = random_corpus(4242, n_runs=130, max_nodes=6)[0]
    assert corpus.n_runs == 130 and max(corpus.graph_size(2 * r + 1) for r in range(130)) <= 6
    sets = label_sets(corpus)
    assert len({frozenset(s) for s in sets.values()}) >= 8
    return corpus, sets


@pytest.mark.parametrize("n", [1, 63, 64, 65, 129])
def test_tile_edges(eng, tiny130, n):
    corpus, sets = tiny130
    its = [int(x) for x in corpus.iteration]
    part = its[130 - n:]
    eng.load(corpus)
    try:
        for ks in (0, 2):
            eng.set_option("near_ksplit", ks)
            check(eng, sets, part, its, f"{n} queries x 130")
            check(eng, sets, its, part, f"130 x {n} candidates")
    finally:
        eng.set_option("near_ksplit", -1)


# ---- 4. long rows: past the LDS path by size, W no multiple of the slab --------------------------------------------
@pytest.fixture(scope="module")
def long130(tiny130):
    corpus, _ = tiny130
    n_lab, top = int(corpus.label.max()) + 1, 599_500
    new_of_old = [(top * l) // (n_lab - 1) if l % 2 else l for l in range(n_lab)]  # spread the odd ids up to `top`
    new_of_old[n_lab - 1 if (n_lab - 1) % 2 else n_lab - 2] = top
    long = relabel(corpus, new_of_old)
    sets = label_sets(long)
    lmax = max(max(s) for s in sets.values() if s)
    words = 2 * ((lmax + 1 + 127) // 128)
    assert 8 * words > 65536 and lmax < 600_000, "rows past the 64 KB LDS path"
    assert words % 16 != 0, "W is not a multiple of the K-slab"
    return long, sets


@pytest.mark.parametrize("ksplit", [0, 1, 7])
def test_long_rows(eng, long130, ksplit):
    corpus, sets = long130
    its = [int(x) for x in corpus.iteration]
    eng.load(corpus)
    try:
        eng.set_option("near_ksplit", ksplit)
        check(eng, sets, its[:70], its, f"long rows, ksplit {ksplit}")
        check(eng, sets, its[5:8], its[60:], f"long rows, few tiles, ksplit {ksplit}")
    finally:
        eng.set_option("near_ksplit", -1)


# ---- 5. against the pair diff, device against device ----------------------------------------------------------------
@pytest.fixture(scope="module")
def c3_12():
    corpus, _ = synth.generate(12, p_fault=0.55, prepend_run0=True, **synth.CONFIGS["c3"])
    return corpus


def _against_pairs(eng, corpus):
    its = [int(x) for x in corpus.iteration]
    pairs = [(q, c) for q in its for c in its if q != c]
    eng.load(corpus)
    eng.mark()
    only_q = []
    for q, c in pairs:  # one call per ordered pair: its row is the pair's
        row = eng.nearest_runs([q], [c])[0]
        assert int(row["cand"]) == 0
        only_q.append(int(row["only_query"]))
    eng.diffprov_pairs([q for q, _ in pairs], [c for _, c in pairs])
    masks = eng.sdiff_masks()
    empty = [not m.any() for m in masks]
    assert [x == 0 for x in only_q] == empty, "only_query == 0 must hold exactly where the S mask is all zero"
    # the search leaves the pair diff's state alone, and the reverse
    rows = eng.nearest_runs(its, its)
    dist = eng.label_distances()
    again = eng.sdiff_masks()
    assert all(np.array_equal(a, b) for a, b in zip(masks, again)), "nemo_nearest_runs disturbed the pair diff's masks"
    picked = [(q, its[int(r["cand"])]) for q, r in zip(its, rows)]
    eng.diffprov_pairs([q for q, _ in picked], [c for _, c in picked])
    assert len(eng.sdiff_masks()) == len(picked)
    assert np.array_equal(eng.label_distances(), dist), "nemo_diffprov_pairs disturbed the distance matrix"
    return only_q, empty


def test_against_the_pair_diff_random(eng):
    corpus = random_corpus(1000, n_runs=6, max_nodes=40)[0]
    only_q, empty = _against_pairs(eng, corpus)
    assert any(empty) or any(only_q), "nothing compared"
    assert not all(empty), "some pair must have a Bad goal"


def test_against_the_pair_diff_c3(eng, c3_12):
    only_q, empty = _against_pairs(eng, c3_12)
    assert any(empty) and not all(empty), "the generator's failed runs derive a subset of the good runs' labels"


# ---- 6. lifetime -----------------------------------------------------------------------------------------------------
def test_results_follow_the_loaded_corpus(eng, hand, tiny130):
    a, sets_a = tiny130
    b, sets_b = hand
    ia, ib = [int(x) for x in a.iteration], [int(x) for x in b.iteration]
    eng.load(a)
    check(eng, sets_a, ia[:9], ia, "first corpus")
    eng.load(b)
    with pytest.raises(E.NemoError) as ei:  # no result of the previous corpus survives the load
        eng.label_distances(0, 0)
    assert ei.value.code == 5
    assert eng.L.nemo_fetch_nearest(eng.h, None, 0, None) == 5
    check(eng, sets_b, ib, ib, "second corpus")  # its own largest label, its own rows
    eng.load(a)
    check(eng, sets_a, ia, ia[:9], "first corpus again")


def test_buffers_grow_and_are_reused(eng, tiny130):
    corpus, sets = tiny130
    its = [int(x) for x in corpus.iteration]
    eng.load(corpus)
    for n in (3, 70, 1, 130, 70):
        check(eng, sets, its[:n], its[::-1][:max(1, 130 - n)], f"{n} queries")
