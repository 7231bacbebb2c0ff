"""GPU checks of nemo_min_label_cuts (k_lc_table, k_lc_lds, k_lc_glob, k_lc_reduce and k_lc_support in
nemo_amd/csrc/k_lcuts.hip, with k_cuts.hip's row kernels): every row, every n_lost and the nine stats, exact.

Reference.  There is no reference code for the call (include/nemohip.h fixes the semantics), so the reference is the
definition in plain Python and never calls the library.  It enumerates every subset of size <= max_size of the
candidate list, translates each to F(i,S) per listed graph and computes lost per (graph, set) in the two existing
forms, which must agree with each other first (Ref.words of tests/test_gpu_knockout_labels.py: lost_at_once of
tests/test_gpu_min_cuts.py for all sets at once, Graph.dead_by_derivation of tests/test_gpu_knockout.py per set, on
every set, or on every third or fifth set where the graphs are large, on every 97th in the straddle case).  It then counts list positions, applies q, keeps the subsets none of whose proper subsets
is a cut, and orders them by (size, colex rank over the live list); the live list is the definition's: the candidates
that are no cut alone and hit a node of some listed graph.

Every case runs on both tiers (knock_lds_max default and 0), with and without NEMO_KL_SINKS, and under kl_grid 0, 1
and 3.  Two further checks are device against device: nemo_min_cuts on one graph whose labels are node indices, and
nemo_knockout_labels on the returned rows and their proper subsets.
"""
import ctypes
import itertools
import sys
import time
from math import comb

import numpy as np
import pytest

from nemo_amd import engine as E
from tests.small import random_corpus
from tests.test_gpu_knockout import Graph, build
from tests.test_gpu_knockout_labels import HAND, Ref, relabel
from tests.test_gpu_min_cuts import chains, fault_tree, hub, level, level_of, three_rules
from tools import synth

pytestmark = pytest.mark.gpu
sys.setrecursionlimit(max(sys.getrecursionlimit(), 20000))
GRIDS = (0, 1, 3)
NONE = 0xFFFFFFFF


@pytest.fixture(scope="module")
def eng():
    e = E.Engine(0)
    yield e
    e.close()


# ---- the reference ----------------------------------------------------------------------------------------------
def colex(pos):
    """the colex rank of live positions a < b < c"""
    return sum(comb(p, k + 1) for k, p in enumerate(pos))


def reference(ref, iters, cond, cand, max_size, min_runs, sinks, sample=1, numpy_form=False):
    """(rows [(size, labels)], n_lost, stats [9], info) by the definition"""
    n, K = len(iters), len(cand)
    stats = [0] * 9
    if not n or not K:
        return [], [], stats, {"K1": 0, "rejected": 0}
    q = min_runs or n
    subsets = [c for s in range(1, max_size + 1) for c in itertools.combinations(range(K), s)]
    sets = [[cand[p] for p in c] for c in subsets]
    count, hits, memo = [0] * len(sets), [0] * K, {}
    for it in iters:  # a run listed twice is computed once and counts twice
        if it not in memo:
            memo[it] = ref.words(it, cond, sets, sinks, sample, numpy_form)[:2]
        lo, hi = memo[it]
        for s in range(len(sets)):
            count[s] += (lo >> s) & 1
        for p in range(K):
            hits[p] += (hi >> p) & 1  # the singletons come first
    cut = {c: count[s] >= q for s, c in enumerate(subsets)}
    cnt = {c: count[s] for s, c in enumerate(subsets)}
    live = [p for p in range(K) if not cut[(p,)] and hits[p]]
    lpos = {p: k for k, p in enumerate(live)}
    found, rejected = [], 0
    for c in subsets:
        if not cut[c]:
            continue
        proper = [x for s in range(1, len(c)) for x in itertools.combinations(c, s)]
        if any(cut[x] for x in proper):
            rejected += len(c) == 3 and not any(cut[(p,)] for p in c)  # a triple of live candidates with a cut pair
            continue
        assert len(c) == 1 or all(p in lpos for p in c), "a minimal cut names live candidates only"
        found.append((len(c), colex([lpos[p] for p in c]) if len(c) > 1 else c[0], c))
    found.sort()
    rows = [(size, tuple(cand[p] for p in c)) for size, _, c in found]
    n_lost = [cnt[c] for _, _, c in found]
    K1 = len(live)
    for s in range(1, max_size + 1):
        stats[3 * (s - 1):3 * s] = [K if s == 1 else K1, comb(K if s == 1 else K1, s), sum(1 for r in rows if r[0] == s)]
    return rows, n_lost, stats, {"K1": K1, "rejected": rejected, "live": [cand[p] for p in live]}


def got_rows(rows):
    return [(int(r["size"]), tuple(int(x) for x in r["label"][:int(r["size"])])) for r in rows]


def compare(eng, iters, cond, cand, max_size, min_runs, sinks, want, what):
    rows, n_lost = eng.min_label_cuts(iters, cond, cand, max_size, min_runs, sinks_only=sinks)
    assert rows.dtype == E.LABEL_CUT_DTYPE and n_lost.dtype == np.uint32 and len(rows) == len(n_lost), what
    for r in rows:
        assert all(int(x) == NONE for x in r["label"][int(r["size"]):]), f"{what}: unused entries"
    assert got_rows(rows) == want[0], f"{what}: rows"
    assert n_lost.tolist() == want[1], f"{what}: n_lost"
    assert eng.min_label_cut_stats().reshape(-1).tolist() == want[2], f"{what}: stats"
    return rows, n_lost


def everywhere(eng, ref, iters, cand, max_size, min_runs, what, cond=1, sample=1, numpy_form=False, grids=GRIDS, loaded=False,
               flags=(False, True)):
    """the case with and without NEMO_KL_SINKS, on both tiers and under every kl_grid; the reference once per flag"""
    if not loaded:
        eng.load(ref.corpus)
    out = {}
    try:
        for sinks in flags:
            want = reference(ref, iters, cond, cand, max_size, min_runs, sinks, sample, numpy_form)
            for lds in (-1, 0):
                for grid in grids:
                    eng.set_option("knock_lds_max", lds)
                    eng.set_option("kl_grid", grid)
                    compare(eng, iters, cond, cand, max_size, min_runs, sinks, want,
                            f"{what}, sinks {sinks}, knock_lds_max {lds}, kl_grid {grid}")
            out[sinks] = want
    finally:
        eng.set_option("knock_lds_max", -1)
        eng.set_option("kl_grid", 0)
    return out


# ---- hand-built graphs -----------------------------------------------------------------------------------------------
# A: goal 0 <- rule 1 <- (x 3, y 4), goal 0 <- rule 2 <- (x 3, z 5); x = 11, y = 10, z = 12
PA = ("grrggg", [(0, 1), (0, 2), (1, 3), (1, 4), (2, 3), (2, 5)], [1, 2, 3, 11, 10, 12])
# B: goal 0 <- rule 1 <- p 3, goal 0 <- rule 2 <- q 4; p = 10, q = 11
PB = ("grrgg", [(0, 1), (0, 2), (1, 3), (2, 4)], [1, 2, 3, 10, 11])


def test_hand_built_pair_of_runs(eng):
    corpus = relabel(build([PA[:2], PB[:2]]), [PA[2], PB[2]])
    ref = Ref(corpus)
    out = everywhere(eng, ref, [0, 1], [10, 11, 12], 3, 0, "pair of runs, q = all")
    for sinks in (False, True):
        assert out[sinks][0] == [(2, (10, 11))] and out[sinks][1] == [2], "exactly one row, the triple is a superset"
        assert out[sinks][2] == [3, 3, 0, 3, 3, 1, 3, 1, 0]
    out = everywhere(eng, ref, [0, 1], [10, 11, 12], 3, 1, "pair of runs, q = 1", loaded=True)
    for sinks in (False, True):
        assert out[sinks][0] == [(1, (11,)), (2, (10, 12))] and out[sinks][1] == [1, 1] and out[sinks][3]["K1"] == 2


@pytest.fixture(scope="module")
def hand():
    return relabel(build([h[:2] for h in HAND]), [h[2] for h in HAND])


def test_hand_built_labels(eng, hand):
    """a label on a goal and a rule, an inner goal and a sink of one label, 300 nodes of one label, two roots, the
    empty graph, the childless rule; an absent label and the roots' labels among the candidates"""
    ref = Ref(hand)
    cand = [10, 11, 12, 13, 777777, 20, 21, 22, 30, 31, 1, 6]
    out = everywhere(eng, ref, [0, 1, 2, 3, 4, 5], cand, 3, 0, "hand, the empty graph listed")
    assert out[False][0] == out[True][0] == [], "a graph without roots is never lost"
    assert out[False][2][3] < len(cand) and 777777 not in out[False][3]["live"]
    out = everywhere(eng, ref, [0, 1, 2, 3, 5], cand, 3, 0, "hand, without the empty graph", loaded=True)
    assert out[False][0], "the roots' labels together are a cut"
    assert out[False][2][3] < len(cand) and 777777 not in out[False][3]["live"]
    for q in (1, 2):
        out = everywhere(eng, ref, [0, 1, 2, 3, 4, 5, 2], cand, 3, q, f"hand, q = {q}", loaded=True)
        assert out[False][0] and out[True][0] and 777777 not in out[False][3]["live"]
        assert out[False][2][3] < len(cand)


# ---- chunk edges -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def trees():
    """build(): a node's label is its corpus-wide index, so a label names one node of one graph"""
    return build([fault_tree(s) for s in (137, 139, 151)] + [h[:2] for h in HAND[:2]])


@pytest.mark.parametrize("K", [1, 63, 64, 65, 129])
def test_chunk_edges_round_1(eng, trees, K):
    """K candidates: the roots' labels (cuts alone under q = 1), absent labels, the others' nodes"""
    ref = Ref(trees)
    roots = [int(trees.node_off[2 * r + 1]) for r in range(5)]
    rng = np.random.default_rng(K)
    pool = [int(x) for x in rng.permutation(len(trees.label))] + [10 ** 6 + k for k in range(40)]
    cand = list(dict.fromkeys(([roots[1]] if K == 1 else roots + [10 ** 6]) + pool))[:K]
    if K > 1:
        cand = [cand[int(x)] for x in rng.permutation(K)]
        cand.remove(roots[4]), cand.append(roots[4])  # a cut in the last bit of the last chunk
    out = everywhere(eng, ref, [0, 1, 2, 3, 4], cand, 1 if K == 129 else 2, 1, f"{K} candidates")
    assert out[False][2][0] == K and out[False][2][2] >= (5 if K > 1 else 1)
    assert K == 1 or out[False][3]["K1"] < K - 5, "absent labels leave the live list"


EDGE_LIVE = [(11, 2), (12, 2), (8, 3), (9, 3), (23, 3)]  # 55 and 66 pairs; 56 and 84 triples; 253 pairs and 1,771 triples


@pytest.fixture(scope="module")
def edges_corpus():
    return build([three_rules(n) for n, _ in EDGE_LIVE] + [PB[:2]])


@pytest.mark.parametrize("k", range(len(EDGE_LIVE)))
def test_chunk_edges_rounds_2_and_3(eng, edges_corpus, k):
    """every leaf of three_rules(n) is live; the root's label is a cut alone, an absent label hits nothing"""
    n, size = EDGE_LIVE[k]
    n0 = int(edges_corpus.node_off[2 * k + 1])
    cand = [n0 + 4 + i for i in range(n)]
    cand = cand[:3] + [n0] + cand[3:] + [10 ** 6]
    out = everywhere(eng, Ref(edges_corpus), [k, len(EDGE_LIVE)], cand, size, 1, f"{n} live, size {size}")
    for sinks in (False, True):
        rows, n_lost, stats, info = out[sinks]
        assert info["K1"] == n and stats[3] == n and stats[4] == comb(n, 2)
        assert stats[5] > 0 and (size < 3 or (stats[7] == comb(n, 3) and stats[8] > 0))
    # every round in play: round 1 finds the root (not under the flag), rounds 2 and 3 find cuts, and round 3 rejects
    # triples that hold a cut pair
    if size == 3:
        assert out[False][2][2] == 1 and out[False][3]["rejected"] > 0 and out[True][3]["rejected"] > 0


# ---- list shapes, a run listed twice, persistence -------------------------------------------------------------------
@pytest.fixture(scope="module")
def seventy():
    return random_corpus(2024, n_runs=70, max_nodes=40)[0]


@pytest.mark.parametrize("n", [1, 3, 70])
def test_list_shapes(eng, seventy, n):
    its = [int(x) for x in seventy.iteration][:n]
    if n == 3:
        its = [its[2], its[0], its[2]]  # a run listed twice: its count is doubled
    ref = Ref(seventy)
    g0 = ref.graph(2 * seventy.run_index(its[0]) + 1)
    seen = [g0.label[r] for r in g0.roots][:3]  # together a cut of the first listed run, if it has at most 3 roots
    seen += [lab for it in its for lab in ref.graph(2 * seventy.run_index(it) + 1).label]
    cand = [int(x) for x in list(dict.fromkeys(seen))[:30]] + [10 ** 6]
    eng.load(seventy)
    for q in sorted({0, 1, n // 2}):
        out = everywhere(eng, ref, its, cand, 3, q, f"{n} graphs, q = {q}", loaded=True, sample=3 if n == 70 else 1)
        if n == 3 and q == 1:
            assert out[False][1] and all(x in (1, 2, 3) for x in out[False][1])
        if q == 1 and n > 1:
            assert out[False][0], "some label set breaks some run"


def test_one_workgroup_walks_graphs_of_different_sizes(eng):
    """kl_grid 1: a hub, an empty graph, the 600-node level and the 301-level chain in turn, some of them again;
    nothing of the previous graph may stay (hit list, rule bits, level offsets)"""
    h, l, c = hub(), level(), chains()
    posts = [h[:2], ("", []), l[:2], c[:2], ("gr", [(0, 1)])]
    corpus = build(posts)
    rng = np.random.default_rng(8)
    corpus.label = np.ascontiguousarray(rng.integers(0, 25, len(corpus.label)), dtype=np.uint32)
    its = [0, 1, 2, 3, 4, 0, 3, 2]
    cand = list(range(25)) + [777777]
    ref = Ref(corpus)
    for q in (1, 3):
        everywhere(eng, ref, its, cand, 2, q, f"one workgroup, five graphs, q = {q}", grids=(1, 0, 3))


@pytest.mark.parametrize("k, name", [(0, "a hub of 300 children"), (1, "a level of 600 nodes"), (2, "301 levels")])
def test_sweep_edges(eng, k, name):
    shapes = [hub(), level(), chains()]
    corpus = build([s[:2] for s in shapes])  # labels: the corpus-wide node index
    n0 = int(corpus.node_off[2 * k + 1])
    cand = [n0 + v for v in shapes[k][2]]
    out = everywhere(eng, Ref(corpus), [k, (k + 1) % 3], cand, 2, 1, name, grids=(1, 0, 3))
    assert out[False][2][4] >= 130 and out[False][2][5] >= 1, "at least 130 pairs and a cut among them"


def lds_image_bytes(V, E, L):
    """knock::knock_lds_bytes (nemo_amd/csrc/knock_host.h)"""
    al = lambda b: (b + 15) & ~15
    return al(8 * V) + al(2 * (V + 1)) + al(2 * E) + al(2 * V) + al(2 * (L + 1)) + al(8 * ((V + 63) // 64))


def test_hit_list_straddles_lds_and_region(eng):
    """An LDS-tier graph whose image nearly fills the tier (76 KB of 80 KB) and all of whose 5,400 leaves carry
    candidate labels: the k1 + 1 offsets and the first rows stay in the LDS tail, the other rows go to the
    workgroup's region, and a chunk's seeds are read from both.  goal 0 <- rule 1 <- 2,700 leaves of labels 0..19,
    goal 0 <- rule 2 <- 2,700 leaves of labels 20..39: a pair is a cut iff it takes a label of either half."""
    N = 2700
    kinds = "grr" + "g" * (2 * N)
    edges = [(0, 1), (0, 2)] + [(1, 3 + k) for k in range(N)] + [(2, 3 + N + k) for k in range(N)]
    labels = [900001, 900002, 900003] + [k % 20 for k in range(N)] + [20 + k % 20 for k in range(N)]
    corpus = relabel(build([(kinds, edges), PB[:2]]), [labels, PB[2]])
    cand = list(range(40))
    image = lds_image_bytes(len(kinds), len(edges), 3)
    # at most half of a CU's 160 KB of LDS per workgroup while two stay resident: the list does not fit behind the image
    assert image <= 81920 and 4 * (len(cand) + 1 + 2 * N) > 160 * 1024 // 2 - image > 4 * (len(cand) + 1)
    out = everywhere(eng, Ref(corpus), [0, 1, 0], cand, 3, 1, "a hit list in LDS and in the region", sample=97)
    for sinks in (False, True):
        rows, n_lost, stats, info = out[sinks]
        pairs = [r for r in rows if r[0] == 2]
        assert len([1 for _, (a, b) in pairs if a < 20 <= b]) >= 19 * 19 and stats[5] == len(pairs) and info["rejected"] > 0


# ---- device against device ----------------------------------------------------------------------------------------------
def test_against_min_cuts(eng):
    """n = 1, label = corpus-wide node index, candidates = the sink goals' labels in node order: nemo_min_cuts' rows
    mapped node -> label, and its stats"""
    corpus = build([fault_tree(s) for s in (137, 139, 151)])
    eng.load(corpus)
    try:
        for k in range(3):
            gr = Graph(corpus, 2 * k + 1)
            n0 = int(corpus.node_off[2 * k + 1])
            cuts = eng.min_cuts(k, 1, None, 3)
            stats = eng.min_cut_stats().reshape(-1).tolist()
            want = [(int(r["size"]), tuple(n0 + int(x) for x in r["node"][:int(r["size"])])) for r in cuts]
            assert want and stats[0] == len(gr.leaves)
            for lds in (-1, 0):
                for grid in GRIDS:
                    eng.set_option("knock_lds_max", lds)
                    eng.set_option("kl_grid", grid)
                    for sinks in (False, True):
                        rows, n_lost = eng.min_label_cuts([k], 1, [n0 + v for v in gr.leaves], 3, 0, sinks_only=sinks)
                        assert got_rows(rows) == want and n_lost.tolist() == [1] * len(want)
                        assert eng.min_label_cut_stats().reshape(-1).tolist() == stats
    finally:
        eng.set_option("knock_lds_max", -1)
        eng.set_option("kl_grid", 0)


def test_against_knockout_labels(eng, seventy):
    """every returned row is lost on n_lost >= q list positions under nemo_knockout_labels, every proper subset of
    it on fewer than q"""
    corpus = seventy
    its = [int(x) for x in corpus.iteration][:12] + [int(corpus.iteration[1])]
    ref = Ref(corpus)
    graphs = [ref.graph(2 * corpus.run_index(it) + 1) for it in its]
    cand = [int(g.label[r]) for g in graphs[:3] for r in g.roots] + [int(x) for g in graphs for x in g.label]
    cand = list(dict.fromkeys(cand))[:36]
    eng.load(corpus)
    total = 0
    try:
        for lds in (-1, 0):
            for grid in GRIDS:
                eng.set_option("knock_lds_max", lds)
                eng.set_option("kl_grid", grid)
                for q in (0, 2, 1):
                    for sinks in (False, True):
                        rows, n_lost = eng.min_label_cuts(its, 1, cand, 3, q, sinks_only=sinks)
                        sets = [list(r[1]) for r in got_rows(rows)]
                        subs = [list(x) for s in sets for k in range(1, len(s)) for x in itertools.combinations(s, k)]
                        eng.knockout_labels(its, 1, sets + subs, sinks_only=sinks)
                        counts = eng.knockout_label_counts()[0].tolist()
                        assert counts[:len(sets)] == n_lost.tolist() and all(x >= (q or len(its)) for x in counts[:len(sets)])
                        assert all(x < (q or len(its)) for x in counts[len(sets):])
                        total += len(sets)
    finally:
        eng.set_option("knock_lds_max", -1)
        eng.set_option("kl_grid", 0)
    assert total > 0


# ---- seeded synthetic corpora ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_synthetic_corpora(eng, seed):
    corpus, _ = synth.generate(5, target_nodes=400, p_fault=0.5, prepend_run0=True, seed=seed)
    its = [int(x) for x in corpus.iteration]
    ref = Ref(corpus)
    g0 = ref.graph(2 * corpus.run_index(its[0]) + 1)
    cand = [int(x) for x in list(dict.fromkeys(g0.label[v] for v in g0.leaves))[:40]]
    t0 = time.perf_counter()
    want = reference(ref, its, 1, cand, 3, 2, True, sample=3)
    assert time.perf_counter() - t0 < 10, "the reference's pair and triple enumeration at K <= 40"
    assert want[2][0] == len(cand)
    eng.load(corpus)
    for q in (0, 2):
        everywhere(eng, ref, its, cand, 3, q, f"synth seed {seed}, q = {q}", loaded=True, sample=3)


# ---- a post graph of >= 65536 nodes: u32 rows, the global tier by size ------------------------------------------------------
def test_graph_past_65535_nodes(eng):
    corpus, _ = synth.generate(3, target_nodes=140000, p_fault=0.9, prepend_run0=True, seed=3, eot=80, body_extra=6,
                               nval=3, nloc=4)
    r = max(range(corpus.n_runs), key=lambda x: corpus.graph_size(2 * x + 1))
    n0 = int(corpus.node_off[2 * r + 1])
    lab = corpus.label.copy()  # the graph's many roots share two labels of their own, so that two events are a cut
    for k, v in enumerate(Graph(corpus, 2 * r + 1).roots):
        lab[n0 + v] = 5000000 + k % 2
    corpus.label = np.ascontiguousarray(lab, dtype=np.uint32)
    ref = Ref(corpus)
    gr = ref.graph(2 * r + 1)
    assert gr.V >= 65536 and len(gr.roots) >= 2
    rng = np.random.default_rng(5)
    leaf_labels = sorted({gr.label[v] for v in gr.leaves})
    roots = list(dict.fromkeys(int(gr.label[v]) for v in gr.roots))
    assert roots == [5000000, 5000001]
    cand = list(dict.fromkeys(roots + [int(x) for x in rng.choice(leaf_labels, 12, replace=False)]))[:12]
    it = int(corpus.iteration[r])
    eng.load(corpus)
    try:
        for sinks in (False, True):
            want = reference(ref, [it], 1, cand, 2, 0, sinks, sample=5, numpy_form=True)
            assert sinks or (2, (5000000, 5000001)) in want[0], "the roots' labels are a cut"
            for lds in (-1, 0):  # the graph is past the LDS tier by its size under either
                for grid in GRIDS:
                    eng.set_option("knock_lds_max", lds)
                    eng.set_option("kl_grid", grid)
                    compare(eng, [it], 1, cand, 2, 0, sinks, want, f"66k nodes, sinks {sinks}, knock_lds_max {lds}, kl_grid {grid}")
    finally:
        eng.set_option("knock_lds_max", -1)
        eng.set_option("kl_grid", 0)


# ---- protocol ----------------------------------------------------------------------------------------------------------------
def raw(eng, iters, cond, cand, n_cand, max_size=2, min_runs=0, flags=0):
    it = np.ascontiguousarray(iters, dtype=np.uint32)
    cand = np.ascontiguousarray(cand, dtype=np.uint32)
    return eng.L.nemo_min_label_cuts(eng.h, it.ctypes.data if len(it) else None, len(it), cond,
                                     cand.ctypes.data if len(cand) else None, n_cand, max_size, min_runs, flags)


def fetch_state(eng):
    return eng.L.nemo_fetch_min_label_cuts(eng.h, None, None, 0, None)


def test_protocol(eng, hand, trees):
    eng.load(hand)
    err = lambda: eng.L.nemo_last_error(eng.h).decode()
    assert fetch_state(eng) == 5  # a fetch before any call
    assert eng.L.nemo_fetch_min_label_cut_stats(eng.h, np.zeros(9, np.uint64).ctypes.data) == 5
    for bad in (0, 4, 0xFFFFFFFF):
        assert raw(eng, [0], 1, [10, 11], 2, max_size=bad) == 1 and "max_size" in err()
    assert raw(eng, [0], 1, [10, 11, 12, 11], 4) == 1 and "candidate 3 names label 11 a second time" in err()
    assert raw(eng, [0], 1, [10, 0xFFFFFFFF, 10], 3) == 1 and "candidate 1" in err() and "UINT32_MAX" in err()
    assert raw(eng, [0], 1, [], 2) == 1 and "no implicit" in err()  # cand_labels == NULL with n_cand > 0
    assert raw(eng, [0, 1], 1, [10], 1, min_runs=3) == 1 and "min_runs 3" in err()
    assert raw(eng, [0], 1, [10], 1, flags=2) == 1 and "flags" in err()
    assert raw(eng, [0], 2, [10], 1) == 1 and "cond" in err()
    assert raw(eng, [0, 4242], 1, [10], 1) == 7  # an iteration that is not loaded
    # n * chunks > 2^28 words, from the sizes alone: 2^22 + 1 list positions (run 0, over and over) x 64 chunks
    assert raw(eng, np.zeros((1 << 22) + 1, np.uint32), 1, np.arange(64 * 64, dtype=np.uint32), 64 * 64) == 6
    assert "2^28 words" in err() and "shorten the candidate list or the run list" in err()
    assert fetch_state(eng) == 5  # the failed calls left no result
    eng.min_label_cuts([0], 1, [10], 1)
    assert fetch_state(eng) == 0
    assert eng.L.nemo_min_label_cuts(eng.h, None, 2, 1, None, 0, 2, 0, 0) == 1 and "no run list" in err()
    assert fetch_state(eng) == 5  # ... and neither does a call without a run list
    # zero rows
    rows, n_lost = eng.min_label_cuts([], 1, [10, 11], 3)
    assert len(rows) == 0 and len(n_lost) == 0 and not eng.min_label_cut_stats().any()
    rows, n_lost = eng.min_label_cuts([0, 1], 1, [], 3)
    assert len(rows) == 0 and not eng.min_label_cut_stats().any()
    # a too-small cap, and the query
    ref = Ref(hand)
    cand = [10, 11, 12, 13, 20, 21, 22, 1, 6]
    want = reference(ref, [0, 1, 3], 1, cand, 3, 1, False)
    compare(eng, [0, 1, 3], 1, cand, 3, 1, False, want, "after the errors")
    assert len(want[0]) >= 2
    n = ctypes.c_uint64()
    out = np.zeros(len(want[0]), E.LABEL_CUT_DTYPE)
    assert eng.L.nemo_fetch_min_label_cuts(eng.h, None, None, 0, ctypes.byref(n)) == 0 and n.value == len(want[0])
    assert eng.L.nemo_fetch_min_label_cuts(eng.h, out.ctypes.data, None, len(out) - 1, ctypes.byref(n)) == 1
    assert eng.L.nemo_fetch_min_label_cuts(eng.h, out.ctypes.data, None, len(out), None) == 0 and got_rows(out) == want[0]
    # a node in the pre graph (cond 0): every pre graph is one goal of its own label
    rows, n_lost = eng.min_label_cuts([0, 3], 0, [900000, 5, 900003], 2, 0)
    assert got_rows(rows) == [(2, (900000, 900003))] and n_lost.tolist() == [2]
    # more than 2^32 - 2 hypotheses in round 3: 2,955 live candidates have 4,296,157,285 triples; K1 is known after round 1
    big = build([level_of(3000)])
    eng.load(big)
    with pytest.raises(E.NemoError) as ei:
        eng.min_label_cuts([0], 1, [int(big.node_off[1]) + 4 + k for k in range(2955)], 3)
    assert ei.value.code == 6 and "2^32 - 2 hypotheses" in ei.value.msg and "shorten the candidate list or the run list" in ei.value.msg
    assert fetch_state(eng) == 5  # and leaves no results
    eng.load(hand)
    compare(eng, [0, 1, 3], 1, cand, 3, 1, False, want, "after the limit")
    eng.load(trees)  # a reload: no result of the previous corpus survives
    assert fetch_state(eng) == 5
    assert eng.L.nemo_fetch_min_label_cut_stats(eng.h, np.zeros(9, np.uint64).ctypes.data) == 5


def test_node_context_refuses(hand):
    node = E.Engine(devices=[0])
    try:
        node.load(hand)
        with pytest.raises(E.NemoError) as ei:
            node.min_label_cuts([0], 1, [10], 2)
        assert ei.value.code == 5 and "single-device contexts only" in ei.value.msg
    finally:
        node.close()


def test_buffers_grow_and_are_reused(eng, seventy):
    its = [int(x) for x in seventy.iteration]
    ref = Ref(seventy)
    labs = [int(x) for x in dict.fromkeys(seventy.label.tolist())]
    eng.load(seventy)
    for n, K in ((3, 10), (70, 25), (1, 3), (130, 12), (70, 25)):
        lst = [its[k % len(its)] for k in range(n)]
        want = reference(ref, lst, 1, labs[:K], 2, max(1, n // 4), False, sample=3)
        compare(eng, lst, 1, labs[:K], 2, max(1, n // 4), False, want, f"{n} list positions, {K} candidates")


def test_other_results_are_left_alone(eng):
    corpus = random_corpus(1000, n_runs=6, max_nodes=40)[0]
    its = [int(x) for x in corpus.iteration]
    f = corpus.failed_iters() or its[1:3]
    labs = [int(x) for x in dict.fromkeys(corpus.label.tolist())][:20]
    eng.load(corpus)
    eng.mark()

    def others():
        return (np.array(eng.diff_masks(len(f))).copy(), eng.missing().copy(), [m.copy() for m in eng.sdiff_masks()],
                eng.surplus().copy(), eng.label_distances().copy(), eng.knockout_rows().copy(), eng.min_cut_rows().copy(),
                eng.knockout_label_counts()[0].copy())

    def same(a, b):
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[3], b[3])
        assert len(a[2]) == len(b[2]) and all(np.array_equal(x, y) for x, y in zip(a[2], b[2]))
        assert all(np.array_equal(a[k], b[k]) for k in (4, 5, 6, 7))

    eng.diffprov(f, 1)
    eng.diffprov_symmetric(f)
    eng.nearest_runs(its, its)
    eng.knockout_leaves(its, 1)
    eng.min_cuts(its[0], 1, None, 2)
    eng.knockout_labels(its, 1, [[x] for x in labs])
    before = others()
    ref = Ref(corpus)
    want = reference(ref, its, 1, labs, 3, 1, False)
    compare(eng, its, 1, labs, 3, 1, False, want, "between the other calls")
    same(before, others())  # their fetches, unchanged by the label-cut call between them
    eng.diffprov(f, 1)
    eng.diffprov_symmetric(f)
    eng.nearest_runs(its, its)
    eng.knockout_leaves(its, 1)
    eng.min_cuts(its[0], 1, None, 2)
    eng.knockout_labels(its, 1, [[x] for x in labs])
    rows, n_lost = eng.min_label_cut_rows()  # and the reverse
    assert got_rows(rows) == want[0] and n_lost.tolist() == want[1]
    assert eng.min_label_cut_stats().reshape(-1).tolist() == want[2]
