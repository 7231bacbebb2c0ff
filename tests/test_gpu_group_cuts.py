"""GPU checks of nemo_min_group_cuts (k_gc_table, k_gc_rows, k_gc_lds and k_gc_glob in nemo_amd/csrc/k_gcuts.hip, with
k_lcuts.hip's reduction and support kernels and k_cuts.hip's row kernels): every row, every n_lost and the nine stats,
exact.

Reference.  There is no reference code for the call (include/nemohip.h fixes the semantics), so the reference is the
definition in plain Python and never calls the library.  It enumerates every subset of size <= max_size of the
candidate positions, takes the union of the subset's groups as a label set and gives it to Ref.words of
tests/test_gpu_knockout_labels.py, which computes lost and hit per (graph, set) in two forms that must agree first
(on every set, or on every third or fifth set where the graphs are large, on every 97th in the straddle case).  It
then counts list positions, applies q, keeps the subsets none of whose proper subsets is a cut, and orders them by
(size, colex rank over the live list); the live list is the definition's: the candidates that are no cut alone and
whose group hits a node of some listed graph.

Every case runs on both tiers (knock_lds_max default and 0), with and without NEMO_KL_SINKS, and under kl_grid 0, 1
and 3.  Two further checks are device against device: nemo_min_label_cuts on singleton groups, and
nemo_knockout_labels on the unions of the returned rows and of their proper subsets.
"""
import ctypes
import itertools
import json
import os
import sys
from math import comb

import numpy as np
import pytest

from nemo_amd import engine as E
from nemo_amd.corpus import load_molly
from nemo_amd.faults import fault_events
from tests.small import random_corpus
from tests.test_gpu_knockout import Graph, build
from tests.test_gpu_knockout_labels import HAND, Ref, relabel
from tests.test_gpu_label_cuts import EDGE_LIVE, PA, PB, colex, lds_image_bytes
from tests.test_gpu_min_cuts import chains, fault_tree, hub, level, level_of, three_rules
from tools import synth

pytestmark = pytest.mark.gpu
sys.setrecursionlimit(max(sys.getrecursionlimit(), 20000))
GRIDS = (0, 1, 3)
NONE = 0xFFFFFFFF
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def eng():
    e = E.Engine(0)
    yield e
    e.close()


# ---- the reference ----------------------------------------------------------------------------------------------
def union(groups, c):
    """the label set candidates c remove: each label once"""
    return list(dict.fromkeys(int(x) for p in c for x in groups[p]))


def reference(ref, iters, cond, groups, max_size, min_runs, sinks, sample=1, numpy_form=False):
    """(rows [(size, candidate positions)], n_lost, stats [9], info) by the definition"""
    n, K = len(iters), len(groups)
    stats = [0] * 9
    if not n or not K:
        return [], [], stats, {"K1": 0, "rejected": 0, "live": []}
    q = min_runs or n
    subsets = [c for s in range(1, max_size + 1) for c in itertools.combinations(range(K), s)]
    sets = [union(groups, c) for c in subsets]
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
    rows = [(size, tuple(c)) for size, _, c in found]
    n_lost = [cnt[c] for _, _, c in found]
    K1 = len(live)
    for s in range(1, max_size + 1):
        stats[3 * (s - 1):3 * s] = [K if s == 1 else K1, comb(K if s == 1 else K1, s), sum(1 for r in rows if r[0] == s)]
    return rows, n_lost, stats, {"K1": K1, "rejected": rejected, "live": live}


def got_rows(rows):
    return [(int(r["size"]), tuple(int(x) for x in r["group"][:int(r["size"])])) for r in rows]


def compare(eng, iters, cond, groups, max_size, min_runs, sinks, want, what):
    rows, n_lost = eng.min_group_cuts(iters, cond, groups, max_size, min_runs, sinks_only=sinks)
    assert rows.dtype == E.GROUP_CUT_DTYPE and n_lost.dtype == np.uint32 and len(rows) == len(n_lost), what
    for r in rows:
        assert all(int(x) == NONE for x in r["group"][int(r["size"]):]), f"{what}: unused entries"
    assert got_rows(rows) == want[0], f"{what}: rows"
    assert n_lost.tolist() == want[1], f"{what}: n_lost"
    assert eng.min_group_cut_stats().reshape(-1).tolist() == want[2], f"{what}: stats"
    return rows, n_lost


def everywhere(eng, ref, iters, groups, max_size, min_runs, what, cond=1, sample=1, numpy_form=False, grids=GRIDS, loaded=False,
               flags=(False, True)):
    """the case with and without NEMO_KL_SINKS, on both tiers and under every kl_grid; the reference once per flag"""
    if not loaded:
        eng.load(ref.corpus)
    out = {}
    try:
        for sinks in flags:
            want = reference(ref, iters, cond, groups, max_size, min_runs, sinks, sample, numpy_form)
            for lds in (-1, 0):
                for grid in grids:
                    eng.set_option("knock_lds_max", lds)
                    eng.set_option("kl_grid", grid)
                    compare(eng, iters, cond, groups, max_size, min_runs, sinks, want,
                            f"{what}, sinks {sinks}, knock_lds_max {lds}, kl_grid {grid}")
            out[sinks] = want
    finally:
        eng.set_option("knock_lds_max", -1)
        eng.set_option("kl_grid", 0)
    return out


# ---- hand-built graphs -----------------------------------------------------------------------------------------------
def test_hand_built_pair_of_runs(eng):
    """PA: goal <- rule <- (x 11, y 10), goal <- rule <- (x 11, z 12); PB: goal <- rule <- p 10, goal <- rule <- q 11.
    Lost on A: {11} or {10, 12}; lost on B: {10, 11}."""
    corpus = relabel(build([PA[:2], PB[:2]]), [PA[2], PB[2]])
    ref = Ref(corpus)
    #          0     1     2     3         4             5   6         7
    groups = [[10], [11], [12], [10, 12], [10, 11, 12], [], [777777], [11]]
    out = everywhere(eng, ref, [0, 1], groups, 3, 0, "pair of runs, q = all")
    for sinks in (False, True):
        rows, n_lost, stats, info = out[sinks]
        # alone only {10, 11, 12} breaks both; live: 0, 1, 2, 3, 7 (the empty group and the absent label hit nothing).
        # Pairs that remove 10 and 11: (0, 1), (0, 7), (1, 3), (3, 7); no triple without one of them is a cut.
        assert rows == [(1, (4,)), (2, (0, 1)), (2, (1, 3)), (2, (0, 7)), (2, (3, 7))] and n_lost == [2] * 5
        assert info["live"] == [0, 1, 2, 3, 7] and stats == [8, 8, 1, 5, 10, 4, 5, 10, 0]
    out = everywhere(eng, ref, [0, 1], groups, 3, 1, "pair of runs, q = 1", loaded=True)
    for sinks in (False, True):
        rows, n_lost, stats, info = out[sinks]
        # q = 1: {11} alone breaks A, and so does each candidate that holds 11 or both 10 and 12: both {11} candidates
        # are rows.  Live: 0 and 2; their pair {10, 12} breaks A.  No pair of nested groups is a row.
        assert rows == [(1, (1,)), (1, (3,)), (1, (4,)), (1, (7,)), (2, (0, 2))] and n_lost == [1, 1, 2, 1, 1]
        assert info["live"] == [0, 2]
        nested = lambda a, b: set(groups[a]) <= set(groups[b]) or set(groups[b]) <= set(groups[a])
        assert not any(size == 2 and nested(*c) for size, c in rows)


@pytest.fixture(scope="module")
def hand():
    return relabel(build([h[:2] for h in HAND]), [h[2] for h in HAND])


def test_group_shapes_on_the_hand_graphs(eng, hand):
    """a label on a goal and a rule; the 300 nodes of one label inside a group of 40 labels; a label named twice in a
    group; a group of 600 labels of which 3 occur; the empty graph listed and not listed"""
    ref = Ref(hand)
    labs = [10, 11, 12, 13, 20, 21, 22, 30, 31, 1, 6]
    present = sorted({int(x) for x in hand.label.tolist() if int(x) != NONE})
    counts = {x: hand.label.tolist().count(x) for x in present}
    many = max(present, key=lambda x: counts[x])
    assert counts[many] >= 300, "HAND's 300 nodes of one label"
    groups = [[x] for x in labs]
    groups.append([many] + [2000000 + k for k in range(39)])                      # 40 labels, one of them on 300 nodes
    groups.append([10, 12, 10, 10, 12])                                           # named twice: counts once
    groups.append([3000000 + k for k in range(597)] + [20, 30, 1])                # 600 labels, 3 occur
    groups.append([])
    groups.append([777777])
    out = everywhere(eng, ref, [0, 1, 2, 3, 4, 5], groups, 2, 0, "hand, the empty graph listed")
    assert out[False][0] == out[True][0] == [], "a graph without roots is never lost"
    out = everywhere(eng, ref, [0, 1, 2, 3, 5], groups, 2, 0, "hand, without the empty graph", loaded=True)
    for q in (1, 2):
        out = everywhere(eng, ref, [0, 1, 2, 3, 4, 5, 2], groups, 3 if q == 1 else 2, q, f"hand, q = {q}", loaded=True)
        assert out[False][0] and out[True][0]
        live = out[False][3]["live"]
        assert len(groups) - 2 not in live and len(groups) - 1 not in live, "the empty group and the absent label are never live"


# ---- chunk edges -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def trees():
    """build(): a node's label is its corpus-wide index, so a label names one node of one graph"""
    return build([fault_tree(s) for s in (137, 139, 151)] + [h[:2] for h in HAND[:2]])


@pytest.mark.parametrize("K", [1, 63, 64, 65, 129])
def test_chunk_edges_round_1(eng, trees, K):
    """K groups of 1 to 3 labels: a root's label in one (a cut alone under q = 1), absent labels, the others' nodes;
    a cut sits in the last bit of the last chunk"""
    ref = Ref(trees)
    roots = [int(trees.node_off[2 * r + 1]) for r in range(5)]
    rng = np.random.default_rng(K)
    pool = [int(x) for x in rng.permutation(len(trees.label)) if int(x) not in roots] + [10 ** 6 + k for k in range(40)]
    groups = [[pool[(3 * k + j) % len(pool)] for j in range(1 + k % 3)] for k in range(K)]
    for k, r in enumerate(roots[:min(4, K - 1)]):
        groups[(7 * k) % (K - 1)].append(r)
    groups[K - 1] = [10 ** 6 + 1, roots[1 if K == 1 else 4]]  # the last bit of the last chunk
    out = everywhere(eng, ref, [0, 1, 2, 3, 4], groups, 1 if K == 129 else 2, 1, f"{K} groups")
    rows, n_lost, stats, info = out[False]
    assert stats[0] == K and (1, (K - 1,)) in rows and stats[2] >= (5 if K > 1 else 1)


@pytest.fixture(scope="module")
def edges_corpus():
    return build([three_rules(n) for n, _ in EDGE_LIVE] + [PB[:2]])


@pytest.mark.parametrize("k", range(len(EDGE_LIVE)))
def test_chunk_edges_rounds_2_and_3(eng, edges_corpus, k):
    """every leaf of three_rules(n) is a live group of its own; one group holds the root and one an absent label"""
    n, size = EDGE_LIVE[k]
    n0 = int(edges_corpus.node_off[2 * k + 1])
    groups = [[n0 + 4 + i] for i in range(n)]
    groups = groups[:3] + [[n0]] + groups[3:] + [[10 ** 6]]
    out = everywhere(eng, Ref(edges_corpus), [k, len(EDGE_LIVE)], groups, size, 1, f"{n} live, size {size}")
    for sinks in (False, True):
        rows, n_lost, stats, info = out[sinks]
        assert info["K1"] == n and stats[3] == n and stats[4] == comb(n, 2)
        assert stats[5] > 0 and (size < 3 or (stats[7] == comb(n, 3) and stats[8] > 0))
    if size == 3:
        assert out[False][2][2] == 1 and out[False][3]["rejected"] > 0 and out[True][3]["rejected"] > 0


# ---- list shapes, a run listed twice ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def seventy():
    return random_corpus(2024, n_runs=70, max_nodes=40)[0]


def random_unions(labels, n_groups, seed):
    rng = np.random.default_rng(seed)
    return [[int(x) for x in rng.choice(labels, int(rng.integers(1, 7)), replace=False)] for _ in range(n_groups)]


@pytest.mark.parametrize("n", [1, 3, 70])
def test_list_shapes(eng, seventy, n):
    """groups: random unions of 1 to 6 of the first 30 labels seen"""
    its = [int(x) for x in seventy.iteration][:n]
    if n == 3:
        its = [its[2], its[0], its[2]]  # a run listed twice: its count is doubled
    ref = Ref(seventy)
    seen = [lab for it in its for lab in ref.graph(2 * seventy.run_index(it) + 1).label]
    labels = [int(x) for x in list(dict.fromkeys(seen))[:30]]
    groups = random_unions(labels, 24, n) + [[10 ** 6]]
    eng.load(seventy)
    for q in sorted({0, 1, n // 2}):
        out = everywhere(eng, ref, its, groups, 2, q, f"{n} graphs, q = {q}", loaded=True, sample=3 if n == 70 else 1)
        if n == 3 and q == 1:
            assert out[False][1] and all(x in (1, 2, 3) for x in out[False][1])
        if q == 1 and n > 1:
            assert out[False][0], "some group set breaks some run"


def test_one_workgroup_walks_graphs_of_different_sizes(eng):
    """kl_grid 1: a hub, an empty graph, the 600-node level and the 301-level chain in turn, some of them again;
    nothing of the previous graph may stay (hit list, rule bits, level offsets)"""
    h, l, c = hub(), level(), chains()
    posts = [h[:2], ("", []), l[:2], c[:2], ("gr", [(0, 1)])]
    corpus = build(posts)
    rng = np.random.default_rng(8)
    corpus.label = np.ascontiguousarray(rng.integers(0, 25, len(corpus.label)), dtype=np.uint32)
    its = [0, 1, 2, 3, 4, 0, 3, 2]
    groups = [[x] for x in range(8)] + random_unions(list(range(25)), 10, 3) + [[777777], []]
    ref = Ref(corpus)
    for q in (1, 3):
        everywhere(eng, ref, its, groups, 2, q, f"one workgroup, five graphs, q = {q}", grids=(1, 0, 3))


def test_hit_list_straddles_lds_and_region(eng):
    """The 5,403-node graph of tests/test_gpu_label_cuts.py's straddle case: an LDS-tier graph whose image nearly
    fills the tier and all of whose 5,400 leaves carry named labels, 135 per label: the D + 1 offsets and the first
    rows stay in the LDS tail, the other rows go to the workgroup's region; every row is past KO_HUB nodes, so a
    whole wave folds it.  goal 0 <- rule 1 <- 2,700 leaves of labels 0..19, goal 0 <- rule 2 <- 2,700 leaves of labels
    20..39: a set is a cut of it iff it takes a label of either half.  Groups of 5 labels."""
    N = 2700
    kinds = "grr" + "g" * (2 * N)
    edges = [(0, 1), (0, 2)] + [(1, 3 + k) for k in range(N)] + [(2, 3 + N + k) for k in range(N)]
    labels = [900001, 900002, 900003] + [k % 20 for k in range(N)] + [20 + k % 20 for k in range(N)]
    corpus = relabel(build([(kinds, edges), PB[:2]]), [labels, PB[2]])
    groups = [list(range(5 * k, 5 * k + 5)) for k in range(8)] + [[0, 7, 19, 33, 900009], [3, 4, 21, 22, 23]]
    image = lds_image_bytes(len(kinds), len(edges), 3)
    assert image <= 81920 and 4 * (40 + 1 + 2 * N) > 160 * 1024 // 2 - image > 4 * (40 + 1)
    out = everywhere(eng, Ref(corpus), [0, 1, 0], groups, 2, 1, "a hit list in LDS and in the region", sample=97)
    for sinks in (False, True):
        rows, n_lost, stats, info = out[sinks]
        # the last two groups take a label of either half: cuts alone; the others are live unless they break the small
        # graph alone, and every live pair across the halves is a cut
        assert (1, (8,)) in rows and (1, (9,)) in rows and stats[5] == len([r for r in rows if r[0] == 2]) > 0
        first, second = [p for p in info["live"] if p < 4], [p for p in info["live"] if 4 <= p < 8]
        assert first and second and all((2, (a, b)) in rows for a in first for b in second)


# ---- device against device ----------------------------------------------------------------------------------------------
def test_against_min_label_cuts(eng, seventy):
    """singleton groups: the rows (position mapped to label), n_lost and stats of nemo_min_label_cuts"""
    corpus = seventy
    its = [int(x) for x in corpus.iteration][:12] + [int(corpus.iteration[1])]
    ref = Ref(corpus)
    graphs = [ref.graph(2 * corpus.run_index(it) + 1) for it in its]
    cand = [int(g.label[r]) for g in graphs[:3] for r in g.roots] + [int(x) for g in graphs for x in g.label]
    cand = list(dict.fromkeys(cand))[:36] + [10 ** 6]
    eng.load(corpus)
    total = 0
    try:
        for lds in (-1, 0):
            for grid in GRIDS:
                eng.set_option("knock_lds_max", lds)
                eng.set_option("kl_grid", grid)
                for q in (0, 2, 1):
                    for sinks in (False, True):
                        lrows, l_lost = eng.min_label_cuts(its, 1, cand, 3, q, sinks_only=sinks)
                        want = [(int(r["size"]), tuple(int(x) for x in r["label"][:int(r["size"])])) for r in lrows]
                        rows, n_lost = eng.min_group_cuts(its, 1, [[x] for x in cand], 3, q, sinks_only=sinks)
                        assert [(s, tuple(cand[p] for p in c)) for s, c in got_rows(rows)] == want
                        assert n_lost.tolist() == l_lost.tolist()
                        assert np.array_equal(eng.min_group_cut_stats(), eng.min_label_cut_stats())
                        total += len(want)
    finally:
        eng.set_option("knock_lds_max", -1)
        eng.set_option("kl_grid", 0)
    assert total > 0


def test_against_knockout_labels(eng, seventy):
    """every returned row, as the union of its groups, is lost on n_lost >= q list positions under
    nemo_knockout_labels, every proper subset of it on fewer than q"""
    corpus = seventy
    its = [int(x) for x in corpus.iteration][:12] + [int(corpus.iteration[1])]
    ref = Ref(corpus)
    seen = [lab for it in its for lab in ref.graph(2 * corpus.run_index(it) + 1).label]
    groups = random_unions([int(x) for x in list(dict.fromkeys(seen))[:30]], 30, 11)
    eng.load(corpus)
    total = 0
    try:
        for lds in (-1, 0):
            for grid in GRIDS:
                eng.set_option("knock_lds_max", lds)
                eng.set_option("kl_grid", grid)
                for q in (0, 2, 1):
                    for sinks in (False, True):
                        rows, n_lost = eng.min_group_cuts(its, 1, groups, 3, q, sinks_only=sinks)
                        cs = [c for _, c in got_rows(rows)]
                        subs = [x for c in cs for k in range(1, len(c)) for x in itertools.combinations(c, k)]
                        eng.knockout_labels(its, 1, [union(groups, c) for c in cs + subs], sinks_only=sinks)
                        counts = eng.knockout_label_counts()[0].tolist()
                        assert counts[:len(cs)] == n_lost.tolist() and all(x >= (q or len(its)) for x in counts[:len(cs)])
                        assert all(x < (q or len(its)) for x in counts[len(cs):])
                        total += len(cs)
    finally:
        eng.set_option("knock_lds_max", -1)
        eng.set_option("kl_grid", 0)
    assert total > 0


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
    picks = [int(x) for x in rng.choice(leaf_labels, 30, replace=False)]
    groups = [[5000000, picks[0]], [picks[1], 5000001]] + [picks[3 * k:3 * k + 3] for k in range(10)]  # 12 groups
    it = int(corpus.iteration[r])
    eng.load(corpus)
    try:
        for sinks in (False, True):
            want = reference(ref, [it], 1, groups, 2, 0, sinks, sample=5, numpy_form=True)
            assert sinks or (2, (0, 1)) in want[0], "the roots' labels are a cut"
            for lds in (-1, 0):  # the graph is past the LDS tier by its size under either
                for grid in GRIDS:
                    eng.set_option("knock_lds_max", lds)
                    eng.set_option("kl_grid", grid)
                    compare(eng, [it], 1, groups, 2, 0, sinks, want, f"66k nodes, sinks {sinks}, knock_lds_max {lds}, kl_grid {grid}")
    finally:
        eng.set_option("knock_lds_max", -1)
        eng.set_option("kl_grid", 0)


# ---- a case-study fixture, end to end through fault_events ----------------------------------------------------------------------
def test_case_study_fault_events(eng):
    """pb_asynchronous (5 good runs, 10 failed): the events of its clock labels by nemo_amd.faults.fault_events with
    the fixture's eot / eff, the good runs' post graphs listed, max_size 2, on every good run and on at least one.
    All 28 events are used: the reference alone takes well under a second at this K (measured on the CPU before
    this test was written)."""
    d = os.path.join(GOLDEN, "cs_pb_asynchronous")
    corpus = load_molly(d)
    runs = json.load(open(os.path.join(d, "runs.json")))
    spec = runs[0]["failureSpec"]
    good = [int(r["iteration"]) for r in runs if r["status"] == "success"]
    assert good and corpus.failed_iters()
    events, groups = fault_events(corpus.labels, spec["eot"], spec["eff"])
    assert any(e[0] == "omit" for e in events) and any(e[0] == "crash" and len(g) > 3 for e, g in zip(events, groups))
    ref = Ref(corpus)
    want = reference(ref, good, 1, groups, 2, 1, False)
    eng.load(corpus)
    everywhere(eng, ref, good, groups, 2, 0, "pb_asynchronous, every good run", loaded=True)
    out = everywhere(eng, ref, good, groups, 2, 1, "pb_asynchronous, q = 1", loaded=True)
    assert out[False][0] == want[0] and want[0], "some fault events defeat a good run"
    kinds = [sorted(events[p][0] for p in c) for _, c in out[False][0]]
    assert ["crash", "omit"] in kinds, "one crash plus one omission, Molly's ordinary hypothesis, is a row"
    crashed = lambda c: len({events[p][1] for p in c if events[p][0] == "crash"})
    assert any(crashed(c) > spec["maxCrashes"] for _, c in out[False][0]), "the crash budget is the caller's filter over the rows"


# ---- protocol ----------------------------------------------------------------------------------------------------------------
def raw(eng, iters, cond, off, labels, n_groups, max_size=2, min_runs=0, flags=0):
    it = np.ascontiguousarray(iters, dtype=np.uint32)
    off = None if off is None else np.ascontiguousarray(off, dtype=np.uint64)
    labels = None if labels is None else np.ascontiguousarray(labels, dtype=np.uint32)
    return eng.L.nemo_min_group_cuts(eng.h, it.ctypes.data if len(it) else None, len(it), cond,
                                     None if off is None else off.ctypes.data,
                                     None if labels is None or not len(labels) else labels.ctypes.data, n_groups, max_size, min_runs, flags)


def fetch_state(eng):
    return eng.L.nemo_fetch_min_group_cuts(eng.h, None, None, 0, None)


def test_protocol(eng, hand, trees):
    eng.load(hand)
    err = lambda: eng.L.nemo_last_error(eng.h).decode()
    assert fetch_state(eng) == 5  # a fetch before any call
    assert eng.L.nemo_fetch_min_group_cut_stats(eng.h, np.zeros(9, np.uint64).ctypes.data) == 5
    for bad in (0, 4, 0xFFFFFFFF):
        assert raw(eng, [0], 1, [0, 1, 2], [10, 11], 2, max_size=bad) == 1 and "max_size must be 1, 2 or 3" in err()
    assert raw(eng, [0], 1, [0, 2, 1, 3], [10, 11, 12], 3) == 1 and "group_off decreases at group 1" in err()
    assert raw(eng, [0], 1, [0, 1, 3], [10, 11, 0xFFFFFFFF], 2) == 1 and "group 1 names label UINT32_MAX" in err() and "position 2" in err()
    assert raw(eng, [0], 1, None, [10], 1) == 1 and "no group_off" in err()
    assert raw(eng, [0], 1, [0, 1], None, 1) == 1 and "no group_labels" in err()
    assert raw(eng, [0], 1, [0, 0, 0], None, 2) == 0  # empty groups name no label: no label array is needed
    assert raw(eng, [0, 1], 1, [0, 1], [10], 1, min_runs=3) == 1 and "min_runs 3" in err()
    assert raw(eng, [0], 1, [0, 1], [10], 1, flags=2) == 1 and "flags" in err()
    assert raw(eng, [0], 2, [0, 1], [10], 1) == 1 and "cond" in err()
    assert raw(eng, [0, 4242], 1, [0, 1], [10], 1) == 7  # an iteration that is not loaded
    # more than 2^32 - 1 labels named in all, from the offsets alone: no label is read (the array holds one)
    assert raw(eng, [0], 1, [0, 1 << 31, 1 << 32], [10], 2) == 6 and "2^32 - 1 labels" in err()
    # more than 2^24 labels in one group, from the offsets alone too
    assert raw(eng, [0], 1, [0, 1, 2 + (1 << 24)], [10], 2) == 6 and "group 1 names 16777217 labels" in err() and "2^24" in err()
    # n * chunks > 2^28 words, from the sizes alone: 2^22 + 1 list positions (run 0, over and over) x 64 chunks
    K = 64 * 64
    assert raw(eng, np.zeros((1 << 22) + 1, np.uint32), 1, np.arange(K + 1), np.arange(K), K) == 6
    assert "2^28 words" in err() and "shorten the group list or the run list" in err()
    assert fetch_state(eng) == 5  # the failed calls (and the one of empty groups before them) left no result
    eng.min_group_cuts([0], 1, [[10]], 1)
    assert fetch_state(eng) == 0
    assert eng.L.nemo_min_group_cuts(eng.h, None, 2, 1, None, None, 0, 2, 0, 0) == 1 and "no run list" in err()
    assert fetch_state(eng) == 5  # ... and neither does a call without a run list
    # zero rows
    rows, n_lost = eng.min_group_cuts([], 1, [[10], [11]], 3)
    assert len(rows) == 0 and len(n_lost) == 0 and not eng.min_group_cut_stats().any()
    rows, n_lost = eng.min_group_cuts([0, 1], 1, [], 3)
    assert len(rows) == 0 and not eng.min_group_cut_stats().any()
    rows, n_lost = eng.min_group_cuts([0, 1], 1, (np.zeros(1, np.uint64), np.zeros(0, np.uint32)), 3)  # the pair form
    assert len(rows) == 0 and not eng.min_group_cut_stats().any()
    # a too-small cap, and the query
    ref = Ref(hand)
    groups = [[10], [11, 12], [13], [20, 21], [22], [1], [6], [10, 13]]
    want = reference(ref, [0, 1, 3], 1, groups, 3, 1, False)
    compare(eng, [0, 1, 3], 1, groups, 3, 1, False, want, "after the errors")
    assert len(want[0]) >= 2
    off = np.cumsum([0] + [len(g) for g in groups]).astype(np.uint64)
    compare(eng, [0, 1, 3], 1, (off, np.array([x for g in groups for x in g], np.uint32)), 3, 1, False, want, "the pair form")
    n = ctypes.c_uint64()
    out = np.zeros(len(want[0]), E.GROUP_CUT_DTYPE)
    assert eng.L.nemo_fetch_min_group_cuts(eng.h, None, None, 0, ctypes.byref(n)) == 0 and n.value == len(want[0])
    assert eng.L.nemo_fetch_min_group_cuts(eng.h, out.ctypes.data, None, len(out) - 1, ctypes.byref(n)) == 1
    assert eng.L.nemo_fetch_min_group_cuts(eng.h, out.ctypes.data, None, len(out), None) == 0 and got_rows(out) == want[0]
    # more than 2^32 - 2 hypotheses in round 3: 2,955 live candidates have 4,296,157,285 triples; K1 is known after round 1
    big = build([level_of(3000)])
    eng.load(big)
    with pytest.raises(E.NemoError) as ei:
        eng.min_group_cuts([0], 1, [[int(big.node_off[1]) + 4 + k] for k in range(2955)], 3)
    assert ei.value.code == 6 and "2^32 - 2 hypotheses" in ei.value.msg and "shorten the group list or the run list" in ei.value.msg
    assert fetch_state(eng) == 5  # and leaves no results
    eng.load(hand)
    compare(eng, [0, 1, 3], 1, groups, 3, 1, False, want, "after the limit")
    eng.load(trees)  # a reload: no result of the previous corpus survives
    assert fetch_state(eng) == 5
    assert eng.L.nemo_fetch_min_group_cut_stats(eng.h, np.zeros(9, np.uint64).ctypes.data) == 5


def test_call_without_a_corpus_and_node_context_refuse(hand):
    fresh = E.Engine(0)
    try:
        with pytest.raises(E.NemoError) as ei:
            fresh.min_group_cuts([0], 1, [[10]], 2)
        assert ei.value.code == 5 and "without a loaded corpus" in ei.value.msg
    finally:
        fresh.close()
    node = E.Engine(devices=[0])
    try:
        node.load(hand)
        with pytest.raises(E.NemoError) as ei:
            node.min_group_cuts([0], 1, [[10]], 2)
        assert ei.value.code == 5 and "single-device contexts only" in ei.value.msg
    finally:
        node.close()


def test_buffers_grow_and_are_reused(eng, seventy):
    its = [int(x) for x in seventy.iteration]
    ref = Ref(seventy)
    labs = [int(x) for x in dict.fromkeys(seventy.label.tolist())][:30]
    eng.load(seventy)
    for n, K in ((3, 10), (70, 25), (1, 3), (130, 12), (70, 25)):
        lst = [its[k % len(its)] for k in range(n)]
        groups = random_unions(labs, K, K)
        want = reference(ref, lst, 1, groups, 2, max(1, n // 4), False, sample=3)
        compare(eng, lst, 1, groups, 2, max(1, n // 4), False, want, f"{n} list positions, {K} groups")


def test_other_results_are_left_alone(eng):
    corpus = random_corpus(1000, n_runs=6, max_nodes=40)[0]
    its = [int(x) for x in corpus.iteration]
    f = corpus.failed_iters() or its[1:3]
    labs = [int(x) for x in dict.fromkeys(corpus.label.tolist())][:20]
    groups = random_unions(labs, 16, 4)
    eng.load(corpus)
    eng.mark()

    def calls():
        eng.diffprov(f, 1)
        eng.diffprov_symmetric(f)
        eng.nearest_runs(its, its)
        eng.knockout_leaves(its, 1)
        eng.min_cuts(its[0], 1, None, 2)
        eng.knockout_labels(its, 1, [[x] for x in labs])
        eng.min_label_cuts(its, 1, labs, 2, 1)

    def others():
        return (np.array(eng.diff_masks(len(f))).copy(), eng.missing().copy(), [m.copy() for m in eng.sdiff_masks()],
                eng.surplus().copy(), eng.label_distances().copy(), eng.knockout_rows().copy(), eng.min_cut_rows().copy(),
                eng.knockout_label_counts()[0].copy(), eng.min_label_cut_rows()[0].copy(), eng.min_label_cut_rows()[1].copy(),
                eng.min_label_cut_stats().copy())

    def same(a, b):
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[3], b[3])
        assert len(a[2]) == len(b[2]) and all(np.array_equal(x, y) for x, y in zip(a[2], b[2]))
        assert all(np.array_equal(a[k], b[k]) for k in range(4, 11))

    calls()
    before = others()
    ref = Ref(corpus)
    want = reference(ref, its, 1, groups, 3, 1, False)
    compare(eng, its, 1, groups, 3, 1, False, want, "between the other calls")
    same(before, others())  # their fetches, unchanged by the group-cut call between them
    calls()
    rows, n_lost = eng.min_group_cut_rows()  # and the reverse
    assert got_rows(rows) == want[0] and n_lost.tolist() == want[1]
    assert eng.min_group_cut_stats().reshape(-1).tolist() == want[2]
