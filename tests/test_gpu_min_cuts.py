"""GPU checks of nemo_min_cuts (k_cut_lds, k_cut_glob, k_cut_count and k_cut_emit in nemo_amd/csrc/k_cuts.hip): every
row, the row order and the round statistics, exact.

Reference.  There is no reference code for the call (include/nemohip.h fixes the semantics), so the reference is the
definition in plain Python over the Corpus arrays, in two forms that must agree with each other before either meets
the device.  (A) brute force: dead_F evaluated for every combination of up to max_size candidates, all hypotheses of a
graph at once (one Python integer per node, bit h = hypothesis h, sinks first), then the lost sets with no lost proper
subset.  (B) the fault-tree derivation, top-down and memoised: the cuts of a rule are the union of its children's, the
cuts of a goal with children the pairwise unions across its children, a candidate adds {v}, everything truncated to
size <= 3 and minimised at every node, the outcome the product over the roots.  Neither calls the library.  The rows'
order is (size, colex rank over the live positions), the live list being the candidates that are no cut alone.

The C3 shape (all sink goals of run 0's post graph, millions of pairs) takes form (A) alone, as the same statement over
numpy words: a u64 row per node and block of 2^18 pairs, pairs enumerated in colex order without any unrank formula.
"""
import itertools
import sys

import numpy as np
import pytest

from nemo_amd import engine as E
from tests.test_gpu_knockout import Graph, build
from tools import synth

pytestmark = pytest.mark.gpu
NONE = 0xFFFFFFFF
sys.setrecursionlimit(max(sys.getrecursionlimit(), 20000))


@pytest.fixture(scope="module")
def eng():
    e = E.Engine(0)
    yield e
    e.close()


# ---- the reference ----------------------------------------------------------------------------------------------
def lost_at_once(gr, sets):
    """bit h of the result: every root is dead under sets[h] (the definition, sinks first)"""
    H, V = len(sets), gr.V
    seed = [0] * V
    for h, F in enumerate(sets):
        for v in F:
            seed[v] |= 1 << h
    full, dead = (1 << H) - 1, [0] * V
    for v in sorted(range(V), key=lambda x: -gr.pos[x]):
        if gr.rule[v]:
            acc = 0
            for c in gr.ch[v]:
                acc |= dead[c]
        else:
            acc = full if gr.ch[v] else 0
            for c in gr.ch[v]:
                acc &= dead[c]
        dead[v] = acc | seed[v]
    lost = full if gr.roots else 0
    for r in gr.roots:
        lost &= dead[r]
    return lost


def cuts_brute(gr, cand, max_size):
    """(A) the minimal cuts as sets of candidate positions"""
    combos = [c for s in range(1, max_size + 1) for c in itertools.combinations(range(len(cand)), s)]
    lost = lost_at_once(gr, [[cand[p] for p in c] for c in combos])
    cut = {frozenset(c) for h, c in enumerate(combos) if (lost >> h) & 1}
    return {c for c in cut if not any(frozenset(s) in cut for k in range(1, len(c)) for s in itertools.combinations(c, k))}


def minimise(sets):
    """the sets with no proper subset among them (sets of at most 3 elements: a set has at most 7 subsets to look up)"""
    pool = set(sets)
    if frozenset() in pool:
        return [frozenset()]
    return [s for s in pool
            if not any(frozenset(t) in pool for k in range(1, len(s)) for t in itertools.combinations(s, k))]


def cuts_fault_tree(gr, cand, max_size):
    """(B) the fault-tree derivation, as sets of candidate positions"""
    where, memo = {v: p for p, v in enumerate(cand)}, {}

    def product(a, b):
        return minimise([x | y for x in a for y in b if len(x | y) <= 3])

    def cuts(v):
        if v not in memo:
            if gr.rule[v]:
                own = [s for c in gr.ch[v] for s in cuts(c)]
            elif gr.ch[v]:
                own = [frozenset()]
                for c in gr.ch[v]:
                    own = product(own, cuts(c))
                    if not own:
                        break
            else:
                own = []
            if v in where:
                own = own + [frozenset([where[v]])]
            memo[v] = minimise(own)
        return memo[v]

    top = [frozenset()] if gr.roots else []
    for r in gr.roots:
        top = product(top, cuts(r))
    return {s for s in top if 1 <= len(s) <= max_size}


def expected(gr, cand, max_size, brute=True):
    """(rows in (size, rank) order, stats) by both forms"""
    b = cuts_fault_tree(gr, cand, max_size)
    if brute:
        a = cuts_brute(gr, cand, max_size)
        assert a == b, f"the two reference forms differ on graph {gr.g}: {sorted(map(sorted, a ^ b))[:6]}"
    K = len(cand)
    single = {next(iter(s)) for s in b if len(s) == 1}
    live = [p for p in range(K) if p not in single]
    at = {p: i for i, p in enumerate(live)}
    c2, c3 = (lambda n: n * (n - 1) // 2), (lambda n: n * (n - 1) * (n - 2) // 6)

    def rank(s):
        p = sorted(s)
        if len(p) == 1:
            return p[0]
        assert all(x in at for x in p), "a minimal cut of size > 1 holds a candidate that is a cut alone"
        q = [at[x] for x in p]
        return c2(q[1]) + q[0] if len(q) == 2 else c3(q[2]) + c2(q[1]) + q[0]

    rows = [(len(s),) + tuple(cand[p] for p in sorted(s)) + (NONE,) * (3 - len(s)) for s in sorted(b, key=lambda s: (len(s), rank(s)))]
    K1 = len(live)
    stats = [[K, K, sum(1 for s in b if len(s) == 1)], [0, 0, 0], [0, 0, 0]]
    if K == 0:
        stats[0] = [0, 0, 0]
    elif max_size >= 2:
        stats[1] = [K1, c2(K1), sum(1 for s in b if len(s) == 2)]
        if max_size >= 3:
            stats[2] = [K1, c3(K1), sum(1 for s in b if len(s) == 3)]
    return rows, stats


def got_rows(arr):
    return [(int(r["size"]),) + tuple(int(x) for x in r["node"]) for r in arr]


def check(eng, corpus, it, cand, max_size, what="", graph=None, brute=True, cond=1, want=None):
    gr = graph or Graph(corpus, 2 * corpus.run_index(it) + cond)
    clist = list(gr.leaves) if cand is None else list(cand)
    rows, stats = want or expected(gr, clist, max_size, brute)
    got = eng.min_cuts(it, cond, cand, max_size)
    assert got.dtype == E.CUT_DTYPE
    g = got_rows(got)
    assert len(g) == len(rows), f"{what}: {len(g)} rows, want {len(rows)}"
    bad = [k for k in range(len(rows)) if g[k] != rows[k]]
    assert not bad, f"{what}: rows {bad[:6]} differ: got {[g[k] for k in bad[:6]]}, want {[rows[k] for k in bad[:6]]}"
    assert eng.min_cut_stats().tolist() == stats, f"{what}: stats {eng.min_cut_stats().tolist()}, want {stats}"
    return rows, stats


def tiers_and_grids(eng, corpus, fn, grids=(0,)):
    """fn(what) on both tiers (knock_lds_max default and 0) and under every cut_grid of `grids`"""
    out = None
    try:
        for lds in (-1, 0):
            for grid in grids:
                eng.set_option("knock_lds_max", lds)
                eng.set_option("cut_grid", grid)
                eng.load(corpus)
                out = fn(f"knock_lds_max {lds}, cut_grid {grid}")
    finally:
        eng.set_option("knock_lds_max", -1)
        eng.set_option("cut_grid", 0)
    return out


# ---- hand-built graphs: one per rule of the semantics ----------------------------------------------------------------
# goal 0 <- rule 1 <- (a 3, b 4); goal 0 <- rule 2 <- (a 3, c 5): {a} is a cut, and so is {b, c}
SINGLE = ("grrggg", [(0, 1), (0, 2), (1, 3), (1, 4), (2, 3), (2, 5)])
# two roots: goal 0 <- rule 2 <- a 4; goal 1 <- rule 3 <- b 5: lost needs both
TWO_ROOTS = ("ggrrgg", [(0, 2), (1, 3), (2, 4), (3, 5)])
# goal 0 <- rule 1 <- a 4; <- rule 2 <- b 5; <- rule 3 <- (c 6, d 7): {a, b, c} and {a, b, d}, nothing smaller
TRIPLES = ("grrrgggg", [(0, 1), (0, 2), (0, 3), (1, 4), (2, 5), (3, 6), (3, 7)])
# goal 0 <- rule 1 <- a 3; goal 0 <- rule 2 <- b 4; the inner goal a <- rule 5 <- c 7 and a <- rule 6 <- e 8:
# {a, b} is a cut, c alone does not kill a, so {a, b, c} is lost and not minimal
INNER = ("grrggrrgg", [(0, 1), (0, 2), (1, 3), (2, 4), (3, 5), (3, 6), (5, 7), (6, 8)])
HAND = [SINGLE, TWO_ROOTS, TRIPLES, INNER]


@pytest.fixture(scope="module")
def hand():
    return build(HAND)


def test_hand_built(eng, hand):
    def run(w):
        out = {}
        out["single"] = check(eng, hand, 0, [3, 4, 5], 3, f"a size-1 cut, {w}")[0]
        out["roots"] = check(eng, hand, 1, [4, 5], 3, f"two roots, {w}")[0]
        out["triples"] = check(eng, hand, 2, [4, 5, 6, 7], 3, f"three rules, {w}")[0]
        out["triples2"] = check(eng, hand, 2, [4, 5, 6, 7], 2, f"three rules, max_size 2, {w}")
        out["inner"] = check(eng, hand, 3, [3, 4, 7], 3, f"an irrelevant candidate, {w}")
        out["kinds"] = check(eng, hand, 3, [1, 2, 3, 4, 5, 6, 7, 8], 3, f"rules and inner goals, {w}")[0]
        out["order"] = check(eng, hand, 3, [4, 3], 2, f"a list in descending node order, {w}")[0]
        out["order3"] = check(eng, hand, 2, [7, 5, 6, 4], 3, f"a list in no order, {w}")[0]
        a = check(eng, hand, 2, None, 3, f"cand NULL, {w}")
        b = check(eng, hand, 2, [4, 5, 6, 7], 3, f"the explicit sink goals, {w}")
        assert a == b
        out["none"] = check(eng, hand, 3, [7], 3, f"no cut at all, {w}")
        out["k1"] = check(eng, hand, 0, [3], 3, f"K = 1, {w}")
        out["k2"] = check(eng, hand, 0, [4, 5], 3, f"K = 2, {w}")
        out["k3"] = check(eng, hand, 2, [4, 5, 6], 3, f"K = 3, {w}")
        assert len(eng.min_cuts(0, 1, [], 3)) == 0 and eng.min_cut_stats().tolist() == [[0, 0, 0]] * 3
        return out
    o = tiers_and_grids(eng, hand, run, grids=(0, 1, 2, 3))
    assert o["single"] == [(1, 3, NONE, NONE), (2, 4, 5, NONE)]  # no pair holds the size-1 cut
    assert o["roots"] == [(2, 4, 5, NONE)]
    assert o["triples"] == [(3, 4, 5, 6), (3, 4, 5, 7)] and o["triples2"] == ([], [[4, 4, 0], [4, 6, 0], [0, 0, 0]])
    assert o["inner"] == ([(2, 3, 4, NONE)], [[3, 3, 0], [3, 3, 1], [3, 1, 0]])  # the triple is lost and filtered
    assert (2, 1, 2, NONE) in o["kinds"] and (2, 1, 4, NONE) in o["kinds"] and (3, 2, 5, 6) in o["kinds"]
    assert o["order"] == [(2, 4, 3, NONE)]  # list order, not node order
    assert o["order3"] == [(3, 7, 5, 4), (3, 5, 6, 4)]
    assert o["none"] == ([], [[1, 1, 0], [1, 0, 0], [1, 0, 0]])  # zero rows, full stats
    assert o["k1"] == ([(1, 3, NONE, NONE)], [[1, 1, 1], [0, 0, 0], [0, 0, 0]])
    assert o["k2"] == ([(2, 4, 5, NONE)], [[2, 2, 0], [2, 1, 1], [2, 0, 0]])
    assert o["k3"] == ([(3, 4, 5, 6)], [[3, 3, 0], [3, 3, 0], [3, 1, 1]])


# ---- chunk edges -----------------------------------------------------------------------------------------------------
def three_rules(n):
    """goal 0 <- rules 1, 2, 3; leaf i is a premise of rule i % 3, every fifth leaf of a second rule as well: no leaf
    is a cut alone, so all n are live; pairs and triples that reach all three rules are cuts"""
    edges = [(0, 1), (0, 2), (0, 3)]
    for i in range(n):
        edges.append((1 + i % 3, 4 + i))
        if i % 5 == 0:
            edges.append((1 + (i % 3 + 1 + (i // 5) % 2) % 3, 4 + i))  # one of the other two rules
    return "grrr" + "g" * n, edges


PAIRS = [11, 12, 63, 64, 65, 128]   # C(128,2) = 8,128 hypotheses: exactly 127 chunks
TRIPLE_SIZES = [8, 9, 64]           # C(64,3) = 41,664: exactly 651 chunks, more than the default grid


@pytest.fixture(scope="module")
def edges_corpus():
    return build([three_rules(n) for n in PAIRS + TRIPLE_SIZES])


@pytest.mark.parametrize("k", range(len(PAIRS) + len(TRIPLE_SIZES)))
def test_chunk_edges(eng, edges_corpus, k):
    n = (PAIRS + TRIPLE_SIZES)[k]
    size = 2 if k < len(PAIRS) else 3
    gr = Graph(edges_corpus, 2 * k + 1)
    cand = list(range(4, 4 + n))
    want = expected(gr, cand, size)
    assert want[1][size - 1][0] == n and want[1][size - 1][2] > 0, "every candidate live, and some cut of the size"
    grids = (0, 1, 2, 3) if n in (65, 128) or size == 3 else (0,)
    tiers_and_grids(eng, edges_corpus, lambda w: check(eng, edges_corpus, k, cand, size, f"{n} live, size {size}, {w}", gr,
                                                       want=want), grids)


# ---- sweep edges inside the persistent loop ------------------------------------------------------------------------
def hub():
    """goal 0 <- 300 rules; rule k <- leaf k % 2 (nodes 301, 302), the first 15 rules also <- a leaf of their own:
    a 300-children AND row; {301, 302} is the only cut"""
    edges = [(0, 1 + k) for k in range(300)] + [(1 + k, 301 + k % 2) for k in range(300)]
    edges += [(1 + k, 303 + k) for k in range(15)]
    return "g" + "r" * 300 + "g" * 17, edges, list(range(301, 318))


def level():
    """goal 0 <- rule 1 <- leaves 3..302, goal 0 <- rule 2 <- leaves 303..602: a level of 600 nodes"""
    edges = [(0, 1), (0, 2)] + [(1, 3 + k) for k in range(300)] + [(2, 303 + k) for k in range(300)]
    return "grr" + "g" * 600, edges, list(range(3, 12)) + list(range(303, 312))


def chains():
    """goal 0 <- rule, rule <- goal ... twice, 150 goal / rule pairs deep each: 301 Kahn levels; the candidates
    are inner goals and rules of both chains"""
    kinds, edges, ends = "g", [], []
    for _ in range(2):
        prev = 0
        for d in range(300):
            kinds += "r" if d % 2 == 0 else "g"
            edges.append((prev, len(kinds) - 1))
            prev = len(kinds) - 1
        ends.append(prev)
    a = [1 + 30 * j for j in range(9)]
    return kinds, edges, a + [300 + x + 1 for x in a]


def level_of(n):
    """goal 0 <- rule 1 <- one leaf (node 3), goal 0 <- rule 2 <- n leaves (4 ..): no cut among the n leaves alone"""
    return "grr" + "g" * (n + 1), [(0, 1), (0, 2), (1, 3)] + [(2, 4 + k) for k in range(n)]


@pytest.fixture(scope="module")
def sweeps():
    shapes = [hub(), level(), chains()]
    return build([s[:2] for s in shapes]), [s[2] for s in shapes]


@pytest.mark.parametrize("k, name", [(0, "a hub of 300 children"), (1, "a level of 600 nodes"), (2, "301 levels")])
def test_sweep_edges(eng, sweeps, k, name):
    corpus, cands = sweeps
    gr = Graph(corpus, 2 * k + 1)
    want = expected(gr, cands[k], 2)
    assert want[1][1][1] >= 130 and want[1][1][2] >= 1, "at least 130 pairs and a cut among them"
    if k == 2:
        assert len(Graph(corpus, 5).roots) == 1 and max(gr.pos) == gr.V - 1 and gr.V == 601
    tiers_and_grids(eng, corpus, lambda w: check(eng, corpus, k, cands[k], 2, f"{name}, {w}", gr, want=want), grids=(1, 0))


# ---- generated fault trees --------------------------------------------------------------------------------------------
def fault_tree(seed, max_leaves=24):
    """an alternating goal / rule tree with shared leaves: goals have 1-3 rules, rules 1-3 premises"""
    rng = np.random.default_rng(seed)
    kinds, edges, leaves = ["g"], [], []
    todo = [(0, 0)]
    while todo:
        g, depth = todo.pop(0)
        if depth >= 3 or (depth and rng.random() < 0.25) or len(kinds) > 90:
            leaves.append(g)
            continue
        for _ in range(int(rng.integers(1, 4))):
            kinds.append("r")
            r = len(kinds) - 1
            edges.append((g, r))
            used = set()
            for _ in range(int(rng.integers(1, 4))):
                if leaves and rng.random() < 0.35:
                    c = leaves[int(rng.integers(0, len(leaves)))]
                    if c in used:
                        continue
                    used.add(c)
                    edges.append((r, c))
                else:
                    kinds.append("g")
                    edges.append((r, len(kinds) - 1))
                    todo.append((len(kinds) - 1, depth + 1))
    return "".join(kinds), edges


GEN_SEEDS = [137, 139, 151, 154, 160]


def test_generated_fault_trees(eng):
    corpus = build([fault_tree(s) for s in GEN_SEEDS])
    graphs = [Graph(corpus, 2 * k + 1) for k in range(len(GEN_SEEDS))]
    cands = [gr.leaves[:24] for gr in graphs]
    wants = [expected(gr, c, 3) for gr, c in zip(graphs, cands)]
    assert sum(1 for w in wants if w[1][1][2] > 0) >= 3, "at least three graphs with a minimal cut of size 2"
    assert sum(1 for w in wants if w[1][2][2] > 0) >= 3, "at least three graphs with a minimal cut of size 3"

    def run(w):
        for k in range(len(GEN_SEEDS)):
            check(eng, corpus, k, cands[k], 3, f"seed {GEN_SEEDS[k]}, {w}", graphs[k], want=wants[k])
    tiers_and_grids(eng, corpus, run, grids=(0, 2))


# ---- against the existing calls, device against device ----------------------------------------------------------------
def test_against_knockout(eng):
    corpus = build([fault_tree(s) for s in GEN_SEEDS] + HAND)
    eng.load(corpus)
    seen = 0
    for it in range(len(GEN_SEEDS) + len(HAND)):
        leaves = eng.knockout_leaves([it], 1).copy()
        cuts = eng.min_cuts(it, 1, None, 3).copy()
        lost1 = [int(r["node"]) for r in leaves if int(r["n_roots"]) > 0 and int(r["roots_dead"]) == int(r["n_roots"])]
        assert [int(r["node"][0]) for r in cuts if int(r["size"]) == 1] == lost1
        sets, is_cut = [], []
        for r in cuts:
            nodes = [int(x) for x in r["node"][:int(r["size"])]]
            sets.append(nodes)
            is_cut.append(True)
            for k in range(1, len(nodes)):
                for sub in itertools.combinations(nodes, k):
                    sets.append(list(sub))
                    is_cut.append(False)
        if not sets:
            continue
        rows = eng.knockout_sets(it, 1, sets)
        for r, c in zip(rows, is_cut):
            assert (int(r["n_roots"]) > 0 and int(r["roots_dead"]) == int(r["n_roots"])) == c
        seen += len(cuts)
    assert seen > 10


# ---- the C3 shape: every sink goal of run 0's post graph, millions of pairs ------------------------------------------
def lost_pairs_numpy(gr, cand, block=1 << 18):
    """(A) over numpy words: bit h of the result = every root is dead under pair h of the candidates, pairs in colex
    order (b outermost, a < b)"""
    K = len(cand)
    H = K * (K - 1) // 2
    pb = np.repeat(np.arange(K, dtype=np.int64), np.arange(K, dtype=np.int64))
    pa = np.arange(H, dtype=np.int64) - pb * (pb - 1) // 2
    node = np.asarray(cand, dtype=np.int64)
    order = sorted(range(gr.V), key=lambda x: -gr.pos[x])
    out = np.zeros(H, bool)
    one = np.uint64(1)
    for h0 in range(0, H, block):
        h1 = min(H, h0 + block)
        W = (h1 - h0 + 63) // 64
        dead = np.zeros((gr.V, W), np.uint64)
        rel = np.arange(h1 - h0, dtype=np.int64)
        bit = one << (rel & 63).astype(np.uint64)
        for pos in (pa[h0:h1], pb[h0:h1]):
            np.bitwise_or.at(dead, (node[pos], rel >> 6), bit)
        for v in order:
            ch = gr.ch[v]
            if not ch:
                continue
            rows = dead[ch]
            acc = np.bitwise_or.reduce(rows, axis=0) if gr.rule[v] else np.bitwise_and.reduce(rows, axis=0)
            dead[v] |= acc
        lost = np.bitwise_and.reduce(dead[gr.roots], axis=0) if gr.roots else np.zeros(W, np.uint64)
        out[h0:h1] = np.unpackbits(lost.view(np.uint8), bitorder="little")[:h1 - h0].astype(bool)
    return pa, pb, out


def check_pairs_at_scale(eng, corpus, it, gr, lists, what):
    """max_size 2 over all sink goals of a graph against form (A) in numpy words; lists: the candidate lists to pass
    (None and / or the explicit list).  Returns the stats."""
    cand = list(gr.leaves)
    K = len(cand)
    single = lost_at_once(gr, [[v] for v in cand])
    is_single = np.array([(single >> p) & 1 for p in range(K)], bool)
    pa, pb, lost = lost_pairs_numpy(gr, cand)
    keep = lost & ~is_single[pa] & ~is_single[pb]  # no lost proper subset
    live_at = np.cumsum(~is_single) - 1             # candidate position -> live position
    K1 = int((~is_single).sum())
    la, lb = live_at[pa[keep]], live_at[pb[keep]]
    by_rank = np.argsort(lb * (lb - 1) // 2 + la, kind="stable")
    node = np.asarray(cand, np.int64)
    n1 = int(is_single.sum())
    want = np.full((n1 + len(by_rank), 4), NONE, np.int64)
    want[:n1, 0], want[:n1, 1] = 1, node[is_single]
    want[n1:, 0], want[n1:, 1], want[n1:, 2] = 2, node[pa[keep]][by_rank], node[pb[keep]][by_rank]
    stats = [[K, K, n1], [K1, K1 * (K1 - 1) // 2, len(by_rank)], [0, 0, 0]]
    eng.load(corpus)
    for cl in lists:
        got = eng.min_cuts(it, 1, cl, 2)
        have = np.column_stack([got["size"].astype(np.int64), got["node"].astype(np.int64)]).reshape(-1, 4)
        assert have.shape == want.shape, f"{what}: {have.shape[0]} rows, want {want.shape[0]}"
        bad = np.nonzero((have != want).any(axis=1))[0]
        assert not len(bad), f"{what}: rows {bad[:6]} differ: got {have[bad[:6]].tolist()}, want {want[bad[:6]].tolist()}"
        assert eng.min_cut_stats().tolist() == stats, what
    return stats


def test_c3_shape_all_sink_goals(eng):
    """The 12-run C3 shape, run 0's post graph, every sink goal, max_size 2.  By the reference this graph (30 roots)
    has no cut of size <= 2: the case checks 4.36 M hypotheses in 68 k chunks for a false positive, and the stats."""
    corpus, _ = synth.generate(12, p_fault=0.55, prepend_run0=True, **synth.CONFIGS["c3"])
    it = int(corpus.iteration[0])
    gr = Graph(corpus, 2 * corpus.run_index(it) + 1)
    assert len(gr.leaves) > 2000, "the C3 shape has thousands of sink goals per graph"
    stats = check_pairs_at_scale(eng, corpus, it, gr, (None, list(gr.leaves)), "c3, run 0")
    assert stats[1][1] > 64 * 4096, "far more chunks than the persistent grid has workgroups"


def test_pairs_at_the_c3_count_with_cuts(eng):
    """As many live candidates as the C3 shape has (2,953), on a graph whose pair cuts lie all over the rank range:
    goal 0 <- rule 1 <- three leaves, goal 0 <- rule 2 <- 2,950 leaves; a cut is one leaf of each rule."""
    edges = [(0, 1), (0, 2)] + [(1, 3 + k) for k in (0, 1500, 2952)] + [(2, 3 + k) for k in range(2953) if k not in (0, 1500, 2952)]
    corpus = build([("grr" + "g" * 2953, edges)])
    gr = Graph(corpus, 1)
    stats = check_pairs_at_scale(eng, corpus, 0, gr, (None,), "2,953 live")
    assert stats == [[2953, 2953, 0], [2953, 2953 * 2952 // 2, 3 * 2950], [0, 0, 0]]


# ---- a post graph of >= 65536 nodes: u32 rows, the global tier by size ------------------------------------------------
def test_graph_past_65535_nodes(eng):
    corpus, _ = synth.generate(3, target_nodes=140000, p_fault=0.9, prepend_run0=True, seed=3, eot=80, body_extra=6,
                               nval=3, nloc=4)
    r = max(range(corpus.n_runs), key=lambda x: corpus.graph_size(2 * x + 1))
    gr = Graph(corpus, 2 * r + 1)
    assert gr.V >= 65536
    rng = np.random.default_rng(5)
    cand = [gr.leaves[int(x)] for x in rng.choice(len(gr.leaves), 40, replace=False)]
    eng.load(corpus)
    check(eng, corpus, int(corpus.iteration[r]), cand, 3, "66k nodes", gr)


# ---- protocol ----------------------------------------------------------------------------------------------------------
def test_protocol(eng, hand, edges_corpus):
    eng.load(hand)
    assert eng.L.nemo_fetch_min_cuts(eng.h, None, 0, None) == 5  # a fetch before any call
    assert eng.L.nemo_fetch_min_cut_stats(eng.h, np.zeros(9, np.uint64).ctypes.data) == 5
    for bad in (0, 4, 0xFFFFFFFF):
        with pytest.raises(E.NemoError) as ei:
            eng.min_cuts(0, 1, [3, 4], bad)
        assert ei.value.code == 1 and "max_size" in ei.value.msg
    with pytest.raises(E.NemoError) as ei:
        eng.min_cuts(0, 1, [3, 4, 3], 2)
    assert ei.value.code == 1 and "second time" in ei.value.msg
    with pytest.raises(E.NemoError) as ei:  # node 6 of the 6-node graph
        eng.min_cuts(0, 1, [3, 6], 2)
    assert ei.value.code == 1 and "out of range" in ei.value.msg
    with pytest.raises(E.NemoError) as ei:
        eng.min_cuts(4242, 1, [3], 2)
    assert ei.value.code == 7
    with pytest.raises(E.NemoError) as ei:
        eng.min_cuts(0, 2, [3], 2)
    assert ei.value.code == 1
    assert eng.L.nemo_fetch_min_cuts(eng.h, None, 0, None) == 5  # the failed calls left no result
    check(eng, hand, 0, [3, 4, 5], 3, "after the errors")
    # more than 2^32 - 2 hypotheses in a round: 2,955 live candidates have 4,296,157,285 triples
    eng.load(build([level_of(3000)]))
    with pytest.raises(E.NemoError) as ei:
        eng.min_cuts(0, 1, list(range(4, 4 + 2955)), 3)
    assert ei.value.code == 6 and "shorten the candidate list" in ei.value.msg
    assert eng.L.nemo_fetch_min_cuts(eng.h, None, 0, None) == 5  # and leaves no results
    eng.load(hand)
    eng.load(edges_corpus)  # a reload: no result of the previous corpus survives
    assert eng.L.nemo_fetch_min_cuts(eng.h, None, 0, None) == 5
    check(eng, edges_corpus, 0, list(range(4, 15)), 2, "after the reload")


def test_node_context_refuses(hand):
    node = E.Engine(devices=[0])
    try:
        node.load(hand)
        with pytest.raises(E.NemoError) as ei:
            node.min_cuts(0, 1, [3], 2)
        assert ei.value.code == 5 and "single-device contexts only" in ei.value.msg
    finally:
        node.close()


def test_buffers_grow_and_are_reused(eng):
    corpus = build([three_rules(130)])
    gr = Graph(corpus, 1)
    eng.load(corpus)
    for n in (3, 70, 1, 130, 70):
        check(eng, corpus, 0, list(range(4, 4 + n)), 2, f"{n} candidates", gr)


def test_other_results_are_left_alone(eng):
    from tests.small import random_corpus
    corpus = random_corpus(1000, n_runs=6, max_nodes=40)[0]
    its = [int(x) for x in corpus.iteration]
    f = corpus.failed_iters() or its[1:3]
    eng.load(corpus)
    eng.mark()

    def others():
        return (np.array(eng.diff_masks(len(f))).copy(), eng.missing().copy(), [m.copy() for m in eng.sdiff_masks()],
                eng.surplus().copy(), eng.label_distances().copy(), eng.knockout_rows().copy())

    def same(a, b):
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[3], b[3])
        assert len(a[2]) == len(b[2]) and all(np.array_equal(x, y) for x, y in zip(a[2], b[2]))
        assert np.array_equal(a[4], b[4]) and np.array_equal(a[5], b[5])

    eng.diffprov(f, 1)
    eng.diffprov_symmetric(f)
    eng.nearest_runs(its, its)
    eng.knockout_leaves(its, 1)
    before = others()
    rows = [check(eng, corpus, it, None, 3, f"run {it} between the other calls")[0] for it in its]
    same(before, others())  # their fetches, unchanged by the cut calls between them
    last = got_rows(eng.min_cut_rows())
    eng.knockout_leaves(its, 1)
    eng.knockout_sets(its[0], 1, [[0]])
    assert got_rows(eng.min_cut_rows()) == last == rows[-1]  # and the reverse
