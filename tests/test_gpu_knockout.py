"""GPU checks of the knock-out analysis (nemo_knockout_leaves / nemo_knockout_sets; k_ko_leaves, k_ko_lds and
k_ko_glob in nemo_amd/csrc/k_knock.hip): every row, and every dead mask where kept, exact.

Reference.  There is no reference code for these calls (include/nemohip.h fixes the semantics), so the reference
is the definition in plain Python over the Corpus arrays, in two forms that must agree with each other before
either is compared with the device: (A) dead_h(v) evaluated per hypothesis in reverse topological order, and
(B) a memoised top-down "is there a derivation" recursion (a goal holds if it has no children or one of them
holds, a rule if all of them hold, nothing in F holds).  Neither calls the library or the oracle.  Both skip the
nodes that are no ancestor of F (such a node is alive: being dead takes membership in F or a dead child).
The two cases with thousands of hypotheses or tens of thousands of ancestors (the C3 shape, the 66k-node graph)
would take Python a quarter of a minute that way, so there all rows come from (A) evaluated for all hypotheses
of a graph at once (one Python integer per node, bit h = hypothesis h: the same statement, sinks first), and
the two per-hypothesis forms are run on every `sample`-th hypothesis and must agree with it.

A goal whose child is a goal.  The definition goes by a node's own kind only, and both reference forms are
checked on such a graph; nemo_load_corpus refuses it (a goal -> goal DUETO edge fails loadProv's count check,
NEMO_ERR_LOAD), so the device never sees one: the test asserts that refusal.
"""
import sys

import numpy as np
import pytest

from nemo_amd import engine as E
from nemo_amd.corpus import NODE_RULE, Corpus
from tests.small import random_corpus
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
class Graph:
    """Graph g of a corpus: kinds, child and parent lists, a topological order, roots and sink goals."""

    def __init__(self, corpus: Corpus, g: int):
        n0, n1 = int(corpus.node_off[g]), int(corpus.node_off[g + 1])
        e0, e1 = int(corpus.edge_off[g]), int(corpus.edge_off[g + 1])
        self.g, self.V = g, n1 - n0
        self.rule = [bool(w & NODE_RULE) for w in corpus.node_word[n0:n1].tolist()]
        self.ch = [[] for _ in range(self.V)]
        self.pa = [[] for _ in range(self.V)]
        for s, d in zip(corpus.edge_src[e0:e1].tolist(), corpus.edge_dst[e0:e1].tolist()):
            self.ch[s].append(d)
            self.pa[d].append(s)
        indeg = [len(p) for p in self.pa]
        self.roots = [v for v in range(self.V) if not indeg[v]]
        order = list(self.roots)
        for v in order:  # Kahn: parents before children
            for c in self.ch[v]:
                indeg[c] -= 1
                if not indeg[c]:
                    order.append(c)
        assert len(order) == self.V, "the graph is not acyclic"
        self.pos = [0] * self.V
        for i, v in enumerate(order):
            self.pos[v] = i
        self.leaves = [v for v in range(self.V) if not self.rule[v] and not self.ch[v]]

    def ancestors(self, F):
        seen, todo = set(F), list(F)
        while todo:
            for p in self.pa[todo.pop()]:
                if p not in seen:
                    seen.add(p)
                    todo.append(p)
        return seen

    def dead_by_definition(self, F):
        """(A) the definition, sinks first, over the ancestors of F"""
        F, dead = set(F), set()
        for v in sorted(self.ancestors(F), key=lambda x: -self.pos[x]):
            if v in F:
                dead.add(v)
            elif self.rule[v]:
                if any(c in dead for c in self.ch[v]):
                    dead.add(v)
            elif self.ch[v] and all(c in dead for c in self.ch[v]):
                dead.add(v)
        return dead

    def dead_by_derivation(self, F):
        """(B) a node is dead iff it has no derivation: memoised recursion from the top"""
        F, anc, memo = set(F), self.ancestors(F), {}

        def holds(v):
            if v not in anc:
                return True
            if v not in memo:
                if v in F:
                    memo[v] = False
                elif self.rule[v]:
                    memo[v] = all(holds(c) for c in self.ch[v])
                else:
                    memo[v] = not self.ch[v] or any(holds(c) for c in self.ch[v])
            return memo[v]

        return {v for v in anc if not holds(v)}

    def row(self, F, node=NONE):
        """(graph, node, n_dead, roots_dead, n_roots) and the dead set; the two forms must agree"""
        a, b = self.dead_by_definition(F), self.dead_by_derivation(F)
        assert a == b, f"the two reference forms differ on graph {self.g}, F = {sorted(F)[:8]}"
        return (self.g, node, len(a), sum(1 for r in self.roots if r in a), len(self.roots)), a

    def rows_at_once(self, sets, nodes, sample):
        """The rows of many hypotheses on this graph: (A) for all of them at once, bit h of a node's integer =
        dead under sets[h]; every `sample`-th hypothesis also through row()"""
        H, V = len(sets), self.V
        seed = [0] * V
        for h, F in enumerate(sets):
            for v in F:
                seed[v] |= 1 << h
        full, dead = (1 << H) - 1, [0] * V
        for v in sorted(range(V), key=lambda x: -self.pos[x]):
            if self.rule[v]:
                acc = 0
                for c in self.ch[v]:
                    acc |= dead[c]
            else:
                acc = full if self.ch[v] else 0
                for c in self.ch[v]:
                    acc &= dead[c]
            dead[v] = acc | seed[v]
        nb = (H + 7) // 8
        cols = lambda x: np.unpackbits(np.frombuffer(x.to_bytes(nb, "little"), np.uint8), bitorder="little")[:H]
        n_dead, r_dead = np.zeros(H, np.int64), np.zeros(H, np.int64)
        for v in range(V):
            if dead[v]:
                n_dead += cols(dead[v])
        for r in self.roots:
            if dead[r]:
                r_dead += cols(dead[r])
        rows = [(self.g, nodes[h], int(n_dead[h]), int(r_dead[h]), len(self.roots)) for h in range(H)]
        for h in range(0, H, sample):
            assert self.row(sets[h], nodes[h])[0] == rows[h], f"the reference forms differ on graph {self.g}, hypothesis {h}"
        return rows

    def mask(self, dead):
        m = np.zeros(self.V, np.uint8)
        m[sorted(dead)] = 1
        return m


def _rows(got):
    return [tuple(int(x) for x in r) for r in got.tolist()]


def check_leaves(eng, corpus, iters, cond=1, masks=False, what="", graphs=None, sample=0):
    """leaves mode over `iters` against the reference: every row, the ranges, and every mask where kept.
    sample: the rows of a graph at once, the per-hypothesis forms on every sample-th (no masks then)"""
    graphs = graphs if graphs is not None else {}
    want, wmask, ranges, cache = [], [], [], {}
    for it in iters:
        g = 2 * corpus.run_index(it) + cond
        if g not in graphs:
            graphs[g] = Graph(corpus, g)
        gr = graphs[g]
        ranges.append((len(want), len(gr.leaves)))
        if sample:
            assert not masks
            if g not in cache:
                cache[g] = gr.rows_at_once([[v] for v in gr.leaves], gr.leaves, sample)
            want += cache[g]
            continue
        for v in gr.leaves:
            row, dead = gr.row([v], v)
            want.append(row)
            wmask.append((gr, dead))
    got = eng.knockout_leaves(iters, cond, masks=masks)
    assert got.dtype == E.KNOCK_DTYPE and len(got) == len(want), f"{what}: {len(got)} rows, want {len(want)}"
    rows = _rows(got)
    bad = [h for h in range(len(want)) if rows[h] != want[h]]
    assert not bad, f"{what}: rows {bad[:6]} differ: got {[rows[h] for h in bad[:6]]}, want {[want[h] for h in bad[:6]]}"
    first, count = eng.knockout_ranges()
    assert [(int(a), int(b)) for a, b in zip(first, count)] == ranges, what
    if masks:
        for h, (gr, dead) in enumerate(wmask):
            assert np.array_equal(eng.knockout_mask(h, gr.V), gr.mask(dead)), f"{what}: mask of hypothesis {h}"
    return rows


def check_sets(eng, corpus, it, cond, sets, masks=False, what="", graph=None, sample=0):
    g = 2 * corpus.run_index(it) + cond
    gr = graph or Graph(corpus, g)
    if sample:
        assert not masks
        want = [(r, None) for r in gr.rows_at_once(sets, [NONE] * len(sets), sample)]
    else:
        want = [gr.row(F) for F in sets]
    got = eng.knockout_sets(it, cond, sets, masks=masks)
    assert len(got) == len(sets), what
    rows = _rows(got)
    bad = [h for h in range(len(sets)) if rows[h] != want[h][0]]
    assert not bad, f"{what}: rows {bad[:6]} differ: got {[rows[h] for h in bad[:6]]}, want {[want[h][0] for h in bad[:6]]}"
    if sets:
        first, count = eng.knockout_ranges()
        assert (int(first[0]), int(count[0])) == (0, len(sets)), what
    if masks:
        for h, (_, dead) in enumerate(want):
            assert np.array_equal(eng.knockout_mask(h, gr.V), gr.mask(dead)), f"{what}: mask of set {h}"
    return rows


def both_tiers(eng, fn):
    """fn() under the LDS tier (where the graph fits it) and with every graph in device memory"""
    try:
        for lds in (-1, 0):
            eng.set_option("knock_lds_max", lds)
            out = fn(f"knock_lds_max {lds}")
    finally:
        eng.set_option("knock_lds_max", -1)
    return out


# ---- hand-built graphs --------------------------------------------------------------------------------------------
def build(posts, iters=None) -> Corpus:
    """A corpus whose run r has the post graph posts[r] = (kinds, edges): kinds a string of 'g' / 'r' per node,
    edges (source, target) pairs along DUETO; every pre graph is one goal.  Tables: 0 pre, 1 post, 2 t."""
    node_off, edge_off, word, src, dst = [0], [0], [], [], []
    for kinds, edges in posts:
        word.append(0)  # the pre graph: one goal of table "pre"
        node_off.append(len(word))
        edge_off.append(len(src))
        word += [(NODE_RULE | 2) if k == "r" else 2 for k in kinds]
        src += [a for a, _ in edges]
        dst += [b for _, b in edges]
        node_off.append(len(word))
        edge_off.append(len(src))
    u32 = lambda x: np.ascontiguousarray(x, dtype=np.uint32)
    iters = list(range(len(posts))) if iters is None else iters
    return Corpus(iteration=u32(iters), node_off=np.ascontiguousarray(node_off, dtype=np.uint64),
                  edge_off=np.ascontiguousarray(edge_off, dtype=np.uint64), node_word=u32(word),
                  label=u32(np.arange(len(word))), edge_src=u32(src), edge_dst=u32(dst), n_tables=3, table_pre=0,
                  table_post=1, status=["success"] * len(posts))


LONE = ("g", [])
# goal 0 <- rules 1, 2; rule 1 <- leaves 3, 4; rule 2 <- leaves 5, 6
TWO_RULES = ("grrgggg", [(0, 1), (0, 2), (1, 3), (1, 4), (2, 5), (2, 6)])
# leaf 3 is a premise of both rules
SHARED = ("grrggg", [(0, 1), (0, 2), (1, 3), (1, 4), (2, 3), (2, 5)])
# rule 2 has no children (alive unless in F); goal 0 <- rules 1, 2; rule 1 <- leaf 3
CHILDLESS_RULE = ("grrg", [(0, 1), (0, 2), (1, 3)])
# two roots: goal 0 <- rule 2 <- leaf 4; goal 1 <- rules 2, 3; rule 3 <- leaf 5
TWO_ROOTS = ("ggrrgg", [(0, 2), (1, 2), (1, 3), (2, 4), (3, 5)])
# no sink goal: goal 0 <- rule 1 (a rule without children is the only sink)
NO_SINK_GOAL = ("gr", [(0, 1)])
HAND = [LONE, TWO_RULES, SHARED, CHILDLESS_RULE, TWO_ROOTS, NO_SINK_GOAL]


@pytest.fixture(scope="module")
def hand():
    return build(HAND)


def test_hand_built_leaves(eng, hand):
    its = list(range(len(HAND)))
    rows = both_tiers(eng, lambda w: (eng.load(hand), check_leaves(eng, hand, its, masks=True, what=w))[1])
    by_graph = {}
    for r in rows:
        by_graph.setdefault(r[0], []).append(r)
    lost = lambda r: r[4] > 0 and r[3] == r[4]
    assert [lost(r) for r in by_graph[1]] == [True]                          # a lone goal is its own outcome
    assert [lost(r) for r in by_graph[3]] == [False] * 4                     # one leaf lost: the other rule derives
    assert [(r[1], lost(r)) for r in by_graph[5]] == [(3, True), (4, False), (5, False)]  # the shared leaf alone
    assert [lost(r) for r in by_graph[7]] == [False]                         # the childless rule still fires
    assert [(r[1], r[3], r[4]) for r in by_graph[9]] == [(4, 1, 2), (5, 0, 2)]  # goal 1 survives rule 2's loss
    assert 11 not in by_graph                                                # no sink goal: no hypothesis
    assert check_leaves(eng, hand, its, cond=0, masks=True, what="pre graphs") == [(2 * r, 0, 1, 1, 1) for r in its]


def test_hand_built_sets(eng, hand):
    def run(w):
        eng.load(hand)
        a = check_sets(eng, hand, 1, 1, [[3], [3, 5], [4, 6], [3, 4], [], [1], [0], [1, 2], [3, 3, 3], [5], [5]],
                       masks=True, what=f"two rules, {w}")
        b = check_sets(eng, hand, 3, 1, [[2], [3], [2, 3], []], masks=True, what=f"childless rule, {w}")
        c = check_sets(eng, hand, 4, 1, [[4], [5], [4, 5], [2], [0], [0, 1]], masks=True, what=f"two roots, {w}")
        d = check_sets(eng, hand, 5, 1, [[], [1], [0]], masks=True, what=f"no sink goal, {w}")
        e = check_sets(eng, hand, 0, 1, [[0], []], masks=True, what=f"lone goal, {w}")
        return a, b, c, d, e
    a, b, c, d, e = both_tiers(eng, run)
    G = 3
    assert a[0] == (G, NONE, 2, 0, 1)                 # one leaf: it and its rule
    assert a[1] == a[2] == (G, NONE, 5, 1, 1)         # one leaf of each rule: the goal dies
    assert a[3] == (G, NONE, 3, 0, 1)                 # both leaves of one rule
    assert a[4] == (G, NONE, 0, 0, 1)                 # F empty: nothing is dead
    assert a[5] == (G, NONE, 1, 0, 1) and a[6] == (G, NONE, 1, 1, 1)  # F a rule; F the root
    assert a[7] == (G, NONE, 3, 1, 1)
    assert a[8] == a[0] and a[9] == a[10]             # a node named twice counts once; two sets naming one node
    assert b[0] == (7, NONE, 1, 0, 1) and b[2] == (7, NONE, 4, 1, 1) and b[3][2] == 0
    assert c[0][3:] == (1, 2) and c[2][3:] == (2, 2) and c[5][3:] == (2, 2)
    assert d == [(11, NONE, 0, 0, 1), (11, NONE, 2, 1, 1), (11, NONE, 1, 1, 1)]
    assert e == [(1, NONE, 1, 1, 1), (1, NONE, 0, 0, 1)]


def test_a_goal_whose_child_is_a_goal(eng):
    # goal 0 <- goal 1 <- rule 2 <- leaf 3, and goal 0 <- rule 4 <- leaf 5: by kind alone, goal 0 dies iff goal 1
    # and rule 4 both do
    corpus = build([("ggrgrg", [(0, 1), (1, 2), (2, 3), (0, 4), (4, 5)])])
    gr = Graph(corpus, 1)
    assert gr.row([3])[0] == (1, NONE, 3, 0, 1) and gr.row([3, 5])[0] == (1, NONE, 6, 1, 1)
    assert gr.row([1])[0] == (1, NONE, 1, 0, 1) and gr.row([1, 4])[0] == (1, NONE, 3, 1, 1)
    with pytest.raises(E.NemoError) as ei:  # loadProv's count check refuses a goal -> goal edge
        eng.load(corpus)
    assert ei.value.code == 3


# ---- chunk edges ------------------------------------------------------------------------------------------------------
def star(n_leaves):
    """goal 0 <- rule 1 <- n leaves, and goal 0 <- rule 2 <- the first leaf: one sweep, every chunk size"""
    kinds = "grr" + "g" * n_leaves
    return kinds, [(0, 1), (0, 2), (2, 3)] + [(1, 3 + k) for k in range(n_leaves)]


@pytest.fixture(scope="module")
def stars():
    sizes = [1, 63, 64, 65, 129]
    return sizes, build([star(n) for n in sizes])


@pytest.mark.parametrize("k", range(5))
def test_chunk_edges(eng, stars, k):
    sizes, corpus = stars
    n = sizes[k]

    def run(w):
        eng.load(corpus)
        rows = check_leaves(eng, corpus, [k], masks=True, what=f"{n} leaves, {w}")
        assert len(rows) == n and rows[0][2:] == (4, 1, 1) and all(r[2:] == (2, 0, 1) for r in rows[1:])
        # sets mode with the same count: singletons of the leaves, from the last one down
        sets = [[2 + n - j] for j in range(n)]
        check_sets(eng, corpus, k, 1, sets, masks=(n <= 65), what=f"{n} sets, {w}")
        return rows
    both_tiers(eng, run)
    rows = check_leaves(eng, corpus, list(range(5)), what="all five graphs in one call")
    assert len(rows) == sum(sizes)


# ---- geometry ---------------------------------------------------------------------------------------------------------
def hub_goal(n=300):
    """goal 0 <- n rules, rule k <- its own leaf: the root dies only when every leaf does"""
    kinds = "g" + "r" * n + "g" * n
    return kinds, [(0, 1 + k) for k in range(n)] + [(1 + k, 1 + n + k) for k in range(n)]


def wide_level(n=600):
    """goal 0 <- rule 1 <- n leaves: a row and a level of n nodes; any leaf kills the root"""
    return "gr" + "g" * n, [(0, 1)] + [(1, 2 + k) for k in range(n)]


def chain(levels=300):
    """goal <- rule <- goal ... : `levels` Kahn levels, one node each, one leaf"""
    kinds = "".join("g" if i % 2 == 0 else "r" for i in range(levels - 1)) + "g"
    if levels % 2 == 0:  # the sink must be a goal: end rule <- goal
        kinds = kinds[:-2] + "rg"
    return kinds, [(i, i + 1) for i in range(levels - 1)]


@pytest.fixture(scope="module")
def geometry():
    return build([hub_goal(), wide_level(), chain(301)])


@pytest.mark.parametrize("k, name", [(0, "hub goal with 300 children"), (1, "a level of 600 nodes"),
                                     (2, "a chain 301 levels deep")])
def test_geometry(eng, geometry, k, name):
    gr = Graph(geometry, 2 * k + 1)

    def run(w):
        eng.load(geometry)
        rows = check_leaves(eng, geometry, [k], masks=(k == 2), what=f"{name}, {w}", graphs={gr.g: gr})
        if k == 0:  # every leaf, all but one, half: the AND over the 300-children row
            sets = [gr.leaves, gr.leaves[:-1], gr.leaves[1:], gr.leaves[::2], [1 + j for j in range(300)], [7]]
            sets += [gr.leaves[:j] for j in (31, 32, 33, 64, 65)]
            srows = check_sets(eng, geometry, k, 1, sets, masks=True, what=f"{name}, sets, {w}", graph=gr)
            assert srows[0][2:] == (601, 1, 1) and srows[1][2:] == (598, 0, 1) and srows[4][2:] == (301, 1, 1)
        if k == 1:
            sets = [gr.leaves[3:5], [1], [], gr.leaves]
            check_sets(eng, geometry, k, 1, sets, masks=True, what=f"{name}, sets, {w}", graph=gr)
        return rows
    rows = both_tiers(eng, run)
    if k == 0:
        assert len(rows) == 300 and all(r[2:] == (2, 0, 1) for r in rows)
    if k == 1:
        assert len(rows) == 600 and all(r[2:] == (3, 1, 1) for r in rows)
    if k == 2:
        assert rows == [(5, 300, 301, 1, 1)]


# ---- random small corpora ------------------------------------------------------------------------------------------------
def some_sets(rng, gr, n):
    """n hypotheses on a graph: singletons, pairs, larger sets with repeats, rules, the roots, the empty set"""
    out = [[], list(gr.roots), list(range(gr.V))]
    while len(out) < n and gr.V:
        size = int(rng.integers(1, 6))
        out.append([int(x) for x in rng.integers(0, gr.V, size)])
    return out[:n]


@pytest.mark.parametrize("seed", range(5))
def test_random_corpora(eng, seed):
    corpus = random_corpus(9000 + 17 * seed, n_runs=5, max_nodes=40)[0]
    its = [int(x) for x in corpus.iteration]
    rng = np.random.default_rng(seed)
    graphs = {}
    n_rows = 0
    try:
        for lds in (-1, 0):
            eng.set_option("knock_lds_max", lds)
            eng.load(corpus)
            for masks in (False, True):
                for cond in (0, 1):
                    n_rows += len(check_leaves(eng, corpus, its + its[:2], cond, masks, f"seed {seed} lds {lds} cond {cond}",
                                               graphs))
                    gr = graphs[2 * corpus.run_index(its[seed % len(its)]) + cond]
                    check_sets(eng, corpus, its[seed % len(its)], cond, some_sets(rng, gr, 70), masks,
                               f"seed {seed} lds {lds} cond {cond} sets", gr)
    finally:
        eng.set_option("knock_lds_max", -1)
    assert n_rows > 0


# ---- device against device ------------------------------------------------------------------------------------------------
def test_singleton_sets_equal_leaves_and_unions(eng):
    corpus = random_corpus(4711, n_runs=4, max_nodes=60)[0]
    its = [int(x) for x in corpus.iteration]
    eng.load(corpus)
    leaves = eng.knockout_leaves(its, 1).copy()
    first, count = eng.knockout_ranges()
    seen = 0
    for i, it in enumerate(its):
        part = leaves[int(first[i]):int(first[i]) + int(count[i])]
        nodes = [int(x) for x in part["node"]]
        if not nodes:
            continue
        sets = eng.knockout_sets(it, 1, [[v] for v in nodes], masks=True)
        for f in ("graph", "n_dead", "roots_dead", "n_roots"):
            assert np.array_equal(sets[f], part[f]), (it, f)
        V = corpus.graph_size(2 * corpus.run_index(it) + 1)
        single = [eng.knockout_mask(h, V) for h in range(len(nodes))]
        pairs = [(a, b) for a in range(len(nodes)) for b in range(a + 1, len(nodes))][:40]
        if not pairs:
            continue
        both = eng.knockout_sets(it, 1, [[nodes[a], nodes[b]] for a, b in pairs], masks=True)
        for h, (a, b) in enumerate(pairs):
            m = eng.knockout_mask(h, V)
            assert not ((single[a] | single[b]) & ~m).any(), "the union of two sets is dead wherever either is"
            assert int(both[h]["n_dead"]) == int(m.sum())
            seen += 1
    assert seen > 0


# ---- the C3 shape ------------------------------------------------------------------------------------------------------------
def test_c3_shape_behind_a_deferred_pass(eng):
    from tests.test_gpu_dedup_consumers import bench_step, replicate_launches
    from nemo_amd.corpus import DIFF_PER_RUN
    corpus, _ = synth.generate(12, p_fault=0.55, prepend_run0=True, **synth.CONFIGS["c3"])
    its = [int(x) for x in corpus.iteration]
    eng.load(corpus)
    try:
        for k in range(3):  # the third step leaves k_build's slices of the duplicate graphs to ensure_whole
            if k == 2:
                eng.set_timing(True)
                eng.reset_timings()
            bench_step(eng, corpus, DIFF_PER_RUN, k == 0)
        before = replicate_launches(eng)
        graphs = {}
        rows = check_leaves(eng, corpus, its, 1, what="c3, 12 runs", graphs=graphs, sample=197)
        assert replicate_launches(eng) == before + 1, "the call must bring the deferred slices first"
    finally:
        eng.set_timing(False)
    first, count = eng.knockout_ranges()
    by_content, dups = {}, 0
    for i, it in enumerate(its):  # duplicate graphs give identical rows (but for the graph id)
        g = 2 * corpus.run_index(it) + 1
        n0, n1, e0, e1 = (int(corpus.node_off[g]), int(corpus.node_off[g + 1]), int(corpus.edge_off[g]),
                          int(corpus.edge_off[g + 1]))
        key = (corpus.node_word[n0:n1].tobytes(), corpus.label[n0:n1].tobytes(), corpus.edge_src[e0:e1].tobytes(),
               corpus.edge_dst[e0:e1].tobytes())
        part = [r[1:] for r in rows[int(first[i]):int(first[i]) + int(count[i])]]
        if key in by_content:
            dups += 1
            assert part == by_content[key]
        by_content[key] = part
    assert dups > 0, "the corpus must hold duplicate post graphs"
    assert len(rows) > 12 * 64, "several chunks per graph"


# ---- a post graph of >= 65536 nodes: u32 rows, the global tier by size ------------------------------------------------------
def test_graph_past_65535_nodes(eng):
    corpus, _ = synth.generate(3, target_nodes=140000, p_fault=0.9, prepend_run0=True, seed=3, eot=80, body_extra=6,
                               nval=3, nloc=4)
    r = max(range(corpus.n_runs), key=lambda x: corpus.graph_size(2 * x + 1))
    gr = Graph(corpus, 2 * r + 1)
    assert gr.V >= 65536
    rng = np.random.default_rng(5)
    pick = [gr.leaves[int(x)] for x in rng.integers(0, len(gr.leaves), 30)]
    sets = [[v] for v in pick[:24]] + [pick[24:27], pick[27:], [], [int(rng.integers(0, gr.V))]]
    rules = [v for v in range(gr.V) if gr.rule[v]]
    sets += [[rules[len(rules) // 2]], [gr.V - 1, 0]]
    eng.load(corpus)
    rows = check_sets(eng, corpus, int(corpus.iteration[r]), 1, sets, what="66k nodes", graph=gr, sample=9)
    check_sets(eng, corpus, int(corpus.iteration[r]), 1, sets[27:30], masks=True, what="66k nodes, masks", graph=gr)
    assert any(x[2] > 1 for x in rows)


# ---- protocol -------------------------------------------------------------------------------------------------------------------
def test_protocol(eng, hand, stars):
    eng.load(hand)
    assert len(eng.knockout_leaves([], 1)) == 0 and len(eng.knockout_sets(1, 1, [])) == 0  # zero hypotheses
    check_leaves(eng, hand, [1, 1, 2, 1], what="duplicate iterations")
    for call in (lambda: eng.knockout_leaves([1, 4242], 1), lambda: eng.knockout_sets(4242, 1, [[0]])):
        with pytest.raises(E.NemoError) as ei:
            call()
        assert ei.value.code == 7 and "unknown run iteration 4242" in ei.value.msg
        assert eng.L.nemo_fetch_knockout(eng.h, None, 0, None) == 5  # the failed call left no result
    with pytest.raises(E.NemoError) as ei:  # node 7 of the 7-node graph
        eng.knockout_sets(1, 1, [[0], [3, 7]])
    assert ei.value.code == 1 and "out of range" in ei.value.msg
    with pytest.raises(E.NemoError) as ei:
        eng.knockout_sets_raw(1, 1, np.array([0, 2, 1, 3], np.uint64), np.array([0, 1, 2], np.uint32), 3)
    assert ei.value.code == 1 and "set_off decreases" in ei.value.msg
    for bad_cond in (2, -1):
        with pytest.raises(E.NemoError) as ei:
            eng.knockout_leaves([1], bad_cond)
        assert ei.value.code == 1
    check_sets(eng, hand, 1, 1, [[3], [4]], masks=False)
    with pytest.raises(E.NemoError) as ei:  # a mask fetch without NEMO_KO_MASKS
        eng.knockout_mask(0, 7)
    assert ei.value.code == 5
    check_sets(eng, hand, 1, 1, [[3], [4]], masks=True)
    with pytest.raises(E.NemoError) as ei:
        eng.knockout_mask(2, 7)
    assert ei.value.code == 1
    # a reload between two calls: no result of the previous corpus survives, the next call is the new corpus'
    sizes, corpus = stars
    eng.load(corpus)
    assert eng.L.nemo_fetch_knockout(eng.h, None, 0, None) == 5
    with pytest.raises(E.NemoError):
        eng.knockout_mask(0, 4)
    check_leaves(eng, corpus, [1, 0], masks=True, what="after the reload")
    eng.load(hand)
    check_leaves(eng, hand, list(range(len(HAND))), masks=True, what="the first corpus again")


def test_node_context_refuses(hand):
    node = E.Engine(devices=[0])
    try:
        node.load(hand)
        for call in (lambda: node.knockout_leaves([1], 1), lambda: node.knockout_sets(1, 1, [[3]])):
            with pytest.raises(E.NemoError) as ei:
                call()
            assert ei.value.code == 5 and "single-device contexts only" in ei.value.msg
    finally:
        node.close()


def test_buffers_grow_and_are_reused(eng):
    corpus = build([star(130)])
    gr = Graph(corpus, 1)
    eng.load(corpus)
    for n in (3, 70, 1, 130, 70):
        check_sets(eng, corpus, 0, 1, [[3 + j] for j in range(n)], masks=(n != 70), what=f"{n} hypotheses", graph=gr)
    check_leaves(eng, corpus, [0], masks=True, what="130 leaves", graphs={1: gr})


def test_other_results_are_left_alone(eng):
    from tests import test_gpu_nearest as TN
    corpus = random_corpus(1000, n_runs=6, max_nodes=40)[0]
    its = [int(x) for x in corpus.iteration]
    f = corpus.failed_iters() or its[1:3]
    eng.load(corpus)
    eng.mark()

    def others():
        return (np.array(eng.diff_masks(len(f))).copy(), eng.missing().copy(), [m.copy() for m in eng.sdiff_masks()],
                eng.surplus().copy(), eng.label_distances().copy())

    def same(a, b):
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[3], b[3])
        assert len(a[2]) == len(b[2]) and all(np.array_equal(x, y) for x, y in zip(a[2], b[2]))
        assert np.array_equal(a[4], b[4])

    eng.diffprov(f, 1)
    eng.diffprov_symmetric(f)
    near = eng.nearest_runs(its, its).copy()
    before = others()
    rows = check_leaves(eng, corpus, its, masks=True, what="between the other calls")
    same(before, others())  # their fetches, unchanged by the knock-out between them
    eng.diffprov(f, 1)
    eng.diffprov_symmetric(f)
    assert np.array_equal(eng.nearest_runs(its, its), near)
    same(before, others())
    assert _rows(eng.knockout_rows()) == rows  # and the reverse
    TN.check(eng, TN.label_sets(corpus), its, its)
