"""GPU checks of nemo_lineage_repair_sets / nemo_lineage_repairs (k_lrep_lds and k_lrep_glob in
nemo_amd/csrc/k_lrepair.hip, with k_lineage.hip's k_lin_filter / k_lin_rehash and k_repair.hip's k_repair_absent): every
row, the row order, the status, |A|, the candidate list and all 18 level stats, exact, on both tiers.  There is no
reference code for these calls, so the reference is the header's definition in plain Python over the Corpus arrays, and
never calls the library:
  dead(gr, F)            dead_F, sinks first, by the node's own kind;
  blame(gr, F, dd)       the blocker B_F, roots first: a blamed node of F stops, a blamed rule blames its dead child of
                         smallest node index, a blamed goal every child;
  search(...)            the specified search, level by level: rows and stats;
  repairs_brute(...)     every S of up to max_size candidates evaluated, the holding sets with no holding proper subset.
search asserts the lemma's consequence on the way: under SEARCHED every evaluated non-repair has a candidate outside it in
its blocker (S = cand is a repair above it), so a frontier empties only through the filter."""
import ctypes
import itertools
import os

import numpy as np
import pytest

from nemo_amd import engine as E
from nemo_amd.corpus import load_molly
from tests.test_gpu_knockout import Graph, build

pytestmark = pytest.mark.gpu
NONE = 0xFFFFFFFF
HOLDS, SEARCHED, BEYOND = 0, 1, 2
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ZERO = [[0, 0] for _ in range(9)]


@pytest.fixture(scope="module")
def eng():
    e = E.Engine(0)
    yield e
    e.close()


# ---- the reference ----------------------------------------------------------------------------------------------
def order_of(gr):
    if not hasattr(gr, "topo"):
        gr.topo = sorted(range(gr.V), key=lambda v: gr.pos[v])  # parents first
        gr.rows = [sorted(c) for c in gr.ch]                    # the forward rows ascend
    return gr.topo


def dead(gr, F):
    """dead_F per node: a node of F; a rule with a dead child; a goal with children, all dead"""
    dd = [False] * gr.V
    for v in reversed(order_of(gr)):
        if v in F:
            dd[v] = True
        elif gr.rule[v]:
            dd[v] = any(dd[c] for c in gr.ch[v])
        else:
            dd[v] = bool(gr.ch[v]) and all(dd[c] for c in gr.ch[v])
    return dd


def lost(gr, dd):
    return bool(gr.roots) and all(dd[r] for r in gr.roots)


def blame(gr, F, dd):
    """B_F of a removed set under which the outcome is lost"""
    assert lost(gr, dd)
    bl = [False] * gr.V
    for r in gr.roots:
        bl[r] = True
    for v in order_of(gr):
        if not bl[v] or v in F:
            continue
        assert dd[v], "a blamed node is dead"
        if gr.rule[v]:
            bl[next(c for c in gr.rows[v] if dd[c])] = True
        else:
            assert gr.rows[v]
            for c in gr.rows[v]:
                bl[c] = True
    return {v for v in range(gr.V) if bl[v]}


def status_of(gr, A, cand):
    if not A or not gr.roots:
        return HOLDS
    if not lost(gr, dead(gr, set(A))):
        return HOLDS
    return BEYOND if lost(gr, dead(gr, set(A) - set(cand))) else SEARCHED


def colex(s):
    return (len(s), tuple(sorted(s, reverse=True)))


def rows_of(sets, cand):
    return [(len(s),) + tuple(cand[p] for p in sorted(s)) + (NONE,) * (8 - len(s)) for s in sorted(sets, key=colex)]


def search(gr, A, cand, max_size):
    """(status, |A|, rows, the 9 x 2 stats, the candidate list) by the specified search"""
    A = list(A)
    cand = list(A) if cand is None else list(cand)
    status = status_of(gr, A, cand)
    if status != SEARCHED:
        return status, len(A), [], ZERO, cand
    stats, repairs, sizes = [[0, 0] for _ in range(9)], set(), set()
    frontier = [frozenset()]
    for d in range(max_size + 1):
        stats[d][0] = len(frontier)
        kids, found = set(), []
        for S in frontier:
            F = set(A) - {cand[p] for p in S}
            dd = dead(gr, F)
            if not lost(gr, dd):
                found.append(S)
                continue
            B = blame(gr, F, dd)
            mine = [k for k, v in enumerate(cand) if v in B and k not in S]
            assert mine, "the lemma: a non-repair below the repair S = cand has a candidate in its blocker"
            if d < max_size:
                kids.update(S | {k} for k in mine)
        stats[d][1] = len(found)
        repairs.update(found)
        if found:
            sizes.add(d)
        if d == max_size:
            break
        frontier = [c for c in kids
                    if not any(frozenset(t) in repairs for k in sizes if 0 < k < len(c) for t in itertools.combinations(c, k))]
        if not frontier:
            break
    return status, len(A), rows_of(repairs, cand), stats, cand


def repairs_brute(gr, A, cand, max_size):
    """the minimal repairs of size <= max_size as sets of candidate positions, by the definition alone"""
    A = list(A)
    cand = list(A) if cand is None else list(cand)
    combos = [frozenset(c) for s in range(1, max_size + 1) for c in itertools.combinations(range(len(cand)), s)]
    rep = {c for c in combos if not lost(gr, dead(gr, set(A) - {cand[p] for p in c}))}
    return {c for c in rep if not any(frozenset(t) in rep for k in range(1, len(c)) for t in itertools.combinations(c, k))}


def expected(gr, A, cand, max_size, brute=False):
    want = search(gr, A, cand, max_size)
    if brute and want[0] == SEARCHED:
        assert want[2] == rows_of(repairs_brute(gr, A, cand, max_size), want[4]), f"the search and the definition differ on graph {gr.g}"
    return want


def got_rows(arr):
    assert arr.dtype == E.LINEAGE_REPAIR_DTYPE
    return [(int(r["size"]),) + tuple(int(x) for x in r["node"]) for r in arr]


def compare(eng, got, want, what):
    status, n_absent, rows, stats, cand = want
    g = got_rows(got)
    st = eng.lineage_repair_stats()
    print(f"{what}: status {st[0]}, |A| {st[1]}, {len(g)} rows, stats {st[2].tolist()}")
    assert st[0] == status, f"{what}: status {st[0]}, want {status}"
    assert len(g) == len(rows), f"{what}: {len(g)} rows, want {len(rows)}"
    bad = [k for k in range(len(rows)) if g[k] != rows[k]]
    assert not bad, f"{what}: rows {bad[:6]} differ: got {[g[k] for k in bad[:6]]}, want {[rows[k] for k in bad[:6]]}"
    assert st[1] == n_absent, f"{what}: |A| {st[1]}, want {n_absent}"
    assert st[2].tolist() == stats, f"{what}: stats {st[2].tolist()}, want {stats}"
    assert eng.lineage_repair_cands().tolist() == list(cand), f"{what}: the candidate list differs"
    assert got_rows(eng.lineage_repair_rows()) == g


def check(eng, corpus, it, A, cand, max_size, what="", graph=None, cond=1, want=None, brute=False):
    gr = graph or Graph(corpus, 2 * corpus.run_index(it) + cond)
    want = want or expected(gr, A, cand, max_size, brute)
    compare(eng, eng.lineage_repair_sets(it, cond, A, cand, max_size), want, what)
    return want


def tiers(eng, fn, grids=(0,)):
    """fn(what) on both tiers (wit_lds_max default and 0) and under every kl_grid of `grids`"""
    out = None
    try:
        for lds in (-1, 0):
            for grid in grids:
                eng.set_option("wit_lds_max", lds)
                eng.set_option("kl_grid", grid)
                out = fn(f"wit_lds_max {lds}, kl_grid {grid}")
    finally:
        eng.set_option("wit_lds_max", -1)
        eng.set_option("kl_grid", 0)
    return out


# ---- 1. all eight ------------------------------------------------------------------------------------------------------
def test_all_eight(eng):
    # root goal 0 <- rule 1 <- eight sink goals 2 .. 9, all absent: the rule blames its first dead child only
    corpus = build([("gr" + "g" * 8, [(0, 1)] + [(1, 2 + k) for k in range(8)])])
    A = list(range(2, 10))
    eng.load(corpus)

    def run(what):
        w = check(eng, corpus, 0, A, None, 8, f"all eight ({what})")
        assert w[0] == SEARCHED and w[2] == [(8,) + tuple(A)] and w[3] == [[1, 0]] * 8 + [[1, 1]]
        w = check(eng, corpus, 0, A, None, 7, f"max_size 7 ({what})")
        assert w[0] == SEARCHED and w[2] == [] and w[3] == [[1, 0]] * 8 + [[0, 0]]
        w = check(eng, corpus, 0, A, A[::-1], 8, f"in reverse candidate order ({what})")
        assert w[2] == [(8,) + tuple(A[::-1])]

    tiers(eng, run)


# ---- 2. product shapes ---------------------------------------------------------------------------------------------------
def product(w, m, extra=0):
    """P(w, m): root goal 0 <- rule 1 <- m goals, each <- w rules <- one sink each; w^m repairs of size m and a frontier
    of w^d sets at level d.  extra: a second rule under the root over `extra` sinks of its own.  Returns the graph
    and the sinks in node order."""
    kinds, edges, sinks = "gr", [(0, 1)], []
    for _ in range(m):
        top = len(kinds)
        kinds += "g" + "rg" * w
        edges.append((1, top))
        for k in range(w):
            edges += [(top, top + 1 + 2 * k), (top + 1 + 2 * k, top + 2 + 2 * k)]
            sinks.append(top + 2 + 2 * k)
    if extra:
        top = len(kinds)
        kinds += "r" + "g" * extra
        edges += [(0, top)] + [(top, top + 1 + k) for k in range(extra)]
        sinks += [top + 1 + k for k in range(extra)]
    return (kinds, edges), sinks


PRODUCTS = [(2, 7, "128 sets: whole chunks"), (4, 3, "64 sets: exactly one chunk"), (3, 5, "243 sets: a short last chunk")]


@pytest.mark.parametrize("w, m, name", PRODUCTS)
def test_product_shapes(eng, w, m, name):
    graph, sinks = product(w, m)
    corpus = build([graph])
    gr = Graph(corpus, 1)
    want = expected(gr, sinks, None, 8)
    assert want[0] == SEARCHED and len(want[2]) == w ** m and all(r[0] == m for r in want[2])
    assert want[3][:m + 1] == [[w ** d, 0] for d in range(m)] + [[w ** m, w ** m]] and want[3][m + 1:] == [[0, 0]] * (8 - m)
    eng.load(corpus)
    tiers(eng, lambda what: check(eng, corpus, 0, sinks, None, 8, f"P({w},{m}) {name} ({what})", gr, want=want))


def on_fresh_engines(corpus, A, max_size, want, what):
    """the call on an engine of its own per tier and under kl_grid 0 and 1: the emission buffer has not grown yet"""
    for lds in (-1, 0):
        for grid in (0, 1):
            fresh = E.Engine(0)
            try:
                fresh.set_option("wit_lds_max", lds)
                fresh.set_option("kl_grid", grid)
                fresh.load(corpus)
                compare(fresh, fresh.lineage_repair_sets(0, 1, A, None, max_size), want, f"{what} (wit_lds_max {lds}, kl_grid {grid})")
                assert len(fresh.lineage_repair_rows()) == len(want[2])  # not doubled
            finally:
                fresh.close()


def test_product_3_7_runs_a_level_again():
    """P(3,7): 2187 repairs from a frontier of 35 chunks, the last of 11 sets; level 6 emits 2187 children, past the
    first emission buffer of 1024, so it runs again behind a grown one.  Also under kl_grid 1."""
    graph, sinks = product(3, 7)
    corpus = build([graph])
    want = expected(Graph(corpus, 1), sinks, None, 7)
    assert len(want[2]) == 2187 and want[3][6] == [729, 0] and want[3][7] == [2187, 2187] and 2187 % 64 == 11
    on_fresh_engines(corpus, sinks, 7, want, "P(3,7)")


def test_a_level_that_finds_repairs_runs_again():
    """P(3,7) beside a rule over six sinks: level 6 finds the repair of the six while its 1093 sets emit 4372 children,
    past the first emission buffer: the level runs again and must not append that repair twice."""
    graph, sinks = product(3, 7, extra=6)
    corpus = build([graph])
    want = expected(Graph(corpus, 1), sinks, None, 7)
    assert want[3][6] == [1093, 1] and want[3][7][1] == 2187 and len(want[2]) == 2188
    on_fresh_engines(corpus, sinks, 7, want, "P(3,7) beside a rule of six")


# ---- 3. the stop rule and inner nodes --------------------------------------------------------------------------------------
# goal 0 <- rule 1 <- (goal 2 <- rule 3 <- leaf 4; leaf 5): an inner goal and a rule may be absent
INNER = ("grgrgg", [(0, 1), (1, 2), (1, 5), (2, 3), (3, 4)])
# goal 0 <- rule 1 <- (x 3, u 4); goal 0 <- rule 2 <- (y 5, v 6)
TWO_RULES = ("grrgggg", [(0, 1), (0, 2), (1, 3), (1, 4), (2, 5), (2, 6)])


def test_stop_rule_and_inner_nodes(eng):
    corpus = build([INNER, TWO_RULES])
    eng.load(corpus)

    def run(what):
        # an absent inner goal over an absent child: the child enters the frontier only after the goal is restored
        w = check(eng, corpus, 0, [2, 4], None, 8, f"inner goal over its leaf ({what})", brute=True)
        assert w[2] == [(2, 2, 4) + (NONE,) * 6] and w[3][:4] == [[1, 0], [1, 0], [1, 1], [0, 0]]
        w = check(eng, corpus, 0, [4, 2], None, 1, f"... max_size 1 ({what})")
        assert w[0] == SEARCHED and w[2] == [] and w[3][1] == [1, 0]  # the one set of level 1 is {goal 2}, not {leaf 4}
        # a restored rule that stays dead through its child
        w = check(eng, corpus, 0, [3, 4], None, 8, f"rule and leaf ({what})", brute=True)
        assert w[2] == [(2, 3, 4) + (NONE,) * 6] and w[3][:3] == [[1, 0], [1, 0], [1, 1]]
        w = check(eng, corpus, 0, [2, 3, 4, 5, 0, 1], None, 8, f"every node ({what})", brute=True)
        assert [r[0] for r in w[2]] == [6]
        # cand a strict subset of A
        w = check(eng, corpus, 1, [3, 4, 5], [4, 3], 8, f"a strict subset ({what})", brute=True)
        assert w[0] == SEARCHED and w[2] == [(2, 4, 3) + (NONE,) * 6]
        w = check(eng, corpus, 0, [2, 4, 5], [2, 4], 8, f"BEYOND ({what})")
        assert w[0] == BEYOND and w[2] == [] and w[3] == ZERO
        w = check(eng, corpus, 1, [3, 4, 5], [], 3, f"no candidate ({what})")
        assert w[0] == BEYOND and w[4] == []
        w = check(eng, corpus, 1, [3, 4], None, 8, f"HOLDS ({what})")
        assert w[0] == HOLDS and w[1] == 2 and w[3] == ZERO
        w = check(eng, corpus, 1, [], None, 8, f"nothing absent ({what})")
        assert w[0] == HOLDS and w[1] == 0
        # {x}'s blocker names the lost u and y; {y} is a repair, so {x, y} is filtered: the frontier empties at level 2
        w = check(eng, corpus, 1, [3, 4, 5], [3, 5], 8, f"the frontier empties before max_size ({what})", brute=True)
        assert w[2] == [(1, 5) + (NONE,) * 7] and w[3][:4] == [[1, 0], [2, 1], [0, 0], [0, 0]]
        # the pre graph (one goal): cond 0
        w = check(eng, corpus, 0, [0], None, 2, f"the pre graph ({what})", cond=0)
        assert w[2] == [(1, 0) + (NONE,) * 7]

    tiers(eng, run)


def test_a_goal_whose_child_is_a_goal():
    # goal 0 <- (goal 1 <- goal 3; goal 2): the load refuses a goal -> goal edge (tests/test_gpu_repairs.py), so the
    # model alone takes it, by kind: the search and the definition agree
    corpus = build([("gggg", [(0, 1), (0, 2), (1, 3)])])
    gr = Graph(corpus, 1)
    assert expected(gr, [1, 2, 3], None, 3, brute=True)[2] == [(1, 2) + (NONE,) * 7, (2, 1, 3) + (NONE,) * 6]


# ---- 4. hubs -----------------------------------------------------------------------------------------------------------
def test_hubs(eng):
    # a rule of 100 children whose first dead child is child 70: the second step of the wave scan
    rule_hub = ("gr" + "g" * 100, [(0, 1)] + [(1, 2 + k) for k in range(100)])
    # a goal of 100 rules, each over its own sink, all dead: the strided OR
    goal_hub = ("g" + "r" * 100 + "g" * 100, [(0, 1 + k) for k in range(100)] + [(1 + k, 101 + k) for k in range(100)])
    corpus = build([rule_hub, goal_hub])
    eng.load(corpus)

    def run(what):
        w = check(eng, corpus, 0, [2 + 90, 2 + 70, 2 + 99], None, 8, f"a rule of 100 children ({what})")
        assert w[2] == [(3, 92, 72, 101) + (NONE,) * 5] and w[3][:4] == [[1, 0], [1, 0], [1, 0], [1, 1]]
        w = check(eng, corpus, 1, list(range(101, 201)), None, 2, f"a goal of 100 dead rules ({what})")
        assert len(w[2]) == 100 and w[3][:3] == [[1, 0], [100, 100], [0, 0]]
        # ... with the first 40 rules absent as well: a rule in F stops, the others blame their sinks
        w = check(eng, corpus, 1, list(range(101, 201)) + list(range(1, 41)), None, 2, f"... 40 rules absent too ({what})")
        assert sum(1 for r in w[2] if r[0] == 1) == 60 and sum(1 for r in w[2] if r[0] == 2) == 40

    tiers(eng, run)


# ---- 5. random graphs -------------------------------------------------------------------------------------------------------
RANDOM_SEEDS = [0, 1, 2, 3, 5, 7, 8, 9, 12, 15, 24, 38]  # chosen on the CPU: the asserts at the end of the test


def random_case(seed):
    """alternating goal / rule layers under one or two roots, rows into deeper layers only; A: most sinks and a few
    inner nodes; cand: a subset of A in an order of its own"""
    rng = np.random.default_rng(1000 + seed)
    kinds, edges, layer = "", [], []
    for _ in range(int(rng.integers(1, 3))):
        layer.append(len(kinds))
        kinds += "g"
    goals = list(layer)
    for depth in range(3):
        rules = []
        for v in layer:
            for _ in range(int(rng.integers(1, 4)) if depth < 2 or rng.random() < 0.5 else 0):
                rules.append(len(kinds))
                edges.append((v, len(kinds)))
                kinds += "r"
        layer = []
        for r in rules:
            for _ in range(int(rng.integers(1, 4))):
                if layer and rng.random() < 0.25:
                    c = layer[int(rng.integers(len(layer)))]
                    if (r, c) in edges:
                        continue
                else:
                    c = len(kinds)
                    kinds += "g"
                    layer.append(c)
                edges.append((r, c))
        goals += layer
    corpus = build([(kinds, edges)])
    gr = Graph(corpus, 1)
    n_sink = int(rng.integers((2 * len(gr.leaves) + 2) // 3, len(gr.leaves) + 1))
    A = [gr.leaves[int(x)] for x in rng.choice(len(gr.leaves), n_sink, replace=False)]
    inner = [v for v in range(gr.V) if gr.ch[v] and v not in gr.roots]
    if inner:
        A += [inner[int(x)] for x in rng.choice(len(inner), min(len(inner), int(rng.integers(0, 3))), replace=False)]
    order = [A[int(x)] for x in rng.permutation(len(A))]
    cand = order[:int(rng.integers(max(1, len(A) - 2), len(A) + 1))]
    return corpus, gr, A, cand


def test_random_graphs(eng):
    big, statuses = 0, set()
    for seed in RANDOM_SEEDS:
        corpus, gr, A, cand = random_case(seed)
        want = expected(gr, A, cand, 6, brute=len(cand) <= 14)
        statuses.add(want[0])
        big += want[0] == SEARCHED and any(r[0] >= 4 for r in want[2])
        eng.load(corpus)
        tiers(eng, lambda what: check(eng, corpus, 0, A, cand, 6, f"seed {seed} ({what})", gr, want=want))
    assert big >= 6, f"only {big} SEARCHED cases with a row of size >= 4"
    assert statuses == {HOLDS, SEARCHED, BEYOND}, f"statuses {sorted(statuses)} only"


# ---- 6. device against device ----------------------------------------------------------------------------------------------
def exhaustive(eng, rows4):
    st = eng.min_repair_stats()
    rows = [tuple(int(x) for x in r) + (NONE,) * 5 for r in rows4.tolist()]
    return st[0], st[1], rows, st[3].tolist()


def lineage(eng, rows):
    st = eng.lineage_repair_stats()
    return st[0], st[1], got_rows(rows), eng.lineage_repair_cands().tolist()


def test_rows_of_the_exhaustive_call_on_its_chunk_edges(eng):
    from tests.test_gpu_repairs import MIXED, PAIR_LEAVES, TRIPLE_LEAVES, rules_of
    graphs = [rules_of(n // 2, 2) for n in PAIR_LEAVES] + [rules_of(n // 3, 3) for n in TRIPLE_LEAVES] + [MIXED]
    corpus = build([g for g, _ in graphs])
    eng.load(corpus)

    def run(what):
        for k, (_, leaves) in enumerate(graphs):
            for size in (1, 2, 3):
                if size == 3 and k < len(PAIR_LEAVES) - 1:
                    continue  # the pairs' graphs at size 3: one of them is enough
                ex = exhaustive(eng, eng.min_repair_sets(k, 1, leaves, None, size))
                li = lineage(eng, eng.lineage_repair_sets(k, 1, leaves, None, size))
                assert ex == li, f"graph {k}, max_size {size} ({what})"
                assert li[0] == SEARCHED
                if size == 3 or (size == 2 and k < len(PAIR_LEAVES)):
                    assert li[2], f"graph {k}, max_size {size}: no rows"
        ex = exhaustive(eng, eng.min_repair_sets(0, 1, graphs[0][1], graphs[0][1][:40][::-1], 2))
        assert ex == lineage(eng, eng.lineage_repair_sets(0, 1, graphs[0][1], graphs[0][1][:40][::-1], 2)) and ex[0] == SEARCHED

    tiers(eng, run)


CASE_STUDIES = [("cs_ca_2434_bootstrap_synchronization", [7, 20]), ("cs_mr_2995_failed_after_expiry", [13, 14])]


@pytest.mark.parametrize("CASE_STUDY, CASE_PAIRS", CASE_STUDIES)
def test_pair_form_case_study(eng, CASE_STUDY, CASE_PAIRS):
    from tests.test_gpu_repairs import absent_sinks
    corpus = load_molly(os.path.join(GOLDEN, CASE_STUDY))
    eng.load(corpus)
    eng.mark()
    models = {}
    for f in CASE_PAIRS:
        for base, other in ((0, f), (f, 0)):
            gr, A = absent_sinks(corpus, base, other)
            models[(base, other)] = (A, search(gr, A, None, 8))
    assert all(models[(0, f)][1][0] == SEARCHED and models[(0, f)][1][2] for f in CASE_PAIRS)

    def run(what):
        for (base, other), (A, want) in models.items():
            for size in (1, 2, 3):
                ex = exhaustive(eng, eng.min_repairs(base, other, size))
                li = lineage(eng, eng.lineage_repairs(base, other, size))
                assert ex == li and li[3] == A, f"{CASE_STUDY} ({base}, {other}) max_size {size} ({what})"
            compare(eng, eng.lineage_repairs(base, other, 8), want, f"{CASE_STUDY} ({base}, {other}) max_size 8 ({what})")
            compare(eng, eng.lineage_repair_sets(base, 1, A, None, 8), want, f"... the same lists by name ({what})")
        compare(eng, eng.lineage_repairs(CASE_PAIRS[0], CASE_PAIRS[0], 8), (HOLDS, 0, [], ZERO, []), f"(x, x) ({what})")

    tiers(eng, run)


# ---- 7. a post graph of >= 65536 nodes: u32 rows, the global tier by size ---------------------------------------------------
def test_graph_past_65535_nodes(eng):
    # P(2,3) whose rule 1 has 66000 present sinks before its three goals: the rule's scan passes 1032 steps of alive
    # children before it meets its first dead one
    fill = 66000
    kinds, edges, sinks = "gr" + "g" * fill, [(0, 1)] + [(1, 2 + k) for k in range(fill)], []
    for _ in range(3):
        top = len(kinds)
        kinds += "g" + "rg" * 2
        edges.append((1, top))
        for k in range(2):
            edges += [(top, top + 1 + 2 * k), (top + 1 + 2 * k, top + 2 + 2 * k)]
            sinks.append(top + 2 + 2 * k)
    corpus = build([(kinds, edges)])
    gr = Graph(corpus, 1)
    assert gr.V >= 65536
    A = sinks + [5, 70]  # two of the present sinks as well: they must come back too
    want = expected(gr, A, None, 5)
    assert want[0] == SEARCHED and len(want[2]) == 8 and all(r[0] == 5 for r in want[2])
    assert want[3][:3] == [[1, 0], [1, 0], [1, 0]]  # level 0 blames node 5 alone, the smallest index; then node 70
    eng.load(corpus)
    check(eng, corpus, 0, A, None, 5, "66k nodes", gr, want=want)
    w = check(eng, corpus, 0, A, sinks, 5, "66k nodes, two sinks stay lost", gr)
    assert w[0] == BEYOND


# ---- 8. protocol ------------------------------------------------------------------------------------------------------------
def last_error(eng):
    return eng.L.nemo_last_error(eng.h).decode()


def fetch_codes(eng):
    z = np.zeros(20, np.uint64)
    return (eng.L.nemo_fetch_lineage_repairs(eng.h, None, 0, None), eng.L.nemo_fetch_lineage_repair_stats(eng.h, z.ctypes.data),
            eng.L.nemo_fetch_lineage_repair_cands(eng.h, None, 0, None))


def test_children_limit(eng):
    graph, sinks = product(3, 5)
    corpus = build([graph])
    gr = Graph(corpus, 1)
    want = expected(gr, sinks, None, 5)
    eng.load(corpus)
    try:
        eng.set_option("lineage_children_max", 64)
        with pytest.raises(E.NemoError) as ei:  # level 3's 27 sets emit 81 children
            eng.lineage_repair_sets(0, 1, sinks, None, 5)
        assert ei.value.code == 6 and "lineage_children_max" in ei.value.msg and "level 3 emits 81 children" in ei.value.msg
        assert "nemo_lineage_repair_sets" in ei.value.msg
        assert fetch_codes(eng) == (5, 5, 5)  # and leaves no results
        eng.set_option("lineage_children_max", 243)  # level 4 emits exactly 243
        check(eng, corpus, 0, sinks, None, 5, "at the limit", gr, want=want)
    finally:
        eng.set_option("lineage_children_max", -1)


def test_protocol(eng):
    hand = build([TWO_RULES, INNER])
    fresh = E.Engine(0)
    try:
        with pytest.raises(E.NemoError) as ei:  # no corpus loaded
            fresh.lineage_repair_sets(0, 1, [3], None, 2)
        assert ei.value.code == 5
        with pytest.raises(E.NemoError) as ei:
            fresh.lineage_repairs(0, 1, 2)
        assert ei.value.code == 5
    finally:
        fresh.close()
    eng.load(hand)
    assert fetch_codes(eng) == (5, 5, 5)  # the fetches before any call
    a = np.array([3, 9, 3], np.uint32)  # the order of the checks: cond, then max_size / flags, then the lists
    assert eng.L.nemo_lineage_repair_sets(eng.h, 0, 2, a.ctypes.data, 3, None, 0, 9, 1) == 1 and "cond must be 0 (pre) or 1 (post)" in last_error(eng)
    assert eng.L.nemo_lineage_repair_sets(eng.h, 0, 1, a.ctypes.data, 3, None, 0, 9, 0) == 1 and "max_size must be 1..8" in last_error(eng)
    assert eng.L.nemo_lineage_repair_sets(eng.h, 0, 1, a.ctypes.data, 3, None, 0, 8, 1) == 1 and "max_size must be 1..8" in last_error(eng)
    assert eng.L.nemo_lineage_repair_sets(eng.h, 0, 1, a.ctypes.data, 3, None, 0, 0, 0) == 1 and "max_size must be 1..8" in last_error(eng)
    assert eng.L.nemo_lineage_repairs(eng.h, 0, 1, 9, 0) == 1 and "max_size must be 1..8" in last_error(eng)
    assert eng.L.nemo_lineage_repairs(eng.h, 0, 1, 2, 8) == 1 and "nemo_lineage_repairs: max_size must be 1..8" in last_error(eng)
    for absent, cand, text in (([3, 9, 3], [3, 3, 7], "absent node 1 is node 9, out of range (7 nodes)"),
                               ([3, 4, 5, 4], [3, 3, 6], "absent node 3 names node 4 a second time"),
                               ([3, 4, 5], [4, 3, 4, 6], "candidate 2 names node 4 a second time"),
                               ([3, 4, 5], [4, 6], "candidate 1 is node 6, which is not in the absent list"),
                               ([], [4], "candidate 0 is node 4, which is not in the absent list")):
        with pytest.raises(E.NemoError) as ei:
            eng.lineage_repair_sets(0, 1, absent, cand, 2)
        assert ei.value.code == 1 and "nemo_lineage_repair_sets: " + text in ei.value.msg, ei.value.msg
    with pytest.raises(E.NemoError) as ei:
        eng.lineage_repair_sets(4242, 1, [3], None, 2)
    assert ei.value.code == 7
    with pytest.raises(E.NemoError) as ei:  # the pair form needs what nemo_min_repairs needs
        eng.lineage_repairs(0, 1, 2)
    assert ei.value.code == 5 and "nemo_mark_holds" in ei.value.msg
    eng.mark()
    with pytest.raises(E.NemoError) as ei:
        eng.lineage_repairs(0, 4242, 2)
    assert ei.value.code == 7
    assert fetch_codes(eng) == (5, 5, 5)  # the failed calls left no result
    check(eng, hand, 0, [3, 4, 5], [3, 5], 8, "after the errors")
    n = ctypes.c_uint64()
    out = np.zeros(1, E.LINEAGE_REPAIR_DTYPE)
    assert eng.L.nemo_fetch_lineage_repairs(eng.h, None, 0, ctypes.byref(n)) == 0 and n.value == 1
    assert eng.L.nemo_fetch_lineage_repairs(eng.h, out.ctypes.data, 0, ctypes.byref(n)) == 1  # capacity too small
    with pytest.raises(E.NemoError):
        eng.lineage_repair_sets(0, 1, [3, 3], None, 2)
    assert fetch_codes(eng) == (5, 5, 5)  # a failed call voids the previous result
    check(eng, hand, 0, [3, 4, 5], [3, 5], 8, "before the reload")
    eng.load(hand)  # a reload: no result of the previous corpus survives
    assert fetch_codes(eng) == (5, 5, 5)
    # more than 65535 candidates: the explicit and the implicit list (70000 leaves under one rule)
    wide = build([("gr" + "g" * 70000, [(0, 1)] + [(1, 2 + k) for k in range(70000)])])
    eng.load(wide)
    leaves = list(range(2, 70002))
    for cand in (None, leaves[:65536]):
        with pytest.raises(E.NemoError) as ei:
            eng.lineage_repair_sets(0, 1, leaves, cand, 2)
        assert ei.value.code == 6 and "65535" in ei.value.msg and "eight u16 candidate positions" in ei.value.msg
    assert fetch_codes(eng) == (5, 5, 5)
    w = check(eng, wide, 0, leaves, leaves[:65535][::-1], 1, "65535 candidates of 70000 absent leaves")
    assert w[0] == BEYOND


def test_node_context_refuses():
    hand = build([TWO_RULES])
    node = E.Engine(devices=[0])
    try:
        node.load(hand)
        with pytest.raises(E.NemoError) as ei:
            node.lineage_repair_sets(0, 1, [3], None, 2)
        assert ei.value.code == 5 and "single-device contexts only" in ei.value.msg
        with pytest.raises(E.NemoError) as ei:
            node.lineage_repairs(0, 1, 2)
        assert ei.value.code == 5 and "single-device contexts only" in ei.value.msg
    finally:
        node.close()


def test_other_results_are_left_alone(eng):
    graph, sinks = product(2, 4)
    corpus = build([graph, TWO_RULES])
    gr = Graph(corpus, 1)
    eng.load(corpus)
    eng.mark()
    cuts, cut_stats = eng.lineage_cuts(0, 1, sinks, 4).copy(), eng.lineage_cut_stats().copy()
    reps = eng.min_repair_sets(0, 1, sinks, None, 3).copy()
    rep_stats = eng.min_repair_stats()
    assert len(cuts) == 4 and len(reps) == 0

    def exhaustive_unchanged(rows, stats, what):  # rows, status, |A|, the round stats and the candidate list
        st = eng.min_repair_stats()
        assert np.array_equal(eng.min_repair_rows(), rows) and st[:2] == stats[:2] and np.array_equal(st[2], stats[2]), what
        assert np.array_equal(st[3], stats[3]), f"{what}: the candidate list differs"

    want = check(eng, corpus, 0, sinks, None, 4, "between the other calls", gr)
    eng.lineage_repairs(1, 0, 2)
    check(eng, corpus, 1, [3, 4, 5], [3, 5], 8, "another graph")
    assert np.array_equal(eng.lineage_cut_rows(), cuts) and np.array_equal(eng.lineage_cut_stats(), cut_stats)
    exhaustive_unchanged(reps, rep_stats, "after the lineage repair calls")
    # and the reverse (compare reads the lineage calls' candidate list too)
    check(eng, corpus, 0, sinks, None, 4, "before the other calls", gr, want=want)
    eng.lineage_cuts(1, 1, None, 3)
    eng.min_repair_sets(1, 1, [3, 4], None, 2)
    eng.min_repairs(0, 1, 2)
    eng.min_cuts(0, 1, None, 2)
    compare(eng, eng.lineage_repair_rows(), want, "after the other calls")
    # the two pair forms against run 1, which is not run 0: each family fills a label table of its own.  Every label
    # of the corpus is distinct, so the absent set is every sink goal of the product graph, in node order
    compare(eng, eng.lineage_repairs(0, 1, 4), want, "the pair form")
    pair = eng.min_repairs(0, 1, 3).copy()
    pair_stats = eng.min_repair_stats()
    assert pair_stats[0] == SEARCHED and pair_stats[1] == len(sinks) and pair_stats[3].tolist() == sinks and len(pair) == 0
    compare(eng, eng.lineage_repair_rows(), want, "the pair form, after the exhaustive pair form")
    eng.lineage_repairs(0, 1, 2)  # the lineage family's table once more, another result
    assert len(eng.lineage_repair_rows()) == 0 and eng.lineage_repair_cands().tolist() == sinks
    exhaustive_unchanged(pair, pair_stats, "the exhaustive pair form, after the lineage pair form")
