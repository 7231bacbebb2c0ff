"""GPU checks of nemo_lineage_cuts (k_lin_lds, k_lin_glob and k_lin_filter in nemo_amd/csrc/k_lineage.hip): every row,
the row order and the per-level statistics, exact.

Reference.  include/nemohip.h fixes the semantics; the reference is that definition in plain Python over the Corpus
arrays: `dead` (sinks first), `witness` (roots first: a needed rule needs every child, a needed goal its alive child of
smallest node index), `search` (the level search as the header states it, which gives rows and stats) and `cuts_brute`
(every candidate subset up to max_size, then minimised: the result as the header defines it, without the search).
Where nemo_min_cuts covers the same ground (sizes 1..3) its rows are compared too, device against device.  None of
the models calls the library.
"""
import itertools

import numpy as np
import pytest

from nemo_amd import engine as E
from tests.test_gpu_knockout import Graph, build
from tests.test_gpu_min_cuts import GEN_SEEDS, HAND, INNER, chains, cuts_brute, fault_tree, hub, level
from tools import synth

pytestmark = pytest.mark.gpu
NONE = 0xFFFFFFFF


@pytest.fixture(scope="module")
def eng():
    e = E.Engine(0)
    yield e
    e.close()


# ---- the reference ----------------------------------------------------------------------------------------------
def dead(gr, F):
    """the nodes dead under F, by the definition"""
    return gr.dead_by_definition(F)


def witness(gr, F):
    """nemo_witness_sets' single derivation under F: the set W_F (empty if every root is dead)"""
    D = dead(gr, F)
    need = {r for r in gr.roots if r not in D}
    for v in sorted(range(gr.V), key=lambda x: gr.pos[x]):
        if v not in need:
            continue
        if gr.rule[v]:
            need.update(gr.ch[v])
        else:
            alive = sorted(c for c in gr.ch[v] if c not in D)
            if alive:
                need.add(alive[0])
    return need


def colex(s):
    return (len(s),) + tuple(sorted(s, reverse=True))


def rows_of(cuts, cand):
    return [(len(s),) + tuple(cand[p] for p in sorted(s)) for s in sorted(cuts, key=colex)]


def search(gr, cand, max_size):
    """the level search of the header: (rows, stats [9][2])"""
    stats = [[0, 0] for _ in range(9)]
    if not gr.roots or not len(cand):
        return [], stats
    where = {v: p for p, v in enumerate(cand)}
    front, cuts = [frozenset()], set()
    for d in range(max_size + 1):
        if not front:
            break
        stats[d][0] = len(front)
        kids = set()
        for F in front:
            D = dead(gr, [cand[p] for p in F])
            if all(r in D for r in gr.roots):
                cuts.add(F)
                stats[d][1] += 1
            elif d < max_size:
                kids.update(F | {where[e]} for e in witness(gr, [cand[p] for p in F]) if e in where)
        front = [k for k in kids if not any(frozenset(s) in cuts for n in range(1, len(k)) for s in itertools.combinations(k, n))]
    return rows_of(cuts, cand), stats


def got_rows(arr):
    out = []
    for r in arr:
        size, node = int(r["size"]), [int(x) for x in r["node"]]
        assert all(x == NONE for x in node[size:]), "unused entries are UINT32_MAX"
        out.append((size,) + tuple(node[:size]))
    return out


def both_tiers(eng, fn, grids=(0,)):
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


def check(eng, it, cand, max_size, rows, stats, what):
    got = eng.lineage_cuts(it, 1, cand, max_size)
    assert got.dtype == E.LINEAGE_CUT_DTYPE
    g = got_rows(got)
    assert g == rows, f"{what}: rows {g[:6]} ({len(g)}), want {rows[:6]} ({len(rows)})"
    if stats is not None:
        assert eng.lineage_cut_stats().tolist() == stats, f"{what}: stats {eng.lineage_cut_stats().tolist()}, want {stats}"


def min_cut_rows(eng, it, cand, max_size):
    """nemo_min_cuts' rows as (size, nodes...) and its hypotheses per round"""
    got = eng.min_cuts(it, 1, cand, max_size)
    rows = [(int(r["size"]),) + tuple(int(x) for x in r["node"][:int(r["size"])]) for r in got]
    return rows, [int(x) for x in eng.min_cut_stats()[:, 1]]


# ---- the graphs ---------------------------------------------------------------------------------------------------
# one root goal, eight rules, one sink goal each: the only cut is all eight sinks
EIGHT = ("g" + "r" * 8 + "g" * 8, [(0, 1 + k) for k in range(8)] + [(1 + k, 9 + k) for k in range(8)])


def and_of_ors(m, with_c=False):
    """root 0 <- rule 1 <- (c,) m goals; goal i <- two rules <- one sink each (a_i, b_i).  Node order: root, rule, c,
    the goals, the rule pairs, the sink pairs: c is the candidate of smallest node index, a_i comes before b_i."""
    c = [2] if with_c else []
    g0 = 2 + len(c)
    r0, s0 = g0 + m, g0 + 3 * m
    kinds = "gr" + "g" * len(c) + "g" * m + "r" * (2 * m) + "g" * (2 * m)
    edges = [(0, 1)] + [(1, x) for x in c] + [(1, g0 + i) for i in range(m)]
    for i in range(m):
        edges += [(g0 + i, r0 + 2 * i), (g0 + i, r0 + 2 * i + 1), (r0 + 2 * i, s0 + 2 * i), (r0 + 2 * i + 1, s0 + 2 * i + 1)]
    return kinds, edges, c + list(range(s0, s0 + 2 * m))


# ---- 1. beyond size 3 -----------------------------------------------------------------------------------------------
def test_beyond_size_three(eng):
    corpus = build([EIGHT])
    eng.load(corpus)
    sinks = list(range(9, 17))

    def run(w):
        full = [[1, 0]] * 8 + [[1, 1]]
        check(eng, 0, None, 8, [(8,) + tuple(sinks)], full, f"max_size 8, {w}")
        check(eng, 0, sinks, 8, [(8,) + tuple(sinks)], full, f"the explicit list, {w}")
        check(eng, 0, None, 7, [], [[1, 0]] * 8 + [[0, 0]], f"max_size 7, {w}")
    both_tiers(eng, run)
    assert len(eng.min_cuts(0, 1, None, 3)) == 0  # the exhaustive search stops at size 3
    assert search(Graph(corpus, 1), sinks, 8) == ([(8,) + tuple(sinks)], [[1, 0]] * 8 + [[1, 1]])


# ---- 2. equal to the exhaustive search ---------------------------------------------------------------------------------
def test_equal_to_min_cuts(eng):
    posts = HAND + [fault_tree(s) for s in GEN_SEEDS]
    corpus = build(posts)
    graphs = [Graph(corpus, 2 * k + 1) for k in range(len(posts))]
    lists = [[3, 4, 5], [4, 5], [4, 5, 6, 7], [1, 2, 3, 4, 5, 6, 7, 8]] + [gr.leaves[:24] for gr in graphs[len(HAND):]]
    eng.load(corpus)
    seen = 0
    for k, cand in enumerate(lists):
        for size in (1, 2, 3):
            want, hyps = min_cut_rows(eng, k, cand, size)
            model = search(graphs[k], cand, size)
            assert model[0] == want, f"graph {k}, size {size}: the model and nemo_min_cuts differ"

            def run(w):
                check(eng, k, cand, size, want, model[1], f"graph {k}, max_size {size}, {w}")
                st = eng.lineage_cut_stats()[:, 0].tolist()
                assert all(st[s] <= hyps[s - 1] for s in range(1, size + 1)), f"graph {k}: {st} sets against {hyps} hypotheses"
            both_tiers(eng, run)
            seen += len(want)
    assert seen > 30
    for k in (2, 4):  # cand NULL: every sink goal in node-index order
        check(eng, k, None, 3, min_cut_rows(eng, k, None, 3)[0], None, f"graph {k}, cand NULL")


# ---- 3. sizes 4 and 5 against brute force ------------------------------------------------------------------------------
def test_sizes_four_and_five(eng):
    posts = [fault_tree(s) for s in GEN_SEEDS] + [EIGHT]
    corpus = build(posts)
    eng.load(corpus)
    big = 0
    for k in range(len(posts)):
        gr = Graph(corpus, 2 * k + 1)
        cand = gr.leaves[:16]
        for size in (4, 5):
            brute = rows_of(cuts_brute(gr, cand, size), cand)
            rows, stats = search(gr, cand, size)
            assert rows == brute, f"graph {k}, size {size}: the search and brute force differ"
            big += sum(1 for r in rows if r[0] >= 4)
            both_tiers(eng, lambda w: check(eng, k, cand, size, brute, stats, f"graph {k}, max_size {size}, {w}"))
    assert big >= 1, "some minimal cut of size >= 4"


# ---- 4. stats equal the model: the 64-set chunk edge, duplicates counted once -----------------------------------------
@pytest.mark.parametrize("m", [63, 64, 65, 129])
def test_and_of_ors_stats(eng, m):
    kinds, edges, sinks = and_of_ors(m)
    corpus = build([(kinds, edges)])
    eng.load(corpus)
    rows = [(2, sinks[2 * i], sinks[2 * i + 1]) for i in range(m)]
    stats = [[1, 0], [m, 0], [m + m * (m - 1) // 2, m]] + [[0, 0]] * 6
    if m == 63:
        assert search(Graph(corpus, 1), sinks, 2) == (rows, stats)
    both_tiers(eng, lambda w: check(eng, 0, None, 2, rows, stats, f"m = {m}, {w}"), grids=(0, 1))


# ---- 5. the subset filter ---------------------------------------------------------------------------------------------------
def test_subset_filter(eng):
    kinds, edges, cand = and_of_ors(8, with_c=True)
    corpus = build([(kinds, edges)])
    gr = Graph(corpus, 1)
    assert cand[0] == 2 == min(cand) and gr.leaves == cand
    rows, stats = search(gr, cand, 3)
    assert rows[0] == (1, 2) and not any(2 in r[1:] for r in rows[1:])
    # level 1: {c} and the eight {a_i}; level 2: {a_i, b_i} and {a_i, a_j}, no {a_i, c}; level 3: the 56 {a_i, a_j, a_k}
    assert stats == [[1, 0], [9, 1], [8 + 28, 8], [56, 0]] + [[0, 0]] * 5, "no superset of {c} is evaluated"
    eng.load(corpus)
    both_tiers(eng, lambda w: check(eng, 0, None, 3, rows, stats, f"c in every witness, {w}"))


# ---- 6. inner candidates, hubs, a deep chain -----------------------------------------------------------------------------
def test_inner_candidates_and_sweep_edges(eng):
    shapes = [hub(), level(), chains()]
    corpus = build([INNER] + [s[:2] for s in shapes])
    eng.load(corpus)
    gr = Graph(corpus, 1)
    cand = [5, 6, 4, 7, 8]  # the two rules under goal 3, and sinks elsewhere
    want = rows_of(cuts_brute(gr, cand, 3), cand)
    assert (3, 5, 6, 4) in want
    both_tiers(eng, lambda w: check(eng, 0, cand, 3, want, search(gr, cand, 3)[1], f"rules as candidates, {w}"))
    for k, name in ((1, "a goal hub of 300 children"), (2, "a rule hub of 300 children"), (3, "301 levels")):
        gk = Graph(corpus, 2 * k + 1)
        ck = shapes[k - 1][2]
        wk = rows_of(cuts_brute(gk, ck, 2), ck)
        assert len(wk) >= 1
        both_tiers(eng, lambda w: check(eng, k, ck, 2, wk, search(gk, ck, 2)[1], f"{name}, {w}"), grids=(0, 1))


# ---- 7. geometry ---------------------------------------------------------------------------------------------------------
def test_graph_past_65535_nodes(eng):
    corpus, _ = synth.generate(3, target_nodes=140000, p_fault=0.9, prepend_run0=True, seed=3, eot=80, body_extra=6,
                               nval=3, nloc=4)
    r = max(range(corpus.n_runs), key=lambda x: corpus.graph_size(2 * x + 1))
    gr = Graph(corpus, 2 * r + 1)
    assert gr.V >= 65536
    rng = np.random.default_rng(5)
    cand = [gr.leaves[int(x)] for x in rng.choice(len(gr.leaves), 40, replace=False)]
    eng.load(corpus)
    it = int(corpus.iteration[r])
    want, hyps = min_cut_rows(eng, it, cand, 3)
    check(eng, it, cand, 3, want, None, "70k nodes")
    st = eng.lineage_cut_stats()[:, 0].tolist()
    assert st[0] == 1 and all(st[s] <= hyps[s - 1] for s in (1, 2, 3))


def test_c3_shape_all_sink_goals(eng):
    corpus, _ = synth.generate(12, p_fault=0.55, prepend_run0=True, **synth.CONFIGS["c3"])
    it = int(corpus.iteration[0])
    eng.load(corpus)
    want, hyps = min_cut_rows(eng, it, None, 2)

    def run(w):
        check(eng, it, None, 2, want, None, f"c3, {w}")
        st = eng.lineage_cut_stats()[:, 0].tolist()
        assert st[0] == 1 and 0 < st[1] <= hyps[0] and st[2] <= hyps[1], f"{w}: {st} against {hyps}"
    both_tiers(eng, run)


# ---- 8. the emission limit ------------------------------------------------------------------------------------------------
def test_emission_limit_and_regrow():
    kinds, edges, sinks = and_of_ors(129)
    corpus = build([(kinds, edges)])
    rows = [(2, sinks[2 * i], sinks[2 * i + 1]) for i in range(129)]
    e = E.Engine(0)  # a fresh context: the emission buffer has not grown yet
    try:
        e.load(corpus)
        e.set_option("lineage_children_max", 64)
        with pytest.raises(E.NemoError) as ei:
            e.lineage_cuts(0, 1, None, 2)
        assert ei.value.code == 6 and "lineage_children_max" in ei.value.msg and "129 children" in ei.value.msg
        assert e.L.nemo_fetch_lineage_cuts(e.h, None, 0, None) == 5
        assert e.L.nemo_fetch_lineage_cut_stats(e.h, np.zeros(18, np.uint64).ctypes.data) == 5
        e.set_option("lineage_children_max", 65536)  # level 1 emits 129 * 129 children: past the first buffer
        assert got_rows(e.lineage_cuts(0, 1, None, 2)) == rows
        assert e.lineage_cut_stats().tolist()[:3] == [[1, 0], [129, 0], [129 + 129 * 128 // 2, 129]]
        assert got_rows(e.lineage_cuts(0, 1, None, 2)) == rows  # and again, behind the grown buffer
        with pytest.raises(E.NemoError) as ei:
            e.set_option("lineage_children_max", 63)
        assert ei.value.code == 1
        e.set_option("lineage_children_max", -1)
        assert got_rows(e.lineage_cuts(0, 1, None, 2)) == rows
    finally:
        e.close()


# ---- 9. protocol ------------------------------------------------------------------------------------------------------------
def test_protocol(eng):
    corpus = build(HAND + [("", [])])
    eng.load(corpus)
    assert eng.L.nemo_fetch_lineage_cuts(eng.h, None, 0, None) == 5  # a fetch before any call
    assert eng.L.nemo_fetch_lineage_cut_stats(eng.h, np.zeros(18, np.uint64).ctypes.data) == 5
    for bad in (0, 9, 0xFFFFFFFF):
        with pytest.raises(E.NemoError) as ei:
            eng.lineage_cuts(0, 1, [3, 4], bad)
        assert ei.value.code == 1 and "max_size must be 1..8" in ei.value.msg
    cand = np.array([3, 4], np.uint32)
    assert eng.L.nemo_lineage_cuts(eng.h, 0, 1, cand.ctypes.data, 2, 2, 1) == 1  # flags
    assert "max_size must be 1..8" in eng.L.nemo_last_error(eng.h).decode()
    for args, code, text in (((0, 1, [3, 4, 3], 2), 1, "second time"), ((0, 1, [3, 6], 2), 1, "out of range"),
                             ((0, 1, [0] * 65536, 2), 6, "65535"), ((4242, 1, [3], 2), 7, ""), ((0, 2, [3], 2), 1, "cond")):
        with pytest.raises(E.NemoError) as ei:
            eng.lineage_cuts(*args)
        assert ei.value.code == code and text in ei.value.msg, args[:2]
    assert eng.L.nemo_fetch_lineage_cuts(eng.h, None, 0, None) == 5  # the failed calls left no result
    assert len(eng.lineage_cuts(0, 1, [], 3)) == 0 and eng.lineage_cut_stats().tolist() == [[0, 0]] * 9
    assert len(eng.lineage_cuts(len(HAND), 1, None, 3)) == 0 and eng.lineage_cut_stats().tolist() == [[0, 0]] * 9  # no root
    assert got_rows(eng.lineage_cuts(0, 1, [3, 4, 5], 3)) == [(1, 3), (2, 4, 5)]
    assert got_rows(eng.lineage_cuts(3, 1, [4, 3], 2)) == [(2, 4, 3)]  # list order, not node order
    none = search(Graph(corpus, 7), [7], 3)
    assert none == ([], [[1, 0], [1, 0]] + [[0, 0]] * 7)  # no cut at all: zero rows, the stats of the sets evaluated
    assert got_rows(eng.lineage_cuts(3, 1, [7], 3)) == [] and eng.lineage_cut_stats().tolist() == none[1]
    eng.load(build([EIGHT]))  # a reload: no result of the previous corpus survives
    assert eng.L.nemo_fetch_lineage_cuts(eng.h, None, 0, None) == 5


def test_node_context_refuses():
    node = E.Engine(devices=[0])
    try:
        node.load(build(HAND))
        with pytest.raises(E.NemoError) as ei:
            node.lineage_cuts(0, 1, [3], 2)
        assert ei.value.code == 5 and "single-device contexts only" in ei.value.msg
    finally:
        node.close()


def test_other_results_are_left_alone_and_buffers_reused(eng):
    posts = [and_of_ors(m)[:2] for m in (3, 70, 1, 130, 70)] + [fault_tree(GEN_SEEDS[0])]
    corpus = build(posts)
    eng.load(corpus)
    gr = Graph(corpus, 11)
    sets = [[v] for v in gr.leaves[:5]] + [gr.leaves[:3]]

    def others():
        return eng.min_cut_rows().copy(), eng.witness_rows().copy(), eng.knockout_rows().copy()

    eng.min_cuts(5, 1, None, 3)
    eng.witness_sets(5, 1, sets)
    eng.knockout_sets(5, 1, sets)
    before = others()
    for k, m in enumerate((3, 70, 1, 130, 70)):  # two calls in a row on different graphs: the buffers grow and are reused
        sinks = and_of_ors(m)[2]
        check(eng, k, None, 2, [(2, sinks[2 * i], sinks[2 * i + 1]) for i in range(m)],
              [[1, 0], [m, 0], [m + m * (m - 1) // 2, m]] + [[0, 0]] * 6, f"m = {m}")
    after = others()
    assert all(np.array_equal(a, b) for a, b in zip(before, after))
    last = got_rows(eng.lineage_cut_rows())
    eng.min_cuts(5, 1, None, 3)
    eng.witness_sets(5, 1, sets)
    eng.knockout_sets(5, 1, sets)
    assert got_rows(eng.lineage_cut_rows()) == last  # and the reverse
