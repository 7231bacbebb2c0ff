"""GPU checks of nemo_lineage_group_cuts (k_lgc_lds, k_lgc_glob and k_lgc_cuts in nemo_amd/csrc/k_lgcuts.hip, with
k_gcuts.hip's table kernels and k_lineage.hip's filter): every row, every n_lost, the row order and the per-level
statistics, exact.

Reference.  include/nemohip.h fixes the semantics; the reference is that definition in plain Python and never calls the
library.  `brute` enumerates every subset of size <= max_size of the candidate positions, gives the unions of their
groups to Ref.words of tests/test_gpu_knockout_labels.py (lost per (graph, set), in two forms that must agree), counts
list positions, applies q, keeps the subsets none of whose proper subsets is a cut and orders them by (size, colex order
of the positions).  `model` is the level search as the header states it, with the witness by the definition (a needed
rule needs every child, a needed goal its alive child of smallest node index): it gives the rows, the per-level stats
and the children counted per level.  Where nemo_min_group_cuts covers the same ground (sizes 1..3) its rows and n_lost
are compared too, device against device.

Every case runs on both tiers (wit_lds_max default and 0) and under kl_grid 0, 1 and 3.
"""
import ctypes
import itertools
import json
import os

import numpy as np
import pytest

from nemo_amd import engine as E
from nemo_amd.corpus import load_molly
from nemo_amd.faults import fault_events
from tests.test_gpu_group_cuts import got_rows, union
from tests.test_gpu_knockout import Graph, build
from tests.test_gpu_knockout_labels import HAND, Ref, relabel
from tests.test_gpu_label_cuts import PA, PB
from tests.test_gpu_lineage import and_of_ors
from tests.test_gpu_min_cuts import fault_tree
from tools import synth

pytestmark = pytest.mark.gpu
GRIDS = (0, 1, 3)
NONE = 0xFFFFFFFF
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def eng():
    e = E.Engine(0)
    yield e
    e.close()


# ---- the reference ----------------------------------------------------------------------------------------------
def colex(c):
    return (len(c),) + tuple(sorted(c, reverse=True))


def brute(ref, iters, cond, groups, max_size, min_runs, sinks, sample=1):
    """(rows [(size, positions)], n_lost) by the definition: every subset, counted, minimised, ordered"""
    n, K = len(iters), len(groups)
    if not n or not K:
        return [], []
    q = min_runs or n
    subsets = [c for s in range(1, max_size + 1) for c in itertools.combinations(range(K), s)]
    sets = [union(groups, c) for c in subsets]
    count, memo = [0] * len(sets), {}
    for it in iters:  # a run listed twice is computed once and counts twice
        if it not in memo:
            memo[it] = ref.words(it, cond, sets, sinks, sample)[0]
        for s in range(len(sets)):
            count[s] += (memo[it] >> s) & 1
    cnt = dict(zip(subsets, count))
    found = [c for c in subsets if cnt[c] >= q and not any(cnt[x] >= q for s in range(1, len(c)) for x in itertools.combinations(c, s))]
    found.sort(key=colex)
    return [(len(c), tuple(c)) for c in found], [cnt[c] for c in found]


def evaluate(ref, gr, groups, by_label, F, sinks):
    """one set on one graph: (lost, the candidates some node of the witness names)"""
    dead = gr.dead_by_definition(ref.nodes(gr, union(groups, sorted(F)), sinks))
    alive = [r for r in gr.roots if r not in dead]
    if not gr.roots or not alive:
        return bool(gr.roots), set()
    need, todo = set(alive), list(alive)
    while todo:  # a needed rule needs every child, a needed goal its alive child of smallest node index
        v = todo.pop()
        if gr.rule[v]:
            nxt = gr.ch[v]
        else:
            nxt = sorted(c for c in gr.ch[v] if c not in dead)[:1]
        for c in nxt:
            if c not in need:
                need.add(c)
                todo.append(c)
    kids = set()
    for v in need:
        if not sinks or v in gr.sink:
            kids.update(by_label.get(gr.label[v], ()))
    assert not kids & set(F), "a candidate of the set is in its own witness"
    return False, kids


def model(ref, iters, cond, groups, max_size, min_runs, sinks):
    """the level search of the header: (rows, n_lost, stats [9][2], info)"""
    n, K = len(iters), len(groups)
    stats = [[0, 0] for _ in range(9)]
    info = {"kids": [], "cut_survived": 0}
    graphs = [ref.graph(2 * ref.corpus.run_index(it) + cond) for it in iters]
    if not n or not K or not any(g.roots for g in graphs):
        return [], [], stats, info
    q = min_runs or n
    by_label = {}
    for k, g in enumerate(groups):
        for lab in g:
            by_label.setdefault(int(lab), set()).add(k)
    front, cuts = [frozenset()], {}
    for d in range(max_size + 1):
        if not front:
            break
        stats[d][0] = len(front)
        kids, counted = set(), 0
        for F in front:
            lost, emitted, memo = 0, [], {}
            for it, gr in zip(iters, graphs):
                if it not in memo:
                    memo[it] = evaluate(ref, gr, groups, by_label, F, sinks)
                lost += memo[it][0]
                if not memo[it][0]:
                    emitted.append(memo[it][1])
            if lost >= q:
                cuts[F] = lost
                stats[d][1] += 1
                info["cut_survived"] += bool(emitted)
            if d < max_size:  # emitted from every position on which the set is not lost, cut or not
                counted += sum(len(e) for e in emitted)
                for e in emitted:
                    kids.update(F | {k} for k in e)
        info["kids"].append(counted if d < max_size else 0)
        front = [k for k in kids if not any(frozenset(s) in cuts for m in range(1, len(k)) for s in itertools.combinations(k, m))]
    order = sorted(cuts, key=colex)
    return [(len(c), tuple(sorted(c))) for c in order], [cuts[c] for c in order], stats, info


def compare(eng, iters, cond, groups, max_size, min_runs, sinks, want, what, against_exhaustive=True):
    rows, n_lost = eng.lineage_group_cuts(iters, cond, groups, max_size, min_runs, sinks_only=sinks)
    assert rows.dtype == E.LINEAGE_GROUP_CUT_DTYPE and n_lost.dtype == np.uint32 and len(rows) == len(n_lost), what
    for r in rows:
        assert all(int(x) == NONE for x in r["group"][int(r["size"]):]), f"{what}: unused entries"
    got = got_rows(rows)
    assert got == want[0], f"{what}: rows {got[:6]} ({len(got)}), want {want[0][:6]} ({len(want[0])})"
    assert n_lost.tolist() == want[1], f"{what}: n_lost"
    assert len(set(got)) == len(got), f"{what}: a cut twice"
    st = eng.lineage_group_cut_stats().tolist()
    assert want[2] is None or st == want[2], f"{what}: stats {st}, want {want[2]}"
    if against_exhaustive and max_size <= 3:  # device against device
        erows, e_lost = eng.min_group_cuts(iters, cond, groups, max_size, min_runs, sinks_only=sinks)
        assert got_rows(erows) == got and e_lost.tolist() == n_lost.tolist(), f"{what}: nemo_min_group_cuts' rows"
    return got, n_lost.tolist()


def everywhere(eng, ref, iters, groups, max_size, min_runs, what, cond=1, flags=(False, True), grids=GRIDS, loaded=False,
               with_brute=True, sample=1):
    """the case with and without NEMO_KL_SINKS, on both tiers and under every kl_grid; the references once per flag"""
    if not loaded:
        eng.load(ref.corpus)
    out = {}
    try:
        for sinks in flags:
            want = model(ref, iters, cond, groups, max_size, min_runs, sinks)
            if with_brute:
                b = brute(ref, iters, cond, groups, max_size, min_runs, sinks, sample)
                assert (want[0], want[1]) == b, f"{what}, sinks {sinks}: the search and brute force differ"
            for lds in (-1, 0):
                for grid in grids:
                    eng.set_option("wit_lds_max", lds)
                    eng.set_option("kl_grid", grid)
                    compare(eng, iters, cond, groups, max_size, min_runs, sinks, want,
                            f"{what}, sinks {sinks}, wit_lds_max {lds}, kl_grid {grid}")
            out[sinks] = want
    finally:
        eng.set_option("wit_lds_max", -1)
        eng.set_option("kl_grid", 0)
    return out


# ---- 1, 4, 8. the hand-built pair of runs: the group shapes, q < n ------------------------------------------------------
PAIR_GROUPS = [[10], [11], [12], [10, 12], [10, 11, 12], [], [777777], [11]]


@pytest.fixture(scope="module")
def pair():
    return relabel(build([PA[:2], PB[:2]]), [PA[2], PB[2]])


def test_hand_built_pair_of_runs(eng, pair):
    """PA: goal <- rule <- (x 11, y 10), goal <- rule <- (x 11, z 12); PB: goal <- rule <- p 10, goal <- rule <- q 11.
    Equal groups (1 and 7), nested groups, an empty group, a label in several groups, an absent label."""
    ref = Ref(pair)
    eng.load(pair)
    for size in (1, 2, 3):
        for q in (0, 1):  # n = 2: min_runs 0, 1 and n - 1
            out = everywhere(eng, ref, [0, 1], PAIR_GROUPS, size, q, f"pair of runs, max_size {size}, q = {q}", loaded=True)
            for sinks in (False, True):
                rows, n_lost, stats, info = out[sinks]
                if size == 3 and q == 0:
                    assert rows == [(1, (4,)), (2, (0, 1)), (2, (1, 3)), (2, (0, 7)), (2, (3, 7))] and n_lost == [2] * 5
                if size == 3 and q == 1:  # both {11} candidates are rows; no pair of nested groups is one
                    assert rows == [(1, (1,)), (1, (3,)), (1, (4,)), (1, (7,)), (2, (0, 2))] and n_lost == [1, 1, 2, 1, 1]
                    # {11} is lost on A, survives on B and is a cut by count: its children are emitted and filtered
                    assert info["cut_survived"] >= 2 and stats[2][0] == 1
                assert stats[0] == [1, 0] and all(5 not in c and 6 not in c for _, c in rows)


@pytest.fixture(scope="module")
def trees():
    """build(): a node's label is its corpus-wide index, so a label names one node of one graph"""
    return build([fault_tree(s) for s in (137, 139, 151)])


def tree_groups(corpus, K, seed):
    rng = np.random.default_rng(seed)
    leaves = [int(corpus.node_off[2 * r + 1]) + v for r in range(3) for v in Graph(corpus, 2 * r + 1).leaves]
    groups = [[int(x) for x in rng.choice(leaves, int(rng.integers(1, 5)), replace=False)] for _ in range(K - 2)]
    return groups + [[], [10 ** 6, leaves[0]]]


def test_generated_fault_trees(eng, trees):
    ref = Ref(trees)
    eng.load(trees)
    groups = tree_groups(trees, 12, 1)
    rows = 0
    for size in (1, 2, 3):
        for q in (0, 1, 2):
            out = everywhere(eng, ref, [0, 1, 2], groups, size, q, f"fault trees, max_size {size}, q = {q}", loaded=True)
            rows += len(out[False][0])
    assert rows > 0


# ---- 2. a cut of size 8 that needs both runs ------------------------------------------------------------------------------
FOUR = ("g" + "r" * 4 + "g" * 4, [(0, 1 + k) for k in range(4)] + [(1 + k, 5 + k) for k in range(4)])


@pytest.fixture(scope="module")
def eight():
    return relabel(build([FOUR, FOUR]), [[900, 901, 902, 903, 904, 10, 11, 12, 13], [900, 901, 902, 903, 904, 20, 21, 22, 23]])


def test_size_eight_across_two_runs(eng, eight):
    ref = Ref(eight)
    groups = [[10], [20], [11], [21], [12], [22], [13], [23]]
    out = everywhere(eng, ref, [0, 1], groups, 8, 0, "size 8, q = n", with_brute=False)
    for sinks in (False, True):
        rows, n_lost, stats, _ = out[sinks]
        assert rows == [(8, tuple(range(8)))] and n_lost == [2]
        # a witness holds the first alive alternative of either run: a set of size d < 4 + 4 has two children at most
        assert stats[0] == [1, 0] and stats[1] == [2, 0] and stats[8] == [1, 1] and all(s[1] == 0 for s in stats[:8])
    assert everywhere(eng, ref, [0, 1], groups, 7, 0, "size 7, q = n", loaded=True, with_brute=False)[False][0] == []
    out = everywhere(eng, ref, [0, 1], groups, 5, 1, "q = 1", loaded=True)
    assert out[False][0] == [(4, (0, 2, 4, 6)), (4, (1, 3, 5, 7))] and out[False][1] == [1, 1]


# ---- 3. sizes 4 and 5 against brute force ------------------------------------------------------------------------------------
def test_sizes_four_and_five(eng, trees):
    ref = Ref(trees)
    eng.load(trees)
    big = 0
    for seed, K in ((2, 12), (3, 14)):
        groups = tree_groups(trees, K, seed)
        for size, q in ((4, 1), (5, 2), (5, 0)):
            out = everywhere(eng, ref, [0, 1, 2], groups, size, q, f"{K} groups, max_size {size}, q = {q}", loaded=True)
            big += sum(1 for r in out[False][0] if r[0] >= 4)
    assert big >= 1, "some minimal cut of size >= 4"


# ---- 5, 6. runs and the flag on the hand graphs -----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hand():
    return relabel(build([h[:2] for h in HAND]), [h[2] for h in HAND])


def test_runs_listed_twice_empty_and_absent_labels(eng, hand):
    ref = Ref(hand)
    eng.load(hand)
    groups = [[x] for x in (10, 11, 12, 13, 20, 21, 22, 30, 31)] + [[10, 12, 10], [21, 31], []]
    out = everywhere(eng, ref, [0, 1, 2, 3, 4, 5], groups, 3, 0, "the empty graph listed, q = n", loaded=True)
    assert out[False][0] == out[True][0] == [], "a graph without roots is never lost"
    assert out[False][2][0] == [1, 0], "the other graphs are evaluated"
    for q in (1, 2, 3):  # run 2 twice: it counts twice; labels 10..13 are absent from runs 1 and 2, 30 and 31 from the others
        out = everywhere(eng, ref, [0, 1, 2, 3, 4, 5, 2], groups, 3, q, f"hand, a run twice, q = {q}", loaded=True)
        assert out[False][0] and (q > 2 or any(x == 2 for x in out[False][1]))
    rows, _ = eng.lineage_group_cuts([4, 4], 1, groups, 3)  # every listed graph empty: nothing is evaluated
    assert len(rows) == 0 and not eng.lineage_group_cut_stats().any()


def test_sinks_flag(eng, hand):
    """H1: label 20 on the inner goal a and on the sink goal c; H0: label 10 on rule 1 and on goal b, 13 on rule 2.  An
    inner goal and a rule are matched without the flag and not with it."""
    ref = Ref(hand)
    eng.load(hand)
    out = everywhere(eng, ref, [1], [[20], [21], [22]], 3, 0, "H1", loaded=True)
    assert out[False][0] == [(2, (0, 1))] and out[True][0] == [(3, (0, 1, 2))]
    out = everywhere(eng, ref, [0], [[10], [13], [11], [12]], 3, 0, "H0", loaded=True)
    assert (2, (0, 1)) in out[False][0] and (2, (0, 1)) not in out[True][0] and out[True][0] == [(1, (2,)), (2, (0, 3))]


# ---- 7, 10. the chunk edge, duplicates, the emission buffer ----------------------------------------------------------------------
M = 65


@pytest.fixture(scope="module")
def straddle():
    kinds, edges, sinks = and_of_ors(M)
    corpus = relabel(build([(kinds, edges)] * 2), [list(range(len(kinds)))] * 2)
    return corpus, [[v] for v in sinks]


STRADDLE_ROWS = [(2, (2 * i, 2 * i + 1)) for i in range(M)]
STRADDLE_STATS = [[1, 0], [M, 0], [M + M * (M - 1) // 2, M]] + [[0, 0]] * 6


def test_and_of_ors_over_two_runs(eng, straddle):
    """level 1 holds 65 sets; every pair {a_i, a_j} is emitted by two parents and from both list positions"""
    corpus, groups = straddle
    ref = Ref(corpus)
    want = model(ref, [0, 1], 1, groups, 2, 0, False)
    assert (want[0], want[1], want[2]) == (STRADDLE_ROWS, [2] * M, STRADDLE_STATS) and want[3]["kids"][:2] == [2 * M, 2 * M * M]
    eng.load(corpus)
    try:
        for lds in (-1, 0):
            for grid in GRIDS:
                eng.set_option("wit_lds_max", lds)
                eng.set_option("kl_grid", grid)
                for sinks in (False, True):
                    compare(eng, [0, 1], 1, groups, 2, 0, sinks, want, f"m = {M}, sinks {sinks}, wit_lds_max {lds}, kl_grid {grid}")
    finally:
        eng.set_option("wit_lds_max", -1)
        eng.set_option("kl_grid", 0)


def test_emission_limit_and_regrow(straddle):
    corpus, groups = straddle
    want = (STRADDLE_ROWS, [2] * M, STRADDLE_STATS)
    e = E.Engine(0)  # a fresh context: the emission buffer has not grown yet
    try:
        e.load(corpus)
        e.set_option("lineage_children_max", 64)
        with pytest.raises(E.NemoError) as ei:
            e.lineage_group_cuts([0, 1], 1, groups, 2)
        assert ei.value.code == 6 and "lineage_children_max" in ei.value.msg and f"{2 * M} children" in ei.value.msg
        assert e.L.nemo_fetch_lineage_group_cuts(e.h, None, None, 0, None) == 5
        assert e.L.nemo_fetch_lineage_group_cut_stats(e.h, np.zeros(18, np.uint64).ctypes.data) == 5
        e.set_option("lineage_children_max", 65536)  # level 1 counts 2 * 65 * 65 children: past the first 1024
        compare(e, [0, 1], 1, groups, 2, 0, False, want, "behind a buffer that grows")
        compare(e, [0, 1], 1, groups, 2, 0, False, want, "and again, behind the grown buffer")
        e.set_option("lineage_children_max", -1)
        compare(e, [0, 1], 1, groups, 2, 1, False, model(Ref(corpus), [0, 1], 1, groups, 2, 1, False), "q = 1")
    finally:
        e.close()


def test_both_searches_interleaved_on_one_engine(straddle):
    """nemo_lineage_cuts (A) and nemo_lineage_group_cuts (B) share the level loop and keep a buffer group each.  On one
    engine, A, B, A, B: the first call of either counts past its first 1024-child buffer (129 * 129 and 2 * 65 * 65
    children) and runs the level again; every call's rows, lost counts and 18 stats are those of a fresh engine."""
    (kinds, edges, _), groups = and_of_ors(M), straddle[1]
    wide, wide_edges, sinks = and_of_ors(129)
    corpus = relabel(build([(kinds, edges)] * 2 + [(wide, wide_edges)]),
                     [list(range(len(kinds)))] * 2 + [list(range(2000000, 2000000 + len(wide)))])

    def call_a(e):
        rows = e.lineage_cuts(2, 1, None, 2)
        return [(int(r["size"]),) + tuple(int(x) for x in r["node"]) for r in rows], e.lineage_cut_stats().tolist()

    def call_b(e):
        rows, n_lost = e.lineage_group_cuts([0, 1], 1, groups, 2)
        return got_rows(rows), n_lost.tolist(), e.lineage_group_cut_stats().tolist()

    def fresh(call):
        e = E.Engine(0)
        try:
            e.load(corpus)
            return call(e)
        finally:
            e.close()

    want_a, want_b = fresh(call_a), fresh(call_b)
    assert want_a[0] == [(2, sinks[2 * i], sinks[2 * i + 1]) + (NONE,) * 6 for i in range(129)]
    assert want_a[1] == [[1, 0], [129, 0], [129 + 129 * 128 // 2, 129]] + [[0, 0]] * 6
    assert want_b == (STRADDLE_ROWS, [2] * M, STRADDLE_STATS)
    e = E.Engine(0)
    try:
        e.load(corpus)
        for k in range(2):
            assert call_a(e) == want_a, f"nemo_lineage_cuts, call {k + 1} of A, B, A, B"
            assert call_b(e) == want_b, f"nemo_lineage_group_cuts, call {k + 1} of A, B, A, B"
    finally:
        e.close()


# ---- 9. sizes ------------------------------------------------------------------------------------------------------------------
def test_hub_label_and_long_group(eng, hand):
    """H2: 300 nodes of label 30 (a row past KO_HUB); a group of 70 labels of which three occur"""
    ref = Ref(hand)
    eng.load(hand)
    groups = [[30], [31], [3000000 + k for k in range(67)] + [30, 21, 12], [20], [21], [11], [12], [10]]
    for q in (0, 1):
        out = everywhere(eng, ref, [2, 1, 0], groups, 3, q, f"a hub row and a long group, q = {q}", loaded=True)
        assert q == 0 or (2, (0, 1)) in out[False][0], "labels 30 and 31 together break H2"


def test_graph_past_65535_nodes_beside_a_small_one(eng):
    corpus, _ = synth.generate(3, target_nodes=140000, p_fault=0.9, prepend_run0=True, seed=3, eot=80, body_extra=6,
                               nval=3, nloc=4)
    r = max(range(corpus.n_runs), key=lambda x: corpus.graph_size(2 * x + 1))
    small = min(range(corpus.n_runs), key=lambda x: corpus.graph_size(2 * x + 1) or 10 ** 9)
    n0 = int(corpus.node_off[2 * r + 1])
    lab = corpus.label.copy()  # the graph's many roots share two labels of their own, so that two events are a cut
    for k, v in enumerate(Graph(corpus, 2 * r + 1).roots):
        lab[n0 + v] = 5000000 + k % 2
    corpus.label = np.ascontiguousarray(lab, dtype=np.uint32)
    ref = Ref(corpus)
    gr = ref.graph(2 * r + 1)
    assert gr.V >= 65536 and len(gr.roots) >= 2 and small != r
    rng = np.random.default_rng(5)
    leaf_labels = sorted({gr.label[v] for v in gr.leaves})
    picks = [int(x) for x in rng.choice(leaf_labels, 30, replace=False)]
    groups = [[5000000, picks[0]], [picks[1], 5000001]] + [picks[3 * k:3 * k + 3] for k in range(10)]
    its = [int(corpus.iteration[r]), int(corpus.iteration[small])]
    eng.load(corpus)
    want = model(ref, its, 1, groups, 2, 1, False)
    assert (2, (0, 1)) in want[0], "the roots' labels are a cut of the large graph"
    try:
        for lds in (-1, 0):  # the large graph is past the LDS tier by its size under either
            for grid in GRIDS:
                eng.set_option("wit_lds_max", lds)
                eng.set_option("kl_grid", grid)
                compare(eng, its, 1, groups, 2, 1, False, want, f"70k nodes, wit_lds_max {lds}, kl_grid {grid}")
    finally:
        eng.set_option("wit_lds_max", -1)
        eng.set_option("kl_grid", 0)


# ---- 11. a case study through fault_events -----------------------------------------------------------------------------------
def test_case_study_fault_events(eng):
    d = os.path.join(GOLDEN, "cs_pb_asynchronous")
    corpus = load_molly(d)
    runs = json.load(open(os.path.join(d, "runs.json")))
    spec = runs[0]["failureSpec"]
    good = [int(r["iteration"]) for r in runs if r["status"] == "success"]
    events, groups = fault_events(corpus.labels, spec["eot"], spec["eff"])
    nonempty = [it for it in good if corpus.graph_size(2 * corpus.run_index(it) + 1)]
    eng.load(corpus)
    ref = Ref(corpus)
    for q in (0, 1):
        want = model(ref, good, 1, groups, 3, q, False)
        got, _ = compare(eng, good, 1, groups, 3, q, False, want, f"pb_asynchronous, q = {q}")
        if q == 0 and len(nonempty) < len(good):
            assert got == [], "an empty post graph among the good runs is never lost"
        if q == 1:
            assert got, "some fault events defeat a good run"
            kinds = [sorted(events[p][0] for p in c) for _, c in got]
            assert ["crash", "omit"] in kinds


# ---- 12. protocol --------------------------------------------------------------------------------------------------------------
def raw(eng, iters, cond, off, labels, n_groups, max_size=2, min_runs=0, flags=0):
    it = np.ascontiguousarray(iters, dtype=np.uint32)
    off = None if off is None else np.ascontiguousarray(off, dtype=np.uint64)
    labels = None if labels is None else np.ascontiguousarray(labels, dtype=np.uint32)
    return eng.L.nemo_lineage_group_cuts(eng.h, it.ctypes.data if len(it) else None, len(it), cond,
                                         None if off is None else off.ctypes.data,
                                         None if labels is None or not len(labels) else labels.ctypes.data, n_groups, max_size, min_runs,
                                         flags)


def fetch_state(eng):
    return eng.L.nemo_fetch_lineage_group_cuts(eng.h, None, None, 0, None)


def test_protocol(eng, hand, pair):
    eng.load(hand)
    err = lambda: eng.L.nemo_last_error(eng.h).decode()
    assert fetch_state(eng) == 5  # a fetch before any call
    assert eng.L.nemo_fetch_lineage_group_cut_stats(eng.h, np.zeros(18, np.uint64).ctypes.data) == 5
    for bad in (0, 9, 0xFFFFFFFF):
        assert raw(eng, [0], 1, [0, 1, 2], [10, 11], 2, max_size=bad) == 1 and "max_size must be 1..8" in err()
    assert raw(eng, [0], 1, [0, 2, 1, 3], [10, 11, 12], 3) == 1 and "group_off decreases at group 1" in err()
    assert raw(eng, [0], 1, [0, 1, 3], [10, 11, 0xFFFFFFFF], 2) == 1 and "group 1 names label UINT32_MAX" in err() and "position 2" in err()
    assert raw(eng, [0], 1, None, [10], 1) == 1 and "no group_off" in err()
    assert raw(eng, [0], 1, [0, 1], None, 1) == 1 and "no group_labels" in err()
    assert eng.L.nemo_lineage_group_cuts(eng.h, None, 2, 1, None, None, 0, 2, 0, 0) == 1 and "no run list" in err()
    assert raw(eng, [0, 1], 1, [0, 1], [10], 1, min_runs=3) == 1 and "min_runs 3" in err()
    assert raw(eng, [0], 1, [0, 1], [10], 1, flags=2) == 1 and "flags" in err()
    assert raw(eng, [0], 2, [0, 1], [10], 1) == 1 and "cond" in err()
    assert raw(eng, [0, 4242], 1, [0, 1], [10], 1) == 7  # an iteration that is not loaded
    assert raw(eng, [0], 1, np.zeros(65537, np.uint64), None, 65536) == 6 and "65535" in err() and "u16" in err()
    assert raw(eng, [0], 1, [0, 1 << 31, 1 << 32], [10], 2) == 6 and "2^32 - 1 labels" in err()
    assert raw(eng, [0], 1, [0, 1, 2 + (1 << 24)], [10], 2) == 6 and "group 1 names 16777217 labels" in err() and "2^24" in err()
    # n * chunks > 2^28 words at level 0 already: 2^28 + 1 list positions (run 0, over and over)
    assert raw(eng, np.zeros((1 << 28) + 1, np.uint32), 1, [0, 1], [10], 1) == 6 and "2^28 words" in err()
    assert fetch_state(eng) == 5  # the failed calls left no result
    assert raw(eng, [0], 1, [0, 0, 0], None, 2) == 0 and fetch_state(eng) == 0  # empty groups name no label
    # zero rows
    for its, groups in (([], [[10], [11]]), ([0, 1], [])):
        rows, n_lost = eng.lineage_group_cuts(its, 1, groups, 3)
        assert len(rows) == 0 and len(n_lost) == 0 and not eng.lineage_group_cut_stats().any()
    # a too-small cap, and the query
    ref = Ref(hand)
    groups = [[10], [11, 12], [13], [20, 21], [22], [1], [6], [10, 13]]
    want = model(ref, [0, 1, 3], 1, groups, 4, 1, False)
    assert (want[0], want[1]) == brute(ref, [0, 1, 3], 1, groups, 4, 1, False) and len(want[0]) >= 2
    compare(eng, [0, 1, 3], 1, groups, 4, 1, False, want, "after the errors")
    off = np.cumsum([0] + [len(g) for g in groups]).astype(np.uint64)
    compare(eng, [0, 1, 3], 1, (off, np.array([x for g in groups for x in g], np.uint32)), 4, 1, False, want, "the pair form")
    n = ctypes.c_uint64()
    out = np.zeros(len(want[0]), E.LINEAGE_GROUP_CUT_DTYPE)
    assert eng.L.nemo_fetch_lineage_group_cuts(eng.h, None, None, 0, ctypes.byref(n)) == 0 and n.value == len(want[0])
    assert eng.L.nemo_fetch_lineage_group_cuts(eng.h, out.ctypes.data, None, len(out) - 1, ctypes.byref(n)) == 1
    assert eng.L.nemo_fetch_lineage_group_cuts(eng.h, out.ctypes.data, None, len(out), None) == 0 and got_rows(out) == want[0]
    # independence, in both directions, from the two parent calls made in between
    eng.lineage_cuts(0, 1, None, 3)
    eng.min_group_cuts([0, 1, 3], 1, groups, 2, 1)
    lin, gc, gcs = eng.lineage_cut_rows().copy(), [x.copy() for x in eng.min_group_cut_rows()], eng.min_group_cut_stats().copy()
    rows, n_lost = eng.lineage_group_cut_rows()
    assert got_rows(rows) == want[0] and n_lost.tolist() == want[1] and eng.lineage_group_cut_stats().tolist() == want[2]
    compare(eng, [0, 1, 3], 1, groups, 4, 1, False, want, "between the other calls", against_exhaustive=False)
    assert np.array_equal(eng.lineage_cut_rows(), lin) and np.array_equal(eng.min_group_cut_stats(), gcs)
    assert all(np.array_equal(a, b) for a, b in zip(eng.min_group_cut_rows(), gc))
    eng.load(pair)  # a reload: no result of the previous corpus survives
    assert fetch_state(eng) == 5
    assert eng.L.nemo_fetch_lineage_group_cut_stats(eng.h, np.zeros(18, np.uint64).ctypes.data) == 5


def test_call_without_a_corpus_and_node_context_refuse(hand):
    fresh = E.Engine(0)
    try:
        with pytest.raises(E.NemoError) as ei:
            fresh.lineage_group_cuts([0], 1, [[10]], 2)
        assert ei.value.code == 5 and "without a loaded corpus" in ei.value.msg
    finally:
        fresh.close()
    node = E.Engine(devices=[0])
    try:
        node.load(hand)
        with pytest.raises(E.NemoError) as ei:
            node.lineage_group_cuts([0], 1, [[10]], 2)
        assert ei.value.code == 5 and "single-device contexts only" in ei.value.msg
    finally:
        node.close()
