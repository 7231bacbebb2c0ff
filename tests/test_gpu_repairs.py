"""GPU checks of nemo_min_repair_sets / nemo_min_repairs (k_repair_lds, k_repair_glob and k_repair_absent in
nemo_amd/csrc/k_repair.hip, with k_cuts.hip's row kernels): every row, the row order, the status, |A|, the nine round
stats and the candidate list, exact.  There is no reference code for this call, so the reference is the definition in
plain Python over the Corpus arrays, in two forms that must agree before either meets the device:
(A) brute force: A \\ S evaluated for every S of up to max_size candidates, the holding sets with no holding proper
    subset kept;
(B) the path-set derivation, top-down and memoised, dual to the cut tests' fault tree: a rule is the product of its
    children's sets, a goal with children the union of theirs, a childless node {{}}; a node of A that is no candidate
    contributes nothing, and a candidate v joins v to each of its own sets (a restored inner node still needs its
    children: for a sink that is {v} alone); all truncated to size 3 and minimised.
The status comes from the definition under S = {} and S = cand, whatever (B) was truncated to."""
import itertools
import os
import sys

import numpy as np
import pytest

from nemo_amd import engine as E
from nemo_amd.corpus import load_molly
from tests.test_gpu_knockout import Graph, both_tiers, build, chain, hub_goal, wide_level
from tests.test_gpu_min_cuts import lost_at_once, minimise
from tools import synth

pytestmark = pytest.mark.gpu
NONE = 0xFFFFFFFF
HOLDS, SEARCHED, BEYOND = 0, 1, 2
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
sys.setrecursionlimit(max(sys.getrecursionlimit(), 20000))


@pytest.fixture(scope="module")
def eng():
    e = E.Engine(0)
    yield e
    e.close()


# ---- the reference ----------------------------------------------------------------------------------------------
def holds_at_once(gr, A, sets):
    """bit h of the result: the outcome is not lost under A \\ sets[h] (lost_at_once: the definition, sinks first)"""
    return ~lost_at_once(gr, [[v for v in A if v not in S] for S in map(set, sets)]) & ((1 << len(sets)) - 1)


def status_of(gr, A, cand):
    if not A or not gr.roots:
        return HOLDS
    h = holds_at_once(gr, A, [[], list(cand)])
    return HOLDS if h & 1 else SEARCHED if h & 2 else BEYOND


def repairs_brute(gr, A, cand, max_size):
    """(A) the minimal repairs as sets of candidate positions"""
    combos = [c for s in range(1, max_size + 1) for c in itertools.combinations(range(len(cand)), s)]
    holds = holds_at_once(gr, A, [[cand[p] for p in c] for c in combos])
    rep = {frozenset(c) for h, c in enumerate(combos) if (holds >> h) & 1}
    return {c for c in rep if not any(frozenset(s) in rep for k in range(1, len(c)) for s in itertools.combinations(c, k))}


def repairs_path_sets(gr, A, cand, max_size):
    """(B) the path-set derivation, as sets of candidate positions; {frozenset()} if the outcome holds as it is"""
    where, absent, memo = {v: p for p, v in enumerate(cand)}, set(A), {}

    def product(a, b):
        return minimise([x | y for x in a for y in b if len(x | y) <= 3])

    def sets(v):
        if v not in memo:
            if v in absent and v not in where:
                own = []
            else:
                if gr.rule[v] or not gr.ch[v]:
                    own = [frozenset()]
                    for c in gr.ch[v]:
                        own = product(own, sets(c))
                        if not own:
                            break
                else:
                    own = minimise([s for c in gr.ch[v] for s in sets(c)])
                if v in where:
                    own = product(own, [frozenset([where[v]])])
            memo[v] = own
        return memo[v]

    top = minimise([s for r in gr.roots for s in sets(r)]) if gr.roots else [frozenset()]
    return {s for s in top if len(s) <= max_size}


def expected(gr, A, cand, max_size, brute=True):
    """(status, |A|, rows in (size, rank) order, the 3 x 3 stats, the candidate list) by both forms"""
    A = list(A)
    cand = list(A) if cand is None else list(cand)
    status = status_of(gr, A, cand)
    zero = [[0, 0, 0], [0, 0, 0], [0, 0, 0]]
    b = repairs_path_sets(gr, A, cand, max_size) if A and gr.roots else {frozenset()}
    assert (frozenset() in b) == (status == HOLDS), f"form (B) and the definition differ on S = {{}} (graph {gr.g})"
    if status != SEARCHED:
        assert status == HOLDS or not b, "a repair where the outcome is lost under S = cand"
        return status, len(A), [], zero, cand
    if brute:
        a = repairs_brute(gr, A, cand, max_size)
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
        assert all(x in at for x in p), "a minimal repair of size > 1 holds a candidate that is a repair alone"
        q = [at[x] for x in p]
        return c2(q[1]) + q[0] if len(q) == 2 else c3(q[2]) + c2(q[1]) + q[0]

    rows = [(len(s),) + tuple(cand[p] for p in sorted(s)) + (NONE,) * (3 - len(s)) for s in sorted(b, key=lambda s: (len(s), rank(s)))]
    K1 = len(live)
    stats = [[K, K, sum(1 for s in b if len(s) == 1)], [0, 0, 0], [0, 0, 0]]
    if max_size >= 2:
        stats[1] = [K1, c2(K1), sum(1 for s in b if len(s) == 2)]
    if max_size >= 3:
        stats[2] = [K1, c3(K1), sum(1 for s in b if len(s) == 3)]
    return status, len(A), rows, stats, cand


def got_rows(arr):
    assert arr.dtype == np.uint32 and arr.ndim == 2 and arr.shape[1] == 4
    return [tuple(int(x) for x in r) for r in arr.tolist()]


def compare(eng, got, want, what):
    status, n_absent, rows, stats, cand = want
    g = got_rows(got)
    st = eng.min_repair_stats()
    print(f"{what}: status {st[0]}, |A| {st[1]}, {len(g)} rows, stats {st[2].tolist()}")
    assert st[0] == status, f"{what}: status {st[0]}, want {status}"
    assert len(g) == len(rows), f"{what}: {len(g)} rows, want {len(rows)}"
    bad = [k for k in range(len(rows)) if g[k] != rows[k]]
    assert not bad, f"{what}: rows {bad[:6]} differ: got {[g[k] for k in bad[:6]]}, want {[rows[k] for k in bad[:6]]}"
    assert st[1] == n_absent, f"{what}: |A| {st[1]}, want {n_absent}"
    assert st[2].tolist() == stats, f"{what}: stats {st[2].tolist()}, want {stats}"
    assert st[3].tolist() == list(cand), f"{what}: the candidate list differs"
    assert got_rows(eng.min_repair_rows()) == g


def check(eng, corpus, it, A, cand, max_size, what="", graph=None, brute=True, cond=1, want=None):
    gr = graph or Graph(corpus, 2 * corpus.run_index(it) + cond)
    want = want or expected(gr, A, cand, max_size, brute)
    compare(eng, eng.min_repair_sets(it, cond, A, cand, max_size), want, what)
    return want


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


# ---- 1. hand-built graphs ------------------------------------------------------------------------------------------------
# goal 0 <- rule 1 <- (a 3, b 4); goal 0 <- rule 2 <- (c 5, d 6, e 7)
TWO_RULES = ("grrggggg", [(0, 1), (0, 2), (1, 3), (1, 4), (2, 5), (2, 6), (2, 7)])
# goal 0 <- rule 1 <- (goal 2 <- rule 3 <- leaf 4; leaf 5): an inner goal and a rule may be absent
INNER = ("grgrgg", [(0, 1), (1, 2), (1, 5), (2, 3), (3, 4)])
HAND = [TWO_RULES, INNER]
a_, b_, c_, d_, e_ = 3, 4, 5, 6, 7


@pytest.fixture(scope="module")
def hand():
    return build(HAND)


def test_hand_built(eng, hand):
    def run(what):
        w = check(eng, hand, 0, [3, 4, 5, 6, 7], None, 3, f"all five leaves ({what})")
        assert w[0] == SEARCHED and w[2] == [(2, a_, b_, NONE), (3, c_, d_, e_)]
        w = check(eng, hand, 0, [3, 4, 5, 6, 7], None, 2, f"max_size 2 ({what})")
        assert w[2] == [(2, a_, b_, NONE)] and w[3] == [[5, 5, 0], [5, 10, 1], [0, 0, 0]]
        w = check(eng, hand, 0, [3, 4, 5, 6, 7], None, 1, f"max_size 1 ({what})")
        assert w[0] == SEARCHED and w[2] == []
        w = check(eng, hand, 0, [a_, c_], None, 2, f"a and c ({what})")
        assert w[2] == [(1, a_, NONE, NONE), (1, c_, NONE, NONE)] and w[3][1] == [0, 0, 0]
        w = check(eng, hand, 0, [a_], None, 2, f"a alone: r2 stands ({what})")
        assert w[0] == HOLDS and w[2] == []
        w = check(eng, hand, 0, [a_, c_], [a_], 2, f"a and c, only a may come back ({what})")
        assert w[2] == [(1, a_, NONE, NONE)]
        w = check(eng, hand, 0, [a_, b_, c_], [a_], 3, f"b stays lost ({what})")
        assert w[0] == BEYOND and w[2] == []
        w = check(eng, hand, 0, [a_, b_, c_], [], 3, f"no candidate ({what})")
        assert w[0] == BEYOND and w[4] == []
        w = check(eng, hand, 0, [e_, a_, b_, d_], [b_, e_, a_, d_], 3, f"rows in candidate order ({what})")
        assert w[2] == [(2, b_, a_, NONE), (2, e_, d_, NONE)]
        w = check(eng, hand, 0, [], None, 3, f"nothing absent ({what})")
        assert w[0] == HOLDS and w[1] == 0
        # an inner goal and a rule in A: a restored inner node still needs its children
        w = check(eng, hand, 1, [2, 3, 4], None, 3, f"inner goal, rule and leaf ({what})")
        assert w[2] == [(3, 2, 3, 4)]
        w = check(eng, hand, 1, [2, 3, 4], None, 2, f"... too large for max_size 2 ({what})")
        assert w[0] == SEARCHED and w[2] == []
        w = check(eng, hand, 1, [4, 2], [2], 3, f"the inner goal without its leaf ({what})")
        assert w[0] == BEYOND
        w = check(eng, hand, 1, [3, 0], [0, 3], 3, f"a rule and the root ({what})")
        assert w[2] == [(2, 0, 3, NONE)]
        # the pre graph (one goal): cond 0
        w = check(eng, hand, 0, [0], None, 2, f"the pre graph ({what})", cond=0)
        assert w[2] == [(1, 0, NONE, NONE)]

    tiers_and_grids(eng, hand, run)


def test_a_goal_whose_child_is_a_goal(eng):
    # goal 0 <- (goal 1 <- goal 3; goal 2): by kind alone the two reference forms agree on it
    corpus = build([("gggg", [(0, 1), (0, 2), (1, 3)])])
    gr = Graph(corpus, 1)
    assert expected(gr, [3, 2], None, 3)[2] == [(1, 3, NONE, NONE), (1, 2, NONE, NONE)]
    assert expected(gr, [1, 2, 3], None, 3)[2] == [(1, 2, NONE, NONE), (2, 1, 3, NONE)]
    assert expected(gr, [1, 2, 3], [3, 2], 3)[2] == [(1, 2, NONE, NONE)]
    with pytest.raises(E.NemoError) as ei:  # loadProv's count check refuses a goal -> goal edge: no device run of it
        eng.load(corpus)
    assert ei.value.code == 3


# ---- 2. chunk edges --------------------------------------------------------------------------------------------------------
def rules_of(m, width, extra=()):
    """goal 0 <- m rules of `width` leaves each, then the rules of `extra` (tuples of leaf numbers)"""
    n_rules = m + len(extra)
    kinds = "g" + "r" * n_rules + "g" * (m * width)
    first = 1 + n_rules
    edges = [(0, 1 + k) for k in range(n_rules)]
    edges += [(1 + k, first + width * k + j) for k in range(m) for j in range(width)]
    edges += [(1 + m + k, first + j) for k, r in enumerate(extra) for j in r]
    return (kinds, edges), list(range(first, first + m * width))


PAIR_LEAVES = [62, 64, 66, 130]  # C(130,2) = 8,385 pairs: 132 chunks, the last one short
TRIPLE_LEAVES = [63, 66]         # C(66,3) = 45,760 triples: exactly 715 chunks
# a pair rule (leaves 0, 1), triples that contain the pair (0, 1, 2), (0, 1, 9), and triples that do not
MIXED = rules_of(4, 3, extra=[(0, 1), (0, 1, 9), (2, 4, 7)])


@pytest.fixture(scope="module")
def edges_corpus():
    graphs = [rules_of(n // 2, 2) for n in PAIR_LEAVES] + [rules_of(n // 3, 3) for n in TRIPLE_LEAVES] + [MIXED]
    return build([g for g, _ in graphs]), [leaves for _, leaves in graphs]


@pytest.mark.parametrize("k", range(len(PAIR_LEAVES) + len(TRIPLE_LEAVES) + 1))
def test_chunk_edges(eng, edges_corpus, k):
    corpus, leaves = edges_corpus
    A, size = leaves[k], 2 if k < len(PAIR_LEAVES) else 3
    gr = Graph(corpus, 2 * k + 1)
    want = expected(gr, A, None, size)
    assert want[0] == SEARCHED and want[3][0] == [len(A), len(A), 0]
    if k < len(PAIR_LEAVES):
        assert len(want[2]) == len(A) // 2 and want[3][1][1] == len(A) * (len(A) - 1) // 2
    elif k < len(PAIR_LEAVES) + len(TRIPLE_LEAVES):
        assert len(want[2]) == len(A) // 3 and want[3][1][2] == 0
    else:  # the pair (0, 1) is a repair; the triples that hold it are none
        assert (2, A[0], A[1], NONE) in want[2] and want[3][1][2] == 1
        assert not any(r[0] == 3 and A[0] in r[1:] and A[1] in r[1:] for r in want[2])
        assert (3, A[2], A[4], A[7]) in want[2]
    tiers_and_grids(eng, corpus, lambda what: check(eng, corpus, k, A, None, size, f"{len(A)} leaves, {what}", gr, want=want),
                    grids=(0, 3))


# ---- 3. geometry -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def geometry():
    return build([hub_goal(), wide_level(), chain(301)])


@pytest.mark.parametrize("k, name", [(0, "hub goal with 300 children"), (1, "a level of 600 nodes"), (2, "301 levels")])
def test_geometry(eng, geometry, k, name):
    gr = Graph(geometry, 2 * k + 1)
    if k == 0:  # every leaf absent, and the first 150 rules: a leaf alone past them, a (rule, leaf) pair before
        A = list(range(301, 601)) + list(range(1, 151))
        want = expected(gr, A, None, 2, brute=False)
        assert sum(1 for r in want[2] if r[0] == 1) == 150 and sum(1 for r in want[2] if r[0] == 2) == 150
    elif k == 1:  # three leaves of the one wide rule
        A = [2, 300, 601]
        want = expected(gr, A, None, 3)
        assert want[2] == [(3, 2, 300, 601)]
    else:  # the sink, an inner goal and an inner rule of the chain
        A = [300, 100, 201]
        want = expected(gr, A, None, 3)
        assert want[2] == [(3, 300, 100, 201)]
    eng.load(geometry)
    both_tiers(eng, lambda what: check(eng, geometry, k, A, None, 3 if k else 2, f"{name} ({what})", gr, want=want))


# ---- 4. random corpora ------------------------------------------------------------------------------------------------------
RANDOM_SEEDS = [0, 3, 7, 12, 22, 25, 33, 35]  # chosen on the CPU: the asserts at the end of the test


def random_case(seed):
    """a small synthetic corpus, and per run (iteration, A, cand): A a random subset of the sinks plus some inner
    nodes, at most 12 candidates among them, in an order of their own"""
    rng = np.random.default_rng(seed)
    corpus, _ = synth.generate(3, target_nodes=60, p_fault=0.5, prepend_run0=True, seed=seed, eot=4, nval=2, nloc=3)
    cases = []
    for r in range(corpus.n_runs):
        gr = Graph(corpus, 2 * r + 1)
        if not gr.V or not gr.leaves:
            continue
        n_sink = int(rng.integers((len(gr.leaves) + 1) // 2, len(gr.leaves) + 1))  # few absent sinks lose no outcome here
        A = [gr.leaves[int(x)] for x in rng.choice(len(gr.leaves), n_sink, replace=False)]
        inner = [v for v in range(gr.V) if gr.ch[v]]
        if inner:
            A += [inner[int(x)] for x in rng.choice(len(inner), min(len(inner), int(rng.integers(0, 3))), replace=False)]
        order = [A[int(x)] for x in rng.permutation(len(A))]
        cand = order[:int(rng.integers(min(6, len(A)), min(12, len(A)) + 1))]
        cases.append((int(corpus.iteration[r]), gr, A, cand))
    return corpus, cases


def test_random_corpora(eng):
    sizes, statuses, empty, total = set(), set(), 0, 0
    for seed in RANDOM_SEEDS:
        corpus, cases = random_case(seed)
        wants = [expected(gr, A, cand, 3) for _, gr, A, cand in cases]
        none = not any(w[2] for w in wants)
        empty, total = empty + none, total + 1
        for w in wants:
            statuses.add(w[0])
            sizes |= {r[0] for r in w[2]}
        eng.load(corpus)
        for (it, gr, A, cand), w in zip(cases, wants):
            both_tiers(eng, lambda what: check(eng, corpus, it, A, cand, 3, f"seed {seed}, run {it} ({what})", gr, want=w))
    assert sizes == {1, 2, 3}, f"rows of sizes {sorted(sizes)} only"
    assert statuses == {HOLDS, SEARCHED, BEYOND}, f"statuses {sorted(statuses)} only"
    assert 4 * empty <= total, f"{empty} of {total} seeds yield zero rows"


# ---- 5. the pair form -------------------------------------------------------------------------------------------------------
def absent_sinks(corpus, base, other):
    """the sinks of run base's post graph whose label is no goal label of run other's post graph, in node order"""
    gb, go = 2 * corpus.run_index(base) + 1, 2 * corpus.run_index(other) + 1
    gr = Graph(corpus, gb)
    n0, o0, o1 = int(corpus.node_off[gb]), int(corpus.node_off[go]), int(corpus.node_off[go + 1])
    rule = (corpus.node_word[o0:o1] & np.uint32(0x80000000)) != 0
    have = set(corpus.label[o0:o1][~rule].tolist())
    return gr, [v for v in gr.leaves if int(corpus.label[n0 + v]) not in have]


def check_pair(eng, corpus, base, other, max_size, what, need_rows=False):
    gr, A = absent_sinks(corpus, base, other)
    want = expected(gr, A, None, max_size, brute=len(A) <= 12)
    if need_rows:
        assert want[0] == SEARCHED and want[2], f"{what}: the reference finds no repair"
    compare(eng, eng.min_repairs(base, other, max_size), want, f"{what}: the pair form")
    rows, st = got_rows(eng.min_repair_rows()), eng.min_repair_stats()
    assert st[3].tolist() == A, f"{what}: the device's candidate list"
    compare(eng, eng.min_repair_sets(base, 1, A, None, max_size), want, f"{what}: the same lists by name")
    st2 = eng.min_repair_stats()
    assert got_rows(eng.min_repair_rows()) == rows and st[:2] == st2[:2] and np.array_equal(st[2], st2[2])
    return want


PAIR_SYNTH = dict(n_runs=6, target_nodes=300, p_fault=0.9, max_drops=6, prepend_run0=True, seed=0, eot=5, nval=2, nloc=3)


def test_pair_form_synthetic(eng):
    corpus, _ = synth.generate(**PAIR_SYNTH)
    failed = corpus.failed_iters()
    assert 0 not in failed and failed
    eng.load(corpus)
    eng.mark()

    # The generator's post graphs have many roots and a failed run keeps some of them derivable, so on these pairs
    # the reference says HOLDS with 3 to 31 absent sinks (sweeps over seeds, sizes and drop counts on the CPU found no
    # synthetic pair it searches): they check the absent list, both label tables and round 0; the case studies below
    # are the pairs with rows.
    def run(what):
        absent = 0
        for f in failed:
            absent += check_pair(eng, corpus, 0, f, 2, f"(0, {f}) {what}")[1]
            check_pair(eng, corpus, f, 0, 2, f"({f}, 0) {what}")  # other = run 0: the load's table
        assert absent >= 3 * len(failed), "the failed runs lack too few of run 0's base events to check the absent list"
        compare(eng, eng.min_repairs(failed[0], failed[0], 3), (HOLDS, 0, [], [[0] * 3] * 3, []), f"(x, x) {what}")
        compare(eng, eng.min_repairs(0, 0, 3), (HOLDS, 0, [], [[0] * 3] * 3, []), f"(0, 0) {what}")

    both_tiers(eng, run)


# chosen on the CPU: the reference searches every (0, f) below and finds a repair (need_rows asserts it)
CASE_STUDIES = [("cs_ca_2434_bootstrap_synchronization", [7, 20]), ("cs_mr_2995_failed_after_expiry", [13, 14])]


@pytest.mark.parametrize("CASE_STUDY, CASE_PAIRS", CASE_STUDIES)
def test_pair_form_case_study(eng, CASE_STUDY, CASE_PAIRS):
    corpus = load_molly(os.path.join(GOLDEN, CASE_STUDY))
    assert all(corpus.status[corpus.run_index(f)] != "success" for f in CASE_PAIRS)
    eng.load(corpus)
    eng.mark()

    def run(what):
        for f in CASE_PAIRS:
            want = check_pair(eng, corpus, 0, f, 3, f"{CASE_STUDY} (0, {f}) {what}", need_rows=True)
            labs = E.repair_labels(corpus, 2 * corpus.run_index(0) + 1, np.array(want[2], np.uint32).reshape(-1, 4))
            assert len(labs) == len(want[2]) and all(len(x) == r[0] and all(isinstance(s, str) and s for s in x) for x, r in zip(labs, want[2]))
            check_pair(eng, corpus, f, 0, 3, f"{CASE_STUDY} ({f}, 0) {what}")

    both_tiers(eng, run)


# ---- 6. duality on the device ---------------------------------------------------------------------------------------------
def test_duality_on_the_device(eng, edges_corpus, hand):
    corpus, leaves = edges_corpus
    eng.load(corpus)
    cases = [(corpus, len(leaves) - 1, leaves[-1], None, 3), (corpus, 0, leaves[0], leaves[0][:40], 2)]
    for cp, it, A, cand, size in cases + [(hand, 1, [2, 3, 4], None, 3), (hand, 0, [3, 4, 5, 6, 7], None, 3)]:
        eng.load(cp)
        rows = got_rows(eng.min_repair_sets(it, 1, A, cand, size))
        assert rows
        sets, kind = [], []
        for r in rows:
            S = list(r[1:1 + r[0]])
            sets.append([v for v in A if v not in S])
            kind.append(False)
            for e in S:
                sets.append([v for v in A if v not in S or v == e])
                kind.append(True)
        ko = eng.knockout_sets(it, 1, sets)
        for row, lost in zip(ko, kind):
            assert (int(row["roots_dead"]) == int(row["n_roots"])) == lost


# ---- 7. a post graph of >= 65536 nodes: u32 rows, the global tier by size ------------------------------------------------
def test_graph_past_65535_nodes(eng):
    from tests.test_gpu_min_cuts import expected as cuts_expected
    corpus, _ = synth.generate(3, target_nodes=140000, p_fault=0.9, prepend_run0=True, seed=3, eot=80, body_extra=6,
                               nval=3, nloc=4)
    r = max(range(corpus.n_runs), key=lambda x: corpus.graph_size(2 * x + 1))
    gr = Graph(corpus, 2 * r + 1)
    assert gr.V >= 65536
    rng = np.random.default_rng(5)
    leaves = [gr.leaves[int(x)] for x in rng.choice(len(gr.leaves), 40, replace=False)]
    # 40 random leaves lose the outcome through 18 of them alone; A keeps three of those and the 22 that are no cut
    # alone, so that the outcome comes back with exactly those three: one triple among 2,300
    single = [row[1] for row in cuts_expected(gr, leaves, 1, brute=False)[0]]
    A = [v for v in leaves if v not in single[3:]]
    want = expected(gr, A, None, 3, brute=False)
    assert want[0] == SEARCHED and len(A) == 25 and want[2] == [(3,) + tuple(v for v in A if v in single[:3])]
    eng.load(corpus)
    check(eng, corpus, int(corpus.iteration[r]), A, None, 3, "66k nodes", gr, want=want)
    st = check(eng, corpus, int(corpus.iteration[r]), A, [v for v in A if v != single[0]], 3, "66k nodes, one cut leaf stays lost", gr)
    assert st[0] == BEYOND


# ---- 8. protocol ------------------------------------------------------------------------------------------------------------
def fetch_codes(eng):
    z = np.zeros(11, np.uint64)
    return (eng.L.nemo_fetch_min_repairs(eng.h, None, 0, None), eng.L.nemo_fetch_min_repair_stats(eng.h, z.ctypes.data),
            eng.L.nemo_fetch_min_repair_cands(eng.h, None, 0, None))


def test_protocol(eng, hand, edges_corpus):
    fresh = E.Engine(0)
    try:
        with pytest.raises(E.NemoError) as ei:  # no corpus loaded
            fresh.min_repair_sets(0, 1, [3], None, 2)
        assert ei.value.code == 5
        with pytest.raises(E.NemoError) as ei:
            fresh.min_repairs(0, 1, 2)
        assert ei.value.code == 5
    finally:
        fresh.close()
    eng.load(hand)
    assert fetch_codes(eng) == (5, 5, 5)  # the fetches before any call
    for bad in (0, 4, 0xFFFFFFFF):
        with pytest.raises(E.NemoError) as ei:
            eng.min_repair_sets(0, 1, [3, 4], None, bad)
        assert ei.value.code == 1 and "max_size" in ei.value.msg
    a = np.array([3, 4], np.uint32)
    assert eng.L.nemo_min_repair_sets(eng.h, 0, 1, a.ctypes.data, 2, None, 0, 2, 1) == 1  # flags
    assert eng.L.nemo_min_repairs(eng.h, 0, 1, 2, 8) == 1
    for absent, cand, text in (([3, 8], None, "absent node 1 is node 8, out of range"),
                               ([3, 4, 5, 4], None, "absent node 3 names node 4 a second time"),
                               ([3, 4, 5], [4, 3, 4], "candidate 2 names node 4 a second time"),
                               ([3, 4, 5], [4, 6], "candidate 1 is node 6, which is not in the absent list"),
                               ([], [4], "candidate 0 is node 4, which is not in the absent list")):
        with pytest.raises(E.NemoError) as ei:
            eng.min_repair_sets(0, 1, absent, cand, 2)
        assert ei.value.code == 1 and text in ei.value.msg, ei.value.msg
    with pytest.raises(E.NemoError) as ei:
        eng.min_repair_sets(4242, 1, [3], None, 2)
    assert ei.value.code == 7
    with pytest.raises(E.NemoError) as ei:
        eng.min_repair_sets(0, 2, [3], None, 2)
    assert ei.value.code == 1 and "cond" in ei.value.msg
    with pytest.raises(E.NemoError) as ei:  # the pair form needs what nemo_diffprov_pairs needs
        eng.min_repairs(0, 1, 2)
    assert ei.value.code == 5 and "nemo_mark_holds" in ei.value.msg
    eng.mark()
    with pytest.raises(E.NemoError) as ei:
        eng.min_repairs(0, 4242, 2)
    assert ei.value.code == 7
    with pytest.raises(E.NemoError) as ei:
        eng.min_repairs(0, 1, 4)
    assert ei.value.code == 1
    assert fetch_codes(eng) == (5, 5, 5)  # the failed calls left no result
    check(eng, hand, 0, [3, 4, 5, 6, 7], None, 3, "after the errors")
    with pytest.raises(E.NemoError):
        eng.min_repair_sets(0, 1, [3, 3], None, 2)
    assert fetch_codes(eng) == (5, 5, 5)  # a failed call voids the previous result
    # more than 2^32 - 2 hypotheses in a round: 2,955 live candidates have 4,296,157,285 triples
    wide = build([wide_level(3000)])
    eng.load(wide)
    with pytest.raises(E.NemoError) as ei:
        eng.min_repair_sets(0, 1, list(range(2, 2 + 2955)), None, 3)
    assert ei.value.code == 6 and "shorten the candidate list" in ei.value.msg
    assert fetch_codes(eng) == (5, 5, 5)  # and leaves no results
    eng.load(hand)
    check(eng, hand, 0, [3, 4], None, 2, "before the reload")
    eng.load(edges_corpus[0])  # a reload: no result of the previous corpus survives
    assert fetch_codes(eng) == (5, 5, 5)
    check(eng, edges_corpus[0], 0, edges_corpus[1][0][:11], None, 2, "after the reload")


def test_node_context_refuses(hand):
    node = E.Engine(devices=[0])
    try:
        node.load(hand)
        with pytest.raises(E.NemoError) as ei:
            node.min_repair_sets(0, 1, [3], None, 2)
        assert ei.value.code == 5 and "single-device contexts only" in ei.value.msg
        with pytest.raises(E.NemoError) as ei:
            node.min_repairs(0, 1, 2)
        assert ei.value.code == 5 and "single-device contexts only" in ei.value.msg
    finally:
        node.close()


def test_buffers_grow_and_are_reused(eng, edges_corpus):
    corpus, leaves = edges_corpus
    k = len(PAIR_LEAVES) - 1
    gr = Graph(corpus, 2 * k + 1)
    eng.load(corpus)
    for n in (4, 70, 2, 130, 70):
        check(eng, corpus, k, leaves[k][:n], None, 2, f"{n} absent leaves", gr)
    check(eng, corpus, len(leaves) - 2, leaves[-2], None, 3, "a second, larger call")


def groups_of(sizes):
    """goal 0 <- rule 1 <- one goal per group, each <- one rule per leaf <- its leaf: the leaves of one group are a
    cut, one leaf of every group is a repair.  Returns the graph and the groups' leaves."""
    kinds, edges, groups = "gr", [(0, 1)], []
    for n in sizes:
        top = len(kinds)
        kinds += "g" + "rg" * n
        edges += [(1, top)] + [e for k in range(n) for e in ((top, top + 1 + 2 * k), (top + 1 + 2 * k, top + 2 + 2 * k))]
        groups.append([top + 2 + 2 * k for k in range(n)])
    return (kinds, edges), groups


# 12 sink goals each: 66 pairs (two chunks, the second of 2) and 220 triples (four chunks, the last of 28).  MIXED has a
# pair repair and triple repairs and no cut of size <= 3; GROUPS has a pair cut, two triple cuts and no repair of size <= 3.
GROUPS = groups_of([2, 3, 3, 4])


@pytest.mark.parametrize("lds, grid", [(-1, 0), (0, 0), (-1, 1), (0, 1)])
def test_cut_and_repair_calls_interleaved(lds, grid):
    """nemo_min_cuts and the two repair calls share their search driver and their sweep loop: on one engine, in turn,
    each call's rows, stats and candidates are those of the same call on a fresh engine.  Both tiers; cut_grid 1: one
    workgroup walks every chunk of a round, so both modes refill the dead words between chunks."""
    from tests.test_gpu_min_cuts import expected as cuts_expected, got_rows as cut_rows
    corpus = build([MIXED[0], GROUPS[0], HAND[0]])
    mixed, flat = MIXED[1], [v for grp in GROUPS[1] for v in grp]
    g_mixed, g_groups = Graph(corpus, 1), Graph(corpus, 3)
    assert len(mixed) == 12 and g_groups.leaves == flat and len(flat) == 12
    # the shapes, by the references: 12 live candidates in every call, a round 3 that drops sets over a found pair
    want_cut = cuts_expected(g_groups, flat, 3)
    assert [r[0] for r in want_cut[0]] == [2, 3, 3] and want_cut[1] == [[12, 12, 0], [12, 66, 1], [12, 220, 2]]
    assert cuts_expected(g_mixed, mixed, 3) == ([], [[12, 12, 0], [12, 66, 0], [12, 220, 0]])
    want_rep = expected(g_mixed, mixed, None, 3)
    assert want_rep[0] == SEARCHED and want_rep[3][1] == [12, 66, 1] and want_rep[3][2][:2] == [12, 220] and want_rep[3][2][2] >= 1
    want_pair = expected(g_groups, flat, None, 3)  # every label is its own: the absent sinks are all sinks
    assert want_pair[0] == SEARCHED and want_pair[2] == [] and want_pair[3][2] == [12, 220, 0]
    order = mixed[::-1]
    want_list = expected(g_mixed, mixed, order, 3)
    assert want_list[2] and want_list[2] != want_rep[2]

    def cuts_call(it):
        def call(e):
            rows = cut_rows(e.min_cuts(it, 1, None, 3))
            assert rows == cut_rows(e.min_cut_rows())
            return rows, e.min_cut_stats().tolist()
        return call

    def repair_result(e, arr):
        st = e.min_repair_stats()
        assert got_rows(e.min_repair_rows()) == got_rows(arr)
        return int(st[0]), int(st[1]), got_rows(arr), st[2].tolist(), st[3].tolist()

    calls = [("nemo_min_cuts, the groups", cuts_call(1), (want_cut[0], want_cut[1])),
             ("nemo_min_repair_sets", lambda e: repair_result(e, e.min_repair_sets(0, 1, mixed, None, 3)), want_rep),
             ("nemo_min_cuts, another graph", cuts_call(0), ([], [[12, 12, 0], [12, 66, 0], [12, 220, 0]])),
             ("nemo_min_repairs", lambda e: repair_result(e, e.min_repairs(1, 0, 3)), want_pair),
             ("nemo_min_repair_sets, a candidate list", lambda e: repair_result(e, e.min_repair_sets(0, 1, mixed, order, 3)), want_list)]

    def engine():
        e = E.Engine(0)
        e.set_option("knock_lds_max", lds)
        e.set_option("cut_grid", grid)
        e.load(corpus)
        e.mark()
        return e

    one = engine()
    try:
        for what, call, want in calls:
            got = call(one)
            fresh = engine()
            try:
                alone = call(fresh)
            finally:
                fresh.close()
            print(f"{what} (knock_lds_max {lds}, cut_grid {grid}): {got[:-1]}")
            assert got == alone, f"{what}: the interleaved call differs from the same call on a fresh engine"
            assert tuple(got) == tuple(want), f"{what}: differs from the reference"
    finally:
        one.close()


def test_other_results_are_left_alone(eng):
    from tests.small import random_corpus
    corpus = random_corpus(1000, n_runs=6, max_nodes=40)[0]
    its = [int(x) for x in corpus.iteration]
    f = corpus.failed_iters() or its[1:3]
    eng.load(corpus)
    eng.mark()

    def others():
        return (np.array(eng.diff_masks(len(f))).copy(), eng.missing().copy(), [m.copy() for m in eng.sdiff_masks()],
                eng.surplus().copy(), eng.label_distances().copy(), eng.knockout_rows().copy(), eng.min_cut_rows().copy(),
                eng.min_cut_stats().copy())

    def same(a, b):
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[3], b[3])
        assert len(a[2]) == len(b[2]) and all(np.array_equal(x, y) for x, y in zip(a[2], b[2]))
        assert all(np.array_equal(a[k], b[k]) for k in (4, 5, 6, 7))

    eng.diffprov(f, 1)
    eng.diffprov_pairs(f, [its[0]] * len(f))
    eng.nearest_runs(its, its)
    eng.knockout_leaves(its, 1)
    eng.min_cuts(its[0], 1, None, 3)
    before = others()
    for it in its:
        gr = Graph(corpus, 2 * corpus.run_index(it) + 1)
        check(eng, corpus, it, gr.leaves[:10], None, 3, f"run {it} between the other calls", gr)
        eng.min_repairs(it, its[0], 2)
    same(before, others())  # their fetches, unchanged by the repair calls between them
    last, st = got_rows(eng.min_repair_rows()), eng.min_repair_stats()
    eng.knockout_leaves(its, 1)
    eng.knockout_sets(its[0], 1, [[0]])
    eng.min_cuts(its[0], 1, None, 2)
    eng.diffprov_pairs(f, [its[0]] * len(f))
    st2 = eng.min_repair_stats()
    assert got_rows(eng.min_repair_rows()) == last and st[:2] == st2[:2]  # and the reverse
    assert np.array_equal(st[2], st2[2]) and np.array_equal(st[3], st2[3])
