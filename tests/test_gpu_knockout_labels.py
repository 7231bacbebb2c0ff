"""GPU checks of nemo_knockout_labels (k_kl_tables, k_kl_lds, k_kl_glob and k_kl_count in nemo_amd/csrc/k_klabel.hip):
every lost and hit word and every count, exact.

Reference.  There is no reference code for the call (include/nemohip.h fixes the semantics), so the reference is the
definition in plain Python over the Corpus arrays, in two forms that must agree with each other before either meets
the device.  Both first translate a label set to F(i,s), the nodes of the listed graph that carry one of its labels
(NEMO_KL_SINKS: the sink goals among them).  (A) per graph, all sets at once: one Python integer per node, bit s =
set s, sinks first (lost_at_once of tests/test_gpu_min_cuts.py).  (B) per (graph, set): the memoised top-down
derivation search of tests/test_gpu_knockout.py; lost iff the graph has roots and every root is dead.  Neither calls
the library.  The C3 shape and the 66,633-node graph take form (A) as the same statement over numpy words, and form (B)
on a sample.  A third check is device against device: the translated sets through nemo_knockout_sets per graph.

Every case runs on both tiers (knock_lds_max default and 0), with and without NEMO_KL_SINKS, and under kl_grid 0, 1
and 3 (1: one workgroup walks every listed graph in turn; 3: a graph's chunks are split over workgroups).  Every case
that goes through everywhere() also runs the LDS tier under kl_hitlist 0 (no hit list: every chunk probes with every
node's label), which must give the same words.
"""
import sys

import numpy as np
import pytest

from nemo_amd import engine as E
from tests.small import random_corpus
from tests.test_gpu_knockout import Graph, build
from tests.test_gpu_min_cuts import chains, fault_tree, hub, level, lost_at_once
from tools import synth

pytestmark = pytest.mark.gpu
sys.setrecursionlimit(max(sys.getrecursionlimit(), 20000))
GRIDS = (0, 1, 3)


@pytest.fixture(scope="module")
def eng():
    e = E.Engine(0)
    yield e
    e.close()


# ---- the reference ----------------------------------------------------------------------------------------------
class Ref:
    """The listed graphs of a corpus with their labels, translated sets and both reference forms."""

    def __init__(self, corpus):
        self.corpus, self.graphs = corpus, {}

    def graph(self, g):
        if g not in self.graphs:
            gr = Graph(self.corpus, g)
            n0 = int(self.corpus.node_off[g])
            gr.label = self.corpus.label[n0:n0 + gr.V].tolist()
            gr.by_label, gr.sink = {}, set(gr.leaves)
            for v, lab in enumerate(gr.label):
                gr.by_label.setdefault(lab, []).append(v)
            self.graphs[g] = gr
        return self.graphs[g]

    def nodes(self, gr, labels, sinks):
        """F(i,s): a label named twice counts once, an absent label matches nothing"""
        out = []
        for lab in dict.fromkeys(int(x) for x in labels):
            out += [v for v in gr.by_label.get(lab, []) if not sinks or v in gr.sink]
        return out

    def words(self, it, cond, sets, sinks, sample=1, numpy_form=False):
        """(lost, hit) of one list position as Python integers (bit s = set s): form (A) for all sets at once, form
        (B) on every `sample`-th set; they must agree"""
        gr = self.graph(2 * self.corpus.run_index(it) + cond)
        F = [self.nodes(gr, s, sinks) for s in sets]
        hit = sum(1 << s for s, f in enumerate(F) if f)
        lost = lost_numpy(gr, F) if numpy_form else lost_at_once(gr, F)
        for s in range(0, len(sets), sample):
            dead = gr.dead_by_derivation(F[s])
            b = bool(gr.roots) and all(r in dead for r in gr.roots)
            assert b == bool((lost >> s) & 1), f"the two reference forms differ on graph {gr.g}, set {s}"
        assert lost & ~hit == 0, "an outcome lost without a hit"
        return lost, hit, gr, F


def lost_numpy(gr, F):
    """form (A) over numpy words: a u64 row per node, bit s of word s / 64 = dead under F[s]; sinks first"""
    H = len(F)
    W = (H + 63) // 64
    dead = np.zeros((max(gr.V, 1), W), np.uint64)
    for s, f in enumerate(F):
        if f:
            dead[np.asarray(f, np.int64), s >> 6] |= np.uint64(1 << (s & 63))
    for v in sorted(range(gr.V), key=lambda x: -gr.pos[x]):
        ch = gr.ch[v]
        if ch:
            rows = dead[ch]
            dead[v] |= np.bitwise_or.reduce(rows, axis=0) if gr.rule[v] else np.bitwise_and.reduce(rows, axis=0)
    lost = np.bitwise_and.reduce(dead[gr.roots], axis=0) if gr.roots else np.zeros(W, np.uint64)
    return sum(int(w) << (64 * k) for k, w in enumerate(lost.tolist()))


def to_words(x, n_chunks):
    return [(x >> (64 * c)) & 0xFFFFFFFFFFFFFFFF for c in range(n_chunks)]


def expect(ref, iters, cond, sets, sinks, sample=1, numpy_form=False):
    """(lost [n][n_chunks], hit, n_lost [n_sets], n_hit): a run listed twice is computed once and counts twice"""
    ck = (len(sets) + 63) // 64
    memo, lost, hit = {}, [], []
    n_lost, n_hit = [0] * len(sets), [0] * len(sets)
    for it in iters:
        if it not in memo:
            memo[it] = ref.words(it, cond, sets, sinks, sample, numpy_form)[:2]
        lo, hi = memo[it]
        lost.append(to_words(lo, ck))
        hit.append(to_words(hi, ck))
        for s in range(len(sets)):
            n_lost[s] += (lo >> s) & 1
            n_hit[s] += (hi >> s) & 1
    return lost, hit, n_lost, n_hit


def compare(eng, iters, cond, sets, sinks, want, what):
    lost, hit = eng.knockout_labels(iters, cond, sets, sinks_only=sinks)
    ck = (len(sets) + 63) // 64
    assert lost.shape == hit.shape == (len(iters), ck) and lost.dtype == hit.dtype == np.uint64, what
    for name, got, exp in (("lost", lost, want[0]), ("hit", hit, want[1])):
        exp = np.array(exp, dtype=np.uint64).reshape(len(iters), ck)
        bad = np.argwhere(got != exp)
        assert not len(bad), f"{what}: {name} words {bad[:6].tolist()} differ: got {[hex(int(got[tuple(b)])) for b in bad[:6]]}, " \
                             f"want {[hex(int(exp[tuple(b)])) for b in bad[:6]]}"
    n_lost, n_hit = eng.knockout_label_counts()
    assert n_lost.tolist() == want[2], f"{what}: n_lost"
    assert n_hit.tolist() == want[3], f"{what}: n_hit"
    return lost, hit


def everywhere(eng, ref, iters, sets, what, cond=1, sample=1, numpy_form=False, grids=GRIDS, loaded=False):
    """the case with and without NEMO_KL_SINKS, on both tiers and under every kl_grid; the reference once per flag"""
    if not loaded:
        eng.load(ref.corpus)
    out = {}
    try:
        for sinks in (False, True):
            want = expect(ref, iters, cond, sets, sinks, sample, numpy_form)
            for lds in (-1, 0):
                for grid in grids:
                    eng.set_option("knock_lds_max", lds)
                    eng.set_option("kl_grid", grid)
                    compare(eng, iters, cond, sets, sinks, want, f"{what}, sinks {sinks}, knock_lds_max {lds}, kl_grid {grid}")
            eng.set_option("knock_lds_max", -1)  # and the LDS tier without the hit list (V probes per chunk)
            eng.set_option("kl_hitlist", 0)
            for grid in (0, 1):
                eng.set_option("kl_grid", grid)
                compare(eng, iters, cond, sets, sinks, want, f"{what}, sinks {sinks}, kl_hitlist 0, kl_grid {grid}")
            eng.set_option("kl_hitlist", 1)
            out[sinks] = want
    finally:
        eng.set_option("knock_lds_max", -1)
        eng.set_option("kl_grid", 0)
        eng.set_option("kl_hitlist", 1)
    return out


def relabel(corpus, posts_labels):
    """build()'s corpus with the post graphs' labels replaced (the pre graphs' single goals keep labels of their own)"""
    lab = corpus.label.copy()
    for r, labels in enumerate(posts_labels):
        n0 = int(corpus.node_off[2 * r + 1])
        assert len(labels) == corpus.graph_size(2 * r + 1)
        lab[n0:n0 + len(labels)] = labels
        lab[int(corpus.node_off[2 * r])] = 900000 + r
    corpus.label = np.ascontiguousarray(lab, dtype=np.uint32)
    return corpus


# ---- hand-built graphs: one per rule of dead_F under label matching ----------------------------------------------
# 0: goal 0 <- rule 1 <- (a 3, b 4); goal 0 <- rule 2 <- (a 3, c 5).  Label 10 on rule 1 and on goal b, 11 on a, 12 on c,
#    13 on rule 2: a label on a goal and on a rule of the same graph
H0 = ("grrggg", [(0, 1), (0, 2), (1, 3), (1, 4), (2, 3), (2, 5)], [1, 10, 13, 11, 10, 12])
# 1: goal 0 <- rule 1 <- a 3; goal 0 <- rule 2 <- b 4; the inner goal a <- rule 5 <- c 7, a <- rule 6 <- e 8.  Label 20 on
#    the inner goal a and on the sink goal c (the flag must tell them apart), 21 on b, 22 on e
H1 = ("grrggrrgg", [(0, 1), (0, 2), (1, 3), (2, 4), (3, 5), (3, 6), (5, 7), (6, 8)], [1, 2, 3, 20, 21, 4, 5, 20, 22])
# 2: goal 0 <- rule 1 <- 300 leaves, all of label 30; goal 0 <- rule 2 <- one leaf of label 31
H2 = ("grr" + "g" * 301, [(0, 1), (0, 2)] + [(1, 3 + k) for k in range(300)] + [(2, 303)], [1, 2, 3] + [30] * 300 + [31])
# 3: two roots, goal 0 <- rule 2 <- a 4; goal 1 <- rule 3 <- b 5; labels 11 and 21 only: label 10 is absent here
H3 = ("ggrrgg", [(0, 2), (1, 3), (2, 4), (3, 5)], [1, 6, 2, 3, 11, 21])
# 4: an empty graph: no nodes, no roots, nothing is hit, nothing is lost
H4 = ("", [], [])
# 5: a rule without children is alive unless named: goal 0 <- rules 1 (label 13), 2; rule 2 <- leaf 3 (label 12)
H5 = ("grrg", [(0, 1), (0, 2), (2, 3)], [1, 13, 7, 12])
HAND = [H0, H1, H2, H3, H4, H5]
HAND_SETS = [[10], [11], [12], [13], [10, 12], [12, 13], [20], [21], [20, 21], [21, 22], [30], [31], [30, 31], [],
             [11, 11], [11, 21], [777777], [1], [22, 20, 21, 22], [12, 13, 10]]


@pytest.fixture(scope="module")
def hand():
    return relabel(build([h[:2] for h in HAND]), [h[2] for h in HAND])


def bits(word_rows, i, n):
    return [s for s in range(n) if (word_rows[i][s >> 6] >> (s & 63)) & 1]


def test_hand_built(eng, hand):
    ref = Ref(hand)
    its = list(range(len(HAND)))
    out = everywhere(eng, ref, its, HAND_SETS, "hand-built")
    n = len(HAND_SETS)
    lost, hit = out[False][0], out[False][1]
    # graph 0: label 10 takes rule 1 and leaf b (not lost: rule 2 stands); 11 takes a (lost); {10, 12} is lost, {12, 13}
    # is not (rule 1 stands); set 17 names the root's own label
    assert bits(lost, 0, n) == [1, 4, 14, 15, 17, 19] and bits(hit, 0, n) == [0, 1, 2, 3, 4, 5, 14, 15, 17, 19]
    # graph 1: label 20 on the inner goal a and the sink c: a alone is no cut, with b (21) it is
    assert bits(lost, 1, n) == [8, 17, 18] and 6 in bits(hit, 1, n)
    assert bits(lost, 2, n) == [12, 17] and bits(hit, 2, n) == [10, 11, 12, 17]  # 300 nodes of one label
    assert bits(lost, 3, n) == [15] and 0 not in bits(hit, 3, n)  # both roots; label 10 absent
    assert bits(lost, 4, n) == [] and bits(hit, 4, n) == []  # the empty graph
    assert bits(lost, 5, n) == [5, 17, 19] and bits(hit, 5, n) == [2, 3, 4, 5, 17, 19]  # the childless rule, named
    # under the flag: rules and inner goals no longer match
    slost, shit = out[True][0], out[True][1]
    assert bits(shit, 0, n) == [0, 1, 2, 4, 5, 14, 15, 19] and bits(slost, 0, n) == [1, 4, 14, 15, 19]
    assert bits(slost, 1, n) == [18] and bits(shit, 1, n) == [6, 7, 8, 9, 15, 18]  # c, b and e, never the inner a
    assert bits(slost, 5, n) == [] and bits(shit, 5, n) == [2, 4, 5, 19]
    assert out[False][2][13] == 0 and out[False][3][13] == 0 and out[False][3][16] == 0  # the empty set, the absent label


def test_device_against_knockout_sets(eng, hand):
    """the same translated sets through nemo_knockout_sets per graph: roots_dead == n_roots > 0 is the lost bit"""
    for corpus in (hand, random_corpus(7, n_runs=5, max_nodes=30)[0]):
        ref = Ref(corpus)
        its = [int(x) for x in corpus.iteration]
        labs = sorted(set(corpus.label.tolist()))
        rng = np.random.default_rng(11)
        sets = HAND_SETS if corpus is hand else [rng.choice(labs, int(rng.integers(0, 4))).tolist() for _ in range(70)]
        eng.load(corpus)
        for sinks in (False, True):
            lost, hit = eng.knockout_labels(its, 1, sets, sinks_only=sinks)
            for i, it in enumerate(its):
                gr = ref.graph(2 * corpus.run_index(it) + 1)
                F = [ref.nodes(gr, s, sinks) for s in sets]
                rows = eng.knockout_sets(it, 1, F)
                for s, r in enumerate(rows):
                    want = int(r["n_roots"]) > 0 and int(r["roots_dead"]) == int(r["n_roots"])
                    assert bool((int(lost[i, s >> 6]) >> (s & 63)) & 1) == want, (it, s, sinks)
                    assert bool((int(hit[i, s >> 6]) >> (s & 63)) & 1) == bool(F[s]), (it, s, sinks)


# ---- chunk edges ---------------------------------------------------------------------------------------------------
def edge_sets(corpus, n_sets, seed, full=False):
    """n_sets sets over the corpus's labels: an empty set first, last and in the middle, a label named twice, a set
    of 1,000 labels, chunk 0 padded to exactly 1,024 or 2,048 entries (half the slots of its table, the densest the
    sizing rule allows: probe chains and wrap-around), and one label in all 64 sets of a chunk: of chunk 1 at 129
    sets (the empty sets are 0, 63 and 128 there); with `full`, of chunk 0, which then holds no empty set"""
    rng = np.random.default_rng(seed)
    labs = sorted(set(corpus.label.tolist()))
    sets = [rng.choice(labs, int(rng.integers(1, 4))).tolist() for _ in range(n_sets)]
    common = int(labs[len(labs) // 2])
    for s in range(min(n_sets, 64)):
        sets[s].append(common)
    if n_sets >= 128:
        for s in range(64, 128):
            sets[s].append(common)
    if not full:
        sets[0] = []
        sets[max(n_sets // 2 - 1, 0)] = []
    if not full or n_sets > 64:
        sets[-1] = []
    if n_sets >= 3:
        sets[1] = [int(x) for x in rng.choice(labs, min(len(labs), 400), replace=False)] + list(range(2000000, 2000600))
        sets[1] = sets[1][:1000] if len(sets[1]) >= 1000 else sets[1] + list(range(3000000, 3000000 + 1000 - len(sets[1])))
        if full:
            sets[1][0] = common
        sets[2] = [sets[2][0] if sets[2] else common] * 2 + sets[2]
        total = sum(len(x) for x in sets[:64])
        sets[2] += list(range(4000000, 4000000 + (1024 if total <= 1024 else 2048) - total))
    else:
        sets[0] = [common, common]
    return sets


def full_chunks(sets):
    """the chunks of 64 sets that all name one label: its table entry carries the mask of all 64 bits"""
    return [c for c in range(len(sets) // 64) if set.intersection(*(set(x) for x in sets[64 * c:64 * c + 64]))]


@pytest.fixture(scope="module")
def trees():
    posts = [fault_tree(s) for s in (137, 139, 151)] + [h[:2] for h in HAND[:2]]
    corpus = build(posts)
    rng = np.random.default_rng(3)  # labels shared between the graphs: 40 events in all
    corpus.label = np.ascontiguousarray(rng.integers(0, 40, len(corpus.label)), dtype=np.uint32)
    return corpus


@pytest.mark.parametrize("n_sets, full", [(1, False), (63, False), (64, False), (64, True), (65, False), (65, True), (129, False)])
def test_chunk_edges(eng, trees, n_sets, full):
    sets = edge_sets(trees, n_sets, n_sets, full)
    if n_sets >= 3:
        assert len(sets[1]) == 1000 and sum(len(x) for x in sets[:64]) in (1024, 2048)
        assert len(set(sets[2])) < len(sets[2]), "a label named twice in a set"
    if not full:
        assert sets[0] in ([], [sets[0][0]] * 2 if sets[0] else []) and (n_sets < 3 or (not sets[0] and not sets[-1] and [] in sets[1:-1]))
    if full or n_sets == 129:
        assert full_chunks(sets) == ([0] if full else [1]), "a label in all 64 sets of a chunk"
    out = everywhere(eng, Ref(trees), [int(x) for x in trees.iteration], sets, f"{n_sets} sets, full {full}")
    assert any(out[False][2]) or n_sets < 3, "some set is lost somewhere"
    if full or n_sets == 129:  # and the device saw the full mask: a graph that carries the label is hit by all 64 sets
        c = 0 if full else 1
        assert any(w[c] == 0xFFFFFFFFFFFFFFFF for w in out[False][1]), "no graph is hit by all 64 sets of the chunk"


# ---- list shapes, a run listed twice, persistence -------------------------------------------------------------------
@pytest.fixture(scope="module")
def seventy():
    return random_corpus(2024, n_runs=70, max_nodes=40)[0]


@pytest.mark.parametrize("n", [1, 3, 70])
def test_list_shapes(eng, seventy, n):
    its = [int(x) for x in seventy.iteration][:n]
    if n == 3:
        its = [its[2], its[0], its[2]]  # a run listed twice: identical rows, counted twice
    labs = sorted(set(seventy.label.tolist()))
    rng = np.random.default_rng(n)
    sets = [rng.choice(labs, int(rng.integers(1, 5))).tolist() for _ in range(70)]
    out = everywhere(eng, Ref(seventy), its, sets, f"{n} graphs")
    if n == 3:
        assert out[False][0][0] == out[False][0][2] and out[False][1][0] == out[False][1][2]
    if n == 70:
        sizes = {seventy.graph_size(2 * seventy.run_index(it) + 1) for it in its}
        assert len(sizes) > 10, "graphs of different sizes in one call"
        assert sum(out[False][3]) > 0 and sum(out[False][2]) > 0


def test_range_splitting(eng, trees):
    """2 graphs, 130 chunks: a graph's chunks are spread over several workgroups (kl_grid 3: two ranges each)"""
    labs = sorted(set(trees.label.tolist()))
    rng = np.random.default_rng(130)
    sets = [[int(labs[s % len(labs)])] if s < 2 * len(labs) else rng.choice(labs, int(rng.integers(1, 6))).tolist()
            for s in range(130 * 64)]
    its = [int(trees.iteration[0]), int(trees.iteration[2])]
    out = everywhere(eng, Ref(trees), its, sets, "130 chunks", sample=97)
    assert len(out[False][0][0]) == 130 and sum(out[False][2]) > 100


def test_one_workgroup_walks_graphs_of_different_sizes(eng):
    """kl_grid 1: a large graph, a small one, an empty one, the large one again, levels and rule bits all different;
    nothing of the previous graph may stay (hit list, rule bits, level offsets)"""
    h, l, c = hub(), level(), chains()
    posts = [h[:2], ("g", []), l[:2], ("", []), c[:2], ("gr", [(0, 1)])]
    corpus = build(posts)
    rng = np.random.default_rng(8)
    corpus.label = np.ascontiguousarray(rng.integers(0, 25, len(corpus.label)), dtype=np.uint32)
    its = [0, 1, 2, 3, 4, 5, 0, 4, 1, 2]
    sets = [[int(x)] for x in range(25)] + [rng.integers(0, 25, 3).tolist() for _ in range(45)]
    everywhere(eng, Ref(corpus), its, sets, "one workgroup, six graphs", grids=(1, 0))


# ---- sweep edges inside the persistent loop ----------------------------------------------------------------------------
@pytest.mark.parametrize("k, name", [(0, "a hub of 300 children"), (1, "a level of 600 nodes"), (2, "301 levels")])
def test_sweep_edges(eng, k, name):
    shapes = [hub(), level(), chains()]
    corpus = build([s[:2] for s in shapes])  # labels: the corpus-wide node index, so a set names nodes of one graph
    gr = Graph(corpus, 2 * k + 1)
    n0 = int(corpus.node_off[2 * k + 1])
    cand = shapes[k][2]
    sets = [[n0 + a, n0 + b] for i, a in enumerate(cand) for b in cand[:i]] + [[n0 + a] for a in cand]
    assert len(sets) >= 130
    out = everywhere(eng, Ref(corpus), [0, 1, 2], sets, name)
    assert sum(out[False][2]) >= 1 and (k != 2 or (gr.V == 601 and max(gr.pos) == gr.V - 1))


# ---- five seeded random corpora ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [1, 2, 3, 4, 5])
def test_random_corpora(eng, seed):
    corpus, _ = synth.generate(5, target_nodes=400, p_fault=0.5, prepend_run0=True, seed=seed)
    its = [int(x) for x in corpus.iteration]
    ref = Ref(corpus)
    g0 = ref.graph(2 * corpus.run_index(its[0]) + 1)
    rng = np.random.default_rng(seed)
    leaf_labels = sorted({g0.label[v] for v in g0.leaves})
    all_labels = sorted(set(corpus.label.tolist()))
    sets = [[int(x)] for x in leaf_labels[:80]]
    sets += [rng.choice(leaf_labels, int(rng.integers(2, 6))).tolist() for _ in range(40)]
    sets += [rng.choice(all_labels, int(rng.integers(1, 4))).tolist() for _ in range(40)] + [[]]
    # sets that do break runs: every sink label of run 0, the labels of its roots, large random parts of the sink labels
    sets += [[int(x) for x in leaf_labels], [int(g0.label[r]) for r in g0.roots]]
    sets += [rng.choice(leaf_labels, (3 * len(leaf_labels)) // 4, replace=False).tolist() for _ in range(6)]
    out = everywhere(eng, ref, its + [its[1]], sets, f"synth seed {seed}", sample=7)
    assert sum(out[False][3]) > len(its) and sum(out[False][2]) > 0 and sum(out[True][2]) > 0


# ---- the C3 shape ------------------------------------------------------------------------------------------------------------
def test_c3_shape(eng):
    """12 runs of the C3 shape, every run listed: 64 single-label sets from run 0's sink goals; form (A) over numpy
    words, form (B) on a sample"""
    corpus, _ = synth.generate(12, p_fault=0.55, prepend_run0=True, **synth.CONFIGS["c3"])
    its = [int(x) for x in corpus.iteration]
    ref = Ref(corpus)
    g0 = ref.graph(2 * corpus.run_index(its[0]) + 1)
    assert len(g0.leaves) > 2000
    labels = list(dict.fromkeys(g0.label[v] for v in g0.leaves))
    step = max(1, len(labels) // 64)
    sets = [[int(x)] for x in labels[::step][:64]]
    assert len(sets) == 64
    out = everywhere(eng, ref, its, sets, "c3, 64 sink labels", sample=16, numpy_form=True, grids=(0, 1, 3))
    assert sum(out[True][3]) >= 64, "every set hits run 0 at least"


def test_min_cut_rows_as_label_sets(eng):
    """The pair cuts nemo_min_cuts finds on the 2,953-leaf graph, turned into label sets: on their own graph every
    such set must be lost (device against device), on a second graph with other labels none is hit"""
    edges = [(0, 1), (0, 2)] + [(1, 3 + k) for k in (0, 1500, 2952)] + [(2, 3 + k) for k in range(2953) if k not in (0, 1500, 2952)]
    corpus = build([("grr" + "g" * 2953, edges), ("grg", [(0, 1), (1, 2)])])
    n0 = int(corpus.node_off[1])
    eng.load(corpus)
    cuts = eng.min_cuts(0, 1, None, 2)
    assert len(cuts) == 3 * 2950 and all(int(r["size"]) == 2 for r in cuts)
    sets = [[n0 + int(r["node"][0]), n0 + int(r["node"][1])] for r in cuts]  # build(): label = corpus-wide node index
    ck = (len(sets) + 63) // 64
    full = [0xFFFFFFFFFFFFFFFF] * (ck - 1) + [(1 << (len(sets) - 64 * (ck - 1))) - 1]
    want = ([full, [0] * ck], [full, [0] * ck], [1] * len(sets), [1] * len(sets))
    try:
        for lds in (-1, 0):
            for grid in GRIDS:
                eng.set_option("knock_lds_max", lds)
                eng.set_option("kl_grid", grid)
                for sinks in (False, True):
                    compare(eng, [0, 1], 1, sets, sinks, want, f"min-cut rows, knock_lds_max {lds}, kl_grid {grid}, sinks {sinks}")
    finally:
        eng.set_option("knock_lds_max", -1)
        eng.set_option("kl_grid", 0)
    ref = Ref(corpus)  # and the reference on a sample of them
    lo, hi, _, _ = ref.words(0, 1, sets[::59], False)
    assert lo == hi == (1 << len(sets[::59])) - 1


# ---- property: a union of two sets is lost wherever either is -------------------------------------------------------------
def test_union_is_monotone(eng):
    corpus, _ = synth.generate(6, target_nodes=600, p_fault=0.5, prepend_run0=True, seed=77)
    its = [int(x) for x in corpus.iteration]
    labs = sorted(set(corpus.label.tolist()))
    rng = np.random.default_rng(77)
    a = [rng.choice(labs, int(rng.integers(0, 30))).tolist() for _ in range(200)]
    b = [rng.choice(labs, int(rng.integers(0, 30))).tolist() for _ in range(200)]
    g0 = Graph(corpus, 1)
    n0 = int(corpus.node_off[1])
    a[0], b[0] = [int(corpus.label[n0 + v]) for v in g0.leaves], []  # a set that is lost on its own, joined with nothing
    eng.load(corpus)
    try:
        for lds in (-1, 0):
            for grid in GRIDS:
                eng.set_option("knock_lds_max", lds)
                eng.set_option("kl_grid", grid)
                for sinks in (False, True):
                    la, ha = eng.knockout_labels(its, 1, a, sinks_only=sinks)
                    lb, hb = eng.knockout_labels(its, 1, b, sinks_only=sinks)
                    lu, hu = eng.knockout_labels(its, 1, [x + y for x, y in zip(a, b)], sinks_only=sinks)
                    assert np.array_equal(hu, ha | hb)
                    assert np.array_equal(lu & (la | lb), la | lb)
                    assert (la | lb).any()
    finally:
        eng.set_option("knock_lds_max", -1)
        eng.set_option("kl_grid", 0)


# ---- a post graph of >= 65536 nodes: u32 rows, the global tier by size ------------------------------------------------------
def test_graph_past_65535_nodes(eng):
    corpus, _ = synth.generate(3, target_nodes=140000, p_fault=0.9, prepend_run0=True, seed=3, eot=80, body_extra=6,
                               nval=3, nloc=4)
    r = max(range(corpus.n_runs), key=lambda x: corpus.graph_size(2 * x + 1))
    ref = Ref(corpus)
    gr = ref.graph(2 * r + 1)
    assert gr.V >= 65536
    rng = np.random.default_rng(5)
    leaf_labels = sorted({gr.label[v] for v in gr.leaves})
    inner = sorted({gr.label[v] for v in range(gr.V) if gr.ch[v]})
    sets = [[int(x)] for x in rng.choice(leaf_labels, 30, replace=False)]
    sets += [rng.choice(inner, 2).tolist() for _ in range(20)] + [rng.choice(leaf_labels, 40).tolist() for _ in range(12)]
    sets += [[int(gr.label[v]) for v in gr.roots], [int(x) for x in leaf_labels], []]  # two sets that are lost
    assert len(sets) == 65
    it = int(corpus.iteration[r])
    eng.load(corpus)
    try:
        for sinks in (False, True):
            want = expect(ref, [it], 1, sets, sinks, sample=13, numpy_form=True)
            assert sum(want[2]) >= 1 and sum(want[3]) >= 40
            for lds in (-1, 0):  # the graph is past the LDS tier by its size under either
                for grid in GRIDS:
                    eng.set_option("knock_lds_max", lds)
                    eng.set_option("kl_grid", grid)
                    compare(eng, [it], 1, sets, sinks, want, f"66k nodes, sinks {sinks}, knock_lds_max {lds}, kl_grid {grid}")
    finally:
        eng.set_option("knock_lds_max", -1)
        eng.set_option("kl_grid", 0)


# ---- protocol ----------------------------------------------------------------------------------------------------------------
def raw(eng, iters, cond, off, labels, n_sets, flags=0):
    it = np.ascontiguousarray(iters, dtype=np.uint32)
    off = np.ascontiguousarray(off, dtype=np.uint64)
    labels = np.ascontiguousarray(labels, dtype=np.uint32)
    return eng.L.nemo_knockout_labels(eng.h, it.ctypes.data if len(it) else None, len(it), cond, off.ctypes.data,
                                      labels.ctypes.data if len(labels) else None, n_sets, flags)


def test_protocol(eng, hand, trees):
    eng.load(hand)
    w = np.zeros(64, np.uint64)
    assert eng.L.nemo_fetch_knockout_labels(eng.h, w.ctypes.data, w.ctypes.data, 64) == 5  # a fetch before any call
    assert eng.L.nemo_fetch_knockout_label_counts(eng.h, w.ctypes.data, w.ctypes.data, 64) == 5
    assert raw(eng, [0], 1, [0, 2, 1], [10, 11], 2) == 1 and "set_off decreases" in eng.L.nemo_last_error(eng.h).decode()
    assert raw(eng, [0], 1, [0, 2], [10, 0xFFFFFFFF], 1) == 1 and "UINT32_MAX" in eng.L.nemo_last_error(eng.h).decode()
    assert raw(eng, [0], 1, [0, 1], [10], 1, flags=2) == 1 and "flags" in eng.L.nemo_last_error(eng.h).decode()
    assert raw(eng, [0], 2, [0, 1], [10], 1) == 1 and "cond" in eng.L.nemo_last_error(eng.h).decode()
    assert raw(eng, [0, 4242], 1, [0, 1], [10], 1) == 7  # an iteration that is not loaded
    # the limits are read from the sizes: 2^32 labels named by a set_off over a two-label array, no label is read
    assert raw(eng, [0], 1, [0, 1, 1 << 32], [10, 11], 2) == 6 and "2^32 - 1 labels" in eng.L.nemo_last_error(eng.h).decode()
    # more than 2^32 - 1 sets: refused on n_sets alone, before set_off is read (the array here holds two offsets)
    assert raw(eng, [0], 1, [0, 0], [], 1 << 32) == 6 and "sets exceed" in eng.L.nemo_last_error(eng.h).decode()
    # n * n_chunks > 2^28 words: 2^22 + 1 list positions (run 0, over and over) x 64 chunks of empty sets
    assert raw(eng, np.zeros((1 << 22) + 1, np.uint32), 1, np.zeros(64 * 64 + 1, np.uint64), [], 64 * 64) == 6
    assert "2^28 words" in eng.L.nemo_last_error(eng.h).decode()
    assert eng.L.nemo_fetch_knockout_labels(eng.h, w.ctypes.data, w.ctypes.data, 64) == 5  # the failed calls left no result
    # zero words
    lost, hit = eng.knockout_labels([], 1, [[10]])
    assert lost.shape == (0, 1) and [x.tolist() for x in eng.knockout_label_counts()] == [[0], [0]]
    lost, hit = eng.knockout_labels([0, 1], 1, [])
    assert lost.shape == (2, 0) and [x.tolist() for x in eng.knockout_label_counts()] == [[], []]
    # a too-small cap
    ref = Ref(hand)
    compare(eng, [0, 1, 2], 1, HAND_SETS, False, expect(ref, [0, 1, 2], 1, HAND_SETS, False), "after the errors")
    assert eng.L.nemo_fetch_knockout_labels(eng.h, w.ctypes.data, w.ctypes.data, 2) == 1
    assert eng.L.nemo_fetch_knockout_labels(eng.h, w.ctypes.data, None, 3) == 0 and eng.L.nemo_fetch_knockout_labels(eng.h, None, None, 3) == 0
    assert eng.L.nemo_fetch_knockout_label_counts(eng.h, w.ctypes.data, w.ctypes.data, len(HAND_SETS) - 1) == 1
    # a node in the pre graph (cond 0): every pre graph is one goal of its own label
    lost, hit = eng.knockout_labels([0, 3], 0, [[900000], [900003], [900000, 900003]])
    assert lost.tolist() == hit.tolist() == [[0b101], [0b110]]
    eng.load(trees)  # a reload: no result of the previous corpus survives
    assert eng.L.nemo_fetch_knockout_labels(eng.h, w.ctypes.data, w.ctypes.data, 64) == 5
    assert eng.L.nemo_fetch_knockout_label_counts(eng.h, w.ctypes.data, w.ctypes.data, 64) == 5


def test_node_context_refuses(hand):
    node = E.Engine(devices=[0])
    try:
        node.load(hand)
        with pytest.raises(E.NemoError) as ei:
            node.knockout_labels([0], 1, [[10]])
        assert ei.value.code == 5 and "single-device contexts only" in ei.value.msg
    finally:
        node.close()


def test_buffers_grow_and_are_reused(eng, seventy):
    its = [int(x) for x in seventy.iteration]
    ref = Ref(seventy)
    labs = sorted(set(seventy.label.tolist()))
    rng = np.random.default_rng(5)
    eng.load(seventy)
    for n in (3, 70, 1, 130, 70):
        lst = [its[k % len(its)] for k in range(n)]
        sets = [rng.choice(labs, int(rng.integers(0, 4))).tolist() for _ in range(n + 5)]
        compare(eng, lst, 1, sets, False, expect(ref, lst, 1, sets, False), f"{n} list positions")


def test_other_results_are_left_alone(eng):
    corpus = random_corpus(1000, n_runs=6, max_nodes=40)[0]
    its = [int(x) for x in corpus.iteration]
    f = corpus.failed_iters() or its[1:3]
    labs = sorted(set(corpus.label.tolist()))
    sets = [[int(x)] for x in labs[:70]]
    eng.load(corpus)
    eng.mark()

    def others():
        return (np.array(eng.diff_masks(len(f))).copy(), eng.missing().copy(), [m.copy() for m in eng.sdiff_masks()],
                eng.surplus().copy(), eng.label_distances().copy(), eng.knockout_rows().copy(), eng.min_cut_rows().copy())

    def same(a, b):
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[3], b[3])
        assert len(a[2]) == len(b[2]) and all(np.array_equal(x, y) for x, y in zip(a[2], b[2]))
        assert np.array_equal(a[4], b[4]) and np.array_equal(a[5], b[5]) and np.array_equal(a[6], b[6])

    eng.diffprov(f, 1)
    eng.diffprov_symmetric(f)
    eng.nearest_runs(its, its)
    eng.knockout_leaves(its, 1)
    eng.min_cuts(its[0], 1, None, 2)
    before = others()
    ref = Ref(corpus)
    want = expect(ref, its, 1, sets, False)
    compare(eng, its, 1, sets, False, want, "between the other calls")
    same(before, others())  # their fetches, unchanged by the label call between them
    eng.diffprov(f, 1)
    eng.diffprov_symmetric(f)
    eng.nearest_runs(its, its)
    eng.knockout_leaves(its, 1)
    eng.knockout_sets(its[0], 1, [[0]])
    eng.min_cuts(its[0], 1, None, 2)
    w = np.zeros((len(its), (len(sets) + 63) // 64), np.uint64)
    h = np.zeros(w.shape, np.uint64)
    assert eng.L.nemo_fetch_knockout_labels(eng.h, w.ctypes.data, h.ctypes.data, w.size) == 0  # and the reverse
    assert w.tolist() == want[0] and h.tolist() == want[1]
