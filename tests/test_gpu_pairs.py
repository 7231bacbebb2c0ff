"""GPU parity of differential provenance between arbitrary pairs of runs (nemo_diffprov_pairs; k_lab_hash and
the k_sdiff kernels in nemo_amd/csrc/k_sdiff.hip): S masks, surplus events and the induced edge lists
(nemo_pull_edges(3)) of every entry, bit-exact.

Reference.  The diff of the pair (base, other) is by definition the ordinary per-run diff
(differential-provenance.go:22-28,82-98) of a two-run corpus [base as iteration 0 / success, other as iteration 1 /
fail]: the existing oracle (oracle/nemo_oracle.c, diff-only, per-run mode) on corpus.subset([run(base), run(other)])
gives S_e as its D mask and the entry's surplus rules as its missing rules; the induced edges come from the corpus
arrays.  The equivalences with nemo_diffprov_symmetric and nemo_diffprov are checked device against device.

Inputs must exercise the walk.  Every test asserts from the ORACLE masks that its input is not empty: every (good
base, failed other) entry at generator shapes, at least 90 % of the pairs against a failed run on the random
corpora (the bar of tests/test_gpu_sdiff.py), every pair named non-empty in the hand-built cases; (x, x) is
asserted empty.
"""
import numpy as np
import pytest

from nemo_amd import engine as E
from nemo_amd.corpus import DIFF_PER_RUN, NODE_RULE, Corpus, corpus_from_graphs
from oracle import oracle as O
from tests.test_gpu_sdiff import DEEP, _rows, _with_iterations, induced, role_exchanged
from tools import synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    e = E.Engine(0)
    yield e
    e.close()


class Want:
    """The oracle's results of `pairs` [(base iteration, other iteration), ...] on `corpus`."""

    def __init__(self, corpus: Corpus, pairs):
        self.corpus, self.pairs = corpus, [(int(b), int(o)) for b, o in pairs]
        self.base = [b for b, _ in self.pairs]
        self.other = [o for _, o in self.pairs]
        per_pair = {}
        self.masks, rows, self.edges, self.graphs = [], [], [], []
        for e, (b, o) in enumerate(self.pairs):
            rb, ro = corpus.run_index(b), corpus.run_index(o)
            if (rb, ro) not in per_pair:  # duplicate pairs share one oracle run
                two = corpus.subset([rb, ro])
                two.iteration = np.array([0, 1], np.uint32)
                two.status = ["success", "fail"]
                orc = O.analyze(two, [0], [1], diff_mode=DIFF_PER_RUN, threads=4, diff_only=True)
                per_pair[(rb, ro)] = (np.asarray(orc.diff_mask[0], np.uint8), _rows(orc.missing)[:, 1])
            m, rules = per_pair[(rb, ro)]
            g = 2 * rb + 1
            assert len(m) == corpus.graph_size(g)
            self.graphs.append(g)
            self.masks.append(m)
            rows += [(e, int(r)) for r in rules]
            self.edges.append(induced(corpus, g, m))
        self.rows = _rows(rows)

    def nonempty(self):
        return [bool(m.any()) for m in self.masks]


def fetch(eng, n):
    """(masks, surplus rows, [(src, dst) per slot]) of the last symmetric / pairs call."""
    masks, rows = eng.sdiff_masks(), _rows(eng.surplus())
    assert len(masks) == n
    eng.pull(3)
    off, cnt, src, dst = eng.pulled_all(n)
    edges = [(src[int(a):int(a) + int(k)].copy(), dst[int(a):int(a) + int(k)].copy()) for a, k in zip(off, cnt)]
    return masks, rows, edges


def check_pairs(eng, want: Want):
    n = len(want.pairs)
    eng.diffprov_pairs(want.base, want.other)
    masks, rows, edges = fetch(eng, n)
    bad = [e for e in range(n) if not np.array_equal(masks[e], want.masks[e])]
    assert not bad, f"S masks of entries {bad[:8]} differ ({len(bad)} of {n}): pairs {[want.pairs[e] for e in bad[:8]]}"
    assert np.array_equal(rows, want.rows), "surplus rows differ"
    for e in range(n):
        ws, wd = want.edges[e]
        assert np.array_equal(edges[e][0], ws) and np.array_equal(edges[e][1], wd), f"pull 3, slot {e} differs"
    for e in sorted({0, n // 2, n - 1}) if n else []:
        s, d = eng.pulled(e)
        assert np.array_equal(s, want.edges[e][0]) and np.array_equal(d, want.edges[e][1]), \
            f"pull 3, slot {e} (fetch_pulled) differs"


def all_paths(eng, want: Want):
    """Both sdiff tiers (graph_lds_max -1 / 0) under both table builds (pair_hash_lds_max -1 / 0)."""
    try:
        for hash_lds in (-1, 0):
            eng.set_option("pair_hash_lds_max", hash_lds)
            for graph_lds in (-1, 0):
                eng.set_option("graph_lds_max", graph_lds)
                check_pairs(eng, want)
    finally:
        eng.set_option("pair_hash_lds_max", -1)
        eng.set_option("graph_lds_max", -1)


def both_hash_paths(eng, want: Want):
    try:
        for hash_lds in (-1, 0):
            eng.set_option("pair_hash_lds_max", hash_lds)
            check_pairs(eng, want)
    finally:
        eng.set_option("pair_hash_lds_max", -1)


def load(eng, corpus):
    eng.load(corpus)
    eng.mark()


# ---- 1. random small corpora: every ordered pair ----------------------------------------------------
def _random_corpora(seed):
    from tests.small import random_corpus
    return [random_corpus(1000 * seed + k, n_runs=5, max_nodes=40)[0] for k in range(3)]


@pytest.mark.parametrize("seed", range(4))
def test_random_corpora_every_ordered_pair(eng, seed):
    vs_failed = []
    for corpus in _random_corpora(seed):
        its = [int(x) for x in corpus.iteration]
        want = Want(corpus, [(b, o) for b in its for o in its])
        ne = want.nonempty()
        for e, (b, o) in enumerate(want.pairs):
            if b == o:
                assert not ne[e], "a run against itself has no Bad goal"
            elif corpus.status[corpus.run_index(o)] != "success":
                vs_failed.append(ne[e])
        load(eng, corpus)
        all_paths(eng, want)
    assert vs_failed and sum(vs_failed) >= 0.9 * len(vs_failed), \
        f"only {sum(vs_failed)} of {len(vs_failed)} pairs against a failed run have a non-empty oracle S"


# ---- 2. equivalences with the two run-0 diffs ----------------------------------------------------------
def _same_as_symmetric(eng, entries):
    eng.diffprov_symmetric(entries)
    sm, sr, se = fetch(eng, len(entries))
    eng.diffprov_pairs(entries, [0] * len(entries))
    pm, pr, pe = fetch(eng, len(entries))
    assert all(np.array_equal(a, b) for a, b in zip(sm, pm)), "pairs(f, 0) masks differ from the symmetric diff's"
    assert np.array_equal(sr, pr), "pairs(f, 0) surplus rows differ from the symmetric diff's"
    assert all(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) for a, b in zip(se, pe)), "pulls differ"
    return sm


def _same_as_diffprov(eng, failed):
    eng.diffprov(failed, DIFF_PER_RUN)
    dm, dr = eng.diff_masks(len(failed)), _rows(eng.missing())
    eng.diffprov_pairs([0] * len(failed), failed)
    pm, pr = eng.sdiff_masks(), _rows(eng.surplus())
    assert len(pm) == len(failed)
    assert all(np.array_equal(dm[e], pm[e]) for e in range(len(failed))), "pairs(0, f) masks differ from the D masks"
    assert np.array_equal(dr, pr), "pairs(0, f) surplus rules differ from the missing rules"
    assert np.array_equal(eng.diff_masks(len(failed)), dm), "the pairs call disturbed nemo_diffprov's results"
    return dm


@pytest.fixture(scope="module")
def c3_12():
    corpus, _ = synth.generate(12, p_fault=0.55, prepend_run0=True, **synth.CONFIGS["c3"])
    return corpus


def test_equivalences_random(eng):
    # one loaded corpus whose failed runs have Bad goals both ways
    corpus = _random_corpora(1)[0]
    f = corpus.failed_iters()
    its = [int(x) for x in corpus.iteration]
    assert f and 0 in its
    assert any(Want(corpus, [(x, 0) for x in f]).nonempty()) and any(Want(corpus, [(0, x) for x in f]).nonempty())
    load(eng, corpus)
    _same_as_symmetric(eng, its + [f[0]])
    _same_as_diffprov(eng, f + [f[0]])


def test_equivalences_c3(eng, c3_12):
    # (iteration 0, f) on the generator corpus: every failed run lacks part of run 0's provenance
    f = c3_12.failed_iters()
    assert len(f) >= 2 and all(Want(c3_12, [(0, x) for x in f]).nonempty())
    load(eng, c3_12)
    dm = _same_as_diffprov(eng, f)
    assert all(m.any() for m in dm)
    # (f, iteration 0) on the role-exchanged corpus (the generator's failed runs derive a subset of run 0's labels)
    ex, entries = role_exchanged(c3_12)
    assert all(Want(ex, [(x, 0) for x in entries]).nonempty())
    load(eng, ex)
    sm = _same_as_symmetric(eng, entries)
    assert all(m.any() for m in sm)


# ---- 3. table corner cases on hand-built graphs ---------------------------------------------------------
def _goal(i, label, table="t1"):
    return {"id": f"goal{i}", "label": label, "table": table, "time": "1"}


def _lab(k):
    return f"t1(a, {k})"


def _flat(labels):
    """A post graph of goals alone (no rule, no edge): only its label set matters to a diff against it."""
    return {"goals": [_goal(i, l) for i, l in enumerate(labels)], "rules": [], "edges": []}


def _chain(labels):
    """goal0 -> rule0 -> goal1 -> ... -> goal{n-1}: 2n - 1 nodes; every Bad goal puts a stretch of the chain in S."""
    n = len(labels)
    rules = [{"id": f"rule{i}", "label": "t1", "table": "t1", "type": "single"} for i in range(n - 1)]
    edges = []
    for i in range(n - 1):
        edges += [{"from": f"goal{i}", "to": f"rule{i}"}, {"from": f"rule{i}", "to": f"goal{i + 1}"}]
    return {"goals": [_goal(i, l) for i, l in enumerate(labels)], "rules": rules, "edges": edges}


PRE = {"goals": [{"id": "goal0", "label": "pre(a)", "table": "pre", "time": "1"}], "rules": [], "edges": []}
NO_GOAL, REPEATED, L33, L1025, FIRST_BASE, N_BASE = 1, 2, 3, 4, 10, 8


@pytest.fixture(scope="module")
def hand():
    """Run 0, four `other` runs (no goal; one label on several goals; 33 and 1025 distinct labels: tables of 128
    and 4096 slots, so probe chains form) and eight base runs of 19 nodes whose chains mix labels inside and
    outside every one of those sets."""
    runs = [(0, "success", PRE, _chain([_lab(k) for k in range(6)])),
            (NO_GOAL, "fail", PRE, {"goals": [], "rules": [{"id": "rule0", "label": "t1", "table": "t1",
                                                            "type": "single"}], "edges": []}),
            (REPEATED, "fail", PRE, _flat([_lab(7)] * 5 + [_lab(3)] * 2 + [_lab(40)])),
            (L33, "fail", PRE, _flat([_lab(k) for k in range(33)])),
            (L1025, "fail", PRE, _flat([_lab(k) for k in range(1025)]))]
    for j in range(N_BASE):
        labels = [_lab((131 * j + 97 * i * i + 5 * i) % 1400) for i in range(7)] + [_lab(7), _lab(3), _lab(j)]
        runs.append((FIRST_BASE + j, "success" if j % 2 else "fail", PRE, _chain(labels)))
    corpus = corpus_from_graphs(runs)
    assert corpus.graph_size(2 * corpus.run_index(L33) + 1) == 33
    assert corpus.graph_size(2 * corpus.run_index(L1025) + 1) == 1025
    assert all(corpus.graph_size(2 * corpus.run_index(FIRST_BASE + j) + 1) == 19 for j in range(N_BASE))
    return corpus


BASES = [FIRST_BASE + j for j in range(N_BASE)]


def test_other_without_a_goal(eng, hand):
    want = Want(hand, [(b, NO_GOAL) for b in BASES])
    for e, b in enumerate(BASES):  # every base goal is Bad
        g = want.graphs[e]
        goals = (hand.node_word[int(hand.node_off[g]):int(hand.node_off[g + 1])] & np.uint32(NODE_RULE)) == 0
        assert goals.sum() == 10 and want.masks[e][goals].all()
    load(eng, hand)
    all_paths(eng, want)


def test_other_with_one_label_on_several_goals(eng, hand):
    want = Want(hand, [(b, REPEATED) for b in BASES] + [(REPEATED, b) for b in BASES])
    assert all(want.nonempty())
    load(eng, hand)
    all_paths(eng, want)


@pytest.mark.parametrize("other", [L33, L1025])
def test_probe_chains_many_entries_share_one_other(eng, hand, other):
    # 33 labels in 128 slots, 1025 in 4096: members are found past occupied slots, strangers end on an empty one
    want = Want(hand, [(b, other) for b in BASES] * 3)
    ne = want.nonempty()
    assert all(ne) and not all(m.all() for m in want.masks), "every entry must hold labels inside and outside the set"
    load(eng, hand)
    all_paths(eng, want)


def test_every_entry_its_own_other_and_duplicates(eng, hand):
    its = [int(x) for x in hand.iteration]
    pairs = [(its[(k + 3) % len(its)], its[k]) for k in range(len(its))]  # every run once as `other`, run 0 included
    pairs += [(x, x) for x in its[:4]] + pairs[:5] + [pairs[2]] * 3  # (x, x), duplicate pairs
    want = Want(hand, pairs)
    ne = want.nonempty()
    assert sum(ne) >= len(its) // 2 and not any(ne[len(its):len(its) + 4])
    load(eng, hand)
    all_paths(eng, want)
    k = len(its) + 4
    masks = eng.sdiff_masks()
    assert all(np.array_equal(masks[k + d], masks[d]) for d in range(5))
    assert all(np.array_equal(masks[k + 5 + d], masks[2]) for d in range(3))


def test_no_entry_and_errors(eng, hand):
    load(eng, hand)
    eng.diffprov_pairs([], [])
    assert eng.sdiff_masks() == [] and len(eng.surplus()) == 0
    eng.pull(3)
    assert eng.pulled_all(0)[2].size == 0
    for base, other in (([BASES[0], 4242], [L33, L33]), ([BASES[0], BASES[1]], [L33, 4242])):
        with pytest.raises(E.NemoError) as ei:
            eng.diffprov_pairs(base, other)
        assert ei.value.code == 7 and "unknown run iteration 4242" in ei.value.msg
        with pytest.raises(E.NemoError) as ei:  # the failed call left no result
            eng.surplus()
        assert ei.value.code == 5
    eng.load(hand)
    with pytest.raises(E.NemoError) as ei:  # before mark
        eng.diffprov_pairs([BASES[0]], [L33])
    assert ei.value.code == 5 and "nemo_diffprov_pairs before nemo_mark_holds" in ei.value.msg


def test_run_0_need_not_be_loaded(eng, hand):
    no0 = _with_iterations(hand, hand.iteration + np.uint32(1))
    want = Want(no0, [(b + 1, o + 1) for b in BASES[:4] for o in (L33, L1025, 0)])
    assert all(want.nonempty())
    load(eng, no0)
    both_hash_paths(eng, want)


def test_node_context_refuses(hand):
    node = E.Engine(devices=[0])
    try:
        node.load(hand)
        node.mark()
        with pytest.raises(E.NemoError) as ei:
            node.diffprov_pairs([BASES[0]], [L33])
        assert ei.value.code == 5 and "single-device contexts only" in ei.value.msg
    finally:
        node.close()


# ---- 4. C3 shape: one launch over about 60 entries -----------------------------------------------------
def test_c3_shape(eng, c3_12):
    its = [int(x) for x in c3_12.iteration]
    good = [it for it in its if c3_12.status[c3_12.run_index(it)] == "success"]
    failed = c3_12.failed_iters()
    gf = [(g, f) for g in good for f in failed][:24]
    fg = [(f, g) for g in good for f in failed][:18]
    gg = [(a, b) for a in good for b in good if a != b][:18]
    assert len(gf) >= 12 and len(fg) >= 12 and len(gg) >= 12
    want = Want(c3_12, gf + fg + gg)
    assert all(want.nonempty()[:len(gf)]), "a good run holds provenance every failed run lacks"
    load(eng, c3_12)
    all_paths(eng, want)


# ---- 5. deep shape: u32 rows, the global sdiff tier, a table past the LDS budget -------------------------
def test_deep_shape_each_way(eng):
    corpus, _ = synth.generate(3, target_nodes=140000, p_fault=0.9, prepend_run0=True, seed=3, **dict(DEEP, eot=80))
    f = corpus.failed_iters()
    good = [int(it) for it in corpus.iteration if int(it) != 0 and int(it) not in f]
    assert f and good, "the three runs hold run 0, another good run and a failed one"
    want = Want(corpus, [(good[0], f[0]), (f[0], good[0])])
    # the good run's post graph has u32 rows (66,239 nodes; the failed run's 60,205); both tables are past the
    # 16,384-slot LDS budget, and neither `other` is iteration 0, so both are built
    assert corpus.graph_size(want.graphs[0]) >= 65536 and corpus.graph_size(want.graphs[1]) >= 32768
    assert want.nonempty()[0]
    load(eng, corpus)
    both_hash_paths(eng, want)


# ---- 6. lifetime: the results are the loaded corpus' -----------------------------------------------------
def test_results_follow_the_loaded_corpus(eng, hand):
    a = _random_corpora(2)[0]
    ia = [int(x) for x in a.iteration]
    want_a = Want(a, [(b, o) for b in ia for o in ia if b != o])
    pairs_b = [(b, o) for b in BASES for o in (L33, L1025)]
    want_b = Want(hand, pairs_b)
    assert any(want_a.nonempty()) and all(want_b.nonempty())
    load(eng, a)
    check_pairs(eng, want_a)
    eng.load(hand)
    for call in (eng.sdiff_masks, eng.surplus, lambda: eng.pull(3)):
        with pytest.raises(E.NemoError) as ei:  # no result of the previous corpus survives the load
            call()
        assert ei.value.code == 5
    eng.mark()
    check_pairs(eng, want_b)


# ---- the host mirror: Neo4J.PairDiffProv on a case-study fixture -------------------------------------------
def test_graphing_pair_diffprov_fixture():
    import os
    from nemo_amd import graphing as GR
    from nemo_amd.corpus import load_molly
    d = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cs_ca_2434_bootstrap_synchronization")
    corpus = load_molly(d)
    f = corpus.failed_iters()
    pairs = [(x, 0) for x in f] + [(0, x) for x in f]
    want = Want(corpus, pairs)
    assert any(want.nonempty()[:len(f)]) and all(want.nonempty()[len(f):])
    db = GR.Neo4J()
    db.InitGraphDB("bolt://127.0.0.1:7687", corpus)
    try:
        db.LoadRawProvenance()
        db.SimplifyProv([int(x) for x in corpus.iteration])
        _, post, _, _ = db.PullPrePostProv()
        _, faileds, _ = db.CreateNaiveDiffProv(True, f, post[0])
        surplus = [list(x) for x in db.SurplusEvents]
        recs = db.PairDiffProv(pairs)
    finally:
        db.CloseDB()
    assert [(r["Base"], r["Other"]) for r in recs] == pairs
    for e in range(len(f)):  # (f, 0) is CreateNaiveDiffProv(True, ...)'s record of f
        assert recs[e]["Dot"].string() == faileds[e].string()
        assert [m.Rule.ID for m in recs[e]["Surplus"]] == [m.Rule.ID for m in surplus[e]]
    for e, rec in enumerate(recs):
        g, n0 = want.graphs[e], int(corpus.node_off[want.graphs[e]])
        ids = {corpus.node_ids[n0 + int(i)] for i in np.nonzero(want.masks[e])[0]}
        assert {k for k, a in rec["Dot"].nodes.items() if a.get("penwidth") == '"3"'} == ids
        assert sum(1 for x in rec["Dot"].edges if x.attrs.get("penwidth") == '"3"') == len(want.edges[e][0])
        rules = sorted(corpus.node_ids[n0 + int(r)] for en, r in want.rows if en == e)
        assert sorted(m.Rule.ID for m in rec["Surplus"]) == rules
