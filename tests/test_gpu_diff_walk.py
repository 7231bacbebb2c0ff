"""The three level-sweep diff kernels share one walk (nemo_amd/csrc/diff_walk.h): every instantiation of it is
pinned to one reference on the same graphs, and so to each other.

Reference: tests/test_gpu_sdiff.Want (the oracle on the role-exchanged two-run corpus), imported, not rewritten.
Per case the S masks and the sorted rule rows of
  nemo_diffprov_symmetric(entries) and nemo_diffprov_pairs(entries, [0, ...])          (TABS false / true)
  under graph_lds_max -1 (k_sdiff_lds) and 0 with global_block 256 and 1024 (k_sdiff_glob<256>, <1024>),
  nemo_diffprov under diff_legacy 1 on swapped(corpus, entry's run)                     (k_diff_lds)
must equal the reference.

Which case reaches which instantiation (worked out below from diff_lds_bytes and the corpus sizes, and asserted):
  k_sdiff_lds<DLDS false, TABS false/true>   every hand-built case: the image of the hand corpus is a few KB, so
                                             the 2V bytes of depths would cost workgroups per CU and stay in HBM
  k_sdiff_lds<DLDS true, TABS false/true>    c3_12 only: 55.5 KB image, two workgroups per CU with or without depths
  k_sdiff_glob<256 / 1024, TABS false/true>  every case (graph_lds_max 0 sends every entry to the global tier)
  k_diff_lds                                 every case (the exchanged two-run corpus is inside the tier's caps)
The strided loops take a second trip in wide_257 (block 256) and wide_1025 (block 1024).
"""
import numpy as np
import pytest

from nemo_amd import engine as E
from nemo_amd.corpus import DIFF_PER_RUN, corpus_from_graphs
from tests.test_gpu_pairs import PRE, _flat, _goal, _lab
from tests.test_gpu_sdiff import Want, _rows, c3_12, swapped  # noqa: F401  (c3_12: the 12-run C3-shaped fixture)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    e = E.Engine(0)
    yield e
    e.close()


# ---- the tier's sizing, as the load does it (api.hip fit_tier / set_lds_tier, k_sdiff.hip launch_sdiff_t) -------
def _align(b):
    return (b + 15) & ~15


def diff_lds_bytes(v, e):  # device.h
    return 2 * _align(2 * (v + 1)) + 2 * _align(2 * e) + _align(4 * ((v + 31) // 32)) + _align(v)


def tier(corpus):
    """t_diff's caps (V, E) and image bytes: graphs by size while the image stays inside the 78 KB budget."""
    ve = sorted((corpus.graph_size(g), int(corpus.edge_off[g + 1] - corpus.edge_off[g]))
                for g in range(corpus.n_graphs))
    cv = ce = em = 0
    for v, e in ve:
        if v > 16384 or e > 65535:
            continue
        em = max(em, e)
        if diff_lds_bytes(v, em) > 78 * 1024:
            break
        cv, ce = v, em
    return cv, ce, diff_lds_bytes(cv, ce)


def reaches(corpus, graphs):
    """(every graph of `graphs` is inside the LDS tier, the LDS tier keeps its depths in LDS)."""
    cv, ce, b = tier(corpus)
    fits = all(corpus.graph_size(g) <= cv and int(corpus.edge_off[g + 1] - corpus.edge_off[g]) <= ce for g in graphs)
    return fits, (160 * 1024) // (b + _align(2 * cv)) == (160 * 1024) // b


# ---- hand-built entry graphs: goal labels K(k) are run 0's (not Bad), B(k) are not (Bad) -----------------------
def K(k):
    return _lab(k)


def B(k):
    return _lab(1000 + k)


def _graph(labels, n_rules, edges):
    """Goals g0.. with `labels`, rules r0..; edges as ("g0", "r0") pairs, parent first."""
    name = lambda x: ("goal" if x[0] == "g" else "rule") + x[1:]
    return {"goals": [_goal(i, l) for i, l in enumerate(labels)],
            "rules": [{"id": f"rule{i}", "label": "t1", "table": "t1", "type": "single"} for i in range(n_rules)],
            "edges": [{"from": name(a), "to": name(b)} for a, b in edges]}


def _path(labels):
    n = len(labels)
    return _graph(labels, n - 1, [e for i in range(n - 1) for e in ((f"g{i}", f"r{i}"), (f"r{i}", f"g{i + 1}"))])


def _wide(n):
    """One Bad root, a level of n rules, a level of n goals (every other one Bad): half the rules tie at the top."""
    edges = [e for i in range(n) for e in (("g0", f"r{i}"), (f"r{i}", f"g{i + 1}"))]
    return _graph([B(0)] + [B(i) if i % 2 else K(i % 90) for i in range(1, n + 1)], n, edges)


# name -> (post graph, surplus rules the reference must report: the case is what it claims to be)
CASES = {
    "one_node": (_graph([B(0)], 0, []), 0),
    "empty_seed": (_path([K(0), K(1), K(2)]), 0),
    # goal -> rule -> goal ..., nine Kahn levels, Bad at both ends
    "chain": (_path([B(0), K(1), K(2), K(3), B(4)]), 1),
    # r0 (depth 1) has the leaf children g1 and g5, and g5 is reached again below r2 (depth 3);
    # r2 and r3 tie at the maximal depth: both are emitted, r0 is not
    "leaf_depths_and_tie": (_graph([B(0), B(1), K(2), B(3), B(4), B(5)], 4,
                                   [("g0", "r0"), ("r0", "g1"), ("r0", "g5"), ("g0", "r1"), ("r1", "g2"),
                                    ("g2", "r2"), ("r2", "g3"), ("r2", "g5"), ("g2", "r3"), ("r3", "g4")]), 2),
    # r0 is inside S, its childless child g3 is not: only r1 has an S-leaf child
    "leaf_outside": (_graph([B(0), K(1), B(2), K(3)], 2,
                            [("g0", "r0"), ("r0", "g1"), ("r0", "g3"), ("g1", "r1"), ("r1", "g2")]), 1),
    # g1 is inside S with one child inside (r1) and one outside (r2): no leaf
    "goal_not_leaf": (_graph([B(0), B(1), B(2), K(3)], 3,
                             [("g0", "r0"), ("r0", "g1"), ("g1", "r1"), ("r1", "g2"), ("g1", "r2"), ("r2", "g3")]), 1),
    # r0 has three parents and three children, g3 three children, g6 three parents
    "fan": (_graph([B(0), B(1), K(2), B(3), K(4), B(5), B(6)], 4,
                   [("g0", "r0"), ("g1", "r0"), ("g2", "r0"), ("r0", "g3"), ("r0", "g4"), ("r0", "g5"),
                    ("g3", "r1"), ("g3", "r2"), ("g3", "r3"), ("r1", "g6"), ("r2", "g6"), ("r3", "g6")]), 3),
    "wide_257": (_wide(257), 129),
    "wide_1025": (_wide(1025), 513),
}
NAMES = list(CASES)


@pytest.fixture(scope="module")
def hand():
    runs = [(0, "success", PRE, _flat([K(k) for k in range(100)]))]
    runs += [(1 + i, "fail", PRE, CASES[n][0]) for i, n in enumerate(NAMES)]
    corpus = corpus_from_graphs(runs)
    assert corpus.graph_size(2 * corpus.run_index(1 + NAMES.index("wide_257")) + 1) == 2 * 257 + 1
    assert corpus.graph_size(2 * corpus.run_index(1 + NAMES.index("wide_1025")) + 1) == 2 * 1025 + 1
    return corpus


def _same(got, want: Want, what):
    masks, rows = got
    assert len(masks) == len(want.masks), what
    bad = [e for e in range(len(masks)) if not np.array_equal(masks[e], want.masks[e])]
    assert not bad, f"{what}: S masks of entries {bad[:8]} differ ({len(bad)} of {len(masks)})"
    assert np.array_equal(rows, want.rows), f"{what}: rule rows differ"


def check_walks(eng, corpus, want: Want, depths_in_lds):
    n = len(want.entries)
    fits, dlds = reaches(corpus, want.graphs)
    assert fits and dlds == depths_in_lds, "the case no longer reaches the k_sdiff_lds instantiation it is named for"
    eng.load(corpus)
    eng.mark()
    try:
        for lds_max, block in ((-1, -1), (0, 256), (0, 1024)):
            eng.set_option("graph_lds_max", lds_max)
            eng.set_option("global_block", block)
            eng.diffprov_symmetric(want.entries)
            _same((eng.sdiff_masks(), _rows(eng.surplus())), want, f"symmetric, lds {lds_max}, block {block}")
            eng.diffprov_pairs(want.entries, [0] * n)
            _same((eng.sdiff_masks(), _rows(eng.surplus())), want, f"pairs, lds {lds_max}, block {block}")
    finally:
        eng.set_option("graph_lds_max", -1)
        eng.set_option("global_block", -1)
    # k_diff_lds: the entry's run as run 0, run 0 as the one failed run
    done = set()
    try:
        eng.set_option("diff_legacy", 1)
        for e, it in enumerate(want.entries):
            rf = corpus.run_index(it)
            if rf in done:
                continue
            done.add(rf)
            two = swapped(corpus, rf)
            assert reaches(two, [1])[0]
            eng.load(two)
            eng.mark()
            eng.diffprov([1], DIFF_PER_RUN)
            assert np.array_equal(eng.diff_masks(1)[0], want.masks[e]), f"k_diff_lds: D mask of entry {e} differs"
            assert np.array_equal(_rows(eng.missing())[:, 1], want.rows[want.rows[:, 0] == e][:, 1]), \
                f"k_diff_lds: rule rows of entry {e} differ"
    finally:
        eng.set_option("diff_legacy", 0)


@pytest.mark.parametrize("name", NAMES)
def test_hand_built(eng, hand, name):
    want = Want(hand, [1 + NAMES.index(name)])
    assert len(want.rows) == CASES[name][1]
    assert want.masks[0].any() == (name != "empty_seed")
    check_walks(eng, hand, want, depths_in_lds=False)


def test_65_entries(eng, hand):
    # past the 64-entry chunk of the per-entry buffers, and more entries than one round of workgroups
    small = [1 + i for i, n in enumerate(NAMES) if not n.startswith("wide")]
    want = Want(hand, [small[k % len(small)] for k in range(65)])
    check_walks(eng, hand, want, depths_in_lds=False)


def test_c3_shape_depths_in_lds(eng, c3_12):  # noqa: F811
    ex, want = c3_12
    assert len(want.entries) >= 2 and all(want.nonempty())
    check_walks(eng, ex, want, depths_in_lds=True)
