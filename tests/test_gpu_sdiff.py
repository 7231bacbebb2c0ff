"""GPU parity of the symmetric differential provenance (nemo_amd/csrc/k_sdiff.hip, nemo_diffprov_symmetric):
S masks, surplus events and the induced edge lists (nemo_pull_edges(3)) of every entry, bit-exact.

Reference.  The symmetric diff of (run 0, run f) is by definition the ordinary per-run diff
(differential-provenance.go:22-28,82-98) with the two runs exchanged.  So for every entry a two-run corpus
[run f as iteration 0 / success, run 0 as iteration 1 / fail] goes through the existing oracle
(oracle/nemo_oracle.c, diff-only, per-run mode): its D mask must equal S_e and its missing rules the entry's
surplus rules.  One shape is also compared with the device's own nemo_diffprov on the exchanged corpus.

Inputs must have non-empty S.  The generator's failed runs derive a subset of run 0's labels (no Bad goal), so
generator-shape corpora are loaded role-exchanged: one failed (sparse) run becomes iteration 0 and the good
runs are the entries.  Every test asserts the condition on its own input from the ORACLE masks: every entry
non-empty at generator shapes, at least 90 % of the failed-run entries on the random corpora.
"""
import dataclasses

import numpy as np
import pytest

from nemo_amd import engine as E
from nemo_amd.corpus import DIFF_PER_RUN, Corpus
from oracle import oracle as O
from tools import synth

pytestmark = pytest.mark.gpu

DEEP = dict(eot=40, body_extra=6, nval=3, nloc=4)  # test_gpu_diff.test_deep_shape's generator arguments


@pytest.fixture(scope="module")
def eng():
    e = E.Engine(0)
    yield e
    e.close()


def _rows(m):
    m = np.asarray(m, np.int64).reshape(-1, 2)
    return m[np.lexsort((m[:, 1], m[:, 0]))]


def _with_iterations(corpus: Corpus, iteration) -> Corpus:
    return dataclasses.replace(corpus, iteration=np.ascontiguousarray(iteration, dtype=np.uint32))


def role_exchanged(corpus: Corpus):
    """The corpus with its first failed run as iteration 0, and the entries: the original run 0 and every
    other successful run (by their iterations in the exchanged corpus)."""
    it = corpus.iteration.astype(np.int64).copy()
    r0 = corpus.run_index(0)
    rf = next(r for r in range(corpus.n_runs) if corpus.status[r] != "success")
    it[r0], it[rf] = it[rf], 0
    ex = _with_iterations(corpus, it)
    entries = [int(it[r]) for r in range(corpus.n_runs) if corpus.status[r] == "success"]
    return ex, entries


def concat(a: Corpus, b: Corpus, shift: int) -> Corpus:
    """Runs of a, then runs of b with their iterations shifted (same table universe: tools/synth.py)."""
    assert (a.n_tables, a.table_pre, a.table_post) == (b.n_tables, b.table_pre, b.table_post)
    cat = lambda x, y: np.ascontiguousarray(np.concatenate([x, y]))
    return Corpus(iteration=cat(a.iteration, b.iteration + np.uint32(shift)),
                  node_off=cat(a.node_off, b.node_off[1:] + a.node_off[-1]),
                  edge_off=cat(a.edge_off, b.edge_off[1:] + a.edge_off[-1]),
                  node_word=cat(a.node_word, b.node_word), label=cat(a.label, b.label),
                  edge_src=cat(a.edge_src, b.edge_src), edge_dst=cat(a.edge_dst, b.edge_dst),
                  n_tables=a.n_tables, table_pre=a.table_pre, table_post=a.table_post,
                  id_rank=None if a.id_rank is None or b.id_rank is None else cat(a.id_rank, b.id_rank),
                  status=list(a.status) + list(b.status), tables=a.tables)


def swapped(corpus: Corpus, rf: int) -> Corpus:
    """[run rf as the good run 0, the corpus' run 0 as the one failed run]."""
    sw = corpus.subset([rf, corpus.run_index(0)])
    sw.iteration = np.array([0, 1], np.uint32)
    sw.status = ["success", "fail"]
    return sw


def induced(corpus: Corpus, g: int, mask: np.ndarray):
    """Edges of graph g induced on mask, in the graph's row order (rows by node, each row by target)."""
    e0, e1 = int(corpus.edge_off[g]), int(corpus.edge_off[g + 1])
    s, d = corpus.edge_src[e0:e1].astype(np.int64), corpus.edge_dst[e0:e1].astype(np.int64)
    o = np.lexsort((d, s))
    s, d = s[o], d[o]
    keep = (mask[s] != 0) & (mask[d] != 0)
    return s[keep], d[keep]


class Want:
    """The oracle's symmetric results of `entries` on `corpus`: masks, surplus rows, induced edges."""

    def __init__(self, corpus: Corpus, entries):
        self.corpus, self.entries = corpus, list(entries)
        per_run = {}
        self.masks, rows, self.edges, self.graphs = [], [], [], []
        for e, it in enumerate(self.entries):
            rf = corpus.run_index(it)
            if rf not in per_run:  # duplicates share one oracle run
                orc = O.analyze(swapped(corpus, rf), [0], [1], diff_mode=DIFF_PER_RUN, threads=4, diff_only=True)
                per_run[rf] = (np.asarray(orc.diff_mask[0], np.uint8), _rows(orc.missing)[:, 1])
            m, rules = per_run[rf]
            g = 2 * rf + 1
            assert len(m) == corpus.graph_size(g)
            self.graphs.append(g)
            self.masks.append(m)
            rows += [(e, int(r)) for r in rules]
            self.edges.append(induced(corpus, g, m))
        self.rows = _rows(rows)

    def nonempty(self, upto=None):
        return [bool(m.any()) for m in self.masks[:upto]]


def check_symmetric(eng, want: Want, pulls=True):
    n = len(want.entries)
    eng.diffprov_symmetric(want.entries)
    masks = eng.sdiff_masks()
    assert len(masks) == n
    bad = [e for e in range(n) if not np.array_equal(masks[e], want.masks[e])]
    assert not bad, f"S masks of entries {bad[:8]} differ ({len(bad)} of {n})"
    assert np.array_equal(_rows(eng.surplus()), want.rows), "surplus rows differ"
    if not pulls:
        return
    eng.pull(3)
    off, cnt, src, dst = eng.pulled_all(n)
    for e in range(n):
        ws, wd = want.edges[e]
        a, k = int(off[e]), int(cnt[e])
        assert k == len(ws) and np.array_equal(src[a:a + k], ws) and np.array_equal(dst[a:a + k], wd), \
            f"pull 3, slot {e} (fetch_pulled_all) differs"
    for e in sorted({0, n // 2, n - 1}):
        s, d = eng.pulled(e)
        assert np.array_equal(s, want.edges[e][0]) and np.array_equal(d, want.edges[e][1]), \
            f"pull 3, slot {e} (fetch_pulled) differs"


def both_tiers(eng, want: Want, pulls=True):
    check_symmetric(eng, want, pulls)
    eng.set_option("graph_lds_max", 0)  # the LDS graph tiers off: every entry takes the global tier
    try:
        check_symmetric(eng, want, pulls)
    finally:
        eng.set_option("graph_lds_max", -1)


# ---- 1. random small corpora ---------------------------------------------------------
def _random_cases(seed):
    from tests.small import random_corpus
    out = []
    for k in range(6):
        corpus, _ = random_corpus(100 * seed + k, n_runs=6, max_nodes=40)
        f = corpus.failed_iters()
        if f and 0 in set(int(x) for x in corpus.iteration):
            # every failed run, then run 0 itself (empty S) and a duplicate entry
            out.append((corpus, f, f + [0, f[0]]))
    return out


@pytest.mark.parametrize("seed", range(8))
def test_random_corpora(eng, seed):
    # isolated Bad goals, empty S, S without longest-path rules, duplicate and iteration-0 entries
    cases = _random_cases(seed)
    assert cases
    ne = []
    for corpus, f, entries in cases:
        want = Want(corpus, entries)
        ne += want.nonempty(len(f))
        assert not want.masks[len(f)].any(), "run 0 against itself has no Bad goal"
        assert np.array_equal(want.masks[-1], want.masks[0])
        eng.load(corpus)
        eng.mark()
        both_tiers(eng, want)
    assert sum(ne) >= 0.9 * len(ne), f"only {sum(ne)} of {len(ne)} failed-run entries have a non-empty oracle S"


# ---- 2. C3 shape, role-exchanged -------------------------------------------------------
@pytest.fixture(scope="module")
def c3_12():
    corpus, _ = synth.generate(12, p_fault=0.55, prepend_run0=True, **synth.CONFIGS["c3"])
    ex, entries = role_exchanged(corpus)
    return ex, Want(ex, entries)


def test_c3_shape(eng, c3_12):
    # u16 rows at the real LDS footprint, several entries per CU
    ex, want = c3_12
    assert len(want.entries) >= 2 and all(want.nonempty())
    eng.load(ex)
    eng.mark()
    both_tiers(eng, want)


def test_c3_shape_more_than_64_entries(eng):
    # one launch over all entries: no 64-entry chunks here
    corpus, _ = synth.generate(80, p_fault=0.15, prepend_run0=True, **synth.CONFIGS["c3"])
    ex, entries = role_exchanged(corpus)
    assert len(entries) > 64
    want = Want(ex, entries)
    assert all(want.nonempty())
    eng.load(ex)
    eng.mark()
    check_symmetric(eng, want)


def test_against_device_diffprov(eng, c3_12):
    # second, device-side reference: the existing nemo_diffprov on the exchanged two-run corpus
    ex, want = c3_12
    rf = ex.run_index(want.entries[0])
    eng.load(swapped(ex, rf))
    eng.mark()
    eng.diffprov([1], DIFF_PER_RUN)
    m, r = eng.diff_masks(1)[0], _rows(eng.missing())
    assert m.any() and np.array_equal(m, want.masks[0])
    assert np.array_equal(r[:, 1], want.rows[want.rows[:, 0] == 0][:, 1])
    eng.load(ex)
    eng.mark()
    eng.diffprov_symmetric(want.entries[:1])
    assert np.array_equal(eng.sdiff_masks()[0], m)
    assert np.array_equal(_rows(eng.surplus())[:, 1], r[:, 1])


# ---- 3. row width and the tier boundary -------------------------------------------------
def test_both_tiers_in_one_launch(eng):
    # ~1.5k-node graphs inside k_diff_lds's caps and ~12k-node graphs past them (and past the pull's
    # single-workgroup tiers) in one corpus: both kernels run in one call
    a, _ = synth.generate(5, target_nodes=1500, p_fault=0.55, prepend_run0=True)
    b, _ = synth.generate(3, target_nodes=12000, p_fault=0.0, seed=11)
    corpus = concat(a, b, 1000)
    ex, entries = role_exchanged(corpus)
    sizes = [ex.graph_size(2 * ex.run_index(it) + 1) for it in entries]
    assert min(sizes) < 4000 and max(sizes) > 8192
    want = Want(ex, entries)
    assert all(want.nonempty())
    eng.load(ex)
    eng.mark()
    check_symmetric(eng, want)


@pytest.mark.parametrize("shape", ["deep_70000", "post_graphs_past_65535"])
def test_u32_rows_global_tier(eng, shape):
    # the global tier on u32 rows: entry offsets beyond 65535 (~33k-node post graphs), then post graphs of
    # >= 65536 nodes.  Seeds and p_fault chosen so that the three runs hold a failed one (the default
    # seed's three runs all succeed); the second case's S has ~5.9k nodes of 66k
    if shape == "deep_70000":
        corpus, _ = synth.generate(3, target_nodes=70000, p_fault=0.9, prepend_run0=True, seed=7, **DEEP)
        vmin = 30000
    else:
        corpus, _ = synth.generate(3, target_nodes=140000, p_fault=0.9, prepend_run0=True, seed=3,
                                   **dict(DEEP, eot=80))
        vmin = 65536
    ex, entries = role_exchanged(corpus)
    want = Want(ex, entries)
    assert len(entries) == 2 and all(ex.graph_size(g) >= vmin for g in want.graphs) and all(want.nonempty())
    eng.load(ex)
    eng.mark()
    check_symmetric(eng, want)


# ---- 4./5. pulls in sequence, independence of the two diffs ------------------------------
def _good_side(corpus, f):
    orc = O.analyze(corpus, [0], f, diff_mode=DIFF_PER_RUN, threads=4, diff_only=True)
    return orc.diff_mask, _rows(orc.missing)


def _check_good_side(eng, corpus, f, want_m, want_r, pull):
    assert np.array_equal(eng.diff_masks(len(f)), want_m), "D masks disturbed"
    assert np.array_equal(_rows(eng.missing()), want_r), "missing rows disturbed"
    if pull:
        g0 = 2 * corpus.run_index(0) + 1
        eng.pull(2)
        for e in range(len(f)):
            s, d = eng.pulled(e)
            ws, wd = induced(corpus, g0, want_m[e])
            assert np.array_equal(s, ws) and np.array_equal(d, wd), f"pull 2, slot {e} differs"


@pytest.mark.parametrize("shape", ["random", "c3"])
def test_independent_of_diffprov(eng, shape, c3_12):
    if shape == "random":
        corpus, f, entries = _random_cases(1)[0]
        want = Want(corpus, entries)
    else:
        corpus, want = c3_12
        f = [int(corpus.iteration[r]) for r in range(corpus.n_runs) if int(corpus.iteration[r]) != 0][:3]
    want_m, want_r = _good_side(corpus, f)
    eng.load(corpus)
    eng.mark()
    # diffprov, then the symmetric call with its pull 3; the good side (and pull 2) still match
    eng.diffprov(f, DIFF_PER_RUN)
    check_symmetric(eng, want)
    _check_good_side(eng, corpus, f, want_m, want_r, pull=True)
    # the reverse order: the symmetric results survive a diffprov and its pull
    eng.diffprov_symmetric(want.entries)
    eng.diffprov(f, DIFF_PER_RUN)
    _check_good_side(eng, corpus, f, want_m, want_r, pull=True)
    masks = eng.sdiff_masks()
    assert all(np.array_equal(a, b) for a, b in zip(masks, want.masks))
    assert np.array_equal(_rows(eng.surplus()), want.rows)
    eng.pull(3)
    s, d = eng.pulled(0)
    assert np.array_equal(s, want.edges[0][0]) and np.array_equal(d, want.edges[0][1])


# ---- 6. errors ----------------------------------------------------------------------------
def test_errors(eng):
    corpus, f, entries = _random_cases(1)[0]
    eng.load(corpus)
    with pytest.raises(E.NemoError) as ei:  # before mark
        eng.diffprov_symmetric(f)
    assert ei.value.code == 5 and "before nemo_mark_holds" in ei.value.msg
    eng.mark()
    with pytest.raises(E.NemoError) as ei:  # pull 3 before any symmetric call on this corpus
        eng.pull(3)
    assert ei.value.code == 5 and "before nemo_diffprov_symmetric" in ei.value.msg
    with pytest.raises(E.NemoError) as ei:
        eng.diffprov_symmetric(f + [4242])
    assert ei.value.code == 7 and "unknown run iteration 4242" in ei.value.msg
    with pytest.raises(E.NemoError) as ei:  # the failed call left no symmetric result
        eng.surplus()
    assert ei.value.code == 5
    # no run of iteration 0: zero entries, no error
    no0 = _with_iterations(corpus, corpus.iteration + np.uint32(1))
    eng.load(no0)
    eng.mark()
    eng.diffprov_symmetric([int(x) for x in no0.iteration])
    assert eng.sdiff_masks() == [] and len(eng.surplus()) == 0
    eng.pull(3)
    assert eng.pulled_all(0)[2].size == 0
    eng.diffprov_symmetric([])
    assert eng.sdiff_masks() == [] and len(eng.surplus()) == 0


def test_node_context_refuses():
    node = E.Engine(devices=[0])
    try:
        corpus, f, _ = _random_cases(1)[0]
        node.load(corpus)
        node.mark()
        with pytest.raises(E.NemoError) as ei:
            node.diffprov_symmetric(f)
        assert ei.value.code == 5 and "single-device contexts only" in ei.value.msg
    finally:
        node.close()


# ---- the host mirror: symmetric=True on a case-study fixture --------------------------------
def test_graphing_symmetric_fixture():
    import os
    from nemo_amd import graphing as GR
    from nemo_amd.corpus import load_molly
    from nemo_amd.dot import read_dot
    d = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cs_ca_2434_bootstrap_synchronization")
    corpus = load_molly(d)
    f = corpus.failed_iters()
    want = Want(corpus, f)
    db = GR.Neo4J()
    db.InitGraphDB("bolt://127.0.0.1:7687", corpus)
    try:
        db.LoadRawProvenance()
        db.SimplifyProv([int(x) for x in corpus.iteration])
        _, post, _, _ = db.PullPrePostProv()
        diffs0, faileds0, missing0 = db.CreateNaiveDiffProv(False, f, post[0])
        assert db.SurplusEvents == []
        diffs, faileds, missing = db.CreateNaiveDiffProv(True, f, post[0])
    finally:
        db.CloseDB()
    assert [x.string() for x in diffs] == [x.string() for x in diffs0] and missing == missing0
    assert len(faileds) == len(f) == len(db.SurplusEvents)
    for e in range(len(f)):
        g, n0 = want.graphs[e], int(corpus.node_off[want.graphs[e]])
        ids = {corpus.node_ids[n0 + int(i)] for i in np.nonzero(want.masks[e])[0]}
        dot = faileds[e]
        assert {k for k, a in dot.nodes.items() if a.get("penwidth") == '"3"'} == ids
        assert sum(1 for x in dot.edges if x.attrs.get("penwidth") == '"3"') == len(want.edges[e][0])
        rules = sorted(corpus.node_ids[n0 + int(r)] for en, r in want.rows if en == e)
        assert sorted(m.Rule.ID for m in db.SurplusEvents[e]) == rules
        assert all(dot.nodes[m.Rule.ID].get("peripheries") == '"2"' for m in db.SurplusEvents[e])
        assert read_dot(dot.string()).attrs.get("bgcolor") == '"transparent"'
