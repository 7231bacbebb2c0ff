"""The consumers of the duplicate-graph classes beyond k_build, k_marksimp and k_chains (DESIGN.md §3 "Duplicate
graphs"): k_proto_lds runs on one run per run class (option proto_dedup) and k_proto_rep copies its rows to the
other runs of the class; the raw and simplified pulls compact one graph per class and the other graphs' slots
share its region (option pull_dedup); k_build's slices reach the duplicates only when something may read them
(option replicate_lazy): the launches under k_replicate are counted, and every reader of arbitrary graphs is run
behind a deferred pass.

Every case runs on graphs of a few to about 200 nodes and compares, bit for bit, with the CPU oracle and with the same
engine under graph_dedup 0.  The run classes are computed here on the host as well (runs whose pre graphs are of one
graph class and whose post graphs are), and compared with the lists the device holds."""
import itertools
import random

import numpy as np
import pytest

from nemo_amd import engine as E
from nemo_amd.corpus import DIFF_PER_RUN, DIFF_REFERENCE, F_DELETED, F_HOLDS, F_KEPT, NODE_RULE, corpus_from_graphs
from oracle import oracle as O
from tests.compare import assert_same
from tests.small import random_prov
from tests.test_gpu_dedup import base_graphs, corpus_of, device_arrays, host_classes, same_results

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    e = E.Engine(0)
    yield e
    e.close()


def run_classes(rep):
    """run -> lowest run whose (pre class, post class) is the same; the (dup, rep) pairs sorted by rep, then dup"""
    seen, out = {}, []
    for r in range(len(rep) // 2):
        out.append(seen.setdefault((int(rep[2 * r]), int(rep[2 * r + 1])), r))
    pairs = sorted((f, r) for r, f in enumerate(out) if f != r)
    return np.array(out), [(d, f) for f, d in pairs]


def device_run_classes(eng, run_rep, pairs):
    """the device's lists against the host's (the lists are in use: graph_dedup and proto_dedup on, duplicates)"""
    reps = [r for r, f in enumerate(run_rep.tolist()) if r == f]
    got = eng.debug_copy("run_list", 0, 4 * len(reps)).view(np.uint32)
    assert got.tolist() == reps
    got = eng.debug_copy("run_pairs", 0, 8 * len(pairs)).view(np.uint32).reshape(-1, 2)
    assert [tuple(x) for x in got.tolist()] == pairs


def one_pass(eng, corpus, reload):
    """main.go's graph calls on the loaded corpus (after a rebuild, unless the corpus was just loaded)"""
    s, f = corpus.success_iters(), corpus.failed_iters()
    if not reload:
        eng.rebuild()
    eng.mark()
    eng.simplify()
    achieved, inter, uni = eng.prototypes(s)
    eng.diffprov(f, DIFF_PER_RUN)
    eng.triggers()
    eng.pull(1)
    off, cnt, src, dst = eng.pulled_all(corpus.n_graphs)
    pulled = [(src[int(a):int(a) + int(n)], dst[int(a):int(a) + int(n)]) for a, n in zip(off, cnt)]
    masks = np.stack([eng.diff_mask(e) for e in range(len(f))]) if len(f) else np.zeros((0, 0))
    pre, post, asy = eng.trigger_rows()
    return E.EngineResult(flags=eng.flags(), chains=eng.chains(), proto_bits=eng.run_tables(0),
                          graph_tables=eng.run_tables(1), achieved=achieved, inter=inter, union=uni, diff_mask=masks,
                          missing=eng.missing(), pre_rows=pre, post_rows=post, async_rules=asy, pulled=pulled)


def passes(eng, corpus, options, n=3):
    """n passes over one load under `options` -> per pass (result, device arrays, gate)"""
    for k, v in options:
        eng.set_option(k, v)
    out = []
    try:
        eng.load(corpus)
        for k in range(n):
            res = one_pass(eng, corpus, k == 0)
            out.append((res, device_arrays(eng, corpus), eng.debug_copy("gate", 0, corpus.n_runs)))
    finally:
        for k, _ in options:
            eng.set_option(k, -1)
    return out


def check_passes(eng, corpus, options=()):
    s, f = corpus.success_iters(), corpus.failed_iters()
    orc = O.analyze(corpus, s, f, diff_mode=DIFF_PER_RUN)
    on = passes(eng, corpus, tuple(options))
    off = passes(eng, corpus, tuple(options) + (("graph_dedup", 0),), n=1)[0]
    assert_same(corpus, off[0], orc, len(f))
    for k, (res, arrays, gate) in enumerate(on):
        assert_same(corpus, res, orc, len(f))
        same_results(res, off[0])
        for name in arrays:
            assert np.array_equal(arrays[name], off[1][name]), (k, name)
        assert np.array_equal(gate, off[2]), k
    return orc


def holding(seed, want):
    """a pre graph whose simplified form has a holding "pre" goal (want) or has none, by the oracle"""
    rng = random.Random(seed)
    post = random_prov(rng, "post", 40, p_next=0.7)
    while True:
        pre = random_prov(rng, "pre", 40, p_next=0.7)
        c = corpus_from_graphs([(0, "success", pre, post)])
        orc = O.analyze(c, c.success_iters(), c.failed_iters(), diff_mode=DIFF_PER_RUN)
        fl = orc.flags[:int(c.node_off[1])]
        goal = (c.node_word[:int(c.node_off[1])] & NODE_RULE) == 0
        kept = bool((((fl & (F_HOLDS | F_KEPT | F_DELETED)) == (F_HOLDS | F_KEPT)) & goal).any())
        if (want and kept) or (not want and not (fl & F_HOLDS).any()):
            return pre


def test_proto_key(eng):
    # runs 0 and 1: one post graph, a pre graph with a holding pre goal against one without: apart.  Runs 2 and 3
    # repeat run 0 and run 1, run 4 run 0 again: the classes {0, 2, 4} and {1, 3}
    rng = random.Random(21)
    post = None
    pre_h, pre_n = holding(22, True), holding(23, False)
    for _ in range(200):
        post = random_prov(rng, "post", 60, p_next=0.7)
        c = corpus_from_graphs([(0, "success", pre_h, post), (1, "success", pre_n, post)])
        orc = O.analyze(c, c.success_iters(), c.failed_iters(), diff_mode=DIFF_PER_RUN)
        if orc.proto_bits[0].any() and not orc.proto_bits[1].any():
            break
    else:
        raise AssertionError("no post graph with a prototype under the holding pre graph")
    runs = [(pre_h, post), (pre_n, post), (pre_h, post), (pre_n, post), (pre_h, post)]
    corpus = corpus_from_graphs([(r, "success" if r != 3 else "failure", a, b) for r, (a, b) in enumerate(runs)])
    rep = host_classes(corpus)
    assert rep.tolist() == [0, 1, 2, 1, 0, 1, 2, 1, 0, 1]
    run_rep, pairs = run_classes(rep)
    assert run_rep.tolist() == [0, 1, 0, 1, 0] and pairs == [(2, 0), (4, 0), (3, 1)]
    orc = check_passes(eng, corpus)
    assert orc.proto_bits[0].any() and not orc.proto_bits[1].any()
    eng.load(corpus)
    res = one_pass(eng, corpus, True)
    device_run_classes(eng, run_rep, pairs)
    gate = eng.debug_copy("gate", 0, corpus.n_runs)
    assert gate.tolist() == [1, 0, 1, 0, 1]
    assert np.array_equal(res.proto_bits, orc.proto_bits)


def test_run_class_representative_not_run0(eng):
    # graph classes interleaved; a run class led by run 1; pre and post classes shared across different run classes;
    # the last run a duplicate
    bases = base_graphs(31, 3, max_nodes=120)
    mixed = [(bases[0][0], bases[1][1]), (bases[1][0], bases[0][1])]  # a pre class with another base's post class
    picks = [bases[0], bases[1], mixed[0], bases[1], mixed[1], bases[2], mixed[0], bases[0], bases[1]]
    corpus = corpus_from_graphs([(r, "success" if r == 0 or r % 3 else "failure", a, b) for r, (a, b) in enumerate(picks)])
    run_rep, pairs = run_classes(host_classes(corpus))
    assert run_rep.tolist() == [0, 1, 2, 1, 4, 5, 2, 0, 1]
    check_passes(eng, corpus)
    eng.load(corpus)
    device_run_classes(eng, run_rep, pairs)


@pytest.mark.parametrize("graph_dedup, proto_dedup, pull_dedup, lazy", list(itertools.product((1, 0), (1, 0), (1, 0), (1, 0))))
def test_each_option_alone_and_together(eng, graph_dedup, proto_dedup, pull_dedup, lazy):
    bases = base_graphs(32, 4, max_nodes=150)
    corpus = corpus_of([0, 1, 2, 1, 3, 2, 2, 0, 1, 3, 1, 2], bases)
    s, f = corpus.success_iters(), corpus.failed_iters()
    orc = O.analyze(corpus, s, f, diff_mode=DIFF_PER_RUN)
    for res, _, _ in passes(eng, corpus, (("graph_dedup", graph_dedup), ("proto_dedup", proto_dedup),
                                            ("pull_dedup", pull_dedup), ("replicate_lazy", lazy))):
        assert_same(corpus, res, orc, len(f))
    if graph_dedup and proto_dedup:  # (the options are back at their defaults: the runs' list is in use)
        device_run_classes(eng, *run_classes(host_classes(corpus)))


@pytest.mark.parametrize("options", [(("build_lds_max", 0),), (("graph_lds_max", 0),), (("chains_lds_max", 4),),
                                     (("build_lds_max", 0), ("graph_lds_max", 0), ("chains_lds_max", 4))])
def test_duplicate_runs_outside_each_lds_tier(eng, options):
    # outside k_build's tier (no e2 / posoff) and outside the LDS tier k_proto_lds returns at once for every run of
    # a class, nothing is copied and the global tier lists the duplicates as it lists their representative; three
    # passes, the later ones with the tier cache captured
    bases = base_graphs(33, 3, max_nodes=150)
    check_passes(eng, corpus_of([0, 1, 0, 2, 1, 1, 0, 2], bases), options)


def pull_tables(eng, corpus, which):
    """one pull through every fetch: (off, cnt, per-slot (src, dst) pairs in order, n_used)"""
    G = corpus.n_graphs
    eng.pull(which)
    off, cnt, src, dst = eng.pulled_all(G)
    edges = []
    for g in range(G):
        a, n = int(off[g]), int(cnt[g])
        assert a + n <= len(src)
        s1, d1 = eng.pulled(g)
        assert int(eng.L.nemo_pulled_count(eng.h, g)) == n == len(s1)
        assert np.array_equal(s1, src[a:a + n]) and np.array_equal(d1, dst[a:a + n])
        edges.append(list(zip(s1.tolist(), d1.tolist())))
    return off, cnt, edges, len(src)


def check_pull_sharing(eng, corpus, options=(), tier_v=8191):
    """which 0 and 1 under the classes against graph_dedup 0: each slot's edges in the same order, duplicates on
    their representative's region, the regions' extent the representatives' alone.  Not shared: the graphs past the
    pull's LDS tier, which keep regions of their own"""
    rep = host_classes(corpus)
    G = corpus.n_graphs
    for g in range(G):  # kept apart by the load (8192 nodes or more), or past the pull's LDS tier (tier_v nodes)
        if corpus.graph_size(g) > tier_v:
            rep[g] = g
    got = {}
    for dedup in (1, 0):
        for k, v in tuple(options) + (("graph_dedup", dedup),):
            eng.set_option(k, v)
        try:
            eng.load(corpus)
            eng.mark()
            eng.simplify()
            got[dedup] = [pull_tables(eng, corpus, which) for which in (0, 1, 0)]  # (a raw pull after a simplified one)
        finally:
            for k, _ in tuple(options) + (("graph_dedup", dedup),):
                eng.set_option(k, -1)
    for (off, cnt, edges, used), (off0, cnt0, edges0, used0) in zip(got[1], got[0]):
        assert edges == edges0  # order, not multiset
        assert np.array_equal(cnt, cnt0)
        assert np.array_equal(off, off[rep])
        assert len({int(off[g]) for g in range(G) if cnt[g]}) == len({int(g) for g in rep[cnt > 0]})
        reps = np.nonzero(rep == np.arange(G))[0]
        assert used == int(cnt[reps].sum()) and used0 == int(cnt0.sum())
        spans = sorted((int(off[g]), int(cnt[g])) for g in reps if cnt[g])  # the representatives' regions are disjoint
        assert all(a + n <= b for (a, n), (b, _) in zip(spans, spans[1:]))
    return rep


def test_pull_sharing(eng):
    # classes interleaved, the last graph a duplicate
    bases = base_graphs(41, 5, max_nodes=120)
    corpus = corpus_of([0, 1, 2, 1, 3, 2, 2, 4, 1, 3, 1, 2], bases)
    rep = check_pull_sharing(eng, corpus)
    assert rep[-1] != corpus.n_graphs - 1
    # every graph past the pull's LDS tier: k_pull's list holds every graph, as without the classes
    check_pull_sharing(eng, corpus, (("graph_lds_max", 0),), tier_v=0)
    # some classes inside the tier and some past it
    dup = np.nonzero(rep != np.arange(corpus.n_graphs))[0]
    sizes = sorted(corpus.graph_size(int(g)) for g in dup)
    cut = sizes[len(sizes) // 2 - 1]
    assert sizes[0] <= cut < sizes[-1]
    part = check_pull_sharing(eng, corpus, (("graph_lds_max", cut),), tier_v=cut)
    assert 0 < int((part != np.arange(corpus.n_graphs)).sum()) < len(dup)


def test_pull_sharing_beside_a_big_graph(eng):
    # a graph of 8192 nodes or more is kept apart and pulled over chunks, a chunk-table row per slot
    from tests.test_gpu_deep import wide_prov
    bases = base_graphs(42, 2, max_nodes=60)
    big = (bases[0][0], wide_prov("post", 2100, 3))
    runs = [bases[0], big, bases[1], bases[0], big, bases[1], bases[0]]
    corpus = corpus_from_graphs([(r, "success" if r % 3 else "failure" if r else "success", a, b)
                                 for r, (a, b) in enumerate(runs)])
    assert corpus.graph_size(3) >= 8192
    rep = check_pull_sharing(eng, corpus)
    assert rep[3] == 3 and rep[9] == 9 and rep[8] == 0 and rep[13] == 1
    check_passes(eng, corpus)


def test_pull_dedup_toggled_between_pulls(eng):
    bases = base_graphs(43, 3, max_nodes=100)
    corpus = corpus_of([0, 1, 0, 2, 1, 1, 0, 2], bases)
    eng.load(corpus)
    eng.mark()
    eng.simplify()
    try:
        want = pull_tables(eng, corpus, 1)
        eng.set_option("pull_dedup", 0)
        off, cnt, edges, used = pull_tables(eng, corpus, 1)
        assert edges == want[2] and used == int(cnt.sum()) and used > want[3]
        eng.set_option("pull_dedup", 1)
        off, cnt, edges, used = pull_tables(eng, corpus, 1)
        assert edges == want[2] and used == want[3]
    finally:
        eng.set_option("pull_dedup", -1)


# ---- the k_build replicate on demand (option replicate_lazy) ------------------------------------------------------
def bench_step(eng, corpus, mode, first):
    """the benchmark step's call sequence on the loaded corpus -> what it hands to the host"""
    s, f = corpus.success_iters(), corpus.failed_iters()
    if not first:
        eng.rebuild()
    eng.mark()
    eng.diffprov(f, mode)
    eng.simplify()
    eng.protos_partial(s, 0)
    eng.stage_simplified()
    eng.protos_stage(0)
    eng.triggers()
    eng.pull(1)
    eng.pull(2)
    protos = eng.protos_finalize(0)
    out = {"protos": protos, "tables": eng.run_tables(1).copy(), "bits": eng.run_tables(0).copy(),
           "trig": eng.trigger_rows(), "masks": np.array(eng.diff_masks_view()).copy(), "missing": eng.missing().copy()}
    state, chain_off, chain_ht = eng.simplified_view()
    out["state"] = (np.array(state).copy(), np.array(chain_off).copy(), np.array(chain_ht).copy())
    n = len(f)
    off, cnt, src, dst = eng.pulled_all(n)  # pull 2's regions
    out["pull2"] = [(src[int(a):int(a) + int(k)].copy(), dst[int(a):int(a) + int(k)].copy()) for a, k in zip(off, cnt)]
    return out


def same_step(got, orc, want):
    """a bench step's results against the oracle's and against graph_dedup 0's step"""
    assert np.array_equal(got["tables"], orc.graph_tables) and np.array_equal(got["bits"], orc.proto_bits)
    assert (got["protos"]["achieved"], got["protos"]["inter"], got["protos"]["union"]) == \
        (orc.achieved, [int(x) for x in orc.inter], [int(x) for x in orc.union])
    if orc.run0 >= 0:
        assert np.array_equal(got["masks"].reshape(orc.diff_mask.shape), orc.diff_mask)
        assert np.array_equal(got["missing"], orc.missing)
        assert np.array_equal(got["trig"][0], orc.pre_rows) and np.array_equal(got["trig"][1], orc.post_rows)
        assert np.array_equal(np.sort(got["trig"][2]), np.sort(orc.async_rules))
    for a, b in zip(got["state"], want["state"]):
        assert np.array_equal(a, b)
    assert len(got["pull2"]) == len(want["pull2"])
    for (s1, d1), (s2, d2) in zip(got["pull2"], want["pull2"]):
        assert np.array_equal(s1, s2) and np.array_equal(d1, d2)


def replicate_launches(eng):
    return eng.timings().get("k_replicate", {"launches": 0})["launches"]


def plain_step(eng, corpus, mode):
    """the step and the device arrays under graph_dedup 0"""
    eng.set_option("graph_dedup", 0)
    try:
        eng.load(corpus)
        return bench_step(eng, corpus, mode, True), device_arrays(eng, corpus)
    finally:
        eng.set_option("graph_dedup", 1)


def deferred_passes(eng, corpus, mode, orc, want):
    """load, then three bench steps, the third with k_build's slices left to ensure_whole: exactly one launch under
    k_replicate (the one behind k_marksimp).  Leaves the corpus loaded with the slices stale and timing on"""
    eng.load(corpus)
    for k in range(3):
        if k == 2:
            eng.set_timing(True)
            eng.reset_timings()
        same_step(bench_step(eng, corpus, mode, k == 0), orc, want)
    assert replicate_launches(eng) == 1


def lazy_corpus(seed=51):
    # every graph inside every LDS tier; the failed runs 3, 6 and 9 carry the graphs of runs 1, 2 and 4
    bases = base_graphs(seed, 4, max_nodes=150)
    corpus = corpus_of([0, 1, 2, 1, 3, 2, 2, 0, 1, 3, 1, 2], bases)
    rep = host_classes(corpus)
    for r in (3, 6, 9):
        assert rep[2 * r + 1] != 2 * r + 1 and corpus.status[r] != "success", r
    return corpus


@pytest.mark.parametrize("mode", [DIFF_REFERENCE, DIFF_PER_RUN])
def test_deferral_happens_and_ends(eng, mode):
    corpus = lazy_corpus()
    orc = O.analyze(corpus, corpus.success_iters(), corpus.failed_iters(), diff_mode=mode)
    want, arrays = plain_step(eng, corpus, mode)
    try:
        deferred_passes(eng, corpus, mode, orc, want)
        fp = eng.debug_copy("fp", 0, len(arrays["fp"]))
        assert replicate_launches(eng) == 2 and np.array_equal(fp, arrays["fp"])
        got = device_arrays(eng, corpus)
        assert replicate_launches(eng) == 2  # nothing is stale any more
        for name in arrays:
            assert np.array_equal(got[name], arrays[name]), name
        # with the option off the slices follow k_build in every pass
        eng.set_option("replicate_lazy", 0)
        eng.reset_timings()
        same_step(bench_step(eng, corpus, mode, False), orc, want)  # (the option reset the tier cache: eager anyway)
        same_step(bench_step(eng, corpus, mode, False), orc, want)
        assert replicate_launches(eng) == 4
    finally:
        eng.set_timing(False)
        eng.set_option("replicate_lazy", -1)


def test_readers_of_any_graph_after_a_deferred_pass(eng):
    from tests import test_gpu_dclass as TC, test_gpu_nearest as TN, test_gpu_pairs as TP, test_gpu_sdiff as TS
    corpus = lazy_corpus()
    f = corpus.failed_iters()
    orc = O.analyze(corpus, corpus.success_iters(), f, diff_mode=DIFF_PER_RUN)
    want, arrays = plain_step(eng, corpus, DIFF_PER_RUN)
    its = [int(x) for x in corpus.iteration]
    readers = {
        "symmetric": lambda: TS.check_symmetric(eng, TS.Want(corpus, f)),
        "pairs": lambda: TP.check_pairs(eng, TP.Want(corpus, [(b, o) for b in f for o in (0, f[0], its[-1])])),
        "nearest": lambda: TN.check(eng, TN.label_sets(corpus), f, its),
        "classes": lambda: (lambda w: (np.array_equal(eng.diff_classes()[0], w[0]) or pytest.fail("class_of"),
                                       np.array_equal(eng.diff_support(), w[2]) or pytest.fail("support")))(
            TC.expected(TC.oracle_masks(corpus, f, DIFF_PER_RUN))),
        "flags": lambda: np.array_equal(eng.flags(), orc.flags) or pytest.fail("flags"),
        "missing_from": lambda: eng.missing_from(f[0], list(orc.union)),
    }
    try:
        for name, read in readers.items():
            deferred_passes(eng, corpus, DIFF_PER_RUN, orc, want)
            read()
            if name != "missing_from":
                assert replicate_launches(eng) == 2, name  # the reader brought the slices first
            got = device_arrays(eng, corpus)
            for k in arrays:
                assert np.array_equal(got[k], arrays[k]), (name, k)
            eng.set_timing(False)
    finally:
        eng.set_timing(False)


@pytest.mark.parametrize("mode", [DIFF_REFERENCE, DIFF_PER_RUN])
def test_run0_not_a_representative(eng, mode):
    # the first run (iteration 5) carries run 0's graphs, so run 0, second, is a duplicate: what reads run 0's build
    # outputs (diffprov, triggers, pull 2) must bring the slices first
    bases = base_graphs(52, 3, max_nodes=150)
    order = [(5, 0), (0, 0), (1, 1), (2, 2), (3, 1), (4, 0), (6, 2)]
    corpus = corpus_from_graphs([(it, "success" if it in (0, 1, 5) else "failure", bases[b][0], bases[b][1])
                                 for it, b in order])
    rep = host_classes(corpus)
    assert rep[2] == 0 and rep[3] == 1
    orc = O.analyze(corpus, corpus.success_iters(), corpus.failed_iters(), diff_mode=mode)
    want, arrays = plain_step(eng, corpus, mode)
    eng.load(corpus)
    try:
        for k in range(4):
            if k == 2:
                eng.set_timing(True)
            eng.reset_timings()
            same_step(bench_step(eng, corpus, mode, k == 0), orc, want)
        # deferred behind k_build, brought by the step's first reader of run 0: two launches, as without the option
        assert replicate_launches(eng) == 2
        got = device_arrays(eng, corpus)
        for name in arrays:
            assert np.array_equal(got[name], arrays[name]), name
    finally:
        eng.set_timing(False)


@pytest.mark.parametrize("option", ["graph_dedup", "pull_dedup", "proto_dedup"])
def test_option_toggled_while_stale(eng, option):
    corpus = lazy_corpus()
    s, f = corpus.success_iters(), corpus.failed_iters()
    orc = O.analyze(corpus, s, f, diff_mode=DIFF_PER_RUN)
    want, arrays = plain_step(eng, corpus, DIFF_PER_RUN)
    try:
        deferred_passes(eng, corpus, DIFF_PER_RUN, orc, want)
        eng.set_option(option, 0)
        assert replicate_launches(eng) == 2  # the option change brought the slices
        eng.mark()  # no rebuild: the kernels below read what the last k_build and its replicates left
        eng.simplify()
        for which in (1, 0):
            off, cnt, edges, used = pull_tables(eng, corpus, which)
            if which == 1:
                pulled = [(np.array([a for a, _ in e], np.uint32), np.array([b for _, b in e], np.uint32)) for e in edges]
            if option != "proto_dedup":
                assert used == int(cnt.sum())
        achieved, inter, uni = eng.prototypes(s)
        res = E.EngineResult(flags=eng.flags(), chains=eng.chains(), proto_bits=eng.run_tables(0),
                             graph_tables=eng.run_tables(1), achieved=achieved, inter=inter, union=uni,
                             diff_mask=orc.diff_mask, missing=orc.missing, pre_rows=orc.pre_rows, post_rows=orc.post_rows,
                             async_rules=orc.async_rules, pulled=pulled)
        assert_same(corpus, res, orc, len(f))
        got = device_arrays(eng, corpus)
        for name in arrays:
            assert np.array_equal(got[name], arrays[name]), name
    finally:
        eng.set_timing(False)
        eng.set_option(option, -1)


def test_node_context():
    from tools import synth
    corpus, _ = synth.generate(24, target_nodes=400, p_fault=0.3)
    run_rep, pairs = run_classes(host_classes(corpus))
    assert len(pairs) > 2
    e = E.Engine(devices=[0, 0])
    try:
        s, f = corpus.success_iters(), corpus.failed_iters()
        orc = O.analyze(corpus, s, f, diff_mode=DIFF_PER_RUN)
        res = {}
        for opts in ((1, 1), (1, 0), (0, 1)):
            e.set_option("graph_dedup", opts[0])
            e.set_option("proto_dedup", opts[1])
            e.set_option("pull_dedup", opts[1])
            e.set_option("replicate_lazy", opts[1])
            res[opts] = E.analyze(corpus, s, f, diff_mode=DIFF_PER_RUN, engine=e, pulls=True)
            assert_same(corpus, res[opts], orc, len(f))
            if opts == (1, 1):  # the shards' shared regions behind the node's merged tables
                assert sum(len(x) for x, _ in res[opts].pulled) > e.pulled_all(corpus.n_graphs)[2].size
        same_results(res[(1, 1)], res[(0, 1)])
        same_results(res[(1, 0)], res[(0, 1)])
        for (s1, d1), (s2, d2) in zip(res[(1, 1)].pulled, res[(0, 1)].pulled):
            assert np.array_equal(s1, s2) and np.array_equal(d1, d2)
    finally:
        e.close()
