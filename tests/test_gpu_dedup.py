"""Duplicate provenance graphs (option graph_dedup; DESIGN.md §3 "Duplicate graphs"): k_build, k_marksimp and the
first chain tier run on one graph per distinct content and k_replicate fills the other graphs' slices.

Every case runs the whole analysis with the option on and off on graphs of a few to a few hundred nodes and
compares both, bit for bit, with the CPU oracle and with each other: flags, chains, table sets, prototypes, D masks,
missing rows, trigger rows and pulled edges of every graph, and the CSR rows, Kahn levels and per-graph scalars
fetched from the device.  The corpus' classes are computed here on the host as well, so that a case knows whether
a replicate launch is due."""
import copy
import random

import numpy as np
import pytest

from nemo_amd import engine as E
from nemo_amd.corpus import DIFF_PER_RUN, DIFF_REFERENCE, corpus_from_graphs
from oracle import oracle as O
from tests.compare import assert_same
from tests.small import random_prov

pytestmark = pytest.mark.gpu

RESULT_FIELDS = ("flags", "chains", "proto_bits", "graph_tables", "diff_mask", "missing", "pre_rows", "post_rows")


@pytest.fixture(scope="module")
def eng():
    e = E.Engine(0)
    yield e
    e.close()


def host_classes(corpus):
    """graph -> lowest graph of identical content (sizes, parity, words, labels, ranks, edges in stored order)"""
    seen, rep = {}, []
    for g in range(corpus.n_graphs):
        n0, n1 = int(corpus.node_off[g]), int(corpus.node_off[g + 1])
        e0, e1 = int(corpus.edge_off[g]), int(corpus.edge_off[g + 1])
        key = (g & 1, corpus.node_word[n0:n1].tobytes(), corpus.label[n0:n1].tobytes(),
               b"" if corpus.id_rank is None else corpus.id_rank[n0:n1].tobytes(),
               corpus.edge_src[e0:e1].tobytes(), corpus.edge_dst[e0:e1].tobytes())
        rep.append(seen.setdefault(key, g))
    return np.array(rep)


def device_arrays(eng, corpus):
    V, Eg, G = int(corpus.node_off[-1]), int(corpus.edge_off[-1]), corpus.n_graphs
    sizes = {"fp": 4 * (V + G), "rp": 4 * (V + G), "fc": 4 * Eg, "rc": 4 * Eg, "nlv": 4 * V, "nlev": 4 * G, "flags": V,
             "err": 4 * G, "redo": G}
    return {k: eng.debug_copy(k, 0, n) for k, n in sizes.items() if n}


def run(eng, corpus, dedup, mode=DIFF_PER_RUN, options=()):
    """one analysis under graph_dedup = dedup -> (result, device arrays, k_replicate launches)"""
    eng.set_option("graph_dedup", dedup)
    for k, v in options:
        eng.set_option(k, v)
    try:
        eng.set_timing(True)
        eng.reset_timings()
        s, f = corpus.success_iters(), corpus.failed_iters()
        res = E.analyze(corpus, s, f, diff_mode=mode, engine=eng, pulls=True)
        arrays = device_arrays(eng, corpus)
        launches = eng.timings().get("k_replicate", {"launches": 0})["launches"]
    finally:
        eng.set_timing(False)
        for k, _ in options:
            eng.set_option(k, -1)
        eng.set_option("graph_dedup", 1)
    return res, arrays, launches


def same_results(a, b):
    for k in RESULT_FIELDS:
        x, y = getattr(a, k), getattr(b, k)
        assert (x is None and y is None) or np.array_equal(x, y), k
    assert (a.achieved, a.inter, a.union) == (b.achieved, b.inter, b.union)
    assert np.array_equal(np.sort(a.async_rules), np.sort(b.async_rules))
    assert len(a.pulled) == len(b.pulled)
    for (s1, d1), (s2, d2) in zip(a.pulled, b.pulled):
        assert sorted(zip(s1.tolist(), d1.tolist())) == sorted(zip(s2.tolist(), d2.tolist()))


def check(eng, corpus, mode=DIFF_PER_RUN, options=(), expect_dups=None):
    s, f = corpus.success_iters(), corpus.failed_iters()
    orc = O.analyze(corpus, s, f, diff_mode=mode)
    rep = host_classes(corpus)
    dups = int((rep != np.arange(len(rep))).sum())
    if expect_dups is not None:
        assert (dups > 0) == expect_dups, dups
    on, arr_on, n_on = run(eng, corpus, 1, mode, options)
    assert_same(corpus, on, orc, len(f))
    off, arr_off, n_off = run(eng, corpus, 0, mode, options)
    assert_same(corpus, off, orc, len(f))
    same_results(on, off)
    for k in arr_on:
        assert np.array_equal(arr_on[k], arr_off[k]), k
    assert n_off == 0
    assert (n_on > 0) == (dups > 0), (n_on, dups)  # no duplicates: nothing new is launched
    return rep


def base_graphs(seed, n, max_nodes=40):
    rng = random.Random(seed)
    return [(random_prov(rng, "pre", max_nodes, p_next=0.7), random_prov(rng, "post", max_nodes, p_next=0.7))
            for _ in range(n)]


def corpus_of(picks, bases):
    """run r carries the graphs of bases[picks[r]]"""
    return corpus_from_graphs([(r, "success" if r == 0 or r % 3 else "failure", bases[p][0], bases[p][1])
                               for r, p in enumerate(picks)])


def test_every_run_a_copy_of_run0(eng):
    bases = base_graphs(1, 1, max_nodes=200)
    rep = check(eng, corpus_of([0] * 12, bases), expect_dups=True)
    assert set(rep.tolist()) == {0, 1}


def test_no_two_graphs_equal(eng):
    check(eng, corpus_of(list(range(9)), base_graphs(2, 9)), expect_dups=False)


@pytest.mark.parametrize("mode", [DIFF_REFERENCE, DIFF_PER_RUN])
def test_duplicates_before_and_after_their_twin(eng, mode):
    # run 0 unique; classes whose members are spread around other classes' members; the last graph a duplicate
    bases = base_graphs(3, 5, max_nodes=120)
    check(eng, corpus_of([0, 1, 2, 1, 3, 2, 2, 4, 1, 3, 1, 2], bases), mode=mode, expect_dups=True)


def _variants(base):
    """near-duplicates of a (pre, post) pair: each differs from it in exactly one place"""
    pre, post = base
    out = []

    def variant(fn):
        p = copy.deepcopy(post)
        fn(p)
        out.append((pre, p))

    variant(lambda p: p["goals"][0].update(label=p["goals"][0]["label"] + "x"))  # one label
    variant(lambda p: p["goals"][-1].update(table="t9", label="t9(a, 0)"))  # one node word: table id
    variant(lambda p: p["rules"][0].update(type="async" if p["rules"][0]["type"] != "async" else "single"))  # type
    variant(lambda p: p["edges"].__setitem__(slice(0, 2), p["edges"][1::-1]))  # two edges swapped in storage order
    variant(lambda p: p["edges"].pop())  # V equal, E smaller by one

    def endpoint(p):  # one edge endpoint: the last edge's source moved to another node of the same kind before it
        names = [n["id"] for n in sorted(p["goals"] + p["rules"], key=lambda n: int(n["id"][4:]))]
        e = p["edges"][-1]
        kind, at = e["from"][:4], names.index(e["from"])
        have = {(x["from"], x["to"]) for x in p["edges"]}
        for n in names[:at]:
            if n[:4] == kind and (n, e["to"]) not in have:
                e["from"] = n
                return
        raise AssertionError("no free endpoint")

    variant(endpoint)
    return out


def test_near_duplicates_stay_apart(eng):
    rng = random.Random(11)
    base = None
    while base is None or len(base[1]["edges"]) < 6 or not base[1]["rules"] or len(base[1]["goals"]) < 2:
        base = (random_prov(rng, "pre", 30, p_next=0.7), random_prov(rng, "post", 30, p_next=0.7))
    bases = [base] + _variants(base)
    picks = [0] + [k for k in range(1, len(bases))] + [0] + [k for k in range(1, len(bases))]
    corpus = corpus_of(picks, bases)
    rep = check(eng, corpus, expect_dups=True)
    post = rep[1::2]
    assert len(set(post.tolist())) == len(bases), post  # every variant a class of its own, each met twice


def test_pre_graph_equal_to_a_post_graph(eng):
    # run 1's post graph has the content of run 0's pre graph (and the reverse): k_build writes e2 / posoff for
    # post graphs only, so the two never share a class
    pre, post = base_graphs(5, 1, max_nodes=60)[0]
    corpus = corpus_from_graphs([(0, "success", pre, post), (1, "success", post, pre), (2, "failure", pre, post)])
    rep = check(eng, corpus, expect_dups=True)
    assert rep.tolist() == [0, 1, 2, 3, 0, 1]


@pytest.mark.parametrize("kind", ["cycle", "nonbipartite", "duplicate_edge", "endpoint"])
def test_failed_load_check_in_every_copy(eng, kind):
    pre, post = base_graphs(6, 1, max_nodes=30)[0]
    corpus = corpus_of([0] * 6, [(pre, post)])
    e0, e1 = int(corpus.edge_off[1]), int(corpus.edge_off[2])  # run 0's post graph, copied into every run's below
    assert e1 - e0 >= 2
    words = corpus.node_word[int(corpus.node_off[1]):int(corpus.node_off[2])]
    src, dst = corpus.edge_src.copy(), corpus.edge_dst.copy()
    for r in range(corpus.n_runs):
        a = int(corpus.edge_off[2 * r + 1])
        if kind == "cycle":
            src[a + 1], dst[a + 1] = dst[a], src[a]
        elif kind == "nonbipartite":
            same = [v for v in range(len(words)) if (words[v] >> 31) == (words[int(src[a])] >> 31) and v != src[a]]
            dst[a] = same[0]
        elif kind == "duplicate_edge":
            src[a + 1], dst[a + 1] = src[a], dst[a]
        else:
            dst[a] = len(words) + 3
    corpus.edge_src, corpus.edge_dst = src, dst
    got = []
    for dedup in (1, 0):
        eng.set_option("graph_dedup", dedup)
        try:
            with pytest.raises(E.NemoError) as ei:
                eng.load(corpus)
            err = eng.debug_copy("err", 0, 4 * corpus.n_graphs).view(np.uint32)
            got.append((ei.value.code, str(ei.value), err.tolist()))
        finally:
            eng.set_option("graph_dedup", 1)
    assert got[0] == got[1]
    err = np.array(got[0][2])
    assert (err[1::2] != 0).all() and len(set(err[1::2].tolist())) == 1 and (err[0::2] == 0).all()


@pytest.mark.parametrize("options", [(("build_lds_max", 0),), (("graph_lds_max", 0),), (("chains_lds_max", 4),),
                                     (("build_lds_max", 0), ("graph_lds_max", 0), ("chains_lds_max", 4)),
                                     (("build_marksimp", 1),)])
def test_duplicates_outside_each_lds_tier(eng, options):
    bases = base_graphs(7, 3, max_nodes=150)
    check(eng, corpus_of([0, 1, 0, 2, 1, 1, 0, 2], bases), options=options, expect_dups=True)


def test_duplicates_handed_back_by_the_first_chain_tier(eng):
    # @next chains of 70 rules (141 Kahn levels): the first chain tier hands the graph back, and every copy of it
    # is then listed for the second tier
    def chain(cond, n):
        goals = [{"id": f"goal{2 * i}", "label": f"{cond}(a, {i})", "table": cond, "time": "1"} for i in range(n + 1)]
        rules = [{"id": f"rule{2 * i + 1}", "label": cond, "table": cond, "type": "next"} for i in range(n)]
        edges = []
        for i in range(n):
            edges += [{"from": f"goal{2 * i}", "to": f"rule{2 * i + 1}"}, {"from": f"rule{2 * i + 1}", "to": f"goal{2 * i + 2}"}]
        return {"goals": goals, "rules": rules, "edges": edges}

    bases = [(chain("pre", 70), chain("post", 70)), (chain("pre", 8), chain("post", 69))]
    check(eng, corpus_of([0, 1, 0, 0, 1, 0], bases), expect_dups=True)


@pytest.mark.parametrize("bits", [0, 1, 128])
def test_dedup_hash_bits(eng, bits):
    bases = base_graphs(8, 6, max_nodes=50)
    eng.set_option("dedup_hash_bits", bits)
    try:
        check(eng, corpus_of([0, 1, 2, 3, 1, 4, 2, 5, 0, 3, 3], bases), expect_dups=True)
    finally:
        eng.set_option("dedup_hash_bits", -1)


def test_reload_and_rebuild(eng):
    a = corpus_of([0, 1, 0, 1, 1, 0], base_graphs(9, 2, max_nodes=80))
    b = corpus_of(list(range(5)), base_graphs(10, 5, max_nodes=80))
    assert (host_classes(b) == np.arange(b.n_graphs)).all()
    want = {}
    for name, c in (("a", a), ("b", b)):
        want[name] = O.analyze(c, c.success_iters(), c.failed_iters(), diff_mode=DIFF_PER_RUN)

    def step(c, first):
        if first:
            eng.load(c)
        else:
            eng.rebuild()
        eng.mark()
        eng.simplify()
        return eng.flags(), eng.chains()

    eng.set_timing(True)
    try:
        for name, c, steps in (("a", a, 3), ("b", b, 2), ("a", a, 2)):
            eng.reset_timings()
            for k in range(steps):
                flags, chains = step(c, k == 0)
                assert np.array_equal(flags, want[name].flags) and np.array_equal(chains, want[name].chains), (name, k)
            n = eng.timings().get("k_replicate", {"launches": 0})["launches"]
            assert n == (0 if name == "b" else 2 * steps), (name, n)  # behind k_build and k_marksimp of every step
    finally:
        eng.set_timing(False)


def test_node_context():
    from tools import synth
    corpus, _ = synth.generate(24, target_nodes=400, p_fault=0.3)
    rep = host_classes(corpus)
    assert (rep != np.arange(len(rep))).sum() > 4
    e = E.Engine(devices=[0, 0])
    try:
        s, f = corpus.success_iters(), corpus.failed_iters()
        orc = O.analyze(corpus, s, f, diff_mode=DIFF_PER_RUN)
        res = {}
        for dedup in (1, 0):
            e.set_option("graph_dedup", dedup)
            res[dedup] = E.analyze(corpus, s, f, diff_mode=DIFF_PER_RUN, engine=e, pulls=True)
            assert_same(corpus, res[dedup], orc, len(f))
        same_results(res[1], res[0])
    finally:
        e.close()


def test_every_slice_alignment(eng):
    # duplicates whose slices start at every residue mod 16 of the u8 arrays (flags: n0), every residue mod 4 of the
    # u32 arrays (n0 + g, e0) and of the chain records (5 n0), the last graph of the corpus among them
    bases = base_graphs(12, 4, max_nodes=23)
    rng = random.Random(13)
    picks = [0, 1, 2, 3] + [rng.randrange(4) for _ in range(60)]
    corpus = corpus_of(picks, bases)
    rep = host_classes(corpus)
    dup = np.nonzero(rep != np.arange(len(rep)))[0]
    n0, e0 = corpus.node_off[:-1].astype(np.int64), corpus.edge_off[:-1].astype(np.int64)
    assert corpus.n_graphs - 1 in dup
    assert set((n0[dup] % 16).tolist()) == set(range(16))
    assert set(((n0[dup] + dup) % 4).tolist()) == set(range(4)) and set((e0[dup] % 4).tolist()) == set(range(4))
    assert set(((5 * n0[dup]) % 4).tolist()) == set(range(4))
    check(eng, corpus, expect_dups=True)
