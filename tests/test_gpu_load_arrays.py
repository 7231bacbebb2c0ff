"""What nemo_load_corpus leaves on the device (forward and reverse CSR, Kahn order and levels, and the post
graphs' edges in source Kahn order) against the plain reference of tests/load_reference.py, exactly, under
every build that can produce them: k_build with peeling or relaxation levels, the global tier (k_csr +
k_topo), and for the graphs of NEMO_CSR_BIG nodes or more the bucketed build with k_topo_deep or k_topo_ell.
The cases sit on the builds' degree- and size-dependent branches: row lengths around the sorting networks'
sizes with mixed lengths in a wave, in-degrees around the u8 counters' end, level counts around the
relaxation's hand-back to peeling, duplicate edges in long rows (the relationships-created count), hub rows
in the bucketed build's sort paths, and the graphs' position in the corpus."""
import functools

import numpy as np
import pytest

from nemo_amd import engine as E
from nemo_amd.corpus import corpus_from_graphs
from tests import load_cases as C
from tests import load_reference as R
from tests.test_gpu_build_input import EMPTY, ONE
from tests.test_gpu_deep import _inject, wide_prov

pytestmark = pytest.mark.gpu

CSR_BIG = 8192  # NEMO_CSR_BIG (device.h)


@pytest.fixture(scope="module")
def eng():
    e = E.Engine(0)
    yield e
    e.close()


@pytest.fixture(params=["peel", "relax", "global"])
def build(request, eng):
    """k_build with peeling levels (the defaults), k_build with relaxation levels, or the global tier."""
    try:
        if request.param == "relax":
            eng.set_option("build_relax", 1)
        elif request.param == "global":
            eng.set_option("build_lds_max", 0)
        yield request.param
    finally:
        eng.set_option("build_relax", -1)
        eng.set_option("build_lds_max", -1)


@pytest.fixture(params=["topo_deep", "topo_ell"])
def kahn(request, eng):
    """The big graphs' Kahn levels by k_topo_deep or by k_topo_ell (as tests/test_gpu_deep.py's kahn)."""
    try:
        if request.param == "topo_ell":
            eng.set_option("topo_ell", 1)
            eng.set_option("chains_glob_min_v", 0)
        else:
            eng.set_option("topo_ell", 0)
        yield request.param
    finally:
        eng.set_option("topo_ell", -1)
        eng.set_option("chains_glob_min_v", 65536)


class Case:
    """A corpus and its reference, computed once and shared by the builds."""

    def __init__(self, runs):
        self.corpus = corpus_from_graphs(runs)
        self.refs = [R.graph_reference(self.corpus, g) for g in range(self.corpus.n_graphs)]
        for ref in self.refs:
            assert ref["created"] == ref["E"]


def check_arrays(eng, corpus, graphs=None, refs=None):
    """The loaded corpus' device arrays against the reference, for every graph (or `graphs`).  Returns the
    graphs k_build built (those outside the global tier's list), the post graphs among them whose e2 /
    posoff were checked, and the redo flags."""
    G = corpus.n_graphs
    no, eo = corpus.node_off.astype(np.int64), corpus.edge_off.astype(np.int64)
    V, Ed = int(no[-1]), int(eo[-1])
    sizes = {"fp": V + G, "rp": V + G, "fc": Ed, "rc": Ed, "topo": V, "lvl": V + G, "nlv": V, "nlev": G, "e2": Ed,
             "posoff": V}
    got = {k: eng.debug_copy(k, 0, 4 * n).view(np.uint32).astype(np.int64) if n else np.zeros(0, np.int64)
           for k, n in sizes.items()}
    redo = eng.debug_copy("redo", 0, G).astype(np.int64)
    # the load worklist (k_load_sel): the graphs k_csr / k_topo or the big-graph kernels take
    sel = eng.debug_copy("sel", 4 * 2 * (G + 1), 4 * (G + 1)).view(np.uint32)
    rest = set(sel[1:1 + int(sel[0])].tolist())
    built, e2_checked = [], []
    for g in (range(G) if graphs is None else graphs):
        ref = refs[g] if refs is not None else R.graph_reference(corpus, g)
        n0, e0, Vg, Eg = int(no[g]), int(eo[g]), ref["V"], ref["E"]
        assert (Vg, Eg) == (int(no[g + 1]) - n0, int(eo[g + 1]) - e0)
        for ptr, col in (("fp", "fc"), ("rp", "rc")):
            assert np.array_equal(got[ptr][n0 + g:n0 + g + Vg + 1], ref[ptr]), (g, ptr)
            assert np.array_equal(got[col][e0:e0 + Eg], ref[col]), (g, col)
        assert int(got["nlev"][g]) == ref["nlev"], g
        assert np.array_equal(got["nlv"][n0:n0 + Vg], ref["nlv"]), (g, "nlv")
        lvl = got["lvl"][n0 + g:n0 + g + ref["nlev"] + 1]
        assert np.array_equal(lvl, ref["lvl"]) and int(lvl[-1]) == Vg, (g, "lvl")
        topo = got["topo"][n0:n0 + Vg]
        assert np.array_equal(np.sort(topo), np.arange(Vg)), (g, "topo is no permutation")
        # level l's slice of topo is exactly the nodes of level l: the level of topo[p] is p's slice
        assert np.array_equal(ref["nlv"][topo], np.repeat(np.arange(ref["nlev"]), np.diff(ref["lvl"]))), (g, "topo")
        if g in rest:
            continue
        built.append(g)
        if g & 1:
            posoff, e2 = R.e2_reference(ref, topo)
            assert np.array_equal(got["posoff"][n0:n0 + Vg], posoff), (g, "posoff")
            assert np.array_equal(got["e2"][e0:e0 + Eg], e2), (g, "e2")
            e2_checked.append(g)
    return {"built": built, "e2": e2_checked, "redo": redo}


def _load_and_check(eng, case, build):
    eng.load(case.corpus)
    out = check_arrays(eng, case.corpus, refs=case.refs)
    if build == "global":
        assert not out["built"]
    else:
        assert out["e2"], "no post graph's e2 / posoff was checked under a k_build setting"
    return out


# ---- (a) row-length ladder, (f) position in the corpus ----

@functools.lru_cache(maxsize=None)
def _ladder_case(layout):
    runs = C.ladder_runs()
    if layout == "reversed":
        runs = [(it, st, pre, post) for it, (_, st, pre, post) in enumerate(reversed(runs))]
    elif layout == "gaps":  # an empty and a one-node graph between the ladder graphs, as pre and as post graphs
        out = []
        for k, (_, st, pre, post) in enumerate(runs):
            out.append((st, pre, post))
            if k % 5 == 4:
                out.append(("success", EMPTY, ONE) if k % 2 else ("success", ONE, EMPTY))
        runs = [(it, st, pre, post) for it, (st, pre, post) in enumerate(out)]
    return Case(runs)


@pytest.mark.parametrize("layout", ["forward", "reversed", "gaps"])
def test_row_length_ladder(eng, build, layout):
    case = _ladder_case(layout)
    assert int(np.diff(case.corpus.node_off.astype(np.int64)).max()) < CSR_BIG
    out = _load_and_check(eng, case, build)
    if build != "global":  # every graph inside k_build's caps, none handed back
        assert out["built"] == list(range(case.corpus.n_graphs)) and not out["redo"].any()
        assert out["e2"] == list(range(1, case.corpus.n_graphs, 2))


# ---- (b) in-degrees around the u8 counters' end ----

INDEG = [(d, kind) for kind in ("goal", "rule") for d in (254, 255, 256, 257)]


@functools.lru_cache(maxsize=None)
def _indegree_case():
    return Case([(it, "success", C.small_path(5), C.indegree(d, kind)) for it, (d, kind) in enumerate(INDEG)])


def test_indegree_redo_boundary(eng, build):
    case = _indegree_case()
    out = _load_and_check(eng, case, build)
    if build != "global":
        for r, (d, kind) in enumerate(INDEG):
            assert int(np.diff(case.refs[2 * r + 1]["rp"]).max()) == d
            assert int(out["redo"][2 * r + 1]) == (1 if d >= 256 else 0), (d, kind)
            assert ((2 * r + 1) in out["built"]) == (d <= 255), (d, kind)


# ---- (c) relaxation hand-back ----

def _lcap(V):
    """k_build's relaxation level cap (k_load.hip: min(254, lds_align(4 * ceil(V / 32)) / 2 - 1))."""
    bitmap = (4 * ((V + 31) // 32) + 15) & ~15
    return min(254, bitmap // 2 - 1)


RELAX_V = (48, 4100)


@functools.lru_cache(maxsize=None)
def _relax_case():
    assert _lcap(RELAX_V[0]) == 7 and _lcap(RELAX_V[1]) == 254
    assert (4 * ((RELAX_V[1] + 31) // 32) + 15 & ~15) // 2 - 1 > 254  # the 254 cap binds, not the bitmap's bytes
    shapes = [(_lcap(V) + k, V, order) for V in RELAX_V for k in (-1, 0, 1, 2) for order in ("asc", "desc")]
    case = Case([(it, "success", C.small_path(5), C.levels(*s)) for it, s in enumerate(shapes)])
    for r, (L, V, _) in enumerate(shapes):
        assert (case.refs[2 * r + 1]["nlev"], case.refs[2 * r + 1]["V"]) == (L, V)
    return case


def test_relaxation_hand_back(eng, build):
    case = _relax_case()
    out = _load_and_check(eng, case, build)
    if build != "global":  # past the cap the levels come from k_build's own peeling: nothing is redone
        assert out["built"] == list(range(case.corpus.n_graphs)) and not out["redo"].any()


# ---- (d) relationships created on the LDS and global tiers ----

def _row(corpus, g, v, forward):
    """Sorted entries of v's forward (reverse) row in graph g of the corpus' edge list."""
    _, src, dst, _ = R.graph_edges(corpus, g)
    return sorted((dst[src == v] if forward else src[dst == v]).tolist())


@pytest.mark.parametrize("n", [2, 4, 5, 8, 9, 16, 17, 33])
def test_created_count_duplicates_in_long_rows(eng, build, n):
    """Duplicates of the first, the last (node V - 1) and, twice, a middle entry of the ladder graph's long
    rows (goal a's forward row: the global tier counts there; goal c's reverse row: k_build does), with a
    goal -> goal edge: the load reports the distinct goal <-> rule edges."""
    for mix8 in (False, True):
        _, _, _, role = C.ladder_index(n, mix8, "shuf")
        runs = [(0, "success", C.small_path(5), C.ladder(n, mix8, "shuf"))]
        clean = corpus_from_graphs(runs)
        Vg = clean.graph_size(1)
        for forward in (True, False):
            v = role["a"] if forward else role["c"]
            row = _row(clean, 1, v, forward)
            assert len(row) == n and row[-1] == Vg - 1
            edge = (lambda t: (v, t)) if forward else (lambda t: (t, v))
            for extra in ([edge(row[0])], [edge(row[-1])], [edge(row[n // 2])] * 2):
                corpus = corpus_from_graphs(runs)
                _inject(corpus, 1, extra + [(role["a"], role["c"])])
                want, E_ = R.created(corpus, 1)
                assert want == E_ - len(extra) - 1
                with pytest.raises(E.NemoError) as ei:
                    eng.load(corpus)
                assert f"inserted number of edges ({want}) does not equal number of antecedent provenance " \
                    f"edges ({E_})" in str(ei.value), (mix8, forward, extra)
        eng.load(clean)
        out = check_arrays(eng, clean)
        assert (out["e2"] == [1]) == (build != "global")


# ---- (e) the big tier's rows ----

def _add_hub(prov, goal, count, tag):
    """`count` rule children (each with a goal child) below goal `goal` of a wide_prov graph."""
    for k in range(count):
        prov["rules"].append({"id": f"rule_{tag}{k}", "label": "t1", "table": "t1", "type": "single"})
        prov["goals"].append({"id": f"goal_{tag}{k}", "label": f"t1({tag}{k})", "table": "t1", "time": "2"})
        prov["edges"] += [{"from": goal, "to": f"rule_{tag}{k}"}, {"from": f"rule_{tag}{k}", "to": f"goal_{tag}{k}"}]
    return prov


@functools.lru_cache(maxsize=None)
def _big_case(name):
    small = (1, "failure", C.small_path(5), C.ladder(9, True, "shuf"))  # one k_build graph beside the big ones
    if name == "hubs":  # rows of 16, 17 (networks / wave sort), 64, 65 (wave / thread sort) and 300 entries
        post = wide_prov("post", 1500, 7)
        for i, h in enumerate((16, 17, 64, 65, 300)):
            goal = f"goal_a{i + 1}"
            have = sum(1 for e in post["edges"] if e["from"] == goal)  # its own rule and the cross edges
            _add_hub(post, goal, h - have, f"hub{h}x")
        case = Case([(0, "success", C.small_path(7), post), small])
        V = case.refs[1]["V"]
        assert CSR_BIG < V < CSR_BIG + 512
        assert {16, 17, 64, 65, 300} <= set(np.diff(case.refs[1]["fp"]).tolist())
    elif name == "hbm_bucket":  # a 15000-entry row: its bucket is past the LDS capacity
        case = Case([(0, "success", C.small_path(7), wide_prov("post", 100, 8, hub=15000)), small])
        assert int(np.diff(case.refs[1]["fp"]).max()) >= 15000 and case.refs[1]["V"] >= CSR_BIG
    else:  # the boundary itself: the last graph of the one-workgroup global build, the first of the bucketed one
        case = Case([(0, "success", C.small_path(7), C.levels(40, CSR_BIG - 1, "desc")),
                     (2, "success", C.small_path(9), C.levels(41, CSR_BIG, "asc")), small])
        assert [case.refs[g]["V"] for g in (1, 3)] == [CSR_BIG - 1, CSR_BIG]
    return case


@pytest.mark.parametrize("name", ["hubs", "hbm_bucket", "boundary"])
def test_big_graph_rows(eng, build, kahn, name):
    case = _big_case(name)
    out = _load_and_check(eng, case, build)
    assert not any(case.refs[g]["V"] >= CSR_BIG - 1 for g in out["built"])
