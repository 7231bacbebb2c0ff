"""Host-side checks of the symmetric diff (no GPU): the C ABI declares and exports the new entry
points, and dot.create_surplus_dot's marks are pinned on a golden fixture with a hand-made mask.

The marks must use attributes createDOT / createDiffDot (graphing/diagrams.go) never set, so that a
marked graph keeps every colour and style the report reads: penwidth for S, peripheries for the
nodes of a surplus event."""
import ctypes
import hashlib
import os
import subprocess

import numpy as np

from nemo_amd import engine as E
from nemo_amd.corpus import NODE_RULE, TABLE_MASK, load_molly
from nemo_amd.dot import ProvNode, create_dot, create_surplus_dot, read_dot

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "cs_mr_2995_failed_after_expiry")
NEW_SYMBOLS = ("nemo_diffprov_symmetric", "nemo_fetch_sdiff_masks", "nemo_fetch_surplus")


def test_header_declares_symmetric_entry_points():
    syms = E.header_symbols()
    for s in NEW_SYMBOLS:
        assert s in syms
    txt = open(E.HEADER).read()
    assert "#define NEMOHIP_ABI_VERSION 1" in txt
    # every new entry point names the reference lines it mirrors; the struct says what `rule` is local to
    assert "differential-provenance.go:18" in txt and ":22-28" in txt and ":82-98" in txt
    assert "in the entry's own failed run's post graph" in txt


def test_library_exports_symmetric_entry_points():
    if not os.path.exists(E.LIB_PATH):
        subprocess.run(["make", "-s", "-C", ROOT, "nemo_amd/libnemohip.so"], check=True)
    L = ctypes.CDLL(E.LIB_PATH)
    assert [s for s in NEW_SYMBOLS if not hasattr(L, s)] == []
    assert L.nemo_abi_version() == 1


def _nodes(corpus, g):
    """ProvNodes of graph g from the corpus' string tables (goal holds flags come from the device: none here)."""
    n0 = int(corpus.node_off[g])
    out = []
    for i in range(corpus.graph_size(g)):
        w = int(corpus.node_word[n0 + i])
        rule = bool(w & NODE_RULE)
        out.append(ProvNode(corpus.node_ids[n0 + i], corpus.labels[int(corpus.label[n0 + i])],
                            corpus.tables[w & TABLE_MASK], corpus.node_types[n0 + i] if rule else None,
                            None, rule, "" if rule else corpus.node_times[n0 + i]))
    return out


def _case():
    corpus = load_molly(FIXTURE)
    r = 2  # a failed run with a 23-node post graph
    assert corpus.status[r] != "success"
    g = 2 * r + 1
    nodes = _nodes(corpus, g)
    e0, e1 = int(corpus.edge_off[g]), int(corpus.edge_off[g + 1])
    src, dst = corpus.edge_src[e0:e1], corpus.edge_dst[e0:e1]
    order = np.lexsort((dst, src))
    edges = [(nodes[int(src[j])], nodes[int(dst[j])]) for j in order]
    return corpus, g, nodes, src, dst, edges


def test_surplus_dot_pinned():
    corpus, g, nodes, src, dst, edges = _case()
    assert (len(nodes), len(edges)) == (23, 22)
    # hand-made S: the first rule (in node order) with a goal parent, that parent and the rule's children
    rule = next(i for i, n in enumerate(nodes) if n.is_rule and (dst == i).any() and (src == i).any())
    parent = int(src[dst == rule][0])
    kids = sorted(int(x) for x in dst[src == rule])
    mask = np.zeros(len(nodes), np.uint8)
    mask[[rule, parent] + kids] = 1
    s_nodes = [nodes[i] for i in np.nonzero(mask)[0]]
    s_edges = [(a, b) for a, b in edges if mask[nodes.index(a)] and mask[nodes.index(b)]]
    ids = {nodes[rule].id} | {nodes[k].id for k in kids}
    got = create_surplus_dot(edges, s_nodes, s_edges, ids)
    plain = create_dot(edges, "post")
    # unmarked nodes and edges are createDOT's, untouched; marked ones gain the two attributes only
    for name, attrs in got.nodes.items():
        extra = {k: v for k, v in attrs.items() if plain.nodes[name].get(k) != v}
        want = {}
        if name in {n.id for n in s_nodes}:
            want["penwidth"] = '"3"'
        if name in ids:
            want["peripheries"] = '"2"'
        assert extra == want, name
    marked = [(e.src, e.dst) for e in got.edges if e.attrs.get("penwidth") == '"3"']
    assert marked == [(a.id, b.id) for a, b in s_edges] and len(marked) == 1 + len(kids)
    assert all(set(e.attrs) <= {"color", "penwidth"} for e in got.edges)
    text = got.string()
    assert read_dot(text).attrs.get("bgcolor") == '"transparent"'
    # pinned statements: the parent goal (S only), the rule (S and surplus event), one S edge
    assert PINNED_PARENT in text and PINNED_RULE in text and PINNED_EDGE in text
    assert hashlib.sha256(text.encode()).hexdigest() == PINNED_SHA256


def test_surplus_dot_isolated_bad_goal():
    # a Bad goal without any edge is in S alone: createDOT never saw it, so the function adds it
    corpus, g, nodes, src, dst, edges = _case()
    lone = ProvNode("run_2_post_goal_lone", "lone(a)", "lone", None, None, False, "1")
    got = create_surplus_dot(edges, [lone], [], set())
    assert got.nodes[lone.id]["penwidth"] == '"3"' and "peripheries" not in got.nodes[lone.id]
    assert got.nodes[lone.id]["shape"] == "ellipse"
    assert not any("penwidth" in e.attrs for e in got.edges)


PINNED_PARENT = ('\trun_2_post_goal0 [ color="black", fillcolor="white", fontcolor="black", label="post(am)", '
                 'penwidth="3", shape=ellipse, style="filled, solid" ];\n')
PINNED_RULE = ('\trun_2_post_rule0 [ color="black", fillcolor="white", fontcolor="black", label="post", '
               'penwidth="3", peripheries="2", shape=rect, style="filled, solid" ];\n')
PINNED_EDGE = '\trun_2_post_rule0->run_2_post_goal1[ color="black", penwidth="3" ];\n'
PINNED_SHA256 = "1813acefeabc480130a4192295cd3cbf31baf236cb8fb716d986fa08346d91e6"
