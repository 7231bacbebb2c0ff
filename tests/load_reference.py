"""A plain reference of what a load leaves on the device, per graph g of a Corpus, from edge_src /
edge_dst / node_word alone (numpy and Python only; nothing of the engine or the oracle is imported):

- fp / fc, rp / rc: row pointers (V + 1 entries, first 0, last E) and rows of the forward and the
  reverse CSR.  A row is the ascending multiset of its entries.  corpus.py's CorpusBuilder drops a
  repeated (src, dst) pair and an edge that does not join a goal and a rule, and then fails the
  graph's edge count, so a loadable corpus holds no duplicate edge and its rows are strictly
  ascending: graph_reference asserts that.
- level(v): the longest path from a source to v (0 for a source), computed twice, by Kahn peeling
  and by a memoised longest-path recursion over the reverse rows; the two must agree.
- nlev, lvl (offsets of the level sizes, nlev + 1 entries, the last V), nlv (level per node).
- created(g): the relationships-created count of pre-post-prov.go:150-210, the number of distinct
  (src, dst) pairs whose endpoints differ in the rule bit.
- e2 / posoff of a post graph that k_build built, given the device's own Kahn order topo (the order
  inside a level depends on timing; topo is checked on its own).  Both halves of an e2 entry are node
  indices local to the graph, not Kahn positions: k_proto_lds indexes its per-node bytes with them.
  posoff has one entry per Kahn position, V per graph at the graph's node offset; k_proto_lds reads
  posoff[lvl[l]] as the first edge leaving level l.  The statement it relies on:
      posoff[p] = sum of the out-degrees of topo[0..p),
      e2[posoff[p] + k] = topo[p] << 16 | (k-th entry of topo[p]'s sorted forward row).
"""
import numpy as np

NODE_RULE = 0x80000000


def graph_edges(corpus, g):
    """(V, src, dst, is_rule) of graph g; src / dst local int64 arrays in the corpus' edge order."""
    no, eo = corpus.node_off.astype(np.int64), corpus.edge_off.astype(np.int64)
    V = int(no[g + 1] - no[g])
    src = corpus.edge_src[eo[g]:eo[g + 1]].astype(np.int64)
    dst = corpus.edge_dst[eo[g]:eo[g + 1]].astype(np.int64)
    rule = (corpus.node_word[no[g]:no[g + 1]].astype(np.int64) & NODE_RULE) != 0
    return V, src, dst, rule


def created(corpus, g):
    """(relationships created, E): distinct edges that join a goal and a rule, and the edge count."""
    _, src, dst, rule = graph_edges(corpus, g)
    pairs = set(zip(src.tolist(), dst.tolist()))
    return sum(1 for x, y in pairs if rule[x] != rule[y]), len(src)


def csr_rows(V, key, val):
    """Row pointers and rows of the CSR keyed by `key`: row v holds the val of every edge whose key is v,
    ascending."""
    ptr = np.zeros(V + 1, np.int64)
    np.cumsum(np.bincount(key, minlength=V), out=ptr[1:])
    col = val[np.lexsort((val, key))]
    return ptr, col


def levels_peel(V, fp, fc, rp):
    """Kahn peeling: level 0 is the nodes without parents; a node joins the level after the one that
    removed its last parent.  None if the graph has a cycle."""
    indeg = np.diff(rp)
    level = np.full(V, -1, np.int64)
    cur = np.flatnonzero(indeg == 0)
    done, l = 0, 0
    while len(cur):
        level[cur] = l
        done += len(cur)
        nxt = []
        for u in cur.tolist():
            for w in fc[fp[u]:fp[u + 1]].tolist():
                indeg[w] -= 1
                if indeg[w] == 0:
                    nxt.append(w)
        cur = np.asarray(nxt, np.int64)
        l += 1
    return level if done == V else None


def levels_longest(V, rp, rc):
    """level(v) = 0 without parents, else 1 + max over v's parents: memoised, on an explicit stack
    (a path of thousands of nodes is deeper than Python's recursion limit).  Needs an acyclic graph."""
    level = [-1] * V
    for root in range(V):
        if level[root] >= 0:
            continue
        stack = [root]
        while stack:
            v = stack[-1]
            par = rc[rp[v]:rp[v + 1]].tolist()
            todo = [u for u in par if level[u] < 0]
            if todo:
                stack.extend(todo)
                continue
            stack.pop()
            level[v] = 1 + max((level[u] for u in par), default=-1)
    return np.asarray(level, np.int64)


def graph_reference(corpus, g):
    """dict of fp, fc, rp, rc, nlv, nlev, lvl, created, V, E of graph g (int64 arrays)."""
    V, src, dst, rule = graph_edges(corpus, g)
    assert len(src) == 0 or (src.min() >= 0 and max(src.max(), dst.max()) < V)
    fp, fc = csr_rows(V, src, dst)
    rp, rc = csr_rows(V, dst, src)
    for ptr, col in ((fp, fc), (rp, rc)):
        assert ptr[0] == 0 and ptr[-1] == len(src)
        row = np.repeat(np.arange(V), np.diff(ptr))
        assert np.all((row[1:] != row[:-1]) | (col[1:] > col[:-1])), "rows of a loadable graph are strictly ascending"
    nlv = levels_peel(V, fp, fc, rp)
    assert nlv is not None, "cycle"
    assert np.array_equal(nlv, levels_longest(V, rp, rc)), "the two level forms disagree"
    nlev = int(nlv.max()) + 1 if V else 0
    lvl = np.zeros(nlev + 1, np.int64)
    np.cumsum(np.bincount(nlv, minlength=nlev), out=lvl[1:])
    w, E = created(corpus, g)
    return {"V": V, "E": E, "fp": fp, "fc": fc, "rp": rp, "rc": rc, "nlv": nlv, "nlev": nlev, "lvl": lvl,
            "created": w}


def e2_reference(ref, topo):
    """(posoff, e2) of a post graph from its reference rows and the device's Kahn order (see the module text)."""
    fp, fc = ref["fp"], ref["fc"]
    topo = np.asarray(topo, np.int64)
    deg = (fp[1:] - fp[:-1])[topo]
    posoff = np.zeros(len(topo), np.int64)
    if len(topo):
        np.cumsum(deg[:-1], out=posoff[1:])
    e2 = np.zeros(ref["E"], np.int64)
    for p, u in enumerate(topo.tolist()):
        row = fc[fp[u]:fp[u + 1]]
        e2[posoff[p]:posoff[p] + len(row)] = (u << 16) | row
    return posoff, e2
