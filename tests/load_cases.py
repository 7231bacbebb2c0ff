"""Graphs for the load's array checks (tests/test_gpu_load_arrays.py, tests/test_load_reference_host.py),
built in index space: CorpusBuilder numbers a graph's goals first, in list order, then its rules, and keeps
the edge list's order, so a generator decides which 64 consecutive indices (one wave of k_build's row
sort) a row shares and in which order a row's entries arrive."""
import random

SHUFFLE_SEED = 20240611  # the shuffled edge orders
LADDER_N = (1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 64, 65)
FILL = 6  # row length of the mixed-wave fillers (the 8-key network's range, 5..8)


def prov(ng, nr, edges):
    """Molly-shaped graph of goals 0..ng-1 and rules ng..ng+nr-1 with `edges` [(src, dst)] in that order."""
    name = lambda i: f"goal{i}" if i < ng else f"rule{i}"
    goals = [{"id": name(i), "label": f"{'post' if i == 0 else 't1'}(a, {i})", "table": "post" if i == 0 else "t1",
              "time": str(1 + i % 3)} for i in range(ng)]
    rules = [{"id": name(i), "label": "t1", "table": "post" if i == ng else "t1", "type": "next" if i % 3 else "single"}
             for i in range(ng, ng + nr)]
    return {"goals": goals, "rules": rules, "edges": [{"from": name(s), "to": name(d)} for s, d in edges]}


def order_edges(edges, order):
    edges = sorted(edges)
    if order == "desc":
        edges.reverse()
    elif order == "shuf":
        random.Random(SHUFFLE_SEED).shuffle(edges)
    else:
        assert order == "asc"
    return edges


def ladder_index(n, mix8, order):
    """(ng, nr, edges, roles) of the ladder graph of row length n.  Goal a has n rule children ra_i, which are
    the n rule parents of goal c; c -> rule b, which has n goal children gb_i, the n goal parents of rule
    d: goal / rule x forward / reverse rows of length n.  With mix8 the waves of a, c and of b, d also hold
    rows of FILL entries (f, h, k, m: the same figure with FILL); without, every other row there has at
    most one entry.  The last rule, node V - 1, is ra_{n-1}: the last entry of a's forward and of c's
    reverse row.  roles: node index of a, c, b, d."""
    gn = ["a", "c"] + (["f", "h"] + [f"gk{j}" for j in range(FILL)] if mix8 else []) + [f"gb{i}" for i in range(n)]
    lead = 4 if mix8 else 2
    while len(gn) % 64 > 64 - lead:  # b, d (k, m) in one wave
        gn.append(f"pad{len(gn)}")
    rn = ["b", "d"] + (["k", "m"] + [f"rf{j}" for j in range(FILL)] if mix8 else []) + [f"ra{i}" for i in range(n)]
    ix = {x: i for i, x in enumerate(gn + rn)}
    e = [("c", "b")]
    for i in range(n):
        e += [("a", f"ra{i}"), (f"ra{i}", "c"), ("b", f"gb{i}"), (f"gb{i}", "d")]
    if mix8:
        e.append(("h", "k"))
        for j in range(FILL):
            e += [("f", f"rf{j}"), (f"rf{j}", "h"), ("k", f"gk{j}"), (f"gk{j}", "m")]
    edges = order_edges([(ix[s], ix[d]) for s, d in e], order)
    assert ix["b"] // 64 == ix[rn[lead - 1]] // 64 and ix[f"ra{n - 1}"] == len(ix) - 1
    return len(gn), len(rn), edges, {k: ix[k] for k in "acbd"}


def ladder(n, mix8, order):
    ng, nr, edges, _ = ladder_index(n, mix8, order)
    return prov(ng, nr, edges)


LADDER_VARIANTS = [(n, mix8, order) for n in LADDER_N for mix8 in (False, True) for order in ("desc", "shuf")]


def small_path(k):
    """The pre graphs: goal -> rule -> goal ... of k nodes."""
    ng = (k + 1) // 2
    node = lambda i: i // 2 if i % 2 == 0 else ng + i // 2
    return prov(ng, k - ng, [(node(i), node(i + 1)) for i in range(k - 1)])


def ladder_runs(variants=LADDER_VARIANTS):
    """One run per ladder variant; the pre graphs are one fixed path (so all but the first are duplicates)."""
    return [(it, "success" if it % 3 else "failure", small_path(5), ladder(*v)) for it, v in enumerate(variants)]


def indegree(d, kind):
    """One node of in-degree d, a goal (kind "goal": d rule parents) or a rule (d goal parents), with a child
    and a grandchild below it; shuffled edges."""
    if kind == "goal":  # goals x, u; rules t, p_i:  p_i -> x -> t -> u
        ng, nr = 2, d + 1
        edges = [(3 + i, 0) for i in range(d)] + [(0, 2), (2, 1)]
    else:  # goals q_i, w, u; rules y, t:  q_i -> y -> w -> t -> u
        ng, nr = d + 2, 2
        y, t = ng, ng + 1
        edges = [(i, y) for i in range(d)] + [(y, d), (d, t), (t, d + 1)]
    return prov(ng, nr, order_edges(edges, "shuf"))


def levels(L, V, order):
    """Exactly L >= 2 Kahn levels on V nodes: a path goal -> rule -> goal ... of L nodes, and V - L rule leaves
    below its first goal (level 1).  order: the edge array by source level, "asc" or "desc"."""
    assert 2 <= L <= V
    pg = (L + 1) // 2
    node = lambda i: i // 2 if i % 2 == 0 else pg + i // 2
    edges = [(0, pg + L // 2 + k) for k in range(V - L)] + [(node(i), node(i + 1)) for i in range(L - 1)]
    if order == "desc":
        edges.reverse()
    return prov(pg, V - pg, edges)
