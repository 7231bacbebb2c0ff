"""Failure classes on the GPU (nemo_diff_classes, nemo_amd/csrc/k_dclass.hip): the entries of a diffprov
grouped by identical D mask, |D| per class and the per-node support.

Expected values always come from the CPU oracle's masks (oracle/nemo_oracle.c, diff-only mode), never from the
device's: the partition by np.unique over the mask rows renumbered by smallest entry, `nodes` as row sums and the
support as column sums.  Every comparison is an exact array comparison.  Option class_hash_bits = 0 makes every
mask collide in the hash buckets, so those runs prove the classes rest on the exact row comparisons alone.

Summarises differential-provenance.go:18-146 (one diff per failed run); no reference code computes classes.
"""
import dataclasses
import functools
import os

import numpy as np
import pytest

from nemo_amd import engine as E
from nemo_amd.corpus import DIFF_PER_RUN, DIFF_REFERENCE, NODE_RULE
from oracle import oracle as O
from tools import synth

pytestmark = pytest.mark.gpu

ERR_STATE = 5


@pytest.fixture(scope="module")
def eng():
    e = E.Engine(0)
    yield e
    e.close()


def expected(masks):
    """(class_of, classes[k] = (rep, size, nodes), support) of mask rows, by membership."""
    m = np.asarray(masks) != 0
    n = m.shape[0]
    if n == 0:
        return np.zeros(0, np.uint32), np.zeros((0, 3), np.uint32), np.zeros(m.shape[1] if m.ndim == 2 else 0, np.uint32)
    _, first, inv = np.unique(m, axis=0, return_index=True, return_inverse=True)
    inv = np.asarray(inv).reshape(-1)
    order = np.argsort(first)  # classes by smallest entry
    rank = np.empty(len(first), np.int64)
    rank[order] = np.arange(len(first))
    class_of = rank[inv]
    size = np.bincount(class_of, minlength=len(first))
    reps = first[order]
    classes = np.stack([reps, size, m[reps].sum(1)], 1)
    return class_of.astype(np.uint32), classes.astype(np.uint32), m.sum(0).astype(np.uint32)


def oracle_masks(corpus, f, mode):
    return np.asarray(O.analyze(corpus, [0], f, diff_mode=mode, threads=8, diff_only=True).diff_mask)


def check(eng, want, bits=128, what=""):
    eng.set_option("class_hash_bits", bits)
    try:
        class_of, classes = eng.diff_classes()
        support = eng.diff_support()
    finally:
        eng.set_option("class_hash_bits", -1)
    assert np.array_equal(class_of, want[0]), f"class_of differs ({what}, {bits} hash bits)"
    assert np.array_equal(classes, want[1]), f"classes differ ({what}, {bits} hash bits)"
    assert np.array_equal(support, want[2]), f"support differs ({what}, {bits} hash bits)"


@functools.lru_cache(maxsize=None)
def c3_corpus(runs):
    return synth.generate(runs, p_fault=0.55, prepend_run0=True, **synth.CONFIGS["c3"])[0]


def test_c3_shape_two_chunks(eng):
    corpus = c3_corpus(170)
    f = corpus.failed_iters()
    assert len(f) > 64  # two 64-source chunks
    want = expected(oracle_masks(corpus, f, DIFF_PER_RUN))
    assert len(want[1]) >= 20 and int((want[1][:, 1] >= 2).sum()) >= 2
    eng.load(corpus)
    eng.mark()
    eng.diffprov(f, DIFF_PER_RUN)
    for bits in (128, 8, 0):
        check(eng, want, bits, "per-run")
    eng.set_option("diff_legacy", 1)  # the masks arrive through d_dumask and the expand
    try:
        eng.diffprov(f, DIFF_PER_RUN)
        check(eng, want, 128, "legacy kernels")
    finally:
        eng.set_option("diff_legacy", 0)
    eng.diffprov(f, DIFF_REFERENCE)
    ref = expected(oracle_masks(corpus, f, DIFF_REFERENCE))
    assert len(ref[1]) == 1 and int(ref[1][0, 1]) == len(f)  # one source: one class of n
    check(eng, ref, 128, "reference")
    check(eng, ref, 0, "reference")


def near_miss_corpus():
    """Run 0 of a 3-run C3-shape corpus and six copies of it as failed runs 1..6; in copy k's post graph the
    goals sets[k - 1] carry a label that no run-0 post goal carries, so that D is exactly what those goals span."""
    base = synth.generate(3, prepend_run0=True, **synth.CONFIGS["c3"])[0]
    r0 = base.run_index(0)
    c = base.subset([r0] * 7)
    label = c.label.copy()
    g0 = 1
    a, b = int(c.node_off[g0]), int(c.node_off[g0 + 1])
    goals = np.nonzero((c.node_word[a:b] & NODE_RULE) == 0)[0]
    first, last, mid = int(goals[0]), int(goals[-1]), int(goals[len(goals) // 2])
    sets = [[first], [last], [first, last], [last], [], [mid]]
    fresh = int(label.max()) + 1
    for k, s in enumerate(sets, start=1):
        off = int(c.node_off[2 * k + 1])
        for v in s:
            label[off + v] = fresh
    c = dataclasses.replace(c, iteration=np.arange(7, dtype=np.uint32), label=np.ascontiguousarray(label),
                            status=["success"] + ["failure"] * 6)
    return c, b - a


def test_near_miss_masks(eng):
    corpus, V0 = near_miss_corpus()
    assert V0 % 16 != 0
    f = [1, 2, 3, 4, 5, 6]
    masks = oracle_masks(corpus, f, DIFF_PER_RUN) != 0
    want = expected(masks)
    sizes = want[1][:, 1].tolist()
    assert 2 in sizes  # [last] twice
    assert 0 in want[1][:, 2].tolist()  # the unchanged copy: an empty D
    reps = want[1][:, 0]
    assert any(int((masks[i] != masks[j]).sum()) == 1 for i in reps for j in reps if i < j)  # classes one node apart
    eng.load(corpus)
    eng.mark()
    for ff in (f, [6, 2, 2, 5, 4, 1, 3, 5, 5, 2]):  # and duplicated, permuted entries
        w = want if ff is f else expected(oracle_masks(corpus, ff, DIFF_PER_RUN))
        eng.diffprov(ff, DIFF_PER_RUN)
        for bits in (128, 0):
            check(eng, w, bits, f"near-miss, {len(ff)} entries")


def test_tiny_graphs(eng):
    from tests.small import random_corpus
    done = 0
    for seed in range(100, 160):
        corpus, _ = random_corpus(seed, n_runs=12, max_nodes=40)
        f = corpus.failed_iters()
        if not f or 0 not in set(int(x) for x in corpus.iteration):
            continue
        want = expected(oracle_masks(corpus, f, DIFF_PER_RUN))
        eng.load(corpus)
        eng.mark()
        eng.diffprov(f, DIFF_PER_RUN)
        for bits in (128, 0):
            check(eng, want, bits, f"tiny seed {seed}")
        done += 1
        if done == 4:
            break
    assert done == 4


def test_deep_shape(eng):
    corpus, _ = synth.generate(10, target_nodes=40000, eot=40, body_extra=6, nval=3, nloc=4, p_fault=0.5,
                               prepend_run0=True)
    f = corpus.failed_iters()
    want = expected(oracle_masks(corpus, f, DIFF_PER_RUN))
    assert sorted(want[1][:, 1].tolist()) == [1, 3]
    eng.load(corpus)
    eng.mark()
    eng.diffprov(f, DIFF_PER_RUN)  # the default windowed walks
    for bits in (128, 0):
        check(eng, want, bits, "deep")


def test_state(eng):
    corpus = c3_corpus(60)
    f = corpus.failed_iters()
    L = eng.L
    eng.load(corpus)
    eng.mark()
    n = E.ctypes.c_uint64()
    sup = np.zeros(1 << 16, np.uint32)
    # no diffprov since the load
    assert L.nemo_diff_classes(eng.h) == ERR_STATE
    assert L.nemo_fetch_diff_classes(eng.h, None, None, 0, E.ctypes.byref(n)) == ERR_STATE
    assert L.nemo_fetch_diff_support(eng.h, sup.ctypes.data, len(sup)) == ERR_STATE
    want = expected(oracle_masks(corpus, f, DIFF_PER_RUN))
    eng.diffprov(f, DIFF_PER_RUN)
    check(eng, want, 128, "first call")
    # a symmetric diff in between leaves the classes fetchable and unchanged
    eng.diffprov_symmetric(f)
    eng.synchronize()
    cls = np.zeros((len(want[1]), 3), np.uint32)
    cof = np.zeros(len(f), np.uint32)
    assert L.nemo_fetch_diff_classes(eng.h, cof.ctypes.data, cls.ctypes.data, len(cls), E.ctypes.byref(n)) == 0
    assert n.value == len(want[1]) and np.array_equal(cof, want[0]) and np.array_equal(cls, want[1])
    # a second diffprov invalidates them until the next nemo_diff_classes
    eng.diffprov(f[:5], DIFF_PER_RUN)
    assert L.nemo_fetch_diff_classes(eng.h, None, None, 0, E.ctypes.byref(n)) == ERR_STATE
    assert L.nemo_fetch_diff_support(eng.h, sup.ctypes.data, len(sup)) == ERR_STATE
    check(eng, expected(oracle_masks(corpus, f[:5], DIFF_PER_RUN)), 128, "five entries")
    # a rebuild invalidates them too
    eng.rebuild()
    eng.mark()
    assert L.nemo_fetch_diff_classes(eng.h, None, None, 0, E.ctypes.byref(n)) == ERR_STATE
    # zero entries: zero classes
    eng.diffprov([], DIFF_PER_RUN)
    class_of, classes = eng.diff_classes()
    assert len(class_of) == 0 and len(classes) == 0
    assert not eng.diff_support().any()


def test_node_context(eng):
    """Three shards on one device: class_of, classes and support identical to the single-device context's."""
    corpus = c3_corpus(60)
    f = corpus.failed_iters()
    want = expected(oracle_masks(corpus, f, DIFF_PER_RUN))
    eng.load(corpus)
    eng.mark()
    eng.diffprov(f, DIFF_PER_RUN)
    one = eng.diff_classes(), eng.diff_support()
    eng.load(synth.generate(2, target_nodes=100)[0])  # release the single context's corpus
    node = E.Engine(devices=[0] * 3)
    try:
        node.load(corpus)
        node.mark()
        node.diffprov(f, DIFF_PER_RUN)
        for bits in (128, 0):
            check(node, want, bits, "node context")
        got = node.diff_classes(), node.diff_support()
        node.diffprov(f, DIFF_REFERENCE)
        check(node, expected(oracle_masks(corpus, f, DIFF_REFERENCE)), 128, "node context, reference")
    finally:
        node.close()
    assert np.array_equal(got[0][0], one[0][0]) and np.array_equal(got[0][1], one[0][1])
    assert np.array_equal(got[1], one[1])


def test_failure_classes_golden():
    """Neo4J.FailureClasses against the grouping computed here from CreateNaiveDiffProv's own per-run outputs."""
    from nemo_amd import graphing as GR
    from nemo_amd.corpus import load_molly
    d = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cs_ca_2434_bootstrap_synchronization")
    corpus = load_molly(d)
    f = corpus.failed_iters()
    assert f
    db = GR.Neo4J()
    db.InitGraphDB("bolt://127.0.0.1:7687", corpus)
    try:
        db.diff_mode = DIFF_PER_RUN
        db.LoadRawProvenance()
        db.SimplifyProv([int(x) for x in corpus.iteration])
        _, post, _, _ = db.PullPrePostProv()
        diffs, _, missing = db.CreateNaiveDiffProv(False, f, post[0])
        masks = db.eng.diff_masks(len(f))
        recs = db.FailureClasses(f, post[0])
        diffs2, _, missing2 = db.CreateNaiveDiffProv(False, f, post[0])
    finally:
        db.CloseDB()
    assert [x.string() for x in diffs2] == [x.string() for x in diffs] and missing2 == missing  # unchanged by the call
    want = expected(oracle_masks(corpus, f, DIFF_PER_RUN))
    assert np.array_equal(expected(masks)[0], want[0])
    groups = sorted(range(len(want[1])), key=lambda k: (-int(want[1][k, 1]), int(want[1][k, 0])))
    assert len(recs) == len(groups)
    for rec, k in zip(recs, groups):
        rep = int(want[1][k, 0])
        assert rec["Representative"] == f[rep]
        assert rec["Members"] == [f[e] for e in range(len(f)) if want[0][e] == k]
        assert rec["Nodes"] == int(want[1][k, 2])
        assert rec["Missing"] == missing[rep]
        assert rec["Diff"].string() == diffs[rep].string()
