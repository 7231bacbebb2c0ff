"""The per-call device buffers (nemo_amd/csrc/ctx.h DevBuf): one Engine runs entry lists of 3, 70, 1, 130 and 70
entries, in that order, through the per-run diff, the symmetric diff, the pair diff and the host-label diff with
their fetches, failure classes and pulls.  The lengths cross the 64-entry chunk of the per-entry buffers twice and
shrink in between, so every buffer grows, is reused at a smaller size and grows again; one round runs the
one-workgroup-per-entry diff kernels (option diff_legacy), whose scratch the growing main buffers drop.  pull(0),
pull(1), the chain fetch and the staged hand-over run between the rounds.

Every result is compared, entry by entry and exactly, with a reference computed once on a fresh Engine from the
distinct failed iterations (the entry points accept repeats; entries with one label source share a computation).
No option that changes a result is set.
"""
import numpy as np
import pytest

from nemo_amd import engine as E
from nemo_amd.corpus import DIFF_PER_RUN
from tests.compare import _edge_multiset
from tools import synth

pytestmark = pytest.mark.gpu

LENGTHS = (3, 70, 1, 130, 70)
LABEL_SET_SIZES = (1, 500, 2)


def _slot_edges(n_slots, off, cnt, src, dst):
    """Per slot, the pulled edges as sorted (src, dst) rows: regions land in any order on the device."""
    out = []
    for k in range(n_slots):
        a, n = int(off[k]), int(cnt[k])
        out.append(_edge_multiset(np.zeros(n, np.int64), src[a:a + n], dst[a:a + n]))
    return out


def _all_slots(eng, n_slots):
    off, cnt, src, dst = eng.pulled_all(n_slots)
    slot = np.repeat(np.arange(n_slots, dtype=np.int64), cnt.astype(np.int64))
    idx = np.concatenate([np.arange(int(off[k]), int(off[k]) + int(cnt[k])) for k in range(n_slots)] +
                         [np.zeros(0, np.int64)]).astype(np.int64)
    return _edge_multiset(slot, src[idx], dst[idx])


def _rows_by_entry(rows, n):
    """(entry, rule) rows -> per entry the sorted rules."""
    return [np.sort(rows[rows[:, 0] == e, 1]) for e in range(n)]


def _rows_of(per_entry):
    """The inverse: rows (entry, rule) ordered by entry, then rule, as the fetches return them."""
    rows = [(e, int(r)) for e, rules in enumerate(per_entry) for r in rules]
    return np.asarray(rows, np.uint32).reshape(-1, 2)


def _classes(masks):
    """(class_of, classes[k] = (smallest entry, size, |D|), support) of the mask rows, by membership."""
    m = np.asarray(masks) != 0
    _, first, inv = np.unique(m, axis=0, return_index=True, return_inverse=True)
    inv = np.asarray(inv).reshape(-1)
    order = np.argsort(first)
    rank = np.empty(len(first), np.int64)
    rank[order] = np.arange(len(first))
    class_of = rank[inv]
    reps = first[order]
    classes = np.stack([reps, np.bincount(class_of, minlength=len(first)), m[reps].sum(1)], 1)
    return class_of.astype(np.uint32), classes.astype(np.uint32), m.sum(0).astype(np.uint32)


def _staged(eng, G):
    eng.stage_simplified()
    state, off, ht = eng.simplified_view()
    seg = np.repeat(np.arange(G, dtype=np.int64), np.diff(off.astype(np.int64)))
    return state.copy(), off.copy(), _edge_multiset(seg, ht[:, 0], ht[:, 1])


def _label_sets(corpus):
    """Label sets of 1, 500 and 2 distinct labels: the corpus's own, then ids past its largest (no goal has them)."""
    uniq = np.unique(corpus.label).astype(np.uint32)
    pool = np.concatenate([uniq, np.arange(500, dtype=np.uint32) + np.uint32(int(uniq.max()) + 1)])
    return [pool[:1], pool[:500], pool[len(uniq) // 2:len(uniq) // 2 + 2]]


def _prepare(eng, corpus):
    eng.load(corpus)
    eng.mark()
    eng.simplify()


@pytest.fixture(scope="module")
def case():
    corpus, _ = synth.generate(12, target_nodes=300, p_fault=0.5, prepend_run0=True)
    f = sorted(set(int(x) for x in corpus.failed_iters()))
    its = [int(x) for x in corpus.iteration]
    assert len(f) >= 2 and 0 in its
    pairs = [(f[i % len(f)], its[(3 * i + 1) % len(its)]) for i in range(len(f) + 2)] + [(f[0], 0)]
    G = corpus.n_graphs
    ref = {}
    eng = E.Engine(0)
    try:
        _prepare(eng, corpus)
        eng.diffprov(f, DIFF_PER_RUN)
        ref["dmask"] = dict(zip(f, eng.diff_masks(len(f))))
        ref["missing"] = dict(zip(f, _rows_by_entry(eng.missing(), len(f))))
        eng.pull(2)
        ref["pull2"] = dict(zip(f, _slot_edges(len(f), *eng.pulled_all(len(f)))))
        eng.diffprov_symmetric(f)
        ref["smask"] = dict(zip(f, eng.sdiff_masks()))
        ref["surplus"] = dict(zip(f, _rows_by_entry(eng.surplus(), len(f))))
        eng.pull(3)
        ref["pull3"] = dict(zip(f, _slot_edges(len(f), *eng.pulled_all(len(f)))))
        eng.diffprov_pairs([p[0] for p in pairs], [p[1] for p in pairs])
        ref["pmask"] = dict(zip(pairs, eng.sdiff_masks()))
        ref["psurplus"] = dict(zip(pairs, _rows_by_entry(eng.surplus(), len(pairs))))
        eng.pull(3)
        ref["ppull3"] = dict(zip(pairs, _slot_edges(len(pairs), *eng.pulled_all(len(pairs)))))
        ref["hl"] = []
        for labels in _label_sets(corpus):
            eng.diffprov_host_labels(f[:1], labels)
            ref["hl"].append((eng.diff_masks(1)[0].copy(), eng.missing()[:, 1].copy()))
        eng.pull(0)
        ref["pull0"] = _all_slots(eng, G)
        eng.pull(1)
        ref["pull1"] = _all_slots(eng, G)
        ref["chains"] = eng.chains()
        ref["staged"] = _staged(eng, G)
    finally:
        eng.close()
    # the reference is not empty: some run lacks something of run 0, and some pair has a surplus (this corpus's
    # failed runs have none over run 0: the symmetric masks are all zero, the pairs' are not)
    assert any(m.any() for m in ref["dmask"].values())
    assert any(m.any() for m in ref["pmask"].values()) or any(m.any() for m in ref["smask"].values())
    assert len(ref["pull0"]) and len(ref["chains"])
    return corpus, f, pairs, ref


def _check_diff(eng, what, ents, ref):
    n = len(ents)
    masks = eng.diff_masks(n)
    want = np.stack([ref["dmask"][e] for e in ents])
    assert np.array_equal(masks, want), f"{what}: D masks differ"
    assert np.array_equal(eng.missing(), _rows_of([ref["missing"][e] for e in ents])), f"{what}: missing rows differ"
    class_of, classes = eng.diff_classes()
    w_of, w_classes, w_support = _classes(want)
    assert np.array_equal(class_of, w_of) and np.array_equal(classes, w_classes), f"{what}: classes differ"
    assert np.array_equal(eng.diff_support(), w_support), f"{what}: support differs"
    eng.pull(2)
    got = _slot_edges(n, *eng.pulled_all(n))
    for k, e in enumerate(ents):
        assert np.array_equal(got[k], ref["pull2"][e]), f"{what}: pull(2) slot {k} differs"


def _check_sdiff(eng, what, keys, mask, surplus, pull):
    n = len(keys)
    got = eng.sdiff_masks()
    assert len(got) == n
    for k, e in enumerate(keys):
        assert np.array_equal(got[k], mask[e]), f"{what}: S mask of entry {k} differs"
    assert np.array_equal(eng.surplus(), _rows_of([surplus[e] for e in keys])), f"{what}: surplus rows differ"
    eng.pull(3)
    got = _slot_edges(n, *eng.pulled_all(n))
    for k, e in enumerate(keys):
        assert np.array_equal(got[k], pull[e]), f"{what}: pull(3) slot {k} differs"


def _check_between(eng, what, corpus, ref):
    G = corpus.n_graphs
    eng.pull(0)
    assert np.array_equal(_all_slots(eng, G), ref["pull0"]), f"{what}: pull(0) differs"
    eng.pull(1)
    assert np.array_equal(_all_slots(eng, G), ref["pull1"]), f"{what}: pull(1) differs"
    assert np.array_equal(eng.chains(), ref["chains"]), f"{what}: chains differ"
    for got, want, name in zip(_staged(eng, G), ref["staged"], ("state", "chain_off", "chain pairs")):
        assert np.array_equal(got, want), f"{what}: staged {name} differ"


def test_buffers_grow_shrink_and_grow_again(case):
    corpus, f, pairs, ref = case
    label_sets = _label_sets(corpus)
    eng = E.Engine(0)
    try:
        _prepare(eng, corpus)
        for rnd, legacy in enumerate((0, 1, 0)):
            _check_between(eng, f"before round {rnd}", corpus, ref)
            eng.set_option("diff_legacy", legacy)
            for n in LENGTHS:
                what = f"round {rnd} (diff_legacy {legacy}), {n} entries"
                ents = [f[i % len(f)] for i in range(n)]
                eng.diffprov(ents, DIFF_PER_RUN)
                _check_diff(eng, what + ", per run", ents, ref)
                eng.diffprov_symmetric(ents)
                _check_sdiff(eng, what + ", symmetric", ents, ref["smask"], ref["surplus"], ref["pull3"])
                prs = [pairs[i % len(pairs)] for i in range(n)]
                eng.diffprov_pairs([p[0] for p in prs], [p[1] for p in prs])
                _check_sdiff(eng, what + ", pairs", prs, ref["pmask"], ref["psurplus"], ref["ppull3"])
                for labels, (mask, rules) in zip(label_sets, ref["hl"]):
                    eng.diffprov_host_labels(ents, labels)
                    hw = f"{what}, {len(labels)} host labels"
                    assert np.array_equal(eng.diff_masks(n), np.tile(mask, (n, 1))), f"{hw}: D masks differ"
                    assert np.array_equal(eng.missing(), _rows_of([rules] * n)), f"{hw}: missing rows differ"
        eng.set_option("diff_legacy", 0)
        _check_between(eng, "after the rounds", corpus, ref)
    finally:
        eng.close()
