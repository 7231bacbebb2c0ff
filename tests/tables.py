"""Corpus transforms that move a corpus' table ids around a universe of up to NEMO_MAX_TABLES ids, and the
fixtures built from them (test helpers, shared by test_tables_host.py and test_gpu_tables.py).

Both transforms return a new Corpus (dataclasses.replace) that differs from the input only in the low 24
bits of node_word, n_tables, table_pre, table_post and tables.
"""
from __future__ import annotations

import dataclasses
import functools
from typing import Dict, Mapping, Optional, Sequence, Tuple

import numpy as np

from nemo_amd.corpus import F_HOLDS, NODE_RULE, TABLE_MASK, Corpus

MAX_TABLES = 16384  # NEMO_MAX_TABLES (include/nemohip.h)


def _names(corpus: Corpus, T: int, new_of_old: Mapping[int, int]) -> list:
    names = [f"_t{i}" for i in range(T)]
    for old, new in new_of_old.items():
        if corpus.tables is not None and old < len(corpus.tables):
            names[new] = corpus.tables[old]
    return names


def _replace(corpus: Corpus, T: int, table: np.ndarray, pre: int, post: int, names: list) -> Corpus:
    word = (corpus.node_word & np.uint32(~TABLE_MASK & 0xFFFFFFFF)) | table.astype(np.uint32)
    return dataclasses.replace(corpus, node_word=np.ascontiguousarray(word, dtype=np.uint32), n_tables=T,
                               table_pre=pre, table_post=post, tables=names)


def used_tables(corpus: Corpus) -> np.ndarray:
    """The table ids some node carries, plus pre and post, sorted."""
    ids = np.unique(corpus.node_word & np.uint32(TABLE_MASK)).astype(np.int64)
    return np.unique(np.concatenate([ids, [corpus.table_pre, corpus.table_post]]))


def relabel_tables(corpus: Corpus, T: int, pi: Mapping[int, int]) -> Corpus:
    """A pure renaming: table id t becomes pi[t].  pi is injective on the ids in use (used_tables) and
    maps them below T."""
    used = used_tables(corpus)
    new = np.array([pi[int(t)] for t in used], np.int64)
    assert len(set(new.tolist())) == len(new), "pi is not injective"
    assert new.min() >= 0 and new.max() < T <= MAX_TABLES
    lut = np.zeros(int(used.max()) + 1, np.int64)
    lut[used] = new
    table = lut[(corpus.node_word & np.uint32(TABLE_MASK)).astype(np.int64)]
    m = {int(o): int(n) for o, n in zip(used, new)}
    return _replace(corpus, T, table, m[corpus.table_pre], m[corpus.table_post], _names(corpus, T, m))


def random_pi(corpus: Corpus, T: int, seed: int, lo: int = 0) -> Dict[int, int]:
    """A random injective map of the ids in use into [lo, T)."""
    used = used_tables(corpus)
    rng = np.random.default_rng(seed)
    new = lo + rng.permutation(T - lo)[:len(used)]
    return {int(o): int(n) for o, n in zip(used, new)}


def last_word_placement(T: int) -> Tuple[int, int]:
    """(pre, post) on the last bit and the first bit of the last bitset word.  Where that word has one
    bit only (T = 32 k + 1) the two would coincide, and the only id that can put the last word into
    inter is that bit (post never is in inter): pre and post then take the last two bits of the word
    before and keep_map puts a kept table on T - 1."""
    pre, post = T - 1, (T - 1) & ~31
    return (pre, post) if post != pre else (T - 2, T - 3)


def split_tables(corpus: Corpus, T: int, seed: int, keep: Mapping[int, int],
                 pre: Optional[int] = None, post: Optional[int] = None) -> Corpus:
    """Rename and split.  `pre` and `post` keep one id each (default: last_word_placement).  The tables
    in `keep` (old id -> new id) are renamed whole.  Every other table in use is split per node by a
    draw seeded with `seed`: the ids left over are cut into one contiguous block per such table and
    each of its nodes draws an id of the block.  With fewer ids left than tables, the tables share
    them round-robin (a merge: only the smallest universes).
    This changes what the analysis computes (HOLDS through Tq, every table set): the oracle on the
    result is the reference."""
    p0, p1 = last_word_placement(T)
    pre = p0 if pre is None else pre
    post = p1 if post is None else post
    fixed = {corpus.table_pre: pre, corpus.table_post: post}
    fixed.update({int(o): int(n) for o, n in keep.items()})
    assert len(set(fixed.values())) == len(fixed) and max(fixed.values()) < T <= MAX_TABLES
    used = used_tables(corpus)
    others = [int(t) for t in used if int(t) not in fixed]
    taken = np.zeros(T, bool)
    taken[list(fixed.values())] = True
    free = np.nonzero(~taken)[0]
    assert len(free) > 0 or not others
    old = (corpus.node_word & np.uint32(TABLE_MASK)).astype(np.int64)
    table = np.zeros(len(old), np.int64)
    for o, n in fixed.items():
        table[old == o] = n
    rng = np.random.default_rng(seed)
    draw = rng.random(len(old))
    nb = len(others)
    # block sizes in proportion to the tables' rule counts in the post graphs (one id at least; only
    # those rules enter the table sets), so that they spread evenly over the universe and no stretch
    # of it stays empty
    is_rule = (corpus.node_word & np.uint32(NODE_RULE)) != 0
    post_graph = np.repeat(np.arange(corpus.n_graphs) & 1, np.diff(corpus.node_off.astype(np.int64))) == 1
    cnt = np.array([int((is_rule & post_graph & (old == o)).sum()) for o in others], np.int64)
    size = np.ones(nb, np.int64)
    if len(free) >= nb and cnt.sum() > 0:
        size += (len(free) - nb) * cnt // cnt.sum()
        size[int(np.argmax(cnt))] += len(free) - int(size.sum())
    start = np.concatenate([[0], np.cumsum(size)])
    for k, o in enumerate(others):
        if len(free) >= nb:
            b0, b1 = int(start[k]), int(start[k + 1])
        else:
            b0, b1 = k % len(free), k % len(free) + 1
        # a stratified draw, rules and goals apart: node k of n (in a seeded order) draws from the k-th
        # n-th of the block, so a table with as many rules as ids reaches every id of its block
        for sel in (np.nonzero(is_rule & (old == o))[0], np.nonzero(~is_rule & (old == o))[0]):
            n = len(sel)
            if n:
                pos = (rng.permutation(n) + draw[sel]) / n
                table[sel] = free[b0 + (pos * (b1 - b0)).astype(np.int64)]
    return _replace(corpus, T, table, pre, post, _names(corpus, T, fixed))


# ---- fixtures ------------------------------------------------------------------------------------

def words_of(T: int) -> int:
    return (T + 31) // 32


@functools.lru_cache(maxsize=None)
def base_corpus() -> Corpus:
    from tools import synth
    return synth.generate(12, target_nodes=1500)[0]


@functools.lru_cache(maxsize=None)
def big_corpus() -> Corpus:
    """Graphs of NEMO_CSR_BIG = 8192 nodes and more (the multi-workgroup mark kernels)."""
    from tools import synth
    return synth.generate(6, target_nodes=14000)[0]


@functools.lru_cache(maxsize=None)
def many_runs_corpus() -> Corpus:
    """More runs than one k_reduce workgroup takes (256), at the smallest synth shape found whose second
    workgroup still gets two success runs with a proto list (257 runs leave it one; below
    target_nodes = 150 the lists are empty or hold two tables)."""
    from tools import synth
    return synth.generate(260, target_nodes=150)[0]


def inter_tables(corpus: Corpus) -> list:
    """Old ids of the untransformed corpus' inter tables (the oracle's)."""
    from oracle import oracle as O
    orc = O.analyze(corpus, corpus.success_iters(), corpus.failed_iters(), skip_pulls=True)
    return [int(t) for t in orc.inter]


def keep_map(corpus: Corpus, T: int, pre: int, post: int, n_keep: int = 6) -> Dict[int, int]:
    """Old id -> new id for the tables kept whole: the n_keep inter tables of the untransformed corpus
    with the fewest rules (the rules of the others are what fills the universe), spread over the
    universe from its top id down (so that for T > 4096 one lies at 4096 or above) and never on
    pre / post."""
    old = corpus.node_word & np.uint32(TABLE_MASK)
    is_rule = (corpus.node_word & np.uint32(NODE_RULE)) != 0
    olds = [t for t in inter_tables(corpus) if t not in (corpus.table_pre, corpus.table_post)]
    olds = sorted(olds, key=lambda t: (int((is_rule & (old == t)).sum()), t))[:n_keep]
    out, taken = {}, {pre, post}
    for k, o in enumerate(olds):
        n = (T - 1 - (k * (T - 1)) // max(len(olds), 1)) % T
        while n in taken:
            n = (n - 1) % T
        taken.add(n)
        out[o] = n
    return out


def split_fixture(corpus: Corpus, T: int, pre: Optional[int] = None, post: Optional[int] = None,
                  seed: int = 1) -> Corpus:
    p0, p1 = last_word_placement(T)
    pre = p0 if pre is None else pre
    post = p1 if post is None else post
    return split_tables(corpus, T, seed, keep_map(corpus, T, pre, post), pre=pre, post=post)


def high_relabel_fixture(corpus: Corpus, seed: int = 2) -> Tuple[Corpus, Dict[int, int]]:
    """One relabel at T = 16384 with every id in use at 8192 and above."""
    pi = random_pi(corpus, MAX_TABLES, seed, lo=8192)
    return relabel_tables(corpus, MAX_TABLES, pi), pi


def bit_ids(bits: np.ndarray) -> np.ndarray:
    """Table ids of one bitset row (or the OR of several rows)."""
    b = np.atleast_2d(bits)
    row = np.bitwise_or.reduce(b, axis=0)
    return np.nonzero(np.unpackbits(row.view(np.uint8), bitorder="little"))[0]


def unpack_bits(bits: np.ndarray, T: int) -> np.ndarray:
    """[rows, T] 0/1 matrix of [rows, W] bitset rows."""
    return np.unpackbits(np.ascontiguousarray(bits).view(np.uint8), axis=1, bitorder="little")[:, :T]


def image_bits(bits: np.ndarray, pi: Mapping[int, int], T_new: int) -> np.ndarray:
    """Bitset rows over the old ids -> the rows over the new ids that hold pi's images."""
    rows, W = bits.shape
    m = unpack_bits(bits, 32 * W)
    out = np.zeros((rows, 32 * words_of(T_new)), np.uint8)
    for o in np.nonzero(m.any(axis=0))[0]:
        out[:, pi[int(o)]] = m[:, o]
    return np.packbits(out, axis=1, bitorder="little").view(np.uint32)


def reduce_vector(corpus: Corpus, proto_bits: np.ndarray, flags: np.ndarray, success: Sequence[int]) -> np.ndarray:
    """The cross-run reduction vector (nemo_reduce_len: 2T + 4 entries) of a corpus whose runs are all
    owned, from per-run proto bits and the node flags: per-table counts over the success runs with a
    non-empty list, the first success run's list, achvdCond, whether that first list is non-empty
    (prototype.go:29-130), the holding "pre" goals of the pre graphs (extensions.go:25-49) and the
    number of runs."""
    T = corpus.n_tables
    red = np.zeros(2 * T + 4, np.uint32)
    bits = unpack_bits(proto_bits, T)
    runs = [corpus.run_index(it) for it in success]
    nonempty = [r for r in runs if bits[r].any()]
    red[:T] = bits[nonempty].sum(axis=0) if nonempty else 0
    if runs:
        red[T:2 * T] = bits[runs[0]]
        red[2 * T + 1] = int(bits[runs[0]].any())
    red[2 * T] = len(nonempty)
    pre_graph = np.repeat(np.arange(corpus.n_graphs) & 1, np.diff(corpus.node_off.astype(np.int64))) == 0
    tab = corpus.node_word & np.uint32(TABLE_MASK)
    red[2 * T + 2] = int((pre_graph & ((flags & F_HOLDS) != 0) & (tab == corpus.table_pre)).sum())
    red[2 * T + 3] = corpus.n_runs
    return red


def assert_nonvacuous(corpus: Corpus, orc, T: int, words: bool = True) -> None:
    """The conditions a split fixture must meet before a comparison at universe T means anything
    (asserted from the oracle's result)."""
    W = words_of(T)
    assert corpus.n_tables == T and orc.proto_bits.shape[1] == W
    if words:
        cover = np.bitwise_or.reduce(orc.proto_bits | orc.graph_tables, axis=0)
        assert (cover != 0).all(), f"bitset words never used: {np.nonzero(cover == 0)[0][:8].tolist()}"
    if T >= 4096:
        assert len(orc.union) >= T // 8, len(orc.union)
    assert len(orc.inter) > 0
    if T > 4096:
        assert max(int(t) for t in orc.inter) >= 4096, orc.inter
    assert int(orc.reduce[:T].max()) >= 2
    if T == MAX_TABLES:
        tab = (corpus.node_word & np.uint32(TABLE_MASK)).astype(np.int64)
        hold = (orc.flags & F_HOLDS) != 0
        assert (hold & (tab >= 8192)).any(), "no holding node with a table id of 8192 or more"
        assert (hold & ((corpus.node_word & np.uint32(NODE_RULE)) == 0)).any()


def assert_big_fixture(corpus: Corpus, orc) -> None:
    """The multi-workgroup mark kernels' fixture at T = 16384: graphs of NEMO_CSR_BIG = 8192 nodes and
    more whose Tq has bits in its first and in its last word (a holding goal of a table other than the
    graph's condition table is in Tq)."""
    assert_nonvacuous(corpus, orc, MAX_TABLES)
    size = np.diff(corpus.node_off.astype(np.int64))
    assert size.max() >= 8192
    g = np.repeat(np.arange(corpus.n_graphs), size)
    tab = (corpus.node_word & np.uint32(TABLE_MASK)).astype(np.int64)
    cond = np.where(g & 1, corpus.table_post, corpus.table_pre)
    in_tq = ((orc.flags & F_HOLDS) != 0) & (tab != cond) & (size[g] >= 8192)
    assert (in_tq & (tab < 32)).any(), "Tq word 0 unused"
    assert (in_tq & (tab >= MAX_TABLES - 32)).any(), "Tq word 511 unused"
    assert {corpus.table_pre >> 5, corpus.table_post >> 5} == {0, 511}


def assert_many_runs_fixture(corpus: Corpus, orc) -> None:
    """k_reduce across workgroups (256 runs each): both the first and the second workgroup's share of
    the runs hold success runs with a proto list, and a table that two of them list."""
    T = corpus.n_tables
    assert corpus.n_runs >= 257 and corpus.owned is None
    succ = np.array([s == "success" for s in corpus.status])
    bits = unpack_bits(orc.proto_bits, T)
    listed = succ & bits.any(axis=1)
    for share in (slice(0, 256), slice(256, None)):
        assert listed[share].any()
        assert int(bits[share][listed[share]].sum(axis=0).max()) >= 2
    assert len(orc.inter) > 0 and int(orc.reduce[:T].max()) >= 2
    if T > 4096:
        assert max(int(t) for t in orc.inter) >= 4096 and int(orc.reduce[4096:T].max()) >= 2
