/*
 * nemohip.h — C ABI of libnemohip, the MI355X (gfx950) engine behind Nemo's
 * provenance-graph analysis.
 *
 * This is the drop-in boundary that replaces the Bolt connection + Neo4j 3.3.3
 * engine underneath the Go `graphing` package of at15/nemo.  Every entry point
 * below names the reference method (file:line, relative to the reference root)
 * whose database round trips it replaces.  The Go side (a cgo stub, see
 * INTEGRATION.md) keeps every string: it interns table names, labels, rule
 * types and node IDs into the integer arrays below and rebuilds IDs, labels,
 * `<code>` wrappers, corrections and DOT graphs from the integer results.
 *
 * Conventions
 *   - Plain C, plain pointers and sizes; no HIP, torch or C++ types.
 *   - Every function returns NEMO_OK (0) or a NEMO_ERR_* code; the message of
 *     the last failure is nemo_last_error(ctx) (reference messages reused where
 *     the reference has one, e.g. graphing/pre-post-prov.go:209).
 *   - A context is bound to one HIP device and is not re-entrant (the
 *     reference's Bolt connections are not thread-safe either:
 *     vendor/github.com/johnnadratowski/golang-neo4j-bolt-driver/driver.go:33-36).
 *   - Graph g of a corpus is run r's antecedent (pre) graph when g == 2r and its
 *     consequent (post) graph when g == 2r+1 (the two loadProv calls of
 *     graphing/pre-post-prov.go:255,269).
 *   - Node indices in every array are local to their graph (0 .. V_g-1).
 */
#ifndef NEMOHIP_H
#define NEMOHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NEMOHIP_ABI_VERSION 1

/* ---- status codes ------------------------------------------------------ */
#define NEMO_OK            0
#define NEMO_ERR_INVALID   1  /* bad argument / malformed corpus               */
#define NEMO_ERR_HIP       2  /* HIP runtime failure                           */
#define NEMO_ERR_LOAD      3  /* loadProv validation (dangling/duplicate edge)  */
#define NEMO_ERR_CYCLE     4  /* provenance graph is not acyclic               */
#define NEMO_ERR_STATE     5  /* call out of order (e.g. simplify before load)  */
#define NEMO_ERR_LIMIT     6  /* a size limit of this build was exceeded        */
#define NEMO_ERR_NOTFOUND  7  /* unknown run iteration                          */
#define NEMO_ERR_NOGPU     8  /* no usable HIP device                           */

/* ---- packed node word (input) ------------------------------------------ *
 * bit 31      : 1 = Rule node, 0 = Goal node   (Neo4j labels :Rule / :Goal,
 *               graphing/pre-post-prov.go:28,91)
 * bits 28..30 : rule type class (goals: 0)      (Rule.type, pre-post-prov.go:91)
 * bits 0..23  : interned table id               (Goal.table / Rule.table)      */
#define NEMO_NODE_RULE    0x80000000u
#define NEMO_TYPE_SHIFT   28
#define NEMO_TYPE_MASK    0x70000000u
#define NEMO_TYPE_OTHER   0u  /* any type string other than the two below      */
#define NEMO_TYPE_NEXT    1u  /* "next"  (preprocessing.go:71, corrections.go:213) */
#define NEMO_TYPE_ASYNC   2u  /* "async" (extensions.go:64, diagrams.go:53)    */
#define NEMO_TABLE_MASK   0x00FFFFFFu
#define NEMO_MAX_TABLES   16384u /* table-id universe supported by this build: 512 words of per-run
                                    bitset; exercised up to the limit on every tier by
                                    tests/test_gpu_tables.py and tests/test_tables_host.py */

#define NEMO_WORD(is_rule, type, table) \
  (((is_rule) ? NEMO_NODE_RULE : 0u) | ((uint32_t)(type) << NEMO_TYPE_SHIFT) | ((uint32_t)(table) & NEMO_TABLE_MASK))

/* ---- per-node result flags (output) ------------------------------------ */
#define NEMO_F_HOLDS    0x01u /* condition_holds after markConditionHolds        */
#define NEMO_F_KEPT     0x02u /* node survives cleanCopyProv (run 1000+i copy)   */
#define NEMO_F_DELETED  0x04u /* removed by collapseNextChains' DETACH DELETE     */
#define NEMO_F_HEAD     0x08u /* first rule of >= 1 accepted @next chain         */
#define NEMO_F_TAIL     0x10u /* last rule of >= 1 accepted @next chain          */

/* ---- corpus (input; replaces fi.Run/ProvData, faultinjectors/data-types.go:43-98) */
typedef struct nemo_corpus {
  uint32_t n_runs;           /* runs in this corpus (or this rank's shard)          */
  uint32_t n_tables;         /* table ids are < n_tables (<= NEMO_MAX_TABLES)       */
  uint32_t table_pre;        /* interned id of table "pre"  (UINT32_MAX if absent)  */
  uint32_t table_post;       /* interned id of table "post" (UINT32_MAX if absent)  */
  const uint32_t *iteration; /* [n_runs] Run.Iteration (data-types.go:82)          */
  const uint8_t *owned;      /* [n_runs] 1 = counted in cross-run reductions;
                                NULL = all owned (replicated run 0 on a shard: 0)   */
  const uint64_t *node_off;  /* [2*n_runs+1] first node of graph g                  */
  const uint64_t *edge_off;  /* [2*n_runs+1] first edge of graph g                  */
  const uint32_t *node_word; /* [V] NEMO_WORD(...)                                  */
  const uint32_t *label;     /* [V] interned label (exact interning, never a hash)  */
  const uint32_t *id_rank;   /* [V] rank of the node's ID string inside its graph,
                                or NULL when local index order == ID string order   */
  const uint32_t *edge_src;  /* [E] local index of the DUETO edge's source          */
  const uint32_t *edge_dst;  /* [E] local index of its target                       */
} nemo_corpus;

/* one accepted @next chain (graphing/preprocessing.go:108-138,249-305) */
typedef struct nemo_chain {
  uint32_t graph;  /* graph index g (2r or 2r+1)                                   */
  uint32_t k;      /* acceptance index: the _<k> of run_<1000+i>_<C>_<t>_collapsed_<k> */
  uint32_t head;   /* r1: local index, its table names the collapsed rule          */
  uint32_t tail;   /* rk: local index                                              */
  uint32_t len;    /* path length (relationships)                                  */
} nemo_chain;

/* one missing event of differential provenance (differential-provenance.go:82-146),
 * or one surplus event of the symmetric diff (nemo_fetch_surplus)              */
typedef struct nemo_missing {
  uint32_t entry;  /* diff entry (index into the failed-run list)                  */
  uint32_t rule;   /* local index of the rule in run 0's post graph; for a surplus
                      event: in the entry's own failed run's post graph (after
                      nemo_diffprov_pairs: in the entry's base run's post graph)   */
} nemo_missing;

/* ---- run sharding --------------------------------------------
 * part_of_run[r] in [0, n_parts) for every run of the corpus: longest-first
 * (LPT) by the run's nodes + edges (pre + post graphs), each run to the least
 * loaded part, ties by index.  Host only; the node context (below) and the
 * one-process-per-GPU path use the same assignment.  The good run 0 is
 * replicated on every part by the caller (owned there by its own part only). */
int nemo_partition_runs(const nemo_corpus *corpus, uint32_t n_parts, uint32_t *part_of_run);

/* ---- context --------------------------------------------------------------
 * Replaces InitGraphDB / CloseDB (graphing/helpers.go:17-55, 58-86): no docker,
 * no 10 s sleep, no Bolt; binds one HIP device.                             */
typedef struct nemo_ctx nemo_ctx;
int nemo_ctx_create(int device, nemo_ctx **out);
/* Node context (SURVEY.md §8b Threading, §8e): one process drives `ndev`
 * devices (`devices` NULL = 0..ndev-1; ndev <= 0 = every visible device).  The
 * corpus given to nemo_load_corpus is run-sharded over them with
 * nemo_partition_runs (run 0 replicated), every entry point fans out over the
 * shards' streams and returns results in the corpus' global numbering
 * (graphs, runs, diff entries, pull slots), and the two cross-run exchanges
 * happen inside the library: the prototype vector is all-reduced with RCCL
 * (ncclSum over one communicator per device) and the reference diff mode's
 * failedRuns[0] label set is broadcast (ncclBroadcast) from its owner.  Shards
 * may share a device (a layout for testing on one GPU): they then exchange by
 * peer copies instead of RCCL.  nemo_protos_partial/_finalize take d_reduce =
 * NULL, nemo_set_stream / nemo_goal_labels / nemo_diffprov_labels are for
 * single-device contexts only.  Replaces InitGraphDB's one database for the
 * whole node (graphing/helpers.go:17-55; main.go:95 constructs one Neo4J). */
int nemo_ctx_create_node(int ndev, const int *devices, nemo_ctx **out);
/* Devices of a context (its shards' devices for a node context); returns the count. */
int nemo_node_devices(const nemo_ctx *ctx, int *devices, int cap);
void nemo_ctx_destroy(nemo_ctx *ctx);
const char *nemo_last_error(const nemo_ctx *ctx);
int nemo_abi_version(void);
/* Launch every kernel on `stream` (a hipStream_t, NULL = the context's own). */
int nemo_set_stream(nemo_ctx *ctx, void *stream);
/* Tuning / test knobs (value -1 restores the default).  None changes a result;
 * each selects which kernel tier runs, so the parity tests force every tier.
 *   "chains_lds_max"    largest chain subgraph H* (nodes) the @next-chain LDS
 *                       tiers take; larger graphs go to the component tier
 *   "chains_comp_max"   largest component the component tier runs in LDS on one
 *                       wave (larger ones take its workgroup-wide global path)
 *   "chains_glob_min_v" graphs with at least this many nodes take the deep
 *                       k_chains_glob tier (default 65536; next nemo_load_corpus)
 *   "build_lds_max"     largest graph (nodes) whose CSR + Kahn levels k_build
 *                       builds in LDS (also capped at 16384 nodes / 8192 edges
 *                       and by the corpus-sized LDS budget); from the next
 *                       nemo_load_corpus / nemo_rebuild
 *   "graph_lds_max"     largest graph (nodes) of the LDS graph tier of k_marksimp,
 *                       k_proto_lds, k_diff_lds and k_pull_lds (0 = off)
 *   "global_block"      workgroup size of the global-memory tiers: 256 or 1024
 *                       (default: 1024 when >= 1/8 of the graphs have >= 64k nodes)
 *   "stage_blocks"      nemo_stage_simplified's bulk copies: 0 = runtime copies
 *                       (default), else a copy kernel on this many workgroups
 *   "stage_slices"      nemo_stage_simplified packs and copies the node state in this
 *                       many slices (1..8, default 2), each slice's copy queued behind
 *                       that slice's kernel only; 1 = one kernel and one copy
 *   "stage_slice_ratio" each slice of the node state this many times the one before
 *                       (1..8, default 4; 1 = equal slices): a short first slice puts
 *                       the link to work sooner
 *   "stage_pair_slices" the same for the chain pairs, in equal slices of the pair
 *                       indices (1..8, default 1)
 *   "stage_sdma"        request nemo_stage_simplified's runtime copies as NoCU
 *                       (SDMA) copies (1) or plain D2H copies (0, default)
 *   "stage_cus"         CUs the copy stream's blit kernels may use (default 8,
 *                       0 = all); set before the first nemo_stage_simplified
 *   "stage_aux"         nemo_stage_simplified's hand-over kernels on the diff
 *                       stream behind the analysis queued so far (1, default)
 *                       or on the context's stream (0)
 *   "pull_aux"          the simplified pull on the diff stream behind the end of
 *                       nemo_simplify (1) or on the context's stream (0, default)
 *   "diff_fuse"         whole-graph diff walks finish LP rules, missing rows and
 *                       one-entry masks themselves (1, default) or hand them to
 *                       separate kernels (0; test knob)
 *   "build_marksimp"    k_build's graphs get their deferred mark + simplification
 *                       at the end of k_build, from the edges it holds (1), or
 *                       from k_marksimp in nemo_simplify (0, default)
 *   "load_parts"        corpora mostly of big graphs: edge uploads in this many
 *                       parts, each part's CSR build behind its own upload
 *                       (default 4; 1 = one upload, then the build)
 *   "load_async"        1: nemo_load_corpus returns once its work is queued; its
 *                       graph checks (validations, acyclicity) are reported by
 *                       the next nemo_rebuild / nemo_mark_holds / nemo_goal_labels /
 *                       nemo_pull_edges, which then leaves no corpus loaded
 *                       (0, default: nemo_load_corpus waits and reports them).
 *                       The corpus' arrays must stay valid until that call: the
 *                       uploads from page-locked memory may still be in flight
 *   "build_relax"       k_build's Kahn levels by relaxation sweeps over the edges
 *                       in registers, peeling if they give up (1), or by peeling
 *                       (0, default)
 *   "topo_ell"          deep graphs' Kahn levels by the edge-parallel k_topo_ell
 *                       (1) or one workgroup per graph, k_topo_deep (0, default)
 *   "class_hash_bits"   nemo_diff_classes buckets the D masks by the low k bits of
 *                       their 128-bit hash, k in 0..128 (default 128); every
 *                       bucket is verified by exact row comparisons, so fewer bits
 *                       only force collisions and more comparison rounds (test
 *                       knob; at 0 every mask collides with every other)
 *   "graph_dedup"       1 (default): nemo_load_corpus groups the graphs of identical
 *                       content (sizes, pre / post, node words, labels, ID ranks,
 *                       edges in stored order); k_build, k_marksimp and the first
 *                       chain tier then run on one graph per class and a streaming
 *                       copy fills the others' slices, so every array holds what
 *                       it held without the option.  Graphs of 8192 nodes or more
 *                       and the deep graphs are kept apart.  0: every graph runs
 *                       (no classes are made by a load under 0; set it before the
 *                       load).  Not applied under "load_async" 1 or to a corpus
 *                       uploaded in parts
 *   "dedup_hash_bits"   that grouping buckets by the low k bits of a 128-bit
 *                       content hash, k in 0..128 (default 128; takes effect at the
 *                       next load); every bucket is confirmed by exact comparisons
 *                       (test knob, as "class_hash_bits")
 *   "proto_dedup"       1 (default, also -1): while "graph_dedup" has duplicates, the
 *                       runs whose pre graphs are of one class and whose post graphs
 *                       are form a run class; the prototype kernel of the LDS tier
 *                       runs on the lowest run of each class and its rows (prototype
 *                       bits, graph tables, gate) are copied to the others.  0: it
 *                       runs every run
 *   "pull_dedup"        1 (default, also -1): while "graph_dedup" has duplicates,
 *                       nemo_pull_edges 0 / 1 compacts one graph per class and the
 *                       other graphs' slots share its region (same edges in the
 *                       same order; see nemo_fetch_pulled_all).  0: every graph is
 *                       compacted into a region of its own
 *   "replicate_lazy"    1 (default, also -1): under "graph_dedup", "proto_dedup" and
 *                       "pull_dedup", once a pass has shown every global tier
 *                       empty, a load / rebuild copies only the per-graph scalars
 *                       to the duplicates; their CSR, Kahn and e2 slices follow
 *                       before the first call that may read them (any fetch of
 *                       graph data, the symmetric / pair diff, nearest runs,
 *                       failure classes, an option change).  0: right behind the
 *                       build, every time
 *   "pair_hash_lds_max" largest label table (slots) nemo_diffprov_pairs builds in
 *                       LDS; larger ones are built in place with global atomics
 *                       (default and upper bound 16384; 0 = every table in place)
 *   "near_bits_lds_max" largest bit row (bytes) nemo_nearest_runs builds in LDS;
 *                       longer rows are zeroed in place and filled with global
 *                       atomics (default and upper bound 65536; 0 = every row in place)
 *   "near_ksplit"       ranges the row words (K) of nemo_nearest_runs' intersection
 *                       counts are split into, each range a workgroup per tile, summed
 *                       with integer atomics (0, default: one range unless the tiles
 *                       alone leave the device under two workgroups per CU; at most
 *                       1024 and the K-slabs of a row)
 *   "knock_lds_max"     largest LDS image (bytes) of a graph the knock-out sweep runs
 *                       in LDS; graphs past it, and graphs of 65536 nodes or more, run
 *                       the sweep over the CSR in device memory (default and upper
 *                       bound 81920; 0 = every graph in device memory); nemo_min_cuts,
 *                       nemo_knockout_labels, nemo_min_label_cuts and
 *                       nemo_min_group_cuts take their tier from the same option
 *   "cut_grid"          most workgroups of nemo_min_cuts' persistent sweeps (0, default:
 *                       as many as are resident on the device, at most one per chunk
 *                       of 64 hypotheses); a test knob: 1 makes one workgroup take
 *                       every chunk
 *   "kl_grid"           most workgroups of nemo_knockout_labels' persistent sweeps (0,
 *                       default: as many as are resident on the device); the twin of
 *                       "cut_grid", a test knob: 1 makes one workgroup walk every
 *                       listed graph in turn, small values split a graph's chunks
 *                       into few ranges; the tier is "knock_lds_max"'s;
 *                       nemo_min_label_cuts' and nemo_min_group_cuts' sweeps take the
 *                       same cap
 *                       (the lineage cut and lineage repair searches' sweeps as well)
 *   "kl_hitlist"        1 (default, also -1): the LDS-tier sweep of nemo_knockout_labels
 *                       lists, once per graph, the nodes whose label some set names,
 *                       and a chunk of 64 sets probes its table with those alone.  0:
 *                       no list, every chunk probes with every node's label (same
 *                       results; the form the list was measured against, tested)
 *   "wit_lds_max"       largest LDS image (bytes) of a graph nemo_witness_sets and
 *                       nemo_witness_labels run in LDS; the image is the knock-out
 *                       sweep's plus a second u64 word per node, so a graph of the
 *                       same shape needs 8 V bytes more than under "knock_lds_max";
 *                       graphs past it, and graphs of 65536 nodes or more, run over
 *                       the CSR in device memory (default and upper bound 159744,
 *                       one workgroup per CU past 81920, the fastest of the three
 *                       points measured at the C3 shape; 0 = every graph in
 *                       device memory; -1 = the default); takes effect at the
 *                       next witness call; the grid cap is "kl_grid"'s;
 *                       nemo_lineage_cuts takes its tier from the same option
 *                       (the lineage repair calls too: their image is 8 V bytes larger)
 *   "lineage_children_max"  most children one level of nemo_lineage_cuts may emit,
 *                       counted before duplicates are removed (default 2^24 =
 *                       16777216: 16 bytes per child gives 256 MiB, a memory bound,
 *                       not a tuned number; at least 64, at most 2^31; -1 = the
 *                       default); a level past it fails the call with
 *                       NEMO_ERR_LIMIT
 *                       (the lineage repair calls' levels are held to the same limit) */
int nemo_set_option(nemo_ctx *ctx, const char *name, int64_t value);
/* Record a hipEvent pair around every launch (per-kernel timing, see nemo_timings). */
int nemo_set_timing(nemo_ctx *ctx, int enable);
/* Restrict the timing to these groups (comma-separated names as nemo_timings
 * reports them, e.g. "k_build"); NULL or "" = every group.  An event pair
 * costs the stream a few microseconds: a benchmark times only the kernel it
 * prices against the roofline.                                              */
int nemo_set_timing_groups(nemo_ctx *ctx, const char *groups);

/* ---- load (loadProv, graphing/pre-post-prov.go:25-213) ---------------------
 * Copies the corpus to HBM, builds forward + reverse CSR and the topological
 * levels of every graph on the device, and validates like loadProv does:
 * dangling or duplicate DUETO edges and goal->goal / rule->rule edges fail with
 * the reference's "inserted number of edges" message (pre-post-prov.go:208-210).
 * Cycles fail with NEMO_ERR_CYCLE.  Host arrays may be freed on return.     */
int nemo_load_corpus(nemo_ctx *ctx, const nemo_corpus *corpus);
/* Page-lock (hipHostRegister) / release a caller-owned host buffer, so that
 * nemo_load_corpus uploads it by DMA instead of through the runtime's staging
 * copies: for corpora loaded more than once (a batch of a pass over a corpus
 * larger than HBM).  No reference counterpart (Neo4j reads its own store).  */
int nemo_host_register(const void *ptr, uint64_t bytes);
int nemo_host_unregister(const void *ptr);
/* Re-run the device part of the load (CSR + topo) on the resident corpus.    */
int nemo_rebuild(nemo_ctx *ctx);
uint64_t nemo_num_nodes(const nemo_ctx *ctx);
uint64_t nemo_num_edges(const nemo_ctx *ctx);

/* ---- markConditionHolds for every graph (pre-post-prov.go:218-244,247-285) */
int nemo_mark_holds(nemo_ctx *ctx);

/* ---- SimplifyProv for every run (preprocessing.go:351-387):
 * cleanCopyProv (:13-63) then collapseNextChains (:66-348), pre and post.   */
int nemo_simplify(nemo_ctx *ctx);

/* ---- prototypes (prototype.go:9-256) --------------------------------------
 * Cross-run reduction vector (u32, device memory, nemo_reduce_len entries):
 *   [0, T)        cnt[t]   = #owned success runs whose proto list holds t
 *   [T, 2T)       first[t] = table bits of the first success run's list
 *   2T            achvdCond (prototype.go:70)
 *   2T+1          first list non-empty (prototype.go:80-103)
 *   2T+2          #holding "pre" goals in raw pre graphs (extensions.go:25-49)
 *   2T+3          #owned runs
 * Every entry is a sum, so a multi-GPU job all-reduces it with ncclSum.     */
size_t nemo_reduce_len(const nemo_ctx *ctx);
int nemo_protos_partial(nemo_ctx *ctx, const uint32_t *success_iters, size_t n_success,
                        uint32_t *d_reduce /* device, nemo_reduce_len() u32; NULL = the context's own */);
/* Optional: queue the (reduced) vector's copy to pinned host memory on the
 * context's stream now, behind the caller's all-reduce, so that
 * nemo_protos_finalize on the same d_reduce only waits for it (no round trip
 * of its own).  A node context reduces inside finalize: a no-op there.      */
int nemo_protos_stage(nemo_ctx *ctx, const uint32_t *d_reduce);
/* Interprets a (reduced) vector (d_reduce NULL = the context's own): inter/union
 * table ids, ascending, "post" excluded (prototype.go:106,120).  Returns counts through n_inter/n_union;
 * `inter`/`uni` may be NULL to query sizes (capacity n_tables is enough).   */
int nemo_protos_finalize(nemo_ctx *ctx, const uint32_t *d_reduce, uint32_t *achieved,
                         uint32_t *inter, uint32_t *n_inter, uint32_t *uni, uint32_t *n_union,
                         uint64_t *pre_holds_count, uint32_t *n_runs_total);
/* Host-only interpretation of a (reduced) vector held in HOST memory; needs no
 * context or device (nemo_protos_finalize = D2H + this). */
int nemo_reduce_interpret(const uint32_t *h_reduce, uint32_t n_tables, uint32_t table_post, uint32_t *achieved,
                          uint32_t *inter, uint32_t *n_inter, uint32_t *uni, uint32_t *n_union);
/* The context's own (for a node context: the all-reduced) vector to host
 * memory, nemo_reduce_len() u32: for callers that reduce across processes
 * themselves from host memory.                                              */
int nemo_fetch_reduce(nemo_ctx *ctx, uint32_t *out, uint64_t cap);
/* Single-process convenience: partial + finalize with the context's own buffer. */
int nemo_prototypes(nemo_ctx *ctx, const uint32_t *success_iters, size_t n_success,
                    uint32_t *achieved, uint32_t *inter, uint32_t *n_inter,
                    uint32_t *uni, uint32_t *n_union);
/* missingFrom (prototype.go:141-206): entries of `proto` (table ids, in the
 * caller's order) absent from the table set of the failed run's simplified
 * post graph (run 1000+f).  `out` receives them in proto order.            */
int nemo_missing_from(nemo_ctx *ctx, uint32_t failed_iter, const uint32_t *proto, uint32_t n_proto,
                      uint32_t *out, uint32_t *n_out);

/* ---- differential provenance (differential-provenance.go:18-243) ----------
 * Good = run-0 post goals whose label is absent from the post goals of the
 * label source run; D = Fwd*(Good) ∩ Bwd*(Good); missing events = deepest
 * leaf-parent rules of D.  mode NEMO_DIFF_REFERENCE reproduces the reference's
 * in-place ###RUN### substitution (:43): every entry uses failed_iters[0] as
 * label source.  NEMO_DIFF_PER_RUN uses each entry's own failed run.        */
#define NEMO_DIFF_REFERENCE 0
#define NEMO_DIFF_PER_RUN   1
int nemo_diffprov(nemo_ctx *ctx, const uint32_t *failed_iters, size_t n_failed, int mode);
/* The run-sharded form of the reference mode (differential-provenance.go:22-43:
 * every entry uses failedRuns[0]'s labels, but that run lives on one shard).
 * nemo_goal_labels writes the goal labels of run `iteration`'s pre (cond 0) or
 * post (cond 1) graph into device memory as [n, label...] (cap >= the graph's
 * nodes + 1), enqueued on the context's stream without a host round trip; the
 * owner's buffer is then broadcast (RCCL) and every shard runs
 * nemo_diffprov_labels with it: failGoals = that set for every entry. */
int nemo_goal_labels(nemo_ctx *ctx, uint32_t iteration, int cond, uint32_t *d_out, uint64_t cap);
int nemo_diffprov_labels(nemo_ctx *ctx, const uint32_t *failed_iters, size_t n_failed, const uint32_t *d_labels,
                         uint64_t labels_cap);
/* The same with the label set in host memory (the caller interned it, e.g. a
 * chunked pipeline whose failedRuns[0] was analysed with an earlier chunk). */
int nemo_diffprov_host_labels(nemo_ctx *ctx, const uint32_t *failed_iters, size_t n_failed, const uint32_t *labels,
                              uint64_t n_labels);
/* D node mask over run 0's post graph for entry e (1 byte per node).        */
int nemo_fetch_diff_mask(nemo_ctx *ctx, uint32_t entry, uint8_t *out, uint64_t cap);
/* D masks of every entry, entry-major (n_entries * V0 bytes).               */
int nemo_fetch_diff_masks(nemo_ctx *ctx, uint8_t *out, uint64_t cap);
/* Zero-copy view of every entry's D mask (n_entries x v0 bytes) in library-
 * owned pinned memory, valid until the next nemo_diffprov.                  */
int nemo_diff_masks_view(nemo_ctx *ctx, const uint8_t **masks, uint64_t *n_entries, uint64_t *v0);
/* Missing rules of every entry; goals = all D-children of each rule.        */
int nemo_fetch_missing(nemo_ctx *ctx, nemo_missing *out, uint64_t cap, uint64_t *n_out);

/* ---- failure classes: diff entries grouped by identical D mask ---------------
 * Replaces nothing in the reference: the calls summarise the output of
 * CreateNaiveDiffProv (differential-provenance.go:18-146), which returns one
 * diff graph and one set of missing events per failed run and leaves "which
 * runs failed the same way" to the reader.  Two entries are in one class iff
 * their D masks have the same membership at every node of run 0's post graph
 * (so they also have the same missing events); an all-zero mask is a class like
 * any other.  Classes are numbered by their smallest entry, ascending; that
 * entry is the class's representative.  In NEMO_DIFF_REFERENCE and the label
 * modes every entry shares one label source: one class of n_entries.           */
typedef struct nemo_diff_class {
  uint32_t rep;    /* representative: the class's smallest diff entry               */
  uint32_t size;   /* member entries (duplicated failed_iters each count)           */
  uint32_t nodes;  /* |D|: nodes of run 0's post graph in the class's mask          */
} nemo_diff_class;
/* Classifies the results of the last nemo_diffprov / _labels / _host_labels call
 * on the device (the masks are not copied to the host for it).  NEMO_ERR_STATE
 * when no corpus is loaded or no diffprov ran since the load; zero entries give
 * zero classes.  Blocks until the classes are known.  A later nemo_diffprov*,
 * nemo_load_corpus or nemo_rebuild invalidates the result (the fetches below
 * then return NEMO_ERR_STATE until the next nemo_diff_classes);
 * nemo_diffprov_symmetric leaves it valid, as it leaves the diff itself.       */
int nemo_diff_classes(nemo_ctx *ctx);
/* class_of[e] = class of entry e (may be NULL); classes[k] for every class k.
 * classes == NULL queries *n_classes.                                          */
int nemo_fetch_diff_classes(nemo_ctx *ctx, uint32_t *class_of /* [n_entries], may be NULL */,
                            nemo_diff_class *classes, uint64_t cap, uint64_t *n_classes);
/* Support of every node of run 0's post graph: out[v] = entries whose D holds v
 * (duplicated entries each count); cap >= V0.                                  */
int nemo_fetch_diff_support(nemo_ctx *ctx, uint32_t *out, uint64_t cap /* >= V0 */);

/* ---- symmetric differential provenance ("bad - good") ----------------------
 * The half the reference's API names and never built: `symmetric` of
 * CreateNaiveDiffProv (differential-provenance.go:18; main.go:160 passes
 * false).  It is the export query (:22-28) and the leaf query (:82-98) with the
 * two runs' roles exchanged: for entry e with failed run f and gf = f's raw post
 * graph, Bad = goals of gf whose label is no post-goal label of run 0;
 * S = Fwd*(Bad) ∩ Bwd*(Bad) over gf; surplus events = the S rules with an
 * S-goal child that has no S child, at maximal depth + 1 inside S.  Every entry
 * uses its own failed run against run 0 (no reference mode: :43's in-place
 * substitution has no counterpart here).  failed_iters may name any loaded
 * run, run 0 (whose S is empty) and duplicates included.  With n_failed == 0 or
 * no run of iteration 0 the call yields zero entries, as nemo_diffprov does.
 * The state is the call's own: results of a previous nemo_diffprov stay
 * valid, and the reverse.  Single-device contexts only (a node context
 * returns NEMO_ERR_STATE).                                                   */
int nemo_diffprov_symmetric(nemo_ctx *ctx, const uint32_t *failed_iters, size_t n_failed);
/* S masks of every entry (the export of :22-28, roles exchanged), ragged: entry
 * e's mask is out[off[e] .. off[e+1]), one byte per node of its own failed
 * post graph.  off has n_entries + 1 elements (may be NULL); out == NULL
 * queries *n_used (= off[n_entries]).                                        */
int nemo_fetch_sdiff_masks(nemo_ctx *ctx, uint64_t *off /* n+1 */, uint8_t *out, uint64_t cap, uint64_t *n_used);
/* Surplus events of every entry (the leaf query of :82-98, roles exchanged),
 * ordered by (entry, rule); `rule` is local to the entry's failed post graph,
 * goals = all S-children of each rule.  out == NULL queries *n_out.         */
int nemo_fetch_surplus(nemo_ctx *ctx, nemo_missing *out, uint64_t cap, uint64_t *n_out);

/* ---- differential provenance between arbitrary pairs of runs ------------------
 * The same two queries (the export of differential-provenance.go:22-28 and the
 * leaf query of :82-98) between any two loaded runs: entry e is the pair
 * (base_iters[e], other_iters[e]); with gb = the base run's raw post graph,
 * Bad = goals of gb whose label is no post-goal label of the other run,
 * S = Fwd*(Bad) ∩ Bwd*(Bad) over gb, surplus events as nemo_diffprov_symmetric
 * defines them, on gb.  So (f, iteration 0) is nemo_diffprov_symmetric's entry
 * for f, (iteration 0, f) is nemo_diffprov's per-run entry for f (S = its D
 * mask, surplus rules = its missing rules), and (x, x) has an empty S.  The
 * reference has no counterpart: it compares with run 0 only.
 * Needs nemo_load_corpus and nemo_mark_holds, as the symmetric call does.  Both
 * lists may name any loaded run, duplicates included (duplicate pairs give
 * identical results); run 0 need not be loaded; an iteration that is not
 * loaded is NEMO_ERR_NOTFOUND; n == 0 gives zero entries and NEMO_OK.
 * The call writes the symmetric diff's state, so its results come through the
 * same accessors with slot = entry: nemo_fetch_sdiff_masks (ragged, one byte
 * per node of the entry's base post graph), nemo_fetch_surplus (`rule` is
 * local to the entry's base run's post graph), nemo_pull_edges(ctx, 3) with
 * nemo_fetch_pulled(_all) (gb's edges induced on S, in gb's row order).  A later
 * nemo_diffprov_symmetric or nemo_diffprov_pairs replaces those results;
 * results of nemo_diffprov stay valid, and the reverse.  The label tables of
 * the distinct `other` runs are built on the device, on the context's stream
 * ahead of the walk (an entry against iteration 0 uses the table of the load).
 * Single-device contexts only (a node context returns NEMO_ERR_STATE).       */
int nemo_diffprov_pairs(nemo_ctx *ctx, const uint32_t *base_iters, const uint32_t *other_iters, size_t n);

/* ---- nearest runs by post-goal label sets -------------------------------------
 * Which run to give nemo_diffprov_pairs as `other`: for every query run, the
 * candidate run whose derived post goals are closest to its own.  The reference
 * has no counterpart (it compares with run 0 only); the call steers the pair
 * diff as nemo_diff_classes summarises the diff.
 * L(r) = the distinct labels of the goal nodes of run r's raw post graph (the
 * key set of the pair diff's label table of r).  For a query q and a candidate c
 *   only_query = |L(q) \ L(c)|,  only_cand = |L(c) \ L(q)|,
 *   dist = only_query + only_cand = |L(q)| + |L(c)| - 2 |L(q) & L(c)|.
 * The row of query position i names the candidate position j of least dist;
 * ties go to the smallest j; candidates whose iteration equals the query's
 * iteration are skipped (a run is not its own neighbour).  If no candidate is
 * left (n_c == 0, or every candidate is the query itself), cand and the three
 * counts are UINT32_MAX.  only_query == 0 exactly when the S mask of the pair
 * (q, c) of nemo_diffprov_pairs is all zero: Bad(q, c) is the goals of q whose
 * label is missing from c.
 * Needs nemo_load_corpus only.  Both lists may name any loaded run, duplicates
 * included; run 0 need not be loaded; an iteration that is not loaded is
 * NEMO_ERR_NOTFOUND; n_q == 0 gives zero rows and NEMO_OK.  n_q * n_c > 2^30, or
 * a bit matrix (distinct runs of the call x ceil((largest goal label + 1) / 64)
 * words, rows rounded up to 16 bytes) past 2^36 bytes, is NEMO_ERR_LIMIT: tile
 * the queries (labels are interned ids; the second limit is what sparse ids
 * meet).  Single-device contexts only (a node context returns NEMO_ERR_STATE).
 * Everything runs on the device on the context's stream; the call blocks until
 * the rows are on the host, as nemo_diff_classes does.  The state is the call's
 * own: valid until the next nemo_nearest_runs or nemo_load_corpus (the fetches
 * return NEMO_ERR_STATE otherwise), independent of every diff state in both
 * directions.                                                                 */
typedef struct nemo_nearest {
  uint32_t cand;       /* position in cand_iters (UINT32_MAX: no candidate left)     */
  uint32_t dist;       /* only_query + only_cand                                     */
  uint32_t only_query; /* labels of the query's post goals the candidate lacks       */
  uint32_t only_cand;  /* labels of the candidate's post goals the query lacks       */
} nemo_nearest;
int nemo_nearest_runs(nemo_ctx *ctx, const uint32_t *query_iters, size_t n_q, const uint32_t *cand_iters, size_t n_c);
/* out[i] for every query position i; out == NULL queries *n_out (= n_q).       */
int nemo_fetch_nearest(nemo_ctx *ctx, nemo_nearest *out, uint64_t cap, uint64_t *n_out);
/* Rows [q_lo, q_hi) of the n_q x n_c distance matrix (dist of every pair of list
 * positions, self-pairs with their true distance 0), copied from the device:
 * for callers that want the k nearest; cap >= (q_hi - q_lo) * n_c.             */
int nemo_fetch_label_distances(nemo_ctx *ctx, uint32_t q_lo, uint32_t q_hi, uint32_t *out, uint64_t cap);

/* ---- knock-out analysis: which events a run's outcome depends on ---------------
 * A provenance graph is an AND/OR circuit: a goal holds if any of its rule
 * firings holds, a rule firing holds if all of its premises hold.  The calls
 * evaluate that circuit under many hypotheses at once; they replace the Cypher
 * path query a Neo4j user could type ("is there still a derivation of post if
 * this message is lost?") and restate on the device what Molly's own search
 * walks.  The reference has no counterpart in its graphing package.
 * The subject is a raw loaded graph g: run r's pre graph (cond 0) or post graph
 * (cond 1), as loaded and not simplified; nemo_mark_holds is not needed.  A
 * hypothesis h is a set F_h of nodes of g, removed by assumption.  dead_h(v) is
 * defined bottom-up along the DUETO edges, sinks first:
 *   - v in F_h: dead;
 *   - v a rule (NEMO_NODE_RULE): dead iff at least one child is dead; a rule
 *     without children is alive unless it is in F_h;
 *   - v a goal with at least one child: dead iff all its children are dead;
 *   - v a goal without children (a base fact): alive unless it is in F_h.
 * The definition goes by the node's own kind only: it does not assume that goals
 * and rules alternate.  Roots are the nodes of in-degree 0 (Kahn level 0).  For
 * every hypothesis the call reports n_dead (dead nodes, F_h included),
 * roots_dead and n_roots; the outcome is lost under h iff roots_dead == n_roots
 * and n_roots > 0, and how to read that stays with the caller.  The empty set is
 * a legal hypothesis (nothing is dead), a node named twice in a set counts once,
 * a node index >= V_g is NEMO_ERR_INVALID.
 * nemo_knockout_leaves makes one hypothesis per sink goal (a goal without
 * children) of each listed run's graph, in node-index order within a graph,
 * graphs in list order: hypothesis k of a graph knocks out its k-th sink goal.
 * nemo_knockout_sets takes explicit hypotheses on one graph: set s is
 * set_nodes[set_off[s] .. set_off[s+1]); set_off must not decrease
 * (NEMO_ERR_INVALID otherwise).
 * n == 0 or n_sets == 0 gives zero hypotheses and NEMO_OK; a graph with no sink
 * goal contributes zero hypotheses; an iteration that is not loaded is
 * NEMO_ERR_NOTFOUND; duplicate iterations give identical rows.  More than
 * 2^32 - 2 hypotheses, dead words kept in device memory past 2^36 bytes (8 V_g
 * bytes per chunk of 64 hypotheses: every chunk with NEMO_KO_MASKS, else only
 * the chunks of graphs past the LDS tier), or sets naming more than 2^32 - 1
 * nodes in all, are NEMO_ERR_LIMIT: tile the call.  Single-device contexts
 * only (a node context returns NEMO_ERR_STATE).  Everything runs on the device
 * on the context's stream; the calls block until the rows are on the host, as
 * nemo_diff_classes does.  The results are the call's own state: valid until
 * the next knock-out call or nemo_load_corpus (the fetches return
 * NEMO_ERR_STATE otherwise), independent of the diff, symmetric diff, nearest
 * and class state in both directions.                                          */
typedef struct nemo_knock {
  uint32_t graph;      /* 2r + cond                                                   */
  uint32_t node;       /* leaves mode: the leaf knocked out (local index); sets mode: UINT32_MAX */
  uint32_t n_dead;     /* dead nodes, F_h included                                    */
  uint32_t roots_dead; /* dead nodes of in-degree 0                                   */
  uint32_t n_roots;    /* nodes of in-degree 0                                        */
} nemo_knock;
#define NEMO_KO_MASKS 1u /* keep the dead masks for nemo_fetch_knockout_mask          */
int nemo_knockout_leaves(nemo_ctx *ctx, const uint32_t *iters, size_t n, int cond, uint32_t flags);
int nemo_knockout_sets(nemo_ctx *ctx, uint32_t iteration, int cond, const uint64_t *set_off, const uint32_t *set_nodes,
                       size_t n_sets, uint32_t flags);
/* out[h] for every hypothesis h; out == NULL queries *n_out.                    */
int nemo_fetch_knockout(nemo_ctx *ctx, nemo_knock *out, uint64_t cap, uint64_t *n_out);
/* Per listed graph (leaves mode: n entries) or the one graph (sets mode: one
 * entry): its first hypothesis and how many it has; cap >= that many entries.  */
int nemo_fetch_knockout_ranges(nemo_ctx *ctx, uint64_t *first, uint32_t *count, uint64_t cap);
/* One byte per node of hypothesis hyp's graph, 1 = dead; cap >= V_g.  Needs a
 * call with NEMO_KO_MASKS (NEMO_ERR_STATE otherwise).                           */
int nemo_fetch_knockout_mask(nemo_ctx *ctx, uint64_t hyp, uint8_t *out, uint64_t cap);

/* ---- minimal cut sets: the smallest fault sets that defeat a run's outcome ------
 * The subject (a raw loaded graph g = 2r + cond), dead_F(v), the roots and "the
 * outcome is lost under F" (roots_dead == n_roots > 0) are the knock-out
 * definitions above.  nemo_min_cuts searches where nemo_knockout_sets evaluates:
 * the caller names candidates, the device makes the hypotheses itself.
 * Candidates: cand[0 .. n_cand) are graph-local node indices of any kind (goals,
 * rules, inner nodes); cand == NULL means every sink goal of the graph in
 * node-index order (the list nemo_knockout_leaves makes).  A node >= V_g, or a
 * node listed twice, is NEMO_ERR_INVALID, checked on the host before anything is
 * uploaded.
 * A cut is a set F of candidates under which the outcome is lost; it is minimal
 * if no proper subset of it is a cut.  dead is monotone in F, so every superset
 * of a cut is a cut.  The call returns all minimal cuts of size <= max_size;
 * max_size must be 1, 2 or 3 and flags 0 (NEMO_ERR_INVALID otherwise).
 * Rounds: round 1 evaluates the K singletons; the candidates that are no cut by
 * themselves form the live list, in candidate order, K1 entries.  Round 2
 * evaluates all C(K1,2) pairs of live positions; every lost pair is minimal.
 * Round 3 evaluates all C(K1,3) triples; a lost triple is minimal iff none of
 * its three pairs was lost in round 2.  A round with fewer live candidates than
 * its size has zero hypotheses.
 * Hypothesis index: live positions a < b < c have the colex rank
 * C(c,3) + C(b,2) + a, pairs C(b,2) + a, singles a; hypothesis h of round s is
 * the set of rank h.  The rows are sorted by (size, rank): the order is
 * deterministic.  A row's nodes are node indices in candidate-list order,
 * unused entries UINT32_MAX.
 * More than 2^32 - 2 hypotheses in one round is NEMO_ERR_LIMIT (shorten the
 * candidate list); the call then leaves no results.  K1 is known after round 1
 * only, so a call may run round 1 before it reports the limit.  n_cand == 0
 * with a list, a graph without roots, and a graph with no cut up to max_size
 * give zero rows and NEMO_OK.  An iteration that is not loaded is
 * NEMO_ERR_NOTFOUND; a node context returns NEMO_ERR_STATE.  The call blocks
 * until the rows are on the host, as the knock-out calls do.  The results are
 * the call's own state: valid until the next nemo_min_cuts or nemo_load_corpus
 * (the fetches return NEMO_ERR_STATE otherwise), independent of the knock-out,
 * diff, symmetric diff, nearest and class state in both directions.            */
typedef struct nemo_cut {
  uint32_t size;    /* 1..3                                                          */
  uint32_t node[3]; /* nodes in candidate-list order, unused = UINT32_MAX            */
} nemo_cut;
int nemo_min_cuts(nemo_ctx *ctx, uint32_t iteration, int cond, const uint32_t *cand, size_t n_cand, uint32_t max_size,
                  uint32_t flags);
/* out[k] for every minimal cut k; out == NULL queries *n_out.                  */
int nemo_fetch_min_cuts(nemo_ctx *ctx, nemo_cut *out, uint64_t cap, uint64_t *n_out);
/* Per size s = 1..3, out[3 (s - 1) ..]: live candidates entering the round,
 * hypotheses evaluated, minimal cuts found (zeros for s > max_size).           */
int nemo_fetch_min_cut_stats(nemo_ctx *ctx, uint64_t out[9]);

/* ---- minimal repair sets: the fewest missing events that restore a run's outcome ----
 * The monotone dual of nemo_min_cuts.  The subject (a raw loaded graph
 * g = 2r + cond), dead_F(v), the roots and "the outcome is lost under F" are the
 * knock-out definitions above, unchanged.
 * A is the absent set: nodes of g assumed lost.  cand is a subset of A: the nodes
 * that may be restored.  For S within cand the outcome holds under S iff it is
 * not lost under F = A \ S.  A repair is an S under which the outcome holds; it
 * is minimal if no proper subset of it is a repair.  "Holds" is monotone in S, so
 * every superset of a repair is a repair.  The call returns all minimal repairs
 * of size <= max_size; max_size must be 1, 2 or 3 and flags 0 (NEMO_ERR_INVALID
 * otherwise, "max_size must be 1, 2 or 3").
 * Status: round 0 is one chunk of two hypotheses, S = {} and S = cand.
 *   NEMO_REPAIR_HOLDS    the outcome already holds under S = {}: the absent
 *                        events do not explain a failure.  Also a graph without
 *                        roots, and an empty A.  Zero rows.
 *   NEMO_REPAIR_BEYOND   the outcome is lost even under S = cand: some absent
 *                        node outside cand is needed by every derivation.  Zero
 *                        rows.
 *   NEMO_REPAIR_SEARCHED otherwise: the rows are all minimal repairs of size
 *                        <= max_size (there may be none that small).
 * Rounds, ranks, row order and limits are nemo_min_cuts', with "cut" read as
 * "repair": round 1 evaluates the K singletons; the candidates that are no
 * repair alone form the live list, in candidate order, K1 entries; round 2
 * evaluates all C(K1,2) pairs of live positions, and every holding pair is
 * minimal; round 3 evaluates all C(K1,3) triples, and a holding triple is
 * minimal iff none of its three pairs held.  Live positions a < b < c have the
 * colex rank C(c,3) + C(b,2) + a; the rows are sorted by (size, rank).  A row's
 * nodes are node indices in candidate-list order, unused entries UINT32_MAX.
 * More than 2^32 - 2 hypotheses in one round is NEMO_ERR_LIMIT (shorten the
 * candidate list); the call then leaves no results.  Rounds 0 and 1 run back to
 * back, so round 1 runs whatever the status is.
 * nemo_min_repair_sets: the caller names both lists, graph-local node indices of
 * any kind.  cand == NULL means cand = absent, in its order.  NEMO_ERR_INVALID,
 * checked on the host in this order before anything is uploaded, with a message
 * that names the position in its list: an absent node >= V_g; an absent node
 * listed twice; a candidate listed twice; a candidate that is not in absent.
 * cond outside 0 / 1 is NEMO_ERR_INVALID.
 * nemo_min_repairs: the pair form.  g is the base run's raw post graph, and
 * A = cand = the sink goals of g (goals without children) whose label is no goal
 * label of the other run's post graph, in node-index order: nemo_diffprov_pairs'
 * label test, restricted to sinks.  Both lists are made on the device.
 * (x, x) gives an empty A, NEMO_REPAIR_HOLDS and zero rows.  The call needs what
 * nemo_diffprov_pairs needs (NEMO_ERR_STATE before nemo_mark_holds).
 * nemo_fetch_min_repair_cands returns the candidate list the call used: rows
 * name nodes, and the stats name K.
 * An iteration that is not loaded is NEMO_ERR_NOTFOUND; a node context and a call
 * with no corpus loaded return NEMO_ERR_STATE.  The calls block until the rows are
 * on the host.  The results are the two calls' own state: valid until the next
 * of them or nemo_load_corpus (the fetches return NEMO_ERR_STATE otherwise),
 * independent of every other call's state in both directions.                    */
#define NEMO_REPAIR_HOLDS 0
#define NEMO_REPAIR_SEARCHED 1
#define NEMO_REPAIR_BEYOND 2
typedef struct nemo_repair {
  uint32_t size;    /* 1..3                                                          */
  uint32_t node[3]; /* nodes in candidate-list order, unused = UINT32_MAX            */
} nemo_repair;      /* nemo_cut's layout                                             */
int nemo_min_repair_sets(nemo_ctx *ctx, uint32_t iteration, int cond, const uint32_t *absent, size_t n_absent,
                         const uint32_t *cand, size_t n_cand, uint32_t max_size, uint32_t flags);
int nemo_min_repairs(nemo_ctx *ctx, uint32_t base_iter, uint32_t other_iter, uint32_t max_size, uint32_t flags);
/* out[k] for every minimal repair k; out == NULL queries *n_out.               */
int nemo_fetch_min_repairs(nemo_ctx *ctx, nemo_repair *out, uint64_t cap, uint64_t *n_out);
/* out[0]: the status; out[1]: |A|; out[2 + 3 (s - 1) ..] per size s = 1..3: live
 * candidates entering the round, hypotheses evaluated, minimal repairs found
 * (zeros for s > max_size, and all nine zero unless NEMO_REPAIR_SEARCHED).      */
int nemo_fetch_min_repair_stats(nemo_ctx *ctx, uint64_t out[11]);
/* out[p] = the node of candidate position p; out == NULL queries *n_out.       */
int nemo_fetch_min_repair_cands(nemo_ctx *ctx, uint32_t *out, uint64_t cap, uint64_t *n_out);

/* ---- lineage repair search: minimal repairs up to size 8 from blockers ----
 * The dual of nemo_lineage_cuts, as nemo_min_repair_sets is the dual of
 * nemo_min_cuts.  The subject (a raw loaded graph g = 2r + cond), dead_F(v), the
 * roots, "the outcome is lost under F", the absent set A, cand within A,
 * F = A \ S, "repair", "minimal" and the three statuses are nemo_min_repair_sets'
 * definitions above, unchanged.
 * Blocker.  Let F be a removed set under which the outcome is lost (every root is
 * dead and there is a root).  blame_F is defined top-down along the DUETO edges,
 * roots first, by the node's own kind only: every root is blamed; a blamed node
 * that is in F blames nothing further; a blamed rule not in F blames exactly one
 * child, its dead child of smallest node index (the forward rows ascend, so that
 * is the first dead child in row order); a blamed goal not in F blames every
 * child (it has children and all are dead, or it would be alive).
 * B_F = {v : blame_F(v)}; every blamed node is dead under F.
 * Lemma.  If F' contains the part of B_F in F, every node of B_F is dead under F' (bottom-up
 * inside B_F: a blamed node of F is in F'; a blamed rule outside F has its blamed
 * child dead; a blamed goal outside F has every child blamed and dead), hence
 * the outcome is lost under F'.  So a repair R that contains S must restore a
 * node of the blocker: it contains a node of B_{A \ S} that is in cand \ S.
 * Result, whatever the search below does: all minimal repairs of size
 * <= max_size.  The rows are sorted by (size, colex order of the candidate
 * positions, largest position first); a row's nodes ascend by candidate position,
 * unused entries UINT32_MAX.  For max_size <= 3 the rows, the status, |A| and
 * the candidate list are nemo_min_repair_sets' / nemo_min_repairs' own, in their
 * order.
 * Status: decided as round 0 of nemo_min_repair_sets decides it, from S = {} and
 * S = cand, before the levels.  NEMO_REPAIR_HOLDS and NEMO_REPAIR_BEYOND give
 * zero rows and every level stat is 0; under NEMO_REPAIR_SEARCHED level 0 reports
 * 1 set evaluated and 0 found.
 * Search (specified, so that the stats are deterministic): the hitting-set tree
 * over blockers, level by level.  Level 0 evaluates S = {}.  Level d evaluates a
 * frontier of distinct sets of d candidate positions; a set under which the
 * outcome holds is a minimal repair of size d and is not expanded.  For every
 * other set S the children are S + {e} for every candidate e in B_{A \ S} with e
 * not in S.  The frontier of level d + 1 holds the distinct children that have no
 * proper subset among the repairs of sizes <= d.  The search stops after level
 * max_size, or at an empty frontier.  Every minimal repair is reached: a minimal
 * repair R and a non-repair S inside it meet in the blocker of A \ S outside S
 * (the lemma), so some child of S lies in R; a reached repair that is not minimal
 * holds a smaller minimal repair found at an earlier level and was filtered
 * before it was evaluated.  A non-repair whose blocker holds no candidate outside
 * S has no children: nothing above it is a repair.
 * nemo_lineage_repair_sets: the caller names both lists, graph-local node indices
 * of any kind.  NEMO_ERR_INVALID, checked on the host in this order before
 * anything is uploaded, with nemo_min_repair_sets' messages under this call's
 * name: cond outside 0 / 1; max_size outside 1..8 or flags != 0 ("max_size must
 * be 1..8"); an absent node >= V_g; an absent node listed twice; a candidate
 * listed twice; a candidate that is not in absent.  cand == NULL means
 * cand = absent, in its order.  More than 65535 candidates is NEMO_ERR_LIMIT (a
 * set is kept as eight u16 candidate positions): the explicit list, the implicit
 * list, and the pair form's device-made list once its count is known.
 * nemo_lineage_repairs: the pair form.  A = cand = the sink goals of the base
 * run's raw post graph whose label is no goal label of the other run's post
 * graph, in node-index order, made on the device as nemo_min_repairs makes them;
 * it needs what that call needs (NEMO_ERR_STATE before nemo_mark_holds).
 * An empty A, a graph without roots and (x, x) give NEMO_REPAIR_HOLDS, as the
 * exhaustive calls do.  An iteration that is not loaded is NEMO_ERR_NOTFOUND; a
 * node context and a call with no corpus loaded return NEMO_ERR_STATE.
 * Limits, NEMO_ERR_LIMIT, the call then leaves no results: nemo_lineage_cuts': a
 * frontier of more than 2^32 - 2 sets; a level that emits more children (counted
 * before duplicates are removed) than the option "lineage_children_max" allows.
 * A level that counted more children than the emission buffer holds runs again,
 * once, behind a buffer of the counted size; its repairs are not appended twice.
 * The calls block until the rows are on the host.  The results are the two calls'
 * own state: valid until the next of them or nemo_load_corpus (the fetches return
 * NEMO_ERR_STATE otherwise), independent of every other call's state in both
 * directions, nemo_lineage_cuts' and the exhaustive repair calls' included.  No
 * option of its own: the tier is "wit_lds_max"'s (the image is the witness calls'
 * plus a third u64 word per node and the absent bitmap), the grid cap
 * "kl_grid"'s, the emission limit "lineage_children_max"'s.                      */
typedef struct nemo_lineage_repair {
  uint32_t size;    /* 1..8                                                          */
  uint32_t node[8]; /* nodes in candidate-list order, unused = UINT32_MAX            */
} nemo_lineage_repair; /* nemo_lineage_cut's layout                                 */
int nemo_lineage_repair_sets(nemo_ctx *ctx, uint32_t iteration, int cond, const uint32_t *absent, size_t n_absent,
                             const uint32_t *cand, size_t n_cand, uint32_t max_size, uint32_t flags);
int nemo_lineage_repairs(nemo_ctx *ctx, uint32_t base_iter, uint32_t other_iter, uint32_t max_size, uint32_t flags);
/* out[k] for every minimal repair k; out == NULL queries *n_out.               */
int nemo_fetch_lineage_repairs(nemo_ctx *ctx, nemo_lineage_repair *out, uint64_t cap, uint64_t *n_out);
/* out[0]: the status; out[1]: |A|; per size d = 0..8: out[2 + 2 d] = sets evaluated
 * at size d, out[3 + 2 d] = minimal repairs found of size d (zeros past the last
 * level the search reached, and all 18 zero unless NEMO_REPAIR_SEARCHED).       */
int nemo_fetch_lineage_repair_stats(nemo_ctx *ctx, uint64_t out[20]);
/* out[p] = the node of candidate position p; out == NULL queries *n_out.       */
int nemo_fetch_lineage_repair_cands(nemo_ctx *ctx, uint32_t *out, uint64_t cap, uint64_t *n_out);

/* ---- lineage-driven cut search: minimal cuts up to size 8 from surviving derivations ----
 * The subject (a raw loaded graph g = 2r + cond), the candidates, dead_F(v), the
 * roots, "the outcome is lost under F", "cut" and "minimal" are nemo_min_cuts'
 * definitions above, unchanged.  cand == NULL means every sink goal of the graph
 * in node-index order; candidates may be goals, rules or inner nodes.  A node
 * >= V_g, or a node listed twice, is NEMO_ERR_INVALID, checked on the host before
 * anything is uploaded.  max_size is 1..8 and flags 0; anything else is
 * NEMO_ERR_INVALID ("max_size must be 1..8").  More than 65535 candidates is
 * NEMO_ERR_LIMIT: a set is kept as eight u16 candidate positions.
 * Result, whatever the search below does: all minimal cuts of size <= max_size
 * among the candidates.  The rows are sorted by (size, colex order of the
 * candidate positions): of two sets of one size the colex order compares the
 * largest position first, then the next largest, and so on.  For size <= 3 this
 * is nemo_min_cuts' row order (its live list keeps candidate order, so colex
 * over live positions and colex over candidate positions agree).  A row's nodes
 * ascend by candidate position, unused entries UINT32_MAX.
 * Search (specified, so that the stats are deterministic): the hitting-set tree
 * over surviving derivations, level by level.  Level 0 evaluates the empty set.
 * Level d evaluates a frontier of distinct sets of size d; a set under which the
 * outcome is lost is a minimal cut of size d and is not expanded.  For every
 * other set F, W_F is nemo_witness_sets' single derivation under F (a needed goal
 * needs its alive child of smallest node index; not NEMO_WIT_ALL), and the
 * children of F are F + {e} for every candidate e that is in W_F.  The frontier
 * of level d + 1 holds the distinct children of level d's non-cuts that have no
 * proper subset among the cuts of sizes <= d.  The search stops after level
 * max_size, or when a frontier is empty.  Every minimal cut is reached: a
 * minimal cut C and a non-cut F inside it meet in W_F outside F (were no node of
 * W_F in C, every node of W_F, an alive root among them, would be alive under C),
 * so some child of F lies in C; a reached cut that is not minimal holds a smaller
 * minimal cut found at an earlier level and was dropped before it was evaluated.
 * Which events a level evaluates depends on the witnesses; the rows do not.
 * n_cand == 0 with a list, a graph without roots, and a graph with no cut up to
 * max_size give zero rows and NEMO_OK; in the first two cases no set is evaluated
 * and every stat is 0.  An iteration that is not loaded is NEMO_ERR_NOTFOUND;
 * cond outside 0 / 1 is NEMO_ERR_INVALID; a node context, and a call without a
 * loaded corpus, return NEMO_ERR_STATE.
 * Limits, NEMO_ERR_LIMIT, the call then leaves no results: a frontier of more
 * than 2^32 - 2 sets; a level that emits more children (counted before duplicates
 * are removed) than the option "lineage_children_max" allows (the message names
 * the count and the option).  The emission buffer grows only: a level that
 * counted more children than it holds runs again, once, behind a buffer of the
 * counted size.
 * The call blocks until the rows are on the host; per level two kernels run and
 * one block of counters comes back (the cuts so far, the children counted, the
 * next frontier's sets).  The results are the call's own state: valid until the
 * next nemo_lineage_cuts or nemo_load_corpus (the fetches return NEMO_ERR_STATE
 * otherwise), independent of every other call's state in both directions.  The
 * tier is "wit_lds_max"'s (the image is the witness calls': the graph, the dead
 * words and the need words), the grid cap "kl_grid"'s.                           */
typedef struct nemo_lineage_cut {
  uint32_t size;    /* 1..8                                                          */
  uint32_t node[8]; /* nodes in candidate-list order, unused = UINT32_MAX            */
} nemo_lineage_cut;
int nemo_lineage_cuts(nemo_ctx *ctx, uint32_t iteration, int cond, const uint32_t *cand, size_t n_cand, uint32_t max_size,
                      uint32_t flags);
/* out[k] for every minimal cut k; out == NULL queries *n_out.                  */
int nemo_fetch_lineage_cuts(nemo_ctx *ctx, nemo_lineage_cut *out, uint64_t cap, uint64_t *n_out);
/* Per size d = 0..8: out[2 d] = sets evaluated at size d, out[2 d + 1] = minimal
 * cuts found of size d (zeros past the last level the search reached).         */
int nemo_fetch_lineage_cut_stats(nemo_ctx *ctx, uint64_t out[18]);

/* ---- knock-out by label: fault sets tested against every listed run in one call ----
 * The subject (a raw loaded graph), dead_F(v), the roots and "the outcome is lost
 * under F" (roots_dead == n_roots > 0) are the knock-out definitions above.  A
 * hypothesis here names events, not nodes: an interned label is the same event
 * in every run of the corpus.  Set s names the labels
 * set_labels[set_off[s] .. set_off[s+1]).  On the graph of list position i,
 * g = 2 * run_index(iters[i]) + cond, set s removes F(i,s): every node of g, goal
 * or rule, whose label is in the set.  Under NEMO_KL_SINKS only sink goals match:
 * nodes that are no rule and have no children (an empty forward row).
 * The result is a bit per (list position, set), in chunks of 64 sets:
 * n_chunks = ceil(n_sets / 64), set s is bit s & 63 of word [i * n_chunks + s / 64].
 *   lost bit (i,s): roots_dead == n_roots > 0 under F(i,s);
 *   hit bit (i,s):  F(i,s) is non-empty.
 * Bits of the last chunk at or past n_sets are 0.  n_lost[s] and n_hit[s] count
 * list positions: a run listed twice counts twice, and its two rows of words are
 * identical.  An empty set hits nothing and loses nothing; a label named twice
 * in a set counts once; a label that no node of a graph carries matches nothing
 * there.  n == 0 or n_sets == 0 gives zero words and NEMO_OK (the counts of
 * n_sets sets over no list position are 0).
 * NEMO_ERR_INVALID, all checked on the host before anything is uploaded: a
 * decreasing set_off, a label equal to UINT32_MAX, flags other than 0 or
 * NEMO_KL_SINKS, cond outside 0 / 1.  An iteration that is not loaded is
 * NEMO_ERR_NOTFOUND; a node context returns NEMO_ERR_STATE.  n * n_chunks > 2^28
 * words, more than 2^32 - 1 labels named in all, or more than 2^32 - 1 sets, is
 * NEMO_ERR_LIMIT: tile the call (the limits are read from n, n_sets and set_off
 * alone, before any label is).
 * The call blocks until the words and counts are on the host, as the knock-out
 * calls do.  The results are the call's own state: valid until the next
 * nemo_knockout_labels or nemo_load_corpus (the fetches return NEMO_ERR_STATE
 * otherwise), independent of the knock-out, cut, diff, symmetric diff, nearest
 * and class state in both directions.                                          */
#define NEMO_KL_SINKS 1u  /* only sink goals (goals without children) match a label */
int nemo_knockout_labels(nemo_ctx *ctx, const uint32_t *iters, size_t n, int cond,
                         const uint64_t *set_off, const uint32_t *set_labels, size_t n_sets,
                         uint32_t flags);
/* n * n_chunks words each, n_chunks = ceil(n_sets / 64); word [i * n_chunks + c], bit s & 63;
 * either pointer may be NULL; cap_words >= n * n_chunks                        */
int nemo_fetch_knockout_labels(nemo_ctx *ctx, uint64_t *lost, uint64_t *hit, uint64_t cap_words);
/* per set: list positions lost, list positions hit; cap >= n_sets each         */
int nemo_fetch_knockout_label_counts(nemo_ctx *ctx, uint32_t *n_lost, uint32_t *n_hit, uint64_t cap);

/* ---- minimal cut sets by label: the smallest fault sets that defeat every listed run ----
 * The search over events across runs: which one, two or three events, lost
 * together, defeat the outcome on all of the listed runs, or on at least q of
 * them.  The subject (a raw loaded graph), dead_F(v), the roots and "the outcome
 * is lost under F" (roots_dead == n_roots > 0) are the knock-out definitions
 * above; F(i,S) is nemo_knockout_labels' definition: every node of graph
 * g = 2 * run_index(iters[i]) + cond, goal or rule, whose label is in S.  Under
 * NEMO_KL_SINKS only sink goals are in F(i,S).  flags is 0 or NEMO_KL_SINKS.
 * Cuts: lost_count(S) is the number of list positions i on which the outcome is
 * lost under F(i,S); a run listed twice counts twice.  q = min_runs, where 0
 * means n; min_runs > n is NEMO_ERR_INVALID.  S is a cut iff n > 0 and
 * lost_count(S) >= q.  lost is monotone in S, so lost_count is, every superset
 * of a cut is a cut, and a cut is minimal iff no proper subset of it is a cut.
 * The call returns all minimal cuts of size <= max_size among the candidates;
 * max_size must be 1, 2 or 3 (NEMO_ERR_INVALID otherwise).  A listed graph
 * without roots is never lost: under q = n such a list yields zero rows.
 * Candidates: cand_labels[0 .. n_cand) must be distinct and differ from
 * UINT32_MAX, which is no label.  A duplicate, or a label equal to UINT32_MAX,
 * is NEMO_ERR_INVALID, checked on the host before anything is uploaded; the
 * message gives the position of the offence and the label.  cand_labels == NULL
 * with n_cand > 0 is NEMO_ERR_INVALID: there is no implicit list.
 * Rounds: round 1 evaluates the K singletons on every list position and keeps
 * the lost bit and the hit bit.  The live list holds, in candidate order, the
 * candidates that are no cut alone and that hit at least one listed graph, K1
 * entries (a label that hits no listed node can be in no minimal cut: S and S
 * without it remove the same nodes).  Round 2 evaluates all C(K1,2) pairs of
 * live positions; every pair with lost_count >= q is minimal.  Round 3
 * evaluates all C(K1,3) triples; a triple with lost_count >= q is minimal iff
 * none of its three pairs was a cut in round 2.
 * Hypothesis index: the colex rank of nemo_min_cuts over the live positions
 * (a < b < c: C(c,3) + C(b,2) + a, pairs C(b,2) + a, singles a).  The rows are
 * sorted by (size, rank); a row's labels are in candidate-list order, unused
 * entries UINT32_MAX; n_lost[k] is lost_count of row k.
 * n == 0 or n_cand == 0 gives zero rows and NEMO_OK.  A round of more than
 * 2^32 - 2 hypotheses, or a round with n * ceil(hyps / 64) > 2^28 words, is
 * NEMO_ERR_LIMIT (shorten the candidate list or the run list); both limits are
 * checked per round, before that round's launch (K1 is known only after round
 * 1), and the call then leaves no results.  An iteration that is not loaded is
 * NEMO_ERR_NOTFOUND; cond outside 0 / 1 and unknown flags are NEMO_ERR_INVALID;
 * a node context, and a call without a loaded corpus, return NEMO_ERR_STATE.
 * The call blocks until the rows are on the host.  The results are the call's
 * own state: valid until the next nemo_min_label_cuts or nemo_load_corpus (the
 * fetches return NEMO_ERR_STATE otherwise), independent of the knock-out, cut,
 * label knock-out, diff, symmetric diff, nearest and class state in both
 * directions.  No option of its own: the tier is "knock_lds_max"'s, the grid cap
 * "kl_grid"'s.                                                                 */
typedef struct nemo_label_cut {
  uint32_t size;     /* 1..3                                                         */
  uint32_t label[3]; /* labels in candidate-list order, unused = UINT32_MAX          */
} nemo_label_cut;
int nemo_min_label_cuts(nemo_ctx *ctx, const uint32_t *iters, size_t n, int cond,
                        const uint32_t *cand_labels, size_t n_cand, uint32_t max_size,
                        uint32_t min_runs, uint32_t flags);
/* out[k] for every minimal cut k, n_lost[k] its lost_count (n_lost may be NULL);
 * out == NULL queries *n_out.                                                  */
int nemo_fetch_min_label_cuts(nemo_ctx *ctx, nemo_label_cut *out, uint32_t *n_lost, uint64_t cap, uint64_t *n_out);
/* As nemo_fetch_min_cut_stats: per size s = 1..3, out[3 (s - 1) ..]: live
 * candidates entering the round, hypotheses evaluated, minimal cuts found.     */
int nemo_fetch_min_label_cut_stats(nemo_ctx *ctx, uint64_t out[9]);

/* ---- minimal cut sets over fault events: groups of labels as candidates ----
 * nemo_min_label_cuts with candidates that are sets of labels: a fault event
 * that removes many labels at once (a crash removes every clock goal its node
 * would send or receive from then on) is one candidate, and a hypothesis of one
 * crash and one omission is a pair.  The subject (a raw loaded graph),
 * dead_F(v), the roots and "the outcome is lost under F"
 * (roots_dead == n_roots > 0) are the knock-out definitions above.
 * Candidates and removal sets: candidate k is the label set
 * G_k = group_labels[group_off[k] .. group_off[k+1]).  For a set S of candidate
 * positions, F(i,S) is every node of graph g = 2 * run_index(iters[i]) + cond,
 * goal or rule, whose label lies in the union of G_k for k in S.  Under
 * NEMO_KL_SINKS only sink goals are in F(i,S).  flags is 0 or NEMO_KL_SINKS.
 * Cuts: lost_count(S) is the number of list positions i on which the outcome is
 * lost under F(i,S); a run listed twice counts twice.  q = min_runs, where 0
 * means n; min_runs > n is NEMO_ERR_INVALID.  S is a cut iff n > 0 and
 * lost_count(S) >= q.  A listed graph without roots is never lost.  F is
 * monotone in S, so lost and lost_count are, and every superset of a cut is a
 * cut; S is minimal iff no proper subset of its candidates is a cut.
 * Minimality is over candidate positions, not over label sets: two candidates
 * with equal or nested groups are different candidates, and if each is a cut
 * alone, each is a row.  A pair of nested groups is never a minimal cut; that
 * follows from monotonicity and needs no special handling: the pair removes
 * what the larger group removes alone, so the pair is a cut only if the larger
 * candidate is one alone, and then it was no live candidate of round 2.
 * Legal input: an empty group is legal, it hits nothing and is never live; a
 * label named twice in a group counts once; a label that no listed node
 * carries matches nothing.
 * Rounds: nemo_min_label_cuts' rounds over candidate positions.  Round 1
 * evaluates the K = n_groups singletons on every list position and keeps the
 * lost bit and the hit bit.  The live list holds, in candidate order, the
 * candidates that are no cut alone and whose group hit at least one listed
 * graph, K1 entries (S and S without a candidate that hits no listed node
 * remove the same nodes).  Round 2 evaluates all C(K1,2) pairs of live
 * positions; every pair with lost_count >= q is minimal.  Round 3 evaluates all
 * C(K1,3) triples; a triple with lost_count >= q is minimal iff none of its
 * three pairs was a cut in round 2.  max_size must be 1, 2 or 3.
 * Hypothesis index: the colex rank of nemo_min_cuts over the live positions
 * (a < b < c: C(c,3) + C(b,2) + a, pairs C(b,2) + a, singles a).  The rows are
 * sorted by (size, rank); a row's entries are candidate positions (indices into
 * the group list), ascending, unused entries UINT32_MAX; n_lost[k] is
 * lost_count of row k.
 * NEMO_ERR_INVALID, all checked on the host before anything is uploaded: a
 * decreasing group_off (the message gives the group); a label equal to
 * UINT32_MAX, which is no label (the message gives the group and the position
 * in group_labels); group_off == NULL with n_groups > 0 or group_labels == NULL
 * where the groups name a label (there is no implicit event list); max_size
 * outside 1..3 ("max_size must be 1, 2 or 3"); min_runs > n; cond outside
 * 0 / 1; unknown flags.  NEMO_ERR_LIMIT: more than 2^32 - 1 labels named in all,
 * or more than 2^24 labels in one group (both read from group_off alone,
 * before any label is; split such a group); more distinct labels D than leave
 * D + 1 + V <= 2^32 - 1 for the largest listed graph; a round of more than
 * 2^32 - 2 hypotheses; a round with n * ceil(hyps / 64) > 2^28 words (shorten
 * the group list or the run list).  The two round limits are checked per
 * round, before that round's launch (K1 is known only after round 1), and the
 * call then leaves no results.  An iteration that is not loaded is
 * NEMO_ERR_NOTFOUND; a node context, and a call without a loaded corpus, return
 * NEMO_ERR_STATE.
 * n == 0 or n_groups == 0 gives zero rows and NEMO_OK.  The call blocks until
 * the rows are on the host.  The results are the call's own state: valid until
 * the next nemo_min_group_cuts or nemo_load_corpus (the fetches return
 * NEMO_ERR_STATE otherwise), independent of the knock-out, cut, label knock-out,
 * label cut, diff, symmetric diff, nearest and class state in both directions.
 * No option of its own: the tier is "knock_lds_max"'s, the grid cap "kl_grid"'s. */
typedef struct nemo_group_cut {
  uint32_t size;     /* 1..3                                                         */
  uint32_t group[3]; /* candidate positions (indices into the group list), ascending, unused = UINT32_MAX */
} nemo_group_cut;
int nemo_min_group_cuts(nemo_ctx *ctx, const uint32_t *iters, size_t n, int cond,
                        const uint64_t *group_off /* [n_groups + 1] */, const uint32_t *group_labels,
                        size_t n_groups, uint32_t max_size, uint32_t min_runs, uint32_t flags);
/* out[k] for every minimal cut k, n_lost[k] its lost_count (n_lost may be NULL);
 * out == NULL queries *n_out.                                                  */
int nemo_fetch_min_group_cuts(nemo_ctx *ctx, nemo_group_cut *out, uint32_t *n_lost, uint64_t cap, uint64_t *n_out);
/* As nemo_fetch_min_cut_stats: per size s = 1..3, out[3 (s - 1) ..]: live
 * candidates entering the round, hypotheses evaluated, minimal cuts found.     */
int nemo_fetch_min_group_cut_stats(nemo_ctx *ctx, uint64_t out[9]);

/* ---- lineage cut search over fault events: minimal cuts up to size 8 across runs ----
 * nemo_min_group_cuts' question, answered by nemo_lineage_cuts' search: which
 * fault events, lost together, defeat the outcome on at least q of the listed
 * runs, for sets of up to eight events.
 * Definitions: the candidates (candidate k is the label set G_k), F(i,S),
 * NEMO_KL_SINKS, lost_count(S), q = min_runs (0 means n), "cut" and minimality
 * over candidate positions are nemo_min_group_cuts' definitions above,
 * unchanged; so is what counts as legal input: empty, nested and overlapping
 * groups, a label named twice, a label no listed node carries, a run listed
 * twice (it counts twice).
 * Result, whatever the search below does: all minimal cuts of size <= max_size
 * (1..8), sorted by (size, colex order of the candidate positions: the largest
 * position first, then the next largest); a row's positions ascend, unused
 * entries UINT32_MAX; n_lost[k] is row k's lost_count.  For max_size <= 3 the
 * rows and n_lost are nemo_min_group_cuts' own, in its order: a minimal cut
 * holds live candidates only (a candidate that hits no listed node changes no
 * F(i,S), and one that is a cut alone is a row by itself), the sets of live
 * candidates it evaluates are all of them, and its live list keeps candidate
 * order, so colex over live positions and colex over candidate positions agree.
 * Search (specified, so that the stats are deterministic): level 0 evaluates the
 * empty set; level d evaluates a frontier of distinct sets of size d on every
 * list position.  A set with lost_count >= q is a minimal cut of size d and is
 * not expanded.  For every other set F the children are F + {k}: candidate k
 * qualifies when, for some list position i on which the outcome is not lost
 * under F(i,F), some label of G_k is the label of a node of W_F^i, where W_F^i
 * is nemo_witness_labels' single derivation on that graph under F(i,F) (a needed
 * goal needs its alive child of smallest node index; not NEMO_WIT_ALL).  Under
 * NEMO_KL_SINKS only sink goals of W_F^i count.  The frontier of level d + 1
 * holds the distinct children that have no proper subset among the cuts of sizes
 * <= d.  The search stops after level max_size or at an empty frontier.
 * Every minimal cut is reached.  Take a minimal cut C and a non-cut F inside it:
 * lost_count(F) < q <= lost_count(C) and lost is monotone, so there is a list
 * position i that is lost under C and not under F.  F(i,C) must hit a node v of
 * W_F^i: otherwise every node of W_F^i, an alive root among them, would stay
 * alive under C.  v is alive under F, so the candidate of C whose group names
 * v's label is not in F; hence a child of F lies in C.  A reached cut that is
 * not minimal holds an earlier minimal cut and was filtered before it was
 * evaluated.
 * Emission: children are emitted from every (list position, set) on which the
 * set is not lost, whether or not the cross-run count later makes the set a
 * cut: the children of a set that turns out to be a cut are supersets of it and
 * the subset filter drops them.  This keeps a level's evaluation one fused pass
 * and costs nothing under q = n, where a cut is lost on every list position and
 * emits nothing.  The child count that the emission limit is checked against is
 * this count: every list position's children, before duplicates are removed.
 * NEMO_ERR_INVALID, all checked on the host before anything is uploaded: a
 * decreasing group_off (the message gives the group); a label equal to
 * UINT32_MAX (the message gives the group and the position in group_labels);
 * iters == NULL with n > 0, group_off == NULL with n_groups > 0, group_labels
 * == NULL where the groups name a label; max_size outside 1..8 ("max_size must
 * be 1..8"); min_runs > n; cond outside 0 / 1; unknown flags.  NEMO_ERR_LIMIT:
 * more than 65535 groups (a set is kept as eight u16 candidate positions);
 * nemo_min_group_cuts' label-count limits (2^32 - 1 labels in all, 2^24 in one
 * group, D + 1 + V <= 2^32 - 1); a level with n * ceil(frontier / 64) > 2^28 lost
 * words; a frontier of more than 2^32 - 2 sets; a level whose counted children
 * pass the option "lineage_children_max" (the message names the count and the
 * option).  A call that ends in a limit leaves no results.  The emission buffer
 * grows only: a level that counted more children than it holds runs again,
 * once, behind a buffer of the counted size, and does not append its cuts twice.
 * n == 0, n_groups == 0, or every listed graph empty: zero rows, every stat 0,
 * NEMO_OK, and nothing is evaluated.  An iteration that is not loaded is
 * NEMO_ERR_NOTFOUND; a node context, and a call without a loaded corpus, return
 * NEMO_ERR_STATE.
 * The call blocks until the rows are on the host; per level three kernels run
 * (the evaluation once per tier) and one block of counters comes back.  The
 * results are the call's own state: valid until the next
 * nemo_lineage_group_cuts or nemo_load_corpus (the fetches return
 * NEMO_ERR_STATE otherwise), independent of every other call's state in both
 * directions.  No option of its own: the tier is "wit_lds_max"'s, the grid cap
 * "kl_grid"'s, the emission limit "lineage_children_max"'s.                     */
typedef struct nemo_lineage_group_cut {
  uint32_t size;     /* 1..8                                                         */
  uint32_t group[8]; /* candidate positions, ascending, unused = UINT32_MAX          */
} nemo_lineage_group_cut;
int nemo_lineage_group_cuts(nemo_ctx *ctx, const uint32_t *iters, size_t n, int cond,
                            const uint64_t *group_off /* [n_groups + 1] */, const uint32_t *group_labels,
                            size_t n_groups, uint32_t max_size, uint32_t min_runs, uint32_t flags);
/* out[k] for every minimal cut k, n_lost[k] its lost_count (n_lost may be NULL);
 * out == NULL queries *n_out.                                                  */
int nemo_fetch_lineage_group_cuts(nemo_ctx *ctx, nemo_lineage_group_cut *out, uint32_t *n_lost, uint64_t cap, uint64_t *n_out);
/* As nemo_fetch_lineage_cut_stats: per size d = 0..8, out[2 d] = sets evaluated
 * at size d, out[2 d + 1] = minimal cuts found of size d.                      */
int nemo_fetch_lineage_group_cut_stats(nemo_ctx *ctx, uint64_t out[18]);

/* ---- surviving derivations: why a run's outcome withstands a fault set ---------
 * The other half of the knock-out family: where those calls say whether a fault
 * set defeats the outcome, these say which derivation is left when it does not,
 * and which base events that derivation rests on (the events the next fault
 * hypothesis must hit).  The subject (a raw loaded graph g = 2r + cond),
 * dead_F(v) and the roots (the nodes of in-degree 0) are the knock-out
 * definitions above, unchanged.  alive = not dead.  Two facts follow from the
 * definition and make the rest well defined: an alive rule has only alive
 * children, and an alive goal with children has at least one alive child.
 * For a hypothesis h with removed set F_h, need_h is defined top-down along the
 * DUETO edges, roots first:
 *   - a root is needed iff it is alive;
 *   - a needed rule needs every child;
 *   - a needed goal with children needs exactly one child, the alive child of
 *     smallest node index; under NEMO_WIT_ALL it needs every alive child;
 *   - a sink goal (a goal without children) needs nothing further.
 * As in the knock-out definition all of this goes by the node's own kind and
 * does not assume that goals and rules alternate.  W_h = {v : need_h(v)} is one
 * derivation of every surviving root; under NEMO_WIT_ALL it is the whole
 * surviving provenance, the union of all remaining derivations.  The loaded
 * forward rows ascend by child index, so "smallest index" is "first alive child
 * in row order", on both tiers.
 * nemo_witness_sets takes explicit node sets on one graph: the arguments, the
 * checks, the messages and the limits are nemo_knockout_sets'; hypothesis s is
 * set s; NEMO_WIT_SINKS is NEMO_ERR_INVALID here.  nemo_witness_labels takes
 * label sets against every listed run: F(i,s), the checks and the messages are
 * nemo_knockout_labels' (NEMO_WIT_SINKS has NEMO_KL_SINKS' meaning: only sink
 * goals match a label); the hypothesis index is i * n_sets + s.  Its limits, all
 * NEMO_ERR_LIMIT with "tile the call": n * n_sets > 2^32 - 2, more than 2^28
 * words (n list positions x chunks of 64 sets), more than 2^32 - 1 labels named,
 * a hit list past 2^32 - 1 entries (distinct labels + 1 + V_g), or, with
 * NEMO_WIT_MASKS, need words kept past 2^36 bytes (8 V_g bytes per list
 * position and chunk of 64 sets; the node-set form has the same limit).
 * Legal input that gives rows, not errors: the empty set (W is the derivation
 * of the unharmed graph), a graph without roots (every count is 0), every root
 * dead (roots_alive 0, W_h empty), a node or label named twice in a set, a label
 * no listed node carries, a run listed twice (identical rows).  n_sets == 0 or
 * n == 0 gives zero rows and NEMO_OK; an iteration that is not loaded is
 * NEMO_ERR_NOTFOUND; cond outside 0 / 1 and unknown flags are NEMO_ERR_INVALID;
 * a node context returns NEMO_ERR_STATE (single-device contexts only).
 * Everything runs on the device on the context's stream (k_wit_lds / k_wit_glob:
 * the knock-out sweep, then one more pass over the same levels, roots first);
 * the calls block until the rows are on the host.  The result is the two calls'
 * own state: valid until the next witness call or nemo_load_corpus (the fetches
 * return NEMO_ERR_STATE otherwise), independent of every other call's state in
 * both directions.  The tier is "wit_lds_max"'s, the grid cap "kl_grid"'s.      */
typedef struct nemo_witness {
  uint32_t graph;       /* 2r + cond                                                  */
  uint32_t n_roots;     /* nodes of in-degree 0                                       */
  uint32_t roots_alive; /* = roots in W_h; 0 means the outcome's every root is dead and W_h is empty */
  uint32_t n_nodes;     /* |W_h|                                                      */
  uint32_t n_sinks;     /* sink goals (no rule, empty forward row) in W_h: the base events W_h rests on */
} nemo_witness;
#define NEMO_WIT_ALL 1u   /* every surviving derivation, not one                       */
#define NEMO_WIT_MASKS 2u /* keep the need words for nemo_fetch_witness_mask           */
#define NEMO_WIT_SINKS 4u /* label form only: NEMO_KL_SINKS' meaning, only sink goals match a label */
int nemo_witness_sets(nemo_ctx *ctx, uint32_t iteration, int cond, const uint64_t *set_off, const uint32_t *set_nodes,
                      size_t n_sets, uint32_t flags);
int nemo_witness_labels(nemo_ctx *ctx, const uint32_t *iters, size_t n, int cond, const uint64_t *set_off,
                        const uint32_t *set_labels, size_t n_sets, uint32_t flags);
/* out[h] for every hypothesis h; out == NULL queries *n_out.                    */
int nemo_fetch_witness(nemo_ctx *ctx, nemo_witness *out, uint64_t cap, uint64_t *n_out);
/* One byte per node of hypothesis hyp's graph, 1 = in W_h; cap >= V_g.  Needs a
 * call with NEMO_WIT_MASKS (NEMO_ERR_STATE otherwise).  The column is taken on
 * the host from the V need words of the hypothesis' chunk.                      */
int nemo_fetch_witness_mask(nemo_ctx *ctx, uint64_t hyp, uint8_t *out, uint64_t cap);

/* ---- corrections / extensions on run 0 (corrections.go:25-193, extensions.go:13-99)
 * pre rows (a, g, r) of findPreTriggers, post rows (g, r) of findPostTriggers,
 * async rules of GenerateExtensions (only meaningful when not all achieved).  */
int nemo_triggers(nemo_ctx *ctx);
int nemo_fetch_triggers(nemo_ctx *ctx, uint32_t *pre_rows /* 3 per row */, uint64_t pre_cap,
                        uint64_t *n_pre, uint32_t *post_rows /* 2 per row */, uint64_t post_cap,
                        uint64_t *n_post, uint32_t *async_rules, uint64_t async_cap, uint64_t *n_async);

/* ---- results ---------------------------------------------------------------- */
/* Per-node flags (NEMO_F_*) of graphs [g_lo, g_hi), concatenated.           */
int nemo_fetch_node_flags(nemo_ctx *ctx, uint32_t g_lo, uint32_t g_hi, uint8_t *out, uint64_t cap);
/* Accepted @next chains of every graph, ordered by (graph, k).              */
int nemo_fetch_chains(nemo_ctx *ctx, nemo_chain *out, uint64_t cap, uint64_t *n_out);
/* Asynchronous hand-over of the simplification (SimplifyProv,
 * preprocessing.go:351-387) to the host, in the compact form a caller needs to
 * rebuild every simplified graph: 2 bits per node (NEMO_STATE_*; node v of the
 * corpus at byte v/4, bits 2*(v%4)) and every graph's accepted chains as dense
 * (head, tail) pairs (graph-local node indices; graph g's chain k at
 * chain_off[g] + k), copied into library-owned pinned memory on a second
 * stream, overlapping whatever the caller launches next.  State + pairs
 * determine the simplified graphs exactly (collapsed rule k of graph g:
 * preds(head) -> V_g + k -> succs(tail)); full flags stay available through
 * nemo_fetch_node_flags.                                                    */
#define NEMO_STATE_ALIVE 0x1u /* node is in the simplified graph (kept, not deleted) */
#define NEMO_STATE_HOLDS 0x2u /* condition_holds                                     */
int nemo_stage_simplified(nemo_ctx *ctx);
/* Waits for the staged copies and returns views into the pinned buffers:
 * state[ceil(V/4)], chain_off[G+1] and the pairs, chain_ht[n] as u32
 * head | tail << 16 when every graph has < 65536 nodes (*wide_pairs = 0),
 * else chain_ht[2n] as (head, tail) u32 (*wide_pairs = 1).  Valid until the
 * next nemo_stage_simplified or nemo_ctx_destroy.  Out-pointers may be NULL. */
int nemo_simplified_view(nemo_ctx *ctx, const uint8_t **state, const uint64_t **chain_off,
                         const uint32_t **chain_ht, uint64_t *n_chains, int *wide_pairs);
/* Per-run table bitsets, words = ceil(n_tables/32) u32 per run:
 *   which = 0: proto list of the run (extractProtos, prototype.go:11-24)
 *   which = 1: all rule tables of the simplified post graph (missingFrom)   */
int nemo_fetch_run_tables(nemo_ctx *ctx, int which, uint32_t *out, uint64_t cap);

/* ---- edge pulls (PullPrePostProv, pre-post-prov.go:288-459; Q24) -----------
 * which = 0: raw graphs, 1: simplified graphs (run 1000+i: kept, not deleted,
 * plus collapsed rules), 2: differential graphs of every diff entry, 3: the
 * symmetric diff's graphs (every entry's failed post graph induced on its S,
 * in that graph's row order; NEMO_ERR_STATE before nemo_diffprov_symmetric).
 * The compacted edge lists stay in HBM; `slot` below is the graph index (which
 * 0/1) or the diff entry (which 2/3).  Collapsed rule k of graph g is reported
 * as node index V_g + k.                                                   */
int nemo_pull_edges(nemo_ctx *ctx, int which);
uint64_t nemo_pulled_count(nemo_ctx *ctx, uint32_t slot);
int nemo_fetch_pulled(nemo_ctx *ctx, uint32_t slot, uint32_t *src, uint32_t *dst, uint64_t cap,
                      uint64_t *n_out);
/* Every slot at once (one call where the Go side would make one per graph):
 * off[slot] / cnt[slot] (pulled-slot count entries each) locate slot s's edges
 * in src/dst, whose used extent is *n_used (regions are claimed in device
 * order, so they are not sorted by slot; they are disjoint, except that diff
 * entries sharing a label source -- one D mask, one graph -- share one
 * region, and so do, under "graph_dedup" with "pull_dedup", the graphs of
 * identical content of a which 0/1 pull: node indices are graph-local, so
 * their edge lists are one list, and the sum of cnt[] then exceeds *n_used).
 * src/dst may be NULL to query *n_used; then cap >= *n_used.               */
int nemo_fetch_pulled_all(nemo_ctx *ctx, uint64_t *off, uint32_t *cnt, uint32_t *src, uint32_t *dst, uint64_t cap,
                          uint64_t *n_used);

/* ---- native ingest of a Molly output directory (host only) ------------------
 * Replaces Molly.LoadOutput's per-run JSON decoding (faultinjectors/molly.go:
 * 15-163) and the per-element interning of loadProv (pre-post-prov.go:25-213)
 * for callers that want the corpus arrays without a Go/Python decoding pass:
 * run_<i>_{pre,post}_provenance.json of runs i = 0..n_runs-1 are parsed on
 * `threads` threads (<= 0: up to 16) and interned in the order the sequential
 * loader would intern them.  `iterations[i]` is runs.json's Run.Iteration of
 * run i (the caller parses runs.json).  Validation failures return
 * NEMO_ERR_LOAD with the reference's message in `err`.  Node IDs are returned
 * without the run_<iteration>_<cond>_ prefix molly.go adds (it is common to a
 * graph, so id_rank is unaffected).                                          */
typedef struct nemo_ingest nemo_ingest;
#define NEMO_STR_TABLE     0  /* interned table names  (index < n_tables)      */
#define NEMO_STR_LABEL     1  /* interned labels                               */
#define NEMO_STR_NODE_ID   2  /* per node: Molly ID (unprefixed)               */
#define NEMO_STR_NODE_TYPE 3  /* per node: rule type ("" for goals)            */
#define NEMO_STR_NODE_TIME 4  /* per node: goal time after the clock rewrite   */
int nemo_ingest_molly(const char *out_dir, const uint32_t *iterations, uint32_t n_runs, int threads,
                      nemo_ingest **out, char *err, size_t err_cap);
/* Pointers into the ingest's arrays (valid until nemo_ingest_free); ready for nemo_load_corpus. */
int nemo_ingest_corpus(const nemo_ingest *h, nemo_corpus *corpus);
uint64_t nemo_ingest_count(const nemo_ingest *h, int kind);
int nemo_ingest_string(const nemo_ingest *h, int kind, uint64_t index, const char **s, size_t *len);
void nemo_ingest_free(nemo_ingest *h);
/* Streaming form: the same directory parsed chunk by chunk
 * so that chunk i is loaded and analysed on the device while chunk i+1 is
 * being parsed.  Interning is shared across chunks; ids are assigned in parse
 * order (below), so they can differ from nemo_ingest_molly's when run 0 or
 * failedRuns[0] is not first in runs.json; table "pre"/"post" ids are fixed
 * by the first chunk.  nemo_ingest_next parses the next `chunk` runs into a
 * corpus and, with `with_run0`, prepends the run of iteration 0 as a
 * replicated, not-owned run to every chunk after the one holding it (the good
 * run of the diffs, differential-provenance.go:26).  Parse order: the run of
 * iteration 0, then the run at index `first_failed` (failedRuns[0], whose
 * post-goal labels every reference-mode diff uses, :22-43; -1: none), then
 * the rest in runs.json order.  So with chunk >= 2 the first chunk holds
 * both, and every chunk that holds a failed run also holds the good run.
 * Returns NEMO_ERR_NOTFOUND when no run is left; validation failures as
 * nemo_ingest_molly.  Lifetime: the ingest keeps two buffers, so the arrays
 * of chunk i stay valid until the call that returns chunk i+2; chunk i can be
 * uploaded while chunk i+1 is parsed.                                      */
typedef struct nemo_ingest_stream nemo_ingest_stream;
int nemo_ingest_open(const char *out_dir, const uint32_t *iterations, uint32_t n_runs, int64_t first_failed,
                     int threads, nemo_ingest_stream **out);
int nemo_ingest_next(nemo_ingest_stream *s, uint32_t chunk, int with_run0, nemo_corpus *corpus, char *err,
                     size_t err_cap);
uint64_t nemo_ingest_stream_count(const nemo_ingest_stream *s, int kind);
int nemo_ingest_stream_string(const nemo_ingest_stream *s, int kind, uint64_t index, const char **str, size_t *len);
void nemo_ingest_close(nemo_ingest_stream *s);

/* ---- instrumentation ------------------------------------------------------ */
typedef struct nemo_timing {
  char name[32];      /* kernel name                                        */
  uint64_t launches;  /* launches recorded since the last reset             */
  double ms;          /* summed HIP-event time                              */
  double bytes;       /* summed algorithmic bytes     */
  double edges;       /* summed edges examined                              */
} nemo_timing;
int nemo_timings(nemo_ctx *ctx, nemo_timing *out, uint32_t cap, uint32_t *n_out);
int nemo_reset_timings(nemo_ctx *ctx);
int nemo_synchronize(nemo_ctx *ctx);
/* Inspection hook for tests: copy bytes of a named internal device array
 * ("topo", "lvl", "nlev", "fp", "fc", "rp", "rc", "flags", "dbits", "dmask",
 * "e2", "posoff").  "e2" (one u32 per edge, at the graph's edge offset: src <<
 * 16 | dst, graph-local node indices, the forward rows in the Kahn order of
 * their source) and "posoff" (one u32 per node, at the graph's node offset:
 * the first e2 entry of each Kahn position) hold the post graphs that the LDS
 * tier of the load built; the entries of every other graph are unspecified. */
int nemo_debug_copy(nemo_ctx *ctx, const char *name, void *out, uint64_t offset, uint64_t bytes);

#ifdef __cplusplus
}
#endif
#endif /* NEMOHIP_H */
