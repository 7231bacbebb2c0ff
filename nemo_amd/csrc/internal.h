// internal.h — host/device interface between the C ABI (api.hip) and the kernels.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

struct DevCorpus;

namespace nemo {

struct DiffArgs {
  uint32_t g0;              // run 0's post graph
  const uint32_t *src;      // [entries] label-source graph per entry
  const uint32_t *ref_labels;  // label mode: [n, label...] used by every entry (NULL: src)
  const uint32_t *r0lab;    // sorted goal labels of g0
  const uint32_t *r0idx;    // local node of each sorted label
  uint32_t n_r0lab;
  const uint32_t *r0hkey;   // open-addressed label -> first sorted entry: key = label + 1 (0 empty)
  const uint32_t *r0hval;
  uint32_t r0hmask;         // table size - 1 (power of two)
  uint8_t *bits;            // [entries * V0] scratch
  int32_t *depth;           // [entries * V0] scratch
  // g0 in Kahn order for the global tier (k_dprep_*): node -> position,
  // parent / child rows as positions, level << 1 | rule, label nodes as positions
  uint32_t *tpos, *trp, *tfp, *trc, *tfc, *tinfo, *r0pos;
  uint8_t *mask;            // [entries * V0] D mask (output)
  uint32_t *missing;        // [2 * cap] (entry, rule)
  uint32_t *n_missing;      // counter
};

// Run 0's post graph g0 relaid in Kahn order (k_dx.hip k_dxp_*, built with the
// CSR in every load / rebuild): positions 0..V0-1 are the Kahn order; parents
// in Kahn order and children in reversed Kahn order ("walk order"), as walk
// indices, so that a window of consecutive positions reads one contiguous row range.
struct DxPrep {
  uint32_t g0, V0, E0;
  uint32_t *tpos;            // [V0] node -> position
  uint32_t *pnode;           // [V0] position -> node (the Kahn order the relayout was built from)
  uint32_t *info;            // [V0] level << 3 | DXI_RULE
  uint32_t *lbeg, *lend;     // [V0] first position of the position's Kahn level / of the next level
  uint32_t *rp, *rc;         // [V0 + 1], [E0 + 4] parents of position i, as positions
  uint32_t *fp, *fc;         // [V0 + 1], [E0 + 4] children of position V0-1-i, as reversed positions
  const uint32_t *r0idx;     // [n_r0lab] node of each sorted run-0 goal label
  uint32_t *r0pos;           // [n_r0lab] its position
  uint32_t n_r0lab;
  uint32_t *r0dense;         // the dense label table (DxArgs::r0dense; null: none): k_dxp_b writes
                             // the run-0 labels' entries, a single position as pos << 4
  const uint32_t *r0lab;     // [n_r0lab] sorted run-0 goal labels
  const uint32_t *err0;      // g0's load error flag (k_build / k_csr / k_topo): set, the CSR and Kahn
                             // order may be partial and every relayout kernel does nothing (the load fails)
};
#define DXI_RULE 1u   // the position is a rule

// A walk image of g0 (k_dx.hip k_dxi_*, built once per load and window
// configuration): the walk order cut into windows, and per window its links
// as ring records, its walk steps (<= 256 links of one level) and, per
// position, the links that leave the ring.  The walks stage a window by
// copying these ranges (no per-window derivation).  Image 0: Kahn order over
// parents (Fwd*, depth), 1: reversed Kahn order over children (Bwd*).
struct DxImg {
  uint32_t W, R, EC;         // positions, ring slots (power of two, >= 4 W; whole: V0), links per window
  uint32_t whole;            // 1: one window, ring = positions (no misses)
  uint32_t rev;              // 1: reversed walk order (children rows)
  uint32_t *nw;              // [1] windows
  uint32_t *wb;              // [V0 + 2] first walk index of window k; wb[nw] = V0
  uint32_t *stepb;           // [V0 + 2] first step of window k; [nw] = total
  uint32_t *steps;           // [2 V0 + E0 / 256 + 4] first link (in the window) | links << 16
  uint32_t *rec;             // [E0 + 4] per link (walk-order rows): linked ring slot (R: a miss) | owner's slot << 16
  uint32_t *moff;            // [V0 + 1] first miss of walk index i in mx
  uint32_t *mx;              // [E0 + 1] walk index linked by each miss
};
struct DxImgScratch {
  uint32_t *fseg;            // [V0 + 1] segment flags -> segment numbers
  uint32_t *segpos;          // [V0 + 2] first walk index of each segment
  uint32_t *fstep;           // [V0 + 1] steps per segment -> first step
  uint32_t *tsum;            // scan tiles
};

// the diff call's row counter (DxArgs::n_missing): rows in the low bits, bit 30 raised when a
// fused walk's hand-off wait gave up (k_dx.hip dx_publish)
#define DX_ROWS 0x3FFFFFFFu
#define DX_ERR_HANDOFF 0x40000000u

// One multi-entry CreateNaiveDiffProv call (k_dx.hip): nu distinct label
// sources in chunks of 64, one bit per source in every u64 word.
struct DxArgs {
  DxPrep p;
  uint32_t nu, nch;          // distinct label sources, 64-source chunks
  const uint32_t *src;       // [nu] label-source graph (post graph of the source run)
  const uint32_t *ref_labels;  // label mode: [n, label...] of the single source (src unused)
  const uint32_t *r0lab, *r0hkey, *r0hval;
  uint32_t r0hmask;
  // label -> its run-0 position << 4 when it labels one run-0 goal, else (first sorted run-0 goal
  // label entry << 4 | min(count, 15)); NEMO_NONE = not a run-0 post-goal label; labels >= nlab are
  // not either (null: the hash table above)
  const uint32_t *r0dense;
  uint32_t nlab;
  uint32_t *pb;              // [nu][w32] present bitmaps over positions
  uint32_t w32;              // ceil(V0 / 32)
  uint32_t lab_per;          // source nodes per k_dx_label workgroup
  uint32_t lab_split;        // workgroups per source (1: LDS bitmap stored whole)
  uint64_t *gw;              // [nch][V0] Good bits by position; after the walks: LP rules (k_dx_lp)
  uint64_t *bw;              // [nch][V0] Bwd*(Good) by REVERSED position (V0 - 1 - pos)
  uint64_t *dw;              // [nch][V0] D = Fwd* & Bwd* by position (k_dx_lp; k_dx_mask reads fb & bw)
  uint64_t *lw;              // [nch][V0] leaf candidates: Bwd* goals without a Bwd* child, by position
  uint8_t *fb;               // [nch][64 / NE][V0] Fwd* bits of the NE sources of longest-path workgroup g
  uint32_t *sval;            // [nu][V0] val = 1 + the longest path from Good (0 off Fwd*) by position
  uint32_t *maxlen;          // [nu] the longest LP val of each source (zeroed per call)
  uint32_t *wflag;           // [nch] Bwd* walk of the chunk done (whole-graph walks; zeroed per call)
  uint32_t ne;               // sources per longest-path workgroup of the walks launched (k_dx_mask)
  uint32_t fuse;             // 1: the longest-path workgroups also take LP rules, maxLen and the missing
                             // rows (whole-graph walks; k_dx_lp / k_dx_emit not launched)
  uint32_t legacy_lp;        // test knob (option diff_fuse 0): no fusion
  const uint32_t *urep;      // [nu] each source's first entry
  uint32_t own_mask;         // 1: one entry per source and fused walks: the longest-path workgroups
                             // write the D masks (k_dx_mask not launched)
  uint8_t *mask;             // [n_entries][V0] D masks by node (output)
  const uint32_t *map;       // [n_entries] entry -> source
  uint32_t n_entries;
  uint32_t *missing;         // [2 * cap] (source, rule node)
  uint32_t *n_missing;
  uint32_t window;           // test knob: 0 by size, 1 windowed walks, 2 tiny windows (ring misses)
  DxImg img[2];              // walk images: Kahn order (Fwd*, depth), reversed (Bwd*)
};

// A post graph's goal labels, open-addressed: key = label + 1 (0 empty), slot hash_label(label) &
// mask, linear probing.  k_lab_hash builds one per distinct `other` run of nemo_diffprov_pairs (the
// layout of the load's run-0 table, load_host.h); sdiff_mark_bad probes entry e's.
struct LabTab {
  uint32_t *key;            // [mask + 1], 16-byte aligned
  uint32_t mask;            // table size - 1 (power of two, >= 15)
  uint32_t graph;           // the post graph whose goals it holds
};

// One nemo_diffprov_symmetric / nemo_diffprov_pairs call (k_sdiff.hip): entry e walks its own graph
// graph[e] (the failed / base run's post graph); masks, bits and depths are ragged,
// entry e's slice starts at off[e] (off[n] = the sum of the entries' nodes).
struct SdiffArgs {
  const uint32_t *graph;    // [entries] the entry's graph gf
  const uint64_t *off;      // [entries + 1] first node of the entry's slices
  const uint32_t *r0hkey;   // run 0's post-goal labels, open-addressed: key = label + 1 (0 empty)
  uint32_t r0hmask;         // table size - 1 (power of two)
  const LabTab *tabs;       // [entries] the pairs call: entry e probes tabs[e] (null: every entry the run-0 table)
  uint8_t *bits;            // [off[n]] node bits of the global tier (null: no such entry)
  int32_t *depth;           // [off[n]] depths (both tiers; only S nodes touch them)
  uint8_t *mask;            // [off[n]] S masks (output)
  uint32_t *rows;           // [2 * off[n]] (entry, rule local to gf)
  uint32_t *n_rows;         // counter
};

// One nemo_nearest_runs call (k_near.hip): a bit row of W u64 words per distinct run of the call (bit
// `label` set for every goal label of its post graph), and the n_q x n_c matrix over list positions.
struct NearArgs {
  const uint32_t *row_graph;  // [rows] the post graph of each bit row
  uint64_t *bits;             // [rows][W], 16-byte aligned rows (W is even)
  uint32_t *size;             // [rows] |L(r)|: the distinct goal labels
  uint32_t rows;
  uint64_t W;
  const uint32_t *qrow, *crow;  // [n_q], [n_c] the bit row of every query / candidate position
  uint32_t n_q, n_c;
  uint32_t *mat;              // [n_q][n_c] intersection counts (zeroed per call under split-K), then distances
  uint32_t *out;              // [n_q][4] nemo_nearest rows: cand, dist, only_query, only_cand
};

// One nemo_knockout_leaves / nemo_knockout_sets call (k_knock.hip): hypotheses in chunks of 64 per graph
// (knock_host.h Chunk, passed as raw 32-byte rows), one bit column per hypothesis in a u64 dead word per node.
struct KnockArgs {
  const uint32_t *list;     // leaves mode: [n_list] the listed graphs
  const uint32_t *loff;     // leaves mode: [n_list + 1] first hypothesis of each list position
  uint32_t *cnt;            // leaves mode: [n_list][2] sink goals and Kahn levels of each listed graph (k_ko_leaves)
  uint32_t n_list;
  const uint4 *chunk;       // [chunks][2] the chunk table
  const uint32_t *sel;      // the launched tier's chunk indices
  uint32_t *leaf;           // leaves mode: [hypotheses] the sink goal of each; sets mode: the sets' nodes
  const uint64_t *set_off;  // sets mode: [sets + 1] offsets into leaf (null: leaves mode)
  uint64_t *dead;           // dead words of the chunks that keep them
  uint32_t *rows;           // [hypotheses][5] nemo_knock
  uint32_t masks;           // 1: every chunk stores its dead words at its moff
};
// k_ko_leaves: write false counts (a.cnt), true lists the sink goals at a.loff (a.leaf)
void launch_ko_leaves(const DevCorpus &c, const KnockArgs &a, bool write, hipStream_t s);
// a.sel: n chunk indices of one tier; lds_bytes: the largest image among them (k_ko_lds's dynamic LDS)
void launch_ko_lds(const DevCorpus &c, const KnockArgs &a, uint32_t n, uint32_t lds_bytes, hipStream_t s);
void launch_ko_glob(const DevCorpus &c, const KnockArgs &a, uint32_t n, hipStream_t s);

// One round of nemo_min_cuts (k_cuts.hip): the hypotheses of the round are the sets of `size` live positions,
// in colex rank order (cut_host.h), 64 consecutive ranks per chunk, one u64 result word per chunk.
struct CutArgs {
  uint32_t graph;           // 2r + cond
  uint32_t size;            // 1..3: the round
  uint32_t n_hyp, n_chunks;
  const uint32_t *cand;     // [K] candidate position -> node
  const uint32_t *live;     // [K1] live position -> candidate position (null in round 1: every candidate is live)
  const uint32_t *lnode;    // [K1] live position -> node: cand[live[p]], as the sweeps read it
  uint64_t *words;          // [n_chunks] bit t of word k: hypothesis 64 k + t is a minimal cut
  const uint64_t *pairs;    // round 3: round 2's words (a lost pair is a minimal one: bit C(y,2) + x)
  uint64_t *dead;           // k_cut_glob: [workgroups][dead_words(V)]
  uint32_t *scan;           // [n_chunks + 1] popcounts of the words, then their exclusive scan; [n_chunks] = total
  uint32_t *rows;           // k_cut_emit: the round's first nemo_cut row (4 u32 each)
};
// the workgroups of round `size`'s k_cut_lds resident on the device at lds_bytes of dynamic LDS (0: the query failed)
uint32_t cut_lds_resident(uint32_t size, uint32_t lds_bytes, uint32_t n_cu);
void launch_cut_lds(const DevCorpus &c, const CutArgs &a, uint32_t grid, uint32_t lds_bytes, hipStream_t s);
void launch_cut_glob(const DevCorpus &c, const CutArgs &a, uint32_t grid, hipStream_t s);
void launch_cut_count(const CutArgs &a, hipStream_t s);  // a.scan[k] = popcount(a.words[k]), a.scan[n_chunks] = 0
void launch_cut_emit(const CutArgs &a, hipStream_t s);   // the rows of the round's set bits at a.rows, by a.scan

// One round of nemo_min_repair_sets / nemo_min_repairs (k_repair.hip): a round of CutArgs read as "repair" (bit t of
// word k: restoring hypothesis 64 k + t's nodes lets the outcome hold; round 3: and none of its pairs does), over
// the absent bitmap.  c.size 0 is round 0: one chunk of two hypotheses, S = {} and S = every candidate.
struct RepairArgs {
  CutArgs c;
  const uint64_t *absent;   // [repair::bitmap_words(V)] bit v: node v is assumed lost; the bits past V are 0
  uint32_t n_cand;          // round 0: the candidates c.cand[0 .. n_cand)
};
// the workgroups of round `size`'s (0..3) k_repair_lds resident on the device at lds_bytes of dynamic LDS (0: the query failed)
uint32_t repair_lds_resident(uint32_t size, uint32_t lds_bytes, uint32_t n_cu);
void launch_repair_lds(const DevCorpus &c, const RepairArgs &a, uint32_t grid, uint32_t lds_bytes, hipStream_t s);
void launch_repair_glob(const DevCorpus &c, const RepairArgs &a, uint32_t grid, hipStream_t s);
// k_repair_absent: graph's sink goals whose label misses the table (key, mask: LabTab's layout), in node order at
// cand[0 .. V) and as the bitmap `absent`; cnt[0] = how many, cnt[1] = the graph's Kahn levels
void launch_repair_absent(const DevCorpus &c, uint32_t graph, const uint32_t *key, uint32_t mask, uint64_t *absent, uint32_t *cand,
                          uint32_t *cnt, hipStream_t s);

// One nemo_knockout_labels call (k_klabel.hip): hypotheses are label sets in chunks of 64, shared by every listed
// graph; table c (c < n_chunks) maps a label to the mask of chunk c's sets that name it, table n_chunks is the
// union filter of all named labels (klabel_host.h: key = label + 1, 0 empty, linear probing).
struct KlArgs {
  const uint64_t *set_off;   // [n_sets + 1] offsets into labels (k_kl_tables)
  const uint32_t *labels;    // the sets' labels
  uint32_t n_sets, n_chunks;
  const uint64_t *tab_off;   // [n_chunks + 2] first slot of every table
  uint32_t *key;             // [tab_off[n_chunks + 1]] the tables' keys
  uint64_t *mask;            // ... and masks (the union filter's stay unused)
  const uint32_t *graph;     // [n] list position -> graph
  const uint32_t *pos;       // [n_tier] the launched tier's list positions
  uint32_t n_tier;           // list positions of the launched tier
  uint32_t parts;            // chunk ranges per graph (klabel::split)
  uint32_t sinks;            // 1: only sink goals match (NEMO_KL_SINKS)
  uint32_t no_list;          // 1: k_kl_lds without the hit list, V probes per chunk (option kl_hitlist 0)
  uint32_t lds_total;        // k_kl_lds: the launch's dynamic LDS; what the image leaves holds the hit list's head
  uint64_t *region;          // [workgroups][region_words] hit-list spill (and k_kl_glob's dead words)
  uint64_t region_words;     // u64 per workgroup
  uint64_t dead_words;       // k_kl_glob: dead words at the region's start (the hit list follows)
  uint64_t *out;             // [n][n_chunks][2] (lost, hit)
  uint32_t n;                // list positions of the call (k_kl_count)
  uint32_t *cnt;             // k_kl_count: [n_chunks * 64] n_lost | [n_chunks * 64] n_hit
};
void launch_kl_tables(const KlArgs &a, hipStream_t s);
// the workgroups of k_kl_lds resident on the device at lds_bytes of dynamic LDS (0: the query failed)
uint32_t kl_lds_resident(uint32_t lds_bytes, uint32_t n_cu, bool list = true);
void launch_kl_lds(const DevCorpus &c, const KlArgs &a, uint32_t grid, hipStream_t s);  // a.lds_total bytes of LDS
void launch_kl_glob(const DevCorpus &c, const KlArgs &a, uint32_t grid, hipStream_t s);
void launch_kl_count(const KlArgs &a, hipStream_t s);

// One round of nemo_min_label_cuts (k_lcuts.hip): the hypotheses are the sets of `size` live candidate positions in
// colex rank order (cut_host.h), shared by every listed graph; one lost word per (list position, chunk of 64 ranks).
struct LcArgs {
  const uint32_t *cand;      // [n_cand] candidate position -> label
  uint32_t n_cand;
  uint32_t *key, *val;       // [slots] the call's table: label + 1 -> candidate position (klabel_host.h's hash)
  uint64_t slots;
  const uint32_t *lmap;      // [n_cand] candidate position -> live position of this round (UINT32_MAX: not live)
  uint32_t k1;               // live positions of this round
  uint32_t size;             // 1..3: the round
  uint32_t n_hyp, n_chunks;
  const uint32_t *graph;     // [n] list position -> graph
  const uint32_t *pos;       // [n_tier] the launched tier's list positions
  uint32_t n_tier;           // list positions of the launched tier
  uint32_t parts;            // chunk ranges per graph (klabel::split)
  uint32_t sinks;            // 1: only sink goals match (NEMO_KL_SINKS)
  uint32_t lds_total;        // k_lc_lds: the launch's dynamic LDS; what the image leaves holds the hit list's head
  uint64_t *region;          // [workgroups][region_words] the hit list's rest (and k_lc_glob's dead words)
  uint64_t region_words;     // u64 per workgroup
  uint64_t dead_words;       // k_lc_glob: dead words at the region's start (the hit list follows)
  uint64_t *lost;            // [n][n_chunks] the round's lost words
  uint64_t *hit;             // round 1: [n][n_chunks] hit words
  uint32_t n, q;             // list positions of the call; a cut is lost on at least q of them
  uint64_t *words;           // k_lc_reduce: [n_chunks] cut words (round 1: then [n_chunks] any-hit words)
  const uint64_t *pairs;     // round 3: round 2's cut words
  const uint32_t *scan;      // k_lc_support: [n_chunks + 1] the round's first rows (CutArgs::scan)
  uint32_t n_rows;           // ... the round's rows
  uint32_t *n_lost;          // ... [n_rows] lost_count of each
};
void launch_lc_table(const LcArgs &a, hipStream_t s);  // the table is zero
// the workgroups of round `size`'s k_lc_lds resident on the device at lds_bytes of dynamic LDS (0: the query failed)
uint32_t lc_lds_resident(uint32_t size, uint32_t lds_bytes, uint32_t n_cu);
void launch_lc_lds(const DevCorpus &c, const LcArgs &a, uint32_t grid, hipStream_t s);  // a.lds_total bytes of LDS
void launch_lc_glob(const DevCorpus &c, const LcArgs &a, uint32_t grid, hipStream_t s);
void launch_lc_reduce(const LcArgs &a, hipStream_t s);
void launch_lc_support(const LcArgs &a, hipStream_t s);

// One round of nemo_min_group_cuts (k_gcuts.hip): a candidate is a group of labels, a hypothesis the set of `size`
// live candidate positions of colex rank h, which removes the union of its groups.  `r` is the round as
// nemo_min_label_cuts' kernels read it (k_lc_reduce and k_lc_support take it as it is; of its fields the sweeps
// leave cand, n_cand, lmap and k1 alone: r.key / r.val / r.slots is the table label + 1 -> row of the n_dist
// distinct labels the groups name).
struct GcArgs {
  LcArgs r;
  const uint32_t *goff;      // [n_groups + 1] candidate position -> its first entry in grow
  uint32_t *grow;            // [n_named] the groups' labels (k_gc_table reads them), then their rows (k_gc_rows, in place)
  uint32_t n_named, n_dist;
  uint32_t *n_rows;          // k_gc_table: the rows handed out so far (zeroed); n_dist at its end
  const uint32_t *live;      // [K1] live position -> candidate position (null in round 1: every candidate is live)
};
void launch_gc_table(const GcArgs &a, hipStream_t s);  // the table and *n_rows are zero
void launch_gc_rows(const GcArgs &a, hipStream_t s);
// the workgroups of round `size`'s k_gc_lds resident on the device at lds_bytes of dynamic LDS (0: the query failed)
uint32_t gc_lds_resident(uint32_t size, uint32_t lds_bytes, uint32_t n_cu);
void launch_gc_lds(const DevCorpus &c, const GcArgs &a, uint32_t grid, hipStream_t s);  // a.r.lds_total bytes of LDS
void launch_gc_glob(const DevCorpus &c, const GcArgs &a, uint32_t grid, hipStream_t s);

// One nemo_witness_sets / nemo_witness_labels call (k_witness.hip): the sets, in chunks of 64, are shared by every
// listed graph (the node-set form lists one); hypothesis pos * n_sets + s is set s on list position pos.  A set's
// entries are nodes (k1 == 0) or rows of the k1 distinct labels the sets name (the label form: key / val is the
// table label + 1 -> row, klabel_host.h's hash).
struct WitArgs {
  const uint64_t *set_off;   // [n_sets + 1] offsets into ent
  const uint32_t *ent;       // the sets' entries
  uint32_t n_sets, n_chunks;
  uint32_t k1;               // the label form: distinct labels (rows of a graph's hit list); 0: the entries are nodes
  const uint32_t *dist;      // [k1] row -> label (k_wit_table)
  uint32_t *key, *val;       // [slots] the table
  uint64_t slots;
  const uint32_t *graph;     // [n] list position -> graph
  const uint32_t *pos;       // [n_tier] the launched tier's list positions
  uint32_t n_tier;           // list positions of the launched tier
  uint32_t parts;            // chunk ranges per graph (klabel::split)
  uint32_t sinks;            // 1: only sink goals match a label (NEMO_WIT_SINKS)
  uint32_t all;              // 1: a needed goal needs every alive child (NEMO_WIT_ALL)
  uint32_t lds_total;        // k_wit_lds: the launch's dynamic LDS; what the image leaves holds the hit list's head
  uint64_t *region;          // [workgroups][region_words] k_wit_glob's dead and need words, the hit list's rest
  uint64_t region_words;     // u64 per workgroup
  uint64_t glob_words;       // k_wit_glob: dead words, then need words at the region's start (the hit list follows)
  uint32_t *rows;            // [n][n_sets][5] nemo_witness
  uint64_t *need;            // NEMO_WIT_MASKS: the kept need words (null: none)
  const uint64_t *moff;      // ... [n] list position -> its first word; chunk c's at c * dead_words(V)
};
void launch_wit_table(const WitArgs &a, hipStream_t s);  // the table is zero
// the workgroups of k_wit_lds resident on the device at lds_bytes of dynamic LDS (0: the query failed)
uint32_t wit_lds_resident(uint32_t lds_bytes, uint32_t n_cu);
void launch_wit_lds(const DevCorpus &c, const WitArgs &a, uint32_t grid, hipStream_t s);  // a.lds_total bytes of LDS
void launch_wit_glob(const DevCorpus &c, const WitArgs &a, uint32_t grid, hipStream_t s);

// One level of nemo_lineage_cuts (k_lineage.hip): the frontier's sets, 64 per chunk, are evaluated on the one graph
// (k_lin_lds / k_lin_glob), which appends the lost ones to the cuts and emits the children of the others; k_lin_filter
// makes the next frontier of the children.  A set is a key of two u64 (lin_host.h).
struct LinArgs {
  uint32_t graph;            // 2r + cond
  const uint32_t *cand;      // [K] candidate position -> node
  uint32_t K;
  const uint64_t *front;     // [n_front][2] the level's sets
  uint32_t n_front, n_chunks;
  uint32_t emit;             // 0: the last level, no children; 1: emit them
  uint32_t redo;             // 1: the level runs again behind a grown emission buffer: its cuts are in place
  uint64_t *kids;            // [kids_cap][2] the emitted children
  uint64_t kids_cap;
  uint64_t *cuts;            // [...][2] the cuts found so far, this level's behind them
  uint32_t *ctab;            // [cslots] the cuts' table: index + 1, 0 = empty
  uint64_t cslots;
  unsigned long long *ctr;   // [0] cuts so far | [1] children counted (not capped) | [2] the next frontier's sets
  uint32_t lds_total;        // k_lin_lds: the launch's dynamic LDS
  uint64_t *region;          // k_lin_glob: [workgroups][region_words] dead words, then need words
  uint64_t region_words;
  // k_lin_filter
  uint32_t *ktab;            // [kslots] the children's table, zero
  uint64_t kslots;
  uint64_t *next;            // [...][2] the next frontier (as many sets as kids_cap)
  uint32_t cut_sizes;        // bit s: a cut of size s was found at an earlier level
  uint32_t size;             // the level: the sets' size
  uint64_t cuts_before;      // cuts before this level
};
uint32_t lin_lds_resident(uint32_t lds_bytes, uint32_t n_cu);
void launch_lin_lds(const DevCorpus &c, const LinArgs &a, uint32_t grid, hipStream_t s);  // a.lds_total bytes of LDS
void launch_lin_glob(const DevCorpus &c, const LinArgs &a, uint32_t grid, hipStream_t s);
void launch_lin_filter(const LinArgs &a, uint32_t grid, hipStream_t s);
// the cuts [0, n) into a zeroed table (behind a grown list)
void launch_lin_rehash(const LinArgs &a, uint64_t n, hipStream_t s);

// One level of nemo_lineage_group_cuts (k_lgcuts.hip): the frontier's sets of candidate positions, 64 per chunk, are
// evaluated on every listed graph (k_lgc_lds / k_lgc_glob: a lost word per (list position, chunk), the children of the
// sets that are not lost); k_lgc_cuts counts a set's lost bits down the list positions and appends the cuts;
// k_lin_filter (on `l`) makes the next frontier.  `l` is the level as nemo_lineage_cuts' kernels read it: of its
// fields the evaluation leaves graph, cand and redo alone; l.K is the number of groups.
struct LgcArgs {
  LinArgs l;
  const uint32_t *goff;      // [K + 1] candidate position -> its first entry in grow
  const uint32_t *grow;      // the groups' labels as rows of the n_dist distinct labels (k_gc_table / k_gc_rows)
  uint32_t n_dist;
  const uint32_t *key, *val; // [slots] the table label + 1 -> row (klabel_host.h's hash)
  uint64_t slots;
  const uint32_t *graph;     // [n] list position -> graph
  const uint32_t *pos;       // [n_tier] the launched tier's list positions
  uint32_t n_tier;           // list positions of the launched tier
  uint32_t parts;            // chunk ranges per graph (klabel::split)
  uint32_t sinks;            // 1: only sink goals match a label (NEMO_KL_SINKS)
  uint64_t glob_words;       // k_lgc_glob: dead words, then need words at the region's start
  uint64_t *lost;            // [n][n_chunks] the level's lost words
  uint32_t n, q;             // list positions of the call; a cut is lost on at least q of them
  uint32_t *n_lost;          // k_lgc_cuts: [...] lost_count of each cut, beside l.cuts
};
uint32_t lgc_lds_resident(uint32_t lds_bytes, uint32_t n_cu);
void launch_lgc_lds(const DevCorpus &c, const LgcArgs &a, uint32_t grid, hipStream_t s);  // a.l.lds_total bytes of LDS
void launch_lgc_glob(const DevCorpus &c, const LgcArgs &a, uint32_t grid, hipStream_t s);
void launch_lgc_cuts(const LgcArgs &a, hipStream_t s);

// One level of nemo_lineage_repair_sets / nemo_lineage_repairs (k_lrepair.hip): the frontier's sets of candidate
// positions, 64 per chunk, are evaluated on the one graph under the absent bitmap (k_lrep_lds / k_lrep_glob), which
// appends the holding ones to the repairs and emits the children of the others; k_lin_filter and k_lin_rehash (on `l`)
// make the next frontier and the repairs' table.  `l` is the level as nemo_lineage_cuts' kernels read it, with "cut"
// read as "repair"; l.region holds three word arrays per workgroup (lrep_host.h).
struct LrepArgs {
  LinArgs l;
  const uint64_t *absent;    // [repair::bitmap_words(V)] bit v: node v is assumed lost; the bits past V are 0
  uint32_t status;           // 1: one workgroup, two hypotheses (S = {}, S = every candidate); l.ctr[3] = their lost word
};
uint32_t lrep_lds_resident(uint32_t lds_bytes, uint32_t n_cu);
void launch_lrep_lds(const DevCorpus &c, const LrepArgs &a, uint32_t grid, hipStream_t s);  // a.l.lds_total bytes of LDS
void launch_lrep_glob(const DevCorpus &c, const LrepArgs &a, uint32_t grid, hipStream_t s);

// One nemo_diff_classes call (k_dclass.hip) over the D masks of the nu distinct label sources.
struct DclassArgs {
  const uint8_t *mask;      // [n_entries][V0] D masks (the buffer ends on a 16-byte boundary)
  uint64_t V0;
  const uint32_t *row;      // [nu] the entry whose row is source u's mask (DxArgs::urep)
  const uint32_t *weight;   // [nu] entries of source u
  uint32_t nu;
  uint32_t rows_per_block;  // rows per k_dclass_hash workgroup (dclass_rows_per_block)
  uint64_t *hash;           // [nu][2] membership hash, summed over column tiles (zeroed per call)
  uint32_t *pop;            // [nu] |D| (zeroed per call)
  uint32_t *support;        // [V0] entries whose D holds the node (zeroed per call)
};

struct PullArgs {
  uint32_t which;           // 0 raw, 1 simplified, 2 diff, 3 symmetric diff
  uint32_t g0;              // graph of which == 2
  const uint32_t *slot_g;   // which == 3: slot -> its graph (the entry's failed post graph); which 0 / 1: one graph
                            // per duplicate-graph class (gdedup::pull_plan; null: slot g is graph g)
  const uint8_t *mask;      // which >= 2: D / S masks of the entries
  uint64_t mask_stride;     // which == 2: bytes between two entries' masks
  const uint64_t *mask_off; // which == 3: first mask byte of every slot (ragged masks)
  const uint32_t *mask_row; // which == 2: slot -> the entry whose mask it takes (null: the slot's own)
  uint32_t *cnt;            // [slots] edges of the slot
  uint64_t *off;            // [slots] first edge of the slot in src/dst
  unsigned long long *cursor;  // region allocator (zeroed before the launch)
  uint64_t cap;             // capacity of src/dst
  uint32_t *src, *dst;      // output
  // big slots (graph of >= NEMO_CSR_BIG nodes): multi-workgroup pull over
  // MWP_CH-node chunks, [row slots][maxck] chunk counts -> offsets (null: none)
  uint32_t *ccnt;
  uint32_t maxck;
  const uint32_t *big_slot;  // which 0 / 1 with slot_g: slot of big graph DevCorpus::big[y] (chunk-table row y)
};

struct TrigArgs {
  uint32_t g_pre, g_post;
  uint32_t *counts;         // [3] pre rows, post rows, async rules
  uint32_t *pre, *post, *async_rules;
};

__host__ __device__ uint32_t build_tier_bytes(uint32_t v, uint32_t e);
// entries the device copies of the edge arrays and the node words end with: k_build's 16-byte input
// loads at an index clamped to a graph's end read up to this many entries past the last graph
#define NEMO_IN_PAD 4
void launch_build(const DevCorpus &c, hipStream_t s);
void launch_load(const DevCorpus &c, hipStream_t s);
void launch_topo(const DevCorpus &c, hipStream_t s, bool list = true);
void launch_csr_big(const DevCorpus &c, uint32_t chunks, hipStream_t s);
// per_graph false: no graph below NEMO_CSR_BIG is past the skipped tier (host count), so only the big-graph kernels run
void launch_mark(const DevCorpus &c, bool skip_tier, hipStream_t s, bool per_graph = true);
void launch_simplify(const DevCorpus &c, bool skip_tier, hipStream_t s, bool per_graph = true);
void launch_marksimp(const DevCorpus &c, hipStream_t s, bool skip_built);
// dd_pairs: the duplicate graphs' (dup, rep) pairs, replicated behind the first tier when c.dd_list is set
void launch_chains(const DevCorpus &c, hipStream_t s, bool tiers = true, const uint32_t *dd_pairs = nullptr,
                   uint32_t dd_npairs = 0);
// duplicate graphs (k_gdedup.hip): content hashes [2 G] and exact comparisons at load; k_replicate
// copies what `phase` wrote for each pair's representative to its duplicate
#define GD_BUILD 0
#define GD_MARKSIMP 1
#define GD_CHAINS 2
#define GD_BUILD_SCALARS 3  // GD_BUILD's per-graph scalars alone (redo, err, created, nlev)
#define GD_BUILD_SLICES 4   // ... and its slices alone (ensure_whole, ctx.h)
void launch_gd_hash(const DevCorpus &c, uint64_t *hash, hipStream_t s);
void launch_gd_cmp(const DevCorpus &c, const uint32_t *pairs, uint32_t n_pairs, uint8_t *verdict, hipStream_t s);
void launch_replicate(const DevCorpus &c, const uint32_t *pairs, uint32_t n_pairs, int phase, hipStream_t s);
void launch_chains_glob(const DevCorpus &c, hipStream_t s);
uint64_t glob_words(uint64_t V, uint64_t E);  // k_chains_glob scratch of one graph (u32)
uint32_t glob_team_words();                   // k_glob_prep's team scratch (u32)
void launch_proto(const DevCorpus &c, hipStream_t s, bool tiers = true);
void launch_reduce(const DevCorpus &c, const uint8_t *is_success, const uint8_t *owned, uint32_t first_run,
                   uint32_t *red, hipStream_t s);
void launch_diff(const DevCorpus &c, const DiffArgs &a, uint32_t n_entries, uint32_t V0, hipStream_t s);
// entry e's D mask = unique result map[e]'s ([n_entries][V0] from [n_uniq][V0])
void launch_diff_expand(uint8_t *mask, const uint8_t *umask, const uint32_t *map, uint64_t V0, uint32_t n_entries,
                        hipStream_t s);
// n_lds / n_glob: entries inside / past k_diff_lds's caps (host counts; an empty tier is not launched)
void launch_sdiff(const DevCorpus &c, const SdiffArgs &a, uint32_t n_entries, uint32_t n_lds, uint32_t n_glob,
                  hipStream_t s);
// tabs[t].key of every table filled from the goals of tabs[t].graph: tables of at most lds_max
// slots are built in LDS (0: none; lds_slots: the largest of them, the launch's LDS size), the
// others in place
#define LAB_HASH_LDS_SLOTS 16384u  // the LDS path's budget: 64 KB, two workgroups per CU
void launch_lab_hash(const DevCorpus &c, const LabTab *tabs, uint32_t n_tabs, uint32_t lds_max, uint32_t lds_slots,
                     hipStream_t s);
// nemo_nearest_runs (k_near.hip).  lmax: the largest goal label of the post graphs, atomicMax'ed into a
// zeroed word by `parts` workgroups per run; bit rows of at most lds_max bytes are built in LDS, larger
// ones in place; the tile / split-K grid is nearest_host.h's
void launch_near_lmax(const DevCorpus &c, uint32_t parts, uint32_t *lmax, hipStream_t s);
void launch_near_bits(const DevCorpus &c, const NearArgs &a, uint32_t lds_max, hipStream_t s);
void launch_near_isect(const NearArgs &a, uint64_t tq, uint64_t tc, uint32_t slabs, uint32_t slabs_per_split,
                       uint32_t ksplit, hipStream_t s);
void launch_near_pick(const NearArgs &a, hipStream_t s);
uint32_t dclass_rows_per_block(uint64_t V0, uint32_t nu);
void launch_dclass_hash(const DclassArgs &a, hipStream_t s);
// verdict[k] = 1 iff rows pairs[2k] and pairs[2k + 1] (sources) have the same membership at every node
void launch_dclass_cmp(const DclassArgs &a, const uint32_t *pairs, uint32_t n_pairs, uint8_t *verdict, hipStream_t s);
void launch_dx_prep(const DevCorpus &c, const DxPrep &p, uint32_t *tsum, hipStream_t s);
void launch_dx(const DevCorpus &c, const DxArgs &a, hipStream_t s);
uint32_t dx_max_row();       // the longest row of g0 the multi-entry diff takes
uint32_t dx_max_row_tiny();  // the same under the tiny-window test knob
// window configurations of the two walk images for g0 (V0, E0) under the test knob `window`
void dx_img_configs(uint32_t V0, uint32_t E0, uint32_t window, DxImg out[2]);
void launch_dx_img(const DxPrep &p, DxImg img[2], const DxImgScratch &t, hipStream_t s);
uint32_t dx_scan_tiles(uint32_t n);  // tile sums launch_scan needs for n entries
void launch_scan(uint32_t *a, uint32_t n, uint32_t *tsum, hipStream_t s);  // in-place exclusive scan
// rest: graphs (which 0/1) or g0 (which 2) past k_pull_lds's LDS tier, counted on the host
void launch_pull(const DevCorpus &c, const PullArgs &a, uint32_t slots, uint32_t rest, hipStream_t s);
// the pairs with index in [lo, hi), hi at most the capacity of `out` in pairs
void launch_chain_pairs(const DevCorpus &c, const uint64_t *off, uint32_t *out, uint64_t lo, uint64_t hi, int wide,
                        hipStream_t s);
// the state's words [w0, w0 + nw)
void launch_pack_state(const uint8_t *flags, uint32_t *out, uint64_t V, uint64_t w0, uint64_t nw, hipStream_t s);
void launch_chain_gather(const DevCorpus &c, uint64_t *off, uint32_t *out, hipStream_t s);
void launch_triggers(const DevCorpus &c, const TrigArgs &a, int phase, hipStream_t s);
void launch_goal_labels(const DevCorpus &c, uint32_t g, uint32_t *out, hipStream_t s);
void launch_to_host(void *dst, const void *src, uint64_t bytes, hipStream_t s, uint32_t max_blocks = 64);
struct HostCopy {
  uint8_t *dst;
  const uint8_t *src;
  uint64_t n;
};
struct HostCopies {  // up to four copies by one k_to_host_multi launch
  HostCopy seg[4];
  uint32_t n = 0;
  void add(void *d, const void *s, uint64_t bytes) {
    if (bytes) seg[n++] = {(uint8_t *)d, (const uint8_t *)s, bytes};
  }
};
void launch_to_host_multi(const HostCopies &h, hipStream_t s);
void launch_zero(void *dst, uint64_t bytes, hipStream_t s);

}  // namespace nemo
