// k_sdiff.hip — symmetric differential provenance ("bad - good"): the part of
// a failed run's own consequent provenance that the good run 0 lacks.  It is
// the export query (differential-provenance.go:22-28) and the leaf query
// (:82-98) with the two runs' roles exchanged; the reference names the
// capability (`symmetric`, :18) and never built it, so DESIGN.md §Symmetric
// diff fixes the semantics.
//
// Every entry walks its OWN graph gf (the failed run's raw post graph), so the
// shape is "one workgroup per graph, one launch over all entries" (k_marksimp,
// k_proto_lds, k_pull_lds); the only shared data is the hash of run 0's
// post-goal labels the load builds.
//
// nemo_diffprov_pairs is the same walk with the run compared against chosen per
// entry: entry e walks its base run's post graph against the label hash of its
// `other` run, which k_lab_hash (below) builds once per distinct `other` run.
//
// The kernels here pick the tier, stage the image and seed the Bad goals (sdiff_mark_bad); the
// level sweeps and the tail are diff_walk's (diff_walk.h, shared with k_diff_lds), where S is DB_D.
#include "device.h"
#include "diff_walk.h"
#include "internal.h"

namespace nemo {

// Bad_e: the goals of gf whose label misses the run-0 label hash.  Each thread
// takes SD_BATCH nodes and walks their probe sequences together (as
// diff_fail_goals does), so a pass is a few rounds of independent loads.
// RULES: the same pass ballots the rule bits into the LDS rule bitmap (64
// consecutive nodes per wave and q: two plain word stores, no atomics).
// The table is the entry's: the pairs call's tabs[e] (TABS), else the run-0 table; the base and
// the mask are read once per workgroup at a uniform address.  TABS is a template parameter so that
// the symmetric call's kernels are the code they were before tabs existed.
#define SD_BATCH 8
#define SD_GLOBAL __attribute__((address_space(1)))
template <int B, bool RULES, bool TABS>
__device__ __forceinline__ void sdiff_mark_bad(const SdiffArgs &a, uint32_t e, const GraphView &gv, uint8_t *bits,
                                               uint32_t *rule) {
  // (a pointer read from memory is a generic one to the compiler: named global here, so that the
  // probes stay the global loads they are with the kernel argument)
  const SD_GLOBAL uint32_t *hkey = (const SD_GLOBAL uint32_t *)a.r0hkey;
  uint32_t hmask = a.r0hmask;
  if (TABS) {
    hkey = (const SD_GLOBAL uint32_t *)a.tabs[e].key;
    hmask = a.tabs[e].mask;
  }
  for (uint32_t base = 0; base < gv.V; base += SD_BATCH * B) {
    uint32_t lab[SD_BATCH], h[SD_BATCH], live = 0, bad = 0;
#pragma unroll
    for (int q = 0; q < SD_BATCH; q++) {
      const uint32_t x = base + q * B + threadIdx.x;
      const bool in = x < gv.V;
      const bool rl = in && is_rule(gv.word[x]);
      if (RULES) {
        const uint64_t m = __ballot(rl);
        const uint32_t n0 = base + q * B + (threadIdx.x & ~63u);
        if (lane_id() == 0 && n0 < gv.V) {  // both words lie inside the bitmap's 16-byte padded region
          rule[n0 >> 5] = (uint32_t)m;
          rule[(n0 >> 5) + 1u] = (uint32_t)(m >> 32);
        }
      }
      lab[q] = in && !rl ? gv.label[x] : 0u;
      h[q] = hash_label(lab[q]) & hmask;
      live |= (in && !rl ? 1u : 0u) << q;
    }
    while (live) {
      uint32_t k[SD_BATCH];
#pragma unroll
      for (int q = 0; q < SD_BATCH; q++) k[q] = ((live >> q) & 1u) ? hkey[h[q]] : 0u;
#pragma unroll
      for (int q = 0; q < SD_BATCH; q++) {
        if (!((live >> q) & 1u)) continue;
        if (k[q] == lab[q] + 1u) {
          live &= ~(1u << q);  // a post-goal label of the run compared with
        } else if (k[q] == 0u) {
          bad |= 1u << q;
          live &= ~(1u << q);
        } else {
          h[q] = (h[q] + 1u) & hmask;
        }
      }
    }
#pragma unroll
    for (int q = 0; q < SD_BATCH; q++) {
      const uint32_t x = base + q * B + threadIdx.x;
      if (x < gv.V) bits[x] = ((bad >> q) & 1u) ? DB_BAD : 0u;
    }
  }
}

// LDS tier: entries whose graph is inside k_diff_lds's caps (t_diff), walked
// over diff_carve's image.  Depths (< V <= 16384) live in LDS
// as u16 behind the image (DLDS) when the 2V bytes they add leave the
// workgroups per CU of 160 KB LDS unchanged, and otherwise in HBM, in the
// entry's slice of the per-call scratch (only S nodes touch them).  At the C3
// shape (caps V 5005, E 7463) the image is 55.5 KB and 65.5 KB with the
// depths: two workgroups per CU either way, so the depths are in LDS there.
__host__ __device__ __forceinline__ uint32_t sdiff_depth_bytes(uint32_t v) { return lds_align(2u * v); }
#define SDIFF_CU_LDS (160u * 1024u)
template <bool DLDS, bool TABS>
__global__ __launch_bounds__(NEMO_BLOCK) void k_sdiff_lds(DevCorpus c, SdiffArgs a) {
  extern __shared__ __align__(16) uint8_t dyn[];
  const uint32_t e = blockIdx.x;
  const GraphView gv = c.view(a.graph[e]);
  if (!tier_fits(c.t_diff, gv.V, gv.E, gv.nlev)) return;  // k_sdiff_glob's entry
  const uint32_t V = gv.V;
  DiffLds L = diff_carve(dyn, V, gv.E);
  {
    const StageDesc d[4] = {{gv.rp, L.rp, V + 1, ST_U16}, {gv.fp, L.fp, V + 1, ST_U16},
                            {gv.rc, L.rc, gv.E, ST_U16},  {gv.fc, L.fc, gv.E, ST_U16}};
    stage_lds<4, NEMO_BLOCK>(d);
  }
  sdiff_mark_bad<NEMO_BLOCK, true, TABS>(a, e, gv, L.bits, L.rule);
  const DiffOut o{a.mask + a.off[e], a.rows, a.n_rows, e};
  // the LDS depths sit behind the image of the tier's caps, so their offset does not depend on the graph
  if constexpr (DLDS)
    diff_walk<NEMO_BLOCK, WF_NONE, true>(gv, L, L.bits, reinterpret_cast<uint16_t *>(dyn + c.t_diff.bytes), o);
  else
    diff_walk<NEMO_BLOCK, WF_DEPTH, true>(gv, L, L.bits, a.depth + a.off[e], o);
}

// Global tier: every other entry (graphs past t_diff's caps, u32 rows of graphs
// of >= 65536 nodes, and every entry under option graph_lds_max 0).  One
// workgroup per entry sweeps the Kahn levels over the HBM CSR; node bits and
// depths live in the entry's slice of the per-call scratch, so every store of
// the walk is fenced before the barrier that follows it (WF_ALL).  Correct, not tuned.
template <int B, bool TABS>
__global__ __launch_bounds__(B) void k_sdiff_glob(DevCorpus c, SdiffArgs a) {
  const uint32_t e = blockIdx.x;
  const GraphView gv = c.view(a.graph[e]);
  if (tier_fits(c.t_diff, gv.V, gv.E, gv.nlev)) return;  // k_sdiff_lds's entry
  uint8_t *bits = a.bits + a.off[e];
  sdiff_mark_bad<B, false, TABS>(a, e, gv, bits, nullptr);
  diff_walk<B, WF_ALL, true>(gv, DiffGlob{gv.rp, gv.fp, gv.rc, gv.fc, gv.word}, bits, a.depth + a.off[e],
                             DiffOut{a.mask + a.off[e], a.rows, a.n_rows, e});
}

// ---- per-run label hash tables (nemo_diffprov_pairs; DESIGN.md §Pair diff) ----------------------
// One workgroup per distinct `other` run fills that run's table from the goals of its post graph:
// key = label + 1 at slot hash_label(label) & mask, linear probing, the layout sdiff_mark_bad
// probes.  A slot is claimed by compare-and-swap against 0, and a label some goal has already
// inserted is found on its own probe sequence, so it is stored once; which slot a label ends in
// depends on the order of the claims, the set of keys does not.  The host sizes a table at twice
// the graph's nodes or more (pairs_host.h), so a probe sequence meets an empty slot; the walk is
// bounded by the table size all the same.
#define LH_BLOCK 256
#define LH_Q 4  // 16-byte chunks of node words and of labels per thread and round: 16 nodes
template <bool LDS>
__device__ __forceinline__ void lab_hash_fill(const DevCorpus &c, const LabTab &t, uint32_t *tab) {
  const uint32_t tid = threadIdx.x, mask = t.mask;
  const uint32_t n4 = (mask >> 2) + 1u;  // 16-byte chunks of the table
  uint4 *t4 = reinterpret_cast<uint4 *>(tab);
  for (uint32_t i = tid; i < n4; i += LH_BLOCK) t4[i] = make_uint4(0u, 0u, 0u, 0u);
  if (!LDS) __threadfence();  // the zeros before any claim
  __syncthreads();
  const uint64_t n0 = c.node_off[t.graph];
  const uint32_t V = (uint32_t)(c.node_off[t.graph + 1] - n0);
  if (V) {
    // The graph's node words and labels in 16-byte aligned chunks (both arrays start on a 16-byte
    // boundary and end in whole chunks: dalloc), every load of a round issued before the first
    // use, at a chunk index clamped to the graph's last chunk (the k_build lesson);
    // nodes before the graph's first or past its last are masked below.
    const uint32_t skip = (uint32_t)(n0 & 3u);
    const uint4 *w4 = reinterpret_cast<const uint4 *>(c.word + (n0 - skip));
    const uint4 *l4 = reinterpret_cast<const uint4 *>(c.label + (n0 - skip));
    const uint32_t nck = (V + skip + 3u) / 4u;
    for (uint32_t base = 0; base < nck; base += LH_Q * LH_BLOCK) {
      uint4 w[LH_Q], l[LH_Q];
#pragma unroll
      for (int q = 0; q < LH_Q; q++) {
        const uint32_t k = min(base + q * LH_BLOCK + tid, nck - 1u);
        w[q] = w4[k];
        l[q] = l4[k];
      }
#pragma unroll
      for (int q = 0; q < LH_Q; q++) {
        const uint32_t k = base + q * LH_BLOCK + tid;
        const uint32_t ww[4] = {w[q].x, w[q].y, w[q].z, w[q].w}, ll[4] = {l[q].x, l[q].y, l[q].z, l[q].w};
#pragma unroll
        for (int b = 0; b < 4; b++) {
          const uint32_t x = 4u * k + (uint32_t)b;  // node x - skip of the graph
          if (k >= nck || x < skip || x - skip >= V || is_rule(ww[b])) continue;
          const uint32_t key = ll[b] + 1u;
          uint32_t h = hash_label(ll[b]) & mask;
          for (uint32_t n = 0; n <= mask; n++) {
            const uint32_t old = atomicCAS(&tab[h], 0u, key);
            if (old == 0u || old == key) break;
            h = (h + 1u) & mask;
          }
        }
      }
    }
  }
  if (LDS) {  // the finished table to HBM in 16-byte stores
    __syncthreads();
    uint4 *o4 = (uint4 *)(SD_GLOBAL uint4 *)t.key;
    for (uint32_t i = tid; i < n4; i += LH_BLOCK) o4[i] = t4[i];
  }
}

// lds_max: tables of at most this many slots are built in the dynamic LDS (the host passes the
// largest of them as the launch's LDS size), the others in place with global compare-and-swap
__global__ __launch_bounds__(LH_BLOCK) void k_lab_hash(DevCorpus c, const LabTab *tabs, uint32_t lds_max) {
  extern __shared__ __align__(16) uint8_t dyn[];
  const LabTab t = tabs[blockIdx.x];
  if (t.mask < lds_max) lab_hash_fill<true>(c, t, reinterpret_cast<uint32_t *>(dyn));
  else lab_hash_fill<false>(c, t, (uint32_t *)(SD_GLOBAL uint32_t *)t.key);  // (global, not generic: see sdiff_mark_bad)
}

void launch_lab_hash(const DevCorpus &c, const LabTab *tabs, uint32_t n_tabs, uint32_t lds_max, uint32_t lds_slots,
                     hipStream_t s) {
  if (!n_tabs) return;
  const uint32_t bytes = 4u * lds_slots;
  if (bytes) hipFuncSetAttribute((const void *)k_lab_hash, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
  hipLaunchKernelGGL(k_lab_hash, dim3(n_tabs), dim3(LH_BLOCK), bytes, s, c, tabs, lds_max);
}

// n_lds / n_glob: the entries of each tier, counted on the host (an empty tier is not launched)
template <bool TABS>
static void launch_sdiff_t(const DevCorpus &c, const SdiffArgs &a, uint32_t n_entries, uint32_t n_lds, uint32_t n_glob,
                           hipStream_t s) {
  if (n_lds && c.t_diff.bytes) {
    const uint32_t bytes = c.t_diff.bytes, with = bytes + sdiff_depth_bytes(c.t_diff.v);
    if (SDIFF_CU_LDS / with == SDIFF_CU_LDS / bytes) {  // the depths cost no workgroup per CU: in LDS
      hipFuncSetAttribute((const void *)k_sdiff_lds<true, TABS>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)with);
      hipLaunchKernelGGL((k_sdiff_lds<true, TABS>), dim3(n_entries), dim3(NEMO_BLOCK), with, s, c, a);
    } else {
      hipFuncSetAttribute((const void *)k_sdiff_lds<false, TABS>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
      hipLaunchKernelGGL((k_sdiff_lds<false, TABS>), dim3(n_entries), dim3(NEMO_BLOCK), bytes, s, c, a);
    }
  }
  if (!n_glob) return;
  if (c.gblock == 1024)
    hipLaunchKernelGGL((k_sdiff_glob<1024, TABS>), dim3(n_entries), dim3(1024), 0, s, c, a);
  else
    hipLaunchKernelGGL((k_sdiff_glob<NEMO_BLOCK, TABS>), dim3(n_entries), dim3(NEMO_BLOCK), 0, s, c, a);
}

void launch_sdiff(const DevCorpus &c, const SdiffArgs &a, uint32_t n_entries, uint32_t n_lds, uint32_t n_glob,
                  hipStream_t s) {
  if (!n_entries) return;
  if (a.tabs) launch_sdiff_t<true>(c, a, n_entries, n_lds, n_glob, s);
  else launch_sdiff_t<false>(c, a, n_entries, n_lds, n_glob, s);
}

}  // namespace nemo
