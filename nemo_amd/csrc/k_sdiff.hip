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
#include "device.h"
#include "internal.h"

namespace nemo {

#define SD_F 0x01u     // Fwd*(Bad)
#define SD_B 0x02u     // Bwd*(Bad)
#define SD_BAD 0x04u   // goal whose label is no run-0 post-goal label
#define SD_LEAF 0x08u  // S goal without an S child
#define SD_S 0x10u     // S = Fwd* & Bwd*
#define SD_LP 0x20u    // S rule with an S-leaf child

// Bad_e: the goals of gf whose label misses the run-0 label hash.  Each thread
// takes SD_BATCH nodes and walks their probe sequences together (as
// diff_fail_goals does), so a pass is a few rounds of independent loads.
// RULES: the same pass ballots the rule bits into the LDS rule bitmap (64
// consecutive nodes per wave and q: two plain word stores, no atomics).
#define SD_BATCH 8
template <int B, bool RULES>
__device__ __forceinline__ void sdiff_mark_bad(const SdiffArgs &a, const GraphView &gv, uint8_t *bits, uint32_t *rule) {
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
      h[q] = hash_label(lab[q]) & a.r0hmask;
      live |= (in && !rl ? 1u : 0u) << q;
    }
    while (live) {
      uint32_t k[SD_BATCH];
#pragma unroll
      for (int q = 0; q < SD_BATCH; q++) k[q] = ((live >> q) & 1u) ? a.r0hkey[h[q]] : 0u;
#pragma unroll
      for (int q = 0; q < SD_BATCH; q++) {
        if (!((live >> q) & 1u)) continue;
        if (k[q] == lab[q] + 1u) {
          live &= ~(1u << q);  // a run-0 post-goal label
        } else if (k[q] == 0u) {
          bad |= 1u << q;
          live &= ~(1u << q);
        } else {
          h[q] = (h[q] + 1u) & a.r0hmask;
        }
      }
    }
#pragma unroll
    for (int q = 0; q < SD_BATCH; q++) {
      const uint32_t x = base + q * B + threadIdx.x;
      if (x < gv.V) bits[x] = ((bad >> q) & 1u) ? SD_BAD : 0u;
    }
  }
}

// LDS image: diff_carve's (k_diff.hip), declared here for this translation unit
// -- u16 rows both ways, a rule bitmap and the node bits (~5V + 4E bytes).
struct SdiffLds {
  uint16_t *rp, *fp, *rc, *fc;
  uint32_t *rule;
  uint8_t *bits;
};
__device__ __forceinline__ SdiffLds sdiff_carve(void *base, uint32_t V, uint32_t E) {
  uint8_t *p = (uint8_t *)base;
  SdiffLds d;
  d.rp = (uint16_t *)p;
  p += lds_align(2u * (V + 1u));
  d.fp = (uint16_t *)p;
  p += lds_align(2u * (V + 1u));
  d.rc = (uint16_t *)p;
  p += lds_align(2u * E);
  d.fc = (uint16_t *)p;
  p += lds_align(2u * E);
  d.rule = (uint32_t *)p;
  p += lds_align(4u * ((V + 31u) / 32u));
  d.bits = p;
  return d;
}

// LDS tier: entries whose graph is inside k_diff_lds's caps (t_diff).  The
// three level sweeps probe parents / children in LDS; the Kahn order is read
// coalesced from HBM, one load per level.  Depths (< V <= 16384) live in LDS
// as u16 behind the image (DLDS) when the 2V bytes they add leave the
// workgroups per CU of 160 KB LDS unchanged, and otherwise in HBM, in the
// entry's slice of the per-call scratch (only S nodes touch them).  At the C3
// shape (caps V 5005, E 7463) the image is 55.5 KB and 65.5 KB with the
// depths: two workgroups per CU either way, so the depths are in LDS there.
__host__ __device__ __forceinline__ uint32_t sdiff_depth_bytes(uint32_t v) { return lds_align(2u * v); }
#define SDIFF_CU_LDS (160u * 1024u)
template <bool DLDS>
__global__ __launch_bounds__(NEMO_BLOCK) void k_sdiff_lds(DevCorpus c, SdiffArgs a) {
  extern __shared__ __align__(16) uint8_t dyn[];
  __shared__ int32_t s_max;
  const uint32_t e = blockIdx.x, tid = threadIdx.x;
  const GraphView gv = c.view(a.graph[e]);
  if (!tier_fits(c.t_diff, gv.V, gv.E, gv.nlev)) return;  // k_sdiff_glob's entry
  const uint32_t V = gv.V, nl = gv.nlev;
  SdiffLds L = sdiff_carve(dyn, V, gv.E);
  uint8_t *mask = a.mask + a.off[e];
  int32_t *depth = a.depth + a.off[e];
  // the depths sit behind the image of the tier's caps, so their offset does not depend on the graph
  uint16_t *ld = reinterpret_cast<uint16_t *>(dyn + c.t_diff.bytes);
#define DEPTH(v) (DLDS ? (int32_t)ld[v] : depth[v])
  {
    const StageDesc d[4] = {{gv.rp, L.rp, V + 1, ST_U16}, {gv.fp, L.fp, V + 1, ST_U16},
                            {gv.rc, L.rc, gv.E, ST_U16},  {gv.fc, L.fc, gv.E, ST_U16}};
    stage_lds<4, NEMO_BLOCK>(d);
  }
  if (tid == 0) s_max = -1;
  uint8_t *bits = L.bits;
  sdiff_mark_bad<NEMO_BLOCK, true>(a, gv, bits, L.rule);
  __syncthreads();
#define LRULE(v) ((L.rule[(v) >> 5] >> ((v) & 31)) & 1u)
  for (uint32_t l = 0; l < nl; l++) {
    for (uint32_t i = gv.lvl[l] + tid; i < gv.lvl[l + 1]; i += NEMO_BLOCK) {
      const uint32_t v = gv.topo[i];
      bool fw = (bits[v] & SD_BAD) != 0;
      for (uint32_t j = L.rp[v]; j < L.rp[v + 1] && !fw; j++) fw = (bits[L.rc[j]] & SD_F) != 0;
      if (fw) bits[v] |= SD_F;
    }
    __syncthreads();
  }
  for (uint32_t l = nl; l-- > 0;) {
    for (uint32_t i = gv.lvl[l] + tid; i < gv.lvl[l + 1]; i += NEMO_BLOCK) {
      const uint32_t v = gv.topo[i];
      uint8_t b = bits[v];
      bool bw = (b & SD_BAD) != 0;
      for (uint32_t j = L.fp[v]; j < L.fp[v + 1] && !bw; j++) bw = (bits[L.fc[j]] & SD_B) != 0;
      if (bw) b |= SD_B;
      if ((b & SD_F) && bw) b |= SD_S;
      bits[v] = b;
    }
    __syncthreads();
  }
  // longest path from an S root (Kahn-level DP restricted to S); S goal leaves
  for (uint32_t l = 0; l < nl; l++) {
    for (uint32_t i = gv.lvl[l] + tid; i < gv.lvl[l + 1]; i += NEMO_BLOCK) {
      const uint32_t v = gv.topo[i];
      const uint8_t b = bits[v];
      if (!(b & SD_S)) continue;
      uint32_t d = 0;
      for (uint32_t j = L.rp[v]; j < L.rp[v + 1]; j++) {
        const uint32_t p = L.rc[j];
        if (bits[p] & SD_S) d = max(d, (uint32_t)DEPTH(p) + 1u);
      }
      if (DLDS) ld[v] = (uint16_t)d;
      else depth[v] = (int32_t)d;
      if (!LRULE(v)) {
        bool leaf = true;
        for (uint32_t j = L.fp[v]; j < L.fp[v + 1]; j++)
          if (bits[L.fc[j]] & SD_S) leaf = false;
        if (leaf) bits[v] = b | SD_LEAF;
      }
    }
    if (!DLDS) __threadfence_block();  // the level's depths (HBM) before the next level reads them
    __syncthreads();
  }
  for (uint32_t v = tid; v < V; v += NEMO_BLOCK) mask[v] = (bits[v] & SD_S) ? 1 : 0;
  for (uint32_t r = tid; r < V; r += NEMO_BLOCK) {
    if (!(bits[r] & SD_S) || !LRULE(r)) continue;
    bool lp = false;
    for (uint32_t j = L.fp[r]; j < L.fp[r + 1]; j++)
      if ((bits[L.fc[j]] & (SD_S | SD_LEAF)) == (SD_S | SD_LEAF)) lp = true;
    if (lp) {
      bits[r] |= SD_LP;
      atomicMax(&s_max, DEPTH(r) + 1);
    }
  }
  __syncthreads();
  const int32_t mx = s_max;
  for (uint32_t r = tid; r < V; r += NEMO_BLOCK) {
    if ((bits[r] & SD_LP) && DEPTH(r) + 1 == mx) {
      const uint32_t k = atomicAdd(a.n_rows, 1u);
      a.rows[2 * k] = e;
      a.rows[2 * k + 1] = r;
    }
  }
#undef LRULE
#undef DEPTH
}

// Global tier: every other entry (graphs past t_diff's caps, u32 rows of graphs
// of >= 65536 nodes, and every entry under option graph_lds_max 0).  One
// workgroup per entry sweeps the Kahn levels over the HBM CSR; node bits and
// depths live in the entry's slice of the per-call scratch.  A level's stores
// are fenced before the barrier that opens the next level.  Correct, not tuned.
template <int B>
__global__ __launch_bounds__(B) void k_sdiff_glob(DevCorpus c, SdiffArgs a) {
  __shared__ int32_t s_max;
  const uint32_t e = blockIdx.x, tid = threadIdx.x;
  const GraphView gv = c.view(a.graph[e]);
  if (tier_fits(c.t_diff, gv.V, gv.E, gv.nlev)) return;  // k_sdiff_lds's entry
  const uint32_t V = gv.V, nl = gv.nlev;
  uint8_t *bits = a.bits + a.off[e];
  uint8_t *mask = a.mask + a.off[e];
  int32_t *depth = a.depth + a.off[e];
  if (tid == 0) s_max = -1;
  sdiff_mark_bad<B, false>(a, gv, bits, nullptr);
  __threadfence();
  __syncthreads();
  for (uint32_t l = 0; l < nl; l++) {
    for (uint32_t i = gv.lvl[l] + tid; i < gv.lvl[l + 1]; i += B) {
      const uint32_t v = gv.topo[i];
      bool fw = (bits[v] & SD_BAD) != 0;
      for (uint32_t j = gv.rp[v]; j < gv.rp[v + 1] && !fw; j++) fw = (bits[gv.rc[j]] & SD_F) != 0;
      if (fw) bits[v] |= SD_F;
    }
    __threadfence();
    __syncthreads();
  }
  for (uint32_t l = nl; l-- > 0;) {
    for (uint32_t i = gv.lvl[l] + tid; i < gv.lvl[l + 1]; i += B) {
      const uint32_t v = gv.topo[i];
      uint8_t b = bits[v];
      bool bw = (b & SD_BAD) != 0;
      for (uint32_t j = gv.fp[v]; j < gv.fp[v + 1] && !bw; j++) bw = (bits[gv.fc[j]] & SD_B) != 0;
      if (bw) b |= SD_B;
      if ((b & SD_F) && bw) b |= SD_S;
      bits[v] = b;
    }
    __threadfence();
    __syncthreads();
  }
  for (uint32_t l = 0; l < nl; l++) {
    for (uint32_t i = gv.lvl[l] + tid; i < gv.lvl[l + 1]; i += B) {
      const uint32_t v = gv.topo[i];
      const uint8_t b = bits[v];
      if (!(b & SD_S)) continue;
      uint32_t d = 0;
      for (uint32_t j = gv.rp[v]; j < gv.rp[v + 1]; j++) {
        const uint32_t p = gv.rc[j];
        if (bits[p] & SD_S) d = max(d, (uint32_t)depth[p] + 1u);
      }
      depth[v] = (int32_t)d;
      if (!is_rule(gv.word[v])) {
        // children are on later levels: their SD_S bit is final since the Bwd* sweep
        bool leaf = true;
        for (uint32_t j = gv.fp[v]; j < gv.fp[v + 1]; j++)
          if (bits[gv.fc[j]] & SD_S) leaf = false;
        if (leaf) bits[v] = b | SD_LEAF;
      }
    }
    __threadfence();
    __syncthreads();
  }
  for (uint32_t v = tid; v < V; v += B) mask[v] = (bits[v] & SD_S) ? 1 : 0;
  for (uint32_t r = tid; r < V; r += B) {
    if (!(bits[r] & SD_S) || !is_rule(gv.word[r])) continue;
    bool lp = false;
    for (uint32_t j = gv.fp[r]; j < gv.fp[r + 1]; j++)
      if ((bits[gv.fc[j]] & (SD_S | SD_LEAF)) == (SD_S | SD_LEAF)) lp = true;
    if (lp) {
      bits[r] |= SD_LP;
      atomicMax(&s_max, depth[r] + 1);
    }
  }
  __threadfence();
  __syncthreads();
  const int32_t mx = s_max;
  for (uint32_t r = tid; r < V; r += B) {
    if ((bits[r] & SD_LP) && depth[r] + 1 == mx) {
      const uint32_t k = atomicAdd(a.n_rows, 1u);
      a.rows[2 * k] = e;
      a.rows[2 * k + 1] = r;
    }
  }
}

// n_lds / n_glob: the entries of each tier, counted on the host (an empty tier is not launched)
void launch_sdiff(const DevCorpus &c, const SdiffArgs &a, uint32_t n_entries, uint32_t n_lds, uint32_t n_glob,
                  hipStream_t s) {
  if (!n_entries) return;
  if (n_lds && c.t_diff.bytes) {
    const uint32_t bytes = c.t_diff.bytes, with = bytes + sdiff_depth_bytes(c.t_diff.v);
    if (SDIFF_CU_LDS / with == SDIFF_CU_LDS / bytes) {  // the depths cost no workgroup per CU: in LDS
      hipFuncSetAttribute((const void *)k_sdiff_lds<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)with);
      hipLaunchKernelGGL(k_sdiff_lds<true>, dim3(n_entries), dim3(NEMO_BLOCK), with, s, c, a);
    } else {
      hipFuncSetAttribute((const void *)k_sdiff_lds<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
      hipLaunchKernelGGL(k_sdiff_lds<false>, dim3(n_entries), dim3(NEMO_BLOCK), bytes, s, c, a);
    }
  }
  if (!n_glob) return;
  if (c.gblock == 1024)
    hipLaunchKernelGGL(k_sdiff_glob<1024>, dim3(n_entries), dim3(1024), 0, s, c, a);
  else
    hipLaunchKernelGGL(k_sdiff_glob<NEMO_BLOCK>, dim3(n_entries), dim3(NEMO_BLOCK), 0, s, c, a);
}

}  // namespace nemo
