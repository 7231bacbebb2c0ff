// diff_walk.h — what the level-sweep diff kernels (k_diff_lds in k_diff.hip; k_sdiff_lds and k_sdiff_glob in
// k_sdiff.hip) share: the node bits, the LDS image of a post graph, and the walk itself, from seeded node bits to
// emitted rule rows (differential-provenance.go:22-32,82-98; DESIGN.md §Symmetric diff).  The windowed k_diff works
// in Kahn-position space and keeps its own sweep.
#pragma once
#include "device.h"

namespace nemo {

// Node bits (the bytes of d_dbits / d_sdbits and of the LDS image).  0x04 is the one bit with two names: the diff
// seeds it on the goals it must NOT start from (label present in the source run), the symmetric diff on the goals
// it starts from (label absent from the run compared with).
#define DB_F 0x01u        // Fwd*(seeds)
#define DB_B 0x02u        // Bwd*(seeds)
#define DB_PRESENT 0x04u  // diff: goal whose label is a post-goal label of the source run
#define DB_BAD 0x04u      // symmetric diff: goal whose label the compared run lacks
#define DB_LEAF 0x08u     // D goal without a D child
#define DB_D 0x10u        // D = Fwd* & Bwd* (the symmetric diff's S)
#define DB_LP 0x20u       // D rule with a D-leaf child

// The rows of a post graph as the walk reads them, and its rule test.  LDS image (diff_lds_bytes, device.h): u16
// rows both ways, a rule bitmap and the entry's node bits, ~5V + 4E bytes; the Kahn order (coalesced, one load per
// level) stays in HBM.
struct DiffLds {
  uint16_t *rp, *fp, *rc, *fc;
  uint32_t *rule;
  uint8_t *bits;
  __device__ __forceinline__ bool is_rule(uint32_t v) const { return (rule[v >> 5] >> (v & 31u)) & 1u; }
};
__device__ __forceinline__ DiffLds diff_carve(void *base, uint32_t V, uint32_t E) {
  uint8_t *p = (uint8_t *)base;
  DiffLds d;
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
// the GraphView's own rows in HBM
struct DiffGlob {
  const uint32_t *rp, *fp, *rc, *fc, *word;
  __device__ __forceinline__ bool is_rule(uint32_t v) const { return ::is_rule(word[v]); }
};

// FENCE: what the walk's stores need before a barrier lets other threads read them
#define WF_NONE 0   // bits and depths in LDS (or depths in HBM behind the barrier alone: k_diff_lds)
#define WF_DEPTH 1  // bits in LDS, depths in HBM: __threadfence_block() after each depth level
#define WF_ALL 2    // bits and depths in HBM: __threadfence() before every barrier

struct DiffOut {
  uint8_t *mask;             // [V] the entry's D mask
  uint32_t *rows, *n_rows;   // (entry, rule) rows and their counter
  uint32_t e;
};

// One workgroup of B threads, one entry over graph gv, bits seeded (0x04 only) by every thread but not yet
// published: the walk opens with the barrier that does that.
//   seeds = SYM ? DB_BAD nodes : goals without DB_PRESENT
//   D     = Fwd*(seeds) ∩ Bwd*(seeds), written to o.mask
//   rows  = D rules with a D-leaf child at maximal depth (longest path inside D), appended to o.rows in any order
// depth: u16 in LDS or i32 in HBM; only D nodes touch it.
template <int B, int FENCE, bool SYM, class Rows, class Depth>
__device__ __forceinline__ void diff_walk(const GraphView &gv, const Rows &R, uint8_t *bits, Depth *depth,
                                          const DiffOut &o) {
  __shared__ int32_t s_max;
  const uint32_t tid = threadIdx.x, V = gv.V, nl = gv.nlev;
  auto seed = [&](uint8_t b, uint32_t v) { return SYM ? (b & DB_BAD) != 0 : !R.is_rule(v) && !(b & DB_PRESENT); };
  auto sync = [] {
    if (FENCE == WF_ALL) __threadfence();
    __syncthreads();
  };
  if (tid == 0) s_max = -1;
  sync();
  for (uint32_t l = 0; l < nl; l++) {
    for (uint32_t i = gv.lvl[l] + tid; i < gv.lvl[l + 1]; i += B) {
      const uint32_t v = gv.topo[i];
      bool fw = seed(bits[v], v);
      for (uint32_t j = R.rp[v]; j < R.rp[v + 1] && !fw; j++) fw = (bits[R.rc[j]] & DB_F) != 0;
      if (fw) bits[v] |= DB_F;
    }
    sync();
  }
  for (uint32_t l = nl; l-- > 0;) {
    for (uint32_t i = gv.lvl[l] + tid; i < gv.lvl[l + 1]; i += B) {
      const uint32_t v = gv.topo[i];
      uint8_t b = bits[v];
      bool bw = seed(b, v);
      for (uint32_t j = R.fp[v]; j < R.fp[v + 1] && !bw; j++) bw = (bits[R.fc[j]] & DB_B) != 0;
      if (bw) b |= DB_B;
      if ((b & DB_F) && bw) b |= DB_D;
      bits[v] = b;
    }
    sync();
  }
  // longest path from a D root (Kahn-level DP restricted to D); D goal leaves
  for (uint32_t l = 0; l < nl; l++) {
    for (uint32_t i = gv.lvl[l] + tid; i < gv.lvl[l + 1]; i += B) {
      const uint32_t v = gv.topo[i];
      const uint8_t b = bits[v];
      if (!(b & DB_D)) continue;
      uint32_t d = 0;
      for (uint32_t j = R.rp[v]; j < R.rp[v + 1]; j++) {
        const uint32_t p = R.rc[j];
        if (bits[p] & DB_D) d = max(d, (uint32_t)depth[p] + 1u);
      }
      depth[v] = (Depth)d;
      if (!R.is_rule(v)) {
        // children are on later levels: their DB_D bit is final since the Bwd* sweep
        bool leaf = true;
        for (uint32_t j = R.fp[v]; j < R.fp[v + 1]; j++)
          if (bits[R.fc[j]] & DB_D) leaf = false;
        if (leaf) bits[v] = b | DB_LEAF;
      }
    }
    if (FENCE == WF_DEPTH) __threadfence_block();  // the level's depths (HBM) before the next level reads them
    sync();
  }
  for (uint32_t v = tid; v < V; v += B) o.mask[v] = (bits[v] & DB_D) ? 1 : 0;
  for (uint32_t r = tid; r < V; r += B) {
    if (!(bits[r] & DB_D) || !R.is_rule(r)) continue;
    bool lp = false;
    for (uint32_t j = R.fp[r]; j < R.fp[r + 1]; j++)
      if ((bits[R.fc[j]] & (DB_D | DB_LEAF)) == (DB_D | DB_LEAF)) lp = true;
    if (lp) {
      bits[r] |= DB_LP;
      atomicMax(&s_max, (int32_t)depth[r] + 1);
    }
  }
  sync();
  const int32_t mx = s_max;
  for (uint32_t r = tid; r < V; r += B) {
    if ((bits[r] & DB_LP) && (int32_t)depth[r] + 1 == mx) {
      const uint32_t k = atomicAdd(o.n_rows, 1u);
      o.rows[2 * k] = o.e;
      o.rows[2 * k + 1] = r;
    }
  }
}

}  // namespace nemo
