// k_gdedup.hip — duplicate provenance graphs (DESIGN.md §3 "Duplicate graphs"): most runs of a fault
// injection sweep carry the graphs of the fault-free run again, so the per-graph kernels (k_build,
// k_marksimp, k_chains) run on one representative per distinct content and k_replicate copies its
// result slices to the duplicates.
//   k_gd_hash   load time: a 128-bit hash of each graph's content (sizes, parity, node words, labels,
//               ID ranks, edge sources and destinations in stored order), one workgroup per graph
//   k_gd_cmp    load time: the exact comparison behind every hash bucket (gdedup_host.h rounds)
//   k_replicate per phase: representative -> duplicate, 16-byte stores aligned to the destination
#include "device.h"
#include "internal.h"

namespace nemo {

#define GD_BLOCK 256

__device__ __forceinline__ uint64_t gd_mix(uint64_t x) {
  x ^= x >> 30;
  x *= 0xBF58476D1CE4E5B9ull;
  x ^= x >> 27;
  x *= 0x94D049BB133111EBull;
  x ^= x >> 31;
  return x;
}

// four consecutive u32 of a[0..n) from index i (zeros past n): one 16-byte load where all four exist
__device__ __forceinline__ uint4 gd_load4(const uint32_t *a, uint32_t i, uint32_t n) {
  uint4 w = make_uint4(0u, 0u, 0u, 0u);
  if (i + 3 < n) {
    __builtin_memcpy(&w, a + i, 16);
  } else {
    if (i < n) w.x = a[i];
    if (i + 1 < n) w.y = a[i + 1];
    if (i + 2 < n) w.z = a[i + 2];
  }
  return w;
}

// A slice's contribution: the sum over its u32 pairs of a mix of the pair and its (array, index) key,
// so that threads add their parts in any order.
__device__ __forceinline__ void gd_hash_slice(const uint32_t *a, uint32_t n, uint64_t seed, uint64_t &h1, uint64_t &h2) {
  for (uint32_t i = 4 * threadIdx.x; i < n; i += 4 * GD_BLOCK) {
    const uint4 w = gd_load4(a, i, n);
    const uint64_t k = seed + (uint64_t)(i + 1u) * 0x9E3779B97F4A7C15ull;
    const uint64_t x = gd_mix((((uint64_t)w.y << 32) | w.x) ^ k);
    const uint64_t y = gd_mix((((uint64_t)w.w << 32) | w.z) ^ (k + 0xD6E8FEB86659FD93ull));
    h1 += x + y;
    h2 += gd_mix(x ^ 0xA0761D6478BD642Full) + gd_mix(y ^ 0xE7037ED1A0B428DBull);
  }
}

__device__ __forceinline__ uint64_t gd_wave_sum(uint64_t v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
  return v;
}

// hash[2g], hash[2g + 1] (zeroed before the launch)
__global__ __launch_bounds__(GD_BLOCK) void k_gd_hash(DevCorpus c, uint64_t *hash) {
  for (uint32_t g = blockIdx.x; g < c.G; g += gridDim.x) {
    const uint64_t n0 = c.node_off[g], e0 = c.edge_off[g];
    const uint32_t V = (uint32_t)(c.node_off[g + 1] - n0), E = (uint32_t)(c.edge_off[g + 1] - e0);
    uint64_t h1 = 0, h2 = 0;
    if (threadIdx.x == 0) {
      h1 = gd_mix((((uint64_t)V << 32) | E) ^ 0x1234567ull);
      h2 = gd_mix(h1 + (g & 1u) + 1u);
    }
    gd_hash_slice(c.word + n0, V, 0x11ull << 56, h1, h2);
    gd_hash_slice(c.label + n0, V, 0x22ull << 56, h1, h2);
    if (c.rank) gd_hash_slice(c.rank + n0, V, 0x33ull << 56, h1, h2);
    gd_hash_slice(c.esrc + e0, E, 0x44ull << 56, h1, h2);
    gd_hash_slice(c.edst + e0, E, 0x55ull << 56, h1, h2);
    h1 = gd_wave_sum(h1);
    h2 = gd_wave_sum(h2);
    if (lane_id() == 0) {
      atomicAdd((unsigned long long *)&hash[2 * (uint64_t)g], (unsigned long long)h1);
      atomicAdd((unsigned long long *)&hash[2 * (uint64_t)g + 1], (unsigned long long)h2);
    }
  }
}

__device__ __forceinline__ bool gd_differ(const uint32_t *a, const uint32_t *b, uint32_t n) {
  bool d = false;
  for (uint32_t i = 4 * threadIdx.x; i < n; i += 4 * GD_BLOCK) {
    const uint4 x = gd_load4(a, i, n), y = gd_load4(b, i, n);
    d |= x.x != y.x || x.y != y.y || x.z != y.z || x.w != y.w;
  }
  return d;
}

// verdict[k] = 1 iff graphs pairs[2k] and pairs[2k + 1] have the same content
__global__ __launch_bounds__(GD_BLOCK) void k_gd_cmp(DevCorpus c, const uint32_t *__restrict__ pairs, uint32_t n_pairs,
                                                      uint8_t *__restrict__ verdict) {
  for (uint32_t k = blockIdx.x; k < n_pairs; k += gridDim.x) {
    const uint32_t a = pairs[2 * k], b = pairs[2 * k + 1];
    const uint64_t na = c.node_off[a], nb = c.node_off[b], ea = c.edge_off[a], eb = c.edge_off[b];
    const uint32_t V = (uint32_t)(c.node_off[a + 1] - na), E = (uint32_t)(c.edge_off[a + 1] - ea);
    bool d = ((a ^ b) & 1u) != 0u || c.node_off[b + 1] - nb != V || c.edge_off[b + 1] - eb != E;
    if (!d) {  // (uniform: the sizes are the same for every thread)
      d |= gd_differ(c.word + na, c.word + nb, V);
      d |= gd_differ(c.label + na, c.label + nb, V);
      if (c.rank) d |= gd_differ(c.rank + na, c.rank + nb, V);
      d |= gd_differ(c.esrc + ea, c.esrc + eb, E);
      d |= gd_differ(c.edst + ea, c.edst + eb, E);
    }
    const int any = __syncthreads_or(d);
    if (threadIdx.x == 0) verdict[k] = any ? 0u : 1u;
  }
}

// ---- replicate ---------------------------------------------------------------------------------
// dst[0..n) = src[0..n) bytes by the whole workgroup.  Slices are not 16-byte aligned, and the two
// differ in alignment: the bytes up to the destination's first 16-byte boundary and after its last
// go one per lane; between them every lane stores whole aligned 16-byte chunks, each shifted out of
// the two aligned source chunks that hold its bytes (stage_lds's realignment, device.h).  A source
// chunk may end after the slice: arrays are allocated in whole 16-byte chunks (dalloc).
template <int WS>
__device__ __forceinline__ uint4 gd_shift(const uint4 &a, const uint4 &b, uint32_t bits) {
  const uint32_t w[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
  uint32_t r[4];
#pragma unroll
  for (int j = 0; j < 4; j++) r[j] = bits ? (w[j + WS] >> bits) | (w[j + WS + 1] << (32u - bits)) : w[j + WS];
  return make_uint4(r[0], r[1], r[2], r[3]);
}
__device__ __forceinline__ uint4 gd_funnel(const uint4 &a, const uint4 &b, uint32_t sh) {
  const uint32_t bits = 8u * (sh & 3u);
  switch (sh >> 2) {  // workgroup-uniform
    case 0: return gd_shift<0>(a, b, bits);
    case 1: return gd_shift<1>(a, b, bits);
    case 2: return gd_shift<2>(a, b, bits);
    default: return gd_shift<3>(a, b, bits);
  }
}
#define GD_DEPTH 4  // chunks in flight per thread
__device__ __forceinline__ void gd_copy(void *dst_, const void *src_, uint64_t n) {
  uint8_t *dst = (uint8_t *)dst_;
  const uint8_t *src = (const uint8_t *)src_;
  const uint32_t tid = threadIdx.x;
  const uint64_t head = min(n, (uint64_t)((16u - (uint32_t)((uintptr_t)dst & 15u)) & 15u));
  if (tid < head) dst[tid] = src[tid];
  dst += head;
  src += head;
  n -= head;
  const uint64_t nc = n >> 4;
  const uint32_t sh = (uint32_t)((uintptr_t)src & 15u);
  const uint4 *base = (const uint4 *)(src - sh);
  uint4 *out = (uint4 *)dst;
  for (uint64_t k0 = 0; k0 < nc; k0 += (uint64_t)GD_DEPTH * GD_BLOCK) {
    uint4 a[GD_DEPTH], b[GD_DEPTH];
#pragma unroll
    for (int q = 0; q < GD_DEPTH; q++) {
      const uint64_t k = min(k0 + (uint64_t)q * GD_BLOCK + tid, nc - 1);  // clamped: the loads stay unconditional
      a[q] = base[k];
      b[q] = sh ? base[k + 1] : a[q];
    }
#pragma unroll
    for (int q = 0; q < GD_DEPTH; q++) {
      const uint64_t k = k0 + (uint64_t)q * GD_BLOCK + tid;
      if (k < nc) out[k] = sh ? gd_funnel(a[q], b[q], sh) : a[q];
    }
  }
  const uint32_t tail = (uint32_t)(n & 15u);
  if (tid < tail) dst[16 * nc + tid] = src[16 * nc + tid];
}

// phase GD_BUILD: what k_build writes (GD_BUILD_SCALARS: its per-graph scalars alone, which the next
// kernels read of every graph; GD_BUILD_SLICES: the rest, deferred until something reads a duplicate's
// slices: ensure_whole, ctx.h); GD_MARKSIMP: what k_marksimp (or k_build's tail) writes;
// GD_CHAINS: what the first chain tier writes.  A pair is copied under the condition its
// representative's kernel ran under, so a class outside a kernel's tier is left to the per-graph
// global kernels, which take duplicates like any other graph.
__global__ __launch_bounds__(GD_BLOCK) void k_replicate(DevCorpus c, const uint32_t *__restrict__ pairs, uint32_t n_pairs,
                                                         int phase) {
  const uint32_t tid = threadIdx.x;
  for (uint32_t k = blockIdx.x; k < n_pairs; k += gridDim.x) {
    const uint32_t d = pairs[2 * k], r = pairs[2 * k + 1];
    const uint64_t nd = c.node_off[d], nr = c.node_off[r], ed = c.edge_off[d], er = c.edge_off[r];
    const uint32_t V = (uint32_t)(c.node_off[r + 1] - nr), E = (uint32_t)(c.edge_off[r + 1] - er);
    if (phase == GD_BUILD || phase == GD_BUILD_SCALARS || phase == GD_BUILD_SLICES) {
      const bool built = c.bld_bytes != 0u && V <= c.bld_v && E <= c.bld_e;
      if (!built) continue;  // k_build returned at once: k_csr / k_topo take every graph of the class
      const uint32_t redo = c.redo[r], nl = min(c.nlev[r], V);
      if (tid == 0 && phase != GD_BUILD_SLICES) {
        c.redo[d] = (uint8_t)redo;
        c.err[d] = c.err[r];
        if (!redo) {
          c.created[d] = c.created[r];
          c.nlev[d] = c.nlev[r];
        }
      }
      if (redo || phase == GD_BUILD_SCALARS) continue;  // redo: handed to the global tier, duplicates included
      gd_copy(c.rp + nd + d, c.rp + nr + r, 4ull * (V + 1u));
      gd_copy(c.rc + ed, c.rc + er, 4ull * E);
      gd_copy(c.fp + nd + d, c.fp + nr + r, 4ull * (V + 1u));
      gd_copy(c.fc + ed, c.fc + er, 4ull * E);
      gd_copy(c.topo + nd, c.topo + nr, 4ull * V);
      gd_copy(c.lvl + nd + d, c.lvl + nr + r, 4ull * (nl + 1u));
      gd_copy(c.nlv + nd, c.nlv + nr, 4ull * V);
      if (d & 1u) {
        gd_copy(c.e2 + ed, c.e2 + er, 4ull * E);
        gd_copy(c.posoff + nd, c.posoff + nr, 4ull * V);
      }
    } else if (phase == GD_MARKSIMP) {
      if (c.err[r] || !tier_fits(c.t_ms, V, E, c.nlev[r])) continue;  // k_marksimp's own conditions
      gd_copy(c.flags + nd, c.flags + nr, V);
      if (tid == 0) {
        c.prehold[d] = c.prehold[r];
        c.holdany[d] = c.holdany[r];
      }
    } else {
      if (c.gs_off[r] != ~0ull) continue;  // a deep graph (never a duplicate): k_chains_glob's
      const uint32_t n = c.nch[r];
      if (tid == 0) {
        c.nch[d] = n;
        if (c.err[r]) c.err[d] = c.err[r];
      }
      if (n != NEMO_NONE) gd_copy(c.chain + 5 * nd, c.chain + 5 * nr, 20ull * min(n, V));
    }
  }
}

#define GD_GRID 4096u
void launch_gd_hash(const DevCorpus &c, uint64_t *hash, hipStream_t s) {
  if (!c.G) return;
  launch_zero(hash, 16ull * c.G, s);
  hipLaunchKernelGGL(k_gd_hash, dim3(std::min(c.G, 8u * GD_GRID)), dim3(GD_BLOCK), 0, s, c, hash);
}
void launch_gd_cmp(const DevCorpus &c, const uint32_t *pairs, uint32_t n_pairs, uint8_t *verdict, hipStream_t s) {
  if (!n_pairs) return;
  hipLaunchKernelGGL(k_gd_cmp, dim3(std::min(n_pairs, 8u * GD_GRID)), dim3(GD_BLOCK), 0, s, c, pairs, n_pairs, verdict);
}
void launch_replicate(const DevCorpus &c, const uint32_t *pairs, uint32_t n_pairs, int phase, hipStream_t s) {
  if (!n_pairs) return;
  hipLaunchKernelGGL(k_replicate, dim3(std::min(n_pairs, GD_GRID)), dim3(GD_BLOCK), 0, s, c, pairs, n_pairs, phase);
}

}  // namespace nemo
