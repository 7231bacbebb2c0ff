// k_dclass.hip — failure classes (nemo_diff_classes; DESIGN.md §Failure classes): one pass over the
// D masks of the distinct label sources for their 128-bit membership hash, |D| and the per-node
// support, and the exact row comparison behind every hash bucket.
//
// A D mask is one byte per node of run 0's post graph; row u of a call starts at byte row[u] * V0
// of the mask buffer, so rows are not 16-byte aligned in general (V0 = 5002 at C3).  Every lane
// loads whole aligned 16-byte chunks and shifts two neighbours into the 16 bytes of "its" nodes
// (dc_load16), so the node set behind a lane and a byte position is the same for every row.
#include "device.h"
#include "internal.h"

namespace nemo {

#define DC_TILE 4u                    // 1024-node wave loads per column tile
#define DC_TILE_NODES (DC_TILE * 1024u)

__device__ __forceinline__ uint32_t dc_shr(uint32_t lo, uint32_t hi, uint32_t bits) {
  return bits ? (lo >> bits) | (hi << (32u - bits)) : lo;
}
template <int WS>
__device__ __forceinline__ void dc_shift(const uint32_t (&w)[9], uint32_t bits, uint32_t (&r)[4]) {
#pragma unroll
  for (int j = 0; j < 4; j++) r[j] = dc_shr(w[j + WS], w[j + WS + 1], bits);
}

// The 16 mask bytes of nodes [16k, 16k + 16) of a row of `len` nodes, bytes of nodes >= len zero.
// base16: the row's first byte rounded down to 16 bytes; sh: the row's offset from it (0..15, the
// same for every lane).  Only aligned chunks that hold a byte of the row are read, and the buffer
// ends on a 16-byte boundary (dalloc), so no read leaves it.
__device__ __forceinline__ void dc_load16(const uint4 *__restrict__ base16, uint32_t sh, uint64_t k, uint64_t len,
                                          uint32_t (&r)[4]) {
  uint32_t w[9] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
  const uint64_t end = sh + len;  // first byte past the row, from base16
  if (16 * k < end) {
    const uint4 q = base16[k];
    w[0] = q.x, w[1] = q.y, w[2] = q.z, w[3] = q.w;
  }
  if (sh && 16 * (k + 1) < end) {
    const uint4 q = base16[k + 1];
    w[4] = q.x, w[5] = q.y, w[6] = q.z, w[7] = q.w;
  }
  const uint32_t bits = 8u * (sh & 3u);
  switch (sh >> 2) {  // wave-uniform
    case 0: dc_shift<0>(w, bits, r); break;
    case 1: dc_shift<1>(w, bits, r); break;
    case 2: dc_shift<2>(w, bits, r); break;
    default: dc_shift<3>(w, bits, r); break;
  }
  const uint64_t left = 16 * k < len ? len - 16 * k : 0;  // nodes of the row from 16k on
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const uint32_t vb = left >= 4u * j + 4u ? 4u : (left > 4u * j ? (uint32_t)(left - 4u * j) : 0u);
    r[j] &= vb == 4u ? 0xFFFFFFFFu : ((1u << (8u * vb)) - 1u);
  }
}

// bit 7 of every byte of x that is not zero
__device__ __forceinline__ uint32_t dc_nz(uint32_t x) {
  return (((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x) & 0x80808080u;
}

__device__ __forceinline__ uint64_t dc_mix(uint64_t x) {
  x ^= x >> 30;
  x *= 0xBF58476D1CE4E5B9ull;
  x ^= x >> 27;
  x *= 0x94D049BB133111EBull;
  x ^= x >> 31;
  return x;
}

// Hash + popcount + support.  Workgroup (x, y): column tile x (DC_TILE_NODES nodes) of the rows
// [y * rows_per_block, ...), one row per wave at a time.  A 1024-node wave load gives sixteen
// ballots of "byte != 0": 64-bit membership words, wave-uniform, hashed in scalar registers.  A
// row's hash is the sum (mod 2^64, two lanes) of a mix of every non-zero word and its index, so
// tiles combine in any order by adding; a zero word adds nothing.  The support counters of the
// tile's columns stay in registers over the workgroup's rows (weighted by the entries of each
// source), are summed over the four waves in LDS, and only the non-zero columns go to memory.
__global__ __launch_bounds__(NEMO_BLOCK) void k_dclass_hash(DclassArgs a) {
  __shared__ uint32_t sup[DC_TILE_NODES];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
  for (uint32_t i = tid; i < DC_TILE_NODES; i += NEMO_BLOCK) sup[i] = 0u;
  __syncthreads();
  uint32_t cnt[DC_TILE][16];
#pragma unroll
  for (uint32_t t = 0; t < DC_TILE; t++)
#pragma unroll
    for (int j = 0; j < 16; j++) cnt[t][j] = 0u;
  const uint32_t r0 = blockIdx.y * a.rows_per_block;
  const uint32_t r1 = min(a.nu, r0 + a.rows_per_block);
  for (uint32_t u = r0 + wv; u < r1; u += NEMO_WAVES) {
    const uintptr_t p = (uintptr_t)(a.mask + (uint64_t)a.row[u] * a.V0);
    const uint4 *base16 = (const uint4 *)(p & ~(uintptr_t)15);
    const uint32_t sh = (uint32_t)(p & 15u), wgt = a.weight[u];
    uint64_t h1 = 0, h2 = 0;
    uint32_t pop = 0;
#pragma unroll
    for (uint32_t t = 0; t < DC_TILE; t++) {
      const uint64_t chunk = (uint64_t)blockIdx.x * DC_TILE + t;  // 1024-node chunk of the row
      if (chunk * 1024u >= a.V0) break;
      uint32_t r[4];
      dc_load16(base16, sh, chunk * 64u + lane, a.V0, r);
#pragma unroll
      for (int j = 0; j < 16; j++) {
        const bool in = (dc_nz(r[j >> 2]) >> (8 * (j & 3) + 7)) & 1u;
        const uint64_t b = __ballot(in);  // nodes chunk * 1024 + 16 * lane + j
        if (b) {
          const uint64_t x = dc_mix(b ^ ((chunk * 16u + j + 1u) * 0x9E3779B97F4A7C15ull));
          h1 += x;
          h2 += dc_mix(x ^ 0xD6E8FEB86659FD93ull);
          pop += (uint32_t)__popcll(b);
        }
        cnt[t][j] += in ? wgt : 0u;
      }
    }
    if (lane == 0 && pop) {  // (a tile without members adds nothing)
      atomicAdd((unsigned long long *)&a.hash[2 * (uint64_t)u], (unsigned long long)h1);
      atomicAdd((unsigned long long *)&a.hash[2 * (uint64_t)u + 1], (unsigned long long)h2);
      atomicAdd(&a.pop[u], pop);
    }
  }
  // sup[t][j][lane]: conflict-free adds; read back in node order below
#pragma unroll
  for (uint32_t t = 0; t < DC_TILE; t++)
#pragma unroll
    for (int j = 0; j < 16; j++)
      if (cnt[t][j]) atomicAdd(&sup[t * 1024u + j * 64u + lane], cnt[t][j]);
  __syncthreads();
  for (uint32_t i = tid; i < DC_TILE_NODES; i += NEMO_BLOCK) {
    const uint32_t v = sup[(i & ~1023u) + (i & 15u) * 64u + ((i >> 4) & 63u)];
    const uint64_t node = (uint64_t)blockIdx.x * DC_TILE_NODES + i;
    if (v && node < a.V0) atomicAdd(&a.support[node], v);
  }
}

// Exact verify: one wave per (row, candidate) pair; verdict 1 iff the two rows have the same
// membership at every node.  A wave stops at the first 1024-node chunk that differs.
__global__ __launch_bounds__(NEMO_BLOCK) void k_dclass_cmp(DclassArgs a, const uint32_t *__restrict__ pairs,
                                                            uint32_t n_pairs, uint8_t *__restrict__ verdict) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t pr = blockIdx.x * NEMO_WAVES + (threadIdx.x >> 6);
  if (pr >= n_pairs) return;
  const uintptr_t pa = (uintptr_t)(a.mask + (uint64_t)a.row[pairs[2 * pr]] * a.V0);
  const uintptr_t pb = (uintptr_t)(a.mask + (uint64_t)a.row[pairs[2 * pr + 1]] * a.V0);
  const uint4 *ba = (const uint4 *)(pa & ~(uintptr_t)15), *bb = (const uint4 *)(pb & ~(uintptr_t)15);
  const uint32_t sa = (uint32_t)(pa & 15u), sb = (uint32_t)(pb & 15u);
  bool same = true;
  for (uint64_t chunk = 0; chunk * 1024u < a.V0; chunk++) {
    uint32_t x[4], y[4];
    dc_load16(ba, sa, chunk * 64u + lane, a.V0, x);
    dc_load16(bb, sb, chunk * 64u + lane, a.V0, y);
    uint32_t d = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) d |= dc_nz(x[j]) ^ dc_nz(y[j]);
    if (__ballot(d != 0u)) {
      same = false;
      break;
    }
  }
  if (lane == 0) verdict[pr] = same ? 1u : 0u;
}

uint32_t dclass_rows_per_block(uint64_t V0, uint32_t nu) {
  // about 2048 workgroups in all, and at least 16 rows behind every flush of the support counters
  const uint64_t gx = std::max<uint64_t>(1, (V0 + DC_TILE_NODES - 1) / DC_TILE_NODES);
  const uint64_t gy = std::max<uint64_t>(1, 2048 / gx);
  uint64_t rpb = std::max<uint64_t>(16, (nu + gy - 1) / gy);
  return (uint32_t)((rpb + NEMO_WAVES - 1) / NEMO_WAVES * NEMO_WAVES);
}

void launch_dclass_hash(const DclassArgs &a, hipStream_t s) {
  if (!a.nu || !a.V0) return;
  const uint32_t gx = (uint32_t)((a.V0 + DC_TILE_NODES - 1) / DC_TILE_NODES);
  const uint32_t gy = (a.nu + a.rows_per_block - 1) / a.rows_per_block;
  hipLaunchKernelGGL(k_dclass_hash, dim3(gx, gy), dim3(NEMO_BLOCK), 0, s, a);
}

void launch_dclass_cmp(const DclassArgs &a, const uint32_t *pairs, uint32_t n_pairs, uint8_t *verdict, hipStream_t s) {
  if (!n_pairs) return;
  hipLaunchKernelGGL(k_dclass_cmp, dim3((n_pairs + NEMO_WAVES - 1) / NEMO_WAVES), dim3(NEMO_BLOCK), 0, s, a, pairs,
                     n_pairs, verdict);
}

}  // namespace nemo
