// k_near.hip — nemo_nearest_runs (DESIGN.md §Nearest runs): the post-goal label set of every run a
// call names as a bit row, the intersection counts of every (query, candidate) pair as a tiled
// popcount-AND "GEMM" over those rows, and per query the nearest candidate by
// dist = |L(q)| + |L(c)| - 2 |L(q) & L(c)|.  Nothing here reads a graph's structure: node words and
// labels only.
#include "device.h"
#include "internal.h"

namespace nemo {

#define NR_BLOCK 256
#define NR_Q 4  // 16-byte chunks of node words and of labels per thread and round: 16 nodes

// The goals of post graph g among chunks [first, ...) in steps of `step` chunk groups, f(label) for
// each: the graph's node words and labels in 16-byte aligned chunks (both arrays start on a 16-byte
// boundary and end in whole chunks: dalloc), every load of a round issued before the first use, at a
// chunk index clamped to the graph's last chunk; rules and the nodes before the graph's first or
// past its last are masked (k_lab_hash's loop, k_sdiff.hip).
template <class F>
__device__ __forceinline__ void near_goals(const DevCorpus &c, uint32_t g, uint32_t first, uint32_t step, F &&f) {
  const uint32_t tid = threadIdx.x;
  const uint64_t n0 = c.node_off[g];
  const uint32_t V = (uint32_t)(c.node_off[g + 1] - n0);
  if (!V) return;
  const uint32_t skip = (uint32_t)(n0 & 3u);
  const uint4 *w4 = reinterpret_cast<const uint4 *>(c.word + (n0 - skip));
  const uint4 *l4 = reinterpret_cast<const uint4 *>(c.label + (n0 - skip));
  const uint32_t nck = (V + skip + 3u) / 4u;
  for (uint32_t base = first * (NR_Q * NR_BLOCK); base < nck; base += step * (NR_Q * NR_BLOCK)) {
    uint4 w[NR_Q], l[NR_Q];
#pragma unroll
    for (int q = 0; q < NR_Q; q++) {
      const uint32_t k = min(base + q * NR_BLOCK + tid, nck - 1u);
      w[q] = w4[k];
      l[q] = l4[k];
    }
#pragma unroll
    for (int q = 0; q < NR_Q; q++) {
      const uint32_t k = base + q * NR_BLOCK + tid;
      const uint32_t ww[4] = {w[q].x, w[q].y, w[q].z, w[q].w}, ll[4] = {l[q].x, l[q].y, l[q].z, l[q].w};
#pragma unroll
      for (int b = 0; b < 4; b++) {
        const uint32_t x = 4u * k + (uint32_t)b;  // node x - skip of the graph
        if (k >= nck || x < skip || x - skip >= V || is_rule(ww[b])) continue;
        f(ll[b]);
      }
    }
  }
}

__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, d));
  return v;
}
__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += (uint32_t)__shfl_xor((int)v, d);
  return v;
}

// ---- the largest goal label of the post graphs (once per load) ------------------------------------
// blockIdx.x = run, blockIdx.y = the part of its post graph; one atomicMax per workgroup.
__global__ __launch_bounds__(NR_BLOCK) void k_near_lmax(DevCorpus c, uint32_t *lmax) {
  __shared__ uint32_t s_m[NR_BLOCK / 64];
  uint32_t m = 0;
  near_goals(c, 2u * blockIdx.x + 1u, blockIdx.y, gridDim.y, [&](uint32_t label) { m = max(m, label); });
  m = wave_max_u32(m);
  if (lane_id() == 0) s_m[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 1; k < NR_BLOCK / 64; k++) m = max(m, s_m[k]);
    if (m) atomicMax(lmax, m);
  }
}

void launch_near_lmax(const DevCorpus &c, uint32_t parts, uint32_t *lmax, hipStream_t s) {
  if (!c.n_runs) return;
  hipLaunchKernelGGL(k_near_lmax, dim3(c.n_runs, parts ? parts : 1u), dim3(NR_BLOCK), 0, s, c, lmax);
}

// ---- bit rows ------------------------------------------------------------------------------------
// One workgroup per distinct run of the call: bit `label` of the row for every goal of its post graph.
// The row is u64 words to the GEMM and u32 words here (little endian: bit l & 63 of u64 word l >> 6
// is bit l & 31 of u32 word l >> 5).  A bit is set by an atomic OR that returns the word it found, so
// the bits a workgroup finds clear are the distinct labels: their count is |L(r)|, the popcount of the
// finished row (several goals may share a label; the count is of labels, not of goals).
template <bool LDS>
__device__ __forceinline__ void near_bits_fill(const DevCorpus &c, const NearArgs &a, uint32_t r, uint32_t *row) {
  __shared__ uint32_t s_n[NR_BLOCK / 64];
  const uint32_t tid = threadIdx.x;
  const uint32_t n4 = (uint32_t)(a.W / 2);  // 16-byte chunks of a row (W is even)
  uint4 *r4 = reinterpret_cast<uint4 *>(row);
  for (uint32_t i = tid; i < n4; i += NR_BLOCK) r4[i] = make_uint4(0u, 0u, 0u, 0u);
  if (!LDS) __threadfence();  // the zeros before any OR
  __syncthreads();
  uint32_t n = 0;
  const uint32_t w32 = 4u * n4;
  near_goals(c, a.row_graph[r], 0u, 1u, [&](uint32_t label) {
    const uint32_t w = label >> 5, bit = 1u << (label & 31u);
    if (w >= w32) return;  // (no label is past lmax: k_near_lmax read the same graphs)
    n += (atomicOr(&row[w], bit) & bit) ? 0u : 1u;
  });
  n = wave_sum_u32(n);
  if (lane_id() == 0) s_n[tid >> 6] = n;
  __syncthreads();
  if (tid == 0) {
#pragma unroll
    for (int k = 1; k < NR_BLOCK / 64; k++) n += s_n[k];
    a.size[r] = n;
  }
  if (LDS) {  // the finished row to HBM in 16-byte stores
    uint4 *o4 = reinterpret_cast<uint4 *>(a.bits + (size_t)r * a.W);
    for (uint32_t i = tid; i < n4; i += NR_BLOCK) o4[i] = r4[i];
  }
}

// lds: rows are built in the dynamic LDS (the launch's LDS size is a row), else in place
__global__ __launch_bounds__(NR_BLOCK) void k_near_bits(DevCorpus c, NearArgs a, uint32_t lds) {
  extern __shared__ __align__(16) uint8_t dyn[];
  const uint32_t r = blockIdx.x;
  if (lds) near_bits_fill<true>(c, a, r, reinterpret_cast<uint32_t *>(dyn));
  else near_bits_fill<false>(c, a, r, reinterpret_cast<uint32_t *>(a.bits + (size_t)r * a.W));
}

void launch_near_bits(const DevCorpus &c, const NearArgs &a, uint32_t lds_max, hipStream_t s) {
  if (!a.rows) return;
  const uint64_t row_bytes = 8 * a.W;
  const uint32_t bytes = row_bytes <= lds_max ? (uint32_t)row_bytes : 0u;
  if (bytes) hipFuncSetAttribute((const void *)k_near_bits, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
  hipLaunchKernelGGL(k_near_bits, dim3(a.rows), dim3(NR_BLOCK), bytes, s, c, a, bytes ? 1u : 0u);
}

// ---- intersection counts: I[i][j] = sum_k popc(Q[i][k] & C[j][k]) ----------------------------------
// One workgroup per NI_T x NI_T tile of (query position, candidate position) and per K range
// (blockIdx.z); thread (ty, tx) of the 16 x 16 holds the 4 x 4 counts of query rows 4 ty + a and
// candidate rows tx + 16 b.  A K-slab of NI_KS u64 words of both operands is staged in LDS k-major,
// [k][row]: the four query words of a thread are 32 contiguous bytes that the 16 threads of one ty
// share (a wave reads four addresses: a broadcast), and its candidate words are b consecutive 8-byte
// words over tx (16 lanes cover 128 contiguous bytes, the other lanes of the group read the same
// ones: conflict-free).  The slab after the current one is loaded from global memory into registers
// (16-byte loads, one row per lane, so the k-major LDS writes are conflict-free too) before the
// current one is counted and written to the other LDS buffer after: one barrier per slab.  Counts
// stay in registers; with one K range they are stored, with several they are added to the zeroed
// matrix with integer atomicAdd (exact in any order).
#define NI_T 64
#define NI_KS 16
static_assert(NI_T * NI_KS / 2 == 2 * NR_BLOCK, "two 16-byte chunks per thread and operand");

__device__ __forceinline__ uint64_t u64_of(uint32_t lo, uint32_t hi) { return (uint64_t)lo | ((uint64_t)hi << 32); }

__global__ __launch_bounds__(NR_BLOCK) void k_near_isect(NearArgs a, uint32_t tc, uint32_t slabs, uint32_t slabs_per_split,
                                                         uint32_t ksplit) {
  __shared__ __align__(16) uint64_t sq[2][NI_KS][NI_T];
  __shared__ __align__(16) uint64_t sc[2][NI_KS][NI_T];
  const uint32_t tid = threadIdx.x;
  const uint32_t q0 = (blockIdx.x / tc) * NI_T, c0 = (blockIdx.x % tc) * NI_T;
  const uint32_t s_lo = blockIdx.z * slabs_per_split, s_hi = min(slabs, s_lo + slabs_per_split);
  // staging: this thread loads chunks kp and kp + 4 (words 2 kp, 2 kp + 1 of the slab) of tile row lrow of
  // both operands; tile rows past the lists are clamped to the last position (their counts are not stored)
  const uint32_t lrow = tid & 63u, kp = tid >> 6;
  const uint32_t w2 = (uint32_t)(a.W / 2);  // chunks per row
  const uint4 *qp = reinterpret_cast<const uint4 *>(a.bits + (size_t)a.qrow[min(q0 + lrow, a.n_q - 1u)] * a.W);
  const uint4 *cp = reinterpret_cast<const uint4 *>(a.bits + (size_t)a.crow[min(c0 + lrow, a.n_c - 1u)] * a.W);
  uint4 r[4];
  uint32_t m0 = 0u, m1 = 0u;
  // chunks past the row's end count as zero: loaded at the row's last chunk (never past the matrix), and
  // masked when the registers go to LDS, so that the loads stay in flight behind the current slab's counts
  auto load = [&](uint32_t s) {
    const uint32_t k0 = s * (NI_KS / 2) + kp, k1 = k0 + 4u;
    const uint32_t k0c = min(k0, w2 - 1u), k1c = min(k1, w2 - 1u);
    m0 = k0 < w2 ? ~0u : 0u;
    m1 = k1 < w2 ? ~0u : 0u;
    r[0] = qp[k0c];
    r[1] = qp[k1c];
    r[2] = cp[k0c];
    r[3] = cp[k1c];
  };
  auto store = [&](uint32_t buf) {
    sq[buf][2u * kp][lrow] = u64_of(r[0].x & m0, r[0].y & m0);
    sq[buf][2u * kp + 1u][lrow] = u64_of(r[0].z & m0, r[0].w & m0);
    sq[buf][2u * kp + 8u][lrow] = u64_of(r[1].x & m1, r[1].y & m1);
    sq[buf][2u * kp + 9u][lrow] = u64_of(r[1].z & m1, r[1].w & m1);
    sc[buf][2u * kp][lrow] = u64_of(r[2].x & m0, r[2].y & m0);
    sc[buf][2u * kp + 1u][lrow] = u64_of(r[2].z & m0, r[2].w & m0);
    sc[buf][2u * kp + 8u][lrow] = u64_of(r[3].x & m1, r[3].y & m1);
    sc[buf][2u * kp + 9u][lrow] = u64_of(r[3].z & m1, r[3].w & m1);
  };
  const uint32_t ty = tid >> 4, tx = tid & 15u;
  uint32_t acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; i++)
#pragma unroll
    for (int j = 0; j < 4; j++) acc[i][j] = 0u;
  if (s_lo < s_hi) {
    load(s_lo);
    store(0u);
  }
  __syncthreads();
  for (uint32_t s = s_lo; s < s_hi; s++) {
    const uint32_t buf = (s - s_lo) & 1u;
    const bool more = s + 1u < s_hi;
    if (more) load(s + 1u);
#pragma unroll 2
    for (int k = 0; k < NI_KS; k++) {
      const ulonglong2 qa = *reinterpret_cast<const ulonglong2 *>(&sq[buf][k][4u * ty]);
      const ulonglong2 qb = *reinterpret_cast<const ulonglong2 *>(&sq[buf][k][4u * ty + 2u]);
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const uint64_t cj = sc[buf][k][tx + 16u * j];
        acc[0][j] += (uint32_t)__popcll(qa.x & cj);
        acc[1][j] += (uint32_t)__popcll(qa.y & cj);
        acc[2][j] += (uint32_t)__popcll(qb.x & cj);
        acc[3][j] += (uint32_t)__popcll(qb.y & cj);
      }
    }
    if (more) store(buf ^ 1u);
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const uint32_t qi = q0 + 4u * ty + (uint32_t)i;
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const uint32_t cj = c0 + tx + 16u * (uint32_t)j;
      if (qi >= a.n_q || cj >= a.n_c) continue;
      uint32_t *o = a.mat + (size_t)qi * a.n_c + cj;
      if (ksplit > 1u) atomicAdd(o, acc[i][j]);
      else *o = acc[i][j];
    }
  }
}

void launch_near_isect(const NearArgs &a, uint64_t tq, uint64_t tc, uint32_t slabs, uint32_t slabs_per_split,
                       uint32_t ksplit, hipStream_t s) {
  if (!a.n_q || !a.n_c) return;
  hipLaunchKernelGGL(k_near_isect, dim3((uint32_t)(tq * tc), 1, ksplit), dim3(NR_BLOCK), 0, s, a, (uint32_t)tc, slabs,
                     slabs_per_split, ksplit);
}

// ---- distances and the nearest candidate -----------------------------------------------------------
// One wave per query position i: dist(i, j) = |L(q)| + |L(c)| - 2 I[i][j] written in place of I[i][j]
// (a self-pair keeps its true distance 0 there), and the least (dist, j) over the candidates of
// another run than the query's, by a wave reduction of dist << 32 | j.
__global__ __launch_bounds__(NR_BLOCK) void k_near_pick(NearArgs a) {
  const uint32_t i = blockIdx.x * (NR_BLOCK / 64) + (threadIdx.x >> 6), lane = lane_id();
  if (i >= a.n_q) return;
  const uint32_t qr = a.qrow[i], szq = a.size[qr];
  uint32_t *m = a.mat + (size_t)i * a.n_c;
  unsigned long long best = ~0ull;
  for (uint32_t j = lane; j < a.n_c; j += 64u) {
    const uint32_t cr = a.crow[j];
    const uint32_t d = szq + a.size[cr] - 2u * m[j];
    m[j] = d;
    if (cr != qr) best = min(best, ((unsigned long long)d << 32) | j);
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) best = min(best, (unsigned long long)__shfl_xor(best, d));
  if (lane == 0) {
    uint4 o = make_uint4(~0u, ~0u, ~0u, ~0u);  // no candidate left
    if (best != ~0ull) {
      const uint32_t j = (uint32_t)best, d = (uint32_t)(best >> 32), szc = a.size[a.crow[j]];
      const uint32_t isect = (szq + szc - d) / 2u;
      o = make_uint4(j, d, szq - isect, szc - isect);
    }
    reinterpret_cast<uint4 *>(a.out)[i] = o;
  }
}

void launch_near_pick(const NearArgs &a, hipStream_t s) {
  if (!a.n_q) return;
  hipLaunchKernelGGL(k_near_pick, dim3((a.n_q + NR_BLOCK / 64 - 1) / (NR_BLOCK / 64)), dim3(NR_BLOCK), 0, s, a);
}

}  // namespace nemo
