// k_knock.hip — nemo_knockout_leaves / nemo_knockout_sets: a raw provenance graph as an
// AND/OR circuit, evaluated bottom-up under 64 hypotheses at once.  Hypothesis b of a chunk is bit b of a u64
// "dead" word per node; one sweep over the graph's Kahn levels, deepest first, folds the children's words into
// each node's (OR for a rule, AND for a goal with children) in pull form: no atomics in the sweep, one barrier
// per level.  k_ko_leaves lists the sink goals (leaves mode), k_ko_lds sweeps a graph staged in LDS, k_ko_glob
// the same over the CSR in device memory.
#include "device.h"
#include "internal.h"
#include "knock_host.h"
#include "ko_sweep.h"

namespace nemo {

struct KoChunk {
  uint32_t graph, first, n;
  uint64_t moff;
};
__device__ __forceinline__ KoChunk ko_chunk(const KnockArgs &a, uint32_t ci) {
  const uint4 c0 = a.chunk[2u * ci], c1 = a.chunk[2u * ci + 1u];
  KoChunk k;
  k.graph = c0.x;
  k.first = c0.y;
  k.n = c0.z;
  k.moff = (uint64_t)c1.x | ((uint64_t)c1.y << 32);
  return k;
}

// ---- the sink goals of the listed graphs -----------------------------------------------------------
// element i (0..7) of two consecutive chunks, without a dynamically indexed array
__device__ __forceinline__ uint32_t pick8(uint4 a, uint4 b, int i) {
  uint32_t r = a.x;
  r = i == 1 ? a.y : r;
  r = i == 2 ? a.z : r;
  r = i == 3 ? a.w : r;
  r = i == 4 ? b.x : r;
  r = i == 5 ? b.y : r;
  r = i == 6 ? b.z : r;
  r = i == 7 ? b.w : r;
  return r;
}

// One workgroup over graph g: a node is a sink goal iff it is not a rule and its forward row is empty.  Node
// words and row pointers are read in 16-byte aligned chunks (both arrays start on a 16-byte boundary and end in
// whole chunks: dalloc), every load of a round issued before the first use, at chunk indices clamped to the
// graph's last chunk; the nodes before the graph's first or past its last are masked (k_lab_hash's loop).  A
// thread takes KO_Q consecutive chunks, so a block scan of the threads' counts gives the sink goals their
// positions in node-index order.  WRITE: list them at out[0 .. cap); else count them.  Returns the count.
template <bool WRITE>
__device__ __forceinline__ uint32_t ko_leaves_graph(const DevCorpus &c, uint32_t g, uint32_t *out, uint32_t cap) {
  __shared__ uint32_t s_scan[KO_BLOCK / 64];
  const uint32_t tid = threadIdx.x;
  const uint64_t n0 = c.node_off[g];
  const uint32_t V = (uint32_t)(c.node_off[g + 1] - n0);
  if (!V) return 0u;
  const uint32_t skipw = (uint32_t)(n0 & 3u), skipf = (uint32_t)((n0 + g) & 3u);
  const uint4 *w4 = reinterpret_cast<const uint4 *>(c.word + (n0 - skipw));
  const uint4 *f4 = reinterpret_cast<const uint4 *>(c.fp + (n0 + g - skipf));
  const uint32_t nck = (V + skipw + 3u) / 4u, nckf = (V + 1u + skipf + 3u) / 4u;
  const int d = (int)skipf - (int)skipw;  // node x of the word chunks has row pointer x + d of the fp chunks
  uint32_t carry = 0;
  for (uint32_t base = 0; base < nck; base += KO_Q * KO_BLOCK) {
    uint4 w[KO_Q], fa[KO_Q], fb[KO_Q];
#pragma unroll
    for (int q = 0; q < KO_Q; q++) {
      const uint32_t k = min(base + tid * KO_Q + (uint32_t)q, nck - 1u);
      const int p = 4 * (int)k + d;
      const uint32_t kf = p < 0 ? 0u : (uint32_t)p >> 2;
      w[q] = w4[k];
      fa[q] = f4[min(kf, nckf - 1u)];
      fb[q] = f4[min(kf + 1u, nckf - 1u)];
    }
    uint32_t m = 0;  // bit 4 q + b: node b of chunk q is a sink goal
#pragma unroll
    for (int q = 0; q < KO_Q; q++) {
      const uint32_t k = base + tid * KO_Q + (uint32_t)q;
      const uint32_t ww[4] = {w[q].x, w[q].y, w[q].z, w[q].w};
      const int p = 4 * (int)min(k, nck - 1u) + d;
      const int o = p - 4 * (int)(p < 0 ? 0u : (uint32_t)p >> 2);  // the node's row pointer in the two fp chunks
#pragma unroll
      for (int b = 0; b < 4; b++) {
        const uint32_t x = 4u * k + (uint32_t)b;
        const bool ok = k < nck && x >= skipw && x - skipw < V && !is_rule(ww[b]);
        const bool empty = pick8(fa[q], fb[q], o + b) == pick8(fa[q], fb[q], o + b + 1);
        m |= (ok && empty) ? 1u << (4 * q + b) : 0u;
      }
    }
    uint32_t tot;
    uint32_t ex = block_exscan<KO_BLOCK>((uint32_t)__popc(m), &tot, s_scan) + carry;
    if (WRITE) {
#pragma unroll
      for (int j = 0; j < 4 * KO_Q; j++) {
        if (!((m >> j) & 1u)) continue;
        const uint32_t x = 4u * (base + tid * KO_Q) + (uint32_t)j;
        if (ex < cap) out[ex] = x - skipw;
        ex++;
      }
    }
    carry += tot;
  }
  return carry;
}

// blockIdx.x = list position.  write 0: (sink goals, Kahn levels) of the graph to a.cnt; 1: the sink goals to
// a.leaf at the position's first hypothesis (a.loff, the host's prefix of the counts)
__global__ __launch_bounds__(KO_BLOCK) void k_ko_leaves(DevCorpus c, KnockArgs a, uint32_t write) {
  const uint32_t i = blockIdx.x, g = a.list[i];
  if (write) {
    const uint32_t lo = a.loff[i];
    ko_leaves_graph<true>(c, g, a.leaf + lo, a.loff[i + 1] - lo);
  } else {
    const uint32_t n = ko_leaves_graph<false>(c, g, nullptr, 0u);
    if (threadIdx.x == 0) {
      a.cnt[2u * i] = n;
      a.cnt[2u * i + 1u] = c.nlev[g];
    }
  }
}

void launch_ko_leaves(const DevCorpus &c, const KnockArgs &a, bool write, hipStream_t s) {
  if (!a.n_list) return;
  hipLaunchKernelGGL(k_ko_leaves, dim3(a.n_list), dim3(KO_BLOCK), 0, s, c, a, write ? 1u : 0u);
}

// ---- the sweep (KoImg, the two tiers' images, ko_zero_dead and ko_sweep: ko_sweep.h) ----------------
// lane b's return value: how many of the wave's 64 words have bit b set (a ballot per bit column)
__device__ __forceinline__ uint32_t ko_colcount(uint64_t w) {
  if (__ballot(w != 0ull) == 0ull) return 0u;
  const uint32_t lane = lane_id(), lo = (uint32_t)w, hi = (uint32_t)(w >> 32);
  uint32_t r = 0;
#pragma unroll
  for (int b = 0; b < 32; b++) {
    const uint64_t m = __ballot((lo >> b) & 1u);
    r = lane == (uint32_t)b ? (uint32_t)__popcll(m) : r;
  }
#pragma unroll
  for (int b = 0; b < 32; b++) {
    const uint64_t m = __ballot((hi >> b) & 1u);
    r = lane == 32u + (uint32_t)b ? (uint32_t)__popcll(m) : r;
  }
  return r;
}

// One chunk on a staged graph whose dead words are zero: seed, sweep, count, rows.  All 256 threads.
template <bool LDS>
__device__ __forceinline__ void ko_run(const KnockArgs &a, const KoChunk &k, const KoImg<LDS> &g) {
  __shared__ uint32_t s_cnt[2][KO_BLOCK / 64][64];
  const uint32_t tid = threadIdx.x, lane = lane_id(), wave = tid >> 6;
  uint64_t *dead = g.dead;
  // seeds: the chunk's own bits into the words of its F nodes
  if (!a.set_off) {
    if (tid < k.n) {
      const uint32_t leaf = a.leaf[k.first + tid];
      if (leaf < g.V) dead[leaf] = 1ull << tid;  // one sink goal per hypothesis, all distinct
    }
  } else {
    for (uint32_t s = wave; s < k.n; s += KO_BLOCK / 64) {  // several sets may name one node: atomic OR
      const uint64_t lo = a.set_off[k.first + s], hi = a.set_off[k.first + s + 1u];
      for (uint64_t j = lo + lane; j < hi; j += 64u) {
        const uint32_t v = a.leaf[j];
        if (v < g.V) atomicOr(reinterpret_cast<unsigned long long *>(&dead[v]), 1ull << s);
      }
    }
  }
  if (!LDS) __threadfence_block();
  __syncthreads();
  ko_sweep<LDS>(g);
  // per bit column: dead nodes, and dead nodes of level 0
  const uint32_t n_roots = g.L ? (uint32_t)g.lvl[1] : 0u;
  uint32_t cd = 0, cr = 0;
  for (uint32_t base = wave * 64u; base < g.V; base += KO_BLOCK) {
    const uint32_t v = base + lane;
    cd += ko_colcount(v < g.V ? dead[v] : 0ull);
  }
  for (uint32_t base = wave * 64u; base < n_roots; base += KO_BLOCK) {
    const uint32_t i = base + lane;
    cr += ko_colcount(i < n_roots ? dead[g.topo[i]] : 0ull);
  }
  s_cnt[0][wave][lane] = cd;
  s_cnt[1][wave][lane] = cr;
  __syncthreads();
  if (tid < k.n) {  // lane b of wave 0 writes hypothesis b's row
    uint32_t nd = 0, rd = 0;
#pragma unroll
    for (int w = 0; w < KO_BLOCK / 64; w++) {
      nd += s_cnt[0][w][tid];
      rd += s_cnt[1][w][tid];
    }
    uint32_t *row = a.rows + 5ull * (k.first + tid);
    row[0] = k.graph;
    row[1] = a.set_off ? NEMO_NONE : a.leaf[k.first + tid];
    row[2] = nd;
    row[3] = rd;
    row[4] = n_roots;
  }
}

// blockIdx.x = a chunk of the LDS tier.  The image: dead words, forward rows, Kahn order and level offsets as
// u16, a rule bit per node (knock_lds_bytes): a level step never goes to device memory.
__global__ __launch_bounds__(KO_BLOCK) void k_ko_lds(DevCorpus c, KnockArgs a) {
  extern __shared__ __align__(16) uint8_t dyn[];
  const uint32_t tid = threadIdx.x;
  const KoChunk k = ko_chunk(a, a.sel[blockIdx.x]);
  const GraphView gv = c.view(k.graph);
  const KoImg<true> g = ko_stage_image(gv, dyn);
  ko_zero_dead<true>(g);  // its barrier ends the staging
  ko_run<true>(a, k, g);
  if (a.masks) {  // the V words out in 16-byte stores (ko_run ends behind a barrier)
    const uint4 *z = reinterpret_cast<const uint4 *>(g.dead);
    uint4 *o = reinterpret_cast<uint4 *>(a.dead + k.moff);
    const uint32_t pairs = (gv.V + 1u) / 2u;
    for (uint32_t i = tid; i < pairs; i += KO_BLOCK) o[i] = z[i];
  }
}

// blockIdx.x = a chunk of the global tier: the same sweep over the CSR in device memory, the dead words in the
// chunk's own region of a.dead (which is also its mask).  Correct, not tuned.
__global__ __launch_bounds__(KO_BLOCK) void k_ko_glob(DevCorpus c, KnockArgs a) {
  const KoChunk k = ko_chunk(a, a.sel[blockIdx.x]);
  const KoImg<false> g = ko_glob_image(c.view(k.graph), a.dead + k.moff);  // pointers only: nothing to order with the zeroing
  ko_zero_dead<false>(g);
  ko_run<false>(a, k, g);
}

void launch_ko_lds(const DevCorpus &c, const KnockArgs &a, uint32_t n, uint32_t lds_bytes, hipStream_t s) {
  if (!n) return;
  hipFuncSetAttribute((const void *)k_ko_lds, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
  hipLaunchKernelGGL(k_ko_lds, dim3(n), dim3(KO_BLOCK), lds_bytes, s, c, a);
}

void launch_ko_glob(const DevCorpus &c, const KnockArgs &a, uint32_t n, hipStream_t s) {
  if (!n) return;
  hipLaunchKernelGGL(k_ko_glob, dim3(n), dim3(KO_BLOCK), 0, s, c, a);
}

}  // namespace nemo
