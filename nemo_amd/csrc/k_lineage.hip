// k_lineage.hip — nemo_lineage_cuts (DESIGN.md §Lineage-driven cut search): the hitting-set tree over surviving
// derivations, one level per pair of launches.  k_lin_lds / k_lin_glob are persistent over chunks of 64 frontier sets
// of the one graph, staged once per workgroup: a chunk seeds the dead words from its sets' candidate positions, runs
// the knock-out sweep (ko_sweep.h), takes the lost word, runs the top-down need pass (wit_down.h) and then, with the
// need words still where the pass left them (LDS on the LDS tier: they never reach device memory there), emits
// (set h) + {k} for every candidate position k and every bit h of need[cand[k]] that is valid and not lost, at a
// wave-aggregated claim on a global cursor; the lost sets go to the cuts' list and table.  The cursor counts past the
// buffer's end, nothing is written there.  k_lin_filter makes the next frontier of the children: exact duplicate
// removal in an open-addressing table of child indices (one atomicCAS per probe, the keys compared in the emission
// buffer the launch before wrote whole), the test of every proper subset against the cuts' table, and a ballot /
// prefix-sum compaction.  No thread waits for another anywhere.
#include "device.h"
#include "internal.h"
#include "ko_sweep.h"
#include "lin_dev.h"
#include "lin_host.h"
#include "wit_down.h"
#include "wit_host.h"

namespace nemo {

static_assert(LIN_BLOCK == KO_BLOCK, "lin_host.h sizes k_lin_filter's grid by KO_BLOCK threads");

// One chunk ci of the frontier on the staged graph.  Ends behind a barrier.  All 256 threads.
template <bool LDS>
__device__ __forceinline__ void lin_chunk(const LinArgs &a, const KoImg<LDS> &g, uint64_t *need, uint32_t ci) {
  __shared__ uint64_t s_w[KO_BLOCK / 64];
  __shared__ uint64_t s_key[KO_CHUNK][2];
  const uint32_t tid = threadIdx.x, lane = lane_id(), wave = tid >> 6;
  const uint32_t first = ci * KO_CHUNK, n = min(KO_CHUNK, a.n_front - first);
  uint64_t *dead = g.dead;
  ko_zero_dead<LDS>(g);  // its barrier: the staging's end, and the previous chunk's last reads of s_key
  lin_stage_keys(a.front, first, n, s_key);
  // seeds: a thread per (set, field); several sets may name one candidate: atomic OR
  for (uint32_t t = tid; t < n * LIN_MAX_SIZE; t += KO_BLOCK) {
    const uint32_t s = t / LIN_MAX_SIZE, j = t % LIN_MAX_SIZE;
    const uint32_t p = lin::key_at(lin_load(a.front, first + s), j);
    if (p < a.K) {
      const uint32_t v = a.cand[p];
      if (v < g.V) wit_or(&dead[v], 1ull << s);
    }
  }
  if (!LDS) __threadfence_block();
  __syncthreads();
  ko_sweep<LDS>(g);
  const uint64_t lost = ko_lost_word<LDS>(g, n, s_w);
  wit_down<LDS>(g, need, n, false);
  const uint64_t tail = n == KO_CHUNK ? ~0ull : (1ull << n) - 1ull;
  const uint64_t live = tail & ~lost;
  // the lost sets are minimal cuts: one claim for the chunk, lane h of wave 0 takes set h
  if (wave == 0u && lost != 0ull && !a.redo) {
    uint32_t base = 0;
    if (lane == 0u) base = (uint32_t)atomicAdd(a.ctr, (unsigned long long)__popcll(lost));
    base = (uint32_t)__shfl((int)base, 0);
    if ((lost >> lane) & 1ull) {
      const uint32_t i = base + (uint32_t)__popcll(lost & ((1ull << lane) - 1ull));
      const lin::Key k{s_key[lane][0], s_key[lane][1]};
      lin_store(a.cuts, i, k);
      lin_cut_insert(a, i, k);
    }
  }
  // the children: a thread per candidate position, a wave-wide claim per 64 positions
  if (a.emit && live != 0ull) {
    for (uint32_t kb = wave * 64u; kb < a.K; kb += KO_BLOCK) {
      const uint32_t k = kb + lane;
      uint64_t w = 0ull;
      if (k < a.K) {
        const uint32_t v = a.cand[k];
        if (v < g.V) w = wit_need<LDS>(&need[v]) & live;
      }
      lin_emit(a, s_key, k, w);
    }
  }
  __syncthreads();  // the image's, the words' and s_key's last reads
}

template <bool LDS>
__device__ __forceinline__ void lin_loop(const DevCorpus &c, const LinArgs &a, uint8_t *dyn) {
  uint64_t *reg = a.region + (uint64_t)blockIdx.x * a.region_words;
  const GraphView gv = c.view(a.graph);
  const KoImg<LDS> g = ko_image(std::integral_constant<bool, LDS>{}, gv, dyn, reg);
  uint64_t *need = LDS ? reinterpret_cast<uint64_t *>(dyn + knock::knock_lds_bytes(gv.V, gv.E, gv.nlev)) : reg + a.region_words / 2u;
  for (uint32_t ci = blockIdx.x; ci < a.n_chunks; ci += gridDim.x) lin_chunk<LDS>(a, g, need, ci);  // its first barrier ends the staging
}

__global__ __launch_bounds__(KO_BLOCK) void k_lin_lds(DevCorpus c, LinArgs a) {
  extern __shared__ __align__(16) uint8_t dyn[];
  lin_loop<true>(c, a, dyn);
}

// the workgroup's dead and need words in its region of a.region; a fence and a barrier per level
__global__ __launch_bounds__(KO_BLOCK) void k_lin_glob(DevCorpus c, LinArgs a) { lin_loop<false>(c, a, nullptr); }

// is k in the cuts' table?
__device__ __forceinline__ bool lin_is_cut(const LinArgs &a, const lin::Key &k) {
  uint64_t h = lin::first_slot(k, a.cslots);
  for (;;) {  // ends: at most half of the slots are taken
    const uint32_t e = a.ctab[h];
    if (!e) return false;
    if (lin::key_eq(lin_load(a.cuts, e - 1u), k)) return true;
    h = lin::next_slot(h, a.cslots);
  }
}

// The next frontier of the children a.kids[0 .. ctr[1]): a grid-stride loop, a thread per child.  A level that
// counted past the buffer is left alone: the host grows the buffer and runs the level again.
__global__ __launch_bounds__(KO_BLOCK) void k_lin_filter(LinArgs a) {
  const unsigned long long n = a.ctr[1];
  if (n > a.kids_cap) return;
  const uint32_t lane = lane_id();
  const uint32_t sizes = a.cut_sizes | (a.ctr[0] > a.cuts_before ? 1u << a.size : 0u);
  for (uint64_t base = (uint64_t)blockIdx.x * KO_BLOCK; base < n; base += (uint64_t)gridDim.x * KO_BLOCK) {  // workgroup-uniform
    const uint64_t i = base + threadIdx.x;
    bool keep = i < n;
    lin::Key k = lin::key_empty();
    if (keep) {
      k = lin_load(a.kids, i);
      uint64_t h = lin::first_slot(k, a.kslots);
      for (;;) {  // ends: at most half of the slots are taken; an entry never leaves its slot
        const uint32_t e = atomicCAS(&a.ktab[h], 0u, (uint32_t)i + 1u);
        if (!e) break;  // the slot is this child's: it stands for its set
        if (lin::key_eq(lin_load(a.kids, e - 1u), k)) {
          keep = false;  // the same set came first
          break;
        }
        h = lin::next_slot(h, a.kslots);
      }
    }
    if (keep && sizes) {  // a proper subset among the cuts: the child is no minimal cut and none lies below it
      const uint32_t m_end = lin::subset_masks(a.size + 1u);
      for (uint32_t m = 1; m <= m_end && keep; m++) {
        if (!((sizes >> __popc(m)) & 1u)) continue;
        if (lin_is_cut(a, lin::key_subset(k, m))) keep = false;
      }
    }
    const uint64_t b = __ballot(keep);
    if (!b) continue;
    unsigned long long at = 0;
    if (lane == 0u) at = atomicAdd(a.ctr + 2, (unsigned long long)__popcll(b));
    at = (unsigned long long)__shfl((unsigned long long)at, 0);
    if (keep) lin_store(a.next, at + (uint64_t)__popcll(b & ((1ull << lane) - 1ull)), k);
  }
}

// a thread per cut: its index into the zeroed table
__global__ __launch_bounds__(KO_BLOCK) void k_lin_rehash(LinArgs a, uint64_t n) {
  const uint64_t i = (uint64_t)blockIdx.x * KO_BLOCK + threadIdx.x;
  if (i < n) lin_cut_insert(a, (uint32_t)i, lin_load(a.cuts, i));
}

uint32_t lin_lds_resident(uint32_t lds_bytes, uint32_t n_cu) { return ko_lds_resident((const void *)k_lin_lds, lds_bytes, n_cu); }

void launch_lin_lds(const DevCorpus &c, const LinArgs &a, uint32_t grid, hipStream_t s) {
  if (!a.n_chunks) return;
  hipFuncSetAttribute((const void *)k_lin_lds, hipFuncAttributeMaxDynamicSharedMemorySize, (int)a.lds_total);
  hipLaunchKernelGGL(k_lin_lds, dim3(grid), dim3(KO_BLOCK), a.lds_total, s, c, a);
}

void launch_lin_glob(const DevCorpus &c, const LinArgs &a, uint32_t grid, hipStream_t s) {
  if (!a.n_chunks) return;
  hipLaunchKernelGGL(k_lin_glob, dim3(grid), dim3(KO_BLOCK), 0, s, c, a);
}

void launch_lin_filter(const LinArgs &a, uint32_t grid, hipStream_t s) {
  hipLaunchKernelGGL(k_lin_filter, dim3(grid), dim3(KO_BLOCK), 0, s, a);
}

void launch_lin_rehash(const LinArgs &a, uint64_t n, hipStream_t s) {
  if (!n) return;
  hipLaunchKernelGGL(k_lin_rehash, dim3((uint32_t)((n + KO_BLOCK - 1) / KO_BLOCK)), dim3(KO_BLOCK), 0, s, a, n);
}

}  // namespace nemo
