// k_lrepair.hip — nemo_lineage_repair_sets / nemo_lineage_repairs (DESIGN.md §Lineage repair search): the hitting-set
// tree over blockers, the dual of k_lineage.hip's tree over surviving derivations, one level per pair of launches.
// k_lrep_lds / k_lrep_glob are persistent over chunks of 64 frontier sets of the one graph, staged once per workgroup
// with the absent bitmap behind it: a chunk fills the dead words from the bitmap and clears its sets' columns on the
// nodes they restore (cut_dev.h's repair seeding; the same words, kept apart from the sweep, are the stop rule's),
// runs the knock-out sweep (ko_sweep.h), takes the lost word, appends the holding sets to the repairs' list and table,
// runs the top-down blame pass (blame_down.h) and then, with the blame words still where the pass left them (LDS on
// the LDS tier), emits (set h) + {k} for every candidate position k and every bit h under which cand[k] is blamed and
// not restored, at lin_dev.h's wave-aggregated claim.  The next frontier is k_lineage.hip's k_lin_filter's, the
// repairs' table k_lin_rehash's.  With a.status set one workgroup evaluates two hypotheses instead, S = {} and
// S = every candidate, and leaves their lost word: what round 0 of nemo_min_repair_sets decides.  No thread waits for
// another anywhere.
#include "blame_down.h"
#include "device.h"
#include "internal.h"
#include "ko_sweep.h"
#include "lin_dev.h"
#include "lrep_host.h"

namespace nemo {

// dead[v] = removed[v] = absent(v) ? ~0 : 0, in whole 16-byte pairs as cut_dev.h's repair_fill writes the dead words
// alone; a fence and a barrier behind them.  The caller's last reads of both lie behind a barrier, and so does the
// staging of the bitmap.  All 256 threads.
template <bool LDS>
__device__ __forceinline__ void lrep_fill(const KoImg<LDS> &g, const uint64_t *absent, uint64_t *removed) {
  uint4 *z = reinterpret_cast<uint4 *>(g.dead), *r = reinterpret_cast<uint4 *>(removed);
  const uint32_t pairs = (g.V + 1u) / 2u;
  for (uint32_t i = threadIdx.x; i < pairs; i += KO_BLOCK) {
    const uint32_t v = 2u * i;
    const uint32_t two = (uint32_t)(absent[v >> 6] >> (v & 63u)) & 3u;
    const uint32_t lo = (two & 1u) ? ~0u : 0u, hi = (two & 2u) ? ~0u : 0u;
    z[i] = r[i] = make_uint4(lo, lo, hi, hi);
  }
  if (!LDS) __threadfence_block();
  __syncthreads();
}

// One chunk ci of the frontier on the staged graph.  Ends behind a barrier.  All 256 threads.
template <bool LDS>
__device__ __forceinline__ void lrep_chunk(const LinArgs &a, const KoImg<LDS> &g, const uint64_t *absent, uint64_t *blame, uint64_t *removed,
                                           uint32_t ci) {
  __shared__ uint64_t s_w[KO_BLOCK / 64];
  __shared__ uint64_t s_key[KO_CHUNK][2];
  const uint32_t tid = threadIdx.x, lane = lane_id(), wave = tid >> 6;
  const uint32_t first = ci * KO_CHUNK, n = min(KO_CHUNK, a.n_front - first);
  unsigned long long *d64 = reinterpret_cast<unsigned long long *>(g.dead), *r64 = reinterpret_cast<unsigned long long *>(removed);
  lrep_fill<LDS>(g, absent, removed);  // its barrier: the staging's end, and the previous chunk's last reads of s_key
  lin_stage_keys(a.front, first, n, s_key);
  // seeds: a thread per (set, field) clears the set's column on the node it restores, in both arrays; several sets may
  // name one candidate: atomic AND
  for (uint32_t t = tid; t < n * LIN_MAX_SIZE; t += KO_BLOCK) {
    const uint32_t s = t / LIN_MAX_SIZE, j = t % LIN_MAX_SIZE;
    const uint32_t p = lin::key_at(lin_load(a.front, first + s), j);
    if (p < a.K) {
      const uint32_t v = a.cand[p];
      if (v < g.V) {
        atomicAnd(&d64[v], ~(1ull << s));
        atomicAnd(&r64[v], ~(1ull << s));
      }
    }
  }
  if (!LDS) __threadfence_block();
  __syncthreads();
  ko_sweep<LDS>(g);
  const uint64_t lost = ko_lost_word<LDS>(g, n, s_w);
  const uint64_t tail = n == KO_CHUNK ? ~0ull : (1ull << n) - 1ull;
  const uint64_t holds = tail & ~lost;
  // the holding sets are minimal repairs: one claim for the chunk, lane h of wave 0 takes set h
  if (wave == 0u && holds != 0ull && !a.redo) {
    uint32_t base = 0;
    if (lane == 0u) base = (uint32_t)atomicAdd(a.ctr, (unsigned long long)__popcll(holds));
    base = (uint32_t)__shfl((int)base, 0);
    if ((holds >> lane) & 1ull) {
      const uint32_t i = base + (uint32_t)__popcll(holds & ((1ull << lane) - 1ull));
      const lin::Key k{s_key[lane][0], s_key[lane][1]};
      lin_store(a.cuts, i, k);
      lin_cut_insert(a, i, k);
    }
  }
  // the children of the lost sets (workgroup-uniform: every thread holds the lost word): the blocker, then a thread per
  // candidate position, a wave-wide claim per 64 positions.  A blamed candidate is blamed under lost bits only; the
  // bits under which it is restored go (it may still be blamed there: dead through its children).
  if (a.emit && lost != 0ull) {
    blame_down<LDS>(g, blame, removed, lost);
    for (uint32_t kb = wave * 64u; kb < a.K; kb += KO_BLOCK) {
      const uint32_t k = kb + lane;
      uint64_t w = 0ull;
      if (k < a.K) {
        const uint32_t v = a.cand[k];
        if (v < g.V) w = wit_need<LDS>(&blame[v]) & wit_need<LDS>(&removed[v]) & lost;
      }
      lin_emit(a, s_key, k, w);
    }
  }
  __syncthreads();  // the image's, the words' and s_key's last reads
}

// The two hypotheses that decide the status, on the staged graph: column 0 restores nothing, column 1 every candidate
// (distinct nodes; atomic as the chunks' seeds).  ctr[3] = the lost word.  All 256 threads of one workgroup.
template <bool LDS>
__device__ __forceinline__ void lrep_status(const LinArgs &a, const KoImg<LDS> &g, const uint64_t *absent, uint64_t *removed) {
  __shared__ uint64_t s_st[KO_BLOCK / 64];
  unsigned long long *d64 = reinterpret_cast<unsigned long long *>(g.dead);
  lrep_fill<LDS>(g, absent, removed);
  for (uint32_t k = threadIdx.x; k < a.K; k += KO_BLOCK) {
    const uint32_t v = a.cand[k];
    if (v < g.V) atomicAnd(&d64[v], ~2ull);
  }
  if (!LDS) __threadfence_block();
  __syncthreads();
  ko_sweep<LDS>(g);
  const uint64_t lost = ko_lost_word<LDS>(g, 2u, s_st);
  if (threadIdx.x == 0u) a.ctr[3] = lost;
}

__global__ __launch_bounds__(KO_BLOCK) void k_lrep_lds(DevCorpus c, LrepArgs a) {
  extern __shared__ __align__(16) uint8_t dyn[];
  const GraphView gv = c.view(a.l.graph);
  const KoImg<true> g = ko_stage_image(gv, dyn);
  uint64_t *blame = reinterpret_cast<uint64_t *>(dyn + lrep::blame_offset(gv.V, gv.E, gv.nlev));
  uint64_t *removed = reinterpret_cast<uint64_t *>(dyn + lrep::removed_offset(gv.V, gv.E, gv.nlev));
  uint64_t *absent = reinterpret_cast<uint64_t *>(dyn + lrep::bitmap_offset(gv.V, gv.E, gv.nlev));
  {  // the bitmap, once per workgroup: whole 16-byte pairs
    const uint4 *src = reinterpret_cast<const uint4 *>(a.absent);
    uint4 *dst = reinterpret_cast<uint4 *>(absent);
    const uint32_t n4 = (uint32_t)(repair::bitmap_words(gv.V) / 2u);
    for (uint32_t i = threadIdx.x; i < n4; i += KO_BLOCK) dst[i] = src[i];
  }
  __syncthreads();  // the image and the bitmap are staged
  if (a.status) {
    lrep_status<true>(a.l, g, absent, removed);
    return;
  }
  for (uint32_t ci = blockIdx.x; ci < a.l.n_chunks; ci += gridDim.x) lrep_chunk<true>(a.l, g, absent, blame, removed, ci);
}

// the workgroup's dead, blame and stop-rule words in its region of a.l.region, the bitmap read where it lies; a fence
// and a barrier per level
__global__ __launch_bounds__(KO_BLOCK) void k_lrep_glob(DevCorpus c, LrepArgs a) {
  const GraphView gv = c.view(a.l.graph);
  uint64_t *reg = a.l.region + (uint64_t)blockIdx.x * a.l.region_words;
  const uint64_t dw = knock::dead_words(gv.V);
  const KoImg<false> g = ko_glob_image(gv, reg);
  uint64_t *blame = reg + dw, *removed = reg + 2ull * dw;
  if (a.status) {
    lrep_status<false>(a.l, g, a.absent, removed);
    return;
  }
  for (uint32_t ci = blockIdx.x; ci < a.l.n_chunks; ci += gridDim.x) lrep_chunk<false>(a.l, g, a.absent, blame, removed, ci);
}

uint32_t lrep_lds_resident(uint32_t lds_bytes, uint32_t n_cu) { return ko_lds_resident((const void *)k_lrep_lds, lds_bytes, n_cu); }

void launch_lrep_lds(const DevCorpus &c, const LrepArgs &a, uint32_t grid, hipStream_t s) {
  if (!a.l.n_chunks && !a.status) return;
  hipFuncSetAttribute((const void *)k_lrep_lds, hipFuncAttributeMaxDynamicSharedMemorySize, (int)a.l.lds_total);
  hipLaunchKernelGGL(k_lrep_lds, dim3(a.status ? 1u : grid), dim3(KO_BLOCK), a.l.lds_total, s, c, a);
}

void launch_lrep_glob(const DevCorpus &c, const LrepArgs &a, uint32_t grid, hipStream_t s) {
  if (!a.l.n_chunks && !a.status) return;
  hipLaunchKernelGGL(k_lrep_glob, dim3(a.status ? 1u : grid), dim3(KO_BLOCK), 0, s, c, a);
}

}  // namespace nemo
