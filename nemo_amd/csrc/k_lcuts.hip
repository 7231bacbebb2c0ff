// k_lcuts.hip — nemo_min_label_cuts (DESIGN.md §Minimal cut sets by label): all minimal sets of <= 3 candidate
// labels whose loss defeats the outcome on at least q of the listed graphs.  It joins k_cuts.hip and k_klabel.hip:
// a round's hypotheses are the sets of 1, 2 or 3 live candidate positions in colex rank order (cut_host.h), so
// nothing but the candidate labels is uploaded; the work items are (list position, chunk range) in contiguous
// blocks per workgroup (klabel_host.h).  k_lc_table hashes the candidates into one label -> position table.
// k_lc_lds is persistent: on a new list position it stages the graph's LDS image (ko_sweep.h, which also holds the
// global tier's image, the zeroing, the sweep, the lost word and the column sums) and groups the
// graph's hit nodes by live position; per chunk a lane unranks its set, ORs its bit into the nodes of its 1 to 3
// rows, the workgroup sweeps and writes one lost word.  k_lc_glob is the same loop over the CSR in device memory.
// k_lc_reduce counts a chunk's bit columns over the list positions against q (round 3: and clears the triples that
// hold a cut pair); k_cut_count / launch_scan / k_cut_emit (k_cuts.hip) turn the cut words into rows and
// k_lc_support recounts a row's column, its n_lost.
#include "device.h"
#include "hit_list.h"
#include "internal.h"
#include "ko_sweep.h"
#include "lcut_host.h"

namespace nemo {

// A thread per candidate: its label's slot takes the candidate position.  The labels are distinct and the table
// is zero; at most half of the slots are taken, so a probe chain ends.
__global__ __launch_bounds__(KO_BLOCK) void k_lc_table(LcArgs a) {
  const uint32_t p = blockIdx.x * KO_BLOCK + threadIdx.x;
  if (p >= a.n_cand) return;
  const uint32_t label = a.cand[p];
  uint64_t h = klabel::first_slot(label, a.slots);
  while (atomicCAS(&a.key[h], 0u, label + 1u) != 0u) h = klabel::next_slot(h, a.slots);
  a.val[h] = p;
}

// the live position of node v's label in this round: LC_NONE if the node carries no label, the table does not hold
// it, its candidate is not live, or (a.sinks) the node is no sink goal.  Behind the barrier that ends the staging.
template <bool LDS>
__device__ __forceinline__ uint32_t lc_live(const LcArgs &a, const KoImg<LDS> &g, uint32_t v, uint32_t label) {
  if (label == LC_NONE) return LC_NONE;
  if (a.sinks && (g.is_rule_node(v) || g.fp[v] != g.fp[v + 1u])) return LC_NONE;
  uint64_t h = klabel::first_slot(label, a.slots);
  for (;;) {
    const uint32_t k = a.key[h];
    if (k == label + 1u) return a.lmap[a.val[h]];
    if (k == 0u) return LC_NONE;
    h = klabel::next_slot(h, a.slots);
  }
}

// The workgroup's block of work items: item t is (list position a.pos[t / parts], chunk range t % parts).  A new
// list position stages its graph and groups its hit nodes by live position: count, scan, scatter.  Every chunk of
// the range zeroes the dead words, seeds them from the rows its 64 sets name, sweeps and writes the lost word
// (round 1: and the hit word).  A chunk whose sets hit nothing on the graph loses nothing: no sweep.  All 256
// threads.
template <bool LDS, uint32_t SIZE>
__device__ __forceinline__ void lc_loop(const DevCorpus &c, const LcArgs &a, uint8_t *dyn) {
  __shared__ uint64_t s_w[KO_BLOCK / 64];
  __shared__ uint64_t s_hit;
  const uint32_t tid = threadIdx.x, lane = lane_id(), wave = tid >> 6;
  uint64_t *reg = a.region + (uint64_t)blockIdx.x * a.region_words;
  const uint32_t items = a.n_tier * a.parts;
  const uint32_t t_lo = (uint32_t)klabel::item_lo(items, gridDim.x, blockIdx.x);
  const uint32_t t_hi = (uint32_t)klabel::item_lo(items, gridDim.x, blockIdx.x + 1u);
  const uint32_t k1 = a.k1;
  LcList ls;
  ls.head = reinterpret_cast<uint32_t *>(dyn), ls.cap = 0u;
  ls.spill = reinterpret_cast<uint32_t *>(LDS ? reg : reg + a.dead_words);
  uint32_t cur = ~0u, pos = 0u;
  KoImg<LDS> g{};  // set with the first item (cur matches no list position)
  for (uint32_t t = t_lo; t < t_hi; t++) {
    const uint32_t ip = t / a.parts, part = t - ip * a.parts;
    if (ip != cur) {  // the previous image's and list's last reads lie behind the barrier that ended its last chunk
      cur = ip;
      pos = a.pos[ip];
      const GraphView gv = c.view(a.graph[pos]);
      g = ko_image(std::integral_constant<bool, LDS>{}, gv, dyn, reg);
      if (LDS) {
        const uint32_t image = knock::knock_lds_bytes(gv.V, gv.E, gv.nlev);
        ls.head = reinterpret_cast<uint32_t *>(dyn + image);
        ls.cap = (a.lds_total - image) / 4u;
      }
      // the graph's hit nodes by live position (hit_list.h): count, scan, scatter
      hit_list_build(ls, g.V, k1, [&](uint32_t v) { return lc_live<LDS>(a, g, v, gv.label[v]); });
    }
    uint64_t *dead = g.dead;
    const uint32_t c_lo = klabel::range_lo(a.n_chunks, a.parts, part), c_hi = klabel::range_lo(a.n_chunks, a.parts, part + 1u);
    for (uint32_t ci = c_lo; ci < c_hi; ci++) {
      ko_zero_dead<LDS>(g);
      const uint32_t first = ci * KO_CHUNK, n = min(KO_CHUNK, a.n_hyp - first);
      // seeds: lane t's hypothesis is the set of rank first + t; it ORs its bit into the nodes of its rows
      if (wave == 0u) {
        bool any = false;
        if (lane < n) {
          const cuts::Pos p = cuts::unrank<SIZE>((uint64_t)first + lane);
          unsigned long long *d64 = reinterpret_cast<unsigned long long *>(dead);
          const unsigned long long bit = 1ull << lane;
          const uint32_t row[3] = {p.a, p.b, p.c};
#pragma unroll
          for (uint32_t r = 0; r < SIZE; r++) {
            const uint32_t lo = row[r] ? ls.get(row[r] - 1u) : 0u, hi = ls.get(row[r]);
            any = any || hi > lo;
            for (uint32_t j = lo; j < hi; j++) atomicOr(&d64[ls.get(k1 + 1u + j)], bit);
          }
        }
        const uint64_t hw = __ballot(any);
        if (lane == 0u) s_hit = hw;
      }
      if (!LDS) __threadfence_block();
      __syncthreads();
      const uint64_t hit = s_hit;
      uint64_t lost = 0ull;
      // every thread has read the same word s_hit behind the barrier above (it is written next behind the next
      // chunk's first barrier), so the branch, and the barriers inside it, are taken by the whole workgroup or by
      // none of it
      if (hit != 0ull) {
        ko_sweep<LDS>(g);
        lost = ko_lost_word<LDS>(g, n, s_w);  // every root dead, per bit column
      }
      if (tid == 0u) {
        a.lost[(uint64_t)pos * a.n_chunks + ci] = lost;
        if (SIZE == 1u) a.hit[(uint64_t)pos * a.n_chunks + ci] = hit;
      }
    }
  }
}

// one instantiation per round (SIZE = 1, 2, 3)
template <uint32_t SIZE>
__global__ __launch_bounds__(KO_BLOCK) void k_lc_lds(DevCorpus c, LcArgs a) {
  extern __shared__ __align__(16) uint8_t dyn[];
  lc_loop<true, SIZE>(c, a, dyn);
}

// the workgroup's dead words and hit list in its region of a.region; a fence and a barrier per level, as
// k_kl_glob.  Correct, not tuned.
template <uint32_t SIZE>
__global__ __launch_bounds__(KO_BLOCK) void k_lc_glob(DevCorpus c, LcArgs a) {
  lc_loop<false, SIZE>(c, a, nullptr);
}

// A wave per chunk, a lane per bit: lane b counts the list positions whose lost word has bit b (a round reads the
// words of 64 list positions, one per lane, and every lane takes its bit of each), cut bit = count >= q.  Round 1
// also ORs the hit words; round 3 clears the triples one of whose pairs is a cut of round 2.  No count is kept.
template <uint32_t SIZE>
__global__ __launch_bounds__(KO_BLOCK) void k_lc_reduce(LcArgs a) {
  const uint32_t ci = blockIdx.x * (KO_BLOCK / 64) + (threadIdx.x >> 6), lane = lane_id();
  if (ci >= a.n_chunks) return;
  uint32_t cnt = 0;
  uint64_t anyhit = 0ull;
  for (uint32_t base = 0; base < a.n; base += 64u) {
    const uint32_t i = base + lane;
    const uint64_t x = i < a.n ? a.lost[(uint64_t)i * a.n_chunks + ci] : 0ull;
    if (SIZE == 1u && i < a.n) anyhit |= a.hit[(uint64_t)i * a.n_chunks + ci];
    cnt += ko_colsum((uint32_t)x, (uint32_t)(x >> 32));
  }
  uint64_t cut = __ballot(cnt >= a.q);
  if (SIZE == 1u) {
#pragma unroll
    for (int dd = 32; dd >= 1; dd >>= 1) anyhit |= (uint64_t)__shfl_xor((unsigned long long)anyhit, dd);
  }
  if (SIZE == 3u) {
    const uint64_t h = (uint64_t)ci * KO_CHUNK + lane;
    const bool sub = h < a.n_hyp && cuts::has_cut_pair(a.pairs, cuts::unrank<3>(h));
    cut &= ~__ballot(sub);
  }
  if (lane == 0u) {
    a.words[ci] = cut;
    if (SIZE == 1u) a.words[a.n_chunks + ci] = anyhit;
  }
}

// A wave per row of the round: the row's chunk by the scan (the last chunk whose first row is not past it), its
// bit the (row - first row)-th set bit of the chunk's cut word; the lanes then recount that column over the list
// positions.
__global__ __launch_bounds__(KO_BLOCK) void k_lc_support(LcArgs a) {
  const uint32_t r = blockIdx.x * (KO_BLOCK / 64) + (threadIdx.x >> 6), lane = lane_id();
  if (r >= a.n_rows) return;
  uint32_t lo = 0, hi = a.n_chunks;
  while (hi - lo > 1u) {
    const uint32_t mid = lo + (hi - lo) / 2u;
    if (a.scan[mid] <= r) lo = mid;
    else hi = mid;
  }
  uint64_t w = a.words[lo];
  for (uint32_t k = r - a.scan[lo]; k; k--) w &= w - 1ull;
  const uint32_t bit = (uint32_t)__ffsll((long long)w) - 1u;
  uint32_t cnt = 0;
  for (uint32_t base = 0; base < a.n; base += 64u) {
    const uint32_t i = base + lane;
    const uint64_t x = i < a.n ? a.lost[(uint64_t)i * a.n_chunks + lo] : 0ull;
    cnt += (uint32_t)__popcll(__ballot(((x >> bit) & 1ull) != 0ull));
  }
  if (lane == 0u) a.n_lost[r] = cnt;
}

void launch_lc_table(const LcArgs &a, hipStream_t s) {
  if (!a.n_cand) return;
  hipLaunchKernelGGL(k_lc_table, dim3((a.n_cand + KO_BLOCK - 1u) / KO_BLOCK), dim3(KO_BLOCK), 0, s, a);
}

static const void *lc_lds_kernel(uint32_t size) {
  const void *f = nullptr;
  ko_by_size(size, [&](auto sz) { f = (const void *)k_lc_lds<decltype(sz)::value>; });
  return f;
}

uint32_t lc_lds_resident(uint32_t size, uint32_t lds_bytes, uint32_t n_cu) { return ko_lds_resident(lc_lds_kernel(size), lds_bytes, n_cu); }

void launch_lc_lds(const DevCorpus &c, const LcArgs &a, uint32_t grid, hipStream_t s) {
  if (!a.n_tier || !a.n_chunks) return;
  hipFuncSetAttribute(lc_lds_kernel(a.size), hipFuncAttributeMaxDynamicSharedMemorySize, (int)a.lds_total);
  ko_by_size(a.size, [&](auto sz) { hipLaunchKernelGGL(k_lc_lds<decltype(sz)::value>, dim3(grid), dim3(KO_BLOCK), a.lds_total, s, c, a); });
}

void launch_lc_glob(const DevCorpus &c, const LcArgs &a, uint32_t grid, hipStream_t s) {
  if (!a.n_tier || !a.n_chunks) return;
  ko_by_size(a.size, [&](auto sz) { hipLaunchKernelGGL(k_lc_glob<decltype(sz)::value>, dim3(grid), dim3(KO_BLOCK), 0, s, c, a); });
}

void launch_lc_reduce(const LcArgs &a, hipStream_t s) {
  if (!a.n_chunks) return;
  const dim3 grid((a.n_chunks + KO_BLOCK / 64 - 1u) / (KO_BLOCK / 64));
  ko_by_size(a.size, [&](auto sz) { hipLaunchKernelGGL(k_lc_reduce<decltype(sz)::value>, grid, dim3(KO_BLOCK), 0, s, a); });
}

void launch_lc_support(const LcArgs &a, hipStream_t s) {
  if (!a.n_rows || !a.n_chunks) return;
  hipLaunchKernelGGL(k_lc_support, dim3((a.n_rows + KO_BLOCK / 64 - 1u) / (KO_BLOCK / 64)), dim3(KO_BLOCK), 0, s, a);
}

}  // namespace nemo
