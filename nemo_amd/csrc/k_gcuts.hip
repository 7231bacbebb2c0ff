// k_gcuts.hip — nemo_min_group_cuts (DESIGN.md §Minimal cut sets over fault events): all minimal sets of <= 3
// candidates, each a group of labels, whose loss together defeats the outcome on at least q of the listed graphs.
// The rounds, the ranks, the work items and the lost words are k_lcuts.hip's; a set removes the union of its groups.
// k_gc_table hashes the labels the groups name into one label -> row table, a row per distinct label, and
// k_gc_rows rewrites the groups in place as lists of rows.  k_gc_lds is persistent: on a new list position it
// stages the graph's LDS image (ko_sweep.h) and groups the graph's hit nodes by row (hit_list.h): a node carries one
// label, so the list is D + 1 + V entries however many groups share a label.  Per chunk the first `SIZE` waves
// unrank the 64 sets and scan their groups' lengths, then all four waves walk the chunk's (set, group, label)
// triples: a triple whose row is empty on this graph costs two offsets, a short row is ORed in by its thread, a row
// past KO_HUB nodes by the whole wave.  The workgroup sweeps and writes one lost word.  k_gc_glob is the same loop
// over the CSR in device memory.  k_lc_reduce, k_lc_support (k_lcuts.hip) and k_cut_count / launch_scan /
// k_cut_emit (k_cuts.hip) turn the lost words into rows of candidate positions.
#include "device.h"
#include "gcut_host.h"
#include "hit_list.h"
#include "internal.h"
#include "ko_sweep.h"

namespace nemo {

// A thread per named label: the first to take the label's slot hands out its row.  The table and *n_rows are
// zero; at most half of the slots are taken, so a probe chain ends.
__global__ __launch_bounds__(KO_BLOCK) void k_gc_table(GcArgs a) {
  const uint32_t e = blockIdx.x * KO_BLOCK + threadIdx.x;
  if (e >= a.n_named) return;
  const uint32_t label = a.grow[e];
  uint64_t h = klabel::first_slot(label, a.r.slots);
  for (;;) {
    const uint32_t k = atomicCAS(&a.r.key[h], 0u, label + 1u);
    if (k == 0u) a.r.val[h] = atomicAdd(a.n_rows, 1u);
    if (k == 0u || k == label + 1u) return;
    h = klabel::next_slot(h, a.r.slots);
  }
}

// A thread per named label, behind k_gc_table: the label gives way to its row.
__global__ __launch_bounds__(KO_BLOCK) void k_gc_rows(GcArgs a) {
  const uint32_t e = blockIdx.x * KO_BLOCK + threadIdx.x;
  if (e >= a.n_named) return;
  const uint32_t label = a.grow[e];
  uint64_t h = klabel::first_slot(label, a.r.slots);
  while (a.r.key[h] != label + 1u) h = klabel::next_slot(h, a.r.slots);
  a.grow[e] = a.r.val[h];
}

// the row of node v's label: LC_NONE if the node carries no label, no group names it, or (a.r.sinks) the node is
// no sink goal.  Behind the barrier that ends the staging.
template <bool LDS>
__device__ __forceinline__ uint32_t gc_row(const GcArgs &a, const KoImg<LDS> &g, uint32_t v, uint32_t label) {
  if (label == LC_NONE) return LC_NONE;
  if (a.r.sinks && (g.is_rule_node(v) || g.fp[v] != g.fp[v + 1u])) return LC_NONE;
  uint64_t h = klabel::first_slot(label, a.r.slots);
  for (;;) {
    const uint32_t k = a.r.key[h];
    if (k == label + 1u) return a.r.val[h];
    if (k == 0u) return LC_NONE;
    h = klabel::next_slot(h, a.r.slots);
  }
}

// Thread (wave r < SIZE, lane t) of chunk ci: group r of the set of rank 64 ci + t as (first entry in a.grow,
// entries); (0, 0) past the round's hypotheses and for the other waves.
template <uint32_t SIZE>
__device__ __forceinline__ uint2 gc_pair(const GcArgs &a, uint32_t ci) {
  const uint32_t lane = lane_id(), wave = threadIdx.x >> 6;
  const uint64_t h = (uint64_t)ci * KO_CHUNK + lane;
  if (wave >= SIZE || h >= a.r.n_hyp) return make_uint2(0u, 0u);
  const cuts::Pos p = cuts::unrank<SIZE>(h);
  const uint32_t lp = wave == 0u ? p.a : wave == 1u ? p.b : p.c;
  const uint32_t k = a.live ? a.live[lp] : lp;
  const uint32_t beg = a.goff[k];
  return make_uint2(beg, a.goff[k + 1u] - beg);
}

// The workgroup's block of work items, as lc_loop's: item t is (list position a.r.pos[t / parts], chunk range
// t % parts).  A new list position stages its graph and groups its hit nodes by row.  Every chunk of the range
// zeroes the dead words, seeds them from the rows its 64 sets' groups name, sweeps and writes the lost word (round
// 1: and the hit word).  A chunk whose sets hit nothing on the graph loses nothing: no sweep.  All 256 threads.
template <bool LDS, uint32_t SIZE>
__device__ __forceinline__ void gc_loop(const DevCorpus &c, const GcArgs &a, uint8_t *dyn) {
  __shared__ uint64_t s_w[KO_BLOCK / 64];
  __shared__ uint32_t s_inc[SIZE * 64u];  // wave r: the inclusive scan of its 64 groups' lengths (u32: a group holds at most
                                          // GC_MAX_GROUP = 2^24 labels, so the three waves' totals stay below 192 x 2^24 < 2^32)
  __shared__ uint32_t s_beg[SIZE * 64u];  // ... and their first entries
  __shared__ uint32_t s_tot[3];           // ... and its total
  __shared__ uint32_t s_any[KO_CHUNK];    // set t hit a node of this graph
  const uint32_t tid = threadIdx.x, lane = lane_id(), wave = tid >> 6;
  uint64_t *reg = a.r.region + (uint64_t)blockIdx.x * a.r.region_words;
  const uint32_t items = a.r.n_tier * a.r.parts;
  const uint32_t t_lo = (uint32_t)klabel::item_lo(items, gridDim.x, blockIdx.x);
  const uint32_t t_hi = (uint32_t)klabel::item_lo(items, gridDim.x, blockIdx.x + 1u);
  const uint32_t D = a.n_dist;
  LcList ls;
  ls.head = reinterpret_cast<uint32_t *>(dyn), ls.cap = 0u;
  ls.spill = reinterpret_cast<uint32_t *>(LDS ? reg : reg + a.r.dead_words);
  uint32_t cur = ~0u, pos = 0u;
  KoImg<LDS> g{};  // set with the first item (cur matches no list position)
  for (uint32_t t = t_lo; t < t_hi; t++) {
    const uint32_t ip = t / a.r.parts, part = t - ip * a.r.parts;
    if (ip != cur) {  // the previous image's and list's last reads lie behind the barrier that ended its last chunk
      cur = ip;
      pos = a.r.pos[ip];
      const GraphView gv = c.view(a.r.graph[pos]);
      g = ko_image(std::integral_constant<bool, LDS>{}, gv, dyn, reg);
      if (LDS) {
        const uint32_t image = knock::knock_lds_bytes(gv.V, gv.E, gv.nlev);
        ls.head = reinterpret_cast<uint32_t *>(dyn + image);
        ls.cap = (a.r.lds_total - image) / 4u;
      }
      // the graph's hit nodes by distinct label (hit_list.h): count, scan, scatter
      hit_list_build(ls, g.V, D, [&](uint32_t v) { return gc_row<LDS>(a, g, v, gv.label[v]); });
    }
    unsigned long long *d64 = reinterpret_cast<unsigned long long *>(g.dead);
    const uint32_t c_lo = klabel::range_lo(a.r.n_chunks, a.r.parts, part), c_hi = klabel::range_lo(a.r.n_chunks, a.r.parts, part + 1u);
    uint2 nxt = gc_pair<SIZE>(a, c_lo);
    for (uint32_t ci = c_lo; ci < c_hi; ci++) {
      const uint32_t n = min(KO_CHUNK, a.r.n_hyp - ci * KO_CHUNK);
      // the chunk's groups: wave r scans the lengths of group r of the 64 sets.  The loads of the next chunk's
      // groups are in flight while this one is seeded and swept.  (The words written here were last read before
      // the barrier behind the previous chunk's seeds; s_any's flags are read behind it, but a chunk that runs no
      // barrier after that read left them all zero, as they are set here.)
      const uint2 pr = nxt;
      if (ci + 1u < c_hi) nxt = gc_pair<SIZE>(a, ci + 1u);
      if (wave < SIZE) {
        uint32_t incl = pr.y;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
          const uint32_t y = (uint32_t)__shfl_up((int)incl, d);
          if ((int)lane >= d) incl += y;
        }
        s_inc[tid] = incl, s_beg[tid] = pr.x;
        if (lane == 63u) s_tot[wave] = incl;
      } else if (wave == 3u) {
        s_any[lane] = 0u;
      }
      ko_zero_dead<LDS>(g);
      // seeds: the chunk's (set, group, label) triples in the order (group, set, label), 256 at a time
      const uint32_t w0 = s_tot[0], w1 = SIZE >= 2u ? w0 + s_tot[1] : w0, total = SIZE >= 3u ? w1 + s_tot[2] : w1;
      for (uint32_t base = 0; base < total; base += KO_BLOCK) {
        const uint32_t i = base + tid;
        uint32_t lo = 0u, hi = 0u, bit = 0u;
        if (i < total) {
          const uint32_t r = SIZE == 1u ? 0u : (uint32_t)(i >= w0) + (uint32_t)(SIZE >= 3u && i >= w1);
          const uint32_t j = i - (r == 0u ? 0u : r == 1u ? w0 : w1);
          const uint32_t *inc = s_inc + r * 64u;
#pragma unroll
          for (uint32_t step = 32u; step; step >>= 1)  // the first set whose scan passes j: its group holds entry j
            if (inc[bit + step - 1u] <= j) bit += step;
          const uint32_t row = a.grow[s_beg[r * 64u + bit] + (j - (bit ? inc[bit - 1u] : 0u))];
          lo = ls.lo(row), hi = ls.hi(row);  // a label absent from this graph: an empty row
          if (hi > lo) s_any[bit] = 1u;
        }
        const bool hub = hi - lo > KO_HUB;
        if (!hub)
          for (uint32_t j = lo; j < hi; j++) atomicOr(&d64[ls.get(D + 1u + j)], 1ull << bit);
        for (uint64_t hm = __ballot(hub); hm; hm &= hm - 1ull) {  // wave-uniform: one long row at a time
          const int src = __ffsll((long long)hm) - 1;
          const uint32_t hl = (uint32_t)__shfl((int)lo, src), hh = (uint32_t)__shfl((int)hi, src);
          const unsigned long long hb = 1ull << (uint32_t)__shfl((int)bit, src);
          for (uint32_t j = hl + lane; j < hh; j += 64u) atomicOr(&d64[ls.get(D + 1u + j)], hb);
        }
      }
      if (!LDS) __threadfence_block();
      __syncthreads();
      // every wave takes the same ballot of the flags behind the barrier above (they are written next behind the
      // next chunk's first barrier, unless they are all zero), so the branch, and the barriers inside it, are
      // taken by the whole workgroup or by none of it
      const uint64_t hit = __ballot(lane < n && s_any[lane] != 0u);
      uint64_t lost = 0ull;
      if (hit != 0ull) {
        ko_sweep<LDS>(g);
        lost = ko_lost_word<LDS>(g, n, s_w);  // every root dead, per bit column
      }
      if (tid == 0u) {
        a.r.lost[(uint64_t)pos * a.r.n_chunks + ci] = lost;
        if (SIZE == 1u) a.r.hit[(uint64_t)pos * a.r.n_chunks + ci] = hit;
      }
    }
  }
}

// one instantiation per round (SIZE = 1, 2, 3)
template <uint32_t SIZE>
__global__ __launch_bounds__(KO_BLOCK) void k_gc_lds(DevCorpus c, GcArgs a) {
  extern __shared__ __align__(16) uint8_t dyn[];
  gc_loop<true, SIZE>(c, a, dyn);
}

// the workgroup's dead words and hit list in its region of a.r.region; a fence and a barrier per level, as
// k_lc_glob.  Correct, not tuned.
template <uint32_t SIZE>
__global__ __launch_bounds__(KO_BLOCK) void k_gc_glob(DevCorpus c, GcArgs a) {
  gc_loop<false, SIZE>(c, a, nullptr);
}

void launch_gc_table(const GcArgs &a, hipStream_t s) {
  if (!a.n_named) return;
  hipLaunchKernelGGL(k_gc_table, dim3((uint32_t)(((uint64_t)a.n_named + KO_BLOCK - 1u) / KO_BLOCK)), dim3(KO_BLOCK), 0, s, a);
}

void launch_gc_rows(const GcArgs &a, hipStream_t s) {
  if (!a.n_named) return;
  hipLaunchKernelGGL(k_gc_rows, dim3((uint32_t)(((uint64_t)a.n_named + KO_BLOCK - 1u) / KO_BLOCK)), dim3(KO_BLOCK), 0, s, a);
}

static const void *gc_lds_kernel(uint32_t size) {
  const void *f = nullptr;
  ko_by_size(size, [&](auto sz) { f = (const void *)k_gc_lds<decltype(sz)::value>; });
  return f;
}

uint32_t gc_lds_resident(uint32_t size, uint32_t lds_bytes, uint32_t n_cu) { return ko_lds_resident(gc_lds_kernel(size), lds_bytes, n_cu); }

void launch_gc_lds(const DevCorpus &c, const GcArgs &a, uint32_t grid, hipStream_t s) {
  if (!a.r.n_tier || !a.r.n_chunks) return;
  hipFuncSetAttribute(gc_lds_kernel(a.r.size), hipFuncAttributeMaxDynamicSharedMemorySize, (int)a.r.lds_total);
  ko_by_size(a.r.size, [&](auto sz) { hipLaunchKernelGGL(k_gc_lds<decltype(sz)::value>, dim3(grid), dim3(KO_BLOCK), a.r.lds_total, s, c, a); });
}

void launch_gc_glob(const DevCorpus &c, const GcArgs &a, uint32_t grid, hipStream_t s) {
  if (!a.r.n_tier || !a.r.n_chunks) return;
  ko_by_size(a.r.size, [&](auto sz) { hipLaunchKernelGGL(k_gc_glob<decltype(sz)::value>, dim3(grid), dim3(KO_BLOCK), 0, s, c, a); });
}

}  // namespace nemo
