// k_lgcuts.hip — nemo_lineage_group_cuts (DESIGN.md §Lineage cut search over fault events): the hitting-set tree of
// k_lineage.hip with fault events (groups of labels) as candidates, across the listed runs.  Three launches per level.
// k_lgc_lds / k_lgc_glob are persistent over work items (list position, range of chunks of 64 frontier sets), as
// k_gc_lds is: on a new list position a workgroup stages the witness image (graph, dead words, need words: wit_host.h)
// and groups the graph's hit nodes by the row of their label (hit_list.h; the label -> row table is k_gc_table's).  A
// chunk seeds the dead words from its keys' positions -> groups -> rows -> nodes, sweeps (ko_sweep.h), writes the lost
// word of (list position, chunk), runs the top-down need pass for the sets that are not lost (wit_down.h) and, with
// the need words still in place (LDS on the LDS tier: they never reach device memory there), ORs them per row, ORs
// the rows' words per candidate and emits (set h) + {k} for every bit h of candidate k's word, at one wave-aggregated
// claim on the global cursor per 64 candidates.  The cursor counts past the buffer's end, nothing is written there.
// k_lgc_cuts counts a set's lost bits down the list positions' words: at q or more the set is a minimal cut and goes
// to the cuts' list, with its count, and table.  k_lin_filter (k_lineage.hip) makes the next frontier of the
// children.  No thread waits for another anywhere.
#include "device.h"
#include "hit_list.h"
#include "internal.h"
#include "ko_sweep.h"
#include "lgc_host.h"
#include "lin_dev.h"
#include "wit_down.h"

namespace nemo {

#define LGC_NONE 0xFFFFFFFFu
#define LGC_WAVE_GROUP 64u  // a group of more labels than this is walked by the whole wave

// the row of node v's label: LGC_NONE if the node carries no label, no group names it, or (a.sinks) the node is no
// sink goal.  Behind the barrier that ends the staging.
template <bool LDS>
__device__ __forceinline__ uint32_t lgc_row(const LgcArgs &a, const KoImg<LDS> &g, uint32_t v, uint32_t label) {
  if (label == LGC_NONE) return LGC_NONE;
  if (a.sinks && (g.is_rule_node(v) || g.fp[v] != g.fp[v + 1u])) return LGC_NONE;
  uint64_t h = klabel::first_slot(label, a.slots);
  for (;;) {  // ends: at most half of the slots are taken
    const uint32_t k = a.key[h];
    if (k == label + 1u) return a.val[h];
    if (k == 0u) return LGC_NONE;
    h = klabel::next_slot(h, a.slots);
  }
}

// the OR of a wave's 64 words, in every lane
__device__ __forceinline__ uint64_t lgc_wave_or(uint64_t w) {
#pragma unroll
  for (int dd = 32; dd >= 1; dd >>= 1) w |= (uint64_t)__shfl_xor((unsigned long long)w, dd);
  return w;
}

// This lane's OR of fetch(e) over e in [lo, hi).  A whole wave calls it, a lane per range: a short range is walked by
// its own lane, a long one (is_long) by the whole wave, one long range at a time.
template <class F>
__device__ __forceinline__ uint64_t lgc_range_or(uint32_t lo, uint32_t hi, bool is_long, F &&fetch) {
  const uint32_t lane = lane_id();
  uint64_t w = 0ull;
  if (!is_long)
    for (uint32_t e = lo; e < hi; e++) w |= fetch(e);
  for (uint64_t hm = __ballot(is_long); hm; hm &= hm - 1ull) {  // wave-uniform
    const int src = __ffsll((long long)hm) - 1;
    const uint32_t hl = (uint32_t)__shfl((int)lo, src), hh = (uint32_t)__shfl((int)hi, src);
    uint64_t part = 0ull;
    for (uint32_t e = hl + lane; e < hh; e += 64u) part |= fetch(e);
    part = lgc_wave_or(part);
    if ((int)lane == src) w = part;
  }
  return w;
}

// One chunk ci of the frontier on the staged graph of list position pos.  rn: the D rows' need words.  Ends behind a
// barrier.  All 256 threads.
template <bool LDS>
__device__ __forceinline__ void lgc_chunk(const LgcArgs &a, const KoImg<LDS> &g, uint64_t *need, const LcList &ls, uint64_t *rn, bool rn_lds,
                                          uint32_t pos, uint32_t ci) {
  __shared__ uint64_t s_w[KO_BLOCK / 64];
  __shared__ uint64_t s_key[KO_CHUNK][2];
  __shared__ uint32_t s_inc[KO_CHUNK];  // the inclusive scan of the lengths of field j's 64 groups (u32: a group holds at most
                                        // GC_MAX_GROUP = 2^24 labels, so the total stays below 2^30)
  __shared__ uint32_t s_beg[KO_CHUNK];  // ... and their first entries
  const LinArgs &l = a.l;
  const uint32_t tid = threadIdx.x, lane = lane_id(), wave = tid >> 6;
  const uint32_t first = ci * KO_CHUNK, n = min(KO_CHUNK, l.n_front - first);
  const uint32_t D = a.n_dist;
  unsigned long long *d64 = reinterpret_cast<unsigned long long *>(g.dead);
  ko_zero_dead<LDS>(g);  // its barrier: the staging's end, and the previous chunk's last reads of s_key
  lin_stage_keys(l.front, first, n, s_key);
  __syncthreads();
  // seeds: field j of the 64 sets at a time (every set of the level holds l.size positions).  Wave 0 scans the groups'
  // lengths, then all four waves walk the (set, label) pairs, 256 at a time: a pair whose row is empty on this graph
  // costs two offsets, a short row is ORed in by its thread, a row past KO_HUB nodes by the whole wave.
  for (uint32_t j = 0; j < l.size; j++) {
    if (wave == 0u) {
      uint32_t beg = 0u, len = 0u;
      if (lane < n) {
        const uint32_t p = lin::key_at(lin::Key{s_key[lane][0], s_key[lane][1]}, j);
        if (p < l.K) beg = a.goff[p], len = a.goff[p + 1u] - beg;
      }
      uint32_t incl = len;
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        const uint32_t y = (uint32_t)__shfl_up((int)incl, d);
        if ((int)lane >= d) incl += y;
      }
      s_inc[lane] = incl, s_beg[lane] = beg;
    }
    __syncthreads();
    const uint32_t total = s_inc[KO_CHUNK - 1u];
    for (uint32_t base = 0; base < total; base += KO_BLOCK) {
      const uint32_t i = base + tid;
      uint32_t lo = 0u, hi = 0u, bit = 0u;
      if (i < total) {
#pragma unroll
        for (uint32_t step = 32u; step; step >>= 1)  // the first set whose scan passes i: its group holds entry i
          if (s_inc[bit + step - 1u] <= i) bit += step;
        const uint32_t row = a.grow[s_beg[bit] + (i - (bit ? s_inc[bit - 1u] : 0u))];
        lo = ls.lo(row), hi = ls.hi(row);  // a label absent from this graph: an empty row
      }
      const bool hub = hi - lo > KO_HUB;
      if (!hub)
        for (uint32_t e = lo; e < hi; e++) atomicOr(&d64[ls.get(D + 1u + e)], 1ull << bit);
      for (uint64_t hm = __ballot(hub); hm; hm &= hm - 1ull) {  // wave-uniform: one long row at a time
        const int src = __ffsll((long long)hm) - 1;
        const uint32_t hl = (uint32_t)__shfl((int)lo, src), hh = (uint32_t)__shfl((int)hi, src);
        const unsigned long long hb = 1ull << (uint32_t)__shfl((int)bit, src);
        for (uint32_t e = hl + lane; e < hh; e += 64u) atomicOr(&d64[ls.get(D + 1u + e)], hb);
      }
    }
    __syncthreads();  // the scan's last reads, before the next field's
  }
  if (!LDS) __threadfence_block();
  __syncthreads();
  ko_sweep<LDS>(g);
  const uint64_t lost = ko_lost_word<LDS>(g, n, s_w);  // the same in every thread
  if (tid == 0u) a.lost[(uint64_t)pos * l.n_chunks + ci] = lost;
  const uint64_t tail = n == KO_CHUNK ? ~0ull : (1ull << n) - 1ull;
  const uint64_t live = tail & ~lost;
  if (l.emit && live != 0ull) {  // workgroup-uniform
    wit_down<LDS>(g, need, n, false);
    // the rows' need words: the OR of the need words of a row's nodes (a lost set needs nothing: no root is alive)
    for (uint32_t base = 0; base < D; base += KO_BLOCK) {
      const uint32_t r = base + tid;
      uint32_t lo = 0u, hi = 0u;
      if (r < D) lo = ls.lo(r), hi = ls.hi(r);
      const uint64_t w = lgc_range_or(lo, hi, hi - lo > KO_HUB, [&](uint32_t e) { return wit_need<LDS>(&need[ls.get(D + 1u + e)]); });
      if (r < D) rn[r] = w;
    }
    if (!rn_lds) __threadfence_block();
    __syncthreads();
    // the children: a thread per candidate position ORs its group's rows, a wave-wide claim per 64 positions.  A
    // candidate of the set itself has no bit: its rows' nodes are dead under the set, and a dead node is not needed.
    for (uint32_t kb = wave * 64u; kb < l.K; kb += KO_BLOCK) {
      const uint32_t k = kb + lane;
      uint32_t beg = 0u, end = 0u;
      if (k < l.K) beg = a.goff[k], end = a.goff[k + 1u];
      const uint64_t w = lgc_range_or(beg, end, end - beg > LGC_WAVE_GROUP, [&](uint32_t e) { return rn[a.grow[e]]; });
      lin_emit(l, s_key, k, w & live);
    }
  }
  __syncthreads();  // the image's, the words', the list's and s_key's last reads
}

// The workgroup's block of work items, as gc_loop's: item t is (list position a.pos[t / parts], chunk range
// t % parts).  A new list position stages its graph (the LDS tier: image, need words, then the rows' need words and
// the hit list's head in what a.l.lds_total leaves: lgc_host.h) and groups its hit nodes by row.  All 256 threads.
template <bool LDS>
__device__ __forceinline__ void lgc_loop(const DevCorpus &c, const LgcArgs &a, uint8_t *dyn) {
  const LinArgs &l = a.l;
  uint64_t *reg = l.region + (uint64_t)blockIdx.x * l.region_words;
  const uint32_t items = a.n_tier * a.parts;
  const uint32_t t_lo = (uint32_t)klabel::item_lo(items, gridDim.x, blockIdx.x);
  const uint32_t t_hi = (uint32_t)klabel::item_lo(items, gridDim.x, blockIdx.x + 1u);
  const uint32_t D = a.n_dist;
  LcList ls;
  ls.head = reinterpret_cast<uint32_t *>(dyn), ls.cap = 0u, ls.spill = reinterpret_cast<uint32_t *>(reg);
  uint32_t cur = ~0u, pos = 0u;
  uint64_t *need = nullptr, *rn = nullptr;
  bool rn_lds = false;
  KoImg<LDS> g{};  // set with the first item (cur matches no list position)
  for (uint32_t t = t_lo; t < t_hi; t++) {
    const uint32_t ip = t / a.parts, part = t - ip * a.parts;
    if (ip != cur) {  // the previous image's and list's last reads lie behind the barrier that ended its last chunk
      cur = ip;
      pos = a.pos[ip];
      const GraphView gv = c.view(a.graph[pos]);
      g = ko_image(std::integral_constant<bool, LDS>{}, gv, dyn, reg);
      if (LDS) {
        const uint32_t image = wit::wit_lds_bytes(gv.V, gv.E, gv.nlev);
        const lgc::Tail tl = lgc::tail(l.lds_total, image, D);
        need = reinterpret_cast<uint64_t *>(dyn + knock::knock_lds_bytes(gv.V, gv.E, gv.nlev));
        rn_lds = tl.rn_lds != 0u;
        rn = rn_lds ? reinterpret_cast<uint64_t *>(dyn + image) : reg + lgc::rn_offset(0);
        ls.head = reinterpret_cast<uint32_t *>(dyn + image + tl.rn_bytes);
        ls.cap = tl.head;
        ls.spill = reinterpret_cast<uint32_t *>(reg + lgc::spill_offset(0, D, tl));
      } else {
        lgc::Tail tl;
        tl.rn_lds = 0u, tl.rn_bytes = 0u, tl.head = 0u;
        need = reg + a.glob_words / 2u;
        rn = reg + lgc::rn_offset(a.glob_words);
        ls.spill = reinterpret_cast<uint32_t *>(reg + lgc::spill_offset(a.glob_words, D, tl));
      }
      // the graph's hit nodes by distinct label (hit_list.h): count, scan, scatter
      hit_list_build(ls, g.V, D, [&](uint32_t v) { return lgc_row<LDS>(a, g, v, gv.label[v]); });
    }
    const uint32_t c_lo = klabel::range_lo(l.n_chunks, a.parts, part), c_hi = klabel::range_lo(l.n_chunks, a.parts, part + 1u);
    for (uint32_t ci = c_lo; ci < c_hi; ci++) lgc_chunk<LDS>(a, g, need, ls, rn, rn_lds, pos, ci);
  }
}

__global__ __launch_bounds__(KO_BLOCK) void k_lgc_lds(DevCorpus c, LgcArgs a) {
  extern __shared__ __align__(16) uint8_t dyn[];
  lgc_loop<true>(c, a, dyn);
}

// the workgroup's dead and need words, the rows' need words and its hit list in its region of a.l.region; a fence and
// a barrier per level.  Correct, not tuned.
__global__ __launch_bounds__(KO_BLOCK) void k_lgc_glob(DevCorpus c, LgcArgs a) { lgc_loop<false>(c, a, nullptr); }

// A thread per frontier set: the popcount of its bit down the list positions' lost words.  At q or more the set is a
// minimal cut of the level's size: its key and count to the cuts' list, at a wave-aggregated claim, its index into
// the cuts' table.
__global__ __launch_bounds__(KO_BLOCK) void k_lgc_cuts(LgcArgs a) {
  const LinArgs &l = a.l;
  const uint32_t lane = lane_id();
  const uint64_t s = (uint64_t)blockIdx.x * KO_BLOCK + threadIdx.x;
  uint32_t cnt = 0u;
  if (s < l.n_front) cnt = lgc::lost_count(a.lost, a.n, l.n_chunks, s);
  const bool cut = s < l.n_front && lgc::is_cut(cnt, a.q);
  const uint64_t b = __ballot(cut);
  if (!b) return;
  unsigned long long at = 0;
  if (lane == 0u) at = atomicAdd(l.ctr, (unsigned long long)__popcll(b));
  at = (unsigned long long)__shfl((unsigned long long)at, 0);
  if (cut) {
    const uint32_t i = (uint32_t)at + (uint32_t)__popcll(b & ((1ull << lane) - 1ull));
    const lin::Key k = lin_load(l.front, s);
    lin_store(l.cuts, i, k);
    a.n_lost[i] = cnt;
    lin_cut_insert(l, i, k);
  }
}

uint32_t lgc_lds_resident(uint32_t lds_bytes, uint32_t n_cu) { return ko_lds_resident((const void *)k_lgc_lds, lds_bytes, n_cu); }

void launch_lgc_lds(const DevCorpus &c, const LgcArgs &a, uint32_t grid, hipStream_t s) {
  if (!a.n_tier || !a.l.n_chunks) return;
  hipFuncSetAttribute((const void *)k_lgc_lds, hipFuncAttributeMaxDynamicSharedMemorySize, (int)a.l.lds_total);
  hipLaunchKernelGGL(k_lgc_lds, dim3(grid), dim3(KO_BLOCK), a.l.lds_total, s, c, a);
}

void launch_lgc_glob(const DevCorpus &c, const LgcArgs &a, uint32_t grid, hipStream_t s) {
  if (!a.n_tier || !a.l.n_chunks) return;
  hipLaunchKernelGGL(k_lgc_glob, dim3(grid), dim3(KO_BLOCK), 0, s, c, a);
}

void launch_lgc_cuts(const LgcArgs &a, hipStream_t s) {
  if (!a.l.n_front) return;
  hipLaunchKernelGGL(k_lgc_cuts, dim3((uint32_t)(((uint64_t)a.l.n_front + KO_BLOCK - 1u) / KO_BLOCK)), dim3(KO_BLOCK), 0, s, a);
}

}  // namespace nemo
