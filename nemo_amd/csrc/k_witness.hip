// k_witness.hip — nemo_witness_sets / nemo_witness_labels (DESIGN.md §Surviving derivations): which derivation
// is left under a fault set that does not defeat the outcome.  The first half is the knock-out family's: 64
// hypotheses per chunk, bit b of a u64 dead word per node, seeded from the chunk's sets and swept bottom-up
// (ko_sweep.h).  The second half is new: a u64 need word per node, seeded at the roots with ~dead and pushed down
// the same Kahn levels, roots first.  A needed rule needs every child; a needed goal needs its first alive child in
// row order (rows ascend by child index), or with a.all every alive child.  Several parents of a level share a
// child, so the pushes are 64-bit atomic ORs, one barrier per level.  k_wit_lds is persistent over work items (list
// position, chunk range) as k_kl_lds is and stages a graph's image, with the need words behind it, once per work
// item; k_wit_glob is the same loop over the CSR in device memory with both word arrays in the workgroup's region.
// The label form groups a staged graph's nodes by the row of their label (hit_list.h) and seeds from the rows a
// set names; the node-set form seeds from the nodes themselves.  k_wit_table hashes the distinct labels.
#include "device.h"
#include "hit_list.h"
#include "internal.h"
#include "ko_sweep.h"
#include "wit_down.h"
#include "wit_host.h"

namespace nemo {

#define WIT_NONE 0xFFFFFFFFu

// A thread per distinct label: its slot takes the label's row.  The table is zero and at most half full.
__global__ __launch_bounds__(KO_BLOCK) void k_wit_table(WitArgs a) {
  const uint32_t r = blockIdx.x * KO_BLOCK + threadIdx.x;
  if (r >= a.k1) return;
  const uint32_t label = a.dist[r];
  uint64_t h = klabel::first_slot(label, a.slots);
  while (atomicCAS(&a.key[h], 0u, label + 1u) != 0u) h = klabel::next_slot(h, a.slots);
  a.val[h] = r;
}

// the row of node v's label: WIT_NONE if the node carries no label, no set names it, or (a.sinks) the node is no
// sink goal.  Behind the barrier that ends the staging.
template <bool LDS>
__device__ __forceinline__ uint32_t wit_row(const WitArgs &a, const KoImg<LDS> &g, uint32_t v, uint32_t label) {
  if (label == WIT_NONE) return WIT_NONE;
  if (a.sinks && (g.is_rule_node(v) || g.fp[v] != g.fp[v + 1u])) return WIT_NONE;
  uint64_t h = klabel::first_slot(label, a.slots);
  for (;;) {  // ends: at most half of the slots are taken
    const uint32_t k = a.key[h];
    if (k == label + 1u) return a.val[h];
    if (k == 0u) return WIT_NONE;
    h = klabel::next_slot(h, a.slots);
  }
}

// One chunk ci of list position pos on a staged graph: zero, seed, sweep, the top-down pass, the counts per bit
// column and a row per hypothesis; with a.need the V need words out in 16-byte stores.  Ends behind a barrier.
template <bool LDS>
__device__ __forceinline__ void wit_chunk(const WitArgs &a, const KoImg<LDS> &g, uint64_t *need, const LcList &ls, uint32_t graph,
                                          uint32_t pos, uint32_t ci) {
  __shared__ uint32_t s_cnt[3][KO_BLOCK / 64][64];
  const uint32_t tid = threadIdx.x, lane = lane_id(), wave = tid >> 6;
  const uint32_t first = ci * KO_CHUNK, n = min(KO_CHUNK, a.n_sets - first);
  uint64_t *dead = g.dead;
  ko_zero_dead<LDS>(g);
  // seeds: a wave per set, a lane per entry; several sets may name one node: atomic OR
  for (uint32_t s = wave; s < n; s += KO_BLOCK / 64) {
    const uint64_t lo = a.set_off[first + s], hi = a.set_off[first + s + 1u];
    const uint64_t bit = 1ull << s;
    for (uint64_t j = lo + lane; j < hi; j += 64u) {
      const uint32_t x = a.ent[j];
      if (a.k1) {
        if (x < a.k1)
          for (uint32_t k = ls.lo(x), ke = ls.hi(x); k < ke; k++) wit_or(&dead[ls.get(a.k1 + 1u + k)], bit);
      } else if (x < g.V) {
        wit_or(&dead[x], bit);
      }
    }
  }
  if (!LDS) __threadfence_block();
  __syncthreads();
  ko_sweep<LDS>(g);
  wit_down<LDS>(g, need, n, a.all != 0u);
  // per bit column: needed nodes, needed sink goals, needed roots
  const uint32_t n_roots = g.L ? (uint32_t)g.lvl[1] : 0u;
  uint32_t cn = 0, cs = 0, cr = 0;
  for (uint32_t base = wave * 64u; base < g.V; base += KO_BLOCK) {
    const uint32_t v = base + lane;
    const uint64_t w = v < g.V ? wit_need<LDS>(&need[v]) : 0ull;
    if (__ballot(w != 0ull) == 0ull) continue;
    cn += ko_colsum((uint32_t)w, (uint32_t)(w >> 32));
    const bool sink = w != 0ull && !g.is_rule_node(v) && g.fp[v] == g.fp[v + 1u];
    const uint64_t ws = sink ? w : 0ull;
    if (__ballot(ws != 0ull) != 0ull) cs += ko_colsum((uint32_t)ws, (uint32_t)(ws >> 32));
  }
  for (uint32_t base = wave * 64u; base < n_roots; base += KO_BLOCK) {
    const uint32_t i = base + lane;
    const uint64_t w = i < n_roots ? wit_need<LDS>(&need[g.topo[i]]) : 0ull;
    if (__ballot(w != 0ull) == 0ull) continue;
    cr += ko_colsum((uint32_t)w, (uint32_t)(w >> 32));
  }
  s_cnt[0][wave][lane] = cn;
  s_cnt[1][wave][lane] = cs;
  s_cnt[2][wave][lane] = cr;
  __syncthreads();
  if (tid < n) {  // lane b of wave 0 writes hypothesis b's row
    uint32_t nn = 0, ns = 0, nr = 0;
#pragma unroll
    for (int w = 0; w < KO_BLOCK / 64; w++) {
      nn += s_cnt[0][w][tid];
      ns += s_cnt[1][w][tid];
      nr += s_cnt[2][w][tid];
    }
    uint32_t *row = a.rows + 5ull * wit::hyp_index(pos, first + tid, a.n_sets);
    row[0] = graph;
    row[1] = n_roots;
    row[2] = nr;
    row[3] = nn;
    row[4] = ns;
  }
  if (a.need) {  // whole pairs: the word behind an odd V is zero
    uint4 *o = reinterpret_cast<uint4 *>(a.need + a.moff[pos] + (uint64_t)ci * knock::dead_words(g.V));
    const uint32_t pairs = (g.V + 1u) / 2u;
    for (uint32_t i = tid; i < pairs; i += KO_BLOCK) {
      const uint64_t x = wit_need<LDS>(&need[2u * i]), y = wit_need<LDS>(&need[2u * i + 1u]);
      o[i] = make_uint4((uint32_t)x, (uint32_t)(x >> 32), (uint32_t)y, (uint32_t)(y >> 32));
    }
  }
  __syncthreads();  // the image's, the words' and s_cnt's last reads
}

// The workgroup's block of work items: item t is (list position a.pos[t / parts], chunk range t % parts).  A new
// list position stages its graph (the LDS tier: image, need words, then the hit list's head in what a.lds_total
// leaves) and, in the label form, groups its nodes by row.  All 256 threads.
template <bool LDS>
__device__ __forceinline__ void wit_loop(const DevCorpus &c, const WitArgs &a, uint8_t *dyn) {
  uint64_t *reg = a.region + (uint64_t)blockIdx.x * a.region_words;
  const uint32_t items = a.n_tier * a.parts;
  const uint32_t t_lo = (uint32_t)klabel::item_lo(items, gridDim.x, blockIdx.x);
  const uint32_t t_hi = (uint32_t)klabel::item_lo(items, gridDim.x, blockIdx.x + 1u);
  LcList ls;
  ls.head = reinterpret_cast<uint32_t *>(dyn), ls.cap = 0u;
  ls.spill = reinterpret_cast<uint32_t *>(LDS ? reg : reg + a.glob_words);
  uint32_t cur = ~0u, pos = 0u, graph = 0u;
  uint64_t *need = nullptr;
  KoImg<LDS> g{};  // set with the first item (cur matches no list position)
  for (uint32_t t = t_lo; t < t_hi; t++) {
    const uint32_t ip = t / a.parts, part = t - ip * a.parts;
    if (ip != cur) {  // the previous image's and list's last reads lie behind the barrier that ended its last chunk
      cur = ip;
      pos = a.pos[ip];
      graph = a.graph[pos];
      const GraphView gv = c.view(graph);
      g = ko_image(std::integral_constant<bool, LDS>{}, gv, dyn, reg);
      if (LDS) {
        const uint32_t image = wit::wit_lds_bytes(gv.V, gv.E, gv.nlev);
        need = reinterpret_cast<uint64_t *>(dyn + knock::knock_lds_bytes(gv.V, gv.E, gv.nlev));
        ls.head = reinterpret_cast<uint32_t *>(dyn + image);
        ls.cap = (a.lds_total - image) / 4u;
      } else {
        need = reg + a.glob_words / 2u;
      }
      if (a.k1) hit_list_build(ls, g.V, a.k1, [&](uint32_t v) { return wit_row<LDS>(a, g, v, gv.label[v]); });
    }
    const uint32_t c_lo = klabel::range_lo(a.n_chunks, a.parts, part), c_hi = klabel::range_lo(a.n_chunks, a.parts, part + 1u);
    for (uint32_t ci = c_lo; ci < c_hi; ci++) wit_chunk<LDS>(a, g, need, ls, graph, pos, ci);  // its first barrier ends the staging
  }
}

__global__ __launch_bounds__(KO_BLOCK) void k_wit_lds(DevCorpus c, WitArgs a) {
  extern __shared__ __align__(16) uint8_t dyn[];
  wit_loop<true>(c, a, dyn);
}

// the workgroup's dead and need words and its hit list in its region of a.region; a fence and a barrier per level
__global__ __launch_bounds__(KO_BLOCK) void k_wit_glob(DevCorpus c, WitArgs a) { wit_loop<false>(c, a, nullptr); }

void launch_wit_table(const WitArgs &a, hipStream_t s) {
  if (!a.k1) return;
  hipLaunchKernelGGL(k_wit_table, dim3((a.k1 + KO_BLOCK - 1u) / KO_BLOCK), dim3(KO_BLOCK), 0, s, a);
}

uint32_t wit_lds_resident(uint32_t lds_bytes, uint32_t n_cu) { return ko_lds_resident((const void *)k_wit_lds, lds_bytes, n_cu); }

void launch_wit_lds(const DevCorpus &c, const WitArgs &a, uint32_t grid, hipStream_t s) {
  if (!a.n_tier || !a.n_chunks) return;
  hipFuncSetAttribute((const void *)k_wit_lds, hipFuncAttributeMaxDynamicSharedMemorySize, (int)a.lds_total);
  hipLaunchKernelGGL(k_wit_lds, dim3(grid), dim3(KO_BLOCK), a.lds_total, s, c, a);
}

void launch_wit_glob(const DevCorpus &c, const WitArgs &a, uint32_t grid, hipStream_t s) {
  if (!a.n_tier || !a.n_chunks) return;
  hipLaunchKernelGGL(k_wit_glob, dim3(grid), dim3(KO_BLOCK), 0, s, c, a);
}

}  // namespace nemo
