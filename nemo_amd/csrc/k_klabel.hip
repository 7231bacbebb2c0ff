// k_klabel.hip — nemo_knockout_labels (DESIGN.md §Knock-out by label): the knock-out sweep under hypotheses that
// name labels, on every listed graph in one call.  k_kl_tables turns the uploaded label sets into one label ->
// mask table per chunk of 64 sets and a union filter of all named labels.  k_kl_lds is persistent: a workgroup
// takes a contiguous block of work items (list position, chunk range), stages a graph's LDS image once
// (ko_sweep.h: the images of both tiers, the zeroing, the sweep, the lost word, the column sums) together with its hit list, the nodes whose label some set names, and then per chunk seeds the dead
// words from the chunk's table, sweeps and writes one (lost, hit) word pair.  k_kl_glob is the same loop over the
// CSR in device memory.  k_kl_count sums the words' bit columns over the list positions.
#include "device.h"
#include "internal.h"
#include "klabel_host.h"
#include "ko_sweep.h"

namespace nemo {

#define KL_NONE (~0ull)

// the slot of `label` in a table of `slots` keys: claimed if it is free
__device__ __forceinline__ uint64_t kl_insert(uint32_t *key, uint64_t slots, uint32_t label) {
  uint64_t h = klabel::first_slot(label, slots);
  for (;;) {  // ends: at most half of the slots are taken
    const uint32_t old = atomicCAS(&key[h], 0u, label + 1u);
    if (old == 0u || old == label + 1u) return h;
    h = klabel::next_slot(h, slots);
  }
}

// ... and without claiming: KL_NONE if the table does not hold the label
__device__ __forceinline__ uint64_t kl_probe(const uint32_t *key, uint64_t slots, uint32_t label) {
  uint64_t h = klabel::first_slot(label, slots);
  for (;;) {
    const uint32_t k = key[h];
    if (k == label + 1u) return h;
    if (k == 0u) return KL_NONE;
    h = klabel::next_slot(h, slots);
  }
}

// A wave per set, a lane per label of it: bit s & 63 into the label's mask of chunk s / 64, the label into the
// union filter.  The tables are zero.
__global__ __launch_bounds__(KO_BLOCK) void k_kl_tables(KlArgs a) {
  const uint32_t lane = lane_id(), waves = gridDim.x * (KO_BLOCK / 64);
  const uint64_t u0 = a.tab_off[a.n_chunks], uslots = a.tab_off[a.n_chunks + 1u] - u0;
  for (uint32_t s = blockIdx.x * (KO_BLOCK / 64) + (threadIdx.x >> 6); s < a.n_sets; s += waves) {
    const uint32_t c = s >> 6;
    const uint64_t t0 = a.tab_off[c], slots = a.tab_off[c + 1u] - t0;
    const uint64_t lo = a.set_off[s], hi = a.set_off[s + 1u];
    for (uint64_t j = lo + lane; j < hi; j += 64u) {
      const uint32_t lab = a.labels[j];
      const uint64_t h = kl_insert(a.key + t0, slots, lab);
      atomicOr(reinterpret_cast<unsigned long long *>(a.mask + t0 + h), 1ull << (s & 63u));
      kl_insert(a.key + u0, uslots, lab);
    }
  }
}

// The hit list of a staged graph: (node, label) of every node whose label is in the union filter (a.sinks: of
// every such sink goal).  Labels are read in rounds of KO_Q coalesced loads at clamped indices, all issued before
// the first use; a wave appends its hits with one atomic on the counter, the lanes' places by prefix popcount.
// The first `cap` pairs go to `head`, the others to `spill`.  Behind a barrier that ends the staging (the rule
// bits and rows are read); no barrier at the end.
template <bool LDS>
__device__ __forceinline__ void kl_hits(const KlArgs &a, const GraphView &gv, const KoImg<LDS> &g, uint2 *head, uint32_t cap,
                                        uint2 *spill, uint32_t *count) {
  const uint32_t tid = threadIdx.x, lane = lane_id(), V = gv.V;
  const uint64_t u0 = a.tab_off[a.n_chunks], uslots = a.tab_off[a.n_chunks + 1u] - u0;
  const uint32_t *ukey = a.key + u0;
  for (uint32_t base = 0; base < V; base += KO_Q * KO_BLOCK) {
    uint32_t lab[KO_Q];
#pragma unroll
    for (int q = 0; q < KO_Q; q++) lab[q] = gv.label[min(base + q * KO_BLOCK + tid, V - 1u)];
#pragma unroll
    for (int q = 0; q < KO_Q; q++) {
      const uint32_t v = base + q * KO_BLOCK + tid;
      bool ok = v < V && lab[q] != KL_NO_LABEL;
      if (ok && a.sinks) ok = !g.is_rule_node(v) && g.fp[v] == g.fp[v + 1u];
      if (ok) ok = kl_probe(ukey, uslots, lab[q]) != KL_NONE;
      const uint64_t m = __ballot(ok);
      if (m == 0ull) continue;
      const int leader = __ffsll((long long)m) - 1;
      uint32_t first = 0;
      if ((int)lane == leader) first = atomicAdd(count, (uint32_t)__popcll(m));
      first = __builtin_amdgcn_readlane(first, leader);
      if (ok) {
        const uint32_t at = first + mbcnt(m);
        const uint2 pair = make_uint2(v, lab[q]);
        if (at < cap) head[at] = pair;
        else spill[at - cap] = pair;
      }
    }
  }
}

// The workgroup's block of work items: item t is (list position a.pos[t / parts], chunk range t % parts).  A new
// list position stages its graph and its hit list; every chunk of the range then zeroes the dead words, stores
// the masks of the hits the chunk's table holds, sweeps and writes (lost, hit).  A chunk that hits nothing on the
// graph loses nothing: no sweep.  dyn: k_kl_lds's dynamic LDS (a.lds_total bytes), the image first, then as many
// hit pairs as the rest holds; the others go to the workgroup's region.  All 256 threads.
// LIST false (option kl_hitlist 0, the form the hit list was measured against): no hit list; every chunk reads all V
// labels in the same batched rounds and probes its table with each.
template <bool LDS, bool LIST>
__device__ __forceinline__ void kl_loop(const DevCorpus &c, const KlArgs &a, uint8_t *dyn) {
  __shared__ uint64_t s_w[2][KO_BLOCK / 64];  // the waves' hit words | ko_lost_word's
  __shared__ uint32_t s_nhit;
  const uint32_t tid = threadIdx.x, lane = lane_id(), wave = tid >> 6;
  uint64_t *reg = a.region + (uint64_t)blockIdx.x * a.region_words;
  const uint32_t items = a.n_tier * a.parts;
  const uint32_t t_lo = (uint32_t)klabel::item_lo(items, gridDim.x, blockIdx.x);
  const uint32_t t_hi = (uint32_t)klabel::item_lo(items, gridDim.x, blockIdx.x + 1u);
  uint2 *spill = reinterpret_cast<uint2 *>(LDS ? reg : reg + a.dead_words);
  uint2 *head = reinterpret_cast<uint2 *>(dyn);
  uint32_t cur = ~0u, pos = 0u, nhit = 0u, cap = 0u;
  const uint32_t *label = nullptr;
  KoImg<LDS> g{};  // set with the first item (cur matches no list position)
  for (uint32_t t = t_lo; t < t_hi; t++) {
    const uint32_t ip = t / a.parts, part = t - ip * a.parts;
    if (ip != cur) {  // the previous image's last reads lie behind the barrier that ended its last chunk
      cur = ip;
      pos = a.pos[ip];
      const GraphView gv = c.view(a.graph[pos]);
      if (tid == 0u) s_nhit = 0u;
      g = ko_image(std::integral_constant<bool, LDS>{}, gv, dyn, reg);
      if (LDS) {
        const uint32_t image = knock::knock_lds_bytes(gv.V, gv.E, gv.nlev);
        head = reinterpret_cast<uint2 *>(dyn + image);
        cap = (a.lds_total - image) / 8u;
      }
      label = gv.label;
      if (LIST) {
        __syncthreads();  // the image and the counter
        kl_hits<LDS>(a, gv, g, head, cap, spill, &s_nhit);
        __threadfence_block();  // the spilled pairs
        __syncthreads();
        nhit = s_nhit;
      }
    }
    uint64_t *dead = g.dead;
    const uint32_t c_lo = klabel::range_lo(a.n_chunks, a.parts, part), c_hi = klabel::range_lo(a.n_chunks, a.parts, part + 1u);
    for (uint32_t ci = c_lo; ci < c_hi; ci++) {
      ko_zero_dead<LDS>(g);
      // seeds: a hit's node gets the mask of the chunk's sets that name its label (a node is one hit: plain stores)
      const uint64_t t0 = a.tab_off[ci], slots = a.tab_off[ci + 1u] - t0;
      uint64_t hw = 0ull;
      if (LIST) {
        for (uint32_t h = tid; h < nhit; h += KO_BLOCK) {
          const uint2 p = h < cap ? head[h] : spill[h - cap];
          const uint64_t at = kl_probe(a.key + t0, slots, p.y);
          if (at != KL_NONE) {
            const uint64_t m = a.mask[t0 + at];
            dead[p.x] = m;
            hw |= m;
          }
        }
      } else {  // (the barrier above also ends the staging: the rule bits and rows are read)
        for (uint32_t base = 0; base < g.V; base += KO_Q * KO_BLOCK) {
          uint32_t lab[KO_Q];
#pragma unroll
          for (int q = 0; q < KO_Q; q++) lab[q] = label[min(base + q * KO_BLOCK + tid, g.V - 1u)];
#pragma unroll
          for (int q = 0; q < KO_Q; q++) {
            const uint32_t v = base + q * KO_BLOCK + tid;
            bool ok = v < g.V && lab[q] != KL_NO_LABEL;
            if (ok && a.sinks) ok = !g.is_rule_node(v) && g.fp[v] == g.fp[v + 1u];
            const uint64_t at = ok ? kl_probe(a.key + t0, slots, lab[q]) : KL_NONE;
            if (at != KL_NONE) {
              const uint64_t m = a.mask[t0 + at];
              dead[v] = m;
              hw |= m;
            }
          }
        }
      }
#pragma unroll
      for (int dd = 32; dd >= 1; dd >>= 1) hw |= (uint64_t)__shfl_xor((unsigned long long)hw, dd);
      if (lane == 0u) s_w[0][wave] = hw;
      if (!LDS) __threadfence_block();
      __syncthreads();
      const uint64_t hit = s_w[0][0] | s_w[0][1] | s_w[0][2] | s_w[0][3];
      uint64_t lost = 0ull;
      // every thread has read the same four words of s_w[0] behind the barrier above, so the branch, and the
      // barriers inside it, are taken by the whole workgroup or by none of it
      if (hit != 0ull) {
        ko_sweep<LDS>(g);
        lost = ko_lost_word<LDS>(g, min(KO_CHUNK, a.n_sets - ci * KO_CHUNK), s_w[1]);  // every root dead, per bit column
      }
      if (tid == 0u)
        reinterpret_cast<uint4 *>(a.out)[(uint64_t)pos * a.n_chunks + ci] =
            make_uint4((uint32_t)lost, (uint32_t)(lost >> 32), (uint32_t)hit, (uint32_t)(hit >> 32));
    }
  }
}

template <bool LIST>
__global__ __launch_bounds__(KO_BLOCK) void k_kl_lds(DevCorpus c, KlArgs a) {
  extern __shared__ __align__(16) uint8_t dyn[];
  kl_loop<true, LIST>(c, a, dyn);
}

// the workgroup's dead words and hit list in its region of a.region; a fence and a barrier per level, as
// k_ko_glob.  Correct, not tuned.
__global__ __launch_bounds__(KO_BLOCK) void k_kl_glob(DevCorpus c, KlArgs a) { kl_loop<false, true>(c, a, nullptr); }

// A wave per chunk, a lane per bit: lane b counts the list positions whose lost / hit word has bit b.  A round
// reads the words of 64 list positions, one per lane, and every lane then takes its bit of each of them.
__global__ __launch_bounds__(KO_BLOCK) void k_kl_count(KlArgs a) {
  const uint32_t ci = blockIdx.x * (KO_BLOCK / 64) + (threadIdx.x >> 6), lane = lane_id();
  if (ci >= a.n_chunks) return;
  const uint4 *w = reinterpret_cast<const uint4 *>(a.out);
  uint32_t nl = 0, nh = 0;
  for (uint32_t base = 0; base < a.n; base += 64u) {
    const uint32_t i = base + lane;
    const uint4 x = i < a.n ? w[(uint64_t)i * a.n_chunks + ci] : make_uint4(0u, 0u, 0u, 0u);
    nl += ko_colsum(x.x, x.y);
    nh += ko_colsum(x.z, x.w);
  }
  a.cnt[(uint64_t)ci * 64u + lane] = nl;
  a.cnt[((uint64_t)a.n_chunks + ci) * 64u + lane] = nh;
}

void launch_kl_tables(const KlArgs &a, hipStream_t s) {
  if (!a.n_sets) return;
  const uint32_t per = KO_BLOCK / 64;
  hipLaunchKernelGGL(k_kl_tables, dim3(std::min<uint32_t>((a.n_sets + per - 1u) / per, 4096u)), dim3(KO_BLOCK), 0, s, a);
}

static const void *kl_lds_kernel(bool list) { return list ? (const void *)k_kl_lds<true> : (const void *)k_kl_lds<false>; }

uint32_t kl_lds_resident(uint32_t lds_bytes, uint32_t n_cu, bool list) { return ko_lds_resident(kl_lds_kernel(list), lds_bytes, n_cu); }

void launch_kl_lds(const DevCorpus &c, const KlArgs &a, uint32_t grid, hipStream_t s) {
  if (!a.n_tier || !a.n_chunks) return;
  hipFuncSetAttribute(kl_lds_kernel(!a.no_list), hipFuncAttributeMaxDynamicSharedMemorySize, (int)a.lds_total);
  if (a.no_list) hipLaunchKernelGGL(k_kl_lds<false>, dim3(grid), dim3(KO_BLOCK), a.lds_total, s, c, a);
  else hipLaunchKernelGGL(k_kl_lds<true>, dim3(grid), dim3(KO_BLOCK), a.lds_total, s, c, a);
}

void launch_kl_glob(const DevCorpus &c, const KlArgs &a, uint32_t grid, hipStream_t s) {
  if (!a.n_tier || !a.n_chunks) return;
  hipLaunchKernelGGL(k_kl_glob, dim3(grid), dim3(KO_BLOCK), 0, s, c, a);
}

void launch_kl_count(const KlArgs &a, hipStream_t s) {
  if (!a.n_chunks) return;
  hipLaunchKernelGGL(k_kl_count, dim3((a.n_chunks + KO_BLOCK / 64 - 1u) / (KO_BLOCK / 64)), dim3(KO_BLOCK), 0, s, a);
}

}  // namespace nemo
