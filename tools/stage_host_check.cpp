// stage_host_check — drives the host arithmetic of the sliced hand-over (nemo_amd/csrc/stage_host.h):
// the slices of the node state's words and of the chain pairs tile their range exactly once, in order,
// nearly equally, for every slice count the option allows; and replays nemo_stage_simplified's slice
// loops on host buffers (pack and copy each slice, as k_pack_state / k_chain_pairs and the copies do),
// so that a range outside a buffer is a sanitizer report.  It calls nothing on a device:
//   g++ -std=c++17 -g -Wall -fsanitize=address,undefined -static-libasan -static-libubsan
//       tools/stage_host_check.cpp -o build/stage_host_check
//   build/stage_host_check
#include "../nemo_amd/csrc/stage_host.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#define CHECK(x)                                            \
  do {                                                      \
    if (!(x)) {                                             \
      fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #x); \
      exit(1);                                              \
    }                                                       \
  } while (0)

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 7;
  rng_state ^= rng_state << 17;
  return rng_state;
}

// the K ranges tile [0, n): in order, no gap, no overlap; equal slices' lengths within one of each other,
// growing slices' lengths non-decreasing (to within the rounding) and in the ratio asked for when n is large
static void check_tiling(uint64_t n, uint32_t K, uint32_t ratio) {
  uint64_t edge = 0, mn = ~0ull, mx = 0, prev = 0;
  for (uint32_t k = 0; k < K; k++) {
    const stage::Range r = stage::slice(n, K, k, ratio);
    CHECK(r.lo == edge && r.hi >= r.lo && r.hi <= n);
    CHECK(r.empty() == (r.size() == 0));
    CHECK(r.size() + 1 >= prev);
    if (k && n >= (1ull << 40) && n < (1ull << 62)) {
      CHECK(r.size() >= ratio * prev - ratio && r.size() <= ratio * prev + ratio);
    }
    prev = r.size();
    edge = r.hi;
    mn = std::min(mn, r.size());
    mx = std::max(mx, r.size());
  }
  CHECK(edge == n && stage::slice_lo(n, K, K, ratio) == n && stage::slice_lo(n, K, K + 3, ratio) == n);
  if (ratio == 1) {
    CHECK(mx - mn <= 1 && mx == n / K + (n % K != 0) && mn == n / K);
    if (n >= K) CHECK(mn >= 1);  // a slice is empty only when there are fewer elements than slices
    for (uint32_t k = 0; k <= K; k++) CHECK(stage::slice_lo(n, K, k) == (uint64_t)((unsigned __int128)n * k / K));
  }
}

// the node state of V nodes in K slices: every word packed once, the tail word in the last non-empty slice
static void check_state(uint64_t V, uint32_t K, uint32_t ratio) {
  const uint64_t words = stage::state_words(V);
  CHECK(words == (V + 15) / 16);
  std::vector<uint8_t> flags(V);
  for (auto &f : flags) f = (uint8_t)(rnd() & 3);
  std::vector<uint32_t> dev(words, 0xDEADBEEFu), host(words, 0xDEADBEEFu), want(words, 0u);
  for (uint64_t v = 0; v < V; v++) want[v / 16] |= (uint32_t)flags[v] << (2 * (v % 16));
  uint64_t nodes = 0, issued = 0;
  for (uint32_t k = 0; k < K; k++) {
    const stage::Range w = stage::slice(words, K, k, ratio);
    if (w.empty() && k + 1 < K) continue;
    issued++;
    nodes += stage::state_nodes(V, w);
    for (uint64_t i = 0; i < w.size(); i++) {  // k_pack_state's threads of this launch
      const uint64_t x = w.lo + i;
      if (16 * x >= V) continue;
      uint32_t word = 0;
      for (int b = 0; b < 16; b++) word |= (16 * x + b < V ? (uint32_t)flags[16 * x + b] : 0u) << (2 * b);
      dev[x] = word;
    }
    std::copy(dev.begin() + w.lo, dev.begin() + w.hi, host.begin() + w.lo);  // the slice's copy
  }
  CHECK(host == want && nodes == V && issued >= 1 && issued <= K);
}

// chain pairs: graphs' ranges [off[g], off[g] + n) against K slices of [0, cap): every pair below cap written
// once, none at or past cap
static void check_pairs(uint32_t G, uint32_t nmax, uint64_t cap_of_total_percent, uint32_t K) {
  std::vector<uint64_t> off(G + 1, 0);
  for (uint32_t g = 0; g < G; g++) off[g + 1] = off[g] + (rnd() % 3 == 0 ? 0 : rnd() % (nmax + 1));
  const uint64_t total = off[G], cap = total * cap_of_total_percent / 100;
  std::vector<uint32_t> dev(cap, 0u), host(cap, 0u);
  bool straddle = false;
  for (uint32_t k = 0; k < K; k++) {
    const stage::Range r = stage::slice(cap, K, k);
    const bool last = k + 1 == K;
    if (r.empty() && !last) continue;
    for (uint32_t g = 0; g < G; g++) {  // k_chain_pairs' workgroups of this launch
      const uint64_t o = off[g], e = off[g + 1];
      const uint64_t a = std::max(o, r.lo), b = std::min(e, r.hi);
      if (a >= b) continue;
      straddle |= (o < r.lo || e > r.hi);
      for (uint64_t i = a; i < b; i++) dev[i] += 1u + g;
    }
    std::copy(dev.begin() + r.lo, dev.begin() + r.hi, host.begin() + r.lo);
  }
  for (uint32_t g = 0; g < G; g++)
    for (uint64_t i = off[g]; i < off[g + 1] && i < cap; i++) CHECK(host[i] == 1u + g);
  // fewer non-empty graphs than slices of a full-size buffer: some graph's pairs lie in two slices
  uint32_t nonempty = 0;
  for (uint32_t g = 0; g < G; g++) nonempty += off[g + 1] > off[g];
  if (cap == total && nonempty && nonempty < K && total >= K) CHECK(straddle);
}

int main() {
  for (uint32_t K = 1; K <= NEMO_STAGE_SLICES_MAX; K++) {
    for (uint32_t ratio = 1; ratio <= NEMO_STAGE_RATIO_MAX; ratio++) {
      for (uint64_t n = 0; n <= 70; n++) check_tiling(n, K, ratio);  // K > n, n not divisible by K
      check_tiling(7300000, K, ratio);
      check_tiling((98769507ull + 15) / 16, K, ratio);
      check_tiling(~0ull, K, ratio);  // no 64-bit product
      check_tiling(~0ull - 5, K, ratio);
      for (int i = 0; i < 200; i++) check_tiling(rnd() >> (rnd() % 64), K, ratio);
      for (uint64_t V : {0ull, 1ull, 15ull, 16ull, 17ull, 31ull, 47ull, 100ull, 127ull, 128ull, 129ull, 1000ull, 4099ull})
        check_state(V, K, ratio);
      for (int i = 0; i < 20; i++) check_state(rnd() % 5000, K, ratio);
    }
    for (uint64_t pct : {0ull, 50ull, 99ull, 100ull, 130ull}) {  // cap = 0, short hints, exact, generous
      check_pairs(1, 5, pct, K);       // more slices than pairs
      check_pairs(3, 40, pct, K);      // a handful of graphs: pairs straddle the slices' ends
      check_pairs(60, 9, pct, K);
      check_pairs(8, 0, pct, K);       // no chain at all
      check_pairs(500, 30, pct, K);
    }
  }
  CHECK(stage::clamp_slices(-1, 4) == 4 && stage::clamp_slices(0, 4) == 1 && stage::clamp_slices(3, 4) == 3);
  CHECK(stage::clamp_slices(8, 4) == 8 && stage::clamp_slices(9, 4) == 8 && stage::clamp_slices(1ll << 40, 4) == 8);
  puts("stage_host_check OK");
  return 0;
}
