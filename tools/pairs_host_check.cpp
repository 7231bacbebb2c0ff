// pairs_host_check — drives the host side of nemo_diffprov_pairs' label hash tables
// (nemo_amd/csrc/pairs_host.h): the distinct `other` graphs of a call, each table's capacity and
// its place in the per-call region, against a brute-force recount; then fills every table the way
// k_lab_hash does (key = label + 1, hash_label, linear probing) and probes it the way
// sdiff_mark_bad does, inside the table's own slots only.  Meant for the host sanitizers; it
// calls nothing on a device:
//   g++ -std=c++17 -g -Wall -fsanitize=address,undefined -static-libasan -static-libubsan
//       tools/pairs_host_check.cpp -o build/pairs_host_check
//   build/pairs_host_check
#include "../nemo_amd/csrc/pairs_host.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <set>

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

// device.h's slot hash (that header needs the HIP runtime)
static uint32_t hash_label(uint32_t x) {
  x *= 0x9E3779B1u;
  return x ^ (x >> 15);
}

static void check_capacity() {
  CHECK(pairs::capacity(0) == 16 && pairs::capacity(8) == 16 && pairs::capacity(9) == 32);
  CHECK(pairs::capacity(33) == 128 && pairs::capacity(64) == 128 && pairs::capacity(65) == 256);
  CHECK(pairs::capacity(1025) == 4096 && pairs::capacity(5005) == 16384 && pairs::capacity(66000) == 262144);
  CHECK(pairs::capacity(1ull << 31) == (1ull << 32) && pairs::capacity((1ull << 31) + 1) == (1ull << 33));
  for (int k = 0; k < 2000; k++) {
    const uint64_t v = rnd() % (1u << (1 + rnd() % 24));
    const uint64_t cap = pairs::capacity(v);
    CHECK((cap & (cap - 1)) == 0 && cap >= 16 && cap >= 2 * v && cap % 4 == 0);
    CHECK(cap == 16 || cap / 2 < 2 * v);  // the smallest such power of two
  }
}

// G post graphs of up to vmax nodes (some empty, some without a goal), n entries drawn from them
static void run_case(uint32_t G, uint32_t vmax, size_t n, int64_t shared, uint32_t label_space) {
  std::vector<uint64_t> node_off(G + 1, 0);
  std::vector<std::vector<uint32_t>> goal_labels(G);  // a graph's goals' labels (several goals may share one)
  for (uint32_t g = 0; g < G; g++) {
    const uint32_t v = rnd() % 4 == 0 ? 0u : (uint32_t)(rnd() % (vmax + 1));
    node_off[g + 1] = node_off[g] + v;
    const bool no_goal = rnd() % 5 == 0;
    for (uint32_t i = 0; i < v && !no_goal; i++)
      if (rnd() % 2) goal_labels[g].push_back((uint32_t)(rnd() % label_space));
  }
  std::vector<uint32_t> other(n);
  for (auto &g : other) g = (uint32_t)(rnd() % (G ? G : 1));
  const pairs::Plan p = pairs::plan(other.data(), n, node_off.data(), shared);
  CHECK(p.ok);
  // dedupe: the distinct graphs other than the shared one, in first-entry order
  std::vector<uint32_t> want;
  uint64_t nodes = 0, max_cap = 0;
  for (size_t e = 0; e < n; e++) {
    if (shared >= 0 && other[e] == (uint32_t)shared) {
      CHECK(p.entry_tab[e] == PAIRS_SHARED);
      continue;
    }
    auto f = std::find(want.begin(), want.end(), other[e]);
    if (f == want.end()) {
      want.push_back(other[e]);
      nodes += node_off[other[e] + 1] - node_off[other[e]];
      f = want.end() - 1;
    }
    CHECK(p.entry_tab[e] == (uint32_t)(f - want.begin()));
  }
  CHECK(p.tab_graph == want && p.nodes == nodes);
  const size_t nt = want.size();
  CHECK(p.tab_off.size() == nt + 1 && p.tab_mask.size() == nt && p.tab_off[0] == 0 && p.words == p.tab_off[nt]);
  // capacities and offsets: back to back, 16-byte aligned, no overlap
  for (size_t t = 0; t < nt; t++) {
    const uint64_t v = node_off[want[t] + 1] - node_off[want[t]], cap = (uint64_t)p.tab_mask[t] + 1;
    CHECK(cap == pairs::capacity(v) && cap >= 2 * goal_labels[want[t]].size());
    CHECK(p.tab_off[t] % 4 == 0 && p.tab_off[t + 1] == p.tab_off[t] + cap);
    max_cap = std::max(max_cap, cap);
  }
  CHECK(p.max_cap == max_cap);
  // fill as k_lab_hash, probe as sdiff_mark_bad: the region is exactly p.words slots, so a slot
  // outside a table's own range is a sanitizer report or a foreign key
  std::vector<uint32_t> region(p.words, 0u);
  std::vector<uint32_t> owner(p.words, 0xFFFFFFFFu);
  for (size_t t = 0; t < nt; t++) {
    uint32_t *tab = region.data() + p.tab_off[t];
    const uint32_t mask = p.tab_mask[t];
    for (uint32_t l : goal_labels[want[t]]) {
      uint32_t h = hash_label(l) & mask;
      while (tab[h] != 0u && tab[h] != l + 1u) h = (h + 1u) & mask;
      tab[h] = l + 1u;  // a label held by several goals is inserted once
      CHECK(owner[p.tab_off[t] + h] == 0xFFFFFFFFu || owner[p.tab_off[t] + h] == t);
      owner[p.tab_off[t] + h] = (uint32_t)t;
    }
    const std::set<uint32_t> have(goal_labels[want[t]].begin(), goal_labels[want[t]].end());
    uint32_t used = 0;
    for (uint32_t h = 0; h <= mask; h++) used += tab[h] != 0u;
    CHECK(used == have.size() && 2ull * used <= (uint64_t)mask + 1);
    for (uint32_t l = 0; l < label_space; l++) {
      uint32_t h = hash_label(l) & mask, steps = 0;
      bool found = false;
      while (tab[h] != 0u) {
        if (tab[h] == l + 1u) {
          found = true;
          break;
        }
        h = (h + 1u) & mask;
        CHECK(++steps <= mask);  // an empty slot ends every probe sequence
      }
      CHECK(found == (have.count(l) != 0));
    }
  }
  printf("graphs %u vmax %u entries %zu shared %lld: %zu tables, %llu slots\n", G, vmax, n, (long long)shared, nt,
         (unsigned long long)p.words);
}

int main() {
  check_capacity();
  run_case(1, 0, 0, -1, 8);      // no entry
  run_case(1, 0, 5, -1, 8);      // an empty graph: a 16-slot table of zeros
  run_case(1, 12, 9, 0, 8);      // every entry against the load's table: nothing built
  run_case(4, 12, 1, -1, 8);     // one entry
  run_case(6, 19, 40, 1, 6);     // many entries share few tables; labels repeat among the goals
  run_case(64, 40, 64, 3, 50);   // about one table per entry
  run_case(300, 70, 1000, -1, 4000);  // no run 0 in the corpus
  run_case(40, 1100, 200, 7, 100000);  // capacities up to 4096: probe chains
  run_case(3, 70000, 8, -1, 1u << 20);  // a table past any LDS budget
  // a graph past 2^31 nodes has no 32-bit mask
  {
    const uint64_t off[2] = {0, (1ull << 31) + 1};
    const uint32_t g = 0;
    CHECK(!pairs::plan(&g, 1, off, -1).ok);
    const uint64_t off2[2] = {0, 1ull << 31};
    const pairs::Plan p = pairs::plan(&g, 1, off2, -1);
    CHECK(p.ok && p.tab_mask[0] == 0xFFFFFFFFu && p.words == (1ull << 32));
  }
  puts("pairs_host_check OK");
  return 0;
}
