// gdedup_host_check — drives the host side of the duplicate-graph classes (nemo_amd/csrc/gdedup_host.h
// over dclass_host.h's rounds) against a brute-force partition of random graph contents, with forced
// hash collisions (dedup_hash_bits 0, 1, 8 and 128), graphs kept apart by size, and pre / post graphs
// of equal content; then the run classes over the graph classes (gdedup::run_plan) against brute force
// and hand-made cases, and the pull's slot plan (gdedup::pull_plan).  The comparisons a device would
// make are vector compares here.  Meant for the host sanitizers; it calls nothing on a device:
//   g++ -std=c++17 -g -Wall -fsanitize=address,undefined tools/gdedup_host_check.cpp -o build/gdedup_host_check
//   build/gdedup_host_check
#include "../nemo_amd/csrc/gdedup_host.h"

#include <cstdio>
#include <cstdlib>

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

// a graph's content as the device sees it: parity first, then its words
typedef std::vector<uint32_t> Content;
static dclass::Hash hash_of(const Content &c) {
  dclass::Hash h{0xCBF29CE484222325ull, 0x84222325CBF29CE4ull};
  for (uint32_t w : c) {
    h.lo = (h.lo ^ w) * 0x100000001B3ull;
    h.hi = (h.hi ^ (w + 1u)) * 0x100000001B3ull;
  }
  return h;
}

// the run classes over the graph classes `rep` against brute force -> the number of duplicate runs
static size_t check_run_plan(const std::vector<uint32_t> &rep) {
  const uint32_t n = (uint32_t)(rep.size() / 2);
  const gdedup::RunPlan rp = gdedup::run_plan(rep);
  CHECK(rp.rep.size() == n);
  std::vector<uint32_t> reps;
  for (uint32_t r = 0; r < n; r++) {
    uint32_t f = 0;  // the lowest run with both graphs of r's classes
    while (rep[2 * f] != rep[2 * r] || rep[2 * f + 1] != rep[2 * r + 1]) f++;
    CHECK(rp.rep[r] == f);
    if (f == r) reps.push_back(r);
  }
  CHECK(rp.list == reps);
  CHECK(rp.pairs.size() == 2 * (size_t)(n - reps.size()));
  std::vector<uint8_t> seen(n, 0);
  for (size_t k = 0; k < rp.pairs.size() / 2; k++) {
    const uint32_t d = rp.pairs[2 * k], r = rp.pairs[2 * k + 1];
    CHECK(d < n && r < d && rp.rep[d] == r && rp.rep[r] == r && !seen[d]);
    seen[d] = 1;
    if (k) {  // sorted by representative, then duplicate
      const uint32_t d0 = rp.pairs[2 * k - 2], r0 = rp.pairs[2 * k - 1];
      CHECK(r0 < r || (r0 == r && d0 < d));
    }
  }
  return rp.pairs.size() / 2;
}

// G graphs whose contents are drawn from n_shapes shapes (ignoring parity: a pre and a post graph
// may draw the same shape and must stay apart); graphs of `big` nodes or more are kept apart
static void run_case(uint32_t G, uint32_t n_shapes, uint32_t vmax, uint32_t big, int bits) {
  std::vector<Content> shape(n_shapes ? n_shapes : 1);
  for (auto &s : shape) {
    s.resize(vmax ? rnd() % (vmax + 1) : 0);
    for (auto &w : s) w = (uint32_t)(rnd() % 3);
  }
  std::vector<Content> g(G);
  std::vector<uint64_t> node_off(G + 1, 0);
  std::vector<uint8_t> eligible(G);
  for (uint32_t i = 0; i < G; i++) {
    const Content &s = shape[rnd() % shape.size()];
    g[i].push_back(i & 1u);
    g[i].insert(g[i].end(), s.begin(), s.end());
    node_off[i + 1] = node_off[i] + s.size();
    eligible[i] = s.size() < big;
  }
  std::vector<dclass::Hash> hash(G);
  for (uint32_t i = 0; i < G; i++) hash[i] = hash_of(g[i]);
  dclass::Refiner ref(hash.data(), G, bits);
  std::vector<uint32_t> pairs;
  std::vector<uint8_t> verdict;
  while (ref.next_round(pairs)) {
    verdict.assign(pairs.size() / 2, 0);
    CHECK(verdict.size() < (G ? G : 1));  // the device buffers hold G pairs
    for (size_t k = 0; k < verdict.size(); k++) {
      CHECK(pairs[2 * k] < G && pairs[2 * k + 1] < pairs[2 * k]);
      verdict[k] = g[pairs[2 * k]] == g[pairs[2 * k + 1]];
    }
    ref.verdicts(verdict.data());
  }
  const gdedup::Plan p = gdedup::plan(ref.rep(), eligible, node_off.data());
  // brute force: the first eligible graph of equal content, else the graph itself
  CHECK(p.rep.size() == G);
  std::vector<uint32_t> reps;
  uint64_t dup_nodes = 0;
  uint32_t classes = 0;
  for (uint32_t i = 0; i < G; i++) {
    uint32_t f = i;
    if (eligible[i])
      for (f = 0; !(eligible[f] && g[f] == g[i]); f++) {
      }
    CHECK(p.rep[i] == f);
    if (f == i) {
      reps.push_back(i);
      classes += eligible[i];
    } else {
      CHECK(((f ^ i) & 1u) == 0);
      dup_nodes += node_off[i + 1] - node_off[i];
    }
  }
  CHECK(p.list == reps);
  CHECK(p.classes == classes);
  CHECK(p.dup_nodes == dup_nodes);
  CHECK(p.pairs.size() == 2 * (size_t)(G - reps.size()));
  std::vector<uint8_t> seen(G, 0);
  for (size_t k = 0; k < p.pairs.size() / 2; k++) {
    const uint32_t d = p.pairs[2 * k], r = p.pairs[2 * k + 1];
    CHECK(d < G && r < d && p.rep[d] == r && p.rep[r] == r && !seen[d]);
    seen[d] = 1;
    if (k) {  // sorted by representative, then duplicate
      const uint32_t d0 = p.pairs[2 * k - 2], r0 = p.pairs[2 * k - 1];
      CHECK(r0 < r || (r0 == r && d0 < d));
    }
  }
  // the pull's slot plan: graph -> the list index of its representative (of itself where its class is kept
  // apart, here by size), never after the graph itself
  for (uint32_t cut : {0u, vmax / 2u + 1u, ~0u}) {
    std::vector<uint8_t> apart(G);
    for (uint32_t i = 0; i < G; i++) apart[i] = node_off[i + 1] - node_off[i] >= cut;
    const gdedup::PullPlan pp = gdedup::pull_plan(p.rep, apart);
    CHECK(pp.map.size() == G);
    std::vector<uint32_t> want;
    for (uint32_t i = 0; i < G; i++)
      if (p.rep[i] == i || apart[i]) want.push_back(i);
    CHECK(pp.list == want);
    for (uint32_t i = 0; i < G; i++)
      CHECK(pp.map[i] <= i && pp.map[i] < pp.list.size() && pp.list[pp.map[i]] == (apart[i] ? i : p.rep[i]));
  }
  const size_t dup_runs = check_run_plan(p.rep);
  printf("G %u shapes %u vmax %u big %u bits %d: %zu representatives, %zu duplicates, %u rounds, %zu duplicate runs\n", G,
         n_shapes, vmax, big, bits, reps.size(), p.pairs.size() / 2, ref.rounds(), dup_runs);
}

// hand-made graph classes (rep per graph, run r = graphs 2r, 2r + 1) -> the run classes expected
static void run_class_cases() {
  struct Case {
    std::vector<uint32_t> rep, run_rep, pairs;
  };
  const Case cases[] = {
      // runs 0 and 1 share the post class only, runs 0 and 2 the pre class only, run 3 = run 0
      {{0, 1, 2, 1, 0, 5, 0, 1}, {0, 1, 2, 0}, {3, 0}},
      // a class whose representative is not run 0 (runs 1, 3), and the last run a duplicate (of run 2)
      {{0, 1, 2, 3, 4, 5, 2, 3, 4, 5}, {0, 1, 2, 1, 2}, {3, 1, 4, 2}},
      // pairs sorted by representative, then duplicate: run 0's duplicates 3 and 5 before run 1's 2 and 4
      {{0, 1, 2, 3, 2, 3, 0, 1, 2, 3, 0, 1}, {0, 1, 1, 0, 1, 0}, {3, 0, 5, 0, 2, 1, 4, 1}},
      // the pre graphs of one class, every post graph its own: no duplicate run
      {{0, 1, 0, 3, 0, 5}, {0, 1, 2}, {}},
  };
  for (const Case &c : cases) {
    const gdedup::RunPlan rp = gdedup::run_plan(c.rep);
    CHECK(rp.rep == c.run_rep);
    CHECK(rp.pairs == c.pairs);
    CHECK(check_run_plan(c.rep) == c.pairs.size() / 2);
  }
}

int main() {
  run_class_cases();
  for (int bits : {0, 1, 8, 128}) {
    run_case(0, 1, 4, 100, bits);       // no graph
    run_case(1, 1, 4, 100, bits);       // one graph
    run_case(2, 1, 4, 100, bits);       // one run: equal content, pre and post stay apart
    run_case(64, 1, 9, 100, bits);      // every run a copy of run 0
    run_case(64, 1, 0, 100, bits);      // empty graphs
    run_case(200, 1000, 12, 100, bits);  // mostly singletons
    run_case(300, 7, 30, 100, bits);    // few classes, duplicates before and after
    run_case(300, 7, 30, 12, bits);     // some classes kept apart by size
    run_case(100, 5, 30, 0, bits);      // nothing eligible
  }
  puts("gdedup_host_check OK");
  return 0;
}
