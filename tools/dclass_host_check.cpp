// dclass_host_check — drives the host side of nemo_diff_classes (nemo_amd/csrc/dclass_host.h: hash
// buckets, comparison rounds, class numbering) against a brute-force partition of random rows, with
// forced hash collisions (class_hash_bits 0, 1, 8 and 128), duplicate sources and zero entries.
// The row comparisons a device would make are memcmp here.  Meant for the host sanitizers; it calls
// nothing on a device:
//   g++ -std=c++17 -g -Wall -fsanitize=address,undefined tools/dclass_host_check.cpp -o build/dclass_host_check
//   build/dclass_host_check
#include "../nemo_amd/csrc/dclass_host.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>

#define CHECK(x)                                            \
  do {                                                      \
    if (!(x)) {                                             \
      fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #x); \
      exit(1);                                              \
    }                                                       \
  } while (0)

static uint64_t rng_state = 0x2545F4914F6CDD1Dull;
static uint64_t rnd() {
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 7;
  rng_state ^= rng_state << 17;
  return rng_state;
}

// FNV-1a twice over a row: equal rows hash alike, which is all the refinement relies on
static dclass::Hash hash_row(const std::vector<uint8_t> &r) {
  dclass::Hash h{0xCBF29CE484222325ull, 0x84222325CBF29CE4ull};
  for (uint8_t b : r) {
    h.lo = (h.lo ^ b) * 0x100000001B3ull;
    h.hi = (h.hi ^ (b + 1u)) * 0x100000001B3ull;
  }
  return h;
}

// n entries over nu distinct sources (entry -> source in order of first use), the sources' rows
// drawn from n_shapes shapes, so that classes of several sources exist
static void run_case(uint32_t n, uint32_t nu, uint32_t n_shapes, uint32_t V, int bits) {
  std::vector<std::vector<uint8_t>> shape(n_shapes ? n_shapes : 1, std::vector<uint8_t>(V, 0));
  for (auto &s : shape)
    for (auto &b : s) b = rnd() % 4 == 0;
  if (!shape.empty() && V) std::fill(shape[0].begin(), shape[0].end(), 0);  // the all-zero mask is a class too
  std::vector<std::vector<uint8_t>> row(nu);
  for (auto &r : row) r = shape[rnd() % shape.size()];
  std::vector<uint32_t> item_of(n), first(nu, 0xFFFFFFFFu), nodes(nu, 0);
  uint32_t used = 0;
  for (uint32_t e = 0; e < n; e++) {
    // a new source while some are left, else (or at random) a duplicate of an earlier one
    const bool fresh = used < nu && (used == 0 || n - e <= nu - used || rnd() % 3);
    item_of[e] = fresh ? used++ : (uint32_t)(rnd() % used);
    if (first[item_of[e]] == 0xFFFFFFFFu) first[item_of[e]] = e;
  }
  CHECK(used == nu);
  std::vector<dclass::Hash> hash(nu);
  for (uint32_t u = 0; u < nu; u++) {
    hash[u] = hash_row(row[u]);
    for (uint8_t b : row[u]) nodes[u] += b;
  }
  dclass::Refiner ref(hash.data(), nu, bits);
  std::vector<uint32_t> pairs;
  std::vector<uint8_t> verdict;
  uint64_t compared = 0;
  while (ref.next_round(pairs)) {
    verdict.assign(pairs.size() / 2, 0);
    for (size_t k = 0; k < verdict.size(); k++) {
      CHECK(pairs[2 * k] < nu && pairs[2 * k + 1] < nu && pairs[2 * k + 1] < pairs[2 * k]);
      verdict[k] = row[pairs[2 * k]] == row[pairs[2 * k + 1]];
    }
    compared += verdict.size();
    CHECK(verdict.size() < (nu ? nu : 1));
    ref.verdicts(verdict.data());
  }
  std::vector<uint32_t> class_of;
  std::vector<nemo_diff_class> classes;
  dclass::finish(ref.rep(), item_of.data(), n, first.data(), nodes.data(), class_of, classes);
  // brute force: entry e's class is that of the smallest entry with an equal row
  std::vector<uint32_t> want(n), reps;
  for (uint32_t e = 0; e < n; e++) {
    uint32_t f = 0;
    while (!(row[item_of[f]] == row[item_of[e]])) f++;
    if (f == e) reps.push_back(e);
    want[e] = f;
  }
  CHECK(classes.size() == reps.size());
  CHECK(class_of.size() == n);
  std::vector<uint32_t> size(reps.size(), 0);
  for (uint32_t e = 0; e < n; e++) {
    CHECK(class_of[e] < classes.size());
    CHECK(classes[class_of[e]].rep == want[e]);
    size[class_of[e]]++;
  }
  for (size_t k = 0; k < classes.size(); k++) {
    CHECK(classes[k].rep == reps[k]);  // numbered by smallest entry
    CHECK(classes[k].size == size[k]);
    CHECK(classes[k].nodes == nodes[item_of[reps[k]]]);
  }
  if (bits == 0 && nu) CHECK(ref.rounds() == classes.size());  // one class per round when every hash collides
  if (bits == 128) CHECK(ref.rounds() <= 1u);
  printf("n %u sources %u shapes %u V %u bits %d: %zu classes, %u rounds, %llu comparisons\n", n, nu, n_shapes, V, bits,
         classes.size(), ref.rounds(), (unsigned long long)compared);
}

int main() {
  for (int bits : {0, 1, 8, 128}) {
    run_case(0, 0, 1, 8, bits);       // zero entries
    run_case(1, 1, 1, 0, bits);       // one entry over an empty graph
    run_case(7, 1, 3, 16, bits);      // one source (reference mode): one class
    run_case(40, 40, 40, 5, bits);    // short rows: many accidental equalities
    run_case(200, 130, 17, 70, bits);  // duplicate sources, classes of several sources
    run_case(300, 300, 1000, 33, bits);  // mostly singletons
  }
  // the option's range: low_bits keeps exactly k bits
  dclass::Hash f{~0ull, ~0ull};
  for (int k = 0; k <= 128; k++) {
    const dclass::Hash g = dclass::low_bits(f, k);
    CHECK(__builtin_popcountll(g.lo) + __builtin_popcountll(g.hi) == k);
  }
  puts("dclass_host_check OK");
  return 0;
}
