// lcut_host_check — drives the host side of nemo_min_label_cuts (nemo_amd/csrc/lcut_host.h): every outcome of the
// candidate check (a duplicate, UINT32_MAX, the position reported), the min_runs rule at 0, n and n + 1, the two
// limits of a round at their edges (from sizes alone), the live list and its inverse from round 1's two words at
// K = 1, 63, 64, 65, 129, the table at its densest with the kernels' own insert order, and the region sizes.
// Meant for the host sanitizers; it calls nothing on a device:
//   g++ -std=c++17 -g -Wall -fsanitize=address,undefined -static-libasan -static-libubsan
//       tools/lcut_host_check.cpp -o tools/lcut_host_check
//   tools/lcut_host_check
#include "../nemo_amd/csrc/lcut_host.h"

#include <cstdio>
#include <cstdlib>

#define CHECK(x)                                            \
  do {                                                      \
    if (!(x)) {                                             \
      fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #x); \
      exit(1);                                              \
    }                                                       \
  } while (0)

static void check_candidates() {
  size_t where = 99;
  CHECK(lcuts::check_cands(nullptr, 0, &where) == cuts::CAND_OK);
  const uint32_t ok[5] = {10, 11, 12, 0, 0xFFFFFFFEu};
  CHECK(lcuts::check_cands(ok, 5, &where) == cuts::CAND_OK);
  CHECK(lcuts::check_cands(ok, 5, nullptr) == cuts::CAND_OK);
  const uint32_t none[4] = {7, 0xFFFFFFFFu, 7, 0xFFFFFFFFu};
  CHECK(lcuts::check_cands(none, 4, &where) == cuts::CAND_RANGE && where == 1);  // before the duplicate
  CHECK(lcuts::check_cands(none, 1, &where) == cuts::CAND_OK);
  const uint32_t dup[6] = {5, 9, 3, 9, 5, 3};
  CHECK(lcuts::check_cands(dup, 6, &where) == cuts::CAND_DUP && where == 3);  // the first second occurrence
  CHECK(lcuts::check_cands(dup, 3, &where) == cuts::CAND_OK);
  std::vector<uint32_t> many(5000);
  for (uint32_t i = 0; i < 5000; i++) many[i] = 0x80000000u + 7u * i;
  CHECK(lcuts::check_cands(many.data(), many.size(), &where) == cuts::CAND_OK);
  many[4999] = many[0];
  CHECK(lcuts::check_cands(many.data(), many.size(), &where) == cuts::CAND_DUP && where == 4999);
}

static void check_min_runs() {
  uint32_t q = 99;
  CHECK(lcuts::min_runs(0, 0, &q) && q == 0);
  CHECK(!lcuts::min_runs(0, 1, &q));
  CHECK(lcuts::min_runs(3, 0, &q) && q == 3);
  CHECK(lcuts::min_runs(3, 1, &q) && q == 1);
  CHECK(lcuts::min_runs(3, 3, &q) && q == 3);
  CHECK(!lcuts::min_runs(3, 4, &q) && q == 3);  // left alone
  CHECK(lcuts::min_runs(70, 35, nullptr));
  CHECK(lcuts::min_runs(0xFFFFFFFFull, 0xFFFFFFFFu, &q) && q == 0xFFFFFFFFu);
}

static void check_limits() {
  // hypotheses: C(92682, 2) = 4294930221 <= 2^32 - 2 < C(92683, 2); C(2954, 3) = 4291795704 <= 2^32 - 2 < C(2955, 3)
  CHECK(lcuts::round_check(1, 0xFFFFFFFEull, 1) == lcuts::ROUND_OK && lcuts::round_check(1, 0xFFFFFFFFull, 1) == lcuts::ROUND_HYPS);
  CHECK(lcuts::round_check(1, 92682, 2) == lcuts::ROUND_OK && lcuts::round_check(1, 92683, 2) == lcuts::ROUND_HYPS);
  CHECK(lcuts::round_check(1, 2954, 3) == lcuts::ROUND_OK && lcuts::round_check(1, 2955, 3) == lcuts::ROUND_HYPS);
  CHECK(lcuts::round_check(1, 1ull << 40, 2) == lcuts::ROUND_HYPS && lcuts::round_check(1, ~0ull, 3) == lcuts::ROUND_HYPS);
  // words: n x ceil(hyps / 64) <= 2^28
  CHECK(lcuts::round_check(1ull << 22, 4096, 1) == lcuts::ROUND_OK);           // 2^22 x 64
  CHECK(lcuts::round_check((1ull << 22) + 1, 4096, 1) == lcuts::ROUND_WORDS);  // (2^22 + 1) x 64
  CHECK(lcuts::round_check(1ull << 22, 4097, 1) == lcuts::ROUND_WORDS);        // 2^22 x 65
  CHECK(lcuts::round_check(1ull << 28, 64, 1) == lcuts::ROUND_OK && lcuts::round_check(1ull << 28, 65, 1) == lcuts::ROUND_WORDS);
  // 70 list positions: 2^28 / 70 = 3834792 chunks; C(22155, 2) makes 3834546 chunks, C(22156, 2) 3834893: too many
  CHECK(lcuts::round_check(70, 22155, 2) == lcuts::ROUND_OK && lcuts::round_check(70, 22156, 2) == lcuts::ROUND_WORDS);
  CHECK(lcuts::round_check(70, 23, 3) == lcuts::ROUND_OK && lcuts::round_check(4, 2954, 3) == lcuts::ROUND_OK);
  CHECK(lcuts::round_check(5, 2954, 3) == lcuts::ROUND_WORDS);  // 67059308 chunks x 5 > 2^28 >= x 4
  // no list position, no candidate: nothing to exceed
  CHECK(lcuts::round_check(0, 100, 3) == lcuts::ROUND_OK && lcuts::round_check(1ull << 40, 0, 1) == lcuts::ROUND_OK);
  CHECK(lcuts::round_check(1ull << 40, 2, 3) == lcuts::ROUND_OK);  // fewer live candidates than the size: zero hypotheses
}

static void check_live() {
  for (size_t K : {1u, 63u, 64u, 65u, 129u}) {
    const size_t ck = cuts::chunks(K);
    std::vector<uint64_t> cut(ck, 0), hit(ck, 0);
    std::vector<uint32_t> want;
    for (size_t p = 0; p < K; p++) {
      const bool is_cut = p % 5 == 1, is_hit = p % 3 != 2 || is_cut;  // a cut hits a node
      if (is_cut) cut[p / 64] |= 1ull << (p % 64);
      if (is_hit) hit[p / 64] |= 1ull << (p % 64);
      if (!is_cut && is_hit) want.push_back((uint32_t)p);
    }
    const std::vector<uint32_t> live = lcuts::live_list(cut.data(), hit.data(), K);
    CHECK(live == want);
    const std::vector<uint32_t> map = lcuts::live_map(live, K);
    CHECK(map.size() == K);
    size_t n_live = 0;
    for (size_t p = 0; p < K; p++) {
      if (map[p] == LC_NONE) continue;
      CHECK(map[p] == n_live && live[map[p]] == p);
      n_live++;
    }
    CHECK(n_live == live.size());
    // bits past K in the last word are not read
    if (K % 64) hit[ck - 1] |= ~((1ull << (K % 64)) - 1);
    CHECK(lcuts::live_list(cut.data(), hit.data(), K) == want);
  }
  const uint64_t all = ~0ull, zero = 0ull;
  CHECK(lcuts::live_list(&zero, &all, 64).size() == 64);  // nothing a cut, everything hit
  CHECK(lcuts::live_list(&all, &all, 64).empty());        // every singleton a cut
  CHECK(lcuts::live_list(&zero, &zero, 64).empty());      // nothing hit
  CHECK(lcuts::live_list(nullptr, nullptr, 0).empty());
  CHECK(lcuts::live_map({}, 3) == std::vector<uint32_t>(3, LC_NONE));
}

static void check_table() {
  CHECK(lcuts::table_slots(0) == 16 && lcuts::table_slots(8) == 16 && lcuts::table_slots(9) == 32 && lcuts::table_slots(129) == 512);
  // K distinct labels, the kernel's insert (first free slot of the chain) and the sweeps' probe: label -> position
  for (uint32_t K : {1u, 64u, 129u, 4096u}) {
    const uint64_t slots = lcuts::table_slots(K);
    CHECK(slots >= 2ull * K);
    std::vector<uint32_t> key(slots, 0), val(slots, LC_NONE);
    for (uint32_t p = 0; p < K; p++) {
      const uint32_t label = 0xFFFFFFFEu - 3u * p;  // the largest legal label among them
      uint64_t h = klabel::first_slot(label, slots);
      while (key[h]) h = klabel::next_slot(h, slots);
      key[h] = label + 1u, val[h] = p;
    }
    for (uint32_t p = 0; p < K; p++) {
      const uint32_t label = 0xFFFFFFFEu - 3u * p;
      uint64_t h = klabel::first_slot(label, slots);
      while (key[h] && key[h] != label + 1u) h = klabel::next_slot(h, slots);
      CHECK(key[h] == label + 1u && val[h] == p);
      CHECK(!klabel::probe(key.data(), nullptr, slots, label - 1u, nullptr));
    }
  }
  // regions: k1 + 1 offsets and at most V nodes; what the head does not hold, in u64, whole 16-byte pairs
  CHECK(lcuts::list_entries(0, 0) == 1 && lcuts::list_entries(12, 300) == 313);
  CHECK(lcuts::region_words(0, 313, 313) == 0 && lcuts::region_words(0, 313, 1000) == 0);
  CHECK(lcuts::region_words(0, 313, 312) == 2 && lcuts::region_words(0, 313, 309) == 2 && lcuts::region_words(0, 313, 308) == 4);
  CHECK(lcuts::region_words(6, 313, 0) == 6 + 158 && lcuts::region_words(5, 0, 0) == 6);
  for (uint64_t e = 0; e < 200; e++)
    for (uint64_t head = 0; head < 200; head += 7) {
      const uint64_t w = lcuts::region_words(0, e, head);
      CHECK(w % 2 == 0 && 2 * w >= (e > head ? e - head : 0));
    }
}

int main() {
  check_candidates();
  check_min_runs();
  check_limits();
  check_live();
  check_table();
  printf("lcut_host_check OK\n");
  return 0;
}
