// repair_host_check — drives the host side of nemo_min_repair_sets / nemo_min_repairs (nemo_amd/csrc/repair_host.h):
// every outcome of the validation of the absent and the candidate list with every reported position, the bitmap's word
// counts and contents, the LDS image's bytes and the tier at its edge, and the status round 0's word decides.
// Meant for the host sanitizers; it calls nothing on a device:
//   g++ -std=c++17 -g -Wall -fsanitize=address,undefined -static-libasan -static-libubsan
//       tools/repair_host_check.cpp -o tools/repair_host_check
//   tools/repair_host_check
#include "../nemo_amd/csrc/repair_host.h"

#include <cstdio>
#include <cstdlib>

#define CHECK(x)                                            \
  do {                                                      \
    if (!(x)) {                                             \
      fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #x); \
      exit(1);                                              \
    }                                                       \
  } while (0)

static repair::ListCheck lists(const std::vector<uint32_t> &a, const std::vector<uint32_t> *c, uint64_t V, size_t *where) {
  *where = ~(size_t)0;
  // exact-size heap copies: a read past either list is the sanitizer's to find
  std::vector<uint32_t> ac(a), cc(c ? *c : std::vector<uint32_t>());
  ac.shrink_to_fit(), cc.shrink_to_fit();
  return repair::check_lists(ac.data(), ac.size(), c ? cc.data() : nullptr, cc.size(), V, where);
}

static void check_lists() {
  size_t w;
  std::vector<uint32_t> none;
  CHECK(lists({}, nullptr, 0, &w) == repair::LIST_OK);
  CHECK(lists({}, &none, 8, &w) == repair::LIST_OK);
  CHECK(lists({3, 1, 7}, nullptr, 8, &w) == repair::LIST_OK);
  // an absent node >= V, at every position; the first offence is reported
  for (size_t p = 0; p < 5; p++) {
    std::vector<uint32_t> a = {0, 1, 2, 3, 4};
    a[p] = 8;
    CHECK(lists(a, nullptr, 8, &w) == repair::ABSENT_RANGE && w == p);
    a[4] = 0xFFFFFFFFu;
    CHECK(lists(a, nullptr, 8, &w) == repair::ABSENT_RANGE && w == (p < 4 ? p : 4));
  }
  CHECK(lists({0}, nullptr, 0, &w) == repair::ABSENT_RANGE && w == 0);
  // a range offence comes before a duplicate, whatever their order in the list
  CHECK(lists({1, 1, 9}, nullptr, 8, &w) == repair::ABSENT_RANGE && w == 2);
  // an absent node twice: the position of the earliest second occurrence
  for (size_t p = 1; p < 6; p++)
    for (size_t q = 0; q < p; q++) {
      std::vector<uint32_t> a = {10, 11, 12, 13, 14, 15};
      a[p] = a[q];
      CHECK(lists(a, nullptr, 16, &w) == repair::ABSENT_DUP && w == p);
    }
  CHECK(lists({5, 4, 4, 5, 5}, nullptr, 8, &w) == repair::ABSENT_DUP && w == 2);
  // more entries than nodes: some node twice within the first V + 1
  {
    std::vector<uint32_t> a(40);
    for (size_t i = 0; i < a.size(); i++) a[i] = (uint32_t)(i % 7);
    CHECK(lists(a, nullptr, 7, &w) == repair::ABSENT_DUP && w == 7);
  }
  // the candidates: a duplicate, at every pair of positions
  const std::vector<uint32_t> A = {20, 3, 9, 14, 6};
  for (size_t p = 1; p < 5; p++)
    for (size_t q = 0; q < p; q++) {
      std::vector<uint32_t> c = {6, 14, 9, 3, 20};
      c[p] = c[q];
      CHECK(lists(A, &c, 32, &w) == repair::CAND_DUP && w == p);
    }
  // a candidate that is not absent, at every position: in range, out of range, and with an empty absent list
  for (size_t p = 0; p < 4; p++) {
    std::vector<uint32_t> c = {6, 14, 9, 3};
    c[p] = 7;
    CHECK(lists(A, &c, 32, &w) == repair::CAND_NOT_ABSENT && w == p);
    c[p] = 32;
    CHECK(lists(A, &c, 32, &w) == repair::CAND_NOT_ABSENT && w == p);
    c[p] = 0xFFFFFFFFu;
    CHECK(lists(A, &c, 32, &w) == repair::CAND_NOT_ABSENT && w == p);
  }
  {
    std::vector<uint32_t> c = {4};
    CHECK(lists({}, &c, 8, &w) == repair::CAND_NOT_ABSENT && w == 0);
    c = {7, 7};  // a duplicate comes before a stranger
    CHECK(lists({3}, &c, 8, &w) == repair::CAND_DUP && w == 1);
    c = {3, 5, 3};  // ... also where the stranger stands first; a list longer than the absent list is cut at |A| + 1
    CHECK(lists({3}, &c, 8, &w) == repair::CAND_NOT_ABSENT && w == 1);
    c = {3, 3, 5};
    CHECK(lists({3}, &c, 8, &w) == repair::CAND_DUP && w == 1);
  }
  // the absent list's offences come before the candidates'
  {
    std::vector<uint32_t> c = {1, 1};
    CHECK(lists({1, 2, 2}, &c, 8, &w) == repair::ABSENT_DUP && w == 2);
    CHECK(lists({1, 8}, &c, 8, &w) == repair::ABSENT_RANGE && w == 1);
  }
  // every subset order is fine
  {
    std::vector<uint32_t> c = {14, 20, 3};
    CHECK(lists(A, &c, 21, &w) == repair::LIST_OK);
    c = A;
    CHECK(lists(A, &c, 21, &w) == repair::LIST_OK);
  }
  CHECK(repair::check_lists(A.data(), A.size(), nullptr, 0, 32, nullptr) == repair::LIST_OK);  // where may be null
  const uint32_t bad[2] = {1, 1};
  CHECK(repair::check_lists(bad, 2, nullptr, 0, 32, nullptr) == repair::ABSENT_DUP);
}

static void check_bitmap() {
  CHECK(repair::bitmap_words(0) == 0);
  for (uint64_t V = 1; V <= 1000; V++) {
    const uint64_t w = repair::bitmap_words(V);
    CHECK(w % 2 == 0 && 64 * w >= V && 64 * w < V + 128);  // whole 16-byte pairs, no pair too many
  }
  CHECK(repair::bitmap_words(64) == 2 && repair::bitmap_words(65) == 2 && repair::bitmap_words(128) == 2 && repair::bitmap_words(129) == 4);
  CHECK(repair::bitmap_words(0xFFFFFFFFull) == 67108864ull);
  for (uint64_t V : {1ull, 63ull, 64ull, 65ull, 127ull, 129ull, 300ull}) {
    std::vector<uint32_t> a;
    for (uint64_t v = 0; v < V; v += 3) a.push_back((uint32_t)v);
    if (a.back() != V - 1) a.push_back((uint32_t)(V - 1));
    const std::vector<uint64_t> b = repair::bitmap(a.data(), a.size(), V);
    CHECK(b.size() == repair::bitmap_words(V));
    uint64_t n = 0;
    for (uint64_t v = 0; v < 64 * b.size(); v++) {
      const bool set = (b[v >> 6] >> (v & 63)) & 1;
      CHECK(set == (v < V && (v % 3 == 0 || v == V - 1)));  // the bits past V are 0
      n += set;
    }
    CHECK(n == a.size());
  }
  CHECK(repair::bitmap(nullptr, 0, 0).empty());
}

static void check_lds() {
  for (uint32_t V : {1u, 2u, 63u, 64u, 65u, 5002u, 65535u})
    for (uint32_t E : {0u, 1u, 7463u, 65535u})
      for (uint32_t L : {1u, 2u, 301u}) {
        const uint32_t b = repair::repair_lds_bytes(V, E, L);
        CHECK(b % 16 == 0 && b == knock::knock_lds_bytes(V, E, L) + 8u * (uint32_t)repair::bitmap_words(V));
        if (L > V) continue;
        CHECK(repair::lds_fits(V, E, L, b) && !repair::lds_fits(V, E, L, b - 1));  // the bitmap counts in the tier decision
        CHECK(!repair::lds_fits(V, E, L, 0));
      }
  // a graph at the edge of k_ko_lds's tier that the bitmap pushes out of k_repair_lds's
  {
    const uint32_t V = 5002, E = 7463, L = 40;
    const uint32_t ko = knock::knock_lds_bytes(V, E, L);
    CHECK(knock::lds_fits(V, E, L, ko) && !repair::lds_fits(V, E, L, ko));
  }
  CHECK(!repair::lds_fits(65536, 10, 3, KO_LDS_MAX) && !repair::lds_fits(100, 65536, 3, KO_LDS_MAX) && !repair::lds_fits(3, 2, 4, KO_LDS_MAX));
  CHECK(repair::lds_fits(5002, 7463, 40, KO_LDS_MAX));  // the C3 shape stays on the LDS tier
}

static void check_status() {
  CHECK(repair::status(0) == REPAIR_BEYOND);
  CHECK(repair::status(1) == REPAIR_HOLDS);
  CHECK(repair::status(2) == REPAIR_SEARCHED);
  CHECK(repair::status(3) == REPAIR_HOLDS);  // monotone: what holds under {} holds under cand
  CHECK(REPAIR_HOLDS == 0 && REPAIR_SEARCHED == 1 && REPAIR_BEYOND == 2);
}

int main() {
  check_lists();
  check_bitmap();
  check_lds();
  check_status();
  printf("repair_host_check OK\n");
  return 0;
}
