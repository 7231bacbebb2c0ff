// lrepair_host_check — drives the host side of nemo_lineage_repair_sets / nemo_lineage_repairs
// (nemo_amd/csrc/lrep_host.h): k_lrep_lds's LDS image, where its three word arrays and the bitmap lie, the tier at its
// edge and at the C3 shape, a workgroup's region on the global tier, the byte model, the candidate limit, the status
// the two-hypothesis launch's lost word decides, and, with lin_host.h's keys, what the kernel does to a chunk's stop
// rule words and what it emits from them.  Meant for the host sanitizers; it calls nothing on a device:
//   g++ -std=c++17 -g -Wall -fsanitize=address,undefined -static-libasan -static-libubsan
//       tools/lrepair_host_check.cpp -o tools/lrepair_host_check
//   tools/lrepair_host_check
#include "../nemo_amd/csrc/lrep_host.h"

#include <cstdio>
#include <cstdlib>

#define CHECK(x)                                            \
  do {                                                      \
    if (!(x)) {                                             \
      fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #x); \
      exit(1);                                              \
    }                                                       \
  } while (0)

static void check_image() {
  for (uint32_t V : {1u, 2u, 63u, 64u, 65u, 5002u, 5106u})
    for (uint32_t E : {0u, 1u, 7463u, 65535u})
      for (uint32_t L : {1u, 2u, 40u, 301u}) {
        const uint32_t b = lrep::lrep_lds_bytes(V, E, L);
        const uint32_t words = knock::ko_align(8u * V);
        CHECK(b % 16 == 0);
        CHECK(b == knock::knock_lds_bytes(V, E, L) + 2u * words + 8u * (uint32_t)repair::bitmap_words(V));
        CHECK(b == wit::wit_lds_bytes(V, E, L) + words + 8u * (uint32_t)repair::bitmap_words(V));
        // the arrays follow one another, whole 16-byte pairs each, and end with the image
        const uint32_t o_blame = lrep::blame_offset(V, E, L), o_rem = lrep::removed_offset(V, E, L), o_bits = lrep::bitmap_offset(V, E, L);
        CHECK(o_blame % 16 == 0 && o_rem % 16 == 0 && o_bits % 16 == 0);
        CHECK(o_blame == knock::knock_lds_bytes(V, E, L) && o_rem == o_blame + words && o_bits == o_rem + words);
        CHECK(o_bits + 8u * (uint32_t)repair::bitmap_words(V) == b);
        CHECK(words >= 8u * ((V + 1u) & ~1u));  // the zeroing and the fill write whole pairs of nodes
        if (L > V) continue;
        if (b <= WIT_LDS_MAX) CHECK(lrep::lds_fits(V, E, L, b) && !lrep::lds_fits(V, E, L, b - 1));
        CHECK(!lrep::lds_fits(V, E, L, 0));
      }
  CHECK(!lrep::lds_fits(65536, 10, 3, WIT_LDS_MAX) && !lrep::lds_fits(100, 65536, 3, WIT_LDS_MAX) && !lrep::lds_fits(3, 2, 4, WIT_LDS_MAX));
  // the C3 shape stays on the LDS tier under the default of wit_lds_max, with a workgroup's static LDS to spare
  const uint32_t c3 = lrep::lrep_lds_bytes(5002, 7463, 40);
  CHECK(c3 == 156384u && lrep::lds_fits(5002, 7463, 40, WIT_LDS_DEFAULT));
  CHECK(wit::lds_fits(5002, 7463, 40, WIT_LDS_DEFAULT) && c3 == wit::wit_lds_bytes(5002, 7463, 40) + 40016u + 640u);
  // the largest graph of the C3 shape (E / V = 7463 / 5002, 40 levels) the tier takes
  uint32_t best = 0;
  for (uint32_t V = 5002; V < 6000; V++) {
    const uint32_t E = (uint32_t)((uint64_t)V * 7463u / 5002u);
    if (lrep::lds_fits(V, E, 40, WIT_LDS_DEFAULT)) best = V;
  }
  printf("largest C3-shaped graph on the LDS tier: %u nodes, %u edges, %u bytes\n", best, (uint32_t)((uint64_t)best * 7463u / 5002u),
         lrep::lrep_lds_bytes(best, (uint32_t)((uint64_t)best * 7463u / 5002u), 40));
  CHECK(best >= 5002 && !lrep::lds_fits(best + 1, (uint32_t)((uint64_t)(best + 1) * 7463u / 5002u), 40, WIT_LDS_DEFAULT));
}

static void check_region() {
  for (uint64_t V : {0ull, 1ull, 2ull, 3ull, 65535ull, 65536ull, 140001ull}) {
    CHECK(lrep::glob_words(V) == 3 * knock::dead_words(V));
    CHECK(lrep::glob_words(V) % 2 == 0 && lrep::glob_words(V) >= 3 * V && lrep::glob_words(V) == wit::glob_words(V) + knock::dead_words(V));
  }
  CHECK(lrep::image_bytes(5002, 7463, 40) == wit::image_bytes(5002, 7463, 40) + 8.0 * 80.0);
}

static void check_limits() {
  CHECK(lrep::cands_fit(0) && lrep::cands_fit(65535) && !lrep::cands_fit(65536) && !lrep::cands_fit(~0ull));
  CHECK(LIN_MAX_CAND == 65535ull && LIN_PAD == 0xFFFFu);  // a position never equals the pad
  for (uint32_t m = 0; m <= 9; m++) CHECK(lin::size_ok(m, 0) == (m >= 1 && m <= 8));
  CHECK(!lin::size_ok(3, 1) && !lin::size_ok(8, 0x80000000u));
}

static void check_status() {
  // bit 0: lost under S = {}; bit 1: lost under S = cand; whatever lies above the two bits is ignored
  CHECK(lrep::status_of_lost(0) == REPAIR_HOLDS);
  CHECK(lrep::status_of_lost(2) == REPAIR_HOLDS);  // cannot occur (monotone), and reads as HOLDS as round 0's word 1 does
  CHECK(lrep::status_of_lost(1) == REPAIR_SEARCHED);
  CHECK(lrep::status_of_lost(3) == REPAIR_BEYOND);
  CHECK(lrep::status_of_lost(~0ull) == REPAIR_BEYOND && lrep::status_of_lost(~0ull << 2 | 1ull) == REPAIR_SEARCHED);
  CHECK(REPAIR_HOLDS == 0 && REPAIR_SEARCHED == 1 && REPAIR_BEYOND == 2);
}

// The chunk's stop rule words as the kernel makes them: an absent node starts with every column set, set h clears
// column h on the nodes it names; a candidate blamed under `blame` is emitted under blame & removed & lost.
static void check_chunk_words() {
  const uint32_t V = 131;  // odd: the words end with a padding word
  const std::vector<uint32_t> absent = {0, 5, 64, 65, 127, 129}, cand = {129, 5, 64, 0};  // 65 and 127 stay lost
  const std::vector<uint64_t> bits = repair::bitmap(absent.data(), absent.size(), V);
  std::vector<lin::Key> front;
  const uint32_t s0[1] = {0}, s1[2] = {1, 3}, s2[3] = {0, 1, 2};
  front.push_back(lin::key_empty());
  front.push_back(lin::key_pack(s0, 1));
  front.push_back(lin::key_pack(s1, 2));
  front.push_back(lin::key_pack(s2, 3));
  std::vector<uint64_t> removed(knock::dead_words(V), 0ull);
  for (uint32_t v = 0; v < V; v++)
    if ((bits[v >> 6] >> (v & 63u)) & 1ull) removed[v] = ~0ull;
  for (uint32_t s = 0; s < front.size(); s++)
    for (uint32_t j = 0; j < LIN_MAX_SIZE; j++) {
      const uint32_t p = lin::key_at(front[s], j);
      if (p < cand.size()) removed[cand[p]] &= ~(1ull << s);
    }
  const uint64_t tail = (1ull << front.size()) - 1ull;
  CHECK((removed[129] & tail) == 0x5ull);  // restored by sets 1 and 3
  CHECK((removed[5] & tail) == 0x3ull && (removed[64] & tail) == 0x7ull && (removed[0] & tail) == 0xBull);
  CHECK((removed[65] & tail) == tail && (removed[127] & tail) == tail && removed[1] == 0 && removed[128] == 0 && removed[V] == 0);
  // a child never names a position twice: the bits under which the candidate is restored are gone
  const uint64_t lost = 0xFull, blame_all = ~0ull;
  for (uint32_t k = 0; k < cand.size(); k++) {
    const uint64_t w = blame_all & removed[cand[k]] & lost;
    for (uint32_t s = 0; s < front.size(); s++) {
      bool named = false;
      for (uint32_t j = 0; j < LIN_MAX_SIZE; j++) named = named || lin::key_at(front[s], j) == k;
      CHECK((((w >> s) & 1ull) != 0) == !named);
      if ((w >> s) & 1ull) CHECK(lin::key_size(lin::key_insert(front[s], k)) == lin::key_size(front[s]) + 1);
    }
  }
}

int main() {
  check_image();
  check_region();
  check_limits();
  check_status();
  check_chunk_words();
  printf("lrepair_host_check OK\n");
  return 0;
}
