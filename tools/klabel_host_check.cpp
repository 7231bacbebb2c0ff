// klabel_host_check — drives the host side of nemo_knockout_labels (nemo_amd/csrc/klabel_host.h): every outcome of
// the validation (the label limit from set_off alone, no label read), the table sizes at 0, 1, 63, 64, 65 entries
// and at the limit, the table offsets, insert / probe in a table at its densest (chains, wrap-around), the cut of a
// call into work items for n in {1, 3, 70, 10000}, R in {1, 2, 512} and n_chunks in {1, 2, 47, 68151} with the
// property that every chunk of every graph lies in exactly one item of exactly one workgroup, and the grids.
// Meant for the host sanitizers; it calls nothing on a device:
//   g++ -std=c++17 -g -Wall -fsanitize=address,undefined -static-libasan -static-libubsan
//       tools/klabel_host_check.cpp -o tools/klabel_host_check
//   tools/klabel_host_check
#include "../nemo_amd/csrc/klabel_host.h"

#include <cstdio>
#include <cstdlib>

#define CHECK(x)                                            \
  do {                                                      \
    if (!(x)) {                                             \
      fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #x); \
      exit(1);                                              \
    }                                                       \
  } while (0)

static void check_validation() {
  uint64_t where = 99;
  CHECK(klabel::check_sets(nullptr, nullptr, 0, &where) == klabel::SET_OK);
  const uint64_t off[5] = {0, 2, 2, 5, 6};  // an empty set in the middle
  const uint32_t lab[6] = {7, 7, 0, 0xFFFFFFFEu, 3, 9};
  CHECK(klabel::check_sets(off, lab, 4, &where) == klabel::SET_OK);
  CHECK(klabel::check_sets(off, lab, 4, nullptr) == klabel::SET_OK);
  const uint64_t dec[4] = {0, 3, 2, 6};
  CHECK(klabel::check_sets(dec, lab, 3, &where) == klabel::SET_NONMONOTONE && where == 1);
  CHECK(klabel::check_offsets(dec, 1, &where) == klabel::SET_OK);  // the offence lies past the first set
  const uint32_t bad[6] = {7, 7, 0, 0xFFFFFFFFu, 3, 0xFFFFFFFFu};
  CHECK(klabel::check_sets(off, bad, 4, &where) == klabel::SET_LABEL && where == 3);
  CHECK(klabel::check_sets(off, bad, 2, &where) == klabel::SET_OK);  // sets 0 and 1 do not reach it
  const uint64_t shifted[3] = {3, 4, 6};  // the first set need not start at 0
  CHECK(klabel::check_sets(shifted, bad, 2, &where) == klabel::SET_LABEL && where == 3);
  // the label limit: read from set_off alone, with a label array far too short to hold the sets
  const uint64_t huge[3] = {0, 1, 0x100000000ull};
  const uint32_t one[1] = {5};
  CHECK(klabel::check_sets(huge, one, 2, &where) == klabel::SET_LIMIT);
  CHECK(klabel::check_sets(huge, nullptr, 2, &where) == klabel::SET_LIMIT);
  const uint64_t edge[2] = {5, 5 + 0xFFFFFFFFull};
  CHECK(klabel::check_offsets(edge, 1, &where) == klabel::SET_OK);  // 2^32 - 1 labels just fit
  const uint64_t over[2] = {5, 6 + 0xFFFFFFFFull};
  CHECK(klabel::check_offsets(over, 1, &where) == klabel::SET_LIMIT);
  // the set limit: a set index is a u32; empty sets name no label, so only this bounds them
  CHECK(klabel::sets_fit(0) && klabel::sets_fit(0xFFFFFFFFull) && !klabel::sets_fit(0x100000000ull) && !klabel::sets_fit(~0ull));
  CHECK(klabel::words_fit(1, 1ull << 34));  // ... which the word limit alone would let through
  // the word limit
  CHECK(klabel::chunks(0) == 0 && klabel::chunks(1) == 1 && klabel::chunks(64) == 1 && klabel::chunks(65) == 2 && klabel::chunks(129) == 3);
  CHECK(klabel::words_fit(0, 1ull << 40) && klabel::words_fit(1ull << 40, 0));
  CHECK(klabel::words_fit(1ull << 28, 64) && !klabel::words_fit(1ull << 28, 65));
  CHECK(klabel::words_fit(10000, 64ull * 26843) && !klabel::words_fit(10000, 64ull * 26844));  // 10000 x 26843 < 2^28 < 10000 x 26844
  CHECK(!klabel::words_fit(~0ull, ~0ull) && klabel::words_fit(1, 64ull << 28) && !klabel::words_fit(1, (64ull << 28) + 1));
}

static void check_tables() {
  CHECK(klabel::table_slots(0) == 16 && klabel::table_slots(1) == 16 && klabel::table_slots(8) == 16 && klabel::table_slots(9) == 32);
  CHECK(klabel::table_slots(63) == 128 && klabel::table_slots(64) == 128 && klabel::table_slots(65) == 256);
  CHECK(klabel::table_slots(1000) == 2048 && klabel::table_slots(1024) == 2048 && klabel::table_slots(1025) == 4096);
  CHECK(klabel::table_slots(KL_MAX_LABELS) == (1ull << 33));  // the limit: no overflow on the way
  for (uint64_t e = 0; e < 5000; e++) {
    const uint64_t s = klabel::table_slots(e);
    CHECK((s & (s - 1)) == 0 && s >= 2 * e && s >= KL_MIN_TABLE && (s == KL_MIN_TABLE || s / 2 < 2 * e));
  }
  // offsets: 130 sets, set s of s % 3 labels; three chunks and the union filter
  std::vector<uint64_t> off(131, 0);
  for (size_t s = 0; s < 130; s++) off[s + 1] = off[s] + s % 3;
  const std::vector<uint64_t> t = klabel::table_offsets(off.data(), 130);
  CHECK(t.size() == 5 && t[0] == 0);
  CHECK(t[1] - t[0] == klabel::table_slots(off[64]) && t[2] - t[1] == klabel::table_slots(off[128] - off[64]));
  CHECK(t[3] - t[2] == klabel::table_slots(off[130] - off[128]) && t[3] - t[2] == 16 && t[4] - t[3] == klabel::table_slots(off[130]));
  const std::vector<uint64_t> none = klabel::table_offsets(nullptr, 0);
  CHECK(none.size() == 2 && none[0] == 0 && none[1] == KL_MIN_TABLE);
  const uint64_t big[2] = {0, KL_MAX_LABELS};
  const std::vector<uint64_t> tb = klabel::table_offsets(big, 1);
  CHECK(tb.size() == 3 && tb[1] == (1ull << 33) && tb[2] == (1ull << 34));
  // a table at its densest: 1024 distinct labels in 2048 slots, each twice; chains and wrap-around
  const uint64_t slots = klabel::table_slots(1024);
  std::vector<uint32_t> key(slots, 0);
  std::vector<uint64_t> mask(slots, 0);
  for (uint32_t k = 0; k < 1024; k++) {
    klabel::insert(key.data(), mask.data(), slots, 3 * k + 1, 1ull << (k % 64));
    klabel::insert(key.data(), mask.data(), slots, 3 * k + 1, 1ull << ((k + 1) % 64));
  }
  size_t used = 0, wrapped = 0;
  for (uint64_t h = 0; h < slots; h++) used += key[h] != 0;
  CHECK(used == 1024);
  for (uint32_t k = 0; k < 1024; k++) {
    uint64_t bits = 0;
    CHECK(klabel::probe(key.data(), mask.data(), slots, 3 * k + 1, &bits));
    CHECK(bits == ((1ull << (k % 64)) | (1ull << ((k + 1) % 64))));
    CHECK(!klabel::probe(key.data(), mask.data(), slots, 3 * k + 2, &bits));
    CHECK(klabel::first_slot(3 * k + 1, slots) < slots);
  }
  // six labels that all hash to the last slot but one: the chain wraps to slot 0
  std::vector<uint32_t> k2(16, 0);
  uint32_t found = 0;
  for (uint32_t l = 0; found < 6; l++)
    if (klabel::first_slot(l, 16) == 14) {
      klabel::insert(k2.data(), nullptr, 16, l, 0);
      found++;
    }
  for (uint64_t h = 0; h < 4; h++) wrapped += k2[h] != 0;
  CHECK(k2[14] && k2[15] && wrapped == 4);
  CHECK(klabel::next_slot(15, 16) == 0 && klabel::next_slot(7, 16) == 8);
  CHECK(klabel::hash(0) == 0 && klabel::hash(1) == (0x9E3779B1u ^ (0x9E3779B1u >> 15)));
}

static void check_items() {
  for (uint64_t n : {1ull, 3ull, 70ull, 10000ull})
    for (uint64_t R : {1ull, 2ull, 512ull})
      for (uint64_t ck : {1ull, 2ull, 47ull, 68151ull}) {
        const klabel::Split s = klabel::split(n, ck, R);
        const uint64_t per = std::max<uint64_t>(1, (R + n - 1) / n);
        CHECK(s.parts == std::min(ck, per) && s.items == n * s.parts && s.items <= 0xFFFFFFFFull);
        // the ranges of a graph: contiguous, none empty, all of the chunks
        uint32_t at = 0;
        for (uint32_t p = 0; p < s.parts; p++) {
          const uint32_t lo = klabel::range_lo((uint32_t)ck, s.parts, p), hi = klabel::range_lo((uint32_t)ck, s.parts, p + 1);
          CHECK(lo == at && hi > lo);
          CHECK(hi - lo == ck / s.parts || hi - lo == ck / s.parts + 1);
          at = hi;
        }
        CHECK(at == ck);
        // the workgroups' blocks of items: contiguous, all of the items, sizes differing by one at most
        for (uint32_t cap : {0u, 1u, 3u}) {
          const uint32_t g = klabel::grid(s.items, R, cap);
          CHECK(g >= 1 && g <= s.items && g <= R && (!cap || g <= cap));
          uint64_t t = 0;
          for (uint32_t b = 0; b < g; b++) {
            const uint64_t lo = klabel::item_lo(s.items, g, b), hi = klabel::item_lo(s.items, g, b + 1);
            CHECK(lo == t && hi >= lo && (hi - lo == s.items / g || hi - lo == s.items / g + 1));
            t = hi;
          }
          CHECK(t == s.items);
        }
        // every chunk of every graph in exactly one item (a count per (graph, chunk) at the sizes that allow it)
        if (n * ck <= 1000000) {
          std::vector<uint8_t> seen(n * ck, 0);
          const uint32_t g = klabel::grid(s.items, R, 0);
          for (uint32_t b = 0; b < g; b++)
            for (uint64_t t = klabel::item_lo(s.items, g, b); t < klabel::item_lo(s.items, g, b + 1); t++) {
              const uint64_t ip = t / s.parts, part = t % s.parts;
              for (uint32_t c = klabel::range_lo((uint32_t)ck, s.parts, (uint32_t)part);
                   c < klabel::range_lo((uint32_t)ck, s.parts, (uint32_t)part + 1); c++)
                seen[ip * ck + c]++;
            }
          for (uint8_t x : seen) CHECK(x == 1);
        }
      }
  const klabel::Split none = klabel::split(0, 47, 512), nock = klabel::split(5, 0, 512);
  CHECK(none.items == 0 && none.parts == 0 && nock.items == 0);
  CHECK(klabel::split(2, 130, 3).parts == 2 && klabel::split(2, 130, 512).parts == 130 && klabel::split(2, 130, 0).parts == 1);
  CHECK(klabel::grid(0, 512, 0) == 1 && klabel::grid(10, 0, 0) == 1 && klabel::grid(260, 512, 0) == 260 && klabel::grid(260, 512, 3) == 3);
  // regions
  CHECK(klabel::region_words(0, 0) == 0 && klabel::region_words(5, 0) == 6 && klabel::region_words(5, 3) == 10);
  CHECK(klabel::region_grid(512, 0) == 512 && klabel::region_grid(0, 0) == 1);
  CHECK(klabel::region_grid(512, 1ull << 20) == 128 && klabel::region_grid(512, 1ull << 40) == 1);
}

int main() {
  check_validation();
  check_tables();
  check_items();
  printf("klabel_host_check OK\n");
  return 0;
}
