// gcut_host_check — drives the host side of nemo_min_group_cuts (nemo_amd/csrc/gcut_host.h): every outcome of the
// group check (a decreasing offset, UINT32_MAX with its group and position, the label total from the offsets alone,
// no label read past a failed offset check, a group past 2^24 labels), the u32 offsets from a first offset that is
// not 0, the count of the distinct labels with duplicates inside and across groups, the table with the kernels' own
// insert order (the first to take a slot hands out the row) and the groups rewritten as rows, and the sizes of a hit
// list and a region: D + 1 + V entries however many groups share a label, at most 2^32 - 1.  Meant for the host
// sanitizers; it calls nothing on a device:
//   g++ -std=c++17 -g -Wall -fsanitize=address,undefined -static-libasan -static-libubsan
//       tools/gcut_host_check.cpp -o tools/gcut_host_check
//   tools/gcut_host_check
#include "../nemo_amd/csrc/gcut_host.h"

#include <cstdio>
#include <cstdlib>

#define CHECK(x)                                            \
  do {                                                      \
    if (!(x)) {                                             \
      fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #x); \
      exit(1);                                              \
    }                                                       \
  } while (0)

static void check_groups() {
  uint64_t group = 99, where = 99;
  CHECK(gcuts::check_groups(nullptr, nullptr, 0, &group, &where) == gcuts::GROUP_OK);
  CHECK(gcuts::named(nullptr, 0) == 0 && gcuts::distinct_labels(nullptr, nullptr, 0) == 0);
  // {10}, {}, {11, 11}, {10, 12}: an empty group and a label named twice are legal
  const uint64_t off[5] = {0, 1, 1, 3, 5};
  const uint32_t lab[5] = {10, 11, 11, 10, 12};
  CHECK(gcuts::check_groups(off, lab, 4, &group, &where) == gcuts::GROUP_OK);
  CHECK(gcuts::check_groups(off, lab, 4, nullptr, nullptr) == gcuts::GROUP_OK);
  CHECK(gcuts::named(off, 4) == 5 && gcuts::distinct_labels(off, lab, 4) == 3);
  CHECK(gcuts::distinct_labels(off, lab, 3) == 2 && gcuts::distinct_labels(off, lab, 2) == 1);
  // only empty groups: a null label array is never read
  const uint64_t flat[4] = {7, 7, 7, 7};
  CHECK(gcuts::check_groups(flat, nullptr, 3, &group, &where) == gcuts::GROUP_OK);
  CHECK(gcuts::named(flat, 3) == 0 && gcuts::distinct_labels(flat, nullptr, 3) == 0);
  // a decreasing offset: the first decreasing group, and no label is read (the array is null)
  const uint64_t dec[5] = {0, 2, 1, 3, 2};
  CHECK(gcuts::check_groups(dec, nullptr, 4, &group, &where) == gcuts::GROUP_NONMONOTONE && group == 1);
  // the forbidden label: its group and its position in group_labels; the first one wins
  const uint32_t bad[5] = {10, 11, 0xFFFFFFFFu, 0xFFFFFFFFu, 12};
  group = where = 99;
  CHECK(gcuts::check_groups(off, bad, 4, &group, &where) == gcuts::GROUP_LABEL && group == 2 && where == 2);
  CHECK(gcuts::check_groups(off, bad, 2, &group, &where) == gcuts::GROUP_OK);  // the groups before it
  const uint32_t top[1] = {0xFFFFFFFEu};  // the largest legal label
  CHECK(gcuts::check_groups(off, top, 1, &group, &where) == gcuts::GROUP_OK);
  // a first offset that is not 0: the labels are read from it on, the u32 offsets start at 0
  const uint64_t late[3] = {3, 4, 5};
  CHECK(gcuts::check_groups(late, bad, 2, &group, &where) == gcuts::GROUP_LABEL && group == 0 && where == 3);
  CHECK(gcuts::check_groups(late + 1, bad, 1, &group, &where) == gcuts::GROUP_OK);
  CHECK(gcuts::named(late, 2) == 2 && gcuts::distinct_labels(late, lab, 2) == 2);
  CHECK(gcuts::offsets32(late, 2) == (std::vector<uint32_t>{0, 1, 2}));
  CHECK(gcuts::offsets32(off, 4) == (std::vector<uint32_t>{0, 1, 1, 3, 5}));
  CHECK(gcuts::offsets32(nullptr, 0) == std::vector<uint32_t>{0});
  // the label total, from the offsets alone (the label array is null): 2^32 - 1 is the last that fits
  const uint64_t big[3] = {5, 5 + 0x7FFFFFFFull, 5 + 0xFFFFFFFFull};
  CHECK(klabel::check_offsets(big, 2, &group) == klabel::SET_OK && gcuts::named(big, 2) == GC_MAX_LABELS);
  const uint64_t over[3] = {5, 5 + 0x7FFFFFFFull, 6 + 0xFFFFFFFFull};
  CHECK(gcuts::check_groups(over, nullptr, 2, &group, &where) == gcuts::GROUP_LIMIT);
  CHECK(gcuts::offsets32(big, 2) == (std::vector<uint32_t>{0, 0x7FFFFFFFu, 0xFFFFFFFFu}));
  // ... and a group's own size, GC_MAX_GROUP at the most: big's groups are too long for the whole check
  CHECK(gcuts::check_groups(big, nullptr, 2, &group, &where) == gcuts::GROUP_SIZE && group == 0);
  const uint64_t edge[4] = {9, 9 + GC_MAX_GROUP, 9 + GC_MAX_GROUP, 10 + 2 * GC_MAX_GROUP};
  CHECK(klabel::check_offsets(edge, 3, &group) == klabel::SET_OK);
  CHECK(gcuts::check_groups(edge, nullptr, 3, &group, &where) == gcuts::GROUP_SIZE && group == 2);
  std::vector<uint32_t> full(GC_MAX_GROUP + 9, 5u);
  CHECK(gcuts::check_groups(edge, full.data(), 2, &group, &where) == gcuts::GROUP_OK);  // 2^24 itself fits
  // the hit list's entries are u32 indices
  CHECK(gcuts::list_fits(0, 0) && gcuts::list_fits(0xFFFFFFFEull, 0) && !gcuts::list_fits(0xFFFFFFFFull, 0));
  CHECK(gcuts::list_fits(0x7FFFFFFFull, 0x7FFFFFFFull) && !gcuts::list_fits(0x80000000ull, 0x7FFFFFFFull));
}

// The table and the rewrite as k_gc_table / k_gc_rows make them, one entry at a time: the first entry of a label
// takes the slot and the next row; every entry then becomes its label's row.  Nested groups that share most labels:
// the rows number the distinct labels, however many groups name each.
static void check_rows() {
  CHECK(gcuts::table_slots(0) == 16 && gcuts::table_slots(8) == 16 && gcuts::table_slots(9) == 32 && gcuts::table_slots(129) == 512);
  for (uint32_t L : {1u, 40u, 600u}) {
    // group k = labels 0 .. k (as crash groups nest), label l spelt as 0xFFFFFFFE - 5 l; the last group twice over
    std::vector<uint64_t> off(1, 0);
    std::vector<uint32_t> lab;
    for (uint32_t k = 0; k < L; k++) {
      for (uint32_t l = 0; l <= k; l++) lab.push_back(0xFFFFFFFEu - 5u * l);
      if (k + 1 == L)
        for (uint32_t l = 0; l <= k; l++) lab.push_back(0xFFFFFFFEu - 5u * l);
      off.push_back(lab.size());
    }
    uint64_t group = 0, where = 0;
    CHECK(gcuts::check_groups(off.data(), lab.data(), L, &group, &where) == gcuts::GROUP_OK);
    const uint64_t T = gcuts::named(off.data(), L), D = gcuts::distinct_labels(off.data(), lab.data(), L);
    CHECK(T == (uint64_t)L * (L + 1) / 2 + L && D == L);
    const uint64_t slots = gcuts::table_slots(D);
    CHECK(slots >= 2 * D);
    std::vector<uint32_t> key(slots, 0), val(slots, LC_NONE), rows(lab);
    uint32_t n_rows = 0;
    for (uint64_t e = 0; e < T; e++) {
      uint64_t h = klabel::first_slot(rows[e], slots);
      while (key[h] && key[h] != rows[e] + 1u) h = klabel::next_slot(h, slots);
      if (!key[h]) key[h] = rows[e] + 1u, val[h] = n_rows++;
    }
    CHECK(n_rows == D);
    for (uint64_t e = 0; e < T; e++) {
      uint64_t h = klabel::first_slot(rows[e], slots);
      while (key[h] != rows[e] + 1u) h = klabel::next_slot(h, slots);
      rows[e] = val[h];
    }
    std::vector<uint32_t> label_of(D, LC_NONE);
    for (uint64_t e = 0; e < T; e++) {
      CHECK(rows[e] < D && (label_of[rows[e]] == LC_NONE || label_of[rows[e]] == lab[e]));  // one label per row
      label_of[rows[e]] = lab[e];
    }
    CHECK(!klabel::probe(key.data(), nullptr, slots, 0xFFFFFFFEu - 1u, nullptr));  // a label no group names
    // the hit list does not grow with the memberships: D + 1 + V entries against T of them
    CHECK(gcuts::list_entries(D, 300) == D + 301);
  }
}

static void check_sizes() {
  // lcut_host.h's layout with a row per distinct label: D + 1 offsets and at most V nodes; what the head does not
  // hold, in u64, whole 16-byte pairs, behind the dead words
  CHECK(gcuts::list_entries(0, 0) == 1 && gcuts::list_entries(12, 300) == 313 && gcuts::list_entries(600, 40) == 641);
  CHECK(gcuts::region_words(0, 313, 313) == 0 && gcuts::region_words(0, 313, 1000) == 0);
  CHECK(gcuts::region_words(0, 313, 312) == 2 && gcuts::region_words(0, 313, 309) == 2 && gcuts::region_words(0, 313, 308) == 4);
  CHECK(gcuts::region_words(6, 313, 0) == 6 + 158 && gcuts::region_words(5, 0, 0) == 6);
  for (uint64_t d = 0; d < 100; d += 9)
    for (uint64_t V = 0; V < 100; V += 11)
      for (uint64_t head = 0; head < 250; head += 7) {
        const uint64_t e = gcuts::list_entries(d, V), w = gcuts::region_words(0, e, head);
        CHECK(w % 2 == 0 && 2 * w >= (e > head ? e - head : 0) && w <= (e + 1) / 2 + 2);
        CHECK(gcuts::region_words(10, e, head) == w + 10);
      }
  // the rounds are lcut_host.h's: the min_runs rule, the limits, the live list (an empty group is never hit)
  uint32_t q = 0;
  CHECK(lcuts::min_runs(3, 0, &q) && q == 3 && !lcuts::min_runs(3, 4, &q));
  CHECK(lcuts::round_check(70, 22155, 2) == lcuts::ROUND_OK && lcuts::round_check(70, 22156, 2) == lcuts::ROUND_WORDS);
  CHECK(lcuts::round_check(1, 92683, 2) == lcuts::ROUND_HYPS);
  const uint64_t cut = 0x1ull, hit = 0xBull;  // candidate 0 a cut alone, 2 never hit (an empty group), 1 and 3 live
  CHECK(lcuts::live_list(&cut, &hit, 4) == (std::vector<uint32_t>{1, 3}));
}

int main() {
  check_groups();
  check_rows();
  check_sizes();
  printf("gcut_host_check OK\n");
  return 0;
}
