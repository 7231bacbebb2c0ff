// wit_host_check — drives the host side of the witness calls (nemo_amd/csrc/wit_host.h): the LDS image with the
// second word array and its tier from both sides of the bound, the option's value, the row limit, the kept need
// words' offsets against a recount and their limit from both sides, the hypothesis index arithmetic of the label form
// over every (list position, set) of small shapes, the distinct labels and the sets' rewrite as rows against the
// table the kernels probe, and a workgroup's region.  Meant for the host sanitizers; it calls nothing on a device:
//   g++ -std=c++17 -g -Wall -fsanitize=address,undefined -static-libasan -static-libubsan
//       tools/wit_host_check.cpp -o tools/wit_host_check
//   tools/wit_host_check
#include "../nemo_amd/csrc/wit_host.h"

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
  // the C3 shape (DESIGN.md §Surviving derivations): past knock_lds_max's bound, within one workgroup per CU
  const uint32_t V = 5002, E = 7600, L = 40;
  const uint32_t ko = knock::knock_lds_bytes(V, E, L), wt = wit::wit_lds_bytes(V, E, L);
  CHECK(ko <= KO_LDS_MAX && wt == ko + knock::ko_align(8u * V) && wt % 16 == 0 && wt > KO_LDS_MAX && wt <= WIT_LDS_MAX);
  CHECK(wit::lds_fits(V, E, L, wt) && !wit::lds_fits(V, E, L, wt - 1) && !wit::lds_fits(V, E, L, 0));
  CHECK(!wit::lds_fits(V, E, L, KO_LDS_MAX) && wit::lds_fits(V, E, L, WIT_LDS_DEFAULT) && wit::lds_fits(V, E, L, WIT_LDS_MAX));
  CHECK(!wit::lds_fits(65536, 10, 3, WIT_LDS_MAX) && !wit::lds_fits(100, 65536, 3, WIT_LDS_MAX) && !wit::lds_fits(3, 2, 4, WIT_LDS_MAX));
  CHECK(wit::lds_fits(0, 0, 0, 64) && wit::wit_lds_bytes(0, 0, 0) == 32);  // an empty graph: two row pointers' worth
  for (uint32_t v = 1; v < 70; v++) {  // the need words hold whole 16-byte pairs
    CHECK(wit::wit_lds_bytes(v, v, 2) - knock::knock_lds_bytes(v, v, 2) >= 8 * knock::dead_words(v));
  }
  CHECK(wit::lds_max_option(-1) == WIT_LDS_DEFAULT && wit::lds_max_option(0) == 0 && wit::lds_max_option(81920) == 81920);
  CHECK(wit::lds_max_option(1ll << 40) == WIT_LDS_MAX && wit::lds_max_option(WIT_LDS_MAX) == WIT_LDS_MAX);
  CHECK(WIT_LDS_MAX + 4096u == 160u * 1024u && WIT_LDS_DEFAULT == WIT_LDS_MAX);
}

static void check_limits() {
  CHECK(wit::rows_fit(0, ~0ull) && wit::rows_fit(~0ull, 0) && wit::rows_fit(1, KO_MAX_HYPS) && !wit::rows_fit(1, KO_MAX_HYPS + 1));
  CHECK(wit::rows_fit(2, KO_MAX_HYPS / 2) && !wit::rows_fit(2, KO_MAX_HYPS / 2 + 1) && !wit::rows_fit(1ull << 33, 1ull << 33));
  CHECK(wit::rows_fit(65536, 65535) && !wit::rows_fit(65536, 65536));
  // the kept need words: offsets against a recount
  const uint64_t v[5] = {7, 0, 64, 1, 5002};
  for (uint64_t ck : {1ull, 2ull, 3ull, 129ull}) {
    std::vector<uint64_t> moff;
    uint64_t total = 0, at = 0;
    CHECK(wit::need_offsets(v, 5, ck, &moff, &total));
    for (int i = 0; i < 5; i++) {
      CHECK(moff[i] == at && at % 2 == 0);
      at += ck * knock::dead_words(v[i]);
    }
    CHECK(total == at);
  }
  // ... and the limit from both sides: 2^33 words
  const uint64_t cap = WIT_MAX_NEED_BYTES / 8;
  uint64_t big[2] = {cap / 2 - 2, cap / 2 - 2}, total = 0;
  CHECK(wit::need_offsets(big, 2, 1, nullptr, &total) && total == cap - 4);
  big[1] = cap / 2 + 2;
  CHECK(wit::need_offsets(big, 2, 1, nullptr, &total) && total == cap);
  big[1] = cap / 2 + 3;
  CHECK(!wit::need_offsets(big, 2, 1, nullptr, &total) && total > cap);
  uint64_t huge[3] = {~0ull - 5, ~0ull - 5, 12};
  CHECK(!wit::need_offsets(huge, 3, ~0ull, nullptr, nullptr));  // saturates, does not wrap
  uint64_t one[1] = {1ull << 20};
  CHECK(wit::need_offsets(one, 1, 1ull << 13, nullptr, &total) && total == cap && !wit::need_offsets(one, 1, (1ull << 13) + 1, nullptr, nullptr));
}

static void check_hyps() {
  const uint64_t v[3] = {5, 130, 1};
  for (uint64_t n_sets : {1ull, 63ull, 64ull, 65ull, 129ull}) {
    const uint64_t ck = klabel::chunks(n_sets);
    std::vector<uint64_t> moff;
    CHECK(wit::need_offsets(v, 3, ck, &moff, nullptr));
    uint64_t h = 0;
    for (uint64_t pos = 0; pos < 3; pos++)
      for (uint64_t s = 0; s < n_sets; s++, h++) {
        CHECK(wit::hyp_index(pos, s, n_sets) == h);
        const wit::Hyp x = wit::hyp_at(h, n_sets);
        CHECK(x.pos == pos && x.set == s && x.chunk == s / 64 && x.bit == s % 64 && x.chunk < ck);
        const uint64_t w0 = wit::need_word0(x, moff.data(), v[pos]);
        CHECK(w0 == moff[pos] + x.chunk * knock::dead_words(v[pos]));
        CHECK(w0 + knock::dead_words(v[pos]) <= (pos < 2 ? moff[pos + 1] : moff[2] + ck * knock::dead_words(v[2])));
      }
  }
}

static void check_rows() {
  const uint32_t labels[9] = {40, 7, 7, 0xFFFFFFFEu, 0, 40, 3, 7, 0};
  const std::vector<uint32_t> dist = wit::distinct_labels(labels, 9);
  CHECK(dist.size() == 5 && dist[0] == 0 && dist[1] == 3 && dist[2] == 7 && dist[3] == 40 && dist[4] == 0xFFFFFFFEu);
  const std::vector<uint32_t> rows = wit::rows_of(labels, 9, dist);
  for (int k = 0; k < 9; k++) CHECK(rows[k] < dist.size() && dist[rows[k]] == labels[k]);
  CHECK(wit::distinct_labels(nullptr, 0).empty() && wit::rows_of(nullptr, 0, dist).empty());
  const uint64_t slots = klabel::table_slots(dist.size());
  CHECK(slots >= 2 * dist.size() && (slots & (slots - 1)) == 0);
  std::vector<uint32_t> key(slots, 0), val(slots, 0);
  wit::table_fill(key.data(), val.data(), slots, dist);
  for (size_t r = 0; r < dist.size(); r++) CHECK(wit::table_row(key.data(), val.data(), slots, dist[r]) == r);
  CHECK(wit::table_row(key.data(), val.data(), slots, 8) == 0xFFFFFFFFu && wit::table_row(key.data(), val.data(), slots, 41) == 0xFFFFFFFFu);
}

static void check_region() {
  CHECK(wit::glob_words(0) == 0 && wit::glob_words(1) == 4 && wit::glob_words(5002) == 2 * 5002 && wit::glob_words(5003) == 2 * 5004);
  CHECK(wit::region_words(0, 0, 5002, 0) == 0);              // the node-set form on the LDS tier keeps nothing in device memory
  CHECK(wit::region_words(wit::glob_words(7), 0, 7, 0) == 16);  // ... and on the global tier its two word arrays
  const uint64_t e = lcuts::list_entries(5, 100);            // 5 rows: 6 offsets and 100 nodes
  CHECK(e == 106 && wit::region_words(0, 5, 100, e) == 0 + 0 + wit::region_words(0, 5, 100, e + 9));
  CHECK(wit::region_words(0, 5, 100, 0) >= (e + 1) / 2 && wit::region_words(0, 5, 100, 0) % 2 == 0);
  CHECK(wit::region_words(16, 5, 100, 6) >= 16 + (e - 6 + 1) / 2 && wit::region_words(16, 5, 100, 6) % 2 == 0);
  CHECK(wit::image_bytes(10, 20, 3) == 4 * 20 + 12 * 10 + 4 * 3 + 8);
}

int main() {
  check_image();
  check_limits();
  check_hyps();
  check_rows();
  check_region();
  printf("wit_host_check OK\n");
  return 0;
}
