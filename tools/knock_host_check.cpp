// knock_host_check — drives the host side of the knock-out calls (nemo_amd/csrc/knock_host.h): the chunk
// table over edge sizes (0, 1, 63, 64, 65 and 129 hypotheses, a graph with zero leaves between two others),
// every chunk's hypotheses and dead-word region against a recount, the two limits from both sides, the LDS
// tier, and the validation of explicit sets (a non-monotone set_off, a node out of range).  Meant for the
// host sanitizers; it calls nothing on a device:
//   g++ -std=c++17 -g -Wall -fsanitize=address,undefined -static-libasan -static-libubsan
//       tools/knock_host_check.cpp -o tools/knock_host_check
//   tools/knock_host_check
#include "../nemo_amd/csrc/knock_host.h"

#include <cstdio>
#include <cstdlib>

#define CHECK(x)                                            \
  do {                                                      \
    if (!(x)) {                                             \
      fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #x); \
      exit(1);                                              \
    }                                                       \
  } while (0)

using knock::Chunk;
using knock::GraphIn;
using knock::Table;

// every property of a table, from the inputs alone
static void check_table(const std::vector<GraphIn> &in, bool masks) {
  const Table t = knock::chunk_table(in.data(), in.size(), masks);
  CHECK(t.tot.limit == knock::LIMIT_OK);
  CHECK(t.first.size() == in.size() && t.count.size() == in.size());
  uint64_t hyp = 0, off = 0;
  size_t k = 0;
  for (size_t i = 0; i < in.size(); i++) {
    CHECK(t.first[i] == hyp && t.count[i] == in[i].n);
    for (uint64_t done = 0; done < in[i].n; k++) {
      CHECK(k < t.chunk.size());
      const Chunk &c = t.chunk[k];
      const uint64_t want = in[i].n - done < KO_CHUNK ? in[i].n - done : KO_CHUNK;
      CHECK(c.graph == in[i].graph && c.slot == i && c.first == hyp + done && c.n == want && c.n >= 1 && c.n <= KO_CHUNK);
      CHECK(c.tier == (in[i].lds ? KO_TIER_LDS : KO_TIER_GLOB));
      if (masks || !in[i].lds) {
        CHECK(c.moff == off && c.moff % 2 == 0);  // 16-byte aligned regions, back to back
        off += knock::dead_words(in[i].V);
        CHECK(knock::dead_words(in[i].V) >= in[i].V && knock::dead_words(in[i].V) <= in[i].V + 1);
      } else {
        CHECK(c.moff == KO_NO_OFF);
      }
      done += want;
    }
    hyp += in[i].n;
  }
  CHECK(k == t.chunk.size() && t.tot.n_chunks == k && t.tot.n_hyp == hyp && t.tot.dead == off);
  // the two tiers' lists: every chunk once, LDS first, each in table order
  CHECK(t.sel.size() == k && t.n_lds + t.n_glob == k);
  for (size_t j = 0; j < t.sel.size(); j++) {
    CHECK(t.sel[j] < k);
    CHECK(t.chunk[t.sel[j]].tier == (j < t.n_lds ? KO_TIER_LDS : KO_TIER_GLOB));
    if (j && j != t.n_lds) CHECK(t.sel[j - 1] < t.sel[j]);
  }
  // hypothesis -> chunk
  for (uint64_t h = 0; h < hyp; h++) {
    const Chunk &c = t.chunk[knock::chunk_of(t, h)];
    CHECK(c.first <= h && h < (uint64_t)c.first + c.n);
  }
}

static void check_tables() {
  const uint64_t sizes[] = {0, 1, 63, 64, 65, 129};
  for (int masks = 0; masks < 2; masks++) {
    check_table({}, masks);
    for (uint64_t n : sizes)
      for (int lds = 0; lds < 2; lds++) {
        check_table({{7, 10, n, lds != 0}}, masks);
        check_table({{7, 11, n, lds != 0}, {9, 0, 0, true}, {3, 4, 65, lds == 0}}, masks);
      }
    // a graph with zero leaves between two others, odd and even node counts, mixed tiers, a duplicate graph
    check_table({{1, 5, 63, true}, {3, 9, 0, true}, {5, 70000, 65, false}, {1, 5, 63, true}, {7, 1, 1, false}}, masks);
  }
  const Table e = knock::chunk_table(nullptr, 0, true);
  CHECK(e.chunk.empty() && e.first.empty() && e.tot.n_hyp == 0 && e.tot.limit == knock::LIMIT_OK);
}

static void check_limits() {
  // hypotheses: 2^32 - 2 is fine, one more is not; from one graph and summed over several
  GraphIn one{1, 8, KO_MAX_HYPS, true};
  CHECK(knock::totals(&one, 1, false).limit == knock::LIMIT_OK);
  CHECK(knock::totals(&one, 1, false).n_chunks == (KO_MAX_HYPS + 63) / 64);
  one.n = KO_MAX_HYPS + 1;
  CHECK(knock::totals(&one, 1, false).limit == knock::LIMIT_HYPS);
  GraphIn two[2] = {{1, 8, KO_MAX_HYPS - 5, true}, {3, 8, 5, true}};
  CHECK(knock::totals(two, 2, false).limit == knock::LIMIT_OK);
  two[1].n = 6;
  CHECK(knock::totals(two, 2, false).limit == knock::LIMIT_HYPS);
  two[0].n = ~0ull;  // the sum saturates, it does not wrap
  CHECK(knock::totals(two, 2, false).limit == knock::LIMIT_HYPS);
  CHECK(knock::chunk_table(two, 2, false).chunk.empty());  // a table past a limit is not built
  // dead words: 2^36 bytes = 2^33 words.  V = 2^20 nodes: 2^13 chunks are fine, one more is not
  const uint64_t V = 1ull << 20, ck = (KO_MAX_DEAD_BYTES / 8) / V;
  GraphIn m{1, V, 64 * ck, true};
  CHECK(knock::totals(&m, 1, true).limit == knock::LIMIT_OK && knock::totals(&m, 1, true).dead == KO_MAX_DEAD_BYTES / 8);
  m.n = 64 * ck + 1;
  CHECK(knock::totals(&m, 1, true).limit == knock::LIMIT_DEAD);
  CHECK(knock::totals(&m, 1, false).limit == knock::LIMIT_OK);  // an LDS graph without masks keeps no words
  m.lds = false;
  CHECK(knock::totals(&m, 1, false).limit == knock::LIMIT_DEAD);  // the global tier sweeps in them
  m.n = 64 * ck;
  CHECK(knock::totals(&m, 1, false).limit == knock::LIMIT_OK);
  GraphIn huge{1, 0xFFFFFFFFull, KO_MAX_HYPS, false};  // no 64-bit overflow in chunks x words
  CHECK(knock::totals(&huge, 1, true).limit == knock::LIMIT_DEAD);
}

static void check_tier() {
  CHECK(knock::knock_lds_bytes(0, 0, 0) == 32);  // row pointer and level offset of an empty graph
  CHECK(knock::knock_lds_bytes(1, 0, 1) == 16 + 16 + 0 + 16 + 16 + 16);
  CHECK(knock::knock_lds_bytes(64, 10, 3) == 512 + 144 + 32 + 128 + 16 + 16);
  CHECK(knock::knock_lds_bytes(65, 10, 3) == 528 + 144 + 32 + 144 + 16 + 16);
  CHECK(knock::lds_fits(100, 300, 7, KO_LDS_MAX) && !knock::lds_fits(100, 300, 7, 0));
  CHECK(!knock::lds_fits(65536, 10, 3, ~0u) && !knock::lds_fits(100, 65536, 3, ~0u) && knock::lds_fits(65535, 65535, 9, ~0u));
  for (uint32_t V = 1; V < 9000; V += 37)  // the cap is a cap: the image of a fitting graph is within it
    for (uint32_t E = 0; E < 30000; E += 4999) {
      const uint32_t b = knock::knock_lds_bytes(V, E, V);
      CHECK(b % 16 == 0 && b >= 12 * V + 2 * E);
      CHECK(knock::lds_fits(V, E, V, KO_LDS_MAX) == (b <= KO_LDS_MAX));
      CHECK(knock::lds_fits(V, E, V, b) && !knock::lds_fits(V, E, V, b - 1));
    }
}

static void check_set_validation() {
  const uint32_t nodes[] = {0, 3, 3, 9, 2, 9};
  uint64_t where = 99;
  const uint64_t ok[] = {0, 2, 2, 5, 6};  // an empty set in the middle, a node named twice
  CHECK(knock::check_sets(ok, nodes, 4, 10, &where) == knock::SET_OK);
  CHECK(knock::check_sets(ok, nodes, 0, 0, &where) == knock::SET_OK);  // no set: nothing is read
  CHECK(knock::check_sets(nullptr, nullptr, 0, 10, nullptr) == knock::SET_OK);
  CHECK(knock::check_sets(ok, nodes, 4, 9, &where) == knock::SET_NODE && where == 3);  // node 9 of a 9-node graph
  const uint64_t shifted[] = {1, 3, 6};  // offsets need not start at 0; the nodes before the first are not read
  CHECK(knock::check_sets(shifted, nodes, 2, 10, &where) == knock::SET_OK);
  CHECK(knock::check_sets(shifted, nodes, 2, 4, &where) == knock::SET_NODE && where == 3);
  const uint64_t down[] = {0, 4, 3, 6};
  CHECK(knock::check_sets(down, nodes, 3, 10, &where) == knock::SET_NONMONOTONE && where == 1);
  const uint64_t down_last[] = {0, 2, 1};
  CHECK(knock::check_sets(down_last, nodes, 2, 10, &where) == knock::SET_NONMONOTONE && where == 1);
  const uint64_t far[] = {0, KO_MAX_SET_NODES + 1};  // refused before a node is read
  CHECK(knock::check_sets(far, nodes, 1, 10, &where) == knock::SET_LIMIT);
  const uint64_t empty_sets[] = {5, 5, 5, 5};
  CHECK(knock::check_sets(empty_sets, nullptr, 3, 0, &where) == knock::SET_OK);  // empty sets on an empty graph
}

int main() {
  check_tables();
  check_limits();
  check_tier();
  check_set_validation();
  printf("knock_host_check OK\n");
  return 0;
}
