// cut_host_check — drives the host side of nemo_min_cuts (nemo_amd/csrc/cut_host.h): unrank(rank(x)) == x for
// every pair and triple of up to 200 positions, ranks monotone and dense in colex order, the ranks around
// 2^32 - 2 (2,953 live candidates give 4,287,437,076 triples, which just fits; 2,955 do not), the per-round limit
// from both sides, round 3's cut-pair test against brute force for every triple of 9 positions, every outcome of the candidate validation, the live list, the chunk and grid counts,
// and the sizes of a search over one graph (the global tier's resident bound, the bound of a round's hypotheses, round 1's words and pinned elements) at small values and at each bound's edge.
// Meant for the host sanitizers; it calls nothing on a device:
//   g++ -std=c++17 -g -Wall -fsanitize=address,undefined -static-libasan -static-libubsan
//       tools/cut_host_check.cpp -o tools/cut_host_check
//   tools/cut_host_check
#include "../nemo_amd/csrc/cut_host.h"

#include <cstdio>
#include <cstdlib>

#define CHECK(x)                                            \
  do {                                                      \
    if (!(x)) {                                             \
      fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #x); \
      exit(1);                                              \
    }                                                       \
  } while (0)

static void check_small() {
  for (uint32_t K = 0; K <= 200; K++) {
    CHECK(cuts::choose2(K) == (uint64_t)K * (K ? K - 1 : 0) / 2);
    CHECK(cuts::choose3(K) == (K < 3 ? 0 : (uint64_t)K * (K - 1) * (K - 2) / 6));
  }
  const uint32_t K = 200;
  uint64_t next = 0;  // colex order: b outermost for pairs, c outermost for triples; ranks count up by one
  for (uint32_t b = 1; b < K; b++)
    for (uint32_t a = 0; a < b; a++) {
      const uint64_t h = cuts::rank2(a, b);
      CHECK(h == next++);
      uint32_t x, y;
      cuts::unrank2(h, &x, &y);
      CHECK(x == a && y == b);
    }
  CHECK(next == cuts::choose2(K) && next == cuts::round_hyps(K, 2));
  next = 0;
  for (uint32_t c = 2; c < K; c++)
    for (uint32_t b = 1; b < c; b++)
      for (uint32_t a = 0; a < b; a++) {
        const uint64_t h = cuts::rank3(a, b, c);
        CHECK(h == next++);
        uint32_t x, y, z;
        cuts::unrank3(h, &x, &y, &z);
        CHECK(x == a && y == b && z == c);
      }
  CHECK(next == cuts::choose3(K) && next == cuts::round_hyps(K, 3));
}

static void check_large() {
  // triples of 2,953 live candidates: the last rank just fits
  CHECK(cuts::choose3(2953) == 4287437076ull && cuts::round_fits(2953, 3));
  CHECK(cuts::choose3(2954) == 4291795704ull && cuts::choose3(2954) == cuts::choose3(2953) + cuts::choose2(2953) && cuts::round_fits(2954, 3));
  CHECK(cuts::choose3(2955) > CUT_MAX_HYPS && !cuts::round_fits(2955, 3));
  CHECK(cuts::round_fits(92682, 2) && !cuts::round_fits(92683, 2));  // C(92682,2) = 4,294,930,221
  CHECK(cuts::round_fits(CUT_MAX_HYPS, 1) && !cuts::round_fits(CUT_MAX_HYPS + 1, 1));
  CHECK(cuts::choose3(2642245) < CUT_SAT && cuts::choose3(2642246) == CUT_SAT && !cuts::round_fits(1ull << 40, 3));
  CHECK(cuts::round_hyps(1ull << 33, 2) == CUT_SAT && !cuts::round_fits(1ull << 33, 2));
  uint32_t a, b, c;
  // the top of the triples of 2,953 and 2,954 positions, every rank of the last two values of c
  for (uint32_t K : {2953u, 2954u}) {
    const uint64_t hi = cuts::choose3(K);
    uint64_t prev = 0;
    for (uint64_t h = cuts::choose3(K - 2); h < hi; h++) {
      cuts::unrank3(h, &a, &b, &c);
      CHECK(a < b && b < c && c < K && cuts::rank3(a, b, c) == h);
      CHECK(h == cuts::choose3(K - 2) || h == prev + 1);
      prev = h;
    }
    cuts::unrank3(hi - 1, &a, &b, &c);
    CHECK(a == K - 3 && b == K - 2 && c == K - 1);
  }
  // around every value of c up to 2,954, and of b up to 92,682: the first and last rank of a block and its neighbours
  for (uint32_t z = 3; z <= 2954; z++)
    for (int d = -2; d <= 2; d++) {
      const uint64_t h = cuts::choose3(z) + (uint64_t)(int64_t)d;
      if (h > CUT_MAX_HYPS) continue;
      cuts::unrank3(h, &a, &b, &c);
      CHECK(a < b && b < c && cuts::rank3(a, b, c) == h && c == (d < 0 ? z - 1 : z));
    }
  for (uint32_t y = 2; y <= 92682; y++)
    for (int d = -1; d <= 1; d++) {  // (the block of b = 2 holds two ranks)
      const uint64_t h = cuts::choose2(y) + (uint64_t)(int64_t)d;
      if (h > CUT_MAX_HYPS) continue;
      cuts::unrank2(h, &a, &b);
      CHECK(a < b && cuts::rank2(a, b) == h && b == (d < 0 ? y - 1 : y));
    }
  for (uint64_t h = CUT_MAX_HYPS - 70000; h <= CUT_MAX_HYPS; h++) {  // the last pairs and triples a round may hold
    cuts::unrank2(h, &a, &b);
    CHECK(a < b && cuts::rank2(a, b) == h);
    cuts::unrank3(h, &a, &b, &c);
    CHECK(a < b && b < c && cuts::rank3(a, b, c) == h);
  }
  cuts::unrank2(0, &a, &b);
  CHECK(a == 0 && b == 1);
  cuts::unrank3(0, &a, &b, &c);
  CHECK(a == 0 && b == 1 && c == 2);
}

// has_cut_pair against a brute-force membership test: every triple of K = 9 positions, under no cut pair, every
// single one of the 36, a few mixed sets and all of them; then a pair whose rank lies in the second word
static void check_cut_pair() {
  const uint32_t K = 9;
  const uint64_t n2 = cuts::choose2(K);
  bool cut[K][K];
  auto run = [&](const std::vector<uint64_t> &ranks) {
    uint64_t words[2] = {0, 0};  // K = 9's 36 pairs lie in the first
    for (uint32_t y = 0; y < K; y++)
      for (uint32_t x = 0; x < K; x++) cut[x][y] = false;
    for (uint64_t r : ranks) {
      uint32_t x, y;
      cuts::unrank2(r, &x, &y);
      cut[x][y] = true;
      words[r >> 6] |= 1ull << (r & 63u);
    }
    for (uint32_t c = 2; c < K; c++)
      for (uint32_t b = 1; b < c; b++)
        for (uint32_t a = 0; a < b; a++) {
          const cuts::Pos p = cuts::unrank<3>(cuts::rank3(a, b, c));
          CHECK(p.a == a && p.b == b && p.c == c);
          CHECK(cuts::has_cut_pair(words, p) == (cut[a][b] || cut[a][c] || cut[b][c]));
        }
  };
  run({});
  for (uint64_t r = 0; r < n2; r++) run({r});
  run({0, 7, 35});
  run({3, 4, 5, 20, 21, 34});
  std::vector<uint64_t> all;
  for (uint64_t r = 0; r < n2; r++) all.push_back(r);
  run(all);
  // positions past 11 have pair ranks past 64: the second word.  Triples of {0, 1, 12, 13} with the pair (12, 13) a cut
  uint64_t words[2] = {0, 0};
  const uint64_t r = cuts::rank2(12, 13);
  CHECK(r >= 64 && r < 128);
  words[r >> 6] |= 1ull << (r & 63u);
  CHECK(cuts::has_cut_pair(words, cuts::Pos{0, 12, 13}) && cuts::has_cut_pair(words, cuts::Pos{1, 12, 13}));
  CHECK(!cuts::has_cut_pair(words, cuts::Pos{0, 1, 12}) && !cuts::has_cut_pair(words, cuts::Pos{0, 1, 13}));
}

static void check_cands() {
  size_t where = 99;
  CHECK(cuts::check_cands(nullptr, 0, 10, &where) == cuts::CAND_OK);
  const uint32_t ok[5] = {4, 0, 9, 2, 7};
  CHECK(cuts::check_cands(ok, 5, 10, &where) == cuts::CAND_OK);
  CHECK(cuts::check_cands(ok, 5, 10, nullptr) == cuts::CAND_OK);
  CHECK(cuts::check_cands(ok, 5, 9, &where) == cuts::CAND_RANGE && where == 2);  // node 9 of a 9-node graph
  const uint32_t range2[4] = {1, 10, 11, 1};
  CHECK(cuts::check_cands(range2, 4, 10, &where) == cuts::CAND_RANGE && where == 1);  // the range comes first
  const uint32_t dup[6] = {5, 3, 8, 3, 5, 3};
  CHECK(cuts::check_cands(dup, 6, 10, &where) == cuts::CAND_DUP && where == 3);  // the first second occurrence
  CHECK(cuts::check_cands(dup, 6, 10, nullptr) == cuts::CAND_DUP);
  CHECK(cuts::check_cands(dup, 3, 10, &where) == cuts::CAND_OK);
  const uint32_t many[5] = {0, 1, 2, 1, 0};  // more candidates than nodes
  CHECK(cuts::check_cands(many, 5, 3, &where) == cuts::CAND_DUP && where == 3);
  CHECK(cuts::check_cands(many, 1, 0, &where) == cuts::CAND_RANGE && where == 0);  // a graph without nodes
}

static void check_live_and_grid() {
  uint64_t w[3] = {0, 0, 0};
  CHECK(cuts::live_list(w, 0).empty());
  CHECK(cuts::live_list(w, 130).size() == 130);
  w[0] = 1ull | (1ull << 63), w[1] = 1ull << 1, w[2] = 1ull << 1;  // candidates 0, 63, 65 and 129 are cuts alone
  const std::vector<uint32_t> live = cuts::live_list(w, 130);
  CHECK(live.size() == 126 && live[0] == 1 && live[61] == 62 && live[62] == 64 && live[63] == 66 && live.back() == 128);
  for (size_t i = 1; i < live.size(); i++) CHECK(live[i] > live[i - 1]);
  w[0] = w[1] = ~0ull;
  CHECK(cuts::live_list(w, 128).empty());
  CHECK(cuts::chunks(0) == 0 && cuts::chunks(1) == 1 && cuts::chunks(64) == 1 && cuts::chunks(65) == 2);
  CHECK(cuts::chunks(cuts::choose2(128)) == 127 && cuts::chunks(cuts::choose3(64)) == 651);
  CHECK(cuts::chunks(CUT_MAX_HYPS) == (1ull << 26));
  CHECK(cuts::grid(651, 512, 0) == 512 && cuts::grid(127, 512, 0) == 127 && cuts::grid(651, 512, 3) == 3);
  CHECK(cuts::grid(2, 512, 3) == 2 && cuts::grid(0, 512, 0) == 1 && cuts::grid(10, 0, 0) == 1);
}

// the sizes node_search takes: small values and each bound's edge
static void check_search_sizes() {
  // 256 CUs: two workgroups each until 512 of them would keep more than CUT_DEAD_BYTES, that is past 2^18 dead words
  CHECK(cuts::glob_resident(256, 0) == 512 && cuts::glob_resident(256, 2) == 512 && cuts::glob_resident(1, 2) == 2);
  CHECK(cuts::glob_resident(256, 1ull << 18) == 512 && cuts::glob_resident(256, (1ull << 18) + 2) == 511);
  CHECK(cuts::glob_resident(256, 1ull << 19) == 256 && cuts::glob_resident(256, 1ull << 26) == 2);
  CHECK(cuts::glob_resident(256, 1ull << 27) == 1 && cuts::glob_resident(256, (1ull << 27) + 2) == 1);  // never none
  CHECK(cuts::glob_resident(0, 2) == 1 && cuts::glob_resident(256, ~0ull >> 3) == 1);
  CHECK(cuts::most_hyps(0, 1) == 1 && cuts::most_hyps(0, 3) == 1 && cuts::most_hyps(1, 3) == 1 && cuts::most_hyps(2, 3) == 2);
  CHECK(cuts::most_hyps(5, 1) == 5 && cuts::most_hyps(5, 2) == 10 && cuts::most_hyps(5, 3) == 10 && cuts::most_hyps(10, 3) == 120);
  CHECK(cuts::most_hyps(12, 2) == 66 && cuts::most_hyps(3, 2) == 3 && cuts::most_hyps(3, 3) == 3);
  // a K at which round_hyps passes CUT_MAX_HYPS: the bound stays there
  CHECK(cuts::most_hyps(2954, 3) == 4291795704ull && cuts::most_hyps(2955, 3) == CUT_MAX_HYPS && cuts::most_hyps(2955, 2) == cuts::choose2(2955));
  CHECK(cuts::most_hyps(92682, 2) == 4294930221ull && cuts::most_hyps(92683, 2) == CUT_MAX_HYPS && cuts::most_hyps(92683, 1) == 92683);
  CHECK(cuts::most_hyps(2642246, 3) == CUT_MAX_HYPS);  // choose3 saturates
  CHECK(cuts::first_words(0, false) == 0 && cuts::first_words(0, true) == 1 && cuts::first_words(64, false) == 1);
  CHECK(cuts::first_words(64, true) == 2 && cuts::first_words(65, false) == 2 && cuts::first_words(65, true) == 3);
  CHECK(cuts::first_pinned(0, false) == 8 && cuts::first_pinned(0, true) == 10);
  CHECK(cuts::first_pinned(65, false) == 2 * 2 + 65 + 8 && cuts::first_pinned(65, true) == 2 * 3 + 65 + 8);
}

int main() {
  check_search_sizes();
  check_small();
  check_large();
  check_cut_pair();
  check_cands();
  check_live_and_grid();
  printf("cut_host_check OK\n");
  return 0;
}
