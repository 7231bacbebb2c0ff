// nearest_host_check — drives the host side of nemo_nearest_runs (nemo_amd/csrc/nearest_host.h): the
// distinct runs of the two lists and the row of every list position against a brute-force recount, the
// words of a row, the two limits, and the tile / split-K grid; then builds the bit rows the way
// k_near_bits does and walks k_near_isect's tiles, slabs and K ranges on the host, every index inside
// the matrix it belongs to, against set arithmetic.  Meant for the host sanitizers; it calls nothing
// on a device:
//   g++ -std=c++17 -g -Wall -fsanitize=address,undefined -static-libasan -static-libubsan
//       tools/nearest_host_check.cpp -o build/nearest_host_check
//   build/nearest_host_check
#include "../nemo_amd/csrc/nearest_host.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <set>

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

static void check_words() {
  CHECK(nearest::words_per_row(0) == 2 && nearest::words_per_row(63) == 2 && nearest::words_per_row(127) == 2);
  CHECK(nearest::words_per_row(128) == 4 && nearest::words_per_row(255) == 4 && nearest::words_per_row(256) == 6);
  CHECK(nearest::words_per_row(3900) == 62 && nearest::words_per_row(599999) == 9376);
  CHECK(nearest::words_per_row(0xFFFFFFFFu) == (1ull << 26));  // no 32-bit overflow at the largest label
  for (int k = 0; k < 2000; k++) {
    const uint32_t lmax = (uint32_t)(rnd() % (1ull << (1 + rnd() % 32)));
    const uint64_t w = nearest::words_per_row(lmax);
    CHECK(w % 2 == 0 && 64 * w > lmax && 64 * (w - 2) <= lmax);
  }
}

static void check_limits() {
  using namespace nearest;
  CHECK(check_limits(0, 0, 0, 2) == LIMIT_OK && check_limits(1, 0, 1, 2) == LIMIT_OK);
  CHECK(check_limits(1u << 15, 1u << 15, 1u << 16, 62) == LIMIT_OK);  // exactly 2^30 pairs
  CHECK(check_limits((1u << 15) + 1, 1u << 15, 1, 2) == LIMIT_PAIRS);
  CHECK(check_limits(1ull << 40, 1ull << 40, 1, 2) == LIMIT_PAIRS);  // the product overflows 64 bits: still caught
  CHECK(check_limits(~0ull, 2, 1, 2) == LIMIT_PAIRS && check_limits(1ull << 30, 1, 1, 2) == LIMIT_OK);
  CHECK(check_limits(1, 1, 1ull << 20, 1ull << 13) == LIMIT_OK);       // exactly 2^36 bytes
  CHECK(check_limits(1, 1, (1ull << 20) + 1, 1ull << 13) == LIMIT_BITS);
  CHECK(check_limits(1, 1, 10000, words_per_row(3900)) == LIMIT_OK);   // the C3 corpus: 5 MB
  CHECK(check_limits(1, 1, 2000, words_per_row(0xFFFFFFFFu)) == LIMIT_BITS);  // sparse ids: 512 MB per row
  CHECK(check_limits(1, 1, 1ull << 32, 1ull << 26) == LIMIT_BITS);     // the largest arguments: no overflow
}

static void check_grid() {
  using namespace nearest;
  for (int k = 0; k < 4000; k++) {
    const uint64_t n_q = 1 + rnd() % 3000, n_c = 1 + rnd() % 3000, W = 2 * (1 + rnd() % 6000);
    const uint32_t n_cu = 1 + (uint32_t)(rnd() % 300), force = rnd() % 3 ? 0u : (uint32_t)(rnd() % 2000);
    const Grid g = grid(n_q, n_c, W, n_cu, force);
    CHECK(g.tq * NEAR_TILE >= n_q && (g.tq - 1) * NEAR_TILE < n_q && g.tc * NEAR_TILE >= n_c && (g.tc - 1) * NEAR_TILE < n_c);
    CHECK((uint64_t)g.slabs * NEAR_SLAB >= W && (uint64_t)(g.slabs - 1) * NEAR_SLAB < W);
    CHECK(g.ksplit >= 1 && g.ksplit <= NEAR_MAX_KSPLIT && g.ksplit <= g.slabs);
    // the ranges cover every slab once and none is empty
    CHECK((uint64_t)g.ksplit * g.slabs_per_split >= g.slabs && (uint64_t)(g.ksplit - 1) * g.slabs_per_split < g.slabs);
    if (force) CHECK(g.ksplit <= force);
    else if (g.tq * g.tc >= 2ull * n_cu) CHECK(g.ksplit == 1);
    else CHECK(g.ksplit == 1 || (g.ksplit - 1) * g.tq * g.tc < 2ull * n_cu);  // no more ranges than fill the device
  }
  const Grid c3 = grid(1139, 8861, 62, 256, 0);  // the C3 corpus: 18 x 139 tiles fill the device
  CHECK(c3.tq == 18 && c3.tc == 139 && c3.slabs == 4 && c3.ksplit == 1 && c3.slabs_per_split == 4);
  const Grid c5 = grid(100, 43, 9376, 256, 0);  // few runs, long rows: 2 tiles, 586 slabs
  CHECK(c5.tq == 2 && c5.tc == 1 && c5.slabs == 586 && c5.ksplit > 128 && c5.ksplit <= 256);
  const Grid f1 = grid(100, 43, 9376, 256, 1), f7 = grid(100, 43, 9376, 256, 7);
  CHECK(f1.ksplit == 1 && f1.slabs_per_split == 586 && f7.ksplit == 7 && f7.slabs_per_split == 84);
  CHECK(grid(5, 0, 2, 256, 0).tc == 0 && grid(5, 0, 2, 256, 3).ksplit == 1);  // no candidate: nothing is launched
}

// n_runs runs with random label sets below label_space; n_q / n_c list positions drawn from them
static void run_case(uint32_t n_runs, size_t n_q, size_t n_c, uint32_t label_space, uint32_t force) {
  std::vector<std::set<uint32_t>> labels(n_runs);
  uint32_t lmax = 0;
  for (auto &s : labels) {
    const uint32_t n = rnd() % 5 == 0 ? 0u : (uint32_t)(rnd() % 40);
    for (uint32_t i = 0; i < n; i++) s.insert((uint32_t)(rnd() % label_space));
    if (!s.empty()) lmax = std::max(lmax, *s.rbegin());
  }
  std::vector<uint32_t> q(n_q), c(n_c);
  for (auto &x : q) x = (uint32_t)(rnd() % n_runs);
  for (auto &x : c) x = (uint32_t)(rnd() % n_runs);
  const nearest::Rows rows = nearest::rows(q.data(), n_q, c.data(), n_c);
  // distinct runs in first-appearance order, queries first; a run in both lists has one row
  std::vector<uint32_t> want;
  auto row_of = [&](uint32_t run) {
    auto f = std::find(want.begin(), want.end(), run);
    if (f == want.end()) {
      want.push_back(run);
      f = want.end() - 1;
    }
    return (uint32_t)(f - want.begin());
  };
  CHECK(rows.qrow.size() == n_q && rows.crow.size() == n_c);
  for (size_t i = 0; i < n_q; i++) CHECK(rows.qrow[i] == row_of(q[i]));
  for (size_t j = 0; j < n_c; j++) CHECK(rows.crow[j] == row_of(c[j]));
  CHECK(rows.run == want);
  const uint64_t W = nearest::words_per_row(lmax), n_rows = want.size();
  CHECK(nearest::check_limits(n_q, n_c, n_rows, W) == nearest::LIMIT_OK);
  // the bit rows as k_near_bits fills them: exactly n_rows * W words
  std::vector<uint64_t> bits(n_rows * W, 0);
  std::vector<uint32_t> size(n_rows, 0);
  for (uint64_t r = 0; r < n_rows; r++)
    for (uint32_t l : labels[want[r]]) {
      CHECK((l >> 6) < W);
      uint64_t &w = bits[r * W + (l >> 6)];
      size[r] += !(w >> (l & 63) & 1);
      w |= 1ull << (l & 63);
    }
  // k_near_isect's walk: tiles, K ranges, slabs, 16-byte chunks clamped to the row's last chunk and masked
  const nearest::Grid g = nearest::grid(n_q, n_c, W, 4, force);
  std::vector<uint32_t> mat(n_q * n_c, 0);
  const uint64_t w2 = W / 2;
  for (uint64_t t = 0; t < g.tq * g.tc; t++)
    for (uint32_t z = 0; z < g.ksplit; z++) {
      const uint64_t q0 = (t / g.tc) * NEAR_TILE, c0 = (t % g.tc) * NEAR_TILE;
      const uint32_t s_lo = z * g.slabs_per_split, s_hi = std::min(g.slabs, s_lo + g.slabs_per_split);
      CHECK(s_lo < s_hi);
      for (uint32_t i = 0; i < NEAR_TILE; i++)
        for (uint32_t j = 0; j < NEAR_TILE; j++) {
          const uint64_t qi = std::min<uint64_t>(q0 + i, n_q - 1), cj = std::min<uint64_t>(c0 + j, n_c - 1);
          uint32_t acc = 0;
          for (uint32_t s = s_lo; s < s_hi; s++)
            for (uint32_t kp = 0; kp < NEAR_SLAB / 2; kp++) {
              const uint64_t k = (uint64_t)s * (NEAR_SLAB / 2) + kp, kc = std::min(k, w2 - 1);
              const uint64_t *a = &bits[rows.qrow[qi] * W + 2 * kc], *b = &bits[rows.crow[cj] * W + 2 * kc];
              if (k < w2) acc += __builtin_popcountll(a[0] & b[0]) + __builtin_popcountll(a[1] & b[1]);
            }
          if (q0 + i < n_q && c0 + j < n_c) mat[(q0 + i) * n_c + (c0 + j)] += acc;
        }
    }
  for (size_t i = 0; i < n_q; i++)
    for (size_t j = 0; j < n_c; j++) {
      std::vector<uint32_t> both;
      std::set_intersection(labels[q[i]].begin(), labels[q[i]].end(), labels[c[j]].begin(), labels[c[j]].end(),
                            std::back_inserter(both));
      CHECK(mat[i * n_c + j] == both.size());
      CHECK(size[rows.qrow[i]] == labels[q[i]].size() && size[rows.crow[j]] == labels[c[j]].size());
    }
  printf("runs %u queries %zu candidates %zu labels < %u: %llu rows of %llu words, %llu x %llu tiles, %u K ranges\n", n_runs,
         n_q, n_c, label_space, (unsigned long long)n_rows, (unsigned long long)W, (unsigned long long)g.tq,
         (unsigned long long)g.tc, g.ksplit);
}

int main() {
  check_words();
  check_limits();
  check_grid();
  run_case(1, 1, 1, 8, 0);          // one run against itself
  run_case(3, 0, 5, 64, 0);         // no query
  run_case(3, 5, 0, 64, 0);         // no candidate
  run_case(6, 40, 40, 64, 0);       // duplicates in both lists; one 16-byte chunk per row
  run_case(6, 40, 40, 129, 0);      // labels 63 / 64 / 127 / 128
  run_case(130, 65, 129, 1100, 0);  // tile + 1 and two tiles + 1; a slab and a part
  run_case(40, 64, 64, 2048, 3);    // exact tiles, exact slabs, three K ranges
  run_case(20, 7, 70, 40000, 0);    // long rows: the automatic split
  run_case(20, 7, 70, 40000, 7);
  run_case(20, 7, 70, 40000, 1);
  puts("nearest_host_check OK");
  return 0;
}
