// lin_host_check — drives the host side of nemo_lineage_cuts (nemo_amd/csrc/lin_host.h): the keys (pack, unpack,
// insert, subsets, equality) over every set of small universes and the edges of the u16 range, the rows' order against
// cut_host.h's colex ranks for sizes 1..3 and against a plain comparison of reversed positions above, the subset
// enumeration, the candidate checks (cut_host.h's, and the limit), the option's value, the table and buffer sizes, a
// level's end, the chunk and grid counts, and the table steps the kernels take (duplicate removal, the subset filter) in a host model
// of the whole level search on AND-of-ORs graphs against brute force, with the stats the definition gives.  Meant for
// the host sanitizers; it calls nothing on a device:
//   g++ -std=c++17 -g -Wall -fsanitize=address,undefined -static-libasan -static-libubsan
//       tools/lin_host_check.cpp -o tools/lin_host_check
//   tools/lin_host_check
#include "../nemo_amd/csrc/lin_host.h"

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

static std::vector<uint32_t> members(uint32_t mask) {
  std::vector<uint32_t> p;
  for (uint32_t j = 0; j < 32; j++)
    if ((mask >> j) & 1u) p.push_back(j);
  return p;
}

static void check_keys() {
  CHECK(sizeof(lin::Key) == 16 && lin::key_size(lin::key_empty()) == 0);
  const uint32_t full[8] = {0, 1, 2, 3, 65531, 65532, 65533, 65534};
  const lin::Key kf = lin::key_pack(full, 8);
  uint32_t pos[8];
  CHECK(lin::key_size(kf) == 8 && lin::key_unpack(kf, pos) == 8);
  for (int j = 0; j < 8; j++) CHECK(pos[j] == full[j] && lin::key_at(kf, j) == full[j]);
  CHECK(kf.lo == (0ull | 1ull << 16 | 2ull << 32 | 3ull << 48) && (kf.hi >> 48) == 65534);
  // every set of at most 8 of 11 positions: pack / unpack, insertion of every absent position, equality
  for (uint32_t m = 0; m < (1u << 11); m++) {
    const std::vector<uint32_t> p = members(m);
    if (p.size() > 8) continue;
    const lin::Key k = lin::key_pack(p.data(), (uint32_t)p.size());
    CHECK(lin::key_size(k) == p.size() && lin::key_unpack(k, pos) == p.size());
    for (size_t j = 0; j < p.size(); j++) CHECK(pos[j] == p[j]);
    for (size_t j = p.size(); j < 8; j++) CHECK(lin::key_at(k, (uint32_t)j) == LIN_PAD);
    if (p.size() == 8) continue;
    for (uint32_t e = 0; e < 11; e++) {
      if ((m >> e) & 1u) continue;
      const std::vector<uint32_t> q = members(m | 1u << e);
      CHECK(lin::key_eq(lin::key_insert(k, e), lin::key_pack(q.data(), (uint32_t)q.size())));
      CHECK(!lin::key_eq(lin::key_insert(k, e), k));
    }
    // above and below everything in the set, at the edges of the range
    const lin::Key hi = lin::key_insert(k, 65534);
    CHECK(lin::key_size(hi) == p.size() + 1 && lin::key_at(hi, (uint32_t)p.size()) == 65534);
  }
}

static void check_subsets() {
  CHECK(lin::subset_masks(0) == 0 && lin::subset_masks(1) == 0 && lin::subset_masks(2) == 2 && lin::subset_masks(8) == 254);
  const uint32_t p[8] = {3, 9, 10, 200, 201, 4000, 65000, 65534};
  for (uint32_t n = 1; n <= 8; n++) {
    const lin::Key k = lin::key_pack(p, n);
    std::set<std::pair<uint64_t, uint64_t>> seen;
    for (uint32_t m = 1; m <= lin::subset_masks(n); m++) {
      const lin::Key s = lin::key_subset(k, m);
      uint32_t q[8];
      const uint32_t sz = lin::key_unpack(s, q);
      CHECK(sz == (uint32_t)__builtin_popcount(m) && sz >= 1 && sz < n);
      for (uint32_t j = 0; j + 1 < sz; j++) CHECK(q[j] < q[j + 1]);
      for (uint32_t j = 0; j < sz; j++) CHECK(std::find(p, p + n, q[j]) != p + n);
      CHECK(seen.insert({s.lo, s.hi}).second);
    }
    CHECK(seen.size() == (1u << n) - 2u);
    CHECK(lin::key_eq(lin::key_subset(k, (1u << n) - 1u), k));
  }
}

static void check_order() {
  // sizes 1..3 over 12 positions: the order of the rows is the order of cut_host.h's colex ranks
  std::vector<lin::Key> keys;
  for (uint32_t m = 1; m < (1u << 12); m++) {
    const std::vector<uint32_t> p = members(m);
    if (p.size() <= 3) keys.push_back(lin::key_pack(p.data(), (uint32_t)p.size()));
  }
  std::sort(keys.begin(), keys.end(), lin::row_less);
  uint32_t size = 1;
  uint64_t want = 0;
  for (const lin::Key &k : keys) {
    uint32_t p[8];
    const uint32_t n = lin::key_unpack(k, p);
    if (n != size) {
      CHECK(n == size + 1);
      size = n, want = 0;
    }
    const uint64_t r = n == 1 ? p[0] : n == 2 ? cuts::rank2(p[0], p[1]) : cuts::rank3(p[0], p[1], p[2]);
    CHECK(r == want++);
  }
  // sizes 4..8: the largest position first, then the next largest
  std::vector<std::vector<uint32_t>> rev;
  keys.clear();
  for (uint32_t m = 1; m < (1u << 10); m++) {
    const std::vector<uint32_t> p = members(m);
    if (p.size() < 4 || p.size() > 8) continue;
    keys.push_back(lin::key_pack(p.data(), (uint32_t)p.size()));
  }
  std::sort(keys.begin(), keys.end(), lin::row_less);
  for (size_t i = 1; i < keys.size(); i++) {
    uint32_t a[8], b[8];
    const uint32_t na = lin::key_unpack(keys[i - 1], a), nb = lin::key_unpack(keys[i], b);
    CHECK(na <= nb && !lin::row_less(keys[i], keys[i - 1]) && !lin::key_eq(keys[i], keys[i - 1]));
    if (na != nb) continue;
    std::vector<uint32_t> ra(a, a + na), rb(b, b + nb);
    std::reverse(ra.begin(), ra.end()), std::reverse(rb.begin(), rb.end());
    CHECK(ra < rb);
  }
  CHECK(!lin::row_less(keys[0], keys[0]));
}

static void check_call() {
  size_t where = 99;
  const uint32_t ok[4] = {5, 0, 9, 3}, range[3] = {1, 10, 2}, dup[4] = {4, 2, 7, 2};
  CHECK(lin::check_cands(ok, 4, 10, &where) == lin::CAND_OK && lin::check_cands(nullptr, 0, 10, &where) == lin::CAND_OK);
  CHECK(lin::check_cands(range, 3, 10, &where) == lin::CAND_RANGE && where == 1);
  CHECK(lin::check_cands(dup, 4, 10, &where) == lin::CAND_DUP && where == 3);
  std::vector<uint32_t> many(65536);
  for (uint32_t i = 0; i < 65536; i++) many[i] = i;
  CHECK(lin::check_cands(many.data(), 65535, 70000, &where) == lin::CAND_OK);
  CHECK(lin::check_cands(many.data(), 65536, 70000, &where) == lin::CAND_LIMIT);
  for (uint32_t s = 0; s <= 10; s++) CHECK(lin::size_ok(s, 0) == (s >= 1 && s <= 8) && !lin::size_ok(s, 1));
  CHECK(!lin::size_ok(0xFFFFFFFFu, 0));
  CHECK(lin::front_fits(0) && lin::front_fits(LIN_MAX_FRONT) && !lin::front_fits(LIN_MAX_FRONT + 1));
  CHECK(lin::children_option(-1) == LIN_CHILDREN_DEFAULT && LIN_CHILDREN_DEFAULT * 16 == 256ull << 20);
  CHECK(lin::children_option(63) == 0 && lin::children_option(0) == 0 && lin::children_option(-2) == 0 && lin::children_option(64) == 64);
  CHECK(lin::children_option(65536) == 65536 && lin::children_option(1ll << 40) == LIN_CHILDREN_MAX);
}

static void check_sizes() {
  for (uint64_t n : {0ull, 1ull, 31ull, 32ull, 33ull, 1000ull, 1024ull, 1025ull, (1ull << 24), (1ull << 31)}) {
    const uint64_t s = lin::table_slots(n);
    CHECK(s >= LIN_MIN_TABLE && s >= 2 * n && (s & (s - 1)) == 0 && (s == LIN_MIN_TABLE || s / 2 < 2 * n));
  }
  CHECK(lin::emit_bound(1, 258, 0) == 258 && lin::emit_bound(129, 258, 1) == 129 * 257 && lin::emit_bound(5, 3, 3) == 0);
  CHECK(lin::emit_bound(5, 2, 3) == 0 && lin::emit_bound(~0ull / 2, 10, 1) == ~0ull);
  CHECK(lin::emit_grown(1024, 16641) == 16641 && lin::emit_grown(1024, 10) == 1024);
  CHECK(lin::cuts_grown(64, 0, 64) == 64 && lin::cuts_grown(64, 1, 64) == 128 && lin::cuts_grown(64, 10, 1000) == 1010);
  CHECK(lin::level_end(10, 1024, 64, 0) == lin::LEVEL_DONE && lin::level_end(65, 1024, 64, 0) == lin::LEVEL_LIMIT);
  CHECK(lin::level_end(1025, 1024, 1 << 20, 0) == lin::LEVEL_AGAIN && lin::level_end(1025, 1024, 1 << 20, 1) == lin::LEVEL_BROKEN);
  CHECK(lin::level_end(1024, 1024, 1024, 1) == lin::LEVEL_DONE && lin::level_end(2000, 1024, 1500, 0) == lin::LEVEL_LIMIT);
  CHECK(lin::chunks(0) == 0 && lin::chunks(1) == 1 && lin::chunks(64) == 1 && lin::chunks(65) == 2 && lin::chunks(129) == 3);
  CHECK(lin::grid(0, 256, 0) == 1 && lin::grid(3, 256, 0) == 3 && lin::grid(1000, 256, 0) == 256 && lin::grid(1000, 256, 1) == 1);
  CHECK(lin::grid(~0ull, 512, 0) == 512 && lin::grid(~0ull, 512, 7) == 7);
  CHECK(lin::filter_grid(0, LIN_BLOCK, 2048) == 1 && lin::filter_grid(256, LIN_BLOCK, 2048) == 1 && lin::filter_grid(257, LIN_BLOCK, 2048) == 2);
  CHECK(lin::filter_grid(1ull << 31, LIN_BLOCK, 2048) == 2048);
}

// ---- a host model of the level search over the table steps -----------------------------------------------
// AND-of-ORs: the outcome needs every one of m goals; goal i holds by sink a_i (position 2 i) or, if that is dead,
// by sink b_i (position 2 i + 1); with an extra sink c (position 2 m) under the top rule if with_c.  The witness of a
// non-cut F: per goal the alive sink of smaller position, and c.
struct AndOfOrs {
  uint32_t m;
  bool with_c;
  uint32_t K() const { return 2 * m + (with_c ? 1 : 0); }
  bool lost(const lin::Key &f) const {
    uint32_t p[8];
    const uint32_t n = lin::key_unpack(f, p);
    std::set<uint32_t> dead(p, p + n);
    if (with_c && dead.count(2 * m)) return true;
    for (uint32_t i = 0; i < m; i++)
      if (dead.count(2 * i) && dead.count(2 * i + 1)) return true;
    return false;
  }
  std::vector<uint32_t> witness(const lin::Key &f) const {
    uint32_t p[8];
    const uint32_t n = lin::key_unpack(f, p);
    std::set<uint32_t> dead(p, p + n);
    std::vector<uint32_t> w;
    for (uint32_t i = 0; i < m; i++) w.push_back(dead.count(2 * i) ? 2 * i + 1 : 2 * i);
    if (with_c) w.push_back(2 * m);
    return w;
  }
};

static void check_search(const AndOfOrs &g, uint32_t max_size) {
  std::vector<lin::Key> front{lin::key_empty()}, cuts_, kids;
  uint64_t cslots = lin::table_slots(64);
  std::vector<uint32_t> ctab(cslots, 0);
  uint32_t sizes = 0;
  std::vector<uint64_t> evaluated, found;
  for (uint32_t d = 0; d <= max_size && !front.empty(); d++) {
    evaluated.push_back(front.size());
    if (lin::cuts_grown(cslots / 2, cuts_.size(), front.size()) != cslots / 2) {  // the table anew, the cuts again
      cslots = lin::table_slots(lin::cuts_grown(cslots / 2, cuts_.size(), front.size()));
      ctab.assign(cslots, 0);
      for (uint32_t i = 0; i < cuts_.size(); i++) CHECK(lin::table_insert(ctab.data(), cslots, cuts_.data(), i));
    }
    const size_t before = cuts_.size();
    kids.clear();
    for (const lin::Key &f : front) {
      if (g.lost(f)) {
        cuts_.push_back(f);
        CHECK(lin::table_insert(ctab.data(), cslots, cuts_.data(), (uint32_t)cuts_.size() - 1));
      } else if (d < max_size) {
        for (uint32_t e : g.witness(f)) kids.push_back(lin::key_insert(f, e));
      }
    }
    found.push_back(cuts_.size() - before);
    if (cuts_.size() > before) sizes |= 1u << d;
    CHECK(kids.size() <= lin::emit_bound(front.size(), g.K(), d));
    const uint64_t kslots = lin::table_slots(kids.size());
    std::vector<uint32_t> ktab(kslots, 0);
    front.clear();
    for (uint32_t i = 0; i < kids.size(); i++) {
      if (!lin::table_insert(ktab.data(), kslots, kids.data(), i)) continue;
      if (lin::has_cut_subset(ctab.data(), cslots, cuts_.data(), kids[i], sizes)) continue;
      front.push_back(kids[i]);
    }
  }
  // brute force: every set of at most max_size positions, the lost ones with no lost proper subset
  std::set<std::pair<uint64_t, uint64_t>> want, got;
  const uint32_t K = g.K();
  for (uint32_t mask = 1; mask < (1u << K); mask++) {
    const std::vector<uint32_t> p = members(mask);
    if (p.size() > max_size) continue;
    const lin::Key k = lin::key_pack(p.data(), (uint32_t)p.size());
    if (!g.lost(k)) continue;
    bool minimal = true;
    for (uint32_t s = 1; s <= lin::subset_masks((uint32_t)p.size()) && minimal; s++) minimal = !g.lost(lin::key_subset(k, s));
    if (minimal) want.insert({k.lo, k.hi});
  }
  for (const lin::Key &k : cuts_) CHECK(got.insert({k.lo, k.hi}).second);
  CHECK(got == want);
  if (!g.with_c && max_size == 2) {  // 1, m and m + C(m, 2) sets: every {a_i, a_j} comes from two parents and counts once
    const uint64_t m = g.m;
    CHECK(evaluated.size() == 3 && evaluated[0] == 1 && evaluated[1] == m && evaluated[2] == m + m * (m - 1) / 2);
    CHECK(found[0] == 0 && found[1] == 0 && found[2] == m);
  }
  if (g.with_c) {  // {c} is a cut at level 1 and no set above it is evaluated
    CHECK(found[1] == 1 && evaluated[1] == g.m + 1);
    if (max_size >= 2) CHECK(evaluated[2] == g.m + (uint64_t)g.m * (g.m - 1) / 2);
  }
}

int main() {
  check_keys();
  check_subsets();
  check_order();
  check_call();
  check_sizes();
  for (uint32_t m = 1; m <= 5; m++)
    for (uint32_t s = 1; s <= 4; s++) {
      check_search(AndOfOrs{m, false}, s);
      check_search(AndOfOrs{m, true}, s);
    }
  check_search(AndOfOrs{9, false}, 2);
  printf("lin_host_check OK\n");
  return 0;
}
