// lgc_host_check — drives the host side of nemo_lineage_group_cuts (nemo_amd/csrc/lgc_host.h): the limits, what a
// workgroup keeps behind its image and in its region, and a host model of the whole search in the steps
// the kernels take (the keys, the lost words and the cross-run count under q, the children as a union over the list
// positions on which a set is not lost, duplicate removal and the subset filter in the two tables, a level that runs
// again behind a grown emission buffer without appending its cuts twice) against brute force over all subsets and
// against a plain search over std::set, on small random AND/OR graphs: 2-3 runs, <= 12 groups with overlaps and an empty
// group, sizes <= 5.  Meant for the host sanitizers; it calls nothing on a device:
//   g++ -std=c++17 -g -Wall -fsanitize=address,undefined -static-libasan -static-libubsan
//       tools/lgc_host_check.cpp -o tools/lgc_host_check
//   tools/lgc_host_check
#include "../nemo_amd/csrc/lgc_host.h"

#include <cstdio>
#include <cstdlib>
#include <map>
#include <random>
#include <set>

#define CHECK(x)                                            \
  do {                                                      \
    if (!(x)) {                                             \
      fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #x); \
      exit(1);                                              \
    }                                                       \
  } while (0)

static void check_limits() {
  CHECK(lgc::groups_fit(0) && lgc::groups_fit(65535) && !lgc::groups_fit(65536));
  for (uint32_t s = 0; s <= 10; s++) CHECK(lgc::size_ok(s) == (s >= 1 && s <= 8));
  CHECK(!lgc::size_ok(0xFFFFFFFFu));
  CHECK(lgc::level_check(1, 1) == lgc::LEVEL_OK && lgc::level_check(1ull << 28, 64) == lgc::LEVEL_OK);
  CHECK(lgc::level_check((1ull << 28) + 1, 1) == lgc::LEVEL_WORDS && lgc::level_check(1ull << 28, 65) == lgc::LEVEL_WORDS);
  CHECK(lgc::level_check(1, LIN_MAX_FRONT + 1) == lgc::LEVEL_FRONT && lgc::level_check(1, LIN_MAX_FRONT) == lgc::LEVEL_OK);
  CHECK(lgc::level_check(0, 5) == lgc::LEVEL_OK);
  CHECK(lgc::emit_bound(2, 65, 130, 1) == 2 * 65 * 129 && lgc::emit_bound(3, 1, 8, 0) == 24 && lgc::emit_bound(0, 5, 8, 0) == 0);
  CHECK(lgc::emit_bound(1ull << 40, 1ull << 30, 65535, 1) == ~0ull);
  CHECK(lgc::is_cut(2, 2) && lgc::is_cut(3, 2) && !lgc::is_cut(1, 2) && !lgc::is_cut(0, 0));
}

static void check_tail() {
  // everything fits: the rows' need words, then the whole list
  lgc::Tail t = lgc::tail(4096 + 80 + 400, 4096, 10);
  CHECK(t.rn_lds == 1 && t.rn_bytes == 80 && t.head == 100);
  CHECK(lgc::spill_offset(0, 10, t) == 0 && lgc::region_words(0, 10, 50, t) == 0);
  // an odd number of rows takes whole 16-byte chunks
  t = lgc::tail(4096 + 100, 4096, 11);
  CHECK(t.rn_lds == 1 && t.rn_bytes == 96 && t.head == 1);
  // the rows' need words do not fit: they go to the region, the head takes all that is left
  t = lgc::tail(4096 + 64, 4096, 10);
  CHECK(t.rn_lds == 0 && t.rn_bytes == 0 && t.head == 16);
  CHECK(lgc::rn_offset(0) == 0 && lgc::spill_offset(0, 10, t) == 10 && lgc::spill_offset(0, 11, t) == 12);
  CHECK(lgc::region_words(0, 10, 50, t) == 10 + (((10 + 1 + 50 - 16 + 1) / 2 + 1) & ~1ull));
  // no LDS at all (the global tier): dead and need words first
  t = lgc::tail(0, 0, 7);
  CHECK(t.rn_lds == 0 && t.head == 0);
  const uint64_t words = wit::glob_words(101);
  CHECK(words == 204 && lgc::rn_offset(words) == 204 && lgc::spill_offset(words, 7, t) == 212);
  CHECK(lgc::region_words(words, 7, 101, t) >= 212 + (7 + 1 + 101 + 1) / 2);
  t = lgc::tail(100, 4096, 3);  // an image larger than the launch's LDS cannot be: nothing is left
  CHECK(t.rn_lds == 0 && t.head == 0);
  CHECK(lgc::tail_want(10, 50) == 80 + 4 * 61);
  for (uint32_t D : {0u, 1u, 2u, 63u, 64u, 1000u})
    for (uint32_t left : {0u, 8u, 16u, 500u, 8000u, 9000u}) {
      const lgc::Tail x = lgc::tail(2048 + left, 2048, D);
      CHECK(x.rn_bytes % 16 == 0 && x.rn_bytes + 4ull * x.head <= left && (!x.rn_lds || x.rn_bytes >= 8ull * D));
      CHECK(lgc::spill_offset(0, D, x) % 2 == 0 && lgc::region_words(0, D, 300, x) % 2 == 0);
      const uint64_t entries = gcuts::list_entries(D, 300), spill = entries > x.head ? entries - x.head : 0;
      CHECK(2 * (lgc::region_words(0, D, 300, x) - lgc::spill_offset(0, D, x)) >= spill);
    }
}

// ---- small random AND/OR graphs -------------------------------------------------------------------------------
struct Graph {  // children have larger indices: the index order is a topological order, roots first
  std::vector<uint8_t> rule;
  std::vector<std::vector<uint32_t>> ch;
  std::vector<uint32_t> label, roots;
  uint32_t V() const { return (uint32_t)rule.size(); }
  bool sink(uint32_t v) const { return !rule[v] && ch[v].empty(); }
};

static Graph random_graph(std::mt19937 &rng, uint32_t n_labels) {
  Graph g;
  const uint32_t V = 6 + rng() % 14;
  g.rule.resize(V), g.ch.resize(V), g.label.resize(V);
  std::vector<uint8_t> has_parent(V, 0);
  for (uint32_t v = 0; v < V; v++) {
    g.rule[v] = v == 0 ? 0 : rng() % 2;
    g.label[v] = rng() % n_labels;
    if (v + 1 < V && (v < V / 2 || rng() % 3 == 0)) {
      const uint32_t k = 1 + rng() % 3;
      std::set<uint32_t> c;
      for (uint32_t j = 0; j < k; j++) c.insert(v + 1 + rng() % (V - v - 1));
      g.ch[v].assign(c.begin(), c.end());
      for (uint32_t x : c) has_parent[x] = 1;
    }
  }
  for (uint32_t v = 0; v < V; v++)
    if (!has_parent[v]) g.roots.push_back(v);
  return g;
}

struct Problem {
  std::vector<Graph> runs;  // a list position each (one of them may be listed twice)
  std::vector<std::vector<uint32_t>> groups;
  bool sinks;
  uint32_t q;
};

// the nodes dead under the set's groups on one graph; *lost: every root is dead
static std::vector<uint8_t> dead_under(const Problem &p, const Graph &g, const std::vector<uint32_t> &set, bool *lost) {
  std::set<uint32_t> labels;
  for (uint32_t k : set) labels.insert(p.groups[k].begin(), p.groups[k].end());
  std::vector<uint8_t> dead(g.V(), 0);
  for (uint32_t v = g.V(); v-- > 0;) {
    bool d = labels.count(g.label[v]) && (!p.sinks || g.sink(v));
    if (!d && !g.ch[v].empty()) {
      if (g.rule[v]) {
        for (uint32_t c : g.ch[v]) d = d || dead[c];
      } else {
        d = true;
        for (uint32_t c : g.ch[v]) d = d && dead[c];
      }
    }
    dead[v] = d;
  }
  *lost = !g.roots.empty();
  for (uint32_t r : g.roots) *lost = *lost && dead[r];
  return dead;
}

// the candidates some node of the single derivation names (a needed goal needs its alive child of smallest index)
static std::set<uint32_t> witness_kids(const Problem &p, const Graph &g, const std::vector<uint8_t> &dead) {
  std::vector<uint8_t> need(g.V(), 0);
  for (uint32_t r : g.roots) need[r] = !dead[r];
  std::set<uint32_t> kids;
  for (uint32_t v = 0; v < g.V(); v++) {
    if (!need[v]) continue;
    if (g.rule[v]) {
      for (uint32_t c : g.ch[v]) need[c] = 1;
    } else {
      for (uint32_t c : g.ch[v])
        if (!dead[c]) {
          need[c] = 1;
          break;
        }
    }
    if (p.sinks && !g.sink(v)) continue;
    for (uint32_t k = 0; k < p.groups.size(); k++)
      if (std::find(p.groups[k].begin(), p.groups[k].end(), g.label[v]) != p.groups[k].end()) kids.insert(k);
  }
  return kids;
}

static std::vector<uint32_t> positions(const lin::Key &k) {
  uint32_t pos[8];
  const uint32_t n = lin::key_unpack(k, pos);
  return std::vector<uint32_t>(pos, pos + n);
}

struct Result {
  std::vector<lin::Key> rows;
  std::vector<uint32_t> n_lost;
  uint64_t stats[18];
};

// the search in the kernels' steps; emit_start: the emission buffer before it has grown
static Result search_model(const Problem &p, uint32_t max_size, uint64_t emit_start, uint32_t *reruns) {
  Result r{};
  const uint64_t n = p.runs.size();
  std::vector<lin::Key> front{lin::key_empty()}, cuts_, kids;
  std::vector<uint32_t> nl;
  uint64_t cuts_cap = LIN_MIN_TABLE, cslots = lin::table_slots(cuts_cap), kids_cap = emit_start;
  std::vector<uint32_t> ctab(cslots, 0);
  uint32_t sizes = 0;
  for (uint32_t d = 0; d <= max_size && !front.empty(); d++) {
    CHECK(lgc::level_check(n, front.size()) == lgc::LEVEL_OK);
    r.stats[2 * d] = front.size();
    const uint64_t grown = lin::cuts_grown(cuts_cap, cuts_.size(), front.size());
    if (grown != cuts_cap) {  // the table anew, the cuts again
      cuts_cap = grown, cslots = lin::table_slots(grown);
      ctab.assign(cslots, 0);
      for (uint32_t i = 0; i < cuts_.size(); i++) CHECK(lin::table_insert(ctab.data(), cslots, cuts_.data(), i));
    }
    const bool emit = d < max_size;
    const uint64_t ck = lin::chunks(front.size()), before = cuts_.size();
    std::vector<uint64_t> lost(n * ck, 0);
    for (int pass = 0;; pass++) {
      // the evaluation: a lost word per (list position, chunk); children from every (position, set) that is not lost
      uint64_t counted = 0;
      kids.clear();
      std::fill(lost.begin(), lost.end(), 0);
      for (uint64_t i = 0; i < n; i++)
        for (uint64_t s = 0; s < front.size(); s++) {
          bool l;
          const std::vector<uint8_t> dead = dead_under(p, p.runs[i], positions(front[s]), &l);
          if (l) {
            lost[i * ck + s / KO_CHUNK] |= 1ull << (s % KO_CHUNK);
          } else if (emit) {
            for (uint32_t k : witness_kids(p, p.runs[i], dead)) {
              if (counted++ < kids_cap) kids.push_back(lin::key_insert(front[s], k));  // counted past the end, not written
            }
          }
        }
      if (!pass)  // the cuts of the level; a second pass finds them in place
        for (uint64_t s = 0; s < front.size(); s++) {
          const uint32_t cnt = lgc::lost_count(lost.data(), n, ck, s);
          if (!lgc::is_cut(cnt, p.q)) continue;
          cuts_.push_back(front[s]), nl.push_back(cnt);
          CHECK(cuts_.size() <= cuts_cap && lin::table_insert(ctab.data(), cslots, cuts_.data(), (uint32_t)cuts_.size() - 1));
        }
      const lin::LevelEnd end = emit ? lin::level_end(counted, kids_cap, LIN_CHILDREN_DEFAULT, pass) : lin::LEVEL_DONE;
      CHECK(end == lin::LEVEL_DONE || end == lin::LEVEL_AGAIN);
      CHECK(counted <= lgc::emit_bound(n, front.size(), p.groups.size(), d));
      if (end == lin::LEVEL_DONE) break;
      kids_cap = lin::emit_grown(kids_cap, counted);
      (*reruns)++;
    }
    r.stats[2 * d + 1] = cuts_.size() - before;
    if (cuts_.size() > before) sizes |= 1u << d;
    const uint64_t kslots = lin::table_slots(kids.size());
    std::vector<uint32_t> ktab(kslots, 0);
    front.clear();
    for (uint32_t i = 0; i < kids.size(); i++) {
      CHECK(lin::key_size(kids[i]) == d + 1);
      if (!lin::table_insert(ktab.data(), kslots, kids.data(), i)) continue;
      if (lin::has_cut_subset(ctab.data(), cslots, cuts_.data(), kids[i], sizes)) continue;
      front.push_back(kids[i]);
    }
  }
  std::vector<uint32_t> order(cuts_.size());
  for (uint32_t i = 0; i < order.size(); i++) order[i] = i;
  std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return lin::row_less(cuts_[a], cuts_[b]); });
  for (uint32_t i : order) r.rows.push_back(cuts_[i]), r.n_lost.push_back(nl[i]);
  return r;
}

static uint32_t count_lost(const Problem &p, const std::vector<uint32_t> &set) {
  uint32_t cnt = 0;
  for (const Graph &g : p.runs) {
    bool l;
    dead_under(p, g, set, &l);
    cnt += l;
  }
  return cnt;
}

// the search as the header states it, over plain sets: the stats
static void search_plain(const Problem &p, uint32_t max_size, uint64_t stats[18]) {
  std::fill(stats, stats + 18, 0ull);
  std::set<std::set<uint32_t>> front{{}}, cuts_;
  for (uint32_t d = 0; d <= max_size && !front.empty(); d++) {
    stats[2 * d] = front.size();
    std::set<std::set<uint32_t>> kids;
    for (const std::set<uint32_t> &f : front) {
      const std::vector<uint32_t> set(f.begin(), f.end());
      if (count_lost(p, set) >= p.q) cuts_.insert(f), stats[2 * d + 1]++;
      if (d == max_size) continue;
      for (const Graph &g : p.runs) {
        bool l;
        const std::vector<uint8_t> dead = dead_under(p, g, set, &l);
        if (l) continue;
        for (uint32_t k : witness_kids(p, g, dead)) {
          std::set<uint32_t> c = f;
          CHECK(c.insert(k).second);  // a candidate of the set is not in its witness
          kids.insert(c);
        }
      }
    }
    front.clear();
    for (const std::set<uint32_t> &c : kids) {
      bool below = false;
      for (const std::set<uint32_t> &x : cuts_) below = below || (x.size() < c.size() && std::includes(c.begin(), c.end(), x.begin(), x.end()));
      if (!below) front.insert(c);
    }
  }
}

static void check_problem(const Problem &p, uint32_t max_size, uint32_t *reruns, uint64_t *rows_seen, uint64_t *big) {
  const Result a = search_model(p, max_size, 1024, reruns), b = search_model(p, max_size, 3, reruns);
  // brute force: every set of at most max_size positions, the cuts with no cut among their proper subsets
  const uint32_t K = (uint32_t)p.groups.size();
  std::map<uint32_t, uint32_t> cnt;
  for (uint32_t m = 0; m < (1u << K); m++)
    if ((uint32_t)__builtin_popcount(m) <= max_size) {
      std::vector<uint32_t> set;
      for (uint32_t k = 0; k < K; k++)
        if ((m >> k) & 1u) set.push_back(k);
      cnt[m] = count_lost(p, set);
    }
  std::vector<lin::Key> want;
  std::vector<uint32_t> want_n;
  std::vector<std::pair<lin::Key, uint32_t>> found;
  for (const auto &e : cnt) {
    if (e.second < p.q) continue;
    bool minimal = true;
    for (uint32_t s = (e.first - 1) & e.first; minimal; s = (s - 1) & e.first) {  // the proper subsets, the empty one last
      minimal = cnt[s] < p.q;
      if (!s) break;
    }
    if (!e.first || !minimal) continue;
    std::vector<uint32_t> set;
    for (uint32_t k = 0; k < K; k++)
      if ((e.first >> k) & 1u) set.push_back(k);
    found.push_back({lin::key_pack(set.data(), (uint32_t)set.size()), e.second});
  }
  std::sort(found.begin(), found.end(), [](const auto &x, const auto &y) { return lin::row_less(x.first, y.first); });
  uint64_t plain[18];
  search_plain(p, max_size, plain);
  for (const Result *r : {&a, &b}) {
    CHECK(r->rows.size() == found.size());
    for (size_t i = 0; i < found.size(); i++) CHECK(lin::key_eq(r->rows[i], found[i].first) && r->n_lost[i] == found[i].second);
    for (int i = 0; i < 18; i++) CHECK(r->stats[i] == plain[i]);
  }
  *rows_seen += found.size();
  for (const auto &f : found) *big += lin::key_size(f.first) >= 3;
}

int main() {
  check_limits();
  check_tail();
  std::mt19937 rng(20240607);
  uint32_t reruns = 0;
  uint64_t rows = 0, big = 0;
  for (int t = 0; t < 180; t++) {
    Problem p;
    const uint32_t n_labels = 8 + rng() % 8, runs = 2 + rng() % 2, K = 4 + rng() % 9;
    for (uint32_t i = 0; i < runs; i++) p.runs.push_back(random_graph(rng, n_labels));
    if (t % 5 == 0) p.runs.push_back(p.runs[0]);  // a run listed twice counts twice
    for (uint32_t k = 0; k < K; k++) {
      std::vector<uint32_t> g;
      const uint32_t len = k == 1 ? 0 : 1 + rng() % 3;  // group 1 is empty; the others overlap
      for (uint32_t j = 0; j < len; j++) g.push_back(rng() % (n_labels + 2));  // a label no node carries among them
      if (k == 3) g = p.groups[0];  // equal groups
      p.groups.push_back(g);
    }
    p.sinks = t % 3 == 1;
    const uint32_t qs[3] = {(uint32_t)p.runs.size(), 1u, (uint32_t)p.runs.size() - 1u};
    p.q = qs[t % 3];
    check_problem(p, 1 + t % 5, &reruns, &rows, &big);
  }
  CHECK(reruns > 10 && rows > 50 && big > 0);
  printf("lgc_host_check OK\n");
  return 0;
}
