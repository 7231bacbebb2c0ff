// load_host_check — runs the host-only parts of nemo_load_corpus (nemo_amd/csrc/load_host.h:
// load_validate and run 0's label tables) on three small corpora: an empty one, one without run 0
// and one whose run-0 post graph has duplicate goal labels.  Meant for the host sanitizers; it
// calls nothing on a device:
//   hipcc -x hip --offload-arch=gfx950 -std=c++17 -g -Wall -Wno-unused-result -Wno-unused-value \
//         -Xarch_host -fsanitize=address,undefined tools/load_host_check.cpp -o build/load_host_check
//   build/load_host_check
#include "../nemo_amd/csrc/load_host.h"

#include <cstdio>
#include <cstdlib>

#define CHECK(x)                                            \
  do {                                                      \
    if (!(x)) {                                             \
      fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #x); \
      exit(1);                                              \
    }                                                       \
  } while (0)

struct Corpus {
  std::vector<uint32_t> iteration, word, label, es, ed;
  std::vector<uint64_t> node_off{0}, edge_off{0};
  // a graph of goals with these labels and one rule behind each (goal -> rule edges)
  void graph(const std::vector<uint32_t> &labels) {
    const uint32_t n = (uint32_t)labels.size();
    for (uint32_t i = 0; i < n; i++) {
      word.push_back(1);
      label.push_back(labels[i]);
    }
    for (uint32_t i = 0; i < n; i++) {
      word.push_back(NEMO_NODE_RULE | 1);
      label.push_back(1000 + i);
      es.push_back(i);
      ed.push_back(n + i);
    }
    node_off.push_back(word.size());
    edge_off.push_back(es.size());
  }
  void run(uint32_t it, const std::vector<uint32_t> &pre, const std::vector<uint32_t> &post) {
    iteration.push_back(it);
    graph(pre);
    graph(post);
  }
  nemo_corpus view() const {
    nemo_corpus c{};
    c.n_runs = (uint32_t)iteration.size();
    c.n_tables = 4;
    c.table_pre = 0;
    c.table_post = 1;
    c.iteration = iteration.data();
    c.node_off = node_off.data();
    c.edge_off = edge_off.data();
    c.node_word = word.data();
    c.label = label.data();
    c.edge_src = es.data();
    c.edge_dst = ed.data();
    return c;
  }
};

static void check_tables(const nemo_ctx &c, const nemo_corpus &in, size_t n_goals, size_t n_distinct) {
  const R0Tables t = r0_tables(c.cs, &in);
  CHECK(t.l.size() == n_goals && t.ix.size() == n_goals);
  CHECK(std::is_sorted(t.l.begin(), t.l.end()));
  CHECK(t.hkey.size() >= 16 && (t.hkey.size() & (t.hkey.size() - 1)) == 0 && t.hkey.size() >= 2 * n_goals);
  size_t used = 0;
  for (uint32_t k : t.hkey) used += k != 0;
  CHECK(used == n_distinct);
  for (size_t i = 0; i < t.l.size(); i++) {  // every label is found, at its first sorted entry, with its count
    uint32_t h = hash_label(t.l[i]) & (uint32_t)(t.hkey.size() - 1);
    while (t.hkey[h] != t.l[i] + 1u) {
      CHECK(t.hkey[h] != 0);
      h = (h + 1) & (uint32_t)(t.hkey.size() - 1);
    }
    const size_t first = std::lower_bound(t.l.begin(), t.l.end(), t.l[i]) - t.l.begin();
    const size_t count = std::upper_bound(t.l.begin(), t.l.end(), t.l[i]) - t.l.begin() - first;
    CHECK(t.hval[h] == first);
    CHECK(t.dense.size() == (size_t)t.l.back() + 1);
    CHECK(t.dense[t.l[i]] == ((uint32_t)(first << 4) | (uint32_t)std::min<size_t>(count, 15)));
  }
  if (t.l.empty()) CHECK(t.dense.empty());
}

int main() {
  {  // an empty corpus: the offset arrays hold their one leading zero
    Corpus e;
    e.iteration.reserve(1);  // a non-null pointer to no runs
    const nemo_corpus in = e.view();
    nemo_ctx c;
    CHECK(load_validate(&c, &in) == NEMO_OK);
    CHECK(c.cs.G == 0 && c.cs.V == 0 && c.cs.E == 0 && c.cs.run0 == -1 && !c.cs.pairs_wide);
  }
  {  // no run 0
    Corpus k;
    k.run(3, {5, 6}, {7});
    k.run(4, {5}, {7, 8, 9});
    const nemo_corpus in = k.view();
    nemo_ctx c;
    CHECK(load_validate(&c, &in) == NEMO_OK);
    CHECK(c.cs.G == 4 && c.cs.run0 == -1 && c.cs.V == 14 && c.cs.E == 7 && c.cs.it2run.at(4) == 1);
    CHECK(c.cs.postV == 8 && c.cs.postE == 4);
  }
  {  // run 0 second, its post goals with duplicate labels (and label 0)
    Corpus k;
    k.run(2, {5}, {6});
    k.run(0, {5, 5}, {9, 0, 9, 4, 9, 0});
    const nemo_corpus in = k.view();
    nemo_ctx c;
    CHECK(load_validate(&c, &in) == NEMO_OK);
    CHECK(c.cs.run0 == 1);
    check_tables(c, in, 6, 3);
    // the same corpus with a duplicate iteration, with too many tables, without its arrays
    Corpus d = k;
    d.iteration[0] = 0;
    nemo_corpus bad = d.view();
    nemo_ctx c2;
    CHECK(load_validate(&c2, &bad) == NEMO_ERR_INVALID && c2.err.find("duplicate run iteration 0") != std::string::npos);
    bad = k.view();
    bad.n_tables = NEMO_MAX_TABLES + 1;
    CHECK(load_validate(&c2, &bad) == NEMO_ERR_LIMIT);
    bad = k.view();
    bad.node_word = nullptr;
    CHECK(load_validate(&c2, &bad) == NEMO_ERR_INVALID);
  }
  {  // run 0 with an empty post graph: empty tables of the smallest size
    Corpus k;
    k.run(0, {1}, {});
    const nemo_corpus in = k.view();
    nemo_ctx c;
    CHECK(load_validate(&c, &in) == NEMO_OK);
    check_tables(c, in, 0, 0);
  }
  puts("load_host_check OK");
  return 0;
}
