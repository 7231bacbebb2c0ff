/* knockout_host_base — the single-thread host baseline of tools/knockout_bench.py: what a caller of the
 * library would write without nemo_knockout_leaves.  Per listed graph the forward CSR and a topological
 * order from the corpus' edge arrays, then the same bit-parallel sweep as the device's: 64 hypotheses per
 * u64 word, one word per node, children before parents (OR for a rule, AND for a goal with children).
 * Same inputs (the corpus arrays), same rows out.  Not part of libnemohip. */
#define _POSIX_C_SOURCE 199309L
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

static double now_s(void) {
  struct timespec t;
  clock_gettime(CLOCK_MONOTONIC, &t);
  return (double)t.tv_sec + 1e-9 * (double)t.tv_nsec;
}

/* node_off / edge_off [G + 1], word [V], src / dst [E] (local indices); graphs [n]: the listed graphs.
 * rows: [cap][5] graph, node, n_dead, roots_dead, n_roots, one per sink goal in node-index order, graphs in
 * list order; *n_rows the rows all listed graphs have (rows past cap are counted, not stored).  secs[0]: the
 * CSR and order builds, secs[1]: the sweeps and counts.  Returns 0, 1 when out of memory, 2 on a cycle. */
int knockout_host_rows(const uint64_t *node_off, const uint64_t *edge_off, const uint32_t *word, const uint32_t *src,
                       const uint32_t *dst, const uint32_t *graphs, uint64_t n, uint32_t *rows, uint64_t cap,
                       uint64_t *n_rows, double *secs) {
  uint64_t vmax = 0, emax = 0, out = 0;
  for (uint64_t i = 0; i < n; i++) {
    const uint32_t g = graphs[i];
    if (node_off[g + 1] - node_off[g] > vmax) vmax = node_off[g + 1] - node_off[g];
    if (edge_off[g + 1] - edge_off[g] > emax) emax = edge_off[g + 1] - edge_off[g];
  }
  uint32_t *fp = (uint32_t *)malloc((vmax + 2) * sizeof *fp), *fc = (uint32_t *)malloc((emax + 1) * sizeof *fc);
  uint32_t *indeg = (uint32_t *)malloc((vmax + 1) * sizeof *indeg), *order = (uint32_t *)malloc((vmax + 1) * sizeof *order);
  uint32_t *leaf = (uint32_t *)malloc((vmax + 1) * sizeof *leaf);
  uint64_t *dead = (uint64_t *)malloc((vmax + 1) * sizeof *dead);
  int rc = 0;
  secs[0] = secs[1] = 0;
  if (!fp || !fc || !indeg || !order || !leaf || !dead) {
    rc = 1;
    goto done;
  }
  for (uint64_t i = 0; i < n && !rc; i++) {
    const uint32_t g = graphs[i];
    const uint32_t V = (uint32_t)(node_off[g + 1] - node_off[g]);
    const uint64_t E = edge_off[g + 1] - edge_off[g];
    const uint32_t *w = word + node_off[g], *s = src + edge_off[g], *d = dst + edge_off[g];
    double t0 = now_s();
    /* forward CSR by a counting sort, in-degrees, Kahn order */
    memset(fp, 0, ((size_t)V + 2) * sizeof *fp);
    memset(indeg, 0, ((size_t)V + 1) * sizeof *indeg);
    for (uint64_t e = 0; e < E; e++) fp[s[e] + 2]++, indeg[d[e]]++;
    for (uint32_t v = 0; v < V; v++) fp[v + 2] += fp[v + 1];
    for (uint64_t e = 0; e < E; e++) fc[fp[s[e] + 1]++] = d[e];
    uint32_t head = 0, tail = 0, n_roots = 0, n_leaf = 0;
    for (uint32_t v = 0; v < V; v++) {
      if (!indeg[v]) order[tail++] = v, n_roots++;
      if (!(w[v] & 0x80000000u) && fp[v + 1] == fp[v]) leaf[n_leaf++] = v;
    }
    while (head < tail) {
      const uint32_t v = order[head++];
      for (uint32_t j = fp[v]; j < fp[v + 1]; j++)
        if (!--indeg[fc[j]]) order[tail++] = fc[j];
    }
    if (tail != V) rc = 2;
    double t1 = now_s();
    secs[0] += t1 - t0;
    for (uint32_t k0 = 0; k0 < n_leaf && !rc; k0 += 64) {
      const uint32_t nk = n_leaf - k0 < 64 ? n_leaf - k0 : 64;
      uint32_t cnt[64], rcnt[64];
      memset(dead, 0, (size_t)V * sizeof *dead);
      memset(cnt, 0, sizeof cnt);
      memset(rcnt, 0, sizeof rcnt);
      for (uint32_t b = 0; b < nk; b++) dead[leaf[k0 + b]] = 1ull << b;
      for (uint32_t i2 = V; i2-- > 0;) { /* children first */
        const uint32_t v = order[i2];
        const int rule = (w[v] & 0x80000000u) != 0;
        uint64_t acc = (rule || fp[v] == fp[v + 1]) ? 0 : ~0ull;
        for (uint32_t j = fp[v]; j < fp[v + 1]; j++) acc = rule ? acc | dead[fc[j]] : acc & dead[fc[j]];
        dead[v] |= acc;
        for (uint64_t x = dead[v]; x; x &= x - 1) cnt[__builtin_ctzll(x)]++;
      }
      for (uint32_t r = 0; r < n_roots; r++)
        for (uint64_t x = dead[order[r]]; x; x &= x - 1) rcnt[__builtin_ctzll(x)]++;
      for (uint32_t b = 0; b < nk; b++, out++) {
        if (out >= cap) continue;
        uint32_t *o = rows + 5 * out;
        o[0] = g, o[1] = leaf[k0 + b], o[2] = cnt[b], o[3] = rcnt[b], o[4] = n_roots;
      }
    }
    secs[1] += now_s() - t1;
  }
done:
  *n_rows = out;
  free(fp), free(fc), free(indeg), free(order), free(leaf), free(dead);
  return rc;
}
