/* nearest_host_base — the single-thread host baseline of tools/nearest_bench.py: what a caller of the
 * library would write without nemo_nearest_runs.  Per run the sorted distinct labels of its post goals,
 * per (query, candidate) pair a merge of the two lists for the intersection, per query the argmin by
 * (dist, position) over the candidates of another run.  Same inputs (the corpus arrays), same rows out.
 * Not part of libnemohip. */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

static int cmp_u32(const void *a, const void *b) {
  const uint32_t x = *(const uint32_t *)a, y = *(const uint32_t *)b;
  return x < y ? -1 : x > y;
}

/* node_off [2 n_runs + 1], word / label [V]; q_run / c_run: run indices; out [4 n_q]: cand, dist, only_query,
 * only_cand (all UINT32_MAX: no candidate left).  Returns 0, or 1 when out of memory. */
int nearest_host_rows(const uint64_t *node_off, const uint32_t *word, const uint32_t *label, uint32_t n_runs,
                      const uint32_t *q_run, uint64_t n_q, const uint32_t *c_run, uint64_t n_c, uint32_t *out) {
  uint64_t *off = (uint64_t *)calloc((size_t)n_runs + 1, sizeof *off);
  if (!off) return 1;
  uint64_t total = 0;
  for (uint32_t r = 0; r < n_runs; r++) total += node_off[2 * r + 2] - node_off[2 * r + 1];
  uint32_t *lab = (uint32_t *)malloc((size_t)(total ? total : 1) * sizeof *lab);
  if (!lab) {
    free(off);
    return 1;
  }
  /* sorted distinct goal labels per run */
  for (uint32_t r = 0; r < n_runs; r++) {
    uint64_t n = 0;
    uint32_t *l = lab + off[r];
    for (uint64_t v = node_off[2 * r + 1]; v < node_off[2 * r + 2]; v++)
      if (!(word[v] & 0x80000000u)) l[n++] = label[v];
    qsort(l, (size_t)n, sizeof *l, cmp_u32);
    uint64_t k = 0;
    for (uint64_t i = 0; i < n; i++)
      if (!i || l[i] != l[i - 1]) l[k++] = l[i];
    off[r + 1] = off[r] + k;
  }
  for (uint64_t i = 0; i < n_q; i++) {
    const uint32_t *a = lab + off[q_run[i]];
    const uint64_t na = off[q_run[i] + 1] - off[q_run[i]];
    uint64_t best_d = ~0ull, best_j = 0, best_i = 0, best_nb = 0;
    for (uint64_t j = 0; j < n_c; j++) {
      if (c_run[j] == q_run[i]) continue;
      const uint32_t *b = lab + off[c_run[j]];
      const uint64_t nb = off[c_run[j] + 1] - off[c_run[j]];
      uint64_t x = 0, y = 0, both = 0;
      while (x < na && y < nb) {
        if (a[x] < b[y]) x++;
        else if (a[x] > b[y]) y++;
        else both++, x++, y++;
      }
      const uint64_t d = na + nb - 2 * both;
      if (d < best_d) best_d = d, best_j = j, best_i = both, best_nb = nb;
    }
    uint32_t *o = out + 4 * i;
    if (best_d == ~0ull) {
      o[0] = o[1] = o[2] = o[3] = 0xFFFFFFFFu;
    } else {
      o[0] = (uint32_t)best_j;
      o[1] = (uint32_t)best_d;
      o[2] = (uint32_t)(na - best_i);
      o[3] = (uint32_t)(best_nb - best_i);
    }
  }
  free(lab);
  free(off);
  return 0;
}
