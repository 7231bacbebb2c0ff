/* dclass_host_base — the host baseline of tools/dclass_bench.py: the partition of D-mask rows
 * (n rows of v0 bytes, as nemo_diff_masks_view hands them out) into classes of identical rows, on
 * one thread: a 64-bit hash of every row eight bytes at a time, an open-addressed table of the
 * classes' first rows, memcmp on a hash hit.  class_of[e] = class of row e, classes numbered by
 * first row.  Returns the number of classes (0 when out of memory).  Not part of libnemohip. */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

static uint64_t row_hash(const uint8_t *p, uint64_t n) {
  uint64_t h = 0x9E3779B97F4A7C15ull, w;
  uint64_t i = 0;
  for (; i + 8 <= n; i += 8) {
    memcpy(&w, p + i, 8);
    h = (h ^ w) * 0xBF58476D1CE4E5B9ull;
    h ^= h >> 29;
  }
  w = 0;
  if (i < n) memcpy(&w, p + i, n - i);
  h = (h ^ w) * 0x94D049BB133111EBull;
  return h ^ (h >> 31);
}

uint32_t dclass_host_partition(const uint8_t *masks, uint64_t n, uint64_t v0, uint32_t *class_of) {
  uint64_t cap = 16;
  while (cap < 2 * n) cap <<= 1;
  uint32_t *slot = (uint32_t *)malloc(cap * sizeof(uint32_t));  /* first row of a class + 1 */
  uint64_t *hs = (uint64_t *)malloc(cap * sizeof(uint64_t));
  uint32_t *cls = (uint32_t *)malloc((n ? n : 1) * sizeof(uint32_t));
  uint32_t k = 0;
  if (!slot || !hs || !cls) {
    free(slot), free(hs), free(cls);
    return 0;
  }
  memset(slot, 0, cap * sizeof(uint32_t));
  for (uint64_t e = 0; e < n; e++) {
    const uint8_t *row = masks + e * v0;
    const uint64_t h = row_hash(row, v0);
    uint64_t i = h & (cap - 1);
    for (;; i = (i + 1) & (cap - 1)) {
      if (!slot[i]) {
        slot[i] = (uint32_t)e + 1;
        hs[i] = h;
        cls[e] = k++;
        break;
      }
      if (hs[i] == h && !memcmp(masks + (uint64_t)(slot[i] - 1) * v0, row, v0)) {
        cls[e] = cls[slot[i] - 1];
        break;
      }
    }
    class_of[e] = cls[e];
  }
  free(slot), free(hs), free(cls);
  return k;
}
