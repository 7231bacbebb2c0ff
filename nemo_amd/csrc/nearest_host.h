// nearest_host.h — the host side of nemo_nearest_runs (k_near.hip; DESIGN.md §Nearest runs) as pure
// functions: the two lists' runs in, the distinct runs that get a bit row and the row of every list
// position out; the words of a row, the limits, and the tile / split-K grid of k_near_isect.  No HIP
// and no context, so tools/nearest_host_check.cpp drives it under the host sanitizers.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <unordered_map>
#include <vector>

namespace nearest {

#define NEAR_TILE 64u                    // k_near_isect: (query, candidate) positions per workgroup tile, each way
#define NEAR_SLAB 16u                    // ... and u64 words of a row per K-slab
#define NEAR_MAX_PAIRS (1ull << 30)      // n_q * n_c of one call
#define NEAR_MAX_BIT_BYTES (1ull << 36)  // the bit matrix of one call
#define NEAR_LDS_MAX 65536u              // largest row (bytes) k_near_bits builds in LDS: two workgroups per CU
#define NEAR_MAX_KSPLIT 1024u

// The distinct runs of a call, in first-appearance order (queries, then candidates): a run named in
// both lists, or several times in one, gets one row.
struct Rows {
  std::vector<uint32_t> run;         // [rows] the run of each bit row
  std::vector<uint32_t> qrow, crow;  // [n_q], [n_c] the row of every list position
};

static inline Rows rows(const uint32_t *q_run, size_t n_q, const uint32_t *c_run, size_t n_c) {
  Rows r;
  r.qrow.resize(n_q);
  r.crow.resize(n_c);
  std::unordered_map<uint32_t, uint32_t> seen;
  auto row_of = [&](uint32_t run) {
    auto ins = seen.emplace(run, (uint32_t)r.run.size());
    if (ins.second) r.run.push_back(run);
    return ins.first->second;
  };
  for (size_t i = 0; i < n_q; i++) r.qrow[i] = row_of(q_run[i]);
  for (size_t j = 0; j < n_c; j++) r.crow[j] = row_of(c_run[j]);
  return r;
}

// u64 words of a bit row that holds labels 0..lmax, rounded up to two words: rows are 16-byte aligned.
static inline uint64_t words_per_row(uint32_t lmax) {
  const uint64_t w = ((uint64_t)lmax + 1 + 63) / 64;
  return (w + 1) & ~1ull;
}

enum Limit { LIMIT_OK = 0, LIMIT_PAIRS = 1, LIMIT_BITS = 2 };

// The call's limits: n_q * n_c <= 2^30 (the matrix is indexed in 32 bits) and rows * W * 8 <= 2^36 bytes.
// Labels are interned (nemohip.h), so a corpus of a million labels takes 128 KB per row; the second
// limit is what a caller with sparse ids meets.
static inline Limit check_limits(uint64_t n_q, uint64_t n_c, uint64_t n_rows, uint64_t W) {
  if (n_q && n_c && (n_q > NEAR_MAX_PAIRS || n_c > NEAR_MAX_PAIRS / n_q)) return LIMIT_PAIRS;
  // n_rows <= 2^32 and W <= 2^26 + 2: the product has no 64-bit overflow
  if (n_rows * W > NEAR_MAX_BIT_BYTES / 8) return LIMIT_BITS;
  return LIMIT_OK;
}

// k_near_isect's grid: tq * tc tiles of NEAR_TILE x NEAR_TILE positions (blockIdx.x, query-major) and
// ksplit ranges of slabs_per_split K-slabs each (blockIdx.z).  The automatic split (force == 0) fills
// a device the tiles alone leave with fewer than two workgroups per CU; no range is empty.
struct Grid {
  uint64_t tq = 0, tc = 0;
  uint32_t slabs = 0, ksplit = 1, slabs_per_split = 0;
};

static inline Grid grid(uint64_t n_q, uint64_t n_c, uint64_t W, uint32_t n_cu, uint32_t force) {
  Grid g;
  g.tq = (n_q + NEAR_TILE - 1) / NEAR_TILE;
  g.tc = (n_c + NEAR_TILE - 1) / NEAR_TILE;
  g.slabs = (uint32_t)((W + NEAR_SLAB - 1) / NEAR_SLAB);
  const uint64_t tiles = g.tq * g.tc;
  uint64_t want = 1;
  if (force) want = force;
  else if (tiles && tiles < 2ull * n_cu) want = (2ull * n_cu + tiles - 1) / tiles;
  if (want > g.slabs) want = g.slabs;
  if (want > NEAR_MAX_KSPLIT) want = NEAR_MAX_KSPLIT;
  if (want < 1) want = 1;
  g.slabs_per_split = (uint32_t)((g.slabs + want - 1) / want);
  g.ksplit = g.slabs_per_split ? (g.slabs + g.slabs_per_split - 1) / g.slabs_per_split : 1;
  if (g.ksplit < 1) g.ksplit = 1;
  return g;
}

}  // namespace nearest
