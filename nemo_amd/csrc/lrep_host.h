// lrep_host.h — the arithmetic of nemo_lineage_repair_sets / nemo_lineage_repairs (k_lrepair.hip; DESIGN.md §Lineage
// repair search) as pure functions: k_lrep_lds's LDS image (the witness calls' image, a third u64 word per node for the
// stop rule, and the absent bitmap) and its tier, a workgroup's region on the global tier, the byte model of one staged
// graph, the limit of a u16 candidate position, and the status word of the two-hypothesis launch.  The keys, the rows'
// order, the tables, the emission buffer and the level's end are lin_host.h's; the validation of the two lists, the
// bitmap and the status rules are repair_host.h's.  No HIP and no context, so tools/lrepair_host_check.cpp drives it
// under the host sanitizers.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "lin_host.h"     // keys, LIN_MAX_CAND, size_ok, front_fits
#include "repair_host.h"  // check_lists, bitmap, bitmap_words, status
#include "wit_host.h"     // wit_lds_bytes, image_bytes

namespace lrep {

// k_lrep_lds's image: k_wit_lds's (the graph, the dead words, a second word per node: here the blame words), then the
// stop rule's word per node (bit h: the node is in F_h = A \ S_h, the chunk's seeds before the sweep), then the absent
// bitmap
KO_HD static inline uint32_t lrep_lds_bytes(uint32_t V, uint32_t E, uint32_t L) {
  return wit::wit_lds_bytes(V, E, L) + knock::ko_align(8u * V) + 8u * (uint32_t)repair::bitmap_words(V);
}
// where the three word arrays and the bitmap lie in the image, in bytes from its start (the dead words are first)
KO_HD static inline uint32_t blame_offset(uint32_t V, uint32_t E, uint32_t L) { return knock::knock_lds_bytes(V, E, L); }
KO_HD static inline uint32_t removed_offset(uint32_t V, uint32_t E, uint32_t L) { return wit::wit_lds_bytes(V, E, L); }
KO_HD static inline uint32_t bitmap_offset(uint32_t V, uint32_t E, uint32_t L) { return wit::wit_lds_bytes(V, E, L) + knock::ko_align(8u * V); }

// The LDS tier: u16 rows as k_ko_lds's, and an image of at most lds_max bytes (option wit_lds_max; 0: no graph).
static inline bool lds_fits(uint64_t V, uint64_t E, uint64_t L, uint32_t lds_max) {
  if (!lds_max || V >= 65536 || E > 65535 || L > V) return false;
  return lrep_lds_bytes((uint32_t)V, (uint32_t)E, (uint32_t)L) <= lds_max;
}

// a workgroup's region on the global tier, in u64: the dead, the blame and the stop rule's words (the bitmap is read
// where it lies)
KO_HD static inline uint64_t glob_words(uint64_t V) { return 3 * knock::dead_words(V); }

// the bytes a workgroup reads to stage one graph: the witness calls' image and the bitmap
static inline double image_bytes(double V, double E, double L) { return wit::image_bytes(V, E, L) + 8.0 * (double)repair::bitmap_words((uint64_t)V); }

// a set is eight u16 candidate positions: the explicit, the implicit and the device-made list alike
static inline bool cands_fit(uint64_t K) { return K <= LIN_MAX_CAND; }

// The two-hypothesis launch leaves the chunk's lost word (bit 0: S = {}, bit 1: S = cand); round 0's word of
// nemo_min_repair_sets, which repair::status reads, is "holds": its complement within the two bits.
static inline uint32_t status_of_lost(uint64_t lost) { return repair::status(~lost & 3ull); }

}  // namespace lrep
