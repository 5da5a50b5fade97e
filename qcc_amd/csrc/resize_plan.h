// resize_plan.h -- host side of qh_extend and qh_release (kernels_resize.hip.h): the bit map of the new handle and, for a
// release, how a source index is squeezed into a destination index.
//
// Plain C++, no HIP: the engine calls it before every launch (and instead of one, on planner-only handles), and
// tools/resize_plan_check.cc runs it stand-alone (with sanitizers) against a bit-by-bit model.
//
// qh_extend (k new qubits): nothing of the source moves.  The new logical bits 0..k-1 sit at physical positions
// nloc..nloc+k-1, logical bit b becomes b + k, a local position stays, a position held by the shard index moves up by k.
//
// qh_release (k listed logical bits, all local): the survivors keep their order, logically and physically, and are
// renumbered densely -- logical l becomes l - |released logical bits below l|, physical p becomes p - |released positions
// below p| (the positions of the shard index all move down by k).  The released positions R cut the local positions into
// at most k + 1 runs of survivors; run s is a mask of adjacent positions and the number of released positions below it, so
// the destination of a kept source index p is the OR over the runs of (p & mask[s]) >> shift[s].
#pragma once
#include <stdint.h>
#include <string.h>

namespace qh {

constexpr int kMaxResizeBits = 16;                   // qubits added or released per call
constexpr int kResizeMaxSegs = kMaxResizeBits + 1;   // runs of surviving positions
constexpr int kResizeMaxGlobalBits = 62;             // what qh_set_shard accepts

// perm: physical position of each of the nglob logical bits (entries from nglob on are ignored).  perm_out gets 64 entries:
// the nglob + k of the new handle, the identity above them.
inline void plan_extend(int nloc, int nglob, const int *perm, int k, int *perm_out) {
  for (int b = 0; b < 64; ++b) perm_out[b] = b;
  for (int j = 0; j < k; ++j) perm_out[j] = nloc + j;
  for (int b = 0; b < nglob; ++b) perm_out[b + k] = perm[b] < nloc ? perm[b] : perm[b] + k;
}

struct ReleasePlan {
  int perm[64];              // the new handle's bit map (identity from its nglob on)
  uint64_t drop;             // R: the released physical positions (all local)
  uint64_t want;             // V: the value a kept index has under R
  int nseg;                  // runs of surviving local positions, ascending
  uint64_t mask[kResizeMaxSegs];
  uint8_t shift[kResizeMaxSegs];
};

// bits: k distinct logical bits in [0, nglob), 1 <= k <= kMaxResizeBits and k < nloc (the caller has checked); bit j of
// `value` is the value required of bits[j].  Returns -1 and fills *out, or the first j whose bit the shard index holds.
inline int plan_release(int nloc, int nglob, const int *perm, int k, const int32_t *bits, uint64_t value, ReleasePlan *out) {
  memset(out, 0, sizeof *out);
  uint64_t rlog = 0;
  for (int j = 0; j < k; ++j) {
    const int p = perm[bits[j]];
    if (p >= nloc) return j;
    rlog |= 1ull << bits[j];
    out->drop |= 1ull << p;
    if ((value >> j) & 1ull) out->want |= 1ull << p;
  }
  for (int b = 0; b < 64; ++b) out->perm[b] = b;
  for (int l = 0; l < nglob; ++l) {
    if ((rlog >> l) & 1ull) continue;
    const int p = perm[l];
    out->perm[l - __builtin_popcountll(rlog & ((1ull << l) - 1ull))] = p - __builtin_popcountll(out->drop & ((1ull << p) - 1ull));
  }
  for (int p = 0; p < nloc;) {
    if ((out->drop >> p) & 1ull) {
      ++p;
      continue;
    }
    int e = p;
    while (e < nloc && !((out->drop >> e) & 1ull)) ++e;
    out->mask[out->nseg] = ((1ull << e) - 1ull) & ~((1ull << p) - 1ull);
    out->shift[out->nseg++] = (uint8_t)__builtin_popcountll(out->drop & ((1ull << p) - 1ull));
    p = e;
  }
  return -1;
}

// the destination index of a source index (whatever it holds under R)
inline uint64_t release_squeeze(const ReleasePlan &r, uint64_t p) {
  uint64_t d = 0;
  for (int s = 0; s < r.nseg; ++s) d |= (p & r.mask[s]) >> r.shift[s];
  return d;
}

}  // namespace qh
