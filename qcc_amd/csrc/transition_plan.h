// transition_plan.h -- host side of qh_transition_pauli (kernels_transition.hip.h): two bit maps and a list of Pauli strings
// -> the walk over the two states, the terms on the two layouts, and the passes.
//
// Plain C++, no HIP: the engine calls it before every launch, qh_transition_plan hands the result to tools and tests, and
// tools/transition_plan_check.cc runs it stand-alone (with sanitizers) over random bit maps and term lists.
//
//   <a|P|b> = (-i)^nY sum_i (-1)^popcount(i & z) conj(a_i) b_{i ^ x}          (i, x, z over LOGICAL bits)
// The walk is the one inner_plan.h finds for (a, b): it matches a_i with b_i.  The partner b_{i ^ x} is reached by XORing
// b's amplitude index with x in B's physical positions (px); the sign is a parity over a's physical index with z in A's
// positions (pz).  A z bit the shard index holds is a sign fixed on this shard (neg); an x bit there would need another
// shard's amplitudes and is refused.  Terms are stably sorted by their LOGICAL x mask (px is a bijective image of it, so
// a group shares px) and every group is cut each transition_batch(width) terms: one pass, one kernel, one read of each
// state.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <numeric>
#include <vector>

#include "../../include/qcc_hip.h"
#include "inner_plan.h"
#include "pauli_plan.h"

namespace qh {

constexpr int kTransT = QH_TRANSITION_BATCH;      // strings per pass at complex128
constexpr int kTransT64 = 8;                      // ... at complex64 (DESIGN.md "Matrix elements between two states": why)
constexpr int kTransSmallT = 4;                   // ... of the smaller instantiation, either width
static_assert(kTransT64 <= kTransT && kTransSmallT <= kTransT64, "QH_TRANSITION_BATCH is the largest batch");
constexpr int transition_batch(int bit_width) { return bit_width == 128 ? kTransT : kTransT64; }

// why plan_transition refused: the first offending term and logical bit (where there is one)
struct TransitionRefusal {
  enum Kind { kNone, kMaskRange, kShardIndex, kSplitBit, kXHeld } kind = kNone;
  uint64_t term = 0;
  int bit = -1;
};

// a mask over logical bits -> the mask over physical positions
inline uint64_t transition_to_phys(int nglob, const int *perm, uint64_t logical) {
  uint64_t p = 0;
  for (int l = 0; l < nglob; ++l)
    if ((logical >> l) & 1ull) p |= 1ull << perm[l];
  return p;
}

// perm_a / perm_b: physical position of each of the nglob logical bits; positions >= nloc are bits of the shard index.
// Returns QH_OK and fills walk, terms (sorted order) and passes, or QH_ERR_BAD_QUBIT / QH_ERR_NONLOCAL and *why; the WHOLE
// list is checked before anything is filled in.
inline int plan_transition(int nloc, int nglob, int bit_width, const int *perm_a, const int *perm_b, uint64_t shard_a, uint64_t shard_b,
                           uint64_t nterms, const uint64_t *xmask, const uint64_t *zmask, qh_inner_tiles *walk,
                           std::vector<qh_pauli_term> *terms, std::vector<qh_transition_pass> *passes, TransitionRefusal *why) {
  *why = TransitionRefusal{};
  if (nglob < 64)
    for (uint64_t t = 0; t < nterms; ++t)
      if ((xmask[t] | zmask[t]) >> nglob) {
        *why = {TransitionRefusal::kMaskRange, t, -1};
        return QH_ERR_BAD_QUBIT;
      }
  if (shard_a != shard_b) {
    *why = {TransitionRefusal::kShardIndex, 0, -1};
    return QH_ERR_NONLOCAL;
  }
  const int split = plan_inner(nloc, nglob, perm_a, perm_b, walk);
  if (split >= 0) {
    *why = {TransitionRefusal::kSplitBit, 0, split};
    return QH_ERR_NONLOCAL;
  }
  const uint64_t local = nloc >= 64 ? ~0ull : (1ull << nloc) - 1ull;
  std::vector<qh_pauli_term> placed(nterms);
  for (uint64_t t = 0; t < nterms; ++t) {
    const uint64_t x = transition_to_phys(nglob, perm_b, xmask[t]), z = transition_to_phys(nglob, perm_a, zmask[t]);
    if (x & ~local) {
      int l = 0;      // the first logical bit of them
      while (!((xmask[t] >> l) & 1ull) || perm_b[l] < nloc) ++l;
      *why = {TransitionRefusal::kXHeld, t, l};
      return QH_ERR_NONLOCAL;
    }
    placed[t] = qh_pauli_term{t, x, z & local, parity64(shard_a & (z >> nloc)), (uint32_t)__builtin_popcountll(xmask[t] & zmask[t]) & 3u};
  }
  std::vector<uint64_t> order(nterms);
  std::iota(order.begin(), order.end(), 0ull);
  std::stable_sort(order.begin(), order.end(), [&](uint64_t l, uint64_t r) { return xmask[l] < xmask[r]; });
  terms->resize(nterms);
  for (uint64_t k = 0; k < nterms; ++k) (*terms)[k] = placed[order[k]];
  passes->clear();
  const uint64_t batch = (uint64_t)transition_batch(bit_width);
  for (uint64_t first = 0; first < nterms;) {
    uint64_t count = 1;
    while (first + count < nterms && count < batch && (*terms)[first + count].px == (*terms)[first].px) ++count;
    passes->push_back(qh_transition_pass{first, count, (*terms)[first].px, walk->path, 0u});
    first += count;
  }
  return QH_OK;
}

// The parts of a term's sign the kernels take (kernels_transition.hip.h); their XOR over an amplitude is the parity of
// (a's physical index & pz).
struct TransZSplit {
  uint64_t uniform;    // over the chunk number (linear) or the tile number (tiles)
  uint32_t reg;        // linear: bit u = parity of z over the register-index part u
  uint32_t thread;     // over the thread index: item bits 0-7 (linear), in-tile index (tiles), the amplitude index (gather)
  uint32_t half;       // linear at complex64: z on the sub-item bit
};
// linear walk: item = amplitude index >> amp_bits = chunk << cw | u << 8 | thread, kLoads = 8 items per thread and chunk
inline TransZSplit transition_split_linear(uint64_t pz, int amp_bits) {
  const PauliZSplit z = pauli_split_z(pz, amp_bits);      // (the same item numbering: kPauliPer == kInnerLoads)
  return {z.chunk, z.reg, z.thread, z.half};
}
// tiles walk: a's index = tile number spread over rest_a | in-tile index spread over tile_a
inline TransZSplit transition_split_tiles(uint64_t pz, const qh_inner_tiles &w) {
  TransZSplit s{};
  for (uint32_t k = 0; k < w.nrest; ++k) s.uniform |= ((pz >> w.rest_a[k]) & 1ull) << k;
  for (int k = 0; k < kInnerTileBits; ++k) s.thread |= (uint32_t)((pz >> w.tile_a[k]) & 1ull) << k;
  return s;
}

}  // namespace qh
