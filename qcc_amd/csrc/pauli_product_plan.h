// pauli_product_plan.h -- host side of qh_apply_pauli_product (kernels_pauli_product.hip.h): terms -> runs, and the pair
// addressing of the run kernel.  The sibling of pauli_plan.h, whose item numbering, sign split and coefficient folding it reuses.
//
// Plain C++, no HIP: the engine calls it before every launch, qh_pauli_product_plan hands the runs to tools and tests, and
// tools/pauli_product_plan_check.cc runs it stand-alone (with sanitizers) over random masks.
//
// Terms arrive in the CALLER'S order with PHYSICAL local masks (px, pz), the sign the shard index gives (neg) and nY mod 4.
// A factor a I + b P with x mask px touches the disjoint pairs {i, i ^ px}; factors whose x masks are 0 or one common X act
// on the same pairs.  pauli_product_cut walks the terms in order and keeps the run's pair mask X (0 while every term so far
// is diagonal): a term joins if the run has fewer than kPauliProdT terms and px == 0, X == 0 or px == X.  One kernel per run.
//
// Pair addressing (16-byte items as in pauli_plan.h; amp_bits index bits inside an item).  With xi = X >> amp_bits and p its
// top set bit, pair number w names item0 = w with a 0 inserted at bit p, and item1 = item0 ^ xi.  Pair numbers are laid out
// like pauli_plan.h's item numbers: chunk << kPauliChunkBits | u << 8 | thread.  At complex64 an item holds two amplitudes:
// (item0, half) pairs with (item1, half ^ (X & 1)).  X == 1 at complex64 has xi == 0: the pair is the two halves of one item
// (QH_PAULI_RUN_HALF) and the kernel walks items.  A PAIR run whose pivot lies inside the 128-byte line walks items too
// (pauli_pair_in_wave below).
//
// Signs for a pair walk: item0 has bit p clear, so popcount(item0 & zi) = popcount(w & zw), zw = zi with bit p removed
// (pauli_pair_z), and pauli_split_z applies to w as it does to an item number.  The partner's sign differs from its own by
// the constant parity(X & pz).
#pragma once
#include <stdint.h>

#include "pauli_plan.h"

namespace qh {

// Two compile-time switches for A/B builds of the engine (tools/bench_pauli_product.py's header has the command line; the
// rows that decided the defaults are profiles/pauli_product/bench_pauli_product_slots16_nolane.txt).  The plan and the kernels
// both follow them, so such a build is consistent in itself; the package is built with neither set.
#ifndef QH_PAULI_PRODUCT_SLOTS
#define QH_PAULI_PRODUCT_SLOTS QH_PAULI_PRODUCT_BATCH
#endif
#ifndef QH_PAULI_LANE_PIVOT_MAX
#define QH_PAULI_LANE_PIVOT_MAX 2      // -1: no in-wave walk
#endif

constexpr int kPauliProdT = QH_PAULI_PRODUCT_SLOTS;      // terms per run
constexpr int kPauliProdMidT = 8;                        // (a build with 16 slots keeps an 8-slot instantiation beside them)
constexpr int kPauliProdSmallT = 4;                      // ... of the smaller instantiation

// the main shape needs a whole chunk of PAIRS (whatever the kind); smaller states take the one-pair-per-thread kernel
constexpr bool pauli_product_main_shape(int nloc, int amp_bits) { return nloc - amp_bits - 1 >= kPauliChunkBits; }
// the walk of a run: pair numbers (half as many as items) for PAIR with a pivot outside the line, item numbers otherwise
constexpr PauliGrid pauli_product_grid(int nloc, int amp_bits, bool pair_walk) { return pauli_grid(pair_walk ? nloc - 1 : nloc, amp_bits); }

// How a PAIR run is walked.  A pivot inside a 128-byte line (item bit <= kPauliLanePivotMax) would split every line between the
// two loads of a pair walk (measured at 30 qubits: 3.2 x a memory pass).  Such runs walk ITEMS instead, as DIAG does: the partner
// item ^ (X >> amp_bits) differs in lane bits only, so it sits in another lane of the same wave and arrives by a lane exchange;
// each thread updates both values of its pair and stores its own.  Loads and stores are then lane-linear.
constexpr int kPauliLanePivotMax = QH_PAULI_LANE_PIVOT_MAX;
constexpr int kPauliWalkLane = 3;      // the kernel's KIND for it, beside QH_PAULI_RUN_*: not a kind of the plan, which says PAIR
constexpr bool pauli_pair_in_wave(uint64_t X, int amp_bits) {
  return (X >> amp_bits) != 0 && 63 - __builtin_clzll(X >> amp_bits) <= kPauliLanePivotMax;
}

constexpr uint32_t pauli_run_kind(uint64_t X, int amp_bits) {
  return X == 0 ? (uint32_t)QH_PAULI_RUN_DIAG : (amp_bits && X == 1ull) ? (uint32_t)QH_PAULI_RUN_HALF : (uint32_t)QH_PAULI_RUN_PAIR;
}

// the top set bit of the item part of X (X >> amp_bits must not be 0)
constexpr int pauli_pair_pivot(uint64_t X, int amp_bits) { return 63 - __builtin_clzll(X >> amp_bits); }
constexpr uint64_t pauli_insert0(uint64_t w, int p) { return ((w >> p) << (p + 1)) | (w & ((1ull << p) - 1ull)); }
constexpr uint64_t pauli_remove_bit(uint64_t v, int p) { return ((v >> (p + 1)) << p) | (v & ((1ull << p) - 1ull)); }
constexpr uint64_t pauli_pair_item0(uint64_t w, int p) { return pauli_insert0(w, p); }
constexpr uint64_t pauli_pair_item1(uint64_t item0, uint64_t X, int amp_bits) { return item0 ^ (X >> amp_bits); }
// pz (amplitude bits) as a mask over (pair number << amp_bits | half): the item part loses bit p
constexpr uint64_t pauli_pair_z(uint64_t pz, int p, int amp_bits) {
  return (pauli_remove_bit(pz >> amp_bits, p) << amp_bits) | (amp_bits ? (pz & 1ull) : 0ull);
}
// 1: the partner's sign is the opposite of its own
constexpr uint32_t pauli_pair_flip(uint64_t X, uint64_t pz) { return parity64(X & pz); }

// terms in the caller's order -> runs; writes at most cap of them and returns their number
inline uint64_t pauli_product_cut(const qh_pauli_term *terms, uint64_t nterms, int amp_bits, qh_pauli_run *out, uint64_t cap) {
  uint64_t nr = 0, first = 0, X = 0;
  auto close = [&](uint64_t end) {
    if (nr < cap && out) out[nr] = qh_pauli_run{first, end - first, X, pauli_run_kind(X, amp_bits), 0u};
    ++nr;
  };
  for (uint64_t t = 0; t < nterms; ++t) {
    const uint64_t px = terms[t].px;
    const bool joins = t - first < (uint64_t)kPauliProdT && (px == 0 || X == 0 || px == X);
    if (!joins) {
      close(t);
      first = t;
      X = 0;
    }
    if (px) X = px;
  }
  if (nterms) close(nterms);
  return nr;
}

}  // namespace qh
