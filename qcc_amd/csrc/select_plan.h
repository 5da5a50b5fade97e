// select_plan.h -- host side of qh_topk (kernels_select.hip.h): histograms of probability keys -> which key range holds the
// k-th largest entry, what to histogram next, when to stop.
//
// Plain C++, no HIP: the engine calls it between the passes, tools/select_plan_check.cc runs it stand-alone (with
// sanitizers) on synthetic histograms and checks the chosen ranges against a sort.
//
// A KEY is the bit pattern of a probability: a non-negative double, so keys order like the probabilities.  The search is a
// radix select from the most significant bits down.  Level 0 bins a key by its top 12 bits below the sign -- the 11
// exponent bits and the leading mantissa bit --, levels 1..4 by the next 12 bits each, level 5 by the last 3: 63 bits, so a
// bin of level 5 is one value.  Every histogram below level 0 counts only the keys under `prefix`, the boundary bins chosen
// so far.  Keys equal to 0 are never counted: an amplitude of probability 0 is not an entry.
//
// After each histogram sel_step says one of
//   kSelCollect  every key >= key_lo is a candidate, `candidates` of them, at most `cap`: one compaction pass, then the
//                host sorts and cuts at k;
//   kSelRefine   the boundary bin alone has too many: histogram it at the next level (the plan has moved on);
//   kSelTies     the boundary bin is ONE value, key_lo, and has too many: the `candidates` keys above it are collected by a
//                compaction pass (none if 0) and `ties_needed` of the `ties_total` entries that equal it are taken in
//                ascending logical index by the tie scan;
//   kSelEmpty    no nonzero amplitude.
#pragma once
#include <stdint.h>

namespace qh {

constexpr int kSelLevels = 6;
constexpr int kSelBinBits = 12;
constexpr uint32_t kSelBins = 1u << kSelBinBits;
constexpr uint64_t kSelKeyInf = 0x7ff0000000000000ull;      // keys above are NaNs

inline int sel_bits(int level) { return level < kSelLevels - 1 ? kSelBinBits : 63 - kSelBinBits * (kSelLevels - 1); }
inline int sel_shift(int level) { return level < kSelLevels - 1 ? 63 - kSelBinBits * (level + 1) : 0; }
// smallest and largest key of bin b at `level` under `prefix` (the key's bits above the level's field)
inline uint64_t sel_bin_lo(int level, uint64_t prefix, uint32_t b) { return ((prefix << sel_bits(level)) | b) << sel_shift(level); }
inline uint64_t sel_bin_hi(int level, uint64_t prefix, uint32_t b) {
  return sel_bin_lo(level, prefix, b) | ((1ull << sel_shift(level)) - 1ull);
}

struct SelPick {
  uint32_t bin;         // the bin that holds the need-th largest key; fewer keys than that: the lowest bin that has any
  uint64_t above;       // keys in the bins above it
  uint64_t in_bin;
  uint64_t total;
};
inline SelPick sel_pick(const uint64_t *hist, uint32_t nbins, uint64_t need) {
  SelPick p{0, 0, 0, 0};
  for (uint32_t b = 0; b < nbins; ++b) p.total += hist[b];
  uint64_t above = 0;
  for (uint32_t b = nbins; b-- > 0;) {
    if (!hist[b]) continue;
    p.bin = b;
    p.above = above;
    p.in_bin = hist[b];
    if (above + hist[b] >= need) break;
    above += hist[b];
  }
  return p;
}

struct SelPlan {
  int level = 0;
  uint64_t prefix = 0;      // the boundary bins of the levels above, most significant first
  uint64_t need = 0;        // entries still wanted from inside the range `prefix` names (1 <= need <= cap)
  uint64_t above = 0;       // keys above that range: all of them are in the answer (above < k)
  uint64_t cap = 0;         // candidates one compaction pass may hand to the host (>= k)
};
inline SelPlan sel_begin(uint64_t k, uint64_t cap) {
  SelPlan pl;
  pl.need = k;
  pl.cap = cap;
  return pl;
}

enum SelNext { kSelCollect = 0, kSelRefine = 1, kSelTies = 2, kSelEmpty = 3 };
struct SelStep {
  SelNext next;
  uint64_t key_lo;
  uint64_t candidates;
  uint64_t ties_needed, ties_total;
};
// hist: 1 << sel_bits(pl.level) counts of the keys under pl.prefix
inline SelStep sel_step(SelPlan &pl, const uint64_t *hist) {
  const SelPick pk = sel_pick(hist, 1u << sel_bits(pl.level), pl.need);
  SelStep s{kSelEmpty, 0, 0, 0, 0};
  if (pk.total == 0) return s;
  const uint64_t above_all = pl.above + pk.above;
  s.key_lo = sel_bin_lo(pl.level, pl.prefix, pk.bin);
  if (above_all + pk.in_bin <= pl.cap) {
    s.next = kSelCollect;
    s.candidates = above_all + pk.in_bin;
    return s;
  }
  if (pl.level == kSelLevels - 1) {
    s.next = kSelTies;
    s.candidates = above_all;
    s.ties_needed = pl.need - pk.above;
    s.ties_total = pk.in_bin;
    return s;
  }
  s.next = kSelRefine;
  pl.above = above_all;
  pl.need -= pk.above;
  pl.prefix = (pl.prefix << sel_bits(pl.level)) | pk.bin;
  pl.level++;
  return s;
}

// Tie scan: the first range of LOGICAL indices to look at, when `total` of the n amplitudes equal the value and `need` of
// them are wanted -- twice the length that holds `need` at the average density, at least `floor_len`, at most n.
inline uint64_t sel_tie_first_len(uint64_t n, uint64_t total, uint64_t need, uint64_t floor_len) {
  const double len = 2.0 * (double)need * ((double)n / (double)(total ? total : 1));
  if (len >= (double)n) return n;
  const uint64_t l = (uint64_t)len;
  return l < floor_len ? (floor_len < n ? floor_len : n) : l;
}

}  // namespace qh
