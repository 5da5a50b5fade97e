// zpoly_plan.h -- host side of qh_apply_zpoly / qh_expect_zpoly (kernels_zpoly.hip.h): terms -> classes, groups and the
// device-side term block.  It reuses pauli_plan.h's item numbering, grid and sign split.
//
// Plain C++, no HIP: the engine calls it before every launch, qh_zpoly_plan hands the result to tools and tests, and
// tools/zpoly_plan_check.cc runs it stand-alone (with sanitizers) over random term lists.
//
// Terms arrive in the CALLER'S order with PHYSICAL local masks pz and weights with the shard's sign already folded in:
//   f(i) = sum_t w_t (-1)^popcount(i & pz_t)   over the amplitude indices i of the shard.
// The main kernel walks 16-byte items in chunks of 2^kPauliChunkBits items; the amplitude index is chunk << low_bits | low,
// low_bits = kPauliChunkBits + amp_bits.  By pauli_split_z a term is
//   CONST     pz == 0;
//   HIGH      bits in the chunk part only: a scalar per chunk;
//   LOW       bits in the low part only (half, thread, register index): a constant of the thread;
//   STRADDLE  both: sign_chunk(q) * sign_low(i).  Straddling terms with the same low mask form a GROUP (numbered in order of
//             first appearance): one scalar per chunk, g_L(q) = sum over the group of w_t sign_chunk_t(q).
// States below one chunk take the small kernel, which sums f by popcount over the terms as given: low_bits = nloc there.
//
// The device block (the host writes it, kernels only read it, uniformly): doubles wd[], then 64-bit words md[].
//   main:  SEGMENT 0 holds the CONST and HIGH terms, every further segment the terms of one group, each in the caller's order.
//          The groups are dealt to the segments by where their low mask lies, stably: first those on THREAD bits only (the sign
//          is one per thread and chunk: ngt of them), then those on register-index and half bits only (the sign is one per
//          (u, half) cell of the chunk, the same for every thread: ngu), then the mixed ones (a sign per amplitude).  A 2-local
//          cost function has single-bit low masks: no mixed group.
//          wd = segment weights (nseg_terms), then the LOW weights (nlow).
//          md = segoff[nseg + 1], the segment terms' chunk masks (nseg_terms), the groups' low masks (nseg; entry 0 unused),
//               the LOW terms' masks (nlow).
//   small: wd = w[nterms], md = pz[nterms].
#pragma once
#include <stdint.h>

#include <unordered_map>
#include <vector>

#include "pauli_plan.h"

namespace qh {

struct ZpolyTerm { double w; uint64_t pz; };

struct ZpolyPlan {
  int nloc = 0, amp_bits = 0, low_bits = 0;
  bool main = false;
  uint64_t nconst = 0, nhigh = 0, nlow = 0, nstraddle = 0;
  std::vector<uint8_t> cls;               // per term, caller's order: QH_ZPOLY_*
  std::vector<uint64_t> group_mask;       // the groups' low masks
  // the device block and where its parts start (indices into wd / md)
  std::vector<double> wd;
  std::vector<uint64_t> md;
  uint32_t nseg = 0, nseg_terms = 0, nterms = 0;
  uint32_t ngt = 0, ngu = 0;              // groups on thread bits only / on register-index and half bits only
  uint32_t off_lw = 0;                    // wd: LOW weights
  uint32_t off_sc = 0, off_gl = 0, off_lm = 0;      // md: chunk masks, group low masks, LOW masks (segoff is at 0)
  uint64_t nblk = 1;
  uint32_t cpb = 0;
  size_t bytes() const { return (wd.size() + md.size()) * 8; }
};

// the most a block can take: five words per term and a few more
constexpr size_t kZpolyBlockBytes = ((size_t)QH_ZPOLY_MAX_TERMS * 5 + 8) * 8;

inline uint32_t zpoly_class(uint64_t pz, int amp_bits, bool main) {
  if (pz == 0) return QH_ZPOLY_CONST;
  if (!main) return QH_ZPOLY_LOW;
  const PauliZSplit z = pauli_split_z(pz, amp_bits);
  const bool low = z.half || z.thread || z.reg, high = z.chunk != 0;
  return high ? (low ? QH_ZPOLY_STRADDLE : QH_ZPOLY_HIGH) : QH_ZPOLY_LOW;
}

inline void zpoly_plan(const ZpolyTerm *terms, uint64_t nterms, int nloc, int amp_bits, ZpolyPlan *p) {
  *p = ZpolyPlan{};
  p->nloc = nloc;
  p->amp_bits = amp_bits;
  p->main = pauli_main_shape(nloc, amp_bits);
  p->low_bits = p->main ? kPauliChunkBits + amp_bits : nloc;
  p->nterms = (uint32_t)nterms;
  p->cls.resize(nterms);
  const uint64_t low_mask = (1ull << p->low_bits) - 1ull;
  std::unordered_map<uint64_t, uint32_t> group_of;
  std::vector<uint32_t> seg(nterms, 0);      // segment of a CONST / HIGH / STRADDLE term
  for (uint64_t t = 0; t < nterms; ++t) {
    const uint32_t c = zpoly_class(terms[t].pz, amp_bits, p->main);
    p->cls[t] = (uint8_t)c;
    if (c == QH_ZPOLY_CONST) ++p->nconst;
    else if (c == QH_ZPOLY_HIGH) ++p->nhigh;
    else if (c == QH_ZPOLY_LOW) ++p->nlow;
    else {
      ++p->nstraddle;
      const uint64_t lm = terms[t].pz & low_mask;
      auto it = group_of.find(lm);
      if (it == group_of.end()) {
        it = group_of.emplace(lm, (uint32_t)p->group_mask.size()).first;
        p->group_mask.push_back(lm);
      }
      seg[t] = it->second + 1;
    }
  }
  if (!p->main) {
    const uint64_t n = 1ull << nloc;
    p->nblk = (n + 255) / 256;
    p->wd.resize(nterms);
    p->md.resize(nterms);
    for (uint64_t t = 0; t < nterms; ++t) {
      p->wd[t] = terms[t].w;
      p->md[t] = terms[t].pz;
    }
    return;
  }
  const PauliGrid g = pauli_grid(nloc, amp_bits);
  p->nblk = g.nblk;
  p->cpb = g.cpb;
  p->nseg = (uint32_t)p->group_mask.size() + 1;
  // group -> segment: thread-only masks, then register-index / half only, then mixed
  const uint64_t thread_bits = 255ull << amp_bits;
  auto kind = [&](uint64_t lm) { return (lm & ~thread_bits) == 0 ? 0 : (lm & thread_bits) == 0 ? 1 : 2; };
  std::vector<uint32_t> seg_of(p->group_mask.size());
  uint32_t next_seg = 1;
  for (int k = 0; k < 3; ++k)
    for (size_t g = 0; g < p->group_mask.size(); ++g)
      if (kind(p->group_mask[g]) == k) {
        seg_of[g] = next_seg++;
        if (k == 0) ++p->ngt;
        if (k == 1) ++p->ngu;
      }
  for (uint64_t t = 0; t < nterms; ++t)
    if (p->cls[t] == QH_ZPOLY_STRADDLE) seg[t] = seg_of[seg[t] - 1];
  p->nseg_terms = (uint32_t)(p->nconst + p->nhigh + p->nstraddle);
  p->off_lw = p->nseg_terms;
  p->off_sc = p->nseg + 1;
  p->off_gl = p->off_sc + p->nseg_terms;
  p->off_lm = p->off_gl + p->nseg;
  p->wd.assign((size_t)p->nseg_terms + p->nlow, 0.0);
  p->md.assign((size_t)p->off_lm + p->nlow, 0ull);
  // segment offsets: a counting sort that keeps the caller's order inside a segment
  std::vector<uint32_t> at(p->nseg + 1, 0);
  for (uint64_t t = 0; t < nterms; ++t)
    if (p->cls[t] != QH_ZPOLY_LOW) ++at[seg[t] + 1];
  for (uint32_t s = 0; s < p->nseg; ++s) at[s + 1] += at[s];
  for (uint32_t s = 0; s <= p->nseg; ++s) p->md[s] = at[s];
  uint32_t nl = 0;
  for (uint64_t t = 0; t < nterms; ++t) {
    if (p->cls[t] == QH_ZPOLY_LOW) {
      p->wd[p->off_lw + nl] = terms[t].w;
      p->md[p->off_lm + nl] = terms[t].pz;
      ++nl;
    } else {
      const uint32_t j = at[seg[t]]++;
      p->wd[j] = terms[t].w;
      p->md[p->off_sc + j] = terms[t].pz >> p->low_bits;
    }
  }
  for (size_t g = 0; g < p->group_mask.size(); ++g) p->md[p->off_gl + seg_of[g]] = p->group_mask[g];
}

// f at amplitude index i, rebuilt from the block's parts exactly as the kernels do (in the kernels' order)
inline double zpoly_eval_block(const ZpolyPlan &p, uint64_t i) {
  if (!p.main) {
    double f = 0.0;
    for (uint32_t t = 0; t < p.nterms; ++t) f += parity64(i & p.md[t]) ? -p.wd[t] : p.wd[t];
    return f;
  }
  const uint64_t q = i >> p.low_bits, low = i & ((1ull << p.low_bits) - 1ull);
  auto segsum = [&](uint32_t s) {
    double acc = 0.0;
    for (uint64_t j = p.md[s]; j < p.md[s + 1]; ++j) acc += parity64(q & p.md[p.off_sc + j]) ? -p.wd[j] : p.wd[j];
    return acc;
  };
  double lowsum = 0.0;
  for (uint64_t j = 0; j < p.nlow; ++j) lowsum += parity64(low & p.md[p.off_lm + j]) ? -p.wd[p.off_lw + j] : p.wd[p.off_lw + j];
  auto signed_seg = [&](uint32_t s) {
    const double c = segsum(s);
    return parity64(low & p.md[p.off_gl + s]) ? -c : c;
  };
  double base = segsum(0), cell = 0.0;      // per thread and chunk; per (u, half) cell and chunk
  for (uint32_t s = 1; s < 1 + p.ngt; ++s) base += signed_seg(s);
  for (uint32_t s = 1 + p.ngt; s < 1 + p.ngt + p.ngu; ++s) cell += signed_seg(s);
  double f = base + lowsum;
  if (p.ngu) f += cell;
  for (uint32_t s = 1 + p.ngt + p.ngu; s < p.nseg; ++s) f += signed_seg(s);
  return f;
}

}  // namespace qh
