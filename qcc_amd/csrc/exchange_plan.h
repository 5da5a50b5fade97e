// exchange_plan.h -- host side of the multi-GPU exchange (exchange.hip.h, engine.hip do_exchange): how one exchange is cut
// into slabs and rounds, where each round's amplitudes lie, the signature the ranks compare and the qh_xgeom record.
//
// Plain C++, no HIP or RCCL: the engine calls plan_exchange() once per exchange -- on real handles and on planner-only
// ones alike -- and both transports take every offset from the plan; tools/exchange_plan_check.cc runs the plan's rounds
// stand-alone (with sanitizers) on host arrays against a bit-by-bit model.
//
// An exchange moves BLOCKS: the amplitudes of the shard whose g block bits (the local positions pos[0..g)) hold a given
// value.  The shard's other local bits are SLAB bits (fixed per slab: up to kMaxSlabBits, see exchange.hip.h "overlap")
// and FREE bits; round ci of a slab moves, for every peer, the 2^chunk_bits amplitudes whose free bits count from
// ci << chunk_bits.  Two ways to move a round:
//   DIRECT  the blocks are contiguous runs of the shard, sent from where they lie and copied home from the staging
//           area -- when the low free bits give runs of a whole chunk (or 16 MiB);
//   PACKED  a gather kernel packs each peer's amplitudes of the round into the staging area, a scatter kernel puts the
//           received ones in place -- whatever the layout (after relayout sweeps the blocks' bits may sit anywhere above
//           the 128-byte line).
#pragma once
#include <stdint.h>
#include <stdlib.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/qcc_hip.h"

namespace qh {

constexpr int kMaxXferMoves = 63;      // peers per round (XferGeom::off, exchange.hip.h)
constexpr int kMaxExchangeBits = 8;    // block bits of one exchange
constexpr int kExchangeSlabBits = 3;   // == kMaxSlabBits (planner.h; static_assert in kernels_sweep.hip.h)
constexpr int kExchangeMaxIns = 15;    // == kMaxIns (kernels_gate.hip.h; static_assert in exchange.hip.h)

// The blocks one exchange moves: block value `blk` of the g bits at `base` goes to `peer`, and
// that peer's data lands in block value `land` (== blk except in the loop-back self test).
struct BlockMove { int peer, blk, land; };

// Picks up to `want` slab bits: the highest local bits outside `avoid`.
inline uint64_t pick_slab_bits(int nloc, uint64_t avoid, int want, int min_bit) {
  uint64_t m = 0;
  for (int b = nloc - 1; b >= min_bit && want > 0; --b)
    if (!((avoid >> b) & 1ull)) { m |= 1ull << b; --want; }
  return m;
}

// deposit the low bits of v into the set bits of mask (ascending)
inline uint64_t deposit_bits(uint64_t v, uint64_t mask) {
  uint64_t out = 0;
  for (uint64_t m = mask; m; m &= m - 1) {
    const int b = __builtin_ctzll(m);
    out |= (v & 1ull) << b;
    v >>= 1;
  }
  return out;
}

// The exchange's switches, read by from_env() once per exchange on the calling thread (tests change them in-process);
// nothing below reads the environment.  QH_EXCHANGE_VERIFY is not here: engine.hip reads it once per process.
struct ExchangeSwitches {
  int slab_bits_asked = kExchangeSlabBits;   // QH_EXCHANGE_SLAB_BITS as written: what the ranks' signature covers
  int slab_bits = kExchangeSlabBits;         // ... clamped to 0..kMaxSlabBits: what the exchange uses (UnitPerm::slab_pos)
  int pack = -1;                             // QH_EXCHANGE_PACK (tests): 1 = always packed, 0 = never, unset = by the layout

  static ExchangeSwitches from_env() {
    ExchangeSwitches w;
    if (const char *e = getenv("QH_EXCHANGE_SLAB_BITS")) w.slab_bits_asked = atoi(e);
    w.slab_bits = std::max(0, std::min(w.slab_bits_asked, kExchangeSlabBits));
    if (const char *e = getenv("QH_EXCHANGE_PACK")) w.pack = atoi(e);
    return w;
  }
  // (the EFFECTIVE values: an unset switch and one set to its default are the same exchange)
  std::string key() const { return std::to_string(slab_bits_asked) + ";" + std::to_string(pack) + ";"; }
};

struct ExchangePlan {
  int nloc = 0, gbits = 0, np = 0;   // local bits, block bits, moves (peers per round)
  uint64_t amp_bytes = 16;
  int pos[kMaxExchangeBits] = {0};   // where the blocks' bits live (bit k of a block value sits at pos[k])
  uint64_t block_bits = 0;
  uint64_t slab_mask = 0;
  std::vector<uint64_t> slab_vals;   // slab k's value under slab_mask
  uint64_t free_mask = 0;            // the local bits a slab's rounds count through
  int chunk_bits = 0;                // log2(amplitudes per peer and round)
  uint64_t rounds_per_slab = 0;
  bool packed = false;
  // staging: [2 receive halves][2 send halves (packed only)] of (peers x chunk) amplitudes
  uint64_t half_bytes = 0, staging_bytes = 0;
  // packed rounds: the block and slab bits, ascending -- the positions the gather / scatter kernels insert zeros at (BitIns)
  int nins = 0;
  int ins_pos[64] = {0};

  int slabs() const { return (int)slab_vals.size(); }
  uint64_t chunk_amps() const { return 1ull << chunk_bits; }
  uint64_t chunk_bytes() const { return chunk_amps() * amp_bytes; }
  // shard offset of block value v (its other bits zero)
  uint64_t block_offset(int v) const {
    uint64_t o = 0;
    for (int k = 0; k < gbits; ++k) if ((v >> k) & 1) o |= 1ull << pos[k];
    return o;
  }
  // DIRECT: block value v's amplitudes of round ci in slab k are the chunk_amps() consecutive ones from
  // round_offset(k, ci) | block_offset(v)
  uint64_t round_offset(int k, uint64_t ci) const { return deposit_bits(ci << chunk_bits, free_mask) | slab_vals[k]; }
  // PACKED: amplitude j of that round is expand_index(round_start(ci) + j, ins) | packed_offset(k, v)
  uint64_t round_start(uint64_t ci) const { return ci << chunk_bits; }
  uint64_t packed_offset(int k, int v) const { return block_offset(v) | slab_vals[k]; }
};

// pos[0..gbits): the positions of the block bits in the layout the flush left; np: moves; chunk_amps: amplitudes per peer and
// round asked for (0 = 2^22).  flushed_vals: the slabs the flush cut its last sweep into, under flushed_mask -- or nullptr
// (nothing was queued, or the last sweep could not be cut): the plan then picks slab bits itself, because slabs still let
// the NEXT sweep start early.
inline ExchangePlan plan_exchange(int nloc, const int *pos, int gbits, uint64_t chunk_amps, int np, uint64_t amp_bytes,
                                  const ExchangeSwitches &sw, uint64_t flushed_mask, const std::vector<uint64_t> *flushed_vals) {
  ExchangePlan p;
  p.nloc = nloc, p.gbits = gbits, p.np = np, p.amp_bytes = amp_bytes;
  for (int k = 0; k < gbits; ++k) { p.pos[k] = pos[k]; p.block_bits |= 1ull << pos[k]; }
  if (flushed_vals) {
    p.slab_mask = flushed_mask;
    p.slab_vals = *flushed_vals;
  } else {
    if (sw.slab_bits > 0)
      p.slab_mask = pick_slab_bits(nloc, p.block_bits | 7ull, std::min(sw.slab_bits, std::max(0, nloc - gbits - 10)), 6);
    for (int k = 0; k < (1 << __builtin_popcountll(p.slab_mask)); ++k) p.slab_vals.push_back(deposit_bits((uint64_t)k, p.slab_mask));
  }
  const uint64_t local_mask = nloc >= 64 ? ~0ull : (1ull << nloc) - 1ull;
  p.free_mask = local_mask & ~p.block_bits & ~p.slab_mask;
  const int nfree = __builtin_popcountll(p.free_mask);
  const int run_bits = (~p.free_mask) ? __builtin_ctzll(~p.free_mask) : 64;
  if (!chunk_amps) chunk_amps = 1ull << 22;
  int want_bits = 0;
  while ((2ull << want_bits) <= chunk_amps && want_bits + 1 <= nfree) want_bits++;
  p.packed = sw.pack >= 0 ? sw.pack != 0 : run_bits < std::min(want_bits, 20);   // direct: whole chunks, or runs of >= 16 MiB
  p.chunk_bits = p.packed ? want_bits : std::min(want_bits, run_bits);
  p.rounds_per_slab = 1ull << (nfree - p.chunk_bits);
  p.half_bytes = (uint64_t)np * p.chunk_bytes();
  p.staging_bytes = (p.packed ? 4 : 2) * p.half_bytes;
  for (int b = 0; b < nloc; ++b) if (!((p.free_mask >> b) & 1ull)) p.ins_pos[p.nins++] = b;
  return p;
}

// Every rank must cut an exchange the same way; this is what they compare (engine.hip verify_geometry).  perm: the handle's
// bit map after the flush (position of each of the nglob logical bits); base: the first logical block bit; env_build: the
// hash of the switches and the build (engine.hip env_build_hash).  The order of the mixing is the value.
inline uint64_t exchange_signature(const ExchangePlan &p, const int *perm, int nglob, int base, int bw, uint64_t env_build) {
  uint64_t sig = 0x9e3779b97f4a7c15ull;
  auto mix = [&](uint64_t v) { sig ^= v + 0x9e3779b97f4a7c15ull + (sig << 6) + (sig >> 2); };
  for (int b = 0; b < nglob; ++b) mix((uint64_t)perm[b]);
  mix(p.slab_mask); mix((uint64_t)p.chunk_bits); mix(p.rounds_per_slab); mix(p.packed); mix((uint64_t)p.slabs()); mix(p.block_bits);
  mix((uint64_t)base); mix((uint64_t)p.gbits);
  for (uint64_t v : p.slab_vals) mix(v);
  mix((uint64_t)p.np); mix((uint64_t)bw); mix(env_build);
  return sig;
}

inline qh_xgeom exchange_record(const ExchangePlan &p, uint64_t signature, uint32_t sweeps_before, bool last_sweep_split) {
  qh_xgeom g{};
  g.signature = signature;
  g.slab_mask = p.slab_mask;
  g.block_bits = p.block_bits;
  g.rounds_per_slab = p.rounds_per_slab;
  g.staging_bytes = p.staging_bytes;
  g.slabs = (uint32_t)p.slabs();
  g.chunk_bits = (uint32_t)p.chunk_bits;
  g.packed = p.packed ? 1 : 0;
  g.peers = (uint32_t)p.np;
  g.sweeps_before = sweeps_before;
  g.last_sweep_split = last_sweep_split ? 1 : 0;
  return g;
}

}  // namespace qh
