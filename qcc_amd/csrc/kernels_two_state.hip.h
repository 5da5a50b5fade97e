// kernels_two_state.hip.h -- the walks over two states that both live in HBM, amplitude by amplitude, matched by LOGICAL
// index.  What is done with a matched pair is an operation given at compile time: qh_inner reads both and sums
// (kernels_inner.hip.h), qh_axpby rewrites the first state in place (kernels_axpby.hip.h).
//
// The two handles rarely share a physical layout (relayout sweeps leave a circuit-dependent bit map), and a walk does not
// move states: inner_plan.h turns the two bit maps into one of three walks.
//   * k_two_linear (same layout): two linear streams, every lane 16 bytes per access (one complex128 amplitude, or two
//     consecutive complex64 ones), kInnerLoads loads of each state in flight per thread, non-temporal.
//   * k_two_tiles (different layouts, >= 8 local bits): tiles of 2^8 amplitudes chosen so that BOTH states are touched in
//     runs of 16 consecutive amplitudes (256 bytes of complex128).  The 256 threads of a block enumerate a tile once in
//     a's order and once in b's order (thread r loads in-tile index r of each); b's values cross through LDS, where thread r
//     picks up slot shuffle(r), the partner of the amplitude of a it holds (slots are stored XOR-swizzled, slot s at
//     s ^ (s >> 4): a shuffle that sends a's low in-tile bits to b's high ones -- a bit reversal -- would otherwise have the
//     16 lanes of a read group 256 bytes apart, all on one bank group).  shuffle(r), the thread's offsets inside a tile
//     and the tile bases of a chunk of tiles are computed once per block; a tile costs two loads, one LDS write and one LDS
//     read per thread.  kInnerU tiles are in flight per thread.
//   * k_two_gather (fewer than 8 local bits): one block, b's partner index bit by bit.
//
// An operation Op says
//   RD, RS      whether a and b are loaded at all; a state that is not loaded is never touched (NaN or Inf in it cannot
//               propagate) and the operation sees zeros in its place;
//   kWrites     whether it stores to a.  Every thread stores to the address it loaded a from, so no thread ever reads what
//               another one writes.  A writer is given only positions that exist; a reader is also given the zero-filled
//               items past the end of a short chunk, which add nothing to its sums;
//   item, amp   what one 16-byte item of the linear walk, or one amplitude pair of the other two, becomes: the operation gets
//               a's address, both values and the thread's two running sums;
//   sums        whether the block's two sums go to its slab row (uniform over the launch: nothing is written to the slab
//               without it).  They do in the fixed order of kernels_common.hip.h: thread (its items in order) ->
//               block_row_sum -> k_slab_fold adds the rows in block order.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "inner_plan.h"
#include "kernels_common.hip.h"
#include "kernels_gate.hip.h"

namespace qh {

constexpr int kInnerLoads = 8;          // k_two_linear: loads of EACH state in flight per thread
constexpr int kInnerU = 4;              // k_two_tiles: tiles in flight per thread (4 KiB of LDS each at complex128)
constexpr int kInnerChunkBits = 6;      // k_two_tiles: tiles per chunk (their bases sit in LDS), at most 2^8

constexpr int kInnerMaxLocalBits = 40;  // what qh_create accepts (engine.hip check_args): at most 40 - 8 tile-number bits

struct InnerTileArgs {
  uint8_t tile_a[8], tile_b[8], shuffle[8];      // qh_inner_tiles
  uint8_t rest_a[kInnerMaxLocalBits], rest_b[kInnerMaxLocalBits];      // (the first nrest <= 32 entries are used)
  int nrest;                   // tile-number bits
  int cbits;                   // log2(tiles per chunk): min(kInnerChunkBits, nrest)
  uint32_t cpb;                // chunks per block
};
static_assert(sizeof(InnerTileArgs::rest_a) <= sizeof(qh_inner_tiles::rest_a) && kInnerMaxLocalBits - kInnerTileBits <= (int)sizeof(InnerTileArgs::rest_a),
              "the launch copies sizeof(InnerTileArgs::rest_a) bytes out of the plan's tables");
struct InnerGatherArgs {
  int nloc;
  uint8_t pos_b[8];
};

// a's amplitudes as the kernels take them: const for a reader
template <typename R, typename Op> using TwoDst = std::conditional_t<Op::kWrites, typename AmpT<R>::type, const typename AmpT<R>::type>;

// chunks of 2^cw ITEMS (cw <= 8 + log2 kInnerLoads), cpb chunks per block; thread t takes positions t + 256 u
template <typename R, typename Op>
__global__ __launch_bounds__(256) void k_two_linear(TwoDst<R, Op> *__restrict__ pa, const typename AmpT<R>::type *__restrict__ pb, Op op, int cw,
                                                     uint32_t cpb, double *__restrict__ slab) {
  using V = typename Item16<R>::vec;
  using VA = std::conditional_t<Op::kWrites, V, const V>;
  VA *__restrict__ qa = (VA *)pa;
  const V *__restrict__ qb = (const V *)pb;
  const uint32_t tid = threadIdx.x, ch = 1u << cw;
  double s0 = 0.0, s1 = 0.0;
  const uint64_t q0 = (uint64_t)blockIdx.x * cpb;
  for (uint64_t q = q0; q < q0 + cpb; ++q) {
    const uint64_t base = q << cw;
    V va[kInnerLoads], vb[kInnerLoads];
#pragma unroll
    for (int u = 0; u < kInnerLoads; ++u) {
      va[u] = (V)0;
      vb[u] = (V)0;
      const uint32_t pos = tid + 256u * u;
      if (pos < ch) {
        if constexpr (Op::RD) va[u] = __builtin_nontemporal_load(qa + (base | pos));
        if constexpr (Op::RS) vb[u] = __builtin_nontemporal_load(qb + (base | pos));
      }
    }
#pragma unroll
    for (int u = 0; u < kInnerLoads; ++u) {
      const uint32_t pos = tid + 256u * u;
      if (!Op::kWrites || pos < ch) op.item(qa + (base | pos), va[u], vb[u], s0, s1);
    }
  }
  if (op.sums()) {
    const double row[2] = {s0, s1};
    block_row_sum(row, slab);
  }
}

// b is always read here (an operation that does not read it takes the linear walk: layouts then do not matter)
template <typename R, typename Op>
__global__ __launch_bounds__(256) void k_two_tiles(TwoDst<R, Op> *__restrict__ pa, const typename AmpT<R>::type *__restrict__ pb, Op op,
                                                    InnerTileArgs t, double *__restrict__ slab) {
  using A = typename AmpT<R>::type;
  static_assert(Op::RS, "the tiles walk reads b");
  __shared__ A xb[kInnerU][256];
  __shared__ uint64_t low_a[1 << kInnerChunkBits], low_b[1 << kInnerChunkBits];
  const uint32_t tid = threadIdx.x, ntc = 1u << t.cbits;
  // this thread inside any tile: its offset in a's and in b's enumeration, and the slot that holds its partner
  uint64_t da = tid & 15u, db = tid & 15u;
  uint32_t slot = 0;
#pragma unroll
  for (int k = 0; k < kInnerTileBits; ++k) {
    const uint64_t bit = (tid >> k) & 1u;
    if (k >= 4) {
      da |= bit << t.tile_a[k];
      db |= bit << t.tile_b[k];
    }
    slot |= (uint32_t)bit << t.shuffle[k];
  }
  const uint32_t put = tid ^ (tid >> 4), get = slot ^ (slot >> 4);      // the swizzle: a permutation inside every row of 16 slots
  // the low cbits of a tile number, spread to a's and to b's positions
  if (tid < ntc) {
    uint64_t la = 0, lb = 0;
    for (int k = 0; k < t.cbits; ++k) {
      const uint64_t bit = (tid >> k) & 1u;
      la |= bit << t.rest_a[k];
      lb |= bit << t.rest_b[k];
    }
    low_a[tid] = la;
    low_b[tid] = lb;
  }
  __syncthreads();
  double s0 = 0.0, s1 = 0.0;
  const uint64_t q0 = (uint64_t)blockIdx.x * t.cpb;
  for (uint64_t q = q0; q < q0 + t.cpb; ++q) {
    uint64_t ha = 0, hb = 0;      // the chunk number, spread likewise (uniform over the block)
    for (int k = t.cbits; k < t.nrest; ++k) {
      const uint64_t bit = (q >> (k - t.cbits)) & 1ull;
      ha |= bit << t.rest_a[k];
      hb |= bit << t.rest_b[k];
    }
    for (uint32_t j0 = 0; j0 < ntc; j0 += kInnerU) {
      A va[kInnerU], vb[kInnerU];
#pragma unroll
      for (int u = 0; u < kInnerU; ++u) {
        va[u].x = 0; va[u].y = 0;
        vb[u].x = 0; vb[u].y = 0;
        if (j0 + u < ntc) {
          if constexpr (Op::RD) va[u] = ld_amp<true>(pa + (ha | low_a[j0 + u] | da));
          vb[u] = ld_amp<true>(pb + (hb | low_b[j0 + u] | db));
        }
      }
#pragma unroll
      for (int u = 0; u < kInnerU; ++u) xb[u][put] = vb[u];
      __syncthreads();
#pragma unroll
      for (int u = 0; u < kInnerU; ++u) {
        if (!Op::kWrites || j0 + u < ntc) {
          const A p = xb[u][get];
          op.amp(pa + (ha | low_a[j0 + u] | da), va[u], p, s0, s1);
        }
      }
      __syncthreads();
    }
  }
  if (op.sums()) {
    const double row[2] = {s0, s1};
    block_row_sum(row, slab);
  }
}

// nloc < 8: one block, thread i holds a_i and fetches b's partner
template <typename R, typename Op>
__global__ __launch_bounds__(256) void k_two_gather(TwoDst<R, Op> *__restrict__ pa, const typename AmpT<R>::type *__restrict__ pb, Op op,
                                                     InnerGatherArgs g, double *__restrict__ slab) {
  using A = typename AmpT<R>::type;
  static_assert(Op::RS, "the gather walk reads b");
  const uint32_t i = threadIdx.x;
  double s0 = 0.0, s1 = 0.0;
  if (i < (1u << g.nloc)) {
    uint32_t j = 0;
    for (int p = 0; p < g.nloc; ++p) j |= ((i >> p) & 1u) << g.pos_b[p];
    A a;
    a.x = 0; a.y = 0;
    if constexpr (Op::RD) a = pa[i];
    const A b = pb[j];
    op.amp(pa + i, a, b, s0, s1);
  }
  if (op.sums()) {
    const double row[2] = {s0, s1};
    block_row_sum(row, slab);
  }
}

}  // namespace qh
