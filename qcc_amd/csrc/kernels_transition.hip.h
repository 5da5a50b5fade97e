// kernels_transition.hip.h -- <a|P|b> for Pauli strings P between two states that both live in HBM (qh_transition_pauli).
//
//   <a|P|b> = (-i)^nY * sum_i (-1)^popcount(i & z) * conj(a_i) * b_{i ^ x}
// A pass holds up to TT strings with ONE x mask: they share the products w_i = conj(a_i) b_{i^x} and differ in the sign
// only, so a pass reads each state once and keeps 2 TT running sums per thread (Re and Im per string).  (-i)^nY and the
// shard sign are left to the host: exact swaps and negations of the folded sums.
//
// The walks are those of kernels_two_state.hip.h in structure -- same chunking, same grids, the same LDS crossing and
// swizzle in the tiles walk -- with two differences:
//   * b's amplitude index is XORed with px, the x mask in B's physical positions, wherever the walk forms b's address.  The
//     XOR permutes addresses inside the runs the walk loads anyway (lanes inside a 16-byte-per-lane row, rows inside a
//     chunk, chunks inside the state): every amplitude of b is still read exactly once per pass.  A complex64 linear item
//     holds two amplitudes: the item index is XORed with px >> 1 and the halves trade places when px & 1.
//   * the sign (-1)^popcount(ia & pz) comes from A's physical index ia with the z mask in A's positions, split as in
//     k_expect_batch so that it costs no vector work: the wave-uniform part of ia (chunk number and register index in the
//     linear walk, tile number in the tiles walk) flips the sign bit of a coefficient +-1.0 held in scalar registers, and
//     the item costs two double FMAs per string; the thread-only part is applied once to the thread's sums at the end.
//     (The complex64 half bit of the linear walk is uniform too: the second amplitude of an item takes the coefficient
//     with that string's half sign folded in.)
//
// Sums are in double from the stored amplitudes and in the fixed order of kernels_common.hip.h, no atomics: thread (its
// items in order) -> block_row_sum<2 TT> -> k_slab_fold.  Items past the end of a short chunk or tile list are zeros and
// add nothing.  Columns of strings past the pass's count hold <a|b'> for the same x and are never folded.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels_common.hip.h"
#include "kernels_expect.hip.h"
#include "kernels_gate.hip.h"
#include "kernels_two_state.hip.h"
#include "transition_plan.h"

namespace qh {

static_assert(kInnerLoads == kPauliPer, "transition_split_linear numbers the items of a chunk as pauli_split_z does");

struct TransArgs {
  uint64_t px;                 // the x mask in b's physical local positions
  uint64_t zc[kTransT];        // z over the chunk number (linear) / the tile number (tiles)
  uint8_t zu[kTransT];         // linear: bit u = parity of z over the register-index part u
  uint8_t zt[kTransT];         // z over the thread index (linear: item bits 0-7; tiles: in-tile index; gather: the index)
  uint32_t zh;                 // linear at complex64: bit t = string t has z on the sub-item bit
  int cw;                      // linear: log2(items per chunk)
  uint32_t cpb;                // linear: chunks per block
};

constexpr uint32_t kOneHi = 0x3FF00000u;      // high word of 1.0; ^ 0x80000000: of -1.0

// acc[2t], acc[2t + 1] += s_t * (wre, wim); flip: bit 31 of flip[t] set where s_t = -1 (wave-uniform)
template <int TT> __device__ __forceinline__ void trans_add(double (&acc)[2 * TT], double wre, double wim, const uint32_t (&flip)[TT]) {
#pragma unroll
  for (int t = 0; t < TT; ++t) {
    const double c = coef(kOneHi ^ flip[t]);
    acc[2 * t] = __builtin_fma(wre, c, acc[2 * t]);
    acc[2 * t + 1] = __builtin_fma(wim, c, acc[2 * t + 1]);
  }
}
// w = conj(a) b
__device__ __forceinline__ void trans_w(double ar, double ai, double br, double bi, double &wre, double &wim) {
  wre = __builtin_fma(ai, bi, ar * br);
  wim = __builtin_fma(ar, bi, -(ai * br));
}
// the thread-only part of the signs, then the block's row
template <int TT> __device__ __forceinline__ void trans_finish(double (&acc)[2 * TT], uint32_t thread_index, const TransArgs &a, double *__restrict__ slab) {
#pragma unroll
  for (int t = 0; t < TT; ++t)
    if (__builtin_popcount(thread_index & a.zt[t]) & 1) {
      acc[2 * t] = -acc[2 * t];
      acc[2 * t + 1] = -acc[2 * t + 1];
    }
  block_row_sum(acc, slab);
}

// same layout: chunks of 2^cw ITEMS (cw <= 8 + log2 kInnerLoads), cpb chunks per block; thread t takes positions t + 256 u
template <typename R, int TT>
__global__ __launch_bounds__(256) void k_trans_linear(const typename AmpT<R>::type *__restrict__ pa, const typename AmpT<R>::type *__restrict__ pb,
                                                       TransArgs a, double *__restrict__ slab) {
  using V = typename Item16<R>::vec;
  constexpr int AB = Item16<R>::kAmpBits;
  const V *__restrict__ qa = (const V *)pa;
  const V *__restrict__ qb = (const V *)pb;
  const uint32_t tid = threadIdx.x, ch = 1u << a.cw;
  const uint64_t xi = a.px >> AB;
  const bool swap = AB && (a.px & 1ull);
  double acc[2 * TT];
#pragma unroll
  for (int t = 0; t < 2 * TT; ++t) acc[t] = 0.0;
  const uint64_t q0 = (uint64_t)blockIdx.x * a.cpb;
  for (uint64_t q = q0; q < q0 + a.cpb; ++q) {
    const uint64_t base = q << a.cw;
    V va[kInnerLoads], vb[kInnerLoads];
#pragma unroll
    for (int u = 0; u < kInnerLoads; ++u) {
      va[u] = (V)0;
      vb[u] = (V)0;
      const uint32_t pos = tid + 256u * u;
      if (pos < ch) {
        va[u] = __builtin_nontemporal_load(qa + (base | pos));
        vb[u] = __builtin_nontemporal_load(qb + ((base | pos) ^ xi));
      }
    }
    uint32_t m[TT];      // bit u: the sign of item u of this chunk, without the thread and half parts (wave-uniform)
#pragma unroll
    for (int t = 0; t < TT; ++t) m[t] = (uint32_t)a.zu[t] ^ (0u - (uint32_t)(__builtin_popcountll(q & a.zc[t]) & 1));
#pragma unroll
    for (int u = 0; u < kInnerLoads; ++u) {
      uint32_t flip[TT];
#pragma unroll
      for (int t = 0; t < TT; ++t) flip[t] = ((m[t] >> u) & 1u) << 31;
      double wre, wim;
      if constexpr (AB == 0) {
        trans_w(va[u].x, va[u].y, vb[u].x, vb[u].y, wre, wim);
        trans_add<TT>(acc, wre, wim, flip);
      } else {
        const V p = swap ? (V){vb[u].z, vb[u].w, vb[u].x, vb[u].y} : vb[u];
        trans_w((double)va[u].x, (double)va[u].y, (double)p.x, (double)p.y, wre, wim);
        trans_add<TT>(acc, wre, wim, flip);
#pragma unroll
        for (int t = 0; t < TT; ++t) flip[t] ^= ((a.zh >> t) & 1u) << 31;
        trans_w((double)va[u].z, (double)va[u].w, (double)p.z, (double)p.w, wre, wim);
        trans_add<TT>(acc, wre, wim, flip);
      }
    }
  }
  trans_finish<TT>(acc, tid, a, slab);
}

// different layouts, >= 8 local bits: k_two_tiles with b's address XORed with px and 2 TT signed sums
template <typename R, int TT>
__global__ __launch_bounds__(256) void k_trans_tiles(const typename AmpT<R>::type *__restrict__ pa, const typename AmpT<R>::type *__restrict__ pb,
                                                      TransArgs a, InnerTileArgs t, double *__restrict__ slab) {
  using A = typename AmpT<R>::type;
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
  const uint32_t put = tid ^ (tid >> 4), get = slot ^ (slot >> 4);      // the swizzle of k_two_tiles
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
  double acc[2 * TT];
#pragma unroll
  for (int s = 0; s < 2 * TT; ++s) acc[s] = 0.0;
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
          va[u] = ld_amp<true>(pa + (ha | low_a[j0 + u] | da));
          vb[u] = ld_amp<true>(pb + ((hb | low_b[j0 + u] | db) ^ a.px));      // slot r of the tile: b_{(b's index r) ^ px}
        }
      }
#pragma unroll
      for (int u = 0; u < kInnerU; ++u) xb[u][put] = vb[u];
      __syncthreads();
#pragma unroll
      for (int u = 0; u < kInnerU; ++u) {
        const A p = xb[u][get];
        const uint64_t tile = (q << t.cbits) | (uint64_t)(j0 + u);      // a's tile number (wave-uniform)
        uint32_t flip[TT];
#pragma unroll
        for (int s = 0; s < TT; ++s) flip[s] = (uint32_t)(__builtin_popcountll(tile & a.zc[s]) & 1) << 31;
        double wre, wim;
        trans_w((double)va[u].x, (double)va[u].y, (double)p.x, (double)p.y, wre, wim);
        trans_add<TT>(acc, wre, wim, flip);
      }
      __syncthreads();
    }
  }
  trans_finish<TT>(acc, tid, a, slab);
}

// nloc < 8: one block, thread i holds a_i and fetches b's partner; the whole sign is the thread's
template <typename R, int TT>
__global__ __launch_bounds__(256) void k_trans_gather(const typename AmpT<R>::type *__restrict__ pa, const typename AmpT<R>::type *__restrict__ pb,
                                                       TransArgs a, InnerGatherArgs g, double *__restrict__ slab) {
  using A = typename AmpT<R>::type;
  const uint32_t i = threadIdx.x;
  double acc[2 * TT];
#pragma unroll
  for (int t = 0; t < 2 * TT; ++t) acc[t] = 0.0;
  if (i < (1u << g.nloc)) {
    uint32_t j = 0;
    for (int p = 0; p < g.nloc; ++p) j |= ((i >> p) & 1u) << g.pos_b[p];
    const A va = pa[i], vb = pb[j ^ (uint32_t)a.px];
    double wre, wim;
    trans_w((double)va.x, (double)va.y, (double)vb.x, (double)vb.y, wre, wim);
#pragma unroll
    for (int t = 0; t < TT; ++t) {
      acc[2 * t] = wre;
      acc[2 * t + 1] = wim;
    }
  }
  trans_finish<TT>(acc, i, a, slab);
}

}  // namespace qh
