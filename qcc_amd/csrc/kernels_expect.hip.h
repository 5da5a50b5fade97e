// kernels_expect.hip.h -- Pauli-string expectations on the device (qh_expect_pauli).
//
// A string is two masks over PHYSICAL index bits: x (X or Y) and z (Z or Y), nY = popcount(x & z):
//   <psi|P|psi> = Re[ (-i)^nY * sum_i conj(a_i) * (-1)^popcount(i & z) * a_{i ^ x} ]
// All strings with one x mask share the products w_i = conj(a_i) a_{i^x} and differ in the sign and in which of Re w,
// Im w they sum (nY mod 4: +Re, +Im, -Re, -Im): k_expect_batch evaluates up to kExpectT of them in ONE read of the state.
//
// Work items, numbered by a work index w (256 threads, thread t takes positions t + 256 u of a chunk of 256 * PER items):
//   * PAIR = false (x below bit 6, x == 0 included): item = amplitude i = w, 16 per thread and chunk.  The partner
//     a_{i^x} sits in lane (lane ^ x) of the same 16-byte load: fetched by a lane permutation, never by a second load.
//     Sums over every i: no factor.
//   * PAIR = true (top x bit tb >= 6): item = the pair (i, i ^ x) with bit tb of i clear, i = w with a zero inserted at
//     tb; 8 per thread and chunk, two 16-byte loads each.  Both loads are lane-linear (whole 1 KiB rows per wave): the
//     second one reads i ^ (x & ~63) and the lane part of x is again a lane permutation.  Every amplitude is read once;
//     the other half of the sum is the mirror image, so the fold doubles the result.
// In both cases sixteen 16-byte (complex64: 8-byte) non-temporal loads are in flight per thread.
//
// Signs cost no vector work: with bit tb squeezed out of z (it is 0 in every i of a pair item), popcount(i & z) is a
// popcount over w, and w = (chunk | u << 8 | thread).  The chunk part and the u part are wave-uniform: they flip the
// sign bit of the term's coefficient (+-1 or 0, one for Re w and one for Im w) in scalar registers, and the item costs
// two double FMAs per term.  The thread part is applied once to the thread's accumulator at the end.
//
// Reductions are in double and in the fixed order of kernels_common.hip.h, no atomics: thread (chunks in order, u in order)
// -> block_row_sum, one slab row per block -> k_slab_fold sums the rows in block order.  The same state in the same layout
// gives bitwise the same values.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels_common.hip.h"
#include "kernels_gate.hip.h"

namespace qh {

constexpr int kExpectT = 16;           // strings per read of the state (DESIGN.md "Pauli expectations": why 16)
constexpr int kExpectLoads = 16;       // loads in flight per thread

struct ExpectArgs {
  uint64_t x;                  // physical x mask (local bits only)
  uint64_t zc[kExpectT];       // z in work-index bits, the part at or above the chunk bits (shifted down by them)
  uint32_t cre[kExpectT];      // high word of the double that multiplies Re w: +1.0, -1.0 or 0
  uint32_t cim[kExpectT];      // ... Im w
  uint16_t zu[kExpectT];       // bit u: parity of z over the register-index part u of the position
  uint8_t zt[kExpectT];        // z over the thread index (work-index bits 0-7)
  int tb;                      // PAIR: top bit of x
  int cw;                      // log2(items per chunk): min(8 + log2 PER, log2 items)
  uint32_t cpb;                // chunks per block
};

template <typename R> __device__ __forceinline__ typename AmpT<R>::type lane_perm(const typename AmpT<R>::type &v, int m) {
  typename AmpT<R>::type o;
  o.x = __shfl_xor(v.x, m, 64);
  o.y = __shfl_xor(v.y, m, 64);
  return o;
}

__device__ __forceinline__ double coef(uint32_t hi) { return __hiloint2double((int)hi, 0); }

template <typename R, int TT, bool PAIR>
__global__ __launch_bounds__(256) void k_expect_batch(const typename AmpT<R>::type *__restrict__ psi, ExpectArgs a,
                                                       double *__restrict__ slab) {
  using A = typename AmpT<R>::type;
  constexpr int PER = PAIR ? kExpectLoads / 2 : kExpectLoads;
  const uint32_t tid = threadIdx.x, ch = 1u << a.cw;
  const int xl = (int)(a.x & 63ull);
  const uint64_t xh = a.x & ~63ull, low = PAIR ? (1ull << a.tb) - 1ull : 0ull;
  double acc[TT];
#pragma unroll
  for (int t = 0; t < TT; ++t) acc[t] = 0.0;
  const uint64_t q0 = (uint64_t)blockIdx.x * a.cpb;
  for (uint64_t q = q0; q < q0 + a.cpb; ++q) {
    const uint64_t wbase = q << a.cw;
    A va[PER], vb[PER];
#pragma unroll
    for (int u = 0; u < PER; ++u) {
      va[u].x = 0; va[u].y = 0;
      vb[u].x = 0; vb[u].y = 0;
      const uint32_t pos = tid + 256u * u;
      if (pos < ch) {
        const uint64_t w = wbase | pos;
        if constexpr (PAIR) {
          const uint64_t i = ((w & ~low) << 1) | (w & low);
          va[u] = ld_amp<true>(psi + i);
          vb[u] = ld_amp<true>(psi + (i ^ xh));
        } else {
          va[u] = ld_amp<true>(psi + w);
        }
      }
    }
    uint32_t m[TT];      // bit u: the sign of item u of this chunk, without the thread part (wave-uniform)
#pragma unroll
    for (int t = 0; t < TT; ++t)
      m[t] = (uint32_t)a.zu[t] ^ (0u - (uint32_t)(__builtin_popcountll((wbase >> (PAIR ? 11 : 12)) & a.zc[t]) & 1));
#pragma unroll
    for (int u = 0; u < PER; ++u) {
      A p = PAIR ? vb[u] : va[u];
      if (xl) p = lane_perm<R>(p, xl);
      const double ar = (double)va[u].x, ai = (double)va[u].y, br = (double)p.x, bi = (double)p.y;
      const double wre = __builtin_fma(ai, bi, ar * br), wim = __builtin_fma(ar, bi, -(ai * br));
#pragma unroll
      for (int t = 0; t < TT; ++t) {
        const uint32_t s = ((m[t] >> u) & 1u) << 31;
        acc[t] = __builtin_fma(wre, coef(a.cre[t] ^ s), acc[t]);
        acc[t] = __builtin_fma(wim, coef(a.cim[t] ^ s), acc[t]);
      }
    }
  }
#pragma unroll
  for (int t = 0; t < TT; ++t)
    if (__builtin_popcount(tid & a.zt[t]) & 1) acc[t] = -acc[t];
  block_row_sum(acc, slab);
}

}  // namespace qh
