// kernels_argmax.hip.h -- qh_argmax: the FIRST basis state, in LOGICAL order, with the largest probability (state.py:60-78
// maxprob).
//
// Probabilities are prob_fma (kernels_common.hip.h), the bits the sweep islands leave as per-unit maxima, so they can be
// compared for equality.
//   * k_argmax_logical: the full pass.  Per block the largest probability and the smallest logical index that has it;
//     physical -> logical through the LDS byte tables of kernels_common.hip.h (MAPPED), or the physical index as it is.
//   * k_tmax_reduce, k_tmax_collect, k_tmax_scan: behind a fused flush whose last sweep left the maximum of every unit it
//     stored: the largest of them, the units that hold it, and the smallest logical index among their amplitudes that have it.
//   * k_prefix_scan: where too many units hold it (a flat state), the first hit in a range of LOGICAL indices.
// The last two visit few amplitudes and map them bit by bit.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels_common.hip.h"
#include "kernels_gate.hip.h"

namespace qh {

// bit p of v goes to bit to[p], for the n lowest bits
__device__ __forceinline__ uint64_t map_bits(uint64_t v, const uint8_t *to, int n) {
  uint64_t o = 0;
  for (int p = 0; p < n; ++p) o |= ((v >> p) & 1ull) << to[p];
  return o;
}
// logical -> physical position of the local bits (the inverse of IndexMap::to)
struct BitMap { int n; uint8_t to[64]; };

// per block: the largest probability and the smallest LOGICAL index that has it (identity map: the physical index)
template <typename A, bool MAPPED>
__global__ __launch_bounds__(256) void k_argmax_logical(const A *__restrict__ psi, uint64_t n, IndexMap bm, double *best_p, uint64_t *best_i) {
  __shared__ double sp[256];
  __shared__ uint64_t si[256];
  __shared__ uint64_t lut[MAPPED ? kIndexLutWords : 1];
  if (MAPPED) {
    build_index_lut(lut, bm);
    __syncthreads();
  }
  auto logical = [&](uint64_t idx) -> uint64_t { return MAPPED ? index_lut_logical(lut, idx) : idx; };
  double bp = -1.0;
  uint64_t bi = ~0ull;
  const uint64_t stride = (uint64_t)gridDim.x * 256;
  uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  auto take = [&](double p, uint64_t idx) {
    if (p > bp) { bp = p; bi = logical(idx); }
    else if (p == bp) { const uint64_t li = logical(idx); if (li < bi) bi = li; }
  };
  for (; i + 3 * stride < n; i += 4 * stride) {      // four loads in flight per thread
    A a[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) a[k] = ld_amp<true>(psi + i + k * stride);
#pragma unroll
    for (int k = 0; k < 4; ++k) take(prob_fma(a[k]), i + k * stride);
  }
  for (; i < n; i += stride) take(prob_fma(ld_amp<true>(psi + i)), i);
  sp[threadIdx.x] = bp;
  si[threadIdx.x] = bi;
  __syncthreads();
  for (unsigned st = 128; st > 0; st >>= 1) {
    if (threadIdx.x < st) {
      const double op = sp[threadIdx.x + st];
      const uint64_t oi = si[threadIdx.x + st];
      if (op > sp[threadIdx.x] || (op == sp[threadIdx.x] && oi < si[threadIdx.x])) { sp[threadIdx.x] = op; si[threadIdx.x] = oi; }
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) { best_p[blockIdx.x] = sp[0]; best_i[blockIdx.x] = si[0]; }
}

// the per-unit maxima of the last sweep (bit patterns of non-negative doubles: they order like the doubles)
__global__ __launch_bounds__(256) void k_tmax_reduce(const uint64_t *__restrict__ t, uint64_t n, uint64_t *out) {
  __shared__ uint64_t sm[256];
  uint64_t m = 0;
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) m = t[i] > m ? t[i] : m;
  sm[threadIdx.x] = m;
  __syncthreads();
  for (unsigned st = 128; st > 0; st >>= 1) {
    if (threadIdx.x < st && sm[threadIdx.x + st] > sm[threadIdx.x]) sm[threadIdx.x] = sm[threadIdx.x + st];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[blockIdx.x] = sm[0];
}
constexpr unsigned kTmaxIds = 64;
// units whose maximum is the global one: ids[0] = how many, ids[1..] the first kTmaxIds of them
__global__ __launch_bounds__(256) void k_tmax_collect(const uint64_t *__restrict__ t, uint64_t n, uint64_t want, unsigned long long *ids) {
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256)
    if (t[i] == want) {
      const unsigned long long k = atomicAdd(ids, 1ull);
      if (k < kTmaxIds) ids[1 + k] = i;
    }
}
// one block per collected unit: the smallest logical index among its amplitudes with probability == want (nloc local bits)
template <typename A>
__global__ __launch_bounds__(256) void k_tmax_scan(const A *__restrict__ psi, const unsigned long long *__restrict__ ids, BitIns ins,
                                                    uint64_t tile_mask, int tile_bits, double want, IndexMap bm, int nloc, unsigned long long *out) {
  const uint64_t base = expand_index(ids[1 + blockIdx.x], ins);
  unsigned long long best = ~0ull;
  for (uint64_t j = threadIdx.x; j < (1ull << tile_bits); j += 256) {
    uint64_t off = 0, jj = j;
    for (uint64_t m = tile_mask; m; m &= m - 1) { off |= (jj & 1ull) << __builtin_ctzll(m); jj >>= 1; }
    const uint64_t idx = base | off;
    if (prob_fma(ld_amp<false>(psi + idx)) == want) {
      const unsigned long long li = map_bits(idx, bm.to, nloc);
      best = li < best ? li : best;
    }
  }
  if (best != ~0ull) atomicMin(out, best);
}

// the smallest logical index in [l0, l1) whose amplitude has probability == want (l2p: logical -> physical)
template <typename A>
__global__ __launch_bounds__(256) void k_prefix_scan(const A *__restrict__ psi, uint64_t l0, uint64_t l1, double want, BitMap l2p,
                                                      unsigned long long *out) {
  unsigned long long best = ~0ull;
  for (uint64_t l = l0 + (uint64_t)blockIdx.x * 256 + threadIdx.x; l < l1; l += (uint64_t)gridDim.x * 256)
    if (prob_fma(ld_amp<false>(psi + map_bits(l, l2p.to, l2p.n))) == want) { best = l; break; }     // (ascending per thread: the first hit is its smallest)
  if (best != ~0ull) atomicMin(out, best);
}

}  // namespace qh
