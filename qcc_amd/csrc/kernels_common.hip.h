// kernels_common.hip.h -- what several kernel files need and none of them owns.
//
//   * The fixed-order sum of the readers: thread (its items in order) -> wave (wave_sum, an xor tree) -> the four waves in
//     order (four_waves) -> one slab row per block (block_row_sum) -> k_slab_fold adds the rows in block order.  No float
//     atomics: the same state in the same layout and grid gives bitwise the same sums.  Every reader that promises that
//     goes through these functions, so the order cannot change for one of them only.
//   * Item16: the 16 bytes a lane moves per access of a linear stream at either width.
//   * prob_fma and prob_sum: the two ways |a|^2 is formed.  They are not interchangeable bit for bit.
//   * IndexMap and its five byte tables in LDS: physical (local) index -> logical index, for kernels that report indices.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace qh {

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// A block of 256 threads, wpart[4][N] in LDS: the sum of v over each wave into wpart[wave][0]; the caller syncs, then
// four_waves adds that column in wave order.  (A caller with N > 1 passes &wpart[0][t] for column t.)
template <int N = 1> __device__ __forceinline__ void wave_partial(double v, double *wpart) {
  v = wave_sum(v);
  if ((threadIdx.x & 63u) == 0) wpart[(threadIdx.x >> 6) * N] = v;
}
template <int N = 1> __device__ __forceinline__ double four_waves(const double *wpart) {
  return ((wpart[0] + wpart[N]) + wpart[2 * N]) + wpart[3 * N];
}

// the block's N sums into its slab row: slab[blockIdx.x * N + t] = the sum of v[t] over the block
template <int N> __device__ __forceinline__ void block_row_sum(const double (&v)[N], double *__restrict__ slab) {
  __shared__ double wpart[4][N];
  const uint32_t tid = threadIdx.x;
#pragma unroll
  for (int t = 0; t < N; ++t) wave_partial<N>(v[t], &wpart[0][t]);
  __syncthreads();
  if (tid < N) slab[(uint64_t)blockIdx.x * N + tid] = four_waves<N>(&wpart[0][tid]);
}

// out[t] = scale * (sum of column t of the slab): block t; thread j sums rows j, j + 256, ... in order, then a fixed tree
__global__ __launch_bounds__(256) void k_slab_fold(const double *__restrict__ slab, uint32_t nblk, int tt, double scale,
                                                   double *__restrict__ out) {
  __shared__ double part[256];
  const uint32_t t = blockIdx.x, j = threadIdx.x;
  double s = 0.0;
  for (uint32_t b = j; b < nblk; b += 256) s += slab[(uint64_t)b * tt + t];
  part[j] = s;
  __syncthreads();
  for (uint32_t h = 128; h > 0; h >>= 1) {
    if (j < h) part[j] += part[j + h];
    __syncthreads();
  }
  if (j == 0) out[t] = part[0] * scale;
}

// One 16-byte item of a linear stream: a complex128 amplitude, or two consecutive complex64 ones.
template <typename R> struct Item16;
template <> struct Item16<double> {
  typedef double vec __attribute__((ext_vector_type(2)));
  static constexpr int kAmpBits = 0;
};
template <> struct Item16<float> {
  typedef float vec __attribute__((ext_vector_type(4)));
  static constexpr int kAmpBits = 1;
};

// |a|^2 in double with the fused multiply-add spelled out: re * re rounded, then one rounding of im * im + that.  The bits
// the sweep islands' tile maxima hold and std::fma gives on the host: for probabilities that are compared for equality or
// ordered as keys.
__device__ __forceinline__ double prob_fma(double2 a) { return __builtin_fma(a.y, a.y, a.x * a.x); }
__device__ __forceinline__ double prob_fma(float2 a) { return __builtin_fma((double)a.y, (double)a.y, (double)a.x * (double)a.x); }
// |a|^2 in double as the plain expression: the compiler may contract it either way round.  For sums, which promise the same
// bits from the same build only.
template <typename T> __device__ __forceinline__ double prob_sum(T re, T im) { return (double)re * (double)re + (double)im * (double)im; }

// Physical (local) index -> logical index: bit p of the index goes to bit to[p]; shard_logical has the logical bits the
// shard index holds, as they are on this shard.  The kernels map through five 256-entry byte tables in LDS (a near-uniform
// state -- a QFT's output -- ties at almost every amplitude: the bit-by-bit map cost k_argmax_logical 10 ms of a 30-qubit
// pass): 256 threads build them, the block syncs, index_lut_logical looks up; the caller ORs shard_logical in.
struct IndexMap {
  uint8_t to[40];
  uint64_t shard_logical;
};
constexpr int kIndexLutWords = 5 * 256;
__device__ __forceinline__ void build_index_lut(uint64_t *lut, const IndexMap &m) {
  for (int t = 0; t < 5; ++t) {
    uint64_t o = 0;
    const uint64_t v = (uint64_t)threadIdx.x << (8 * t);
    for (int p = 8 * t; p < 8 * t + 8 && p < 40; ++p) o |= ((v >> p) & 1ull) << m.to[p];
    lut[t * 256 + threadIdx.x] = o;
  }
}
__device__ __forceinline__ uint64_t index_lut_logical(const uint64_t *lut, uint64_t idx) {
  return lut[idx & 255] | lut[256 + ((idx >> 8) & 255)] | lut[512 + ((idx >> 16) & 255)] | lut[768 + ((idx >> 24) & 255)] |
         lut[1024 + ((idx >> 32) & 255)];
}

}  // namespace qh
