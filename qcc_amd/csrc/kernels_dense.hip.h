// kernels_dense.hip.h -- a dense complex 2^K x 2^K matrix on K arbitrary bits of the local state (qh_apply_matrix).
//
// Work item: one GROUP of 2^K amplitudes.  Its base index is expand_index() of the item counter with the K target
// positions inserted as 0 and the control bits as 1; member m of the group is base | sum_j ((m >> j) & 1) << t[j], and
// the group is replaced by out[r] = sum_c M[r][c] in[c] (matrix bit j <-> index bit t[j], t[0] least significant).
// Every amplitude of a touched group is read once and written once, 16-byte non-temporal accesses as in k_pair:
// 2S / 2^c bytes for c local controls.  Controls on bits 0-1 are not inserted (same 64-byte half line, see the header
// of kernels_gate.hip.h): they are a per-lane predicate, and groups that fail it are written back unchanged.
//
// Two shapes (VGPR counts and occupancy from the gfx950 ISA: DESIGN.md "Dense k-qubit matrices"):
//   * K <= 4, k_dense_reg: a thread holds whole groups (4 * 2^K VGPRs of complex128 inputs per group, U groups per
//     thread so that >= 8 loads are in flight) and computes one output row at a time.  M is wave-uniform and indexed
//     by compile-time constants, so it is read with scalar loads straight into SGPR operands of the FMAs (K = 4:
//     4 KiB of complex128, inside the scalar cache).
//   * K = 5, 6, k_dense_split: 2^S lanes (S = K - 4, neighbours in one quad) share a group; lane q holds the 16
//     members whose top S matrix bits are q and accumulates the 16 output rows with those top bits.  The other lanes'
//     inputs come in one at a time by DPP quad permutes.  The rows a lane needs depend on q, so M is staged in LDS
//     (K = 6: 64 KiB of complex128) with one element of padding per 16 rows: the 2^S addresses of one ds_read_b128
//     then fall on different banks (identical addresses within a q broadcast).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels_gate.hip.h"

namespace qh {

constexpr int kMaxDenseBits = 6;

struct DenseArgs {
  BitIns ins;              // targets inserted as 0, inserted controls as 1
  int t[kMaxDenseBits];    // physical position of matrix bit j
  uint32_t lowpred;        // controls on bits 0-1: the group is updated where (base & lowpred) == lowpred
  uint64_t nwork;          // groups
};

template <int K> __device__ __forceinline__ uint64_t member_offset(int m, const DenseArgs &a) {
  uint64_t o = 0;
#pragma unroll
  for (int j = 0; j < K; ++j)
    if ((m >> j) & 1) o |= 1ull << a.t[j];
  return o;
}

template <typename R, typename A>
__device__ __forceinline__ void cmac(A &acc, const A &m, const A &x) {
  acc.x = fma(m.x, x.x, acc.x);
  acc.x = fma(-m.y, x.y, acc.x);
  acc.y = fma(m.x, x.y, acc.y);
  acc.y = fma(m.y, x.x, acc.y);
}

// K <= 4: U groups per thread, grid-stride over groups.
template <typename R, int K, int U>
__global__ __launch_bounds__(256) void k_dense_reg(typename AmpT<R>::type *__restrict__ psi,
                                                    const typename AmpT<R>::type *__restrict__ mat, DenseArgs a) {
  using A = typename AmpT<R>::type;
  constexpr int D = 1 << K;
  const uint64_t stride = (uint64_t)gridDim.x * (256ull * U);
  for (uint64_t first = (uint64_t)blockIdx.x * (256ull * U) + threadIdx.x; first < a.nwork; first += stride) {
    A in[U][D];
    uint64_t base[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const uint64_t j = first + 256ull * u;
      if (j < a.nwork) {
        base[u] = expand_index(j, a.ins);
#pragma unroll
        for (int m = 0; m < D; ++m) in[u][m] = ld_amp<true>(&psi[base[u] | member_offset<K>(m, a)]);
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const uint64_t j = first + 256ull * u;
      if (j < a.nwork) {
        const bool on = ((uint32_t)base[u] & a.lowpred) == a.lowpred;
#pragma unroll
        for (int r = 0; r < D; ++r) {
          A acc;
          acc.x = (R)0;
          acc.y = (R)0;
#pragma unroll
          for (int c = 0; c < D; ++c) cmac<R, A>(acc, mat[r * D + c], in[u][c]);
          st_amp<true>(&psi[base[u] | member_offset<K>(r, a)], on ? acc : in[u][r]);
        }
      }
    }
  }
}

// value of lane l ^ d within its quad (d = 1..3), DPP quad_perm
template <int D> __device__ __forceinline__ int quad_xor_i32(int v) {
  static_assert(D >= 1 && D <= 3, "quad partner");
  constexpr int ctl = D == 1 ? 0xB1 : D == 2 ? 0x4E : 0x1B;   // [1,0,3,2] / [2,3,0,1] / [3,2,1,0]
  return __builtin_amdgcn_update_dpp(0, v, ctl, 0xf, 0xf, false);
}
template <int D> __device__ __forceinline__ double quad_xor(double v) {
  const long long w = __double_as_longlong(v);
  const int lo = quad_xor_i32<D>((int)(w & 0xffffffffll)), hi = quad_xor_i32<D>((int)(w >> 32));
  return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}
template <int D> __device__ __forceinline__ float quad_xor(float v) {
  return __int_as_float(quad_xor_i32<D>(__float_as_int(v)));
}
template <int D, typename A> __device__ __forceinline__ A quad_xor_amp(const A &v) {
  A o;
  o.x = quad_xor<D>(v.x);
  o.y = quad_xor<D>(v.y);
  return o;
}

// LDS index of M[r][c]: one element of padding per 16 rows (see the header)
template <int K> __device__ __forceinline__ int lds_index(int r, int c) { return r * (1 << K) + c + (r >> 4); }
template <int K> constexpr int lds_elems() { return (1 << (2 * K)) + (1 << (K - 4)); }

// lane q's partial sums from the 16 inputs of lane q ^ DQ (x: already fetched from that lane)
template <typename R, int K, int DQ>
__device__ __forceinline__ void split_partner(typename AmpT<R>::type (&acc)[16], const typename AmpT<R>::type (&in)[16],
                                              const typename AmpT<R>::type *sm, int q) {
  using A = typename AmpT<R>::type;
  const A *row = sm + lds_index<K>(q << 4, (q ^ DQ) << 4);
#pragma unroll
  for (int ci = 0; ci < 16; ++ci) {
    const A x = DQ == 0 ? in[ci] : quad_xor_amp<(DQ ? DQ : 1)>(in[ci]);
#pragma unroll
    for (int ri = 0; ri < 16; ++ri) cmac<R, A>(acc[ri], row[ri * (1 << K) + ci], x);
  }
}

// K = 5, 6: 2^(K-4) lanes per group, 16 members and 16 output rows per lane.
template <typename R, int K>
__global__ __launch_bounds__(256, 2) void k_dense_split(typename AmpT<R>::type *__restrict__ psi,
                                                      const typename AmpT<R>::type *__restrict__ mat, DenseArgs a) {
  using A = typename AmpT<R>::type;
  constexpr int S = K - 4, Q = 1 << S, D = 1 << K;
  static_assert(S >= 1 && S <= 2, "k_dense_split: K = 5 or 6");
  __shared__ A sm[lds_elems<K>()];
  for (int i = threadIdx.x; i < D * D; i += 256) sm[lds_index<K>(i >> K, i & (D - 1))] = mat[i];
  __syncthreads();
  const int q = threadIdx.x & (Q - 1);
  const uint64_t hi = member_offset<K>(q << 4, a);                 // this lane's top matrix bits
  uint64_t lo[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) lo[i] = member_offset<K>(i, a);
  const uint64_t stride = (uint64_t)gridDim.x * 256ull;
  // (the Q lanes of a group are in one quad and share the loop condition: the DPP partners are always active)
  for (uint64_t t = (uint64_t)blockIdx.x * 256ull + threadIdx.x; (t >> S) < a.nwork; t += stride) {
    // M does not change inside the loop: without this barrier the compiler hoists all D*D/Q LDS reads of it out of the
    // loop into registers, and spills them to scratch
    __asm__ volatile("" ::: "memory");
    const uint64_t base = expand_index(t >> S, a.ins) | hi;
    A in[16], acc[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) in[i] = ld_amp<true>(&psi[base | lo[i]]);
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      acc[i].x = (R)0;
      acc[i].y = (R)0;
    }
    split_partner<R, K, 0>(acc, in, sm, q);
    split_partner<R, K, 1>(acc, in, sm, q);
    if constexpr (S == 2) {
      split_partner<R, K, 2>(acc, in, sm, q);
      split_partner<R, K, 3>(acc, in, sm, q);
    }
    const bool on = ((uint32_t)base & a.lowpred) == a.lowpred;
#pragma unroll
    for (int i = 0; i < 16; ++i) st_amp<true>(&psi[base | lo[i]], on ? acc[i] : in[i]);
  }
}

}  // namespace qh
