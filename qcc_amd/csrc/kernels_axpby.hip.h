// kernels_axpby.hip.h -- dst := alpha * dst + beta * src for two states that both live in HBM (qh_axpby), amplitude by
// amplitude, matched by LOGICAL index, written in place into dst where it lies.
//
// The siblings of the k_inner_* readers (kernels_inner.hip.h) that WRITE: the same plan (inner_plan.h, a = dst, b = src), the
// same geometry (chunks of 256 * kInnerLoads items, chunks of 2^kInnerChunkBits tiles, at most 4096 blocks), the same three
// walks.  Every thread stores to the address it loaded dst from, so no thread ever reads what another one writes.
//   * k_axpby_linear (same layout, or src not read at all): 16 bytes per lane and access at both widths, kInnerLoads loads of
//     each state in flight per thread, non-temporal loads and non-temporal 16-byte stores.
//   * k_axpby_tiles (different layouts, >= 8 local bits): thread r loads dst's in-tile index r and src's in-tile index r in
//     src's enumeration; src's values cross through the XOR-swizzled LDS slots exactly as in k_inner_tiles; the thread
//     combines and stores one amplitude (16 bytes of complex128, 8 of complex64).  Both states are touched in runs of 16.
//   * k_axpby_gather (fewer than 8 local bits): one block, src's partner index bit by bit.
// RD = false (alpha == 0 exactly): dst's old values are never loaded -- NaN or Inf in them cannot propagate and the pass is
// two streams.  RS = false (beta == 0 exactly): src is never loaded; layouts then do not matter and the linear kernel runs
// whatever the plan says.  Both false: one stream of zeros.
//
// Arithmetic: each component of the new amplitude is formed in double from the stored amplitudes, as
// (ar*dr - ai*di) + (br*sr - bi*si) and (ar*di + ai*dr) + (br*si + bi*sr) without fused multiply-adds, and rounded once to the
// handle's width.  A product whose COEFFICIENT component is exactly 0 is taken as 0 whatever the amplitude holds, so
// coefficients made of 0, 1 and -1 reproduce d + s, d - s, s ... as numbers (the sum of two floats formed in double and
// rounded to float equals the float sum: 53 >= 2 * 24 + 2 bits).
//
// norm (a uniform branch; nothing is summed or written to the slab without it): sum |a|^2 of the values AS STORED, after the
// rounding, in double and in the fixed order of the readers: thread (its items in order) -> wave (xor tree) -> the four waves
// in order -> one row per block (inner_block_sum) -> k_expect_fold adds the rows in block order.  No atomics.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels_inner.hip.h"

namespace qh {

struct AxpbyCoef {
  double ar, ai, br, bi;       // alpha, beta
  int norm;                    // sum |new|^2 into the slab
};

// c * v, with an exactly zero coefficient giving 0 (c is uniform over the launch: a scalar compare)
__device__ __forceinline__ double axpby_mul(double c, double v) { return c == 0.0 ? 0.0 : c * v; }

template <bool RD, bool RS>
__device__ __forceinline__ void axpby_amp(const AxpbyCoef &c, double dr, double di, double sr, double si, double &outr, double &outi) {
#pragma clang fp contract(off)
  double xr = 0.0, xi = 0.0, yr = 0.0, yi = 0.0;
  if constexpr (RD) {
    xr = axpby_mul(c.ar, dr) - axpby_mul(c.ai, di);
    xi = axpby_mul(c.ar, di) + axpby_mul(c.ai, dr);
  }
  if constexpr (RS) {
    yr = axpby_mul(c.br, sr) - axpby_mul(c.bi, si);
    yi = axpby_mul(c.br, si) + axpby_mul(c.bi, sr);
  }
  if constexpr (RD && RS) {
    outr = xr + yr;
    outi = xi + yi;
  } else if constexpr (RD) {
    outr = xr;
    outi = xi;
  } else {
    outr = yr;
    outi = yi;
  }
}

// one amplitude: combined, rounded to the handle's width, its weight as stored
template <typename R, bool RD, bool RS>
__device__ __forceinline__ void axpby_round(const AxpbyCoef &c, R dr, R di, R sr, R si, R &outr, R &outi, double &n2) {
#pragma clang fp contract(off)
  double r, i;
  axpby_amp<RD, RS>(c, (double)dr, (double)di, (double)sr, (double)si, r, i);
  outr = (R)r;
  outi = (R)i;
  if (c.norm) n2 += (double)outr * (double)outr + (double)outi * (double)outi;
}

template <bool RD, bool RS>
__device__ __forceinline__ InnerItem<double>::vec axpby_item(const AxpbyCoef &c, const InnerItem<double>::vec &d, const InnerItem<double>::vec &s,
                                                             double &n2) {
  InnerItem<double>::vec o;
  double re, im;
  axpby_round<double, RD, RS>(c, d.x, d.y, s.x, s.y, re, im, n2);
  o.x = re;
  o.y = im;
  return o;
}
template <bool RD, bool RS>
__device__ __forceinline__ InnerItem<float>::vec axpby_item(const AxpbyCoef &c, const InnerItem<float>::vec &d, const InnerItem<float>::vec &s,
                                                            double &n2) {
  InnerItem<float>::vec o;
  float re0, im0, re1, im1;
  axpby_round<float, RD, RS>(c, d.x, d.y, s.x, s.y, re0, im0, n2);
  axpby_round<float, RD, RS>(c, d.z, d.w, s.z, s.w, re1, im1, n2);
  o.x = re0;
  o.y = im0;
  o.z = re1;
  o.w = im1;
  return o;
}

// one amplitude out, as one non-temporal store of its full size
__device__ __forceinline__ void axpby_store(double2 *p, double re, double im) {
  InnerItem<double>::vec v;
  v.x = re;
  v.y = im;
  __builtin_nontemporal_store(v, (InnerItem<double>::vec *)p);
}
__device__ __forceinline__ void axpby_store(float2 *p, float re, float im) {
  typedef float half_item __attribute__((ext_vector_type(2)));
  half_item v;
  v.x = re;
  v.y = im;
  __builtin_nontemporal_store(v, (half_item *)p);
}

// chunks of 2^cw ITEMS (cw <= 8 + log2 kInnerLoads), cpb chunks per block; thread t takes positions t + 256 u (k_inner_linear)
template <typename R, bool RD, bool RS>
__global__ __launch_bounds__(256) void k_axpby_linear(typename AmpT<R>::type *__restrict__ pd, const typename AmpT<R>::type *__restrict__ ps,
                                                       AxpbyCoef c, int cw, uint32_t cpb, double *__restrict__ slab) {
  using V = typename InnerItem<R>::vec;
  V *__restrict__ qd = (V *)pd;
  const V *__restrict__ qs = (const V *)ps;
  const uint32_t tid = threadIdx.x, ch = 1u << cw;
  double n2 = 0.0;
  const uint64_t q0 = (uint64_t)blockIdx.x * cpb;
  for (uint64_t q = q0; q < q0 + cpb; ++q) {
    const uint64_t base = q << cw;
    V vd[kInnerLoads], vs[kInnerLoads];
#pragma unroll
    for (int u = 0; u < kInnerLoads; ++u) {
      vd[u] = (V)0;
      vs[u] = (V)0;
      const uint32_t pos = tid + 256u * u;
      if (pos < ch) {
        if constexpr (RD) vd[u] = __builtin_nontemporal_load(qd + (base | pos));
        if constexpr (RS) vs[u] = __builtin_nontemporal_load(qs + (base | pos));
      }
    }
#pragma unroll
    for (int u = 0; u < kInnerLoads; ++u) {
      const uint32_t pos = tid + 256u * u;
      if (pos < ch) __builtin_nontemporal_store(axpby_item<RD, RS>(c, vd[u], vs[u], n2), qd + (base | pos));
    }
  }
  if (c.norm) inner_block_sum(n2, 0.0, slab);
}

// the walk of k_inner_tiles with a = dst, b = src; src is always read here (beta == 0 takes the linear kernel)
template <typename R, bool RD>
__global__ __launch_bounds__(256) void k_axpby_tiles(typename AmpT<R>::type *__restrict__ pd, const typename AmpT<R>::type *__restrict__ ps,
                                                      AxpbyCoef c, InnerTileArgs t, double *__restrict__ slab) {
  using A = typename AmpT<R>::type;
  __shared__ A xb[kInnerU][256];
  __shared__ uint64_t low_a[1 << kInnerChunkBits], low_b[1 << kInnerChunkBits];
  const uint32_t tid = threadIdx.x, ntc = 1u << t.cbits;
  // this thread inside any tile: its offset in dst's and in src's enumeration, and the slot that holds its partner
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
  const uint32_t put = tid ^ (tid >> 4), get = slot ^ (slot >> 4);
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
  double n2 = 0.0;
  const uint64_t q0 = (uint64_t)blockIdx.x * t.cpb;
  for (uint64_t q = q0; q < q0 + t.cpb; ++q) {
    uint64_t ha = 0, hb = 0;      // the chunk number, spread to dst's and to src's positions (uniform over the block)
    for (int k = t.cbits; k < t.nrest; ++k) {
      const uint64_t bit = (q >> (k - t.cbits)) & 1ull;
      ha |= bit << t.rest_a[k];
      hb |= bit << t.rest_b[k];
    }
    for (uint32_t j0 = 0; j0 < ntc; j0 += kInnerU) {
      A vd[kInnerU], vs[kInnerU];
#pragma unroll
      for (int u = 0; u < kInnerU; ++u) {
        vd[u].x = 0; vd[u].y = 0;
        vs[u].x = 0; vs[u].y = 0;
        if (j0 + u < ntc) {
          if constexpr (RD) vd[u] = ld_amp<true>(pd + (ha | low_a[j0 + u] | da));
          vs[u] = ld_amp<true>(ps + (hb | low_b[j0 + u] | db));
        }
      }
#pragma unroll
      for (int u = 0; u < kInnerU; ++u) xb[u][put] = vs[u];
      __syncthreads();
#pragma unroll
      for (int u = 0; u < kInnerU; ++u) {
        if (j0 + u < ntc) {
          const A p = xb[u][get];
          R outr, outi;
          axpby_round<R, RD, true>(c, vd[u].x, vd[u].y, p.x, p.y, outr, outi, n2);
          axpby_store(pd + (ha | low_a[j0 + u] | da), outr, outi);
        }
      }
      __syncthreads();
    }
  }
  if (c.norm) inner_block_sum(n2, 0.0, slab);
}

// nloc < 8: one block, thread i holds dst_i and fetches src's partner
template <typename R, bool RD>
__global__ __launch_bounds__(256) void k_axpby_gather(typename AmpT<R>::type *__restrict__ pd, const typename AmpT<R>::type *__restrict__ ps,
                                                       AxpbyCoef c, InnerGatherArgs g, double *__restrict__ slab) {
  using A = typename AmpT<R>::type;
  const uint32_t i = threadIdx.x;
  double n2 = 0.0;
  if (i < (1u << g.nloc)) {
    uint32_t j = 0;
    for (int p = 0; p < g.nloc; ++p) j |= ((i >> p) & 1u) << g.pos_b[p];
    A d;
    d.x = 0; d.y = 0;
    if constexpr (RD) d = pd[i];
    const A s = ps[j];
    R outr, outi;
    axpby_round<R, RD, true>(c, d.x, d.y, s.x, s.y, outr, outi, n2);
    axpby_store(pd + i, outr, outi);
  }
  if (c.norm) inner_block_sum(n2, 0.0, slab);
}

}  // namespace qh
