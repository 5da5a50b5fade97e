// kernels_axpby.hip.h -- dst := alpha * dst + beta * src for two states that both live in HBM (qh_axpby), amplitude by
// amplitude, matched by LOGICAL index, written in place into dst where it lies.
//
// The operation of the two-state walks (kernels_two_state.hip.h, a = dst, b = src) that WRITES: it combines the pair and
// stores the new amplitude at dst's address, 16 bytes per lane in the linear walk at both widths, one amplitude (16 bytes of
// complex128, 8 of complex64) in the other two, non-temporal.
// RD = false (alpha == 0 exactly): dst's old values are never loaded -- NaN or Inf in them cannot propagate and the pass is
// two streams.  RS = false (beta == 0 exactly): src is never loaded; layouts then do not matter and the linear walk runs
// whatever the plan says.  Both false: one stream of zeros.
//
// Arithmetic: each component of the new amplitude is formed in double from the stored amplitudes, as
// (ar*dr - ai*di) + (br*sr - bi*si) and (ar*di + ai*dr) + (br*si + bi*sr) without fused multiply-adds, and rounded once to the
// handle's width.  A product whose COEFFICIENT component is exactly 0 is taken as 0 whatever the amplitude holds, so
// coefficients made of 0, 1 and -1 reproduce d + s, d - s, s ... as numbers (the sum of two floats formed in double and
// rounded to float equals the float sum: 53 >= 2 * 24 + 2 bits).
//
// norm (a uniform branch; nothing is summed or written to the slab without it): sum |a|^2 of the values AS STORED, after the
// rounding, in double and in the fixed order of the readers (kernels_common.hip.h), as the first of the walk's two sums.
// No atomics.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels_common.hip.h"

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
__device__ __forceinline__ Item16<double>::vec axpby_item(const AxpbyCoef &c, const Item16<double>::vec &d, const Item16<double>::vec &s,
                                                             double &n2) {
  Item16<double>::vec o;
  double re, im;
  axpby_round<double, RD, RS>(c, d.x, d.y, s.x, s.y, re, im, n2);
  o.x = re;
  o.y = im;
  return o;
}
template <bool RD, bool RS>
__device__ __forceinline__ Item16<float>::vec axpby_item(const AxpbyCoef &c, const Item16<float>::vec &d, const Item16<float>::vec &s,
                                                            double &n2) {
  Item16<float>::vec o;
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
  Item16<double>::vec v;
  v.x = re;
  v.y = im;
  __builtin_nontemporal_store(v, (Item16<double>::vec *)p);
}
__device__ __forceinline__ void axpby_store(float2 *p, float re, float im) {
  typedef float half_item __attribute__((ext_vector_type(2)));
  half_item v;
  v.x = re;
  v.y = im;
  __builtin_nontemporal_store(v, (half_item *)p);
}

template <bool RD_, bool RS_> struct AxpbyOp {
  static constexpr bool RD = RD_, RS = RS_, kWrites = true;
  AxpbyCoef c;
  __device__ __forceinline__ bool sums() const { return c.norm; }
  template <typename V> __device__ __forceinline__ void item(V *at, const V &d, const V &s, double &n2, double &) const {
    __builtin_nontemporal_store(axpby_item<RD, RS>(c, d, s, n2), at);
  }
  template <typename A> __device__ __forceinline__ void amp(A *at, const A &d, const A &s, double &n2, double &) const {
    decltype(d.x) outr, outi;
    axpby_round<decltype(d.x), RD, RS>(c, d.x, d.y, s.x, s.y, outr, outi, n2);
    axpby_store(at, outr, outi);
  }
};

}  // namespace qh
