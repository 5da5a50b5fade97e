// kernels_inner.hip.h -- <a|b> of two states that both live in HBM (qh_inner): sum_i conj(a_i) b_i by LOGICAL index.
//
// The operation of the two-state walks (kernels_two_state.hip.h) that loads both states, stores nothing and adds
// conj(a) b to the thread's (re, im).  Sums are in double from the stored amplitudes and in the fixed order of
// kernels_common.hip.h, no atomics: the same states in the same layouts give bitwise the same result.  Im is formed from two
// ROUNDED products (no fused multiply-add): for b == a, or b a bitwise copy of a, every item's ar*bi - ai*br is exactly 0.
#pragma once
#include <hip/hip_runtime.h>

#include "kernels_common.hip.h"

namespace qh {

__device__ __forceinline__ void inner_acc(double ar, double ai, double br, double bi, double &re, double &im) {
#pragma clang fp contract(off)
  re += ar * br + ai * bi;
  im += ar * bi - ai * br;
}

struct InnerOp {
  static constexpr bool RD = true, RS = true, kWrites = false;
  __device__ __forceinline__ bool sums() const { return true; }
  __device__ __forceinline__ void item(const void *, const Item16<double>::vec &a, const Item16<double>::vec &b, double &re, double &im) const {
    inner_acc(a.x, a.y, b.x, b.y, re, im);
  }
  __device__ __forceinline__ void item(const void *, const Item16<float>::vec &a, const Item16<float>::vec &b, double &re, double &im) const {
    inner_acc((double)a.x, (double)a.y, (double)b.x, (double)b.y, re, im);
    inner_acc((double)a.z, (double)a.w, (double)b.z, (double)b.w, re, im);
  }
  template <typename A> __device__ __forceinline__ void amp(const A *, const A &a, const A &b, double &re, double &im) const {
    inner_acc((double)a.x, (double)a.y, (double)b.x, (double)b.y, re, im);
  }
};

}  // namespace qh
