// kernels_zpoly.hip.h -- diagonal Z-polynomial operators (qh_apply_zpoly, qh_expect_zpoly):
//   f(i) = sum_t w_t (-1)^popcount(i & pz_t),   apply: a_i *= exp(c f(i)),   expect: sum |a_i|^2 (1, f, f^2).
//
// One kernel, one read (apply: and one write) of the state for any number of terms.  The walk is k_pauli_product's DIAG
// kind: 256 threads, Item16 items, thread t takes items t + 256 u, u < kPauliPer, of a chunk (8 loads in flight), at most
// kPauliBlocks blocks, each a contiguous run of chunks; loads non-temporal, the apply kernel's stores too.
//
// f by the classes of zpoly_plan.h, whose device block (ZpolyArgs::wd / md) the kernels read uniformly and never write:
//   once per kernel   each thread sums the LOW terms for its kPauliPer x (1 or 2) amplitudes: registers;
//   once per chunk    the block forms coef[0] = the CONST and HIGH terms' sum and coef[g] = g_L(q) of every group: wave v takes
//                     segments v, v + 4, ...; its lanes take the segment's terms 64 apart, then wave_sum.  The results and
//                     (once per kernel) the groups' low masks sit in LDS, and so do the segments' terms themselves where
//                     there are at most kZpolyLdsTerms of them: a chunk then waits for LDS, not for dependent global loads.
//                     This runs while the chunk's loads are in flight.
//                     Then, still once per chunk: each thread adds the groups whose low mask lies on thread bits only, with
//                     its sign, to coef[0] (base); threads 0 .. 8 H - 1 add those on register-index and half bits only into one
//                     value per (u, half) cell, in LDS.  A 2-local cost function has no other group.
//   per amplitude     f = (base + low) + cell + sum over the MIXED groups of +-coef[g] (the sign being the parity of the low
//                     index under the group's low mask).  Then one sincos (one exp more unless c.re == 0, a uniform test), one
//                     complex product in double, one rounding to the handle's width.
// The next chunk's loads are issued before the current chunk's arithmetic (two sets of kPauliPer items in registers).
// The order of every sum is fixed by the term list, the layout and the grid: no atomics.
//
// norm / moments: thread (chunks in order, u in order, halves in order) -> block_row_sum -> k_slab_fold.
//
// k_zpoly_small: states below one chunk.  One amplitude per thread, f by popcount over the terms as given; both operations.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels_common.hip.h"
#include "kernels_gate.hip.h"
#include "kernels_pauli.hip.h"
#include "zpoly_plan.h"

namespace qh {

struct ZpolyArgs {
  const double *wd;
  const uint64_t *md;
  uint32_t nseg, nlow, nterms;
  uint32_t nseg_terms, cached;   // the segments' terms; 1: the kernel keeps them in LDS
  uint32_t ngt, ngu;             // groups on thread bits only / on register-index and half bits only (the first segments)
  uint32_t off_lw, off_sc, off_gl, off_lm;
  double cre, cim;
  int norm;                      // apply: sum |new|^2 into the slab
  uint32_t cpb;                  // chunks per block
};

__device__ __forceinline__ double zpoly_signed(double v, uint32_t neg) { return neg ? -v : v; }

// exp(c f) as (re, im)
__device__ __forceinline__ void zpoly_factor(double cre, double cim, double f, double &fr, double &fi) {
  double s, c;
  sincos(cim * f, &s, &c);
  if (cre != 0.0) {
    const double e = exp(cre * f);
    s *= e;
    c *= e;
  }
  fr = c;
  fi = s;
}

// The evaluator both main kernels share.  LDS: doubles coef[nseg], cell[kZpolyCells], tw[nseg_terms]; then words glow[nseg],
// soff[nseg + 1], tsc[nseg_terms] -- tw, soff and tsc (the segments' weights, bounds and chunk masks) only where cached.
constexpr int kZpolyCells = 2 * kPauliPer;      // (u, half) cells of a thread's part of a chunk, at the most
constexpr uint32_t kZpolyLdsTerms = 2048;       // (2049 segments and 2048 terms: 56 KiB)
constexpr size_t zpoly_lds_bytes(uint32_t nseg, uint32_t nseg_terms, bool cached) {
  return (size_t)nseg * 12 + kZpolyCells * 8 + (cached ? (size_t)nseg_terms * 12 + ((size_t)nseg + 1) * 4 : 0);
}

template <typename R> struct ZpolyEval {
  static constexpr int AB = Item16<R>::kAmpBits, H = 1 << AB, U = kPauliPer;
  double *coef, *cell, *tw;
  uint32_t *glow, *soff, *tsc;
  double low[U][H];      // the thread's LOW sums
  double base;           // coef[0] + the thread-only groups, of the current chunk

  // once per kernel (ends with a barrier)
  __device__ __forceinline__ void setup(const ZpolyArgs &a, unsigned char *lds) {
    coef = (double *)lds;
    cell = coef + a.nseg;
    tw = cell + kZpolyCells;
    glow = (uint32_t *)(tw + (a.cached ? a.nseg_terms : 0u));
    soff = glow + a.nseg;
    tsc = soff + a.nseg + 1;
    const uint32_t tid = threadIdx.x;
    for (uint32_t s = tid; s < a.nseg; s += 256) glow[s] = (uint32_t)a.md[a.off_gl + s];
    if (a.cached) {
      for (uint32_t s = tid; s <= a.nseg; s += 256) soff[s] = (uint32_t)a.md[s];
      for (uint32_t j = tid; j < a.nseg_terms; j += 256) {
        tw[j] = a.wd[j];
        tsc[j] = (uint32_t)a.md[a.off_sc + j];
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int k = 0; k < H; ++k) low[u][k] = 0.0;
    for (uint32_t j = 0; j < a.nlow; ++j) {
      const double w = a.wd[a.off_lw + j];
      const uint32_t m = (uint32_t)a.md[a.off_lm + j];
      const uint32_t tp = __builtin_popcount(tid & (m >> AB) & 255u) & 1u;
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const uint32_t up = tp ^ (__builtin_popcount((uint32_t)u & (m >> (AB + 8))) & 1u);
#pragma unroll
        for (int k = 0; k < H; ++k) low[u][k] += zpoly_signed(w, up ^ ((uint32_t)k & m & 1u));
      }
    }
    __syncthreads();
  }

  // once per chunk: coef[] of chunk q (a barrier before, so that nobody still reads the last chunk's, and one after)
  __device__ __forceinline__ void chunk(const ZpolyArgs &a, uint64_t q) {
    const uint32_t lane = threadIdx.x & 63u, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    __syncthreads();
    for (uint32_t s = wave; s < a.nseg; s += 4) {
      double acc = 0.0;
      if (a.cached) {
        const uint32_t b = soff[s], e = soff[s + 1];
        for (uint32_t j = b + lane; j < e; j += 64) acc += zpoly_signed(tw[j], __builtin_popcount((uint32_t)q & tsc[j]) & 1u);
      } else {
        const uint32_t b = (uint32_t)a.md[s], e = (uint32_t)a.md[s + 1];
        for (uint32_t j = b + lane; j < e; j += 64) acc += zpoly_signed(a.wd[j], __builtin_popcountll(q & a.md[a.off_sc + j]) & 1u);
      }
      acc = wave_sum(acc);
      if (lane == 0) coef[s] = acc;
    }
    __syncthreads();
    const uint32_t tid = threadIdx.x;
    base = coef[0];
    for (uint32_t s = 1; s < 1 + a.ngt; ++s) base += zpoly_signed(coef[s], __builtin_popcount(tid & (glow[s] >> AB) & 255u) & 1u);
    if (a.ngu) {
      if (tid < (uint32_t)(U * H)) {
        const uint32_t u = tid >> AB, k = tid & (uint32_t)(H - 1);
        double acc = 0.0;
        for (uint32_t s = 1 + a.ngt; s < 1 + a.ngt + a.ngu; ++s) {
          const uint32_t m = glow[s];
          acc += zpoly_signed(coef[s], (__builtin_popcount(u & (m >> (AB + 8))) & 1u) ^ (k & m & 1u));
        }
        cell[tid] = acc;
      }
      __syncthreads();
    }
  }

  // f of the thread's U x H amplitudes of the current chunk
  __device__ __forceinline__ void eval(const ZpolyArgs &a, double (&f)[U][H]) const {
    const uint32_t tid = threadIdx.x;
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int k = 0; k < H; ++k) f[u][k] = base + low[u][k];
    if (a.ngu) {
#pragma unroll
      for (int u = 0; u < U; ++u)
#pragma unroll
        for (int k = 0; k < H; ++k) f[u][k] += cell[u * H + k];
    }
    for (uint32_t s = 1 + a.ngt + a.ngu; s < a.nseg; ++s) {
      const uint32_t m = __builtin_amdgcn_readfirstlane(glow[s]);
      const double ct = zpoly_signed(coef[s], __builtin_popcount(tid & (m >> AB) & 255u) & 1u);
      const uint32_t mu = m >> (AB + 8);
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const uint32_t up = __builtin_popcount((uint32_t)u & mu) & 1u;
#pragma unroll
        for (int k = 0; k < H; ++k) f[u][k] += zpoly_signed(ct, up ^ ((uint32_t)k & m & 1u));
      }
    }
  }
};

template <typename R>
__global__ __launch_bounds__(256) void k_zpoly_apply(typename Item16<R>::vec *__restrict__ psi, ZpolyArgs a, double *__restrict__ slab) {
  using V = typename Item16<R>::vec;
  constexpr int H = ZpolyEval<R>::H, U = kPauliPer;
  extern __shared__ __attribute__((aligned(16))) unsigned char zpoly_lds[];
  ZpolyEval<R> ev;
  ev.setup(a, zpoly_lds);
  const uint32_t tid = threadIdx.x;
  double n2 = 0.0;
  const uint64_t q0 = (uint64_t)blockIdx.x * a.cpb;
  V v[U], nx[U];
#pragma unroll
  for (int u = 0; u < U; ++u) v[u] = __builtin_nontemporal_load(psi + pauli_item(q0, (uint32_t)u, tid));
  for (uint64_t q = q0; q < q0 + a.cpb; ++q) {
    if (q + 1 < q0 + a.cpb) {
#pragma unroll
      for (int u = 0; u < U; ++u) nx[u] = __builtin_nontemporal_load(psi + pauli_item(q + 1, (uint32_t)u, tid));
    }
    ev.chunk(a, q);
    double f[U][H];
    ev.eval(a, f);
#pragma unroll
    for (int u = 0; u < U; ++u) {
      V o;
#pragma unroll
      for (int k = 0; k < H; ++k) {
        double fr, fi;
        zpoly_factor(a.cre, a.cim, f[u][k], fr, fi);
        const double xr = (double)v[u][2 * k], xi = (double)v[u][2 * k + 1];
        const R nr = (R)__builtin_fma(-xi, fi, xr * fr), ni = (R)__builtin_fma(xi, fr, xr * fi);
        o[2 * k] = nr;
        o[2 * k + 1] = ni;
        if (a.norm) n2 += prob_sum(nr, ni);
      }
      __builtin_nontemporal_store(o, psi + pauli_item(q, (uint32_t)u, tid));
    }
    if (q + 1 < q0 + a.cpb) {
#pragma unroll
      for (int u = 0; u < U; ++u) v[u] = nx[u];
    }
  }
  if (a.norm) {
    const double row[1] = {n2};
    block_row_sum(row, slab);
  }
}

template <typename R>
__global__ __launch_bounds__(256) void k_zpoly_expect(const typename Item16<R>::vec *__restrict__ psi, ZpolyArgs a, double *__restrict__ slab) {
  using V = typename Item16<R>::vec;
  constexpr int H = ZpolyEval<R>::H, U = kPauliPer;
  extern __shared__ __attribute__((aligned(16))) unsigned char zpoly_lds[];
  ZpolyEval<R> ev;
  ev.setup(a, zpoly_lds);
  const uint32_t tid = threadIdx.x;
  double m0 = 0.0, m1 = 0.0, m2 = 0.0;
  const uint64_t q0 = (uint64_t)blockIdx.x * a.cpb;
  V v[U], nx[U];
#pragma unroll
  for (int u = 0; u < U; ++u) v[u] = __builtin_nontemporal_load(psi + pauli_item(q0, (uint32_t)u, tid));
  for (uint64_t q = q0; q < q0 + a.cpb; ++q) {
    if (q + 1 < q0 + a.cpb) {
#pragma unroll
      for (int u = 0; u < U; ++u) nx[u] = __builtin_nontemporal_load(psi + pauli_item(q + 1, (uint32_t)u, tid));
    }
    ev.chunk(a, q);
    double f[U][H];
    ev.eval(a, f);
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int k = 0; k < H; ++k) {
        const double p = prob_sum(v[u][2 * k], v[u][2 * k + 1]), pf = p * f[u][k];
        m0 += p;
        m1 += pf;
        m2 = __builtin_fma(pf, f[u][k], m2);
      }
    if (q + 1 < q0 + a.cpb) {
#pragma unroll
      for (int u = 0; u < U; ++u) v[u] = nx[u];
    }
  }
  const double row[3] = {m0, m1, m2};
  block_row_sum(row, slab);
}

// n amplitudes, one per thread; blocks of 256, one slab row each (EXPECT: three columns, otherwise one, written if a.norm)
template <typename R, bool EXPECT>
__global__ __launch_bounds__(256) void k_zpoly_small(typename AmpT<R>::type *__restrict__ psi, ZpolyArgs a, uint64_t n, double *__restrict__ slab) {
  using A = typename AmpT<R>::type;
  const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  double m0 = 0.0, m1 = 0.0, m2 = 0.0;
  if (i < n) {
    double f = 0.0;
    for (uint32_t t = 0; t < a.nterms; ++t) f += zpoly_signed(a.wd[t], __builtin_popcountll(i & a.md[t]) & 1u);
    A v = psi[i];
    if constexpr (EXPECT) {
      const double p = prob_sum(v.x, v.y), pf = p * f;
      m0 = p;
      m1 = pf;
      m2 = pf * f;
    } else {
      double fr, fi;
      zpoly_factor(a.cre, a.cim, f, fr, fi);
      const double xr = (double)v.x, xi = (double)v.y;
      v.x = (R)__builtin_fma(-xi, fi, xr * fr);
      v.y = (R)__builtin_fma(xi, fr, xr * fi);
      psi[i] = v;
      m0 = prob_sum(v.x, v.y);
    }
  }
  if constexpr (EXPECT) {
    const double row[3] = {m0, m1, m2};
    block_row_sum(row, slab);
  } else if (a.norm) {
    const double row[1] = {m0};
    block_row_sum(row, slab);
  }
}

}  // namespace qh
