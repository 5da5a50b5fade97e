// kernels_pauli_product.hip.h -- products of Pauli factors in place (qh_apply_pauli_product):
//   state := F_{n-1} ... F_0 state,   F_t = a_t I + b_t P_t.
//
// The in-place sibling of kernels_pauli.hip.h.  A term is two masks over PHYSICAL index bits and two coefficients, a and
// b' = b * (-i)^nY * (shard sign), formed on the host:   (F v)_i = a v_i + b' (-1)^popcount(i & z) v_{i ^ x}.
// A factor with x mask X is a 2x2 update of the disjoint pairs {i, i ^ X}; a diagonal factor (x == 0) acts on each amplitude
// alone.  One kernel applies a RUN of up to kPauliProdT terms whose x masks are 0 or one common X (pauli_product_plan.h), in
// the caller's order, in registers: one read and one write of the state, whatever the weight of the strings.
//
// k_pauli_product<R, TT, KIND>: 256 threads, 16-byte items, at most kPauliBlocks blocks, each a contiguous run of chunks.
//   DIAG  walks items; thread t takes items t + 256 u, u < kPauliPer, of a chunk: 8 loads in flight, one load and one store
//         per item.
//   PAIR  walks PAIR numbers laid out the same way; pair w names item0 = w with a 0 inserted at the pivot (the top bit of
//         X >> amp bits) and item1 = item0 ^ (X >> amp bits).  A thread owns both items of a pair: it loads both (8 + 8
//         loads in flight), applies the terms and stores both.  Pairs are disjoint: no LDS, no lane exchange, no atomics.
//         A pivot on a thread bit outside the 128-byte line makes the two loads of a wave take alternate whole lines, the
//         access shape of the k_pair* gate kernels.  At complex64 (item0, half) pairs with (item1, half ^ (X & 1)).
//   HALF  complex64 with X == 1: the pair is the two halves of one item; walks items as DIAG does.
//   LANE  (kPauliWalkLane; the plan says PAIR) a pivot inside the 128-byte line: walks items as DIAG does, so loads and stores
//         stay lane-linear; the partner item sits in lane ^ (X >> amp bits) of the same wave and arrives by __shfl_xor.  Both
//         threads of a pair update both values (the arithmetic is symmetric in the two) and each stores its own.
// A step's loads are issued before its arithmetic.  All loads and stores are non-temporal.
//
// Signs as in k_pauli_batch: the chunk and register-index parts of the index are wave-uniform, a scalar bit per term and
// item; the thread part is folded into the thread's copy of b' once per kernel; the partner's sign differs from the
// amplitude's own by a constant of the term (bit t of `flip`).  Terms sit in static slots -- slot t is live if t < count,
// a uniform test -- so every register index is a compile-time constant.  TT = kPauliProdT or kPauliProdSmallT slots.
//
// Arithmetic: every term in double on the amplitudes as stored (complex64 widened unrounded), rounded once per run.
// unit = 1 + k (a run of one term, a == 0, b' = i^k): the stored bits are moved, negated and / or with their components
// swapped.  unit = 5 (one term, a == 1, b == 0): every item is stored as it was loaded.
//
// norm (uniform): sum |v|^2 of the values AS STORED, in double, in the fixed order of kernels_common.hip.h -- thread (chunks
// in order, u in order, own amplitudes then partners) -> block_row_sum -> k_slab_fold.  No atomics.
//
// k_pauli_product_small: states with fewer pairs than one chunk.  One amplitude pair (DIAG: one amplitude) per thread, signs
// by popcount, from 1 local bit up.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels_common.hip.h"
#include "kernels_gate.hip.h"
#include "kernels_pauli.hip.h"
#include "pauli_product_plan.h"

namespace qh {

struct PauliProdArgs {
  double are[kPauliProdT], aim[kPauliProdT];      // a
  double bre[kPauliProdT], bim[kPauliProdT];      // b'
  uint32_t zc[kPauliProdT];      // PauliZSplit::chunk, over the walk's numbers (pair numbers for PAIR)
  uint16_t zu[kPauliProdT];      // PauliZSplit::reg
  uint8_t zt[kPauliProdT];       // PauliZSplit::thread
  uint32_t zh;                   // bit t: PauliZSplit::half
  uint32_t offd;                 // bit t: the term's x mask is X (it exchanges the pair); 0: diagonal
  uint32_t flip;                 // bit t: the partner's sign is the opposite of the amplitude's own
  uint64_t X;                    // the run's pair mask (physical, amplitude bits)
  int pivot;                     // PAIR: top bit of X >> amp bits; small kernel: top bit of X
  int count;                     // terms of the run
  int norm;                      // sum |new|^2 into the slab (the last run)
  int unit;                      // 0; 1 + k: one term, a == 0, b' = i^k; 5: one term, a == 1, b == 0
  uint32_t cpb;                  // chunks per block
};
// what k_pauli_product_small needs beside it: signs by popcount
struct PauliProdZ {
  uint64_t pz[kPauliProdT];      // physical z mask
};

// one term on one pair (x, y) -- or, DIAG, on x alone -- in double: w = b' with the sign of x
template <bool PAIRED>
__device__ __forceinline__ void pauli_factor(double ar, double ai, double wr, double wi, bool off, bool flip, double &xr, double &xi,
                                             double &yr, double &yi) {
  const double pr = (PAIRED && off) ? yr : xr, pi = (PAIRED && off) ? yi : xi;
  double nr = ar * xr, ni = ar * xi;
  nr = __builtin_fma(-ai, xi, nr);
  ni = __builtin_fma(ai, xr, ni);
  nr = __builtin_fma(wr, pr, nr);
  ni = __builtin_fma(wr, pi, ni);
  nr = __builtin_fma(-wi, pi, nr);
  ni = __builtin_fma(wi, pr, ni);
  if constexpr (PAIRED) {
    const double vr = flip ? -wr : wr, vi = flip ? -wi : wi;
    const double qr = off ? xr : yr, qi = off ? xi : yi;
    double mr = ar * yr, mi = ar * yi;
    mr = __builtin_fma(-ai, yi, mr);
    mi = __builtin_fma(ai, yr, mi);
    mr = __builtin_fma(vr, qr, mr);
    mi = __builtin_fma(vr, qi, mi);
    mr = __builtin_fma(-vi, qi, mr);
    mi = __builtin_fma(vi, qr, mi);
    yr = mr;
    yi = mi;
  }
  xr = nr;
  xi = ni;
}

template <typename R, int TT, int KIND>
__global__ __launch_bounds__(256) void k_pauli_product(typename Item16<R>::vec *__restrict__ psi, PauliProdArgs a, double *__restrict__ slab) {
  using V = typename Item16<R>::vec;
  constexpr int AB = Item16<R>::kAmpBits, H = 1 << AB, U = kPauliPer;
  constexpr bool PAIR = KIND == QH_PAULI_RUN_PAIR, HALF = KIND == QH_PAULI_RUN_HALF, LANE = KIND == kPauliWalkLane, PAIRED = PAIR || HALF || LANE;
  static_assert(!HALF || AB == 1, "HALF is a complex64 shape");
  constexpr int NP = HALF ? 1 : H;      // amplitudes of item0 that head a pair (DIAG: amplitudes of the item)
  const uint32_t tid = threadIdx.x;
  double br[TT], bi[TT];      // b' with the thread's part of the sign
#pragma unroll
  for (int t = 0; t < TT; ++t) {
    const bool neg = parity64(tid & a.zt[t]) != 0;
    br[t] = neg ? -a.bre[t] : a.bre[t];
    bi[t] = neg ? -a.bim[t] : a.bim[t];
  }
  const uint32_t tp0 = parity64(tid & a.zt[0]);
  const uint64_t xi = a.X >> AB;
  const bool cross = AB && (PAIR || LANE) && (a.X & 1ull);      // complex64: the pair also trades halves
  double n2 = 0.0;
  const uint64_t q0 = (uint64_t)blockIdx.x * a.cpb;
  for (uint64_t q = q0; q < q0 + a.cpb; ++q) {
    uint32_t m[TT];      // bit u: the sign of number u of this chunk, without the thread and half parts (wave-uniform)
#pragma unroll
    for (int t = 0; t < TT; ++t) m[t] = (uint32_t)a.zu[t] ^ (0u - (uint32_t)(__builtin_popcount((uint32_t)q & a.zc[t]) & 1));
    V v0[U], v1[U];
    uint64_t at0[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const uint64_t w = pauli_item(q, (uint32_t)u, tid);
      at0[u] = PAIR ? pauli_pair_item0(w, a.pivot) : w;
      v0[u] = __builtin_nontemporal_load(psi + at0[u]);
      if constexpr (PAIR) v1[u] = __builtin_nontemporal_load(psi + (at0[u] ^ xi));
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      // the element as NP pairs (x, y) of stored values; DIAG has no y
      R x[NP][2], y[NP][2];
      if constexpr (PAIR || LANE) {
        V p1;
        if constexpr (PAIR) {
          p1 = v1[u];
        } else {
#pragma unroll
          for (int c = 0; c < 2 * H; ++c) p1[c] = __shfl_xor(v0[u][c], (int)xi, 64);
        }
        if constexpr (H == 2)
          if (cross) p1 = V{p1.z, p1.w, p1.x, p1.y};
#pragma unroll
        for (int k = 0; k < NP; ++k) {
          x[k][0] = v0[u][2 * k];
          x[k][1] = v0[u][2 * k + 1];
          y[k][0] = p1[2 * k];
          y[k][1] = p1[2 * k + 1];
        }
      } else if constexpr (HALF) {
        x[0][0] = v0[u][0];
        x[0][1] = v0[u][1];
        y[0][0] = v0[u][2];
        y[0][1] = v0[u][3];
      } else {
#pragma unroll
        for (int k = 0; k < NP; ++k) {
          x[k][0] = v0[u][2 * k];
          x[k][1] = v0[u][2 * k + 1];
          y[k][0] = y[k][1] = (R)0;
        }
      }
      if (a.unit) {
        if (a.unit < 5) {
          const bool off = PAIRED && (a.offd & 1u);
#pragma unroll
          for (int k = 0; k < NP; ++k) {
            const uint32_t neg = ((m[0] >> u) & 1u) ^ tp0 ^ (HALF ? 0u : ((uint32_t)k & a.zh & 1u));
            const R sx0 = off ? y[k][0] : x[k][0], sx1 = off ? y[k][1] : x[k][1];
            const R sy0 = off ? x[k][0] : y[k][0], sy1 = off ? x[k][1] : y[k][1];
            pauli_rot<R>(sx0, sx1, (uint32_t)(a.unit - 1) + 2u * neg, x[k][0], x[k][1]);
            if constexpr (PAIRED) pauli_rot<R>(sy0, sy1, (uint32_t)(a.unit - 1) + 2u * (neg ^ (a.flip & 1u)), y[k][0], y[k][1]);
          }
        }
      } else {
#pragma unroll
        for (int k = 0; k < NP; ++k) {
          double xr = (double)x[k][0], xim = (double)x[k][1], yr = (double)y[k][0], yim = (double)y[k][1];
#pragma unroll
          for (int t = 0; t < TT; ++t) {
            if (t < a.count) {
              const uint32_t sb = ((m[t] >> u) & 1u) ^ (HALF ? 0u : ((uint32_t)k & (a.zh >> t) & 1u));
              const double s = pauli_pm1(sb);
              pauli_factor<PAIRED>(a.are[t], a.aim[t], br[t] * s, bi[t] * s, ((a.offd >> t) & 1u) != 0, ((a.flip >> t) & 1u) != 0, xr, xim,
                                   yr, yim);
            }
          }
          x[k][0] = (R)xr;
          x[k][1] = (R)xim;
          y[k][0] = (R)yr;
          y[k][1] = (R)yim;
        }
      }
      if (a.norm) {
#pragma unroll
        for (int k = 0; k < NP; ++k) n2 += prob_sum(x[k][0], x[k][1]);
        if constexpr (PAIR || HALF) {      // (LANE: the partner thread counts it)
#pragma unroll
          for (int k = 0; k < NP; ++k) n2 += prob_sum(y[k][0], y[k][1]);
        }
      }
      V o0, o1;
      if constexpr (HALF) {
        o0 = V{x[0][0], x[0][1], y[0][0], y[0][1]};
      } else {
#pragma unroll
        for (int k = 0; k < NP; ++k) {
          o0[2 * k] = x[k][0];
          o0[2 * k + 1] = x[k][1];
          o1[2 * k] = y[k][0];
          o1[2 * k + 1] = y[k][1];
        }
      }
      __builtin_nontemporal_store(o0, psi + at0[u]);
      if constexpr (PAIR) {
        if constexpr (H == 2)
          if (cross) o1 = V{o1.z, o1.w, o1.x, o1.y};
        __builtin_nontemporal_store(o1, psi + (at0[u] ^ xi));
      }
    }
  }
  if (a.norm) {
    const double row[1] = {n2};
    block_row_sum(row, slab);
  }
}

// nwork pairs (a.X != 0; amplitude i = w with a 0 inserted at a.pivot, partner i ^ X) or nwork amplitudes (a.X == 0), one
// per thread; blocks of 256, one slab row each
template <typename R>
__global__ __launch_bounds__(256) void k_pauli_product_small(typename AmpT<R>::type *__restrict__ psi, PauliProdArgs a, PauliProdZ zs,
                                                              uint64_t nwork, double *__restrict__ slab) {
  using A = typename AmpT<R>::type;
  const uint64_t w = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  const bool paired = a.X != 0;
  double n2 = 0.0;
  if (w < nwork) {
    const uint64_t i = paired ? pauli_insert0(w, a.pivot) : w, j = i ^ a.X;
    A vx = psi[i], vy = paired ? psi[j] : A{(R)0, (R)0};
    if (a.unit) {
      if (a.unit < 5) {
        const bool off = paired && (a.offd & 1u);
        const uint32_t neg = parity64(i & zs.pz[0]);
        const A sx = off ? vy : vx, sy = off ? vx : vy;
        pauli_rot<R>(sx.x, sx.y, (uint32_t)(a.unit - 1) + 2u * neg, vx.x, vx.y);
        pauli_rot<R>(sy.x, sy.y, (uint32_t)(a.unit - 1) + 2u * (neg ^ (a.flip & 1u)), vy.x, vy.y);
      }
    } else {
      double xr = (double)vx.x, xim = (double)vx.y, yr = (double)vy.x, yim = (double)vy.y;
#pragma unroll
      for (int t = 0; t < kPauliProdT; ++t) {
        if (t < a.count) {
          const double s = parity64(i & zs.pz[t]) ? -1.0 : 1.0;
          pauli_factor<true>(a.are[t], a.aim[t], a.bre[t] * s, a.bim[t] * s, ((a.offd >> t) & 1u) != 0, ((a.flip >> t) & 1u) != 0, xr, xim, yr,
                             yim);
        }
      }
      vx.x = (R)xr;
      vx.y = (R)xim;
      vy.x = (R)yr;
      vy.y = (R)yim;
    }
    psi[i] = vx;
    if (paired) psi[j] = vy;
    if (a.norm) n2 = prob_sum(vx.x, vx.y) + (paired ? prob_sum(vy.x, vy.y) : 0.0);
  }
  if (a.norm) {
    const double row[1] = {n2};
    block_row_sum(row, slab);
  }
}

}  // namespace qh
