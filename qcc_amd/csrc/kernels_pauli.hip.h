// kernels_pauli.hip.h -- Pauli-sum operators on the device (qh_apply_pauli_sum): dst := (sum_t c_t P_t) src, out of place.
//
// The write-side sibling of kernels_expect.hip.h.  A term is two masks over PHYSICAL index bits and a coefficient
// c' = c * (-i)^nY * (shard sign), formed on the host:   (c P a)_i = c' * (-1)^popcount(i & z) * a_{i ^ x}.
// One kernel applies a BATCH of up to kPauliT terms, sorted by x.  Terms of one x mask (a group) share one partner read:
//   out_i = [acc] dst_i + sum_g w_g(i) * src_{i ^ x_g},   w_g(i) = sum over terms t of g of c'_t * (-1)^popcount(i & z_t).
//
// k_pauli_batch (pauli_plan.h has the index arithmetic): 256 threads, 16-byte items, thread t takes items t + 256 u,
// u < kPauliPer, of a chunk; at most kPauliBlocks blocks, each a contiguous run of chunks.  The partner of a group is ONE
// plain 16-byte load at item ^ (x >> amp bits): x bits inside a 128-byte line or on lane bits fetch the same lines in
// another lane order, so neither LDS nor a lane permutation is needed; at complex64 bit 0 of x swaps the two halves of the
// item in registers.  The partner loads of an item (and dst's own value when the batch accumulates) are issued before the
// arithmetic.  Instantiations: TT = 16 or 4 term slots (a batch of at most 4 terms takes the smaller), and GG group slots:
// GG = TT holds a partner per slot, 16 partner loads in flight per thread (TT = 16: one item per step, TT = 4: four);
// GG = 1 is a batch with ONE x mask -- a single string, a diagonal Hamiltonian -- and takes the thread's 8 items of a chunk
// in one step, 8 (+ 8) loads in flight.
// All loads and stores are lane-linear up to the XOR and non-temporal.
//
// Signs cost no per-term vector logic.  The chunk and register-index parts of i are wave-uniform: a scalar +-1.0 per term
// and item.  The thread part is folded into the thread's copy of c'_t once per kernel.  An item then costs two double FMAs
// per term (four at complex64: the sub-item bit of z gives the second half its own w) and one complex product per group.
// Terms sit in static slots; bit t of `start` says that slot t opens a group, so every register index is a constant.
//
// Arithmetic: every component in double from the stored amplitudes (complex64 widened unrounded), rounded once per batch
// to the handle's width.  unit != 0 (a batch of one term, first batch, c' = i^(unit - 1)): the partner is stored as it
// is, negated and / or with its components swapped -- c' = 1 stores the source bits.
//
// norm (uniform; nothing is summed or written to the slab without it): sum |a|^2 of the values AS STORED, in double, in the
// fixed order of kernels_common.hip.h -- thread (chunks in order, u in order, halves in order) -> block_row_sum ->
// k_slab_fold.  No atomics.
//
// k_pauli_small: states with fewer items than one chunk.  One amplitude per thread, signs by popcount.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels_common.hip.h"
#include "kernels_gate.hip.h"
#include "pauli_plan.h"

namespace qh {

struct PauliArgs {
  uint64_t px[kPauliT];        // physical x mask (local bits) of the group slot t opens; k_pauli_small: of every term
  uint64_t pz[kPauliT];        // physical z mask (k_pauli_small)
  uint32_t zc[kPauliT];        // PauliZSplit::chunk (at most 40 - 11 bits)
  double cre[kPauliT], cim[kPauliT];      // c'; 0 in unused slots
  uint16_t zu[kPauliT];        // PauliZSplit::reg
  uint8_t zt[kPauliT];         // PauliZSplit::thread
  uint32_t start;              // bit t: slot t opens a group
  uint32_t zh;                 // bit t: PauliZSplit::half
  int count;                   // terms of the batch
  int acc;                     // read dst and add to it (every batch but the first)
  int norm;                    // sum |new|^2 into the slab (the last batch)
  int unit;                    // 0, or 1 + k: the batch is one term with c' = i^k
  uint32_t cpb;                // chunks per block
};

// v * i^k: k & 1 swaps the components (times i), k & 2 negates
template <typename R> __device__ __forceinline__ void pauli_rot(R re, R im, uint32_t k, R &ore, R &oim) {
  const R r1 = (k & 1u) ? -im : re, i1 = (k & 1u) ? re : im;
  ore = (k & 2u) ? -r1 : r1;
  oim = (k & 2u) ? -i1 : i1;
}

__device__ __forceinline__ double pauli_pm1(uint32_t negative) { return __hiloint2double((int)(0x3FF00000u ^ (negative << 31)), 0); }

template <typename R, int TT, int GG>
__global__ __launch_bounds__(256) void k_pauli_batch(const typename Item16<R>::vec *__restrict__ src, typename Item16<R>::vec *__restrict__ dst,
                                                      PauliArgs a, double *__restrict__ slab) {
  using V = typename Item16<R>::vec;
  static_assert(GG == 1 || GG == TT, "one group, or a slot per term");
  constexpr int AB = Item16<R>::kAmpBits, H = 1 << AB, U = GG == 1 ? kPauliPer : kPauliT / TT;
  const uint32_t tid = threadIdx.x;
  double cr[TT], ci[TT];      // c' with the thread's part of the sign
#pragma unroll
  for (int t = 0; t < TT; ++t) {
    const bool neg = parity64(tid & a.zt[t]) != 0;
    cr[t] = neg ? -a.cre[t] : a.cre[t];
    ci[t] = neg ? -a.cim[t] : a.cim[t];
  }
  const uint32_t tp0 = parity64(tid & a.zt[0]);
  double n2 = 0.0;
  const uint64_t q0 = (uint64_t)blockIdx.x * a.cpb;
  for (uint64_t q = q0; q < q0 + a.cpb; ++q) {
    uint32_t m[TT];      // bit u: the sign of item u of this chunk, without the thread and half parts (wave-uniform)
#pragma unroll
    for (int t = 0; t < TT; ++t) m[t] = (uint32_t)a.zu[t] ^ (0u - (uint32_t)(__builtin_popcount((uint32_t)q & a.zc[t]) & 1));
#pragma unroll
    for (int u0 = 0; u0 < kPauliPer; u0 += U) {
      V v[U][GG], d[U];
#pragma unroll
      for (int uu = 0; uu < U; ++uu) {
        const uint64_t item = pauli_item(q, (uint32_t)(u0 + uu), tid);
#pragma unroll
        for (int t = 0; t < GG; ++t)
          if ((a.start >> t) & 1u) v[uu][t] = __builtin_nontemporal_load(src + pauli_partner_item(item, a.px[t], AB));
        if (a.acc) d[uu] = __builtin_nontemporal_load(dst + item);
      }
#pragma unroll
      for (int uu = 0; uu < U; ++uu) {
        const int u = u0 + uu;
        V o;
        if (a.unit) {
          V p = v[uu][0];
          if constexpr (H == 2)
            if (a.px[0] & 1ull) p = V{p.z, p.w, p.x, p.y};
#pragma unroll
          for (int h = 0; h < H; ++h) {
            const uint32_t neg = ((m[0] >> u) & 1u) ^ tp0 ^ ((uint32_t)h & a.zh & 1u);
            R re, im;
            pauli_rot<R>(p[2 * h], p[2 * h + 1], (uint32_t)(a.unit - 1) + 2u * neg, re, im);
            o[2 * h] = re;
            o[2 * h + 1] = im;
          }
        } else {
          double wr[H], wi[H], outr[H], outi[H];
#pragma unroll
          for (int h = 0; h < H; ++h) {
            wr[h] = 0.0;
            wi[h] = 0.0;
            outr[h] = a.acc ? (double)d[uu][2 * h] : 0.0;
            outi[h] = a.acc ? (double)d[uu][2 * h + 1] : 0.0;
          }
          V cur = (V)0;
          auto flush = [&]() {
#pragma unroll
            for (int h = 0; h < H; ++h) {
              const double pr = (double)cur[2 * h], pi = (double)cur[2 * h + 1];
              outr[h] = __builtin_fma(wr[h], pr, outr[h]);
              outr[h] = __builtin_fma(-wi[h], pi, outr[h]);
              outi[h] = __builtin_fma(wr[h], pi, outi[h]);
              outi[h] = __builtin_fma(wi[h], pr, outi[h]);
              wr[h] = 0.0;
              wi[h] = 0.0;
            }
          };
#pragma unroll
          for (int t = 0; t < TT; ++t) {
            if ((t == 0 || GG > 1) && ((a.start >> t) & 1u)) {
              if (t) flush();
              cur = v[uu][t < GG ? t : 0];
              if constexpr (H == 2)
                if (a.px[t] & 1ull) cur = V{cur.z, cur.w, cur.x, cur.y};
            }
            const uint32_t sb = (m[t] >> u) & 1u;
#pragma unroll
            for (int h = 0; h < H; ++h) {
              const double s = pauli_pm1(sb ^ ((uint32_t)h & (a.zh >> t) & 1u));
              wr[h] = __builtin_fma(cr[t], s, wr[h]);
              wi[h] = __builtin_fma(ci[t], s, wi[h]);
            }
          }
          flush();
#pragma unroll
          for (int h = 0; h < H; ++h) {
            o[2 * h] = (R)outr[h];
            o[2 * h + 1] = (R)outi[h];
          }
        }
        if (a.norm) {
#pragma unroll
          for (int h = 0; h < H; ++h) n2 += prob_sum(o[2 * h], o[2 * h + 1]);
        }
        __builtin_nontemporal_store(o, dst + pauli_item(q, (uint32_t)u, tid));
      }
    }
  }
  if (a.norm) {
    const double row[1] = {n2};
    block_row_sum(row, slab);
  }
}

// n amplitudes, one per thread; blocks of 256, one slab row each
template <typename R>
__global__ __launch_bounds__(256) void k_pauli_small(const typename AmpT<R>::type *__restrict__ src, typename AmpT<R>::type *__restrict__ dst,
                                                      PauliArgs a, uint64_t n, double *__restrict__ slab) {
  using A = typename AmpT<R>::type;
  const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  double n2 = 0.0;
  if (i < n) {
    A o;
    if (a.unit) {
      const A p = src[i ^ a.px[0]];
      pauli_rot<R>(p.x, p.y, (uint32_t)(a.unit - 1) + 2u * parity64(i & a.pz[0]), o.x, o.y);
    } else {
      double wr = 0.0, wi = 0.0, outr = 0.0, outi = 0.0, pr = 0.0, pi = 0.0;
      if (a.acc) {
        outr = (double)dst[i].x;
        outi = (double)dst[i].y;
      }
      auto flush = [&]() {
        outr = __builtin_fma(wr, pr, outr);
        outr = __builtin_fma(-wi, pi, outr);
        outi = __builtin_fma(wr, pi, outi);
        outi = __builtin_fma(wi, pr, outi);
        wr = 0.0;
        wi = 0.0;
      };
#pragma unroll
      for (int t = 0; t < kPauliT; ++t) {
        if (t < a.count) {
          if ((a.start >> t) & 1u) {
            if (t) flush();
            const A p = src[i ^ a.px[t]];
            pr = (double)p.x;
            pi = (double)p.y;
          }
          const double s = parity64(i & a.pz[t]) ? -1.0 : 1.0;
          wr = __builtin_fma(a.cre[t], s, wr);
          wi = __builtin_fma(a.cim[t], s, wi);
        }
      }
      flush();
      o.x = (R)outr;
      o.y = (R)outi;
    }
    if (a.norm) n2 = prob_sum(o.x, o.y);
    dst[i] = o;
  }
  if (a.norm) {
    const double row[1] = {n2};
    block_row_sum(row, slab);
  }
}

}  // namespace qh
