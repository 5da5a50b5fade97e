// kernels_density.hip.h -- qh_reduced_density: rho = A A^H of the k listed bits, A of shape 2^k x 2^(nloc - k) (a ZHERK with
// the state as its only operand), walked as density_plan.h says.
//
//   * k_density_direct (k <= 2): a streaming read.  Every thread keeps the whole 2^k x 2^k tile (its upper triangle) in
//     registers and takes columns t, t + 256, ... of a chunk straight from global memory, 8 loads in flight; the 256
//     partial tiles of a workgroup are added by block_row_sum (kernels_common.hip.h).
//   * k_density_tiles (k >= 3): a chunk of columns of a tile of 2^KT rows (KT = min(k, 6)) goes into LDS once, with 16-byte
//     loads in physical order (consecutive lanes, consecutive addresses: runs of at least 2^min(6, chunk_bits)
//     amplitudes), widened to complex128 and stored column by column.  A thread owns a 4 x 4 block of complex accumulators:
//     rows ti + TR i and columns tj + TR j, TR = 2^(KT-2), interleaved so that the 16 lanes of an LDS read group read 16
//     consecutive slots.  Per column it reads 4 + 4 values and issues 64 FMAs.  The 4^(KT-2) thread tiles fill 256 / 4^(KT-2)
//     GROUPS of threads that take columns g, g + G, ... of the chunk; at the end the groups are added through LDS in group
//     order (columns of a tile are padded by one slot for KT < 6, so that the groups of a wave sit on different banks).
//     k = 7, 8 (PAIRS): the workgroup belongs to one block pair (R, C >= R) and keeps both blocks' rows of the chunk.
//   * Every workgroup writes its partial tile, 4^KT complex128 in kernel row order, to row blockIdx.x of the slab.
//     k_density_fold adds the rows of a pair in a fixed order (a wave per entry: a serial walk over 2048 rows cost more
//     than the read of the state), sets the imaginary part of a diagonal entry to 0.0, maps kernel row numbers to the
//     caller's (row_bit) and writes every entry of one triangle and its conjugate mirror: the other triangle of a diagonal
//     tile is computed by the tile kernel but never read.
//   * k_density_gather (fewer than 8 local bits): one workgroup, thread by output entry, the same fold arithmetic.
// No float atomics anywhere: the same state in the same layout gives the same bits.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "density_plan.h"
#include "kernels_common.hip.h"
#include "kernels_gate.hip.h"

namespace qh {

struct DensityArgs {
  uint8_t upos[12];      // bit i of an in-chunk amplitude index (tile rows and chunk columns merged, ascending) is this position
  uint8_t udst[12];      // ... and lands on this bit of (row | column << 16)
  uint8_t row_pos[8];    // qh_density_tiles
  uint8_t col_pos[12];
  uint8_t rest_pos[40];
  int k, kt, cb, nrest;
  uint64_t rest_mask;    // the rest positions as a mask: the next chunk's offset is ((offset | ~rest_mask) + 1) & rest_mask
  uint32_t wgpp;         // workgroups per block pair
  uint64_t cpw;          // chunks per workgroup
};
struct DensityFoldArgs {
  uint8_t row_bit[8];
  int k, kt;
  uint32_t wgpp, npairs;
};
struct DensityGatherArgs {
  uint8_t row_pos[8], row_bit[8], rest_pos[8];
  int k, ne;
};

__device__ __forceinline__ uint64_t density_spread(uint64_t v, const uint8_t *pos, int n) {
  uint64_t o = 0;
  for (int b = 0; b < n; ++b) o |= ((v >> b) & 1ull) << pos[b];
  return o;
}
template <typename R, int K>
__global__ __launch_bounds__(256) void k_density_direct(const typename AmpT<R>::type *__restrict__ psi, DensityArgs a, double *__restrict__ slab) {
  using A = typename AmpT<R>::type;
  constexpr int NR = 1 << K, NL = 8 >> K;      // rows; columns a thread has in flight
  const uint32_t tid = threadIdx.x, ncols = 1u << a.cb;
  uint64_t rowoff[NR];
#pragma unroll
  for (int r = 0; r < NR; ++r) rowoff[r] = density_spread((uint64_t)r, a.row_pos, K);
  const uint64_t lo = density_spread(tid, a.col_pos, a.cb < 8 ? a.cb : 8);
  double re[NR][NR], im[NR][NR];
#pragma unroll
  for (int r = 0; r < NR; ++r)
#pragma unroll
    for (int c = 0; c < NR; ++c) re[r][c] = im[r][c] = 0.0;
  // the tables are read once: a chunk costs three scalar operations for its offset, not a walk over the positions
  uint64_t offu[NL];
#pragma unroll
  for (int u = 0; u < NL; ++u) offu[u] = density_spread((uint64_t)u, a.col_pos + 8, a.cb - 8);      // (a.cb <= 8: only u = 0 is live)
  uint64_t qoff = density_spread((uint64_t)blockIdx.x * a.cpw, a.rest_pos, a.nrest);
  for (uint64_t i = 0; i < a.cpw; ++i, qoff = ((qoff | ~a.rest_mask) + 1) & a.rest_mask) {
    A v[NL][NR];
#pragma unroll
    for (int u = 0; u < NL; ++u) {
      const uint64_t off = qoff | offu[u] | lo;
#pragma unroll
      for (int r = 0; r < NR; ++r) {
        v[u][r].x = 0;
        v[u][r].y = 0;
        if (tid + 256u * u < ncols) v[u][r] = ld_amp<true>(psi + (off | rowoff[r]));
      }
    }
#pragma unroll
    for (int u = 0; u < NL; ++u)
#pragma unroll
      for (int r = 0; r < NR; ++r)
#pragma unroll
        for (int c = r; c < NR; ++c) {
          const double xr = (double)v[u][r].x, xi = (double)v[u][r].y, yr = (double)v[u][c].x, yi = (double)v[u][c].y;
          re[r][c] = __builtin_fma(xi, yi, __builtin_fma(xr, yr, re[r][c]));
          im[r][c] = __builtin_fma(-xr, yi, __builtin_fma(xi, yr, im[r][c]));
        }
  }
  double row[2 * NR * NR];
#pragma unroll
  for (int r = 0; r < NR; ++r)
#pragma unroll
    for (int c = 0; c < NR; ++c) {
      row[2 * (r * NR + c)] = re[r][c];
      row[2 * (r * NR + c) + 1] = im[r][c];
    }
  block_row_sum(row, slab);
}

template <typename R, int KT, bool PAIRS>
__global__ __launch_bounds__(256, 4) void k_density_tiles(const typename AmpT<R>::type *__restrict__ psi, DensityArgs a, double2 *__restrict__ slab) {
  using V = typename Item16<R>::vec;
  constexpr int AB = Item16<R>::kAmpBits;
  constexpr int NROW = 1 << KT, TR = 1 << (KT - 2), NT = TR * TR, G = 256 / NT;
  constexpr int STR = NROW + (KT < 6 ? 1 : 0);                      // slots per column
  constexpr int NCOL = 1 << (kDensityLdsBits - KT - (PAIRS ? 1 : 0));
  constexpr int NLOAD = (NROW * NCOL) >> (8 + AB);                  // items per thread and tile
  static_assert(KT >= 3 && KT <= kDensityTileBits && (!PAIRS || KT == kDensityTileBits), "tile shapes");
  static_assert(NLOAD >= 1 && (G == 1 || (size_t)NCOL * STR * 16 >= (size_t)256 * 8 * 16), "the group fold reuses the chunk's LDS");
  __shared__ double2 tile[PAIRS ? 2 : 1][NCOL * STR];
  const uint32_t tid = threadIdx.x, g = tid / NT, tt = tid % NT, ti = tt / TR, tj = tt % TR;
  const int nu = a.kt + a.cb;
  const uint32_t nitems = 1u << (nu - AB), ncols = 1u << a.cb;
  uint32_t pair = 0, w = blockIdx.x, bR = 0, bC = 0;
  uint64_t baseR = 0, baseC = 0;
  if constexpr (PAIRS) {
    pair = blockIdx.x / a.wgpp;
    w = blockIdx.x % a.wgpp;
    density_pair(1u << (a.k - KT), pair, &bR, &bC);
    baseR = density_spread(bR, a.row_pos + KT, a.k - KT);
    baseC = density_spread(bC, a.row_pos + KT, a.k - KT);
  }
  // this thread's items tid + 256 u inside a chunk of a tile: where they are in memory and in LDS, without the bits of u
  const int nlo = nu - AB < 8 ? nu - AB : 8;
  uint64_t goff_lo = 0;
  uint32_t rc_lo = 0;
  for (int b = 0; b < nlo; ++b) {
    const uint32_t bit = (tid >> b) & 1u;
    goff_lo |= (uint64_t)bit << a.upos[AB + b];
    rc_lo |= bit << a.udst[AB + b];
  }
  double re[4][4], im[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) re[i][j] = im[i][j] = 0.0;
  const double2 *ta = tile[0], *tb = tile[(PAIRS && bC != bR) ? 1 : 0];
  // ... and with them, per u; the tables are read once: a chunk costs three scalar operations for its offset
  uint64_t goff[NLOAD];
  uint32_t rc[NLOAD];
#pragma unroll
  for (int u = 0; u < NLOAD; ++u) {
    goff[u] = 0;      // (uniform: scalar registers)
    rc[u] = 0;
    for (int b = 8; b < nu - AB; ++b) {
      const uint32_t bit = ((uint32_t)u >> (b - 8)) & 1u;
      goff[u] |= (uint64_t)bit << a.upos[AB + b];
      rc[u] |= bit << a.udst[AB + b];
    }
  }
  const uint32_t rc_odd = AB ? 1u << a.udst[0] : 0u;      // (complex64: the item's second amplitude, position 0)
  uint64_t qoff = density_spread((uint64_t)w * a.cpw, a.rest_pos, a.nrest);
  for (uint64_t c = 0; c < a.cpw; ++c, qoff = ((qoff | ~a.rest_mask) + 1) & a.rest_mask) {
    __syncthreads();      // the previous chunk has been read
#pragma unroll
    for (int s = 0; s < (PAIRS ? 2 : 1); ++s) {
      if (s == 1 && bC == bR) break;
      const typename AmpT<R>::type *__restrict__ src = psi + (qoff | (s ? baseC : baseR));
      V v[NLOAD];
#pragma unroll
      for (int u = 0; u < NLOAD; ++u) {
        v[u] = (V)0;      // (AB = 1: position 0 is upos[0], outside goff: the offsets are even)
        if (tid + 256u * u < nitems) v[u] = __builtin_nontemporal_load((const V *)(src + (goff_lo | goff[u])));
      }
#pragma unroll
      for (int u = 0; u < NLOAD; ++u) {
        if (tid + 256u * u < nitems) {
          const uint32_t rc0 = rc_lo | rc[u];
          tile[s][(rc0 >> 16) * STR + (rc0 & 0xffffu)] = make_double2((double)v[u].x, (double)v[u].y);
          if constexpr (AB == 1) {
            const uint32_t rc1 = rc0 | rc_odd;
            tile[s][(rc1 >> 16) * STR + (rc1 & 0xffffu)] = make_double2((double)v[u].z, (double)v[u].w);
          }
        }
      }
    }
    __syncthreads();
    for (uint32_t e = g; e < ncols; e += G) {
      const double2 *ca = ta + e * STR + ti, *cc = tb + e * STR + tj;
      double2 x[4], y[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) x[i] = ca[TR * i];
#pragma unroll
      for (int j = 0; j < 4; ++j) y[j] = cc[TR * j];
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          re[i][j] = __builtin_fma(x[i].y, y[j].y, __builtin_fma(x[i].x, y[j].x, re[i][j]));
          im[i][j] = __builtin_fma(-x[i].x, y[j].y, __builtin_fma(x[i].y, y[j].x, im[i][j]));
        }
    }
  }
  double2 *__restrict__ row = slab + (uint64_t)blockIdx.x * (NROW * NROW);
  if constexpr (G == 1) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) row[(ti + TR * i) * NROW + tj + TR * j] = make_double2(re[i][j], im[i][j]);
  } else {
    // the groups through LDS, two accumulator rows at a time: F[g][thread tile][8 entries], added in group order
    double2 *F = &tile[0][0];
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      __syncthreads();
#pragma unroll
      for (int v = 0; v < 8; ++v) F[(g * NT + tt) * 8 + v] = make_double2(re[2 * p + v / 4][v % 4], im[2 * p + v / 4][v % 4]);
      __syncthreads();
      for (uint32_t el = tid; el < NT * 8; el += 256) {
        double2 s = F[el];
        for (uint32_t gg = 1; gg < G; ++gg) {
          const double2 t = F[gg * NT * 8 + el];
          s.x += t.x;
          s.y += t.y;
        }
        const uint32_t t2 = el / 8, v = el % 8, i = 2 * p + v / 4, j = v % 4;
        row[((t2 / TR) + TR * i) * NROW + (t2 % TR) + TR * j] = s;
      }
    }
  }
}

// one wave per (pair, entry of a tile): lane j adds the pair's slab rows j, j + 64, ... in workgroup order, the lanes are added
// by wave_sum's fixed tree, lane 0 scatters
__global__ __launch_bounds__(256) void k_density_fold(const double2 *__restrict__ slab, DensityFoldArgs f, double2 *__restrict__ out) {
  const uint32_t lane = threadIdx.x & 63u, idx = blockIdx.x * 4u + (threadIdx.x >> 6), tsz = 1u << (2 * f.kt);
  if (idx >= f.npairs * tsz) return;
  const uint32_t pair = idx >> (2 * f.kt), el = idx & (tsz - 1), tr = el >> f.kt, tc = el & ((1u << f.kt) - 1);
  uint32_t bR, bC;
  density_pair(1u << (f.k - f.kt), pair, &bR, &bC);
  const bool diag = bR == bC;
  if (diag && tr > tc) return;
  const double2 *p = slab + (uint64_t)pair * f.wgpp * tsz + el;
  double2 s = make_double2(0.0, 0.0);
  for (uint32_t w = lane; w < f.wgpp; w += 64) {
    const double2 t = p[(uint64_t)w * tsz];
    s.x += t.x;
    s.y += t.y;
  }
  s.x = wave_sum(s.x);
  s.y = wave_sum(s.y);
  if (lane != 0) return;
  const uint32_t kr = tr | (bR << f.kt), kc = tc | (bC << f.kt);
  uint32_t r = 0, c = 0;
  for (int j = 0; j < f.k; ++j) {
    r |= ((kr >> j) & 1u) << f.row_bit[j];
    c |= ((kc >> j) & 1u) << f.row_bit[j];
  }
  if (kr == kc) {
    out[((uint64_t)r << f.k) + c] = make_double2(s.x, 0.0);
    return;
  }
  out[((uint64_t)r << f.k) + c] = s;
  out[((uint64_t)c << f.k) + r] = make_double2(s.x, -s.y);
}

// nloc < 8: thread by entry (kernel row numbers kr <= kc), columns in order
template <typename R>
__global__ __launch_bounds__(256) void k_density_gather(const typename AmpT<R>::type *__restrict__ psi, DensityGatherArgs a, double2 *__restrict__ out) {
  const uint32_t n = 1u << (2 * a.k), ncols = 1u << a.ne;
  for (uint32_t idx = threadIdx.x; idx < n; idx += 256) {
    const uint32_t kr = idx >> a.k, kc = idx & ((1u << a.k) - 1);
    if (kr > kc) continue;
    const uint64_t offr = density_spread(kr, a.row_pos, a.k), offc = density_spread(kc, a.row_pos, a.k);
    double sr = 0.0, si = 0.0;
    for (uint32_t e = 0; e < ncols; ++e) {
      const uint64_t eo = density_spread(e, a.rest_pos, a.ne);
      const auto x = psi[eo | offr], y = psi[eo | offc];
      sr = __builtin_fma((double)x.y, (double)y.y, __builtin_fma((double)x.x, (double)y.x, sr));
      si = __builtin_fma(-(double)x.x, (double)y.y, __builtin_fma((double)x.y, (double)y.x, si));
    }
    uint32_t r = 0, c = 0;
    for (int j = 0; j < a.k; ++j) {
      r |= ((kr >> j) & 1u) << a.row_bit[j];
      c |= ((kc >> j) & 1u) << a.row_bit[j];
    }
    if (kr == kc) {
      out[((uint64_t)r << a.k) + c] = make_double2(sr, 0.0);
    } else {
      out[((uint64_t)r << a.k) + c] = make_double2(sr, si);
      out[((uint64_t)c << a.k) + r] = make_double2(sr, -si);
    }
  }
}

}  // namespace qh
