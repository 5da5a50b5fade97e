// kernels_mux.hip.h -- gates selected by a table (qh_apply_mux, qh_apply_diag): one read and one write of the state, the
// operand of every work item fetched from a table indexed by bits gathered from the amplitude's index.
//
//   qh_apply_mux   entry s = one 2x2 (4 amplitudes-wide complex numbers, row-major a b c d) applied to the target bit
//   qh_apply_diag  entry s = one complex factor
//
// The gather.  The host compiles the physical positions of the selection bits into at most 16 RUNS: a run of physically
// adjacent bits that feed adjacent table bits is one shift and one mask (TabGather).  A gather is a bitwise OR of
// fields, and so is the index of a work item: index = (the wave's tile base, wave-uniform) | (the lane's part, fixed
// for the whole kernel).  So s = gather(uniform part) | gather(lane part): the first is scalar arithmetic once per 64
// work items, the second is computed once per thread, and the cost per amplitude is one OR.
//
// Tiers (the host picks one per call, engine.hip pick_tier):
//   TAB_UNIFORM  no selector on a position that varies with the lane: the entry is wave-uniform, read by scalar loads
//                straight into SGPR operands (as k_dense_reg reads M) -- the kernel costs what k_pair does;
//   TAB_LDS      the table (after the shard restriction) is at most 64 KiB: staged in LDS once per block, the blocks
//                grid-stride over the tiles, entries come in by ds_read_b128.  A mux table is staged as four planes
//                (component c of entry s at c * entries + s): lanes with consecutive s read consecutive 16-byte slots;
//   TAB_GLOBAL   larger tables: ordinary cached loads through L2; the state stream stays non-temporal so that it does
//                not evict the table.
//
// Shapes.  A wave owns a tile of 64 * U consecutive work items and issues all its loads before the first result is
// needed: k_mux_pair (target bit >= 3) U = 4 pairs = 8 loads of 16 bytes in flight per thread; k_mux_line (target on
// bits 0-2, inside the 128-byte line) one amplitude per lane, U = 8, the partner by DPP as in k_pair_line, so no
// thread's pair straddles a line; k_diag_tab U = 16 amplitudes per thread.  Ragged tails (states smaller than a tile)
// take the guarded body; the loop condition is wave-uniform, so every lane of a wave reaches the DPP moves.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "kernels_gate.hip.h"

namespace qh {

constexpr int kMaxMuxBits = 16;
constexpr int kMaxTabRuns = 16;
constexpr size_t kTabLdsBytes = 64u << 10;      // two blocks per CU within the 160 KiB LDS
enum { TAB_UNIFORM = 1, TAB_LDS = 2, TAB_GLOBAL = 3 };

// run r: table bits [dst, dst + len) = index bits [src, src + len); packed src | dst << 8 | len << 16
struct TabGather {
  int n;
  uint32_t run[kMaxTabRuns];
};

__device__ __forceinline__ uint32_t tab_gather(uint64_t idx, const TabGather &g) {
  uint32_t s = 0;
#pragma nounroll
  for (int r = 0; r < g.n; ++r) {          // (a rolled loop over the kernel arguments: 16 unrolled runs spill SGPRs)
    const uint32_t w = g.run[r];
    s |= ((uint32_t)(idx >> (w & 0xffu)) & ((1u << (w >> 16)) - 1u)) << ((w >> 8) & 0xffu);
  }
  return s;
}

struct TabArgs {
  TabGather g;
  uint64_t nwork;     // work items: pairs (k_mux_pair) or amplitudes
  uint32_t nent;      // table entries (after the shard restriction)
  int p;              // target bit (mux)
};

__device__ __forceinline__ uint64_t insert_zero(uint64_t j, int p) {
  const uint64_t low = (1ull << p) - 1ull;
  return ((j & ~low) << 1) | (j & low);
}

extern __shared__ __attribute__((aligned(16))) char tab_smem[];

// C components per entry; plane layout (see the header)
template <int C, typename A> __device__ __forceinline__ void tab_stage(A *sm, const A *__restrict__ tab, uint32_t nent) {
  for (uint32_t i = threadIdx.x; i < nent * C; i += 256) sm[(i % C) * nent + i / C] = tab[i];
  __syncthreads();
}

// component c of entry s (C components per entry)
template <int TIER, int C, typename A>
__device__ __forceinline__ A tab_entry(const A *__restrict__ tab, const A *sm, uint32_t nent, uint32_t s, int c) {
  if constexpr (TIER == TAB_LDS) return sm[(uint32_t)c * nent + s];
  else return tab[(size_t)s * C + c];
}

__device__ __forceinline__ uint32_t wave_of_block() { return __builtin_amdgcn_readfirstlane(threadIdx.x >> 6); }

// ---- mux, target bit >= 3: one PAIR per work item ---------------------------------------------------------------
template <typename R, int TIER>
__global__ __launch_bounds__(256) void k_mux_pair(typename AmpT<R>::type *__restrict__ psi,
                                                   const typename AmpT<R>::type *__restrict__ tab, TabArgs a) {
  using A = typename AmpT<R>::type;
  constexpr int U = 4;
  A *sm = (A *)tab_smem;
  if constexpr (TIER == TAB_LDS) tab_stage<4, A>(sm, tab, a.nent);
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t lane_idx = insert_zero(lane, a.p), q2 = 1ull << a.p;
  const uint32_t s_lane = TIER == TAB_UNIFORM ? 0u : tab_gather(lane_idx, a.g);
  const uint64_t ntiles = (a.nwork + 64 * U - 1) / (64 * U);
  for (uint64_t t = (uint64_t)blockIdx.x * 4 + wave_of_block(); t < ntiles; t += (uint64_t)gridDim.x * 4) {
    auto body = [&](auto guard) {
      constexpr bool GUARD = decltype(guard)::value;
      A x[U], y[U];
      uint64_t idx[U];
      uint32_t s[U];
      bool ok[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const uint64_t jb = (t * U + u) * 64ull;                  // wave-uniform
        const uint64_t ib = insert_zero(jb, a.p);
        s[u] = tab_gather(ib, a.g) | s_lane;
        idx[u] = ib | lane_idx;
        ok[u] = !GUARD || jb + lane < a.nwork;
      }
#pragma unroll
      for (int u = 0; u < U; ++u)
        if (ok[u]) x[u] = ld_amp<true>(&psi[idx[u]]);
#pragma unroll
      for (int u = 0; u < U; ++u)
        if (ok[u]) y[u] = ld_amp<true>(&psi[idx[u] | q2]);
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (ok[u]) {
          const A g0 = tab_entry<TIER, 4>(tab, sm, a.nent, s[u], 0), g1 = tab_entry<TIER, 4>(tab, sm, a.nent, s[u], 1),
                  g2 = tab_entry<TIER, 4>(tab, sm, a.nent, s[u], 2), g3 = tab_entry<TIER, 4>(tab, sm, a.nent, s[u], 3);
          const Gate2<R> g{g0.x, g0.y, g1.x, g1.y, g2.x, g2.y, g3.x, g3.y};
          butterfly<R, A>(g, x[u], y[u]);
          st_amp<true>(&psi[idx[u]], x[u]);
          st_amp<true>(&psi[idx[u] | q2], y[u]);
        }
      }
    };
    if ((t + 1) * (64ull * U) <= a.nwork) body(std::false_type{});
    else body(std::true_type{});
  }
}

// value of lane l ^ (1 << p), p = 0..2 (wave-uniform p: one of three DPP sequences)
template <typename R> __device__ __forceinline__ R lane_xor_low(R v, int p) {
  if (p == 0) return lane_xor<0>(v);
  if (p == 1) return lane_xor<1>(v);
  return lane_xor<2>(v);
}

// ---- mux, target bit inside the line (0..2): one AMPLITUDE per work item, lane l and lane l ^ 2^p hold the pair ---
template <typename R, int TIER>
__global__ __launch_bounds__(256) void k_mux_line(typename AmpT<R>::type *__restrict__ psi,
                                                   const typename AmpT<R>::type *__restrict__ tab, TabArgs a) {
  using A = typename AmpT<R>::type;
  constexpr int U = 8;
  A *sm = (A *)tab_smem;
  if constexpr (TIER == TAB_LDS) tab_stage<4, A>(sm, tab, a.nent);
  const uint32_t lane = threadIdx.x & 63u;
  const bool hi = (lane >> a.p) & 1u;        // (index bit p == lane bit p: the 64 items of a wave row are consecutive indices)
  const int ca = hi ? 3 : 0, cb = hi ? 2 : 1;  // new = M[ca] * own + M[cb] * partner
  const uint32_t s_lane = TIER == TAB_UNIFORM ? 0u : tab_gather(lane, a.g);
  const uint64_t ntiles = (a.nwork + 64 * U - 1) / (64 * U);
  for (uint64_t t = (uint64_t)blockIdx.x * 4 + wave_of_block(); t < ntiles; t += (uint64_t)gridDim.x * 4) {
    auto body = [&](auto guard) {
      constexpr bool GUARD = decltype(guard)::value;
      A x[U];
      uint64_t idx[U];
      uint32_t s[U];
      bool ok[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const uint64_t jb = (t * U + u) * 64ull;                  // wave-uniform
        s[u] = tab_gather(jb, a.g) | s_lane;
        idx[u] = jb | lane;
        ok[u] = !GUARD || idx[u] < a.nwork;
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        x[u].x = (R)0;
        x[u].y = (R)0;
        if (ok[u]) x[u] = ld_amp<true>(&psi[idx[u]]);
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        A q;                                                       // every lane of the wave takes part in the moves
        q.x = lane_xor_low<R>(x[u].x, a.p);
        q.y = lane_xor_low<R>(x[u].y, a.p);
        if (ok[u]) {
          A ga, gb;
          if constexpr (TIER == TAB_UNIFORM) {                     // the whole entry is in SGPRs: select per lane
            const A g0 = tab_entry<TIER, 4>(tab, sm, a.nent, s[u], 0), g1 = tab_entry<TIER, 4>(tab, sm, a.nent, s[u], 1),
                    g2 = tab_entry<TIER, 4>(tab, sm, a.nent, s[u], 2), g3 = tab_entry<TIER, 4>(tab, sm, a.nent, s[u], 3);
            ga.x = hi ? g3.x : g0.x; ga.y = hi ? g3.y : g0.y;
            gb.x = hi ? g2.x : g1.x; gb.y = hi ? g2.y : g1.y;
          } else {
            ga = tab_entry<TIER, 4>(tab, sm, a.nent, s[u], ca);
            gb = tab_entry<TIER, 4>(tab, sm, a.nent, s[u], cb);
          }
          A o;
          o.x = (ga.x * x[u].x - ga.y * x[u].y) + (gb.x * q.x - gb.y * q.y);
          o.y = (ga.x * x[u].y + ga.y * x[u].x) + (gb.x * q.y + gb.y * q.x);
          st_amp<true>(&psi[idx[u]], o);
        }
      }
    };
    if ((t + 1) * (64ull * U) <= a.nwork) body(std::false_type{});
    else body(std::true_type{});
  }
}

// ---- diagonal over a register: a_i *= tab[s(i)] ------------------------------------------------------------------
template <typename R, int TIER>
__global__ __launch_bounds__(256) void k_diag_tab(typename AmpT<R>::type *__restrict__ psi,
                                                   const typename AmpT<R>::type *__restrict__ tab, TabArgs a) {
  using A = typename AmpT<R>::type;
  constexpr int U = 16;
  A *sm = (A *)tab_smem;
  if constexpr (TIER == TAB_LDS) tab_stage<1, A>(sm, tab, a.nent);
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t s_lane = TIER == TAB_UNIFORM ? 0u : tab_gather(lane, a.g);
  const uint64_t ntiles = (a.nwork + 64 * U - 1) / (64 * U);
  for (uint64_t t = (uint64_t)blockIdx.x * 4 + wave_of_block(); t < ntiles; t += (uint64_t)gridDim.x * 4) {
    auto body = [&](auto guard) {
      constexpr bool GUARD = decltype(guard)::value;
      A x[U];
      uint64_t idx[U];
      bool ok[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        idx[u] = ((t * U + u) * 64ull) | lane;
        ok[u] = !GUARD || idx[u] < a.nwork;
      }
#pragma unroll
      for (int u = 0; u < U; ++u)
        if (ok[u]) x[u] = ld_amp<true>(&psi[idx[u]]);
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (ok[u]) {
          const uint32_t s = tab_gather((t * U + u) * 64ull, a.g) | s_lane;
          const A f = tab_entry<TIER, 1>(tab, sm, a.nent, s, 0);
          A o;
          o.x = f.x * x[u].x - f.y * x[u].y;
          o.y = f.x * x[u].y + f.y * x[u].x;
          st_amp<true>(&psi[idx[u]], o);
        }
      }
    };
    if ((t + 1) * (64ull * U) <= a.nwork) body(std::false_type{});
    else body(std::true_type{});
  }
}

}  // namespace qh
