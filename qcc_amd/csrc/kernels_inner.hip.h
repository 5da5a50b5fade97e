// kernels_inner.hip.h -- <a|b> of two states that both live in HBM (qh_inner): sum_i conj(a_i) b_i by LOGICAL index.
//
// The two handles rarely share a physical layout (relayout sweeps leave a circuit-dependent bit map), and a reader does not
// move states: inner_plan.h turns the two bit maps into one of three walks.
//   * k_inner_linear (same layout): two linear streams, every lane 16 bytes per load (one complex128 amplitude, or two
//     consecutive complex64 ones), eight loads of each state in flight per thread, non-temporal.
//   * k_inner_tiles (different layouts, >= 8 local bits): tiles of 2^8 amplitudes chosen so that BOTH states are read in
//     runs of 16 consecutive amplitudes (256 bytes of complex128).  The 256 threads of a block enumerate a tile once in
//     a's order and once in b's order (thread r loads in-tile index r of each); b's values cross through LDS, where thread r
//     picks up slot shuffle(r), the partner of the amplitude of a it holds (slots are stored XOR-swizzled, slot s at
//     s ^ (s >> 4): a shuffle that sends a's low in-tile bits to b's high ones -- a bit reversal -- would otherwise have the
//     16 lanes of a read group 256 bytes apart, all on one bank group).  shuffle(r), the thread's offsets inside a tile
//     and the tile bases of a chunk of tiles are computed once per block; a tile costs two loads, one LDS write and one LDS
//     read per thread.  U tiles are in flight per thread.
//   * k_inner_gather (fewer than 8 local bits): one block, b's partner index bit by bit.
//
// Sums are in double from the stored amplitudes and in a fixed order, no atomics: thread (its items in order) -> wave (xor
// tree) -> the four waves in order -> one (re, im) row per block -> k_expect_fold adds the rows in block order.  The same
// states in the same layouts give bitwise the same result.  Im is formed from two ROUNDED products (no fused multiply-add):
// for b == a, or b a bitwise copy of a, every item's ar*bi - ai*br is exactly 0.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "inner_plan.h"
#include "kernels_expect.hip.h"

namespace qh {

constexpr int kInnerLoads = 8;          // k_inner_linear: loads of EACH state in flight per thread
constexpr int kInnerU = 4;              // k_inner_tiles: tiles in flight per thread (4 KiB of LDS each at complex128)
constexpr int kInnerChunkBits = 6;      // k_inner_tiles: tiles per chunk (their bases sit in LDS), at most 2^8

constexpr int kInnerMaxLocalBits = 40;  // what qh_create accepts (engine.hip check_args): at most 40 - 8 tile-number bits

struct InnerTileArgs {
  uint8_t tile_a[8], tile_b[8], shuffle[8];      // qh_inner_tiles
  uint8_t rest_a[kInnerMaxLocalBits], rest_b[kInnerMaxLocalBits];      // (the first nrest <= 32 entries are used)
  int nrest;                   // tile-number bits
  int cbits;                   // log2(tiles per chunk): min(kInnerChunkBits, nrest)
  uint32_t cpb;                // chunks per block
};
static_assert(sizeof(InnerTileArgs::rest_a) <= sizeof(qh_inner_tiles::rest_a) && kInnerMaxLocalBits - kInnerTileBits <= (int)sizeof(InnerTileArgs::rest_a),
              "the launch copies sizeof(InnerTileArgs::rest_a) bytes out of the plan's tables");
struct InnerGatherArgs {
  int nloc;
  uint8_t pos_b[8];
};

__device__ __forceinline__ void inner_acc(double ar, double ai, double br, double bi, double &re, double &im) {
#pragma clang fp contract(off)
  re += ar * br + ai * bi;
  im += ar * bi - ai * br;
}

// the block's (re, im) into its slab row
__device__ __forceinline__ void inner_block_sum(double re, double im, double *__restrict__ slab) {
  __shared__ double wpart[4][2];
  const uint32_t tid = threadIdx.x;
  re = wave_sum(re);
  im = wave_sum(im);
  if ((tid & 63u) == 0) {
    wpart[tid >> 6][0] = re;
    wpart[tid >> 6][1] = im;
  }
  __syncthreads();
  if (tid < 2) slab[(uint64_t)blockIdx.x * 2 + tid] = ((wpart[0][tid] + wpart[1][tid]) + wpart[2][tid]) + wpart[3][tid];
}

// One 16-byte item of a linear stream: a complex128 amplitude, or two consecutive complex64 ones.
template <typename R> struct InnerItem;
template <> struct InnerItem<double> {
  typedef double vec __attribute__((ext_vector_type(2)));
  static constexpr int kAmpBits = 0;
};
template <> struct InnerItem<float> {
  typedef float vec __attribute__((ext_vector_type(4)));
  static constexpr int kAmpBits = 1;
};
__device__ __forceinline__ void inner_acc_item(const InnerItem<double>::vec &a, const InnerItem<double>::vec &b, double &re, double &im) {
  inner_acc(a.x, a.y, b.x, b.y, re, im);
}
__device__ __forceinline__ void inner_acc_item(const InnerItem<float>::vec &a, const InnerItem<float>::vec &b, double &re, double &im) {
  inner_acc((double)a.x, (double)a.y, (double)b.x, (double)b.y, re, im);
  inner_acc((double)a.z, (double)a.w, (double)b.z, (double)b.w, re, im);
}

// chunks of 2^cw ITEMS (cw <= 8 + log2 kInnerLoads), cpb chunks per block; thread t takes positions t + 256 u
template <typename R>
__global__ __launch_bounds__(256) void k_inner_linear(const typename AmpT<R>::type *__restrict__ pa,
                                                       const typename AmpT<R>::type *__restrict__ pb, int cw, uint32_t cpb,
                                                       double *__restrict__ slab) {
  using V = typename InnerItem<R>::vec;
  const V *__restrict__ qa = (const V *)pa, *__restrict__ qb = (const V *)pb;
  const uint32_t tid = threadIdx.x, ch = 1u << cw;
  double re = 0.0, im = 0.0;
  const uint64_t q0 = (uint64_t)blockIdx.x * cpb;
  for (uint64_t q = q0; q < q0 + cpb; ++q) {
    const uint64_t base = q << cw;
    V va[kInnerLoads], vb[kInnerLoads];
#pragma unroll
    for (int u = 0; u < kInnerLoads; ++u) {
      va[u] = (V)0;
      vb[u] = (V)0;
      const uint32_t pos = tid + 256u * u;
      if (pos < ch) {
        va[u] = __builtin_nontemporal_load(qa + (base | pos));
        vb[u] = __builtin_nontemporal_load(qb + (base | pos));
      }
    }
#pragma unroll
    for (int u = 0; u < kInnerLoads; ++u) inner_acc_item(va[u], vb[u], re, im);
  }
  inner_block_sum(re, im, slab);
}

template <typename R>
__global__ __launch_bounds__(256) void k_inner_tiles(const typename AmpT<R>::type *__restrict__ pa,
                                                      const typename AmpT<R>::type *__restrict__ pb, InnerTileArgs t,
                                                      double *__restrict__ slab) {
  using A = typename AmpT<R>::type;
  __shared__ A xb[kInnerU][256];
  __shared__ uint64_t low_a[1 << kInnerChunkBits], low_b[1 << kInnerChunkBits];
  const uint32_t tid = threadIdx.x, ntc = 1u << t.cbits;
  // this thread inside any tile: its offset in a's and in b's enumeration, and the slot that holds its partner
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
  const uint32_t put = tid ^ (tid >> 4), get = slot ^ (slot >> 4);      // the swizzle: a permutation inside every row of 16 slots
  // the low cbits of a tile number, spread to a's and to b's positions
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
  double re = 0.0, im = 0.0;
  const uint64_t q0 = (uint64_t)blockIdx.x * t.cpb;
  for (uint64_t q = q0; q < q0 + t.cpb; ++q) {
    uint64_t ha = 0, hb = 0;      // the chunk number, spread likewise (uniform over the block)
    for (int k = t.cbits; k < t.nrest; ++k) {
      const uint64_t bit = (q >> (k - t.cbits)) & 1ull;
      ha |= bit << t.rest_a[k];
      hb |= bit << t.rest_b[k];
    }
    for (uint32_t j0 = 0; j0 < ntc; j0 += kInnerU) {
      A va[kInnerU], vb[kInnerU];
#pragma unroll
      for (int u = 0; u < kInnerU; ++u) {
        va[u].x = 0; va[u].y = 0;
        vb[u].x = 0; vb[u].y = 0;
        if (j0 + u < ntc) {
          va[u] = ld_amp<true>(pa + (ha | low_a[j0 + u] | da));
          vb[u] = ld_amp<true>(pb + (hb | low_b[j0 + u] | db));
        }
      }
#pragma unroll
      for (int u = 0; u < kInnerU; ++u) xb[u][put] = vb[u];
      __syncthreads();
#pragma unroll
      for (int u = 0; u < kInnerU; ++u) {
        const A p = xb[u][get];
        inner_acc((double)va[u].x, (double)va[u].y, (double)p.x, (double)p.y, re, im);
      }
      __syncthreads();
    }
  }
  inner_block_sum(re, im, slab);
}

// nloc < 8: one block, thread i holds a_i and fetches b's partner
template <typename R>
__global__ __launch_bounds__(256) void k_inner_gather(const typename AmpT<R>::type *__restrict__ pa,
                                                       const typename AmpT<R>::type *__restrict__ pb, InnerGatherArgs g,
                                                       double *__restrict__ slab) {
  const uint32_t i = threadIdx.x;
  double re = 0.0, im = 0.0;
  if (i < (1u << g.nloc)) {
    uint32_t j = 0;
    for (int p = 0; p < g.nloc; ++p) j |= ((i >> p) & 1u) << g.pos_b[p];
    const auto a = pa[i], b = pb[j];
    inner_acc((double)a.x, (double)a.y, (double)b.x, (double)b.y, re, im);
  }
  inner_block_sum(re, im, slab);
}

}  // namespace qh
