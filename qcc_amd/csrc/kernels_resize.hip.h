// kernels_resize.hip.h -- a state of another size in a fresh buffer: qh_extend (src (x) f) and qh_release (the slice of src
// at given values of k local bits).  resize_plan.h holds the host arithmetic; both kernels stream.
//
// Both read src front to back in 16-byte ITEMS (one complex128 amplitude, two consecutive complex64 ones), non-temporal,
// kResizeLoads items in flight per thread: thread t of a block takes items t + 256 u of a chunk of 256 * kResizeLoads, and
// the blocks of a launch stride over the chunks.
//   * k_extend: new[(j << nloc) | p] = f[j] * src[p].  A block keeps its chunk in registers and writes it into every slab j
//     of its share of the 2^k slabs: src is read once, every slab is written with 16-byte stores, consecutive lanes at
//     consecutive addresses.  The grid's y dimension splits the slabs.  Where all of src is smaller than a chunk the spare
//     positions of the chunk take further slabs (position w holds item w mod 2^cw for slab w >> cw), so a 2-qubit state
//     extended by 16 qubits still runs full waves; the repeated reads of such a src are cache hits.  One complex product
//     per amplitude, in the handle's width, from the table in the handle's width; entries 0 and 1 reproduce the stored
//     value as a number.
//   * k_release: keep = (p & R) == V, destination = the source index squeezed run by run (ReleaseArgs), one store per kept
//     item, |a|^2 added to the thread's kept or dropped sum.  With position 0 surviving, the two amplitudes of a complex64
//     item share their fate and land in one item (a 16-byte store); with position 0 released exactly one of them can be
//     kept, and it goes out as one 8-byte store (SPLIT).  Amplitudes are copied as stored.  Sums are in double, in a fixed
//     order, no atomics: thread (chunks in order, u in order) -> wave -> the four waves in order -> one (kept, dropped) row
//     per block (block_row_sum, kernels_common.hip.h) -> k_slab_fold adds the rows in block order.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels_common.hip.h"
#include "kernels_gate.hip.h"
#include "resize_plan.h"

namespace qh {

constexpr int kResizeLoads = 4;                          // 16-byte loads in flight per thread
constexpr int kResizeChunkBits = 8 + 2;                  // log2(256 * kResizeLoads) items per chunk
constexpr uint32_t kResizeBlocks = 2048;                 // blocks at most along x: eight per CU
static_assert(256 * kResizeLoads == 1 << kResizeChunkBits, "a chunk is what one block loads in one trip");

struct ExtendArgs {
  int ib;                      // log2(items of src)
  int cw;                      // log2(items per chunk): min(kResizeChunkBits, ib)
  uint32_t nj;                 // 2^k slabs
  uint32_t jper;               // slabs per block row (blockIdx.y), a multiple of the slabs one trip covers
  uint64_t nchunks;            // 2^(ib - cw)
};

__device__ __forceinline__ Item16<double>::vec resize_mul(const double2 &f, const Item16<double>::vec &v) {
  Item16<double>::vec o;
  o.x = f.x * v.x - f.y * v.y;
  o.y = f.x * v.y + f.y * v.x;
  return o;
}
__device__ __forceinline__ Item16<float>::vec resize_mul(const float2 &f, const Item16<float>::vec &v) {
  Item16<float>::vec o;
  o.x = f.x * v.x - f.y * v.y;
  o.y = f.x * v.y + f.y * v.x;
  o.z = f.x * v.z - f.y * v.w;
  o.w = f.x * v.w + f.y * v.z;
  return o;
}

template <typename R>
__global__ __launch_bounds__(256) void k_extend(const typename AmpT<R>::type *__restrict__ src, typename AmpT<R>::type *__restrict__ dst,
                                                 const typename AmpT<R>::type *__restrict__ tab, ExtendArgs a) {
  using V = typename Item16<R>::vec;
  const V *__restrict__ qs = (const V *)src;
  V *__restrict__ qd = (V *)dst;
  const uint32_t tid = threadIdx.x, pmask = (1u << a.cw) - 1u, jstep = 1u << (kResizeChunkBits - a.cw);
  const uint32_t j0 = blockIdx.y * a.jper, j1 = min(j0 + a.jper, a.nj);
  for (uint64_t q = blockIdx.x; q < a.nchunks; q += gridDim.x) {
    V v[kResizeLoads];
    uint64_t p[kResizeLoads];
#pragma unroll
    for (int u = 0; u < kResizeLoads; ++u) {
      p[u] = (q << a.cw) | ((tid + 256u * u) & pmask);
      v[u] = __builtin_nontemporal_load(qs + p[u]);
    }
    for (uint32_t jj = j0; jj < j1; jj += jstep) {
#pragma unroll
      for (int u = 0; u < kResizeLoads; ++u) {
        const uint32_t j = jj + ((tid + 256u * u) >> a.cw);
        if (j < j1) __builtin_nontemporal_store(resize_mul(tab[j], v[u]), qd + (((uint64_t)j << a.ib) | p[u]));
      }
    }
  }
}

struct ReleaseArgs {
  uint64_t drop, want;         // R and V over amplitude indices of src
  uint64_t mask[kResizeMaxSegs];
  uint32_t shift[kResizeMaxSegs];      // (whole words: scalar loads have no byte form)
  int nseg;
  int cw;                      // log2(items per chunk): min(kResizeChunkBits, log2 items)
  uint64_t nchunks;
};

// (unrolled: every run is read at a constant offset of the kernel arguments, into scalar registers, once)
__device__ __forceinline__ uint64_t release_dest(const ReleaseArgs &a, uint64_t p) {
  uint64_t d = 0;
#pragma unroll
  for (int s = 0; s < kResizeMaxSegs; ++s) {
    if (s >= a.nseg) break;
    d |= (p & a.mask[s]) >> a.shift[s];
  }
  return d;
}

// one item: where it goes, and its weight to the side it ends on
template <bool SPLIT>
__device__ __forceinline__ void release_item(const ReleaseArgs &a, uint64_t item, const Item16<double>::vec &v, double2 *__restrict__ dst,
                                             double &kept, double &dropped) {
  const bool keep = (item & a.drop) == a.want;
  const double w = prob_sum(v.x, v.y);
  if (keep) __builtin_nontemporal_store(v, (Item16<double>::vec *)dst + release_dest(a, item));
  kept += keep ? w : 0.0;
  dropped += keep ? 0.0 : w;
}
template <bool SPLIT>
__device__ __forceinline__ void release_item(const ReleaseArgs &a, uint64_t item, const Item16<float>::vec &v, float2 *__restrict__ dst,
                                             double &kept, double &dropped) {
  const uint64_t p = item << 1;
  const double w0 = prob_sum(v.x, v.y), w1 = prob_sum(v.z, v.w);
  if constexpr (SPLIT) {      // position 0 is released: the halves of the item part ways
    const bool k0 = (p & a.drop) == a.want, k1 = ((p | 1ull) & a.drop) == a.want;
    typedef float half_item __attribute__((ext_vector_type(2)));
    if (k0 | k1) {
      half_item h;
      h.x = k0 ? v.x : v.z;
      h.y = k0 ? v.y : v.w;
      __builtin_nontemporal_store(h, (half_item *)dst + release_dest(a, p));      // (position 0 is in no run: p and p | 1 squeeze alike)
    }
    kept += k0 ? w0 : 0.0;
    kept += k1 ? w1 : 0.0;
    dropped += k0 ? 0.0 : w0;
    dropped += k1 ? 0.0 : w1;
  } else {                    // position 0 survives, at position 0: both halves share the predicate and one destination item
    const bool keep = (p & a.drop) == a.want;
    if (keep) __builtin_nontemporal_store(v, (Item16<float>::vec *)dst + (release_dest(a, p) >> 1));
    kept += keep ? w0 : 0.0;
    kept += keep ? w1 : 0.0;
    dropped += keep ? 0.0 : w0;
    dropped += keep ? 0.0 : w1;
  }
}

template <typename R, bool SPLIT>
__global__ __launch_bounds__(256) void k_release(const typename AmpT<R>::type *__restrict__ src, typename AmpT<R>::type *__restrict__ dst,
                                                  ReleaseArgs a, double *__restrict__ slab) {
  using V = typename Item16<R>::vec;
  const V *__restrict__ qs = (const V *)src;
  const uint32_t tid = threadIdx.x, ch = 1u << a.cw;
  double kept = 0.0, dropped = 0.0;
  for (uint64_t q = blockIdx.x; q < a.nchunks; q += gridDim.x) {
    const uint64_t base = q << a.cw;
    V v[kResizeLoads];
#pragma unroll
    for (int u = 0; u < kResizeLoads; ++u) {
      v[u] = (V)0;
      const uint32_t pos = tid + 256u * u;
      if (pos < ch) v[u] = __builtin_nontemporal_load(qs + (base | pos));
    }
#pragma unroll
    for (int u = 0; u < kResizeLoads; ++u) {
      const uint32_t pos = tid + 256u * u;
      if (pos < ch) release_item<SPLIT>(a, base | pos, v[u], dst, kept, dropped);
    }
  }
  const double row[2] = {kept, dropped};
  block_row_sum(row, slab);
}

}  // namespace qh
