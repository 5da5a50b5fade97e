// kernels_select.hip.h -- sparse readout on the device: a short list of (logical index, amplitude) entries instead of a
// reduction.  qh_select (everything at or above a threshold), qh_topk (the k most probable) and qh_amplitudes (the entries
// at given indices).
//
// A probability is prob_fma (kernels_common.hip.h: as qh_argmax and the sweep islands compute it); its bit pattern, the
// KEY, orders like the probability because it is never negative (the remark k_tmax_reduce relies on).  Every selection is
// a range of keys.
//
//   * k_select: a stream compaction, one read of the state.  Chunks as k_chunk_sums: 2^c amplitudes per chunk, 256
//     threads, 16-byte non-temporal loads (one complex128 or two complex64 amplitudes), all of a thread's in flight at
//     once.  A wave ranks its hits with one ballot per load slot and mbcnt, and its first lane makes ONE returning 64-bit
//     atomicAdd of the wave's hits per chunk on the device counter; the hits are written at base + rank.  Writes at or past `cap` are suppressed while the count keeps running,
//     and a wave that has seen the counter at or past `cap` stops asking: the counter only grows, so none of its later
//     hits could be written.  It counts them in a register and adds them once when it leaves (the dense case -- every
//     amplitude a hit, count only -- starts there and makes one atomic per wave, not one per chunk).  The physical -> logical map is
//     applied to hits only, through the LDS byte tables of kernels_common.hip.h.  The order of the entries depends on
//     the order in which waves reach the counter: the host sorts.  The weight (sum of the hits' probabilities) is summed
//     per thread over its chunks in order, then over the block in the fixed order of block_sum_256, one partial per block:
//     no float atomics, the same bits for the same state, layout and grid.
//   * k_key_hist: one read; counts the nonzero keys under a prefix into 2^bits bins of the next key bits (select_plan.h), per
//     block in LDS with integer atomics, then into the global bins with one 64-bit integer atomic per nonempty bin and
//     block.  A wave whose valid lanes all fall into one bin -- every wave of a flat state -- makes one add of its
//     popcount instead of 64 adds that serialise on one LDS address.
//   * k_tie_scan: the entries of a range of LOGICAL indices (of this shard, in ascending order) whose key equals one value,
//     gathered through the logical -> physical map; appended like k_select's.
//   * k_gather_amps: out[j] = the amplitude at global logical index idx[j], (0, 0) where another shard holds it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels_common.hip.h"
#include "kernels_gate.hip.h"
#include "kernels_measure.hip.h"

namespace qh {

struct SelEntry {            // == qh_entry (include/qcc_hip.h)
  uint64_t index;
  double re, im;
};

__device__ __forceinline__ uint64_t sel_key(double p) { return (uint64_t)__double_as_longlong(p); }

// One 16-byte non-temporal load per thread and slot at either width: one complex128 amplitude, or two consecutive complex64
// ones (8-byte loads left a complex64 read at 0.6 of qh_norm2's rate).  Slot j of a thread's kMeasPer amplitudes of a chunk
// sits at chunk position sel_pos(j): PACK = amplitudes per load.
typedef float sel_v4f __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void sel_load16(const double2 *p, double2 *v) { v[0] = ld_amp<true>(p); }
__device__ __forceinline__ void sel_load16(const float2 *p, float2 *v) {
  const sel_v4f t = __builtin_nontemporal_load((const sel_v4f *)p);
  v[0].x = t.x;
  v[0].y = t.y;
  v[1].x = t.z;
  v[1].y = t.w;
}
template <int PACK> __device__ __forceinline__ uint32_t sel_pos(int j) {
  return (threadIdx.x + 256u * (uint32_t)(j / PACK)) * PACK + (uint32_t)(j % PACK);
}
template <typename A> __device__ __forceinline__ void sel_load_chunk(const A *base, uint32_t ch, A *v) {
  constexpr int PACK = sizeof(double2) / sizeof(A);
#pragma unroll
  for (int u = 0; u < kMeasPer / PACK; ++u)
    if (sel_pos<PACK>(u * PACK) < ch) sel_load16(base + sel_pos<PACK>(u * PACK), v + u * PACK);
}

__device__ __forceinline__ uint32_t lane_rank(uint64_t ballot) {      // set bits below this lane
  return __builtin_amdgcn_mbcnt_hi((uint32_t)(ballot >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)ballot, 0u));
}

// Hits: klo <= key <= khi.  counter: the running number of hits (u64, zeroed by the host).  out: cap entries (may be
// null with cap == 0).  wpart: one weight partial per block.
template <typename R>
__global__ __launch_bounds__(256) void k_select(const typename AmpT<R>::type *__restrict__ psi, int c, uint64_t nchunks, uint64_t klo,
                                                 uint64_t khi, IndexMap mm, unsigned long long *__restrict__ counter,
                                                 SelEntry *__restrict__ out, uint64_t cap, double *__restrict__ wpart) {
  using A = typename AmpT<R>::type;
  constexpr int PACK = sizeof(double2) / sizeof(A);
  __shared__ uint64_t lut[kIndexLutWords];
  __shared__ double wsum[4];
  const uint32_t tid = threadIdx.x, ch = 1u << c, lane = tid & 63;
  build_index_lut(lut, mm);
  __syncthreads();
  double weight = 0.0;
  unsigned long long late = 0;      // this wave's hits after it has seen the counter at or past cap (the same in every lane)
  bool full = cap == 0;
  for (uint64_t q = blockIdx.x; q < nchunks; q += gridDim.x) {
    const A *base = psi + (q << c);
    A v[kMeasPer];
    sel_load_chunk(base, ch, v);
    uint32_t hitmask = 0, total = 0, before[kMeasPer];
#pragma unroll
    for (int u = 0; u < kMeasPer; ++u) {
      bool hit = false;
      if (sel_pos<PACK>(u) < ch) {
        const double p = prob_fma(v[u]);
        const uint64_t key = sel_key(p);
        hit = key >= klo && key <= khi;
        if (hit) weight += p;
      }
      const uint64_t b = __ballot(hit);
      before[u] = total + lane_rank(b);
      total += (uint32_t)__popcll(b);
      hitmask |= (hit ? 1u : 0u) << u;
    }
    if (total == 0) continue;       // (wave-uniform)
    if (full) {
      late += total;
      continue;
    }
    unsigned long long at = 0;
    if (lane == 0) at = atomicAdd(counter, (unsigned long long)total);
    at = __shfl(at, 0, 64);
    if (at >= cap) {
      full = true;
      continue;
    }
#pragma unroll
    for (int u = 0; u < kMeasPer; ++u) {
      if (!((hitmask >> u) & 1u)) continue;
      const uint64_t pos = at + before[u];
      if (pos >= cap) continue;
      const uint64_t idx = (q << c) | (uint64_t)sel_pos<PACK>(u);
      SelEntry e;
      e.index = index_lut_logical(lut, idx) | mm.shard_logical;
      e.re = (double)v[u].x;
      e.im = (double)v[u].y;
      out[pos] = e;
    }
  }
  if (late && lane == 0) atomicAdd(counter, late);
  wave_partial(weight, wsum);
  __syncthreads();
  if (tid == 0) wpart[blockIdx.x] = four_waves(wsum);
}

// ghist[b] += the number of keys k != 0 with (k >> (shift + bits)) == prefix and ((k >> shift) & (2^bits - 1)) == b
template <typename R>
__global__ __launch_bounds__(256) void k_key_hist(const typename AmpT<R>::type *__restrict__ psi, int c, uint64_t nchunks, uint64_t prefix,
                                                   int shift, int bits, unsigned long long *__restrict__ ghist) {
  using A = typename AmpT<R>::type;
  constexpr int PACK = sizeof(double2) / sizeof(A);
  __shared__ uint32_t hist[1 << 12];
  const uint32_t tid = threadIdx.x, ch = 1u << c, lane = tid & 63, nb = 1u << bits;
  for (uint32_t b = tid; b < nb; b += 256) hist[b] = 0;
  __syncthreads();
  for (uint64_t q = blockIdx.x; q < nchunks; q += gridDim.x) {
    const A *base = psi + (q << c);
    A v[kMeasPer];
    sel_load_chunk(base, ch, v);
#pragma unroll
    for (int u = 0; u < kMeasPer; ++u) {
      bool valid = false;
      uint32_t bin = 0;
      if (sel_pos<PACK>(u) < ch) {
        const uint64_t key = sel_key(prob_fma(v[u]));
        valid = key != 0 && ((key >> shift) >> bits) == prefix;
        bin = (uint32_t)(key >> shift) & (nb - 1u);
      }
      const uint64_t vb = __ballot(valid);
      if (vb == 0) continue;
      const int first = __builtin_ctzll(vb);
      const uint32_t fbin = (uint32_t)__shfl((int)bin, first, 64);
      const uint64_t same = __ballot(valid && bin == fbin);
      if (same == vb) {
        if ((int)lane == first) atomicAdd(&hist[fbin], (uint32_t)__popcll(vb));
      } else if (valid) {
        atomicAdd(&hist[bin], 1u);
      }
    }
  }
  __syncthreads();
  for (uint32_t b = tid; b < nb; b += 256)
    if (hist[b]) atomicAdd(&ghist[b], (unsigned long long)hist[b]);
}

// The shard's amplitudes in ascending LOGICAL order: bit j of a rank r stands for the j-th local logical bit, which is
// physical position phys[j] and global logical bit log[j].
struct TieMap {
  int n;
  uint8_t phys[40], log[40];
  uint64_t shard_logical;
};

template <typename A>
__global__ __launch_bounds__(256) void k_tie_scan(const A *__restrict__ psi, uint64_t r0, uint64_t r1, uint64_t want, TieMap tm,
                                                   unsigned long long *__restrict__ counter, SelEntry *__restrict__ out, uint64_t cap) {
  for (uint64_t r = r0 + (uint64_t)blockIdx.x * 256 + threadIdx.x; r < r1; r += (uint64_t)gridDim.x * 256) {
    uint64_t p = 0, l = tm.shard_logical;
    for (int j = 0; j < tm.n; ++j) {
      const uint64_t bit = (r >> j) & 1ull;
      p |= bit << tm.phys[j];
      l |= bit << tm.log[j];
    }
    const A a = ld_amp<false>(psi + p);
    if (sel_key(prob_fma(a)) != want) continue;
    const unsigned long long at = atomicAdd(counter, 1ull);
    if (at < cap) {
      SelEntry e;
      e.index = l;
      e.re = (double)a.x;
      e.im = (double)a.y;
      out[at] = e;
    }
  }
}

// l2p[b]: physical (local) position of logical bit b, 0xff where the shard index holds it; held: those logical bits,
// held_ones: their values on this shard
struct GatherMap {
  int nglob;
  uint8_t l2p[64];
  uint64_t held, held_ones;
};

template <typename A>
__global__ __launch_bounds__(256) void k_gather_amps(const A *__restrict__ psi, const uint64_t *__restrict__ idx, uint64_t count, GatherMap gm,
                                                      double2 *__restrict__ out) {
  for (uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x; j < count; j += (uint64_t)gridDim.x * 256) {
    const uint64_t l = idx[j];
    double2 o;
    o.x = 0.0;
    o.y = 0.0;
    if ((l & gm.held) == gm.held_ones) {
      uint64_t p = 0;
      for (int b = 0; b < gm.nglob; ++b)
        if (gm.l2p[b] != 0xff) p |= ((l >> b) & 1ull) << gm.l2p[b];
      const A a = ld_amp<false>(psi + p);
      o.x = (double)a.x;
      o.y = (double)a.y;
    }
    out[j] = o;
  }
}

}  // namespace qh
