// kernels_measure.hip.h -- register readout on the device: marginals (qh_marginal), inverse-CDF sampling (qh_sample) and the
// projection on several bits at once (qh_project_bits).
//
// The state is cut into CHUNKS of 2^c physical amplitudes (c = kMeasChunkBits, or the whole shard if it is smaller); 256
// threads read a chunk with 16 coalesced, non-temporal 16-byte loads each (thread t: positions t + 256 u).  Every
// reduction is in double and in a fixed order (no float atomics): the same state in the same layout gives bitwise the
// same sums.  The sampler's two passes sum a chunk in different orders (k_chunk_sums: strided positions and a wave
// reduction; k_chunk_locate: contiguous runs of 16 and a scan), so they agree only to rounding: a target at or above the
// chunk's scanned total goes to its last nonzero amplitude, and a landing on an exact zero moves to the next nonzero one.
//
//   * k_marginal_bins: a block owns cpb chunks that share one value of the OUTER bits (register bits at or above c), and
//     accumulates |a|^2 position by position over them in registers (16 per thread).  Then the 2^c position sums go to
//     LDS and are folded into the 2^ki bins of the INNER bits (register bits below c): each bin by G threads that sum 16
//     members each, then a fixed tree over the G partials.  The bins go to a slab, one row per block.
//     k_marginal_fold sums the rows of one outer value in block order and scatters (outer, inner) to the output index.
//     One read of the state.
//   * k_chunk_sums: one fixed-order sum per chunk (one read).  The host prefixes them and places every shot in a chunk.
//     k_chunk_locate: one block per chunk that has shots re-reads the chunk, scans it (thread-sequential runs of 16 +
//     a wave scan + the four wave totals, all fixed order) and places each shot by binary search.  At most one more read
//     of the state whatever the number of shots: two reads + O(shots) in all.
//   * k_project_mask: zeros where (i & mask) != want; nothing is read.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels_common.hip.h"
#include "kernels_gate.hip.h"

namespace qh {

constexpr int kMeasChunkBits = 12;
constexpr int kMeasPer = (1 << kMeasChunkBits) / 256;    // amplitudes per thread and chunk
constexpr int kMaxMarginalBits = 16;

struct MarginalArgs {
  int c;                     // chunk bits: chunk q is amplitudes [q << c, (q + 1) << c)
  uint32_t inner;            // register bits below c (mask within a chunk)
  int ki;                    // popcount(inner)
  int ko;                    // register bits at or above c
  uint8_t opos[kMaxMarginalBits];   // their positions in the CHUNK index, ascending
  uint64_t cpb;              // chunks per block
  uint32_t bpo;              // blocks per outer value
};

struct FoldArgs {
  int ki, ko;
  uint32_t bpo;
  uint8_t tin[kMeasChunkBits];      // output bit of inner bin bit s
  uint8_t tout[kMaxMarginalBits];   // output bit of outer bit s
  uint64_t fixed;                   // output bits of the register bits the shard index holds
};

__device__ __forceinline__ uint32_t pdep32(uint32_t v, uint32_t mask) {
  uint32_t o = 0;
  for (uint32_t m = mask; m; m &= m - 1) {
    o |= (v & 1u) << __builtin_ctz(m);
    v >>= 1;
  }
  return o;
}

// chunk index of the r-th chunk whose outer bits equal o (bits inserted at opos, ascending: as expand_index)
__device__ __forceinline__ uint64_t outer_chunk(uint64_t r, uint64_t o, const MarginalArgs &a) {
  for (int s = 0; s < a.ko; ++s) {
    const uint64_t low = (1ull << a.opos[s]) - 1ull;
    r = ((r & ~low) << 1) | (r & low) | (((o >> s) & 1ull) << a.opos[s]);
  }
  return r;
}

template <typename R>
__global__ __launch_bounds__(256) void k_marginal_bins(const typename AmpT<R>::type *__restrict__ psi, MarginalArgs a,
                                                        double *__restrict__ slab) {
  using A = typename AmpT<R>::type;
  __shared__ double lds[1 << kMeasChunkBits];
  const uint32_t tid = threadIdx.x, ch = 1u << a.c;
  const uint64_t o = blockIdx.x / a.bpo, r0 = (uint64_t)(blockIdx.x % a.bpo) * a.cpb;
  double acc[kMeasPer];
#pragma unroll
  for (int u = 0; u < kMeasPer; ++u) acc[u] = 0.0;
  for (uint64_t r = r0; r < r0 + a.cpb; ++r) {
    const A *base = psi + (outer_chunk(r, o, a) << a.c);
    A v[kMeasPer];
#pragma unroll
    for (int u = 0; u < kMeasPer; ++u)
      if (tid + 256u * u < ch) v[u] = ld_amp<true>(base + tid + 256u * u);
#pragma unroll
    for (int u = 0; u < kMeasPer; ++u)
      if (tid + 256u * u < ch) acc[u] += prob_sum(v[u].x, v[u].y);
  }
#pragma unroll
  for (int u = 0; u < kMeasPer; ++u)
    if (tid + 256u * u < ch) lds[tid + 256u * u] = acc[u];
  __syncthreads();
  // bin j (inner bits == j) has nm = ch / J members; G threads share a bin, 16 members each (G = 1 from J = 256 on)
  const uint32_t J = 1u << a.ki, nm = ch >> a.ki;
  const uint32_t G = min(max(256u >> a.ki, 1u), nm), per = nm / G, slots = J * G;
  const uint32_t rest = (ch - 1u) & ~a.inner;
  double part[kMeasPer];
#pragma unroll
  for (int m = 0; m < kMeasPer; ++m) {
    const uint32_t w = tid + 256u * m;
    part[m] = 0.0;
    if (w < slots) {
      const uint32_t jb = pdep32(w & (J - 1u), a.inner), g = w >> a.ki;
      for (uint32_t r = g * per; r < (g + 1u) * per; ++r) part[m] += lds[jb | pdep32(r, rest)];
    }
  }
  __syncthreads();
#pragma unroll
  for (int m = 0; m < kMeasPer; ++m)
    if (tid + 256u * m < slots) lds[tid + 256u * m] = part[m];
  __syncthreads();
  for (uint32_t s = G >> 1; s > 0; s >>= 1) {         // partial g += partial g + s, for g < s: a fixed tree per bin
    for (uint32_t w = tid; w < s * J; w += 256) lds[w] += lds[w + s * J];
    __syncthreads();
  }
  for (uint32_t j = tid; j < J; j += 256) slab[(uint64_t)blockIdx.x * J + j] = lds[j];
}

__global__ __launch_bounds__(256) void k_marginal_fold(const double *__restrict__ slab, FoldArgs f, double *__restrict__ out) {
  const uint64_t J = 1ull << f.ki, total = J << f.ko;
  for (uint64_t w = (uint64_t)blockIdx.x * 256 + threadIdx.x; w < total; w += (uint64_t)gridDim.x * 256) {
    const uint64_t j = w & (J - 1), o = w >> f.ki;
    double s = 0.0;
    for (uint32_t p = 0; p < f.bpo; ++p) s += slab[((o * f.bpo + p) << f.ki) + j];
    uint64_t jj = f.fixed;
    for (int b = 0; b < f.ki; ++b) jj |= ((j >> b) & 1ull) << f.tin[b];
    for (int b = 0; b < f.ko; ++b) jj |= ((o >> b) & 1ull) << f.tout[b];
    out[jj] = s;
  }
}

// the block's sum to every thread, in the readers' fixed order (kernels_common.hip.h); wpart may be used again on return
__device__ __forceinline__ double block_sum_256(double v, double *wpart) {
  wave_partial(v, wpart);
  __syncthreads();
  const double s = four_waves(wpart);
  __syncthreads();
  return s;
}

template <typename R>
__global__ __launch_bounds__(256) void k_chunk_sums(const typename AmpT<R>::type *__restrict__ psi, int c, uint64_t nchunks,
                                                     double *__restrict__ sums) {
  using A = typename AmpT<R>::type;
  __shared__ double wpart[4];
  const uint32_t tid = threadIdx.x, ch = 1u << c;
  for (uint64_t q = blockIdx.x; q < nchunks; q += gridDim.x) {
    const A *base = psi + (q << c);
    A v[kMeasPer];
#pragma unroll
    for (int u = 0; u < kMeasPer; ++u)
      if (tid + 256u * u < ch) v[u] = ld_amp<true>(base + tid + 256u * u);
    double acc = 0.0;
#pragma unroll
    for (int u = 0; u < kMeasPer; ++u)
      if (tid + 256u * u < ch) acc += prob_sum(v[u].x, v[u].y);
    acc = block_sum_256(acc, wpart);
    if (tid == 0) sums[q] = acc;
  }
}

// Shot s of the chunk list entry e (chunk ids[e], shots [first[e], first[e + 1])) has target[s] in [0, chunk sum): its
// amplitude is the first one at which the chunk's running sum exceeds the target (clamped to the chunk's last nonzero
// amplitude, and moved to the next nonzero one if rounding lands on a zero).
template <typename R>
__global__ __launch_bounds__(256) void k_chunk_locate(const typename AmpT<R>::type *__restrict__ psi, int c,
                                                       const uint64_t *__restrict__ ids, const uint64_t *__restrict__ first,
                                                       uint64_t nlist, const double *__restrict__ target, IndexMap mm,
                                                       uint64_t *__restrict__ out) {
  using A = typename AmpT<R>::type;
  __shared__ double S[1 << kMeasChunkBits];
  __shared__ uint64_t nzw[(1 << kMeasChunkBits) / 64];
  __shared__ uint64_t lut[kIndexLutWords];      // (read behind the syncs of the scan)
  __shared__ double wtot[4];
  __shared__ int lastnz;
  const uint32_t tid = threadIdx.x, ch = 1u << c;
  build_index_lut(lut, mm);
  const uint32_t per = ch >= 256 ? ch / 256 : 1u;        // positions per thread in the scan (contiguous run)
  const bool active = tid * per < ch;
  const uint32_t nwords = (ch + 63) / 64;
  for (uint64_t e = blockIdx.x; e < nlist; e += gridDim.x) {
    const uint64_t q = ids[e];
    const A *base = psi + (q << c);
    A v[kMeasPer];
#pragma unroll
    for (int u = 0; u < kMeasPer; ++u)
      if (tid + 256u * u < ch) v[u] = ld_amp<true>(base + tid + 256u * u);
    if (tid < nwords) nzw[tid] = 0;
    if (tid == 0) lastnz = -1;
    __syncthreads();
#pragma unroll
    for (int u = 0; u < kMeasPer; ++u)
      if (tid + 256u * u < ch) S[tid + 256u * u] = prob_sum(v[u].x, v[u].y);
    __syncthreads();
    double run = 0.0;
    int nz = -1;
    uint64_t bits = 0;
    if (active) {
      for (uint32_t e2 = 0; e2 < per; ++e2) {
        const uint32_t i = tid * per + e2;
        const double p = S[i];
        if (p > 0.0) { nz = (int)i; bits |= 1ull << (i & 63); }
        run += p;
        S[i] = run;
      }
    }
    if (bits) atomicOr((unsigned long long *)&nzw[(tid * per) >> 6], (unsigned long long)bits);
    if (nz >= 0) atomicMax(&lastnz, nz);
    // exclusive prefix of the threads' runs: inclusive wave scan (fixed shuffles), then the wave totals in order
    const uint32_t lane = tid & 63, wave = tid >> 6;
    double incl = run;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const double y = __shfl_up(incl, d, 64);
      if (lane >= (uint32_t)d) incl += y;
    }
    if (lane == 63) wtot[wave] = incl;
    __syncthreads();
    double off = __shfl_up(incl, 1, 64);
    if (lane == 0) off = 0.0;
    for (uint32_t w = 0; w < wave; ++w) off += wtot[w];
    if (active)
      for (uint32_t e2 = 0; e2 < per; ++e2) S[tid * per + e2] += off;
    __syncthreads();
    const uint64_t s1 = first[e + 1];
    for (uint64_t s = first[e] + tid; s < s1; s += 256) {
      const double x = target[s];
      uint32_t lo = 0, hi = ch;           // first i with S[i] > x, or ch
      while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (S[mid] > x) hi = mid; else lo = mid + 1;
      }
      int i = (int)lo;
      if (i >= (int)ch) {
        i = lastnz;
      } else if (!((nzw[i >> 6] >> (i & 63)) & 1ull)) {      // a zero amplitude: the next nonzero one, else the last
        int j = -1;
        for (uint32_t wd = (uint32_t)i >> 6; wd < nwords && j < 0; ++wd) {
          uint64_t m = nzw[wd];
          if (wd == ((uint32_t)i >> 6)) m &= ~0ull << (i & 63);
          if (m) j = (int)(wd * 64 + __builtin_ctzll(m));
        }
        i = j >= 0 ? j : lastnz;
      }
      if (i < 0) i = 0;                   // (cannot happen: a chunk with shots has a nonzero amplitude)
      const uint64_t idx = (q << c) | (uint64_t)i;
      out[s] = index_lut_logical(lut, idx) | mm.shard_logical;
    }
    __syncthreads();
  }
}

template <typename R>
__global__ __launch_bounds__(256) void k_project_mask(typename AmpT<R>::type *__restrict__ psi, uint64_t n, uint64_t mask,
                                                       uint64_t want) {
  typename AmpT<R>::type z;
  z.x = 0;
  z.y = 0;
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256)
    if ((i & mask) != want) st_amp<true>(psi + i, z);
}

}  // namespace qh
