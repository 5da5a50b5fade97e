// kernels_rank1.hip.h -- rank-one register updates (qh_apply_rank1): psi'[s, r] = a psi[s, r] + b u[s] m_r with
// m_r = sum_s conj(v[s]) psi[s, r] on every fibre r of a k-bit register whose controls are met.  One inner product and one
// axpy over 2^k amplitudes per fibre: memory-bound, never a matrix.  The host (rank1_plan.h) picks the tile and the path and
// uploads conj(v) and b * u as complex doubles, indexed by the register field as it lies in memory (compressed order).
// All arithmetic is in double from the amplitudes as stored; a new component is rounded once to the state's width.
//
// k_rank1_tile, in place, the shape of k_perm_lds.  A block owns one tile at a time and grid-strides over the tiles whose
// out-of-tile controls are met.  A thread holds its share of the tile in registers (at most kPermItems items of 16 bytes,
// read as whole lines) and keeps it there until the tile is stored.  Per tile:
//   1. products conj(v_s) psi, formed in registers.  Item u * threads + tid: the bits of u are the TOP bits of the in-tile
//      index, so the register bits among them are summed inside the thread first, in ascending u (a tile above 2^10 amplitudes is register and
//      line bits only: every bit of u is then a register bit, and a complex64 tile of 2^14 amplitudes needs 2^13 slots of
//      complex double, the 128 KiB the tile itself would take);
//   2. the surviving products go to LDS, slot = the in-tile index with the summed bits of u squeezed out: linear
//      ds_write_b128, conflict-free (the write is the slow side, kernels_perm.hip.h);
//   3. the whole block sums the remaining register bits pairwise, one level per bit in ascending position, a barrier per
//      level: level j touches slots / 2^(j+1) pairs, so the tree moves about three times the products once, against two
//      passes of the tile through HBM.  (One thread per fibre would not do: a 10-bit register leaves 8 fibres of 1024 terms.)
//      The fibre's sum m_r ends in the slot whose register bits are 0;
//   4. a psi + (b u_s) m_r from the registers, m_r one LDS read (a broadcast inside a fibre), stored where the item came
//      from; an in-tile control is a predicate per amplitude, and an amplitude that fails it keeps its bits.  As soon as an
//      item is stored, the same item of the block's NEXT tile is loaded into its registers: the loads of the next tile are in
//      flight while this one is stored (a second register set would not fit 128 VGPRs at 1024 threads);
//   5. barrier, before the next tile's products overwrite LDS.
// The tables (2 x 2^k complex doubles) are staged in LDS behind the products once per block: the table form takes this path
// for k <= 10 only (rank1_plan.h), 32 KiB at most, and 128 + 32 KiB is the 160 KiB a workgroup may have.  The uniform form has
// no table: conj(v) and b u are two scalars.
//
// Two passes, for tiles that do not fit (k >= 11, and the uniform form up to the whole state):
//   k_rank1_dot   pass 1.  The state is read as linear 16-byte non-temporal streams, a chunk of 2048 items per block and
//                 step, as k_expect_batch reads it.  A thread's 8 items keep their chunk-local place from chunk to chunk, so
//                 the products of the chunks of one fibre group (the register bits above the chunk, ascending) are added up
//                 in registers; the register bits inside the chunk are then summed by the tree of step 3.  A block writes
//                 fibres_per_chunk sums: into m, or, where the walk is split over several blocks, into its segment's partial
//                 sums, which k_rank1_fold adds in segment order.  k = nbits_local is one group of one fibre: 256 segments,
//                 a full-width reduction like k_norm2.  conj(v) (2^11 to 2^16 entries) is read through L2.
//   k_rank1_axpy  pass 2: the shape of k_diag_tab, a chunk per block and step, with one extra load of m_r per amplitude
//                 (fibre index = the physical index with the register bits taken out: like the table index an OR of a
//                 chunk part, scalar, a per-item part and a per-thread part).
// sums: |psi'|^2 as stored and |m_r|^2 (counted at the fibre's amplitude with register field 0) per thread, then wave_sum, the
// waves in order, one slab row per block, k_slab_fold: the readers' fixed order.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "kernels_common.hip.h"
#include "kernels_gate.hip.h"
#include "kernels_mux.hip.h"
#include "kernels_perm.hip.h"

namespace qh {

constexpr int kRank1Items = 8;      // items of a pass-1 / pass-2 chunk per thread (256 threads: rank1_plan.h kRank1ChunkItems)

// complex double in a perm_item
__device__ __forceinline__ perm_item r1_mul(perm_item x, perm_item y) {
  perm_item o;
  o.x = x.x * y.x - x.y * y.y;
  o.y = x.x * y.y + x.y * y.x;
  return o;
}

// amplitude e of a 16-byte item, widened unrounded
template <typename R> __device__ __forceinline__ perm_item r1_get(const perm_item &it, uint32_t e) {
  if constexpr (std::is_same<R, double>::value) {
    return it;
  } else {
    float f[4];
    __builtin_memcpy(f, &it, 16);
    perm_item o;
    o.x = (double)f[2 * e];
    o.y = (double)f[2 * e + 1];
    return o;
  }
}
// ... and rounded once into it; returns |stored|^2
template <typename R> __device__ __forceinline__ double r1_put(perm_item &it, uint32_t e, perm_item v) {
  if constexpr (std::is_same<R, double>::value) {
    it = v;
    return prob_sum(v.x, v.y);
  } else {
    float f[4];
    __builtin_memcpy(f, &it, 16);
    f[2 * e] = (float)v.x;
    f[2 * e + 1] = (float)v.y;
    __builtin_memcpy(&it, f, 16);
    return prob_sum(f[2 * e], f[2 * e + 1]);
  }
}

// the bits of v on the set positions of mask, packed (the inverse of perm_pdep)
__device__ __forceinline__ uint64_t r1_pext(uint64_t v, uint64_t mask) {
  uint64_t o = 0;
  for (uint32_t b = 0; mask; mask &= mask - 1ull, ++b)
    if (v & mask & (~mask + 1ull)) o |= 1ull << b;
  return o;
}

// Pairwise sums over the set bits of `bits` (ascending) of sm[0, nslots): level by level, sm[i] += sm[i | bit] for the slots
// i that have this bit and the earlier ones 0.  The caller has synchronised behind the writes; bits, nslots are block-uniform.
__device__ __forceinline__ void r1_lds_tree(perm_item *sm, uint32_t nslots, uint32_t bits) {
  uint32_t done = 0, n = nslots;
  for (uint32_t rest = bits; rest; rest &= rest - 1u) {
    const uint32_t bit = rest & (~rest + 1u);
    done |= bit;
    n >>= 1;
    const uint32_t keep = (nslots - 1u) & ~done;
    for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) {
      const uint32_t s = (uint32_t)perm_pdep(i, keep);
      sm[s] += sm[s | bit];
    }
    __syncthreads();
  }
}

extern __shared__ __attribute__((aligned(16))) char rank1_smem[];

struct Rank1TileArgs {
  TabGather g;          // in-tile index -> register field, compressed (perm_plan.h)
  uint64_t tile_mask;   // positions of the in-tile index bits
  uint64_t rest_mask;   // positions of the tile-number bits (out-of-tile controls left out)
  uint64_t ctl_out;     // out-of-tile controls: ones of every tile base
  uint64_t ntiles;      // tiles to run
  uint32_t m;           // in-tile index bits
  uint32_t nent;        // table entries (uniform form: 0)
  uint32_t reg_tile;    // in-tile index bits of the register
  uint32_t ctl_tile;    // in-tile index bits of the controls inside the tile
  uint32_t nslots;      // product slots in LDS: 2^m / 2^(register bits among the bits of u)
  uint32_t pad;
  double ar, ai;        // a
  double vr, ubr, ubi;  // uniform form: conj(v_s) = vr, b u_s = (ubr, ubi)
};

// TAB: 0 the uniform form, 1 tables staged in LDS
// U: items per thread the registers are sized for, 4 or kPermItems (tiles of 128 KiB: every bit of u is a register bit)
template <typename R, int TAB, int U>
__global__ __launch_bounds__(1024) void k_rank1_tile(typename AmpT<R>::type *__restrict__ psi, const perm_item *__restrict__ tab,
                                                      Rank1TileArgs a, double *__restrict__ slab) {
  using A = typename AmpT<R>::type;
  constexpr uint32_t E = 16 / sizeof(A);          // amplitudes per item
  perm_item *sm = (perm_item *)rank1_smem;
  constexpr bool UNI = TAB == 0;
  const perm_item *svc = sm + a.nslots, *sub = svc + a.nent;      // conj(v), b u behind the products
  const uint32_t nt = blockDim.x, tid = threadIdx.x;              // nt: a power of two
  const uint32_t nitems = (1u << a.m) / E;        // (the host sends no tile smaller than one item, none larger than U * threads)
  if constexpr (TAB == 1) {
    perm_item *stab = sm + a.nslots;
    for (uint32_t i = tid; i < 2 * a.nent; i += nt) stab[i] = tab[i];
    __syncthreads();
  }
  const uint32_t lbits = (uint32_t)__builtin_ctz(nt * E);         // in-tile index bits below the bits of u
  // bits of u that are register bits.  Eight items: a tile of 128 KiB is register and line bits only, so all three are (the
  // host checks): one sum per thread, one slot, and the compiler drops the other combinations
  const uint32_t ureg = U == kPermItems ? (uint32_t)(U - 1) : (a.reg_tile >> lbits) & (uint32_t)(U - 1);
  const uint32_t reg_low = a.reg_tile & ((1u << lbits) - 1u);
  const uint64_t off_tid = perm_pdep((uint64_t)tid * E, a.tile_mask);
  const uint32_t s_tid = tab_gather((uint64_t)tid * E, a.g);
  const uint32_t s_odd = E == 2 ? tab_gather(1ull, a.g) : 0u;
  // item u * nt + tid of every tile: where it lies in memory, the register field of its in-tile index, whether it exists,
  // whether its products survive the sums inside the thread, and the slot of its first product
  uint64_t off[U];
  uint32_t s_u[U], slot_u[U];
  bool on[U], live[U];
  const uint32_t ueff = nitems > nt ? nitems / nt : 1u;          // items per thread
  const bool active = tid < nitems;                               // (a tile smaller than the block)
  const uint32_t slot_tid = tid * E;
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const uint32_t r0 = (uint32_t)u * nt * E;                                        // block-uniform
    on[u] = (uint32_t)u < ueff && active;
    live[u] = ((uint32_t)u & ureg) == 0;
    off[u] = perm_pdep(r0, a.tile_mask);
    s_u[u] = tab_gather(r0, a.g);
    slot_u[u] = (uint32_t)r1_pext((uint32_t)u, (uint32_t)(U - 1) & ~ureg) * nt * E;      // block-uniform
  }
  perm_item x[U];
  auto load = [&](const A *base) {
#pragma unroll
    for (int u = 0; u < U; ++u)
      if (on[u]) x[u] = __builtin_nontemporal_load((const perm_item *)(base + (off[u] | off_tid)));
  };
  double acc0 = 0.0, acc1 = 0.0;
  uint64_t t = blockIdx.x;
  A *base = psi + (perm_pdep(t, a.rest_mask) | a.ctl_out);
  if (t < a.ntiles) load(base);
  for (; t < a.ntiles; t += gridDim.x) {          // block-uniform bounds: every thread reaches every barrier of every tile
#pragma unroll
    for (int u0 = 0; u0 < U; ++u0) {              // a surviving item: the items that differ from it in register bits of u, ascending
      if (on[u0] && live[u0]) {
        perm_item p[E];
#pragma unroll
        for (uint32_t e = 0; e < E; ++e) {
          p[e].x = 0.0;
          p[e].y = 0.0;
        }
#pragma unroll
        for (int u = u0; u < U; ++u) {
          if (((uint32_t)u & ~ureg) == (uint32_t)u0) {      // (block-uniform)
#pragma unroll
            for (uint32_t e = 0; e < E; ++e) {
              const perm_item w = r1_get<R>(x[u], e);
              if constexpr (UNI) p[e] += w * a.vr;
              else p[e] += r1_mul((svc + s_u[u])[s_tid | (e ? s_odd : 0u)], w);      // (a block-uniform base and one lane offset)
            }
          }
        }
#pragma unroll
        for (uint32_t e = 0; e < E; ++e) sm[(slot_u[u0] | slot_tid) + e] = p[e];
      }
    }
    __syncthreads();
    r1_lds_tree(sm, a.nslots, reg_low);
    // an item of the next tile is loaded into the registers of this tile's item as soon as that one is stored
    const uint64_t tn = t + gridDim.x;
    A *next = psi + (perm_pdep(tn, a.rest_mask) | a.ctl_out);
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (on[u]) {
        const uint32_t r0 = ((uint32_t)u * nt + tid) * E;
        perm_item o = x[u];
        bool any = false;
#pragma unroll
        for (uint32_t e = 0; e < E; ++e) {
          const uint32_t r = r0 | e;
          if ((r & a.ctl_tile) == a.ctl_tile) {
            const uint32_t s_lane = s_tid | (e ? s_odd : 0u);
            const perm_item mr = (sm + slot_u[u])[(slot_tid + e) & ~reg_low];      // (the bits of slot_u lie above reg_low)
            const perm_item w = r1_get<R>(x[u], e);
            perm_item bu;
            if constexpr (UNI) {
              bu.x = a.ubr;
              bu.y = a.ubi;
            } else {
              bu = (sub + s_u[u])[s_lane];
            }
            perm_item av;
            av.x = a.ar;
            av.y = a.ai;
            acc0 += r1_put<R>(o, e, r1_mul(av, w) + r1_mul(bu, mr));
            if ((s_u[u] | s_lane) == 0) acc1 += prob_sum(mr.x, mr.y);
            any = true;
          }
        }
        if (any) __builtin_nontemporal_store(o, (perm_item *)(base + (off[u] | off_tid)));
        if (tn < a.ntiles) x[u] = __builtin_nontemporal_load((const perm_item *)(next + (off[u] | off_tid)));
      }
    }
    __syncthreads();                              // before the next tile's products overwrite LDS
    base = next;
  }
  if (slab) {                                     // (the last barrier of the loop is behind every read of the products)
    double *wp = (double *)rank1_smem;
    const double w0 = wave_sum(acc0), w1 = wave_sum(acc1);
    if ((tid & 63u) == 0) {
      wp[(tid >> 6) * 2] = w0;
      wp[(tid >> 6) * 2 + 1] = w1;
    }
    __syncthreads();
    if (tid < 2) {
      double s = 0.0;
      for (uint32_t w = 0; w < (nt + 63u) / 64u; ++w) s += wp[w * 2 + tid];      // the waves in order
      slab[(uint64_t)blockIdx.x * 2 + tid] = s;
    }
  }
}

struct Rank1DotArgs {
  TabGather g;          // chunk-local amplitude index -> the low bits of the compressed register field
  uint64_t grp_mask;    // bits of the chunk number that number the fibre groups
  uint64_t abv_mask;    // bits of the chunk number that are register bits
  uint64_t nunits;      // groups * split: (group, segment) pairs, a block each
  uint64_t walk;        // chunks per segment
  uint64_t nfib;        // fibres of the shard
  uint32_t split;       // segments per group (a power of two)
  uint32_t nin;         // register bits inside a chunk
  uint32_t reg_low;     // ... as chunk-local index bits
  uint32_t fpc;         // fibres per chunk
  uint32_t cb;          // amplitude-index bits of a chunk: 256 * kRank1Items items, or the whole of a smaller shard
  uint32_t pad;
  double vr;            // uniform form: conj(v_s)
};

// out[seg * nfib + f], f = group * fpc + (chunk-local index with the register bits taken out)
template <typename R, bool UNI>
__global__ __launch_bounds__(256) void k_rank1_dot(const typename AmpT<R>::type *__restrict__ psi, const perm_item *__restrict__ vc,
                                                    Rank1DotArgs a, perm_item *__restrict__ out) {
  using A = typename AmpT<R>::type;
  constexpr uint32_t E = 16 / sizeof(A);
  constexpr int U = kRank1Items;
  const uint32_t nslots = 1u << a.cb;             // amplitudes of a chunk
  const uint32_t ci = nslots / E, ui = ci / 256u; // its items, and items per thread (the host sends no chunk below 256 items)
  perm_item *sm = (perm_item *)rank1_smem;
  const perm_item *items = (const perm_item *)psi;
  const uint32_t tid = threadIdx.x;
  const uint32_t s_tid = UNI ? 0u : tab_gather((uint64_t)tid * E, a.g);
  const uint32_t s_odd = (!UNI && E == 2) ? tab_gather(1ull, a.g) : 0u;
  uint32_t s_u[U];
#pragma unroll
  for (int u = 0; u < U; ++u) s_u[u] = UNI ? 0u : tab_gather((uint64_t)u * 256u * E, a.g);      // block-uniform
  for (uint64_t unit = blockIdx.x; unit < a.nunits; unit += gridDim.x) {      // block-uniform bounds
    const uint64_t grp = unit / a.split, seg = unit % a.split;
    const uint64_t cbase = perm_pdep(grp, a.grp_mask);
    perm_item acc[U][E];
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (uint32_t e = 0; e < E; ++e) {
        acc[u][e].x = 0.0;
        acc[u][e].y = 0.0;
      }
    perm_item x[U], xn[U];
    auto load = [&](perm_item (&d)[U], uint64_t wi) {
      const perm_item *p = items + (cbase | perm_pdep(wi, a.abv_mask)) * (uint64_t)ci + tid;
#pragma unroll
      for (int u = 0; u < U; ++u)
        if ((uint32_t)u < ui) d[u] = __builtin_nontemporal_load(p + 256 * u);
    };
    const uint64_t w0 = seg * a.walk, w1 = w0 + a.walk;
    load(x, w0);
    for (uint64_t wi = w0; wi < w1; ++wi) {       // the chunks of this segment, ascending register field
      if (wi + 1 < w1) load(xn, wi + 1);
      const uint32_t s_hi = (uint32_t)(wi << a.nin);
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if ((uint32_t)u >= ui) continue;
#pragma unroll
        for (uint32_t e = 0; e < E; ++e) {
          const perm_item w = r1_get<R>(x[u], e);
          if constexpr (UNI) acc[u][e] += w;
          else acc[u][e] += r1_mul(vc[s_hi | s_u[u] | s_tid | (e ? s_odd : 0u)], w);
        }
      }
#pragma unroll
      for (int u = 0; u < U; ++u) x[u] = xn[u];
    }
#pragma unroll
    for (int u = 0; u < U; ++u)
      if ((uint32_t)u < ui) {
#pragma unroll
        for (uint32_t e = 0; e < E; ++e) sm[((uint32_t)u * 256u + tid) * E + e] = acc[u][e];
      }
    __syncthreads();
    r1_lds_tree(sm, nslots, a.reg_low);
    perm_item *o = out + seg * a.nfib + grp * a.fpc;
    for (uint32_t i = tid; i < a.fpc; i += 256u) {
      perm_item v = sm[(uint32_t)perm_pdep(i, (nslots - 1u) & ~a.reg_low)];
      if constexpr (UNI) v *= a.vr;
      o[i] = v;
    }
    __syncthreads();                              // before the next unit's sums overwrite LDS
  }
}

// m[f] = the partial sums of fibre f, in segment order
__global__ __launch_bounds__(256) void k_rank1_fold(const perm_item *__restrict__ part, perm_item *__restrict__ m, uint64_t nfib,
                                                     uint32_t split) {
  for (uint64_t f = (uint64_t)blockIdx.x * 256 + threadIdx.x; f < nfib; f += (uint64_t)gridDim.x * 256) {
    perm_item s = part[f];
    for (uint32_t g = 1; g < split; ++g) s += part[(uint64_t)g * nfib + f];
    m[f] = s;
  }
}

struct Rank1AxpyArgs {
  TabGather g;          // physical index -> register field, compressed
  uint64_t free_mask;   // the local positions outside the register
  uint64_t reg_mask;    // ... and of the register
  uint64_t ctl;         // positions of the local controls
  uint64_t nchunks;     // chunks of 2^cb amplitudes
  uint32_t cb;          // as in Rank1DotArgs
  uint32_t pad;
  double ar, ai;        // a
  double ubr, ubi;      // uniform form: b u_s
};

template <typename R, bool UNI>
__global__ __launch_bounds__(256) void k_rank1_axpy(typename AmpT<R>::type *__restrict__ psi, const perm_item *__restrict__ ub,
                                                     const perm_item *__restrict__ m, Rank1AxpyArgs a, double *__restrict__ slab) {
  using A = typename AmpT<R>::type;
  constexpr uint32_t E = 16 / sizeof(A);
  constexpr int U = kRank1Items;
  perm_item *items = (perm_item *)psi;
  const uint32_t tid = threadIdx.x;
  const uint32_t ci = (1u << a.cb) / E, ui = ci / 256u;
  const uint64_t f_tid = r1_pext((uint64_t)tid * E, a.free_mask), f_odd = E == 2 ? r1_pext(1ull, a.free_mask) : 0ull;
  const uint32_t s_tid = UNI ? 0u : tab_gather((uint64_t)tid * E, a.g), s_odd = (!UNI && E == 2) ? tab_gather(1ull, a.g) : 0u;
  uint64_t f_u[U];
  uint32_t s_u[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {                   // block-uniform
    f_u[u] = r1_pext((uint64_t)u * 256u * E, a.free_mask);
    s_u[u] = UNI ? 0u : tab_gather((uint64_t)u * 256u * E, a.g);
  }
  perm_item av;
  av.x = a.ar;
  av.y = a.ai;
  double acc[2] = {0.0, 0.0};
  for (uint64_t c = blockIdx.x; c < a.nchunks; c += gridDim.x) {
    const uint64_t ibase = c << a.cb;                              // first amplitude of the chunk: block-uniform
    const uint64_t f_c = r1_pext(ibase, a.free_mask);
    const uint32_t s_c = UNI ? 0u : tab_gather(ibase, a.g);
    perm_item *p = items + c * (uint64_t)ci + tid;
    perm_item x[U];
#pragma unroll
    for (int u = 0; u < U; ++u)
      if ((uint32_t)u < ui) x[u] = __builtin_nontemporal_load(p + 256 * u);
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if ((uint32_t)u >= ui) continue;
      perm_item o = x[u];
      bool any = false;
#pragma unroll
      for (uint32_t e = 0; e < E; ++e) {
        const uint64_t i = ibase | (((uint64_t)u * 256u + tid) * E + e);
        if ((i & a.ctl) == a.ctl) {
          const uint32_t s = s_c | s_u[u] | s_tid | (e ? s_odd : 0u);
          const perm_item mr = m[f_c | f_u[u] | f_tid | (e ? f_odd : 0ull)];
          perm_item bu;
          if constexpr (UNI) {
            bu.x = a.ubr;
            bu.y = a.ubi;
          } else {
            bu = ub[s];
          }
          acc[0] += r1_put<R>(o, e, r1_mul(av, r1_get<R>(x[u], e)) + r1_mul(bu, mr));
          if ((i & a.reg_mask) == 0) acc[1] += prob_sum(mr.x, mr.y);
          any = true;
        }
      }
      if (any) __builtin_nontemporal_store(o, p + 256 * u);
    }
  }
  if (slab) block_row_sum<2>(acc, slab);
}

}  // namespace qh
