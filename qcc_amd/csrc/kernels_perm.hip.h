// kernels_perm.hip.h -- register permutations (qh_apply_perm): amplitudes moved by a table, |s> -> |table[s]> on the k bits of
// a register, under controls.  No arithmetic touches an amplitude: both kernels copy 8- or 16-byte values as stored.
//
// The host (perm_plan.h) picks the tile -- the register's positions, the positions inside a 128-byte line, padded to 2^10
// amplitudes -- and the path.
//
// k_perm_lds, in place.  A block owns one tile at a time and grid-strides over the tiles whose out-of-tile controls are met
// (the others are never touched: the host numbers only those).  A thread holds its share of a whole tile in registers (at
// most kPermItems items of 16 bytes: one complex128, two complex64).  Per tile:
//   1. the items, loaded from their lines in memory -- in-tile index bit r is the r-th lowest position of the tile,
//      positions 0-2 / 0-3 are always in it, so a wave reads whole lines -- are written to LDS, item v to slot v: LINEAR
//      ds_write_b128, conflict-free;
//   2. barrier;
//   3. the loads of the block's NEXT tile are issued into the same registers: a block always has a tile of reads in flight
//      (without this the kernel took 1.5 x the time: loads and stores alternated instead of overlapping);
//   4. item v is read back from the slot of the amplitude that moves there, src(r) = r with the register field replaced
//      by inverse[field] (r itself where an in-tile control is 0), and stored to the place in memory it was loaded from;
//   5. barrier, before the next tile overwrites LDS.
// Why the random side is the LDS READ: on gfx950 every ds_write banks over 32 dwords and a ds_write_b128 already costs 13
// cycles per wave when it is conflict-free, while ds_read_b128 / ds_read_b64 bank over 64 dwords at 256 B/clk, so a
// scattered read loses a fraction of a fast instruction and a scattered write would multiply a slow one.  It costs the host
// the inverse table, which it builds anyway while it checks that the table is a bijection.
// The table (2^k entries of 16 bits: the source's register field spread over in-tile index bits) is staged in LDS behind
// the tile once per block: 128 KiB of tile + at most 32 KiB of table is the 160 KiB a workgroup may have, and a 64-KiB tile
// with its table leaves room for a second block on the CU.  An entry is fetched by ds_read_u16 with a fixed latency,
// independent of what the non-temporal state stream does to L1.
// Index arithmetic: an item number is (u * threads) | thread, two disjoint bit fields, and both the spread of an in-tile
// index over memory (pdep) and the gather of its register field are ORs of per-bit terms: both parts are computed once per
// kernel, u's part block-uniform (scalar); the cost per amplitude is one OR, and per tile one pdep of the tile number.
// The loop bound is block-uniform: every thread reaches both barriers of every tile.
//
// k_perm_gather, out of place, for tiles that do not fit: dst[i] = src[i with register := inverse[s(i)]], linear 16-byte
// non-temporal writes, gathered reads through the caches, s(i) by tab_gather over the register's runs, entries of 64 bits
// (the field spread over physical positions) through L2.  Read amplification: a gathered read fetches a whole 128-byte
// line for the 8 or 16 bytes it wants unless neighbours in the register-free positions 0-2 (0-3) come with it -- with b
// register bits inside the line only 2^(line bits - b) amplitudes of a fetched line are used by the lanes that fetched it;
// the rest is served from L2 if the line is still there when its other fibres are written.  The engine copies dst back.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels_gate.hip.h"
#include "kernels_mux.hip.h"

namespace qh {

typedef double perm_item __attribute__((ext_vector_type(2)));      // 16 bytes: one complex128 or two complex64
constexpr int kPermItems = 8;                                      // items of a tile per thread, at most

struct PermArgs {
  TabGather g;          // in-tile index -> register field, compressed (perm_plan.h)
  uint64_t tile_mask;   // positions of the in-tile index bits
  uint64_t rest_mask;   // positions of the tile-number bits (out-of-tile controls left out)
  uint64_t ctl_out;     // out-of-tile controls: ones of every tile base
  uint64_t ntiles;      // tiles to run
  uint32_t m;           // in-tile index bits
  uint32_t nent;        // table entries
  uint32_t reg_tile;    // in-tile index bits of the register
  uint32_t ctl_tile;    // in-tile index bits of the controls inside the tile
};

// bit b of v to the b-th lowest set position of mask
__device__ __forceinline__ uint64_t perm_pdep(uint64_t v, uint64_t mask) {
  uint64_t o = 0;
  while (mask && v) {
    const uint64_t low = mask & (~mask + 1ull);
    if (v & 1ull) o |= low;
    v >>= 1;
    mask ^= low;
  }
  return o;
}

extern __shared__ __attribute__((aligned(16))) char perm_smem[];

template <typename R>
__global__ __launch_bounds__(1024) void k_perm_lds(typename AmpT<R>::type *__restrict__ psi, const uint16_t *__restrict__ tab,
                                                    PermArgs a) {
  using A = typename AmpT<R>::type;
  constexpr uint32_t E = 16 / sizeof(A);          // amplitudes per item
  constexpr int U = kPermItems;                   // a thread holds its share of a whole tile in registers
  perm_item *sm = (perm_item *)perm_smem;
  const A *sma = (const A *)perm_smem;
  const uint32_t nitems = (1u << a.m) / E;        // (the host sends no tile smaller than one item, none larger than U * threads)
  uint16_t *stab = (uint16_t *)(perm_smem + (size_t)nitems * 16);
  const uint32_t nt = blockDim.x, tid = threadIdx.x;      // nt: a power of two
  for (uint32_t i = tid; i < a.nent; i += nt) stab[i] = tab[i];      // (visible after the first barrier)
  const uint64_t off_tid = perm_pdep((uint64_t)tid * E, a.tile_mask);
  const uint32_t s_tid = tab_gather((uint64_t)tid * E, a.g);
  const uint32_t s_odd = E == 2 ? tab_gather(1ull, a.g) : 0u;
  // item u * nt + tid of every tile: where it lies in memory, the register field of its in-tile index, whether it exists
  uint64_t off[U];
  uint32_t s_u[U];
  bool on[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const uint32_t r0 = (uint32_t)u * nt * E;                                        // block-uniform
    on[u] = (uint32_t)u * nt + tid < nitems;
    off[u] = perm_pdep(r0, a.tile_mask);
    s_u[u] = tab_gather(r0, a.g);
  }
  perm_item x[U];
  auto load = [&](const A *base) {
#pragma unroll
    for (int u = 0; u < U; ++u)
      if (on[u]) x[u] = __builtin_nontemporal_load((const perm_item *)(base + (off[u] | off_tid)));
  };
  uint64_t t = blockIdx.x;
  A *base = psi + (perm_pdep(t, a.rest_mask) | a.ctl_out);
  if (t < a.ntiles) load(base);
  for (; t < a.ntiles; t += gridDim.x) {          // block-uniform bounds: every thread reaches both barriers of every tile
#pragma unroll
    for (int u = 0; u < U; ++u)
      if (on[u]) sm[(uint32_t)u * nt + tid] = x[u];
    __syncthreads();
    // the next tile's loads go out before this tile's stores: the block always has a tile of reads in flight
    const uint64_t tn = t + gridDim.x;
    A *next = psi + (perm_pdep(tn, a.rest_mask) | a.ctl_out);
    if (tn < a.ntiles) load(next);
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (on[u]) {
        const uint32_t r0 = ((uint32_t)u * nt + tid) * E;
        A o[E];
#pragma unroll
        for (uint32_t e = 0; e < E; ++e) {
          const uint32_t r = r0 | e;
          const uint32_t s = s_u[u] | s_tid | (e ? s_odd : 0u);
          const uint32_t src = (r & a.ctl_tile) == a.ctl_tile ? ((r & ~a.reg_tile) | stab[s]) : r;
          o[e] = sma[src];
        }
        perm_item v;
        __builtin_memcpy(&v, o, 16);
        __builtin_nontemporal_store(v, (perm_item *)(base + (off[u] | off_tid)));
      }
    }
    __syncthreads();                              // before the next tile overwrites LDS
    base = next;
  }
}

struct PermGatherArgs {
  TabGather g;          // physical index -> register field, compressed
  uint64_t nitems;      // 16-byte items of the state
  uint64_t reg_mask;    // positions of the register
  uint64_t ctl;         // positions of the local controls
};

template <typename R>
__global__ __launch_bounds__(256) void k_perm_gather(const typename AmpT<R>::type *__restrict__ src,
                                                      typename AmpT<R>::type *__restrict__ dst,
                                                      const uint64_t *__restrict__ tab, PermGatherArgs a) {
  using A = typename AmpT<R>::type;
  constexpr uint32_t E = 16 / sizeof(A);
  for (uint64_t item = (uint64_t)blockIdx.x * 256 + threadIdx.x; item < a.nitems; item += (uint64_t)gridDim.x * 256) {
    A o[E];
#pragma unroll
    for (uint32_t e = 0; e < E; ++e) {
      const uint64_t i = item * E + e;
      uint64_t j = i;
      if ((i & a.ctl) == a.ctl) j = (i & ~a.reg_mask) | tab[tab_gather(i, a.g)];
      o[e] = src[j];
    }
    perm_item v;
    __builtin_memcpy(&v, o, 16);
    __builtin_nontemporal_store(v, (perm_item *)dst + item);
  }
}

}  // namespace qh
