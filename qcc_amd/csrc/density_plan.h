// density_plan.h -- host side of qh_reduced_density (kernels_density.hip.h): the register's physical positions -> how the
// state is walked.
//
// Plain C++, no HIP: the engine calls it before every launch, qh_density_plan hands the result to tools and tests, and
// tools/density_plan_check.cc runs it stand-alone (with sanitizers) and walks every plan amplitude by amplitude.
//
// rho = A A^H with A of shape 2^k x 2^(nloc - k): row bits are the register's positions, column bits the others (the
// environment).  Ascending by physical position, the lowest tile_bits = min(k, 6) register positions number the rows of a
// tile; the remaining (highest) ones number the blocks of 64 rows that k = 7, 8 are cut into, so that a tile together with
// the lowest environment positions -- a chunk's columns -- is made of whole runs of consecutive amplitudes: every position
// below the lowest one that a chunk of a tile does NOT hold belongs to it, and that lowest missing position is at least
// min(6, chunk_bits).  The other environment positions number the chunks; a workgroup takes consecutive chunk numbers.
//
// A tile and a chunk hold 2^kDensityLdsBits amplitudes at most (32 KiB of complex128 in LDS: complex64 is widened on the
// way in); with row blocks a workgroup keeps two tiles, of half as many columns each.  The grid is bounded twice: by
// kDensityMaxWgs workgroups (8 per CU) and by kDensitySlabBytes of slab, since every workgroup leaves a partial tile of
// 4^tile_bits complex128.
#pragma once
#include <stdint.h>
#include <string.h>

#include "../../include/qcc_hip.h"

namespace qh {

constexpr int kDensityTileBits = 6;                   // a tile has at most 64 rows
constexpr int kDensityLdsBits = 11;                   // amplitudes of (tiles x chunk) a workgroup keeps in LDS
constexpr int kDensityGatherBelow = 8;                // fewer local bits: QH_DENSITY_GATHER
constexpr uint32_t kDensityMaxWgs = 2048;
constexpr uint64_t kDensitySlabBytes = 32ull << 20;

#if defined(__HIPCC__)
#define QH_DENSITY_HD __host__ __device__
#else
#define QH_DENSITY_HD
#endif

// block pair p of nb row blocks -> (R, C) with C >= R, in the order R = 0: C = 0..nb-1, R = 1: C = 1..nb-1, ...  (The one
// function here that the kernels call too.)
QH_DENSITY_HD inline void density_pair(uint32_t nb, uint32_t p, uint32_t *R, uint32_t *C) {
  uint32_t r = 0;
  while (p >= nb - r) {
    p -= nb - r;
    ++r;
  }
  *R = r;
  *C = r + p;
}

// pos[t]: the physical (local) position of bits[t], t < k; all different and below nloc; 0 <= k <= min(8, nloc)
inline void plan_density(int nloc, int k, const int *pos, qh_density_tiles *out) {
  memset(out, 0, sizeof *out);
  out->k = (uint32_t)k;
  uint64_t reg = 0;
  for (int t = 0; t < k; ++t) reg |= 1ull << pos[t];
  int nr = 0, ne = 0;
  uint8_t env[64];
  for (int p = 0; p < nloc; ++p) {
    if ((reg >> p) & 1ull) {
      for (int t = 0; t < k; ++t)
        if (pos[t] == p) out->row_bit[nr] = (uint8_t)t;
      out->row_pos[nr++] = (uint8_t)p;
    } else {
      env[ne++] = (uint8_t)p;
    }
  }
  const int kt = k < kDensityTileBits ? k : kDensityTileBits;
  out->tile_bits = (uint32_t)kt;
  out->amps_swept = 1ull << (nloc + k - kt);
  if (nloc < kDensityGatherBelow) {      // one workgroup, one column at a time, the whole matrix as its one tile
    out->path = QH_DENSITY_GATHER;
    out->tile_bits = (uint32_t)k;
    out->nrest = (uint32_t)ne;
    memcpy(out->rest_pos, env, (size_t)ne);
    out->block_pairs = 1;
    out->wg_per_pair = 1;
    out->chunks_per_wg = 1ull << ne;
    out->amps_swept = 1ull << nloc;
    return;
  }
  out->path = QH_DENSITY_TILES;
  const uint32_t nb = 1u << (k - kt);
  out->block_pairs = nb * (nb + 1) / 2;
  int cb = kDensityLdsBits - kt - (nb > 1 ? 1 : 0);
  if (cb > ne) cb = ne;
  out->chunk_bits = (uint32_t)cb;
  out->nrest = (uint32_t)(ne - cb);
  memcpy(out->col_pos, env, (size_t)cb);
  memcpy(out->rest_pos, env + cb, (size_t)(ne - cb));
  const uint64_t row_bytes = 16ull << (2 * kt), nchunks = 1ull << (ne - cb);
  uint64_t cap = kDensitySlabBytes / row_bytes;
  if (cap > kDensityMaxWgs) cap = kDensityMaxWgs;
  cap /= out->block_pairs;
  uint64_t wg = 1;
  while (wg * 2 <= cap && wg * 2 <= nchunks) wg *= 2;
  out->wg_per_pair = (uint32_t)wg;
  out->chunks_per_wg = nchunks / wg;
  out->slab_bytes = row_bytes * wg * out->block_pairs;
}

}  // namespace qh
