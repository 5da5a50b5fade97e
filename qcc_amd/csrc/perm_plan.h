// perm_plan.h -- host side of qh_apply_perm (kernels_perm.hip.h): bit map, register and controls -> the tile a block
// permutes in LDS, the path, and the table in the form the kernels read.
//
// Plain C++, no HIP: the engine calls it before every launch, qh_perm_plan hands the tile to tools and tests, and
// tools/perm_plan_check.cc runs it stand-alone (with sanitizers) against a brute-force model.
//
// A permutation of a register moves amplitudes only inside a FIBRE: the 2^k amplitudes that agree on every bit outside the
// register.  A TILE is a set of physical positions that holds the register, so a tile is a union of whole fibres and can be
// permuted on its own:
//   tile = register positions  u  the positions inside a 128-byte line (0-2 at complex128, 0-3 at complex64)
//          padded with the lowest positions left to min(kPermPadBits, nloc) bits.
// The line positions make every memory access of a tile a whole line (16 bytes per lane, coalesced); the padding gives small
// registers full blocks and long runs.  In-tile index bit r stands for the r-th lowest position of the tile; the positions
// left number the tiles.  A local control inside the tile is a predicate per amplitude, one outside it fixes a bit of the tile
// number: the tiles where it is 0 are neither read nor written.
// The path follows from the tile alone: QH_PERM_LDS when 2^tile_bits amplitudes fit kPermLdsBytes, QH_PERM_GATHER otherwise.
//
// The table.  The kernels compute where an amplitude COMES FROM (linear writes, gathered reads), so they want the inverse.
// They index it by the register field as it lies in memory: bit c of a compressed value is the register bit on the c-th
// lowest position (one shift and one mask per run of adjacent positions, whatever order the caller listed the bits in), and
// an entry is the source's register field already spread over the positions it is ORed into.
#pragma once
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../include/qcc_hip.h"

namespace qh {

constexpr int kPermPadBits = 10;                 // a tile has at least 2^10 amplitudes (or is the whole state)
constexpr size_t kPermLdsBytes = 128u << 10;     // amplitudes of one tile in LDS; the table sits behind them
constexpr int kPermMaxRuns = 16;

// 2^k entries, each below 2^k, none twice.  Returns -1, or the first offending entry s; *other = -1 (table[s] out of
// range) or the earlier entry with the same value.
inline int64_t perm_check_table(int k, const uint32_t *table, int64_t *other) {
  const uint32_t n = 1u << k;
  std::vector<int32_t> hit(n, -1);
  for (uint32_t s = 0; s < n; ++s) {
    if (table[s] >= n) {
      *other = -1;
      return s;
    }
    if (hit[table[s]] >= 0) {
      *other = hit[table[s]];
      return s;
    }
    hit[table[s]] = (int32_t)s;
  }
  return -1;
}

// reg_pos[j]: physical position (local: < nloc) of register bit j.  ctl_local: physical positions of the local controls.
// Fills path, tile, register and control fields of *out (ctl_met is the caller's).
inline void plan_perm_tiles(int nloc, int bit_width, int k, const int *reg_pos, uint64_t ctl_local, qh_perm_tiles *out) {
  memset(out, 0, sizeof *out);
  const int line = std::min(bit_width == 128 ? 3 : 4, nloc);
  uint64_t reg = 0;
  for (int j = 0; j < k; ++j) reg |= 1ull << reg_pos[j];
  uint64_t tile = reg | ((1ull << line) - 1ull);
  const int want = std::min(kPermPadBits, nloc);
  for (int p = 0; __builtin_popcountll(tile) < want; ++p) tile |= 1ull << p;      // (lowest positions left)
  const int m = __builtin_popcountll(tile);
  out->tile_bits = (uint32_t)m;
  out->tile_mask = tile;
  out->reg_mask = reg;
  out->ctl_in = ctl_local & tile;
  out->ctl_out = ctl_local & ~tile;
  out->lds_bytes = (uint64_t)(bit_width / 8) << m;
  out->path = out->lds_bytes <= kPermLdsBytes ? QH_PERM_LDS : QH_PERM_GATHER;
  out->ntiles = 1ull << (nloc - m);
  out->tiles_skipped = out->ntiles - (out->ntiles >> __builtin_popcountll(out->ctl_out));
  for (int j = 0; j < k; ++j) {
    out->reg_pos[j] = (uint8_t)reg_pos[j];
    out->reg_rank[j] = (uint8_t)__builtin_popcountll(tile & ((1ull << reg_pos[j]) - 1ull));
  }
}

// order[c] = the register bit j on the c-th lowest position
inline void perm_order(int k, const uint8_t *reg_pos, int *order) {
  for (int c = 0; c < k; ++c) order[c] = c;
  std::sort(order, order + k, [&](int a, int b) { return reg_pos[a] < reg_pos[b]; });
}

// a register value as the caller numbers it -> compressed (bit c = register bit order[c])
inline uint32_t perm_compress(uint32_t s, int k, const int *order) {
  uint32_t c = 0;
  for (int b = 0; b < k; ++b) c |= ((s >> order[b]) & 1u) << b;
  return c;
}

// The inverse table in compressed numbering: inv[compress(table[s])] = compress(s).  `table` must have passed
// perm_check_table.
inline std::vector<uint32_t> perm_inverse(int k, const uint32_t *table, const int *order) {
  const uint32_t n = 1u << k;
  std::vector<uint32_t> comp(n), inv(n);
  for (uint32_t s = 0; s < n; ++s) comp[s] = perm_compress(s, k, order);
  for (uint32_t s = 0; s < n; ++s) inv[comp[table[s]]] = comp[s];
  return inv;
}

// a compressed value spread over sorted[0..k) (ascending bit positions: physical ones, or ranks inside the tile)
inline uint64_t perm_deposit(uint32_t c, int k, const uint8_t *sorted) {
  uint64_t o = 0;
  for (int b = 0; b < k; ++b) o |= (uint64_t)((c >> b) & 1u) << sorted[b];
  return o;
}

// The compressed value of an index as runs: compressed bits [dst, dst + len) = index bits [src, src + len), packed
// src | dst << 8 | len << 16 (the TabGather of kernels_mux.hip.h).  sorted ascending; returns the number of runs (<= k).
inline int perm_runs(int k, const uint8_t *sorted, uint32_t *run) {
  int n = 0;
  for (int c = 0; c < k;) {
    int e = c + 1;
    while (e < k && sorted[e] == sorted[c] + (e - c)) ++e;
    run[n++] = (uint32_t)sorted[c] | ((uint32_t)c << 8) | ((uint32_t)(e - c) << 16);
    c = e;
  }
  return n;
}

}  // namespace qh
