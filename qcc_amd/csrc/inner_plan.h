// inner_plan.h -- host side of qh_inner (kernels_inner.hip.h): two bit maps -> how the two states are walked together.
//
// Plain C++, no HIP: the engine calls it before every launch, qh_inner_plan hands the result to tools and tests, and
// tools/inner_plan_check.cc runs it stand-alone (with sanitizers) over many permutations.
//
// pi maps a local position of `a` to the position where `b` keeps the same logical bit.  pi == identity: both states are
// read front to back.  Otherwise (8 local bits or more) the index space is cut into tiles of 2^8 amplitudes whose free
// bits are, in a's positions, F = {0..3} u pi^-1({0..3}) padded to 8 bits with the lowest positions left; in b's positions
// pi(F), which contains {0..3}.  Both sets hold bits 0..3, so a tile is 16 runs of 16 consecutive amplitudes in EITHER
// state.  The remaining nloc - 8 positions, ascending in a, number the tiles: bit k of a tile number goes to rest_a[k] in a
// and rest_b[k] = pi(rest_a[k]) in b.  Inside a tile, in-tile index bit k stands for a's position tile_a[k] (ascending) and,
// in b's enumeration, for b's position tile_b[k] (ascending); the amplitude a holds at in-tile index r pairs with the one b
// holds at in-tile index sum_k bit_k(r) << shuffle[k].
#pragma once
#include <stdint.h>
#include <string.h>

#include "../../include/qcc_hip.h"

namespace qh {

constexpr int kInnerTileBits = 8;

// perm_a / perm_b: physical position of each of the nglob logical bits.  Returns -1 and fills *out, or the first logical
// bit that one handle keeps in the shard index (position >= nloc) and the other elsewhere.
inline int plan_inner(int nloc, int nglob, const int *perm_a, const int *perm_b, qh_inner_tiles *out) {
  memset(out, 0, sizeof *out);
  uint8_t inv[64] = {};      // a's position of the logical bit b keeps at position q
  bool same = true;
  for (int l = 0; l < nglob; ++l) {
    const int pa = perm_a[l], pb = perm_b[l];
    if (pa >= nloc || pb >= nloc) {
      if (pa != pb) return l;
      continue;
    }
    out->pos_b[pa] = (uint8_t)pb;
    inv[pb] = (uint8_t)pa;
    same = same && pa == pb;
  }
  if (same) {
    out->path = QH_INNER_LINEAR;
    return -1;
  }
  if (nloc < kInnerTileBits) {
    out->path = QH_INNER_GATHER;
    return -1;
  }
  out->path = QH_INNER_TILES;
  uint64_t fa = 0xFull;
  for (int q = 0; q < 4; ++q) fa |= 1ull << inv[q];
  for (int p = 0; __builtin_popcountll(fa) < kInnerTileBits; ++p) fa |= 1ull << p;      // (lowest positions left)
  uint64_t fb = 0;
  for (int p = 0; p < nloc; ++p)
    if ((fa >> p) & 1ull) fb |= 1ull << out->pos_b[p];
  out->free_a = fa;
  out->free_b = fb;
  int ka = 0, kb = 0, kr = 0;
  for (int p = 0; p < nloc; ++p) {
    if ((fa >> p) & 1ull) out->tile_a[ka++] = (uint8_t)p;
    else {
      out->rest_a[kr] = (uint8_t)p;
      out->rest_b[kr++] = out->pos_b[p];
    }
    if ((fb >> p) & 1ull) out->tile_b[kb++] = (uint8_t)p;
  }
  out->nrest = (uint32_t)kr;
  for (int k = 0; k < kInnerTileBits; ++k)
    for (int j = 0; j < kInnerTileBits; ++j)
      if (out->tile_b[j] == out->pos_b[out->tile_a[k]]) out->shuffle[k] = (uint8_t)j;
  return -1;
}

}  // namespace qh
