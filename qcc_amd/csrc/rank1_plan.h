// rank1_plan.h -- host side of qh_apply_rank1 (kernels_rank1.hip.h): bit map, register and controls -> the tile, the path,
// the cut of pass 1, scratch, kernel count and bytes, and the tables in the order the kernels index them.
//
// Plain C++, no HIP: the engine launches from plan_rank1, qh_rank1_plan hands the result to tools and tests, and
// tools/rank1_plan_check.cc runs it stand-alone (with sanitizers) against a brute-force model.
//
// psi'[s, r] = a psi[s, r] + b u[s] m_r,  m_r = sum_s conj(v[s]) psi[s, r]  touches one FIBRE r at a time (the 2^k amplitudes
// that agree outside the register), so the tile of perm_plan.h -- register positions, line positions, padding to 2^10 -- is a
// union of whole fibres and can be updated on its own:
//   QH_RANK1_TILE      the tile's amplitudes fit kPermLdsBytes and, in the table form, k <= kPermPadBits (the two tables are
//                      staged in LDS behind the products: 32 KiB at most): k_rank1_tile, in place, the met tiles read and
//                      written once;
//   QH_RANK1_TWO_PASS  otherwise.  Pass 1 (k_rank1_dot) cuts the state into CHUNKS of 2^chunk_bits consecutive amplitudes
//                      (2048 items of 16 bytes).  reg_in_chunk register bits lie below chunk_bits and are summed inside the
//                      block; reg_above lie in the chunk number, and the 2^reg_above chunks that differ only there are one
//                      fibre GROUP, walked in ascending order of their register field.  A group holds fibres_per_chunk
//                      fibres; fibre f = group * fibres_per_chunk + (the chunk-local index with the register bits taken out)
//                      = the physical index with the register bits taken out.  Where groups alone give fewer than
//                      kRank1Blocks blocks, the walk is cut into `split` equal segments, one block each, whose partial sums
//                      k_rank1_fold adds in segment order.  Pass 2 (k_rank1_axpy) streams the state once more.
//                      Scratch: m (nfibres complex doubles) and, when split > 1, split x nfibres partial sums behind it.
//
// Tables.  The kernels index a table by the register field as it lies in memory: bit c of a compressed value is the register
// bit on the c-th lowest position (perm_order / perm_compress of perm_plan.h).  The engine uploads conj(v) and b * u in that
// order, as complex doubles at both widths.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../include/qcc_hip.h"
#include "perm_plan.h"

namespace qh {

constexpr int kRank1ChunkItems = 2048;      // 16-byte items of a pass-1 / pass-2 chunk: 256 threads x 8
constexpr uint64_t kRank1Blocks = 1024;     // pass 1: blocks to aim for when the groups are few
constexpr uint32_t kRank1MaxSplit = 256;    // ... and the most segments a walk is cut into

// The tile of plan_perm_tiles for any k <= nloc: registers wider than QH_PERM_MAX_BITS (the uniform form) never fit LDS and
// have no room in reg_pos / reg_rank, which then stay 0.
inline void plan_rank1_tile(int nloc, int bit_width, int k, const int *reg_pos, uint64_t ctl_local, qh_perm_tiles *out) {
  if (k <= QH_PERM_MAX_BITS) return plan_perm_tiles(nloc, bit_width, k, reg_pos, ctl_local, out);
  memset(out, 0, sizeof *out);
  const int line = std::min(bit_width == 128 ? 3 : 4, nloc);
  uint64_t reg = 0;
  for (int j = 0; j < k; ++j) reg |= 1ull << reg_pos[j];
  const uint64_t tile = reg | ((1ull << line) - 1ull);      // (k > 16: no padding is ever needed)
  const int m = __builtin_popcountll(tile);
  out->tile_bits = (uint32_t)m;
  out->tile_mask = tile;
  out->reg_mask = reg;
  out->ctl_in = ctl_local & tile;
  out->ctl_out = ctl_local & ~tile;
  out->lds_bytes = (uint64_t)(bit_width / 8) << m;
  out->path = QH_PERM_GATHER;
  out->ntiles = 1ull << (nloc - m);
  out->tiles_skipped = out->ntiles - (out->ntiles >> __builtin_popcountll(out->ctl_out));
}

// reg_pos[j]: physical position (< nloc) of register bit j; ctl_local: positions of the local controls.  Fills everything
// but tile.k and tile.ctl_met (the caller's).
inline void plan_rank1(int nloc, int bit_width, int k, const int *reg_pos, uint64_t ctl_local, int uniform, qh_rank1_info *out) {
  memset(out, 0, sizeof *out);
  plan_rank1_tile(nloc, bit_width, k, reg_pos, ctl_local, &out->tile);
  out->uniform = uniform ? 1u : 0u;
  const uint64_t amp = (uint64_t)bit_width / 8, state = amp << nloc;
  out->nfibres = 1ull << (nloc - k);
  if (out->tile.lds_bytes <= kPermLdsBytes && (uniform || k <= kPermPadBits)) {
    out->path = QH_RANK1_TILE;
    out->kernels = 1;
    out->bytes_swept = 2 * (out->tile.ntiles - out->tile.tiles_skipped) * out->tile.lds_bytes;
    return;
  }
  out->path = QH_RANK1_TWO_PASS;
  const int cb = std::min(nloc, bit_width == 128 ? 11 : 12);      // kRank1ChunkItems items
  const uint64_t low = (1ull << cb) - 1ull;
  out->chunk_bits = (uint32_t)cb;
  out->reg_in_chunk = (uint32_t)__builtin_popcountll(out->tile.reg_mask & low);
  out->reg_above = (uint32_t)k - out->reg_in_chunk;
  out->groups = 1ull << (nloc - cb - (int)out->reg_above);
  out->fibres_per_chunk = 1ull << (cb - (int)out->reg_in_chunk);
  uint64_t split = 1;
  while (out->groups * split < kRank1Blocks && split < kRank1MaxSplit && split < (1ull << out->reg_above)) split *= 2;
  out->split = (uint32_t)split;
  out->walk = (1ull << out->reg_above) / split;
  out->scratch_bytes = 16 * out->nfibres * (split > 1 ? 1 + split : 1);
  out->kernels = split > 1 ? 3 : 2;
  out->bytes_swept = 3 * state;      // two reads and one write
}

// The first non-finite number of a[0..n): its index, or -1.
inline int64_t rank1_first_nonfinite(const double *a, uint64_t n) {
  for (uint64_t i = 0; i < n; ++i)
    if (!std::isfinite(a[i])) return (int64_t)i;
  return -1;
}

// conj(v) and b * u in compressed order, interleaved re, im.  u == nullptr: u = v.
inline void rank1_tables(int k, const uint8_t *reg_pos, const double *u, const double *v, const double b[2], std::vector<double> *vc,
                         std::vector<double> *ub) {
  int order[QH_PERM_MAX_BITS];
  perm_order(k, reg_pos, order);
  const uint32_t n = 1u << k;
  vc->resize(2 * (size_t)n);
  ub->resize(2 * (size_t)n);
  if (!u) u = v;
  for (uint32_t s = 0; s < n; ++s) {
    const uint32_t c = perm_compress(s, k, order);
    (*vc)[2 * c] = v[2 * s];
    (*vc)[2 * c + 1] = -v[2 * s + 1];
    (*ub)[2 * c] = b[0] * u[2 * s] - b[1] * u[2 * s + 1];
    (*ub)[2 * c + 1] = b[0] * u[2 * s + 1] + b[1] * u[2 * s];
  }
}

}  // namespace qh
