// density_plan_check.cc -- stand-alone check of qcc_amd/csrc/density_plan.h (the host side of qh_reduced_density), for
// sanitizer builds:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -static-libasan -static-libubsan
//       tools/density_plan_check.cc -o density_plan_check
// (the sanitizer runtimes linked statically: the program then runs as it is, in any environment).
// For every size from 1 to nmax local bits (default 12), every k the size allows and `count` register placements each
// (default 6: the lowest positions, the highest, and random ones, in random list order), it
//   * checks the tables: rows and columns disjoint and ascending, row_bit the inverse of the caller's list, the columns the
//     lowest positions the register does not hold, rows + columns + rest a partition of the local positions;
//   * checks the geometry: 1, 3 or 10 block pairs in density_pair's order, workgroups x chunks x columns = the environment,
//     the slab and the swept amplitudes, the gather path exactly below 8 local bits, runs of a chunk of a tile;
//   * checks that position 0 opens the load order of a chunk of a tile (a complex64 item is the pair that differs there);
//   * walks the state as the kernels do -- pair, workgroup, chunk, in-chunk index spread over the merged row and column
//     positions -- and checks that every amplitude is visited exactly once per block pair that holds its row block, at the
//     (row, column) the positions spell.
// Exit status 0 = all good.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <random>
#include <vector>

#include "../qcc_amd/csrc/density_plan.h"

static int failures = 0;
#define CHECK(cond, ...)                  \
  do {                                    \
    if (!(cond)) {                        \
      ++failures;                         \
      fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); \
      fprintf(stderr, __VA_ARGS__);       \
      fputc('\n', stderr);                \
    }                                     \
  } while (0)

static uint64_t spread(uint64_t v, const uint8_t *pos, int n) {
  uint64_t o = 0;
  for (int b = 0; b < n; ++b) o |= ((v >> b) & 1ull) << pos[b];
  return o;
}

static void check_one(int nloc, int k, const std::vector<int> &pos) {
  qh_density_tiles pl;
  qh::plan_density(nloc, k, pos.data(), &pl);
  const int kt = (int)pl.tile_bits, cb = (int)pl.chunk_bits, nrest = (int)pl.nrest, ne = nloc - k;
  CHECK((int)pl.k == k && kt == (nloc < 8 ? k : std::min(k, 6)), "n=%d k=%d: k %u tile_bits %d", nloc, k, pl.k, kt);
  CHECK(pl.path == (nloc < 8 ? (uint32_t)QH_DENSITY_GATHER : (uint32_t)QH_DENSITY_TILES), "n=%d k=%d: path %u", nloc, k, pl.path);
  CHECK(cb + nrest == ne, "n=%d k=%d: chunk_bits %d + nrest %d != %d", nloc, k, cb, nrest, ne);
  // the tables
  uint64_t reg = 0, cols = 0, rest = 0;
  for (int j = 0; j < k; ++j) {
    CHECK(j == 0 || pl.row_pos[j] > pl.row_pos[j - 1], "n=%d k=%d: rows not ascending", nloc, k);
    CHECK(pl.row_bit[j] < k && pos[pl.row_bit[j]] == pl.row_pos[j], "n=%d k=%d: row_bit[%d]", nloc, k, j);
    reg |= 1ull << pl.row_pos[j];
  }
  for (int c = 0; c < cb; ++c) {
    CHECK(c == 0 || pl.col_pos[c] > pl.col_pos[c - 1], "n=%d k=%d: columns not ascending", nloc, k);
    cols |= 1ull << pl.col_pos[c];
  }
  for (int q = 0; q < nrest; ++q) {
    CHECK(q == 0 || pl.rest_pos[q] > pl.rest_pos[q - 1], "n=%d k=%d: rest not ascending", nloc, k);
    CHECK(cb == 0 || pl.rest_pos[q] > pl.col_pos[cb - 1], "n=%d k=%d: a rest position below a column", nloc, k);
    rest |= 1ull << pl.rest_pos[q];
  }
  CHECK(__builtin_popcountll(reg) == k && __builtin_popcountll(cols) == cb && __builtin_popcountll(rest) == nrest, "n=%d k=%d: repeated positions", nloc, k);
  CHECK((reg & cols) == 0 && (reg & rest) == 0 && (cols & rest) == 0 && (reg | cols | rest) == (1ull << nloc) - 1, "n=%d k=%d: not a partition", nloc, k);
  // the geometry
  const uint32_t nb = 1u << (k - kt), npairs = nb * (nb + 1) / 2;
  CHECK(pl.block_pairs == npairs && (npairs == 1 || npairs == 3 || npairs == 10), "n=%d k=%d: %u block pairs", nloc, k, pl.block_pairs);
  CHECK((uint64_t)pl.wg_per_pair * pl.chunks_per_wg << cb == 1ull << ne, "n=%d k=%d: %u x %llu x 2^%d columns", nloc, k, pl.wg_per_pair,
        (unsigned long long)pl.chunks_per_wg, cb);
  if (pl.path == QH_DENSITY_GATHER) {
    CHECK(cb == 0 && pl.wg_per_pair == 1 && pl.slab_bytes == 0 && pl.amps_swept == 1ull << nloc, "n=%d k=%d: gather geometry", nloc, k);
  } else {
    CHECK(cb == std::min(ne, qh::kDensityLdsBits - kt - (nb > 1 ? 1 : 0)), "n=%d k=%d: chunk_bits %d", nloc, k, cb);
    CHECK(pl.slab_bytes == ((uint64_t)16 << (2 * kt)) * pl.wg_per_pair * npairs && pl.slab_bytes <= qh::kDensitySlabBytes, "n=%d k=%d: slab", nloc, k);
    CHECK(pl.wg_per_pair * npairs <= qh::kDensityMaxWgs, "n=%d k=%d: grid", nloc, k);
    CHECK(pl.amps_swept == (uint64_t)nb << nloc, "n=%d k=%d: swept", nloc, k);
    // a chunk of a tile is made of runs: every position below the lowest one it does not hold belongs to it
    const uint64_t held = cols | spread((1ull << kt) - 1, pl.row_pos, kt);
    int run = 0;
    while ((held >> run) & 1ull) ++run;
    CHECK(run >= std::min(6, cb), "n=%d k=%d: runs of 2^%d", nloc, k, run);
  }
  // the walk
  uint8_t upos[16], urow[16];
  for (int i = 0, jr = 0, jc = 0; i < kt + cb; ++i) {
    const bool row = jc == cb || (jr < kt && pl.row_pos[jr] < pl.col_pos[jc]);
    upos[i] = row ? pl.row_pos[jr] : pl.col_pos[jc];
    urow[i] = row ? (uint8_t)jr++ : (uint8_t)(16 + jc++);
    CHECK(i == 0 || upos[i] > upos[i - 1], "n=%d k=%d: load order not ascending", nloc, k);
  }
  // a 16-byte item of complex64 is the two amplitudes that differ in position 0: the load order must begin there
  CHECK(pl.path != QH_DENSITY_TILES || upos[0] == 0, "n=%d k=%d: position 0 is not the first of the load order", nloc, k);
  const uint64_t n = 1ull << nloc;
  std::vector<uint8_t> seen(n * npairs, 0);
  for (uint32_t p = 0; p < npairs; ++p) {
    uint32_t R, C;
    qh::density_pair(nb, p, &R, &C);
    CHECK(R <= C && C < nb, "n=%d k=%d: pair %u = (%u, %u)", nloc, k, p, R, C);
    for (uint32_t w = 0; w < pl.wg_per_pair; ++w)
      for (uint64_t q = w * pl.chunks_per_wg; q < (w + 1) * pl.chunks_per_wg; ++q)
        for (int side = 0; side < (R == C ? 1 : 2); ++side) {
          const uint32_t blk = side ? C : R;
          const uint64_t base = spread(q, pl.rest_pos, nrest) | spread(blk, pl.row_pos + kt, k - kt);
          for (uint64_t j = 0; j < 1ull << (kt + cb); ++j) {
            uint64_t at = base;
            uint32_t rc = 0;
            for (int i = 0; i < kt + cb; ++i) {
              at |= ((j >> i) & 1ull) << upos[i];
              rc |= (uint32_t)((j >> i) & 1u) << urow[i];
            }
            CHECK(at < n, "n=%d k=%d: index %llu", nloc, k, (unsigned long long)at);
            if (at >= n) continue;
            ++seen[p * n + at];
            // the kernel's (row, column) against the positions
            uint32_t row = 0, col = 0;
            for (int jr = 0; jr < kt; ++jr) row |= (uint32_t)((at >> pl.row_pos[jr]) & 1ull) << jr;
            for (int jc = 0; jc < cb; ++jc) col |= (uint32_t)((at >> pl.col_pos[jc]) & 1ull) << jc;
            CHECK((rc & 0xffffu) == row && (rc >> 16) == col, "n=%d k=%d: amplitude %llu lands on (%u, %u)", nloc, k,
                  (unsigned long long)at, rc & 0xffffu, rc >> 16);
          }
        }
    for (uint64_t i = 0; i < n; ++i) {
      uint32_t blk = 0;
      for (int j = kt; j < k; ++j) blk |= (uint32_t)((i >> pl.row_pos[j]) & 1ull) << (j - kt);
      const uint8_t want = (blk == R || blk == C) ? 1 : 0;
      if (seen[p * n + i] != want) {
        CHECK(false, "n=%d k=%d pair %u: amplitude %llu visited %u times, want %u", nloc, k, p, (unsigned long long)i, seen[p * n + i], want);
        break;
      }
    }
  }
}

int main(int argc, char **argv) {
  const int count = argc > 1 ? atoi(argv[1]) : 6, nmax = argc > 2 ? atoi(argv[2]) : 12;
  std::mt19937_64 rng(14);
  int plans = 0;
  for (int nloc = 1; nloc <= nmax; ++nloc)
    for (int k = 0; k <= std::min(nloc, QH_DENSITY_MAX_BITS); ++k)
      for (int s = 0; s < count; ++s) {
        std::vector<int> all(nloc);
        std::iota(all.begin(), all.end(), 0);
        if (s == 1) std::reverse(all.begin(), all.end());      // s == 0: the lowest positions; 1: the highest; then random
        if (s >= 2) std::shuffle(all.begin(), all.end(), rng);
        std::vector<int> pos(all.begin(), all.begin() + k);
        if (s >= 1) std::shuffle(pos.begin(), pos.end(), rng);
        pos.resize(QH_DENSITY_MAX_BITS, 0);
        check_one(nloc, k, pos);
        ++plans;
      }
  if (failures) {
    fprintf(stderr, "%d failures\n", failures);
    return 1;
  }
  printf("ok: %d plans\n", plans);
  return 0;
}
