// perm_plan_check.cc -- stand-alone check of qcc_amd/csrc/perm_plan.h (the host side of qh_apply_perm), for sanitizer builds:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -static-libasan -static-libubsan \
//       tools/perm_plan_check.cc -o perm_plan_check
// (the sanitizer runtimes linked statically: the program then runs as it is, in any environment).
// For `count` random cases per size (1..14 local bits, default 200; both widths) -- a random bit map, a random register in
// random order, random controls, a random table -- it executes the plan as the kernels do (the LDS walk tile by tile from
// the 16-bit table over in-tile index bits, the gather walk from the 64-bit table over physical positions) and compares
// with a brute-force model of new[i with register := table[s(i)]] = old[i]; every amplitude must be written exactly once by
// the gather walk, and exactly the amplitudes of the tiles that are not skipped by the LDS walk.  Then the table checker
// must name the first offending entry.  Exit status 0 = all good.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <random>
#include <vector>

#include "../qcc_amd/csrc/perm_plan.h"

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

static uint64_t pdep(uint64_t v, uint64_t mask) {
  uint64_t o = 0;
  for (; mask; mask &= mask - 1, v >>= 1)
    if (v & 1ull) o |= mask & (~mask + 1ull);
  return o;
}
static uint32_t gather(uint64_t idx, int n, const uint32_t *run) {
  uint32_t s = 0;
  for (int r = 0; r < n; ++r) s |= ((uint32_t)(idx >> (run[r] & 0xffu)) & ((1u << (run[r] >> 16)) - 1u)) << ((run[r] >> 8) & 0xffu);
  return s;
}

static void check_case(int nloc, int bw, int k, const std::vector<int> &reg_pos, uint64_t ctl, const std::vector<uint32_t> &table) {
  const uint64_t n = 1ull << nloc;
  // the model: amplitude i holds the number i; want[j] = the old index of what ends at j
  std::vector<uint64_t> want(n);
  for (uint64_t i = 0; i < n; ++i) {
    uint64_t j = i;
    if ((i & ctl) == ctl) {
      uint32_t s = 0;
      for (int b = 0; b < k; ++b) s |= (uint32_t)((i >> reg_pos[b]) & 1ull) << b;
      const uint32_t t = table[s];
      for (int b = 0; b < k; ++b) j = (j & ~(1ull << reg_pos[b])) | ((uint64_t)((t >> b) & 1u) << reg_pos[b]);
    }
    want[j] = i;
  }
  int64_t other = 0;
  CHECK(qh::perm_check_table(k, table.data(), &other) == -1, "a bijection was refused");
  qh_perm_tiles t;
  qh::plan_perm_tiles(nloc, bw, k, reg_pos.data(), ctl, &t);
  const int line = std::min(bw == 128 ? 3 : 4, nloc);
  const int m = (int)t.tile_bits;
  CHECK(__builtin_popcountll(t.tile_mask) == m && m >= std::min(nloc, qh::kPermPadBits) && m <= k + line + qh::kPermPadBits,
        "nloc %d: tile of %d bits", nloc, m);
  CHECK((t.tile_mask & t.reg_mask) == t.reg_mask && (t.tile_mask & ((1ull << line) - 1)) == (1ull << line) - 1 && (t.tile_mask >> nloc) == 0,
        "nloc %d: tile %llx does not hold register %llx and the line", nloc, (unsigned long long)t.tile_mask, (unsigned long long)t.reg_mask);
  CHECK(m <= std::max(k + line, std::min(nloc, qh::kPermPadBits)), "nloc %d: tile padded beyond need", nloc);
  CHECK(t.ctl_in == (ctl & t.tile_mask) && t.ctl_out == (ctl & ~t.tile_mask), "nloc %d: controls split wrongly", nloc);
  CHECK(t.lds_bytes == ((uint64_t)(bw / 8) << m) && (t.path == QH_PERM_LDS) == (t.lds_bytes <= qh::kPermLdsBytes), "nloc %d: path", nloc);
  CHECK(t.ntiles == (1ull << (nloc - m)) && t.tiles_skipped == t.ntiles - (t.ntiles >> __builtin_popcountll(t.ctl_out)), "nloc %d: tile counts", nloc);
  int order[QH_PERM_MAX_BITS];
  qh::perm_order(k, t.reg_pos, order);
  const std::vector<uint32_t> inv = qh::perm_inverse(k, table.data(), order);
  std::vector<uint64_t> got(n, ~0ull);
  std::vector<uint8_t> written(n, 0);
  {   // the gather walk
    uint8_t pos[QH_PERM_MAX_BITS];
    for (int b = 0; b < k; ++b) pos[b] = t.reg_pos[b];
    std::sort(pos, pos + k);
    uint32_t run[qh::kPermMaxRuns];
    const int nr = qh::perm_runs(k, pos, run);
    CHECK(nr >= 1 && nr <= k, "runs");
    for (uint64_t i = 0; i < n; ++i) {
      uint64_t j = i;
      if ((i & ctl) == ctl) j = (i & ~t.reg_mask) | qh::perm_deposit(inv[gather(i, nr, run)], k, pos);
      CHECK(j < n, "gather source out of range");
      if (j >= n) return;
      got[i] = j;
      ++written[i];
    }
    for (uint64_t i = 0; i < n; ++i) CHECK(written[i] == 1 && got[i] == want[i], "nloc %d k %d: gather walk: %llu comes from %llu, want %llu",
                                           nloc, k, (unsigned long long)i, (unsigned long long)got[i], (unsigned long long)want[i]);
  }
  {   // the LDS walk (also where the tile does not fit: the geometry is the same)
    uint8_t ranks[QH_PERM_MAX_BITS];
    for (int b = 0; b < k; ++b) ranks[b] = t.reg_rank[b];
    std::sort(ranks, ranks + k);
    uint32_t run[qh::kPermMaxRuns];
    const int nr = qh::perm_runs(k, ranks, run);
    uint32_t reg_tile = 0, ctl_tile = 0;
    for (int p = 0, r = 0; p < nloc; ++p) {
      if (!((t.tile_mask >> p) & 1ull)) continue;
      if ((t.reg_mask >> p) & 1ull) reg_tile |= 1u << r;
      if ((t.ctl_in >> p) & 1ull) ctl_tile |= 1u << r;
      ++r;
    }
    std::fill(written.begin(), written.end(), 0);
    for (uint64_t i = 0; i < n; ++i) got[i] = i;          // skipped tiles keep what they hold
    const uint64_t rest = (n - 1) & ~t.tile_mask & ~t.ctl_out;
    std::vector<uint64_t> lds(1ull << m);
    for (uint64_t tile = 0; tile < t.ntiles - t.tiles_skipped; ++tile) {
      const uint64_t base = pdep(tile, rest) | t.ctl_out;
      for (uint32_t r = 0; r < (1u << m); ++r) lds[r] = base | pdep(r, t.tile_mask);      // "load": the old index
      for (uint32_t r = 0; r < (1u << m); ++r) {
        uint32_t src = r;
        if ((r & ctl_tile) == ctl_tile) {
          const uint64_t e = qh::perm_deposit(inv[gather(r, nr, run)], k, ranks);
          CHECK(e < (1u << m) && (e & ~(uint64_t)reg_tile) == 0 && e <= 0xffffu, "table entry outside the register's in-tile bits");
          src = (r & ~reg_tile) | (uint32_t)e;
        }
        const uint64_t dst = base | pdep(r, t.tile_mask);
        CHECK(dst < n && src < (1u << m), "LDS walk out of range");
        if (dst >= n || src >= (1u << m)) return;
        got[dst] = lds[src];
        ++written[dst];
      }
    }
    for (uint64_t i = 0; i < n; ++i) {
      const bool run_tile = (i & t.ctl_out) == t.ctl_out;
      CHECK(written[i] == (run_tile ? 1 : 0), "nloc %d: index %llu written %d times", nloc, (unsigned long long)i, written[i]);
      CHECK(got[i] == want[i], "nloc %d k %d: LDS walk: %llu comes from %llu, want %llu", nloc, k, (unsigned long long)i,
            (unsigned long long)got[i], (unsigned long long)want[i]);
    }
  }
}

int main(int argc, char **argv) {
  const int count = argc > 1 ? atoi(argv[1]) : 200;
  std::mt19937_64 rng(20241019);
  for (int nloc = 1; nloc <= 14; ++nloc)
    for (int c = 0; c < count; ++c) {
      const int bw = (c & 1) ? 64 : 128;
      std::vector<int> pos(nloc);
      std::iota(pos.begin(), pos.end(), 0);
      std::shuffle(pos.begin(), pos.end(), rng);
      const int k = 1 + (int)(rng() % (uint64_t)nloc);
      std::vector<int> reg(pos.begin(), pos.begin() + k);
      uint64_t ctl = 0;
      const int nctl = (int)(rng() % 4);
      for (int j = 0; j < nctl && k + j < nloc; ++j) ctl |= 1ull << pos[k + j];
      std::vector<uint32_t> table(1u << k);
      std::iota(table.begin(), table.end(), 0u);
      std::shuffle(table.begin(), table.end(), rng);
      check_case(nloc, bw, k, reg, ctl, table);
    }
  {   // a 16-bit register: the largest tables, both paths' arithmetic
    std::vector<int> reg(16);
    std::iota(reg.begin(), reg.end(), 0);
    std::shuffle(reg.begin(), reg.end(), rng);
    std::vector<uint32_t> table(1u << 16);
    std::iota(table.begin(), table.end(), 0u);
    std::shuffle(table.begin(), table.end(), rng);
    check_case(16, 128, 16, reg, 0, table);
  }
  {   // the table checker names the first offending entry
    std::vector<uint32_t> t = {0, 3, 1, 2};
    int64_t other = 7;
    CHECK(qh::perm_check_table(2, t.data(), &other) == -1, "identity-like table refused");
    t = {0, 3, 4, 2};
    CHECK(qh::perm_check_table(2, t.data(), &other) == 2 && other == -1, "an entry out of range was not reported");
    t = {2, 3, 1, 3};
    CHECK(qh::perm_check_table(2, t.data(), &other) == 3 && other == 1, "a value hit twice was not reported");
  }
  if (failures) {
    fprintf(stderr, "%d failures\n", failures);
    return 1;
  }
  printf("perm_plan_check: ok\n");
  return 0;
}
