// rank1_plan_check.cc -- stand-alone check of qcc_amd/csrc/rank1_plan.h (the host side of qh_apply_rank1), for sanitizer builds:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -static-libasan -static-libubsan \
//       tools/rank1_plan_check.cc -o rank1_plan_check
// (the sanitizer runtimes linked statically: the program then runs as it is, in any environment).
// For `count` random cases per size (1..16 local bits, default 60; both widths; table and uniform form) -- a random register
// in random order, random controls, random u, v, a, b -- it executes the plan as the kernels do and compares with a brute-force
// model of psi'[s, r] = a psi[s, r] + b u[s] sum_s' conj(v[s']) psi[s', r]:
//   TILE      tile by tile: products by the compressed table over in-tile index bits, fibre sums, update; exactly the
//             amplitudes of the tiles that are not skipped are written, once;
//   TWO_PASS  pass 1 unit by unit (group, segment) over the chunks of its walk, the sums of a chunk's fibres written to
//             scratch[segment][fibre], the fold in segment order, pass 2 with the fibre index = the physical index with the
//             register bits taken out; every scratch entry is written exactly once and lies inside scratch_bytes.
// Exit status 0 = all good.
#include <algorithm>
#include <complex>
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <random>
#include <vector>

#include "../qcc_amd/csrc/rank1_plan.h"

typedef std::complex<double> cplx;

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
static uint64_t pext(uint64_t v, uint64_t mask) {
  uint64_t o = 0;
  for (int b = 0; mask; mask &= mask - 1, ++b)
    if (v & mask & (~mask + 1ull)) o |= 1ull << b;
  return o;
}

static void check_case(int nloc, int bw, int k, const std::vector<int> &reg_pos, uint64_t ctl, bool uniform, std::mt19937_64 &rng) {
  const uint64_t n = 1ull << nloc;
  std::normal_distribution<double> g;
  std::vector<cplx> psi(n), u((size_t)1 << k), v((size_t)1 << k);
  for (auto &x : psi) x = cplx(g(rng), g(rng));
  for (auto &x : u) x = uniform ? cplx(std::sqrt(std::ldexp(1.0, -k)), 0) : cplx(g(rng), g(rng));
  for (auto &x : v) x = uniform ? cplx(std::sqrt(std::ldexp(1.0, -k)), 0) : cplx(g(rng), g(rng));
  const cplx a(g(rng), g(rng)), b(g(rng), g(rng));
  uint64_t reg_mask = 0;
  for (int j = 0; j < k; ++j) reg_mask |= 1ull << reg_pos[j];
  auto field = [&](uint64_t i) {      // the register's value in the caller's numbering
    uint32_t s = 0;
    for (int j = 0; j < k; ++j) s |= (uint32_t)((i >> reg_pos[j]) & 1ull) << j;
    return s;
  };
  // the model
  std::vector<cplx> mfull(n, cplx(0, 0)), want(n);
  for (uint64_t i = 0; i < n; ++i) mfull[i & ~reg_mask] += std::conj(v[field(i)]) * psi[i];
  double scale = 0;
  for (uint64_t i = 0; i < n; ++i) {
    want[i] = (i & ctl) == ctl ? a * psi[i] + b * u[field(i)] * mfull[i & ~reg_mask] : psi[i];
    scale = std::max(scale, std::abs(want[i]));
  }
  qh_rank1_info pl;
  qh::plan_rank1(nloc, bw, k, reg_pos.data(), ctl, uniform, &pl);
  const qh_perm_tiles &t = pl.tile;
  const int m = (int)t.tile_bits;
  const uint64_t state = (uint64_t)(bw / 8) << nloc;
  CHECK((t.tile_mask & reg_mask) == reg_mask && t.reg_mask == reg_mask && (t.tile_mask >> nloc) == 0, "nloc %d: tile does not hold the register", nloc);
  CHECK(t.lds_bytes == ((uint64_t)(bw / 8) << m), "lds_bytes");
  CHECK((pl.path == QH_RANK1_TILE) == (t.lds_bytes <= qh::kPermLdsBytes && (uniform || k <= qh::kPermPadBits)), "nloc %d k %d: path", nloc, k);
  CHECK(pl.nfibres == n >> k && pl.uniform == (uniform ? 1u : 0u), "nfibres / uniform");
  // the tables as the engine uploads them
  std::vector<double> vc, ub;
  const double bb[2] = {b.real(), b.imag()};
  if (!uniform) {
    CHECK(k <= QH_RANK1_MAX_BITS, "table form above 16 bits");
    qh::rank1_tables(k, t.reg_pos, (const double *)u.data(), (const double *)v.data(), bb, &vc, &ub);
    CHECK(vc.size() == (size_t)2 << k && ub.size() == (size_t)2 << k, "table sizes");
  }
  auto tab = [&](const std::vector<double> &tb, uint64_t c, cplx uni) {
    if (uniform) return uni;
    CHECK(c < ((uint64_t)1 << k), "table index %llu out of range", (unsigned long long)c);
    if (c >= ((uint64_t)1 << k)) return cplx(0, 0);
    return cplx(tb[2 * c], tb[2 * c + 1]);
  };
  const cplx uni_v = v[0], uni_ub = b * u[0];
  std::vector<cplx> got = psi;
  std::vector<uint8_t> written(n, 0);
  if (pl.path == QH_RANK1_TILE) {
    CHECK(pl.kernels == 1 && pl.scratch_bytes == 0, "TILE: kernels / scratch");
    CHECK(pl.bytes_swept == 2 * (t.ntiles - t.tiles_skipped) * t.lds_bytes, "TILE: bytes_swept");
    uint32_t reg_tile = 0, ctl_tile = 0;
    for (int p = 0, r = 0; p < nloc; ++p) {
      if (!((t.tile_mask >> p) & 1ull)) continue;
      if ((t.reg_mask >> p) & 1ull) reg_tile |= 1u << r;
      if ((t.ctl_in >> p) & 1ull) ctl_tile |= 1u << r;
      ++r;
    }
    const uint64_t rest = (n - 1) & ~t.tile_mask & ~t.ctl_out;
    std::vector<cplx> sums((size_t)1 << m);
    for (uint64_t tile = 0; tile < t.ntiles - t.tiles_skipped; ++tile) {
      const uint64_t base = pdep(tile, rest) | t.ctl_out;
      std::fill(sums.begin(), sums.end(), cplx(0, 0));
      for (uint32_t r = 0; r < (1u << m); ++r) {
        const uint64_t i = base | pdep(r, t.tile_mask);
        CHECK(i < n, "TILE: index out of range");
        if (i >= n) return;
        sums[r & ~reg_tile] += tab(vc, pext(r, reg_tile), uni_v) * psi[i];      // compressed field: the register's in-tile bits, ascending
      }
      for (uint32_t r = 0; r < (1u << m); ++r) {
        const uint64_t i = base | pdep(r, t.tile_mask);
        if ((r & ctl_tile) != ctl_tile) continue;
        got[i] = a * psi[i] + tab(ub, pext(r, reg_tile), uni_ub) * sums[r & ~reg_tile];
        ++written[i];
      }
    }
    for (uint64_t i = 0; i < n; ++i) CHECK(written[i] == ((i & ctl) == ctl ? 1 : 0), "TILE nloc %d: index %llu written %d times", nloc, (unsigned long long)i, written[i]);
  } else {
    const int cb = (int)pl.chunk_bits;
    CHECK(cb == std::min(nloc, bw == 128 ? 11 : 12), "chunk_bits");
    const uint64_t low = (1ull << cb) - 1;
    CHECK(pl.reg_in_chunk == (uint32_t)__builtin_popcountll(reg_mask & low) && pl.reg_in_chunk + pl.reg_above == (uint32_t)k, "register split");
    CHECK(pl.groups << (cb + pl.reg_above) == n && pl.fibres_per_chunk << pl.reg_in_chunk == (1ull << cb), "groups / fibres per chunk");
    CHECK(pl.split >= 1 && (pl.split & (pl.split - 1)) == 0 && pl.walk * pl.split == (1ull << pl.reg_above), "split / walk");
    CHECK(pl.split == 1 || pl.groups * pl.split <= 2 * qh::kRank1Blocks, "split beyond need");
    CHECK(pl.scratch_bytes == 16 * pl.nfibres * (pl.split > 1 ? 1 + pl.split : 1), "scratch_bytes");
    CHECK(pl.kernels == (pl.split > 1 ? 3u : 2u) && pl.bytes_swept == 3 * state, "kernels / bytes");
    CHECK(pl.groups * pl.fibres_per_chunk == pl.nfibres, "fibre count");
    const size_t nscr = (size_t)(pl.scratch_bytes / 16);
    std::vector<cplx> scratch(nscr);
    std::vector<uint8_t> filled(nscr, 0);
    const size_t part_at = pl.split > 1 ? (size_t)pl.nfibres : 0;
    const uint64_t abv = reg_mask >> cb, grp = ((n - 1) >> cb) & ~abv;
    const uint64_t reg_low = reg_mask & low;
    std::vector<cplx> acc((size_t)1 << cb);
    for (uint64_t unit = 0; unit < pl.groups * pl.split; ++unit) {
      const uint64_t gi = unit / pl.split, seg = unit % pl.split;
      std::fill(acc.begin(), acc.end(), cplx(0, 0));
      for (uint64_t wi = seg * pl.walk; wi < (seg + 1) * pl.walk; ++wi) {
        const uint64_t chunk = pdep(gi, grp) | pdep(wi, abv);
        for (uint64_t c = 0; c <= low; ++c) {
          const uint64_t i = (chunk << cb) | c;
          CHECK(i < n, "pass 1: index out of range");
          if (i >= n) return;
          acc[c] += tab(vc, (wi << pl.reg_in_chunk) | pext(c, reg_low), uni_v) * psi[i];
        }
      }
      for (uint64_t c = 0; c <= low; ++c)
        if (c & reg_low) acc[c & ~reg_low] += acc[c];
      for (uint64_t f = 0; f < pl.fibres_per_chunk; ++f) {
        const size_t at = part_at + (size_t)(seg * pl.nfibres + gi * pl.fibres_per_chunk + f);
        CHECK(at < nscr, "pass 1: scratch entry %zu of %zu", at, nscr);
        if (at >= nscr) return;
        scratch[at] = acc[pdep(f, low & ~reg_low)];
        ++filled[at];
      }
    }
    for (size_t i = part_at; i < part_at + (size_t)(pl.split * pl.nfibres) && i < nscr; ++i) CHECK(filled[i] == 1, "pass 1: scratch entry %zu written %d times", i, filled[i]);
    if (pl.split > 1)
      for (uint64_t f = 0; f < pl.nfibres; ++f) {
        cplx s = scratch[part_at + f];
        for (uint32_t sg = 1; sg < pl.split; ++sg) s += scratch[part_at + (size_t)sg * pl.nfibres + f];
        scratch[f] = s;
      }
    const uint64_t free_mask = (n - 1) & ~reg_mask;
    for (uint64_t i = 0; i < n; ++i) {
      const uint64_t f = pext(i, free_mask);
      CHECK(f < pl.nfibres, "pass 2: fibre out of range");
      if (f >= pl.nfibres) return;
      CHECK(std::abs(scratch[f] - mfull[i & ~reg_mask]) <= 1e-11 * (1 + std::abs(scratch[f])), "nloc %d k %d: m of fibre %llu", nloc, k, (unsigned long long)f);
      if ((i & ctl) != ctl) continue;
      got[i] = a * psi[i] + tab(ub, pext(i, reg_mask), uni_ub) * scratch[f];
    }
  }
  for (uint64_t i = 0; i < n; ++i)
    CHECK(std::abs(got[i] - want[i]) <= 1e-11 * (1 + scale), "nloc %d k %d bw %d path %u: amplitude %llu", nloc, k, bw, pl.path, (unsigned long long)i);
}

int main(int argc, char **argv) {
  const int count = argc > 1 ? atoi(argv[1]) : 60;
  std::mt19937_64 rng(20261021);
  int paths[2] = {0, 0};
  for (int nloc = 1; nloc <= 16; ++nloc)
    for (int c = 0; c < (nloc > 13 ? std::max(4, count / 2) : count); ++c) {
      const int bw = (c & 1) ? 64 : 128;
      const bool uniform = (c & 2) != 0;
      std::vector<int> pos(nloc);
      std::iota(pos.begin(), pos.end(), 0);
      std::shuffle(pos.begin(), pos.end(), rng);
      int k = 1 + (int)(rng() % (uint64_t)nloc);
      if (nloc > 13 && (c & 4)) k = std::max(k, nloc - 3);      // wide registers: the second path
      std::vector<int> reg(pos.begin(), pos.begin() + k);
      uint64_t ctl = 0;
      const int nctl = (int)(rng() % 4);
      for (int j = 0; j < nctl && k + j < nloc; ++j) ctl |= 1ull << pos[k + j];
      check_case(nloc, bw, k, reg, ctl, uniform, rng);
      qh_rank1_info pl;
      qh::plan_rank1(nloc, bw, k, reg.data(), ctl, uniform, &pl);
      ++paths[pl.path];
    }
  {   // a register wider than the tile struct has room for: the uniform form only
    std::vector<int> reg(18);
    std::iota(reg.begin(), reg.end(), 0);
    std::shuffle(reg.begin(), reg.end(), rng);
    check_case(18, 64, 18, reg, 0, true, rng);
    reg.resize(17);
    check_case(18, 128, 17, reg, 0, true, rng);
  }
  CHECK(paths[0] > 0 && paths[1] > 0, "both paths must have been taken (%d, %d)", paths[0], paths[1]);
  {
    const double x[6] = {0, 1, 2, INFINITY, NAN, 5};
    CHECK(qh::rank1_first_nonfinite(x, 3) == -1 && qh::rank1_first_nonfinite(x, 6) == 3 && qh::rank1_first_nonfinite(x + 4, 2) == 0, "non-finite entries");
  }
  if (failures) {
    fprintf(stderr, "%d failures\n", failures);
    return 1;
  }
  printf("rank1_plan_check: ok (%d tile, %d two-pass)\n", paths[0], paths[1]);
  return 0;
}
