// pauli_plan_check.cc -- stand-alone check of qcc_amd/csrc/pauli_plan.h (the host side of qh_apply_pauli_sum), for sanitizer
// builds:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -static-libasan -static-libubsan \
//       tools/pauli_plan_check.cc -o pauli_plan_check
// (the sanitizer runtimes linked statically: the program then runs as it is, in any environment).
// For `count` random term lists (default 20) on a random bit map of each size from 10 to 14 local bits, at both widths, it
// walks the state as k_pauli_batch does -- chunk, register index u, thread, half -- and checks at EVERY amplitude index i that
//   * the product of the four split signs equals (-1)^popcount(i & pz),
//   * the partner address (item, half) is i ^ px,
// and that the walk covers every index exactly once; then that the sort is stable, the cut is every kPauliT terms, the
// group counts are the distinct x masks and the coefficients c' are c (-i)^nY (shard sign).  Exit status 0 = all good.
#include <algorithm>
#include <complex>
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <random>
#include <vector>

#include "../qcc_amd/csrc/pauli_plan.h"

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

static uint64_t spread(uint64_t v, const std::vector<int> &perm) {      // logical mask -> physical
  uint64_t o = 0;
  for (size_t l = 0; l < perm.size(); ++l) o |= ((v >> l) & 1ull) << perm[l];
  return o;
}

// every index of a 2^nloc state at amp_bits, for one term: in the order of the blocks' runs of chunks where the state has the
// main shape, item by item below it (there the chunk number is 0 and the register index stops early)
static void check_walk(int nloc, int amp_bits, uint64_t px, uint64_t pz) {
  const qh::PauliZSplit z = qh::pauli_split_z(pz, amp_bits);
  const uint64_t n = 1ull << nloc, nitems = n >> amp_bits;
  std::vector<uint64_t> items;
  if (qh::pauli_main_shape(nloc, amp_bits)) {
    const qh::PauliGrid g = qh::pauli_grid(nloc, amp_bits);
    CHECK(g.nblk * g.cpb == g.nchunks && g.nblk <= qh::kPauliBlocks, "nloc %d: %llu blocks x %u chunks != %llu", nloc,
          (unsigned long long)g.nblk, g.cpb, (unsigned long long)g.nchunks);
    for (uint64_t blk = 0; blk < g.nblk; ++blk)
      for (uint64_t q = blk * g.cpb; q < (blk + 1) * g.cpb; ++q)
        for (uint32_t u = 0; u < (uint32_t)qh::kPauliPer; ++u)
          for (uint32_t t = 0; t < 256; ++t) items.push_back(qh::pauli_item(q, u, t));
  } else {
    for (uint64_t item = 0; item < nitems; ++item) items.push_back(item);
  }
  std::vector<uint8_t> seen(n, 0);
  for (const uint64_t item : items) {
    const uint64_t q = item >> qh::kPauliChunkBits;
    const uint32_t u = (uint32_t)(item >> 8) & (uint32_t)(qh::kPauliPer - 1), t = (uint32_t)(item & 255ull);
    CHECK(item < nitems && qh::pauli_item(q, u, t) == item, "nloc %d: item %llu", nloc, (unsigned long long)item);
    if (item >= nitems) return;
    for (uint32_t h = 0; h < (1u << amp_bits); ++h) {
      const uint64_t i = (item << amp_bits) | h;
      ++seen[i];
      const uint32_t s = qh::pauli_sign_half(z, h) ^ qh::pauli_sign_thread(z, t) ^ qh::pauli_sign_reg(z, u) ^ qh::pauli_sign_chunk(z, q);
      CHECK(s == (uint32_t)(__builtin_popcountll(i & pz) & 1), "nloc %d width bit %d: sign at %llu for z 0x%llx", nloc, amp_bits,
            (unsigned long long)i, (unsigned long long)pz);
      const uint64_t pi = (qh::pauli_partner_item(item, px, amp_bits) << amp_bits) | qh::pauli_partner_half(h, px, amp_bits);
      CHECK(pi == (i ^ px), "nloc %d width bit %d: partner of %llu for x 0x%llx is %llu", nloc, amp_bits, (unsigned long long)i,
            (unsigned long long)px, (unsigned long long)pi);
    }
  }
  for (uint64_t i = 0; i < n; ++i) CHECK(seen[i] == 1, "nloc %d: index %llu covered %d times", nloc, (unsigned long long)i, seen[i]);
}

int main(int argc, char **argv) {
  const int count = argc > 1 ? atoi(argv[1]) : 20;
  std::mt19937_64 rng(20240911);
  uint64_t walks = 0;
  for (int nloc = 10; nloc <= 14; ++nloc)
    for (int c = 0; c < count; ++c) {
      std::vector<int> perm(nloc);
      std::iota(perm.begin(), perm.end(), 0);
      std::shuffle(perm.begin(), perm.end(), rng);
      const uint64_t mask = (1ull << nloc) - 1ull;
      const uint64_t nterms = 1 + rng() % 40, nx = 1 + rng() % 20;
      std::vector<uint64_t> xs(nx);
      for (auto &x : xs) x = rng() & mask;
      std::vector<qh_pauli_term> terms(nterms);
      std::vector<uint64_t> lx(nterms), lz(nterms);
      for (uint64_t t = 0; t < nterms; ++t) {
        lx[t] = xs[rng() % nx];
        lz[t] = rng() & mask;
        terms[t] = qh_pauli_term{t, spread(lx[t], perm), spread(lz[t], perm), (uint32_t)(rng() & 1u),
                                 (uint32_t)__builtin_popcountll(lx[t] & lz[t]) & 3u};
      }
      const std::vector<qh_pauli_term> given = terms;
      qh::pauli_sort(terms.data(), nterms);
      for (uint64_t k = 1; k < nterms; ++k)
        CHECK(terms[k - 1].px < terms[k].px || (terms[k - 1].px == terms[k].px && terms[k - 1].index < terms[k].index), "sort not stable at %llu",
              (unsigned long long)k);
      std::vector<qh_pauli_batch> batches(nterms);
      const uint64_t nb = qh::pauli_cut(terms.data(), nterms, batches.data(), batches.size());
      CHECK(nb == (nterms + qh::kPauliT - 1) / qh::kPauliT, "%llu terms cut into %llu batches", (unsigned long long)nterms, (unsigned long long)nb);
      CHECK(qh::pauli_cut(terms.data(), nterms, nullptr, 0) == nb, "the count-only form disagrees");
      uint64_t at = 0;
      for (uint64_t b = 0; b < nb; ++b) {
        const qh_pauli_batch &bt = batches[b];
        CHECK(bt.first == at && bt.count >= 1 && bt.count <= (uint64_t)qh::kPauliT && (b + 1 == nb || bt.count == (uint64_t)qh::kPauliT),
              "batch %llu: first %llu count %llu", (unsigned long long)b, (unsigned long long)bt.first, (unsigned long long)bt.count);
        std::vector<uint64_t> distinct;
        for (uint64_t k = 0; k < bt.count; ++k) distinct.push_back(terms[bt.first + k].px);
        distinct.erase(std::unique(distinct.begin(), distinct.end()), distinct.end());
        CHECK(bt.ngroups == distinct.size() && bt.streams == bt.ngroups + 1 + (b ? 1 : 0), "batch %llu: %llu groups, %llu streams",
              (unsigned long long)b, (unsigned long long)bt.ngroups, (unsigned long long)bt.streams);
        at += bt.count;
      }
      CHECK(at == nterms, "batches hold %llu of %llu terms", (unsigned long long)at, (unsigned long long)nterms);
      for (uint64_t k = 0; k < nterms; ++k) {      // c' against complex arithmetic, and the unit detection
        const qh_pauli_term &tm = terms[k];
        CHECK(tm.px == given[tm.index].px && tm.pz == given[tm.index].pz, "term %llu lost its masks", (unsigned long long)k);
        const double re = (double)(int)(rng() % 5) - 2.0, im = (double)(int)(rng() % 5) - 2.0;
        double cp[2];
        qh::pauli_coef(re, im, tm.ny, tm.neg, cp);
        std::complex<double> want(re, im);
        for (uint32_t j = 0; j < tm.ny; ++j) want *= std::complex<double>(0.0, -1.0);
        if (tm.neg) want = -want;
        CHECK(cp[0] == want.real() && cp[1] == want.imag(), "c' of (%g, %g) ny %u neg %u is (%g, %g)", re, im, tm.ny, tm.neg, cp[0], cp[1]);
        const int unit = qh::pauli_unit(cp);
        if (unit >= 0) {
          std::complex<double> p(1.0, 0.0);
          for (int j = 0; j < unit; ++j) p *= std::complex<double>(0.0, 1.0);
          CHECK(p == std::complex<double>(cp[0], cp[1]), "unit %d for (%g, %g)", unit, cp[0], cp[1]);
        } else {
          CHECK(std::abs(std::complex<double>(cp[0], cp[1])) != 1.0 || (cp[0] != 0.0 && cp[1] != 0.0), "unit missed (%g, %g)", cp[0], cp[1]);
        }
      }
      // every index, for two of the terms at either width (the first of the sorted list and a random one)
      for (int amp_bits = 0; amp_bits <= 1; ++amp_bits)
        for (const uint64_t k : {(uint64_t)0, (uint64_t)(rng() % nterms)}) {
          check_walk(nloc, amp_bits, terms[k].px, terms[k].pz);
          ++walks;
        }
    }
  // the masks that exercise one part each: the sub-item bit, thread, register index, chunk, all
  for (int amp_bits = 0; amp_bits <= 1; ++amp_bits)
    for (const uint64_t m : {0x1ull, 0x2ull, 0x40ull, 0x100ull, 0x200ull, 0x400ull, 0x800ull, 0x1000ull, 0x2000ull, 0x3fffull, 0x0ull}) {
      check_walk(14, amp_bits, m, m);
      check_walk(14, amp_bits, 0x3fffull ^ m, m);
      walks += 2;
    }
  CHECK(!qh::pauli_main_shape(10, 0) && qh::pauli_main_shape(11, 0) && !qh::pauli_main_shape(11, 1) && qh::pauli_main_shape(12, 1),
        "the threshold between the two kernels moved");
  if (failures) {
    fprintf(stderr, "%d failures\n", failures);
    return 1;
  }
  printf("pauli_plan_check: ok (%llu walks)\n", (unsigned long long)walks);
  return 0;
}
