// pauli_product_plan_check.cc -- stand-alone check of qcc_amd/csrc/pauli_product_plan.h (the host side of
// qh_apply_pauli_product), for sanitizer builds:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -static-libasan -static-libubsan \
//       tools/pauli_product_plan_check.cc -o pauli_product_plan_check
// (the sanitizer runtimes linked statically: the program then runs as it is, in any environment).
// For `count` random term lists (default 20) on a random bit map of each size from 1 to 14 local bits, at both widths, it
//   * cuts the list into runs and checks that the runs partition the terms in order, that every run obeys the rule (at most
//     kPauliProdT terms, x masks 0 or one common X) and that no run could have taken the next term (the cut is greedy);
//   * walks the state as the kernels do -- PAIR: pair numbers, chunk / register index / thread as in pauli_plan.h where the
//     state has the main shape, one pair per thread below it; DIAG, HALF and PAIR with a pivot inside the line (the partner
//     then sits in another lane of the same wave): items -- and checks that every item is visited exactly once (as item0
//     or item1), that item1 = item0 ^ (X >> amp_bits) and that, at EVERY amplitude, the split signs of the walk's number
//     equal (-1)^popcount(i & pz) and the partner's sign differs by pauli_pair_flip.
// Exit status 0 = all good.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <random>
#include <vector>

#include "../qcc_amd/csrc/pauli_product_plan.h"

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

static uint32_t par(uint64_t v) { return (uint32_t)(__builtin_popcountll(v) & 1); }

// one run with pair mask X and one of its terms (z mask pz, x mask 0 or X) over a 2^nloc state
static void check_walk(int nloc, int amp_bits, uint64_t X, uint64_t pz) {
  const uint64_t n = 1ull << nloc;
  const uint32_t kind = qh::pauli_run_kind(X, amp_bits);
  const uint32_t flip = qh::pauli_pair_flip(X, pz);
  std::vector<uint8_t> seen(n, 0);
  if (!qh::pauli_product_main_shape(nloc, amp_bits)) {
    // k_pauli_product_small: amplitude pairs (X != 0) or amplitudes
    if (X) {
      const int p = 63 - __builtin_clzll(X);
      for (uint64_t w = 0; w < n / 2; ++w) {
        const uint64_t i = qh::pauli_insert0(w, p), j = i ^ X;
        CHECK(i < n && j < n && !((i >> p) & 1ull), "nloc %d: pair %llu -> (%llu, %llu)", nloc, (unsigned long long)w, (unsigned long long)i, (unsigned long long)j);
        if (i >= n || j >= n) return;
        ++seen[i];
        ++seen[j];
        CHECK((par(i & pz) ^ flip) == par(j & pz), "nloc %d: partner sign of %llu for X 0x%llx z 0x%llx", nloc, (unsigned long long)i, (unsigned long long)X,
              (unsigned long long)pz);
      }
    } else {
      for (uint64_t i = 0; i < n; ++i) ++seen[i];
    }
  } else {
    const bool lane = kind == QH_PAULI_RUN_PAIR && qh::pauli_pair_in_wave(X, amp_bits);      // items; the partner by a lane exchange
    const bool pair = kind == QH_PAULI_RUN_PAIR && !lane;
    const qh::PauliGrid g = qh::pauli_product_grid(nloc, amp_bits, pair);
    if (kind == QH_PAULI_RUN_PAIR) CHECK(lane == (qh::pauli_pair_pivot(X, amp_bits) <= qh::kPauliLanePivotMax), "X 0x%llx: in-wave rule", (unsigned long long)X);
    CHECK(g.nblk * g.cpb == g.nchunks && g.nblk <= qh::kPauliBlocks && (g.nchunks << qh::kPauliChunkBits) == (n >> amp_bits) >> (pair ? 1 : 0),
          "nloc %d kind %u: %llu blocks x %u chunks", nloc, kind, (unsigned long long)g.nblk, g.cpb);
    const int p = pair ? qh::pauli_pair_pivot(X, amp_bits) : 0;
    const qh::PauliZSplit z = qh::pauli_split_z(pair ? qh::pauli_pair_z(pz, p, amp_bits) : pz, amp_bits);
    const uint64_t nitems = n >> amp_bits;
    for (uint64_t blk = 0; blk < g.nblk; ++blk)
      for (uint64_t q = blk * g.cpb; q < (blk + 1) * g.cpb; ++q)
        for (uint32_t u = 0; u < (uint32_t)qh::kPauliPer; ++u)
          for (uint32_t t = 0; t < 256; ++t) {
            const uint64_t w = qh::pauli_item(q, u, t);
            const uint64_t item0 = pair ? qh::pauli_pair_item0(w, p) : w;
            const uint64_t item1 = pair ? qh::pauli_pair_item1(item0, X, amp_bits) : item0;
            CHECK(item0 < nitems && item1 < nitems, "nloc %d kind %u: number %llu -> items (%llu, %llu)", nloc, kind, (unsigned long long)w,
                  (unsigned long long)item0, (unsigned long long)item1);
            if (item0 >= nitems || item1 >= nitems) return;
            if (pair) CHECK(item1 != item0 && !((item0 >> p) & 1ull) && ((item1 >> p) & 1ull), "nloc %d: pivot %d of pair %llu", nloc, p, (unsigned long long)w);
            const uint32_t base = qh::pauli_sign_thread(z, t) ^ qh::pauli_sign_reg(z, u) ^ qh::pauli_sign_chunk(z, q);
            for (uint32_t h = 0; h < (1u << amp_bits); ++h) {
              const uint64_t i = (item0 << amp_bits) | h;
              ++seen[i];
              CHECK((base ^ qh::pauli_sign_half(z, h)) == par(i & pz), "nloc %d width bit %d kind %u: sign at %llu for X 0x%llx z 0x%llx", nloc, amp_bits,
                    kind, (unsigned long long)i, (unsigned long long)X, (unsigned long long)pz);
              if (pair) {      // the kernel pairs (item0, h) with (item1, h ^ (X & 1))
                const uint64_t j = (item1 << amp_bits) | (h ^ (uint32_t)(amp_bits ? (X & 1ull) : 0ull));
                ++seen[j];
                CHECK(j == (i ^ X), "nloc %d width bit %d: partner of %llu for X 0x%llx is %llu", nloc, amp_bits, (unsigned long long)i,
                      (unsigned long long)X, (unsigned long long)j);
                CHECK((par(i & pz) ^ flip) == par(j & pz), "nloc %d: partner sign of %llu", nloc, (unsigned long long)i);
              }
            }
            if (lane) {      // the thread's own item; its partner sits in lane ^ xi of the same wave, in the same step
              const uint64_t xi = X >> amp_bits, other = item0 ^ xi;
              CHECK(xi < 64 && (other >> 6) == (item0 >> 6) && qh::pauli_item(q, u, t ^ (uint32_t)xi) == other, "nloc %d: lane partner of item %llu", nloc,
                    (unsigned long long)item0);
              for (uint32_t h = 0; h < (1u << amp_bits); ++h) {
                const uint64_t i = (item0 << amp_bits) | h, j = (other << amp_bits) | (h ^ (uint32_t)(amp_bits ? (X & 1ull) : 0ull));
                CHECK(j == (i ^ X) && (par(i & pz) ^ flip) == par(j & pz), "nloc %d width bit %d: lane partner of %llu for X 0x%llx", nloc, amp_bits,
                      (unsigned long long)i, (unsigned long long)X);
              }
            }
            if (kind == QH_PAULI_RUN_HALF) {      // the pair is (item, 0) and (item, 1): the second half's sign by the flip
              const uint64_t i = item0 << 1;
              CHECK((i ^ X) == (i | 1ull) && (par(i & pz) ^ flip) == par((i | 1ull) & pz), "nloc %d: half pair at %llu", nloc, (unsigned long long)i);
            }
          }
  }
  for (uint64_t i = 0; i < n; ++i) CHECK(seen[i] == 1, "nloc %d width bit %d X 0x%llx: index %llu covered %d times", nloc, amp_bits, (unsigned long long)X,
                                          (unsigned long long)i, seen[i]);
}

static void check_runs(const std::vector<qh_pauli_term> &terms, int amp_bits) {
  const uint64_t nterms = terms.size();
  std::vector<qh_pauli_run> runs(nterms + 1);
  const uint64_t nr = qh::pauli_product_cut(terms.data(), nterms, amp_bits, runs.data(), runs.size());
  CHECK(qh::pauli_product_cut(terms.data(), nterms, amp_bits, nullptr, 0) == nr, "the count-only form disagrees");
  CHECK(nr <= nterms, "%llu runs for %llu terms", (unsigned long long)nr, (unsigned long long)nterms);
  uint64_t at = 0;
  for (uint64_t r = 0; r < nr && r < runs.size(); ++r) {
    const qh_pauli_run &rn = runs[r];
    CHECK(rn.first == at && rn.count >= 1 && rn.count <= (uint64_t)qh::kPauliProdT && rn.first + rn.count <= nterms, "run %llu: first %llu count %llu",
          (unsigned long long)r, (unsigned long long)rn.first, (unsigned long long)rn.count);
    if (rn.first + rn.count > nterms) return;
    uint64_t X = 0;
    for (uint64_t k = 0; k < rn.count; ++k) {
      const uint64_t px = terms[rn.first + k].px;
      CHECK(px == 0 || X == 0 || px == X, "run %llu holds x masks 0x%llx and 0x%llx", (unsigned long long)r, (unsigned long long)X, (unsigned long long)px);
      if (px) X = px;
    }
    CHECK(rn.px == X && rn.kind == qh::pauli_run_kind(X, amp_bits), "run %llu: px 0x%llx kind %u", (unsigned long long)r, (unsigned long long)rn.px, rn.kind);
    at += rn.count;
    if (at < nterms) {      // greedy: the next term could not have joined
      const uint64_t px = terms[at].px;
      CHECK(rn.count == (uint64_t)qh::kPauliProdT || (px != 0 && X != 0 && px != X), "run %llu stopped early", (unsigned long long)r);
    }
  }
  CHECK(at == nterms, "runs hold %llu of %llu terms", (unsigned long long)at, (unsigned long long)nterms);
}

int main(int argc, char **argv) {
  const int count = argc > 1 ? atoi(argv[1]) : 20;
  std::mt19937_64 rng(20241020);
  uint64_t walks = 0, lists = 0;
  for (int nloc = 1; nloc <= 14; ++nloc)
    for (int c = 0; c < count; ++c) {
      std::vector<int> perm(nloc);
      std::iota(perm.begin(), perm.end(), 0);
      std::shuffle(perm.begin(), perm.end(), rng);
      const uint64_t mask = (1ull << nloc) - 1ull;
      const uint64_t nterms = 1 + rng() % 50, nx = 1 + rng() % 3;
      std::vector<uint64_t> xs(nx);
      for (auto &x : xs) x = rng() & mask;
      std::vector<qh_pauli_term> terms(nterms);
      uint64_t cur = xs[0];
      for (uint64_t t = 0; t < nterms; ++t) {
        if (rng() % 6 == 0) cur = xs[rng() % nx];      // long stretches of one mask, diagonal terms in between
        const uint64_t lx = rng() % 3 == 0 ? 0 : cur, lz = rng() & mask;
        terms[t] = qh_pauli_term{t, spread(lx, perm), spread(lz, perm), (uint32_t)(rng() & 1u), (uint32_t)__builtin_popcountll(lx & lz) & 3u};
      }
      for (int amp_bits = 0; amp_bits <= 1; ++amp_bits) {
        check_runs(terms, amp_bits);
        ++lists;
        for (const uint64_t k : {(uint64_t)0, (uint64_t)(rng() % nterms)}) {
          check_walk(nloc, amp_bits, terms[k].px, terms[k].pz);
          check_walk(nloc, amp_bits, terms[k].px, 0);
          walks += 2;
        }
      }
    }
  // the lists that exercise the rule's edges: all diagonal, exactly kPauliProdT and one more, alternating masks
  for (int amp_bits = 0; amp_bits <= 1; ++amp_bits) {
    for (const int n : {0, 1, qh::kPauliProdT, qh::kPauliProdT + 1, 3 * qh::kPauliProdT}) {
      std::vector<qh_pauli_term> d(n), x(n), alt(n);
      for (int t = 0; t < n; ++t) {
        d[t] = qh_pauli_term{(uint64_t)t, 0, (uint64_t)t, 0, 0};
        x[t] = qh_pauli_term{(uint64_t)t, 1, (uint64_t)t, 0, 0};
        alt[t] = qh_pauli_term{(uint64_t)t, (uint64_t)(1 + t % 2), 0, 0, 0};
      }
      check_runs(d, amp_bits);
      check_runs(x, amp_bits);
      check_runs(alt, amp_bits);
      lists += 3;
      CHECK(qh::pauli_product_cut(alt.data(), n, amp_bits, nullptr, 0) == (uint64_t)n, "alternating masks share a run");
      CHECK(qh::pauli_product_cut(d.data(), n, amp_bits, nullptr, 0) == (uint64_t)(n + qh::kPauliProdT - 1) / qh::kPauliProdT, "diagonal runs");
    }
    // the masks that exercise one part each: the sub-item bit, thread, register index, chunk, top, all
    for (const uint64_t m : {0x1ull, 0x2ull, 0x40ull, 0x100ull, 0x200ull, 0x400ull, 0x800ull, 0x1000ull, 0x2000ull, 0x3fffull, 0x0ull}) {
      check_walk(14, amp_bits, m, m);
      check_walk(14, amp_bits, m, 0x3fffull ^ m);
      check_walk(14, amp_bits, m, 0x3fffull);
      check_walk(14, amp_bits, m | 1ull, 0x3fffull);
      walks += 4;
    }
  }
  CHECK(!qh::pauli_product_main_shape(11, 0) && qh::pauli_product_main_shape(12, 0) && !qh::pauli_product_main_shape(12, 1) &&
            qh::pauli_product_main_shape(13, 1),
        "the threshold between the two kernels moved");
  if (failures) {
    fprintf(stderr, "%d failures\n", failures);
    return 1;
  }
  printf("pauli_product_plan_check: ok (%llu lists, %llu walks)\n", (unsigned long long)lists, (unsigned long long)walks);
  return 0;
}
