// zpoly_plan_check.cc -- stand-alone check of qcc_amd/csrc/zpoly_plan.h (the host side of qh_apply_zpoly and
// qh_expect_zpoly), for sanitizer builds:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -static-libasan -static-libubsan \
//       tools/zpoly_plan_check.cc -o zpoly_plan_check
// (the sanitizer runtimes linked statically: the program then runs as it is, in any environment).
// For `count` random term lists (default 12) of each size from 1 to 14 local bits, at both widths, it checks that
//   * the classes partition the terms: every term has exactly one class, the counts add up, a class agrees with where the
//     mask's bits lie, and the groups are the distinct low masks of the straddling terms in order of first appearance;
//   * the device block is laid out inside its arrays (every offset and every segment bound) and within kZpolyBlockBytes;
//   * at EVERY amplitude index of the state, f rebuilt from the block's parts the way the kernels rebuild it
//     (zpoly_eval_block) equals the direct popcount sum.  Weights are small integers, so both sums are exact;
//   * the grid covers every item exactly once (main shape: blocks x chunks x register index x thread; below it: one
//     amplitude per thread).
// Lists are drawn with masks of weight 0-4 (constants and duplicates among them), with masks confined to each part of the
// index, and with up to QH_ZPOLY_MAX_TERMS terms.  Exit status 0 = all good.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../qcc_amd/csrc/zpoly_plan.h"

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

static uint32_t par(uint64_t v) { return (uint32_t)(__builtin_popcountll(v) & 1); }

static void check_list(int nloc, int ab, const std::vector<qh::ZpolyTerm> &terms) {
  qh::ZpolyPlan p;
  qh::zpoly_plan(terms.data(), terms.size(), nloc, ab, &p);
  const uint64_t n = 1ull << nloc, T = terms.size();
  CHECK(p.bytes() <= qh::kZpolyBlockBytes, "block of %zu bytes", p.bytes());
  CHECK(p.main == qh::pauli_main_shape(nloc, ab), "shape");
  CHECK(p.low_bits == (p.main ? qh::kPauliChunkBits + ab : nloc), "low_bits %d", p.low_bits);
  // classes
  CHECK(p.cls.size() == T && p.nconst + p.nhigh + p.nlow + p.nstraddle == T, "the classes do not partition %llu terms", (unsigned long long)T);
  const uint64_t lowm = (1ull << p.low_bits) - 1ull;
  uint64_t cnt[4] = {0, 0, 0, 0};
  std::vector<uint64_t> groups;
  for (uint64_t t = 0; t < T; ++t) {
    const uint64_t pz = terms[t].pz, lo = pz & lowm, hi = pz >> p.low_bits;
    const uint32_t want = pz == 0 ? QH_ZPOLY_CONST : (hi && lo) ? QH_ZPOLY_STRADDLE : hi ? QH_ZPOLY_HIGH : QH_ZPOLY_LOW;
    CHECK(p.cls[t] == want, "term %llu (pz 0x%llx): class %u, want %u", (unsigned long long)t, (unsigned long long)pz, p.cls[t], want);
    if (p.cls[t] < 4) ++cnt[p.cls[t]];
    if (want == QH_ZPOLY_STRADDLE) {
      bool known = false;
      for (uint64_t g : groups) known |= g == lo;
      if (!known) groups.push_back(lo);
    }
  }
  CHECK(cnt[0] == p.nconst && cnt[1] == p.nhigh && cnt[2] == p.nlow && cnt[3] == p.nstraddle, "class counts");
  CHECK(groups == p.group_mask, "groups");
  if (!p.main) CHECK(p.nhigh == 0 && p.nstraddle == 0 && p.group_mask.empty(), "a small state has no chunk part");
  // the block
  if (p.main) {
    CHECK(p.nseg == p.group_mask.size() + 1 && p.nseg_terms == p.nconst + p.nhigh + p.nstraddle, "segments");
    // the segments' low masks: every group once; thread-only masks first, then register-index / half only, then mixed
    CHECK(1 + p.ngt + p.ngu <= p.nseg, "group kinds");
    const uint64_t tb = 255ull << ab;
    std::vector<uint64_t> dealt;
    for (uint32_t s = 1; s < p.nseg; ++s) {
      const uint64_t lm = p.md[p.off_gl + s];
      dealt.push_back(lm);
      const int kind = (lm & ~tb) == 0 ? 0 : (lm & tb) == 0 ? 1 : 2;
      CHECK(kind == (s < 1 + p.ngt ? 0 : s < 1 + p.ngt + p.ngu ? 1 : 2), "segment %u: low mask 0x%llx among the wrong kind", s, (unsigned long long)lm);
    }
    std::vector<uint64_t> a = dealt, b = p.group_mask;
    std::sort(a.begin(), a.end());
    std::sort(b.begin(), b.end());
    CHECK(a == b, "the segments' low masks are not the groups'");
    CHECK(p.wd.size() == (size_t)p.nseg_terms + p.nlow && p.off_lw == p.nseg_terms, "wd");
    CHECK(p.off_sc == p.nseg + 1 && p.off_gl == p.off_sc + p.nseg_terms && p.off_lm == p.off_gl + p.nseg && p.md.size() == (size_t)p.off_lm + p.nlow,
          "md");
    CHECK(p.md[0] == 0 && p.md[p.nseg] == p.nseg_terms, "segment bounds");
    for (uint32_t s = 0; s < p.nseg; ++s) CHECK(p.md[s] <= p.md[s + 1] && (s == 0 || p.md[s] < p.md[s + 1]), "segment %u", s);
    for (uint32_t j = 0; j < p.nseg_terms; ++j) CHECK((p.md[p.off_sc + j] >> (nloc - p.low_bits)) == 0, "chunk mask %u", j);
    for (uint64_t j = 0; j < p.nlow; ++j) CHECK((p.md[p.off_lm + j] & ~lowm) == 0, "low mask");
  } else {
    CHECK(p.wd.size() == T && p.md.size() == T, "small block");
  }
  // f at every amplitude
  for (uint64_t i = 0; i < n; ++i) {
    double want = 0.0;
    for (uint64_t t = 0; t < T; ++t) want += par(i & terms[t].pz) ? -terms[t].w : terms[t].w;
    const double got = qh::zpoly_eval_block(p, i);
    if (got != want) {
      CHECK(false, "nloc %d amp_bits %d index %llu: f = %g, want %g", nloc, ab, (unsigned long long)i, got, want);
      break;
    }
  }
  // the grid
  std::vector<uint8_t> seen(n >> (p.main ? ab : 0), 0);
  if (p.main) {
    const qh::PauliGrid g = qh::pauli_grid(nloc, ab);
    CHECK(g.nblk == p.nblk && g.cpb == p.cpb && g.nblk <= qh::kPauliBlocks, "grid");
    for (uint64_t b = 0; b < p.nblk; ++b)
      for (uint64_t q = b * p.cpb; q < (b + 1) * p.cpb; ++q)
        for (uint32_t u = 0; u < (uint32_t)qh::kPauliPer; ++u)
          for (uint32_t t = 0; t < 256; ++t) {
            const uint64_t item = qh::pauli_item(q, u, t);
            if (item >= seen.size()) {
              CHECK(false, "item %llu outside the state", (unsigned long long)item);
              return;
            }
            ++seen[item];
          }
  } else {
    for (uint64_t b = 0; b < p.nblk; ++b)
      for (uint32_t t = 0; t < 256; ++t)
        if (b * 256 + t < n) ++seen[b * 256 + t];
  }
  for (size_t k = 0; k < seen.size(); ++k)
    if (seen[k] != 1) {
      CHECK(false, "nloc %d amp_bits %d: item %zu visited %d times", nloc, ab, k, (int)seen[k]);
      break;
    }
}

int main(int argc, char **argv) {
  const int count = argc > 1 ? atoi(argv[1]) : 12;
  std::mt19937_64 rng(118);
  int lists = 0;
  for (int ab = 0; ab <= 1; ++ab)
    for (int nloc = 1; nloc <= 14; ++nloc) {
      const uint64_t all = (1ull << nloc) - 1ull;
      const int lowb = qh::pauli_main_shape(nloc, ab) ? qh::kPauliChunkBits + ab : nloc;
      const uint64_t lowm = (1ull << lowb) - 1ull;
      for (int rep = 0; rep < count; ++rep) {
        // sizes: a few terms, a few dozen, and (once per size) the most
        uint64_t T = rep % 3 == 0 ? 1 + rng() % 6 : 1 + rng() % 60;
        if (rep == 1) T = QH_ZPOLY_MAX_TERMS;
        std::vector<qh::ZpolyTerm> terms(T);
        for (auto &tm : terms) {
          uint64_t pz = 0;
          const int weight = (int)(rng() % 5);
          for (int k = 0; k < weight; ++k) pz |= 1ull << (rng() % nloc);
          const int where = (int)(rng() % 4);      // anywhere, low only, high only, anywhere
          if (where == 1) pz &= lowm;
          if (where == 2) pz &= ~lowm & all;
          tm.pz = pz;
          tm.w = (double)((int)(rng() % 17) - 8);
        }
        if (T > 3) terms[T - 1] = terms[0], terms[1].pz = 0;      // a duplicate and a constant
        check_list(nloc, ab, terms);
        ++lists;
      }
    }
  // no terms at all
  check_list(5, 0, {});
  check_list(13, 1, {});
  if (failures) {
    fprintf(stderr, "%d failures\n", failures);
    return 1;
  }
  printf("ok: %d term lists, 1 to 14 local bits, both widths\n", lists);
  return 0;
}
