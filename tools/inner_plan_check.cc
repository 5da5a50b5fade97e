// inner_plan_check.cc -- stand-alone check of qcc_amd/csrc/inner_plan.h (the host side of qh_inner), for sanitizer builds:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -static-libasan -static-libubsan \
//       tools/inner_plan_check.cc -o inner_plan_check
// (the sanitizer runtimes linked statically: the program then runs as it is, in any environment).
// For hand-made bit maps and `count` random pairs of permutations per size (8..14 local bits, default 200) it walks the
// tiles as k_two_tiles does and checks that the (a index, b index) pairs cover every index of both states exactly once
// and are the pairs the bit maps define; then shard bits that differ must be reported.  Exit status 0 = all good.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <random>
#include <vector>

#include "../qcc_amd/csrc/inner_plan.h"

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

static uint64_t spread(uint64_t v, const int *perm, int n) {      // logical index -> physical
  uint64_t o = 0;
  for (int l = 0; l < n; ++l) o |= ((v >> l) & 1ull) << perm[l];
  return o;
}

static void check_pair(int nloc, const std::vector<int> &pa, const std::vector<int> &pb) {
  qh_inner_tiles t;
  const int bad = qh::plan_inner(nloc, nloc, pa.data(), pb.data(), &t);
  CHECK(bad == -1, "nloc %d: plan refused local maps (bit %d)", nloc, bad);
  if (bad != -1) return;
  const uint64_t n = 1ull << nloc;
  std::vector<uint64_t> want(n);      // b's index of a's index
  for (uint64_t l = 0; l < n; ++l) want[spread(l, pa.data(), nloc)] = spread(l, pb.data(), nloc);
  if (pa == pb) {
    CHECK(t.path == QH_INNER_LINEAR, "nloc %d: equal maps not linear", nloc);
    return;
  }
  if (nloc < qh::kInnerTileBits) {
    CHECK(t.path == QH_INNER_GATHER, "nloc %d: small register not gathered", nloc);
    for (uint64_t i = 0; i < n; ++i) {
      uint64_t j = 0;
      for (int p = 0; p < nloc; ++p) j |= ((i >> p) & 1ull) << t.pos_b[p];
      CHECK(j == want[i], "nloc %d: gather pairs %llu with %llu", nloc, (unsigned long long)i, (unsigned long long)j);
    }
    return;
  }
  CHECK(t.path == QH_INNER_TILES && (int)t.nrest == nloc - 8, "nloc %d: path %u nrest %u", nloc, t.path, t.nrest);
  CHECK(__builtin_popcountll(t.free_a) == 8 && __builtin_popcountll(t.free_b) == 8 && (t.free_a & 15) == 15 && (t.free_b & 15) == 15,
        "nloc %d: free bits %llx %llx", nloc, (unsigned long long)t.free_a, (unsigned long long)t.free_b);
  for (int k = 0; k < 4; ++k) CHECK(t.tile_a[k] == k && t.tile_b[k] == k, "nloc %d: runs shorter than 16", nloc);
  std::vector<uint8_t> seen_a(n, 0), seen_b(n, 0);
  for (uint64_t tile = 0; tile < (1ull << t.nrest); ++tile) {
    uint64_t ba = 0, bb = 0;
    for (uint32_t k = 0; k < t.nrest; ++k) {
      ba |= ((tile >> k) & 1ull) << t.rest_a[k];
      bb |= ((tile >> k) & 1ull) << t.rest_b[k];
    }
    uint64_t slot_b[256];      // b's enumeration: what thread r loads into LDS slot r
    for (unsigned r = 0; r < 256; ++r) {
      uint64_t db = 0;
      for (int k = 0; k < 8; ++k) db |= (uint64_t)((r >> k) & 1u) << t.tile_b[k];
      slot_b[r] = bb | db;
    }
    for (unsigned r = 0; r < 256; ++r) {
      uint64_t da = 0;
      unsigned slot = 0;
      for (int k = 0; k < 8; ++k) {
        da |= (uint64_t)((r >> k) & 1u) << t.tile_a[k];
        slot |= ((r >> k) & 1u) << t.shuffle[k];
      }
      const uint64_t ia = ba | da, ib = slot_b[slot];
      CHECK(ia < n && ib < n, "nloc %d: index out of range", nloc);
      if (ia >= n || ib >= n) return;
      CHECK(want[ia] == ib, "nloc %d: a %llu paired with b %llu, want %llu", nloc, (unsigned long long)ia, (unsigned long long)ib,
            (unsigned long long)want[ia]);
      ++seen_a[ia];
      ++seen_b[ib];
    }
  }
  for (uint64_t i = 0; i < n; ++i) CHECK(seen_a[i] == 1 && seen_b[i] == 1, "nloc %d: index %llu covered %d / %d times", nloc,
                                         (unsigned long long)i, seen_a[i], seen_b[i]);
}

static std::vector<int> identity(int n) {
  std::vector<int> p(n);
  std::iota(p.begin(), p.end(), 0);
  return p;
}
// the map qh_remap_swap(x, y) leaves: the logical bits at positions x and y trade places
static void swap_pos(std::vector<int> &perm, int x, int y) {
  int lx = -1, ly = -1;
  for (size_t l = 0; l < perm.size(); ++l) {
    if (perm[l] == x) lx = (int)l;
    if (perm[l] == y) ly = (int)l;
  }
  std::swap(perm[lx], perm[ly]);
}

int main(int argc, char **argv) {
  const int count = argc > 1 ? atoi(argv[1]) : 200;
  for (int nloc : {4, 7, 8, 9, 12, 16}) {
    const std::vector<int> id = identity(nloc);
    check_pair(nloc, id, id);
    std::vector<int> p = id;      // low bits 0..3 <-> the top four
    for (int k = 0; k < 4 && nloc - 4 + k > k; ++k) swap_pos(p, k, nloc - 4 + k);
    check_pair(nloc, id, p);
    check_pair(nloc, p, id);
    p = id;                       // bits 0, 1 <-> two high bits
    swap_pos(p, 0, nloc - 1);
    swap_pos(p, 1, nloc - 2);
    check_pair(nloc, id, p);
    p = id;                       // inside bits 0..3
    swap_pos(p, 0, 3);
    swap_pos(p, 1, 2);
    swap_pos(p, 0, 1);
    check_pair(nloc, id, p);
    std::vector<int> rev(nloc);   // full bit reversal
    for (int l = 0; l < nloc; ++l) rev[l] = nloc - 1 - l;
    check_pair(nloc, id, rev);
    check_pair(nloc, p, rev);     // both sides permuted, differently
  }
  std::mt19937_64 rng(20240607);
  for (int nloc = 8; nloc <= 14; ++nloc)
    for (int c = 0; c < count; ++c) {
      std::vector<int> pa = identity(nloc), pb = identity(nloc);
      std::shuffle(pa.begin(), pa.end(), rng);
      std::shuffle(pb.begin(), pb.end(), rng);
      check_pair(nloc, pa, pb);
    }
  {   // shard bits: the same bit at the same place is fine, anything else is reported by its logical bit
    qh_inner_tiles t;
    std::vector<int> pa = identity(12), pb = identity(12);
    swap_pos(pb, 2, 7);
    CHECK(qh::plan_inner(10, 12, pa.data(), pb.data(), &t) == -1 && t.path == QH_INNER_TILES, "shard bits in place refused");
    swap_pos(pb, 3, 11);
    CHECK(qh::plan_inner(10, 12, pa.data(), pb.data(), &t) == 3, "a shard bit held by one side only was not reported");
    pb = identity(12);
    swap_pos(pb, 10, 11);
    CHECK(qh::plan_inner(10, 12, pa.data(), pb.data(), &t) == 10, "shard bits at different shard positions were not reported");
  }
  if (failures) {
    fprintf(stderr, "%d failures\n", failures);
    return 1;
  }
  printf("inner_plan_check: ok\n");
  return 0;
}
