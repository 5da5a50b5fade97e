// resize_plan_check.cc -- stand-alone check of qcc_amd/csrc/resize_plan.h (the host side of qh_extend / qh_release), for
// sanitizer builds:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -static-libasan -static-libubsan \
//       tools/resize_plan_check.cc -o resize_plan_check
// (the sanitizer runtimes linked statically: the program then runs as it is, in any environment).
// For 1..10 local bits with 0..3 bits in the shard index, under the identity and shuffled bit maps (local <-> local and
// local <-> shard), it compares with a bit-by-bit model
//   * qh_release, for EVERY subset of local logical bits that leaves one: the new bit map, the predicate (R, V) and the
//     segment squeeze of every local source index; and end to end, that the amplitude of logical index L of the source lands
//     at the logical index of the result that L has with the listed bits struck out;
//   * qh_extend for k = 1, 2, 5, 16: that amplitude (L, j) of src (x) f sits where new[(j << nloc) | p] puts it.
// Exit status 0 = all good.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <random>
#include <vector>

#include "../qcc_amd/csrc/resize_plan.h"

static int failures = 0;
#define CHECK(cond, ...)                  \
  do {                                    \
    if (!(cond)) {                        \
      if (++failures < 20) {              \
        fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); \
        fprintf(stderr, __VA_ARGS__);     \
        fputc('\n', stderr);              \
      }                                   \
    }                                     \
  } while (0)

static uint64_t spread(uint64_t v, const int *perm, int n) {      // logical index -> physical
  uint64_t o = 0;
  for (int l = 0; l < n; ++l) o |= ((v >> l) & 1ull) << perm[l];
  return o;
}

// the model of a squeeze: the bits of p at the positions not in `drop`, ascending, packed
static uint64_t strike(uint64_t p, uint64_t drop, int n) {
  uint64_t o = 0;
  int at = 0;
  for (int b = 0; b < n; ++b)
    if (!((drop >> b) & 1ull)) o |= ((p >> b) & 1ull) << at++;
  return o;
}

static void check_release(int nloc, int nglob, const std::vector<int> &perm, uint64_t listed, bool reversed, std::mt19937_64 &rng) {
  std::vector<int32_t> bits;
  for (int l = 0; l < nglob; ++l)
    if ((listed >> l) & 1ull) bits.push_back(l);
  if (reversed) std::reverse(bits.begin(), bits.end());
  const int k = (int)bits.size();
  const uint64_t value = rng() & ((1ull << k) - 1ull);
  qh::ReleasePlan pl;
  const int held = qh::plan_release(nloc, nglob, perm.data(), k, bits.data(), value, &pl);
  int first_held = -1;
  for (int j = 0; j < k && first_held < 0; ++j)
    if (perm[bits[j]] >= nloc) first_held = j;
  CHECK(held == first_held, "nloc %d of %d: listed %llx: held bit %d, want %d", nloc, nglob, (unsigned long long)listed, held, first_held);
  if (held >= 0 || first_held >= 0) return;
  // the model, bit by bit
  uint64_t drop = 0, want = 0, lwant = 0;
  for (int j = 0; j < k; ++j) {
    drop |= 1ull << perm[bits[j]];
    if ((value >> j) & 1ull) {
      want |= 1ull << perm[bits[j]];
      lwant |= 1ull << bits[j];
    }
  }
  CHECK(pl.drop == drop && pl.want == want, "nloc %d: R/V %llx/%llx, want %llx/%llx", nloc, (unsigned long long)pl.drop,
        (unsigned long long)pl.want, (unsigned long long)drop, (unsigned long long)want);
  CHECK(pl.nseg >= 1 && pl.nseg <= k + 1, "nloc %d: %d runs for k = %d", nloc, pl.nseg, k);
  uint64_t covered = 0;
  for (int s = 0; s < pl.nseg; ++s) {
    CHECK(!(covered & pl.mask[s]) && !(pl.mask[s] & drop), "nloc %d: run %d overlaps", nloc, s);
    covered |= pl.mask[s];
  }
  CHECK(covered == (((1ull << nloc) - 1ull) & ~drop), "nloc %d: runs cover %llx", nloc, (unsigned long long)covered);
  for (uint64_t p = 0; p < (1ull << nloc); ++p)
    CHECK(qh::release_squeeze(pl, p) == strike(p, drop, nloc), "nloc %d: R %llx: %llx squeezed to %llx", nloc, (unsigned long long)drop,
          (unsigned long long)p, (unsigned long long)qh::release_squeeze(pl, p));
  // the new map: the surviving logical bits in order, each at the rank of its position among the surviving positions
  int nl = 0;
  for (int l = 0; l < nglob; ++l) {
    if ((listed >> l) & 1ull) continue;
    const int rank = perm[l] - __builtin_popcountll(drop & ((1ull << perm[l]) - 1ull));
    CHECK(pl.perm[nl] == rank, "nloc %d: new logical bit %d at %d, want %d", nloc, nl, pl.perm[nl], rank);
    ++nl;
  }
  for (int b = nl; b < 64; ++b) CHECK(pl.perm[b] == b, "nloc %d: map entry %d above the new size is %d", nloc, b, pl.perm[b]);
  // end to end over every logical index of the source (all shards)
  for (uint64_t L = 0; L < (1ull << nglob); ++L) {
    const uint64_t P = spread(L, perm.data(), nglob), loc = P & ((1ull << nloc) - 1ull), shard = P >> nloc;
    const bool kept = (L & listed) == lwant;
    CHECK(kept == ((loc & pl.drop) == pl.want), "nloc %d: logical %llx kept %d by the model", nloc, (unsigned long long)L, (int)kept);
    if (!kept) continue;
    const uint64_t L2 = strike(L, listed, nglob), P2 = spread(L2, pl.perm, nglob - k);
    CHECK(P2 == ((shard << (nloc - k)) | qh::release_squeeze(pl, loc)), "nloc %d of %d: logical %llx -> %llx lands at %llx", nloc, nglob,
          (unsigned long long)L, (unsigned long long)L2, (unsigned long long)P2);
  }
}

static void check_extend(int nloc, int nglob, const std::vector<int> &perm, int k, std::mt19937_64 &rng) {
  int out[64];
  qh::plan_extend(nloc, nglob, perm.data(), k, out);
  std::vector<int> seen(nglob + k, 0);
  for (int b = 0; b < nglob + k; ++b) {
    CHECK(out[b] >= 0 && out[b] < nglob + k, "extend nloc %d k %d: bit %d at %d", nloc, k, b, out[b]);
    if (out[b] >= 0 && out[b] < nglob + k) ++seen[out[b]];
  }
  for (int b = 0; b < nglob + k; ++b) CHECK(seen[b] == 1, "extend nloc %d k %d: position %d used %d times", nloc, k, b, seen[b]);
  for (int b = nglob + k; b < 64; ++b) CHECK(out[b] == b, "extend: map entry %d above the new size is %d", b, out[b]);
  const uint64_t nL = 1ull << nglob, nj = 1ull << k;
  for (int c = 0; c < 4096; ++c) {      // (every pair where there are few)
    const bool all = nL * nj <= 4096;
    const uint64_t L = all ? (uint64_t)c / nj : rng() % nL, j = all ? (uint64_t)c % nj : rng() % nj;
    if (all && (uint64_t)c >= nL * nj) break;
    const uint64_t P = spread(L, perm.data(), nglob), loc = P & ((1ull << nloc) - 1ull), shard = P >> nloc;
    const uint64_t P2 = spread((L << k) | j, out, nglob + k);
    CHECK(P2 == ((shard << (nloc + k)) | (j << nloc) | loc), "extend nloc %d of %d k %d: (%llx, %llx) lands at %llx", nloc, nglob, k,
          (unsigned long long)L, (unsigned long long)j, (unsigned long long)P2);
  }
}

int main() {
  std::mt19937_64 rng(20241018);
  long cases = 0;
  for (int nloc = 1; nloc <= 10; ++nloc)
    for (int g = 0; g <= 3; ++g) {
      const int nglob = nloc + g;
      std::vector<std::vector<int>> maps;
      std::vector<int> id(nglob);
      std::iota(id.begin(), id.end(), 0);
      maps.push_back(id);
      std::vector<int> p = id;
      std::reverse(p.begin(), p.begin() + nloc);      // the local positions reversed
      maps.push_back(p);
      p = id;
      std::shuffle(p.begin(), p.end(), rng);          // local <-> local and local <-> shard
      maps.push_back(p);
      for (const auto &perm : maps) {
        for (int k : {1, 2, 5, 16}) check_extend(nloc, nglob, perm, k, rng);
        uint64_t local_logical = 0;
        for (int l = 0; l < nglob; ++l)
          if (perm[l] < nloc) local_logical |= 1ull << l;
        // every non-empty subset of the local logical bits that leaves one
        for (uint64_t sub = local_logical; sub; sub = (sub - 1) & local_logical) {
          if (__builtin_popcountll(sub) >= nloc) continue;
          check_release(nloc, nglob, perm, sub, (sub & 1ull) != 0, rng);
          ++cases;
        }
        // a listed bit the shard index holds is reported by its place in the list
        for (int l = 0; l < nglob; ++l)
          if (perm[l] >= nloc && nloc > 1) check_release(nloc, nglob, perm, (1ull << l) | (local_logical & (~local_logical + 1ull)), false, rng);
      }
    }
  if (failures) {
    fprintf(stderr, "%d failures\n", failures);
    return 1;
  }
  printf("resize_plan_check: ok (%ld releases)\n", cases);
  return 0;
}
