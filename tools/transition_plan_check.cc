// transition_plan_check.cc -- stand-alone check of qcc_amd/csrc/transition_plan.h (the host side of qh_transition_pauli),
// for plain and sanitizer builds:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -static-libasan -static-libubsan \
//       tools/transition_plan_check.cc -o transition_plan_check
// For `count` random cases (default 40) of each size from 1 to 13 local bits, with 0 to 2 bits in the shard index, at both
// widths -- random bit maps for a and for b (equal, or different in the local positions), random term lists with repeated x
// masks -- it checks that
//   * every term lands in exactly one pass, the passes tile the sorted list, share one x mask, hold at most the batch of the
//     width and are as many as sum over distinct x masks of ceil(count / batch); equal x masks keep the caller's order;
//   * px maps back to the logical x mask through B's bit map and pz to the local part of the logical z mask through A's;
//     neg is the parity of the z bits the shard index holds at 1; ny is nY mod 4;
//   * for EVERY amplitude pair the planned walk visits (linear, tiles, gather: enumerated the way the kernels do), b's
//     index XOR px is where b keeps logical index (i ^ x), and the sign parts the kernels combine (uniform, register,
//     thread, half) XOR to the parity of (i & z) over the local logical bits;
//   * masks out of range are QH_ERR_BAD_QUBIT, an x bit the shard index holds, different shard indices and a logical bit that
//     only one handle keeps in the shard index are QH_ERR_NONLOCAL, each naming what it should.
// Exit status 0 = all good.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <random>
#include <vector>

#include "../qcc_amd/csrc/transition_plan.h"

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

// physical mask -> logical mask under perm (physical position of each logical bit)
static uint64_t to_logical(int nglob, const int *perm, uint64_t phys) {
  uint64_t l = 0;
  for (int b = 0; b < nglob; ++b)
    if ((phys >> perm[b]) & 1ull) l |= 1ull << b;
  return l;
}
static uint64_t spread(uint64_t v, const uint8_t *pos, int n) {
  uint64_t o = 0;
  for (int k = 0; k < n; ++k) o |= ((v >> k) & 1ull) << pos[k];
  return o;
}

struct Case {
  int nloc, nglob, bw;
  std::vector<int> pa, pb;
  uint64_t shard;
  std::vector<uint64_t> x, z;
};

// the pairs (a's index, b's index of the same logical amplitude) in the order of the walk, with the sign parts of term t
// checked on the way
static void check_walk(const Case &c, const qh_inner_tiles &w, const std::vector<qh_pauli_term> &terms) {
  const int ab = c.bw == 128 ? 0 : 1;
  const uint64_t n = 1ull << c.nloc, local = n - 1;
  std::vector<uint8_t> seen_a(n, 0), seen_b(n, 0);
  auto visit = [&](uint64_t ia, uint64_t ib, const std::vector<uint32_t> &sign) {
    CHECK(ia < n && ib < n, "index out of the shard: %llu %llu", (unsigned long long)ia, (unsigned long long)ib);
    if (ia >= n || ib >= n) return;
    ++seen_a[ia];
    ++seen_b[ib];
    const uint64_t la = to_logical(c.nglob, c.pa.data(), ia), lb = to_logical(c.nglob, c.pb.data(), ib);
    CHECK(la == lb, "the walk pairs logical %llu with %llu", (unsigned long long)la, (unsigned long long)lb);
    for (size_t t = 0; t < terms.size(); ++t) {
      const uint64_t x = c.x[terms[t].index], z = c.z[terms[t].index];
      const uint64_t jb = ib ^ terms[t].px;
      CHECK(jb < n, "partner out of the shard");
      CHECK(to_logical(c.nglob, c.pb.data(), jb) == (la ^ x), "term %zu: partner of logical %llu is not %llu", t, (unsigned long long)la,
            (unsigned long long)(la ^ x));
      const uint64_t zl = z & to_logical(c.nglob, c.pa.data(), local);      // the local logical bits of z
      CHECK(sign[t] == par(la & zl), "term %zu: sign parts give %u at a's index %llu", t, sign[t], (unsigned long long)ia);
    }
  };
  std::vector<uint32_t> sign(terms.size());
  if (w.path == QH_INNER_LINEAR) {
    const int items = c.nloc - ab, cw = std::min(11, items);
    for (uint64_t q = 0; q < (1ull << (items - cw)); ++q)
      for (uint32_t u = 0; u < 8; ++u)
        for (uint32_t tid = 0; tid < 256; ++tid) {
          const uint32_t pos = tid + 256u * u;
          if (pos >= (1u << cw)) continue;
          const uint64_t item = (q << cw) | pos;
          for (uint32_t half = 0; half < (1u << ab); ++half) {
            for (size_t t = 0; t < terms.size(); ++t) {
              const qh::TransZSplit s = qh::transition_split_linear(terms[t].pz, ab);
              sign[t] = par(q & s.uniform) ^ ((s.reg >> u) & 1u) ^ par(tid & s.thread) ^ (s.half & half);
            }
            // b's item is XORed with px >> ab, its halves swapped when px & 1: together, the amplitude index ^ px
            visit((item << ab) | half, (item << ab) | half, sign);
          }
        }
  } else if (w.path == QH_INNER_TILES) {
    for (uint64_t tile = 0; tile < (1ull << w.nrest); ++tile)
      for (uint32_t r = 0; r < 256; ++r) {
        const uint64_t ia = spread(tile, w.rest_a, (int)w.nrest) | spread(r, w.tile_a, 8);
        const uint64_t ib = spread(tile, w.rest_b, (int)w.nrest) | spread(spread(r, w.shuffle, 8), w.tile_b, 8);
        for (size_t t = 0; t < terms.size(); ++t) {
          const qh::TransZSplit s = qh::transition_split_tiles(terms[t].pz, w);
          sign[t] = par(tile & s.uniform) ^ par(r & s.thread);
          CHECK(s.thread < 256 && s.reg == 0 && s.half == 0, "tiles split out of range");
        }
        visit(ia, ib, sign);
      }
  } else {
    for (uint64_t i = 0; i < n; ++i) {
      for (size_t t = 0; t < terms.size(); ++t) sign[t] = par(i & terms[t].pz);
      visit(i, spread(i, w.pos_b, c.nloc), sign);
    }
  }
  for (uint64_t i = 0; i < n; ++i) CHECK(seen_a[i] == 1 && seen_b[i] == 1, "index %llu visited %d / %d times", (unsigned long long)i, seen_a[i], seen_b[i]);
}

static void check_case(const Case &c, bool walk_too) {
  qh_inner_tiles w;
  std::vector<qh_pauli_term> terms;
  std::vector<qh_transition_pass> passes;
  qh::TransitionRefusal why;
  const uint64_t T = c.x.size();
  const int rc = qh::plan_transition(c.nloc, c.nglob, c.bw, c.pa.data(), c.pb.data(), c.shard, c.shard, T, c.x.data(), c.z.data(), &w, &terms,
                                     &passes, &why);
  CHECK(rc == QH_OK && why.kind == qh::TransitionRefusal::kNone, "plan refused a valid case: %d kind %d", rc, (int)why.kind);
  if (rc != QH_OK) return;
  const uint64_t batch = (uint64_t)qh::transition_batch(c.bw), local = (1ull << c.nloc) - 1;
  CHECK(terms.size() == T, "%zu terms of %llu", terms.size(), (unsigned long long)T);
  std::vector<int> hits(T, 0);
  for (const qh_pauli_term &t : terms) {
    CHECK(t.index < T, "index out of range");
    if (t.index >= T) return;
    ++hits[t.index];
    const uint64_t x = c.x[t.index], z = c.z[t.index];
    CHECK(!(t.px & ~local) && !(t.pz & ~local), "masks outside the local bits");
    CHECK(to_logical(c.nglob, c.pb.data(), t.px) == x, "px does not map back to x through b's map");
    const uint64_t zl = to_logical(c.nglob, c.pa.data(), t.pz);
    const uint64_t held = to_logical(c.nglob, c.pa.data(), ~local);      // the logical bits the shard index holds
    CHECK(zl == (z & ~held), "pz does not map back to the local part of z through a's map");
    uint32_t neg = 0;
    for (int l = 0; l < c.nglob; ++l)
      if (((z >> l) & 1ull) && c.pa[l] >= c.nloc) neg ^= (uint32_t)((c.shard >> (c.pa[l] - c.nloc)) & 1ull);
    CHECK(t.neg == neg, "neg %u, want %u", t.neg, neg);
    CHECK(t.ny == ((uint32_t)__builtin_popcountll(x & z) & 3u), "ny");
  }
  for (uint64_t t = 0; t < T; ++t) CHECK(hits[t] == 1, "term %llu appears %d times", (unsigned long long)t, hits[t]);
  for (uint64_t k = 1; k < T; ++k) {
    const uint64_t xl = c.x[terms[k - 1].index], xr = c.x[terms[k].index];
    CHECK(xl < xr || (xl == xr && terms[k - 1].index < terms[k].index), "not stably sorted by x at %llu", (unsigned long long)k);
  }
  std::map<uint64_t, uint64_t> per_x;
  for (uint64_t t = 0; t < T; ++t) ++per_x[c.x[t]];
  uint64_t want_passes = 0;
  for (const auto &kv : per_x) want_passes += (kv.second + batch - 1) / batch;
  CHECK(passes.size() == want_passes, "%zu passes, want %llu", passes.size(), (unsigned long long)want_passes);
  uint64_t next = 0;
  for (const qh_transition_pass &p : passes) {
    CHECK(p.first == next && p.count >= 1 && p.count <= batch && p.first + p.count <= T, "pass [%llu, +%llu)", (unsigned long long)p.first,
          (unsigned long long)p.count);
    if (p.first + p.count > T) return;
    for (uint64_t k = 0; k < p.count; ++k) CHECK(terms[p.first + k].px == p.px, "a pass with two x masks");
    CHECK(p.walk == w.path && p.pad == 0, "pass walk %u, plan %u", p.walk, w.path);
    next = p.first + p.count;
  }
  CHECK(next == T, "the passes end at %llu of %llu", (unsigned long long)next, (unsigned long long)T);
  const bool same = std::equal(c.pa.begin(), c.pa.end(), c.pb.begin());
  CHECK(w.path == (same ? QH_INNER_LINEAR : c.nloc < 8 ? QH_INNER_GATHER : QH_INNER_TILES), "walk %u", w.path);
  if (walk_too) check_walk(c, w, terms);
}

static void check_refusals(const Case &c, std::mt19937_64 &rng) {
  qh_inner_tiles w;
  std::vector<qh_pauli_term> terms{qh_pauli_term{7, 7, 7, 7, 7}};
  std::vector<qh_transition_pass> passes;
  qh::TransitionRefusal why;
  const uint64_t T = c.x.size();
  auto plan = [&](const Case &k, uint64_t shard_b) {
    return qh::plan_transition(k.nloc, k.nglob, k.bw, k.pa.data(), k.pb.data(), k.shard, shard_b, k.x.size(), k.x.data(), k.z.data(), &w, &terms,
                               &passes, &why);
  };
  const uint64_t at = T ? rng() % T : 0;
  if (T && c.nglob < 64) {      // a mask bit out of range, in x or in z
    Case k = c;
    ((rng() & 1) ? k.x : k.z)[at] |= 1ull << c.nglob;
    CHECK(plan(k, k.shard) == QH_ERR_BAD_QUBIT && why.kind == qh::TransitionRefusal::kMaskRange && why.term <= at, "mask range");
  }
  if (c.nglob > c.nloc) {
    CHECK(plan(c, c.shard ^ 1ull) == QH_ERR_NONLOCAL && why.kind == qh::TransitionRefusal::kShardIndex, "another shard index");
    int held = 0;
    while (c.pb[held] < c.nloc) ++held;      // a logical bit the shard index holds
    if (T) {
      Case k = c;
      k.x[at] |= 1ull << held;
      const int rc = plan(k, k.shard);
      CHECK(rc == QH_ERR_NONLOCAL && why.kind == qh::TransitionRefusal::kXHeld && why.term <= at && why.bit >= 0 && k.pb[why.bit] >= k.nloc,
            "x on a shard bit: %d kind %d", rc, (int)why.kind);
      k = c;
      k.z[at] |= 1ull << held;      // z there is only a sign
      CHECK(plan(k, k.shard) == QH_OK, "z on a shard bit refused");
      terms.assign(1, qh_pauli_term{7, 7, 7, 7, 7});
    }
    Case k = c;      // b keeps another logical bit in the shard index
    int loc = 0;
    while (k.pb[loc] >= k.nloc) ++loc;
    std::swap(k.pb[loc], k.pb[held]);
    CHECK(plan(k, k.shard) == QH_ERR_NONLOCAL && why.kind == qh::TransitionRefusal::kSplitBit && (why.bit == loc || why.bit == held), "split bit");
  }
  CHECK(terms.size() == 1 && terms[0].index == 7, "a refused plan wrote terms");
}

int main(int argc, char **argv) {
  const int count = argc > 1 ? atoi(argv[1]) : 40;
  std::mt19937_64 rng(119);
  long cases = 0;
  for (int nloc = 1; nloc <= 13; ++nloc)
    for (int bw : {128, 64})
      for (int k = 0; k < count; ++k) {
        Case c;
        c.nloc = nloc;
        c.nglob = nloc + (int)(rng() % 3);
        c.bw = bw;
        c.shard = c.nglob > nloc ? rng() % (1ull << (c.nglob - nloc)) : 0;
        // a's map: any permutation of the positions; b's: the same, with the local positions shuffled again (or not)
        std::vector<int> pos(c.nglob);
        for (int p = 0; p < c.nglob; ++p) pos[p] = p;
        std::shuffle(pos.begin(), pos.end(), rng);
        c.pa = pos;
        c.pb = pos;
        if (k % 3) {
          std::vector<int> locals;
          for (int l = 0; l < c.nglob; ++l)
            if (c.pb[l] < nloc) locals.push_back(l);
          std::vector<int> where;
          for (int l : locals) where.push_back(c.pb[l]);
          std::shuffle(where.begin(), where.end(), rng);
          for (size_t j = 0; j < locals.size(); ++j) c.pb[locals[j]] = where[j];
        }
        uint64_t xlocal = 0;      // the logical bits x may use: the local ones
        for (int l = 0; l < c.nglob; ++l)
          if (c.pb[l] < nloc) xlocal |= 1ull << l;
        const uint64_t all = (1ull << c.nglob) - 1;
        const int nx = 1 + (int)(rng() % 5), T = (int)(rng() % 45);
        std::vector<uint64_t> xs(nx);
        for (uint64_t &x : xs) x = (rng() & xlocal) & ((rng() & 1) ? all : rng());
        for (int t = 0; t < T; ++t) {
          c.x.push_back(xs[rng() % nx]);
          c.z.push_back((rng() & all) & ((rng() & 3) ? all : rng()));
        }
        Case walk = c;      // the walk check costs 2^nloc x T: on a few of the terms
        if (walk.x.size() > 6) {
          walk.x.resize(6);
          walk.z.resize(6);
        }
        check_case(c, false);
        check_case(walk, true);
        check_refusals(c, rng);
        ++cases;
      }
  if (failures) {
    fprintf(stderr, "%d failures\n", failures);
    return 1;
  }
  printf("transition_plan_check: %ld cases ok\n", cases);
  return 0;
}
