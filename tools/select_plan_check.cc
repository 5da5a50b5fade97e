// select_plan_check.cc -- qcc_amd/csrc/select_plan.h stand-alone: the radix select of qh_topk driven by histograms computed
// here from synthetic key sets, its chosen key ranges checked against a sort.  Plain host C++ (build with
// -fsanitize=address,undefined); prints "ok" and exits 0, or says what is wrong and exits 1.
//
//   select_plan_check [rounds]
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <random>
#include <string>
#include <vector>

#include "../qcc_amd/csrc/select_plan.h"

namespace {

uint64_t key_of(double p) {
  uint64_t k;
  memcpy(&k, &p, 8);
  return k;
}

int g_bad = 0;
void expect(bool ok, const std::string &what) {
  if (!ok) {
    printf("FAIL: %s\n", what.c_str());
    ++g_bad;
  }
}

// what k_key_hist counts: the nonzero keys under the plan's prefix, by the level's field
std::vector<uint64_t> histogram(const std::vector<uint64_t> &keys, const qh::SelPlan &pl) {
  const int bits = qh::sel_bits(pl.level), shift = qh::sel_shift(pl.level);
  std::vector<uint64_t> h((size_t)1 << bits, 0);
  for (uint64_t k : keys)
    if (k != 0 && ((k >> shift) >> bits) == pl.prefix) h[(k >> shift) & ((1ull << bits) - 1)]++;
  return h;
}

// runs the plan to its end; returns the number of histogram passes
int run(const std::string &name, const std::vector<uint64_t> &keys, uint64_t k, uint64_t cap, qh::SelNext want_end, int max_passes) {
  std::vector<uint64_t> sorted;
  for (uint64_t x : keys)
    if (x) sorted.push_back(x);
  std::sort(sorted.begin(), sorted.end(), std::greater<uint64_t>());
  qh::SelPlan pl = qh::sel_begin(k, cap);
  qh::SelStep st{};
  int passes = 0;
  do {
    const std::vector<uint64_t> h = histogram(keys, pl);
    st = qh::sel_step(pl, h.data());
    ++passes;
    if (passes > qh::kSelLevels) break;
  } while (st.next == qh::kSelRefine);
  expect(passes <= qh::kSelLevels, name + ": more histogram passes than levels");
  expect(passes <= max_passes, name + ": " + std::to_string(passes) + " histogram passes, expected at most " + std::to_string(max_passes));
  expect(st.next == want_end, name + ": ended with " + std::to_string((int)st.next) + ", expected " + std::to_string((int)want_end));
  if (sorted.empty()) {
    expect(st.next == qh::kSelEmpty, name + ": no nonzero key must end empty");
    return passes;
  }
  const uint64_t m = std::min<uint64_t>(k, sorted.size());
  const uint64_t kth = sorted[m - 1];
  auto count_ge = [&](uint64_t lo) { return (uint64_t)(std::upper_bound(sorted.begin(), sorted.end(), lo, std::greater<uint64_t>()) - sorted.begin()); };
  if (st.next == qh::kSelCollect) {
    expect(st.key_lo <= kth, name + ": the k-th key lies under the collected range");
    expect(st.candidates == count_ge(st.key_lo), name + ": candidates differ from the keys at or above key_lo");
    expect(st.candidates <= cap && st.candidates >= m, name + ": candidates outside [min(k, support), cap]");
  } else if (st.next == qh::kSelTies) {
    expect(st.key_lo == kth, name + ": the tied value is not the k-th key");
    const uint64_t above = st.key_lo == ~0ull ? 0 : count_ge(st.key_lo + 1);
    expect(st.candidates == above, name + ": candidates differ from the keys above the tied value");
    expect(st.ties_total == count_ge(st.key_lo) - above, name + ": ties_total");
    expect(st.ties_needed == m - above && st.ties_needed >= 1 && st.ties_needed <= st.ties_total, name + ": ties_needed");
    expect(st.candidates + st.ties_total > cap, name + ": a tie scan although the candidates fit");
  } else {
    expect(false, name + ": unexpected end state");
  }
  return passes;
}

}  // namespace

int main(int argc, char **argv) {
  const int rounds = argc > 1 ? atoi(argv[1]) : 20;
  const uint64_t cap = 4096;
  // the level geometry: 63 key bits, contiguous fields, bin edges that nest
  int total_bits = 0;
  for (int l = 0; l < qh::kSelLevels; ++l) {
    total_bits += qh::sel_bits(l);
    expect(qh::sel_shift(l) + qh::sel_bits(l) == (l ? qh::sel_shift(l - 1) : 63), "level fields are not contiguous");
  }
  expect(total_bits == 63 && qh::sel_shift(qh::kSelLevels - 1) == 0, "levels do not cover 63 bits");
  expect(qh::sel_bin_lo(0, 0, 1) == (1ull << 51) && qh::sel_bin_hi(0, 0, 0) == (1ull << 51) - 1, "level-0 bin edges");
  expect(qh::sel_bin_lo(qh::kSelLevels - 1, 5, 3) == qh::sel_bin_hi(qh::kSelLevels - 1, 5, 3), "a last-level bin is one value");

  std::mt19937_64 rng(12345);
  std::uniform_real_distribution<double> uni(0.0, 1.0);

  {   // peaked: a few large keys over a small background -> one histogram, a handful of candidates
    std::vector<uint64_t> keys(1 << 16);
    for (auto &x : keys) x = key_of(1e-9 * uni(rng));
    for (int j = 0; j < 20; ++j) keys[997 * j] = key_of(0.01 + 0.001 * j);
    run("peaked k=16", keys, 16, cap, qh::kSelCollect, 1);
    run("peaked k=1", keys, 1, cap, qh::kSelCollect, 1);
  }
  {   // flat: all mass in one bin, one value -> six histograms, then the tie scan takes k of them
    std::vector<uint64_t> keys(1 << 16, key_of(1.0 / 65536));
    run("flat k=16", keys, 16, cap, qh::kSelTies, qh::kSelLevels);
    run("flat k=4096", keys, 4096, cap, qh::kSelTies, qh::kSelLevels);
    keys[5] = key_of(0.5);
    keys[9] = key_of(0.25);
    run("flat + 2 above, k=3", keys, 3, cap, qh::kSelTies, qh::kSelLevels);
    run("flat + 2 above, k=2", keys, 2, cap, qh::kSelCollect, 1);
    std::vector<uint64_t> few(1 << 12, key_of(0.125));
    run("flat that fits", few, 7, cap, qh::kSelCollect, 1);
  }
  {   // k at a bin edge: exactly k keys in the bins above the boundary, and one more
    std::vector<uint64_t> keys;
    for (int j = 0; j < 100; ++j) keys.push_back(key_of(0.5 + 0.001 * j));       // bin of [0.5, 0.75)
    for (int j = 0; j < 10000; ++j) keys.push_back(key_of(0.25 + 1e-5 * j));      // bin of [0.25, 0.375)
    run("edge k=100", keys, 100, cap, qh::kSelCollect, 1);
    run("edge k=101", keys, 101, cap, qh::kSelCollect, 2);
    run("edge k=4096", keys, 4096, cap, qh::kSelCollect, 3);
  }
  {   // k larger than the support, zeros never counted
    std::vector<uint64_t> keys(1 << 12, 0);
    run("all zero", keys, 5, cap, qh::kSelEmpty, 1);
    keys[3] = key_of(0.5);
    keys[77] = key_of(0.5);
    keys[78] = key_of(1e-300);
    run("support 3, k=16", keys, 16, cap, qh::kSelCollect, 1);
    run("support 3, k=3", keys, 3, cap, qh::kSelCollect, 1);
  }
  {   // subnormal and extreme keys
    std::vector<uint64_t> keys(10000);
    for (size_t j = 0; j < keys.size(); ++j) keys[j] = 1 + j % 5000;      // the smallest subnormals, each twice
    run("subnormals k=10", keys, 10, cap, qh::kSelCollect, qh::kSelLevels);
    keys.push_back(qh::kSelKeyInf);
    run("with inf k=1", keys, 1, cap, qh::kSelCollect, 1);
  }
  for (int r = 0; r < rounds; ++r) {   // random mixtures: exponential weights (a random circuit's output), clusters of ties
    const size_t n = (size_t)1 << (8 + r % 9);
    std::vector<uint64_t> keys(n);
    const int kind = r % 4;
    for (size_t j = 0; j < n; ++j) {
      const double u = uni(rng);
      if (kind == 0) keys[j] = key_of(-std::log(1.0 - u) / (double)n);
      else if (kind == 1) keys[j] = key_of((double)(rng() % 7) / 8.0);                     // seven values, zero among them
      else if (kind == 2) keys[j] = key_of(0.3 + 1e-17 * (double)(rng() % 3));             // neighbours in the last bits
      else keys[j] = key_of(u < 0.01 ? u : 0.0);
    }
    for (uint64_t k : {1ull, 2ull, 16ull, 255ull, 4096ull}) {
      qh::SelPlan pl = qh::sel_begin(k, cap);
      const std::vector<uint64_t> h0 = histogram(keys, pl);
      qh::SelPlan probe = pl;
      const qh::SelStep first = qh::sel_step(probe, h0.data());
      // whatever the mixture ends with, run() checks it against the sort
      qh::SelNext end = first.next;
      if (end == qh::kSelRefine) {
        qh::SelStep st = first;
        while (st.next == qh::kSelRefine) {
          const std::vector<uint64_t> h = histogram(keys, probe);
          st = qh::sel_step(probe, h.data());
        }
        end = st.next;
      }
      run("random " + std::to_string(r) + " k=" + std::to_string(k), keys, k, cap, end, qh::kSelLevels);
    }
  }
  // the tie scan's first range
  expect(qh::sel_tie_first_len(1ull << 20, 1ull << 20, 16, 4096) == 4096, "tie range of a flat state starts at the floor");
  expect(qh::sel_tie_first_len(1ull << 20, 1ull << 10, 16, 4096) == 32768, "tie range scales with the density");
  expect(qh::sel_tie_first_len(1ull << 10, 1ull << 10, 16, 4096) == 1024, "tie range is at most the state");
  expect(qh::sel_tie_first_len(1ull << 30, 5000, 4096, 4096) == (1ull << 30), "sparse ties: the whole state");
  if (g_bad) {
    printf("%d check(s) failed\n", g_bad);
    return 1;
  }
  printf("ok\n");
  return 0;
}
