// exchange_plan_check.cc -- stand-alone check of qcc_amd/csrc/exchange_plan.h (the host side of the multi-GPU exchange), for
// sanitizer builds:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -static-libasan -static-libubsan
//       tools/exchange_plan_check.cc -o exchange_plan_check
// (the sanitizer runtimes linked statically: the program then runs as it is, in any environment).
//
// P = 2^g ranks are P host arrays of 2^nloc distinct values.  The program EXECUTES the rounds of a plan on them with memcpy,
// the way engine.hip's two runners do -- the RCCL one (two receive halves and, packed, two send halves of the staging area,
// alternating from round to round) and the host-staged one (two pinned buffers of one half; staging only for packed rounds)
// -- with every buffer allocated at exactly the size the plan states, so that the sanitizer sees a round that leaves it
// (both runners up to 2^8 amplitudes per rank; above, the executions take them in turn).
// Then it compares amplitude by amplitude with a bit-by-bit model (worked out once per placement of the block bits) of
//   all-to-all   the g shard bits change places with the g block bits,
//   pairwise     one shard bit changes places with one local bit,
//   loop-back    an X on one local bit (one rank, two moves to itself),
// for nloc 4..12 and g 1..3 (nloc >= 2g), the block bits at EVERY set of g positions (in a shuffled order: bit k of a block
// value sits at pos[k]), 0..3 slab bits both given by the flush (random positions outside the block bits, the values in a
// shuffled order) and picked by the plan, chunk_amps 0, 1, 2, .. 2^nloc, QH_EXCHANGE_PACK unset / 0 / 1 and both amplitude
// widths.  Many of these combinations give the same plan (chunk sizes above the free bits, an unset switch and the one it
// resolves to, picked slabs below 2^11 amplitudes per block): the relations below are checked for every combination, and a
// plan equal to one already executed for the same ranks and moves is not executed again.
// Besides the end-to-end result:
//   * every amplitude whose block value is some move's blk leaves in exactly one (slab, round, move), every one whose block
//     value is some move's land is written exactly once, and no other amplitude is touched;
//   * a direct round's run of 2^chunk_bits amplitudes is contiguous, aligned and inside one block and one slab value;
//   * amplitude j of a packed round, by a host model of expand_index, is amplitude j of the direct formula whenever the
//     direct formula is valid (chunk_bits within the run of low free bits);
//   * slabs x rounds x peers << chunk_bits == the amplitudes moved, staging == (4 if packed else 2) x peers x chunk bytes;
//   * the record repeats the plan, the switches parse and clamp.
// Exit status 0 = all good.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../qcc_amd/csrc/exchange_plan.h"

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

typedef unsigned long long ull;
typedef std::vector<uint64_t> Words;      // amplitudes are one (complex64) or two (complex128) 64-bit words

// the model of the kernels' expand_index (kernels_gate.hip.h): a zero inserted at each position, ascending
static uint64_t expand_model(uint64_t j, const int *pos, int n) {
  for (int k = 0; k < n; ++k) {
    const uint64_t low = (1ull << pos[k]) - 1ull;
    j = ((j & ~low) << 1) | (j & low);
  }
  return j;
}
// ... of every counter value a plan's packed rounds run through
static std::vector<uint64_t> expand_table(const qh::ExchangePlan &pl) {
  std::vector<uint64_t> t(pl.rounds_per_slab << pl.chunk_bits);
  for (uint64_t j = 0; j < t.size(); ++j) t[j] = expand_model(j, pl.ins_pos, pl.nins);
  return t;
}

__attribute__((always_inline)) inline static uint64_t amp_value(uint64_t global_index) { return (global_index + 1ull) * 0x9e3779b97f4a7c15ull; }   // (odd factor: distinct)

enum Mode { ALLTOALL, PAIRWISE, LOOPBACK };

struct Rank {
  std::vector<qh::BlockMove> moves;
  std::vector<int> slot_at_peer;     // move m's data arrives in this slot of its peer
  Words psi, staging, h_send, h_recv;
  std::vector<uint8_t> left, written;
};

struct Counts { long combos = 0, skipped = 0, executed = 0; };
static Counts counts;

// the moves of engine.hip qh_exchange_alltoall / _pair / _loopback
static std::vector<Rank> make_ranks(Mode mode, int g, int shard_bit) {
  const int P = mode == LOOPBACK ? 1 : 1 << g;
  std::vector<Rank> R(P);
  for (int r = 0; r < P; ++r) {
    if (mode == ALLTOALL) {
      for (int j = 0; j < P; ++j) if (j != r) R[r].moves.push_back(qh::BlockMove{j, j, j});
    } else if (mode == PAIRWISE) {
      const int mybit = (r >> shard_bit) & 1;
      R[r].moves.push_back(qh::BlockMove{r ^ (1 << shard_bit), 1 - mybit, 1 - mybit});
    } else {
      R[r].moves = {qh::BlockMove{r, 0, 1}, qh::BlockMove{r, 1, 0}};
    }
  }
  // sends and receives between two ranks are matched in order
  for (int r = 0; r < P; ++r)
    for (size_t m = 0; m < R[r].moves.size(); ++m) {
      const int q = R[r].moves[m].peer;
      int nth = 0;
      for (size_t i = 0; i < m; ++i) nth += R[r].moves[i].peer == q;
      int slot = -1;
      for (size_t i = 0; i < R[q].moves.size() && slot < 0; ++i)
        if (R[q].moves[i].peer == r && nth-- == 0) slot = (int)i;
      R[r].slot_at_peer.push_back(slot);
    }
  return R;
}

__attribute__((always_inline)) inline static int block_value(const qh::ExchangePlan &pl, uint64_t p) {
  int v = 0;
  for (int k = 0; k < pl.gbits; ++k) v |= (int)((p >> pl.pos[k]) & 1ull) << k;
  return v;
}

// one packed round's gather (scatter) of one rank: what k_xpack (k_xunpack) does with launch_packed_round's arguments
static void packed_kernel(const qh::ExchangePlan &pl, const std::vector<uint64_t> &expanded, Rank &rk, bool unpack, uint64_t *stage, int k,
                          uint64_t ci) {
  const uint64_t n = pl.chunk_amps(), w = pl.amp_bytes / 8, N = 1ull << pl.nloc;
  const uint64_t *counter = expanded.data() + pl.round_start(ci);
  uint64_t *psi = rk.psi.data();
  uint8_t *touched = (unpack ? rk.written : rk.left).data();
  for (int m = 0; m < pl.np; ++m) {
    const uint64_t off = pl.packed_offset(k, unpack ? rk.moves[m].land : rk.moves[m].blk);
    for (uint64_t j = 0; j < n; ++j) {
      const uint64_t idx = counter[j] | off;
      CHECK(idx < N, "packed index %llx outside the shard", (ull)idx);
      if (idx >= N) continue;
      uint64_t *in_shard = psi + idx * w, *in_stage = stage + (m * n + j) * w;
      for (uint64_t i = 0; i < w; ++i) if (unpack) in_shard[i] = in_stage[i]; else in_stage[i] = in_shard[i];
      touched[idx]++;
    }
  }
}

static void touch(std::vector<uint8_t> &cnt, uint64_t at, uint64_t n) {
  CHECK(at + n <= cnt.size(), "direct run [%llx, +%llx) outside the shard", (ull)at, (ull)n);
  uint8_t *c = cnt.data();
  for (uint64_t j = at; j < at + n && j < cnt.size(); ++j) c[j]++;
}

// Executes the plan: every round on every rank -- sends first, landings after -- as run_rounds_rccl (host == false) or
// run_rounds_host_staged (host == true) order them inside one round.  Sizes and offsets are the plan's bytes, in 64-bit words.
static void execute(const qh::ExchangePlan &pl, const std::vector<uint64_t> &expanded, std::vector<Rank> &R, bool host) {
  const uint64_t w = pl.amp_bytes / 8, nb = pl.chunk_bytes() / 8, half = pl.half_bytes / 8, N = 1ull << pl.nloc;
  uint64_t block_off[1 << qh::kMaxExchangeBits];
  for (int v = 0; v < (1 << pl.gbits); ++v) block_off[v] = pl.block_offset(v);
  for (size_t r = 0; r < R.size(); ++r) {
    Rank &rk = R[r];
    rk.psi.resize(N * w);
    uint64_t *psi = rk.psi.data();
    for (uint64_t p = 0; p < N; ++p) {
      psi[p * w] = amp_value(((uint64_t)r << pl.nloc) | p);
      if (w == 2) psi[p * w + 1] = ~psi[p * w];
    }
    rk.left.assign(N, 0);
    rk.written.assign(N, 0);
    // (the host-staged transport reserves no device staging for direct rounds)
    rk.staging = Words(host && !pl.packed ? 0 : pl.staging_bytes / 8);
    rk.h_send = Words(host ? half : 0);
    rk.h_recv = Words(host ? half : 0);
  }
  uint64_t round = 0;
  for (int k = 0; k < pl.slabs(); ++k)
    for (uint64_t ci = 0; ci < pl.rounds_per_slab; ++ci, ++round) {
      const int par = (int)(round & 1);
      const uint64_t off = pl.round_offset(k, ci);
      for (Rank &rk : R) {          // pack and send
        uint64_t *sstage = host ? rk.staging.data() : rk.staging.data() + (2 + par) * half;
        if (pl.packed) {
          packed_kernel(pl, expanded, rk, false, sstage, k, ci);
          if (host) memcpy(rk.h_send.data(), sstage, half * 8);
        }
        for (int m = 0; m < pl.np; ++m) {
          const uint64_t at = off | block_off[rk.moves[m].blk];
          if (!pl.packed) touch(rk.left, at, pl.chunk_amps());
          const uint64_t *src = !pl.packed ? &rk.psi[at * w] : host ? rk.h_send.data() + m * nb : sstage + m * nb;
          if (host && !pl.packed) { memcpy(rk.h_send.data() + m * nb, src, nb * 8); src = rk.h_send.data() + m * nb; }
          Rank &peer = R[rk.moves[m].peer];
          uint64_t *dst = (host ? peer.h_recv.data() : peer.staging.data() + par * half) + rk.slot_at_peer[m] * nb;
          memcpy(dst, src, nb * 8);
        }
      }
      for (Rank &rk : R) {          // land
        uint64_t *stage = host ? rk.staging.data() : rk.staging.data() + par * half;
        if (pl.packed) {
          if (host) memcpy(stage, rk.h_recv.data(), half * 8);
          packed_kernel(pl, expanded, rk, true, stage, k, ci);
          continue;
        }
        for (int m = 0; m < pl.np; ++m) {
          const uint64_t at = off | block_off[rk.moves[m].land];
          touch(rk.written, at, pl.chunk_amps());
          memcpy(&rk.psi[at * w], (host ? rk.h_recv.data() : stage) + m * nb, nb * 8);
        }
      }
    }
}

// The model, bit by bit: where the amplitude of rank r, local index p has gone -- (rank << nloc) | index, one entry per
// amplitude of every rank -- and the block value of every local index.  Computed once per layout.
struct Model {
  std::vector<uint64_t> dest;
  std::vector<uint8_t> block;
};
static Model make_model(Mode mode, int nloc, int nranks, int shard_bit, const std::vector<int> &pos) {
  const uint64_t N = 1ull << nloc;
  Model md;
  md.dest.resize(nranks * N);
  md.block.resize(N);
  for (uint64_t p = 0; p < N; ++p)
    for (size_t k = 0; k < pos.size(); ++k) md.block[p] |= (uint8_t)(((p >> pos[k]) & 1ull) << k);
  for (uint64_t r = 0; r < (uint64_t)nranks; ++r)
    for (uint64_t p = 0; p < N; ++p) {
      uint64_t r2 = r, p2 = p;
      if (mode == LOOPBACK) p2 = p ^ (1ull << pos[0]);
      else
        for (size_t k = 0; k < pos.size(); ++k) {      // shard bit rbit <-> local bit pbit
          const int rbit = mode == PAIRWISE ? shard_bit : (int)k, pbit = pos[k];
          const uint64_t br = (r >> rbit) & 1ull, bp = (p >> pbit) & 1ull;
          r2 = (r2 & ~(1ull << rbit)) | (bp << rbit);
          p2 = (p2 & ~(1ull << pbit)) | (br << pbit);
        }
      md.dest[r * N + p] = (r2 << nloc) | p2;
    }
  return md;
}

static void check_result(const qh::ExchangePlan &pl, const std::vector<Rank> &R, const Model &md, const char *what) {
  const uint64_t N = 1ull << pl.nloc, w = pl.amp_bytes / 8;
  for (uint64_t r = 0; r < R.size(); ++r) {
    bool leaves[256] = {false}, lands[256] = {false};
    for (const qh::BlockMove &mv : R[r].moves) leaves[mv.blk] = lands[mv.land] = true;
    const uint8_t *left = R[r].left.data(), *written = R[r].written.data(), *block = md.block.data();
    const uint64_t *dest = md.dest.data() + r * N;
    for (uint64_t p = 0; p < N; ++p) {
      const uint64_t r2 = dest[p] >> pl.nloc, p2 = dest[p] & (N - 1);
      const uint64_t want = amp_value((r << pl.nloc) | p), *got = R[r2].psi.data() + p2 * w;
      CHECK(got[0] == want && (w == 1 || got[1] == ~want),
            "%s nloc %d blocks %llx slabs %llx chunk_bits %d packed %d: amplitude (%llu, %llx) is not at (%llu, %llx)", what, pl.nloc,
            (ull)pl.block_bits, (ull)pl.slab_mask, pl.chunk_bits, (int)pl.packed, (ull)r, (ull)p, (ull)r2, (ull)p2);
      const int v = block[p];
      CHECK(left[p] == (leaves[v] ? 1 : 0) && written[p] == (lands[v] ? 1 : 0),
            "%s nloc %d blocks %llx slabs %llx chunk_bits %d packed %d: rank %llu index %llx left %d times, was written %d times", what,
            pl.nloc, (ull)pl.block_bits, (ull)pl.slab_mask, pl.chunk_bits, (int)pl.packed, (ull)r, (ull)p, left[p], written[p]);
    }
  }
}

// the relations that hold for every plan, executed or not
static void check_relations(const qh::ExchangePlan &pl, int nslab_bits) {
  const uint64_t local = (1ull << pl.nloc) - 1ull, n = pl.chunk_amps();
  int nb = 0;
  for (int k = 0; k < pl.gbits; ++k) nb += (int)((pl.block_bits >> pl.pos[k]) & 1ull);
  CHECK(nb == pl.gbits && __builtin_popcountll(pl.block_bits) == pl.gbits, "block bits %llx", (ull)pl.block_bits);
  CHECK(!(pl.slab_mask & pl.block_bits) && !(pl.slab_mask & ~local) && __builtin_popcountll(pl.slab_mask) == nslab_bits &&
            pl.slabs() == 1 << nslab_bits, "nloc %d blocks %llx: slab mask %llx, %d slabs, want %d bits", pl.nloc, (ull)pl.block_bits,
        (ull)pl.slab_mask, pl.slabs(), nslab_bits);
  std::vector<uint64_t> sv = pl.slab_vals;
  std::sort(sv.begin(), sv.end());
  for (size_t k = 0; k < sv.size(); ++k) CHECK(sv[k] == qh::deposit_bits(k, pl.slab_mask), "slab value %llx", (ull)sv[k]);
  CHECK(pl.free_mask == (local & ~pl.block_bits & ~pl.slab_mask), "free mask %llx", (ull)pl.free_mask);
  CHECK((uint64_t)pl.slabs() * pl.rounds_per_slab * (uint64_t)pl.np << pl.chunk_bits == (uint64_t)pl.np << (pl.nloc - pl.gbits),
        "nloc %d: %d slabs x %llu rounds x %d peers << %d", pl.nloc, pl.slabs(), (ull)pl.rounds_per_slab, pl.np, pl.chunk_bits);
  CHECK(pl.half_bytes == (uint64_t)pl.np * n * pl.amp_bytes && pl.staging_bytes == (pl.packed ? 4u : 2u) * pl.np * n * pl.amp_bytes,
        "staging %llu, half %llu", (ull)pl.staging_bytes, (ull)pl.half_bytes);
  CHECK(pl.nins == pl.gbits + nslab_bits, "%d inserted bits", pl.nins);
  for (int i = 0; i < pl.nins; ++i)
    CHECK(!((pl.free_mask >> pl.ins_pos[i]) & 1ull) && (i == 0 || pl.ins_pos[i] > pl.ins_pos[i - 1]), "inserted bit %d at %d", i, pl.ins_pos[i]);
  const int run_bits = __builtin_ctzll(~pl.free_mask);
  CHECK(pl.packed || pl.chunk_bits <= run_bits, "direct rounds of 2^%d amplitudes, runs of 2^%d", pl.chunk_bits, run_bits);
  const qh_xgeom G = qh::exchange_record(pl, 77, 3, true);
  CHECK(G.signature == 77 && G.slab_mask == pl.slab_mask && G.block_bits == pl.block_bits && G.rounds_per_slab == pl.rounds_per_slab &&
            G.staging_bytes == pl.staging_bytes && G.slabs == (uint32_t)pl.slabs() && G.chunk_bits == (uint32_t)pl.chunk_bits &&
            G.packed == (pl.packed ? 1u : 0u) && G.peers == (uint32_t)pl.np && G.sweeps_before == 3 && G.last_sweep_split == 1,
        "the record does not repeat the plan");
}

// per round and block value: the direct run and the packed indices
static void check_rounds(const qh::ExchangePlan &pl, const std::vector<uint64_t> &expanded) {
  const uint64_t n = pl.chunk_amps();
  const bool direct_valid = pl.chunk_bits <= __builtin_ctzll(~pl.free_mask);
  for (int k = 0; k < pl.slabs(); ++k)
    for (uint64_t ci = 0; ci < pl.rounds_per_slab; ++ci)
      for (int v = 0; v < (1 << pl.gbits); ++v) {
        const uint64_t at = pl.round_offset(k, ci) | pl.block_offset(v);
        if (direct_valid) {
          CHECK(!(at & (n - 1)) && !((n - 1) & ~pl.free_mask) && block_value(pl, at) == v && (at & pl.slab_mask) == pl.slab_vals[k],
                "direct run at %llx of 2^%d: block %d, slab %llx", (ull)at, pl.chunk_bits, v, (ull)pl.slab_vals[k]);
          CHECK(block_value(pl, at + n - 1) == v && ((at + n - 1) & pl.slab_mask) == pl.slab_vals[k], "direct run at %llx leaves its block", (ull)at);
        }
        for (uint64_t j = 0; j < n; ++j) {
          const uint64_t idx = expanded[pl.round_start(ci) + j] | pl.packed_offset(k, v);
          CHECK(block_value(pl, idx) == v && (idx & pl.slab_mask) == pl.slab_vals[k], "packed index %llx: block %d, slab %llx", (ull)idx, v,
                (ull)pl.slab_vals[k]);
          if (direct_valid) CHECK(idx == at + j, "packed index %llx, direct %llx", (ull)idx, (ull)(at + j));
        }
      }
}

static bool same_plan(const qh::ExchangePlan &a, const qh::ExchangePlan &b) {      // (what differs most often first)
  return a.chunk_bits == b.chunk_bits && a.packed == b.packed && a.amp_bytes == b.amp_bytes && a.slab_mask == b.slab_mask &&
         a.nloc == b.nloc && a.gbits == b.gbits && a.np == b.np && a.block_bits == b.block_bits && a.free_mask == b.free_mask &&
         a.rounds_per_slab == b.rounds_per_slab && a.half_bytes == b.half_bytes && a.staging_bytes == b.staging_bytes && a.nins == b.nins &&
         a.slab_vals == b.slab_vals && !memcmp(a.pos, b.pos, sizeof a.pos) && !memcmp(a.ins_pos, b.ins_pos, sizeof a.ins_pos);
}

// one choice of ranks, moves and block-bit positions: slabs x chunk sizes x packing x width
static void check_layout(Mode mode, int nloc, int g, int shard_bit, const std::vector<int> &pos, std::mt19937_64 &rng, const char *what) {
  const int gbits = (int)pos.size();
  std::vector<Rank> R = make_ranks(mode, g, shard_bit);
  const int np = (int)R[0].moves.size();
  const Model md = make_model(mode, nloc, (int)R.size(), shard_bit, pos);
  uint64_t block_bits = 0;
  for (int b : pos) block_bits |= 1ull << b;
  std::vector<int> others;
  for (int b = 0; b < nloc; ++b) if (!((block_bits >> b) & 1ull)) others.push_back(b);
  std::vector<qh::ExchangePlan> done;
  for (int variant = 0; variant < 8; ++variant) {
    const bool given = variant < 4;
    const int bits = variant & 3;
    if (given && bits > (int)others.size()) continue;      // (no such flush)
    uint64_t mask = 0;
    std::vector<uint64_t> vals;
    if (given) {
      std::shuffle(others.begin(), others.end(), rng);
      for (int k = 0; k < bits; ++k) mask |= 1ull << others[k];
      for (uint64_t k = 0; k < (1ull << bits); ++k) vals.push_back(qh::deposit_bits(k, mask));
      std::shuffle(vals.begin(), vals.end(), rng);
    }
    // picked: only where a slab still holds 2^10 amplitudes per block (bits 6.. are then free to pick from)
    const int want_slab_bits = given ? bits : std::min(bits, std::max(0, nloc - gbits - 10));
    for (int c = -1; c <= nloc; ++c)
      for (int pack = -1; pack <= 1; ++pack)
        for (uint64_t ab : {16, 8}) {
          qh::ExchangeSwitches sw;
          sw.pack = pack;
          if (!given) sw.slab_bits = sw.slab_bits_asked = bits;
          const qh::ExchangePlan pl = qh::plan_exchange(nloc, pos.data(), gbits, c < 0 ? 0 : 1ull << c, np, ab, sw, mask, given ? &vals : nullptr);
          ++counts.combos;
          if (pl.packed && pl.nins > qh::kExchangeMaxIns) {      // (what do_exchange refuses)
            ++counts.skipped;
            continue;
          }
          check_relations(pl, want_slab_bits);
          CHECK(pack < 0 || pl.packed == (pack != 0), "QH_EXCHANGE_PACK=%d gave packed %d", pack, (int)pl.packed);
          int want_bits = 0;      // the chunk asked for, within the free bits; direct rounds may be shorter
          while (want_bits < (c < 0 ? 22 : c) && want_bits < nloc - gbits - want_slab_bits) ++want_bits;
          CHECK(pl.packed ? pl.chunk_bits == want_bits : pl.chunk_bits <= want_bits, "chunk 2^%d asked, 2^%d planned", c, pl.chunk_bits);
          bool seen = false;
          for (const qh::ExchangePlan &d : done) seen = seen || same_plan(d, pl);
          if (seen) continue;
          done.push_back(pl);
          const std::vector<uint64_t> expanded = expand_table(pl);
          check_rounds(pl, expanded);
          // both transports up to 2^8 amplitudes per rank, one of them in turn above
          for (int t = 0; t < (nloc <= 8 ? 2 : 1); ++t) {
            execute(pl, expanded, R, nloc <= 8 ? t != 0 : (counts.executed & 1) != 0);
            check_result(pl, R, md, what);
            ++counts.executed;
          }
        }
  }
}

static void check_switches() {
  unsetenv("QH_EXCHANGE_SLAB_BITS");
  unsetenv("QH_EXCHANGE_PACK");
  qh::ExchangeSwitches w = qh::ExchangeSwitches::from_env();
  CHECK(w.slab_bits == 3 && w.pack == -1 && w.key() == "3;-1;", "defaults: %s", w.key().c_str());
  const struct { const char *slab, *pack; int bits; const char *key; } cases[] = {
      {"0", "1", 0, "0;1;"}, {"2", "0", 2, "2;0;"}, {"5", nullptr, 3, "5;-1;"}, {"-2", "7", 0, "-2;7;"}, {"3", "-1", 3, "3;-1;"}};
  for (const auto &cs : cases) {
    setenv("QH_EXCHANGE_SLAB_BITS", cs.slab, 1);
    if (cs.pack) setenv("QH_EXCHANGE_PACK", cs.pack, 1); else unsetenv("QH_EXCHANGE_PACK");
    w = qh::ExchangeSwitches::from_env();
    CHECK(w.slab_bits == cs.bits && w.key() == cs.key, "QH_EXCHANGE_SLAB_BITS=%s: %d bits, key %s", cs.slab, w.slab_bits, w.key().c_str());
  }
  unsetenv("QH_EXCHANGE_SLAB_BITS");
  unsetenv("QH_EXCHANGE_PACK");
}

int main() {
  std::mt19937_64 rng(20261019);
  check_switches();
  long layouts = 0;
  for (int nloc = 4; nloc <= 12; ++nloc) {
    for (int g = 1; g <= 3 && 2 * g <= nloc; ++g) {
      // all-to-all: every set of g positions, among them non-adjacent ones and ones below bit 3
      for (uint64_t set = 0; set < (1ull << nloc); ++set) {
        if (__builtin_popcountll(set) != g) continue;
        std::vector<int> pos;
        for (int b = 0; b < nloc; ++b) if ((set >> b) & 1ull) pos.push_back(b);
        std::shuffle(pos.begin(), pos.end(), rng);
        check_layout(ALLTOALL, nloc, g, 0, pos, rng, "all-to-all");
        ++layouts;
      }
      // pairwise: every shard bit with every local bit
      for (int s = 0; s < g; ++s)
        for (int b = 0; b < nloc; ++b, ++layouts) check_layout(PAIRWISE, nloc, g, s, {b}, rng, "pairwise");
    }
    for (int b = 0; b < nloc; ++b, ++layouts) check_layout(LOOPBACK, nloc, 0, 0, {b}, rng, "loop-back");
  }
  printf("exchange_plan_check: %ld layouts, %ld combinations, %ld refused by the engine and skipped, %ld executions\n", layouts,
         counts.combos, counts.skipped, counts.executed);
  if (counts.skipped * 20 >= counts.combos) {
    fprintf(stderr, "more than 5 %% of the combinations skipped\n");
    return 1;
  }
  if (failures) {
    fprintf(stderr, "%d failures\n", failures);
    return 1;
  }
  printf("exchange_plan_check: ok\n");
  return 0;
}
