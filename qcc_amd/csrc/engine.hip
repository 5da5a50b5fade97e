// engine.hip -- C-ABI (include/qcc_hip.h) of the MI355X gate-application engine.
//
// Replaces the reference's native hot path: apply1<>/applyc<> and their CPython
// wrappers in /root/reference/src/lib/xgates.cc:23-145.  One handle owns (or
// borrows) 2^nbits amplitudes in HBM plus a HIP stream; gates are either
// launched one kernel each (QH_FUSE_OFF, kernels_gate.hip.h) or queued and
// executed as fused register-tile sweeps (QH_FUSE_SWEEP, planner.h +
// kernels_sweep.hip.h).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <string>
#include <vector>

#include "../../include/qcc_hip.h"
#include "buffers.hip.h"
#include "kernels_common.hip.h"
#include "kernels_gate.hip.h"
#include "kernels_argmax.hip.h"
#include "kernels_dense.hip.h"
#include "kernels_mux.hip.h"
#include "kernels_perm.hip.h"
#include "perm_plan.h"
#include "kernels_rank1.hip.h"
#include "rank1_plan.h"
#include "kernels_measure.hip.h"
#include "kernels_select.hip.h"
#include "select_plan.h"
#include "kernels_expect.hip.h"
#include "kernels_density.hip.h"
#include "density_plan.h"
#include "kernels_pauli.hip.h"
#include "pauli_plan.h"
#include "kernels_pauli_product.hip.h"
#include "pauli_product_plan.h"
#include "kernels_zpoly.hip.h"
#include "zpoly_plan.h"
#include "kernels_two_state.hip.h"
#include "kernels_inner.hip.h"
#include "kernels_axpby.hip.h"
#include "kernels_transition.hip.h"
#include "transition_plan.h"
#include "kernels_resize.hip.h"
#include "planner.h"
#include "kernels_sweep.hip.h"

namespace {

thread_local std::string g_err = "";

int fail(int code, const char *fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}

#define HIP_TRY(expr)                                                                  \
  do {                                                                                 \
    hipError_t e_ = (expr);                                                            \
    if (e_ != hipSuccess)                                                              \
      return fail(e_ == hipErrorOutOfMemory ? QH_ERR_NOMEM : QH_ERR_HIP, "%s: %s (%s:%d)", \
                  #expr, hipGetErrorString(e_), __FILE__, __LINE__);                   \
  } while (0)

constexpr int kRedBlocks = 1024;
constexpr int kMatSlots = 8;                                              // qh_apply_matrix staging ring
constexpr size_t kMatSlotBytes = (size_t)16 << (2 * qh::kMaxDenseBits);   // one complex128 2^6 x 2^6 matrix

}  // namespace

struct qh_state_s {
  int nloc = 0, nglob = 0, bw = 128, device = 0;
  uint64_t shard = 0;
  void *d_psi = nullptr;
  void *host_psi = nullptr;    // qh_create_host_mapped: the pinned, GPU-visible host allocation d_psi points into
  void *d_alt = nullptr;       // second buffer of the same size: target of relayout sweeps (lazily allocated)
  int relayout = -1;           // -1 undecided, 0 off (attached memory, no room, QH_RELAYOUT=0), 1 on
  bool owns_mem = false, owns_stream = false, dry = false;
  bool poisoned = false;       // a sweep of a flush failed after others had run: the amplitudes are undefined until re-initialised
  hipStream_t stream = nullptr;
  int fusion = QH_FUSE_OFF;
  int perm[64];  // physical bit of logical bit
  std::vector<qh::GateRec> queue;
  qh_stats stats{};
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  hipEvent_t ev_read = nullptr;   // qh_inner: recorded behind this handle's flushed work when ANOTHER handle's stream reads it
  std::vector<hipEvent_t> laps;   // qh_timer_lap: events on the stream, read back by qh_timer_laps
  size_t laps_used = 0;
  // Scratch (buffers.hip.h): released by the members' destructors at `delete h`, after qh_destroy has made the device
  // current and drained the stream.  A new feature adds its buffer here and nowhere else.
  qh::DeviceBuffer red, redi;  // kRedBlocks doubles / kRedBlocks u64
  qh::SweepBuffers sweep;      // device/pinned op buffers for fused sweeps
  qh::DeviceBuffer tmax;       // per-unit maxima the last sweep of a flush leaves for qh_argmax (SweepParams::tilemax)
  qh::Comm *comm = nullptr;    // multi-GPU exchange (exchange.hip.h)
  // qh_apply_matrix: the caller's matrix is copied into pinned slot i, uploaded on the stream into device slot i, and slot i
  // is reused only after the event recorded behind the kernel that read it has completed
  qh::StagedUpload<kMatSlots> mat;
  // qh_apply_mux / qh_apply_diag: one pinned staging buffer and one device table, grown on demand (a k = 16 mux table is
  // 4 MiB: the ring's slots are too small); reused only after the event recorded behind the kernel that read the table
  qh::StagedUpload<1> tab;
  // qh_apply_zpoly / qh_expect_zpoly: the term block (zpoly_plan.h), written on the host, read by one kernel; one slot of a
  // fixed size, reused only after the event recorded behind that kernel
  qh::StagedUpload<1> zpoly;
  qh::DeviceBuffer rank1;      // qh_apply_rank1, second path: m_r per fibre and the partial sums of a split walk
  qh::DeviceBuffer meas;       // the readers' scratch (slabs, chunk sums, shot lists, results), grown on demand
  double *d_red() const { return red.as<double>(); }
  uint64_t *d_redi() const { return redi.as<uint64_t>(); }
  uint64_t amp_bytes() const { return bw == 128 ? 16 : 8; }
  uint64_t local_mask() const { return nloc >= 64 ? ~0ull : ((1ull << nloc) - 1ull); }
};

namespace {

// The one choice of the amplitude width: f(double{}) on complex128 handles, f(float{}) on complex64 ones.  Launch sites are
// generic lambdas that take R = decltype(x) (and A = qh::AmpT<R>::type, i.e. double2 / float2) from their argument x.
template <typename F> decltype(auto) with_real(const qh_state_s *h, F &&f) {
  if (h->bw == 128) return f(double{});
  return f(float{});
}

// Logical -> physical through the handle's bit map, on whole masks, and back.
uint64_t to_phys(const qh_state_s *h, uint64_t logical) {
  uint64_t p = 0;
  for (int b = 0; b < h->nglob; ++b)
    if ((logical >> b) & 1ull) p |= 1ull << h->perm[b];
  return p;
}
uint64_t to_logical(const qh_state_s *h, uint64_t phys) {
  uint64_t l = 0;
  for (int b = 0; b < h->nglob; ++b)
    if ((phys >> h->perm[b]) & 1ull) l |= 1ull << b;
  return l;
}
// A physical mask split at nloc: `local` are index bits of this shard's amplitudes, `held` are bits of the shard index
// (h->shard & held = the ones among them on this shard).  Host arithmetic only: valid on dry handles.
struct Placed { uint64_t local, held; };
Placed place(const qh_state_s *h, uint64_t phys) { return {phys & h->local_mask(), phys >> h->nloc}; }
Placed place_bit(const qh_state_s *h, int logical_bit) { return place(h, 1ull << h->perm[logical_bit]); }

// Physical local control bits as the kernels take them: bits 0-1 are never skipped in an index enumeration (the same
// 64-byte half line), so controls there are a predicate (`lowpred`) and only the others (`cm`) are inserted as ones.
struct LowSplit { uint32_t lowpred; uint64_t cm; };
LowSplit split_low(const qh_state_s *h, uint64_t cm_all) {
  const uint64_t low = (h->nloc > 2) ? 3ull : 0ull;
  return {(uint32_t)(cm_all & low), cm_all & ~low};
}

// k logical bits: every one in [0, nglob), then none twice.  *mask = the logical bits listed.
int check_bit_list(const qh_state_s *h, const char *who, int k, const int32_t *bits, uint64_t *mask) {
  *mask = 0;
  for (int j = 0; j < k; ++j)
    if (bits[j] < 0 || bits[j] >= h->nglob) return fail(QH_ERR_BAD_QUBIT, "%s: bit %d out of range [0,%d)", who, bits[j], h->nglob);
  for (int j = 0; j < k; ++j) {
    if ((*mask >> bits[j]) & 1ull) return fail(QH_ERR_SAME_QUBIT, "%s: bit %d appears twice", who, bits[j]);
    *mask |= 1ull << bits[j];
  }
  return QH_OK;
}

// The listed bits on this shard: the local ones as (physical position, index j in the list), ascending by position, and
// the j whose bit the shard index holds at 1 (`held_ones`; held at 0: in neither).
struct SplitBits {
  std::vector<std::pair<int, int>> local;
  uint64_t held_ones = 0;
};
SplitBits split_bits(const qh_state_s *h, int k, const int32_t *bits) {
  SplitBits s;
  for (int j = 0; j < k; ++j) {
    const Placed b = place_bit(h, bits[j]);
    if (!b.held) s.local.push_back({h->perm[bits[j]], j});
    else if (h->shard & b.held) s.held_ones |= 1ull << j;
  }
  std::sort(s.local.begin(), s.local.end());
  return s;
}

unsigned grid_for(uint64_t n, uint64_t cap) { return (unsigned)std::min<uint64_t>((n + 255) / 256, cap); }   // 256-thread blocks

// one kernel over the state: amplitudes the gate had to touch / amplitudes the kernel did, each read and written
void count_kernel(qh_state_s *h, uint64_t algorithmic_amps, uint64_t swept_amps) {
  h->stats.kernels_launched++;
  h->stats.bytes_algorithmic += algorithmic_amps * h->amp_bytes() * 2;
  h->stats.bytes_swept += swept_amps * h->amp_bytes() * 2;
}

template <typename R> qh::Gate2<R> to_gate(const double g[8]) {
  qh::Gate2<R> o;
  o.g0r = (R)g[0]; o.g0i = (R)g[1]; o.g1r = (R)g[2]; o.g1i = (R)g[3];
  o.g2r = (R)g[4]; o.g2i = (R)g[5]; o.g3r = (R)g[6]; o.g3i = (R)g[7];
  return o;
}

qh::BitIns make_ins(uint64_t ones_mask, int zero_pos) {
  qh::BitIns ins{};
  ins.n = 0;
  ins.ones = ones_mask;
  for (int b = 0; b < 64; ++b) {
    if (((ones_mask >> b) & 1ull) || b == zero_pos) ins.pos[ins.n++] = b;
  }
  return ins;
}

unsigned pick_grid(uint64_t nwork, int per_block) {
  uint64_t blocks = (nwork + per_block - 1) / per_block;
  if (blocks < 1) blocks = 1;
  // HIP refuses launches of 2^32 threads or more (a per-gate kernel over a 2^33-amplitude shard
  // would be 2^24 blocks of 256): the kernels are grid-stride, so cap the grid
  if (blocks > (1ull << 23)) blocks = 1ull << 23;
  return (unsigned)blocks;
}

using qh::env_int;
// Launch shape of the per-gate kernels (tools/membench on MI355X): small blocks
// of work, one chunk per block (no grid-stride), non-temporal access.

template <typename R, int U, bool NT>
void launch_pair_u(qh_state_s *h, uint64_t nwork, int p, const qh::BitIns &ins, const double g[8],
                   uint32_t lowpred) {
  using A = typename qh::AmpT<R>::type;
  const unsigned grid = pick_grid(nwork, 256 * U);
  if (nwork % (256 * U) == 0)
    hipLaunchKernelGGL((qh::k_pair<R, U, false, NT>), dim3(grid), dim3(256), 0, h->stream,
                       (A *)h->d_psi, nwork, p, ins, to_gate<R>(g), lowpred);
  else
    hipLaunchKernelGGL((qh::k_pair<R, U, true, NT>), dim3(grid), dim3(256), 0, h->stream,
                       (A *)h->d_psi, nwork, p, ins, to_gate<R>(g), lowpred);
}
// Launch shapes of the per-gate kernels, chosen by measurement (tools/membench/pairbench.hip, profiles/r04/):
int log2_u64(uint64_t v) { int g = 0; while ((1ull << g) < v) ++g; return g; }
bool tile_fits(uint64_t nwork, int per_block) {     // full tiles only (DPP partner fetch and the block rotation need them)
  return nwork >= (uint64_t)per_block && nwork % per_block == 0 && ((nwork / per_block) & (nwork / per_block - 1)) == 0 &&
         nwork / per_block < (1ull << 31);
}

template <typename R, int U, int WPB>
void launch_pair_tile(qh_state_s *h, uint64_t nwork, int p, const qh::BitIns &ins, const double g[8], uint32_t lowpred) {
  using A = typename qh::AmpT<R>::type;
  const uint64_t blocks = nwork / (64 * U * WPB);
  hipLaunchKernelGGL((qh::k_pair_tile<R, U, WPB, 3>), dim3((unsigned)blocks), dim3(64 * WPB), 0, h->stream, (A *)h->d_psi, p, ins,
                     to_gate<R>(g), lowpred, log2_u64(blocks));
}
template <typename R, int P>
void launch_pair_line(qh_state_s *h, uint64_t namps, const qh::BitIns &ins1, const double g[8], uint32_t lowpred) {
  using A = typename qh::AmpT<R>::type;
  const uint64_t blocks = namps / (64 * 8 * 4);
  hipLaunchKernelGGL((qh::k_pair_line<R, P, 8, 4, 3>), dim3((unsigned)blocks), dim3(256), 0, h->stream, (A *)h->d_psi, ins1,
                     to_gate<R>(g), lowpred, log2_u64(blocks));
}

// `ins` enumerates pairs (a zero inserted at p); `ins1` the amplitudes of the same set (no zero at p)
template <typename R>
void launch_pair(qh_state_s *h, uint64_t nwork, int p, const qh::BitIns &ins, const qh::BitIns &ins1, const double g[8],
                 uint32_t lowpred) {
  if (p < 3 && tile_fits(2 * nwork, 64 * 8 * 4)) {
    if (p == 0) launch_pair_line<R, 0>(h, 2 * nwork, ins1, g, lowpred);
    else if (p == 1) launch_pair_line<R, 1>(h, 2 * nwork, ins1, g, lowpred);
    else launch_pair_line<R, 2>(h, 2 * nwork, ins1, g, lowpred);
    return;
  }
  if (p >= 3 && p <= 8 && tile_fits(nwork, 64 * 8 * 4)) return launch_pair_tile<R, 8, 4>(h, nwork, p, ins, g, lowpred);
  if (p >= 20 && p <= 25 && tile_fits(nwork, 64 * 16 * 2)) return launch_pair_tile<R, 16, 2>(h, nwork, p, ins, g, lowpred);
  launch_pair_u<R, 1, true>(h, nwork, p, ins, g, lowpred);      // one pair per thread, 256-thread blocks (small / ragged states too)
}

template <typename R, int U, bool NT>
void launch_diag_u(qh_state_s *h, uint64_t nwork, int sel, const qh::BitIns &ins, double f0r, double f0i,
                   double f1r, double f1i, uint32_t lowpred) {
  using A = typename qh::AmpT<R>::type;
  const unsigned grid = pick_grid(nwork, 256 * U);
  if (nwork % (256 * U) == 0)
    hipLaunchKernelGGL((qh::k_diag<R, U, false, NT>), dim3(grid), dim3(256), 0, h->stream,
                       (A *)h->d_psi, nwork, sel, ins, (R)f0r, (R)f0i, (R)f1r, (R)f1i, lowpred);
  else
    hipLaunchKernelGGL((qh::k_diag<R, U, true, NT>), dim3(grid), dim3(256), 0, h->stream,
                       (A *)h->d_psi, nwork, sel, ins, (R)f0r, (R)f0i, (R)f1r, (R)f1i, lowpred);
}
template <typename R>
void launch_diag(qh_state_s *h, uint64_t nwork, int sel, const qh::BitIns &ins, double f0r, double f0i,
                 double f1r, double f1i, uint32_t lowpred = 0) {
  using A = typename qh::AmpT<R>::type;
  if (tile_fits(nwork, 64 * 8 * 4)) {
    const uint64_t blocks = nwork / (64 * 8 * 4);
    hipLaunchKernelGGL((qh::k_diag_tile<R, 8, 4, 3>), dim3((unsigned)blocks), dim3(256), 0, h->stream, (A *)h->d_psi, sel, ins,
                       (R)f0r, (R)f0i, (R)f1r, (R)f1i, lowpred, log2_u64(blocks));
    return;
  }
  launch_diag_u<R, 2, true>(h, nwork, sel, ins, f0r, f0i, f1r, f1i, lowpred);   // (a diagonal work item is one amplitude, a pair item two)
}

// One gate, physical bit positions, one kernel.  Returns QH_* status.
int launch_single(qh_state_s *h, const qh::GateRec &r) {
  const Placed ctl = place(h, r.ctl_mask);
  if ((h->shard & ctl.held) != ctl.held) {
    h->stats.gates_noop++;
    return QH_OK;
  }
  const uint64_t cm_all = ctl.local;
  const LowSplit low = split_low(h, cm_all);
  uint32_t lowpred = low.lowpred;
  const uint64_t cm = low.cm;
  const int nc_all = __builtin_popcountll(cm_all);
  const int nc = __builtin_popcountll(cm);
  if (nc + 1 > qh::kMaxIns) return fail(QH_ERR_ARG, "too many local control bits (%d)", nc);
  const double *g = r.g;
  const bool diag = qh::is_diag(g);
  // a diagonal kernel: factors (f0, f1) by bit `sel` of the index (-1: f1 everywhere), `ones` inserted as 1s
  auto diag_kernel = [&](uint64_t nwork, int sel, uint64_t ones, double f0r, double f0i, double f1r, double f1i) {
    if (h->dry) return;
    const qh::BitIns ins = make_ins(ones, -1);
    with_real(h, [&](auto x) { launch_diag<decltype(x)>(h, nwork, sel, ins, f0r, f0i, f1r, f1i, lowpred); });
  };
  if (r.tgt >= h->nloc) {
    if (!diag)
      return fail(QH_ERR_NONLOCAL,
                  "non-diagonal gate targets physical bit %d held by the shard index "
                  "(local bits: %d); exchange first",
                  r.tgt, h->nloc);
    const bool set = (h->shard >> (r.tgt - h->nloc)) & 1ull;
    const double fr = set ? g[6] : g[0], fi = set ? g[7] : g[1];
    if (fr == 1.0 && fi == 0.0) {
      h->stats.gates_noop++;
      return QH_OK;
    }
    const uint64_t nwork = 1ull << (h->nloc - nc);
    diag_kernel(nwork, -1, cm, 1, 0, fr, fi);
    count_kernel(h, 1ull << (h->nloc - nc_all), nwork);
    return QH_OK;
  }
  if (diag) {
    const bool one_sided = (g[0] == 1.0 && g[1] == 0.0);
    if (one_sided && g[6] == 1.0 && g[7] == 0.0) {
      h->stats.gates_noop++;
      return QH_OK;  // identity
    }
    if (one_sided) {
      const bool tgt_low = h->nloc > 2 && r.tgt < 2;        // target itself inside the half line
      if (tgt_low) lowpred |= 1u << r.tgt;
      const uint64_t nwork = 1ull << (h->nloc - nc - (tgt_low ? 0 : 1));
      diag_kernel(nwork, -1, tgt_low ? cm : (cm | (1ull << r.tgt)), 1, 0, g[6], g[7]);
      count_kernel(h, 1ull << (h->nloc - nc_all - 1), nwork);
    } else {
      const uint64_t nwork = 1ull << (h->nloc - nc);
      diag_kernel(nwork, r.tgt, cm, g[0], g[1], g[6], g[7]);
      count_kernel(h, 1ull << (h->nloc - nc_all), nwork);
    }
    return QH_OK;
  }
  const uint64_t nwork = 1ull << (h->nloc - nc - 1);      // pairs
  if (!h->dry) {
    const qh::BitIns ins = make_ins(cm, r.tgt), ins1 = make_ins(cm, -1);
    with_real(h, [&](auto x) { launch_pair<decltype(x)>(h, nwork, r.tgt, ins, ins1, g, lowpred); });
  }
  count_kernel(h, 1ull << (h->nloc - nc_all), 2 * nwork);
  return QH_OK;
}

int check_launch(qh_state_s *h) {
  if (h->dry) return QH_OK;
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(QH_ERR_HIP, "kernel launch: %s", hipGetErrorString(e));
  return QH_OK;
}

// Kernels, op-buffer allocations and events of a handle belong to ITS device, whatever device
// the calling thread had current (a process may hold handles on several GPUs).
int use_device(qh_state_s *h) {
  if (h->dry) return QH_OK;
  HIP_TRY(hipSetDevice(h->device));
  return QH_OK;
}

// Host waits.  A handle whose communicator has several ranks may wait for work that depends on OTHER processes (a
// grouped send/recv completes only when every peer has posted its half): if a peer is missing, or the ranks disagree
// about a round, a plain hipStreamSynchronize never returns.  Such handles poll instead and give up after
// QH_COMM_TIMEOUT_MS (default 300 s): QH_ERR_COMM, the handle poisoned -- an error line instead of a hung job.
int comm_timeout_ms() { return env_int("QH_COMM_TIMEOUT_MS", 300000); }      // (read at every wait: tests shorten it)
// QH_COMM_WATCH_ALL=1 (tests): watch every handle that has a communicator, the one-rank loop-back included
bool watched(const qh_state_s *h) {
  if (!h->comm || h->comm->dry) return false;
  return (h->comm->nranks > 1 && !h->comm->custom) || env_int("QH_COMM_WATCH_ALL", 0) != 0;
}
// A watched wait that gives up must not leave work behind that still writes into the CALLER's memory (the readers' D2H
// copies of a few bytes, qh_download's buffer) once this call has returned: abort the RCCL communicator -- its kernels
// then end, whatever the peers do -- and let the handle's streams drain (bounded: 10 s) before the error goes up.  The
// communicator is gone afterwards (exchanges and all-reduces fail with QH_ERR_COMM); the process should tear the job down.
void abort_comm_and_drain(qh_state_s *h) {
  qh::Comm *c = h->comm;
  if (!c || c->dry) return;
  if (c->nccl) {
    (void)qh::rccl().CommAbort(c->nccl);
    c->nccl = nullptr;
  }
  const auto t0 = std::chrono::steady_clock::now();
  for (hipStream_t s : {c->xstream, c->cstream, c->pstream, h->stream}) {
    if (!s) continue;
    while (hipStreamQuery(s) == hipErrorNotReady) {
      if (std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > 10.0) return;
      struct timespec ts = {0, 200000};
      nanosleep(&ts, nullptr);
    }
  }
  (void)hipGetLastError();
}
template <typename Query> int poll_until_done(qh_state_s *h, Query query, const char *what) {
  const auto t0 = std::chrono::steady_clock::now();
  for (unsigned spins = 0;; ++spins) {
    const hipError_t e = query();
    if (e == hipSuccess) return QH_OK;
    if (e != hipErrorNotReady) {
      (void)hipGetLastError();
      return fail(QH_ERR_HIP, "%s: %s", what, hipGetErrorString(e));
    }
    if (spins > 2000) {
      const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
      if (ms > comm_timeout_ms()) {
        h->poisoned = true;
        abort_comm_and_drain(h);
        return fail(QH_ERR_COMM, "%s: rank %d of %d still waiting after %.0f s (QH_COMM_TIMEOUT_MS): a peer is missing or the "
                    "ranks disagree about an exchange; the communicator was aborted, the state of this handle is undefined", what,
                    h->comm->rank, h->comm->nranks, ms * 1e-3);
      }
      struct timespec ts = {0, 50000};
      nanosleep(&ts, nullptr);
    }
  }
}
int wait_stream(qh_state_s *h, hipStream_t s, const char *what) {
  if (!watched(h)) {
    HIP_TRY(hipStreamSynchronize(s));
    return QH_OK;
  }
  return poll_until_done(h, [&] { return hipStreamQuery(s); }, what);
}
int wait_event(qh_state_s *h, hipEvent_t e, const char *what) {
  if (!watched(h)) {
    HIP_TRY(hipEventSynchronize(e));
    return QH_OK;
  }
  return poll_until_done(h, [&] { return hipEventQuery(e); }, what);
}

// Sweeps may re-lay the state out into a second buffer (planner.h, Planner::relayout) when the handle owns its
// memory and a second buffer of the same size fits.  A handle with a communicator of more than one rank only
// does so after qh_set_relayout(h, 1) -- the ranks must agree (an exchange needs the same layout everywhere),
// and only the caller can ask them all.
bool relayout_eligible(const qh_state_s *h) {
  return env_int("QH_RELAYOUT", 1) != 0 && h->owns_mem && !h->host_psi && qh::sweep_supported(h->nloc, h->bw);
}
// what a flush would get, without allocating anything (plans shown by qh_plan_json / qh_plan_export)
bool relayout_wanted(const qh_state_s *h) {
  if (h->dry) return env_int("QH_RELAYOUT", 1) != 0;      // planner-only handles: plan what a real handle would
  if (h->relayout >= 0) return h->relayout == 1;
  return relayout_eligible(h) && !(h->comm && h->comm->nranks > 1);
}
// What the planner works from for this handle, the switches read now (planner.h PlanSwitches)
qh::PlanRequest plan_request(const qh_state_s *h, bool relayout) {
  return qh::PlanRequest{h->nloc, h->bw, h->shard, relayout, h->nglob > h->nloc, qh::PlanSwitches::from_env()};
}
// A state buffer.  Buffers of 4..32 GiB (QH_ALLOC_CONTIG=1: every buffer >= 64 MiB, =0: none) are asked for as
// PHYSICALLY contiguous VRAM first (hipDeviceMallocContiguous); if the driver has no contiguous range left it is plain
// hipMalloc.  Measured, not derived (DESIGN 7 "placement", profiles/r03/alloc_contiguous_*): where the driver puts a
// buffer decides +-2.5 % of a sweep's time; contiguous 8- and 16-GiB buffers land in the fast mode 11 times of 12
// (30-qubit QFT 16.54 ms mean vs 16.92 over 12 interleaved fresh processes), a contiguous 256-GiB state is 6 % slower.
// (round 5, profiles/r05/alloc_second_buffer_ab.txt: on that box plain buffers cost 1.3-1.5 ms of a 17-ms QFT, a plain SECOND
// buffer 0.5-1.2; and the seconds an allocation sometimes takes are not the contiguous search -- any allocation that follows the
// release of a 128- or 256-GiB state pays ~6.2 s of driver work, plain ones too.)
hipError_t alloc_state_buffer(void **p, size_t bytes) {
  static const int contig = env_int("QH_ALLOC_CONTIG", -1), debug = env_int("QH_ALLOC_DEBUG", 0);
  const auto t0 = std::chrono::steady_clock::now();
  hipError_t e = hipErrorOutOfMemory;
  bool got_contig = false;
  const bool want_contig = contig < 0 ? (bytes >= (4ull << 30) && bytes <= (32ull << 30)) : (contig > 0 && bytes >= (64ull << 20));
  if (want_contig) {
    e = hipExtMallocWithFlags(p, bytes, hipDeviceMallocContiguous);
    got_contig = e == hipSuccess;
    if (!got_contig) {
      (void)hipGetLastError();
      *p = nullptr;
    }
  }
  if (!got_contig) e = hipMalloc(p, bytes);
  if (debug)
    fprintf(stderr, "[qh alloc %zu MiB %s at %p in %.1f ms]\n", bytes >> 20, got_contig ? "contiguous" : "plain", *p,
            std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
  return e;
}
bool second_buffer_fits(const qh_state_s *h, size_t bytes) {
  size_t fr = 0, total = 0;
  // (a communicator of several ranks will want its staging halves too: up to 4 x (P-1) x chunk amplitudes)
  const size_t reserve = (bytes >> 5) + (3ull << 29) + ((h->comm && h->comm->nranks > 1) ? (4ull << 30) : 0);
  return hipMemGetInfo(&fr, &total) == hipSuccess && fr > bytes + reserve;
}
bool alloc_second_buffer(qh_state_s *h) {
  if (h->d_alt) return true;
  const size_t bytes = (size_t)h->amp_bytes() << h->nloc;
  if (second_buffer_fits(h, bytes) && alloc_state_buffer(&h->d_alt, bytes) == hipSuccess)
    return true;
  (void)hipGetLastError();
  h->d_alt = nullptr;
  return false;
}
bool relayout_ready(qh_state_s *h) {
  if (h->dry) return relayout_wanted(h);
  if (h->relayout < 0) {
    h->relayout = 0;
    if (relayout_eligible(h) && !(h->comm && h->comm->nranks > 1) && alloc_second_buffer(h)) h->relayout = 1;
  }
  return h->relayout == 1;
}

bool layout_is_canonical(const qh_state_s *h) {
  int last = -1;
  for (int b = 0; b < h->nglob; ++b) {
    if (h->perm[b] >= h->nloc) continue;
    if (h->perm[b] < last) return false;
    last = h->perm[b];
  }
  return true;
}

// Brings the local index bits back into ascending logical order (one gather pass into the second
// buffer): for the entry points that hand out or take amplitudes in physical order.  A handle that keeps no second buffer
// (no flush has asked for one yet, relayout off, attached or host-mapped memory: qh_remap_swap alone can put its local bits
// out of order) borrows one for the pass: the result is copied back, so d_psi stays where the caller knows it, and the
// buffer is freed again.
int canonicalize(qh_state_s *h) {
  if (h->dry || layout_is_canonical(h)) return QH_OK;
  const bool borrowed = !h->d_alt;
  if (borrowed && !alloc_second_buffer(h))
    return fail(QH_ERR_NOMEM, "no room for the second buffer of %llu bytes that bringing a permuted layout back to canonical order needs",
                (unsigned long long)(h->amp_bytes() << h->nloc));
  std::vector<int> loc;                       // logical bits that live on local positions, ascending
  for (int b = 0; b < h->nglob; ++b) if (h->perm[b] < h->nloc) loc.push_back(b);
  std::vector<int> posn;                      // the local positions they occupy, ascending
  for (int b : loc) posn.push_back(h->perm[b]);
  std::sort(posn.begin(), posn.end());
  qh::BitPerm bp{};
  bp.n = h->nloc;
  for (size_t k = 0; k < loc.size(); ++k) bp.src_of_dst[posn[k]] = (uint8_t)h->perm[loc[k]];
  const uint64_t n = 1ull << h->nloc;
  with_real(h, [&](auto x) {
    using R = decltype(x);
    using A = typename qh::AmpT<R>::type;
    hipLaunchKernelGGL(qh::k_permute_bits<R>, dim3(grid_for(n, 1ull << 22)), dim3(256), 0, h->stream, (const A *)h->d_psi, (A *)h->d_alt, n, bp);
  });
  int rc = check_launch(h);
  if (rc == QH_OK && borrowed) {
    hipError_t e = hipMemcpyAsync(h->d_psi, h->d_alt, (size_t)h->amp_bytes() << h->nloc, hipMemcpyDefault, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) rc = fail(QH_ERR_HIP, hipGetErrorString(e));
  }
  if (borrowed) {
    if (rc) (void)hipStreamSynchronize(h->stream);      // (the gather may still be reading or writing)
    (void)hipFree(h->d_alt);
    h->d_alt = nullptr;
  } else if (rc == QH_OK) {
    std::swap(h->d_psi, h->d_alt);
  }
  if (rc) return rc;
  for (size_t k = 0; k < loc.size(); ++k) h->perm[loc[k]] = posn[k];
  return QH_OK;
}

// Runs the queue.  On failure the gates that did NOT run stay queued (qh_pending_gates):
// a planning / allocation failure keeps the whole queue, a failed per-gate launch keeps the
// failing gate and everything after it.  Only a failed launch of a planned sweep leaves the
// state partially updated; the queue is then dropped and the error says so.
int flush_impl(qh_state_s *h, qh::SlabIO *split = nullptr, qh::TileMaxOut *tmax = nullptr) {
  int rc = use_device(h);
  if (rc) return rc;
  if (h->poisoned)
    return fail(QH_ERR_HIP, "the state of this handle is undefined: a sweep of an earlier flush failed after others had run; "
                            "re-initialise it (qh_init_basis / qh_init_product / qh_upload of the whole shard)");
  std::vector<qh::Arrival> *arr = (h->comm && !h->comm->arrivals.empty()) ? &h->comm->arrivals : nullptr;
  if (h->queue.empty()) {
    qh::wait_all_arrivals(arr, h->stream);   // whoever called touches the state next
    return QH_OK;
  }
  if (h->fusion == QH_FUSE_SWEEP && qh::sweep_supported(h->nloc, h->bw)) {
    const uint64_t launched0 = h->stats.kernels_launched;
    qh::SlabIO local;
    qh::SlabIO *io = split ? split : &local;
    io->arrivals = arr;
    io->comm = h->comm;
    const bool relay = relayout_ready(h);
    void *result = h->d_psi;
    uint8_t final_pos[64];
    rc = qh::run_fused(h->queue, plan_request(h, relay), h->d_psi, h->stream, h->dry, &h->sweep, &h->stats, &g_err,
                       h->comm ? io : nullptr, h->d_alt, &result, final_pos, tmax);
    if (rc == QH_OK && relay) {
      if (result != h->d_psi) std::swap(h->d_psi, h->d_alt);
      for (int b = 0; b < h->nglob; ++b)
        if (h->perm[b] < h->nloc) h->perm[b] = final_pos[h->perm[b]];
    }
    qh::wait_all_arrivals(arr, h->stream);   // (a flush that planned no sweep)
    if (h->comm) h->comm->stats.sweeps_overlapped += io->sweeps_overlapped;
    if (rc != QH_OK && h->stats.kernels_launched == launched0) return rc;   // nothing ran: queue kept
    if (rc == QH_OK) rc = check_launch(h);
    if (rc != QH_OK) {
      g_err += " [sweeps of this flush may have run partially: its gates were dropped and the state is undefined until re-initialised]";
      h->poisoned = true;
    }
    h->queue.clear();
    return rc;
  }
  qh::wait_all_arrivals(arr, h->stream);
  size_t done = 0;
  for (const auto &r : h->queue) {
    rc = launch_single(h, r);
    if (rc == QH_OK) rc = check_launch(h);
    if (rc) break;
    ++done;
  }
  h->queue.erase(h->queue.begin(), h->queue.begin() + done);
  return rc;
}

// The prologue of every entry point that works on the amplitudes, called after its argument checks: planner-only handles are
// refused, the handle's device becomes current and what is queued runs (flush_impl begins with use_device).
int enter(qh_state_s *h) {
  if (h->dry) return fail(QH_ERR_ARG, "not on a dry (planner-only) handle");
  return flush_impl(h);
}
// ... and the tail of the readers: `bytes` from the device to the caller on the handle's stream, then the host waits.
int read_back(qh_state_s *h, void *host, const void *dev, size_t bytes, const char *what = "reader") {
  HIP_TRY(hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, h->stream));
  return wait_stream(h, h->stream, what);
}
// The host half of the readers' fixed-order sum (kernels_common.hip.h), in h->meas: a slab of rows x cols doubles, of which
// the reading kernel writes one row per block, and nout results.  fold() adds the rows in block order, get() is the read_back.
struct SlabSum {
  qh_state_s *h;
  size_t bytes = 0;
  double *slab = nullptr, *out = nullptr;
  hipError_t reserve(size_t rows, size_t cols, size_t nout) {
    qh::ScratchLayout lay;
    const size_t slab_off = lay.add(rows * cols * sizeof(double)), out_off = lay.add(nout * sizeof(double));
    bytes = lay.total;
    const hipError_t e = h->meas.reserve(bytes);
    if (e != hipSuccess) return e;
    slab = (double *)(h->meas.as<char>() + slab_off);
    out = (double *)(h->meas.as<char>() + out_off);
    return hipSuccess;
  }
  // out[at + t] = scale * (column t of the first nblk rows), for t < n
  void fold(uint64_t nblk, int cols, unsigned n, double scale = 1.0, uint64_t at = 0) const {
    hipLaunchKernelGGL(qh::k_slab_fold, dim3(n), dim3(256), 0, h->stream, (const double *)slab, (uint32_t)nblk, cols, scale, out + at);
  }
  int get(double *vals, size_t n, const char *what = "reader") const { return read_back(h, vals, out, n * sizeof(double), what); }
};

// on: allocate the second buffer now (false if it does not fit); off: queued gates run, the layout returns to
// canonical order, the second buffer is freed.  *actual (optional) = the resulting mode.
int set_relayout(qh_state_s *h, bool on, int *actual = nullptr) {
  if (h->dry) {
    if (actual) *actual = relayout_wanted(h) ? 1 : 0;
    return QH_OK;
  }
  int rc = use_device(h);
  if (rc) return rc;
  if (on) {
    if (h->relayout != 1) h->relayout = (relayout_eligible(h) && alloc_second_buffer(h)) ? 1 : 0;
  } else {
    rc = flush_impl(h);
    if (rc == QH_OK) rc = canonicalize(h);
    if (rc) return rc;
    if (h->d_alt) {
      HIP_TRY(hipStreamSynchronize(h->stream));
      (void)hipFree(h->d_alt);
      h->d_alt = nullptr;
    }
    h->relayout = 0;
  }
  if (actual) *actual = h->relayout == 1 ? 1 : 0;
  return QH_OK;
}

int submit_phys(qh_state_s *h, uint64_t cmask, int tbit, const double g[8]) {
  qh::GateRec r;
  r.ctl_mask = cmask;
  r.tgt = tbit;
  memcpy(r.g, g, sizeof r.g);
  if (h->fusion != QH_FUSE_OFF) {
    // a non-diagonal gate on a shard bit can never be executed: report now.
    if (tbit >= h->nloc && !qh::is_diag(g))
      return fail(QH_ERR_NONLOCAL,
                  "non-diagonal gate targets physical bit %d held by the shard index", tbit);
    h->queue.push_back(r);
    h->stats.gates_submitted++;
    if (h->queue.size() >= 8192) return flush_impl(h);
    return QH_OK;
  }
  int rc = use_device(h);
  if (rc == QH_OK) rc = launch_single(h, r);
  if (rc == QH_OK) rc = check_launch(h);
  if (rc == QH_OK) h->stats.gates_submitted++;
  return rc;
}

int apply_logical(qh_state_s *h, uint64_t ctl_mask, int tgt_bit, const double g[8]) {
  if (!h) return fail(QH_ERR_ARG, "null handle");
  if (!g) return fail(QH_ERR_ARG, "null gate");
  if (tgt_bit < 0 || tgt_bit >= h->nglob)
    return fail(QH_ERR_BAD_QUBIT, "target bit %d out of range [0,%d)", tgt_bit, h->nglob);
  if (h->nglob < 64 && (ctl_mask >> h->nglob))
    return fail(QH_ERR_BAD_QUBIT, "control mask 0x%llx has bits >= %d",
                (unsigned long long)ctl_mask, h->nglob);
  if ((ctl_mask >> tgt_bit) & 1ull) return fail(QH_ERR_SAME_QUBIT, "control == target (bit %d)", tgt_bit);
  return submit_phys(h, to_phys(h, ctl_mask), h->perm[tgt_bit], g);
}

// Reference control semantics incl. quirk Q7 (see oracle/xgates_oracle.c):
// maps a reference control qubit number to a logical control bit, -1 = no-op,
// -2 = error.
int ref_ctl_bit(int nbits, int ctl, int tgt_bit) {
  const long c = (long)nbits - (long)ctl - 1;
  if (c < 0) return -2;
  if (c < nbits) return (int)c;
  const long b = c - nbits;  // bit b of the block base g
  if (b > tgt_bit && b < nbits) return (int)b;
  return -1;
}

int make_events(qh_state_s *h) {
  if (!h->ev0) {
    HIP_TRY(hipEventCreate(&h->ev0));
    HIP_TRY(hipEventCreate(&h->ev1));
  }
  return QH_OK;
}

int common_init(qh_state_s *h) {
  for (int b = 0; b < 64; ++b) h->perm[b] = b;
  if (h->dry) return QH_OK;
  HIP_TRY(h->red.reserve(kRedBlocks * sizeof(double)));
  HIP_TRY(h->redi.reserve(kRedBlocks * sizeof(uint64_t)));
  return QH_OK;
}

int check_args(int nbits, int bit_width) {
  static_assert(qh::kInnerMaxLocalBits == 40, "kernels_two_state.hip.h sizes its tables for the limit below");
  if (nbits < 1 || nbits > 40) return fail(QH_ERR_ARG, "nbits %d out of range [1,40]", nbits);
  if (bit_width != 64 && bit_width != 128)
    return fail(QH_ERR_BAD_DTYPE, "bit_width %d (want 64 or 128)", bit_width);
  return QH_OK;
}

int select_device(int device) {
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n <= 0)
    return fail(QH_ERR_NO_DEVICE, "no HIP device visible (%s); this engine has no CPU fallback",
                e == hipSuccess ? "count=0" : hipGetErrorString(e));
  if (device < 0 || device >= n) return fail(QH_ERR_ARG, "device %d of %d", device, n);
  HIP_TRY(hipSetDevice(device));
  return QH_OK;
}

}  // namespace

extern "C" {

const char *qh_last_error(void) { return g_err.c_str(); }
int qh_version(void) { return 120; }   // 100 + round: bumped whenever plans, exchange geometry or the C-ABI change

int qh_device_count(int *count) {
  if (!count) return fail(QH_ERR_ARG, "null");
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  *count = (e == hipSuccess) ? n : 0;
  return QH_OK;
}

int qh_create(int nbits, int bit_width, int device, qh_handle *out) {
  if (!out) return fail(QH_ERR_ARG, "null out");
  int rc = check_args(nbits, bit_width);
  if (rc) return rc;
  rc = select_device(device);
  if (rc) return rc;
  auto *h = new qh_state_s;
  h->nloc = h->nglob = nbits;
  h->bw = bit_width;
  h->device = device;
  const uint64_t bytes = (1ull << nbits) * h->amp_bytes();
  hipError_t e = alloc_state_buffer(&h->d_psi, bytes);
  if (e != hipSuccess) {
    delete h;
    return fail(QH_ERR_NOMEM, "hipMalloc(%llu bytes) for %d qubits: %s", (unsigned long long)bytes,
                nbits, hipGetErrorString(e));
  }
  h->owns_mem = true;
  e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking);
  if (e != hipSuccess) {
    (void)hipFree(h->d_psi);
    delete h;
    return fail(QH_ERR_HIP, "hipStreamCreate: %s", hipGetErrorString(e));
  }
  h->owns_stream = true;
  rc = common_init(h);
  if (rc) {
    qh_destroy(h);
    return rc;
  }
  *out = h;
  return QH_OK;
}

int qh_create_host_mapped(int nbits, int bit_width, int device, qh_handle *out) {
  if (!out) return fail(QH_ERR_ARG, "null out");
  int rc = check_args(nbits, bit_width);
  if (rc) return rc;
  if (nbits > 28) return fail(QH_ERR_ARG, "host-mapped states are for small registers (<= 28 qubits): every gate crosses PCIe");
  rc = select_device(device);
  if (rc) return rc;
  void *host = nullptr, *dev = nullptr;
  const size_t bytes = (size_t)(bit_width == 128 ? 16 : 8) << nbits;
  hipError_t e = hipHostMalloc(&host, bytes, hipHostMallocMapped);
  if (e == hipSuccess) e = hipHostGetDevicePointer(&dev, host, 0);
  if (e != hipSuccess) {
    if (host) (void)hipHostFree(host);
    return fail(QH_ERR_NOMEM, "hipHostMalloc(%zu bytes, mapped): %s", bytes, hipGetErrorString(e));
  }
  memset(host, 0, bytes);
  rc = qh_attach(nbits, bit_width, device, dev, nullptr, out);
  if (rc) {
    (void)hipHostFree(host);
    return rc;
  }
  (*out)->host_psi = host;
  return QH_OK;
}

int qh_host_ptr(qh_handle h, void **host_ptr) {
  if (!h || !host_ptr) return fail(QH_ERR_ARG, "null");
  *host_ptr = h->host_psi;
  return QH_OK;
}

int qh_attach(int nbits, int bit_width, int device, void *device_ptr, void *hip_stream,
              qh_handle *out) {
  if (!out || !device_ptr) return fail(QH_ERR_ARG, "null pointer");
  int rc = check_args(nbits, bit_width);
  if (rc) return rc;
  rc = select_device(device);
  if (rc) return rc;
  auto *h = new qh_state_s;
  h->nloc = h->nglob = nbits;
  h->bw = bit_width;
  h->device = device;
  h->d_psi = device_ptr;
  if (hip_stream) {
    h->stream = (hipStream_t)hip_stream;
  } else {
    hipError_t e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking);
    if (e != hipSuccess) {
      delete h;
      return fail(QH_ERR_HIP, "hipStreamCreate: %s", hipGetErrorString(e));
    }
    h->owns_stream = true;
  }
  rc = common_init(h);
  if (rc) {
    qh_destroy(h);
    return rc;
  }
  *out = h;
  return QH_OK;
}

int qh_create_dry(int nbits, int bit_width, qh_handle *out) {
  if (!out) return fail(QH_ERR_ARG, "null out");
  int rc = check_args(nbits, bit_width);
  if (rc) return rc;
  auto *h = new qh_state_s;
  h->nloc = h->nglob = nbits;
  h->bw = bit_width;
  h->dry = true;
  common_init(h);
  *out = h;
  return QH_OK;
}

int qh_destroy(qh_handle h) {
  if (!h) return QH_OK;
  if (h->dry) (void)qh_comm_destroy(h);
  if (!h->dry) {
    (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    (void)qh_comm_destroy(h);
    if (h->ev0) (void)hipEventDestroy(h->ev0);
    if (h->ev1) (void)hipEventDestroy(h->ev1);
    if (h->ev_read) (void)hipEventDestroy(h->ev_read);
    for (hipEvent_t e : h->laps) (void)hipEventDestroy(e);
    if (h->owns_mem && h->d_psi) (void)hipFree(h->d_psi);
    if (h->d_alt) (void)hipFree(h->d_alt);
    if (h->host_psi) (void)hipHostFree(h->host_psi);
    if (h->owns_stream && h->stream) (void)hipStreamDestroy(h->stream);
  }
  delete h;      // (the scratch members release themselves here: the device is current, the stream drained)
  return QH_OK;
}

int qh_set_shard(qh_handle h, int nbits_global, uint64_t shard_index) {
  if (!h) return fail(QH_ERR_ARG, "null handle");
  if (nbits_global < h->nloc || nbits_global > 62)
    return fail(QH_ERR_ARG, "nbits_global %d < local %d", nbits_global, h->nloc);
  if (nbits_global - h->nloc < 64 && (shard_index >> (nbits_global - h->nloc)) != 0)
    return fail(QH_ERR_ARG, "shard index %llu does not fit %d shard bits",
                (unsigned long long)shard_index, nbits_global - h->nloc);
  h->nglob = nbits_global;
  h->shard = shard_index;
  h->sweep.plans.clear();   // cached plans were made for another shard geometry
  return QH_OK;
}

int qh_device_ptr(qh_handle h, void **ptr) {
  if (!h || !ptr) return fail(QH_ERR_ARG, "null");
  if (!h->dry) {
    // the caller will address amplitudes in physical order through this pointer for as long as it likes: run
    // what is queued, bring the layout back to canonical order, and stop re-laying the state out (a later
    // relayout sweep would swap the two buffers under the caller: ADVICE r2)
    int rc = set_relayout(h, false);
    if (rc) return rc;
  }
  *ptr = h->d_psi;
  return QH_OK;
}
int qh_stream(qh_handle h, void **stream) {
  if (!h || !stream) return fail(QH_ERR_ARG, "null");
  *stream = (void *)h->stream;
  return QH_OK;
}
int qh_nbits(qh_handle h, int *nl, int *ng) {
  if (!h) return fail(QH_ERR_ARG, "null");
  if (nl) *nl = h->nloc;
  if (ng) *ng = h->nglob;
  return QH_OK;
}

int qh_logical_to_phys(qh_handle h, uint64_t logical, uint64_t *phys) {
  if (!h || !phys) return fail(QH_ERR_ARG, "null");
  *phys = to_phys(h, logical);
  return QH_OK;
}
int qh_phys_to_logical(qh_handle h, uint64_t phys, uint64_t *logical) {
  if (!h || !logical) return fail(QH_ERR_ARG, "null");
  *logical = to_logical(h, phys);
  return QH_OK;
}
int qh_get_bitmap(qh_handle h, int32_t *out) {
  if (!h || !out) return fail(QH_ERR_ARG, "null");
  for (int b = 0; b < h->nglob; ++b) out[b] = h->perm[b];
  return QH_OK;
}
int qh_remap_swap(qh_handle h, int a, int b) {
  if (!h) return fail(QH_ERR_ARG, "null");
  if (a < 0 || b < 0 || a >= h->nglob || b >= h->nglob)
    return fail(QH_ERR_BAD_QUBIT, "physical bits %d,%d out of range", a, b);
  int rc = flush_impl(h);
  if (rc) return rc;
  int la = -1, lb = -1;
  for (int l = 0; l < h->nglob; ++l) {
    if (h->perm[l] == a) la = l;
    if (h->perm[l] == b) lb = l;
  }
  std::swap(h->perm[la], h->perm[lb]);
  return QH_OK;
}

// An initialisation replaces every amplitude, so whatever layout relayout sweeps left behind can go: a plain handle (no
// shard bits, no communicator: nobody else has a say in its bit map) starts over in canonical order.  (A state parked by
// the API mirror's pool comes back in the layout its last circuit left; k_init_product then un-permuted every index bit by
// bit: 11.9 ms for a 30-qubit register instead of the 2.9 ms of writing it, tools/probes/single_shot_breakdown.py.)
static void reset_layout_for_init(qh_handle h) {
  if (h->nglob == h->nloc && !h->comm)
    for (int b = 0; b < 64; ++b) h->perm[b] = b;
}

int qh_init_basis(qh_handle h, uint64_t index) {
  if (!h) return fail(QH_ERR_ARG, "null handle");
  if (h->nglob < 64 && (index >> h->nglob)) return fail(QH_ERR_ARG, "basis index out of range");
  h->queue.clear();
  h->poisoned = false;
  reset_layout_for_init(h);
  if (h->dry) return QH_OK;
  HIP_TRY(hipSetDevice(h->device));
  if (h->comm) qh::wait_all_arrivals(&h->comm->arrivals, h->stream);
  const Placed at = place(h, to_phys(h, index));
  HIP_TRY(hipMemsetAsync(h->d_psi, 0, (1ull << h->nloc) * h->amp_bytes(), h->stream));
  if (at.held == h->shard)
    with_real(h, [&](auto x) {
      using R = decltype(x);
      hipLaunchKernelGGL(qh::k_set_one<R>, dim3(1), dim3(1), 0, h->stream, (typename qh::AmpT<R>::type *)h->d_psi, at.local);
    });
  return check_launch(h);
}

int qh_init_product(qh_handle h, int nfactors, const int *nq, const double *const *amps, const uint64_t *basis) {
  if (!h || !nq || nfactors < 1) return fail(QH_ERR_ARG, "null handle / no factors");
  if (nfactors > qh::kMaxFactors) return fail(QH_ERR_ARG, "too many factors (merge small ones on the host)");
  {   // every factor a basis state: the product is ONE basis state (a memset and one amplitude, not a pass of arithmetic)
    bool all_basis = basis != nullptr;
    int total = 0;
    uint64_t index = 0;
    for (int f = 0; all_basis && f < nfactors; ++f) {
      all_basis = (!amps || !amps[f]) && nq[f] >= 1 && nq[f] <= 63 && !(basis[f] >> nq[f]) && total + nq[f] <= 64;
      if (all_basis) { index = nq[f] >= 64 ? basis[f] : ((index << nq[f]) | basis[f]); total += nq[f]; }
    }
    if (all_basis && total == h->nglob) return qh_init_basis(h, index);
  }
  // (validation first: a call that fails must leave the handle -- layout, queue -- exactly as it found it)
  int total = 0;
  uint64_t entries = 0;
  for (int f = 0; f < nfactors; ++f) {
    if (nq[f] < 1 || nq[f] > 63) return fail(QH_ERR_ARG, "factor size out of range");
    total += nq[f];
    const bool is_basis = !amps || !amps[f];
    if (is_basis && !basis) return fail(QH_ERR_ARG, "basis factor without basis[]");
    if (is_basis && (basis[f] >> nq[f])) return fail(QH_ERR_ARG, "basis index out of range");
    if (!is_basis) {
      if (nq[f] > 24) return fail(QH_ERR_ARG, "table factor larger than 2^24 amplitudes");
      entries += 1ull << nq[f];
    }
  }
  if (total != h->nglob) return fail(QH_ERR_ARG, "factor sizes do not add up to the number of qubits");
  if (entries > (1ull << 25)) return fail(QH_ERR_ARG, "factor tables larger than 2^25 amplitudes");
  reset_layout_for_init(h);
  h->queue.clear();
  h->poisoned = false;
  qh::ProductSpec sp{};
  sp.nf = nfactors;
  sp.nglob = h->nglob;
  sp.identity = 1;
  for (int b = 0; b < h->nglob; ++b) {
    sp.perm[b] = (uint8_t)h->perm[b];
    if (h->perm[b] != b) sp.identity = 0;
  }
  if (h->dry) return QH_OK;
  if (h->comm) qh::wait_all_arrivals(&h->comm->arrivals, h->stream);
  std::vector<double> tab(2 * std::max<uint64_t>(entries, 1));
  uint64_t off = 0;
  int shift = h->nglob;
  for (int f = 0; f < nfactors; ++f) {   // f_0 holds the most significant qubits (np.kron order)
    shift -= nq[f];
    sp.shift[f] = (uint8_t)shift;
    sp.nq[f] = (uint8_t)nq[f];
    sp.is_basis[f] = (!amps || !amps[f]) ? 1 : 0;
    if (sp.is_basis[f]) { sp.basis[f] = basis[f]; continue; }
    sp.off[f] = (uint32_t)off;
    memcpy(&tab[2 * off], amps[f], (size_t)16 << nq[f]);
    off += 1ull << nq[f];
  }
  HIP_TRY(hipSetDevice(h->device));
  qh::DeviceBuffer d_tab;
  HIP_TRY(d_tab.reserve(tab.size() * sizeof(double)));
  hipError_t e = hipMemcpyAsync(d_tab.ptr, tab.data(), tab.size() * sizeof(double), hipMemcpyHostToDevice, h->stream);
  if (e == hipSuccess) {
    const uint64_t n = 1ull << h->nloc;
    const uint64_t idx_high = h->shard << h->nloc;
    with_real(h, [&](auto x) {
      using R = decltype(x);
      hipLaunchKernelGGL(qh::k_init_product<R>, dim3(grid_for(n, 1ull << 22)), dim3(256), 0, h->stream,
                         (typename qh::AmpT<R>::type *)h->d_psi, n, idx_high, sp, d_tab.as<double2>());
    });
    e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);   // `tab` and d_tab are released on return
  }
  if (e != hipSuccess) return fail(QH_ERR_HIP, hipGetErrorString(e));
  return QH_OK;
}

int qh_upload(qh_handle h, const void *host, uint64_t offset, uint64_t count) {
  if (!h || !host) return fail(QH_ERR_ARG, "null handle or buffer");
  if (offset + count > (1ull << h->nloc)) return fail(QH_ERR_ARG, "upload range out of bounds");
  if (!h->dry && offset == 0 && count == (1ull << h->nloc)) {
    // the whole shard is replaced: a fresh start -- nothing queued is worth running, a failed flush is forgotten, and a
    // plain handle goes back to canonical order without moving a byte (like the initialisations)
    h->queue.clear();
    h->poisoned = false;
    reset_layout_for_init(h);
  }
  int rc = enter(h);
  if (rc == QH_OK) rc = canonicalize(h);
  if (rc) return rc;
  HIP_TRY(hipMemcpyAsync((char *)h->d_psi + offset * h->amp_bytes(), host, count * h->amp_bytes(),
                         hipMemcpyHostToDevice, h->stream));
  return wait_stream(h, h->stream, "qh_upload");
}

int qh_download(qh_handle h, void *host, uint64_t offset, uint64_t count) {
  if (!h || !host) return fail(QH_ERR_ARG, "null handle or buffer");
  if (offset + count > (1ull << h->nloc)) return fail(QH_ERR_ARG, "download range out of bounds");
  int rc = enter(h);
  if (rc == QH_OK) rc = canonicalize(h);
  if (rc) return rc;
  return read_back(h, host, (const char *)h->d_psi + offset * h->amp_bytes(), count * h->amp_bytes(), "qh_download");
}

int qh_amplitude(qh_handle h, uint64_t logical_index, double out[2]) {
  if (!h || !out) return fail(QH_ERR_ARG, "null handle or out");
  if (h->nglob < 64 && (logical_index >> h->nglob)) return fail(QH_ERR_ARG, "index out of range");
  int rc = enter(h);
  if (rc) return rc;
  const Placed at = place(h, to_phys(h, logical_index));
  if (at.held != h->shard) return fail(QH_ERR_NONLOCAL, "amplitude %llu lives on shard %llu", (unsigned long long)logical_index, (unsigned long long)at.held);
  return with_real(h, [&](auto x) {
    decltype(x) v[2];
    const int rc = read_back(h, v, (const char *)h->d_psi + at.local * sizeof v, sizeof v, "qh_amplitude");
    if (rc) return rc;
    out[0] = v[0];
    out[1] = v[1];
    return (int)QH_OK;
  });
}

int qh_apply_bits(qh_handle h, uint64_t ctl_mask, int tgt_bit, const double gate[8]) {
  return apply_logical(h, ctl_mask, tgt_bit, gate);
}

int qh_apply1(qh_handle h, int tgt, const double gate[8]) {
  if (!h) return fail(QH_ERR_ARG, "null handle");
  const int p = h->nglob - tgt - 1;  // xgates.cc:26
  if (p < 0 || p >= h->nglob)
    return fail(QH_ERR_BAD_QUBIT, "apply1: qubit %d out of range for %d qubits", tgt, h->nglob);
  return apply_logical(h, 0, p, gate);
}

int qh_applyc(qh_handle h, int ctl, int tgt, const double gate[8]) {
  if (!h) return fail(QH_ERR_ARG, "null handle");
  const int p = h->nglob - tgt - 1;  // xgates.cc:48
  if (p < 0 || p >= h->nglob)
    return fail(QH_ERR_BAD_QUBIT, "applyc: target qubit %d out of range for %d qubits", tgt, h->nglob);
  const int c = ref_ctl_bit(h->nglob, ctl, p);  // xgates.cc:49,58-59
  if (c == -2)
    return fail(QH_ERR_BAD_QUBIT, "applyc: control qubit %d out of range for %d qubits", ctl, h->nglob);
  if (c == -1) {  // out-of-range (negative) control whose predicate is never true
    h->stats.gates_submitted++;
    h->stats.gates_noop++;
    return QH_OK;
  }
  if (c == p) return fail(QH_ERR_SAME_QUBIT, "applyc: control == target (qubit %d)", tgt);
  return apply_logical(h, 1ull << c, p, gate);
}

int qh_set_fusion(qh_handle h, int level) {
  if (!h) return fail(QH_ERR_ARG, "null handle");
  if (level != QH_FUSE_OFF && level != QH_FUSE_SWEEP) return fail(QH_ERR_ARG, "fusion level %d", level);
  int rc = flush_impl(h);
  h->fusion = level;
  return rc;
}

int qh_flush(qh_handle h) {
  if (!h) return fail(QH_ERR_ARG, "null handle");
  return flush_impl(h);
}

int qh_pending_gates(qh_handle h, uint64_t *count) {
  if (!h || !count) return fail(QH_ERR_ARG, "null");
  *count = h->queue.size();
  return QH_OK;
}

int qh_discard_pending(qh_handle h) {
  if (!h) return fail(QH_ERR_ARG, "null handle");
  h->queue.clear();
  return QH_OK;
}

int qh_sync(qh_handle h) {
  if (!h) return fail(QH_ERR_ARG, "null handle");
  if (h->dry) {
    return flush_impl(h);
  }
  HIP_TRY(hipSetDevice(h->device));
  int rc = flush_impl(h);
  if (rc) return rc;
  return wait_stream(h, h->stream, "qh_sync");
}

int qh_set_relayout(qh_handle h, int on, int *actual) {
  if (!h) return fail(QH_ERR_ARG, "null handle");
  return set_relayout(h, on != 0, actual);
}

int qh_apply_stream(qh_handle h, uint64_t count, const int32_t *ops, const double *gates) {
  if (!h || (count && (!ops || !gates))) return fail(QH_ERR_ARG, "null");
  for (uint64_t k = 0; k < count; ++k) {
    const int32_t c = ops[2 * k], t = ops[2 * k + 1];
    const int rc = c == INT32_MIN ? qh_apply1(h, t, gates + 8 * k) : qh_applyc(h, c, t, gates + 8 * k);
    if (rc) {
      g_err = "gate " + std::to_string(k) + " of the stream: " + g_err;
      return rc;
    }
  }
  return QH_OK;
}

// sum of |amplitude|^2 over the local indices i with (i & mask) == want
static int masked_norm2(qh_handle h, uint64_t mask, uint64_t want, double *out) {
  const uint64_t n = 1ull << h->nloc;
  const unsigned nblk = grid_for(n, 4096);
  SlabSum sum{h};                                           // one slab row per block, folded in block order: no atomics
  HIP_TRY(sum.reserve(std::max<uint64_t>(nblk, 8), 1, 1));
  with_real(h, [&](auto x) {
    using R = decltype(x);
    hipLaunchKernelGGL(qh::k_norm2<R>, dim3(nblk), dim3(256), 0, h->stream,
                       (const typename qh::AmpT<R>::type *)h->d_psi, n, mask, want, sum.slab);
  });
  sum.fold(nblk, 1, 1);
  return sum.get(out, 1, "norm2 reader");
}

int qh_norm2(qh_handle h, double *out) {
  if (!h || !out) return fail(QH_ERR_ARG, "null handle or out");
  const int rc = enter(h);
  if (rc) return rc;
  return masked_norm2(h, 0ull, 0ull, out);
}

int qh_prob_bit_value(qh_handle h, int logical_bit, int value, double *p) {
  if (!h || !p) return fail(QH_ERR_ARG, "null handle or out");
  if (logical_bit < 0 || logical_bit >= h->nglob) return fail(QH_ERR_BAD_QUBIT, "bit %d", logical_bit);
  const int rc = enter(h);
  if (rc) return rc;
  const Placed b = place_bit(h, logical_bit);
  if (b.held && ((h->shard & b.held) != 0) != (value != 0)) {   // held by the shard index at the other value
    *p = 0.0;
    return QH_OK;
  }
  return masked_norm2(h, b.local, value ? b.local : 0ull, p);
}

int qh_prob_bit(qh_handle h, int logical_bit, double *p1) { return qh_prob_bit_value(h, logical_bit, 1, p1); }

}  // extern "C"

// ---- argmax (state.py:60-78 maxprob: the FIRST basis state, in logical order, with the largest probability) ----------
namespace {
// The tables of the kernels that report LOGICAL indices, as the layout is now: physical -> logical of the local bits with
// the logical bits the shard index holds at 1 on this shard (p2l), and the inverse for the one kernel that walks in logical
// order (l2p).
struct LocalBits {
  qh::IndexMap p2l{};
  qh::BitMap l2p{};
  bool mapped = false;      // some local bit is off its canonical position
};
LocalBits local_bits(const qh_state_s *h) {
  LocalBits lb;
  lb.l2p.n = h->nloc;
  for (int b = 0; b < h->nglob; ++b) {
    const Placed at = place_bit(h, b);
    if (at.held) {
      if (h->shard & at.held) lb.p2l.shard_logical |= 1ull << b;
      continue;
    }
    const int p = h->perm[b];
    lb.p2l.to[p] = (uint8_t)b;
    lb.l2p.to[b] = (uint8_t)p;
    lb.mapped |= p != b;
  }
  return lb;
}
// The last sweep of the flush left per-unit maxima: the largest of them is the answer's probability; the answer's index is the
// smallest logical index that has it.  Few units hold it (a peaked state: Grover, most algorithms' outputs): those units are
// scanned.  Many do (a flat state: a QFT's output ties at a tenth of its amplitudes): the first of them in LOGICAL order is
// near the start -- growing prefixes of the logical index range are scanned until one has a hit.  Exact either way.
int argmax_from_tilemax(qh_state_s *h, const qh::TileMaxOut &tm, const LocalBits &lb, uint64_t *logical, double *prob, bool *found) {
  *found = false;
  const unsigned grid = grid_for(tm.nunits, kRedBlocks);
  hipLaunchKernelGGL(qh::k_tmax_reduce, dim3(grid), dim3(256), 0, h->stream, (const uint64_t *)tm.buf, tm.nunits, h->d_redi());
  std::vector<uint64_t> part(grid);
  int rc = read_back(h, part.data(), h->d_redi(), grid * sizeof(uint64_t));
  if (rc) return rc;
  uint64_t top = 0;
  for (uint64_t v : part) top = std::max(top, v);
  double want;
  memcpy(&want, &top, 8);
  unsigned long long *ids = (unsigned long long *)h->d_redi();      // (kRedBlocks u64: room for 1 + qh::kTmaxIds + the result)
  static_assert(kRedBlocks >= 2 + qh::kTmaxIds, "reduction scratch");
  HIP_TRY(hipMemsetAsync(ids, 0, 8, h->stream));
  HIP_TRY(hipMemsetAsync(ids + 1 + qh::kTmaxIds, 0xff, 8, h->stream));
  hipLaunchKernelGGL(qh::k_tmax_collect, dim3(grid), dim3(256), 0, h->stream, (const uint64_t *)tm.buf, tm.nunits, top, ids);
  unsigned long long cnt = 0;
  if ((rc = read_back(h, &cnt, ids, 8))) return rc;
  if (cnt == 0) return QH_OK;
  if (cnt > qh::kTmaxIds) {
    const uint64_t n = 1ull << h->nloc;
    uint64_t l0 = 0;
    for (uint64_t l1 = std::min<uint64_t>(n, 1ull << 16); l0 < n; l0 = l1, l1 = std::min<uint64_t>(n, l1 << 6)) {
      with_real(h, [&](auto x) {
        using A = typename qh::AmpT<decltype(x)>::type;
        hipLaunchKernelGGL(qh::k_prefix_scan<A>, dim3(grid_for(l1 - l0, 1u << 16)), dim3(256), 0, h->stream, (const A *)h->d_psi, l0, l1, want,
                           lb.l2p, ids + 1 + qh::kTmaxIds);
      });
      unsigned long long hit = ~0ull;
      if ((rc = read_back(h, &hit, ids + 1 + qh::kTmaxIds, 8))) return rc;
      if (hit != ~0ull) {
        *logical = hit;
        *prob = want;
        *found = true;
        return QH_OK;
      }
    }
    return QH_OK;      // (cannot happen)
  }
  with_real(h, [&](auto x) {
    using A = typename qh::AmpT<decltype(x)>::type;
    hipLaunchKernelGGL(qh::k_tmax_scan<A>, dim3((unsigned)cnt), dim3(256), 0, h->stream, (const A *)h->d_psi, ids, tm.ins, tm.tile_mask,
                       __builtin_popcountll(tm.tile_mask), want, lb.p2l, h->nloc, ids + 1 + qh::kTmaxIds);
  });
  unsigned long long li = ~0ull;
  if ((rc = read_back(h, &li, ids + 1 + qh::kTmaxIds, 8))) return rc;
  if (li == ~0ull) return QH_OK;       // (cannot happen: a unit's maximum is one of its amplitudes) -> the full pass decides
  *logical = li;
  *prob = want;
  *found = true;
  return QH_OK;
}
}  // namespace

extern "C" int qh_argmax(qh_handle h, uint64_t *phys_index, double *prob) {
  if (!h || !phys_index || !prob || h->dry) return fail(QH_ERR_ARG, "null/dry");
  HIP_TRY(hipSetDevice(h->device));
  // the flush in front of the reader: its last sweep may leave the maximum of every unit it stores (no communicator)
  qh::TileMaxOut tm;
  if (h->fusion == QH_FUSE_SWEEP && !h->comm && !h->queue.empty() && qh::sweep_supported(h->nloc, h->bw) &&
      h->nloc >= qh::kLaneBits + 3 &&      // (sweep_supported() admits nloc = kLaneBits + 2: no shift by a negative count below)
      env_int("QH_FUSED_ARGMAX", 1) != 0) {
    const uint64_t need = 1ull << (h->nloc - qh::kLaneBits - 3);       // units of a three-register-bit tile (a sweep without dense gates); plans
                                                                       // with dense gates use five: a flush that wants more entries takes the full pass
    (void)h->tmax.reserve(need * 8);      // (no room: the full pass decides)
    tm.buf = h->tmax.ptr;
    tm.cap = h->tmax.cap / 8;
  }
  int rc = flush_impl(h, nullptr, tm.buf ? &tm : nullptr);
  if (rc) return rc;
  // ties go to the smallest LOGICAL index, whatever layout relayout sweeps have left the state in
  const LocalBits lb = local_bits(h);
  uint64_t logical = 0;
  bool found = false;
  if (tm.valid) {
    rc = argmax_from_tilemax(h, tm, lb, &logical, prob, &found);
    if (rc) return rc;
  }
  if (!found) {
    const uint64_t n = 1ull << h->nloc;
    const unsigned grid = grid_for(n, kRedBlocks);
    with_real(h, [&](auto x) {
      using A = typename qh::AmpT<decltype(x)>::type;
      if (lb.mapped) hipLaunchKernelGGL((qh::k_argmax_logical<A, true>), dim3(grid), dim3(256), 0, h->stream, (const A *)h->d_psi, n, lb.p2l, h->d_red(), h->d_redi());
      else hipLaunchKernelGGL((qh::k_argmax_logical<A, false>), dim3(grid), dim3(256), 0, h->stream, (const A *)h->d_psi, n, lb.p2l, h->d_red(), h->d_redi());
    });
    std::vector<double> bp(grid);
    std::vector<uint64_t> bi(grid);
    HIP_TRY(hipMemcpyAsync(bp.data(), h->d_red(), grid * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if ((rc = read_back(h, bi.data(), h->d_redi(), grid * sizeof(uint64_t)))) return rc;
    double best = -1.0;
    uint64_t idx = 0;
    for (unsigned k = 0; k < grid; ++k)
      if (bp[k] > best || (bp[k] == best && bi[k] < idx)) { best = bp[k]; idx = bi[k]; }
    logical = idx;
    *prob = best;
  }
  // the caller gets the PHYSICAL index of the shard-local amplitude (qh_phys_to_logical turns it back)
  *phys_index = (h->shard << h->nloc) | place(h, to_phys(h, logical)).local;
  return QH_OK;
}

extern "C" {
int qh_scale(qh_handle h, double re, double im) {
  if (!h) return fail(QH_ERR_ARG, "null handle");
  const int rc = enter(h);
  if (rc) return rc;
  const qh::BitIns ins{};
  with_real(h, [&](auto x) { launch_diag<decltype(x)>(h, 1ull << h->nloc, -1, ins, 1, 0, re, im); });
  return check_launch(h);
}

int qh_project_bit(qh_handle h, int logical_bit, int value) {
  if (!h) return fail(QH_ERR_ARG, "null handle");
  if (logical_bit < 0 || logical_bit >= h->nglob) return fail(QH_ERR_BAD_QUBIT, "bit %d", logical_bit);
  const int rc = enter(h);
  if (rc) return rc;
  const Placed b = place_bit(h, logical_bit);
  if (b.held) {      // a shard whose index contradicts the value is zeroed whole
    if (((h->shard & b.held) != 0) != (value != 0))
      HIP_TRY(hipMemsetAsync(h->d_psi, 0, (1ull << h->nloc) * h->amp_bytes(), h->stream));
    return QH_OK;
  }
  const qh::BitIns ins = make_ins(value ? 0ull : b.local, value ? h->perm[logical_bit] : -1);
  const uint64_t nwork = 1ull << (h->nloc - 1);
  with_real(h, [&](auto x) {
    using R = decltype(x);
    hipLaunchKernelGGL(qh::k_project<R>, dim3(grid_for(nwork, 1u << 20)), dim3(256), 0, h->stream, (typename qh::AmpT<R>::type *)h->d_psi, nwork, ins);
  });
  return check_launch(h);
}
}  // extern "C"

namespace {

// The next slot of a staged upload, once the kernel that last read it has finished (watched handles poll: wait_event).
template <int N>
int acquire(qh_state_s *h, qh::StagedUpload<N> &up, size_t bytes_per_slot, const char *who, char **host, char **dev, unsigned *slot) {
  if (hipEvent_t e = up.busy()) {
    const int rc = wait_event(h, e, who);
    if (rc) return rc;
  }
  HIP_TRY(up.acquire(bytes_per_slot, host, dev, slot));
  return QH_OK;
}

// Copies the caller's matrix (4^k complex128) into the next staging slot, converted to the state's width, and uploads
// it on the handle's stream.  *dev = the device copy; *slot = the slot whose event goes behind the kernel.
int stage_matrix(qh_state_s *h, int k, const double *m, const void **dev, unsigned *slot) {
  char *host = nullptr, *d = nullptr;
  const int rc = acquire(h, h->mat, kMatSlotBytes, "qh_apply_matrix", &host, &d, slot);
  if (rc) return rc;
  const size_t n = (size_t)1 << (2 * k);
  size_t bytes = n * 16;
  if (h->bw == 128) {
    memcpy(host, m, bytes);
  } else {
    float *f = (float *)host;
    for (size_t i = 0; i < 2 * n; ++i) f[i] = (float)m[i];
    bytes = n * 8;
  }
  HIP_TRY(hipMemcpyAsync(d, host, bytes, hipMemcpyHostToDevice, h->stream));
  *dev = d;
  return QH_OK;
}

template <typename R, int K>
void launch_dense_k(qh_state_s *h, const qh::DenseArgs &a, const void *mat) {
  using A = typename qh::AmpT<R>::type;
  if constexpr (K <= 4) {
    constexpr int U = K == 1 ? 4 : K == 2 ? 2 : 1;   // >= 8 amplitude loads in flight per thread
    hipLaunchKernelGGL((qh::k_dense_reg<R, K, U>), dim3(pick_grid(a.nwork, 256 * U)), dim3(256), 0, h->stream, (A *)h->d_psi,
                       (const A *)mat, a);
  } else {
    // every block stages M in LDS first: a grid of a few blocks per CU, grid-stride over the groups
    const unsigned grid = (unsigned)std::min<uint64_t>(pick_grid(a.nwork << (K - 4), 256), 2048);
    hipLaunchKernelGGL((qh::k_dense_split<R, K>), dim3(grid), dim3(256), 0, h->stream, (A *)h->d_psi, (const A *)mat, a);
  }
}

template <typename R>
void launch_dense(qh_state_s *h, int k, const qh::DenseArgs &a, const void *mat) {
  switch (k) {
    case 1: return launch_dense_k<R, 1>(h, a, mat);
    case 2: return launch_dense_k<R, 2>(h, a, mat);
    case 3: return launch_dense_k<R, 3>(h, a, mat);
    case 4: return launch_dense_k<R, 4>(h, a, mat);
    case 5: return launch_dense_k<R, 5>(h, a, mat);
    default: return launch_dense_k<R, 6>(h, a, mat);
  }
}

}  // namespace

extern "C" {

int qh_apply_matrix(qh_handle h, int k, const int32_t *bits, uint64_t ctl_mask, const double *matrix) {
  if (!h || !bits || !matrix) return fail(QH_ERR_ARG, "apply_matrix: null handle, bits or matrix");
  if (k < 1 || k > qh::kMaxDenseBits) return fail(QH_ERR_ARG, "apply_matrix: k = %d outside [1,%d]", k, qh::kMaxDenseBits);
  if (h->nglob < 64 && (ctl_mask >> h->nglob))
    return fail(QH_ERR_BAD_QUBIT, "apply_matrix: control mask 0x%llx has bits >= %d", (unsigned long long)ctl_mask, h->nglob);
  uint64_t tmask = 0;
  int rc = check_bit_list(h, "apply_matrix", k, bits, &tmask);
  if (rc) return rc;
  if (ctl_mask & tmask)
    return fail(QH_ERR_SAME_QUBIT, "apply_matrix: control and target share bits 0x%llx", (unsigned long long)(ctl_mask & tmask));
  // (a logical bit stays local or in the shard index whatever the relayout sweeps do)
  const int nlc = __builtin_popcountll(place(h, to_phys(h, ctl_mask)).local);
  if (k + nlc > qh::kMaxIns)
    return fail(QH_ERR_ARG, "apply_matrix: %d targets + %d local controls exceed the %d bits one index enumeration inserts (kMaxIns)",
                k, nlc, qh::kMaxIns);
  for (int j = 0; j < k; ++j)
    if (h->perm[bits[j]] >= h->nloc)
      return fail(QH_ERR_NONLOCAL, "apply_matrix: logical bit %d is held by the shard index (physical bit %d, local bits: %d); "
                  "exchange first", bits[j], h->perm[bits[j]], h->nloc);
  if ((rc = enter(h))) return rc;          // a barrier: what is queued runs first, on whatever layout it leaves
  const Placed ctl = place(h, to_phys(h, ctl_mask));
  if ((h->shard & ctl.held) != ctl.held) {   // a shard-bit control that is 0 on this shard (met: dropped)
    h->stats.gates_submitted++;
    h->stats.gates_noop++;
    return QH_OK;
  }
  const uint64_t cm_all = ctl.local;         // physical local control bits
  const LowSplit low = split_low(h, cm_all);
  const uint64_t cm = low.cm;
  qh::DenseArgs a{};
  a.lowpred = low.lowpred;
  uint64_t ptmask = 0;
  for (int j = 0; j < k; ++j) {
    a.t[j] = h->perm[bits[j]];
    ptmask |= 1ull << a.t[j];
  }
  a.ins.ones = cm;
  for (int b = 0; b < 64; ++b)
    if (((cm | ptmask) >> b) & 1ull) a.ins.pos[a.ins.n++] = b;
  a.nwork = 1ull << (h->nloc - k - __builtin_popcountll(cm));
  const void *dmat = nullptr;
  unsigned slot = 0;
  if ((rc = stage_matrix(h, k, matrix, &dmat, &slot))) return rc;
  with_real(h, [&](auto x) { launch_dense<decltype(x)>(h, k, a, dmat); });
  if ((rc = check_launch(h))) return rc;
  HIP_TRY(h->mat.commit(h->stream, slot));
  h->stats.gates_submitted++;
  count_kernel(h, 1ull << (h->nloc - __builtin_popcountll(cm_all)), a.nwork << k);
  return QH_OK;
}

}  // extern "C"

// ---- table-selected gates: qh_apply_mux, qh_apply_diag (kernels_mux.hip.h) --------------------------------------------
namespace {

// What a call makes of its k selection bits on this handle: the bits held by the shard index are fixed (`fixed`: their
// table bits that are 1 on this shard), the others keep their order and number the entries of the restricted table
// (`tbits`: the table bits they had); `g` gathers the restricted index from a physical amplitude index.
struct TabPlan {
  qh::TabGather g{};
  int kl = 0;
  uint32_t fixed = 0, tbits = 0;
  uint64_t local_pos = 0;      // physical positions of the local selection bits
};

TabPlan plan_table(const qh_state_s *h, int k, const int32_t *bits) {
  TabPlan t;
  const SplitBits sb = split_bits(h, k, bits);
  t.fixed = (uint32_t)sb.held_ones;
  t.kl = (int)sb.local.size();
  for (const auto &pj : sb.local) {
    t.tbits |= 1u << pj.second;
    t.local_pos |= 1ull << pj.first;
  }
  std::vector<std::pair<int, int>> loc = sb.local;       // (physical position, bit of the restricted index)
  for (auto &pj : loc) pj.second = __builtin_popcount(t.tbits & ((1u << pj.second) - 1u));
  for (size_t i = 0; i < loc.size();) {       // a run: adjacent positions that feed adjacent table bits
    size_t e = i + 1;
    while (e < loc.size() && loc[e].first == loc[i].first + (int)(e - i) && loc[e].second == loc[i].second + (int)(e - i)) ++e;
    t.g.run[t.g.n++] = (uint32_t)loc[i].first | ((uint32_t)loc[i].second << 8) | ((uint32_t)(e - i) << 16);
    i = e;
  }
  return t;
}

// The restricted table (2^kl entries of C complex numbers, picked from the caller's 2^k) in the state's width, into the
// pinned staging buffer and from there, on the handle's stream, into the device table.  One buffer of each: the
// previous call's kernel must have read its table before the staging buffer is written again.
int stage_table(qh_state_s *h, const TabPlan &t, int C, const double *src, const void **dev) {
  const size_t nent = (size_t)1 << t.kl, elem = h->bw == 128 ? 16 : 8, bytes = nent * C * elem;
  size_t cap = 64u << 10;
  while (cap < bytes) cap *= 2;
  char *host = nullptr, *d = nullptr;
  unsigned slot = 0;
  const int rc = acquire(h, h->tab, cap, "qh_apply_mux/diag", &host, &d, &slot);
  if (rc) return rc;
  for (size_t s = 0; s < nent; ++s) {
    uint32_t full = t.fixed;                    // entry s of the restricted table = entry `full` of the caller's
    for (uint32_t m = t.tbits, r = (uint32_t)s; m; m &= m - 1, r >>= 1)
      if (r & 1u) full |= m & (~m + 1u);
    const double *e = src + (size_t)full * C * 2;
    if (h->bw == 128) memcpy(host + s * C * 16, e, (size_t)C * 16);
    else
      for (int i = 0; i < 2 * C; ++i) ((float *)host)[s * C * 2 + i] = (float)e[i];
  }
  HIP_TRY(hipMemcpyAsync(d, host, bytes, hipMemcpyHostToDevice, h->stream));
  *dev = d;
  return QH_OK;
}

// lane_pos: the index positions that vary with the lane inside one wave row of the kernel that will run
int pick_tier(const TabPlan &t, uint64_t lane_pos, size_t table_bytes) {
  if (!(t.local_pos & lane_pos)) return qh::TAB_UNIFORM;
  return table_bytes <= qh::kTabLdsBytes ? qh::TAB_LDS : qh::TAB_GLOBAL;
}

// tiles of 64 * U work items, one per wave, four waves per block; LDS blocks stage the table first and grid-stride
unsigned tab_grid(uint64_t nwork, int U, int tier) {
  const unsigned g = pick_grid(nwork, 256 * U);
  return tier == qh::TAB_LDS ? std::min(g, 2048u) : g;
}

template <typename R, int TIER>
void launch_tab_tier(qh_state_s *h, int kind, const qh::TabArgs &a, const void *tab, size_t lds) {
  using A = typename qh::AmpT<R>::type;
  const size_t sm = TIER == qh::TAB_LDS ? lds : 0;
  if (kind == 0)
    hipLaunchKernelGGL((qh::k_mux_pair<R, TIER>), dim3(tab_grid(a.nwork, 4, TIER)), dim3(256), sm, h->stream, (A *)h->d_psi, (const A *)tab, a);
  else if (kind == 1)
    hipLaunchKernelGGL((qh::k_mux_line<R, TIER>), dim3(tab_grid(a.nwork, 8, TIER)), dim3(256), sm, h->stream, (A *)h->d_psi, (const A *)tab, a);
  else
    hipLaunchKernelGGL((qh::k_diag_tab<R, TIER>), dim3(tab_grid(a.nwork, 16, TIER)), dim3(256), sm, h->stream, (A *)h->d_psi, (const A *)tab, a);
}

// kind: 0 k_mux_pair, 1 k_mux_line, 2 k_diag_tab
template <typename R>
void launch_tab(qh_state_s *h, int kind, int tier, const qh::TabArgs &a, const void *tab, size_t lds) {
  if (tier == qh::TAB_UNIFORM) launch_tab_tier<R, qh::TAB_UNIFORM>(h, kind, a, tab, lds);
  else if (tier == qh::TAB_LDS) launch_tab_tier<R, qh::TAB_LDS>(h, kind, a, tab, lds);
  else launch_tab_tier<R, qh::TAB_GLOBAL>(h, kind, a, tab, lds);
}

// argument checks shared by the two calls: the target of a mux (has_tgt) must not be among the bits
int check_tab_bits(const qh_state_s *h, const char *who, int k, const int32_t *bits, bool has_tgt, int extra) {
  if (k < 0 || k > qh::kMaxMuxBits) return fail(QH_ERR_ARG, "%s: k = %d outside [0,%d]", who, k, qh::kMaxMuxBits);
  if (k > 0 && !bits) return fail(QH_ERR_ARG, "%s: null bit list", who);
  if (has_tgt && (extra < 0 || extra >= h->nglob)) return fail(QH_ERR_BAD_QUBIT, "%s: target bit %d out of range [0,%d)", who, extra, h->nglob);
  uint64_t seen = 0;
  const int rc = check_bit_list(h, who, k, bits, &seen);
  if (rc) return rc;
  if (has_tgt && ((seen >> extra) & 1ull)) return fail(QH_ERR_SAME_QUBIT, "%s: target bit %d is among the selection bits", who, extra);
  return QH_OK;
}

// the tail of both calls: stage, launch one kernel, record the event, count
int run_tab(qh_state_s *h, int kind, const TabPlan &t, uint64_t lane_pos, int C, const double *src, qh::TabArgs a) {
  const size_t bytes = ((size_t)C << t.kl) * h->amp_bytes();
  const int tier = pick_tier(t, lane_pos, bytes);
  a.g = t.g;
  a.nent = 1u << t.kl;
  const void *dtab = nullptr;
  int rc = stage_table(h, t, C, src, &dtab);
  if (rc) return rc;
  with_real(h, [&](auto x) { launch_tab<decltype(x)>(h, kind, tier, a, dtab, bytes); });
  if ((rc = check_launch(h))) return rc;
  HIP_TRY(h->tab.commit(h->stream, 0));
  h->stats.gates_submitted++;
  count_kernel(h, 1ull << h->nloc, 1ull << h->nloc);
  return QH_OK;
}

}  // namespace

extern "C" {

int qh_apply_mux(qh_handle h, int k, const int32_t *sel_bits, int tgt_bit, const double *gates) {
  if (!h || !gates) return fail(QH_ERR_ARG, "apply_mux: null handle or gates");
  int rc = check_tab_bits(h, "apply_mux", k, sel_bits, true, tgt_bit);
  if (rc) return rc;
  // (a logical bit stays local or in the shard index whatever the relayout sweeps do)
  if (h->perm[tgt_bit] >= h->nloc)
    return fail(QH_ERR_NONLOCAL, "apply_mux: target bit %d is held by the shard index (physical bit %d, local bits: %d); exchange first",
                tgt_bit, h->perm[tgt_bit], h->nloc);
  if ((rc = enter(h))) return rc;          // a barrier: what is queued runs first, on whatever layout it leaves
  const TabPlan t = plan_table(h, k, sel_bits);
  qh::TabArgs a{};
  a.p = h->perm[tgt_bit];
  if (a.p < 3) {                           // inside the line: one amplitude per lane
    a.nwork = 1ull << h->nloc;
    return run_tab(h, 1, t, 0x3full, 4, gates, a);
  }
  a.nwork = 1ull << (h->nloc - 1);
  const uint64_t low = (1ull << a.p) - 1ull;
  return run_tab(h, 0, t, ((0x3full & ~low) << 1) | (0x3full & low), 4, gates, a);
}

int qh_apply_diag(qh_handle h, int k, const int32_t *bits, const double *values) {
  if (!h || !values) return fail(QH_ERR_ARG, "apply_diag: null handle or values");
  int rc = check_tab_bits(h, "apply_diag", k, bits, false, 0);
  if (rc) return rc;
  if ((rc = enter(h))) return rc;
  const TabPlan t = plan_table(h, k, bits);
  qh::TabArgs a{};
  a.nwork = 1ull << h->nloc;
  return run_tab(h, 2, t, 0x3full, 1, values, a);
}

}  // extern "C"

// ---- register permutations: qh_apply_perm, qh_perm_plan (kernels_perm.hip.h, perm_plan.h) -----------------------------
namespace {

// The argument checks both calls share, then the tile (perm_plan.h) on the bit map as it is now.
int plan_perm_call(const qh_state_s *h, const char *who, int k, const int32_t *bits, uint64_t ctl_mask, qh_perm_tiles *out) {
  if (k < 1 || k > QH_PERM_MAX_BITS) return fail(QH_ERR_ARG, "%s: k = %d outside [1,%d]", who, k, QH_PERM_MAX_BITS);
  if (h->nglob < 64 && (ctl_mask >> h->nglob))
    return fail(QH_ERR_BAD_QUBIT, "%s: control mask 0x%llx has bits >= %d", who, (unsigned long long)ctl_mask, h->nglob);
  uint64_t rmask = 0;
  const int rc = check_bit_list(h, who, k, bits, &rmask);
  if (rc) return rc;
  if (ctl_mask & rmask)
    return fail(QH_ERR_SAME_QUBIT, "%s: control and register share bits 0x%llx", who, (unsigned long long)(ctl_mask & rmask));
  // (a logical bit stays local or in the shard index whatever the relayout sweeps do)
  int pos[QH_PERM_MAX_BITS];
  for (int j = 0; j < k; ++j) {
    pos[j] = h->perm[bits[j]];
    if (pos[j] >= h->nloc)
      return fail(QH_ERR_NONLOCAL, "%s: register bit %d is held by the shard index (physical bit %d, local bits: %d); exchange first",
                  who, bits[j], pos[j], h->nloc);
  }
  const Placed ctl = place(h, to_phys(h, ctl_mask));
  qh::plan_perm_tiles(h->nloc, h->bw, k, pos, ctl.local, out);
  out->k = (uint32_t)k;
  out->ctl_met = (h->shard & ctl.held) == ctl.held;
  return QH_OK;
}

// `bytes` of table through the handle's staging pair (the one qh_apply_mux / qh_apply_diag use)
int stage_perm_table(qh_state_s *h, const void *src, size_t bytes, const void **dev) {
  size_t cap = 64u << 10;
  while (cap < bytes) cap *= 2;
  char *host = nullptr, *d = nullptr;
  unsigned slot = 0;
  const int rc = acquire(h, h->tab, cap, "qh_apply_perm", &host, &d, &slot);
  if (rc) return rc;
  memcpy(host, src, bytes);
  HIP_TRY(hipMemcpyAsync(d, host, bytes, hipMemcpyHostToDevice, h->stream));
  *dev = d;
  return QH_OK;
}

// a block may declare more than 64 KiB of LDS only after the kernel has been told so (on the device that is current)
template <typename R> int allow_big_lds() {
  const hipError_t e =
      hipFuncSetAttribute((const void *)qh::k_perm_lds<R>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 << 10);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    return fail(QH_ERR_HIP, "apply_perm: hipFuncSetAttribute(MaxDynamicSharedMemorySize): %s", hipGetErrorString(e));
  }
  return QH_OK;
}

int run_perm_lds(qh_state_s *h, const qh_perm_tiles &t, const std::vector<uint32_t> &inv) {
  const int k = (int)t.k;
  uint8_t ranks[QH_PERM_MAX_BITS];
  memcpy(ranks, t.reg_rank, sizeof ranks);
  std::sort(ranks, ranks + k);
  qh::PermArgs a{};
  a.g.n = qh::perm_runs(k, ranks, a.g.run);
  a.tile_mask = t.tile_mask;
  a.rest_mask = h->local_mask() & ~t.tile_mask & ~t.ctl_out;
  a.ctl_out = t.ctl_out;
  a.ntiles = t.ntiles - t.tiles_skipped;
  a.m = t.tile_bits;
  a.nent = 1u << k;
  for (int p = 0, r = 0; p < h->nloc; ++p) {
    if (!((t.tile_mask >> p) & 1ull)) continue;
    if ((t.reg_mask >> p) & 1ull) a.reg_tile |= 1u << r;
    if ((t.ctl_in >> p) & 1ull) a.ctl_tile |= 1u << r;
    ++r;
  }
  std::vector<uint16_t> tab(a.nent);
  for (uint32_t c = 0; c < a.nent; ++c) tab[c] = (uint16_t)qh::perm_deposit(inv[c], k, ranks);
  const size_t lds = (size_t)t.lds_bytes + tab.size() * sizeof(uint16_t);
  const uint64_t nitems = t.lds_bytes / 16;
  unsigned threads = 64;                                   // four items per thread (eight in the largest tiles), one to sixteen waves
  while (threads < 1024 && threads * 4ull < nitems) threads *= 2;
  if ((uint64_t)threads * qh::kPermItems < nitems) return fail(QH_ERR_ARG, "apply_perm: a tile of %llu items", (unsigned long long)nitems);
  int rc = QH_OK;
  if (lds > (64u << 10)) with_real(h, [&](auto x) { rc = allow_big_lds<decltype(x)>(); });
  if (rc) return rc;
  const void *dtab = nullptr;
  if ((rc = stage_perm_table(h, tab.data(), tab.size() * sizeof(uint16_t), &dtab))) return rc;
  // every block stages the table first and grid-strides over the tiles (QH_PERM_GRID: another cap, read at every call)
  const unsigned grid = (unsigned)std::min<uint64_t>(a.ntiles, (uint64_t)std::max(1, env_int("QH_PERM_GRID", 2048)));
  with_real(h, [&](auto x) {
    using R = decltype(x);
    hipLaunchKernelGGL(qh::k_perm_lds<R>, dim3(grid), dim3(threads), lds, h->stream, (typename qh::AmpT<R>::type *)h->d_psi,
                       (const uint16_t *)dtab, a);
  });
  if ((rc = check_launch(h))) return rc;
  HIP_TRY(h->tab.commit(h->stream, 0));
  h->stats.gates_submitted++;
  count_kernel(h, 1ull << (h->nloc - __builtin_popcountll(t.ctl_in | t.ctl_out)), a.ntiles << t.tile_bits);
  return QH_OK;
}

int run_perm_gather(qh_state_s *h, const qh_perm_tiles &t, const std::vector<uint32_t> &inv) {
  const int k = (int)t.k;
  uint8_t pos[QH_PERM_MAX_BITS];
  memcpy(pos, t.reg_pos, sizeof pos);
  std::sort(pos, pos + k);
  qh::PermGatherArgs a{};
  a.g.n = qh::perm_runs(k, pos, a.g.run);
  a.reg_mask = t.reg_mask;
  a.ctl = t.ctl_in | t.ctl_out;
  const size_t bytes = (size_t)h->amp_bytes() << h->nloc;
  a.nitems = bytes / 16;
  std::vector<uint64_t> tab((size_t)1 << k);
  for (size_t c = 0; c < tab.size(); ++c) tab[c] = qh::perm_deposit(inv[c], k, pos);
  // the second buffer: the one relayout sweeps keep, or a temporary that goes when this call returns
  qh::DeviceBuffer tmp;
  void *scratch = h->d_alt;
  if (!scratch) {
    if (tmp.reserve(bytes) != hipSuccess)
      return fail(QH_ERR_NOMEM, "apply_perm: no room for the second buffer of %llu bytes that a register of %d bits on these positions "
                  "needs (the state is unchanged)", (unsigned long long)bytes, k);
    scratch = tmp.ptr;
  }
  const void *dtab = nullptr;
  int rc = stage_perm_table(h, tab.data(), tab.size() * sizeof(uint64_t), &dtab);
  if (rc) return rc;
  with_real(h, [&](auto x) {
    using R = decltype(x);
    using A = typename qh::AmpT<R>::type;
    hipLaunchKernelGGL(qh::k_perm_gather<R>, dim3(grid_for(a.nitems, 1ull << 16)), dim3(256), 0, h->stream, (const A *)h->d_psi,
                       (A *)scratch, (const uint64_t *)dtab, a);
  });
  rc = check_launch(h);
  if (rc == QH_OK) {
    hipError_t e = h->tab.commit(h->stream, 0);
    if (e == hipSuccess) e = hipMemcpyAsync(h->d_psi, scratch, bytes, hipMemcpyDeviceToDevice, h->stream);
    if (e != hipSuccess) rc = fail(QH_ERR_HIP, "apply_perm: %s", hipGetErrorString(e));
  }
  if (tmp.ptr) {                                           // (the kernel and the copy still use it)
    const hipError_t e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess && rc == QH_OK) rc = fail(QH_ERR_HIP, "apply_perm: %s", hipGetErrorString(e));
  }
  if (rc) return rc;
  h->stats.gates_submitted++;
  count_kernel(h, 1ull << (h->nloc - __builtin_popcountll(a.ctl)), 1ull << h->nloc);
  h->stats.bytes_swept += 2 * bytes;                       // the copy back
  return QH_OK;
}

}  // namespace

extern "C" {

int qh_perm_plan(qh_handle h, int k, const int32_t *bits, uint64_t ctl_mask, qh_perm_tiles *out) {
  if (!h || !bits || !out) return fail(QH_ERR_ARG, "perm_plan: null handle, bits or out");
  return plan_perm_call(h, "perm_plan", k, bits, ctl_mask, out);
}

int qh_apply_perm(qh_handle h, int k, const int32_t *bits, uint64_t ctl_mask, const uint32_t *table) {
  if (!h || !bits || !table) return fail(QH_ERR_ARG, "apply_perm: null handle, bits or table");
  qh_perm_tiles t;
  int rc = plan_perm_call(h, "apply_perm", k, bits, ctl_mask, &t);
  if (rc) return rc;
  int64_t other = -1;
  const int64_t bad = qh::perm_check_table(k, table, &other);
  if (bad >= 0 && other < 0)
    return fail(QH_ERR_ARG, "apply_perm: table[%lld] = %u is outside [0,%u): not a permutation of the register's values",
                (long long)bad, table[bad], 1u << k);
  if (bad >= 0)
    return fail(QH_ERR_ARG, "apply_perm: table[%lld] = %u is hit twice (table[%lld] has the same value): not a bijection",
                (long long)bad, table[bad], (long long)other);
  if ((rc = enter(h))) return rc;          // a barrier: what is queued runs first, on whatever layout it leaves
  if ((rc = plan_perm_call(h, "apply_perm", k, bits, ctl_mask, &t))) return rc;
  if (!t.ctl_met) {                        // a shard-bit control that is 0 on this shard (met: dropped)
    h->stats.gates_submitted++;
    h->stats.gates_noop++;
    return QH_OK;
  }
  int order[QH_PERM_MAX_BITS];
  qh::perm_order(k, t.reg_pos, order);
  const std::vector<uint32_t> inv = qh::perm_inverse(k, table, order);
  return t.path == QH_PERM_LDS ? run_perm_lds(h, t, inv) : run_perm_gather(h, t, inv);
}

}  // extern "C"

// ---- rank-one register updates: qh_apply_rank1, qh_rank1_plan (kernels_rank1.hip.h, rank1_plan.h) --------------------
namespace {

// The argument checks both calls share, then the plan (rank1_plan.h) on the bit map as it is now.
int plan_rank1_call(const qh_state_s *h, const char *who, int k, const int32_t *bits, uint64_t ctl_mask, int uniform, qh_rank1_info *out) {
  const int kmax = uniform ? h->nloc : QH_RANK1_MAX_BITS;
  if (k < 1 || k > kmax)
    return fail(QH_ERR_ARG, "%s: k = %d outside [1,%d] (%s)", who, k, kmax, uniform ? "uniform form: the local bits" : "table form");
  if (h->nglob < 64 && (ctl_mask >> h->nglob))
    return fail(QH_ERR_BAD_QUBIT, "%s: control mask 0x%llx has bits >= %d", who, (unsigned long long)ctl_mask, h->nglob);
  uint64_t rmask = 0;
  const int rc = check_bit_list(h, who, k, bits, &rmask);
  if (rc) return rc;
  if (ctl_mask & rmask)
    return fail(QH_ERR_SAME_QUBIT, "%s: control and register share bits 0x%llx", who, (unsigned long long)(ctl_mask & rmask));
  // (a logical bit stays local or in the shard index whatever the relayout sweeps do)
  int pos[64];
  for (int j = 0; j < k; ++j) {
    pos[j] = h->perm[bits[j]];
    if (pos[j] >= h->nloc)
      return fail(QH_ERR_NONLOCAL, "%s: register bit %d is held by the shard index (physical bit %d, local bits: %d); exchange first",
                  who, bits[j], pos[j], h->nloc);
  }
  const Placed ctl = place(h, to_phys(h, ctl_mask));
  qh::plan_rank1(h->nloc, h->bw, k, pos, ctl.local, uniform, out);
  out->tile.k = (uint32_t)k;
  out->tile.ctl_met = (h->shard & ctl.held) == ctl.held;
  return QH_OK;
}

// what the call computes with besides the plan: a, and the tables (empty: the uniform form, conj(v_s) = vr, b u_s = ub)
struct Rank1Op {
  double a[2], vr, ub[2];
  std::vector<double> tab;      // conj(v), then b u: compressed order, interleaved re, im
  bool uniform() const { return tab.empty(); }
};

template <typename R, int TAB, int U> int allow_big_lds_rank1() {
  const hipError_t e =
      hipFuncSetAttribute((const void *)qh::k_rank1_tile<R, TAB, U>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 << 10);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    return fail(QH_ERR_HIP, "apply_rank1: hipFuncSetAttribute(MaxDynamicSharedMemorySize): %s", hipGetErrorString(e));
  }
  return QH_OK;
}

// the tail of both paths: the two sums from the slab rows of `nblk` blocks
int finish_rank1(qh_state_s *h, const qh_rank1_info &pl, const SlabSum &sum, unsigned nblk, double *sums) {
  h->stats.gates_submitted++;
  h->stats.kernels_launched += pl.kernels;
  h->stats.bytes_swept += pl.bytes_swept;
  h->stats.bytes_algorithmic += (2 * h->amp_bytes() << h->nloc) >> __builtin_popcountll(pl.tile.ctl_in | pl.tile.ctl_out);
  if (!sums) return QH_OK;
  sum.fold(nblk, 2, 2);
  return sum.get(sums, 2, "apply_rank1 sums");
}

int run_rank1_tile(qh_state_s *h, const qh_rank1_info &pl, const Rank1Op &op, double *sums) {
  const qh_perm_tiles &t = pl.tile;
  const int k = (int)t.k;
  uint8_t ranks[QH_PERM_MAX_BITS];
  memcpy(ranks, t.reg_rank, sizeof ranks);
  std::sort(ranks, ranks + k);
  qh::Rank1TileArgs a{};
  a.g.n = qh::perm_runs(k, ranks, a.g.run);
  a.tile_mask = t.tile_mask;
  a.rest_mask = h->local_mask() & ~t.tile_mask & ~t.ctl_out;
  a.ctl_out = t.ctl_out;
  a.ntiles = t.ntiles - t.tiles_skipped;
  a.m = t.tile_bits;
  a.nent = op.uniform() ? 0u : 1u << k;
  for (int p = 0, r = 0; p < h->nloc; ++p) {
    if (!((t.tile_mask >> p) & 1ull)) continue;
    if ((t.reg_mask >> p) & 1ull) a.reg_tile |= 1u << r;
    if ((t.ctl_in >> p) & 1ull) a.ctl_tile |= 1u << r;
    ++r;
  }
  a.ar = op.a[0]; a.ai = op.a[1];
  a.vr = op.vr; a.ubr = op.ub[0]; a.ubi = op.ub[1];
  const uint64_t nitems = std::max<uint64_t>(t.lds_bytes / 16, 1);
  unsigned threads = 64;                                   // four items per thread (eight in the largest tiles), one to sixteen waves
  while (threads < 1024 && threads * 4ull < nitems) threads *= 2;
  if ((uint64_t)threads * qh::kPermItems < nitems) return fail(QH_ERR_ARG, "apply_rank1: a tile of %llu items", (unsigned long long)nitems);
  const uint32_t lbits = (uint32_t)log2_u64((uint64_t)threads * (16 / h->amp_bytes()));
  const uint32_t ureg = lbits < 32 ? (a.reg_tile >> lbits) & (uint32_t)(qh::kPermItems - 1) : 0u;
  a.nslots = (1u << a.m) >> __builtin_popcount(ureg);
  const int tab = op.uniform() ? 0 : 1;
  const bool eight = (uint64_t)threads * 4 < nitems;       // (then every bit of the item number is a register bit: checked below)
  const size_t lds = std::max<size_t>((size_t)a.nslots * 16 + (tab == 1 ? (size_t)a.nent * 32 : 0), 256);
  if ((size_t)a.nslots * 16 > qh::kPermLdsBytes || lds > (160u << 10))
    return fail(QH_ERR_ARG, "apply_rank1: %zu bytes of LDS for a tile of %u bits", lds, a.m);
  int rc = QH_OK;
  if (eight && ureg != (uint32_t)(qh::kPermItems - 1)) return fail(QH_ERR_ARG, "apply_rank1: a tile of %u bits with free top bits", a.m);
  auto with_kernel = [&](auto &&f) {       // f(R, TAB, U)
    with_real(h, [&](auto x) {
      using I0 = std::integral_constant<int, 0>;
      using I1 = std::integral_constant<int, 1>;
      using U4 = std::integral_constant<int, 4>;
      using U8 = std::integral_constant<int, qh::kPermItems>;
      if (tab == 0 && !eight) f(x, I0{}, U4{});
      else if (tab == 0) f(x, I0{}, U8{});
      else if (!eight) f(x, I1{}, U4{});
      else f(x, I1{}, U8{});
    });
  };
  if (lds > (64u << 10)) with_kernel([&](auto x, auto tb, auto uu) { rc = allow_big_lds_rank1<decltype(x), decltype(tb)::value, decltype(uu)::value>(); });
  if (rc) return rc;
  const unsigned grid = (unsigned)std::min<uint64_t>(a.ntiles, (uint64_t)std::max(1, env_int("QH_RANK1_GRID", 2048)));
  SlabSum sum{h};
  if (sums) HIP_TRY(sum.reserve(std::max<uint64_t>(grid, 8), 2, 2));
  const void *dtab = nullptr;
  if (tab && (rc = stage_perm_table(h, op.tab.data(), op.tab.size() * sizeof(double), &dtab))) return rc;
  with_kernel([&](auto x, auto tb, auto uu) {
    using R = decltype(x);
    hipLaunchKernelGGL((qh::k_rank1_tile<R, decltype(tb)::value, decltype(uu)::value>), dim3(grid), dim3(threads), lds, h->stream,
                       (typename qh::AmpT<R>::type *)h->d_psi, (const qh::perm_item *)dtab, a, sums ? sum.slab : nullptr);
  });
  if ((rc = check_launch(h))) return rc;
  if (tab) HIP_TRY(h->tab.commit(h->stream, 0));
  return finish_rank1(h, pl, sum, grid, sums);
}

int run_rank1_two_pass(qh_state_s *h, const qh_rank1_info &pl, const Rank1Op &op, double *sums) {
  const qh_perm_tiles &t = pl.tile;
  const int k = (int)t.k, cb = (int)pl.chunk_bits;
  const uint64_t items = ((uint64_t)h->amp_bytes() << h->nloc) / 16, ci = ((uint64_t)h->amp_bytes() << cb) / 16, nchunks = items / ci;
  if (ci < 256 || ci > (uint64_t)qh::kRank1ChunkItems || items % ci)      // (the second path starts at 11 register bits)
    return fail(QH_ERR_ARG, "apply_rank1: a shard of %llu items on the second path", (unsigned long long)items);
  if (h->rank1.reserve(pl.scratch_bytes) != hipSuccess)
    return fail(QH_ERR_NOMEM, "apply_rank1: no room for the %llu bytes of fibre sums that a register of %d bits on these positions needs "
                "(the state is unchanged)", (unsigned long long)pl.scratch_bytes, k);
  qh::perm_item *m = h->rank1.as<qh::perm_item>(), *part = pl.split > 1 ? m + pl.nfibres : m;
  uint8_t pos[64];
  int np = 0;
  for (int p = 0; p < h->nloc; ++p)
    if ((t.reg_mask >> p) & 1ull) pos[np++] = (uint8_t)p;
  qh::Rank1DotArgs d{};
  qh::Rank1AxpyArgs x{};
  if (!op.uniform()) {
    d.g.n = qh::perm_runs((int)pl.reg_in_chunk, pos, d.g.run);
    x.g.n = qh::perm_runs(k, pos, x.g.run);
  }
  d.abv_mask = t.reg_mask >> cb;
  d.grp_mask = (h->local_mask() >> cb) & ~d.abv_mask;
  d.nunits = pl.groups * pl.split;
  d.walk = pl.walk;
  d.nfib = pl.nfibres;
  d.split = pl.split;
  d.nin = pl.reg_in_chunk;
  d.reg_low = (uint32_t)(t.reg_mask & ((1ull << cb) - 1ull));
  d.fpc = (uint32_t)pl.fibres_per_chunk;
  d.cb = x.cb = (uint32_t)cb;
  d.vr = op.vr;
  x.free_mask = h->local_mask() & ~t.reg_mask;
  x.reg_mask = t.reg_mask;
  x.ctl = t.ctl_in | t.ctl_out;
  x.nchunks = nchunks;
  x.ar = op.a[0]; x.ai = op.a[1];
  x.ubr = op.ub[0]; x.ubi = op.ub[1];
  const unsigned grid2 = (unsigned)std::min<uint64_t>(nchunks, 1ull << 20);
  SlabSum sum{h};
  if (sums) HIP_TRY(sum.reserve(std::max<uint64_t>(grid2, 8), 2, 2));
  int rc = QH_OK;
  const void *dtab = nullptr;
  if (!op.uniform() && (rc = stage_perm_table(h, op.tab.data(), op.tab.size() * sizeof(double), &dtab))) return rc;
  const qh::perm_item *dvc = (const qh::perm_item *)dtab, *dub = dvc ? dvc + ((size_t)1 << k) : nullptr;
  const size_t lds = (size_t)16 << cb;      // one complex double per amplitude of a chunk
  with_real(h, [&](auto r) {
    using R = decltype(r);
    using A = typename qh::AmpT<R>::type;
    const dim3 g1((unsigned)std::min<uint64_t>(d.nunits, 1ull << 20));
    if (op.uniform()) hipLaunchKernelGGL((qh::k_rank1_dot<R, true>), g1, dim3(256), lds, h->stream, (const A *)h->d_psi, dvc, d, part);
    else hipLaunchKernelGGL((qh::k_rank1_dot<R, false>), g1, dim3(256), lds, h->stream, (const A *)h->d_psi, dvc, d, part);
    if (pl.split > 1)
      hipLaunchKernelGGL(qh::k_rank1_fold, dim3(grid_for(pl.nfibres, 1ull << 16)), dim3(256), 0, h->stream, (const qh::perm_item *)part, m,
                         pl.nfibres, pl.split);
    double *slab = sums ? sum.slab : nullptr;
    if (op.uniform()) hipLaunchKernelGGL((qh::k_rank1_axpy<R, true>), dim3(grid2), dim3(256), 0, h->stream, (A *)h->d_psi, dub, (const qh::perm_item *)m, x, slab);
    else hipLaunchKernelGGL((qh::k_rank1_axpy<R, false>), dim3(grid2), dim3(256), 0, h->stream, (A *)h->d_psi, dub, (const qh::perm_item *)m, x, slab);
  });
  if ((rc = check_launch(h))) return rc;
  if (!op.uniform()) HIP_TRY(h->tab.commit(h->stream, 0));
  return finish_rank1(h, pl, sum, grid2, sums);
}

}  // namespace

extern "C" {

int qh_rank1_plan(qh_handle h, int k, const int32_t *bits, uint64_t ctl_mask, int uniform, qh_rank1_info *out) {
  if (!h || !bits || !out) return fail(QH_ERR_ARG, "rank1_plan: null handle, bits or out");
  return plan_rank1_call(h, "rank1_plan", k, bits, ctl_mask, uniform, out);
}

int qh_apply_rank1(qh_handle h, int k, const int32_t *bits, uint64_t ctl_mask, const double *u, const double *v, const double a[2],
                   const double b[2], double *sums) {
  if (!h || !bits || !a || !b) return fail(QH_ERR_ARG, "apply_rank1: null handle, bits, a or b");
  if (u && !v) return fail(QH_ERR_ARG, "apply_rank1: u without v (v == NULL is the uniform form and takes no u)");
  const int uniform = v ? 0 : 1;
  qh_rank1_info pl;
  int rc = plan_rank1_call(h, "apply_rank1", k, bits, ctl_mask, uniform, &pl);
  if (rc) return rc;
  for (int i = 0; i < 2; ++i) {
    if (!std::isfinite(a[i])) return fail(QH_ERR_ARG, "apply_rank1: a[%d] = %g is not finite", i, a[i]);
    if (!std::isfinite(b[i])) return fail(QH_ERR_ARG, "apply_rank1: b[%d] = %g is not finite", i, b[i]);
  }
  if (v) {
    int64_t bad = u ? qh::rank1_first_nonfinite(u, 2ull << k) : -1;
    if (bad >= 0) return fail(QH_ERR_ARG, "apply_rank1: u[%lld] = %g (%s part) is not finite", (long long)(bad / 2), u[bad], bad % 2 ? "imaginary" : "real");
    if ((bad = qh::rank1_first_nonfinite(v, 2ull << k)) >= 0)
      return fail(QH_ERR_ARG, "apply_rank1: v[%lld] = %g (%s part) is not finite", (long long)(bad / 2), v[bad], bad % 2 ? "imaginary" : "real");
  }
  if ((rc = enter(h))) return rc;          // a barrier: what is queued runs first, on whatever layout it leaves
  if ((rc = plan_rank1_call(h, "apply_rank1", k, bits, ctl_mask, uniform, &pl))) return rc;
  if (!pl.tile.ctl_met) {                  // a shard-bit control that is 0 on this shard (met: dropped)
    h->stats.gates_submitted++;
    h->stats.gates_noop++;
    if (sums) sums[0] = sums[1] = 0.0;
    return QH_OK;
  }
  Rank1Op op;
  op.a[0] = a[0]; op.a[1] = a[1];
  op.vr = std::sqrt(std::ldexp(1.0, -k));
  op.ub[0] = b[0] * op.vr; op.ub[1] = b[1] * op.vr;
  if (v) {
    std::vector<double> vc, ub;
    qh::rank1_tables(k, pl.tile.reg_pos, u, v, b, &vc, &ub);
    op.tab = std::move(vc);
    op.tab.insert(op.tab.end(), ub.begin(), ub.end());
  }
  return pl.path == QH_RANK1_TILE ? run_rank1_tile(h, pl, op, sums) : run_rank1_two_pass(h, pl, op, sums);
}

}  // extern "C"

// ---- register readout: qh_marginal, qh_sample, qh_project_bits (kernels_measure.hip.h) -------------------------------
namespace {

constexpr uint64_t kMeasBlocks = 1024;      // k_marginal_bins: blocks to aim for (four 32 KiB-LDS blocks per CU)

int meas_chunk_bits(const qh_state_s *h) { return std::min(h->nloc, qh::kMeasChunkBits); }

}  // namespace

extern "C" {

int qh_marginal(qh_handle h, int k, const int32_t *bits, double *out) {
  if (!h || !out || (k > 0 && !bits)) return fail(QH_ERR_ARG, "marginal: null handle, bits or out");
  if (k < 0 || k > qh::kMaxMarginalBits) return fail(QH_ERR_ARG, "marginal: k = %d outside [0,%d]", k, qh::kMaxMarginalBits);
  uint64_t seen = 0;
  int rc = check_bit_list(h, "marginal", k, bits, &seen);
  if (rc) return rc;
  if ((rc = enter(h))) return rc;
  const int c = meas_chunk_bits(h);
  qh::MarginalArgs a{};
  qh::FoldArgs f{};
  a.c = c;
  const SplitBits sb = split_bits(h, k, bits);     // (physical bit, output bit) of the register bits this shard holds locally
  f.fixed = sb.held_ones;                          // fixed on this shard
  for (const auto &pt : sb.local) {
    if (pt.first < c) {
      a.inner |= 1u << pt.first;
      f.tin[a.ki++] = (uint8_t)pt.second;
    } else {
      a.opos[a.ko] = (uint8_t)(pt.first - c);
      f.tout[a.ko++] = (uint8_t)pt.second;
    }
  }
  f.ki = a.ki;
  f.ko = a.ko;
  const uint64_t rest_chunks = 1ull << (h->nloc - c - a.ko);    // chunks per outer value
  uint32_t bpo = 1;
  while (bpo * 2ull <= rest_chunks && ((bpo * 2ull) << a.ko) <= kMeasBlocks) bpo *= 2;
  a.bpo = f.bpo = bpo;
  a.cpb = rest_chunks / bpo;
  const uint64_t nblk = (uint64_t)bpo << a.ko;
  const size_t out_bytes = ((size_t)1 << k) * sizeof(double);
  qh::ScratchLayout lay;
  const size_t slab_off = lay.add((size_t)(nblk << a.ki) * sizeof(double)), out_off = lay.add(out_bytes);
  HIP_TRY(h->meas.reserve(lay.total));
  char *scr = h->meas.as<char>();
  double *slab = (double *)(scr + slab_off), *dout = (double *)(scr + out_off);
  HIP_TRY(hipMemsetAsync(dout, 0, out_bytes, h->stream));
  with_real(h, [&](auto x) {
    using R = decltype(x);
    hipLaunchKernelGGL(qh::k_marginal_bins<R>, dim3((unsigned)nblk), dim3(256), 0, h->stream, (const typename qh::AmpT<R>::type *)h->d_psi, a, slab);
  });
  const uint64_t nfold = 1ull << (a.ki + a.ko);
  hipLaunchKernelGGL(qh::k_marginal_fold, dim3(grid_for(nfold, kRedBlocks)), dim3(256), 0, h->stream, (const double *)slab, f, dout);
  if ((rc = check_launch(h))) return rc;
  return read_back(h, out, dout, out_bytes);
}

int qh_sample(qh_handle h, uint64_t count, const double *u, uint64_t *logical_out) {
  if (!h || (count && (!u || !logical_out))) return fail(QH_ERR_ARG, "sample: null handle, u or out");
  for (uint64_t s = 0; s < count; ++s) {
    if (!(u[s] >= 0.0 && u[s] < 1.0)) return fail(QH_ERR_ARG, "sample: u[%llu] = %g outside [0,1)", (unsigned long long)s, u[s]);
    if (s && u[s] < u[s - 1]) return fail(QH_ERR_ARG, "sample: u is not ascending at %llu", (unsigned long long)s);
  }
  int rc = enter(h);
  if (rc) return rc;
  if (count == 0) return QH_OK;
  const int c = meas_chunk_bits(h);
  const uint64_t nchunks = 1ull << (h->nloc - c);
  const uint64_t maxlist = std::min<uint64_t>(nchunks, count);
  qh::ScratchLayout lay;
  const size_t sums_off = lay.add(nchunks * 8), tgt_off = lay.add(count * 8), ids_off = lay.add(maxlist * 8),
               first_off = lay.add((maxlist + 1) * 8), out_off = lay.add(count * 8);
  HIP_TRY(h->meas.reserve(lay.total));
  char *scr = h->meas.as<char>();
  double *d_sums = (double *)(scr + sums_off), *d_tgt = (double *)(scr + tgt_off);
  uint64_t *d_ids = (uint64_t *)(scr + ids_off), *d_first = (uint64_t *)(scr + first_off), *d_out = (uint64_t *)(scr + out_off);
  const unsigned g1 = (unsigned)std::min<uint64_t>(nchunks, 2048);
  with_real(h, [&](auto x) {
    using R = decltype(x);
    hipLaunchKernelGGL(qh::k_chunk_sums<R>, dim3(g1), dim3(256), 0, h->stream, (const typename qh::AmpT<R>::type *)h->d_psi, c, nchunks, d_sums);
  });
  if ((rc = check_launch(h))) return rc;
  std::vector<double> sums(nchunks);
  if ((rc = read_back(h, sums.data(), d_sums, nchunks * 8))) return rc;
  // the CDF over chunks, in physical order; every shot goes to the first chunk whose inclusive prefix exceeds u * norm
  double total = 0.0;
  uint64_t lastc = 0;
  for (uint64_t q = 0; q < nchunks; ++q) {
    total += sums[q];
    if (sums[q] > 0.0) lastc = q;
  }
  if (!(total > 0.0)) return fail(QH_ERR_ARG, "sample: the shard's norm is 0");
  std::vector<double> tgt(count);
  std::vector<uint64_t> ids, first;
  ids.reserve(maxlist);
  first.reserve(maxlist + 1);
  uint64_t j = 0;
  double excl = 0.0, incl = sums[0];
  for (uint64_t s = 0; s < count; ++s) {
    const double x = u[s] * total;
    while (j < lastc && incl <= x) {
      excl = incl;
      incl += sums[++j];
    }
    if (ids.empty() || ids.back() != j) {
      ids.push_back(j);
      first.push_back(s);
    }
    tgt[s] = std::max(0.0, x - excl);      // (at or above the chunk's sum: the kernel clamps to its last nonzero amplitude)
  }
  first.push_back(count);
  const uint64_t m = ids.size();
  HIP_TRY(hipMemcpyAsync(d_tgt, tgt.data(), count * 8, hipMemcpyHostToDevice, h->stream));
  HIP_TRY(hipMemcpyAsync(d_ids, ids.data(), m * 8, hipMemcpyHostToDevice, h->stream));
  HIP_TRY(hipMemcpyAsync(d_first, first.data(), (m + 1) * 8, hipMemcpyHostToDevice, h->stream));
  const qh::IndexMap mm = local_bits(h).p2l;
  const unsigned g2 = (unsigned)std::min<uint64_t>(m, 2048);
  with_real(h, [&](auto x) {
    using R = decltype(x);
    hipLaunchKernelGGL(qh::k_chunk_locate<R>, dim3(g2), dim3(256), 0, h->stream, (const typename qh::AmpT<R>::type *)h->d_psi, c,
                       (const uint64_t *)d_ids, (const uint64_t *)d_first, m, (const double *)d_tgt, mm, d_out);
  });
  if ((rc = check_launch(h))) return rc;
  return read_back(h, logical_out, d_out, count * 8);
}

int qh_project_bits(qh_handle h, uint64_t mask, uint64_t value) {
  if (!h) return fail(QH_ERR_ARG, "project_bits: null handle");
  if (value & ~mask)
    return fail(QH_ERR_ARG, "project_bits: value 0x%llx has bits outside mask 0x%llx", (unsigned long long)value, (unsigned long long)mask);
  if (h->nglob < 64 && (mask >> h->nglob))
    return fail(QH_ERR_BAD_QUBIT, "project_bits: mask 0x%llx has bits >= %d", (unsigned long long)mask, h->nglob);
  const int rc = enter(h);
  if (rc) return rc;
  const Placed m = place(h, to_phys(h, mask)), v = place(h, to_phys(h, value));
  if ((h->shard ^ v.held) & m.held) {      // (as qh_project_bit: a shard whose index contradicts the value is zeroed whole)
    HIP_TRY(hipMemsetAsync(h->d_psi, 0, (1ull << h->nloc) * h->amp_bytes(), h->stream));
    return QH_OK;
  }
  if (!m.local) return QH_OK;
  const uint64_t n = 1ull << h->nloc;
  with_real(h, [&](auto x) {
    using R = decltype(x);
    hipLaunchKernelGGL(qh::k_project_mask<R>, dim3(grid_for(n, 1u << 20)), dim3(256), 0, h->stream, (typename qh::AmpT<R>::type *)h->d_psi, n,
                       m.local, v.local);
  });
  return check_launch(h);
}

}  // extern "C"

// ---- sparse readout: qh_select, qh_topk, qh_amplitudes (kernels_select.hip.h, select_plan.h) --------------------------
namespace {

constexpr uint64_t kSelectBlocks = 2048;            // blocks at most (one weight partial each)
// qh_topk: candidates one compaction pass may hand to the host for sorting: four times k, at least QH_TOPK_MAX.  A boundary
// bin that holds more is refined on the next key bits (one more read) instead of shipping and sorting entries that cannot
// make the cut; the headroom over k keeps a large k on a generic state from refining down to single values before
// above + in_bin happens to land in [k, cap].
inline uint64_t topk_candidates(uint64_t k) { return std::max<uint64_t>(4 * k, QH_TOPK_MAX); }
constexpr uint64_t kTieCap = 2 * QH_TOPK_MAX;       // entries one tie scan may append
constexpr uint64_t kTieFloor = QH_TOPK_MAX;         // a range this short cannot overflow kTieCap
constexpr uint64_t kKeyMax = 0x7fffffffffffffffull;
static_assert(sizeof(qh_entry) == sizeof(qh::SelEntry) && offsetof(qh_entry, re) == offsetof(qh::SelEntry, re), "qh_entry layout");

void count_state_read(qh_state_s *h, uint64_t amps) {
  h->stats.kernels_launched++;
  h->stats.bytes_swept += amps * h->amp_bytes();
  h->stats.bytes_algorithmic += amps * h->amp_bytes();
}

double entry_prob(const qh_entry &e) { return std::fma(e.im, e.im, e.re * e.re); }     // (the device's prob_fma, bit for bit)

// One compaction pass: the entries with klo <= key <= khi.  *count: how many there are; *weight (optional): the sum of
// their probabilities; out (optional, cap entries): written, in the order the waves arrived, iff *count <= cap.
int select_pass(qh_state_s *h, uint64_t klo, uint64_t khi, uint64_t cap, qh_entry *out, uint64_t *count, double *weight) {
  const int c = meas_chunk_bits(h);
  const uint64_t nchunks = 1ull << (h->nloc - c);
  const unsigned grid = (unsigned)std::min<uint64_t>(nchunks, kSelectBlocks);
  qh::ScratchLayout lay;
  const size_t cnt_off = lay.add(8), w_off = lay.add(grid * sizeof(double)), ent_off = lay.add(cap * sizeof(qh::SelEntry));
  HIP_TRY(h->meas.reserve(lay.total));
  char *scr = h->meas.as<char>();
  unsigned long long *d_cnt = (unsigned long long *)(scr + cnt_off);
  double *d_w = (double *)(scr + w_off);
  qh::SelEntry *d_ent = cap ? (qh::SelEntry *)(scr + ent_off) : nullptr;
  HIP_TRY(hipMemsetAsync(d_cnt, 0, 8, h->stream));
  const qh::IndexMap mm = local_bits(h).p2l;
  with_real(h, [&](auto x) {
    using R = decltype(x);
    hipLaunchKernelGGL(qh::k_select<R>, dim3(grid), dim3(256), 0, h->stream, (const typename qh::AmpT<R>::type *)h->d_psi, c, nchunks, klo,
                       khi, mm, d_cnt, d_ent, cap, d_w);
  });
  int rc = check_launch(h);
  if (rc) return rc;
  count_state_read(h, 1ull << h->nloc);
  std::vector<double> wp(grid);
  unsigned long long cnt = 0;
  HIP_TRY(hipMemcpyAsync(wp.data(), d_w, grid * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  if ((rc = read_back(h, &cnt, d_cnt, 8, "select"))) return rc;
  *count = cnt;
  if (weight) {
    double w = 0.0;
    for (unsigned b = 0; b < grid; ++b) w += wp[b];
    *weight = w;
  }
  if (out && cnt && cnt <= cap) return read_back(h, out, d_ent, cnt * sizeof(qh::SelEntry), "select");
  return QH_OK;
}

// One histogram pass of the radix select (select_plan.h): hist[b] for the 2^sel_bits(level) bins under pl.prefix
int key_hist_pass(qh_state_s *h, const qh::SelPlan &pl, std::vector<uint64_t> *hist) {
  const int c = meas_chunk_bits(h), bits = qh::sel_bits(pl.level), shift = qh::sel_shift(pl.level);
  const uint64_t nchunks = 1ull << (h->nloc - c);
  const unsigned grid = (unsigned)std::min<uint64_t>(nchunks, kSelectBlocks);
  const size_t bytes = sizeof(uint64_t) << bits;
  HIP_TRY(h->meas.reserve(bytes));
  unsigned long long *d_hist = h->meas.as<unsigned long long>();
  HIP_TRY(hipMemsetAsync(d_hist, 0, bytes, h->stream));
  with_real(h, [&](auto x) {
    using R = decltype(x);
    hipLaunchKernelGGL(qh::k_key_hist<R>, dim3(grid), dim3(256), 0, h->stream, (const typename qh::AmpT<R>::type *)h->d_psi, c, nchunks,
                       pl.prefix, shift, bits, d_hist);
  });
  const int rc = check_launch(h);
  if (rc) return rc;
  count_state_read(h, 1ull << h->nloc);
  hist->assign((size_t)1 << bits, 0);
  return read_back(h, hist->data(), d_hist, bytes, "topk");
}

// `need` entries whose key is `want`, the smallest LOGICAL indices first, appended to out: growing ranges of the shard's
// amplitudes in logical order are gathered through the logical -> physical map until enough are found (as
// argmax_from_tilemax finishes a flat state).  `total` of the shard's amplitudes have that key.
int tie_scan(qh_state_s *h, uint64_t want, uint64_t need, uint64_t total, std::vector<qh_entry> *out) {
  qh::TieMap tm{};
  for (int b = 0; b < h->nglob; ++b) {
    const Placed at = place_bit(h, b);
    if (at.held) {
      if (h->shard & at.held) tm.shard_logical |= 1ull << b;
      continue;
    }
    tm.phys[tm.n] = (uint8_t)h->perm[b];
    tm.log[tm.n++] = (uint8_t)b;
  }
  qh::ScratchLayout lay;
  const size_t cnt_off = lay.add(8), ent_off = lay.add(kTieCap * sizeof(qh::SelEntry));
  HIP_TRY(h->meas.reserve(lay.total));
  unsigned long long *d_cnt = (unsigned long long *)(h->meas.as<char>() + cnt_off);
  qh::SelEntry *d_ent = (qh::SelEntry *)(h->meas.as<char>() + ent_off);
  const uint64_t n = 1ull << h->nloc;
  uint64_t len = qh::sel_tie_first_len(n, total, need, kTieFloor), r0 = 0, found = 0;
  std::vector<qh_entry> got;
  while (found < need && r0 < n) {
    const uint64_t r1 = std::min(n, r0 + len);
    HIP_TRY(hipMemsetAsync(d_cnt, 0, 8, h->stream));
    with_real(h, [&](auto x) {
      using A = typename qh::AmpT<decltype(x)>::type;
      hipLaunchKernelGGL(qh::k_tie_scan<A>, dim3(grid_for(r1 - r0, kRedBlocks)), dim3(256), 0, h->stream, (const A *)h->d_psi, r0, r1, want,
                         tm, d_cnt, d_ent, kTieCap);
    });
    int rc = check_launch(h);
    if (rc) return rc;
    count_state_read(h, r1 - r0);
    unsigned long long cnt = 0;
    if ((rc = read_back(h, &cnt, d_cnt, 8, "topk"))) return rc;
    if (cnt > kTieCap) {      // denser here than on average: a shorter range (one of kTieFloor amplitudes cannot overflow)
      len = std::max(len / 16, kTieFloor);
      continue;
    }
    got.resize(cnt);
    if (cnt && (rc = read_back(h, got.data(), d_ent, cnt * sizeof(qh::SelEntry), "topk"))) return rc;
    std::sort(got.begin(), got.end(), [](const qh_entry &a, const qh_entry &b) { return a.index < b.index; });
    for (uint64_t j = 0; j < cnt && found < need; ++j, ++found) out->push_back(got[j]);
    r0 = r1;
    len = std::min(n, len * 4);
  }
  return QH_OK;
}

}  // namespace

extern "C" {

int qh_select(qh_handle h, double threshold, uint64_t cap, qh_entry *out, uint64_t *count, double *weight) {
  if (!h || !count) return fail(QH_ERR_ARG, "select: null handle or count");
  if (!(threshold >= 0.0)) return fail(QH_ERR_ARG, "select: threshold %g is negative or not a number", threshold);
  if (cap > QH_SELECT_MAX) return fail(QH_ERR_ARG, "select: cap %llu above QH_SELECT_MAX", (unsigned long long)cap);
  if (cap && !out) return fail(QH_ERR_ARG, "select: cap %llu without out", (unsigned long long)cap);
  int rc = enter(h);
  if (rc) return rc;
  const double t = threshold + 0.0;      // (-0.0 -> +0.0)
  uint64_t klo, cnt = 0;
  memcpy(&klo, &t, 8);
  double w = 0.0;
  if ((rc = select_pass(h, klo, qh::kSelKeyInf, cap, out, &cnt, &w))) return rc;
  if (cnt <= cap) std::sort(out, out + cnt, [](const qh_entry &a, const qh_entry &b) { return a.index < b.index; });
  *count = cnt;
  if (weight) *weight = w;
  return QH_OK;
}

int qh_topk(qh_handle h, uint64_t k, qh_entry *out, uint64_t *count) {
  if (!h || !count || (k && !out)) return fail(QH_ERR_ARG, "topk: null handle, out or count");
  if (k > QH_TOPK_MAX) return fail(QH_ERR_ARG, "topk: k = %llu above QH_TOPK_MAX", (unsigned long long)k);
  int rc = enter(h);
  if (rc) return rc;
  if (k == 0) {
    *count = 0;
    return QH_OK;
  }
  qh::SelPlan pl = qh::sel_begin(k, topk_candidates(k));
  std::vector<uint64_t> hist;
  qh::SelStep st{};
  do {
    if ((rc = key_hist_pass(h, pl, &hist))) return rc;
    st = qh::sel_step(pl, hist.data());
  } while (st.next == qh::kSelRefine);
  if (st.next == qh::kSelEmpty) {
    *count = 0;
    return QH_OK;
  }
  // the candidates above the cut: keys >= key_lo, or, in front of a tie scan, the keys above the tied value
  std::vector<qh_entry> ent(st.candidates);
  if (st.candidates) {
    uint64_t cnt = 0;
    const uint64_t klo = st.next == qh::kSelTies ? st.key_lo + 1 : st.key_lo;
    if ((rc = select_pass(h, klo, kKeyMax, st.candidates, ent.data(), &cnt, nullptr))) return rc;
    if (cnt != st.candidates)
      return fail(QH_ERR_HIP, "topk: %llu candidates where the histogram counted %llu (the state changed under the call?)",
                  (unsigned long long)cnt, (unsigned long long)st.candidates);
    std::sort(ent.begin(), ent.end(), [](const qh_entry &a, const qh_entry &b) {
      const double pa = entry_prob(a), pb = entry_prob(b);
      return pa > pb || (pa == pb && a.index < b.index);
    });
  }
  if (st.next == qh::kSelTies && (rc = tie_scan(h, st.key_lo, st.ties_needed, st.ties_total, &ent))) return rc;
  const uint64_t m = std::min<uint64_t>(k, ent.size());
  if (m) memcpy(out, ent.data(), m * sizeof(qh_entry));
  *count = m;
  return QH_OK;
}

int qh_amplitudes(qh_handle h, uint64_t count, const uint64_t *logical, double *out, uint64_t *nlocal) {
  if (!h || (count && (!logical || !out))) return fail(QH_ERR_ARG, "amplitudes: null handle, indices or out");
  if (count > (1ull << 24)) return fail(QH_ERR_ARG, "amplitudes: %llu indices (at most 2^24 a call)", (unsigned long long)count);
  if (h->nglob < 64)
    for (uint64_t j = 0; j < count; ++j)
      if (logical[j] >> h->nglob)
        return fail(QH_ERR_ARG, "amplitudes: index %llu (entry %llu) out of range", (unsigned long long)logical[j], (unsigned long long)j);
  int rc = enter(h);
  if (rc) return rc;
  qh::GatherMap gm{};
  gm.nglob = h->nglob;
  for (int b = 0; b < h->nglob; ++b) {
    const Placed at = place_bit(h, b);
    gm.l2p[b] = at.held ? 0xff : (uint8_t)h->perm[b];
    if (at.held) {
      gm.held |= 1ull << b;
      if (h->shard & at.held) gm.held_ones |= 1ull << b;
    }
  }
  uint64_t mine = 0;
  for (uint64_t j = 0; j < count; ++j) mine += (logical[j] & gm.held) == gm.held_ones;
  if (count) {
    qh::ScratchLayout lay;
    const size_t idx_off = lay.add(count * 8), out_off = lay.add(count * 16);
    HIP_TRY(h->meas.reserve(lay.total));
    uint64_t *d_idx = (uint64_t *)(h->meas.as<char>() + idx_off);
    double2 *d_out = (double2 *)(h->meas.as<char>() + out_off);
    HIP_TRY(hipMemcpyAsync(d_idx, logical, count * 8, hipMemcpyHostToDevice, h->stream));
    with_real(h, [&](auto x) {
      using A = typename qh::AmpT<decltype(x)>::type;
      hipLaunchKernelGGL(qh::k_gather_amps<A>, dim3(grid_for(count, kRedBlocks)), dim3(256), 0, h->stream, (const A *)h->d_psi,
                         (const uint64_t *)d_idx, count, gm, d_out);
    });
    if ((rc = check_launch(h))) return rc;
    if ((rc = read_back(h, out, d_out, count * 16, "amplitudes"))) return rc;
  }
  if (nlocal) *nlocal = mine;
  return QH_OK;
}

}  // extern "C"

// ---- reduced density matrices: qh_reduced_density, qh_density_plan (kernels_density.hip.h, density_plan.h) -------------------
namespace {

// The argument checks both entry points share, then the plan; nothing touches the device
int plan_density_for(const qh_state_s *h, const char *who, int k, const int32_t *bits, const void *out, qh_density_tiles *pl) {
  if (!h || !out || (k > 0 && !bits)) return fail(QH_ERR_ARG, "%s: null handle, bits or out", who);
  const int kmax = std::min(QH_DENSITY_MAX_BITS, h->nloc);
  if (k < 0 || k > kmax) return fail(QH_ERR_ARG, "%s: k = %d outside [0,%d]", who, k, kmax);
  uint64_t seen = 0;
  const int rc = check_bit_list(h, who, k, bits, &seen);
  if (rc) return rc;
  int pos[QH_DENSITY_MAX_BITS] = {};
  for (int t = 0; t < k; ++t) {
    if (place_bit(h, bits[t]).held)
      return fail(QH_ERR_NONLOCAL, "%s: logical bit %d is at physical bit %d, held by the shard index (local bits: %d); exchange first",
                  who, bits[t], h->perm[bits[t]], h->nloc);
    pos[t] = h->perm[bits[t]];
  }
  qh::plan_density(h->nloc, k, pos, pl);
  return QH_OK;
}

template <typename R, int KT>
void launch_density_tiles(qh_state_s *h, const qh_density_tiles &pl, const qh::DensityArgs &a, double2 *slab) {
  using A = typename qh::AmpT<R>::type;
  const dim3 grid(pl.block_pairs * pl.wg_per_pair);
  if constexpr (KT <= 2) {
    hipLaunchKernelGGL((qh::k_density_direct<R, KT>), grid, dim3(256), 0, h->stream, (const A *)h->d_psi, a, (double *)slab);
  } else if constexpr (KT == qh::kDensityTileBits) {
    if (pl.block_pairs > 1) hipLaunchKernelGGL((qh::k_density_tiles<R, KT, true>), grid, dim3(256), 0, h->stream, (const A *)h->d_psi, a, slab);
    else hipLaunchKernelGGL((qh::k_density_tiles<R, KT, false>), grid, dim3(256), 0, h->stream, (const A *)h->d_psi, a, slab);
  } else {
    hipLaunchKernelGGL((qh::k_density_tiles<R, KT, false>), grid, dim3(256), 0, h->stream, (const A *)h->d_psi, a, slab);
  }
}

}  // namespace

extern "C" {

int qh_density_plan(qh_handle h, int k, const int32_t *bits, qh_density_tiles *out) {
  qh_density_tiles pl;
  const int rc = plan_density_for(h, "density_plan", k, bits, out, &pl);
  if (rc) return rc;
  *out = pl;
  return QH_OK;
}

int qh_reduced_density(qh_handle h, int k, const int32_t *bits, double *out) {
  qh_density_tiles pl;
  int rc = plan_density_for(h, "reduced_density", k, bits, out, &pl);
  if (rc) return rc;
  if ((rc = enter(h))) return rc;
  if ((rc = plan_density_for(h, "reduced_density", k, bits, out, &pl))) return rc;      // the flush may have re-laid the state out
  const size_t out_bytes = (size_t)16 << (2 * k);
  qh::ScratchLayout lay;
  const size_t slab_off = lay.add(pl.slab_bytes), out_off = lay.add(out_bytes);
  HIP_TRY(h->meas.reserve(lay.total));
  double2 *slab = (double2 *)(h->meas.as<char>() + slab_off), *dout = (double2 *)(h->meas.as<char>() + out_off);
  if (pl.path == QH_DENSITY_GATHER) {
    qh::DensityGatherArgs g{};
    memcpy(g.row_pos, pl.row_pos, 8);
    memcpy(g.row_bit, pl.row_bit, 8);
    memcpy(g.rest_pos, pl.rest_pos, 8);
    g.k = k;
    g.ne = (int)pl.nrest;
    with_real(h, [&](auto x) {
      using R = decltype(x);
      hipLaunchKernelGGL(qh::k_density_gather<R>, dim3(1), dim3(256), 0, h->stream, (const typename qh::AmpT<R>::type *)h->d_psi, g, dout);
    });
  } else {
    qh::DensityArgs a{};
    memcpy(a.row_pos, pl.row_pos, 8);
    memcpy(a.col_pos, pl.col_pos, sizeof a.col_pos);
    memcpy(a.rest_pos, pl.rest_pos, sizeof a.rest_pos);
    a.k = k;
    a.kt = (int)pl.tile_bits;
    a.cb = (int)pl.chunk_bits;
    a.nrest = (int)pl.nrest;
    a.wgpp = pl.wg_per_pair;
    a.cpw = pl.chunks_per_wg;
    for (uint32_t q = 0; q < pl.nrest; ++q) a.rest_mask |= 1ull << pl.rest_pos[q];
    // the load order of a chunk of a tile: its row and column positions merged, ascending
    for (int i = 0, jr = 0, jc = 0; i < a.kt + a.cb; ++i) {
      const bool row = jc == a.cb || (jr < a.kt && pl.row_pos[jr] < pl.col_pos[jc]);
      a.upos[i] = row ? pl.row_pos[jr] : pl.col_pos[jc];
      a.udst[i] = (uint8_t)(row ? jr++ : 16 + jc++);
    }
    with_real(h, [&](auto x) {
      using R = decltype(x);
      switch (a.kt) {
        case 0: launch_density_tiles<R, 0>(h, pl, a, slab); break;
        case 1: launch_density_tiles<R, 1>(h, pl, a, slab); break;
        case 2: launch_density_tiles<R, 2>(h, pl, a, slab); break;
        case 3: launch_density_tiles<R, 3>(h, pl, a, slab); break;
        case 4: launch_density_tiles<R, 4>(h, pl, a, slab); break;
        case 5: launch_density_tiles<R, 5>(h, pl, a, slab); break;
        default: launch_density_tiles<R, 6>(h, pl, a, slab); break;
      }
    });
    qh::DensityFoldArgs f{};
    memcpy(f.row_bit, pl.row_bit, 8);
    f.k = k;
    f.kt = a.kt;
    f.wgpp = pl.wg_per_pair;
    f.npairs = pl.block_pairs;
    const uint32_t nfold = pl.block_pairs << (2 * a.kt);
    hipLaunchKernelGGL(qh::k_density_fold, dim3((nfold + 3) / 4), dim3(256), 0, h->stream, (const double2 *)slab, f, dout);
  }
  if ((rc = check_launch(h))) return rc;
  if ((rc = read_back(h, out, dout, out_bytes, "reduced_density"))) return rc;
  h->stats.kernels_launched += 1;      // (the fold is not counted, as in qh_inner)
  h->stats.bytes_algorithmic += (1ull << h->nloc) * h->amp_bytes();
  h->stats.bytes_swept += pl.amps_swept * h->amp_bytes();
  return QH_OK;
}

}  // extern "C"

// ---- two states: qh_clone, qh_copy, qh_inner, qh_axpby (kernels_two_state.hip.h and its two operations) ---------------------
namespace {

constexpr uint64_t kInnerBlocks = 4096;     // blocks at most (one slab row of (re, im) each)

// both handles live, on one device, of one shape
int check_pair(const qh_state_s *a, const qh_state_s *b, const char *who) {
  if (!a || !b) return fail(QH_ERR_ARG, "%s: null handle", who);
  if (a->dry || b->dry) return fail(QH_ERR_ARG, "%s: not on a dry (planner-only) handle", who);
  if (a->device != b->device) return fail(QH_ERR_ARG, "%s: the handles live on devices %d and %d", who, a->device, b->device);
  if (a->nloc != b->nloc || a->nglob != b->nglob || a->bw != b->bw)
    return fail(QH_ERR_ARG, "%s: %d of %d qubits at width %d against %d of %d at width %d", who, a->nloc, a->nglob, a->bw, b->nloc,
                b->nglob, b->bw);
  return QH_OK;
}

int plan_pair(const qh_state_s *a, const qh_state_s *b, const char *who, qh_inner_tiles *out) {
  if (a->shard != b->shard)
    return fail(QH_ERR_NONLOCAL, "%s: shard %llu against shard %llu; exchange first", who, (unsigned long long)a->shard,
                (unsigned long long)b->shard);
  const int l = qh::plan_inner(a->nloc, a->nglob, a->perm, b->perm, out);
  if (l >= 0)
    return fail(QH_ERR_NONLOCAL, "%s: logical bit %d is at physical bit %d of one handle and %d of the other, and the shard index "
                "holds one of them (local bits: %d); exchange first", who, l, a->perm[l], b->perm[l], a->nloc);
  return QH_OK;
}

// A handle that make_sibling made goes away again (what was to fill it failed): rc and its message are kept
int drop_sibling(qh_state_s *h, int rc) {
  const std::string why = g_err;
  qh_destroy(h);
  g_err = why;
  return rc;
}

// A new handle beside src, for qh_clone / qh_extend / qh_release: on src's device, of src's width, shard index and fusion
// level, with nloc of nglob qubits, HBM memory and a stream of its own, zeroed stats, nothing queued, relayout undecided, no
// communicator and the identity bit map.  Beside a planner-only src: planner-only, no device call.  QH_ERR_NOMEM: nothing
// is created.
int make_sibling(const qh_state_s *src, int nloc, int nglob, const char *who, qh_state_s **out) {
  auto *h = new qh_state_s;
  h->nloc = nloc;
  h->nglob = nglob;
  h->bw = src->bw;
  h->device = src->device;
  h->shard = src->shard;
  h->dry = src->dry;
  if (!h->dry) {
    const size_t bytes = (size_t)h->amp_bytes() << nloc;
    hipError_t e = alloc_state_buffer(&h->d_psi, bytes);
    if (e != hipSuccess) {
      (void)hipGetLastError();
      h->d_psi = nullptr;
      delete h;
      return fail(QH_ERR_NOMEM, "%s: hipMalloc(%zu bytes) for %d qubits: %s", who, bytes, nloc, hipGetErrorString(e));
    }
    h->owns_mem = true;
    e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking);
    if (e != hipSuccess) {
      (void)hipFree(h->d_psi);
      delete h;
      return fail(QH_ERR_HIP, "%s: hipStreamCreate: %s", who, hipGetErrorString(e));
    }
    h->owns_stream = true;
  }
  const int rc = common_init(h);
  if (rc) return drop_sibling(h, rc);
  h->fusion = src->fusion;
  *out = h;
  return QH_OK;
}

// b's stream has been given work that a's stream is about to read (or must not overtake): an event between them
int order_after(qh_state_s *a, qh_state_s *b) {
  if (!b->ev_read) HIP_TRY(hipEventCreateWithFlags(&b->ev_read, hipEventDisableTiming));
  HIP_TRY(hipEventRecord(b->ev_read, b->stream));
  HIP_TRY(hipStreamWaitEvent(a->stream, b->ev_read, 0));
  return QH_OK;
}

// The geometry of the linear walk: 2^items 16-byte items in chunks of 256 threads x kInnerLoads, at most kInnerBlocks blocks,
// a whole number of chunks per block
struct LinearGrid { int cw; uint32_t cpb; uint64_t nblk; };
LinearGrid linear_grid(int items) {
  const int cw = std::min(8 + 3, items);
  const uint64_t nchunks = 1ull << (items - cw), nblk = std::min(nchunks, kInnerBlocks);
  return {cw, (uint32_t)(nchunks / nblk), nblk};
}
// ... and of the tiles walk: the plan's tables as the kernels take them, chunks of 2^cbits tiles; *nblk = the blocks
qh::InnerTileArgs tile_args(const qh_inner_tiles &pl, uint64_t *nblk) {
  qh::InnerTileArgs t{};
  memcpy(t.tile_a, pl.tile_a, 8);
  memcpy(t.tile_b, pl.tile_b, 8);
  memcpy(t.shuffle, pl.shuffle, 8);
  memcpy(t.rest_a, pl.rest_a, sizeof t.rest_a);
  memcpy(t.rest_b, pl.rest_b, sizeof t.rest_b);
  t.nrest = (int)pl.nrest;
  t.cbits = std::min(qh::kInnerChunkBits, t.nrest);
  const uint64_t nchunks = 1ull << (t.nrest - t.cbits);
  *nblk = std::min(nchunks, kInnerBlocks);
  t.cpb = (uint32_t)(nchunks / *nblk);
  return t;
}

// The one dispatch of the two-state walks (kernels_two_state.hip.h): the walk pl names, with its geometry (at most
// kInnerBlocks blocks, a whole number of chunks per block), on a's stream.  Returns the blocks launched: the slab rows an
// operation that sums has written.
template <typename Op> uint64_t launch_two_state(qh_state_s *a, const qh_state_s *b, const qh_inner_tiles &pl, const Op &op, double *slab) {
  uint64_t nblk = 1;
  with_real(a, [&](auto x) {
    using R = decltype(x);
    qh::TwoDst<R, Op> *pa = (qh::TwoDst<R, Op> *)a->d_psi;
    const typename qh::AmpT<R>::type *pb = (const typename qh::AmpT<R>::type *)b->d_psi;
    if (pl.path == QH_INNER_LINEAR) {
      const LinearGrid g = linear_grid(a->nloc - qh::Item16<R>::kAmpBits);
      nblk = g.nblk;
      hipLaunchKernelGGL((qh::k_two_linear<R, Op>), dim3((unsigned)nblk), dim3(256), 0, a->stream, pa, pb, op, g.cw, g.cpb, slab);
    } else if constexpr (Op::RS) {      // (the other two walks read b)
      if (pl.path == QH_INNER_TILES) {
        const qh::InnerTileArgs t = tile_args(pl, &nblk);
        hipLaunchKernelGGL((qh::k_two_tiles<R, Op>), dim3((unsigned)nblk), dim3(256), 0, a->stream, pa, pb, op, t, slab);
      } else {
        qh::InnerGatherArgs g{};
        g.nloc = a->nloc;
        memcpy(g.pos_b, pl.pos_b, sizeof g.pos_b);
        hipLaunchKernelGGL((qh::k_two_gather<R, Op>), dim3(1), dim3(256), 0, a->stream, pa, pb, op, g, slab);
      }
    }
  });
  return nblk;
}

// <a|b> into vals, on a's stream, behind what b's stream has been given; both flushed, pl = their plan.  The host waits.
// No stats: the callers count.
int run_inner(qh_state_s *a, qh_state_s *b, const qh_inner_tiles &pl, double vals[2]) {
  int rc;
  SlabSum sum{a};
  HIP_TRY(sum.reserve(kInnerBlocks, 2, 2));
  if (b != a && (rc = order_after(a, b))) return rc;      // a's stream reads b: behind everything b's stream has been given
  sum.fold(launch_two_state(a, b, pl, qh::InnerOp{}, sum.slab), 2, 2);
  if ((rc = check_launch(a))) return rc;
  return sum.get(vals, 2, "qh_inner");
}

}  // namespace

extern "C" {

int qh_clone(qh_handle src, qh_handle *out) {
  if (!src || !out) return fail(QH_ERR_ARG, "clone: null handle or out");
  int rc = enter(src);
  if (rc) return rc;
  qh_state_s *h = nullptr;
  if ((rc = make_sibling(src, src->nloc, src->nglob, "clone", &h))) return rc;
  memcpy(h->perm, src->perm, sizeof h->perm);
  const hipError_t e = hipMemcpyAsync(h->d_psi, src->d_psi, (size_t)src->amp_bytes() << src->nloc, hipMemcpyDefault, src->stream);
  if (e != hipSuccess) rc = fail(QH_ERR_HIP, "clone: hipMemcpyAsync: %s", hipGetErrorString(e));
  else rc = wait_stream(src, src->stream, "qh_clone");
  if (rc) return drop_sibling(h, rc);
  *out = h;
  return QH_OK;
}

int qh_copy(qh_handle dst, qh_handle src) {
  int rc = check_pair(dst, src, "copy");
  if (rc) return rc;
  if (dst == src) return fail(QH_ERR_ARG, "copy: dst == src");
  if (dst->shard != src->shard)
    return fail(QH_ERR_ARG, "copy: shard %llu against shard %llu", (unsigned long long)dst->shard, (unsigned long long)src->shard);
  if ((rc = enter(src))) return rc;
  // dst is replaced whole: nothing it has queued is worth running and a failed flush is forgotten (as the initialisations)
  dst->queue.clear();
  dst->poisoned = false;
  if (dst->comm) qh::wait_all_arrivals(&dst->comm->arrivals, dst->stream);
  if ((rc = wait_stream(dst, dst->stream, "qh_copy"))) return rc;
  HIP_TRY(hipMemcpyAsync(dst->d_psi, src->d_psi, (size_t)src->amp_bytes() << src->nloc, hipMemcpyDefault, src->stream));
  if ((rc = wait_stream(src, src->stream, "qh_copy"))) return rc;
  memcpy(dst->perm, src->perm, sizeof dst->perm);
  return QH_OK;
}

int qh_inner_plan(qh_handle a, qh_handle b, qh_inner_tiles *out) {
  if (!a || !b || !out) return fail(QH_ERR_ARG, "inner_plan: null handle or out");
  if (a->nloc != b->nloc || a->nglob != b->nglob || a->bw != b->bw) return fail(QH_ERR_ARG, "inner_plan: handles of different shapes");
  qh_inner_tiles t;
  const int rc = plan_pair(a, b, "inner_plan", &t);
  if (rc) return rc;
  *out = t;
  return QH_OK;
}

int qh_inner(qh_handle a, qh_handle b, double out[2]) {
  int rc = check_pair(a, b, "inner");
  if (rc) return rc;
  if (!out) return fail(QH_ERR_ARG, "inner: null out");
  if ((rc = enter(a))) return rc;
  if (b != a && (rc = enter(b))) return rc;
  qh_inner_tiles pl;
  if ((rc = plan_pair(a, b, "inner", &pl))) return rc;
  double vals[2];
  if ((rc = run_inner(a, b, pl, vals))) return rc;
  out[0] = vals[0];
  out[1] = vals[1];
  a->stats.kernels_launched += 1;      // one read of the two states (the fold is not counted, as in qh_expect_pauli)
  a->stats.bytes_swept += 2 * ((1ull << a->nloc) * a->amp_bytes());
  return QH_OK;
}

int qh_axpby(qh_handle dst, const double alpha[2], qh_handle src, const double beta[2], double *norm2) {
  int rc = check_pair(dst, src, "axpby");
  if (rc) return rc;
  if (!alpha || !beta) return fail(QH_ERR_ARG, "axpby: null coefficient");
  if (dst == src) return fail(QH_ERR_ARG, "axpby: dst == src (use qh_scale)");
  qh_inner_tiles pl;
  // which bits the shard index holds is not something a flush changes: refused before anything runs
  if ((rc = plan_pair(dst, src, "axpby", &pl))) return rc;
  if ((rc = enter(dst))) return rc;      // (queued gates run, exchange arrivals are waited for on dst's stream)
  if ((rc = enter(src))) return rc;
  if ((rc = plan_pair(dst, src, "axpby", &pl))) return rc;      // the layouts the flushes left
  const bool rd = alpha[0] != 0.0 || alpha[1] != 0.0, rs = beta[0] != 0.0 || beta[1] != 0.0;
  if (!rs && alpha[0] == 1.0 && alpha[1] == 0.0) {      // dst as it is: no kernel; the norm from the readers' fixed-order sum
    if (!norm2) return QH_OK;
    double vals[2];
    if ((rc = plan_pair(dst, dst, "axpby", &pl)) || (rc = run_inner(dst, dst, pl, vals))) return rc;
    *norm2 = vals[0];
    return QH_OK;
  }
  SlabSum sum{dst};
  if (norm2) HIP_TRY(sum.reserve(kInnerBlocks, 2, 2));
  if (rs && (rc = order_after(dst, src))) return rc;      // dst's stream reads src: behind everything src's stream has been given
  if (!rs) pl.path = QH_INNER_LINEAR;      // (src not read: the layouts do not matter)
  const qh::AxpbyCoef c{alpha[0], alpha[1], beta[0], beta[1], norm2 ? 1 : 0};
  uint64_t nblk;
  if (rd && rs) nblk = launch_two_state(dst, src, pl, qh::AxpbyOp<true, true>{c}, sum.slab);
  else if (rs) nblk = launch_two_state(dst, src, pl, qh::AxpbyOp<false, true>{c}, sum.slab);
  else if (rd) nblk = launch_two_state(dst, src, pl, qh::AxpbyOp<true, false>{c}, sum.slab);
  else nblk = launch_two_state(dst, src, pl, qh::AxpbyOp<false, false>{c}, sum.slab);
  if (norm2) sum.fold(nblk, 2, 1);
  if ((rc = check_launch(dst))) return rc;
  // the host waits: on return src may be changed and dst read at once
  if (norm2) rc = sum.get(norm2, 1, "qh_axpby");
  else rc = wait_stream(dst, dst->stream, "qh_axpby");
  if (rc) return rc;
  const uint64_t streams = 1 + (rd ? 1 : 0) + (rs ? 1 : 0), bytes = streams * ((1ull << dst->nloc) * dst->amp_bytes());
  dst->stats.kernels_launched += 1;      // (the fold is not counted, as in qh_inner)
  dst->stats.bytes_swept += bytes;
  dst->stats.bytes_algorithmic += bytes;
  return QH_OK;
}

}  // extern "C"

// ---- growing and shrinking a state: qh_extend, qh_release (kernels_resize.hip.h, resize_plan.h) ----------------------------
namespace {

// the checks both calls share, before anything runs
int check_resize(const qh_state_s *src, const void *out, const char *who, int k, int nloc_new) {
  if (!src || !out) return fail(QH_ERR_ARG, "%s: null handle or out", who);
  if (k < 1 || k > qh::kMaxResizeBits) return fail(QH_ERR_ARG, "%s: k = %d outside [1,%d]", who, k, qh::kMaxResizeBits);
  if (nloc_new < 1 || nloc_new > 40) return fail(QH_ERR_ARG, "%s: %d local qubits would become %d, outside [1,40]", who, src->nloc, nloc_new);
  if (src->nglob + (nloc_new - src->nloc) > qh::kResizeMaxGlobalBits)
    return fail(QH_ERR_ARG, "%s: %d global qubits would become more than %d", who, src->nglob, qh::kResizeMaxGlobalBits);
  return QH_OK;
}

// one kernel has read src once and written the new state once
void count_resize(qh_state_s *src, const qh_state_s *h) {
  const uint64_t amps = (1ull << src->nloc) + (1ull << h->nloc);      // (both terms are even: every handle has a local bit)
  count_kernel(src, amps / 2, amps / 2);
}

}  // namespace

extern "C" {

int qh_extend(qh_handle src, int k, const double *amps, uint64_t basis, qh_handle *out) {
  int rc = check_resize(src, out, "extend", k, src ? src->nloc + k : 0);
  if (rc) return rc;
  if (!amps && basis >= (1ull << k)) return fail(QH_ERR_ARG, "extend: basis state %llu of %d qubits", (unsigned long long)basis, k);
  if ((rc = flush_impl(src))) return rc;          // (planner-only handles too: the bit map is the one the queue leaves)
  qh_state_s *h = nullptr;
  if ((rc = make_sibling(src, src->nloc + k, src->nglob + k, "extend", &h))) return rc;
  qh::plan_extend(src->nloc, src->nglob, src->perm, k, h->perm);
  if (src->dry) {
    *out = h;
    return QH_OK;
  }
  TabPlan t;                                      // the whole table, in order, through the staged upload of the table gates
  t.kl = k;
  t.tbits = (1u << k) - 1u;
  std::vector<double> unit;
  if (!amps) {
    unit.assign((size_t)2 << k, 0.0);
    unit[2 * basis] = 1.0;
    amps = unit.data();
  }
  const void *dtab = nullptr;
  if ((rc = stage_table(src, t, 1, amps, &dtab))) return drop_sibling(h, rc);
  with_real(src, [&](auto x) {
    using R = decltype(x);
    using A = typename qh::AmpT<R>::type;
    qh::ExtendArgs a{};
    a.ib = src->nloc - qh::Item16<R>::kAmpBits;
    a.cw = std::min(qh::kResizeChunkBits, a.ib);
    a.nj = 1u << k;
    a.nchunks = 1ull << (a.ib - a.cw);
    const uint32_t gx = (uint32_t)std::min<uint64_t>(a.nchunks, qh::kResizeBlocks);
    // the slabs one trip of a block covers (more than one where src is smaller than a chunk), shared out over enough block
    // rows to fill the machine
    const uint32_t jstep = 1u << (qh::kResizeChunkBits - a.cw), units = (a.nj + jstep - 1) / jstep;
    uint32_t gy = std::min(units, std::max(1u, qh::kResizeBlocks / gx));
    a.jper = (units + gy - 1) / gy * jstep;
    gy = (a.nj + a.jper - 1) / a.jper;
    hipLaunchKernelGGL(qh::k_extend<R>, dim3(gx, gy), dim3(256), 0, src->stream, (const A *)src->d_psi, (A *)h->d_psi, (const A *)dtab, a);
  });
  rc = check_launch(src);
  if (rc == QH_OK && src->tab.commit(src->stream, 0) != hipSuccess) rc = fail(QH_ERR_HIP, "extend: hipEventRecord failed");
  if (rc == QH_OK) rc = wait_stream(src, src->stream, "qh_extend");
  if (rc) return drop_sibling(h, rc);
  count_resize(src, h);
  *out = h;
  return QH_OK;
}

int qh_release(qh_handle src, int k, const int32_t *bits, uint64_t value, double weight[2], qh_handle *out) {
  int rc = check_resize(src, out, "release", k, src ? src->nloc - k : 0);
  if (rc) return rc;
  if (!bits) return fail(QH_ERR_ARG, "release: null bit list");
  if (value >= (1ull << k)) return fail(QH_ERR_ARG, "release: value %llu of %d bits", (unsigned long long)value, k);
  uint64_t seen = 0;
  if ((rc = check_bit_list(src, "release", k, bits, &seen))) return rc;
  // (a logical bit stays local or in the shard index whatever the relayout sweeps do)
  for (int j = 0; j < k; ++j)
    if (place_bit(src, bits[j]).held)
      return fail(QH_ERR_NONLOCAL, "release: bit %d is held by the shard index (physical bit %d, local bits: %d); exchange first", bits[j],
                  src->perm[bits[j]], src->nloc);
  if ((rc = flush_impl(src))) return rc;
  qh::ReleasePlan pl;
  qh::plan_release(src->nloc, src->nglob, src->perm, k, bits, value, &pl);
  qh_state_s *h = nullptr;
  if ((rc = make_sibling(src, src->nloc - k, src->nglob - k, "release", &h))) return rc;
  memcpy(h->perm, pl.perm, sizeof h->perm);
  if (src->dry) {
    *out = h;
    return QH_OK;
  }
  qh::ReleaseArgs a{};
  a.drop = pl.drop;
  a.want = pl.want;
  a.nseg = pl.nseg;
  for (int s = 0; s < pl.nseg; ++s) {
    a.mask[s] = pl.mask[s];
    a.shift[s] = pl.shift[s];
  }
  const int ib = src->nloc - (src->bw == 128 ? 0 : 1);      // log2 of the 16-byte items of src
  a.cw = std::min(qh::kResizeChunkBits, ib);
  a.nchunks = 1ull << (ib - a.cw);
  const uint32_t nblk = (uint32_t)std::min<uint64_t>(a.nchunks, qh::kResizeBlocks);
  SlabSum sum{src};
  if (sum.reserve(nblk, 2, 2) != hipSuccess) return drop_sibling(h, fail(QH_ERR_NOMEM, "release: no room for %zu bytes of scratch", sum.bytes));
  with_real(src, [&](auto x) {
    using R = decltype(x);
    using A = typename qh::AmpT<R>::type;
    const A *from = (const A *)src->d_psi;
    A *to = (A *)h->d_psi;
    if (qh::Item16<R>::kAmpBits && (pl.drop & 1ull))      // a complex64 item loses one of its halves
      hipLaunchKernelGGL((qh::k_release<R, true>), dim3(nblk), dim3(256), 0, src->stream, from, to, a, sum.slab);
    else
      hipLaunchKernelGGL((qh::k_release<R, false>), dim3(nblk), dim3(256), 0, src->stream, from, to, a, sum.slab);
  });
  sum.fold(nblk, 2, 2);
  double vals[2];
  rc = check_launch(src);
  if (rc == QH_OK) rc = sum.get(vals, 2, "qh_release");
  if (rc) return drop_sibling(h, rc);
  if (weight) {
    weight[0] = vals[0];
    weight[1] = vals[1];
  }
  count_resize(src, h);
  *out = h;
  return QH_OK;
}

}  // extern "C"

// ---- Pauli-string expectations: qh_expect_pauli (kernels_expect.hip.h) -----------------------------------------------
namespace {

constexpr uint64_t kExpectBlocks = 4096;    // k_expect_batch: blocks at most (one slab row each)

template <typename R, int TT>
void launch_expect(qh_state_s *h, bool pair, unsigned nblk, const qh::ExpectArgs &a, double *slab) {
  using A = typename qh::AmpT<R>::type;
  if (pair)
    hipLaunchKernelGGL((qh::k_expect_batch<R, TT, true>), dim3(nblk), dim3(256), 0, h->stream, (const A *)h->d_psi, a, slab);
  else
    hipLaunchKernelGGL((qh::k_expect_batch<R, TT, false>), dim3(nblk), dim3(256), 0, h->stream, (const A *)h->d_psi, a, slab);
}

}  // namespace

extern "C" {

int qh_expect_pauli(qh_handle h, uint64_t nterms, const uint64_t *xmask, const uint64_t *zmask, double *out) {
  if (!h || (nterms && (!xmask || !zmask || !out))) return fail(QH_ERR_ARG, "expect_pauli: null handle, masks or out");
  if (h->nglob < 64)
    for (uint64_t t = 0; t < nterms; ++t)
      if ((xmask[t] | zmask[t]) >> h->nglob)
        return fail(QH_ERR_BAD_QUBIT, "expect_pauli: term %llu (x 0x%llx, z 0x%llx) has bits >= %d", (unsigned long long)t,
                    (unsigned long long)xmask[t], (unsigned long long)zmask[t], h->nglob);
  int rc = enter(h);
  if (rc) return rc;
  if (nterms == 0) return QH_OK;
  // masks through the bit map: local bits stay masks, a z bit the shard index holds is a sign fixed on this shard
  struct Term { uint64_t px, pz, idx; uint32_t neg, ny; };
  std::vector<Term> terms(nterms);
  for (uint64_t t = 0; t < nterms; ++t) {
    const Placed x = place(h, to_phys(h, xmask[t])), z = place(h, to_phys(h, zmask[t]));
    if (x.held) {
      const int b = __builtin_ctzll(to_logical(h, x.held << h->nloc));     // the first of them
      return fail(QH_ERR_NONLOCAL, "expect_pauli: term %llu has X or Y on logical bit %d, held by the shard index (physical bit %d, "
                  "local bits: %d); exchange first", (unsigned long long)t, b, h->perm[b], h->nloc);
    }
    terms[t] = Term{x.local, z.local, t, (uint32_t)__builtin_popcountll(h->shard & z.held) & 1u,
                    (uint32_t)__builtin_popcountll(xmask[t] & zmask[t]) & 3u};
  }
  // terms that share a physical x mask share a read of the state, kExpectT at a time
  std::stable_sort(terms.begin(), terms.end(), [](const Term &l, const Term &r) { return l.px < r.px; });
  SlabSum sum{h};
  HIP_TRY(sum.reserve(kExpectBlocks, qh::kExpectT, nterms));
  uint64_t batches = 0;
  for (uint64_t first = 0; first < nterms;) {
    uint64_t cnt = 1;
    while (first + cnt < nterms && cnt < (uint64_t)qh::kExpectT && terms[first + cnt].px == terms[first].px) ++cnt;
    const uint64_t px = terms[first].px;
    const bool pair = (px >> 6) != 0;
    qh::ExpectArgs a{};
    a.x = px;
    a.tb = pair ? 63 - __builtin_clzll(px) : 0;
    const int per_bits = pair ? 3 : 4, nom = 8 + per_bits, wbits = pair ? h->nloc - 1 : h->nloc;
    a.cw = std::min(nom, wbits);
    const uint64_t nchunks = 1ull << (wbits - a.cw), nblk = std::min(nchunks, kExpectBlocks);
    a.cpb = (uint32_t)(nchunks / nblk);
    for (uint64_t k = 0; k < cnt; ++k) {
      const Term &tm = terms[first + k];
      uint64_t z = tm.pz;     // in work-index bits: bit tb (0 in the i of every pair) squeezed out
      if (pair) z = (z & ((1ull << a.tb) - 1ull)) | ((z >> (a.tb + 1)) << a.tb);
      a.zt[k] = (uint8_t)(z & 255ull);
      const uint32_t zu = (uint32_t)(z >> 8) & ((1u << per_bits) - 1u);
      for (uint32_t u = 0; u < (1u << per_bits); ++u) a.zu[k] |= (uint16_t)((__builtin_popcount(u & zu) & 1) << u);
      a.zc[k] = z >> nom;
      const uint32_t one = (((tm.ny >> 1) ^ tm.neg) & 1u) ? 0xBFF00000u : 0x3FF00000u;     // nY mod 4: +Re, +Im, -Re, -Im
      if (tm.ny & 1u) a.cim[k] = one; else a.cre[k] = one;
    }
    const int tt = cnt <= 4 ? 4 : qh::kExpectT;
    with_real(h, [&](auto x) {
      using R = decltype(x);
      if (tt == 4) launch_expect<R, 4>(h, pair, (unsigned)nblk, a, sum.slab);
      else launch_expect<R, qh::kExpectT>(h, pair, (unsigned)nblk, a, sum.slab);
    });
    sum.fold(nblk, tt, (unsigned)cnt, pair ? 2.0 : 1.0, first);
    if ((rc = check_launch(h))) return rc;
    first += cnt;
    ++batches;
  }
  std::vector<double> vals(nterms);
  if ((rc = sum.get(vals.data(), nterms))) return rc;
  for (uint64_t k = 0; k < nterms; ++k) out[terms[k].idx] = vals[k];
  h->stats.kernels_launched += batches;      // reads of the state: one per batch
  h->stats.bytes_swept += batches * ((1ull << h->nloc) * h->amp_bytes());
  return QH_OK;
}

}  // extern "C"

// ---- Pauli-sum operators: qh_apply_pauli_sum, qh_pauli_sum_new, qh_pauli_sum_plan (kernels_pauli.hip.h, pauli_plan.h) ------
namespace {

// The terms on h's bit map as it is now, sorted (qh_apply_pauli_product: in the caller's order): masks checked against nglob,
// local bits as physical masks, a z bit the shard index holds as a sign, an x bit there refused.  Host arithmetic only: valid
// on dry handles.
int plan_pauli(const qh_state_s *h, const char *who, uint64_t nterms, const uint64_t *xmask, const uint64_t *zmask,
               std::vector<qh_pauli_term> *terms, bool sorted = true) {
  if (h->nglob < 64)
    for (uint64_t t = 0; t < nterms; ++t)
      if ((xmask[t] | zmask[t]) >> h->nglob)
        return fail(QH_ERR_BAD_QUBIT, "%s: term %llu (x 0x%llx, z 0x%llx) has bits >= %d", who, (unsigned long long)t,
                    (unsigned long long)xmask[t], (unsigned long long)zmask[t], h->nglob);
  terms->resize(nterms);
  for (uint64_t t = 0; t < nterms; ++t) {
    const Placed x = place(h, to_phys(h, xmask[t])), z = place(h, to_phys(h, zmask[t]));
    if (x.held) {
      const int b = __builtin_ctzll(to_logical(h, x.held << h->nloc));     // the first of them
      return fail(QH_ERR_NONLOCAL, "%s: term %llu has X or Y on logical bit %d, held by the shard index (physical bit %d, "
                  "local bits: %d); exchange first", who, (unsigned long long)t, b, h->perm[b], h->nloc);
    }
    (*terms)[t] = qh_pauli_term{t, x.local, z.local, (uint32_t)__builtin_popcountll(h->shard & z.held) & 1u,
                                (uint32_t)__builtin_popcountll(xmask[t] & zmask[t]) & 3u};
  }
  if (sorted) qh::pauli_sort(terms->data(), nterms);
  return QH_OK;
}

// one batch (count == 0: the kernel of zeros) on dst's stream
void launch_pauli_batch(qh_state_s *dst, const qh_state_s *src, const qh_pauli_term *terms, const double *coeffs, uint64_t count,
                        bool acc, bool norm, double *slab, uint64_t *nblk) {
  qh::PauliArgs a{};
  const int ab = dst->bw == 128 ? 0 : 1;
  for (uint64_t k = 0; k < count; ++k) {
    const qh_pauli_term &tm = terms[k];
    double c[2];
    qh::pauli_coef(coeffs[2 * tm.index], coeffs[2 * tm.index + 1], tm.ny, tm.neg, c);
    const qh::PauliZSplit z = qh::pauli_split_z(tm.pz, ab);
    a.px[k] = tm.px;
    a.pz[k] = tm.pz;
    a.zc[k] = (uint32_t)z.chunk;
    a.cre[k] = c[0];
    a.cim[k] = c[1];
    a.zu[k] = (uint16_t)z.reg;
    a.zt[k] = (uint8_t)z.thread;
    a.zh |= z.half << k;
    if (k == 0 || tm.px != terms[k - 1].px) a.start |= 1u << k;
    if (count == 1 && !acc) a.unit = 1 + qh::pauli_unit(c);
  }
  a.count = (int)count;
  a.acc = acc ? 1 : 0;
  a.norm = norm ? 1 : 0;
  with_real(dst, [&](auto x) {
    using R = decltype(x);
    if (qh::pauli_main_shape(dst->nloc, ab)) {
      using V = typename qh::Item16<R>::vec;
      const qh::PauliGrid g = qh::pauli_grid(dst->nloc, ab);
      a.cpb = g.cpb;
      *nblk = g.nblk;
      const bool few = count <= (uint64_t)qh::kPauliSmallT, one = (a.start & ~1u) == 0;      // (one x mask, or no term at all)
      const V *ps = (const V *)src->d_psi;
      V *pd = (V *)dst->d_psi;
      const dim3 grid((unsigned)g.nblk), block(256);
      if (few && one) hipLaunchKernelGGL((qh::k_pauli_batch<R, qh::kPauliSmallT, 1>), grid, block, 0, dst->stream, ps, pd, a, slab);
      else if (few) hipLaunchKernelGGL((qh::k_pauli_batch<R, qh::kPauliSmallT, qh::kPauliSmallT>), grid, block, 0, dst->stream, ps, pd, a, slab);
      else if (one) hipLaunchKernelGGL((qh::k_pauli_batch<R, qh::kPauliT, 1>), grid, block, 0, dst->stream, ps, pd, a, slab);
      else hipLaunchKernelGGL((qh::k_pauli_batch<R, qh::kPauliT, qh::kPauliT>), grid, block, 0, dst->stream, ps, pd, a, slab);
    } else {
      using A = typename qh::AmpT<R>::type;
      const uint64_t n = 1ull << dst->nloc;
      *nblk = (n + 255) / 256;
      hipLaunchKernelGGL((qh::k_pauli_small<R>), dim3((unsigned)*nblk), dim3(256), 0, dst->stream, (const A *)src->d_psi, (A *)dst->d_psi, a, n,
                         slab);
    }
  });
}

int check_pauli_arrays(const char *who, uint64_t nterms, const double *coeffs, const uint64_t *xmask, const uint64_t *zmask) {
  if (nterms && (!coeffs || !xmask || !zmask)) return fail(QH_ERR_ARG, "%s: null coefficients or masks with %llu terms", who, (unsigned long long)nterms);
  return QH_OK;
}

}  // namespace

extern "C" {

int qh_pauli_sum_plan(qh_handle src, uint64_t nterms, const uint64_t *xmask, const uint64_t *zmask, qh_pauli_term *terms,
                      qh_pauli_batch *batches, uint64_t cap, uint64_t *nbatches) {
  if (!src || !nbatches || (nterms && (!xmask || !zmask)) || (cap && !batches))
    return fail(QH_ERR_ARG, "pauli_sum_plan: null handle, masks, batches or nbatches");
  std::vector<qh_pauli_term> tv;
  const int rc = plan_pauli(src, "pauli_sum_plan", nterms, xmask, zmask, &tv);
  if (rc) return rc;
  if (terms && nterms) memcpy(terms, tv.data(), nterms * sizeof(qh_pauli_term));
  *nbatches = qh::pauli_cut(tv.data(), nterms, batches, cap);
  return QH_OK;
}

int qh_apply_pauli_sum(qh_handle dst, qh_handle src, uint64_t nterms, const double *coeffs, const uint64_t *xmask,
                       const uint64_t *zmask, double *norm2) {
  int rc = check_pair(dst, src, "apply_pauli_sum");
  if (rc) return rc;
  if ((rc = check_pauli_arrays("apply_pauli_sum", nterms, coeffs, xmask, zmask))) return rc;
  if (dst == src) return fail(QH_ERR_ARG, "apply_pauli_sum: dst == src (the operator is applied out of place)");
  if (dst->shard != src->shard)
    return fail(QH_ERR_ARG, "apply_pauli_sum: shard %llu against shard %llu", (unsigned long long)dst->shard, (unsigned long long)src->shard);
  std::vector<qh_pauli_term> terms;
  // which bits the shard index holds is not something a flush changes: refused before anything runs
  if ((rc = plan_pauli(src, "apply_pauli_sum", nterms, xmask, zmask, &terms))) return rc;
  if ((rc = enter(src))) return rc;
  if ((rc = plan_pauli(src, "apply_pauli_sum", nterms, xmask, zmask, &terms))) return rc;      // the layout the flush left
  std::vector<qh_pauli_batch> batches(qh::pauli_cut(terms.data(), nterms, nullptr, 0));
  qh::pauli_cut(terms.data(), nterms, batches.data(), batches.size());
  // dst is replaced whole, as by qh_copy
  dst->queue.clear();
  dst->poisoned = false;
  if (dst->comm) qh::wait_all_arrivals(&dst->comm->arrivals, dst->stream);
  if ((rc = wait_stream(dst, dst->stream, "qh_apply_pauli_sum"))) return rc;
  SlabSum sum{dst};
  if (norm2) HIP_TRY(sum.reserve(std::max<uint64_t>(qh::kPauliBlocks, 8), 1, 1));
  if ((rc = order_after(dst, src))) return rc;      // dst's stream reads src: behind everything src's stream has been given
  uint64_t nblk = 1, streams = 0;
  if (batches.empty()) {
    launch_pauli_batch(dst, src, nullptr, coeffs, 0, false, norm2 != nullptr, sum.slab, &nblk);
    streams = 1;
  }
  for (size_t b = 0; b < batches.size(); ++b) {
    launch_pauli_batch(dst, src, terms.data() + batches[b].first, coeffs, batches[b].count, b > 0, norm2 && b + 1 == batches.size(), sum.slab,
                       &nblk);
    streams += batches[b].streams;
  }
  if (norm2) sum.fold(nblk, 1, 1);
  if ((rc = check_launch(dst))) return rc;
  // the host waits: on return src may be changed and dst read at once
  if (norm2) rc = sum.get(norm2, 1, "qh_apply_pauli_sum");
  else rc = wait_stream(dst, dst->stream, "qh_apply_pauli_sum");
  if (rc) return rc;
  memcpy(dst->perm, src->perm, sizeof dst->perm);      // written in src's physical layout
  const uint64_t shard_bytes = (1ull << dst->nloc) * dst->amp_bytes();
  dst->stats.kernels_launched += batches.empty() ? 1 : batches.size();      // (the fold is not counted, as in qh_axpby)
  dst->stats.bytes_swept += streams * shard_bytes;
  dst->stats.bytes_algorithmic += (batches.empty() ? 1 : 2) * shard_bytes;
  return QH_OK;
}

int qh_pauli_sum_new(qh_handle src, uint64_t nterms, const double *coeffs, const uint64_t *xmask, const uint64_t *zmask,
                     double *norm2, qh_handle *out) {
  if (!src || !out) return fail(QH_ERR_ARG, "pauli_sum_new: null handle or out");
  if (src->dry) return fail(QH_ERR_ARG, "pauli_sum_new: not on a dry (planner-only) handle");
  int rc = check_pauli_arrays("pauli_sum_new", nterms, coeffs, xmask, zmask);
  if (rc) return rc;
  std::vector<qh_pauli_term> terms;
  if ((rc = plan_pauli(src, "pauli_sum_new", nterms, xmask, zmask, &terms))) return rc;      // refused before anything is made
  if ((rc = use_device(src))) return rc;
  qh_state_s *h = nullptr;
  if ((rc = make_sibling(src, src->nloc, src->nglob, "pauli_sum_new", &h))) return rc;
  if ((rc = qh_apply_pauli_sum(h, src, nterms, coeffs, xmask, zmask, norm2))) return drop_sibling(h, rc);
  *out = h;
  return QH_OK;
}

}  // extern "C"

// ---- Pauli products: qh_apply_pauli_product, qh_pauli_product_plan (kernels_pauli_product.hip.h, pauli_product_plan.h) ------
namespace {

// the terms in the caller's order on h's bit map as it is now, and their runs
int plan_pauli_product(const qh_state_s *h, const char *who, uint64_t nterms, const uint64_t *xmask, const uint64_t *zmask,
                       std::vector<qh_pauli_term> *terms, std::vector<qh_pauli_run> *runs) {
  const int rc = plan_pauli(h, who, nterms, xmask, zmask, terms, false);
  if (rc) return rc;
  const int ab = h->bw == 128 ? 0 : 1;
  runs->resize(qh::pauli_product_cut(terms->data(), nterms, ab, nullptr, 0));
  qh::pauli_product_cut(terms->data(), nterms, ab, runs->data(), runs->size());
  return QH_OK;
}

// kind: QH_PAULI_RUN_* of the plan, or qh::kPauliWalkLane for a PAIR run whose pairs lie inside a wave
template <typename R, int TT>
void launch_pauli_product_kind(qh_state_s *h, uint32_t kind, unsigned nblk, const qh::PauliProdArgs &a, double *slab) {
  using V = typename qh::Item16<R>::vec;
  V *psi = (V *)h->d_psi;
  const dim3 grid(nblk), block(256);
  if (kind == QH_PAULI_RUN_DIAG) hipLaunchKernelGGL((qh::k_pauli_product<R, TT, QH_PAULI_RUN_DIAG>), grid, block, 0, h->stream, psi, a, slab);
  else if (kind == QH_PAULI_RUN_PAIR) hipLaunchKernelGGL((qh::k_pauli_product<R, TT, QH_PAULI_RUN_PAIR>), grid, block, 0, h->stream, psi, a, slab);
  else if (kind == (uint32_t)qh::kPauliWalkLane) hipLaunchKernelGGL((qh::k_pauli_product<R, TT, qh::kPauliWalkLane>), grid, block, 0, h->stream, psi, a, slab);
  else if constexpr (qh::Item16<R>::kAmpBits == 1)
    hipLaunchKernelGGL((qh::k_pauli_product<R, TT, QH_PAULI_RUN_HALF>), grid, block, 0, h->stream, psi, a, slab);
}

// one run on h's stream
void launch_pauli_run(qh_state_s *h, const qh_pauli_run &run, const qh_pauli_term *terms, const double *coef, bool norm, double *slab,
                      uint64_t *nblk) {
  qh::PauliProdArgs a{};
  qh::PauliProdZ zs{};      // (k_pauli_product_small alone)
  const int ab = h->bw == 128 ? 0 : 1;
  const bool main_shape = qh::pauli_product_main_shape(h->nloc, ab);
  const bool lane = run.kind == QH_PAULI_RUN_PAIR && qh::pauli_pair_in_wave(run.px, ab);      // walks items; the partner by a lane exchange
  const bool pair = run.kind == QH_PAULI_RUN_PAIR && !lane;                                     // walks pair numbers
  a.X = run.px;
  if (main_shape) a.pivot = pair ? qh::pauli_pair_pivot(run.px, ab) : 0;
  else a.pivot = run.px ? 63 - __builtin_clzll(run.px) : 0;
  for (uint64_t k = 0; k < run.count; ++k) {
    const qh_pauli_term &tm = terms[run.first + k];
    const double *c = coef + 4 * tm.index;
    double b[2];
    qh::pauli_coef(c[2], c[3], tm.ny, tm.neg, b);
    // PAIR walks pair numbers: the z mask over them (the pivot bit, clear in item0, removed)
    const qh::PauliZSplit z = qh::pauli_split_z(main_shape && pair ? qh::pauli_pair_z(tm.pz, a.pivot, ab) : tm.pz, ab);
    a.are[k] = c[0];
    a.aim[k] = c[1];
    a.bre[k] = b[0];
    a.bim[k] = b[1];
    zs.pz[k] = tm.pz;
    a.zc[k] = (uint32_t)z.chunk;
    a.zu[k] = (uint16_t)z.reg;
    a.zt[k] = (uint8_t)z.thread;
    a.zh |= z.half << k;
    if (tm.px) a.offd |= 1u << k;
    a.flip |= qh::pauli_pair_flip(run.px, tm.pz) << k;
    if (run.count == 1) {
      if (c[0] == 0.0 && c[1] == 0.0) a.unit = 1 + qh::pauli_unit(b);
      else if (c[0] == 1.0 && c[1] == 0.0 && c[2] == 0.0 && c[3] == 0.0) a.unit = 5;
    }
  }
  a.count = (int)run.count;
  a.norm = norm ? 1 : 0;
  with_real(h, [&](auto x) {
    using R = decltype(x);
    if (main_shape) {
      const qh::PauliGrid g = qh::pauli_product_grid(h->nloc, ab, pair);
      const uint32_t kind = lane ? (uint32_t)qh::kPauliWalkLane : run.kind;
      a.cpb = g.cpb;
      *nblk = g.nblk;
      if (run.count <= (uint64_t)qh::kPauliProdSmallT) launch_pauli_product_kind<R, qh::kPauliProdSmallT>(h, kind, (unsigned)g.nblk, a, slab);
      else if (qh::kPauliProdT > qh::kPauliProdMidT && run.count <= (uint64_t)qh::kPauliProdMidT)      // (A/B builds with 16 slots)
        launch_pauli_product_kind<R, qh::kPauliProdMidT>(h, kind, (unsigned)g.nblk, a, slab);
      else launch_pauli_product_kind<R, qh::kPauliProdT>(h, kind, (unsigned)g.nblk, a, slab);
    } else {
      using A = typename qh::AmpT<R>::type;
      const uint64_t nwork = 1ull << (run.px ? h->nloc - 1 : h->nloc);
      *nblk = (nwork + 255) / 256;
      hipLaunchKernelGGL((qh::k_pauli_product_small<R>), dim3((unsigned)*nblk), dim3(256), 0, h->stream, (A *)h->d_psi, a, zs, nwork, slab);
    }
  });
}

}  // namespace

extern "C" {

int qh_pauli_product_plan(qh_handle h, uint64_t nterms, const uint64_t *xmask, const uint64_t *zmask, qh_pauli_term *terms,
                          qh_pauli_run *runs, uint64_t cap, uint64_t *nruns) {
  if (!h || !nruns || (nterms && (!xmask || !zmask)) || (cap && !runs))
    return fail(QH_ERR_ARG, "pauli_product_plan: null handle, masks, runs or nruns");
  std::vector<qh_pauli_term> tv;
  std::vector<qh_pauli_run> rv;
  const int rc = plan_pauli_product(h, "pauli_product_plan", nterms, xmask, zmask, &tv, &rv);
  if (rc) return rc;
  if (terms && nterms) memcpy(terms, tv.data(), nterms * sizeof(qh_pauli_term));
  for (uint64_t r = 0; r < rv.size() && r < cap; ++r) runs[r] = rv[r];
  *nruns = rv.size();
  return QH_OK;
}

int qh_apply_pauli_product(qh_handle h, uint64_t nterms, const double *ab, const uint64_t *xmask, const uint64_t *zmask, double *norm2) {
  if (!h) return fail(QH_ERR_ARG, "apply_pauli_product: null handle");
  if (nterms && (!ab || !xmask || !zmask))
    return fail(QH_ERR_ARG, "apply_pauli_product: null coefficients or masks with %llu terms", (unsigned long long)nterms);
  for (uint64_t t = 0; t < nterms; ++t)
    for (int j = 0; j < 4; ++j)
      if (!std::isfinite(ab[4 * t + j]))
        return fail(QH_ERR_ARG, "apply_pauli_product: term %llu has a non-finite coefficient (a = %g%+gi, b = %g%+gi)", (unsigned long long)t,
                    ab[4 * t], ab[4 * t + 1], ab[4 * t + 2], ab[4 * t + 3]);
  std::vector<qh_pauli_term> terms;
  std::vector<qh_pauli_run> runs;
  // which bits the shard index holds is not something a flush changes: the whole list is refused before anything runs
  int rc = plan_pauli_product(h, "apply_pauli_product", nterms, xmask, zmask, &terms, &runs);
  if (rc) return rc;
  if (h->dry) return fail(QH_ERR_ARG, "apply_pauli_product: not on a dry (planner-only) handle");
  if ((rc = enter(h))) return rc;          // a barrier: what is queued runs first, on whatever layout it leaves
  if (nterms == 0) return norm2 ? masked_norm2(h, 0ull, 0ull, norm2) : QH_OK;
  if ((rc = plan_pauli_product(h, "apply_pauli_product", nterms, xmask, zmask, &terms, &runs))) return rc;
  SlabSum sum{h};
  if (norm2) HIP_TRY(sum.reserve(std::max<uint64_t>(qh::kPauliBlocks, 8), 1, 1));
  uint64_t nblk = 1;
  for (size_t r = 0; r < runs.size(); ++r)
    launch_pauli_run(h, runs[r], terms.data(), ab, norm2 && r + 1 == runs.size(), sum.slab, &nblk);
  if (norm2) sum.fold(nblk, 1, 1);
  if ((rc = check_launch(h))) return rc;
  if (norm2 && (rc = sum.get(norm2, 1, "qh_apply_pauli_product"))) return rc;
  const uint64_t shard_bytes = (1ull << h->nloc) * h->amp_bytes();
  h->stats.gates_submitted += nterms;
  h->stats.kernels_launched += runs.size();      // (the fold is not counted, as in qh_axpby)
  h->stats.bytes_swept += 2 * runs.size() * shard_bytes;
  h->stats.bytes_algorithmic += 2 * runs.size() * shard_bytes;
  return QH_OK;
}

}  // extern "C"

// ---- Z-polynomial operators: qh_apply_zpoly, qh_expect_zpoly, qh_zpoly_plan (kernels_zpoly.hip.h, zpoly_plan.h) ------------
namespace {

// Argument checks of the three calls, then the terms on h's bit map as it is now (masks through the bit map, the shard's
// sign folded into the weight) and their plan.  Host arithmetic only: valid on dry handles.
int check_zpoly(const qh_state_s *h, const char *who, uint64_t nterms, const double *w, const uint64_t *zmask) {
  if (!h) return fail(QH_ERR_ARG, "%s: null handle", who);
  if (nterms && (!w || !zmask)) return fail(QH_ERR_ARG, "%s: null weights or masks with %llu terms", who, (unsigned long long)nterms);
  if (nterms > QH_ZPOLY_MAX_TERMS)
    return fail(QH_ERR_ARG, "%s: %llu terms (at most %d)", who, (unsigned long long)nterms, QH_ZPOLY_MAX_TERMS);
  for (uint64_t t = 0; t < nterms; ++t) {
    if (!std::isfinite(w[t])) return fail(QH_ERR_ARG, "%s: term %llu has a non-finite weight (%g)", who, (unsigned long long)t, w[t]);
    if (h->nglob < 64 && (zmask[t] >> h->nglob))
      return fail(QH_ERR_BAD_QUBIT, "%s: term %llu (z 0x%llx) has bits >= %d", who, (unsigned long long)t, (unsigned long long)zmask[t],
                  h->nglob);
  }
  return QH_OK;
}

void plan_zpoly(const qh_state_s *h, uint64_t nterms, const double *w, const uint64_t *zmask, std::vector<qh::ZpolyTerm> *terms,
                qh::ZpolyPlan *plan) {
  terms->resize(nterms);
  for (uint64_t t = 0; t < nterms; ++t) {
    const Placed z = place(h, to_phys(h, zmask[t]));
    (*terms)[t] = qh::ZpolyTerm{(__builtin_popcountll(h->shard & z.held) & 1) ? -w[t] : w[t], z.local};
  }
  qh::zpoly_plan(terms->data(), nterms, h->nloc, h->bw == 128 ? 0 : 1, plan);
}

// the block into the pinned slot and from there, on the handle's stream, to the device; a filled in with where its parts are
int stage_zpoly(qh_state_s *h, const qh::ZpolyPlan &p, const char *who, qh::ZpolyArgs *a) {
  char *host = nullptr, *d = nullptr;
  unsigned slot = 0;
  const int rc = acquire(h, h->zpoly, qh::kZpolyBlockBytes, who, &host, &d, &slot);
  if (rc) return rc;
  const size_t wb = p.wd.size() * 8, mb = p.md.size() * 8;
  if (wb) memcpy(host, p.wd.data(), wb);
  if (mb) memcpy(host + wb, p.md.data(), mb);
  HIP_TRY(hipMemcpyAsync(d, host, wb + mb, hipMemcpyHostToDevice, h->stream));
  a->wd = (const double *)d;
  a->md = (const uint64_t *)(d + wb);
  a->nseg = p.nseg;
  a->nlow = (uint32_t)p.nlow;
  a->nterms = p.nterms;
  a->nseg_terms = p.nseg_terms;
  a->cached = p.main && p.nseg_terms <= qh::kZpolyLdsTerms ? 1u : 0u;
  a->ngt = p.ngt;
  a->ngu = p.ngu;
  a->off_lw = p.off_lw;
  a->off_sc = p.off_sc;
  a->off_gl = p.off_gl;
  a->off_lm = p.off_lm;
  a->cpb = p.cpb;
  return QH_OK;
}

// one kernel on h's stream: the apply (expect == false) or the three moments
void launch_zpoly(qh_state_s *h, const qh::ZpolyPlan &p, const qh::ZpolyArgs &a, bool expect, double *slab) {
  with_real(h, [&](auto x) {
    using R = decltype(x);
    const dim3 grid((unsigned)p.nblk), block(256);
    if (p.main) {
      using V = typename qh::Item16<R>::vec;
      const size_t lds = qh::zpoly_lds_bytes(p.nseg, p.nseg_terms, a.cached != 0);
      if (expect) hipLaunchKernelGGL((qh::k_zpoly_expect<R>), grid, block, lds, h->stream, (const V *)h->d_psi, a, slab);
      else hipLaunchKernelGGL((qh::k_zpoly_apply<R>), grid, block, lds, h->stream, (V *)h->d_psi, a, slab);
    } else {
      using A = typename qh::AmpT<R>::type;
      const uint64_t n = 1ull << h->nloc;
      if (expect) hipLaunchKernelGGL((qh::k_zpoly_small<R, true>), grid, block, 0, h->stream, (A *)h->d_psi, a, n, slab);
      else hipLaunchKernelGGL((qh::k_zpoly_small<R, false>), grid, block, 0, h->stream, (A *)h->d_psi, a, n, slab);
    }
  });
}

}  // namespace

extern "C" {

int qh_zpoly_plan(qh_handle h, uint64_t nterms, const double *w, const uint64_t *zmask, qh_zpoly_info *out) {
  int rc = check_zpoly(h, "zpoly_plan", nterms, w, zmask);
  if (rc) return rc;
  if (!out) return fail(QH_ERR_ARG, "zpoly_plan: null out");
  std::vector<qh::ZpolyTerm> terms;
  qh::ZpolyPlan p;
  plan_zpoly(h, nterms, w, zmask, &terms, &p);
  memset(out, 0, sizeof *out);
  out->nterms = nterms;
  out->nconst = p.nconst;
  out->nhigh = p.nhigh;
  out->nlow = p.nlow;
  out->nstraddle = p.nstraddle;
  out->ngroups = p.group_mask.size();
  out->nblk = p.nblk;
  out->kernel = p.main ? QH_ZPOLY_KERNEL_MAIN : QH_ZPOLY_KERNEL_SMALL;
  out->low_bits = (uint32_t)p.low_bits;
  out->cpb = p.cpb;
  for (size_t g = 0; g < p.group_mask.size(); ++g) out->group_mask[g] = p.group_mask[g];
  for (uint64_t t = 0; t < nterms; ++t) {
    out->pz[t] = terms[t].pz;
    out->w[t] = terms[t].w;
    out->cls[t] = p.cls[t];
  }
  return QH_OK;
}

int qh_apply_zpoly(qh_handle h, uint64_t nterms, const double *w, const uint64_t *zmask, const double c[2], double *norm2) {
  int rc = check_zpoly(h, "apply_zpoly", nterms, w, zmask);
  if (rc) return rc;
  if (!c) return fail(QH_ERR_ARG, "apply_zpoly: null c");
  if (!std::isfinite(c[0]) || !std::isfinite(c[1])) return fail(QH_ERR_ARG, "apply_zpoly: c = %g%+gi is not finite", c[0], c[1]);
  if (h->dry) return fail(QH_ERR_ARG, "apply_zpoly: not on a dry (planner-only) handle");
  if ((rc = enter(h))) return rc;          // a barrier: what is queued runs first, on whatever layout it leaves
  if (nterms == 0 || (c[0] == 0.0 && c[1] == 0.0)) return norm2 ? masked_norm2(h, 0ull, 0ull, norm2) : QH_OK;
  std::vector<qh::ZpolyTerm> terms;
  qh::ZpolyPlan p;
  plan_zpoly(h, nterms, w, zmask, &terms, &p);
  qh::ZpolyArgs a{};
  if ((rc = stage_zpoly(h, p, "qh_apply_zpoly", &a))) return rc;
  a.cre = c[0];
  a.cim = c[1];
  a.norm = norm2 ? 1 : 0;
  SlabSum sum{h};
  if (norm2) HIP_TRY(sum.reserve(std::max<uint64_t>(qh::kPauliBlocks, 8), 1, 1));
  launch_zpoly(h, p, a, false, sum.slab);
  if (norm2) sum.fold(p.nblk, 1, 1);
  if ((rc = check_launch(h))) return rc;
  HIP_TRY(h->zpoly.commit(h->stream, 0));
  if (norm2 && (rc = sum.get(norm2, 1, "qh_apply_zpoly"))) return rc;
  const uint64_t shard_bytes = (1ull << h->nloc) * h->amp_bytes();
  h->stats.gates_submitted += 1;
  h->stats.kernels_launched += 1;      // (the fold is not counted, as in qh_axpby)
  h->stats.bytes_swept += 2 * shard_bytes;
  h->stats.bytes_algorithmic += 2 * shard_bytes;
  return QH_OK;
}

int qh_expect_zpoly(qh_handle h, uint64_t nterms, const double *w, const uint64_t *zmask, double out[3]) {
  int rc = check_zpoly(h, "expect_zpoly", nterms, w, zmask);
  if (rc) return rc;
  if (!out) return fail(QH_ERR_ARG, "expect_zpoly: null out");
  if (h->dry) return fail(QH_ERR_ARG, "expect_zpoly: not on a dry (planner-only) handle");
  if ((rc = enter(h))) return rc;
  if (nterms == 0) {
    double n2 = 0.0;
    if ((rc = masked_norm2(h, 0ull, 0ull, &n2))) return rc;
    out[0] = n2;
    out[1] = out[2] = 0.0;
    return QH_OK;
  }
  std::vector<qh::ZpolyTerm> terms;
  qh::ZpolyPlan p;
  plan_zpoly(h, nterms, w, zmask, &terms, &p);
  qh::ZpolyArgs a{};
  if ((rc = stage_zpoly(h, p, "qh_expect_zpoly", &a))) return rc;
  SlabSum sum{h};
  HIP_TRY(sum.reserve(std::max<uint64_t>(qh::kPauliBlocks, 8), 3, 3));
  launch_zpoly(h, p, a, true, sum.slab);
  sum.fold(p.nblk, 3, 3);
  if ((rc = check_launch(h))) return rc;
  HIP_TRY(h->zpoly.commit(h->stream, 0));
  if ((rc = sum.get(out, 3, "qh_expect_zpoly"))) return rc;
  const uint64_t shard_bytes = (1ull << h->nloc) * h->amp_bytes();
  h->stats.kernels_launched += 1;
  h->stats.bytes_swept += shard_bytes;
  h->stats.bytes_algorithmic += shard_bytes;
  return QH_OK;
}

}  // extern "C"

// ---- matrix elements between two states: qh_transition_pauli, qh_transition_plan (kernels_transition.hip.h, transition_plan.h)
namespace {

struct TransitionPlan {
  qh_inner_tiles walk;
  std::vector<qh_pauli_term> terms;
  std::vector<qh_transition_pass> passes;
};

int check_transition_args(const qh_state_s *a, const qh_state_s *b, const char *who, uint64_t nterms, const uint64_t *xmask,
                          const uint64_t *zmask) {
  if (!a || !b) return fail(QH_ERR_ARG, "%s: null handle", who);
  if (nterms && (!xmask || !zmask)) return fail(QH_ERR_ARG, "%s: null masks with %llu terms", who, (unsigned long long)nterms);
  if (a->nloc != b->nloc || a->nglob != b->nglob || a->bw != b->bw)
    return fail(QH_ERR_ARG, "%s: %d of %d qubits at width %d against %d of %d at width %d", who, a->nloc, a->nglob, a->bw, b->nloc,
                b->nglob, b->bw);
  return QH_OK;
}

// The strings on the two bit maps as they are now (transition_plan.h).  Host arithmetic only: valid on dry handles.
int plan_transition_for(const qh_state_s *a, const qh_state_s *b, const char *who, uint64_t nterms, const uint64_t *xmask,
                        const uint64_t *zmask, TransitionPlan *p) {
  qh::TransitionRefusal why;
  const int rc = qh::plan_transition(a->nloc, a->nglob, a->bw, a->perm, b->perm, a->shard, b->shard, nterms, xmask, zmask, &p->walk,
                                     &p->terms, &p->passes, &why);
  switch (why.kind) {
    case qh::TransitionRefusal::kNone: break;
    case qh::TransitionRefusal::kMaskRange:
      return fail(rc, "%s: term %llu (x 0x%llx, z 0x%llx) has bits >= %d", who, (unsigned long long)why.term,
                  (unsigned long long)xmask[why.term], (unsigned long long)zmask[why.term], a->nglob);
    case qh::TransitionRefusal::kShardIndex:
      return fail(rc, "%s: shard %llu against shard %llu; exchange first", who, (unsigned long long)a->shard, (unsigned long long)b->shard);
    case qh::TransitionRefusal::kSplitBit:
      return fail(rc, "%s: logical bit %d is at physical bit %d of one handle and %d of the other, and the shard index holds one of "
                  "them (local bits: %d); exchange first", who, why.bit, a->perm[why.bit], b->perm[why.bit], a->nloc);
    case qh::TransitionRefusal::kXHeld:
      return fail(rc, "%s: term %llu has X or Y on logical bit %d, held by the shard index (physical bit %d, local bits: %d); "
                  "exchange first", who, (unsigned long long)why.term, why.bit, b->perm[why.bit], a->nloc);
  }
  return rc;
}

template <typename R, int TT>
void launch_transition_tt(qh_state_s *a, const qh_state_s *b, const qh_inner_tiles &walk, qh::TransArgs ta, double *slab, uint64_t *nblk) {
  using A = typename qh::AmpT<R>::type;
  const A *pa = (const A *)a->d_psi, *pb = (const A *)b->d_psi;
  *nblk = 1;
  if (walk.path == QH_INNER_LINEAR) {
    const LinearGrid g = linear_grid(a->nloc - qh::Item16<R>::kAmpBits);
    ta.cw = g.cw;
    ta.cpb = g.cpb;
    *nblk = g.nblk;
    hipLaunchKernelGGL((qh::k_trans_linear<R, TT>), dim3((unsigned)g.nblk), dim3(256), 0, a->stream, pa, pb, ta, slab);
  } else if (walk.path == QH_INNER_TILES) {
    const qh::InnerTileArgs t = tile_args(walk, nblk);
    hipLaunchKernelGGL((qh::k_trans_tiles<R, TT>), dim3((unsigned)*nblk), dim3(256), 0, a->stream, pa, pb, ta, t, slab);
  } else {
    qh::InnerGatherArgs g{};
    g.nloc = a->nloc;
    memcpy(g.pos_b, walk.pos_b, sizeof g.pos_b);
    hipLaunchKernelGGL((qh::k_trans_gather<R, TT>), dim3(1), dim3(256), 0, a->stream, pa, pb, ta, g, slab);
  }
}

// one pass on a's stream: its strings' signs split as the walk's kernel takes them.  Returns the columns of a slab row
// (2 per string of the instantiation) and the blocks launched.
int launch_transition_pass(qh_state_s *a, const qh_state_s *b, const TransitionPlan &p, const qh_transition_pass &pass, double *slab,
                           uint64_t *nblk) {
  qh::TransArgs ta{};
  ta.px = pass.px;
  const int ab = a->bw == 128 ? 0 : 1;
  for (uint64_t k = 0; k < pass.count; ++k) {
    const uint64_t pz = p.terms[pass.first + k].pz;
    qh::TransZSplit z{};
    if (p.walk.path == QH_INNER_LINEAR) z = qh::transition_split_linear(pz, ab);
    else if (p.walk.path == QH_INNER_TILES) z = qh::transition_split_tiles(pz, p.walk);
    else z.thread = (uint32_t)pz;
    ta.zc[k] = z.uniform;
    ta.zu[k] = (uint8_t)z.reg;
    ta.zt[k] = (uint8_t)z.thread;
    ta.zh |= z.half << k;
  }
  const bool few = pass.count <= (uint64_t)qh::kTransSmallT;
  if (a->bw == 128) {
    if (few) launch_transition_tt<double, qh::kTransSmallT>(a, b, p.walk, ta, slab, nblk);
    else launch_transition_tt<double, qh::kTransT>(a, b, p.walk, ta, slab, nblk);
    return 2 * (few ? qh::kTransSmallT : qh::kTransT);
  }
  if (few) launch_transition_tt<float, qh::kTransSmallT>(a, b, p.walk, ta, slab, nblk);
  else launch_transition_tt<float, qh::kTransT64>(a, b, p.walk, ta, slab, nblk);
  return 2 * (few ? qh::kTransSmallT : qh::kTransT64);
}

}  // namespace

extern "C" {

int qh_transition_plan(qh_handle a, qh_handle b, uint64_t nterms, const uint64_t *xmask, const uint64_t *zmask, qh_pauli_term *terms,
                       qh_transition_pass *passes, uint64_t cap, uint64_t *npasses) {
  int rc = check_transition_args(a, b, "transition_plan", nterms, xmask, zmask);
  if (rc) return rc;
  if (!npasses || (cap && !passes)) return fail(QH_ERR_ARG, "transition_plan: null passes or npasses");
  TransitionPlan p;
  if ((rc = plan_transition_for(a, b, "transition_plan", nterms, xmask, zmask, &p))) return rc;
  if (terms && nterms) memcpy(terms, p.terms.data(), nterms * sizeof(qh_pauli_term));
  for (uint64_t k = 0; k < p.passes.size() && k < cap; ++k) passes[k] = p.passes[k];
  *npasses = p.passes.size();
  return QH_OK;
}

int qh_transition_pauli(qh_handle a, qh_handle b, uint64_t nterms, const uint64_t *xmask, const uint64_t *zmask, double *out) {
  int rc = check_transition_args(a, b, "transition_pauli", nterms, xmask, zmask);
  if (rc) return rc;
  if (nterms && !out) return fail(QH_ERR_ARG, "transition_pauli: null out with %llu terms", (unsigned long long)nterms);
  if (a->nglob < 64)
    for (uint64_t t = 0; t < nterms; ++t)
      if ((xmask[t] | zmask[t]) >> a->nglob)
        return fail(QH_ERR_BAD_QUBIT, "transition_pauli: term %llu (x 0x%llx, z 0x%llx) has bits >= %d", (unsigned long long)t,
                    (unsigned long long)xmask[t], (unsigned long long)zmask[t], a->nglob);
  if ((rc = check_pair(a, b, "transition_pauli"))) return rc;      // (dry handles, another device)
  TransitionPlan p;
  // which bits the shard index holds is not something a flush changes: refused before anything runs
  if ((rc = plan_transition_for(a, b, "transition_pauli", nterms, xmask, zmask, &p))) return rc;
  if ((rc = enter(a))) return rc;
  if (b != a && (rc = enter(b))) return rc;
  if (nterms == 0) return QH_OK;
  if ((rc = plan_transition_for(a, b, "transition_pauli", nterms, xmask, zmask, &p))) return rc;      // the layouts the flushes left
  SlabSum sum{a};
  HIP_TRY(sum.reserve(kInnerBlocks, 2 * qh::kTransT, 2 * nterms));
  if (b != a && (rc = order_after(a, b))) return rc;      // a's stream reads b: behind everything b's stream has been given
  for (const qh_transition_pass &pass : p.passes) {
    uint64_t nblk = 1;
    const int cols = launch_transition_pass(a, b, p, pass, sum.slab, &nblk);
    sum.fold(nblk, cols, (unsigned)(2 * pass.count), 1.0, 2 * pass.first);
    if ((rc = check_launch(a))) return rc;
  }
  std::vector<double> vals(2 * nterms);
  if ((rc = sum.get(vals.data(), vals.size(), "qh_transition_pauli"))) return rc;
  for (uint64_t k = 0; k < nterms; ++k) {      // (-i)^nY and the shard sign: swaps and negations
    const qh_pauli_term &tm = p.terms[k];
    qh::pauli_coef(vals[2 * k], vals[2 * k + 1], tm.ny, tm.neg, out + 2 * tm.index);
  }
  const uint64_t bytes = p.passes.size() * 2 * ((1ull << a->nloc) * a->amp_bytes());
  a->stats.kernels_launched += p.passes.size();      // reads of the two states: one per pass (the folds are not counted)
  a->stats.bytes_swept += bytes;
  a->stats.bytes_algorithmic += bytes;
  return QH_OK;
}

int qh_get_stats(qh_handle h, qh_stats *out) {
  if (!h || !out) return fail(QH_ERR_ARG, "null");
  *out = h->stats;
  return QH_OK;
}
int qh_reset_stats(qh_handle h) {
  if (!h) return fail(QH_ERR_ARG, "null");
  h->stats = qh_stats{};
  return QH_OK;
}

int qh_timer_begin(qh_handle h) {
  if (!h) return fail(QH_ERR_ARG, "null handle");
  int rc = enter(h);
  if (rc) return rc;
  rc = make_events(h);
  if (rc) return rc;
  HIP_TRY(hipEventRecord(h->ev0, h->stream));
  return QH_OK;
}
int qh_timer_end(qh_handle h, float *ms) {
  if (!h || !ms) return fail(QH_ERR_ARG, "null handle or out");
  if (!h->ev0) return fail(QH_ERR_ARG, "qh_timer_end without qh_timer_begin");
  int rc = enter(h);
  if (rc) return rc;
  HIP_TRY(hipEventRecord(h->ev1, h->stream));
  if ((rc = wait_event(h, h->ev1, "qh_timer_end"))) return rc;
  HIP_TRY(hipEventElapsedTime(ms, h->ev0, h->ev1));
  return QH_OK;
}

int qh_timer_lap(qh_handle h) {
  if (!h) return fail(QH_ERR_ARG, "null handle");
  const int rc = enter(h);
  if (rc) return rc;
  if (h->laps_used == h->laps.size()) {
    hipEvent_t e = nullptr;
    HIP_TRY(hipEventCreate(&e));
    h->laps.push_back(e);
  }
  HIP_TRY(hipEventRecord(h->laps[h->laps_used++], h->stream));
  return QH_OK;
}
int qh_timer_laps(qh_handle h, float *ms, int cap, int *count) {
  if (!h || !count || h->dry) return fail(QH_ERR_ARG, "null/dry");
  HIP_TRY(hipSetDevice(h->device));
  const int n = h->laps_used > 0 ? (int)h->laps_used - 1 : 0;
  if (h->laps_used) {
    const int rc = wait_event(h, h->laps[h->laps_used - 1], "qh_timer_laps");
    if (rc) return rc;
  }
  for (int k = 0; k < n && ms && k < cap; ++k) HIP_TRY(hipEventElapsedTime(&ms[k], h->laps[k], h->laps[k + 1]));
  *count = n;
  h->laps_used = 0;
  return QH_OK;
}

int qh_plan_json(qh_handle h, char *buf, uint64_t cap, uint64_t *needed) {
  if (!h) return fail(QH_ERR_ARG, "null");
  std::string s;
  if (int rc = qh::guard_planning(&g_err, [&] { s = qh::plan_to_json(h->queue, plan_request(h, relayout_wanted(h))); })) return rc;
  if (needed) *needed = s.size() + 1;
  if (buf && cap) {
    const uint64_t n = std::min<uint64_t>(cap - 1, s.size());
    memcpy(buf, s.data(), n);
    buf[n] = 0;
  }
  return QH_OK;
}

int qh_plan_export(qh_handle h, void *buf, uint64_t cap, uint64_t *needed) {
  if (!h) return fail(QH_ERR_ARG, "null");
  if (!qh::sweep_supported(h->nloc, h->bw)) return fail(QH_ERR_ARG, "state too small for sweeps");
  qh::PlanResult pr;
  if (int rc = qh::guard_planning(&g_err, [&] { pr = qh::plan_best(h->queue, plan_request(h, relayout_wanted(h))); })) return rc;
  std::vector<uint64_t> out;
  auto put_bytes = [&](const void *p, size_t n) {
    const size_t w = (n + 7) / 8, at = out.size();
    out.resize(at + w, 0);
    if (n) memcpy(&out[at], p, n);
  };
  out.push_back(0x51485033ull);
  out.push_back(pr.sweeps.size());
  out.push_back(pr.noop_gates);
  put_bytes(pr.final_pos, 64);
  for (auto &sp : pr.sweeps) {
    int64_t hdr[28] = {0};
    int k = 0;
    hdr[k++] = sp.rb;
    for (int i = 0; i < 6; ++i) hdr[k++] = sp.regpos[i];
    for (int i = 0; i < 6; ++i) hdr[k++] = sp.regpos_store[i];
    for (int i = 0; i < 3; ++i) hdr[k++] = sp.lanehi[i];
    hdr[k++] = sp.nwave;
    for (int i = 0; i < 2; ++i) hdr[k++] = sp.wavepos[i];
    hdr[k++] = (int64_t)sp.fixed_ones;
    hdr[k++] = (int64_t)sp.ntiles;
    hdr[k++] = (int64_t)sp.ops.size();
    hdr[k++] = (int64_t)sp.groups.size();
    hdr[k++] = (int64_t)sp.oterms.size();
    hdr[k++] = (int64_t)sp.tables.size();
    hdr[k++] = sp.n_ltab;
    hdr[k++] = sp.lane_low;
    hdr[k++] = sp.relayout ? 1 : 0;
    put_bytes(hdr, sizeof hdr);
    put_bytes(sp.dest_pos, 64);
    {
      // lanes: the index bit on lane bit i at load time, at store time, and the position 0..5 a relayout store sends it to;
      // then the wave bits at store time
      int64_t st[20] = {0};
      for (int i = 0; i < 6; ++i) { st[i] = sp.seat[i]; st[6 + i] = sp.seat_store[i]; st[12 + i] = sp.seat_dest[i]; }
      st[18] = sp.wavepos_store[0];
      st[19] = sp.wavepos_store[1];
      put_bytes(st, sizeof st);
      // what the kernel is handed for a relayout store: register / wave bit destinations and the runs of
      // unit-index bits (count, then 8 x mask, 8 x shift)
      int64_t kd[8 + 1 + 2 * qh::kMaxUnitSegs] = {0};
      for (int i = 0; i < 6; ++i) kd[i] = sp.reg_dest[i];
      kd[6] = sp.wave_dest[0];
      kd[7] = sp.wave_dest[1];
      uint64_t masks[qh::kMaxUnitSegs] = {0};
      int shifts[qh::kMaxUnitSegs] = {0};
      kd[8] = sp.relayout ? qh::unit_segments(sp, h->nloc, masks, shifts) : 0;
      for (int i = 0; i < qh::kMaxUnitSegs; ++i) { kd[9 + i] = (int64_t)masks[i]; kd[9 + qh::kMaxUnitSegs + i] = shifts[i]; }
      put_bytes(kd, sizeof kd);
    }
    put_bytes(sp.ops.data(), sp.ops.size() * sizeof(qh::SweepOp));
    put_bytes(sp.groups.data(), sp.groups.size() * sizeof(qh::DGroup));
    put_bytes(sp.oterms.data(), sp.oterms.size() * sizeof(qh::OTerm));
    put_bytes(sp.tables.data(), sp.tables.size() * sizeof(double));
  }
  const uint64_t bytes = out.size() * 8;
  if (needed) *needed = bytes;
  if (buf && cap) {
    if (cap < bytes) return fail(QH_ERR_ARG, "buffer too small (call with NULL to get the size)");
    memcpy(buf, out.data(), bytes);
  }
  return QH_OK;
}

int qh_plan_handlers(qh_handle h, void *buf, uint64_t cap, uint64_t *needed) {
  if (!h) return fail(QH_ERR_ARG, "null");
  if (!qh::sweep_supported(h->nloc, h->bw)) return fail(QH_ERR_ARG, "state too small for sweeps");
  qh::PlanResult pr;
  if (int rc = qh::guard_planning(&g_err, [&] { pr = qh::plan_best(h->queue, plan_request(h, relayout_wanted(h))); })) return rc;
  std::vector<uint32_t> out{0x51484831u, (uint32_t)pr.sweeps.size()};
  std::vector<qh::SweepOp> ops;
  std::vector<qh::DGroup> groups;
  for (auto &sp : pr.sweeps) {
    // the device copy of the sweep, built by the function a flush builds it with
    ops.assign(sp.ops.size() + 1, qh::SweepOp{});
    groups.assign(sp.groups.size(), qh::DGroup{});
    const uint32_t n_ltab_lds = (uint32_t)(h->bw == 128 ? qh::ltab_lds_count<true>(sp) : qh::ltab_lds_count<false>(sp));
    qh::build_device_copy(sp, h->bw, n_ltab_lds, ops.data(), groups.data());
    for (uint32_t v : {(uint32_t)h->bw, (uint32_t)sp.rb, (uint32_t)sp.nwave, (uint32_t)(sp.relayout ? 1 : 0), (uint32_t)sp.ops.size(),
                       (uint32_t)sp.groups.size()})
      out.push_back(v);
    for (size_t k = 0; k < sp.ops.size(); ++k) { out.push_back(ops[k].kind); out.push_back(ops[k].flags); }
    for (const qh::DGroup &g : groups) out.push_back(g.flags);
  }
  if (out.size() & 1) out.push_back(0);
  const uint64_t bytes = out.size() * 4;
  if (needed) *needed = bytes;
  if (buf && cap) {
    if (cap < bytes) return fail(QH_ERR_ARG, "buffer too small (call with NULL to get the size)");
    memcpy(buf, out.data(), bytes);
  }
  return QH_OK;
}

}  // extern "C"

// ---- multi-GPU exchange (exchange.hip.h) --------------------------------------------------
namespace {

#define NCCL_TRY(expr)                                                                     \
  do {                                                                                     \
    ncclResult_t r_ = (expr);                                                              \
    if (r_ != ncclSuccess)                                                                 \
      return fail(QH_ERR_COMM, "%s: %s (%s:%d)", #expr, qh::rccl().GetErrorString(r_), __FILE__, __LINE__); \
  } while (0)

// what every transport asks of (nranks, rank)
int check_ranks(int nranks, int rank) {
  if (nranks < 1 || (nranks & (nranks - 1)) || rank < 0 || rank >= nranks)
    return fail(QH_ERR_ARG, "nranks %d must be a power of two, rank %d inside it", nranks, rank);
  if (nranks > qh::kMaxXferMoves + 1) return fail(QH_ERR_ARG, "at most %d ranks", qh::kMaxXferMoves + 1);
  return QH_OK;
}

int comm_common_init(qh_state_s *h, int nranks, int rank) {
  if (!h) return fail(QH_ERR_ARG, "null handle");
  if (h->comm) return fail(QH_ERR_ARG, "handle already has a communicator");
  if (int rc = check_ranks(nranks, rank)) return rc;
  if (h->bw != 128 && h->bw != 64) return fail(QH_ERR_BAD_DTYPE, "bit width");
  int rc0 = enter(h);
  if (rc0) return rc0;
  if (nranks > 1 && h->relayout != 0) {
    // The ranks of a sharded state must hold the same layout whenever they exchange.  They do if all of them
    // re-lay out (the planner keeps rank-dependent gates as ghosts: planner.h) or none does; a rank that could
    // not get its second buffer would break that, so with several ranks relayout starts OFF and the caller
    // turns it on after every rank has said it can (qh_set_relayout; qcc_amd/sharded.py does).
    rc0 = set_relayout(h, false);
    if (rc0) return rc0;
  }
  auto *c = new qh::Comm;
  c->nranks = nranks;
  c->rank = rank;
  hipError_t e = hipStreamCreateWithFlags(&c->xstream, hipStreamNonBlocking);
  if (e == hipSuccess) e = hipStreamCreateWithFlags(&c->cstream, hipStreamNonBlocking);
  if (e == hipSuccess) e = hipStreamCreateWithFlags(&c->pstream, hipStreamNonBlocking);
  if (e == hipSuccess) e = hipEventCreate(&c->t0);
  if (e == hipSuccess) e = hipEventCreate(&c->t1);
  if (e != hipSuccess) {
    delete c;
    return fail(QH_ERR_HIP, "exchange streams/events: %s", hipGetErrorString(e));
  }
  h->comm = c;
  return QH_OK;
}

// closes the timing bracket of the previous exchange (waits for it)
void close_timing(qh::Comm *c) {
  if (!c->timing_open) return;
  float ms = 0;
  if (hipEventSynchronize(c->t1) == hipSuccess && hipEventElapsedTime(&ms, c->t0, c->t1) == hipSuccess)
    c->stats.span_ms += ms;
  c->timing_open = false;
}

template <typename A>
void launch_xfer(bool unpack, void *psi, void *stage, uint64_t n, uint64_t start, const qh::XferGeom &g, hipStream_t st) {
  const uint64_t total = n * (uint64_t)g.np;
  const unsigned grid = grid_for(total, 1ull << 20);
  if (unpack) hipLaunchKernelGGL(qh::k_xunpack<A>, dim3(grid), dim3(256), 0, st, (A *)psi, (const A *)stage, n, start, g);
  else hipLaunchKernelGGL(qh::k_xpack<A>, dim3(grid), dim3(256), 0, st, (const A *)psi, (A *)stage, n, start, g);
}

// Every rank must cut an exchange the same way (rounds, chunk sizes, slabs, where each index bit lives): the
// geometry is a function of rank-invariant inputs only -- the planner keeps rank-dependent gates as ghosts, so
// plans, tiles and layouts agree by construction -- and this is the check of that claim: a 64-bit signature of
// the geometry is compared with every peer's (always on the host-staged transport; on RCCL with
// QH_EXCHANGE_VERIFY=1, a host wait).  A mismatch is an error here instead of a hang or misplaced data there.
int verify_geometry(qh_state_s *h, uint64_t sig) {
  qh::Comm *c = h->comm;
  if (c->nranks <= 1) return QH_OK;
  if (c->custom) {
    const int np = c->nranks - 1;
    std::vector<uint64_t> mine(np, sig), theirs(np, 0);
    std::vector<int> peers;
    std::vector<void *> sp, rp;
    for (int j = 0, k = 0; j < c->nranks; ++j) {
      if (j == c->rank) continue;
      peers.push_back(j);
      sp.push_back(&mine[k]);
      rp.push_back(&theirs[k]);
      ++k;
    }
    if (c->custom(c->custom_user, np, peers.data(), sp.data(), rp.data(), sizeof(uint64_t)) != 0)
      return fail(QH_ERR_COMM, "host-staged transport: the round callback failed (geometry check)");
    for (int k = 0; k < np; ++k)
      if (theirs[k] != sig)
        return fail(QH_ERR_COMM, "exchange geometry differs between rank %d (%016llx) and rank %d (%016llx): the ranks "
                    "planned different sweeps or layouts", c->rank, (unsigned long long)sig, peers[k], (unsigned long long)theirs[k]);
    c->stats.geometry_checks++;
    return QH_OK;
  }
  if (!c->nccl) return fail(QH_ERR_COMM, "no RCCL communicator on this handle (never set up, or aborted by the watchdog)");
  // RCCL: every geometry this communicator has not compared yet (QH_EXCHANGE_VERIFY=1: every exchange, =0: never).
  // The all-reduce runs on the EXCHANGE stream -- it does not wait for the sweeps queued on the compute stream --
  // and the host waits for it: once per distinct geometry (a loop over one circuit cycles through a few layouts).
  static const int mode = env_int("QH_EXCHANGE_VERIFY", -1);
  if (mode == 0) return QH_OK;
  if (mode < 0 && std::find(c->verified.begin(), c->verified.end(), sig) != c->verified.end()) return QH_OK;
  HIP_TRY(c->d_sig.reserve(4 * sizeof(double)));
  HIP_TRY(c->h_sig.reserve(8 * sizeof(double)));
  double *v = c->h_sig.as<double>(), *w = v + 4, *d_sig = c->d_sig.as<double>();
  v[0] = (double)(sig >> 32); v[1] = (double)(sig & 0xffffffffu); v[2] = -v[0]; v[3] = -v[1];
  HIP_TRY(hipMemcpyAsync(d_sig, v, 4 * sizeof(double), hipMemcpyHostToDevice, c->xstream));
  NCCL_TRY(qh::rccl().AllReduce(d_sig, d_sig, 4, ncclDouble, ncclMax, c->nccl, c->xstream));
  HIP_TRY(hipMemcpyAsync(w, d_sig, 4 * sizeof(double), hipMemcpyDeviceToHost, c->xstream));
  const int rc = wait_stream(h, c->xstream, "exchange geometry check (all-reduce of the signature)");
  if (rc) return rc;
  if (w[0] != -w[2] || w[1] != -w[3])
    return fail(QH_ERR_COMM, "exchange geometry differs between ranks (signature of rank %d: %016llx; largest / smallest halves seen: "
                "%08x%08x / %08x%08x): the ranks planned different sweeps or layouts, or run with different planner switches "
                "(QH_* environment) or builds", c->rank, (unsigned long long)sig, (unsigned)w[0], (unsigned)w[1], (unsigned)-w[2], (unsigned)-w[3]);
  if (c->verified.size() >= 256) c->verified.erase(c->verified.begin());
  c->verified.push_back(sig);
  c->stats.geometry_checks++;
  return QH_OK;
}

// What must be equal on every rank besides the geometry itself: the planner's switches and the build.
uint64_t env_build_hash(const qh::ExchangeSwitches &xsw) {
  std::string s = qh::PlanSwitches::from_env().key();
  s += xsw.key() + std::to_string(env_int("QH_RELAYOUT", 1) != 0) + ";";
  // the build: the library's version and the layouts the planner and the kernels share -- NOT the time of compilation (two
  // nodes that build the same sources in-tree must be able to exchange)
  s += "v" + std::to_string(qh_version()) + ":" + std::to_string(sizeof(qh::SweepArgs)) + ":" + std::to_string(sizeof(qh::SweepOp)) +
       ":" + std::to_string(sizeof(qh::SweepPlan)) + ":" + std::to_string(sizeof(qh_xgeom));
  uint64_t hsh = 0xcbf29ce484222325ull;
  for (unsigned char ch : s) { hsh ^= ch; hsh *= 0x100000001b3ull; }
  return hsh;
}

// The gather (or scatter) kernel of packed round ci of slab k: every move's amplitudes to (from) `stage`, peer after peer.
void launch_packed_round(qh_state_s *h, const qh::ExchangePlan &pl, const std::vector<qh::BlockMove> &moves, bool unpack, void *stage,
                         int k, uint64_t ci, hipStream_t st) {
  qh::XferGeom g{};
  g.ins.n = pl.nins;
  for (int i = 0; i < pl.nins; ++i) g.ins.pos[i] = pl.ins_pos[i];
  g.np = pl.np;
  for (int m = 0; m < pl.np; ++m) g.off[m] = pl.packed_offset(k, unpack ? moves[m].land : moves[m].blk);
  with_real(h, [&](auto x) {
    launch_xfer<typename qh::AmpT<decltype(x)>::type>(unpack, h->d_psi, stage, pl.chunk_amps(), pl.round_start(ci), g, st);
  });
}

// The rounds of the host-staged transport: synchronous, all on the exchange stream.  slab_done[k]: slab k is written.
int run_rounds_host_staged(qh_state_s *h, const qh::ExchangePlan &pl, const std::vector<qh::BlockMove> &moves,
                           const std::vector<hipEvent_t> &slab_done) {
  qh::Comm *c = h->comm;
  char *const psi = (char *)h->d_psi, *const staging = c->staging.as<char>();
  const size_t np = moves.size(), need = pl.half_bytes;
  const uint64_t ab = pl.amp_bytes, nb = pl.chunk_bytes();
  HIP_TRY(c->h_send.reserve(need));
  HIP_TRY(c->h_recv.reserve(need));
  char *const h_send = c->h_send.as<char>(), *const h_recv = c->h_recv.as<char>();
  std::vector<int> peers(np);
  std::vector<void *> sp(np), rp(np);
  for (size_t m = 0; m < np; ++m) {
    peers[m] = moves[m].peer;
    sp[m] = h_send + m * nb;
    rp[m] = h_recv + m * nb;
  }
  for (int k = 0; k < pl.slabs(); ++k) {
    HIP_TRY(hipEventSynchronize(slab_done[k]));
    if (k == 0) { HIP_TRY(hipEventRecord(c->t0, c->xstream)); }
    for (uint64_t ci = 0; ci < pl.rounds_per_slab; ++ci) {
      const uint64_t off = pl.round_offset(k, ci);
      if (pl.packed) {
        launch_packed_round(h, pl, moves, false, staging, k, ci, c->xstream);
        HIP_TRY(hipMemcpyAsync(h_send, staging, need, hipMemcpyDeviceToHost, c->xstream));
      } else {
        for (size_t m = 0; m < np; ++m)
          HIP_TRY(hipMemcpyAsync(sp[m], psi + (off | pl.block_offset(moves[m].blk)) * ab, nb, hipMemcpyDeviceToHost, c->xstream));
      }
      HIP_TRY(hipStreamSynchronize(c->xstream));
      if (c->custom(c->custom_user, (int)np, peers.data(), sp.data(), rp.data(), nb) != 0)
        return fail(QH_ERR_COMM, "host-staged transport: the round callback failed");
      if (pl.packed) {
        HIP_TRY(hipMemcpyAsync(staging, h_recv, need, hipMemcpyHostToDevice, c->xstream));
        launch_packed_round(h, pl, moves, true, staging, k, ci, c->xstream);
      } else {
        for (size_t m = 0; m < np; ++m)
          HIP_TRY(hipMemcpyAsync(psi + (off | pl.block_offset(moves[m].land)) * ab, rp[m], nb, hipMemcpyHostToDevice, c->xstream));
      }
      HIP_TRY(hipStreamSynchronize(c->xstream));
      c->stats.rounds++;
    }
    hipEvent_t ev = c->event();
    if (!ev) return fail(QH_ERR_HIP, "hipEventCreate failed");
    HIP_TRY(hipEventRecord(ev, c->xstream));
    c->arrivals.push_back(qh::Arrival{pl.slab_mask, pl.slab_vals[k], ev});
  }
  HIP_TRY(hipEventRecord(c->t1, c->xstream));
  return QH_OK;
}

// The rounds of the RCCL transport: grouped send/recv per round on xstream, landing (copies / scatter kernel) on cstream,
// packing on pstream; the two halves of the staging area alternate from round to round.
int run_rounds_rccl(qh_state_s *h, const qh::ExchangePlan &pl, const std::vector<qh::BlockMove> &moves,
                    const std::vector<hipEvent_t> &slab_done) {
  qh::Comm *c = h->comm;
  if (!c->nccl) return fail(QH_ERR_COMM, "no communicator (qh_comm_init)");
  char *const psi = (char *)h->d_psi, *const staging = c->staging.as<char>();
  const size_t np = moves.size(), half = pl.half_bytes;
  const uint64_t ab = pl.amp_bytes, nb = pl.chunk_bytes();
  const bool packed = pl.packed;
  const ncclDataType_t dt = h->bw == 128 ? ncclDouble : ncclFloat;
  const size_t cnt = (size_t)pl.chunk_amps() * 2;
  auto &R = qh::rccl();
  hipEvent_t copied[2] = {nullptr, nullptr};   // receive half free again
  hipEvent_t sent[2] = {nullptr, nullptr};     // send half free again (packed)
  uint64_t round = 0;
  for (int k = 0; k < pl.slabs(); ++k) {
    HIP_TRY(hipStreamWaitEvent(packed ? c->pstream : c->xstream, slab_done[k], 0));
    if (k == 0) { HIP_TRY(hipEventRecord(c->t0, packed ? c->pstream : c->xstream)); }
    hipEvent_t last_copy = nullptr;
    for (uint64_t ci = 0; ci < pl.rounds_per_slab; ++ci, ++round) {
      const int par = (int)(round & 1);
      const uint64_t off = pl.round_offset(k, ci);
      char *stage = staging + par * half;
      char *sstage = staging + (2 + par) * half;
      if (packed) {
        if (sent[par]) HIP_TRY(hipStreamWaitEvent(c->pstream, sent[par], 0));
        launch_packed_round(h, pl, moves, false, sstage, k, ci, c->pstream);
        hipEvent_t pk = c->event();
        if (!pk) return fail(QH_ERR_HIP, "hipEventCreate failed");
        HIP_TRY(hipEventRecord(pk, c->pstream));
        HIP_TRY(hipStreamWaitEvent(c->xstream, pk, 0));
      }
      if (copied[par]) HIP_TRY(hipStreamWaitEvent(c->xstream, copied[par], 0));   // this half is free again
      NCCL_TRY(R.GroupStart());
      for (size_t m = 0; m < np; ++m) {
        const void *src = packed ? (const void *)(sstage + m * nb) : (const void *)(psi + (off | pl.block_offset(moves[m].blk)) * ab);
        NCCL_TRY(R.Send(src, cnt, dt, moves[m].peer, c->nccl, c->xstream));
        NCCL_TRY(R.Recv(stage + m * nb, cnt, dt, moves[m].peer, c->nccl, c->xstream));
      }
      NCCL_TRY(R.GroupEnd());
      hipEvent_t landed = c->event();
      if (!landed) return fail(QH_ERR_HIP, "hipEventCreate failed");
      HIP_TRY(hipEventRecord(landed, c->xstream));
      sent[par] = landed;
      HIP_TRY(hipStreamWaitEvent(c->cstream, landed, 0));
      if (packed) {
        launch_packed_round(h, pl, moves, true, stage, k, ci, c->cstream);
      } else {
        for (size_t m = 0; m < np; ++m)
          HIP_TRY(hipMemcpyAsync(psi + (off | pl.block_offset(moves[m].land)) * ab, stage + m * nb, nb, hipMemcpyDeviceToDevice,
                                 c->cstream));
      }
      hipEvent_t cp = c->event();
      if (!cp) return fail(QH_ERR_HIP, "hipEventCreate failed");
      HIP_TRY(hipEventRecord(cp, c->cstream));
      copied[par] = cp;
      last_copy = cp;
      c->stats.rounds++;
    }
    c->arrivals.push_back(qh::Arrival{pl.slab_mask, pl.slab_vals[k], last_copy});
  }
  HIP_TRY(hipEventRecord(c->t1, c->cstream));
  return QH_OK;
}

// The exchange proper.  `moves`: block value blk of the g LOGICAL local bits [base, base+g) goes to `peer`,
// whose data lands in block value `land`.  Logical = the bit numbers the caller uses (canonical positions);
// where those bits live now is the handle's business (relayout sweeps move them).
int do_exchange(qh_state_s *h, const std::vector<qh::BlockMove> &moves, int base, int gbits, uint64_t chunk_amps) {
  qh::Comm *c = h->comm;
  if (base < 0 || base + gbits > h->nglob || gbits > qh::kMaxExchangeBits)
    return fail(QH_ERR_BAD_QUBIT, "exchange bits [%d,%d)", base, base + gbits);
  for (int k = 0; k < gbits; ++k)
    if (h->perm[base + k] >= h->nloc) return fail(QH_ERR_BAD_QUBIT, "exchange bit %d is not a local bit of this shard", base + k);
  if (moves.size() > (size_t)qh::kMaxXferMoves) return fail(QH_ERR_ARG, "too many peers");
  if (h->poisoned) return fail(QH_ERR_HIP, "the state of this handle is undefined (an earlier sweep or exchange failed); re-initialise it");
  const bool dry = h->dry;
  if (!dry) {
    HIP_TRY(hipSetDevice(h->device));
    close_timing(c);
  }
  const qh::ExchangeSwitches xsw = qh::ExchangeSwitches::from_env();
  // 1. the queued gates, the last sweep cut into slabs
  qh::SlabIO io;
  io.split_last = true;
  for (int k = 0; k < gbits; ++k) io.avoid |= 1ull << h->perm[base + k];   // (layout before the flush; run_fused follows the moves)
  io.want_bits = xsw.slab_bits;
  c->pool_used = 0;   // (arrivals of the previous exchange are waited for by this flush)
  const uint64_t sweeps0 = h->stats.sweeps;
  int rc = flush_impl(h, &io);
  if (rc) return rc;
  // 2. how the exchange is cut, in the layout the flush left (exchange_plan.h)
  int pos[qh::kMaxExchangeBits];
  for (int k = 0; k < gbits; ++k) pos[k] = h->perm[base + k];
  const bool flush_cut = !io.slab_done.empty();
  const qh::ExchangePlan pl = qh::plan_exchange(h->nloc, pos, gbits, chunk_amps, (int)moves.size(), h->amp_bytes(), xsw, io.slab_mask,
                                                flush_cut ? &io.slab_vals : nullptr);
  if (!dry && (!flush_cut || std::find(io.slab_done.begin(), io.slab_done.end(), nullptr) != io.slab_done.end())) {
    hipEvent_t all_done = c->event();
    if (!all_done) return fail(QH_ERR_HIP, "hipEventCreate failed");
    HIP_TRY(hipEventRecord(all_done, h->stream));
    io.slab_done.assign(pl.slabs(), all_done);
  }
  if (moves.empty()) return QH_OK;
  const uint64_t sig = qh::exchange_signature(pl, h->perm, h->nglob, base, h->bw, env_build_hash(xsw));
  c->last_geom = qh::exchange_record(pl, sig, (uint32_t)(h->stats.sweeps - sweeps0), io.split_done);
  if (dry) {
    // 3. planner-only handle: the decisions are on record, the next flush sees the arrivals it would see
    for (uint64_t sv : pl.slab_vals) c->arrivals.push_back(qh::Arrival{pl.slab_mask, sv, nullptr});
    c->stats.rounds += (uint64_t)pl.slabs() * pl.rounds_per_slab;
  } else {
    // 3. the rounds
    rc = verify_geometry(h, sig);
    if (rc) return rc;
    if (pl.packed && pl.nins > qh::kMaxIns) return fail(QH_ERR_ARG, "exchange: more than %d block + slab bits", qh::kMaxIns);
    if (c->staging.cap < pl.staging_bytes && (pl.packed || !c->custom)) {   // (direct host-staged rounds copy shard <-> pinned memory)
      if (c->staging.ptr) {      // (rounds of the previous exchange may still use it)
        HIP_TRY(hipStreamSynchronize(c->cstream));
        HIP_TRY(hipStreamSynchronize(c->pstream));
        HIP_TRY(hipStreamSynchronize(c->xstream));
      }
      HIP_TRY(c->staging.reserve(pl.staging_bytes));
    }
    rc = c->custom ? run_rounds_host_staged(h, pl, moves, io.slab_done) : run_rounds_rccl(h, pl, moves, io.slab_done);
    if (rc) return rc;
    rc = check_launch(h);
    if (rc) return rc;
    c->timing_open = true;
  }
  c->stats.exchanges++;
  c->stats.slabs += pl.slabs();
  c->stats.rounds_packed += pl.packed ? (uint64_t)pl.slabs() * pl.rounds_per_slab : 0;
  c->stats.bytes_sent += (uint64_t)pl.np * (1ull << (h->nloc - gbits)) * pl.amp_bytes;
  return QH_OK;
}

int log2_exact(int v) {
  int g = 0;
  while ((1 << g) < v) ++g;
  return g;
}

}  // namespace

extern "C" {

int qh_comm_unique_id(void *id) {
  if (!id) return fail(QH_ERR_ARG, "null");
  std::string err;
  if (!qh::rccl().load(&err)) return fail(QH_ERR_COMM, "%s", err.c_str());
  static_assert(sizeof(ncclUniqueId) == QH_COMM_ID_BYTES, "id size");
  NCCL_TRY(qh::rccl().GetUniqueId((ncclUniqueId *)id));
  return QH_OK;
}

int qh_comm_init(qh_handle h, int nranks, int rank, const void *id) {
  if (!id) return fail(QH_ERR_ARG, "null id");
  std::string err;
  if (!qh::rccl().load(&err)) return fail(QH_ERR_COMM, "%s", err.c_str());
  int rc = comm_common_init(h, nranks, rank);
  if (rc) return rc;
  ncclUniqueId uid;
  memcpy(&uid, id, sizeof uid);
  ncclResult_t r = qh::rccl().CommInitRank(&h->comm->nccl, nranks, uid, rank);
  if (r != ncclSuccess) {
    (void)qh_comm_destroy(h);
    return fail(QH_ERR_COMM, "ncclCommInitRank(%d of %d): %s", rank, nranks, qh::rccl().GetErrorString(r));
  }
  int cnt = 0, ur = -1;      // what the communicator itself says (reported in qh_xstats: bench.py prints it)
  if (qh::rccl().CommCount(h->comm->nccl, &cnt) == ncclSuccess) h->comm->stats.comm_ranks = (uint32_t)cnt;
  if (qh::rccl().CommUserRank(h->comm->nccl, &ur) == ncclSuccess) h->comm->stats.comm_rank = (uint32_t)ur;
  if (cnt != nranks || ur != rank) {
    (void)qh_comm_destroy(h);
    return fail(QH_ERR_COMM, "the RCCL communicator reports rank %d of %d, asked for %d of %d", ur, cnt, rank, nranks);
  }
  return QH_OK;
}

int qh_comm_init_custom(qh_handle h, int nranks, int rank, qh_round_fn fn, void *user) {
  if (!fn) return fail(QH_ERR_ARG, "null callback");
  int rc = comm_common_init(h, nranks, rank);
  if (rc) return rc;
  h->comm->custom = fn;
  h->comm->custom_user = user;
  h->comm->stats.comm_ranks = (uint32_t)nranks;
  h->comm->stats.comm_rank = (uint32_t)rank;
  return QH_OK;
}

int qh_comm_init_dry(qh_handle h, int nranks, int rank) {
  if (!h || !h->dry) return fail(QH_ERR_ARG, "qh_comm_init_dry is for planner-only handles (qh_create_dry)");
  if (h->comm) return fail(QH_ERR_ARG, "handle already has a communicator");
  if (int rc = check_ranks(nranks, rank)) return rc;
  auto *c = new qh::Comm;
  c->nranks = nranks;
  c->rank = rank;
  c->dry = true;
  h->comm = c;
  return QH_OK;
}

int qh_exchange_geometry(qh_handle h, qh_xgeom *out) {
  if (!h || !out) return fail(QH_ERR_ARG, "null");
  if (!h->comm) return fail(QH_ERR_ARG, "no communicator on this handle");
  *out = h->comm->last_geom;
  return QH_OK;
}

int qh_comm_destroy(qh_handle h) {
  if (!h || !h->comm) return QH_OK;
  qh::Comm *c = h->comm;
  if (c->dry) {
    delete c;
    h->comm = nullptr;
    return QH_OK;
  }
  (void)hipSetDevice(h->device);
  if (c->pstream) (void)hipStreamSynchronize(c->pstream);
  if (c->xstream) (void)hipStreamSynchronize(c->xstream);
  if (c->cstream) (void)hipStreamSynchronize(c->cstream);
  if (c->nccl) (void)qh::rccl().CommDestroy(c->nccl);
  for (hipEvent_t e : c->pool) (void)hipEventDestroy(e);
  if (c->t0) (void)hipEventDestroy(c->t0);
  if (c->t1) (void)hipEventDestroy(c->t1);
  if (c->xstream) (void)hipStreamDestroy(c->xstream);
  if (c->cstream) (void)hipStreamDestroy(c->cstream);
  if (c->pstream) (void)hipStreamDestroy(c->pstream);
  delete c;      // (staging and the pinned buffers go with it: the three streams were drained above)
  h->comm = nullptr;
  return QH_OK;
}

int qh_exchange_alltoall(qh_handle h, int base_bit, uint64_t chunk_amps) {
  if (!h || !h->comm) return fail(QH_ERR_ARG, "no communicator on this handle (qh_comm_init)");
  const int g = log2_exact(h->comm->nranks);
  std::vector<qh::BlockMove> mv;
  for (int j = 0; j < h->comm->nranks; ++j)
    if (j != h->comm->rank) mv.push_back(qh::BlockMove{j, j, j});
  return do_exchange(h, mv, base_bit, g, chunk_amps);
}

int qh_exchange_pair(qh_handle h, int shard_bit, int local_bit, uint64_t chunk_amps) {
  if (!h || !h->comm) return fail(QH_ERR_ARG, "no communicator on this handle (qh_comm_init)");
  const int g = log2_exact(h->comm->nranks);
  if (shard_bit < 0 || shard_bit >= g) return fail(QH_ERR_BAD_QUBIT, "shard bit %d of %d", shard_bit, g);
  const int mybit = (h->comm->rank >> shard_bit) & 1;
  std::vector<qh::BlockMove> mv{qh::BlockMove{h->comm->rank ^ (1 << shard_bit), 1 - mybit, 1 - mybit}};
  return do_exchange(h, mv, local_bit, 1, chunk_amps);
}

int qh_exchange_loopback(qh_handle h, int local_bit, uint64_t chunk_amps) {
  if (!h || !h->comm) return fail(QH_ERR_ARG, "no communicator on this handle (qh_comm_init)");
  std::vector<qh::BlockMove> mv{qh::BlockMove{h->comm->rank, 0, 1}, qh::BlockMove{h->comm->rank, 1, 0}};
  return do_exchange(h, mv, local_bit, 1, chunk_amps);
}

int qh_exchange_wait(qh_handle h) {
  if (!h || !h->comm || h->comm->dry) return QH_OK;
  HIP_TRY(hipSetDevice(h->device));
  for (const qh::Arrival &a : h->comm->arrivals) {
    if (!a.ev) continue;
    const int rc = wait_event(h, a.ev, "qh_exchange_wait");
    if (rc) return rc;
  }
  close_timing(h->comm);
  return QH_OK;
}

int qh_exchange_stats(qh_handle h, qh_xstats *out) {
  if (!h || !out) return fail(QH_ERR_ARG, "null");
  if (!h->comm) {
    memset(out, 0, sizeof *out);
    return QH_OK;
  }
  if (!h->comm->dry) {
    HIP_TRY(hipSetDevice(h->device));
    close_timing(h->comm);
  }
  *out = h->comm->stats;
  return QH_OK;
}

int qh_comm_allreduce_sum(qh_handle h, double *inout, int count) {
  if (!h || !h->comm || !inout) return fail(QH_ERR_ARG, "null / no communicator");
  if (!h->comm->nccl) return fail(QH_ERR_COMM, "qh_comm_allreduce_sum needs the RCCL transport");
  if (count < 1 || count > kRedBlocks) return fail(QH_ERR_ARG, "count %d", count);
  const int rc = enter(h);
  if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(h->d_red(), inout, count * sizeof(double), hipMemcpyHostToDevice, h->stream));
  NCCL_TRY(qh::rccl().AllReduce(h->d_red(), h->d_red(), (size_t)count, ncclDouble, ncclSum, h->comm->nccl, h->stream));
  return read_back(h, inout, h->d_red(), count * sizeof(double));
}

}  // extern "C"

extern "C" {

// ---- literal drop-in on host buffers ------------------------------------------
// The device-side scratch of qh_host_apply1/applyc: per calling THREAD (the boundary is "one host
// thread per handle"), the two most recently used (nbits, width) shapes are kept so that an
// algorithm alternating between two register sizes does not pay a hipMalloc/hipFree pair per gate.
// qh_host_release() frees the calling thread's scratch; threads that exit without calling it leak
// nothing but address space until process exit (the handles are owned by the thread_local object).
namespace {
struct HostScratch {
  qh_handle slot[2] = {nullptr, nullptr};
  ~HostScratch() {
    for (qh_handle &h : slot) {
      if (h) qh_destroy(h);
      h = nullptr;
    }
  }
};
thread_local HostScratch g_host;
}  // namespace

static int host_handle(int nbits, int bw, qh_handle *out) {
  for (int k = 0; k < 2; ++k)
    if (g_host.slot[k] && g_host.slot[k]->nloc == nbits && g_host.slot[k]->bw == bw) {
      if (k == 1) std::swap(g_host.slot[0], g_host.slot[1]);   // most recent first
      *out = g_host.slot[0];
      return QH_OK;
    }
  if (g_host.slot[1]) qh_destroy(g_host.slot[1]);
  g_host.slot[1] = g_host.slot[0];
  g_host.slot[0] = nullptr;
  int rc = qh_create(nbits, bw, 0, &g_host.slot[0]);
  if (rc) return rc;
  g_host.slot[0]->relayout = 0;   // one gate per call: nothing to gain from a second buffer
  *out = g_host.slot[0];
  return QH_OK;
}

int qh_host_release(void) {
  for (qh_handle &h : g_host.slot) {
    if (h) qh_destroy(h);
    h = nullptr;
  }
  return QH_OK;
}

int qh_host_apply1(void *psi, const double gate[8], int nbits, int tgt, int bit_width) {
  if (!psi || !gate) return fail(QH_ERR_ARG, "null pointer");
  int rc = check_args(nbits, bit_width);
  if (rc) return rc;
  if (tgt < 0 || tgt >= nbits) return fail(QH_ERR_BAD_QUBIT, "apply1: qubit %d out of range for %d qubits", tgt, nbits);
  qh_handle h;
  rc = host_handle(nbits, bit_width, &h);
  if (rc) return rc;
  if ((rc = qh_upload(h, psi, 0, 1ull << nbits))) return rc;
  if ((rc = qh_apply1(h, tgt, gate))) return rc;
  return qh_download(h, psi, 0, 1ull << nbits);
}

int qh_host_applyc(void *psi, const double gate[8], int nbits, int ctl, int tgt, int bit_width) {
  if (!psi || !gate) return fail(QH_ERR_ARG, "null pointer");
  int rc = check_args(nbits, bit_width);
  if (rc) return rc;
  if (tgt < 0 || tgt >= nbits) return fail(QH_ERR_BAD_QUBIT, "applyc: qubit %d out of range for %d qubits", tgt, nbits);
  const int c = ref_ctl_bit(nbits, ctl, nbits - tgt - 1);
  if (c == -2) return fail(QH_ERR_BAD_QUBIT, "applyc: control qubit %d out of range for %d qubits", ctl, nbits);
  if (c == -1) return QH_OK;  // predicate never true: the reference leaves psi untouched
  qh_handle h;
  rc = host_handle(nbits, bit_width, &h);
  if (rc) return rc;
  if ((rc = qh_upload(h, psi, 0, 1ull << nbits))) return rc;
  if ((rc = qh_applyc(h, ctl, tgt, gate))) return rc;
  return qh_download(h, psi, 0, 1ull << nbits);
}

}  // extern "C"
