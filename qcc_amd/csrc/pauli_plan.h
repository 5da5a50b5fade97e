// pauli_plan.h -- host side of qh_apply_pauli_sum (kernels_pauli.hip.h): terms -> batches, and the index arithmetic of
// the batch kernel.
//
// Plain C++, no HIP: the engine calls it before every launch, qh_pauli_sum_plan hands the batches to tools and tests, and
// tools/pauli_plan_check.cc runs it stand-alone (with sanitizers) over random masks.  pauli_item and pauli_partner_item are the
// very functions k_pauli_batch addresses with, and the engine fills the kernel's sign tables from pauli_split_z.
//
// Terms arrive with PHYSICAL local masks (px, pz), the sign the shard index gives (neg) and nY mod 4.  They are stably
// sorted by px and cut every kPauliT terms; a batch is one kernel and may hold several x masks (its groups: runs of equal
// px, each one partner read).
//
// The batch kernel walks 16-byte ITEMS (Item16: one complex128 amplitude, or two consecutive complex64 ones; amp_bits =
// 0 or 1 index bits inside an item).  Item number = chunk << kPauliChunkBits | u << 8 | thread: 256 threads, thread t
// takes items t + 256 u, u < kPauliPer, of a chunk.  An amplitude index is item << amp_bits | half.  The sign
// (-1)^popcount(i & pz) of a term at amplitude i is the product of four signs, one per part of i:
//   half    pz bit 0 at complex64: differs between the two amplitudes of an item;
//   thread  constant per thread and term: folded into the thread's copy of the coefficient once per kernel;
//   reg     the u part, wave-uniform: a table of kPauliPer bits per term;
//   chunk   wave-uniform, once per chunk: parity of chunk & zc.
// The partner of a group is the item at item ^ (px >> amp_bits); at complex64 bit 0 of px swaps the halves.
#pragma once
#include <stdint.h>

#include <algorithm>

#include "../../include/qcc_hip.h"

namespace qh {

constexpr int kPauliT = QH_PAULI_SUM_BATCH;      // terms per batch
constexpr int kPauliSmallT = 4;                  // ... of the smaller instantiation
constexpr int kPauliPerBits = 3;
constexpr int kPauliPer = 1 << kPauliPerBits;    // items per thread and chunk
constexpr int kPauliChunkBits = 8 + kPauliPerBits;      // log2(items per chunk)
constexpr uint64_t kPauliBlocks = 4096;          // blocks at most (one slab row each), each a contiguous run of chunks

// the main shape needs whole chunks; smaller states take the one-amplitude-per-thread kernel
constexpr bool pauli_main_shape(int nloc, int amp_bits) { return nloc - amp_bits >= kPauliChunkBits; }
struct PauliGrid { uint64_t nchunks, nblk; uint32_t cpb; };
constexpr PauliGrid pauli_grid(int nloc, int amp_bits) {
  const uint64_t nchunks = 1ull << (nloc - amp_bits - kPauliChunkBits), nblk = nchunks < kPauliBlocks ? nchunks : kPauliBlocks;
  return {nchunks, nblk, (uint32_t)(nchunks / nblk)};
}

constexpr uint64_t pauli_item(uint64_t chunk, uint32_t u, uint32_t thread) { return (chunk << kPauliChunkBits) | ((uint64_t)u << 8) | thread; }
// the partner read of a group: which item, and whether the two complex64 halves trade places
constexpr uint64_t pauli_partner_item(uint64_t item, uint64_t px, int amp_bits) { return item ^ (px >> amp_bits); }
constexpr uint32_t pauli_partner_half(uint32_t half, uint64_t px, int amp_bits) { return amp_bits ? half ^ (uint32_t)(px & 1ull) : half; }

struct PauliZSplit {
  uint32_t half;       // 1: z on the sub-item bit (complex64)
  uint32_t thread;     // z over the thread index (item bits 0-7)
  uint32_t reg;        // bit u: parity of z over the register-index part u
  uint64_t chunk;      // z over the chunk number
};
constexpr uint32_t parity64(uint64_t v) {
  v ^= v >> 32; v ^= v >> 16; v ^= v >> 8; v ^= v >> 4; v ^= v >> 2; v ^= v >> 1;
  return (uint32_t)(v & 1ull);
}
constexpr PauliZSplit pauli_split_z(uint64_t pz, int amp_bits) {
  const uint64_t zi = pz >> amp_bits;
  const uint32_t zu = (uint32_t)(zi >> 8) & (uint32_t)(kPauliPer - 1);
  uint32_t reg = 0;
  for (uint32_t u = 0; u < (uint32_t)kPauliPer; ++u) reg |= parity64(u & zu) << u;
  return {amp_bits ? (uint32_t)(pz & 1ull) : 0u, (uint32_t)(zi & 255ull), reg, zi >> kPauliChunkBits};
}
// the four signs as 0 / 1 (1: negative); their XOR is the parity of i & pz
constexpr uint32_t pauli_sign_half(const PauliZSplit &z, uint32_t half) { return z.half & half; }
constexpr uint32_t pauli_sign_thread(const PauliZSplit &z, uint32_t thread) { return parity64(thread & z.thread); }
constexpr uint32_t pauli_sign_reg(const PauliZSplit &z, uint32_t u) { return (z.reg >> u) & 1u; }
constexpr uint32_t pauli_sign_chunk(const PauliZSplit &z, uint64_t chunk) { return parity64(chunk & z.chunk); }

// c' = c * (-i)^ny * (neg ? -1 : 1): swaps and negations only
inline void pauli_coef(double re, double im, uint32_t ny, uint32_t neg, double out[2]) {
  for (uint32_t k = 0; k < (ny & 3u); ++k) {      // times -i: (re, im) -> (im, -re)
    const double t = re;
    re = im;
    im = -t;
  }
  out[0] = neg ? -re : re;
  out[1] = neg ? -im : im;
}
// c' as a power of i: k with c' = i^k, or -1
inline int pauli_unit(const double c[2]) {
  if (c[0] == 1.0 && c[1] == 0.0) return 0;
  if (c[0] == 0.0 && c[1] == 1.0) return 1;
  if (c[0] == -1.0 && c[1] == 0.0) return 2;
  if (c[0] == 0.0 && c[1] == -1.0) return 3;
  return -1;
}

inline void pauli_sort(qh_pauli_term *terms, uint64_t nterms) {
  std::stable_sort(terms, terms + nterms, [](const qh_pauli_term &l, const qh_pauli_term &r) { return l.px < r.px; });
}
// sorted terms -> batches; writes at most cap of them and returns their number
inline uint64_t pauli_cut(const qh_pauli_term *terms, uint64_t nterms, qh_pauli_batch *out, uint64_t cap) {
  uint64_t nb = 0;
  for (uint64_t first = 0; first < nterms; first += (uint64_t)kPauliT, ++nb) {
    const uint64_t count = std::min<uint64_t>((uint64_t)kPauliT, nterms - first);
    uint64_t groups = 1;
    for (uint64_t k = 1; k < count; ++k) groups += terms[first + k].px != terms[first + k - 1].px;
    if (nb < cap && out) out[nb] = qh_pauli_batch{first, count, groups, groups + 1 + (nb > 0 ? 1u : 0u)};
  }
  return nb;
}

}  // namespace qh
