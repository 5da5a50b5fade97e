"""Times qh_apply_pauli_sum (dst := (sum_t c_t P_t) src, out of place, into a second state of the same size) on a 30-qubit
state left permuted by a fused QFT flush, with qh_clone and qh_norm2 timed the same way in the same run as the yardsticks.

Cases, in complex128 and complex64; bits are chosen by PHYSICAL position (the layout the flush left, from qh_get_bitmap):
  * one Z string;
  * one X string per position class of its bit: sub-item (complex64), line, lane, wave, register index, chunk, top;
  * 16 ZZ terms (one batch, one group) and all 435 ZZ pairs (28 batches of one group);
  * the transverse-field Ising Hamiltonian: 30 X + 29 ZZ (31 x masks);
  * 100 terms over 20 x masks.
The call waits for its kernels, so each case is timed on the host (median of --reps calls, after one warm-up).  `kernels` and
`streams` are what qh_pauli_sum_plan predicts and qh_stats counts: a batch with G distinct x masks asks for G + 1 + [b > 0]
passes over the state.  `expected` is streams / 2 clones (a clone is two streams), `vs_expected` the measured time over that;
TB/s counts the requested bytes, an upper bound on HBM traffic.  One JSON line at the end holds every case.

  python tools/bench_pauli_sum.py [--nbits 30] [--reps 5] [--quick]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from qcc_amd import device, native, workloads  # noqa: E402


def timed(fn, reps):
  fn()
  times = []
  for _ in range(reps):
    t0 = time.perf_counter()
    fn()
    times.append((time.perf_counter() - t0) * 1e3)
  return statistics.median(times)


def cases(n, bw, phys_of_logical, rng):
  at = {p: b for b, p in enumerate(phys_of_logical)}
  ab = 0 if bw == 128 else 1
  m = lambda ps: sum(1 << at[p] for p in ps if p < n)      # noqa: E731
  pairs = [(i, j) for i in range(n) for j in range(i + 1, n)]
  rnd = lambda: int(rng.integers(0, 1 << n))               # noqa: E731
  xs20 = [rnd() for _ in range(20)]
  out = [('Z x1', [0], [m([n // 2])])]
  if ab:
    out.append(('X sub-item', [m([0])], [0]))
  out += [
      ('X line', [m([ab + 1])], [0]),
      ('X lane', [m([ab + 4])], [0]),
      ('X wave', [m([ab + 7])], [0]),
      ('X register index', [m([ab + 9])], [0]),
      ('X chunk', [m([ab + 14])], [0]),
      ('X top', [m([n - 1])], [0]),
      ('ZZ x16', [0] * 16, [(1 << i) | (1 << j) for i, j in pairs[:16]]),
      ('ZZ x435', [0] * len(pairs), [(1 << i) | (1 << j) for i, j in pairs]),
      ('Ising 30 X + 29 ZZ', [1 << q for q in range(n)] + [0] * (n - 1), [0] * n + [3 << q for q in range(n - 1)]),
      ('H 100 terms / 20 x', [xs20[t % 20] for t in range(100)], [rnd() for _ in range(100)]),
  ]
  return out


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--nbits', type=int, default=30)
  ap.add_argument('--reps', type=int, default=5)
  ap.add_argument('--quick', action='store_true', help='one timed call per case (kernel-name check under a profiler)')
  args = ap.parse_args()
  n, reps = args.nbits, 1 if args.quick else args.reps
  rows = []
  ops, g8 = workloads.qft_stream(range(n)).arrays()
  for bw in (128, 64):
    state_bytes = (bw // 8) << n
    with device.DeviceState(n, bw, fusion=native.QH_FUSE_SWEEP) as st, device.DeviceState(n, bw) as dst:
      st.init_basis(0x2345678 & ((1 << n) - 1))
      st.run_stream(ops, g8)
      st.flush()
      bm = (ctypes.c_int32 * n)()
      native.check(st.lib.qh_get_bitmap(st.h, bm))
      norm_ms = timed(st.norm2, reps)
      clone_ms = timed(lambda: st.clone().close(), reps)      # allocation included: what a caller of qh_clone sees
      copy_ms = timed(lambda: dst.copy_from(st), reps)        # the same two streams into memory that is already there
      for name, ms, streams in (('qh_norm2', norm_ms, 1), ('qh_clone', clone_ms, 2), ('qh_copy', copy_ms, 2)):
        tbs = streams * state_bytes / (ms * 1e-3) / 1e12
        rows.append({'bw': bw, 'case': name, 'ms': round(ms, 4), 'streams': streams, 'tbs': round(tbs, 3), 'permuted': list(bm) != list(range(n))})
        print(f'bw={bw:3d} {name:20s} {ms:8.3f} ms  {streams:3d} streams  {tbs:5.2f} TB/s', flush=True)
      two = min(clone_ms, copy_ms)      # the yardstick: two streams
      rng = np.random.default_rng(0)
      for name, xs, zs in cases(n, bw, list(bm), rng):
        coeffs = [complex(a, b) for a, b in rng.normal(size=(len(xs), 2))]
        _, batches = st.pauli_sum_plan(xs, zs)
        streams = sum(b['streams'] for b in batches)
        k0 = dst.stats()
        st.apply_pauli_sum(coeffs, xs, zs, out=dst)
        k1 = dst.stats()
        assert k1['kernels_launched'] - k0['kernels_launched'] == len(batches)
        assert k1['bytes_swept'] - k0['bytes_swept'] == streams * state_bytes
        ms = timed(lambda: st.apply_pauli_sum(coeffs, xs, zs, out=dst), reps)
        ms_norm = timed(lambda: st.apply_pauli_sum(coeffs, xs, zs, out=dst, norm=True), reps)
        expected = streams / 2.0 * two
        tbs = streams * state_bytes / (ms * 1e-3) / 1e12
        rows.append({'bw': bw, 'case': name, 'terms': len(xs), 'kernels': len(batches), 'groups': sum(b['ngroups'] for b in batches),
                     'streams': streams, 'ms': round(ms, 4), 'ms_with_norm2': round(ms_norm, 4), 'expected_ms': round(expected, 4),
                     'vs_expected': round(ms / expected, 3), 'tbs': round(tbs, 3)})
        print(f'bw={bw:3d} {name:20s} {ms:8.3f} ms  (norm2: {ms_norm:8.3f})  {len(batches):3d} kernels  {streams:3d} streams  '
              f'expected {expected:8.3f} ms  x{ms / expected:5.2f}  {tbs:5.2f} TB/s requested', flush=True)
  print(json.dumps({'tool': 'bench_pauli_sum', 'nbits': n, 'reps': reps, 'cases': rows}))


if __name__ == '__main__':
  main()
