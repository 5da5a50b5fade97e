"""Times qh_expect_pauli on a 30-qubit state left permuted by a fused QFT flush, with qh_norm2 timed the same way in the same
run as the yardstick.

Cases, in complex128 and complex64; bits are chosen by PHYSICAL position (the layout the flush left, from qh_get_bitmap):
  * one Z string; 1 / 16 / 435 ZZ terms (all pairs of 30 bits: one X-group, x = 0);
  * one X string per position class of its bit: line (0-2), lane (3-5), chunk (6-11: wave / register index of the kernel),
    high, and a mixed X string over all classes;
  * 16 strings sharing one mixed x mask (a full batch of the pair kernel);
  * a weight-30 mixed string;
  * a 100-term Hamiltonian with 20 distinct x masks.
The call waits for its result, so each case is timed on the host (median of --reps calls, after one warm-up): what a caller
sees, the D2H copy included.  `reads` is the engine's count of passes over the state (qh_stats.kernels_launched), TB/s counts
those bytes.  One JSON line at the end holds every case.

  python tools/bench_expect.py [--nbits 30] [--reps 5] [--quick]
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

PEAK_TBS = 8.0


def timed(fn, reps):
  fn()
  times = []
  for _ in range(reps):
    t0 = time.perf_counter()
    fn()
    times.append((time.perf_counter() - t0) * 1e3)
  return statistics.median(times)


def cases(n, phys_of_logical, rng):
  at = {p: b for b, p in enumerate(phys_of_logical)}
  m = lambda ps: sum(1 << at[p] for p in ps if p < n)      # noqa: E731
  full = (1 << n) - 1
  pairs = [(i, j) for i in range(n) for j in range(i + 1, n)]
  mixed = m([1, 4, 9, 17, n - 1])
  rnd = lambda: int(rng.integers(0, 1 << n))               # noqa: E731
  xs20 = [rnd() for _ in range(20)]
  return [
      ('Z x1', [0], [m([n // 2])]),
      ('ZZ x1', [0], [m([2, n - 2])]),
      ('ZZ x16', [0] * 16, [(1 << i) | (1 << j) for i, j in pairs[:16]]),
      ('ZZ x435', [0] * len(pairs), [(1 << i) | (1 << j) for i, j in pairs]),
      ('X line', [m([1])], [0]),
      ('X lane', [m([4])], [0]),
      ('X chunk', [m([9])], [0]),
      ('X high', [m([n - 5])], [0]),
      ('X mixed', [mixed], [0]),
      ('X mixed x16', [mixed] * 16, [rnd() for _ in range(16)]),
      ('weight-n', [rnd() | m([n - 1])], [full]),
      ('H 100 terms / 20 x', [xs20[t % 20] for t in range(100)], [rnd() for _ in range(100)]),
  ]


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
    with device.DeviceState(n, bw, fusion=native.QH_FUSE_SWEEP) as st:
      st.init_basis(0x2345678 & ((1 << n) - 1))
      st.run_stream(ops, g8)
      st.flush()
      bm = (ctypes.c_int32 * n)()
      native.check(st.lib.qh_get_bitmap(st.h, bm))
      norm_ms = timed(st.norm2, reps)
      tbs = state_bytes / (norm_ms * 1e-3) / 1e12
      rows.append({'bw': bw, 'case': 'qh_norm2', 'ms': round(norm_ms, 4), 'reads': 1, 'tbs': round(tbs, 3),
                   'permuted': list(bm) != list(range(n))})
      print(f'bw={bw:3d} {"qh_norm2":20s} {norm_ms:8.3f} ms  {tbs:5.2f} TB/s', flush=True)
      for name, xs, zs in cases(n, list(bm), np.random.default_rng(0)):
        k0 = st.stats()['kernels_launched']
        st.expect_pauli(xs, zs)
        reads = st.stats()['kernels_launched'] - k0
        ms = timed(lambda: st.expect_pauli(xs, zs), reps)
        tbs = reads * state_bytes / (ms * 1e-3) / 1e12
        rows.append({'bw': bw, 'case': name, 'terms': len(xs), 'reads': reads, 'ms': round(ms, 4), 'per_read_vs_norm2': round(ms / reads / norm_ms, 3),
                     'tbs': round(tbs, 3), 'of_8tbs': round(tbs / PEAK_TBS, 3)})
        print(f'bw={bw:3d} {name:20s} {ms:8.3f} ms  {reads:3d} reads  {ms / reads / norm_ms:5.2f} x norm2 per read  {tbs:5.2f} TB/s', flush=True)
  print(json.dumps({'tool': 'bench_expect', 'nbits': n, 'reps': reps, 'cases': rows}))


if __name__ == '__main__':
  main()
