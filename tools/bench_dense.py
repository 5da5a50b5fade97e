"""Times qh_apply_matrix (dense 2^K x 2^K matrices, K = 1..6) on a 30-qubit state with the engine's event timer.

Cases: complex128 and complex64; no control and one control; targets on the K highest bits ("high") and on bits that
include the 128-byte line bits 0-2 ("line").  Per case: milliseconds per call (median of --reps timed calls), TB/s on
algorithmic bytes (2S / 2^c), that as a fraction of 8 TB/s, and FP64 (or FP32) FMA/s (2^n / 2^c groups x 4^K complex
multiply-adds x 4 FMAs).  One JSON line at the end holds every case.

  python tools/bench_dense.py [--nbits 30] [--reps 5] [--quick]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from qcc_amd import device, native  # noqa: E402

PEAK_TBS = 8.0


def targets(kind, k, n):
  if kind == 'high':
    return list(range(n - k, n))
  return [0, 1, 2, 10, 11, 12][:k] if k > 3 else list(range(k))


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--nbits', type=int, default=30)
  ap.add_argument('--reps', type=int, default=5)
  ap.add_argument('--quick', action='store_true', help='one timed call per case (kernel-name check under a profiler)')
  args = ap.parse_args()
  n, reps = args.nbits, 1 if args.quick else args.reps
  rng = np.random.default_rng(0)
  rows = []
  for bw in (128, 64):
    with device.DeviceState(n, bw) as st:
      st.init_basis(0)
      for k in range(1, 7):
        a = rng.normal(size=(1 << k, 1 << k)) + 1j * rng.normal(size=(1 << k, 1 << k))
        m, _ = np.linalg.qr(a)
        for kind in ('high', 'line'):
          bits = targets(kind, k, n)
          for nctl in (0, 1):
            ctl = (1 << (20 if kind == 'line' else 5)) if nctl else 0
            st.apply_matrix(m, bits, ctl)                 # warm-up (and the staging ring's first use)
            st.sync()
            times = []
            for _ in range(reps):
              st.timer_begin()
              st.apply_matrix(m, bits, ctl)
              times.append(st.timer_end())
            ms = statistics.median(times)
            groups = (1 << n) >> (k + nctl)
            alg = (2 * (bw // 8) << n) >> nctl
            tbs = alg / (ms * 1e-3) / 1e12
            fma = groups * (4 ** k) * 4 / (ms * 1e-3)
            row = {'bw': bw, 'k': k, 'targets': kind, 'bits': bits, 'controls': nctl, 'ms': round(ms, 4),
                   'tbs': round(tbs, 3), 'of_8tbs': round(tbs / PEAK_TBS, 3), 'fma_per_s': float(f'{fma:.4g}')}
            rows.append(row)
            print(f'bw={bw:3d} K={k} {kind:4s} ctl={nctl}  {ms:8.3f} ms  {tbs:5.2f} TB/s  {tbs / PEAK_TBS:5.3f} of 8 TB/s  '
                  f'{fma:.3e} FMA/s', flush=True)
  print(json.dumps({'tool': 'bench_dense', 'nbits': n, 'reps': reps, 'cases': rows}))


if __name__ == '__main__':
  main()
