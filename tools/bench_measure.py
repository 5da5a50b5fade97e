"""Times the register readers qh_marginal, qh_sample and qh_project_bits on a 30-qubit state left permuted by a fused flush.

Cases, in complex128 and complex64:
  * marginal for k = 1, 4, 8, 12, 16 on bits at PHYSICAL positions (the layout the flush left, from qh_get_bitmap):
    low (0..k-1), lane (from 3 up), high (the top k) and a mixed set spread over the whole index;
  * sample for 1, 10^3, 10^6 and 10^7 shots (sorted uniforms);
  * project_bits for k = 1 and 8.
The readers wait for their result, so each case is timed on the host (median of --reps calls, after one warm-up): what a
caller sees, D2H copies and the sampler's host-side placement included.  TB/s counts one read of the state (marginal) or
the bytes written (projection).  One JSON line at the end holds every case.

  python tools/bench_measure.py [--nbits 30] [--reps 5] [--quick]
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


def bit_sets(k, n, phys_of_logical):
  """LOGICAL bits whose PHYSICAL positions (in the layout the flush left) are the low bits 0..k-1, the lane bits from 3
  up, the top k bits, or k positions spread over the whole index"""
  logical_at = {p: b for b, p in enumerate(phys_of_logical)}
  spread = sorted({int(round(i * (n - 1) / max(1, k - 1))) for i in range(k)}) if k > 1 else [n // 2]
  return {name: [logical_at[p] for p in pos] for name, pos in
          (('low', range(k)), ('lane', range(3, 3 + k)), ('high', range(n - k, n)), ('mixed', spread))}


def timed(fn, reps):
  fn()
  times = []
  for _ in range(reps):
    t0 = time.perf_counter()
    fn()
    times.append((time.perf_counter() - t0) * 1e3)
  return statistics.median(times)


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
      permuted = list(bm) != list(range(n))
      for k in (1, 4, 8, 12, 16):
        for kind, bits in bit_sets(k, n, list(bm)).items():
          ms = timed(lambda: st.marginal(bits), reps)
          tbs = state_bytes / (ms * 1e-3) / 1e12
          rows.append({'bw': bw, 'op': 'marginal', 'k': len(bits), 'bits': kind, 'ms': round(ms, 4), 'tbs': round(tbs, 3),
                       'of_8tbs': round(tbs / PEAK_TBS, 3)})
          print(f'bw={bw:3d} marginal k={len(bits):2d} {kind:5s} {ms:8.3f} ms  {tbs:5.2f} TB/s (one read)', flush=True)
      rng = np.random.default_rng(0)
      for shots in (1, 10 ** 3, 10 ** 6, 10 ** 7):
        u = np.sort(rng.random(shots))
        ms = timed(lambda: st.sample(u), reps if shots < 10 ** 7 else min(reps, 3))
        rows.append({'bw': bw, 'op': 'sample', 'shots': shots, 'ms': round(ms, 4),
                     'read_passes': round(ms / (state_bytes / (PEAK_TBS * 0.8e12) * 1e3), 2)})
        print(f'bw={bw:3d} sample shots={shots:>8d} {ms:8.3f} ms', flush=True)
      for k in (1, 8):
        mask = sum(1 << b for b in bit_sets(k, n, list(bm))['mixed'])
        ms = timed(lambda: st.project_bits(mask, 0) or st.sync(), reps)
        written = state_bytes - (state_bytes >> k)
        tbs = written / (ms * 1e-3) / 1e12
        rows.append({'bw': bw, 'op': 'project_bits', 'k': k, 'ms': round(ms, 4), 'tbs': round(tbs, 3)})
        print(f'bw={bw:3d} project_bits k={k} {ms:8.3f} ms  {tbs:5.2f} TB/s (bytes written)', flush=True)
      rows.append({'bw': bw, 'op': 'layout', 'permuted': permuted})
  print(json.dumps({'tool': 'bench_measure', 'nbits': n, 'reps': reps, 'cases': rows}))


if __name__ == '__main__':
  main()
