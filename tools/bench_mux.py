"""Times qh_apply_mux / qh_apply_diag (gates selected by a table over k bits) on a 30-qubit state with the engine's event
timer, on the permuted layout a fused QFT flush leaves.

Cases are placed by PHYSICAL position (through qh_get_bitmap) so that each takes the tier it is named after: selectors above
the lane bits (scalar loads), selectors on lane bits with a table that fits LDS, larger tables through L2 with scattered
selectors, and a mux target inside the 128-byte line.  Baselines in the same run: the same target bit through qh_apply_bits
with fusion off (mux) and qh_scale (diag).  Per case: milliseconds per call (median of --reps timed calls), the ratio to the
baseline and the fraction of 8 TB/s on the state once read and once written.  One JSON line at the end holds every case.

  python tools/bench_mux.py [--nbits 30] [--reps 5] [--quick]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from qcc_amd import device, native, workloads  # noqa: E402

PEAK_TBS = 8.0


def scattered(n, k, avoid, seed):
  """k physical positions spread over the index, bit 0 among them, none in `avoid`"""
  rng = np.random.default_rng(seed)
  pool = [p for p in range(1, n) if p not in avoid]
  return [0] + sorted(int(p) for p in rng.choice(pool, size=k - 1, replace=False)) if k else []


def mux_cases(n, bw):
  lds_k = 10 if bw == 128 else 11                 # the largest mux table that fits 64 KiB
  hi = lambda k: list(range(n - k, n))            # noqa: E731
  return [
      ('tier1', 4, hi(4), 10),
      ('tier1', 16, [p for p in range(n - 17, n) if p != n - 9][:16], n - 9),
      ('tier2-lane-selectors', lds_k, list(range(6)) + list(range(12, 12 + lds_k - 6)), 10),
      ('tier3-scattered', lds_k + 1, scattered(n, lds_k + 1, {10}, 1), 10),
      ('tier3-scattered', 16, scattered(n, 16, {10}, 2), 10),
      ('line-target', 4, [3, 9, 15, 22], 1),
      ('line-target-tier1', 4, hi(4), 1),
  ]


def diag_cases(n, bw):
  lds_k = 12 if bw == 128 else 13
  hi = lambda k: list(range(n - k, n))            # noqa: E731
  return [
      ('tier1', 4, hi(4)),
      ('tier1', 16, hi(16)),
      ('tier2-lane-selectors', lds_k, list(range(6)) + list(range(12, 12 + lds_k - 6))),
      ('tier3-scattered', lds_k + 1, scattered(n, lds_k + 1, set(), 3)),
      ('tier3-scattered', 16, scattered(n, 16, set(), 4)),
  ]


def timed(st, reps, fn):
  fn()                                            # warm-up (and the table buffer's growth)
  st.sync()
  times = []
  for _ in range(reps):
    st.timer_begin()
    fn()
    times.append(st.timer_end())
  return statistics.median(times)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--nbits', type=int, default=30)
  ap.add_argument('--reps', type=int, default=5)
  ap.add_argument('--quick', action='store_true', help='one timed call per case (kernel-name check under a profiler)')
  args = ap.parse_args()
  n, reps = args.nbits, 1 if args.quick else args.reps
  rng = np.random.default_rng(0)
  h_gate = np.array([[1, 1], [1, -1]], dtype=np.complex128) / np.sqrt(2)
  qft_ops, qft_g8 = workloads.qft_stream(range(n)).arrays()
  rows = []
  for bw in (128, 64):
    state_bytes = 2 * (bw // 8) << n
    with device.DeviceState(n, bw, fusion=native.QH_FUSE_SWEEP) as st:
      st.init_basis(0x2CB9A5 & ((1 << n) - 1))
      st.run_stream(qft_ops, qft_g8)
      st.flush()
      st.set_fusion(native.QH_FUSE_OFF)
      bm = (ctypes.c_int32 * n)()
      native.check(st.lib.qh_get_bitmap(st.h, bm))
      at = {p: b for b, p in enumerate(bm)}       # logical bit on physical position p
      permuted = list(bm) != list(range(n))

      def report(call, tier, k, ms, base_ms, base, where):
        tbs = state_bytes / (ms * 1e-3) / 1e12
        rows.append({'call': call, 'bw': bw, 'tier': tier, 'k': k, 'ms': round(ms, 4), 'baseline': base,
                     'baseline_ms': round(base_ms, 4), 'ratio': round(ms / base_ms, 3), 'tbs': round(tbs, 3),
                     'of_8tbs': round(tbs / PEAK_TBS, 3), 'physical': where, 'permuted_layout': permuted})
        print(f'{call:4s} bw={bw:3d} {tier:22s} k={k:2d}  {ms:8.3f} ms  baseline {base} {base_ms:8.3f} ms  x{ms / base_ms:5.2f}  '
              f'{tbs:5.2f} TB/s  {tbs / PEAK_TBS:5.3f} of 8 TB/s', flush=True)

      for tier, k, selp, tp in mux_cases(n, bw):
        g, _ = np.linalg.qr(rng.normal(size=(1 << k, 2, 2)) + 1j * rng.normal(size=(1 << k, 2, 2)))
        sel, tgt = [at[p] for p in selp], at[tp]
        base_ms = timed(st, reps, lambda: st.apply_bits(0, tgt, h_gate))
        ms = timed(st, reps, lambda: st.apply_mux(g, sel, tgt))
        report('mux', tier, k, ms, base_ms, 'qh_apply_bits', {'selectors': selp, 'target': tp})
      for tier, k, bitp in diag_cases(n, bw):
        v = np.exp(1j * rng.uniform(0, 2 * np.pi, size=1 << k))
        bits = [at[p] for p in bitp]
        base_ms = timed(st, reps, lambda: st.scale(np.exp(0.3j)))
        ms = timed(st, reps, lambda: st.apply_diag(v, bits))
        report('diag', tier, k, ms, base_ms, 'qh_scale', {'bits': bitp})
  print(json.dumps({'tool': 'bench_mux', 'nbits': n, 'reps': reps, 'cases': rows}))


if __name__ == '__main__':
  main()
