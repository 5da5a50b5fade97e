"""Times qh_apply_pauli_product (state := F_{n-1} ... F_0 state in place, F_t = a_t I + b_t P_t) on a 30-qubit state left
permuted by a fused QFT flush, with its yardsticks timed the same way in the same run:
  * qh_apply_diag with k = 1 on the same handle: one in-place read + write of the state;
  * the three-call composition of a rotation, qh_pauli_sum_new + qh_axpby (+ the release of the second state);
  * the same rotation as a CX ladder + rz through a fused flush, for weights 2, 8 and 30.

Cases, in complex128 and complex64; bits are chosen by PHYSICAL position (the layout the flush left, from qh_get_bitmap):
  * one rotation per position class of its pivot: sub-item (complex64: HALF), line, lane, wave, register index, chunk, top;
  * one diagonal rotation;
  * DIAG and PAIR runs of 1, 4, 8 and 16 terms (one kernel each while the run fits QH_PAULI_PRODUCT_BATCH), the same for a
    PAIR run whose pivot lies inside the 128-byte line (the in-wave walk: twice the arithmetic per amplitude) and, in
    complex64, for X == 1 (HALF);
  * rotations about Z...Z of weight 2, 8 and 30 (against the ladders);
  * one first-order Ising step: 30 X + 29 ZZ.
Every call is followed by qh_sync and timed on the host (median of --reps calls, after one warm-up).  `runs` is what
qh_pauli_product_plan predicts and qh_stats counts.  `vs_diag` is the time over runs x the k = 1 qh_apply_diag: above 1.25 a
run costs more than a memory pass.  One JSON line at the end holds every case.

  python tools/bench_pauli_product.py [--nbits 30] [--reps 5] [--quick]

A/B builds.  pauli_product_plan.h has two compile-time switches, the slots per run and the highest pivot that takes the in-wave
walk.  The rows that decided their defaults (profiles/pauli_product/bench_pauli_product_slots16_nolane.txt) come from

  hipcc --offload-arch=gfx950 -O3 -std=c++17 -shared -fPIC -DQH_PAULI_PRODUCT_SLOTS=16 -DQH_PAULI_LANE_PIVOT_MAX=-1 \
        -o /tmp/libqcc_hip_slots16_nolane.so qcc_amd/csrc/engine.hip qcc_amd/csrc/libq_facade.cc
  QCC_HIP_LIB=/tmp/libqcc_hip_slots16_nolane.so python tools/bench_pauli_product.py
"""
import argparse
import ctypes
import json
import math
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from qcc_amd import device, gates, native, workloads  # noqa: E402


def timed(fn, reps):
  fn()
  times = []
  for _ in range(reps):
    t0 = time.perf_counter()
    fn()
    times.append((time.perf_counter() - t0) * 1e3)
  return statistics.median(times)


def rot(theta):
  return math.cos(theta), -1j * math.sin(theta)


def cases(n, bw, phys_of_logical, rng):
  at = {p: b for b, p in enumerate(phys_of_logical)}
  ab = 0 if bw == 128 else 1
  m = lambda ps: sum(1 << at[p] for p in ps if p < n)      # noqa: E731
  rnd = lambda: int(rng.integers(0, 1 << n))               # noqa: E731
  out = []
  if ab:
    out.append(('X sub-item', [m([0])], [0]))
  out += [(f'X {name}', [m([p])], [0]) for name, p in (('line', ab + 1), ('lane', ab + 4), ('wave', ab + 7), ('register index', ab + 9),
                                                         ('chunk', ab + 14), ('top', n - 1))]
  out.append(('Z x1', [0], [m([n // 2])]))
  X = m([ab + 5, ab + 12, n - 2])
  for k in (1, 4, 8, 16):
    out.append((f'DIAG run x{k}', [0] * k, [rnd() for _ in range(k)]))
    out.append((f'PAIR run x{k}', [X] * k, [rnd() for _ in range(k)]))
  for k in (1, 4, 8, 16):
    out.append((f'in-line PAIR run x{k}', [m([ab + 1, 0])] * k, [rnd() for _ in range(k)]))
    if ab:
      out.append((f'HALF run x{k}', [m([0])] * k, [rnd() for _ in range(k)]))
  for w in (2, 8, 30):
    if w <= n:
      out.append((f'ZZ..Z weight {w}', [0], [sum(1 << (n - 1 - q) for q in range(w))]))
  out.append(('Ising step 30 X + 29 ZZ', [1 << q for q in range(n)] + [0] * (n - 1), [0] * n + [3 << q for q in range(n - 1)]))
  return out


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--nbits', type=int, default=30)
  ap.add_argument('--reps', type=int, default=5)
  ap.add_argument('--quick', action='store_true', help='one timed call per case (kernel-name check under a profiler)')
  args = ap.parse_args()
  n, reps = args.nbits, 1 if args.quick else args.reps
  rows, slots = [], 0
  ops, g8 = workloads.qft_stream(range(n)).arrays()
  for bw in (128, 64):
    state_bytes = (bw // 8) << n
    with device.DeviceState(n, bw, fusion=native.QH_FUSE_SWEEP) as st:
      st.init_basis(0x2345678 & ((1 << n) - 1))
      st.run_stream(ops, g8)
      st.flush()
      bm = (ctypes.c_int32 * n)()
      native.check(st.lib.qh_get_bitmap(st.h, bm))
      rng = np.random.default_rng(0)

      def synced(fn):
        def run():
          fn()
          st.sync()
        return run
      phase = np.exp(1j * 0.3)
      diag_ms = timed(synced(lambda: st.apply_diag([np.conj(phase), phase], [n // 2])), reps)
      rows.append({'bw': bw, 'case': 'qh_apply_diag k=1', 'ms': round(diag_ms, 4), 'tbs': round(2 * state_bytes / (diag_ms * 1e-3) / 1e12, 3),
                   'permuted': list(bm) != list(range(n))})
      print(f'bw={bw:3d} {"qh_apply_diag k=1":26s} {diag_ms:8.3f} ms  {2 * state_bytes / (diag_ms * 1e-3) / 1e12:5.2f} TB/s', flush=True)

      # the three-call composition of one rotation: w = (-i sin P) psi in a second state, psi := cos psi + w, the second state released
      zz = sum(1 << (n - 1 - q) for q in range(min(8, n)))
      c, s = rot(0.3)

      def three_calls():
        w = st.apply_pauli_sum([s], [0], [zz])
        st.axpby(c, w, 1.0)
        w.close()
      comp_ms = timed(synced(three_calls), reps)
      rows.append({'bw': bw, 'case': 'pauli_sum_new + axpby', 'ms': round(comp_ms, 4)})
      print(f'bw={bw:3d} {"pauli_sum_new + axpby":26s} {comp_ms:8.3f} ms', flush=True)

      # the same rotation as a CX ladder + rz through a fused flush
      ladder_ms = {}
      xg, rz = gates.pauli_x(), gates.rz(0.6)
      for w in (2, 8, 30):
        if w > n:
          continue

        def ladder():
          for q in range(w - 1):
            st.applyc(xg, q, q + 1)
          st.apply1(rz, w - 1)
          for q in reversed(range(w - 1)):
            st.applyc(xg, q, q + 1)
          st.flush()
        ladder_ms[w] = timed(synced(ladder), reps)
        rows.append({'bw': bw, 'case': f'CX ladder + rz weight {w}', 'gates': 2 * (w - 1) + 1, 'ms': round(ladder_ms[w], 4)})
        print(f'bw={bw:3d} {f"CX ladder + rz weight {w}":26s} {ladder_ms[w]:8.3f} ms  {2 * (w - 1) + 1:3d} gates', flush=True)
      native.check(st.lib.qh_get_bitmap(st.h, bm))      # (the ladders' flushes may have re-laid the state out)

      for name, xs, zs in cases(n, bw, list(bm), rng):
        ab_ = [rot(float(t)) for t in rng.uniform(-1.5, 1.5, size=len(xs))]
        a, b = [u for u, _ in ab_], [v for _, v in ab_]
        _, runs = st.pauli_product_plan(xs, zs)
        slots = max([slots] + [r['count'] for r in runs])
        k0 = st.stats()
        st.apply_pauli_product(a, b, xs, zs)
        k1 = st.stats()
        assert k1['kernels_launched'] - k0['kernels_launched'] == len(runs)
        assert k1['bytes_swept'] - k0['bytes_swept'] == 2 * len(runs) * state_bytes
        ms = timed(synced(lambda: st.apply_pauli_product(a, b, xs, zs)), reps)
        ms_norm = timed(lambda: st.apply_pauli_product(a, b, xs, zs, norm=True), reps)
        tbs = 2 * len(runs) * state_bytes / (ms * 1e-3) / 1e12
        row = {'bw': bw, 'case': name, 'terms': len(xs), 'runs': len(runs), 'kinds': sorted({r['kind'] for r in runs}), 'ms': round(ms, 4),
               'ms_with_norm2': round(ms_norm, 4), 'ms_per_term': round(ms / len(xs), 4), 'vs_diag': round(ms / (len(runs) * diag_ms), 3),
               'vs_three_calls': round(ms / (len(xs) * comp_ms), 4), 'tbs': round(tbs, 3)}
        extra = ''
        if name.startswith('ZZ..Z weight'):
          w = int(name.split()[-1])
          row['vs_ladder'] = round(ms / ladder_ms[w], 4)
          extra = f'  x{row["vs_ladder"]:6.3f} of the ladder'
        rows.append(row)
        print(f'bw={bw:3d} {name:26s} {ms:8.3f} ms  (norm2: {ms_norm:8.3f})  {len(xs):3d} terms  {len(runs):3d} runs  {ms / len(xs):7.3f} ms/term  '
              f'x{row["vs_diag"]:5.2f} of runs x diag  x{row["vs_three_calls"]:6.3f} of the three calls  {tbs:5.2f} TB/s{extra}', flush=True)
  print(json.dumps({'tool': 'bench_pauli_product', 'nbits': n, 'reps': reps, 'batch': native.QH_PAULI_PRODUCT_BATCH, 'largest_run': slots, 'lib': os.path.basename(native.LIB_PATH), 'cases': rows}))


if __name__ == '__main__':
  main()
