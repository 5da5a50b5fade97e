"""Times qh_apply_perm at 30 qubits, complex128 and complex64, beside qh_apply_diag on the same bits in the same process (the
yardstick: it too is one read and one write of the state behind a table) and beside qh_clone / qh_copy (one read, one write,
no table):
  * tables: x -> a x mod N (qc.modmul's table) over k = 5, 10 and 13 bits, without a control and under one control;
  * the register placed on the top bits, on the lane bits from position 3 up, across the line bits (from position 1 up) and
    scattered over the whole index.
Every call is timed twice: between two HIP events on the handle's stream (qh_timer_begin / qh_timer_end), and on the host
around the call.  One warm-up call, then the median of --reps calls.  GB/s counts bytes read + written by the algorithm's
minimum (the state once each way; half of it under the control).  One JSON line at the end holds every row.

  python tools/bench_perm.py [--nbits 30] [--reps 7] [--widths 128,64]
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from qcc_amd import device, native  # noqa: E402


def timed(st, fn, reps):
  """(median event ms, median host ms) of fn(), events on st's stream"""
  fn()
  st.sync()
  ev, host = [], []
  for _ in range(reps):
    st.timer_begin()
    t0 = time.perf_counter()
    fn()
    host.append((time.perf_counter() - t0) * 1e3)
    ev.append(st.timer_end())
  return statistics.median(ev), statistics.median(host)


def modmul_table(k):
  """x -> a x mod N for x < N, identity above: N the largest prime below 2^k, a of full multiplicative order or close to it"""
  size = 1 << k
  N = next(v for v in range(size - 1, 1, -1) if all(v % d for d in range(2, int(math.isqrt(v)) + 1)))
  a = next(v for v in range(N // 3, N) if math.gcd(v, N) == 1)
  x = np.arange(size, dtype=np.int64)
  return np.where(x < N, (x * a) % N, x), a, N


def placements(n, k):
  step = (n - 1) / (k - 1) if k > 1 else 0
  return [('top', list(range(n - k, n))), ('lane 3+', list(range(3, 3 + k))), ('across line', list(range(1, 1 + k))),
          ('scattered', sorted({int(round(j * step)) for j in range(k)}))]


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--nbits', type=int, default=30)
  ap.add_argument('--reps', type=int, default=7)
  ap.add_argument('--widths', default='128,64')
  ap.add_argument('--ks', default='5,10,13')
  args = ap.parse_args()
  n, reps = args.nbits, args.reps
  rows = []

  def row(**r):
    rows.append(r)
    print('  '.join(f'{k} {v}' for k, v in r.items()), flush=True)

  for bw in (int(w) for w in args.widths.split(',')):
    state_bytes = (bw // 8) << n
    with device.DeviceState(n, bw) as st:
      st.init_basis(1)
      st.sync()
      c = st.clone()
      ev_t = []
      for _ in range(3):                       # qh_clone: allocation + copy; the previous clone is released outside the window
        c.close()
        st.timer_begin()
        c = st.clone()
        ev_t.append(st.timer_end())
      clone_ms = statistics.median(ev_t)
      copy_ms, _ = timed(st, lambda: c.copy_from(st), reps)
      c.close()
      row(bw=bw, case='qh_clone', event_ms=round(clone_ms, 3), gbs=round(2 * state_bytes / clone_ms / 1e6, 1))
      row(bw=bw, case='qh_copy', event_ms=round(copy_ms, 3), gbs=round(2 * state_bytes / copy_ms / 1e6, 1))
      for k in (int(v) for v in args.ks.split(',')):
        table, a, N = modmul_table(k)
        values = np.exp(2j * np.pi * np.arange(1 << k) / (1 << k))
        for name, reg in placements(n, k):
          if len(reg) != k:
            continue
          free = [b for b in range(n - 1, -1, -1) if b not in reg]
          diag_ms, diag_host = timed(st, lambda: st.apply_diag(values, reg), reps)
          for ctl_bit in (None, free[0]):
            ctl = 0 if ctl_bit is None else 1 << ctl_bit
            plan = st.perm_plan(reg, ctl)
            ev, host = timed(st, lambda: st.apply_perm(table, reg, ctl), reps)
            moved = 2 * state_bytes // (2 if ctl else 1)
            row(bw=bw, case=f'perm k={k} {name}', ctl=ctl_bit, path='lds' if plan['path'] == native.QH_PERM_LDS else 'gather',
                tile_bits=plan['tile_bits'], event_ms=round(ev, 3), host_ms=round(host, 3), gbs=round(moved / ev / 1e6, 1),
                diag_ms=round(diag_ms, 3), vs_diag=round(ev / diag_ms, 3), vs_clone_plus_copy=round(ev / (clone_ms + copy_ms), 3),
                a=a, N=N)
  print(json.dumps({'tool': 'bench_perm', 'nbits': n, 'reps': reps, 'rows': rows}))


if __name__ == '__main__':
  main()
