"""Times qh_extend and qh_release at 30 qubits, complex128 and complex64, beside qh_norm2 (one read of one state) and
qh_clone (allocation + a device-to-device copy of the state) from the same run:
  * qh_extend 29 -> 30, with a basis factor and with a table factor;
  * qh_release 30 -> 29 of one bit: the top logical bit, logical bit 0, and the logical bit that sits in the middle of the
    layout the relayout sweeps left (physical position nbits / 2).
The states are supremacy circuits of --depth layers, fused.  Every call is timed between two HIP events on the source's
stream (qh_timer_begin / qh_timer_end around the blocking call: allocation, kernel and the wait included) and on the host.  One
warm-up call, then the median of --reps calls; every call allocates, and the previous result is freed OUTSIDE the timed
window.  TB/s counts the bytes the call has to move: src read once plus the new state written once (qh_clone: 2 S).
The rows, and one JSON line holding them all, go to stdout and to profiles/resize/bench_resize.txt.

  python tools/bench_resize.py [--nbits 30] [--reps 9] [--depth 20]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from qcc_amd import device, native, workloads  # noqa: E402


def prepared(n, bw, depth, seed):
  st = device.DeviceState(n, bw, fusion=native.QH_FUSE_SWEEP)
  ops, g8 = workloads.supremacy_stream(n, depth, seed=seed).arrays()
  st.init_basis(0)
  st.run_stream(ops, g8)
  st.sync()
  return st


def bitmap(st):
  bm = (ctypes.c_int32 * st.nbits)()
  native.check(st.lib.qh_get_bitmap(st.h, bm))
  return list(bm)


def timed_making(src, make, reps):
  """(median event ms, median host ms) of make() -> a new handle; the previous one is closed outside the window"""
  made = make()
  ev, host = [], []
  for _ in range(reps):
    made.close()
    src.timer_begin()
    t0 = time.perf_counter()
    made = make()
    host.append((time.perf_counter() - t0) * 1e3)
    ev.append(src.timer_end())
  made.close()
  return statistics.median(ev), statistics.median(host)


def timed(src, fn, reps):
  fn()
  ev, host = [], []
  for _ in range(reps):
    src.timer_begin()
    t0 = time.perf_counter()
    fn()
    host.append((time.perf_counter() - t0) * 1e3)
    ev.append(src.timer_end())
  return statistics.median(ev), statistics.median(host)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--nbits', type=int, default=30)
  ap.add_argument('--reps', type=int, default=9)
  ap.add_argument('--depth', type=int, default=20)
  ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'resize', 'bench_resize.txt'))
  args = ap.parse_args()
  n, reps = args.nbits, args.reps
  rows, lines = [], []

  def say(text):
    print(text, flush=True)
    lines.append(text)

  def row(bw, case, ev_ms, host_ms, moved, clone_ms=None, norm_ms=None, **more):
    r = {'bw': bw, 'case': case, 'event_ms': round(ev_ms, 4), 'host_ms': round(host_ms, 4), 'tbs': round(moved / (ev_ms * 1e-3) / 1e12, 3), **more}
    if clone_ms:
      r['vs_clone'] = round(ev_ms / clone_ms, 3)
    if norm_ms:
      r['vs_norm2'] = round(ev_ms / norm_ms, 3)
    rows.append(r)
    extra = '  '.join(f'{k} {v}' for k, v in r.items() if k not in ('bw', 'case', 'event_ms', 'host_ms', 'tbs'))
    say(f'bw={bw:3d} {case:34s} {ev_ms:8.3f} ms (events) {host_ms:8.3f} ms (host)  {r["tbs"]:6.3f} TB/s  {extra}')

  for bw in (128, 64):
    S = (bw // 8) << n                                  # bytes of an n-qubit state
    with prepared(n, bw, args.depth, 0) as a:
      norm_ev, norm_host = timed(a, a.norm2, reps)
      row(bw, f'qh_norm2 {n}', norm_ev, norm_host, S)
      clone_ev, clone_host = timed_making(a, a.clone, reps)
      row(bw, f'qh_clone {n}', clone_ev, clone_host, 2 * S, norm_ms=norm_ev)
      bm = bitmap(a)
      cases = [('top logical bit', n - 1), ('logical bit 0', 0), (f'bit at physical {n // 2}', bm.index(n // 2))]
      for name, bit in cases:
        ev, host = timed_making(a, lambda b=bit: a.release([b], 1)[0], reps)
        row(bw, f'qh_release {n}->{n - 1} {name}', ev, host, S + S // 2, clone_ev, norm_ev, logical=bit, physical=bm[bit])
    with prepared(n - 1, bw, args.depth, 0) as b:
      ev, host = timed_making(b, lambda: b.extend(1, basis=1), reps)
      row(bw, f'qh_extend {n - 1}->{n} basis', ev, host, S // 2 + S, clone_ev, norm_ev)
      ev, host = timed_making(b, lambda: b.extend(1, amps=[0.6, 0.8j]), reps)
      row(bw, f'qh_extend {n - 1}->{n} table', ev, host, S // 2 + S, clone_ev, norm_ev)
  say(json.dumps({'tool': 'bench_resize', 'nbits': n, 'reps': reps, 'depth': args.depth, 'rows': rows}))
  os.makedirs(os.path.dirname(args.out), exist_ok=True)
  with open(args.out, 'w') as f:
    f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
  main()
