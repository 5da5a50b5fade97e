"""Times the sparse readers at 30 qubits, complex128 and complex64, with qh_norm2 timed the same way in the same process as
the yardstick (one read of the state):
  * qh_select on a GHZ state (2 hits), on a supremacy circuit's output at a threshold that keeps about 2^10 entries
    (found by bisection on count-only calls), and on a QFT's output with threshold 0, count only (every amplitude a hit);
  * qh_topk(16) on a peaked state (ry(0.2) on every qubit of |0>: one large amplitude, n ties behind it), on the
    supremacy output, on the QFT output (near-equal probabilities: refinement of the boundary bin) and on H applied to every
    qubit (2^n exact ties: six histograms, then the tie scan), and qh_topk(4096) on the supremacy output;
  * qh_amplitudes of 4096 sampled indices against 4096 qh_amplitude calls.
Every call is timed twice: between two HIP events on the handle's stream (qh_timer_begin / qh_timer_end), and on the host
around the call (what a caller sees: the read-backs, the host's sort and the waits included).  One warm-up call, then the
median of --reps calls.  `reads` is the growth of qh_stats.kernels_launched per call; x_norm2 is event time over qh_norm2's
in the same run, per_read that ratio over the number of reads.  One JSON line at the end holds every row.

  python tools/bench_readout.py [--nbits 30] [--reps 9] [--depth 20]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from qcc_amd import device, gates, native, workloads  # noqa: E402


def timed(st, fn, reps):
  """(median event ms, median host ms, kernels launched per call) of fn(), events on st's stream"""
  fn()
  ev, host = [], []
  k0 = st.stats()['kernels_launched']
  for _ in range(reps):
    st.timer_begin()
    t0 = time.perf_counter()
    fn()
    host.append((time.perf_counter() - t0) * 1e3)
    ev.append(st.timer_end())
  reads = (st.stats()['kernels_launched'] - k0) / reps
  return statistics.median(ev), statistics.median(host), reads


def fresh(n, bw):
  st = device.DeviceState(n, bw, fusion=native.QH_FUSE_SWEEP)
  st.init_basis(0)
  return st


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--nbits', type=int, default=30)
  ap.add_argument('--reps', type=int, default=9)
  ap.add_argument('--depth', type=int, default=20)
  args = ap.parse_args()
  n, reps = args.nbits, args.reps
  rows = []

  def row(bw, case, ev_ms, host_ms, reads, norm_ev, **more):
    r = {'bw': bw, 'case': case, 'event_ms': round(ev_ms, 4), 'host_ms': round(host_ms, 4), 'reads': round(reads, 2),
         'x_norm2': round(ev_ms / norm_ev, 3), **more}
    if reads >= 1:
      r['per_read'] = round(ev_ms / norm_ev / reads, 3)
    rows.append(r)
    extra = '  '.join(f'{k} {v}' for k, v in r.items() if k not in ('bw', 'case', 'event_ms', 'host_ms'))
    print(f'bw={bw:3d} {case:34s} {ev_ms:8.3f} ms (events) {host_ms:8.3f} ms (host)  {extra}', flush=True)

  for bw in (128, 64):
    # ---- GHZ: two hits
    with fresh(n, bw) as st:
      st.apply1(gates.hadamard(), 0)
      for q in range(1, n):
        st.applyc(gates.pauli_x(), q - 1, q)
      st.sync()
      norm_ev, norm_host, _ = timed(st, st.norm2, reps)
      row(bw, 'qh_norm2 (GHZ)', norm_ev, norm_host, 1, norm_ev)
      ev, host, reads = timed(st, lambda: st.select(0.25), reps)
      row(bw, 'qh_select GHZ, 2 hits', ev, host, reads, norm_ev, count=st.select(0.25)[2])
    # ---- peaked: ry(0.2) everywhere
    with fresh(n, bw) as st:
      for q in range(n):
        st.apply1(gates.ry(0.2), q)
      st.sync()
      nev, nhost, _ = timed(st, st.norm2, reps)
      row(bw, 'qh_norm2 (peaked)', nev, nhost, 1, nev)
      ev, host, reads = timed(st, lambda: st.topk(16), reps)
      row(bw, 'qh_topk(16) peaked', ev, host, reads, nev, first=int(st.topk(16)[0][0]))
    # ---- supremacy
    with fresh(n, bw) as st:
      st.run_stream(*workloads.supremacy_stream(n, args.depth, seed=0).arrays())
      st.sync()
      nev, nhost, _ = timed(st, st.norm2, reps)
      row(bw, 'qh_norm2 (supremacy)', nev, nhost, 1, nev)
      lo, hi = 0.0, 1.0                       # the threshold that keeps about 2^10 entries: bisection on count-only calls
      for _ in range(60):
        thr = 0.5 * (lo + hi)
        lo, hi = (thr, hi) if st.select(thr, 0)[2] > 1 << 10 else (lo, thr)
      thr = hi
      ev, host, reads = timed(st, lambda: st.select(thr), reps)
      row(bw, 'qh_select supremacy, ~2^10 hits', ev, host, reads, nev, count=st.select(thr)[2], threshold=thr)
      ev, host, reads = timed(st, lambda: st.topk(16), reps)
      row(bw, 'qh_topk(16) supremacy', ev, host, reads, nev)
      ev, host, reads = timed(st, lambda: st.topk(4096), reps)
      row(bw, 'qh_topk(4096) supremacy', ev, host, reads, nev)
      u = np.sort(np.random.default_rng(1).random(4096))
      shots = st.sample(u)
      ev, host, reads = timed(st, lambda: st.amplitudes(shots), reps)
      row(bw, 'qh_amplitudes, 4096 indices', ev, host, reads, nev)
      ev, host, reads = timed(st, lambda: [st.amplitude(int(i)) for i in shots], max(1, reps // 3))
      row(bw, 'qh_amplitude x 4096', ev, host, reads, nev)
    # ---- QFT of a basis state: flat
    with fresh(n, bw) as st:
      st.init_basis(int('1011' * n, 2) & ((1 << n) - 1))
      st.run_stream(*workloads.qft_stream(range(n)).arrays())
      st.sync()
      nev, nhost, _ = timed(st, st.norm2, reps)
      row(bw, 'qh_norm2 (QFT output)', nev, nhost, 1, nev)
      ev, host, reads = timed(st, lambda: st.select(0.0, 0), reps)
      row(bw, 'qh_select QFT, thr 0, count only', ev, host, reads, nev, count=st.select(0.0, 0)[2])
      ev, host, reads = timed(st, lambda: st.topk(16), reps)
      row(bw, 'qh_topk(16) QFT output', ev, host, reads, nev)
    # ---- H on every qubit: 2^n bitwise-equal amplitudes, the worst case of qh_topk (six histograms, then the tie scan)
    with fresh(n, bw) as st:
      for q in range(n):
        st.apply1(gates.hadamard(), q)
      st.sync()
      nev, nhost, _ = timed(st, st.norm2, reps)
      row(bw, 'qh_norm2 (H on every qubit)', nev, nhost, 1, nev)
      ev, host, reads = timed(st, lambda: st.topk(16), reps)
      row(bw, 'qh_topk(16) H on every qubit', ev, host, reads, nev, last=int(st.topk(16)[0][-1]))
  print(json.dumps({'tool': 'bench_readout', 'nbits': n, 'reps': reps, 'depth': args.depth, 'rows': rows}))


if __name__ == '__main__':
  main()
