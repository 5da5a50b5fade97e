"""Times qh_reduced_density at 30 qubits, complex128 and complex64, k = 1, 2, 4, 6, 7, 8, with qh_norm2 (one read of the
state) and qh_marginal on the same bits timed the same way in the same process.  The state is the output of a supremacy
circuit run with fused sweeps, so the bit map is the one such a circuit leaves; the register sits
  * low      on the k lowest PHYSICAL positions (line and lane bits),
  * top      on the k highest physical positions,
  * circuit  on logical bits n-k..n-1 (qubits 0..k-1), wherever the circuit left them.
Every call is timed between two HIP events on the handle's stream (qh_timer_begin / qh_timer_end: the fold kernel and the
copy of the result included) and on the host around the call.  One warm-up call, then the median of --reps calls.
x_norm2 is event time over qh_norm2's; GB/s is the state's bytes over the event time; TF_exec counts the FP64 flop the tile
kernels execute (8 per complex multiply-add: block_pairs * 4^tile_bits of them per column), TF_herm the 4 * 2^k flop per
amplitude of the Hermitian half.  One JSON line at the end holds every row.

  python tools/bench_density.py [--nbits 30] [--reps 7] [--depth 20] [--widths 128,64] [--ks 1,2,4,6,7,8]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from qcc_amd import device, native, workloads  # noqa: E402


def timed(st, fn, reps):
  """(median event ms, median host ms) of fn(), events on st's stream"""
  fn()
  ev, host = [], []
  for _ in range(reps):
    st.timer_begin()
    t0 = time.perf_counter()
    fn()
    host.append((time.perf_counter() - t0) * 1e3)
    ev.append(st.timer_end())
  return statistics.median(ev), statistics.median(host)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--nbits', type=int, default=30)
  ap.add_argument('--reps', type=int, default=7)
  ap.add_argument('--depth', type=int, default=20)
  ap.add_argument('--widths', default='128,64')
  ap.add_argument('--ks', default='1,2,4,6,7,8')
  args = ap.parse_args()
  n, reps = args.nbits, args.reps
  rows = []
  for bw in (int(w) for w in args.widths.split(',')):
    with device.DeviceState(n, bw, fusion=native.QH_FUSE_SWEEP) as st:
      st.init_basis(0)
      st.run_stream(*workloads.supremacy_stream(n, args.depth, seed=0).arrays())
      st.sync()
      bm = (ctypes.c_int32 * n)()
      native.check(st.lib.qh_get_bitmap(st.h, bm))
      inv = {int(p): b for b, p in enumerate(bm)}
      nbytes = (16 if bw == 128 else 8) << n
      nev, nhost = timed(st, st.norm2, reps)
      print(f'bw={bw:3d} qh_norm2 {nev:8.3f} ms (events) {nhost:8.3f} ms (host)  {nbytes / nev / 1e6:7.1f} GB/s  bitmap {[int(p) for p in bm]}',
            flush=True)
      rows.append({'bw': bw, 'case': 'qh_norm2', 'event_ms': round(nev, 4), 'host_ms': round(nhost, 4)})
      for k in (int(v) for v in args.ks.split(',')):
        places = {'low': [inv[p] for p in range(k)], 'top': [inv[p] for p in range(n - k, n)], 'circuit': list(range(n - k, n))}
        for name, bits in places.items():
          pl = st.density_plan(bits)
          ev, host = timed(st, lambda: st.reduced_density(bits), reps)      # pylint: disable=cell-var-from-loop
          mev, _ = timed(st, lambda: st.marginal(bits), reps)               # pylint: disable=cell-var-from-loop
          flop_exec = 8.0 * pl['block_pairs'] * (1 << (2 * pl['tile_bits'])) * (1 << (n - k))
          flop_herm = 4.0 * (1 << k) * (1 << n)
          r = {'bw': bw, 'case': f'k={k} {name}', 'event_ms': round(ev, 4), 'host_ms': round(host, 4), 'x_norm2': round(ev / nev, 3),
               'marginal_ms': round(mev, 4), 'GBps': round(nbytes / ev / 1e6, 1), 'reads': pl['amps_swept'] >> n,
               'TF_exec': round(flop_exec / ev / 1e9, 2), 'TF_herm': round(flop_herm / ev / 1e9, 2),
               'pos': sorted(int(bm[b]) for b in bits), 'wg': pl['block_pairs'] * pl['wg_per_pair'], 'chunk_bits': pl['chunk_bits']}
          rows.append(r)
          extra = '  '.join(f'{key} {v}' for key, v in r.items() if key not in ('bw', 'case', 'event_ms', 'host_ms'))
          print(f'bw={bw:3d} {r["case"]:14s} {ev:8.3f} ms (events) {host:8.3f} ms (host)  {extra}', flush=True)
  print(json.dumps({'nbits': n, 'reps': reps, 'rows': rows}))


if __name__ == '__main__':
  main()
