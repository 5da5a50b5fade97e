"""Times the two-state operations at 30 qubits, complex128 and complex64, with qh_norm2 timed the same way in the same run
as the yardstick (one read of one state):
  * qh_norm2;
  * qh_inner on identical layouts (a state and its clone: two linear streams, twice the bytes of qh_norm2);
  * qh_inner on two different relayout-sweep layouts (supremacy seeds 0 and 1, fused: tiles, b's values through LDS), and
    on a clone whose bit map is re-labelled low4<->top4 and fully reversed (the in-tile shuffle's worst cases);
  * qh_clone (allocation + one device-to-device copy) and qh_copy into an existing handle (the copy alone).
Every call is timed twice: between two HIP events on the stream that does the work (qh_timer_begin / qh_timer_end), and on
the host around the call (what a caller sees: the 16-byte read-back and the wait included).  One warm-up call, then the
median of --reps calls (qh_clone: every call allocates; the previous clone is freed outside the timed window).  GB/s counts the bytes READ.  One JSON line at the end holds every row.

  python tools/bench_inner.py [--nbits 30] [--reps 9] [--depth 20]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from qcc_amd import device, native, workloads  # noqa: E402


def timed(timer_state, fn, reps):
  """(median event ms, median host ms) of fn(), events on timer_state's stream"""
  fn()
  ev, host = [], []
  for _ in range(reps):
    timer_state.timer_begin()
    t0 = time.perf_counter()
    fn()
    host.append((time.perf_counter() - t0) * 1e3)
    ev.append(timer_state.timer_end())
  return statistics.median(ev), statistics.median(host)


def prepared(n, bw, depth, seed):
  st = device.DeviceState(n, bw, fusion=native.QH_FUSE_SWEEP)
  ops, g8 = workloads.supremacy_stream(n, depth, seed=seed).arrays()
  st.init_basis(0)
  st.run_stream(ops, g8)
  st.sync()
  return st


def bitmap(st):
  import ctypes
  bm = (ctypes.c_int32 * st.nbits)()
  native.check(st.lib.qh_get_bitmap(st.h, bm))
  return list(bm)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--nbits', type=int, default=30)
  ap.add_argument('--reps', type=int, default=9)
  ap.add_argument('--depth', type=int, default=20)
  args = ap.parse_args()
  n, reps = args.nbits, args.reps
  rows = []

  def row(bw, case, ev_ms, host_ms, bytes_read, **more):
    r = {'bw': bw, 'case': case, 'event_ms': round(ev_ms, 4), 'host_ms': round(host_ms, 4),
         'gbs': round(bytes_read / (ev_ms * 1e-3) / 1e9, 1), **more}
    rows.append(r)
    extra = '  '.join(f'{k} {v}' for k, v in more.items())
    print(f'bw={bw:3d} {case:28s} {ev_ms:8.3f} ms (events) {host_ms:8.3f} ms (host)  {r["gbs"]:7.1f} GB/s read  {extra}', flush=True)

  for bw in (128, 64):
    state_bytes = (bw // 8) << n
    with prepared(n, bw, args.depth, 0) as a:
      norm_ev, norm_host = timed(a, a.norm2, reps)
      row(bw, 'qh_norm2', norm_ev, norm_host, state_bytes)
      # qh_clone: allocation + copy; the previous clone is released OUTSIDE the timed window
      c = a.clone()
      ev_t, host_t = [], []
      for _ in range(reps):
        c.close()
        a.timer_begin()
        t0 = time.perf_counter()
        c = a.clone()
        host_t.append((time.perf_counter() - t0) * 1e3)
        ev_t.append(a.timer_end())
      row(bw, 'qh_clone', statistics.median(ev_t), statistics.median(host_t), state_bytes)
      ev, host = timed(a, lambda: c.copy_from(a), reps)
      row(bw, 'qh_copy', ev, host, state_bytes)
      assert a.inner_plan(c)['path'] == native.QH_INNER_LINEAR
      lin_ev, lin_host = timed(a, lambda: a.inner(c), reps)
      row(bw, 'qh_inner same layout', lin_ev, lin_host, 2 * state_bytes, vs_2x_norm2=round(lin_ev / (2 * norm_ev), 3))
      lin_self, _ = timed(a, lambda: a.inner(a), reps)
      row(bw, 'qh_inner(a, a)', lin_self, _, 2 * state_bytes, vs_2x_norm2=round(lin_self / (2 * norm_ev), 3))
      # layouts whose in-tile shuffle sends a's low bits to b's high ones (the LDS read's worst case) and whose tile bits are
      # all high in one state: the clone's bit map re-labelled by swaps (qh_remap_swap moves nothing: another state, same cost)
      for name, swaps in (('low4<->top4', [(k, n - 4 + k) for k in range(4)]), ('bit reversal', [(k, n - 1 - k) for k in range(n // 2)])):
        for x, y in swaps:
          c.remap_swap(x, y)
        plan = a.inner_plan(c)
        assert plan['path'] == native.QH_INNER_TILES
        ev, host = timed(a, lambda: a.inner(c), reps)
        row(bw, f'qh_inner {name}', ev, host, 2 * state_bytes, vs_same_layout=round(ev / lin_ev, 3), shuffle=plan['shuffle'],
            tile_a=plan['tile_a'], tile_b=plan['tile_b'])
        for x, y in reversed(swaps):
          c.remap_swap(x, y)
      c.close()
      with prepared(n, bw, args.depth, 1) as b:
        plan = a.inner_plan(b)
        differ = bitmap(a) != bitmap(b)
        if plan['path'] != native.QH_INNER_TILES:
          print(f'bw={bw}: the two circuits left the same layout; no mapped case', flush=True)
          continue
        ev, host = timed(a, lambda: a.inner(b), reps)
        row(bw, 'qh_inner different layouts', ev, host, 2 * state_bytes, vs_same_layout=round(ev / lin_ev, 3),
            vs_2x_norm2=round(ev / (2 * norm_ev), 3), maps_differ=differ, tile_a=plan['tile_a'], tile_b=plan['tile_b'])
  print(json.dumps({'tool': 'bench_inner', 'nbits': n, 'reps': reps, 'depth': args.depth, 'rows': rows}))


if __name__ == '__main__':
  main()
