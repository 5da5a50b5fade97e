"""Times qh_axpby (dst := alpha dst + beta src) at 30 qubits, complex128 and complex64, with qh_copy and qh_inner timed the
same way in the same run as the yardsticks (two streams each: one read and one write, two reads):
  * qh_axpby on identical layouts (a state and its clone: two linear reads, one linear write -- three streams);
  * the alpha == 0 variant (dst not read: two streams) and the variant that also returns the norm;
  * qh_axpby on the layouts two different supremacy circuits leave (seeds 0 and 1, fused: tiles, src's values through LDS),
    and on a clone whose bit map is re-labelled low4<->top4 and fully reversed (the in-tile shuffle's worst cases).
Every call is timed twice: between two HIP events on the stream that does the work (qh_timer_begin / qh_timer_end), and on
the host around the call (what a caller sees, the wait included).  One warm-up call, then the median of --reps calls.
Coefficients of modulus < 1 keep the repeated in-place updates bounded.  GB/s counts the bytes read AND written.
The bars: 1.5 x the same run's qh_copy on equal layouts (three streams against two) with a margin of 15 %; different layouts
against the equal-layout time of the same run (qh_inner measured 1.00-1.12 x there).  One JSON line at the end holds every row.

  python tools/bench_axpby.py [--nbits 30] [--reps 9] [--depth 20]
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

ALPHA, BETA = 0.6 - 0.3j, 0.2 + 0.25j      # |alpha| + |beta| < 1: the state shrinks, nothing overflows over the repetitions


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

  def row(bw, case, ev_ms, host_ms, bytes_moved, **more):
    r = {'bw': bw, 'case': case, 'event_ms': round(ev_ms, 4), 'host_ms': round(host_ms, 4),
         'gbs': round(bytes_moved / (ev_ms * 1e-3) / 1e9, 1), **more}
    rows.append(r)
    extra = '  '.join(f'{k} {v}' for k, v in more.items())
    print(f'bw={bw:3d} {case:30s} {ev_ms:8.3f} ms (events) {host_ms:8.3f} ms (host)  {r["gbs"]:7.1f} GB/s moved  {extra}', flush=True)

  for bw in (128, 64):
    state_bytes = (bw // 8) << n
    with prepared(n, bw, args.depth, 0) as a, a.clone() as d:      # d: the destination, in a's layout
      copy_ev, copy_host = timed(a, lambda: d.copy_from(a), reps)   # (runs on the source's stream)
      row(bw, 'qh_copy', copy_ev, copy_host, 2 * state_bytes)
      assert d.inner_plan(a)['path'] == native.QH_INNER_LINEAR
      inner_ev, inner_host = timed(d, lambda: d.inner(a), reps)
      row(bw, 'qh_inner same layout', inner_ev, inner_host, 2 * state_bytes)
      lin_ev, lin_host = timed(d, lambda: d.axpby(ALPHA, a, BETA), reps)
      row(bw, 'qh_axpby same layout', lin_ev, lin_host, 3 * state_bytes, vs_copy=round(lin_ev / copy_ev, 3),
          vs_1p5x_copy=round(lin_ev / (1.5 * copy_ev), 3), vs_inner=round(lin_ev / inner_ev, 3))
      ev, host = timed(d, lambda: d.axpby(ALPHA, a, BETA, norm=True), reps)
      row(bw, 'qh_axpby same layout + norm', ev, host, 3 * state_bytes, vs_same_layout=round(ev / lin_ev, 3),
          vs_1p5x_copy=round(ev / (1.5 * copy_ev), 3))
      ev, host = timed(d, lambda: d.axpby(0.0, a, BETA), reps)
      row(bw, 'qh_axpby alpha == 0', ev, host, 2 * state_bytes, vs_copy=round(ev / copy_ev, 3), vs_inner=round(ev / inner_ev, 3))
      d.copy_from(a)
      # the clone's bit map re-labelled by swaps (qh_remap_swap moves nothing: another state, same cost)
      for name, swaps in (('low4<->top4', [(k, n - 4 + k) for k in range(4)]), ('bit reversal', [(k, n - 1 - k) for k in range(n // 2)])):
        for x, y in swaps:
          d.remap_swap(x, y)
        plan = d.inner_plan(a)
        assert plan['path'] == native.QH_INNER_TILES
        ev, host = timed(d, lambda: d.axpby(ALPHA, a, BETA), reps)
        row(bw, f'qh_axpby {name}', ev, host, 3 * state_bytes, vs_same_layout=round(ev / lin_ev, 3),
            vs_1p5x_copy=round(ev / (1.5 * copy_ev), 3), shuffle=plan['shuffle'], tile_a=plan['tile_a'], tile_b=plan['tile_b'])
        for x, y in reversed(swaps):
          d.remap_swap(x, y)
    with prepared(n, bw, args.depth, 0) as d, prepared(n, bw, args.depth, 1) as b:
      plan = d.inner_plan(b)
      if plan['path'] != native.QH_INNER_TILES:
        print(f'bw={bw}: the two circuits left the same layout; no mapped case', flush=True)
        continue
      inner2_ev, _ = timed(d, lambda: d.inner(b), reps)
      for case, fn in (('qh_axpby different layouts', lambda: d.axpby(ALPHA, b, BETA)),
                       ('qh_axpby different + norm', lambda: d.axpby(ALPHA, b, BETA, norm=True))):
        ev, host = timed(d, fn, reps)
        row(bw, case, ev, host, 3 * state_bytes, vs_same_layout=round(ev / lin_ev, 3), vs_1p5x_copy=round(ev / (1.5 * copy_ev), 3),
            vs_inner_different=round(ev / inner2_ev, 3), maps_differ=bitmap(d) != bitmap(b), tile_a=plan['tile_a'], tile_b=plan['tile_b'])
  print(json.dumps({'tool': 'bench_axpby', 'nbits': n, 'reps': reps, 'depth': args.depth, 'rows': rows}))


if __name__ == '__main__':
  main()
