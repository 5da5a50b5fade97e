"""Times qh_transition_pauli at 30 qubits, complex128 and complex64, against two baselines timed the same way in the same run
on the same handles:
  * qh_inner(a, b): the bytes one pass moves, through the same walk;
  * the composition a caller had before: qh_pauli_sum_new(b, P) + qh_inner(a, .) + qh_destroy, per string.
Cases, on equal layouts (a state and its clone: the linear walk): one string for each x placement, chosen by PHYSICAL
position in b (x = 0, a line bit, a lane bit, a chunk bit, the top bit, mixed); a full batch on the mixed x mask; 100 strings
on 20 x masks.  On different layouts (the tiles walk): the two relayout-sweep layouts of supremacy seeds 0 and 1, and the
clone with its bit map re-labelled low4<->top4, each with one mixed string and a full batch.
Every call is timed as tools/bench_inner.py times its cases: between two HIP events on a's stream and on the host around the
call (what a caller sees: the read-back and the wait included); one warm-up call, then the median of --reps calls.  `per_pass /
inner` is the host time per pass over the host time of qh_inner on the same pair: the expectation is <= 1.25.  One JSON line at
the end holds every row.

  python tools/bench_transition.py [--nbits 30] [--reps 7] [--depth 20]
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


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--nbits', type=int, default=30)
  ap.add_argument('--reps', type=int, default=7)
  ap.add_argument('--depth', type=int, default=20)
  args = ap.parse_args()
  n, reps = args.nbits, args.reps
  rows = []

  def row(bw, pair, case, ev_ms, host_ms, passes, inner_host, **more):
    r = {'bw': bw, 'pair': pair, 'case': case, 'event_ms': round(ev_ms, 4), 'host_ms': round(host_ms, 4), 'passes': passes, **more}
    if passes and inner_host:
      r['per_pass_over_inner'] = round(host_ms / passes / inner_host, 3)
      r['missed'] = r['per_pass_over_inner'] > 1.25
    rows.append(r)
    extra = '  '.join(f'{k} {v}' for k, v in r.items() if k not in ('bw', 'pair', 'case', 'event_ms', 'host_ms'))
    print(f'bw={bw:3d} {pair:12s} {case:34s} {ev_ms:9.3f} ms (events) {host_ms:9.3f} ms (host)  {extra}', flush=True)

  def phys(st, *bits):
    """the LOGICAL mask whose bits sit at these physical positions of st"""
    return st.phys_to_logical(sum(1 << b for b in bits))

  def cases(bw, pair, a, b, full):
    """the baselines and the transition cases on one pair of handles"""
    batch = native.QH_TRANSITION_BATCH if bw == 128 else native.QH_TRANSITION_BATCH // 2
    ev, inner_host = timed(a, lambda: a.inner(b), reps)
    row(bw, pair, 'qh_inner', ev, inner_host, 0, None, walk=a.inner_plan(b)['path'])
    mixed = phys(b, 1, 4, 9, 17, n - 1)
    zmix = phys(a, 0, 5, 12, n - 2)

    def composed():
      w = b.apply_pauli_sum([1.0], [mixed], [zmix])
      a.inner(w)
      w.close()
    ev, comp_host = timed(a, composed, reps)
    row(bw, pair, 'pauli_sum_new + inner + destroy', ev, comp_host, 0, None, over_inner=round(comp_host / inner_host, 3))

    def one(case, xs, zs):
      npass = len(a.transition_plan(b, xs, zs)[1])
      ev, host = timed(a, lambda: a.transition_pauli(b, xs, zs), reps)
      row(bw, pair, case, ev, host, npass, inner_host, strings=len(xs),
          composition_over_this=round(comp_host * len(xs) / host, 2))

    placements = [('x = 0 (one Z)', 0), ('x on a line bit (1)', phys(b, 1)), ('x on a lane bit (4)', phys(b, 4)),
                  ('x on a chunk bit (13)', phys(b, 13)), (f'x on the top bit ({n - 1})', phys(b, n - 1)), ('x mixed (1, 4, 9, 17, top)', mixed)]
    for name, x in (placements if full else placements[-1:]):
      one(f'one string, {name}', [x], [zmix])
    zs = [phys(a, *[p for p in range(n) if (k * 2654435761 >> p) & 1]) for k in range(1, 101)]
    one(f'full batch ({batch}) on the mixed x', [mixed] * batch, zs[:batch])
    if full:
      xmasks = [phys(b, *[p for p in range(n) if ((k * 40503 + 7) >> (p % 16)) & 1 and p % 3 != k % 3]) for k in range(20)]
      assert len(set(xmasks)) == 20
      one('100 strings on 20 x masks', [xmasks[k % 20] for k in range(100)], zs)

  for bw in (128, 64):
    with prepared(n, bw, args.depth, 0) as a:
      with a.clone() as c:
        assert a.inner_plan(c)['path'] == native.QH_INNER_LINEAR
        cases(bw, 'equal', a, c, True)
        swaps = [(k, n - 4 + k) for k in range(4)]
        for x, y in swaps:
          c.remap_swap(x, y)      # (moves nothing: another state, same cost)
        assert a.inner_plan(c)['path'] == native.QH_INNER_TILES
        cases(bw, 'low4<->top4', a, c, False)
      with prepared(n, bw, args.depth, 1) as b:
        if a.inner_plan(b)['path'] != native.QH_INNER_TILES:
          print(f'bw={bw}: the two circuits left the same layout; no relayout-sweep case', flush=True)
          continue
        cases(bw, 'seeds 0 / 1', a, b, False)
  print(json.dumps({'tool': 'bench_transition', 'nbits': n, 'reps': reps, 'depth': args.depth, 'rows': rows}))


if __name__ == '__main__':
  main()
