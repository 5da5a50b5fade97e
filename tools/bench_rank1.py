"""Times qh_apply_rank1 at 30 qubits, complex128 and complex64, beside its yardsticks in the same process: qh_apply_diag on the
same bits (one read and one write of the state behind a table: two streams) and qh_norm2 (one read: one stream).

  * TILE path: k = 1, 3, 6 and 10, table form and uniform form, the register placed by physical position (a fresh handle's bit
    map is the identity): on the line bits (from 0), the lane bits (from 3), the wave bits (from 8), the register-index bits
    (from 10), the top bits, and scattered over the whole index; k = 6 on the lane and top bits also under 1 and 2 controls.
  * TWO_PASS path: k = 11 and 16 in table form, k = 15 and 30 in uniform form.
  * One Grover iteration on 15 and on 30 qubits: oracle + uniform rank-one update, against the gate spelling of the diffusion
    (H layer, X layer, multi-controlled Z through qh_apply_bits, X layer, H layer) queued with fusion on and flushed.  The
    oracle is qh_apply_diag on 15 qubits and one multi-controlled Z on 30 (a table stops at 16 bits).
Expectations written down before measuring (DESIGN.md "Rank-one register updates"): TILE <= 1.25 x qh_apply_diag on the same
bits, TWO_PASS <= 1.25 x (qh_norm2 + qh_apply_diag).  Every row carries its ratio.

Method: one warm-up call, then the median of --reps calls, each timed on the host around call + qh_sync.  One JSON line at the
end holds every row.  --quick: 26 qubits, two repetitions, one case per kernel (for a kernel trace).

  python tools/bench_rank1.py [--nbits 30] [--reps 5] [--widths 128,64] [--quick]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from qcc_amd import device, gates, native  # noqa: E402


def timed(st, fn, reps):
  """median host ms of fn() + sync"""
  fn()
  st.sync()
  ms = []
  for _ in range(reps):
    t0 = time.perf_counter()
    fn()
    st.sync()
    ms.append((time.perf_counter() - t0) * 1e3)
  return statistics.median(ms)


def placements(n, k):
  step = (n - 1) / (k - 1) if k > 1 else 0
  out = [('line', list(range(0, k))), ('lane', list(range(3, 3 + k))), ('wave', list(range(8, 8 + k))),
         ('regidx', list(range(10, 10 + k))), ('top', list(range(n - k, n))),
         ('scattered', sorted({int(round(j * step)) for j in range(k)}) if k > 1 else [n // 2])]
  return [(name, reg) for name, reg in out if len(reg) == k and max(reg) < n]


def vector(k, seed):
  rng = np.random.default_rng(seed)
  v = rng.normal(size=1 << k) + 1j * rng.normal(size=1 << k)
  return v / np.linalg.norm(v)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--nbits', type=int, default=30)
  ap.add_argument('--reps', type=int, default=5)
  ap.add_argument('--widths', default='128,64')
  ap.add_argument('--quick', action='store_true')
  args = ap.parse_args()
  n, reps = (26, 2) if args.quick else (args.nbits, args.reps)
  rows = []

  def row(**r):
    rows.append(r)
    print('  '.join(f'{k} {v}' for k, v in r.items()), flush=True)

  for bw in (int(w) for w in args.widths.split(',')):
    with device.DeviceState(n, bw) as st:
      st.init_basis(1)
      st.sync()
      norm_ms = timed(st, st.norm2, reps)
      row(bw=bw, case='qh_norm2', ms=round(norm_ms, 3))

      def one(case, reg, ctl_bits, uniform):
        k = len(reg)
        ctl = sum(1 << c for c in ctl_bits)
        kd = min(k, 16)
        values = np.exp(2j * np.pi * np.arange(1 << kd) / (1 << kd))
        diag_ms = timed(st, lambda: st.apply_diag(values, reg[:kd]), reps)
        v = None if uniform else vector(k, k)
        plan = st.rank1_plan(reg, ctl, uniform=uniform)
        ms = timed(st, lambda: st.apply_rank1(reg, v=v, ctl_mask=ctl), reps)
        tile = plan['path'] == native.QH_RANK1_TILE
        yard = diag_ms if tile else diag_ms + norm_ms
        row(bw=bw, case=case, k=k, form='uniform' if uniform else 'table', ctl=len(ctl_bits), path='tile' if tile else 'two_pass',
            tile_bits=plan['tile']['tile_bits'], kernels=plan['kernels'], ms=round(ms, 3), diag_ms=round(diag_ms, 3),
            yardstick_ms=round(yard, 3), ratio=round(ms / yard, 3), expectation='ok' if ms <= 1.25 * yard else 'MISS')

      if args.quick:
        one('tile lane', list(range(3, 9)), [], False)
        one('tile top', list(range(n - 10, n)), [n - 11], True)
        one('two_pass top', list(range(n - 11, n)), [], False)
        one('two_pass all', list(range(n)), [], True)
        continue
      for k in (1, 3, 6, 10):
        for name, reg in placements(n, k):
          for uniform in (False, True):
            one(f'tile {name}', reg, [], uniform)
      for name in ('lane', 'top'):
        reg = dict(placements(n, 6))[name]
        free = [b for b in range(n - 1, -1, -1) if b not in reg]
        for nc in (1, 2):
          one(f'tile {name}', reg, free[:nc], False)
      for k, uniform in ((11, False), (16, False), (15, True), (30, True)):
        if k > n:
          continue
        for name, reg in placements(n, k):
          if name in ('line', 'top', 'scattered') and (k < n or name == 'line'):
            one(f'two_pass {name}', reg, [], uniform)
    # one Grover iteration: oracle + diffusion, the rank-one call against the gate spelling
    h_gate, x_gate, z_gate = (np.asarray(g, np.complex128) for g in (gates.hadamard(), gates.pauli_x(), gates.pauli_z()))
    for kq in (15, 30):
      if kq > n or args.quick:
        continue
      reg = list(range(kq))
      allmask = sum(1 << b for b in reg)

      def oracle(st):
        if kq <= 16:
          st.apply_diag(np.where(np.arange(1 << kq) == 12345, -1.0, 1.0), reg)
        else:
          st.apply_bits(allmask & ~1, 0, z_gate)           # flips |1...1>

      def spelled(st):
        for b in reg:
          st.apply_bits(0, b, h_gate)
        for b in reg:
          st.apply_bits(0, b, x_gate)
        st.apply_bits(allmask & ~1, 0, z_gate)
        for b in reg:
          st.apply_bits(0, b, x_gate)
        for b in reg:
          st.apply_bits(0, b, h_gate)
        st.flush()

      with device.DeviceState(n, bw, fusion=native.QH_FUSE_SWEEP) as st:
        st.init_basis(0)
        for b in reg:
          st.apply_bits(0, b, h_gate)
        st.sync()
        gate_ms = timed(st, lambda: (oracle(st), spelled(st)), reps)
      with device.DeviceState(n, bw, fusion=native.QH_FUSE_SWEEP) as st:
        st.init_basis(0)
        for b in reg:
          st.apply_bits(0, b, h_gate)
        st.sync()
        r1_ms = timed(st, lambda: (oracle(st), st.apply_rank1(reg)), reps)
      row(bw=bw, case=f'grover iteration on {kq} of {n} qubits', rank1_ms=round(r1_ms, 3), gates_fused_ms=round(gate_ms, 3),
          speedup=round(gate_ms / r1_ms, 2))
  print(json.dumps({'tool': 'bench_rank1', 'nbits': n, 'reps': reps, 'rows': rows}))


if __name__ == '__main__':
  main()
