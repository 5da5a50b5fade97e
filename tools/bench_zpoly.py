"""Times qh_apply_zpoly (a_i *= exp(c f(i)), one kernel for any number of terms) and qh_expect_zpoly on a 30-qubit state left
permuted by a fused QFT flush, in complex128 and complex64, with their yardsticks timed in the same run, ALTERNATING with
them inside every repeat:
  * the same factors exp(-i gamma w_t Z..Z) through qh_apply_pauli_product, the path there was before: ceil(T / 8) runs;
  * qh_apply_diag with k = 1 on the same handle: one in-place read + write of the state;
  * qh_norm2 (one read) and qh_expect_pauli on the same masks (ceil(T / 16) reads) for the moments.
Term lists, all ZZ cost functions on 30 nodes (node q on logical bit n - 1 - q):
  (a) ring                       30 terms
  (b) random 3-regular, seeded   45 terms
  (c) complete graph + fields   465 terms
Every call is followed by qh_sync and timed on the host; a row gives the median of --reps calls after one warm-up, and the
spread (min .. max).  `groups` and the class counts are what qh_zpoly_plan reports on the layout the flush left.  One JSON
line at the end holds every row.

  python tools/bench_zpoly.py [--nbits 30] [--reps 7] [--quick]
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
from qcc_amd import device, native, workloads  # noqa: E402


def regular3(n, rng):
  """a simple 3-regular graph on n nodes by the pairing model (retry until no loop and no double edge)"""
  while True:
    stubs = rng.permutation(np.repeat(np.arange(n), 3))
    edges = {(int(min(a, b)), int(max(a, b))) for a, b in stubs.reshape(-1, 2)}
    if len(edges) == 3 * n // 2 and all(a != b for a, b in edges):
      return sorted(edges)


def term_lists(n, rng):
  bit = lambda q: 1 << (n - 1 - q)      # noqa: E731
  ring = [(bit(q) | bit((q + 1) % n), 1.0) for q in range(n)]
  reg = [(bit(a) | bit(b), float(w)) for (a, b), w in zip(regular3(n, rng), rng.uniform(0.5, 1.5, size=3 * n // 2))]
  full = [(bit(a) | bit(b), float(rng.uniform(-1, 1))) for a in range(n) for b in range(a + 1, n)] + [(bit(q), float(rng.uniform(-1, 1))) for q in range(n)]
  return [('(a) ring', ring), ('(b) 3-regular', reg), ('(c) complete + fields', full)]


def alternate(fns, reps):
  """each function once to warm up, then reps rounds of all of them in turn; (median, min, max) ms per function"""
  for fn in fns:
    fn()
  times = [[] for _ in fns]
  for _ in range(reps):
    for k, fn in enumerate(fns):
      t0 = time.perf_counter()
      fn()
      times[k].append((time.perf_counter() - t0) * 1e3)
  return [(statistics.median(t), min(t), max(t)) for t in times]


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--nbits', type=int, default=30)
  ap.add_argument('--reps', type=int, default=7)
  ap.add_argument('--quick', action='store_true', help='one timed call per case (kernel-name check under a profiler)')
  args = ap.parse_args()
  n, reps = args.nbits, 1 if args.quick else args.reps
  rows = []
  ops, g8 = workloads.qft_stream(range(n)).arrays()
  for bw in (128, 64):
    state_bytes = (bw // 8) << n
    with device.DeviceState(n, bw, fusion=native.QH_FUSE_SWEEP) as st:
      st.init_basis(0x2345678 & ((1 << n) - 1))
      st.run_stream(ops, g8)
      st.flush()
      bm = (ctypes.c_int32 * n)()
      native.check(st.lib.qh_get_bitmap(st.h, bm))
      print(f'bw={bw}: bit map after the flush {list(bm)}', flush=True)
      rng = np.random.default_rng(30)
      phase = np.exp(1j * 0.3)

      def synced(fn):
        def run():
          fn()
          st.sync()
        return run
      diag = synced(lambda: st.apply_diag([np.conj(phase), phase], [n // 2]))
      for name, terms in term_lists(n, rng):
        zs, ws = [z for z, _ in terms], [w for _, w in terms]
        T = len(zs)
        gamma = 0.4 / max(abs(w) for w in ws)
        p = st.zpoly_plan(ws, zs)
        _, runs = st.pauli_product_plan([0] * T, zs)
        a, b = [math.cos(gamma * w) for w in ws], [-1j * math.sin(gamma * w) for w in ws]
        k0 = st.stats()
        st.apply_zpoly(ws, zs, -1j * gamma)
        k1 = st.stats()
        assert k1['kernels_launched'] - k0['kernels_launched'] == 1 and k1['bytes_swept'] - k0['bytes_swept'] == 2 * state_bytes
        fns = [synced(lambda: st.apply_zpoly(ws, zs, -1j * gamma)), lambda: st.apply_zpoly(ws, zs, -1j * gamma, norm=True),
               synced(lambda: st.apply_zpoly(ws, zs, -0.01 - 1j * gamma)), synced(lambda: st.apply_pauli_product(a, b, [0] * T, zs)), diag,
               lambda: st.expect_zpoly(ws, zs), st.norm2, lambda: st.expect_pauli([0] * T, zs)]
        (zp, zpn, zpc, prod, dg, ez, nrm, ep) = alternate(fns, reps)
        st.scale(1.0 / math.sqrt(st.norm2()))      # (the complex c is not unitary)
        row = {'bw': bw, 'case': name, 'terms': T, 'groups': p['ngroups'], 'classes': [p['nconst'], p['nhigh'], p['nlow'], p['nstraddle']],
               'apply_zpoly_ms': [round(v, 4) for v in zp], 'apply_zpoly_norm2_ms': [round(v, 4) for v in zpn],
               'apply_zpoly_complex_c_ms': [round(v, 4) for v in zpc], 'product_runs': len(runs), 'apply_pauli_product_ms': [round(v, 4) for v in prod],
               'apply_diag_k1_ms': [round(v, 4) for v in dg], 'expect_zpoly_ms': [round(v, 4) for v in ez], 'norm2_ms': [round(v, 4) for v in nrm],
               'expect_pauli_reads': -(-T // 16), 'expect_pauli_ms': [round(v, 4) for v in ep],
               'zpoly_vs_product': round(zp[0] / prod[0], 4), 'zpoly_vs_diag': round(zp[0] / dg[0], 3), 'expect_vs_norm2': round(ez[0] / nrm[0], 3),
               'expect_vs_expect_pauli': round(ez[0] / ep[0], 4), 'tbs': round(2 * state_bytes / (zp[0] * 1e-3) / 1e12, 3)}
        rows.append(row)
        fmt = lambda t: f'{t[0]:8.3f} ms ({t[1]:.3f} .. {t[2]:.3f})'      # noqa: E731
        print(f'bw={bw:3d} {name:22s} {T:4d} terms, {p["ngroups"]:3d} groups, classes const/high/low/straddle {row["classes"]}\n'
              f'    qh_apply_zpoly            {fmt(zp)}  {row["tbs"]:5.2f} TB/s   with norm2 {fmt(zpn)}   complex c {fmt(zpc)}\n'
              f'    qh_apply_pauli_product    {fmt(prod)}  {len(runs):3d} runs      zpoly / product = {row["zpoly_vs_product"]:.4f}\n'
              f'    qh_apply_diag k=1         {fmt(dg)}                zpoly / diag = {row["zpoly_vs_diag"]:.3f}\n'
              f'    qh_expect_zpoly           {fmt(ez)}   qh_norm2 {fmt(nrm)}  (x{row["expect_vs_norm2"]:.3f})   qh_expect_pauli {fmt(ep)}, '
              f'{row["expect_pauli_reads"]} reads  (x{row["expect_vs_expect_pauli"]:.4f})', flush=True)
  print(json.dumps({'tool': 'bench_zpoly', 'nbits': n, 'reps': reps, 'lib': os.path.basename(native.LIB_PATH), 'cases': rows}))


if __name__ == '__main__':
  main()
