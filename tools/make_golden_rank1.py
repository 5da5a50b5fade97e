#!/usr/bin/env python3
"""tests/golden/g16_reflections.npz: reflections built by the reference as dense matrices and applied to seeded random states
(run in the build container only; same provenance rules as tools/make_golden.py, whose helpers it uses: the reference is RUN,
never copied).

(a) n = 3, 5, 8: the reference's inversion about the mean, built as its grover.py builds it -- reflection =
    ZeroProjector(n) * 2.0 - Identity(n), hn = Hadamard(n), inversion = hn(reflection(hn)) -- applied to random states:
    a{n}_in, a{n}_out, each (states, 2^n) complex128.
(b) n = 3, 6: algo.adjoint()(reflection(algo)) with the "somewhat random" algorithm of its amplitude_estimation.py (a Hadamard
    layer times one RotationY(random() / 2) per qubit, `random` seeded), the unit vector phi for which that matrix is
    2 phi phi^dagger - I (asserted here to 1e-12), and states before and after: b{n}_phi (2^n), b{n}_in, b{n}_out.
Only these arrays are stored; the largest is 256 complex numbers."""
import os
import random
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402


def _states(rng, n):
  count = max(1, min(4, 256 >> n))
  v = rng.normal(size=(count, 1 << n)) + 1j * rng.normal(size=(count, 1 << n))
  return v / np.linalg.norm(v, axis=1, keepdims=True)


def main():
  xg = mg.load_ref_xgates()
  sys.modules['libxgates'] = xg
  mg.install_absl_stub(tempfile.mkdtemp(prefix='qcc_golden_rank1_'))
  sys.path.insert(0, mg.REF)
  from absl import flags
  from src.lib import ops, state  # the reference
  flags.FLAGS.tensor_width = 128   # (the reference's default is complex64)
  out = {}
  for n in (3, 5, 8):
    rng = np.random.default_rng(1600 + n)
    reflection = ops.ZeroProjector(n) * 2.0 - ops.Identity(n)
    hn = ops.Hadamard(n)
    inversion = hn(reflection(hn))
    psi = _states(rng, n)
    res = np.stack([np.asarray(inversion(state.State(p)), dtype=np.complex128).reshape(-1) for p in psi])
    out[f'a{n}_in'], out[f'a{n}_out'] = psi, res
  for n in (3, 6):
    random.seed(1600 + n)
    rng = np.random.default_rng(1650 + n)
    i1 = ops.Identity(1)
    algo = ops.Hadamard(n)
    for q in range(n):
      layer = ops.RotationY(random.random() / 2) if q == 0 else i1
      for j in range(1, n):
        layer = layer * (ops.RotationY(random.random() / 2) if j == q else i1)
      algo = algo @ layer
    reflection = ops.ZeroProjector(n) * 2.0 - ops.Identity(n)
    inversion = algo.adjoint()(reflection(algo))
    mat = np.asarray(inversion, dtype=np.complex128)
    phi = np.conj(np.asarray(algo, dtype=np.complex128)[0, :])       # algo^dagger |0>
    assert abs(np.linalg.norm(phi) - 1) < 1e-12
    assert np.max(np.abs(mat - (2 * np.outer(phi, np.conj(phi)) - np.eye(1 << n)))) < 1e-12
    psi = _states(rng, n)
    res = np.stack([np.asarray(inversion(state.State(p)), dtype=np.complex128).reshape(-1) for p in psi])
    out[f'b{n}_phi'], out[f'b{n}_in'], out[f'b{n}_out'] = phi.astype(np.complex128), psi, res
  path = os.path.join(mg.OUT, 'g16_reflections.npz')
  np.savez_compressed(path, **out)
  print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
  main()
