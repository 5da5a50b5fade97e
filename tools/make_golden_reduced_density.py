#!/usr/bin/env python3
"""tests/golden/g14_reduced_density.npz: reduced density matrices computed by the reference (run in the build container
only; same provenance rules as tools/make_golden.py, whose helpers it uses: the reference is RUN, never copied).

The state is a random normalised 8-qubit state held in the reference's own state.State.  For every kept subset the record
is ops.TraceOut(psi.density(), [every other qubit]) -- the reference's own 4^n route.  Subsets: every single qubit,
adjacent and scattered pairs, three subsets of 3-4 qubits and one of 6.  Records: the state, the subsets (a flat list and
offsets), and the matrices, flattened one after the other."""
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402


def main():
  xg = mg.load_ref_xgates()
  sys.modules['libxgates'] = xg
  mg.install_absl_stub(tempfile.mkdtemp(prefix='qcc_golden_reduced_density_'))
  sys.path.insert(0, mg.REF)
  from absl import flags
  from src.lib import ops, state  # the reference
  flags.FLAGS.tensor_width = 128
  rng = np.random.default_rng(14)
  n = 8
  v = rng.normal(size=1 << n) + 1j * rng.normal(size=1 << n)
  psi = state.State(v / np.linalg.norm(v))
  subsets = [[q] for q in range(n)]
  subsets += [[0, 1], [3, 4], [6, 7], [0, 7], [2, 5], [1, 6]]
  subsets += [[0, 1, 2], [1, 4, 6], [2, 3, 5, 7], [0, 1, 3, 4, 6, 7]]
  rho = psi.density()
  flat, offsets, mats = [], [0], []
  for keep in subsets:
    red = ops.TraceOut(rho, [q for q in range(n) if q not in keep])
    red = np.asarray(red, dtype=np.complex128)
    assert red.shape == (1 << len(keep), 1 << len(keep))
    flat += keep
    offsets.append(len(flat))
    mats.append(red.reshape(-1))
  path = os.path.join(mg.OUT, 'g14_reduced_density.npz')
  np.savez_compressed(path, nbits=np.array(n), psi=np.asarray(psi, dtype=np.complex128).reshape(-1),
                      qubits=np.asarray(flat, dtype=np.int32), offsets=np.asarray(offsets, dtype=np.int32),
                      rho=np.concatenate(mats).astype(np.complex128))
  print('wrote', path, len(subsets), 'records', os.path.getsize(path), 'bytes')


if __name__ == '__main__':
  main()
