#!/usr/bin/env python3
"""tests/golden/g13_pauli_rot.npz: rotations about Pauli strings computed by the reference (run in the build container
only; same provenance rules as tools/make_golden.py, whose helpers it uses: the reference is RUN, never copied).

The state is a random normalised 8-qubit state held in the reference's own state.State.  Every string is built as the
np.kron product of the reference's ops.Identity / PauliX / PauliY / PauliZ (Operator.__mul__) and applied with the
operator's own call; the record is (cos(t) I - i sin(t) P) psi.  Strings: every single-letter kind (all X, all Y, all Z,
one letter on one qubit), a weight-8 mixed string, a Y-heavy one and a few random ones.  Records: the state, the strings
(one letter per qubit, qubit 0 first), the angles t and the rotated states."""
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
  mg.install_absl_stub(tempfile.mkdtemp(prefix='qcc_golden_pauli_rot_'))
  sys.path.insert(0, mg.REF)
  from absl import flags
  from src.lib import ops, state  # the reference
  flags.FLAGS.tensor_width = 128
  rng = np.random.default_rng(13)
  n = 8
  paulis = {'I': ops.Identity, 'X': ops.PauliX, 'Y': ops.PauliY, 'Z': ops.PauliZ}
  v = rng.normal(size=1 << n) + 1j * rng.normal(size=1 << n)
  psi = state.State(v / np.linalg.norm(v))
  strings = ['X' * n, 'Y' * n, 'Z' * n, 'XIIIIIII', 'IIIYIIII', 'IIIIIIIZ', 'IIXIIIII', 'XYZZYXXY', 'YYYIYYXY', 'YYYYYYYZ']
  strings += [''.join(rng.choice(list('IXYZ'), size=n)) for _ in range(3)]
  thetas = rng.uniform(-3.0, 3.0, size=len(strings))
  rotated = []
  for s, t in zip(strings, thetas):
    op = paulis[s[0]]()
    for ch in s[1:]:
      op = op * paulis[ch]()
    ppsi = np.asarray(op(psi), dtype=np.complex128).reshape(-1)
    rotated.append(np.cos(t) * np.asarray(psi, dtype=np.complex128).reshape(-1) - 1j * np.sin(t) * ppsi)
  path = os.path.join(mg.OUT, 'g13_pauli_rot.npz')
  np.savez_compressed(path, nbits=np.array(n), psi=np.asarray(psi, dtype=np.complex128).reshape(-1), strings=np.array(strings),
                      thetas=np.asarray(thetas, dtype=np.float64), rotated=np.array(rotated, dtype=np.complex128))
  print('wrote', path, len(strings), 'records', os.path.getsize(path), 'bytes')


if __name__ == '__main__':
  main()
