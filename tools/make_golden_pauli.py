#!/usr/bin/env python3
"""tests/golden/g12_pauli_expect.npz: Pauli-string expectation values computed by the reference (run in the build
container only; same provenance rules as tools/make_golden.py, whose helpers it uses: the reference is RUN, never
copied).

States come from the reference's own circuits (random ry / rz / cx / h layers through its qc class, n = 2 .. 10); every
string is built as the np.kron product of the reference's ops.Identity / PauliX / PauliY / PauliZ (Operator.__mul__),
applied to the state with the operator's own call, and the value is np.dot(psi.adjoint(), P(psi)) as the reference's
vqe_simple does.  Records: the state, the string (one letter per qubit, qubit 0 first) and the complex value (its
imaginary part is rounding)."""
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
  mg.install_absl_stub(tempfile.mkdtemp(prefix='qcc_golden_pauli_'))
  sys.path.insert(0, mg.REF)
  from absl import flags
  from src.lib import circuit, ops  # the reference
  flags.FLAGS.tensor_width = 128
  rng = np.random.default_rng(12)
  paulis = {'I': ops.Identity, 'X': ops.PauliX, 'Y': ops.PauliY, 'Z': ops.PauliZ}
  out = {}
  strings, values, which = [], [], []
  sizes = (2, 3, 4, 5, 6, 7, 8, 9, 10)
  for k, n in enumerate(sizes):
    qc = circuit.qc(f'pauli{n}')
    qc.reg(n, 0)
    for _ in range(3):
      for q in range(n):
        qc.ry(q, float(rng.random() * 3))
        qc.rz(q, float(rng.random() * 3))
      for q in range(n - 1):
        qc.cx(q, q + 1)
      qc.h(int(rng.integers(n)))
    psi = qc.psi
    out[f'psi{k}'] = np.asarray(psi, dtype=np.complex128).copy()
    todo = ['I' * n, 'Z' * n, 'X' * n, 'Y' * n] + [''.join(rng.choice(list('IXYZ'), size=n)) for _ in range(4)]
    for s in todo:
      op = paulis[s[0]]()
      for ch in s[1:]:
        op = op * paulis[ch]()
      strings.append(s.ljust(max(sizes), '-'))
      values.append(complex(np.dot(psi.adjoint(), op(psi))))
      which.append(k)
  path = os.path.join(mg.OUT, 'g12_pauli_expect.npz')
  np.savez_compressed(path, nbits=np.array(sizes), state=np.array(which), strings=np.array(strings),
                      values=np.array(values, dtype=np.complex128), **out)
  print('wrote', path, len(values), 'records', os.path.getsize(path), 'bytes')


if __name__ == '__main__':
  main()
