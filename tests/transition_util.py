"""TEST-ONLY helpers shared by the CPU and GPU tests of qh_transition_pauli / qc.matrix_element / qc.rotation_gradients:
the NumPy reference on amplitudes in logical order, Pauli strings as masks and as np.kron products, and the
parameter-shift rule."""
import functools

import numpy as np

from qcc_amd.lib import ops


def np_pauli(b, x, z):
  """P b for the string (x, z) over LOGICAL bits: (P b)_i = (-i)^nY (-1)^popcount(i & z) b_{i ^ x}, complex128"""
  b = np.asarray(b, dtype=np.complex128).reshape(-1)
  idx = np.arange(b.size, dtype=np.uint64)
  par = np.zeros(b.size, dtype=np.uint64)
  for bit in range(64):
    if (int(z) >> bit) & 1:
      par ^= (idx >> np.uint64(bit)) & np.uint64(1)
  return (-1j) ** (bin(int(x) & int(z)).count('1') % 4) * (1.0 - 2.0 * par.astype(np.float64)) * b[idx ^ np.uint64(x)]


def np_transition(a, b, x, z):
  """<a|P|b> = (-i)^nY sum_i (-1)^popcount(i & z) conj(a_i) b_{i ^ x} of two states in logical order"""
  a = np.asarray(a, dtype=np.complex128).reshape(-1)
  return complex(np.sum(np.conj(a) * np_pauli(b, x, z)))


def masks_of(s):
  """(x, z) of a string over IXYZ, letter q on qubit q (qubit 0 is the most significant logical bit, as in qc)"""
  n = len(s)
  x = sum(1 << (n - 1 - q) for q, p in enumerate(s) if p in 'XY')
  z = sum(1 << (n - 1 - q) for q, p in enumerate(s) if p in 'ZY')
  return x, z


def kron_pauli(s):
  """the np.kron product of qcc_amd.lib.ops Paulis, letter q of s on qubit q"""
  mats = {'I': np.eye(2), 'X': np.asarray(ops.PauliX()), 'Y': np.asarray(ops.PauliY()), 'Z': np.asarray(ops.PauliZ())}
  return functools.reduce(np.kron, [mats[c] for c in s])


def parameter_shift(energy_of, thetas):
  """[E(theta_k + pi/2) - E(theta_k - pi/2)] / 2 for every k: exact for rotations exp(-i theta/2 P).  energy_of(thetas)
  builds a fresh circuit and returns <H>."""
  grad = np.zeros(len(thetas), dtype=np.float64)
  for k in range(len(thetas)):
    up, dn = list(thetas), list(thetas)
    up[k] += np.pi / 2
    dn[k] -= np.pi / 2
    grad[k] = (energy_of(up) - energy_of(dn)) / 2
  return grad
