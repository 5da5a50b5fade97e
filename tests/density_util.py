"""TEST-ONLY NumPy references for the reduced density matrices (qh_reduced_density, qc.reduced_density)."""
import numpy as np


def np_reduced_density(psi, bits):
  """(2^k, 2^k) complex128 in the engine's convention: psi in LOGICAL order, rho[r][c] = sum_e a(r,e) conj(a(c,e)) where
  logical bit bits[t] of the amplitude's index is bit t of r.  A @ A^H in complex128."""
  psi = np.asarray(psi, dtype=np.complex128).reshape(-1)
  n, k = psi.size.bit_length() - 1, len(bits)
  if n == 0:
    return (psi * psi.conj()).reshape(1, 1)
  rows = [n - 1 - int(b) for b in reversed(list(bits))]      # (index bit b is axis n-1-b; bits[k-1] is the top row bit)
  rest = [ax for ax in range(n) if ax not in rows]
  a = np.ascontiguousarray(psi.reshape((2,) * n).transpose(rows + rest)).reshape(1 << k, 1 << (n - k))
  return a @ a.conj().T


def logical_order(phys, bitmap):
  """the amplitudes in LOGICAL order, from a download in physical order and the bit map (physical position of every logical
  bit): what tests/test_gpu_expect.py _logical_state computes index by index, as one transpose"""
  phys = np.asarray(phys).reshape(-1)
  n = len(bitmap)
  axes = [0] * n
  for b, p in enumerate(bitmap):
    axes[n - 1 - b] = n - 1 - p
  return np.ascontiguousarray(phys.reshape((2,) * n).transpose(axes)).reshape(-1)


def np_qubit_density(psi, qubits):
  """The same for reference qubit numbers (qubit q is logical bit n-1-q), qubits[0] the most significant bit of an index:
  for ascending qubits, ops.TraceOut(psi.density(), [the others])."""
  n = np.asarray(psi).size.bit_length() - 1
  return np_reduced_density(psi, [n - 1 - q for q in reversed(list(qubits))])


def tolerance(rho, m):
  """(2^k, 2^k) float64: the worst-case bound of a sum of m products in double, whatever the order:
  4 m 2^-53 sqrt(rho_rr rho_cc).  On the diagonal the products are the m probabilities |a|^2 >= 0 that qh_marginal sums too (each
  formed with at most three roundings, added in some order: an error below (m + 2) 2^-53 rho_rr), so the same bound holds the
  marginal to the exact value as well; rho_rr and the marginal, each within it, lie within twice the bound of each other."""
  d = np.sqrt(np.abs(np.real(np.diag(rho))))
  return 4.0 * m * 2.0 ** -53 * np.outer(d, d)


def entropy(rho, base=2):
  ev = np.linalg.eigvalsh(rho / np.trace(rho).real)
  ev = ev[ev > 0]
  return float(-np.sum(ev * np.log(ev)) / np.log(base))
