"""TEST-ONLY: the reference of the Pauli-sum tests and their error bound.

np_pauli_sum is NumPy in complex128 on the amplitudes as stored:
  (P a)_i = (-i)^nY (-1)^popcount(i & z) a_{i ^ x},  nY = popcount(x & z),  out_i = sum_t c_t (P_t a)_i
(test_pauli_sum_cpu.py checks it once against np.kron of qcc_amd.lib.ops Paulis)."""
import numpy as np


def parity(idx, mask):
  par = np.zeros(idx.size, dtype=np.uint64)
  for b in range(64):
    if (int(mask) >> b) & 1:
      par ^= (idx >> np.uint64(b)) & np.uint64(1)
  return par


def np_pauli(psi, x, z, base=0, at=None):
  """(P a) over the indices base .. base + size - 1 that psi holds (x must stay inside them), or at the indices `at` of
  them only: signs, swaps and negations only -- exact"""
  a = np.asarray(psi).reshape(-1)
  idx = np.uint64(base) + (np.arange(a.size, dtype=np.uint64) if at is None else np.asarray(at, dtype=np.uint64))
  v = a[((idx ^ np.uint64(x)) - np.uint64(base)).astype(np.int64)].astype(np.complex128)
  v = np.where(parity(idx, z) == 1, -v, v)
  for _ in range(bin(int(x) & int(z)).count('1') % 4):      # times -i: (re, im) -> (im, -re)
    v = v.imag - 1j * v.real
  return v


def np_pauli_sum(psi, coeffs, xmasks, zmasks, base=0, at=None):
  a = np.asarray(psi).reshape(-1)
  out = np.zeros(a.size if at is None else len(at), dtype=np.complex128)
  for c, x, z in zip(coeffs, xmasks, zmasks):
    out += complex(c) * np_pauli(a, x, z, base, at)
  return out


def bound(width, coeffs, amax, nbatches=None):
  """Per-component error of dst against np_pauli_sum, derived: with C = sum |c_t|, each of the nterms products and sums of a
  component rounds once in double, relative to a partial sum of at most C * amax, plus the complex product of a group and
  the rounding of the stored value: (nterms + 4) * 2^-52 * C * amax.  complex64 adds one rounding to float per batch."""
  n = len(coeffs)
  c = float(sum(abs(complex(v)) for v in coeffs))
  nbatches = max(1, -(-n // 16)) if nbatches is None else nbatches
  b = (n + 4) * 2.0 ** -52 * c * amax
  if width == 64:
    b += nbatches * 2.0 ** -23 * c * amax
  return b
