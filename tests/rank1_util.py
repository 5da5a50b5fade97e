"""Shared by tests/test_rank1_cpu.py and tests/test_gpu_rank1.py: the NumPy reference of qh_apply_rank1, the derived
tolerance, and a stand-in device for the CPU tests of the qc layer."""
import os

import numpy as np

from tests import fake_device

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'g16_reflections.npz')


def rand_state(rng, n):
  v = rng.normal(size=1 << n) + 1j * rng.normal(size=1 << n)
  return v / np.linalg.norm(v)


def rand_vector(rng, k):
  v = rng.normal(size=1 << k) + 1j * rng.normal(size=1 << k)
  return v / np.linalg.norm(v)


def register_value(n, bits):
  """s(i) for every index i: bit j of s = bit bits[j] of i"""
  idx = np.arange(1 << n, dtype=np.int64)
  s = np.zeros_like(idx)
  for j, b in enumerate(bits):
    s |= ((idx >> b) & 1) << j
  return idx, s


def rank1_parts(psi, n, bits, u, v, a, b, ctl_mask=0):
  """(new state, m per index, controls met per index) in complex128: psi'[s, r] = a psi[s, r] + b u[s] m_r with
  m_r = sum_s conj(v[s]) psi[s, r] on the fibres whose bits under ctl_mask are all 1; u = None: u = v; v = None: both are
  the uniform vector 2^(-k/2)."""
  psi = np.asarray(psi).astype(np.complex128)
  k = len(bits)
  if v is None:
    assert u is None
    v = np.full(1 << k, 2.0 ** (-k / 2.0), dtype=np.complex128)
  v = np.asarray(v, dtype=np.complex128)
  u = v if u is None else np.asarray(u, dtype=np.complex128)
  idx, s = register_value(n, bits)
  reg_mask = sum(1 << b for b in bits)
  fibre = idx & ~reg_mask                                  # the fibre's index with the register at 0
  prod = np.conj(v[s]) * psi
  m = (np.bincount(fibre, weights=prod.real, minlength=1 << n) + 1j * np.bincount(fibre, weights=prod.imag, minlength=1 << n))[fibre]
  met = (idx & ctl_mask) == ctl_mask
  new = np.where(met, complex(a) * psi + complex(b) * u[s] * m, psi)
  return new, m, met


def rank1_reference(psi, n, bits, u, v, a, b, ctl_mask=0):
  return rank1_parts(psi, n, bits, u, v, a, b, ctl_mask)[0]


def sums_tolerance(after, m, met, first, dm):
  """Bounds for the two sums.  sums[0] is formed from the amplitudes as stored, which the test has: only the two summations
  differ, each within (terms) * 2^-53 * sum.  sums[1] adds the error dm of every m_r: 2 |m| dm + dm^2 per fibre."""
  a2 = np.abs(np.asarray(after).astype(np.complex128)[met]) ** 2
  m2 = np.abs(m[met & first])
  t0 = 2 * max(a2.size, 1) * 2.0 ** -53 * float(a2.sum()) + 1e-300
  t1 = float(np.sum(2 * m2 * dm + dm * dm)) + 2 * max(m2.size, 1) * 2.0 ** -53 * float(np.sum(m2 * m2)) + 1e-300
  return t0, t1


def rank1_sums(psi_new_stored, n, bits, m, met):
  """the two sums of qh_apply_rank1: |psi'|^2 as stored over the met amplitudes, |m_r|^2 over the met fibres"""
  reg_mask = sum(1 << b for b in bits)
  idx = np.arange(1 << n, dtype=np.int64)
  first = (idx & reg_mask) == 0
  stored = np.asarray(psi_new_stored).astype(np.complex128)
  return float(np.sum(np.abs(stored[met]) ** 2)), float(np.sum(np.abs(m[met & first]) ** 2))


def tolerance(psi, k, u, v, a, b, bw, new=None):
  """Per component.  B = |a| amax + |b| max|u| (sum |v|) amax bounds every new component; a component carries at most a
  2^k-term inner product in double plus a few products: (2^k + 8) 2^-52 B.  complex64 adds one rounding to float,
  2^-24 (|new| + B), taken at max |new|."""
  psi = np.asarray(psi).astype(np.complex128)
  amax = float(np.max(np.abs(psi)))
  if v is None:
    umax, vsum = 2.0 ** (-k / 2.0), 2.0 ** (k / 2.0)
  else:
    v = np.asarray(v, dtype=np.complex128)
    uu = v if u is None else np.asarray(u, dtype=np.complex128)
    umax, vsum = float(np.max(np.abs(uu))), float(np.sum(np.abs(v)))
  B = abs(complex(a)) * amax + abs(complex(b)) * umax * vsum * amax
  tol = ((1 << k) + 8) * 2.0 ** -52 * B
  if bw == 64:
    nmax = B if new is None else float(np.max(np.abs(new)))
    tol += 2.0 ** -24 * (nmax + B)
  return tol


class Rank1Oracle(fake_device.OracleDevice):
  """OracleDevice with apply_rank1 through the reference (and apply_diag, for the oracles of Grover search); records what it
  is asked."""
  calls_seen = []

  def apply_diag(self, values, bits):
    _, s = register_value(self.nbits, [int(x) for x in bits])
    self.psi[:] = (self.psi * np.asarray(values, dtype=np.complex128)[s]).astype(self.dtype)

  def apply_rank1(self, bits, u=None, v=None, a=-1.0, b=2.0, ctl_mask=0, sums=False):
    bits = [int(x) for x in bits]
    Rank1Oracle.calls_seen.append(dict(bits=bits, u=None if u is None else np.array(u), v=None if v is None else np.array(v),
                                       a=complex(a), b=complex(b), ctl_mask=int(ctl_mask), sums=sums, ngates=len(self.trace)))
    new, m, met = rank1_parts(self.psi, self.nbits, bits, u, v, a, b, ctl_mask)
    self.psi[:] = new.astype(self.dtype)
    return rank1_sums(self.psi, self.nbits, bits, m, met) if sums else None
