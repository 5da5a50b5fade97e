"""TEST-ONLY: the reference of the Pauli-product tests, their error bound and the greedy run rule restated.

np_pauli_product applies the factors F_t = a_t I + b_t P_t one by one, term 0 first, in complex128 NumPy on the amplitudes as
stored, with pauli_util's formula for P:
  (P v)_i = (-i)^nY (-1)^popcount(i & z) v_{i ^ x},  nY = popcount(x & z)
(test_pauli_product_cpu.py checks it once against np.kron of qcc_amd.lib.ops Paulis)."""
import numpy as np

from tests import pauli_util


def np_pauli_product(psi, a, b, xmasks, zmasks, base=0):
  """prod_t (a_t I + b_t P_t) psi over the indices base .. base + size - 1 that psi holds (x must stay inside them)"""
  v = np.asarray(psi).reshape(-1).astype(np.complex128)
  for at, bt, x, z in zip(a, b, xmasks, zmasks):
    v = complex(at) * v + complex(bt) * pauli_util.np_pauli(v, x, z, base)
  return v


def magnitude(a, b):
  """M = prod_t (|a_t| + |b_t|): how much the factors can grow an amplitude"""
  m = 1.0
  for at, bt in zip(a, b):
    m *= abs(complex(at)) + abs(complex(bt))
  return m


def bound(width, a, b, amax, nruns):
  """Per-component error against np_pauli_product, derived: each term is two complex products and a sum whose rounding is at
  most about 4 * 2^-53 (|a| + |b|) times the running magnitude, which gives (4 nterms + 4) 2^-52 M amax in complex128 (the
  factor 2 covers second-order terms).  complex64 adds one rounding to float per run: nruns * 2^-23 M amax."""
  m = magnitude(a, b)
  t = (4 * len(a) + 4) * 2.0 ** -52 * m * amax
  if width == 64:
    t += nruns * 2.0 ** -23 * m * amax
  return t


def greedy_runs(pxs, batch, amp_bits, kinds):
  """The run rule restated: [(first, count, X, kind)] for physical x masks pxs; kinds = (DIAG, PAIR, HALF)"""
  runs, first, X = [], 0, 0
  for t, px in enumerate(pxs):
    if not (t - first < batch and (px == 0 or X == 0 or px == X)):
      runs.append((first, t - first, X))
      first, X = t, 0
    X = px or X
  if pxs:
    runs.append((first, len(pxs) - first, X))
  return [(f, c, X, kinds[0] if X == 0 else kinds[2] if (amp_bits and X == 1) else kinds[1]) for f, c, X in runs]
