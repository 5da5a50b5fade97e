"""TEST-ONLY: the reference of the Z-polynomial tests and their error bounds.

Model.  f(i) = sum_t w_t (-1)^popcount(i & z_t) by popcount in float64, term by term in the caller's order; the apply is
exp(c f) in complex128 on the amplitudes as stored; the moments are sums of |a_i|^2 (1, f, f^2) in float64.

Tolerances, derived, not measured.  Notation: F = sum |w_t|, T = nterms, amax = max |a_i|, E = exp(|c.re| F).

Apply, per component.  Each of the T - 1 additions of the sum rounds by at most 2^-53 of a partial sum bounded by F, and the
products c.im * f and c.re * f round once more: the angle (and the exponent) carries an absolute error of at most
(T + 2) 2^-53 |c| F, in the kernel and in the model alike (their orders of summation differ), which moves the factor by that
much relative to its modulus <= E.  sincos / exp are good to about an ulp and the complex product is two multiplications and
one fused add per component: a few ulp of amax E.  Both sides together:
  amax * E * ((T + 4) 2^-52 |c| F + 8 * 2^-52)
at complex128; the leading factor 2 (2^-52 for 2^-53) covers the model's own rounding.  complex64 adds one rounding of the
result to float: 2^-23 amax E.

Expectation.  p_i f_i^k is formed with a relative error of about (T + 4) 2^-53 per power of f, |f| <= F; the fixed order adds
at most cpb * 16 <= 2^7 terms serially per thread at the sizes tested (2^26 amplitudes over 4096 blocks of 256 threads: 64),
then trees of 6 + 2 + 12 levels: fewer than 160 additions on any path, each 2^-53 relative to a partial sum <= F^k norm2.
NumPy's pairwise sum and the model's own f are covered by the factor 2:
  (2 T + 160) 2^-52 * F^k * norm2      for the moment k = 1, 2 (k = 0: the same with T = 0)."""
import numpy as np


def parity(idx, z):
  """popcount(idx & z) mod 2 as uint64, for an index array"""
  v = np.asarray(idx, dtype=np.uint64) & np.uint64(z)
  for s in (32, 16, 8, 4, 2, 1):
    v = v ^ (v >> np.uint64(s))
  return v & np.uint64(1)


def np_f(idx, weights, zmasks):
  """f at the indices idx, float64, the terms in the caller's order"""
  idx = np.asarray(idx, dtype=np.uint64)
  f = np.zeros(idx.shape, dtype=np.float64)
  for w, z in zip(weights, zmasks):
    f += np.where(parity(idx, int(z)) == 1, -float(w), float(w))
  return f


def np_apply(psi, weights, zmasks, c, idx=None, f=None):
  """exp(c f) psi in complex128; psi holds the amplitudes at idx (default: every index in order); f: np_f at idx where the
  caller has it already (the program fuzzer evaluates a step's f once)"""
  v = np.asarray(psi).reshape(-1).astype(np.complex128)
  if f is None:
    f = np_f(np.arange(v.size, dtype=np.uint64) if idx is None else idx, weights, zmasks)
  return v * np.exp(complex(c) * f)


def np_moments(psi, weights, zmasks, idx=None, f=None):
  """(sum p, sum p f, sum p f^2) in float64; f as for np_apply"""
  v = np.asarray(psi).reshape(-1).astype(np.complex128)
  p = v.real * v.real + v.imag * v.imag
  if f is None:
    f = np_f(np.arange(v.size, dtype=np.uint64) if idx is None else idx, weights, zmasks)
  return float(np.sum(p)), float(np.dot(p, f)), float(np.dot(p, f * f))


def big_f(weights):
  return float(sum(abs(float(w)) for w in weights))


def apply_bound(width, weights, c, amax):
  """per component, against np_apply"""
  c = complex(c)
  F, T = big_f(weights), len(weights)
  E = float(np.exp(abs(c.real) * F))
  t = amax * E * ((T + 4) * 2.0 ** -52 * abs(c) * F + 8 * 2.0 ** -52)
  if width == 64:
    t += 2.0 ** -23 * amax * E
  return t


def moment_bound(weights, k, norm2):
  """moment k = 0, 1, 2 against np_moments"""
  F, T = big_f(weights), len(weights) if k else 0
  return (2 * T + 160) * 2.0 ** -52 * F ** k * norm2
