"""TEST-ONLY helpers shared by the GPU tests that read a state back through the engine's bit map (qh_get_bitmap):
physical <-> logical indices of plain handles and of shard handles (qh_set_shard: the global physical index of local
amplitude i on shard s is (s << nloc) | i), and the exact inverse-CDF check of qh_sample."""
import ctypes

import numpy as np

from qcc_amd import native


def bitmap(st, nbits=None):
  """physical bit of every logical bit of the handle (all nbits_global of them on a shard handle)"""
  n = int(nbits if nbits is not None else getattr(st, 'nbits_global', st.nbits))
  bm = (ctypes.c_int32 * n)()
  native.check(st.lib.qh_get_bitmap(st.h, bm))
  return [int(b) for b in bm]


def logical_of(bm, phys):
  """logical index of every physical index in `phys` (uint64 array) under the bit map bm"""
  phys = np.asarray(phys, dtype=np.uint64)
  out = np.zeros_like(phys)
  for b, p in enumerate(bm):
    out |= ((phys >> np.uint64(p)) & np.uint64(1)) << np.uint64(b)
  return out


def logical_of_phys(bm, size):
  """logical index of every physical index 0..size-1 under the bit map bm (physical bit of each logical bit)"""
  return logical_of(bm, np.arange(size, dtype=np.uint64))


def phys_to_logical(st, shard, local_idx, nglob):
  """global logical index of the local amplitudes local_idx of shard handle st, through ITS bit map as it is now"""
  phys = (np.uint64(shard) << np.uint64(st.nbits)) | np.asarray(local_idx, dtype=np.uint64)
  return logical_of(bitmap(st, nglob), phys)


def check_exact_cdf(pp, g, u):
  """Shots g (PHYSICAL indices into pp) against the inverse CDF of the probabilities pp, taken in physical order, at the
  ascending uniforms u scaled by sum(pp): never a zero amplitude; where a shot differs from NumPy's, the target must sit
  on the boundary of the amplitude it went to (ties at a boundary may go to either side)."""
  cdf = np.cumsum(pp)
  total = cdf[-1]
  x = u * total
  exp_phys = np.minimum(np.searchsorted(cdf, x, side='right'), np.flatnonzero(pp)[-1])
  assert np.all(pp[g] > 0)                                            # never a zero amplitude
  bad = g != exp_phys
  if bad.any():
    lo = np.where(g > 0, cdf[np.maximum(g - 1, 0)], 0.0)
    ok = (lo[bad] - 1e-12 * total <= x[bad]) & (x[bad] < cdf[g[bad]] + 1e-12 * total)
    assert ok.all(), (np.flatnonzero(bad)[:5], g[bad][:5], exp_phys[bad][:5])
