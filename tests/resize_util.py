"""TEST-ONLY helpers of the qh_extend / qh_release tests: NumPy models of the two calls (amplitudes by logical index, and
the bit maps bit by bit), and a stand-in device for circuit.qc that HAS extend / release and records what it is asked."""
import numpy as np

from tests import fake_device, shard_util


# ---- amplitudes, by logical index ---------------------------------------------------------------------------------------
def np_extend(psi, f):
  return np.kron(np.asarray(psi), np.asarray(f))


def np_release(psi, bits, value):
  """(slice, kept, dropped): logical bit bits[j] == bit j of value; the remaining bits keep their order"""
  psi = np.asarray(psi).reshape(-1)
  idx = np.arange(psi.size, dtype=np.uint64)
  keep = np.ones(psi.size, dtype=bool)
  for j, b in enumerate(bits):
    keep &= ((idx >> np.uint64(b)) & np.uint64(1)) == np.uint64((value >> j) & 1)
  w = np.abs(psi.astype(np.complex128)) ** 2
  return psi[keep], float(w[keep].sum()), float(w[~keep].sum())


# ---- bit maps, bit by bit ---------------------------------------------------------------------------------------------------
def strike(idx, mask, nbits):
  """the bits of idx (uint64 array) at the positions not in mask, packed in order"""
  idx = np.asarray(idx, dtype=np.uint64)
  out = np.zeros_like(idx)
  at = 0
  for b in range(nbits):
    if not (mask >> b) & 1:
      out |= ((idx >> np.uint64(b)) & np.uint64(1)) << np.uint64(at)
      at += 1
  return out


def deposit(idx, mask, fill, nbits):
  """the inverse: the bits of idx spread over the nbits positions not in mask, the positions in mask taken from fill"""
  idx = np.asarray(idx, dtype=np.uint64)
  out = np.zeros_like(idx)
  at = 0
  for b in range(nbits):
    if (mask >> b) & 1:
      out |= np.uint64(((fill >> b) & 1) << b)
    else:
      out |= ((idx >> np.uint64(at)) & np.uint64(1)) << np.uint64(b)
      at += 1
  return out


def check_extend_map(bm_old, bm_new, nloc, nglob, k):
  """every global physical index of the new handle holds the logical index (L << k) | j of the amplitude f[j] * src[p]
  that new[(j << nloc) | p] puts there (the shard index moved up by k)"""
  assert sorted(bm_new) == list(range(nglob + k))
  phys = np.arange(1 << (nglob + k), dtype=np.uint64)
  low = phys & np.uint64((1 << nloc) - 1)
  j = (phys >> np.uint64(nloc)) & np.uint64((1 << k) - 1)
  old = ((phys >> np.uint64(nloc + k)) << np.uint64(nloc)) | low
  want = (shard_util.logical_of(bm_old, old) << np.uint64(k)) | j
  assert np.array_equal(shard_util.logical_of(bm_new, phys), want)


def check_release_map(bm_old, bm_new, nloc, nglob, bits, value):
  """every global physical index q of the new handle holds the amplitude of the source index that q becomes with the
  released positions put back (at their values): its logical index is the source's with the listed bits struck out"""
  k = len(bits)
  assert sorted(bm_new) == list(range(nglob - k))
  drop = sum(1 << bm_old[b] for b in bits)
  fill = sum(((value >> j) & 1) << bm_old[b] for j, b in enumerate(bits))
  q = np.arange(1 << (nglob - k), dtype=np.uint64)
  old = deposit(q, drop, fill, nglob)
  assert np.array_equal(strike(old, drop, nglob), q)
  want = strike(shard_util.logical_of(bm_old, old), sum(1 << b for b in bits), nglob)
  assert np.array_equal(shard_util.logical_of(bm_new, q), want)


# ---- a stand-in device with extend / release --------------------------------------------------------------------------------
class ResizeOracle(fake_device.OracleDevice):
  """OracleDevice with extend / release in NumPy (logical order = the array's order).  Class-level records: every extend
  / release call, every download, every close."""
  events = []
  downloads = 0

  @classmethod
  def reset(cls):
    cls.events = []
    cls.downloads = 0

  def _sibling(self, nbits, psi):
    other = ResizeOracle(nbits, self.bit_width)
    other.psi[:] = psi.astype(self.dtype)
    return other

  def extend(self, nqubits, amps=None, basis=0):
    ResizeOracle.events.append(('extend', int(nqubits), None if amps is None else np.array(amps), int(basis)))
    if amps is None:
      f = np.zeros(1 << nqubits, dtype=np.complex128)
      f[basis] = 1
    else:
      f = np.asarray(amps, dtype=np.complex128).reshape(-1)
    return self._sibling(self.nbits + nqubits, np_extend(self.psi.astype(np.complex128), f))

  def release(self, bits, value=0):
    ResizeOracle.events.append(('release', [int(b) for b in bits], int(value)))
    small, kept, dropped = np_release(self.psi, list(bits), int(value))
    return self._sibling(self.nbits - len(bits), small), kept, dropped

  def download(self, offset=0, count=None, out=None):
    ResizeOracle.downloads += 1
    return super().download(offset, count, out)

  def close(self):
    ResizeOracle.events.append(('close', self.nbits))
    self.closed = True
