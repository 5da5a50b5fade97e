"""TEST-ONLY helpers of the sparse-readout tests: NumPy references for select / topk, the probability as the engine computes
it, and stand-in devices that implement select / topk / amplitudes (single process and per shard)."""
from fractions import Fraction

import numpy as np

from tests.fake_device import MeasureOracle, MeasureShardEngine


def fma_prob(a):
  """fma(im, im, re * re) of one complex amplitude, rounded as the hardware rounds it (exact rational arithmetic)."""
  re, im = float(a.real), float(a.imag)
  return float(Fraction(im) * Fraction(im) + Fraction(re * re))


def fma_probs(amps):
  """The engine's probabilities of complex128 amplitudes.  Short lists one by one in rational arithmetic; long ones through
  the vectorised qcc_amd.sharded.fma_probs, spot-checked here against the rational form on 2048 entries."""
  a = np.asarray(amps, dtype=np.complex128).reshape(-1)
  if a.size <= 4096:
    return np.array([fma_prob(x) for x in a], dtype=np.float64)
  from qcc_amd.sharded import fma_probs as fast
  p = fast(a)
  probe = np.random.default_rng(a.size).integers(0, a.size, size=2048)
  assert p[probe].tolist() == [fma_prob(x) for x in a[probe]]
  return p


def np_select(psi, threshold, base=0, probs=None):
  """(idx, amp, weight) of the entries with probability >= threshold, ascending; psi holds indices base ..."""
  a = np.asarray(psi, dtype=np.complex128).reshape(-1)
  p = fma_probs(a) if probs is None else probs
  hit = np.flatnonzero(p >= threshold)
  return (np.uint64(base) + hit.astype(np.uint64)), a[hit], float(p[hit].sum())


def np_topk(psi, k, base=0, probs=None):
  """(idx, amp): the k most probable nonzero entries, ties by ascending index"""
  a = np.asarray(psi, dtype=np.complex128).reshape(-1)
  p = fma_probs(a) if probs is None else probs
  order = np.lexsort((np.arange(p.size), -p))
  order = order[p[order] > 0][:k]
  return (np.uint64(base) + order.astype(np.uint64)), a[order]


class SelectOracle(MeasureOracle):
  """MeasureOracle with the sparse readers, in NumPy (logical order = the array's order); counts downloads."""
  downloads = 0

  def download(self, offset=0, count=None, out=None):
    SelectOracle.downloads += 1
    return super().download(offset, count, out)

  def select(self, threshold, cap=1 << 16):
    idx, amp, w = np_select(self.psi, threshold)
    if idx.size > cap:
      return np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=np.complex128), int(idx.size), w
    return idx, amp, int(idx.size), w

  def topk(self, k):
    return np_topk(self.psi, k)

  def amplitudes(self, indices):
    return np.asarray(self.psi, dtype=np.complex128)[np.asarray(indices, dtype=np.uint64).astype(np.int64)]


class SelectShardEngine(MeasureShardEngine):
  """MeasureShardEngine with the sparse readers as qh_select / qh_topk / qh_amplitudes answer on a shard handle: global
  indices, ties by the ENGINE's index order, exact zeros for what another shard holds."""

  def select(self, threshold, cap=1 << 16):
    idx, amp, w = np_select(self.psi, threshold, self.shard << self.nbits)
    if idx.size > cap:
      return np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=np.complex128), int(idx.size), w
    return idx, amp, int(idx.size), w

  def topk(self, k):
    return np_topk(self.psi, k, self.shard << self.nbits)

  def amplitudes(self, indices):
    idx = np.asarray(indices, dtype=np.uint64)
    mine = (idx >> np.uint64(self.nbits)) == np.uint64(self.shard)
    out = np.zeros(idx.size, dtype=np.complex128)
    out[mine] = self.psi[(idx[mine] & np.uint64((1 << self.nbits) - 1)).astype(np.int64)]
    return out


def sharded_select_worker(rank, n, out_dir, device_factory):
  """One rank of the sharded sparse-readout test, inside an initialised process group: ShardedDevice.select / topk /
  amplitudes on three states -- a random circuit's, one with exact ties that straddle the ranks, and a flat one -- after
  gates that exchange shard bits (so the router's bit map is not the identity).  Results go to out_dir/s<rank>.npz."""
  import os
  from qcc_amd.lib import backend, tensor
  from tests.fake_device import readout_circuit
  tensor.set_tensor_width(128)
  backend.set_device_factory(device_factory)
  res = {}
  q = readout_circuit(n, 5)
  q.h(0)
  q.cx(0, n - 1)
  psi = np.asarray(q.psi).copy()
  dev = q._ensure_device()                                # pylint: disable=protected-access
  res['perm'] = np.array(dev.st.perm)
  res['psi'] = psi
  p = np.sort(np.abs(psi) ** 2)
  for name, thr in (('all', 0.0), ('med', float(p[p.size // 2])), ('hi', float(p[-5])), ('none', 2.0)):
    idx, amp, cnt, w = dev.select(thr, 1 << 16)
    res['sel_idx_' + name], res['sel_amp_' + name], res['sel_cw_' + name] = idx, amp, np.array([cnt, w, thr])
  idx, amp, cnt, w = dev.select(0.0, 3)                   # more than cap: empty arrays, count and weight hold
  res['sel_over'] = np.array([idx.size, amp.size, cnt, w])
  for k in (1, 5, 1 << n, (1 << n) + 9):
    res[f'top_idx_{k}'], res[f'top_amp_{k}'] = dev.topk(k)
  want = np.array([0, (1 << n) - 1, 5, 5, 1 << (n - 1), 3], dtype=np.uint64)
  res['amp_idx'], res['amps'] = want, dev.amplitudes(want)
  res['amps_empty'] = dev.amplitudes([])
  res['support'] = np.array([[helper_val(b), a.real, a.imag, pr] for b, a, pr in q.support(float(p[-5]))])
  res['top3'] = np.array([[helper_val(b), a.real, a.imag, pr] for b, a, pr in q.top(3)])
  # ties that straddle ranks: four values, every one repeated over the whole index range, in a layout the exchanges above
  # have permuted (upload resets the map: run a few gates again so that the shard bits move)
  vals = np.array([0.5, 0.5j, -0.25, 0.125 + 0.125j])
  tie = vals[(np.arange(1 << n) * 7 // 3) % 4]
  tie = tie / np.linalg.norm(tie)
  q2 = readout_circuit(n, 6)
  q2.psi = tie
  q2.x(0)                                                 # (permutations of the amplitudes: the ties stay exact)
  q2.cx(0, 1)
  q2.cx(0, 1)
  q2.x(0)
  dev2 = q2._ensure_device()                              # pylint: disable=protected-access
  res['tie_psi'] = np.asarray(q2.psi).copy()
  res['tie_perm'] = np.array(dev2.st.perm)
  for k in (1, 3, 9, (1 << n) // 4 + 3):
    res[f'tie_idx_{k}'], res[f'tie_amp_{k}'] = dev2.topk(k)
  type(dev2).TIE_SELECT_CAP = 4                           # more ties than that: the prefix path
  for k in (3, 9):
    res[f'tiescan_idx_{k}'], res[f'tiescan_amp_{k}'] = dev2.topk(k)
  np.savez(os.path.join(out_dir, f's{rank}.npz'), **res)


def helper_val(bits):
  v = 0
  for b in bits:
    v = 2 * v + int(b)
  return v


def check_sharded_select(out_dir, world, n):
  """What the ranks of sharded_select_worker saw against the single-process NumPy answer."""
  import os
  res = [dict(np.load(os.path.join(out_dir, f's{r}.npz'))) for r in range(world)]
  for r in res[1:]:
    for k, v in res[0].items():
      assert np.array_equal(v, r[k]), k                    # every rank returns the same
  r0 = res[0]
  psi = r0['psi']
  assert r0['perm'].tolist() != list(range(n))             # the router's map moved: engine order != logical order
  for name in ('all', 'med', 'hi', 'none'):
    cnt, w, thr = r0['sel_cw_' + name]
    idx, amp, ww = np_select(psi, thr)
    assert int(cnt) == idx.size and abs(w - ww) < 1e-13
    assert np.array_equal(r0['sel_idx_' + name], idx) and np.array_equal(r0['sel_amp_' + name], amp), name
  assert r0['sel_cw_all'][0] == 1 << n and r0['sel_cw_none'][0] == 0 and 0 < r0['sel_cw_hi'][0] <= 5
  assert r0['sel_over'][:3].tolist() == [0, 0, 1 << n] and abs(r0['sel_over'][3] - 1) < 1e-13
  nz = int(np.count_nonzero(fma_probs(psi)))
  for k in (1, 5, 1 << n, (1 << n) + 9):
    idx, amp = np_topk(psi, k)
    assert idx.size == min(k, nz)
    assert np.array_equal(r0[f'top_idx_{k}'], idx) and np.array_equal(r0[f'top_amp_{k}'], amp), k
  assert np.array_equal(r0['amps'], psi[r0['amp_idx'].astype(np.int64)])
  assert r0['amps_empty'].size == 0
  thr = float(np.sort(np.abs(psi) ** 2)[-5])
  idx, amp, _ = np_select(psi, thr)
  assert np.array_equal(r0['support'][:, 0], idx.astype(np.float64)) and np.array_equal(r0['support'][:, 1] + 1j * r0['support'][:, 2], amp)
  idx, amp = np_topk(psi, 3)
  assert np.array_equal(r0['top3'][:, 0], idx.astype(np.float64))
  tie = r0['tie_psi']
  for k in (1, 3, 9, (1 << n) // 4 + 3):
    idx, amp = np_topk(tie, k)
    assert np.array_equal(r0[f'tie_idx_{k}'], idx) and np.array_equal(r0[f'tie_amp_{k}'], amp), ('tie', k)
  assert r0['tie_perm'].tolist() != list(range(n))
  for k in (3, 9):
    idx, amp = np_topk(tie, k)
    assert np.array_equal(r0[f'tiescan_idx_{k}'], idx) and np.array_equal(r0[f'tiescan_amp_{k}'], amp), ('tie scan', k)
