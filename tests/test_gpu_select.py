"""Sparse readout on the MI355X: qh_select, qh_topk and qh_amplitudes against NumPy on the downloaded state.

States from a gate stream as test_gpu_measure makes them (n = 1 .. 20, both widths, per-gate and fused runs that leave a
permuted bit map), the tie path of qh_topk on flat states, its pass count on a peaked one, shard handles in the layouts of
test_gpu_shard_readout, and qc.dump / _LazyPsi.dump printing a resident state without a download.

Probabilities are compared as the engine computes them -- fma(im, im, re * re) in double from the stored values
(tests/select_util.fma_probs), exactly, so that near-ties at a threshold or at the cut are decided as the kernel decides them."""
import contextlib
import ctypes
import io

import numpy as np
import pytest

from qcc_amd import device, gates, native, workloads
from qcc_amd.lib import circuit, state, tensor
from tests.select_util import fma_probs
from tests.shard_util import bitmap as _bitmap
from tests.test_gpu_measure import _logical_state, _prepared
from tests.test_gpu_shard_readout import shards

pytestmark = pytest.mark.gpu

SIZES = (1, 4, 7, 9, 12, 13, 15, 20)
both_widths = pytest.mark.parametrize('bw', [128, 64])
both_fusions = pytest.mark.parametrize('fusion', [native.QH_FUSE_OFF, native.QH_FUSE_SWEEP])


def _state(n, bw, fusion, seed):
  if n >= 4:
    return _prepared(n, bw, fusion, seed)
  st = device.DeviceState(n, bw, fusion=fusion)
  st.init_basis(0)
  for q in range(n):
    st.apply1(gates.ry(0.9 + q), q)
    st.apply1(gates.u1(0.4), q)
  st.flush()
  return st


def _plain(a):
  return a.real * a.real + a.imag * a.imag


def _probs(a):
  """probabilities of the complex128 array a exactly as the engine computes them"""
  return fma_probs(a)


def _want_topk(a, k, p=None):
  """indices of the k most probable nonzero entries of a, ties by ascending index, decided on the engine's probabilities"""
  p = _probs(a) if p is None else p
  order = np.lexsort((np.arange(p.size), -p))
  return order[p[order] > 0][:int(k)].astype(np.uint64)


def _weight_close(got, want, bw):
  if bw == 128:
    assert abs(got - want) < 1e-12, (got, want)
  else:
    assert abs(got - want) <= 1e-6 * max(want, 1e-30) + 1e-9, (got, want)     # test_gpu_measure's rule for complex64


def _launched(st):
  return st.stats()['kernels_launched']


# ---- select ----------------------------------------------------------------------------------------------------------------
@both_widths
@both_fusions
def test_select_thresholds(bw, fusion):
  permuted = []
  for n in SIZES:
    with _state(n, bw, fusion, seed=n) as st, st.clone() as twin:
      bm = _bitmap(st)
      permuted.append(n >= 14 and bm != list(range(n)))
      size = 1 << n
      # the readers first, in the layout the flush left; thresholds from a rough copy of the probabilities
      rough = np.sort(_plain(twin.download().astype(np.complex128)))
      thresholds = [0.0, float(rough[size // 2]), float(rough[min(size - 1, (99 * size) // 100)]), float(rough[-1]) * 1.5]
      got = []
      for thr in thresholds:
        k0 = _launched(st)
        s0 = st.stats()
        idx, amp, cnt, w = st.select(thr, 1 << 20)
        s1 = st.stats()
        assert _launched(st) - k0 == 1
        assert s1['bytes_swept'] - s0['bytes_swept'] == size * (16 if bw == 128 else 8)
        assert s1['bytes_algorithmic'] - s0['bytes_algorithmic'] == size * (16 if bw == 128 else 8)
        idx2, amp2, cnt2, w2 = st.select(thr, 1 << 20)
        assert np.array_equal(idx, idx2) and amp.tobytes() == amp2.tobytes() and cnt == cnt2
        assert np.float64(w).tobytes() == np.float64(w2).tobytes()          # bitwise reproducible
        got.append((idx, amp, cnt, w))
      # cap too small: the count is exact and out is untouched
      full = got[0][2]
      assert full == size
      if size > 1:
        buf = np.empty(size - 1, dtype=[('index', np.uint64), ('re', np.float64), ('im', np.float64)])
        buf[:] = (77, 7.0, -7.0)                                            # a sentinel in every entry
        c, wt = ctypes.c_uint64(), ctypes.c_double()
        native.check(st.lib.qh_select(st.h, 0.0, size - 1, buf.ctypes.data_as(ctypes.POINTER(native.QhEntry)),
                                      ctypes.byref(c), ctypes.byref(wt)))
        assert c.value == size and np.float64(wt.value).tobytes() == np.float64(got[0][3]).tobytes()
        assert np.all(buf['index'] == 77) and np.all(buf['re'] == 7.0) and np.all(buf['im'] == -7.0)
        i0, a0, c0, _ = st.select(0.0, 0)                                   # count only
        assert (i0.size, a0.size, c0) == (0, 0, size)
      assert _bitmap(st) == bm                                              # reads only: the layout is as it was
      a = _logical_state(st)
      assert a.tobytes() == _logical_state(twin).tobytes()                  # ... and so is the state
    p = _probs(a)
    for thr, (idx, amp, cnt, w) in zip(thresholds, got):
      want = np.flatnonzero(p >= thr)
      assert cnt == want.size == idx.size
      assert np.array_equal(idx, want.astype(np.uint64))                    # the index set, ascending
      assert amp.tobytes() == a[want].tobytes()                             # bitwise the stored amplitudes
      _weight_close(w, float(p[want].sum()), bw)
    assert got[3][2] == 0 and got[3][3] == 0.0
  if fusion == native.QH_FUSE_SWEEP:
    assert any(permuted), permuted                      # relayout sweeps left a permuted bit map in some n >= 14 case


# ---- topk ------------------------------------------------------------------------------------------------------------------
@both_widths
@both_fusions
def test_topk_against_a_sort(bw, fusion):
  permuted = []
  for n in SIZES:
    with _state(n, bw, fusion, seed=50 + n) as st:
      bm = _bitmap(st)
      permuted.append(n >= 14 and bm != list(range(n)))
      ks = [k for k in (1, 2, 16, 255, 4096) if k <= (1 << n)]
      if (1 << n) + 3 <= native.QH_TOPK_MAX:
        ks.append((1 << n) + 3)                            # more than the support (n < 12; larger n: the sparse-state test)
      got = [st.topk(k) for k in ks]
      best, pbest = st.argmax()
      empty = st.topk(0)
      assert _bitmap(st) == bm
      a = _logical_state(st)
    assert empty[0].size == 0 and empty[1].size == 0
    p = _probs(a)
    for k, (idx, amp) in zip(ks, got):
      want = _want_topk(a, k, p)
      assert np.array_equal(idx, want), (n, k)
      assert amp.tobytes() == a[want.astype(np.int64)].tobytes()
      pr = fma_probs(amp)
      assert np.all(pr > 0) and np.all(np.diff(pr) <= 0)                    # descending, never a zero
    assert int(got[0][0][0]) == best and fma_probs(got[0][1])[0] == pbest  # topk(1) names qh_argmax's amplitude
  if fusion == native.QH_FUSE_SWEEP:
    assert any(permuted), permuted


def _flat(n, bw, fusion, qft):
  st = device.DeviceState(n, bw, fusion=fusion)
  st.init_basis(0)
  if qft:
    st.run_stream(*workloads.qft_stream(range(n)).arrays())
  else:
    for q in range(n):
      st.apply1(gates.hadamard(), q)
  st.flush()
  return st


def _cap(k):
  """candidates one compaction of qh_topk(k) may collect (engine.hip topk_candidates)"""
  return max(4 * k, native.QH_TOPK_MAX)


@both_widths
@both_fusions
@pytest.mark.parametrize('n', [13, 20])
def test_topk_tie_path_flat_state(bw, fusion, n):
  """H on every qubit of |0>: 2^n bitwise-equal amplitudes, more ties than a candidate list holds.  The k smallest logical
  indices are the answer, whatever layout the flush left."""
  with _flat(n, bw, fusion, qft=False) as st:
    got = []
    for k in (1, 16, 4096):
      k0 = _launched(st)
      got.append((k, st.topk(k), _launched(st) - k0))
    a = st.download()
  assert np.unique(a).size == 1 and a[0] != 0
  for k, (idx, amp), reads in got:
    assert np.array_equal(idx, np.arange(k, dtype=np.uint64))
    assert amp.tobytes() == a[:k].astype(np.complex128).tobytes()
    if (1 << n) > _cap(k):
      assert reads == 7                                    # six histograms down to one value, one tie scan of 4096 or 8192
    else:
      assert reads == 2                                    # the whole state fits the candidate list
  assert got[0][2] == 7 and got[1][2] == 7


@both_widths
@both_fusions
@pytest.mark.parametrize('n', [13, 20])
def test_topk_qft_of_a_basis_state(bw, fusion, n):
  """A QFT's output: equal magnitudes up to rounding, so a handful of probability values a few ulps apart with many exact
  ties each, unevenly spread over the logical index range, and entries above the tied value.  Refinement down to single
  values, then ties by logical index.  Whether a call ends in the tie scan is known from the reference: it does iff the
  entries at or above the k-th value outnumber the candidate list."""
  with _flat(n, bw, fusion, qft=True) as st:
    got = []
    for k in (1, 16, 255, 4096):
      k0 = _launched(st)
      got.append((k, st.topk(k), _launched(st) - k0))
    a = _logical_state(st)
  p = _probs(a)
  order = np.lexsort((np.arange(p.size), -p))
  for k, (idx, amp), reads in got:
    assert np.array_equal(idx, order[:k].astype(np.uint64)), k
    assert amp.tobytes() == a[order[:k]].tobytes()
    v = p[order[k - 1]]
    above, at_or_above = int(np.count_nonzero(p > v)), int(np.count_nonzero(p >= v))
    if at_or_above > _cap(k):
      assert reads >= 6 + (1 if above else 0) + 1, (k, reads)       # six histograms, the entries above, at least one scan
    else:
      assert 2 <= reads <= 7, (k, reads)


@both_widths
@pytest.mark.parametrize('swaps', [[], [(0, 19), (3, 12), (7, 16)]])
def test_topk_tie_scan_retries_and_grows(bw, swaps):
  """Ties that are absent from the low logical indices and dense above: the scan's first ranges find nothing and grow
  fourfold, the first range that reaches the dense part overflows the scan buffer and is cut by 16 and read again.  Three
  entries lie above the tied value.  The scan sequence follows from the lengths alone (4096, x 4 after a range with too few,
  / 16 after one with more than 8192 hits): 12 scans before 16 ties from index 2^16 on are in hand."""
  n, first = 20, 1 << 16
  rng = np.random.default_rng(5)
  a = np.zeros(1 << n, dtype=np.complex128)
  a[:first] = 2.0 ** -14 * (rng.random(first) + 0.1)                          # distinct, all below the tied value
  a[first:] = 2.0 ** -10 * (1 + 1j) / np.sqrt(2)                              # bitwise equal
  top = np.array([5, 70000, 999999])
  a[top] = [0.05, 0.04j, -0.03]
  a = a.astype(np.complex128 if bw == 128 else np.complex64)
  with device.DeviceState(n, bw) as st:
    st.upload(a)
    for x, y in swaps:
      st.remap_swap(x, y)                                  # relabelled: logical order is no longer the physical one
    k0 = _launched(st)
    idx, amp = st.topk(19)
    reads = _launched(st) - k0
    logical = _logical_state(st)
  p = _probs(logical)
  want = _want_topk(logical, 19, p)
  assert np.array_equal(idx, want) and amp.tobytes() == logical[want.astype(np.int64)].tobytes()
  tied = np.flatnonzero(p == p[want[-1]])
  assert tied.size == (1 << n) - first - 2 and np.array_equal(want[3:], tied[:16].astype(np.uint64))
  if not swaps:
    assert reads == 6 + 1 + 12                             # histograms, the three entries above, the scans


def _peaked(n, bw, seed):
  rng = np.random.default_rng(seed)
  a = 1e-3 * (rng.standard_normal(1 << n) + 1j * rng.standard_normal(1 << n))
  where = rng.choice(1 << n, 40, replace=False)
  a[where] = (0.2 + 0.01 * np.arange(40)) * np.exp(1j * rng.random(40) * 6)
  a /= np.linalg.norm(a)
  return a.astype(np.complex128 if bw == 128 else np.complex64)


@both_widths
@pytest.mark.parametrize('n', [7, 12, 16])
def test_topk_peaked_state_takes_two_reads(bw, n):
  a = _peaked(n, bw, n)
  with device.DeviceState(n, bw) as st:
    st.upload(a)
    for k in (1, 16):
      k0 = _launched(st)
      idx, amp = st.topk(k)
      assert _launched(st) - k0 == 2                       # one histogram, one compaction
      want = _want_topk(a.astype(np.complex128), k)
      assert np.array_equal(idx, want) and amp.tobytes() == a[want.astype(np.int64)].astype(np.complex128).tobytes()


@both_widths
@both_fusions
def test_topk_sparse_states(bw, fusion):
  for n in (1, 5, 13):
    with device.DeviceState(n, bw, fusion=fusion) as st:
      st.init_basis((1 << n) - 2 if n > 1 else 1)
      idx, amp = st.topk(16)
      assert idx.tolist() == [(1 << n) - 2 if n > 1 else 1] and amp.tolist() == [1.0]
      st.init_basis(0)
      st.apply1(gates.hadamard(), 0)
      for q in range(1, n):
        st.applyc(gates.pauli_x(), q - 1, q)
      idx, amp = st.topk(16)                               # GHZ: two entries, no zero-probability ones
      want = [0, (1 << n) - 1]
      assert idx.tolist() == want and np.all(np.abs(amp) > 0.7)
      sidx, samp, cnt, w = st.select(0.25)
      assert sidx.tolist() == want and cnt == 2 and abs(w - 1) < (1e-12 if bw == 128 else 1e-6)
      assert samp.tobytes() == amp.tobytes()


# ---- amplitudes ------------------------------------------------------------------------------------------------------------
@both_widths
@both_fusions
def test_amplitudes_gather(bw, fusion):
  rng = np.random.default_rng(9)
  for n in (1, 7, 12, 15):
    with _state(n, bw, fusion, seed=70 + n) as st:
      idx = rng.integers(0, 1 << n, size=4096).astype(np.uint64)            # with duplicates
      k0 = _launched(st)
      got, nlocal = st.amplitudes(idx, nlocal=True)
      assert _launched(st) - k0 == 0                       # no read of the state
      one = [st.amplitude(int(i)) for i in idx[:8]]
      none = st.amplitudes([])
      with pytest.raises(native.QhError) as e:
        st.amplitudes([0, 1 << n])
      assert e.value.code == native.QH_ERR_ARG
      a = _logical_state(st)
    assert got.dtype == np.complex128 and got.tobytes() == a[idx.astype(np.int64)].tobytes()
    assert nlocal == 4096 and none.size == 0
    assert [complex(x) for x in one] == got[:8].tolist()


@both_widths
def test_amplitudes_of_sampled_shots(bw):
  """the companion of qh_sample: the ideal probabilities of exactly the bit strings that were drawn, on a 20-qubit
  supremacy state (test_gpu_measure._prepared runs workloads.supremacy_stream(n, 12, seed) under fused sweeps)"""
  n = 20
  with _prepared(n, bw, native.QH_FUSE_SWEEP, seed=3) as st:
    shots = st.sample(np.sort(np.random.default_rng(4).random(4096)))
    amps = st.amplitudes(shots)
    a = _logical_state(st)
  assert amps.tobytes() == a[shots.astype(np.int64)].tobytes()
  assert np.all(_plain(amps) > 0)                                           # a shot never lands on an exact zero


# ---- shard handles ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('layout', ['canonical', 'sweep', 'mid3', 'midhalf'])
@both_widths
@pytest.mark.parametrize('nloc,g', [(10, 1), (10, 2), (14, 1), (14, 2)])
def test_shard_handles(nloc, g, bw, layout):
  n = nloc + g
  rng = np.random.default_rng(nloc * 8 + g)
  with shards(nloc, g, bw, layout, seed=300 + nloc + g) as F:
    a = F.before
    rough = np.sort(_plain(a))
    thr = float(rough[(99 * a.size) // 100])
    p = _probs(a)
    want = np.flatnonzero(p >= thr)
    idx_all = rng.integers(0, 1 << n, size=2048).astype(np.uint64)
    k = 64
    parts, tops, total_w, total_local = [], [], 0.0, 0
    summed = np.zeros(idx_all.size, dtype=np.complex128)
    for s, st in enumerate(F.sts):
      bm = F.bm(s)
      mine = np.sort(F.logical(s))                         # the global logical indices this shard holds
      idx, amp, cnt, w = st.select(thr)
      assert cnt == idx.size and np.all(np.diff(idx.astype(np.int64)) > 0)
      assert np.all(np.isin(idx.astype(np.int64), mine))   # indices are global, shard bits included
      assert amp.tobytes() == a[idx.astype(np.int64)].tobytes()
      parts.append(idx)
      total_w += w
      tops.append(st.topk(k))
      got, nlocal = st.amplitudes(idx_all, nlocal=True)
      held = np.isin(idx_all.astype(np.int64), mine)
      assert nlocal == int(held.sum())
      assert np.all(got[~held] == 0) and got[held].tobytes() == a[idx_all[held].astype(np.int64)].tobytes()
      summed += got
      assert F.bm(s) == bm
    # the per-shard selections partition the full-state selection
    assert np.array_equal(np.sort(np.concatenate(parts)), want.astype(np.uint64))
    _weight_close(total_w, float(p[want].sum()), bw)
    assert summed.tobytes() == a[idx_all.astype(np.int64)].tobytes()         # a sum over ranks is the answer
    # merging the per-shard topk gives the global one
    midx = np.concatenate([t[0] for t in tops])
    mamp = np.concatenate([t[1] for t in tops])
    order = np.lexsort((midx, -fma_probs(mamp)))[:k]
    assert np.array_equal(midx[order], _want_topk(a, k))
    assert mamp[order].tobytes() == a[midx[order].astype(np.int64)].tobytes()
    assert float(np.max(np.abs(F.gather() - a))) == 0.0    # read only


# ---- qc ------------------------------------------------------------------------------------------------------------------
def _printed(fn, *a, **kw):
  out = io.StringIO()
  with contextlib.redirect_stdout(out):
    fn(*a, **kw)
  return out.getvalue()


@both_widths
def test_qc_dump_prints_a_resident_state_without_a_download(bw):
  tensor.set_tensor_width(bw)
  try:
    q = circuit.qc()
    q.reg(12, 0b101100101110)
    for i in range(0, 12, 3):
      q.h(i)
      q.ry(i + 1, 0.3 + i)
      q.cx(i, i + 2)
      q.rz(i + 2, 1.1 * (i + 1))
      q.x(i + 1)
    dev = q._ensure_device()                               # pylint: disable=protected-access
    calls = []
    orig = dev.download
    dev.download = lambda *a, **kw: (calls.append(1), orig(*a, **kw))[1]
    got = _printed(q.dump)
    top = q.top(3)
    sup = q.support(1e-3)
    assert not calls
    del dev.download
    host = state.State(dev.download())

    def reference():
      print(q.ir, end='')
      host.dump('Current state')
    want = _printed(reference)
    assert got == want and len(want.splitlines()) > 8
    a = np.asarray(host).astype(np.complex128)
    assert [circuit.helper.bits2val(b) for b, _, _ in top] == _want_topk(a, 3).tolist()
    assert [circuit.helper.bits2val(b) for b, _, _ in sup] == np.flatnonzero(_probs(a) >= 1e-3).tolist()
    q.close()
  finally:
    tensor.set_tensor_width(None)


def test_lazy_psi_dump_above_the_snapshot_size_takes_no_snapshot():
  n = 22
  assert n > circuit._MEASURE_SNAPSHOT_BITS              # pylint: disable=protected-access
  tensor.set_tensor_width(128)
  try:
    q = circuit.qc()
    q.reg(n, 0)
    q.h(0)
    for i in range(1, n):
      q.cx(i - 1, i)
    q.s(n - 1)
    prob, psi = q.measure_bit(3, 1, collapse=False)
    assert isinstance(psi, circuit._LazyPsi) and abs(prob - 0.5) < 1e-12      # pylint: disable=protected-access
    dev = q._ensure_device()                               # pylint: disable=protected-access
    calls = []
    orig = dev.download
    dev.download = lambda *a, **kw: (calls.append(1), orig(*a, **kw))[1]
    got = _printed(psi.dump, 'ghz')
    assert not calls and psi._snap is None and not q._host_ok                 # pylint: disable=protected-access
    del dev.download
    amps = dev.amplitudes([0, (1 << n) - 1])
    want = '\n'.join([state.dump_header(n, 'ghz'), state.dump_row(n, 0, np.complex128(amps[0])),
                      state.dump_row(n, (1 << n) - 1, np.complex128(amps[1]))]) + '\n'
    assert got == want
    assert abs(amps[0] - 2 ** -0.5) < 1e-12 and abs(amps[1] - 1j * 2 ** -0.5) < 1e-12
    with pytest.raises(ValueError):
      psi.dump(prob_only=False)                            # 2^22 rows: refused, still no snapshot
    assert psi._snap is None                               # pylint: disable=protected-access
    q.close()
  finally:
    tensor.set_tensor_width(None)
