"""qh_extend / qh_release on the MI355X, at both widths, against NumPy on the LOGICAL amplitudes (np.kron(psi, f) and
reshape-and-index), brought to the host through the handle's bit map as test_gpu_inner.py does.

qh_download re-lays a permuted state out, so a handle under test is downloaded LAST; what src held before a call is read
from a clone taken before it.  (device_ptr() brings a state to canonical order too: the pointer of src is compared before and
after only where the layout is canonical or the memory is the caller's.)

Sizes: 1, 2, 3, 5 qubits (less than one wave), 8 and 9 (one block and its edge), 12, and the smallest size at which every
thread of a launch makes more than one trip of its stride loop: the kernels take 256 * 4 16-byte items per block and trip and
launch at most 2048 blocks along the source (kernels_resize.hip.h: kResizeLoads, kResizeBlocks), so two trips need 2^22 items
-- 22 qubits at complex128, 23 at complex64."""
import ctypes

import numpy as np
import pytest

from qcc_amd import device, gates, native, workloads
from qcc_amd.lib import backend, circuit, tensor
from tests import resize_util, shard_util

pytestmark = pytest.mark.gpu

TOL = 1e-12                        # readers that accumulate in double from the stored amplitudes (test_gpu_inner.TOL)
PARITY = {128: 1e-12, 64: 2e-6}    # amplitudes after gates (test_gpu_parity)
UNIT = {128: 2.0 ** -53, 64: 2.0 ** -24}
SIZES = [1, 2, 3, 5, 8, 9, 12]
_i32p = ctypes.POINTER(ctypes.c_int32)


# ---- helpers (the pattern of test_gpu_inner.py) -------------------------------------------------------------------------------
def _state(st, shard=0, nglob=None):
  """(global logical indices, amplitudes as complex128) of everything the handle holds, whatever layout the download leaves"""
  phys = st.download().astype(np.complex128)
  bm = shard_util.bitmap(st, nglob or st.nbits)
  if shard == 0 and bm == list(range(len(bm))):
    return np.arange(phys.size, dtype=np.int64), phys
  return shard_util.phys_to_logical(st, shard, np.arange(phys.size), nglob or st.nbits).astype(np.int64), phys


def _logical(st):
  lo, phys = _state(st)
  out = np.empty_like(phys)
  out[lo] = phys
  return out


def _random_state(n, seed):
  rng = np.random.default_rng(seed)
  v = rng.normal(size=1 << n) + 1j * rng.normal(size=1 << n)
  return v / np.linalg.norm(v)


def _uploaded(n, bw, seed, swaps=(), fusion=native.QH_FUSE_OFF):
  st = device.DeviceState(n, bw, fusion=fusion)
  st.upload(_random_state(n, seed))
  for x, y in swaps:
    st.remap_swap(x, y)
  return st


def _fused(n, bw, seed, depth=12):
  st = device.DeviceState(n, bw, fusion=native.QH_FUSE_SWEEP)
  ops, g8 = workloads.supremacy_stream(n, depth, seed=seed).arrays()
  st.init_basis(0)
  st.run_stream(ops, g8)
  st.flush()
  return st


def _fused_permuted(n, bw, first_seed=0):
  """a fused run whose relayout sweeps left a permuted bit map (which circuits do depends on the planner: the first of
  six seeds that does)"""
  for seed in range(first_seed, first_seed + 6):
    st = _fused(n, bw, seed)
    if shard_util.bitmap(st) != list(range(n)):
      return st
    st.close()
  raise AssertionError(f'no supremacy-{n} circuit of seeds {first_seed}..{first_seed + 5} left a permuted bit map')


def _layouts(n):
  """canonical, and re-labelled by remap_swap: low <-> high, full reversal, neighbours"""
  out = [('canonical', [])]
  if n > 1:
    out += [('low-high', [(0, n - 1)]), ('reversal', [(k, n - 1 - k) for k in range(n // 2)]),
            ('neighbours', [(k, k + 1) for k in range(0, n - 1, 2)])]
  return out


def _random_table(k, seed):
  rng = np.random.default_rng(seed)
  f = rng.normal(size=1 << k) + 1j * rng.normal(size=1 << k)
  return f / np.linalg.norm(f)


class _Watch:
  """what a call must leave alone in src and add to its counters; `with _Watch(src) as w: new = ...; w.made(new)`"""

  def __init__(self, src, nglob=None):
    self.src, self.nglob = src, nglob

  def __enter__(self):
    s = self.src
    self.bm, self.marg, self.stats = shard_util.bitmap(s, self.nglob), s.marginal([]).tobytes(), s.stats()
    return self

  def made(self, new):
    s, after = self.src, self.src.stats()
    assert after['kernels_launched'] - self.stats['kernels_launched'] == 1
    moved = ((1 << s.nbits) + (1 << new.nbits)) * (s.bit_width // 8)      # src read once + the new state written once
    assert after['bytes_algorithmic'] - self.stats['bytes_algorithmic'] == moved
    assert after['bytes_swept'] - self.stats['bytes_swept'] == moved
    assert new.stats() == dict.fromkeys(new.stats(), 0)
    pend = ctypes.c_uint64(9)
    native.check(new.lib.qh_pending_gates(new.h, ctypes.byref(pend)))
    assert pend.value == 0
    self.stats = after

  def __exit__(self, *a):
    if a[0] is None:
      assert shard_util.bitmap(self.src, self.nglob) == self.bm and self.src.marginal([]).tobytes() == self.marg


def _check_extend(src, psi, k, bw, amps=None, basis=0, exact=True, what=''):
  """psi: src's logical amplitudes (complex128 of the stored values)"""
  with _Watch(src) as w:
    new = src.extend(k, amps, basis)
    w.made(new)
  with new:
    assert (new.nbits, new.nbits_global, new.bit_width) == (src.nbits + k, src.nbits + k, bw)
    got = _logical(new)
  f = np.asarray(amps, dtype=np.complex128) if amps is not None else (np.arange(1 << k) == basis).astype(np.complex128)
  want = np.kron(psi, f)
  if exact:
    assert np.array_equal(got, want), what
  else:
    bound = 4 * UNIT[bw] * np.kron(np.abs(psi), np.abs(f))
    err = np.abs(got - want)
    print(f'{what}: max |gpu - numpy| / (u |f||a|) = {np.max(err / np.maximum(bound / 4, 1e-300)):.3f} (bound 4)')
    assert np.all(err <= bound), what


def _raw_release(src, bits, value, weight=True):
  b = (ctypes.c_int32 * len(bits))(*bits)
  w = (ctypes.c_double * 2)(7.0, 7.0)
  h = ctypes.c_void_p()
  rc = src.lib.qh_release(src.h, len(bits), b, int(value), w if weight else None, ctypes.byref(h))
  return rc, h, list(w)


def _check_release(src, psi, bits, value, what=''):
  with _Watch(src) as w:
    new, kept, dropped = src.release(bits, value)
    w.made(new)
    again, kept2, dropped2 = src.release(bits, value)
    w.made(again)
    rc, h, untouched = _raw_release(src, bits, value, weight=False)
    assert rc == native.QH_OK and untouched == [7.0, 7.0]
    w.stats = src.stats()
  want, wk, wd = resize_util.np_release(psi, bits, value)
  total = src.inner(src)
  blind = object.__new__(device.DeviceState)
  blind.lib, blind.h, blind.nbits, blind.nbits_global, blind.bit_width, blind.dtype = src.lib, h, new.nbits, new.nbits, src.bit_width, src.dtype
  with new, again, blind:
    assert new.nbits == src.nbits - len(bits)
    got = _logical(new)
    assert np.array_equal(got, want), what                              # copied as stored
    assert np.array_equal(_logical(again), got) and np.array_equal(_logical(blind), got), what
  print(f'{what}: kept {kept!r} (numpy {wk!r}) dropped {dropped!r} (numpy {wd!r}) kept + dropped - inner = {kept + dropped - total.real:.2e}')
  assert (kept, dropped) == (kept2, dropped2), what                     # bitwise reproducible
  assert abs(kept - wk) < TOL and abs(dropped - wd) < TOL, what
  assert abs(kept + dropped - total.real) < TOL and total.imag == 0.0, what


# ---- 1. extend ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('bw', [128, 64])
@pytest.mark.parametrize('n', SIZES)
def test_extend_small_registers(n, bw):
  for name, swaps in _layouts(n):
    with _uploaded(n, bw, 10 + n, swaps) as src, src.clone() as before:
      psi = _logical(before)
      ptr = src.device_ptr if name == 'canonical' else None             # (moves nothing on a canonical layout)
      for k in (1, 2, 5):
        what = f'extend n={n} bw={bw} {name} k={k}'
        for basis in (range(1 << k) if k == 2 else [(1 << k) - 2]):
          _check_extend(src, psi, k, bw, basis=basis, what=what)
        ones = (np.arange(1 << k) % 3 != 1).astype(np.complex128)        # entries exactly 0 and 1
        _check_extend(src, psi, k, bw, amps=ones, what=what)
        _check_extend(src, psi, k, bw, amps=_random_table(k, 7 * n + k), exact=False, what=what)
      assert ptr is None or src.device_ptr == ptr                        # src is where it was
      assert np.array_equal(_logical(src), psi)


@pytest.mark.parametrize('bw', [128, 64])
def test_extend_two_qubits_by_sixteen(bw):
  with _uploaded(2, bw, 3, [(0, 1)]) as src, src.clone() as before:
    psi = _logical(before)
    _check_extend(src, psi, 16, bw, basis=0xBEEF, what=f'2 (x) 16 basis bw={bw}')
    _check_extend(src, psi, 16, bw, amps=_random_table(16, 5), exact=False, what=f'2 (x) 16 table bw={bw}')
    assert np.array_equal(_logical(src), psi)


@pytest.mark.parametrize('bw', [128, 64])
def test_resize_where_every_thread_makes_two_trips(bw):
  n = 22 if bw == 128 else 23                       # 2^22 items: 4096 chunks over 2048 blocks (see the module docstring)
  rng = np.random.default_rng(n)
  v = (rng.random(1 << n) - 0.5) + 1j * (rng.random(1 << n) - 0.5)
  v /= np.linalg.norm(v)
  with device.DeviceState(n, bw) as src:
    src.upload(v)
    psi = src.download().astype(np.complex128)      # canonical: physical == logical
    ptr = src.device_ptr
    f = _random_table(1, 1)
    with _Watch(src) as w:
      big = src.extend(1, f)
      w.made(big)
    with big:
      got = big.download().astype(np.complex128)
    want = np.kron(psi, f)
    assert np.all(np.abs(got - want) <= 4 * UNIT[bw] * np.kron(np.abs(psi), np.abs(f)))
    del got, want
    w2 = np.abs(psi) ** 2
    for bits, value in (([n // 2], 1), ([0], 1), ([n - 1, 1], 0b01)):
      with _Watch(src) as w:
        small, kept, dropped = src.release(bits, value)
        w.made(small)
      with small:
        got = small.download().astype(np.complex128)
      want, wk, wd = resize_util.np_release(psi, bits, value)
      assert np.array_equal(got, want), bits
      print(f'n={n} bw={bw} release {bits}: kept - numpy {kept - wk:.2e}, dropped - numpy {dropped - wd:.2e}')
      assert abs(kept - wk) < TOL and abs(dropped - wd) < TOL and abs(kept + dropped - w2.sum()) < TOL
    assert src.device_ptr == ptr
    assert np.array_equal(src.download().astype(np.complex128), psi)


# ---- 2. release ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('bw', [128, 64])
@pytest.mark.parametrize('n', [2, 3, 5, 8, 9, 12])
def test_release_small_registers(n, bw):
  for name, swaps in _layouts(n):
    with _uploaded(n, bw, 30 + n, swaps) as src, src.clone() as before:
      psi = _logical(before)
      bm = shard_util.bitmap(src)
      cases = [([b], v) for b in (range(n) if n <= 9 else (0, 1, n // 2, n - 1)) for v in (0, 1)]      # every single bit, both values
      # the released bit at physical position 0 and at position 1: at complex64 the first splits every 16-byte item
      cases += [([bm.index(0)], 1), ([bm.index(1)], 0)]
      if n >= 3:
        cases += [([0, n - 1], 0b10), ([bm.index(0), bm.index(n - 1)], 0b01)]
      if n >= 5:
        cases += [([n - 2, 1, n // 2], 0b101), ([bm.index(0), bm.index(1), bm.index(n - 1)], 0b110)]
      if n >= 3:
        rest = [b for b in range(n) if b != n // 2]                                                    # k = n - 1: one qubit is left
        cases.append((rest, (0x5A5A5 >> 2) & ((1 << (n - 1)) - 1)))
      for bits, value in cases:
        _check_release(src, psi, bits, value, what=f'release n={n} bw={bw} {name} bits={bits} value={value}')
      assert np.array_equal(_logical(src), psi)


@pytest.mark.parametrize('bw', [128, 64])
def test_round_trip_is_bitwise(bw):
  for n, k, v, swaps in ((5, 2, 0b10, [(0, 4)]), (9, 5, 0b10110, []), (12, 1, 1, [(k, 11 - k) for k in range(6)]), (2, 16, 0xA5C3, [])):
    with _uploaded(n, bw, 50 + n, swaps) as src, src.clone() as before:
      psi = _logical(before)
      with src.extend(k, basis=v) as big:
        back, kept, dropped = big.release(list(range(k)), v)
        with back:
          assert dropped == 0.0 and abs(kept - src.inner(src).real) < TOL
          assert shard_util.bitmap(back) == shard_util.bitmap(src)
          assert back.inner(src) == src.inner(src)                      # same layout, same amplitudes: the linear path, bitwise
          assert np.array_equal(_logical(back), psi)
        other, kept, dropped = big.release(list(range(k)), v ^ 1)     # any other value of the new qubits holds nothing
        with other:
          assert kept == 0.0 and abs(dropped - src.inner(src).real) < TOL
          assert not np.any(_logical(other))


# ---- 3. layouts left by fused flushes; the new handle is a full handle ----------------------------------------------------------
@pytest.mark.parametrize('bw', [128, 64])
def test_fused_permuted_source(bw):
  n = 16
  with _fused_permuted(n, bw) as src, src.clone() as before:
    bm = shard_util.bitmap(src)
    psi = _logical(before)
    _check_extend(src, psi, 2, bw, amps=_random_table(2, 4), exact=False, what=f'fused-permuted extend bw={bw}')
    _check_extend(src, psi, 1, bw, basis=1, what=f'fused-permuted extend basis bw={bw}')
    for bits, value in (([bm.index(0)], 1), ([bm.index(1), bm.index(n - 1)], 0b10), ([3, 7, 12], 0b011)):
      _check_release(src, psi, bits, value, what=f'fused-permuted release bw={bw} bits={bits}')
    assert shard_util.bitmap(src) == bm
    assert np.array_equal(_logical(src), psi)


def _np_gate(psi, g, tgt, ctl=None):
  """2x2 g on LOGICAL bit tgt where logical bit ctl is 1"""
  g = np.asarray(g, dtype=np.complex128).reshape(2, 2)
  idx = np.arange(psi.size)
  sel = ((idx >> tgt) & 1) == 0
  if ctl is not None:
    sel &= ((idx >> ctl) & 1) == 1
  lo = idx[sel]
  hi = lo | (1 << tgt)
  out = psi.copy()
  out[lo] = g[0, 0] * psi[lo] + g[0, 1] * psi[hi]
  out[hi] = g[1, 0] * psi[lo] + g[1, 1] * psi[hi]
  return out


@pytest.mark.parametrize('bw', [128, 64])
@pytest.mark.parametrize('fusion', [native.QH_FUSE_OFF, native.QH_FUSE_SWEEP])
def test_new_handle_accepts_gates(fusion, bw):
  n = 12
  with _uploaded(n, bw, 71, [(1, 9)], fusion=fusion) as src, src.clone() as before:
    psi = _logical(before)
    with src.extend(1) as big:
      big.apply_bits(0, 0, gates.hadamard())                             # H on the new qubit ...
      big.apply_bits(1 << 5, 0, gates.pauli_x())                         # ... and a CX from an old qubit (logical 4 of src) onto it
      pend = ctypes.c_uint64()
      native.check(big.lib.qh_pending_gates(big.h, ctypes.byref(pend)))
      assert pend.value == (2 if fusion == native.QH_FUSE_SWEEP else 0)  # the parent's fusion level
      big.flush()
      assert (big.stats()['sweeps'] >= 1) == (fusion == native.QH_FUSE_SWEEP)
      want = _np_gate(_np_gate(np.kron(psi, [1, 0]), gates.hadamard(), 0), gates.pauli_x(), 0, ctl=5)
      assert np.max(np.abs(_logical(big) - want)) <= PARITY[bw]
    small, _, _ = src.release([3], 0)
    with small:
      small.apply_bits(0, 3, gates.hadamard())
      small.apply_bits(1 << 3, 10, gates.pauli_x())
      small.flush()
      want = _np_gate(_np_gate(resize_util.np_release(psi, [3], 0)[0], gates.hadamard(), 3), gates.pauli_x(), 10, ctl=3)
      assert np.max(np.abs(_logical(small) - want)) <= PARITY[bw]
    assert np.array_equal(_logical(src), psi)


# ---- 4. attached and host-mapped sources ------------------------------------------------------------------------------------------
def _owns_hbm(st):
  p = ctypes.c_void_p(1)
  native.check(st.lib.qh_host_ptr(st.h, ctypes.byref(p)))
  return not p.value


@pytest.mark.parametrize('bw', [128, 64])
def test_host_mapped_source(bw):
  n = 9
  with device.DeviceState(n, bw, host_mapped=True) as src:
    src.upload(_random_state(n, 77))
    src.apply1(gates.hadamard(), 3)
    src.sync()
    held = np.asarray(src.host_array()).copy()
    psi = held.astype(np.complex128)
    f = _random_table(2, 1)
    with src.extend(2, f) as big:
      assert _owns_hbm(big) and not _owns_hbm(src)
      assert np.all(np.abs(_logical(big) - np.kron(psi, f)) <= 4 * UNIT[bw] * np.kron(np.abs(psi), np.abs(f)))
    small, kept, dropped = src.release([0, 8], 0b01)
    with small:
      assert _owns_hbm(small)
      want, wk, wd = resize_util.np_release(psi, [0, 8], 0b01)
      assert np.array_equal(_logical(small), want) and abs(kept - wk) < TOL and abs(dropped - wd) < TOL
    src.sync()
    assert np.asarray(src.host_array()).tobytes() == held.tobytes()


@pytest.mark.parametrize('bw', [128, 64])
def test_attached_source(bw):
  n = 10
  with device.DeviceState(n, bw) as owner:
    owner.upload(_random_state(n, 78))
    ptr = owner.device_ptr
    held = owner.download()
    psi = held.astype(np.complex128)
    att = device.DeviceState(n, bw, device_ptr=ptr)
    big = att.extend(1, basis=1)
    small, kept, dropped = att.release([4], 1)
    assert att.device_ptr == ptr
    att.close()                                                          # the results own their memory and streams
    with big, small:
      assert big.device_ptr != ptr and small.device_ptr != ptr
      assert np.array_equal(_logical(big), np.kron(psi, [0, 1]))
      want, wk, wd = resize_util.np_release(psi, [4], 1)
      assert np.array_equal(_logical(small), want) and abs(kept - wk) < TOL and abs(dropped - wd) < TOL
    assert owner.download().tobytes() == held.tobytes()


# ---- 5. shard handles on one GPU ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('bw', [128, 64])
def test_shard_handles(bw):
  nloc, nglob, k = 10, 12, 2
  swaps = [(2, 7), (3, 11)]                                              # local <-> local, and a shard bit swapped in
  held_data = _random_state(nglob, 90).astype(np.complex128 if bw == 128 else np.complex64).astype(np.complex128)
  f = _random_table(k, 91)
  # Shard s is uploaded in physical order (an upload brings a handle to canonical order first) and re-labelled afterwards,
  # the same way on every shard: the global state the four of them then hold is held_data read through that bit map.
  with device.DeviceState(nloc, bw, dry=True) as model:
    model.set_shard(nglob, 0)
    for x, y in swaps:
      model.remap_swap(x, y)
    bm = shard_util.bitmap(model, nglob)
  v = np.empty_like(held_data)
  v[shard_util.logical_of_phys(bm, 1 << nglob).astype(np.int64)] = held_data
  want_big = np.kron(v, f)
  for s in range(4):
    with device.DeviceState(nloc, bw) as src:
      src.set_shard(nglob, s)
      src.upload(held_data[s << nloc:(s + 1) << nloc])
      for x, y in swaps:
        src.remap_swap(x, y)
      assert shard_util.bitmap(src, nglob) == bm
      lo = shard_util.phys_to_logical(src, s, np.arange(1 << nloc), nglob).astype(np.int64)
      mine = v[lo]
      with _Watch(src, nglob) as w:
        big = src.extend(k, f)
        w.made(big)
      with big:
        assert (big.nbits, big.nbits_global) == (nloc + k, nglob + k)
        glo, got = _state(big, s, nglob + k)
        assert np.all(np.abs(got - want_big[glo]) <= 4 * UNIT[bw] * np.kron(np.abs(v), np.abs(f))[glo])
      local = [b for b in range(nglob) if bm[b] < nloc]
      held = [b for b in range(nglob) if bm[b] >= nloc]
      bits, value = [local[1], local[6], bm.index(0)], 0b101
      want_small = resize_util.np_release(v, bits, value)[0]
      with _Watch(src, nglob) as w:
        small, kept, dropped = src.release(bits, value)
        w.made(small)
      with small:
        assert (small.nbits, small.nbits_global) == (nloc - 3, nglob - 3)
        glo, got = _state(small, s, nglob - 3)
        assert np.array_equal(got, want_small[glo])
      keep = np.ones(lo.size, dtype=bool)
      for j, b in enumerate(bits):
        keep &= ((lo >> b) & 1) == ((value >> j) & 1)
      w2 = np.abs(mine) ** 2
      assert abs(kept - w2[keep].sum()) < TOL and abs(dropped - w2[~keep].sum()) < TOL      # per shard, not normalised
      for h in held:
        rc, new, untouched = _raw_release(src, [local[1], h], 0)
        assert rc == native.QH_ERR_NONLOCAL and not new.value and untouched == [7.0, 7.0]
      glo, got = _state(src, s, nglob)
      assert np.array_equal(got, v[glo])


# ---- 6. qc, end to end ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(params=[128, 64])
def width(request):
  tensor.set_tensor_width(request.param)
  yield request.param
  tensor.set_tensor_width(None)
  backend.drop_device_pool()


def _layers(q, nq, seed, depth):
  rng = np.random.default_rng(seed)
  for _ in range(depth):
    for i in range(nq):
      q.ry(i, float(rng.uniform(0.3, 2.8)))
    for i in range(nq - 1):
      q.cu1(i, i + 1, float(rng.uniform(0, 3)))
    q.cx(int(rng.integers(1, nq)), 0)


def _amps(q):
  return np.array(q.psi, dtype=np.complex128).reshape(-1)


def test_qc_late_ancillae_and_release(width):
  from qcc_amd.lib import ops
  n = 14
  q = circuit.qc('aux')
  q.reg(n, 0)
  _layers(q, n, 1, 2)
  psi = _amps(q)
  aux = q.reg(3, 0)                                                       # after the first gate: built on the device
  assert list(aux) == [14, 15, 16] and q.nbits == 17 and q._dev_ok and q._dev.nbits == 17 and not q._host_ok
  q.multi_control([0, 3, 7, 12], 5, aux, ops.PauliX(), 'mcx')           # ANDs into aux, fires, uncomputes
  kept, dropped = q.release(aux)
  print(f'qc width {width}: kept {kept!r}, dropped {dropped!r}')
  assert q.nbits == n and dropped <= 1e-9 * kept
  idx = np.arange(1 << n)
  on = np.ones(1 << n, dtype=bool)
  for c in (0, 3, 7, 12):
    on &= ((idx >> (n - 1 - c)) & 1) == 1
  want = np.where(on, psi[idx ^ (1 << (n - 1 - 5))], psi)
  err = float(np.max(np.abs(_amps(q) - want)))
  print(f'qc width {width}: max |gpu - numpy| after multi_control over late ancillae = {err:.3e}')
  assert err <= PARITY[width]
  q.close()


def test_qc_measure_then_release_and_a_refused_release(width):
  n = 10
  q = circuit.qc('m')
  q.reg(n, 0)
  _layers(q, n, 2, 2)
  before = _amps(q)
  with pytest.raises(ValueError):
    q.release([2, 6], 0)                                                  # not in |00>: refused ...
  assert q.nbits == n
  q.h(1)                                                                  # ... and the circuit goes on, on the old state
  q.h(1)
  assert np.max(np.abs(_amps(q) - before)) <= 10 * PARITY[width]
  before = _amps(q)
  qs = [6, 2, 9]
  v, prob = q.measure(qs, seed=5)
  kept, dropped = q.release(qs, v)
  want, wk, _ = resize_util.np_release(before, [n - 1 - t for t in reversed(qs)], v)
  assert q.nbits == n - 3 and abs(prob - wk) < 10 * PARITY[width] and abs(kept - 1) < 10 * PARITY[width] and dropped <= 1e-9 * kept
  assert np.max(np.abs(_amps(q) - want / np.sqrt(wk))) <= 10 * PARITY[width]
  q.close()


def test_qc_late_qubit_at_20_qubits_without_a_host_copy(width, monkeypatch):
  n = 20
  q = circuit.qc('big')
  q.reg(n, 0)
  _layers(q, n, 3, 1)

  def no_download(*a, **kw):
    raise AssertionError('the state was copied to the host')
  monkeypatch.setattr(device.DeviceState, 'download', no_download)
  monkeypatch.setattr(device.DeviceState, 'upload', no_download)
  p_old = q.probabilities([3, 11])
  q.qubit(0.6, 0.8)
  assert q.nbits == n + 1 and q._dev.nbits == n + 1
  tol = 1e-12 if width == 128 else 1e-6
  assert np.allclose(q.probabilities([n]), [0.36, 0.64], atol=tol) and abs(q.norm2() - 1) < tol
  assert np.allclose(q.probabilities([3, 11]), p_old, atol=tol)
  q.cx(n, 0)                                                              # gates reach the new qubit
  q.h(n)
  assert abs(q.norm2() - 1) < tol
  kept, dropped = q.release([n], 0, tol=None)                             # ... and it can be given back, still on the device
  assert q.nbits == n and abs(kept + dropped - 1) < tol
  q.close()
