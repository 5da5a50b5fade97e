"""CPU tests of qh_extend / qh_release: the C-ABI symbols and their argument checks, the bit maps of both calls on
planner-only handles against a bit-by-bit NumPy model (shard bits and shuffled maps included), the host arithmetic
stand-alone under sanitizers, and circuit.qc -- qc.release and the late registers of qc.reg / qubit / bitstring -- over a
NumPy stand-in device without extend / release (the host route) and over a recording one that has them (the device route)."""
import ctypes
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

from qcc_amd import device, native
from qcc_amd.lib import backend, circuit, tensor
from tests import fake_device, resize_util, shard_util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_i32p = ctypes.POINTER(ctypes.c_int32)


def _bits(*b):
  return (ctypes.c_int32 * len(b))(*b)


# ---- the C-ABI ---------------------------------------------------------------------------------------------------------
def test_version_and_symbols_bound():
  lib = native.load()
  assert lib.qh_version() >= 111
  want = {'qh_extend': [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_double), ctypes.c_uint64, ctypes.POINTER(ctypes.c_void_p)],
          'qh_release': [ctypes.c_void_p, ctypes.c_int, _i32p, ctypes.c_uint64, ctypes.POINTER(ctypes.c_double),
                         ctypes.POINTER(ctypes.c_void_p)]}
  for name, args in want.items():
    assert native.SIGNATURES[name] == (ctypes.c_int, args)
    assert getattr(lib, name).argtypes == args and getattr(lib, name).restype == ctypes.c_int


def test_argument_errors():
  lib = native.load()
  d = ctypes.c_void_p()
  native.check(lib.qh_create_dry(10, 128, ctypes.byref(d)))
  big, tiny, shard = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
  native.check(lib.qh_create_dry(30, 128, ctypes.byref(big)))
  native.check(lib.qh_create_dry(3, 64, ctypes.byref(tiny)))
  native.check(lib.qh_create_dry(10, 128, ctypes.byref(shard)))
  native.check(lib.qh_set_shard(shard, 12, 2))
  new = ctypes.c_void_p()
  w = (ctypes.c_double * 2)(7.0, 7.0)
  try:
    # null pointers
    assert lib.qh_extend(None, 1, None, 0, ctypes.byref(new)) == native.QH_ERR_ARG
    assert lib.qh_extend(d, 1, None, 0, None) == native.QH_ERR_ARG
    assert lib.qh_release(None, 1, _bits(0), 0, w, ctypes.byref(new)) == native.QH_ERR_ARG
    assert lib.qh_release(d, 1, None, 0, w, ctypes.byref(new)) == native.QH_ERR_ARG
    assert lib.qh_release(d, 1, _bits(0), 0, w, None) == native.QH_ERR_ARG
    # k out of range
    for k in (0, 17, -1):
      assert lib.qh_extend(d, k, None, 0, ctypes.byref(new)) == native.QH_ERR_ARG
      assert lib.qh_release(d, k, _bits(*range(17)), 0, w, ctypes.byref(new)) == native.QH_ERR_ARG
    # basis / value that do not fit k bits
    assert lib.qh_extend(d, 2, None, 4, ctypes.byref(new)) == native.QH_ERR_ARG
    assert lib.qh_extend(d, 16, None, 1 << 16, ctypes.byref(new)) == native.QH_ERR_ARG
    assert lib.qh_release(d, 2, _bits(0, 1), 4, w, ctypes.byref(new)) == native.QH_ERR_ARG
    # a bit twice, a bit out of range
    assert lib.qh_release(d, 2, _bits(3, 3), 0, w, ctypes.byref(new)) == native.QH_ERR_SAME_QUBIT
    assert lib.qh_release(d, 1, _bits(10), 0, w, ctypes.byref(new)) == native.QH_ERR_BAD_QUBIT
    assert lib.qh_release(d, 2, _bits(1, -1), 0, w, ctypes.byref(new)) == native.QH_ERR_BAD_QUBIT
    # resulting sizes
    assert lib.qh_release(tiny, 3, _bits(0, 1, 2), 0, w, ctypes.byref(new)) == native.QH_ERR_ARG        # nothing would remain
    assert lib.qh_release(tiny, 4, _bits(0, 1, 2, 3), 0, w, ctypes.byref(new)) == native.QH_ERR_ARG
    assert lib.qh_extend(big, 11, None, 0, ctypes.byref(new)) == native.QH_ERR_ARG                       # 41 local qubits
    assert lib.qh_extend(big, 10, None, 0, ctypes.byref(new)) == native.QH_OK and new.value             # 40 is the limit
    nl, ng = ctypes.c_int(), ctypes.c_int()
    native.check(lib.qh_nbits(new, ctypes.byref(nl), ctypes.byref(ng)))
    assert (nl.value, ng.value) == (40, 40)
    lib.qh_destroy(new)
    new = ctypes.c_void_p()
    # a released bit held by the shard index: nothing created, weight untouched
    for held in (10, 11):
      assert lib.qh_release(shard, 2, _bits(3, held), 0, w, ctypes.byref(new)) == native.QH_ERR_NONLOCAL
      assert b'exchange first' in lib.qh_last_error()
    assert not new.value and list(w) == [7.0, 7.0]
    # every refusal above left `out` alone
    assert not new.value
    # planner-only in, planner-only out: weight untouched, the sizes new
    assert lib.qh_release(shard, 2, _bits(3, 9), 1, w, ctypes.byref(new)) == native.QH_OK and list(w) == [7.0, 7.0]
    native.check(lib.qh_nbits(new, ctypes.byref(nl), ctypes.byref(ng)))
    assert (nl.value, ng.value) == (8, 10)
    out = ctypes.c_double()
    assert lib.qh_norm2(new, ctypes.byref(out)) == native.QH_ERR_ARG and b'dry' in lib.qh_last_error()
    lib.qh_destroy(new)
  finally:
    for h in (d, big, tiny, shard):
      lib.qh_destroy(h)


# ---- the maps, on planner-only handles -------------------------------------------------------------------------------------
def _dry(nloc, g, shard, swaps, bw=128):
  st = device.DeviceState(nloc, bw, dry=True)
  if g:
    st.set_shard(nloc + g, shard)
  for x, y in swaps:
    st.remap_swap(x, y)
  return st


def _layouts(nloc, g, rng):
  """the identity, local <-> local swaps, and (with shard bits) local <-> shard swaps on top"""
  out = [[]]
  local = [(int(rng.integers(nloc)), int(rng.integers(nloc))) for _ in range(4)]
  out.append([(x, y) for x, y in local if x != y] or [(0, nloc - 1)])
  if g:
    out.append(out[1] + [(int(rng.integers(nloc)), nloc + s) for s in range(g)])
  return out


@pytest.mark.parametrize('nloc', range(3, 11))
def test_maps_on_dry_handles(nloc):
  rng = np.random.default_rng(nloc)
  checked = 0
  for g in (0, 1, 2):
    nglob = nloc + g
    for swaps in _layouts(nloc, g, rng):
      shard = int(rng.integers(1 << g))
      with _dry(nloc, g, shard, swaps, bw=128 if nloc % 2 else 64) as st:
        bm = shard_util.bitmap(st)
        for k in (1, 2, 5):
          with st.extend(k, basis=(1 << k) - 1) as big:
            assert (big.nbits, big.nbits_global, big.bit_width) == (nloc + k, nglob + k, st.bit_width)
            nl, ng = ctypes.c_int(), ctypes.c_int()
            native.check(big.lib.qh_nbits(big.h, ctypes.byref(nl), ctypes.byref(ng)))
            assert (nl.value, ng.value) == (nloc + k, nglob + k)
            resize_util.check_extend_map(bm, shard_util.bitmap(big), nloc, nglob, k)
            assert shard_util.bitmap(st) == bm
        local = [b for b in range(nglob) if bm[b] < nloc]
        for k in (1, 2, 3):
          if k >= nloc:
            continue
          for sub in itertools.combinations(local, k):
            bits = list(sub) if (sum(sub) & 1) else list(reversed(sub))      # the list's order is the caller's
            value = int(rng.integers(1 << k))
            small, kept, dropped = st.release(bits, value)
            with small:
              assert (small.nbits, small.nbits_global) == (nloc - k, nglob - k)
              assert (kept, dropped) == (0.0, 0.0)                           # planner-only: weight untouched
              resize_util.check_release_map(bm, shard_util.bitmap(small), nloc, nglob, bits, value)
              checked += 1
        assert shard_util.bitmap(st) == bm
  assert checked >= 3 * 2 * nloc


def test_dry_siblings_keep_shard_index_and_fusion():
  """shard 1 of 4: shard-index bit 0 is set, bit 1 is clear.  A gate controlled by the logical bit at physical position
  nloc + s runs where bit s of the shard index is set and is a counted no-op where it is clear (qh_apply_bits on a
  planner-only handle, unfused: one gate, one count)."""
  had = (ctypes.c_double * 8)(*(np.array([1, 1, 1, -1]) / np.sqrt(2)).astype(np.complex128).view(np.float64))
  for fusion in (native.QH_FUSE_OFF, native.QH_FUSE_SWEEP):
    with _dry(8, 2, 1, [(1, 9)]) as st:
      st.set_fusion(fusion)
      for new in (st.extend(2), st.release([0], 1)[0], st.release([9, 3], 2)[0]):
        with new:
          assert new.stats() == dict.fromkeys(new.stats(), 0)                # counts from zero
          bm = shard_util.bitmap(new)
          tgt = bm.index(0)
          if fusion == native.QH_FUSE_SWEEP:                                 # the fusion level is copied: gates queue
            native.check(new.lib.qh_apply_bits(new.h, 0, tgt, had))
            pend = ctypes.c_uint64()
            native.check(new.lib.qh_pending_gates(new.h, ctypes.byref(pend)))
            assert pend.value == 1
            continue
          for s, noop in ((0, 0), (1, 1)):
            before = new.stats()['gates_noop']
            native.check(new.lib.qh_apply_bits(new.h, 1 << bm.index(new.nbits + s), tgt, had))
            assert new.stats()['gates_noop'] - before == noop


def test_host_arithmetic_stand_alone_under_sanitizers(tmp_path):
  """qcc_amd/csrc/resize_plan.h is plain C++: maps, predicate and segment squeeze against a bit-by-bit model, for every
  subset of released bits up to 10 local bits with 0 to 3 shard bits, in a stand-alone program built with AddressSanitizer
  and UndefinedBehaviorSanitizer (runtimes linked statically; host code only, nothing is loaded into this process)."""
  cxx = shutil.which('g++') or shutil.which('clang++')
  if not cxx:
    pytest.skip('no host C++ compiler')
  static = ['-static-libasan', '-static-libubsan'] if os.path.basename(cxx).startswith('g++') else ['-static-libsan']
  exe = str(tmp_path / 'resize_plan_check')
  subprocess.check_call([cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', *static,
                         os.path.join(ROOT, 'tools', 'resize_plan_check.cc'), '-o', exe])
  res = subprocess.run([exe], capture_output=True, text=True, timeout=300)
  assert res.returncode == 0, res.stdout + res.stderr
  assert 'ok' in res.stdout


# ---- qc over stand-in devices ------------------------------------------------------------------------------------------------
@pytest.fixture(params=[128, 64])
def host_backend(request):
  """a device without extend / release"""
  tensor.set_tensor_width(request.param)
  backend.set_device_factory(fake_device.OracleDevice)
  yield request.param
  backend.set_device_factory(None)
  tensor.set_tensor_width(None)


@pytest.fixture
def recording_backend():
  tensor.set_tensor_width(128)
  backend.set_device_factory(resize_util.ResizeOracle)
  resize_util.ResizeOracle.reset()
  yield
  backend.set_device_factory(None)
  tensor.set_tensor_width(None)


def _circuit(nq, seed, depth=2, **kw):
  rng = np.random.default_rng(seed)
  q = circuit.qc('c', **kw)
  q.reg(nq, 0)
  for _ in range(depth):
    for i in range(nq):
      q.ry(i, float(rng.uniform(0.2, 2.9)))
    for i in range(nq - 1):
      q.cu1(i, i + 1, float(rng.uniform(0, 3)))
    q.cx(int(rng.integers(1, nq)), 0)
  return q


def _slice(psi, n, qubits, value):
  """NumPy: the register `qubits` (qubits[0] most significant) at `value`"""
  return resize_util.np_release(psi, [n - 1 - q for q in reversed(qubits)], value)


def _amps(q):
  return np.array(q.psi, dtype=np.complex128).reshape(-1)


def test_release_on_the_host_route(host_backend):
  tol = 1e-12 if host_backend == 128 else 1e-6
  n = 6
  q = _circuit(n, 1)
  assert not hasattr(q._ensure_device(), 'release')
  before = _amps(q)
  greg = q.global_reg
  qubits, value = [4, 1], 0b10                      # qubit 4 == 1, qubit 1 == 0
  want, wk, wd = _slice(before, n, qubits, value)
  # far from |value>: refused, and nothing has changed
  with pytest.raises(ValueError):
    q.release(qubits, value)
  assert q.nbits == n and q.global_reg == greg and np.array_equal(_amps(q), before)
  with pytest.raises(ValueError):
    q.release(qubits, value, tol=1e-3)
  kept, dropped = q.release(qubits, value, tol=None)                         # post-selection
  assert abs(kept - wk) < tol and abs(dropped - wd) < tol and abs(kept + dropped - 1) < tol
  assert q.nbits == n - 2 and q.global_reg == greg - 2
  assert np.array_equal(_amps(q), want)
  # the remaining qubits are renumbered from 0 and the circuit goes on: old qubits 0, 2, 3, 5 are 0, 1, 2, 3
  q.h(3)
  q.cx(3, 0)
  ref = circuit.qc('ref')
  ref.psi = want
  ref.h(3)
  ref.cx(3, 0)
  assert np.allclose(_amps(q), _amps(ref), atol=tol)
  r = q.reg(2, 1)                                                            # new registers are numbered from the new size
  assert list(r) == [4, 5] and q.nbits == 6


def test_release_value_forms_and_normalize(host_backend):
  tol = 1e-12 if host_backend == 128 else 1e-6
  n = 5
  for value, as_int in (([1, 0, 1], 0b101), ((0, 1, 1), 0b011), (np.int64(6), 6), (0, 0)):
    q = _circuit(n, 2)
    before = _amps(q)
    want, wk, _ = _slice(before, n, [0, 3, 2], as_int)
    kept, _ = q.release([0, 3, 2], value, tol=None, normalize=True)
    assert abs(kept - wk) < tol
    assert np.allclose(_amps(q), want / np.sqrt(wk), atol=tol) and abs(q.norm2() - 1) < 10 * tol
  q = _circuit(n, 2)
  for bad in ([1, 0], [1, 0, 2], 8, -1):
    with pytest.raises(ValueError):
      q.release([0, 3, 2], bad, tol=None)
  for bad_qubits in ([0, 0], [5], list(range(n)), []):
    with pytest.raises(ValueError):
      q.release(bad_qubits, 0, tol=None)
  assert q.nbits == n


def test_measure_then_release_composes(host_backend):
  tol = 1e-12 if host_backend == 128 else 1e-6
  n = 6
  q = _circuit(n, 3)
  before = _amps(q)
  qs = [5, 0, 2]
  v, prob = q.measure(qs, seed=11)
  kept, dropped = q.release(qs, v)                                            # default tol: the register IS in |v> now
  want, wk, _ = _slice(before, n, qs, v)
  assert abs(wk - prob) < tol and abs(kept - 1) < 10 * tol and dropped <= 1e-9 * kept
  assert q.nbits == n - 3
  assert np.allclose(_amps(q), want / np.sqrt(wk), atol=10 * tol)


def test_late_registers_take_the_device_route(recording_backend):
  dev_cls = resize_util.ResizeOracle
  q = circuit.qc('late')
  q.reg(3, 0b101)
  q.h(0)
  q.cx(0, 2)
  psi = _amps(q)                                       # (the reference run below starts here)
  dev_cls.reset()
  first = q._ensure_device()
  r = q.reg(2, 0b10)
  assert list(r) == [3, 4] and q.nbits == 5 and q.global_reg == 5
  q.qubit(0.6, 0.8)
  q.bitstring(1, 1, 0)
  assert q.nbits == 9 and q.global_reg == 9
  ev = dev_cls.events
  ext = [e for e in ev if e[0] == 'extend']
  assert [(e[1], e[3]) for e in ext] == [(2, 0b10), (1, 0), (3, 0b110)]
  assert ext[0][2] is None and ext[2][2] is None and np.allclose(ext[1][2], [0.6, 0.8])
  assert dev_cls.downloads == 0                        # the state never came to the host
  assert [e for e in ev if e[0] == 'close'] == [('close', 3), ('close', 5), ('close', 6)] and first.closed
  assert q._dev_ok and not q._host_ok and not q._is_product
  want = np.kron(np.kron(np.kron(psi, np.eye(4)[2]), [0.6, 0.8]), np.eye(8)[6])
  assert np.allclose(_amps(q), want, atol=1e-15)
  # ... and gates go on, on the grown state
  q.h(8)
  q.cx(8, 0)
  ref = circuit.qc('ref')
  ref.psi = want
  ref.h(8)
  ref.cx(8, 0)
  assert np.allclose(_amps(q), _amps(ref), atol=1e-14)
  # release on the device route: logical bits, least significant first, and the old device state goes back
  dev_cls.reset()
  before = _amps(q)
  dev_cls.downloads = 0
  kept, dropped = q.release([3, 4], 0b10)
  assert dev_cls.events[0] == ('release', [9 - 1 - 4, 9 - 1 - 3], 0b10) and ('close', 9) in dev_cls.events
  assert dev_cls.downloads == 0 and q.nbits == 7 and q.global_reg == 7
  want2, wk, wd = _slice(before, 9, [3, 4], 0b10)
  assert abs(kept - wk) < 1e-12 and abs(dropped - wd) < 1e-12 and dropped < 1e-20
  assert np.array_equal(_amps(q), want2)
  # a refused release closes the new state and keeps the old one
  dev_cls.reset()
  cur = q._dev
  with pytest.raises(ValueError):
    q.release([0], 0)
  assert q._dev is cur and not getattr(cur, 'closed', False) and dev_cls.events[-1] == ('close', 6) and q.nbits == 7


def test_situations_that_stay_on_the_host_route(recording_backend):
  dev_cls = resize_util.ResizeOracle
  # a product state: the description grows, nothing is built
  q = circuit.qc('product')
  q.reg(3, 1)
  q.qubit(0.6, 0.8)
  q.reg(2, 3)
  assert q._is_product and q._dev is None and not dev_cls.events
  assert np.allclose(_amps(q), np.kron(np.kron(np.eye(8)[1], [0.6, 0.8]), np.eye(4)[3]))
  # a factor of more than 16 qubits
  dev_cls.reset()
  q = circuit.qc('wide')
  q.reg(1, 0)
  q.h(0)
  q.zeros(17)
  assert q.nbits == 18 and not [e for e in dev_cls.events if e[0] == 'extend'] and dev_cls.downloads == 1
  assert np.allclose(_amps(q)[[0, 1 << 17]], [2 ** -0.5, 2 ** -0.5])
  # an aliased circuit: the state is the mapped buffer, registers and releases go through it
  backend.set_host_mapped_factory(resize_util.ResizeOracle)
  try:
    dev_cls.reset()
    q = circuit.qc('aliased', alias_psi=True)
    q.reg(3, 0)
    q.h(1)
    q.reg(2, 1)
    assert q.nbits == 5 and not [e for e in dev_cls.events if e[0] in ('extend', 'release')]
    assert np.allclose(_amps(q), np.kron(np.kron([1, 0], np.kron([2 ** -0.5, 2 ** -0.5], [1, 0])), np.eye(4)[1]))
    kept, dropped = q.release([3, 4], 1)
    assert q.nbits == 3 and abs(kept - 1) < 1e-12 and dropped < 1e-20
    assert not [e for e in dev_cls.events if e[0] in ('extend', 'release')]
    assert np.allclose(_amps(q), np.kron([1, 0], np.kron([2 ** -0.5, 2 ** -0.5], [1, 0])))
  finally:
    backend.set_host_mapped_factory(None)
