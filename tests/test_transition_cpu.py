"""CPU tests of matrix elements between two states: the C-ABI symbols and their argument checks on planner-only handles,
qh_transition_plan on planner-only handles whose bit maps were changed (every term once, passes cut at the batch, px in b's
positions and pz in a's, shard signs and refusals), tools/transition_plan_check.cc stand-alone, and qc.matrix_element /
qc.rotation_gradients with the GPU replaced by a NumPy stand-in that implements the device calls and over the fallback
that reads qc.psi."""
import ctypes
import itertools
import os
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

from qcc_amd import device, native
from qcc_amd.lib import backend, circuit, tensor
from tests import fake_device, transition_util as tu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_up = ctypes.POINTER(ctypes.c_uint64)


def _u64(vals):
  arr = np.ascontiguousarray(vals, dtype=np.uint64)
  return arr, arr.ctypes.data_as(_up)


# ---- the C-ABI ---------------------------------------------------------------------------------------------------------
def test_version_and_symbols_bound():
  lib = native.load()
  assert lib.qh_version() >= 119
  for name in ('qh_transition_pauli', 'qh_transition_plan'):
    assert name in native.SIGNATURES
    assert getattr(lib, name).argtypes == native.SIGNATURES[name][1]
  assert native.QH_TRANSITION_BATCH >= 4
  assert ctypes.sizeof(native.QhTransitionPass) == 32
  with open(os.path.join(ROOT, 'include', 'qcc_hip.h')) as f:
    assert f'#define QH_TRANSITION_BATCH {native.QH_TRANSITION_BATCH}\n' in f.read()


def test_argument_errors_on_dry_handles():
  lib = native.load()
  hs = {}
  for key, (n, bw) in {'a': (10, 128), 'b': (10, 128), 'n11': (11, 128), 'w64': (10, 64), 'sh': (10, 128)}.items():
    hs[key] = ctypes.c_void_p()
    native.check(lib.qh_create_dry(n, bw, ctypes.byref(hs[key])))
  native.check(lib.qh_set_shard(hs['sh'], 12, 1))      # another nbits_global
  try:
    a, b = hs['a'], hs['b']
    out = (ctypes.c_double * 4)(7.0, 7.0, 7.0, 7.0)
    (_x, xp), (_z, zp) = _u64([1, 2]), _u64([0, 3])
    assert lib.qh_transition_pauli(None, b, 2, xp, zp, out) == native.QH_ERR_ARG
    assert lib.qh_transition_pauli(a, None, 2, xp, zp, out) == native.QH_ERR_ARG
    assert lib.qh_transition_pauli(a, b, 2, None, zp, out) == native.QH_ERR_ARG
    assert lib.qh_transition_pauli(a, b, 2, xp, None, out) == native.QH_ERR_ARG
    assert lib.qh_transition_pauli(a, b, 2, xp, zp, None) == native.QH_ERR_ARG
    # mask bits out of range: before the dry-handle refusal, in x and in z, the second term too
    for xs, zs in (([1, 1 << 10], [0, 3]), ([1, 2], [1 << 63, 3]), ([1 << 10, 2], [0, 0])):
      (_x2, xq), (_z2, zq) = _u64(xs), _u64(zs)
      assert lib.qh_transition_pauli(a, b, 2, xq, zq, out) == native.QH_ERR_BAD_QUBIT
      assert b'has bits >= 10' in lib.qh_last_error()
    assert lib.qh_transition_pauli(a, b, 2, xp, zp, out) == native.QH_ERR_ARG and b'dry' in lib.qh_last_error()
    assert lib.qh_transition_pauli(a, a, 2, xp, zp, out) == native.QH_ERR_ARG and b'dry' in lib.qh_last_error()
    assert lib.qh_transition_pauli(a, b, 0, None, None, None) == native.QH_ERR_ARG and b'dry' in lib.qh_last_error()
    for other in ('n11', 'w64', 'sh'):
      assert lib.qh_transition_pauli(a, hs[other], 2, xp, zp, out) == native.QH_ERR_ARG and b'dry' not in lib.qh_last_error()
      assert lib.qh_transition_pauli(hs[other], a, 2, xp, zp, out) == native.QH_ERR_ARG
    assert list(out) == [7.0] * 4
    # the plan: null pointers and shapes
    npass = ctypes.c_uint64(99)
    passes = (native.QhTransitionPass * 2)()
    assert lib.qh_transition_plan(None, b, 2, xp, zp, None, passes, 2, ctypes.byref(npass)) == native.QH_ERR_ARG
    assert lib.qh_transition_plan(a, b, 2, None, zp, None, passes, 2, ctypes.byref(npass)) == native.QH_ERR_ARG
    assert lib.qh_transition_plan(a, b, 2, xp, zp, None, passes, 2, None) == native.QH_ERR_ARG
    assert lib.qh_transition_plan(a, b, 2, xp, zp, None, None, 2, ctypes.byref(npass)) == native.QH_ERR_ARG
    assert lib.qh_transition_plan(a, hs['w64'], 2, xp, zp, None, passes, 2, ctypes.byref(npass)) == native.QH_ERR_ARG
    assert lib.qh_transition_plan(a, hs['n11'], 2, xp, zp, None, passes, 2, ctypes.byref(npass)) == native.QH_ERR_ARG
    (_x3, xq), (_z3, zq) = _u64([1, 2]), _u64([0, 1 << 10])
    assert lib.qh_transition_plan(a, b, 2, xq, zq, None, passes, 2, ctypes.byref(npass)) == native.QH_ERR_BAD_QUBIT
    assert npass.value == 99
    # cap = 0 counts only; no terms: no passes
    native.check(lib.qh_transition_plan(a, b, 2, xp, zp, None, None, 0, ctypes.byref(npass)))
    assert npass.value == 2
    native.check(lib.qh_transition_plan(a, b, 0, None, None, None, None, 0, ctypes.byref(npass)))
    assert npass.value == 0
  finally:
    for h in hs.values():
      lib.qh_destroy(h)


# ---- the plan ----------------------------------------------------------------------------------------------------------
def _bitmap(st, n):
  bm = (ctypes.c_int32 * 64)()
  native.check(st.lib.qh_get_bitmap(st.h, bm))
  return list(bm)[:n]


def _to_logical(bm, phys):
  return sum(1 << l for l, p in enumerate(bm) if (phys >> p) & 1)


def _dry_pair(nloc, bw, swaps_a, swaps_b, nglob=None, shard=1):
  a, b = device.DeviceState(nloc, bw, dry=True), device.DeviceState(nloc, bw, dry=True)
  if nglob:
    a.set_shard(nglob, shard)
    b.set_shard(nglob, shard)
  for st, swaps in ((a, swaps_a), (b, swaps_b)):
    for x, y in swaps:
      st.remap_swap(x, y)
  return a, b


def _check_plan(a, b, nloc, nglob, bw, xs, zs, shard=0):
  terms, passes = a.transition_plan(b, xs, zs)
  bma, bmb = _bitmap(a, nglob), _bitmap(b, nglob)
  batch = native.QH_TRANSITION_BATCH if bw == 128 else native.QH_TRANSITION_BATCH // 2
  local = (1 << nloc) - 1
  held = _to_logical(bma, ((1 << nglob) - 1) & ~local)
  assert sorted(t['index'] for t in terms) == list(range(len(xs)))                    # every term once
  for t in terms:
    x, z = xs[t['index']], zs[t['index']]
    assert t['px'] <= local and t['pz'] <= local
    assert _to_logical(bmb, t['px']) == x                                               # px in B's positions
    assert _to_logical(bma, t['pz']) == z & ~held                                       # pz in A's positions
    ones = sum(1 for l in range(nglob) if (z >> l) & 1 and bma[l] >= nloc and (shard >> (bma[l] - nloc)) & 1)
    assert t['neg'] == ones % 2
    assert t['ny'] == bin(x & z).count('1') % 4
  keys = [(xs[t['index']], t['index']) for t in terms]
  assert keys == sorted(keys)                                                            # stably sorted by logical x
  counts = {}
  for x in xs:
    counts[x] = counts.get(x, 0) + 1
  assert len(passes) == sum(-(-c // batch) for c in counts.values())
  at = 0
  walk = a.inner_plan(b)['path']
  for p in passes:
    assert p['first'] == at and 1 <= p['count'] <= batch
    assert all(terms[k]['px'] == p['px'] for k in range(at, at + p['count']))
    assert p['walk'] == walk
    at += p['count']
  assert at == len(xs)
  return terms, passes


@pytest.mark.parametrize('bw', [128, 64])
@pytest.mark.parametrize('nloc', [10, 11, 12])
def test_plan_on_changed_bit_maps(nloc, bw):
  rng = np.random.default_rng(nloc * 1000 + bw)
  T = native.QH_TRANSITION_BATCH
  for swaps_a, swaps_b, walk in (([], [], native.QH_INNER_LINEAR), ([(0, 7), (3, 9)], [(0, 7), (3, 9)], native.QH_INNER_LINEAR),
                                 ([], [(0, nloc - 1), (2, 5)], native.QH_INNER_TILES), ([(1, 8), (4, 6)], [(9, 2)], native.QH_INNER_TILES)):
    a, b = _dry_pair(nloc, bw, swaps_a, swaps_b)
    try:
      assert a.inner_plan(b)['path'] == walk
      xmasks = [int(v) for v in rng.integers(0, 1 << nloc, size=5)] + [0]
      xs = [xmasks[int(k)] for k in rng.integers(0, len(xmasks), size=2 * T + 9)] + [xmasks[0]] * (T + 1)
      zs = [int(v) for v in rng.integers(0, 1 << nloc, size=len(xs))]
      _terms, passes = _check_plan(a, b, nloc, nloc, bw, xs, zs)
      assert max(p['count'] for p in passes) == (T if bw == 128 else T // 2)           # a group larger than the batch is cut at it
      _check_plan(b, a, nloc, nloc, bw, xs, zs)
      assert a.transition_plan(b, [], []) == ([], [])
    finally:
      a.close()
      b.close()


def test_plan_shard_bits():
  lib = native.load()
  nloc, nglob = 10, 12
  npass = ctypes.c_uint64()
  passes = (native.QhTransitionPass * 8)()
  for shard in range(4):
    a, b = _dry_pair(nloc, 128, [(1, 11)], [(1, 11), (2, 7)], nglob=nglob, shard=shard)      # logical bits 1 and 10 in the shard index
    try:
      xs = [0, 1 << 3, 1 << 3, (1 << 0) | (1 << 9)]
      zs = [1 << 1, (1 << 10) | (1 << 3), (1 << 1) | (1 << 10), (1 << 1) | (1 << 5)]
      terms, _passes = _check_plan(a, b, nloc, nglob, 128, xs, zs, shard=shard)
      by_index = {t['index']: t for t in terms}
      # logical bit 1 sits at physical 11 (shard bit 1), logical 10 at physical 10 (shard bit 0)
      assert [by_index[k]['neg'] for k in range(4)] == [(shard >> 1) & 1, shard & 1, ((shard >> 1) ^ shard) & 1, (shard >> 1) & 1]
      (_x, xp), (_z, zp) = _u64([1 << 3, 1 << 10]), _u64([0, 0])
      assert lib.qh_transition_plan(a.h, b.h, 2, xp, zp, None, passes, 8, ctypes.byref(npass)) == native.QH_ERR_NONLOCAL     # x on a shard bit
      assert b'term 1 has X or Y on logical bit 10' in lib.qh_last_error()
      out = (ctypes.c_double * 4)(7.0, 7.0, 7.0, 7.0)
      assert lib.qh_transition_pauli(a.h, b.h, 2, xp, zp, out) == native.QH_ERR_ARG       # (dry: the refusal that comes first)
      b.set_shard(nglob, shard ^ 1)
      (_x, xp), (_z, zp) = _u64([1 << 3]), _u64([0])
      assert lib.qh_transition_plan(a.h, b.h, 1, xp, zp, None, passes, 8, ctypes.byref(npass)) == native.QH_ERR_NONLOCAL     # another shard
      assert b'exchange first' in lib.qh_last_error()
      b.set_shard(nglob, shard)
      b.remap_swap(3, 10)                                                   # b now holds another logical bit in the shard index
      assert lib.qh_transition_plan(a.h, b.h, 1, xp, zp, None, passes, 8, ctypes.byref(npass)) == native.QH_ERR_NONLOCAL
      assert b'exchange first' in lib.qh_last_error()
      assert list(out) == [7.0] * 4
    finally:
      a.close()
      b.close()


def test_plan_check_stand_alone():
  """tools/transition_plan_check.cc is plain C++ over transition_plan.h with its own main: random bit maps for a and b, random
  term lists, shard bits; every term in one pass, masks mapped back through the two bit maps, the walks' index and sign
  arithmetic at every amplitude, the refusals.  A plain build; nothing is loaded into this process."""
  cxx = shutil.which('g++')
  assert cxx, 'no g++'
  with tempfile.TemporaryDirectory() as tmp:
    exe = os.path.join(tmp, 'transition_plan_check')
    subprocess.check_call([cxx, '-std=c++17', '-O2', os.path.join(ROOT, 'tools', 'transition_plan_check.cc'), '-o', exe])
    res = subprocess.run([exe, '12'], capture_output=True, text=True, timeout=120)
  assert res.returncode == 0, res.stdout + res.stderr
  assert 'ok' in res.stdout


# ---- qc on NumPy devices -------------------------------------------------------------------------------------------------
class TransitionOracle(fake_device.OracleDevice):
  """OracleDevice with the two-state and Pauli calls qc.matrix_element and qc.rotation_gradients use, in NumPy (logical order
  = the array's order)."""
  reads = 0
  live = 0

  def __init__(self, nbits, bit_width):
    super().__init__(nbits, bit_width)
    TransitionOracle.live += 1
    self.closed = False

  def close(self):
    if not self.closed:
      TransitionOracle.live -= 1
      self.closed = True

  def _like(self, amps):
    new = TransitionOracle(self.nbits, self.bit_width)
    new.psi[:] = np.asarray(amps).astype(self.dtype)
    return new

  def clone(self):
    return self._like(self.psi)

  def transition_pauli(self, other, xmasks, zmasks):
    TransitionOracle.reads += 1
    return np.array([tu.np_transition(self.psi, other.psi, x, z) for x, z in zip(xmasks, zmasks)], dtype=np.complex128)

  def apply_pauli_sum(self, coeffs, xmasks, zmasks, out=None, norm=False):
    assert out is None and not norm
    v = np.zeros(self.psi.size, dtype=np.complex128)
    for c, x, z in zip(coeffs, xmasks, zmasks):
      v += complex(c) * tu.np_pauli(self.psi, x, z)
    return self._like(v)

  def apply_pauli_product(self, a, b, xmasks, zmasks, norm=False):
    v = self.psi.astype(np.complex128)
    for at, bt, x, z in zip(a, b, xmasks, zmasks):
      v = complex(at) * v + complex(bt) * tu.np_pauli(v, x, z)
    self.psi[:] = v.astype(self.dtype)
    return float(np.vdot(self.psi, self.psi).real) if norm else None


class ComposeOracle(fake_device.OracleDevice):
  """... with inner and apply_pauli_sum only: matrix_element composes them"""
  sums = 0

  def inner(self, other):
    return complex(np.vdot(self.psi, other.psi))

  def apply_pauli_sum(self, coeffs, xmasks, zmasks, out=None, norm=False):
    ComposeOracle.sums += 1
    new = ComposeOracle(self.nbits, self.bit_width)
    for c, x, z in zip(coeffs, xmasks, zmasks):
      new.psi += (complex(c) * tu.np_pauli(self.psi, x, z)).astype(self.dtype)
    return new


FACTORIES = {'transition_pauli': TransitionOracle, 'composed': ComposeOracle, 'fallback': fake_device.OracleDevice}


@pytest.fixture(params=['transition_pauli', 'composed', 'fallback'])
def cpu_backend(request):
  tensor.set_tensor_width(128)
  backend.set_device_factory(FACTORIES[request.param])
  yield request.param
  backend.set_device_factory(None)
  tensor.set_tensor_width(None)


def _circuit(nq, seed, depth=3):
  rng = np.random.default_rng(seed)
  q = circuit.qc('c')
  q.reg(nq, 0)
  for _ in range(depth):
    for i in range(nq):
      q.h(i) if rng.random() < 0.5 else q.ry(i, float(rng.uniform(0, 3)))
    for i in range(nq - 1):
      q.cu1(i, i + 1, float(rng.uniform(0, 3)))
    q.cx(int(rng.integers(1, nq)), 0)
  return q


def _amps(q):
  return np.asarray(q.psi, dtype=np.complex128).reshape(-1)


def test_matrix_element_all_strings_on_three_qubits(cpu_backend):
  a, b = _circuit(3, 1), _circuit(3, 2)
  pa, pb = _amps(a), _amps(b)
  strings = [''.join(s) for s in itertools.product('IXYZ', repeat=3)]
  TransitionOracle.reads = ComposeOracle.sums = 0
  got = a.matrix_element(b, [(1.0, s) for s in strings], per_term=True)
  if cpu_backend == 'transition_pauli':
    assert TransitionOracle.reads == 1                                       # one device call for the whole list
  elif cpu_backend == 'composed':
    assert ComposeOracle.sums == 64
  assert got.dtype == np.complex128 and got.shape == (64,)
  for s, v in zip(strings, got):
    assert abs(v - np.vdot(pa, tu.kron_pauli(s) @ pb)) < 1e-14, s
  rng = np.random.default_rng(3)
  coeffs = rng.normal(size=64) + 1j * rng.normal(size=64)
  total = a.matrix_element(b, list(zip(coeffs, strings)))
  assert isinstance(total, complex) and abs(total - np.dot(coeffs, got)) < 1e-13


def test_matrix_element_properties_and_forms(cpu_backend):
  a, b = _circuit(4, 5), _circuit(4, 6)
  pa, pb = _amps(a), _amps(b)
  ham = [(0.7, 'XXII'), (-1.3, 'IZZI'), (0.4, 'YIIY'), (2.0, 'IIII'), (0.9, 'ZXYI')]
  # other is self: the real part is the expectation value
  self_me = a.matrix_element(a, ham)
  assert abs(self_me.real - a.expectation(ham)) < 1e-13 and abs(self_me.imag) < 1e-13
  per = a.matrix_element(a, ham, per_term=True)
  assert np.allclose(per.real, a.expectation(ham, per_term=True), atol=1e-13, rtol=0)
  # Hermitian H: <a|H|b> = conj(<b|H|a>)
  ab, ba = a.matrix_element(b, ham), b.matrix_element(a, ham)
  assert abs(ab - np.conj(ba)) < 1e-13
  m = sum(c * tu.kron_pauli(s) for c, s in ham)
  assert abs(ab - np.vdot(pa, m @ pb)) < 1e-13
  # str, dict and lower-case forms of one string
  want = np.vdot(pa, tu.kron_pauli('IXZY') @ pb)
  for form in ('IXZY', 'ixzy', {1: 'X', 2: 'Z', 3: 'Y'}, {1: 'x', 2: 'z', 3: 'y', 0: 'I'}):
    assert abs(a.matrix_element(b, [(1.0, form)]) - want) < 1e-14
  assert a.matrix_element(b, []) == 0j and isinstance(a.matrix_element(b, []), complex)
  assert a.matrix_element(b, [], per_term=True).shape == (0,)
  # against a Snapshot
  with b.snapshot() as snap:
    b.h(0)
    assert abs(a.matrix_element(snap, [(1.0, 'IXZY')]) - want) < 1e-14
  with pytest.raises(ValueError):
    a.matrix_element(snap, ham)                                              # closed
  with pytest.raises(ValueError):
    a.matrix_element(_circuit(3, 1), [(1.0, 'XII')])                         # another size
  with pytest.raises(ValueError):
    a.matrix_element(pb, ham)
  with pytest.raises(ValueError):
    a.matrix_element(b, [(1.0, 'XX')])                                       # a string of the wrong length
  with pytest.raises(ValueError):
    a.matrix_element(b, [(1.0, {0: 'Q'})])
  tensor.set_tensor_width(64)
  try:
    snap64 = _circuit(4, 7).snapshot()                                       # (a circuit's width is the global one: a snapshot keeps its own)
  finally:
    tensor.set_tensor_width(128)
  assert snap64.width == 64
  with pytest.raises(ValueError):
    a.matrix_element(snap64, ham)                                            # another width


ROTATIONS = {
    4: ['XIIZ', 'IYYI', 'ZZII', 'XIIZ', 'IIII', 'IXYZ', 'YIIX'],
    5: ['XIIZI', 'IYYII', 'ZZIIZ', 'XIIZI', 'IIIII', 'IXYZI', 'YIIXX', 'IYYII', 'ZIIII'],
    6: ['XIIZII', 'IYYIIX', 'ZZIIZI', 'XIIZII', 'IIIIII', 'IXYZIY', 'YIIXXI', 'IYYIIX', 'ZIIIII', 'IIXIII'],
}


def _hamiltonian(nq):
  ham = [(-1.0, {q: 'Z', q + 1: 'Z'}) for q in range(nq - 1)] + [(-0.6, {q: 'X'}) for q in range(nq)]
  return ham + [(0.3, {0: 'Y', nq - 1: 'Y'}), (0.25, 'I' * nq)]


@pytest.fixture(params=['transition_pauli', 'fallback'])
def grad_backend(request):
  """the two paths of rotation_gradients: the device calls, and the NumPy loop over qc.psi"""
  tensor.set_tensor_width(128)
  backend.set_device_factory(FACTORIES[request.param])
  yield request.param
  backend.set_device_factory(None)
  tensor.set_tensor_width(None)


@pytest.mark.parametrize('nq', [4, 5, 6])
def test_rotation_gradients_against_parameter_shift(grad_backend, nq):
  cpu_backend = grad_backend
  rots = ROTATIONS[nq]
  assert 6 <= len(rots) <= 10 and len(set(rots)) < len(rots) and 'I' * nq in rots
  thetas = [float(t) for t in np.random.default_rng(40 + nq).uniform(-3, 3, size=len(rots))]
  ham = _hamiltonian(nq)

  def rotated(angles):
    q = _circuit(nq, 9, depth=2)
    for s, t in zip(rots, angles):
      q.pauli_rot(s, t)
    return q

  q = _circuit(nq, 9, depth=2)
  q._ensure_device()                                                        # (made on first use)
  live = TransitionOracle.live
  energy, grad = q.rotation_gradients(list(zip(rots, thetas)), ham)
  assert TransitionOracle.live == live                                      # the two scratch states are closed
  ref = rotated(thetas)
  assert isinstance(energy, float) and grad.dtype == np.float64 and grad.shape == (len(rots),)
  assert energy == q.expectation(ham) and abs(energy - ref.expectation(ham)) < 1e-13
  assert np.array_equal(_amps(q), _amps(ref))                               # left in the rotated state, as pauli_rot leaves it
  want = tu.parameter_shift(lambda angles: rotated(angles).expectation(ham), thetas)
  print(f'{cpu_backend} {nq} qubits: max |adjoint - parameter shift| = {np.max(np.abs(grad - want)):.3e}')
  assert np.max(np.abs(grad - want)) < 1e-12
  assert abs(grad[rots.index('I' * nq)]) < 1e-15                            # a global phase
  # an unnormalised state: the gradient is quadratic in the amplitudes
  q2 = _circuit(nq, 9, depth=2)
  q2.psi = np.asarray(q2.psi).reshape(-1) * 2
  energy2, grad2 = q2.rotation_gradients(list(zip(rots, thetas)), ham)
  assert abs(energy2 - 4 * energy) < 1e-12 and np.max(np.abs(grad2 - 4 * grad)) < 1e-12
  with pytest.raises(ValueError):
    q.rotation_gradients([(rots[0], 0.1)], [(1j, rots[1])])                  # complex coefficients
  with pytest.raises(ValueError):
    q.rotation_gradients([rots[0]], ham)                                     # not a (paulis, theta) pair
  assert q.rotation_gradients([], ham)[1].shape == (0,)


def test_rotation_gradients_closes_its_scratch_on_an_error(monkeypatch):
  tensor.set_tensor_width(128)
  backend.set_device_factory(TransitionOracle)
  try:
    q = _circuit(4, 2)
    q._ensure_device()
    live = TransitionOracle.live

    def boom(*_a, **_k):
      raise RuntimeError('boom')
    monkeypatch.setattr(TransitionOracle, 'transition_pauli', boom)
    with pytest.raises(RuntimeError):
      q.rotation_gradients([('XIIZ', 0.3)], _hamiltonian(4))
    assert TransitionOracle.live == live
  finally:
    backend.set_device_factory(None)
    tensor.set_tensor_width(None)
