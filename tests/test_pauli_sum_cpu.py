"""CPU tests of the Pauli-sum operators: the C-ABI symbols and their argument checks on planner-only handles,
qh_pauli_sum_plan's batches, qc.apply_hamiltonian / hamiltonian_times / variance with the GPU replaced by a NumPy stand-in
that implements apply_pauli_sum and over the fallback that reads qc.psi, and tools/pauli_plan_check.cc stand-alone.

The reference value everywhere is pauli_util.np_pauli_sum: NumPy in complex128 on the amplitudes as stored,
(P a)_i = (-i)^nY (-1)^popcount(i & z) a_{i ^ x}; it is cross-checked once against np.kron of qcc_amd.lib.ops Paulis."""
import ctypes
import functools
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

from qcc_amd import device, native
from qcc_amd.lib import backend, circuit, ops, tensor
from tests import fake_device, pauli_util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_dp = ctypes.POINTER(ctypes.c_double)
_up = ctypes.POINTER(ctypes.c_uint64)


class PauliOracle(fake_device.OracleDevice):
  """OracleDevice with apply_pauli_sum in NumPy (logical order = the array's order)."""
  applied = 0

  def apply_pauli_sum(self, coeffs, xmasks, zmasks, out=None, norm=False):
    PauliOracle.applied += 1
    new = PauliOracle(self.nbits, self.bit_width) if out is None else out
    new.psi[:] = pauli_util.np_pauli_sum(self.psi, coeffs, xmasks, zmasks).astype(self.dtype)
    n2 = float(np.vdot(new.psi.astype(np.complex128), new.psi.astype(np.complex128)).real)
    return (new, n2) if norm else new


def kron_matrix(terms, n):
  """sum_t c_t P_t as a dense matrix: np.kron of qcc_amd.lib.ops Paulis, letter q of a string on qubit q"""
  mats = {'I': np.eye(2, dtype=np.complex128), 'X': np.asarray(ops.PauliX(), dtype=np.complex128),
          'Y': np.asarray(ops.PauliY(), dtype=np.complex128), 'Z': np.asarray(ops.PauliZ(), dtype=np.complex128)}
  return sum(c * functools.reduce(np.kron, [mats[ch] for ch in s]) for c, s in terms) + np.zeros((1 << n, 1 << n))


def string_masks(s):
  n = len(s)
  x = sum(1 << (n - 1 - q) for q, ch in enumerate(s) if ch in 'XY')
  z = sum(1 << (n - 1 - q) for q, ch in enumerate(s) if ch in 'ZY')
  return x, z


def test_reference_formula_against_kron():
  """The formula every other test trusts, once against the dense matrices at 6 qubits: every single-qubit Pauli on every
  qubit, and random strings with complex coefficients."""
  rng = np.random.default_rng(6)
  n = 6
  psi = rng.normal(size=1 << n) + 1j * rng.normal(size=1 << n)
  strings = [''.join('I' * q + p + 'I' * (n - 1 - q)) for q in range(n) for p in 'XYZ']
  strings += [''.join(rng.choice(list('IXYZ'), size=n)) for _ in range(20)]
  for s in strings:
    x, z = string_masks(s)
    np.testing.assert_allclose(pauli_util.np_pauli_sum(psi, [1.0], [x], [z]), kron_matrix([(1.0, s)], n) @ psi, atol=1e-13, err_msg=s)
  terms = [(complex(rng.normal(), rng.normal()), s) for s in strings]
  xs, zs = zip(*[string_masks(s) for _, s in terms])
  np.testing.assert_allclose(pauli_util.np_pauli_sum(psi, [c for c, _ in terms], xs, zs), kron_matrix(terms, n) @ psi, atol=1e-11)
  y = pauli_util.np_pauli_sum(np.array([2.0, 3.0]), [1.0], [1], [1])      # (Ya)_0 = -i a_1, (Ya)_1 = i a_0
  assert y[0] == -3j and y[1] == 2j


# ---- the C-ABI ---------------------------------------------------------------------------------------------------------
def test_version_and_symbols_bound():
  lib = native.load()
  assert lib.qh_version() >= 115
  for name in ('qh_apply_pauli_sum', 'qh_pauli_sum_new', 'qh_pauli_sum_plan'):
    assert name in native.SIGNATURES
    assert getattr(lib, name).argtypes == native.SIGNATURES[name][1]
  assert native.QH_PAULI_SUM_BATCH == 16
  assert ctypes.sizeof(native.QhPauliTerm) == 32 and ctypes.sizeof(native.QhPauliBatch) == 32


def _dry(n, bw=128, nglob=None, shard=0):
  st = device.DeviceState(n, bw, dry=True)
  if nglob is not None:
    st.set_shard(nglob, shard)
  return st


def test_apply_argument_errors():
  lib = native.load()
  a, b, c64, small = _dry(10), _dry(10), _dry(10, 64), _dry(9)
  sh0, sh1 = _dry(10, nglob=12, shard=1), _dry(10, nglob=12, shard=2)
  try:
    n2 = ctypes.c_double(7.0)

    def call(dst, src, xs, zs, cp=True, xp=True, zp=True, n=None):
      x, z = np.asarray(xs, dtype=np.uint64), np.asarray(zs, dtype=np.uint64)
      co = np.ones(2 * max(x.size, 1))
      return lib.qh_apply_pauli_sum(dst.h if dst else None, src.h if src else None, x.size if n is None else n,
                                    co.ctypes.data_as(_dp) if cp else None, x.ctypes.data_as(_up) if xp else None,
                                    z.ctypes.data_as(_up) if zp else None, ctypes.byref(n2))
    assert call(None, a, [1], [0]) == native.QH_ERR_ARG
    assert call(a, None, [1], [0]) == native.QH_ERR_ARG
    assert call(a, b, [1], [0]) == native.QH_ERR_ARG                  # dry handles hold no state
    assert b'dry' in lib.qh_last_error()
    assert call(a, a, [1], [0]) == native.QH_ERR_ARG
    assert call(a, c64, [1], [0]) == native.QH_ERR_ARG
    assert call(a, small, [1], [0]) == native.QH_ERR_ARG
    assert call(sh0, sh1, [1], [0]) == native.QH_ERR_ARG
    assert n2.value == 7.0
    # qh_pauli_sum_new: the same checks, nothing is created
    out = ctypes.c_void_p()
    co, x, z = np.ones(2), np.array([1], dtype=np.uint64), np.array([0], dtype=np.uint64)
    args = (co.ctypes.data_as(_dp), x.ctypes.data_as(_up), z.ctypes.data_as(_up), ctypes.byref(n2))
    assert lib.qh_pauli_sum_new(None, 1, *args, ctypes.byref(out)) == native.QH_ERR_ARG
    assert lib.qh_pauli_sum_new(a.h, 1, *args, None) == native.QH_ERR_ARG
    assert lib.qh_pauli_sum_new(a.h, 1, *args, ctypes.byref(out)) == native.QH_ERR_ARG      # dry
    assert lib.qh_pauli_sum_new(a.h, 1, None, *args[1:], ctypes.byref(out)) == native.QH_ERR_ARG
    assert out.value is None and n2.value == 7.0
  finally:
    for st in (a, b, c64, small, sh0, sh1):
      st.close()


def _plan_rc(st, xs, zs, xp=True, zp=True, nbp=True, cap=8, bp=True):
  lib = native.load()
  x, z = np.asarray(xs, dtype=np.uint64), np.asarray(zs, dtype=np.uint64)
  batches = (native.QhPauliBatch * max(cap, 1))()
  nb = ctypes.c_uint64(99)
  rc = lib.qh_pauli_sum_plan(st.h if st else None, x.size, x.ctypes.data_as(_up) if xp else None, z.ctypes.data_as(_up) if zp else None,
                             None, batches if bp else None, cap, ctypes.byref(nb) if nbp else None)
  return rc, nb.value


def test_plan_argument_errors_on_planner_only_handles():
  """qh_pauli_sum_plan makes every check of qh_apply_pauli_sum that needs no state, on planner-only handles: null pointers,
  mask bits at or above nbits_global, and X or Y on a bit the shard index holds."""
  st, sh = _dry(10), _dry(10, nglob=12, shard=2)
  try:
    assert _plan_rc(None, [1], [0])[0] == native.QH_ERR_ARG
    assert _plan_rc(st, [1], [0], xp=False)[0] == native.QH_ERR_ARG
    assert _plan_rc(st, [1], [0], zp=False)[0] == native.QH_ERR_ARG
    assert _plan_rc(st, [1], [0], nbp=False)[0] == native.QH_ERR_ARG
    assert _plan_rc(st, [1], [0], bp=False)[0] == native.QH_ERR_ARG
    assert _plan_rc(st, [1], [0], bp=False, cap=0) == (native.QH_OK, 1)            # the count-only form
    assert _plan_rc(st, [1, 1 << 10], [0, 0])[0] == native.QH_ERR_BAD_QUBIT
    assert _plan_rc(st, [1, 2], [0, 1 << 63])[0] == native.QH_ERR_BAD_QUBIT
    assert _plan_rc(sh, [1], [1 << 12])[0] == native.QH_ERR_BAD_QUBIT
    assert _plan_rc(sh, [1, 1 << 11], [0, 0])[0] == native.QH_ERR_NONLOCAL        # x on a bit held by the shard index
    assert b'shard index' in native.load().qh_last_error()
    assert _plan_rc(sh, [1, 3], [1 << 11, 1 << 10]) == (native.QH_OK, 1)          # z there is a sign
    sh.remap_swap(11, 0)                                                           # logical 0 is now held, logical 11 local
    assert _plan_rc(sh, [1 << 11], [0]) == (native.QH_OK, 1)
    assert _plan_rc(sh, [1], [0])[0] == native.QH_ERR_NONLOCAL
    assert _plan_rc(st, [], [], xp=False, zp=False) == (native.QH_OK, 0)           # nterms == 0: no batch (one kernel of zeros)
  finally:
    st.close()
    sh.close()


def test_plan_batches_groups_and_streams():
  """Hand-made term lists: the stable sort by physical x mask, the cut every 16 terms, the distinct x masks per batch and
  streams = groups + 1 + [b > 0]."""
  st = _dry(12)
  try:
    terms, batches = st.pauli_sum_plan([5, 0, 5, 0, 9], [1, 2, 3, 4, 5])
    assert [t['index'] for t in terms] == [1, 3, 0, 2, 4]                          # stable
    assert [t['px'] for t in terms] == [0, 0, 5, 5, 9] and [t['pz'] for t in terms] == [2, 4, 1, 3, 5]
    assert [t['ny'] for t in terms] == [0, 0, 1, 1, 1] and all(t['neg'] == 0 for t in terms)
    assert batches == [dict(first=0, count=5, ngroups=3, streams=4)]
    for n, nx, want in [(1, 1, [(1, 1, 2)]), (4, 1, [(4, 1, 2)]), (16, 1, [(16, 1, 2)]), (17, 1, [(16, 1, 2), (1, 1, 3)]),
                        (17, 3, [(16, 3, 4), (1, 1, 3)]), (40, 3, [(16, 2, 3), (16, 2, 4), (8, 1, 3)]),
                        (40, 20, [(16, 8, 9), (16, 8, 10), (8, 4, 6)]), (32, 32, [(16, 16, 17), (16, 16, 18)])]:
      xs = [(k * nx) // n + 1 for k in range(n)]                                   # nx distinct masks in equal runs
      _, batches = st.pauli_sum_plan(xs, [7] * n)
      assert [(b['count'], b['ngroups'], b['streams']) for b in batches] == want, (n, nx)
      assert [b['first'] for b in batches] == [16 * k for k in range(len(batches))]
    # a group split by the cut counts in both batches
    _, batches = st.pauli_sum_plan([1] * 10 + [2] * 10, [0] * 20)
    assert [(b['count'], b['ngroups']) for b in batches] == [(16, 2), (4, 1)]
    # cap smaller than the number of batches: *nbatches still says how many
    assert _plan_rc(st, list(range(40)), [0] * 40, cap=1) == (native.QH_OK, 3)
    # after qh_remap_swap the masks are physical
    st.remap_swap(0, 11)
    st.remap_swap(3, 4)
    terms, _ = st.pauli_sum_plan([1, 1 << 3, 1 << 11], [1 << 4, 1, 9])
    by_index = {t['index']: t for t in terms}
    assert by_index[0]['px'] == 1 << 11 and by_index[0]['pz'] == 1 << 3
    assert by_index[1]['px'] == 1 << 4 and by_index[1]['pz'] == 1 << 11
    assert by_index[2]['px'] == 1 and by_index[2]['pz'] == (1 << 11) | (1 << 4)
    assert [t['index'] for t in terms] == [2, 1, 0]                                # sorted by the PHYSICAL mask
  finally:
    st.close()


def test_plan_on_a_shard_handle():
  """A z bit held by the shard index is the sign `neg`, as it is on this shard; the local part of the masks remains."""
  for shard, negs in [(0, [0, 0, 0]), (1, [1, 0, 1]), (2, [0, 1, 1]), (3, [1, 1, 0])]:
    sh = _dry(10, nglob=12, shard=shard)
    try:
      terms, batches = sh.pauli_sum_plan([3, 3, 3], [(1 << 10) | 1, (1 << 11) | 2, (3 << 10) | 4])
      assert [t['neg'] for t in terms] == negs
      assert [t['pz'] for t in terms] == [1, 2, 4] and [t['px'] for t in terms] == [3, 3, 3]
      assert batches == [dict(first=0, count=3, ngroups=1, streams=2)]
    finally:
      sh.close()


def test_plan_check_stand_alone(tmp_path):
  """tools/pauli_plan_check.cc is plain C++ over pauli_plan.h: random masks on random bit maps of 10 to 14 local bits, the
  split signs and the partner address at every index.  Built without a sanitizer here (the tool's header has the sanitizer
  command line); nothing is loaded into this process."""
  cxx = shutil.which('g++') or shutil.which('clang++')
  assert cxx, 'no host C++ compiler'
  exe = str(tmp_path / 'pauli_plan_check')
  subprocess.check_call([cxx, '-std=c++17', '-O1', os.path.join(ROOT, 'tools', 'pauli_plan_check.cc'), '-o', exe])
  res = subprocess.run([exe, '4'], capture_output=True, text=True, timeout=120)
  assert res.returncode == 0, res.stdout + res.stderr
  assert 'ok' in res.stdout


# ---- qc on NumPy devices -------------------------------------------------------------------------------------------------
@pytest.fixture(params=[('apply_pauli_sum', 128), ('apply_pauli_sum', 64), ('fallback', 128), ('fallback', 64)], ids=lambda p: f'{p[0]}-{p[1]}')
def cpu_backend(request):
  kind, width = request.param
  tensor.set_tensor_width(width)
  backend.set_device_factory(PauliOracle if kind == 'apply_pauli_sum' else fake_device.OracleDevice)
  yield kind, width
  backend.set_device_factory(None)
  tensor.set_tensor_width(None)


def _circuit(nq, seed):
  rng = np.random.default_rng(seed)
  q = circuit.qc('p')
  q.reg(nq, 0)
  for _ in range(3 * nq):
    a = int(rng.integers(nq))
    q.ry(a, float(rng.random() * 3))
    b = int(rng.integers(nq))
    if b != a:
      q.cx(a, b)
    q.rz(int(rng.integers(nq)), float(rng.random() * 3))
  return q


def _random_terms(rng, n, count, real=False):
  out = []
  for _ in range(count):
    c = float(rng.normal()) if real else complex(rng.normal(), rng.normal())
    out.append((c, ''.join(rng.choice(list('IXYZ'), size=n))))
  return out


def _want(psi, terms):
  xs, zs = zip(*[string_masks(s) for _, s in terms]) if terms else ((), ())
  return pauli_util.np_pauli_sum(psi, [c for c, _ in terms], xs, zs)


def _tol(width, terms, psi):
  return pauli_util.bound(width, [c for c, _ in terms], float(np.max(np.abs(psi))))


def test_hamiltonian_times_leaves_self_and_feeds_the_two_state_calls(cpu_backend):
  kind, width = cpu_backend
  rng = np.random.default_rng(11)
  for n in (1, 3, 6):
    q = _circuit(n, 20 + n)
    psi = np.asarray(q.psi).copy()
    terms = _random_terms(rng, n, 7)
    applied = PauliOracle.applied
    w = q.hamiltonian_times(terms)
    if kind == 'apply_pauli_sum':
      assert PauliOracle.applied == applied + 1              # one device call for the whole operator
    assert isinstance(w, circuit.Snapshot) and w.nbits == n and w.width == width
    assert np.array_equal(np.asarray(q.psi), psi)           # self unchanged
    want = _want(psi, terms)
    tol = _tol(width, terms, psi)
    got = w._dev.download() if w._dev is not None else w._host      # pylint: disable=protected-access
    assert got.dtype == psi.dtype and np.max(np.abs(got - want)) <= tol
    stored = np.asarray(got).astype(np.complex128)
    assert abs(q.overlap(w) - np.vdot(psi.astype(np.complex128), stored)) <= 4 * (1 << n) * tol * max(1.0, float(np.max(np.abs(psi))))
    # combine, project_out and restore take it like any snapshot
    q2 = _circuit(n, 20 + n)
    q2.combine(w, 1.0, -0.5)
    np.testing.assert_allclose(np.asarray(q2.psi), psi.astype(np.complex128) - 0.5 * stored, atol=10 * tol + 1e-6 * (width == 64))
    q3 = _circuit(n, 20 + n)
    if float(np.vdot(stored, stored).real) > 0:
      q3.project_out(w)
      assert abs(q3.overlap(w)) <= 1e-5 if width == 64 else abs(q3.overlap(w)) <= 1e-12
    q3.restore(w)
    assert np.array_equal(np.asarray(q3.psi), got)
    w.close()


def test_apply_hamiltonian_replaces_the_state(cpu_backend):
  _kind, width = cpu_backend
  rng = np.random.default_rng(12)
  for n in (2, 5):
    q = _circuit(n, 30 + n)
    psi = np.asarray(q.psi).copy()
    terms = _random_terms(rng, n, 19)                        # more than one batch on a device
    norm2 = q.apply_hamiltonian(terms)
    want = _want(psi, terms)
    got = np.asarray(q.psi)
    tol = _tol(width, terms, psi)
    assert got.dtype == psi.dtype and np.max(np.abs(got - want)) <= tol
    n2 = float(np.vdot(got.astype(np.complex128), got.astype(np.complex128)).real)
    assert isinstance(norm2, float) and abs(norm2 - n2) <= 1e-12 * max(1.0, n2)      # of the values as stored
    # dict terms, and gates afterwards act on the new state
    q.h(0)
    ref = circuit.qc('r')
    ref.reg(n, 0)
    ref.psi = got
    ref.h(0)
    np.testing.assert_allclose(np.asarray(q.psi), np.asarray(ref.psi), atol=1e-6 if width == 64 else 1e-13)
  # normalize
  q = _circuit(4, 5)
  psi = np.asarray(q.psi).copy()
  terms = [(1.0, 'XIII'), (0.5, {1: 'Z', 2: 'z'}), (-0.25, {3: 'Y'})]
  strs = [(1.0, 'XIII'), (0.5, 'IZZI'), (-0.25, 'IIIY')]
  norm2 = q.apply_hamiltonian(terms, normalize=True)
  want = _want(psi, strs)
  assert abs(norm2 - float(np.vdot(want, want).real)) <= 1e-5 * norm2
  np.testing.assert_allclose(np.asarray(q.psi), want / np.sqrt(norm2), atol=1e-6 if width == 64 else 1e-13)
  assert abs(q.norm2() - 1.0) <= (1e-6 if width == 64 else 1e-13)
  # H psi == 0: the state is that result and ValueError says so
  q = _circuit(3, 6)
  with pytest.raises(ValueError, match='nothing to normalise'):
    q.apply_hamiltonian([(1.0, 'ZII'), (-1.0, 'ZII')], normalize=True)
  assert not np.any(np.asarray(q.psi))
  q = _circuit(3, 6)
  assert q.apply_hamiltonian([]) == 0.0 and not np.any(np.asarray(q.psi))      # the empty sum is the zero operator


def test_variance(cpu_backend):
  _kind, width = cpu_backend
  rng = np.random.default_rng(13)
  for n in (2, 6):
    q = _circuit(n, 40 + n)
    psi = np.asarray(q.psi).copy()
    terms = _random_terms(rng, n, 9, real=True)
    a = psi.astype(np.complex128)
    m = kron_matrix(terms, n)
    want = float(np.vdot(m @ a, m @ a).real) - float(np.vdot(a, m @ a).real) ** 2
    got = q.variance(terms)
    assert isinstance(got, float) and abs(got - want) <= (2e-5 if width == 64 else 1e-11) * max(1.0, abs(want))
    assert np.array_equal(np.asarray(q.psi), psi)
    assert abs(q.variance(iter(terms)) - got) == 0.0         # any iterable, once
  # an eigenstate has none
  q = circuit.qc('z')
  q.reg(3, 0)
  q.x(1)
  assert abs(q.variance([(2.0, 'ZZI'), (0.5, 'IIZ')])) <= 1e-12
  with pytest.raises(ValueError, match='real coefficients'):
    q.variance([(1j, 'ZII')])


def test_argument_errors(cpu_backend):
  q = _circuit(4, 2)
  psi = np.asarray(q.psi).copy()
  for method in (q.apply_hamiltonian, q.hamiltonian_times, q.variance):
    for bad in ('XYZ', 'XYZII', 'XAZI', {4: 'X'}, {-1: 'Z'}, {0: 'Q'}, 17):
      with pytest.raises(ValueError):
        method([(1.0, bad)])
    with pytest.raises(ValueError):
      method([1.0])
  assert np.array_equal(np.asarray(q.psi), psi)


def test_every_string_of_two_qubits(cpu_backend):
  _kind, width = cpu_backend
  q = _circuit(2, 1)
  psi = np.asarray(q.psi).copy()
  for s in (''.join(p) for p in itertools.product('IXYZ', repeat=2)):
    w = q.hamiltonian_times([(1.0, s)])
    got = w._dev.download() if w._dev is not None else w._host      # pylint: disable=protected-access
    want = kron_matrix([(1.0, s)], 2) @ psi.astype(np.complex128)
    assert np.array_equal(got, want.astype(psi.dtype)), s          # one term, coefficient 1: exact
