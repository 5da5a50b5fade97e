"""CPU tests of the dense k-qubit matrix path: the C-ABI symbol and its argument checks (planner-only handles), and the
routing of qc.unitary / qc.apply_matrix with the GPU replaced by a NumPy stand-in that implements apply_matrix."""
import ctypes

import numpy as np
import pytest

from qcc_amd import native
from qcc_amd.lib import backend, circuit, ops, state, tensor
from tests import fake_device

_dp = ctypes.POINTER(ctypes.c_double)


def _call(h, bits, ctl_mask=0, matrix=None, k=None):
  lib = native.load()
  k = len(bits) if k is None else k
  b = (ctypes.c_int32 * max(1, len(bits)))(*bits)
  m = np.eye(1 << min(max(k, 1), 6), dtype=np.complex128) if matrix is None else matrix
  return lib.qh_apply_matrix(h, k, b, ctl_mask, np.ascontiguousarray(m).ctypes.data_as(_dp))


@pytest.fixture
def dry():
  lib = native.load()
  handles = []

  def make(n, nglob=None, shard=0):
    h = ctypes.c_void_p()
    native.check(lib.qh_create_dry(n, 128, ctypes.byref(h)))
    if nglob is not None:
      native.check(lib.qh_set_shard(h, nglob, shard))
    handles.append(h)
    return h
  yield make
  for h in handles:
    lib.qh_destroy(h)


def test_symbol_exported_and_bound():
  lib = native.load()
  assert 'qh_apply_matrix' in native.SIGNATURES
  assert lib.qh_apply_matrix.argtypes == native.SIGNATURES['qh_apply_matrix'][1]
  assert lib.qh_version() >= 106


def test_argument_errors_on_dry_handle(dry):
  lib = native.load()
  h = dry(10)
  m = np.eye(4, dtype=np.complex128)
  assert lib.qh_apply_matrix(None, 2, (ctypes.c_int32 * 2)(0, 1), 0, m.ctypes.data_as(_dp)) == native.QH_ERR_ARG
  assert lib.qh_apply_matrix(h, 2, None, 0, m.ctypes.data_as(_dp)) == native.QH_ERR_ARG
  assert lib.qh_apply_matrix(h, 2, (ctypes.c_int32 * 2)(0, 1), 0, None) == native.QH_ERR_ARG
  assert _call(h, [], k=0) == native.QH_ERR_ARG
  assert _call(h, list(range(7)), matrix=np.eye(64, dtype=np.complex128), k=7) == native.QH_ERR_ARG
  assert _call(h, [0, 10]) == native.QH_ERR_BAD_QUBIT
  assert _call(h, [-1, 3]) == native.QH_ERR_BAD_QUBIT
  assert _call(h, [0, 1], ctl_mask=1 << 10) == native.QH_ERR_BAD_QUBIT
  assert _call(h, [3, 3]) == native.QH_ERR_SAME_QUBIT
  assert _call(h, [3, 3, 10]) == native.QH_ERR_BAD_QUBIT     # both faults: every bit's range is checked first
  assert _call(h, [2, 5], ctl_mask=(1 << 5) | (1 << 7)) == native.QH_ERR_SAME_QUBIT
  # a valid call: dry handles have no state to apply it to
  assert _call(h, [2, 5], ctl_mask=1 << 7) == native.QH_ERR_ARG
  assert b'dry' in lib.qh_last_error()


def test_too_many_insertions(dry):
  lib = native.load()
  h = dry(24)
  ctl = sum(1 << b for b in range(14, 24))           # 10 local controls + 6 targets = 16 > kMaxIns (15)
  assert _call(h, list(range(6)), ctl_mask=ctl) == native.QH_ERR_ARG
  assert b'kMaxIns' in lib.qh_last_error()
  ctl9 = sum(1 << b for b in range(15, 24))          # 9 + 6 = 15: accepted (then refused as dry)
  assert _call(h, list(range(6)), ctl_mask=ctl9) == native.QH_ERR_ARG
  assert b'dry' in lib.qh_last_error()


def test_shard_bit_target_is_nonlocal(dry):
  h = dry(10, nglob=12, shard=1)
  assert _call(h, [3, 11]) == native.QH_ERR_NONLOCAL
  assert _call(h, [3, 4], ctl_mask=1 << 11) == native.QH_ERR_ARG   # a shard-bit CONTROL is fine (dry refuses the rest)


class DenseOracle(fake_device.OracleDevice):
  """OracleDevice with apply_matrix, by tensordot over the target axes."""
  matrix_calls = []

  def apply_matrix(self, matrix, bits, ctl_mask=0):
    m = np.asarray(matrix, dtype=np.complex128)
    DenseOracle.matrix_calls.append((list(bits), int(ctl_mask)))
    self.psi[:] = dense_reference(self.psi, self.nbits, m, bits, ctl_mask).astype(self.dtype)


def dense_reference(psi, n, m, bits, ctl_mask=0):
  """Reference: matrix bit j <-> logical bit bits[j]; applied where all bits of ctl_mask are 1."""
  k = len(bits)
  t = np.asarray(psi, dtype=np.complex128).reshape([2] * n)          # axis a <-> logical bit n-1-a
  mt = m.reshape([2] * (2 * k))                                       # axes: row bits k-1..0, column bits k-1..0
  axes = [n - 1 - bits[k - 1 - i] for i in range(k)]                  # column axis i <-> matrix bit k-1-i
  out = np.tensordot(mt, t, axes=(list(range(k, 2 * k)), axes))     # row axes first, then the remaining axes of t
  rest = [a for a in range(n) if a not in axes]
  perm = np.empty(n, dtype=int)
  perm[axes] = np.arange(k)
  perm[rest] = np.arange(k, n)
  out = np.transpose(out, perm).reshape(-1)
  if ctl_mask:
    idx = np.arange(1 << n)
    out = np.where((idx & ctl_mask) == ctl_mask, out, np.asarray(psi, dtype=np.complex128))
  return out


@pytest.fixture
def cpu_backend():
  tensor.set_tensor_width(128)
  DenseOracle.matrix_calls = []
  backend.set_device_factory(DenseOracle)
  yield
  backend.set_device_factory(None)
  tensor.set_tensor_width(None)


def _random_op(rng, k, unitary):
  a = rng.normal(size=(1 << k, 1 << k)) + 1j * rng.normal(size=(1 << k, 1 << k))
  if unitary:
    a, _ = np.linalg.qr(a)
  return a


def _prepared(n, rng):
  q = circuit.qc('dense')
  q.reg(n, 0)
  for i in range(n):
    q.ry(i, float(rng.uniform(0, np.pi)))
  q.cx(0, n - 1)
  return q


def test_reference_helper_matches_kron():
  rng = np.random.default_rng(5)
  n, k, idx = 6, 3, 2
  psi = rng.normal(size=1 << n) + 1j * rng.normal(size=1 << n)
  m = _random_op(rng, k, False)
  full = np.kron(np.kron(np.eye(1 << idx), m), np.eye(1 << (n - idx - k)))
  got = dense_reference(psi, n, m, [n - idx - k + j for j in range(k)])
  assert np.max(np.abs(got - full @ psi)) < 1e-12


@pytest.mark.parametrize('k', [1, 2, 3, 4, 5, 6])
def test_unitary_routes_to_apply_matrix(cpu_backend, k):
  rng = np.random.default_rng(100 + k)
  for n in sorted({max(k, 3), k + 2, 12}):
    for unitary in (True, False):
      op = _random_op(rng, k, unitary)
      idx = int(rng.integers(0, n - k + 1))
      q = _prepared(n, np.random.default_rng(n))
      DenseOracle.matrix_calls = []
      q.unitary(op, idx)
      got = np.asarray(q.psi)
      assert DenseOracle.matrix_calls == [([n - idx - k + j for j in range(k)], 0)]
      want = ops.Operator(op)(_prepared(n, np.random.default_rng(n)).psi, idx)     # today's host path
      assert np.max(np.abs(got - np.asarray(want))) < 1e-12


def test_out_of_range_and_wide_ops_take_the_host_path(cpu_backend):
  rng = np.random.default_rng(7)
  q = _prepared(5, rng)
  with pytest.raises(ValueError):                  # idx + k > nbits: the host path's own error
    q.unitary(_random_op(rng, 2, True), 4)
  q = _prepared(8, rng)
  before = np.asarray(q.psi).copy()
  op7 = _random_op(rng, 7, True)
  q.unitary(op7, 1)
  assert DenseOracle.matrix_calls == []
  assert np.max(np.abs(np.asarray(q.psi) - np.asarray(ops.Operator(op7)(state.State(before), 1)))) < 1e-12


def test_queued_gates_are_drained_first(cpu_backend):
  q = circuit.qc('order')
  q.reg(4, 0)
  q.x(0)                                              # queued on the host side
  swap_top = np.eye(4)[[0, 2, 1, 3]]                  # swaps qubits 0 and 1
  q.unitary(swap_top, 0)
  assert q.prob(0, 1, 0, 0) == pytest.approx(1.0)
  tr = q._dev.trace
  assert len(tr) == 1 and tr[0][1] == 0               # the X reached the device before the matrix did


def test_apply_matrix_general_form(cpu_backend):
  rng = np.random.default_rng(11)
  n = 7
  op = _random_op(rng, 3, False)
  q = _prepared(n, rng)
  psi0 = np.asarray(q.psi).copy()
  q.apply_matrix(op, [5, 1, 3], ctl=[0, 6])
  bits = [n - 1 - 3, n - 1 - 1, n - 1 - 5]
  mask = (1 << (n - 1)) | 1
  assert DenseOracle.matrix_calls[-1] == (bits, mask)
  assert np.max(np.abs(np.asarray(q.psi) - dense_reference(psi0, n, op, bits, mask))) < 1e-12
  with pytest.raises(ValueError):
    q.apply_matrix(op, [1, 1, 2])
  with pytest.raises(ValueError):
    q.apply_matrix(op, [1, 2, 3], ctl=[3])
  with pytest.raises(ValueError):
    q.apply_matrix(op, [1, 2])
