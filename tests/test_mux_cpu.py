"""CPU tests of the table-selected gates: NumPy references for qh_apply_mux / qh_apply_diag (checked against the CPU oracle
and the reference-compatible operators), the two C-ABI symbols and their argument checks on planner-only handles, and the
routing of qc.multiplex / qc.diagonal / qc.oracle / qc.phase_oracle with the GPU replaced by a NumPy stand-in."""
import ctypes

import numpy as np
import pytest

from qcc_amd import gates, native
from qcc_amd.lib import backend, circuit, ops, state, tensor
from tests import fake_device, oracle_lib

_dp = ctypes.POINTER(ctypes.c_double)
_ip = ctypes.POINTER(ctypes.c_int32)


def _select(n, bits):
  """s(i) for every index i: bit j of s = bit bits[j] of i"""
  idx = np.arange(1 << n)
  s = np.zeros_like(idx)
  for j, b in enumerate(bits):
    s |= ((idx >> b) & 1) << j
  return idx, s


def mux_reference(psi, n, gates_, sel_bits, tgt_bit):
  """gates_[s] (shape (2^k, 2, 2)) on LOGICAL bit tgt_bit where the selection bits have the value s."""
  g = np.asarray(gates_, dtype=np.complex128).reshape(-1, 2, 2)
  psi = np.asarray(psi, dtype=np.complex128)
  out = psi.copy()
  idx, s = _select(n, sel_bits)
  q = 1 << tgt_bit
  for v in range(g.shape[0]):
    lo = idx[(s == v) & (idx & q == 0)]
    a, b = psi[lo], psi[lo | q]
    out[lo] = g[v, 0, 0] * a + g[v, 0, 1] * b
    out[lo | q] = g[v, 1, 0] * a + g[v, 1, 1] * b
  return out


def diag_reference(psi, n, values, bits):
  _, s = _select(n, bits)
  return np.asarray(psi, dtype=np.complex128) * np.asarray(values, dtype=np.complex128)[s]


def mux_reference_fast(psi, n, gates_, sel_bits, tgt_bit):
  """mux_reference without the loop over s (the GPU tests' tables have up to 2^16 entries): one gather of the gates."""
  g = np.asarray(gates_, dtype=np.complex128).reshape(-1, 2, 2)
  psi = np.asarray(psi, dtype=np.complex128)
  idx, s = _select(n, sel_bits)
  q = 1 << tgt_bit
  lo = idx[idx & q == 0]
  gs, a, b = g[s[lo]], psi[lo], psi[lo | q]
  out = np.empty_like(psi)
  out[lo] = gs[:, 0, 0] * a + gs[:, 0, 1] * b
  out[lo | q] = gs[:, 1, 0] * a + gs[:, 1, 1] * b
  return out


def _rand_state(rng, n):
  v = rng.normal(size=1 << n) + 1j * rng.normal(size=1 << n)
  return v / np.linalg.norm(v)


def _rand_gates(rng, k):
  return rng.normal(size=(1 << k, 2, 2)) + 1j * rng.normal(size=(1 << k, 2, 2))


# ---- the references themselves ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [2, 5, 10])
def test_mux_reference_k1_matches_oracle_applyc(n):
  rng = np.random.default_rng(n)
  o = oracle_lib.load()
  x = np.asarray(gates.pauli_x(), np.complex128) if hasattr(gates, 'pauli_x') else np.array([[0, 1], [1, 0]], np.complex128)
  for _ in range(4):
    c, t = (int(v) for v in rng.permutation(n)[:2])        # reference qubits
    g = _rand_gates(rng, 1)
    psi = _rand_state(rng, n)
    want = psi.copy()
    o.applyc(want, g[1], n, c, t)                            # gates[1] where the selector is 1 ...
    o.apply1(want, x, n, c)
    o.applyc(want, g[0], n, c, t)                            # ... gates[0] where it is 0
    o.apply1(want, x, n, c)
    got = mux_reference(psi, n, g, [n - 1 - c], n - 1 - t)
    assert np.max(np.abs(got - want)) < 1e-13


def test_mux_reference_k0_and_diag_reference_match_oracle():
  rng = np.random.default_rng(1)
  o = oracle_lib.load()
  n = 7
  psi = _rand_state(rng, n)
  g = _rand_gates(rng, 0)
  want = psi.copy()
  o.apply1(want, g[0], n, 2)
  assert np.max(np.abs(mux_reference(psi, n, g, [], n - 1 - 2) - want)) < 1e-13
  # a diagonal over two bits = two phase gates and one controlled phase
  a, b, c = np.exp(1j * rng.uniform(0, 6, size=3))
  vals = np.array([1, a, b, a * b * c])                      # s = bit(q1) + 2 bit(q4)
  want = psi.copy()
  o.apply1(want, np.diag([1, a]), n, 1)
  o.apply1(want, np.diag([1, b]), n, 4)
  o.applyc(want, np.diag([1, c]), n, 1, 4)
  assert np.max(np.abs(diag_reference(psi, n, vals, [n - 1 - 1, n - 1 - 4]) - want)) < 1e-13
  assert np.array_equal(diag_reference(psi, n, [2 - 1j], []), psi * (2 - 1j))


def test_mux_reference_matches_kron_of_blocks():
  rng = np.random.default_rng(2)
  n, k = 6, 3
  g = _rand_gates(rng, k)
  psi = _rand_state(rng, n)
  # selectors = qubits 1,2,3 (qubit 1 most significant), target = qubit 4: a block-diagonal 16 x 16 on qubits 1..4
  blk = np.zeros((16, 16), dtype=np.complex128)
  for s in range(8):
    blk[2 * s:2 * s + 2, 2 * s:2 * s + 2] = g[s]
  full = np.kron(np.kron(np.eye(2), blk), np.eye(2))
  got = mux_reference(psi, n, g, [n - 1 - 3, n - 1 - 2, n - 1 - 1], n - 1 - 4)
  assert np.max(np.abs(got - full @ psi)) < 1e-13


def test_fast_reference_equals_the_loop():
  rng = np.random.default_rng(8)
  for n, k in ((1, 0), (4, 3), (9, 5), (10, 9)):
    perm = [int(b) for b in rng.permutation(n)]
    g, psi = _rand_gates(rng, k), _rand_state(rng, n)
    assert np.array_equal(mux_reference_fast(psi, n, g, perm[:k], perm[k]), mux_reference(psi, n, g, perm[:k], perm[k]))


# ---- the C-ABI on planner-only handles -------------------------------------------------------------------------------
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


def _mux(h, sel, tgt, k=None, table=True):
  lib = native.load()
  k = len(sel) if k is None else k
  b = (ctypes.c_int32 * max(1, len(sel)))(*sel)
  g = np.tile(np.eye(2, dtype=np.complex128), (1 << min(max(k, 0), 16), 1, 1))
  return lib.qh_apply_mux(h, k, b, tgt, g.ctypes.data_as(_dp) if table else None)


def _diag(h, bits, k=None, table=True):
  lib = native.load()
  k = len(bits) if k is None else k
  b = (ctypes.c_int32 * max(1, len(bits)))(*bits)
  v = np.ones(1 << min(max(k, 0), 16), dtype=np.complex128)
  return lib.qh_apply_diag(h, k, b, v.ctypes.data_as(_dp) if table else None)


def test_symbols_exported_and_bound():
  lib = native.load()
  for name in ('qh_apply_mux', 'qh_apply_diag'):
    assert name in native.SIGNATURES
    assert getattr(lib, name).argtypes == native.SIGNATURES[name][1]
  assert lib.qh_version() >= 109


def test_argument_errors_on_dry_handle(dry):
  lib = native.load()
  h = dry(20)
  one = np.eye(2, dtype=np.complex128)
  assert lib.qh_apply_mux(None, 0, None, 0, one.ctypes.data_as(_dp)) == native.QH_ERR_ARG
  assert lib.qh_apply_diag(None, 0, None, one.ctypes.data_as(_dp)) == native.QH_ERR_ARG
  assert _mux(h, [1, 2], 0, table=False) == native.QH_ERR_ARG
  assert _diag(h, [1, 2], table=False) == native.QH_ERR_ARG
  assert lib.qh_apply_mux(h, 2, None, 0, one.ctypes.data_as(_dp)) == native.QH_ERR_ARG
  assert lib.qh_apply_diag(h, 2, None, one.ctypes.data_as(_dp)) == native.QH_ERR_ARG
  assert _mux(h, [], 0, k=-1) == native.QH_ERR_ARG
  assert _diag(h, [], k=-1) == native.QH_ERR_ARG
  assert _mux(h, list(range(17)), 19, k=17) == native.QH_ERR_ARG
  assert _diag(h, list(range(17)), k=17) == native.QH_ERR_ARG
  assert _mux(h, [0, 20], 1) == native.QH_ERR_BAD_QUBIT
  assert _mux(h, [-1, 3], 1) == native.QH_ERR_BAD_QUBIT
  assert _mux(h, [0, 3], 20) == native.QH_ERR_BAD_QUBIT
  assert _mux(h, [0, 3], -1) == native.QH_ERR_BAD_QUBIT
  assert _diag(h, [0, 20]) == native.QH_ERR_BAD_QUBIT
  assert _diag(h, [-2]) == native.QH_ERR_BAD_QUBIT
  assert _mux(h, [3, 3], 1) == native.QH_ERR_SAME_QUBIT
  assert _mux(h, [3, 4], 4) == native.QH_ERR_SAME_QUBIT
  assert _diag(h, [5, 1, 5]) == native.QH_ERR_SAME_QUBIT
  assert _diag(h, [5, 5, 20]) == native.QH_ERR_BAD_QUBIT     # both faults: every bit's range is checked first
  # valid calls, k = 0 and k = 16 included: a planner-only handle has no state to apply them to
  for rc in (_mux(h, [2, 5], 7), _mux(h, [], 3), _mux(h, list(range(16)), 19), _diag(h, [2, 5]), _diag(h, []),
             _diag(h, list(range(4, 20)))):
    assert rc == native.QH_ERR_ARG
    assert b'dry' in lib.qh_last_error()


def test_shard_bits_on_dry_handle(dry):
  lib = native.load()
  h = dry(10, nglob=12, shard=1)
  assert _mux(h, [3, 4], 11) == native.QH_ERR_NONLOCAL              # a shard-bit target
  assert _mux(h, [3, 11, 10], 4) == native.QH_ERR_ARG               # shard-bit selectors are fine (dry refuses the rest)
  assert b'dry' in lib.qh_last_error()
  assert _diag(h, [11, 0, 10]) == native.QH_ERR_ARG
  assert b'dry' in lib.qh_last_error()


# ---- routing of the qc methods ---------------------------------------------------------------------------------------
class MuxOracle(fake_device.OracleDevice):
  """OracleDevice with apply_mux / apply_diag through the references; records what it is asked."""
  mux_calls = []
  diag_calls = []

  def apply_mux(self, gates_, sel_bits, tgt_bit):
    g = np.array(gates_, dtype=np.complex128)
    MuxOracle.mux_calls.append((g, [int(b) for b in sel_bits], int(tgt_bit), len(self.trace)))
    self.psi[:] = mux_reference(self.psi, self.nbits, g, list(sel_bits), tgt_bit).astype(self.dtype)

  def apply_diag(self, values, bits):
    v = np.array(values, dtype=np.complex128)
    MuxOracle.diag_calls.append((v, [int(b) for b in bits], len(self.trace)))
    self.psi[:] = diag_reference(self.psi, self.nbits, v, list(bits)).astype(self.dtype)


@pytest.fixture
def cpu_backend():
  tensor.set_tensor_width(128)
  MuxOracle.mux_calls = []
  MuxOracle.diag_calls = []
  backend.set_device_factory(MuxOracle)
  yield
  backend.set_device_factory(None)
  tensor.set_tensor_width(None)


def _prepared(n, seed):
  rng = np.random.default_rng(seed)
  q = circuit.qc('mux')
  q.reg(n, 0)
  for i in range(n):
    q.ry(i, float(rng.uniform(0, np.pi)))
  q.cx(0, n - 1)
  return q


def test_multiplex_routes_logical_bits_and_table_order(cpu_backend):
  rng = np.random.default_rng(3)
  n = 7
  g = _rand_gates(rng, 3)
  q = _prepared(n, 1)
  psi0 = np.asarray(q.psi).copy()
  q.multiplex(g, [5, 1, 3], 2)
  got_g, bits, tgt, _ = MuxOracle.mux_calls[-1]
  assert bits == [n - 1 - 3, n - 1 - 1, n - 1 - 5] and tgt == n - 1 - 2      # sel[0] = most significant table bit
  assert np.array_equal(got_g, g)
  # independent check: gate g[s] where (q5, q1, q3) spell s, most significant first
  idx = np.arange(1 << n)
  bit = lambda qb: (idx >> (n - 1 - qb)) & 1                                   # noqa: E731
  s = (bit(5) << 2) | (bit(1) << 1) | bit(3)
  want = psi0.copy()
  lo = idx[bit(2) == 0]
  hi = lo | (1 << (n - 1 - 2))
  want[lo] = g[s[lo], 0, 0] * psi0[lo] + g[s[lo], 0, 1] * psi0[hi]
  want[hi] = g[s[lo], 1, 0] * psi0[lo] + g[s[lo], 1, 1] * psi0[hi]
  assert np.max(np.abs(np.asarray(q.psi) - want)) < 1e-12
  # k = 0: a plain gate
  q.multiplex(g[:1], [], 4)
  assert MuxOracle.mux_calls[-1][1:3] == ([], n - 1 - 4)


def test_diagonal_routes_logical_bits_and_table_order(cpu_backend):
  rng = np.random.default_rng(4)
  n = 6
  v = rng.normal(size=8) + 1j * rng.normal(size=8)
  q = _prepared(n, 2)
  psi0 = np.asarray(q.psi).copy()
  q.diagonal(v, [4, 0, 2])
  got_v, bits, _ = MuxOracle.diag_calls[-1]
  assert bits == [n - 1 - 2, n - 1 - 0, n - 1 - 4] and np.array_equal(got_v, v)
  idx = np.arange(1 << n)
  bit = lambda qb: (idx >> (n - 1 - qb)) & 1                                   # noqa: E731
  want = psi0 * v[(bit(4) << 2) | (bit(0) << 1) | bit(2)]
  assert np.max(np.abs(np.asarray(q.psi) - want)) < 1e-12


@pytest.mark.parametrize('k', [1, 2, 4])
def test_oracle_matches_OracleUf_full_matrix(cpu_backend, k):
  rng = np.random.default_rng(10 + k)
  table = rng.integers(0, 2, size=1 << k)
  f = lambda bits: int(table[int(''.join(str(b) for b in bits), 2)])            # noqa: E731  (bits[0] = qubit xs[0])
  n, idx = k + 3, 1
  for form in (f, table):
    q = _prepared(n, k)
    before = state.State(np.asarray(q.psi).copy())
    q.oracle(form, list(range(idx, idx + k)), idx + k)
    want = ops.OracleUf(k + 1, f)(before, idx)
    assert np.array_equal(np.asarray(q.psi), np.asarray(want))                  # a permutation: exact
    g = MuxOracle.mux_calls[-1][0]
    assert all(np.array_equal(g[s], np.eye(2)[::-1] if table[s] else np.eye(2)) for s in range(1 << k))
  # a non-adjacent, unordered register: y <- y xor f(x) read off the basis states
  q = circuit.qc('basis')
  q.reg(5, 0)
  q.x(3)
  q.x(0)
  t2 = [0, 1, 1, 0]
  q.oracle(t2, [3, 0], 2)                                                       # x = (q3, q0) = (1, 1): f = 0
  assert q.prob(1, 0, 0, 1, 0) == pytest.approx(1.0)
  q.x(0)                                                                        # x = (1, 0): f = 1
  q.oracle(t2, [3, 0], 2)
  assert q.prob(0, 0, 1, 1, 0) == pytest.approx(1.0)


def test_phase_oracle_is_the_sign_table(cpu_backend):
  n = 5
  table = [0, 1, 1, 0, 1, 0, 0, 0]
  q = _prepared(n, 7)
  psi0 = np.asarray(q.psi).copy()
  q.phase_oracle(lambda bits: table[bits[0] * 4 + bits[1] * 2 + bits[2]], [4, 1, 2])
  v, bits, _ = MuxOracle.diag_calls[-1]
  assert bits == [n - 1 - 2, n - 1 - 1, n - 1 - 4]
  assert np.array_equal(v, 1.0 - 2.0 * np.array(table))
  idx = np.arange(1 << n)
  bit = lambda qb: (idx >> (n - 1 - qb)) & 1                                   # noqa: E731
  sign = 1.0 - 2.0 * np.array(table)[(bit(4) << 2) | (bit(1) << 1) | bit(2)]
  assert np.array_equal(np.asarray(q.psi), psi0 * sign)
  q.phase_oracle(table, [4, 1, 2])                                              # the sequence form; twice = identity
  assert np.array_equal(np.asarray(q.psi), psi0)


def test_queued_gates_are_drained_first(cpu_backend):
  x = np.array([[0, 1], [1, 0]])
  for call in ('multiplex', 'diagonal', 'oracle', 'phase_oracle'):
    q = circuit.qc('order')
    q.reg(4, 0)
    q.x(0)                                            # queued on the host side
    if call == 'multiplex':
      q.multiplex([np.eye(2), x], [0], 1)             # X on qubit 1 where qubit 0 is 1
      seen = MuxOracle.mux_calls[-1][3]
    elif call == 'oracle':
      q.oracle([0, 1], [0], 1)
      seen = MuxOracle.mux_calls[-1][3]
    elif call == 'diagonal':
      q.diagonal([1, -1], [0])
      seen = MuxOracle.diag_calls[-1][2]
    else:
      q.phase_oracle([0, 1], [0])
      seen = MuxOracle.diag_calls[-1][2]
    assert seen == 1                                  # the X had reached the device when the table call arrived
    if call in ('multiplex', 'oracle'):
      assert q.prob(1, 1, 0, 0) == pytest.approx(1.0)
    else:
      assert q.ampl(1, 0, 0, 0) == pytest.approx(-1.0)


def test_value_errors(cpu_backend):
  q = _prepared(6, 9)
  g = np.tile(np.eye(2), (4, 1, 1))
  with pytest.raises(ValueError):
    q.multiplex(g, [1, 1], 2)                         # a selector twice
  with pytest.raises(ValueError):
    q.multiplex(g, [1, 2], 2)                         # the target among the selectors
  with pytest.raises(ValueError):
    q.multiplex(g, [1, 6], 2)                         # out of range
  with pytest.raises(ValueError):
    q.multiplex(g, [1, 2], -1)
  with pytest.raises(ValueError):
    q.multiplex(g, [1, 2, 3], 4)                      # 4 gates for 3 selectors
  with pytest.raises(ValueError):
    q.multiplex(np.eye(4), [1, 2], 4)                 # not (2^k, 2, 2)
  with pytest.raises(ValueError):
    q.diagonal(np.ones(4), [3, 3])
  with pytest.raises(ValueError):
    q.diagonal(np.ones(4), [3, 7])
  with pytest.raises(ValueError):
    q.diagonal(np.ones(8), [3, 4])
  with pytest.raises(ValueError):
    q.oracle([0, 1, 1], [0, 1], 2)                    # 3 entries for 2 qubits
  with pytest.raises(ValueError):
    q.oracle([0, 1, 2, 0], [0, 1], 2)                 # not 0/1
  with pytest.raises(ValueError):
    q.oracle([0, 1, 1, 0], [0, 1], 1)
  with pytest.raises(ValueError):
    q.phase_oracle([0, 1, 1, 0], [2, 2])
  with pytest.raises(ValueError):
    q.phase_oracle([0, 1], [0, 1])
  assert MuxOracle.mux_calls == [] and MuxOracle.diag_calls == []


def test_devices_without_the_methods_raise(cpu_backend):
  backend.set_device_factory(fake_device.OracleDevice)
  q = _prepared(4, 1)
  with pytest.raises(NotImplementedError):
    q.multiplex(np.tile(np.eye(2), (2, 1, 1)), [0], 1)
  with pytest.raises(NotImplementedError):
    q.diagonal([1, 1], [0])
  with pytest.raises(NotImplementedError):
    q.oracle([0, 1], [0], 1)
  with pytest.raises(NotImplementedError):
    q.phase_oracle([0, 1], [0])
