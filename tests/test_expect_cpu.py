"""CPU tests of Pauli-string expectations: the C-ABI symbol and its argument checks (planner-only handles), qc.expectation
with the GPU replaced by a NumPy stand-in that implements expect_pauli and over the fallback that reads qc.psi, the
golden values recorded from the reference, and the sharded layer over gloo (world sizes 2 and 4) against the
single-process answer."""
import ctypes
import functools
import itertools
import os
import socket

import numpy as np
import pytest
import torch.multiprocessing as mp

from qcc_amd import native
from qcc_amd.lib import backend, circuit, ops, tensor
from tests import fake_device

_dp = ctypes.POINTER(ctypes.c_double)
_up = ctypes.POINTER(ctypes.c_uint64)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'g12_pauli_expect.npz')


def np_expect(psi, x, z, base=0):
  """Re sum_i conj(a_i) (P a)_i over the indices base .. base + size - 1 that psi holds (x must stay inside them)"""
  a = np.asarray(psi, dtype=np.complex128).reshape(-1)
  idx = np.uint64(base) + np.arange(a.size, dtype=np.uint64)
  par = np.zeros(a.size, dtype=np.uint64)
  for b in range(64):
    if (int(z) >> b) & 1:
      par ^= (idx >> np.uint64(b)) & np.uint64(1)
  partner = (idx ^ np.uint64(x)) - np.uint64(base)
  s = np.sum(np.conj(a) * (1.0 - 2.0 * par.astype(np.float64)) * a[partner.astype(np.int64)])
  return float(((-1j) ** (bin(int(x) & int(z)).count('1') % 4) * s).real)


class ExpectOracle(fake_device.OracleDevice):
  """OracleDevice with expect_pauli in NumPy (logical order = the array's order)."""
  reads = 0

  def expect_pauli(self, xmasks, zmasks):
    ExpectOracle.reads += 1
    return np.array([np_expect(self.psi, x, z) for x, z in zip(xmasks, zmasks)], dtype=np.float64)


class ExpectShardEngine(fake_device.NumpyShardEngine):
  """NumpyShardEngine with expect_pauli as qh_expect_pauli resolves shard bits: z on a shard bit is a sign of the shard,
  x on a shard bit is QH_ERR_NONLOCAL."""

  def expect_pauli(self, xmasks, zmasks):
    if any(int(x) >> self.nbits for x in xmasks):
      raise native.QhError(native.QH_ERR_NONLOCAL, 'expect_pauli: X or Y on a bit held by the shard index')
    return np.array([np_expect(self.psi, x, z, self.shard << self.nbits) for x, z in zip(xmasks, zmasks)], dtype=np.float64)


def kron_value(psi, s):
  """<psi| P |psi> with P the np.kron product of qcc_amd.lib.ops Paulis, letter q of s on qubit q"""
  mats = {'I': np.eye(2), 'X': np.asarray(ops.PauliX()), 'Y': np.asarray(ops.PauliY()), 'Z': np.asarray(ops.PauliZ())}
  m = functools.reduce(np.kron, [mats[c] for c in s])
  a = np.asarray(psi, dtype=np.complex128).reshape(-1)
  return complex(np.vdot(a, m @ a))


# ---- the C-ABI ---------------------------------------------------------------------------------------------------------
def test_version_and_symbol_bound():
  lib = native.load()
  assert lib.qh_version() >= 108
  assert 'qh_expect_pauli' in native.SIGNATURES
  assert lib.qh_expect_pauli.argtypes == native.SIGNATURES['qh_expect_pauli'][1]


def test_expect_argument_errors():
  lib = native.load()
  h = ctypes.c_void_p()
  native.check(lib.qh_create_dry(10, 128, ctypes.byref(h)))
  try:
    out = np.full(4, 7.0)

    def call(xs, zs, hh=h, xp=True, zp=True, op=True, n=None):
      x, z = np.asarray(xs, dtype=np.uint64), np.asarray(zs, dtype=np.uint64)
      return lib.qh_expect_pauli(hh, x.size if n is None else n, x.ctypes.data_as(_up) if xp else None,
                                 z.ctypes.data_as(_up) if zp else None, out.ctypes.data_as(_dp) if op else None)
    assert call([1], [0], hh=None) == native.QH_ERR_ARG
    assert call([1], [0], xp=False) == native.QH_ERR_ARG
    assert call([1], [0], zp=False) == native.QH_ERR_ARG
    assert call([1], [0], op=False) == native.QH_ERR_ARG
    assert call([1, 1 << 10], [0, 0]) == native.QH_ERR_BAD_QUBIT       # mask checks come before the dry-handle refusal
    assert call([1, 2], [0, 1 << 63]) == native.QH_ERR_BAD_QUBIT
    assert call([1], [3]) == native.QH_ERR_ARG                          # valid, but a dry handle has no state
    assert b'dry' in lib.qh_last_error()
    assert call([], [], n=0) == native.QH_ERR_ARG                       # (as qh_marginal: no state to flush)
    assert out.tolist() == [7.0] * 4
  finally:
    lib.qh_destroy(h)


# ---- qc.expectation on NumPy devices ------------------------------------------------------------------------------------
@pytest.fixture(params=['expect_pauli', 'fallback'])
def cpu_backend(request):
  tensor.set_tensor_width(128)
  backend.set_device_factory(ExpectOracle if request.param == 'expect_pauli' else fake_device.OracleDevice)
  yield request.param
  backend.set_device_factory(None)
  tensor.set_tensor_width(None)


def _circuit(nq, seed):
  rng = np.random.default_rng(seed)
  q = circuit.qc('e')
  q.reg(nq, 0)
  for _ in range(3 * nq):
    a = int(rng.integers(nq))
    q.ry(a, float(rng.random() * 3))
    b = int(rng.integers(nq))
    if b != a:
      q.cx(a, b)
    q.rz(int(rng.integers(nq)), float(rng.random() * 3))
  return q


def test_every_string_of_three_qubits(cpu_backend):
  q = _circuit(3, 1)
  psi = np.asarray(q.psi).copy()
  strings = [''.join(s) for s in itertools.product('IXYZ', repeat=3)]
  reads = ExpectOracle.reads
  got = q.expectation([(1.0, s) for s in strings], per_term=True)
  if cpu_backend == 'expect_pauli':
    assert ExpectOracle.reads == reads + 1                 # one device call for the whole Hamiltonian
  assert got.dtype == np.float64 and got.shape == (64,)
  for s, v in zip(strings, got):
    want = kron_value(psi, s)
    assert abs(want.imag) < 1e-14 and abs(v - want.real) < 1e-14, s
  assert np.array_equal(np.asarray(q.psi), psi)


def test_random_strings_and_forms(cpu_backend):
  rng = np.random.default_rng(3)
  for n in range(4, 11):
    q = _circuit(n, 10 + n)
    psi = np.asarray(q.psi).copy()
    strings = [''.join(rng.choice(list('IXYZ'), size=n)) for _ in range(6)]
    coeffs = rng.normal(size=6)
    vals = q.expectation([(1, s) for s in strings], per_term=True)
    want = np.array([kron_value(psi, s).real for s in strings])
    np.testing.assert_allclose(vals, want, atol=1e-13)
    total = q.expectation(zip(coeffs, strings))
    assert isinstance(total, float) and abs(total - float(np.dot(coeffs, want))) < 1e-12
    dicts = [{k: c for k, c in enumerate(s) if c != 'I'} for s in strings]
    assert np.array_equal(q.expectation([(1, d) for d in dicts], per_term=True), vals)
    assert np.array_equal(q.expectation([(1, {k: c.lower() for k, c in d.items()}) for d in dicts], per_term=True), vals)
    ctotal = q.expectation([(1j * c, s) for c, s in zip(coeffs, strings)])
    assert isinstance(ctotal, complex) and abs(ctotal - 1j * float(np.dot(coeffs, want))) < 1e-12
  assert q.expectation([]) == 0.0
  assert q.expectation([], per_term=True).shape == (0,)
  # not normalised: it reports what the state holds
  q.psi = 2.0 * np.asarray(q.psi)
  assert abs(q.expectation([(1, {})]) - 4.0) < 1e-12


def test_argument_errors(cpu_backend):
  q = _circuit(4, 2)
  for bad in ('XYZ', 'XYZII', 'XAZI', {4: 'X'}, {-1: 'Z'}, {0: 'Q'}, {0: 1}, {'0': 'X'}, 17):
    with pytest.raises(ValueError):
      q.expectation([(1.0, bad)])
  with pytest.raises(ValueError):
    q.expectation([1.0])
  with pytest.raises(ValueError):
    q.expectation([(1.0, 'XXXX', 3)])


def test_pauli_expectation_is_unchanged(cpu_backend):
  q = _circuit(4, 5)
  for k in range(4):
    assert abs(q.pauli_expectation(k) - q.expectation([(1, {k: 'Z'})])) < 1e-13


def test_golden_values_from_the_reference(cpu_backend):
  g = np.load(GOLDEN)
  assert len(g['values']) >= 36
  for k, s, v in zip(g['state'], g['strings'], g['values']):
    n = int(g['nbits'][k])
    q = circuit.qc('g')
    q.reg(n, 0)
    q.psi = g[f'psi{k}']
    s = str(s)[:n]
    assert abs(v.imag) < 1e-13
    assert abs(q.expectation([(1.0, s)]) - v.real) < 1e-13, (n, s)


# ---- sharded: gloo, world sizes 2 and 4 ----------------------------------------------------------------------------------
def _free_port():
  s = socket.socket()
  s.bind(('127.0.0.1', 0))
  p = s.getsockname()[1]
  s.close()
  return p


def _shard_qubits(q):
  st = q._ensure_device().st                             # pylint: disable=protected-access
  return [qb for qb in range(q.nbits) if st.perm[q.nbits - 1 - qb] >= st.nloc]


def _sharded_terms(n, sq):
  local = [qb for qb in range(n) if qb not in sq]
  return [
      (1.0, {}),
      (1.0, {q: 'Z' for q in sq}),                                        # Z on every shard bit
      (1.0, {sq[0]: 'Z', local[0]: 'Z'}),
      (0.5, {local[0]: 'X', local[-1]: 'Y', sq[0]: 'Z'}),                 # local x mask, sign from the shard index
      (-0.25, {local[1]: 'Y'}),
      (2.0, {sq[0]: 'X'}),                                                # X on a shard bit: forces an exchange
      (1.5, {sq[-1]: 'Y', local[0]: 'Z', local[2]: 'X'}),
      (1.0, {q: 'X' for q in sq}),
  ]


def _sharded_worker(rank, world, port, n, out_dir):
  os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                    LOCAL_RANK=str(rank))
  import torch.distributed as dist
  dist.init_process_group('gloo', rank=rank, world_size=world)
  from qcc_amd import sharded
  tensor.set_tensor_width(128)
  backend.set_device_factory(lambda nbits, bw: sharded.ShardedDevice(nbits, bw, engine_factory=ExpectShardEngine,
                                                                      chunk_amps=16))
  q = _circuit(n, 5)
  q.h(0)                                                  # dense gates on the top qubits: shard bits get exchanged
  q.cx(0, n - 1)
  res = {'psi': np.asarray(q.psi).copy()}
  dev = q._ensure_device()                                # pylint: disable=protected-access
  sq = _shard_qubits(q)
  res['sq'] = np.array(sq)
  terms = _sharded_terms(n, sq)
  x0 = dev.st.exchanges
  res['local_vals'] = q.expectation(terms[:5], per_term=True)
  res['x_local'] = np.array([dev.st.exchanges - x0])      # Z on shard bits and local x masks: nothing moves
  res['vals'] = q.expectation(terms, per_term=True)
  res['x_all'] = np.array([dev.st.exchanges - x0])
  res['total'] = np.array([q.expectation(terms)])
  res['psi_after'] = np.asarray(q.psi).copy()
  q.h(1)                                                  # later gates still see the right state
  q.cx(1, 0)
  q.ry(n - 1, 0.4)
  res['psi_gates'] = np.asarray(q.psi).copy()
  np.savez(os.path.join(out_dir, f'r{rank}.npz'), **res)
  dist.barrier()
  dist.destroy_process_group()


@pytest.mark.parametrize('world,n', [(2, 6), (4, 7)])
def test_sharded_expectation_equals_single_process(tmp_path, world, n):
  mp.spawn(_sharded_worker, args=(world, _free_port(), n, str(tmp_path)), nprocs=world, join=True)
  res = [dict(np.load(tmp_path / f'r{r}.npz')) for r in range(world)]
  for r in res[1:]:
    for k, v in res[0].items():
      assert np.array_equal(v, r[k]), k                  # every rank returns the same floats
  r0 = res[0]
  psi = r0['psi']
  sq = r0['sq'].tolist()
  assert len(sq) == world.bit_length() - 1
  assert int(r0['x_local'][0]) == 0
  assert int(r0['x_all'][0]) >= 1                         # the X-on-shard-bit strings went through the exchange
  tensor.set_tensor_width(128)
  backend.set_device_factory(ExpectOracle)
  try:
    q = circuit.qc('single')
    q.reg(n, 0)
    q.psi = psi
    terms = _sharded_terms(n, sq)
    want = q.expectation(terms, per_term=True)
    np.testing.assert_allclose(r0['vals'], want, atol=1e-12)
    np.testing.assert_allclose(r0['local_vals'], want[:5], atol=1e-12)
    assert abs(float(r0['total'][0]) - q.expectation(terms)) < 1e-12
    np.testing.assert_allclose(r0['psi_after'], psi, atol=1e-14)      # the exchange moved amplitudes, not the state
    q.h(1)
    q.cx(1, 0)
    q.ry(n - 1, 0.4)
    np.testing.assert_allclose(r0['psi_gates'], np.asarray(q.psi), atol=1e-13)
  finally:
    backend.set_device_factory(None)
    tensor.set_tensor_width(None)
