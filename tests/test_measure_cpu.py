"""CPU tests of register readout: the C-ABI symbols and their argument checks (planner-only handles), qc.probabilities /
sample / measure with the GPU replaced by a NumPy stand-in that implements marginal / sample / project_bits, and the
sharded layer over gloo (world sizes 2 and 4) against the single-process answer."""
import ctypes
import os
import socket

import numpy as np
import pytest
import torch.multiprocessing as mp

from qcc_amd import native
from qcc_amd.lib import backend, circuit, tensor
from tests import fake_device
from tests.fake_device import MeasureOracle, MeasureShardEngine, np_keep, np_marginal, np_sample  # noqa: F401
from tests.fake_device import readout_circuit as _circuit

_dp = ctypes.POINTER(ctypes.c_double)
_up = ctypes.POINTER(ctypes.c_uint64)


# ---- the C-ABI ---------------------------------------------------------------------------------------------------------
def test_version_and_symbols_bound():
  lib = native.load()
  assert lib.qh_version() >= 107
  for name in ('qh_marginal', 'qh_sample', 'qh_project_bits'):
    assert name in native.SIGNATURES
    assert getattr(lib, name).argtypes == native.SIGNATURES[name][1]


@pytest.fixture
def dry():
  lib = native.load()
  h = ctypes.c_void_p()
  native.check(lib.qh_create_dry(10, 128, ctypes.byref(h)))
  yield h
  lib.qh_destroy(h)


def _marg(h, bits, k=None, out=True):
  lib = native.load()
  b = (ctypes.c_int32 * max(1, len(bits)))(*bits)
  o = np.zeros(1 << 17)
  return lib.qh_marginal(h, len(bits) if k is None else k, b, o.ctypes.data_as(_dp) if out else None)


def test_marginal_argument_errors(dry):
  lib = native.load()
  o = np.zeros(4)
  assert lib.qh_marginal(None, 1, (ctypes.c_int32 * 1)(0), o.ctypes.data_as(_dp)) == native.QH_ERR_ARG
  assert lib.qh_marginal(dry, 1, None, o.ctypes.data_as(_dp)) == native.QH_ERR_ARG
  assert _marg(dry, [0], out=False) == native.QH_ERR_ARG
  assert _marg(dry, list(range(10)) + [0] * 7, k=17) == native.QH_ERR_ARG
  assert _marg(dry, [0], k=-1) == native.QH_ERR_ARG
  assert _marg(dry, [10]) == native.QH_ERR_BAD_QUBIT
  assert _marg(dry, [-1]) == native.QH_ERR_BAD_QUBIT
  assert _marg(dry, [3, 5, 3]) == native.QH_ERR_SAME_QUBIT
  assert _marg(dry, [3, 3, 10]) == native.QH_ERR_BAD_QUBIT    # both faults: every bit's range is checked first
  assert _marg(dry, [3, 5]) == native.QH_ERR_ARG           # valid, but a dry handle has no state
  assert b'dry' in lib.qh_last_error()
  assert _marg(dry, []) == native.QH_ERR_ARG


def test_sample_argument_errors(dry):
  lib = native.load()
  out = np.zeros(4, dtype=np.uint64)

  def call(u, h=dry, outp=True):
    u = np.asarray(u, dtype=np.float64)
    return lib.qh_sample(h, u.size, u.ctypes.data_as(_dp) if u.size else None, out.ctypes.data_as(_up) if outp else None)
  assert call([0.5], h=None) == native.QH_ERR_ARG
  assert call([0.5], outp=False) == native.QH_ERR_ARG
  assert lib.qh_sample(dry, 1, None, out.ctypes.data_as(_up)) == native.QH_ERR_ARG
  assert call([0.5, 0.2]) == native.QH_ERR_ARG
  assert b'ascending' in lib.qh_last_error()
  assert call([0.2, 1.0]) == native.QH_ERR_ARG
  assert call([-0.1]) == native.QH_ERR_ARG
  assert call([float('nan')]) == native.QH_ERR_ARG
  assert call([0.0, 0.2, 0.2, 0.99]) == native.QH_ERR_ARG
  assert b'dry' in lib.qh_last_error()


def test_project_bits_argument_errors(dry):
  lib = native.load()
  assert lib.qh_project_bits(None, 1, 1) == native.QH_ERR_ARG
  assert lib.qh_project_bits(dry, 0b0110, 0b1000) == native.QH_ERR_ARG
  assert b'outside mask' in lib.qh_last_error()
  assert lib.qh_project_bits(dry, 1 << 10, 0) == native.QH_ERR_BAD_QUBIT
  assert lib.qh_project_bits(dry, 0b0110, 0b0100) == native.QH_ERR_ARG
  assert b'dry' in lib.qh_last_error()


# ---- qc on a NumPy device ------------------------------------------------------------------------------------------------
@pytest.fixture
def cpu_backend():
  tensor.set_tensor_width(128)
  backend.set_device_factory(MeasureOracle)
  yield
  backend.set_device_factory(None)
  tensor.set_tensor_width(None)


def _ref_probs(psi, qubits):
  """the reference's way: psi.prob(*bits) summed over every basis state, register value in bits2val order"""
  nq = psi.nbits
  out = np.zeros(1 << len(qubits))
  for i in range(1 << nq):
    bits = [(i >> (nq - 1 - q)) & 1 for q in range(nq)]
    v = 0
    for q in qubits:
      v = 2 * v + bits[q]
    out[v] += float(psi.prob(*bits))
  return out


def test_probabilities_bit_order(cpu_backend):
  q = _circuit(5, 1)
  psi = q.psi
  for qubits in ([0], [4], [0, 1], [1, 0], [3, 0, 4], [2, 4, 1, 0, 3]):
    np.testing.assert_allclose(q.probabilities(qubits), _ref_probs(psi, qubits), atol=1e-14)
  with pytest.raises(ValueError):
    q.probabilities([0, 0])
  with pytest.raises(ValueError):
    q.probabilities([5])


def test_sample_seeds_order_and_distribution(cpu_backend):
  q = _circuit(6, 2)
  a = q.sample(2000, [5, 0, 2], seed=11)
  assert a.dtype == np.uint64 and a.shape == (2000,)
  assert a.tolist() == q.sample(2000, [5, 0, 2], seed=11).tolist()
  assert a.tolist() != q.sample(2000, [5, 0, 2], seed=12).tolist()
  # draw order: shot s is the inverse CDF of the s-th uniform of the stream
  u = np.random.default_rng(11).random(2000)
  full = np_sample(np.asarray(q.psi), u)
  want = (((full >> np.uint64(0)) & np.uint64(1)) << np.uint64(2)) | (((full >> np.uint64(5)) & np.uint64(1)) << np.uint64(1)) | \
      ((full >> np.uint64(3)) & np.uint64(1))
  assert a.tolist() == want.tolist()
  assert q.sample(2000, seed=11).tolist() == full.tolist()
  np.random.seed(7)
  b = q.sample(500, [1, 2])
  np.random.seed(7)
  assert q.sample(500, [1, 2]).tolist() == b.tolist()
  freq = np.bincount(q.sample(20000, [1, 2], seed=1).astype(np.int64), minlength=4) / 20000
  np.testing.assert_allclose(freq, _ref_probs(q.psi, [1, 2]), atol=0.02)
  assert q.sample(0, [1]).size == 0


def test_measure_collapses(cpu_backend):
  for seed in range(4):
    q = _circuit(5, 10 + seed)
    psi = np.asarray(q.psi).copy()
    qubits = [3, 0] if seed % 2 else [1, 4, 2]
    probs = _ref_probs(q.psi, qubits)
    value, prob = q.measure(qubits, seed=seed, collapse=False)
    u = np.random.default_rng(seed).random(1)[0]          # the inverse CDF of the register's distribution at one uniform
    assert value == int(np.searchsorted(np.cumsum(probs), u * probs.sum(), side='right'))
    assert abs(prob - probs[value]) < 1e-14
    assert np.array_equal(np.asarray(q.psi), psi)
    value, prob = q.measure(qubits, seed=seed)
    idx = np.arange(32)
    keep = np.ones(32, dtype=bool)
    for t, qb in enumerate(qubits):
      keep &= ((idx >> (4 - qb)) & 1) == ((value >> (len(qubits) - 1 - t)) & 1)
    want = np.where(keep, psi, 0) / np.sqrt(prob)
    got = np.asarray(q.psi)
    assert np.max(np.abs(got - want)) < 1e-14
    assert abs(np.vdot(got, got).real - 1) < 1e-14


def test_measure_reads_the_state_once(cpu_backend):
  q = _circuit(6, 21)
  dev = q._ensure_device()                               # pylint: disable=protected-access
  calls = []
  for name in ('marginal', 'sample', 'norm2', 'prob_bit'):
    orig = getattr(dev, name)
    setattr(dev, name, lambda *a, _o=orig, _n=name, **kw: (calls.append(_n), _o(*a, **kw))[1])
  q.measure([2, 5, 0], seed=4)
  assert calls == ['marginal']


def test_marginal_refuses_k_above_16_before_allocating():
  from qcc_amd import device
  st = device.DeviceState(40, 128, dry=True)
  with pytest.raises(native.QhError) as e:
    st.marginal(list(range(40)))                          # 2^40 doubles would be 8 TiB
  assert e.value.code == native.QH_ERR_ARG
  with pytest.raises(native.QhError) as e:
    st.marginal(list(range(17)))
  assert e.value.code == native.QH_ERR_ARG
  st.close()


def test_devices_without_readout_methods_fall_back_to_numpy():
  tensor.set_tensor_width(128)
  backend.set_device_factory(fake_device.OracleDevice)
  try:
    q = _circuit(4, 3)
    psi = np.asarray(q.psi).copy()
    np.testing.assert_allclose(q.probabilities([2, 0]), _ref_probs(q.psi, [2, 0]), atol=1e-14)
    assert q.sample(300, [1], seed=4).tolist() == ((np_sample(psi, np.random.default_rng(4).random(300)) >> np.uint64(2)) &
                                                 np.uint64(1)).tolist()
    value, prob = q.measure([0, 3], seed=2)
    keep = np.array([((i >> 3) & 1) * 2 + (i & 1) == value for i in range(16)])
    np.testing.assert_allclose(np.asarray(q.psi), np.where(keep, psi, 0) / np.sqrt(prob), atol=1e-14)
  finally:
    backend.set_device_factory(None)
    tensor.set_tensor_width(None)


# ---- sharded: gloo, world sizes 2 and 4 ----------------------------------------------------------------------------------
def _free_port():
  s = socket.socket()
  s.bind(('127.0.0.1', 0))
  p = s.getsockname()[1]
  s.close()
  return p


def _sharded_worker(rank, world, port, n, out_dir):
  os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                    LOCAL_RANK=str(rank))
  import torch.distributed as dist
  dist.init_process_group('gloo', rank=rank, world_size=world)
  from qcc_amd import sharded
  fake_device.sharded_readout_worker(
      rank, n, out_dir, lambda nbits, bw: sharded.ShardedDevice(nbits, bw, engine_factory=MeasureShardEngine, chunk_amps=16))
  dist.barrier()
  dist.destroy_process_group()


@pytest.mark.parametrize('world,n', [(2, 6), (4, 7)])
def test_sharded_readout_equals_single_process(tmp_path, world, n):
  mp.spawn(_sharded_worker, args=(world, _free_port(), n, str(tmp_path)), nprocs=world, join=True)
  fake_device.check_sharded_readout(tmp_path, world, n, atol=1e-13)
