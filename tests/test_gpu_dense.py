"""qh_apply_matrix on the MI355X: dense 2^k x 2^k matrices (k = 1..6) on arbitrary bits, against NumPy / torch references.

Small registers (every k, random and unordered targets, 0-2 controls with line bits among them, both widths, fusion off
and on, 2x2 gates around the call, host-mapped handles), a permuted bit map left by relayout sweeps, exact cases,
matrices queued back to back, sharded handles, whole 30-qubit states compared in HBM, and qc.unitary / qc.apply_matrix."""
import ctypes
import gc

import numpy as np
import pytest

from qcc_amd import device, gates, native, workloads
from qcc_amd.lib import backend, circuit, ops, tensor
from tests.test_dense_cpu import dense_reference
from tests import oracle_lib

pytestmark = pytest.mark.gpu


def _rand_op(rng, k, unitary=True):
  a = rng.normal(size=(1 << k, 1 << k)) + 1j * rng.normal(size=(1 << k, 1 << k))
  if unitary:
    a, _ = np.linalg.qr(a)
  return a


def _rand_state(rng, n):
  v = rng.normal(size=1 << n) + 1j * rng.normal(size=1 << n)
  return v / np.linalg.norm(v)


def _bitmap(st, n):
  bm = (ctypes.c_int32 * n)()
  native.check(st.lib.qh_get_bitmap(st.h, bm))
  return list(bm)


def _check(got, want, bw):
  got = np.asarray(got, dtype=np.complex128)
  if bw == 128:
    err = float(np.max(np.abs(got - want)))
    assert err < 1e-12, err
  else:
    err = float(np.linalg.norm(got - want) / np.linalg.norm(want))
    assert err < 1e-5, err


def _case(rng, n, k, nctl):
  """targets (unordered) and controls; line bits 0/1 are likely among the controls"""
  bits = [int(b) for b in rng.permutation(n)[:k]]
  free = [b for b in range(n) if b not in bits]
  low = [b for b in free if b < 2]
  ctl = []
  for _ in range(min(nctl, len(free))):
    pool = low if (low and rng.random() < 0.6) else free
    c = int(pool[int(rng.integers(len(pool)))])
    if c not in ctl:
      ctl.append(c)
    low = [b for b in low if b not in ctl]
    free = [b for b in free if b not in ctl]
  return bits, sum(1 << c for c in ctl)


@pytest.mark.parametrize('bw', [128, 64])
@pytest.mark.parametrize('fusion', [native.QH_FUSE_OFF, native.QH_FUSE_SWEEP])
def test_small_registers_every_k(bw, fusion):
  rng = np.random.default_rng(bw + 7 * fusion)
  o = oracle_lib.load()
  h_gate, ry = np.asarray(gates.hadamard(), np.complex128), np.asarray(gates.ry(0.7), np.complex128)
  dtype = np.complex128 if bw == 128 else np.complex64
  for k in range(1, 7):
    for n in sorted({k, k + 2, 11, 20}):
      for nctl in (0, 1, 2):
        if k + nctl > n:
          continue
        bits, ctl = _case(rng, n, k, nctl)
        m = _rand_op(rng, k, unitary=bool(rng.integers(2)))
        psi = _rand_state(rng, n)
        want = psi.copy()
        with device.DeviceState(n, bw, fusion=fusion) as st:
          st.upload(psi.astype(dtype))
          st.apply1(h_gate, 0)                       # queued (fusion on) before the call
          o.apply1(want, h_gate, n, 0)
          st.apply_matrix(m, bits, ctl)
          want = dense_reference(want, n, m, bits, ctl)
          st.apply1(ry, n - 1)                       # and after it
          o.apply1(want, ry, n, n - 1)
          _check(st.download(), want, bw)


@pytest.mark.parametrize('bw', [128, 64])
def test_host_mapped_handle(bw):
  rng = np.random.default_rng(3)
  dtype = np.complex128 if bw == 128 else np.complex64
  for k, n in ((2, 9), (4, 12), (6, 13)):
    bits, ctl = _case(rng, n, k, 1)
    m = _rand_op(rng, k)
    psi = _rand_state(rng, n)
    with device.DeviceState(n, bw, host_mapped=True) as st:
      st.upload(psi.astype(dtype))
      st.apply_matrix(m, bits, ctl)
      st.sync()
      _check(st.host_array().copy(), dense_reference(psi, n, m, bits, ctl), bw)


def test_permuted_layout_and_readers():
  from tests.test_gpu_relayout import _high_bit_circuit   # (a circuit whose sweeps re-lay the state out)
  n = 22
  rng = np.random.default_rng(9)
  ops_, g8 = _high_bit_circuit(n, 7)
  psi = _rand_state(rng, n)
  want = psi.copy()
  oracle_lib.load().run_stream(want, n, ops_, g8)
  m = _rand_op(rng, 5, unitary=False)
  bits, ctl = [17, 0, 21, 2, 9], (1 << 1) | (1 << 12)
  want = dense_reference(want, n, m, bits, ctl)
  with device.DeviceState(n, 128, fusion=native.QH_FUSE_SWEEP) as st:
    st.upload(psi)
    st.run_stream(ops_, g8)
    st.flush()
    bm = _bitmap(st, n)
    assert bm != list(range(n)), 'the sweeps should have left a permuted bit map'
    st.apply_matrix(m, bits, ctl)
    assert _bitmap(st, n) == bm                       # the call works on the layout it finds
    for i in (0, 12345, (1 << n) - 1, int(np.argmax(np.abs(want)))):
      assert abs(st.amplitude(i) - want[i]) < 1e-12
    idx = np.arange(1 << n)
    for b in (0, 2, 9, 17, 21):
      p1 = float(np.sum(np.abs(want[(idx >> b) & 1 == 1]) ** 2))
      assert abs(st.prob_bit(b) - p1) < 1e-12
    _check(st.download(), want, 128)


def test_exact_permutation_and_tensor_product():
  rng = np.random.default_rng(21)
  n = 14
  psi = _rand_state(rng, n)
  for k in range(1, 7):
    bits = [int(b) for b in rng.permutation(n)[:k]]
    shift = np.roll(np.eye(1 << k), 1, axis=0)       # |c> -> |c + 1 mod 2^k>
    with device.DeviceState(n, 128) as st:
      st.upload(psi)
      st.apply_matrix(shift, bits)
      got = st.download()
    idx = np.arange(1 << n)
    c = np.zeros_like(idx)
    for j, b in enumerate(bits):
      c |= ((idx >> b) & 1) << j
    src = idx.copy()
    cm = (c - 1) % (1 << k)
    for j, b in enumerate(bits):
      src = (src & ~(1 << b)) | (((cm >> j) & 1) << b)
    assert np.array_equal(got, psi[src])             # exactly the permuted amplitudes
    gs = [np.asarray(_rand_op(rng, 1)) for _ in range(k)]
    prod = np.ones((1, 1))
    for g in reversed(gs):                           # matrix bit j <-> gs[j]: the least significant factor last
      prod = np.kron(prod, g)
    with device.DeviceState(n, 128) as a, device.DeviceState(n, 128) as b:
      a.upload(psi)
      b.upload(psi)
      a.apply_matrix(prod, bits)
      for j, g in enumerate(gs):
        b.apply_bits(0, bits[j], g)
      assert np.max(np.abs(a.download() - b.download())) < 1e-13


def test_queued_matrices_each_take_effect():
  rng = np.random.default_rng(5)
  n = 16
  psi = _rand_state(rng, n)
  ms = [_rand_op(rng, 6, unitary=False) / 8 for _ in range(12)]   # more than the staging ring holds
  bits = [[int(b) for b in rng.permutation(n)[:6]] for _ in ms]
  want = psi.copy()
  with device.DeviceState(n, 128) as st:
    st.upload(psi)
    lib = st.lib
    buf = np.zeros((64, 64), dtype=np.complex128)
    for m, b in zip(ms, bits):
      buf[:] = m
      bb = np.asarray(b, dtype=np.int32)
      native.check(lib.qh_apply_matrix(st.h, 6, bb.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), 0,
                                       buf.ctypes.data_as(ctypes.POINTER(ctypes.c_double))))
      buf[:] = np.nan                                # the caller's buffer is overwritten right away
      want = dense_reference(want, n, m, b)
    _check(st.download(), want, 128)


def test_sharded_handles():
  rng = np.random.default_rng(13)
  n, nl = 20, 19
  psi = _rand_state(rng, n)
  m = _rand_op(rng, 3)
  shards = [device.DeviceState(nl, 128) for _ in range(2)]
  try:
    for s, st in enumerate(shards):
      st.set_shard(n, s)
      st.upload(psi[s << nl:(s + 1) << nl])
    for st in shards:
      with pytest.raises(native.QhError) as e:
        st.apply_matrix(m, [3, 19, 0])
      assert e.value.code == native.QH_ERR_NONLOCAL
    assert np.array_equal(np.concatenate([st.download() for st in shards]), psi)
    bits, ctl = [3, 10, 0], (1 << 19) | (1 << 1)
    for st in shards:
      st.reset_stats()
      st.apply_matrix(m, bits, ctl)
    assert shards[0].stats()['gates_noop'] == 1 and shards[0].stats()['kernels_launched'] == 0
    assert shards[1].stats()['kernels_launched'] == 1
    got = np.concatenate([st.download() for st in shards])
    assert np.max(np.abs(got - dense_reference(psi, n, m, bits, ctl))) < 1e-12
  finally:
    for st in shards:
      st.close()


def test_full_state_30_qubits():
  """Whole 2^30 states in HBM against torch: the QFT of a basis state (closed form), then k = 2 on the two highest bits
  and k = 5 on bits including 0-2 (tests/test_gpu_fullstate.py's bounds for complex128)."""
  import torch
  from tests import torch_reference as tr
  n, x = 30, 0x1B2CB9A5
  rng = np.random.default_rng(30)
  qft_ops, qft_g8 = workloads.qft_stream(range(n)).arrays()
  m2, m5 = _rand_op(rng, 2), _rand_op(rng, 5)
  bits5 = [2, 0, 6, 1, 4]
  # k = 5 on bits < 8: one 256 x 256 matrix on rows of 256 consecutive amplitudes
  blk = np.stack([dense_reference(np.eye(256)[c], 8, m5, bits5) for c in range(256)], axis=1)
  blk_t = torch.from_numpy(blk.T.copy()).to('cuda')
  m2_t = torch.from_numpy(m2).to('cuda')
  qft = lambda off, cnt: tr.qft_closed_form(n, x, off, cnt, 'cuda')              # noqa: E731

  def ref(off, cnt):
    # chunks of 2^24 keep bits 28, 29 fixed: out = sum_c M2[r][c] * (the chunk with those bits = c)
    r = off >> 28
    low = off & ((1 << 28) - 1)
    acc = None
    for c in range(4):
      t = m2_t[r, c] * qft((c << 28) | low, cnt)
      acc = t if acc is None else acc + t
    return (acc.view(-1, 256) @ blk_t).reshape(-1)

  try:
    with device.DeviceState(n, 128, fusion=native.QH_FUSE_SWEEP) as st:
      st.init_basis(x)
      st.run_stream(qft_ops, qft_g8)
      st.apply_matrix(m2, [28, 29])
      st.reset_stats()
      st.apply_matrix(m5, bits5)
      s = st.stats()
      assert s['kernels_launched'] == 1 and s['bytes_algorithmic'] == 2 * 16 << n
      r = tr.compare(st, ref)
    print(f'dense 30q: {r}')
    assert r['max_abs'] <= 1e-10 and r['rel_l2'] <= 1e-12
  finally:
    del blk_t, m2_t
    gc.collect()
    torch._C._cuda_clearCublasWorkspaces()        # the reference's matmul left a BLAS workspace in torch's cache
    torch.cuda.empty_cache()
  assert torch.cuda.memory_reserved() == 0


@pytest.fixture
def width128():
  tensor.set_tensor_width(128)
  yield
  tensor.set_tensor_width(None)


def test_qc_unitary_24_qubits_on_the_device(width128, monkeypatch):
  """At 24 qubits the host path builds 2^24 x 2^24 identities with np.kron (MemoryError after many GiB); the device path
  launches one kernel and never downloads the state."""
  n, idx = 24, 2
  rng = np.random.default_rng(24)
  u = _rand_op(rng, 3)
  q = circuit.qc('u24')
  q.reg(n, 0)
  for i in range(6):
    q.h(i)
  q.ry(20, 0.3)
  q.sync()
  want = np.asarray(q.psi).copy()
  q._dev.reset_stats()                                                  # pylint: disable=protected-access
  with monkeypatch.context() as mp:
    mp.setattr(device.DeviceState, 'download', lambda *a, **k: pytest.fail('qc.unitary downloaded the state'))
    mp.setattr(ops.Operator, 'apply', lambda *a, **k: pytest.fail('qc.unitary took the host path'))
    q.unitary(u, idx)
    q.sync()
    assert q._dev.stats()['kernels_launched'] == 1                      # pylint: disable=protected-access
  want = dense_reference(want, n, u, [n - idx - 3 + j for j in range(3)])
  assert np.max(np.abs(np.asarray(q.psi) - want)) < 1e-12
  q.close()
  backend.drop_device_pool()


def test_qc_unitary_controlled_u_matches_host_path(width128):
  """hhl-style: ControlledU spanning 5 qubits (control, 3 idle, target) on a 10-qubit register."""
  rng = np.random.default_rng(10)
  cu = ops.ControlledU(0, 4, ops.Operator(_rand_op(rng, 1)))
  assert cu.shape == (32, 32)
  q = circuit.qc('cu')
  q.reg(10, 0)
  for i in range(10):
    q.ry(i, float(rng.uniform(0, np.pi)))
  before = q.psi
  q.unitary(cu, 3)
  want = ops.Operator(cu)(before, 3)
  assert np.max(np.abs(np.asarray(q.psi) - np.asarray(want))) < 1e-12
  q.apply_matrix(cu, [3, 4, 5, 6, 7])                                   # the general form of the same call
  want = ops.Operator(cu)(want, 3)
  assert np.max(np.abs(np.asarray(q.psi) - np.asarray(want))) < 1e-12
  q.close()
  backend.drop_device_pool()
