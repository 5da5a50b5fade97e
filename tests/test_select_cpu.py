"""CPU tests of the sparse readout: the C-ABI symbols and their argument checks (NULL and planner-only handles, nothing
written), the host side of qh_topk stand-alone under sanitizers (select_plan.h against a sort), qc.support / top / ampls /
probs / dump and _LazyPsi.dump over a NumPy stand-in device that is never downloaded, and ShardedDevice.select / topk /
amplitudes over gloo (world sizes 2 and 4) against the single-process answer."""
import contextlib
import ctypes
import io
import os
import shutil
import socket
import subprocess

import numpy as np
import pytest
import torch.multiprocessing as mp

from qcc_amd import device, native, sharded
from qcc_amd.lib import backend, circuit, state, tensor
from tests import fake_device, select_util
from tests.select_util import SelectOracle, SelectShardEngine, fma_probs, np_select, np_topk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_dp = ctypes.POINTER(ctypes.c_double)
_up = ctypes.POINTER(ctypes.c_uint64)


# ---- the C-ABI ---------------------------------------------------------------------------------------------------------
def test_version_and_symbols_bound():
  lib = native.load()
  assert lib.qh_version() >= 113
  for name in ('qh_select', 'qh_topk', 'qh_amplitudes'):
    assert name in native.SIGNATURES
    assert getattr(lib, name).argtypes == native.SIGNATURES[name][1]
  assert ctypes.sizeof(native.QhEntry) == 24
  assert native.QH_SELECT_MAX == 1 << 20 and native.QH_TOPK_MAX == 4096


@pytest.fixture
def dry():
  lib = native.load()
  h = ctypes.c_void_p()
  native.check(lib.qh_create_dry(10, 128, ctypes.byref(h)))
  yield h
  lib.qh_destroy(h)


def _sentinel_entries(n):
  buf = (native.QhEntry * n)()
  for e in buf:
    e.index, e.re, e.im = 77, 7.0, -7.0
  return buf


def _untouched(buf):
  return all((e.index, e.re, e.im) == (77, 7.0, -7.0) for e in buf)


def test_select_argument_errors(dry):
  lib = native.load()
  buf = _sentinel_entries(4)
  cnt, w = ctypes.c_uint64(99), ctypes.c_double(9.5)
  args = (ctypes.byref(cnt), ctypes.byref(w))
  assert lib.qh_select(None, 0.1, 4, buf, *args) == native.QH_ERR_ARG
  assert lib.qh_select(dry, 0.1, 4, buf, None, ctypes.byref(w)) == native.QH_ERR_ARG
  assert lib.qh_select(dry, -1e-300, 4, buf, *args) == native.QH_ERR_ARG
  assert b'threshold' in lib.qh_last_error()
  assert lib.qh_select(dry, float('nan'), 4, buf, *args) == native.QH_ERR_ARG
  assert lib.qh_select(dry, 0.1, native.QH_SELECT_MAX + 1, buf, *args) == native.QH_ERR_ARG
  assert b'QH_SELECT_MAX' in lib.qh_last_error()
  assert lib.qh_select(dry, 0.1, 4, None, *args) == native.QH_ERR_ARG
  assert lib.qh_select(dry, 0.1, 4, buf, *args) == native.QH_ERR_ARG and b'dry' in lib.qh_last_error()
  assert lib.qh_select(dry, 0.0, 0, None, *args) == native.QH_ERR_ARG and b'dry' in lib.qh_last_error()     # count only
  assert _untouched(buf) and cnt.value == 99 and w.value == 9.5


def test_topk_argument_errors(dry):
  lib = native.load()
  buf = _sentinel_entries(4)
  cnt = ctypes.c_uint64(99)
  assert lib.qh_topk(None, 4, buf, ctypes.byref(cnt)) == native.QH_ERR_ARG
  assert lib.qh_topk(dry, 4, buf, None) == native.QH_ERR_ARG
  assert lib.qh_topk(dry, 4, None, ctypes.byref(cnt)) == native.QH_ERR_ARG
  assert lib.qh_topk(dry, native.QH_TOPK_MAX + 1, buf, ctypes.byref(cnt)) == native.QH_ERR_ARG
  assert b'QH_TOPK_MAX' in lib.qh_last_error()
  assert lib.qh_topk(dry, 4, buf, ctypes.byref(cnt)) == native.QH_ERR_ARG and b'dry' in lib.qh_last_error()
  assert lib.qh_topk(dry, 0, None, ctypes.byref(cnt)) == native.QH_ERR_ARG and b'dry' in lib.qh_last_error()
  assert _untouched(buf) and cnt.value == 99


def test_amplitudes_argument_errors(dry):
  lib = native.load()
  idx = np.array([0, 5, 1023], dtype=np.uint64)
  out = np.full(6, 7.0)
  nl = ctypes.c_uint64(99)

  def call(h, count, ip, op):
    return lib.qh_amplitudes(h, count, ip, op, ctypes.byref(nl))
  ip, op = idx.ctypes.data_as(_up), out.ctypes.data_as(_dp)
  assert call(None, 3, ip, op) == native.QH_ERR_ARG
  assert call(dry, 3, None, op) == native.QH_ERR_ARG
  assert call(dry, 3, ip, None) == native.QH_ERR_ARG
  assert call(dry, (1 << 24) + 1, ip, op) == native.QH_ERR_ARG and b'2^24' in lib.qh_last_error()
  bad = np.array([0, 1024, 3], dtype=np.uint64)                       # 2^nbits_global
  assert call(dry, 3, bad.ctypes.data_as(_up), op) == native.QH_ERR_ARG and b'out of range' in lib.qh_last_error()
  assert call(dry, 3, ip, op) == native.QH_ERR_ARG and b'dry' in lib.qh_last_error()
  assert call(dry, 0, None, None) == native.QH_ERR_ARG and b'dry' in lib.qh_last_error()
  assert np.all(out == 7.0) and nl.value == 99


def test_device_state_wrappers_refuse_dry_handles():
  st = device.DeviceState(12, 128, dry=True)
  try:
    for call in (lambda: st.select(0.1), lambda: st.select(0.0, 0), lambda: st.topk(3), lambda: st.amplitudes([1, 2])):
      with pytest.raises(native.QhError) as e:
        call()
      assert e.value.code == native.QH_ERR_ARG
  finally:
    st.close()


def test_fma_probs_is_the_fused_form():
  # re * re rounds, the sum with im * im does not round twice: differs from the two-rounding form on some inputs
  rng = np.random.default_rng(3)
  a = rng.standard_normal(2000) + 1j * rng.standard_normal(2000)
  got = sharded.fma_probs(a)
  assert np.array_equal(got, fma_probs(a))
  plain = a.real * a.real + a.imag * a.imag
  assert np.max(np.abs(got - plain)) <= np.max(np.spacing(plain))
  assert np.any(got != plain)
  assert sharded.fma_probs([3 + 4j, 0j]).tolist() == [25.0, 0.0]
  # float32-valued amplitudes at a QFT's scale, tiny and huge ones (the rational fallback), a power of two
  b = np.concatenate([(a.astype(np.complex64).astype(np.complex128)) * 2.0 ** -10, a * 1e-160, a * 1e152, [2.0 ** -10 * (1 + 1j)]])
  assert np.array_equal(sharded.fma_probs(b), np.array([select_util.fma_prob(z) for z in b]))


# ---- select_plan.h stand-alone ---------------------------------------------------------------------------------------------
def test_select_plan_stand_alone_under_sanitizers(tmp_path):
  """qcc_amd/csrc/select_plan.h is plain C++: synthetic histograms (peaked, flat with all mass in one bin, k at a bin edge,
  k larger than the support, random mixtures) through a stand-alone program built with AddressSanitizer and
  UndefinedBehaviorSanitizer; the chosen key ranges are checked against a sort.  Host code only; nothing is loaded into
  this process."""
  cxx = shutil.which('g++') or shutil.which('clang++')
  assert cxx, 'no host C++ compiler'
  static = ['-static-libasan', '-static-libubsan'] if os.path.basename(cxx).startswith('g++') else ['-static-libsan']
  exe = str(tmp_path / 'select_plan_check')
  subprocess.check_call([cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', *static,
                         os.path.join(ROOT, 'tools', 'select_plan_check.cc'), '-o', exe])
  res = subprocess.run([exe, '24'], capture_output=True, text=True, timeout=120)
  assert res.returncode == 0, res.stdout + res.stderr
  assert 'ok' in res.stdout


# ---- qc on a NumPy device --------------------------------------------------------------------------------------------------
@pytest.fixture(params=[128, 64])
def cpu_backend(request):
  tensor.set_tensor_width(request.param)
  backend.set_device_factory(SelectOracle)
  SelectOracle.downloads = 0
  yield request.param
  backend.set_device_factory(None)
  tensor.set_tensor_width(None)


def _resident(psi):
  """a circuit whose state `psi` lives on the stand-in device only (no host copy)"""
  n = int(np.log2(len(psi)))
  q = circuit.qc('sel')
  q.reg(n, 0)
  dev = q._ensure_device()                                # pylint: disable=protected-access
  dev.upload(np.asarray(psi))
  q._is_product = False                                   # pylint: disable=protected-access
  q._host_ok = False                                      # pylint: disable=protected-access
  assert q._sparse_device() is dev                        # pylint: disable=protected-access
  return q, dev


def _quadrant_state(n, seed, width):
  """A normalised state whose amplitudes have phases in all four quadrants, magnitudes from a few well-separated levels
  (many of them far below the print threshold), and no probability within 1e-9 of that threshold."""
  rng = np.random.default_rng(seed)
  size = 1 << n
  level = rng.choice([1.0, 0.5, 0.05, 1e-4, 0.0], size=size, p=[0.1, 0.2, 0.2, 0.3, 0.2])
  quadrant = rng.integers(4, size=size)
  where = rng.choice(size, 4, replace=False)              # one large amplitude in each quadrant, wherever
  level[where], quadrant[where] = 1.0, np.arange(4)
  mag = level * (0.75 + 0.5 * rng.random(size))
  phase = (quadrant * 0.5 + 0.05 + 0.4 * rng.random(size)) * np.pi
  a = mag * np.exp(1j * phase)
  a = (a / np.linalg.norm(a)).astype(np.complex128 if width == 128 else np.complex64)
  p = np.abs(a.astype(np.complex128)) ** 2
  assert np.all(np.abs(p - state.DUMP_MIN_PROB) > 1e-9)
  assert {(x.real > 0, x.imag > 0) for x in a[p > 1e-3]} == {(True, True), (True, False), (False, True), (False, False)}
  return a


def _printed(fn, *a, **kw):
  out = io.StringIO()
  with contextlib.redirect_stdout(out):
    fn(*a, **kw)
  return out.getvalue()


@pytest.mark.parametrize('n', range(3, 11))
def test_dump_is_byte_identical_to_state_dump(cpu_backend, n):
  a = _quadrant_state(n, 100 + n, cpu_backend)
  want_state = state.State(a.copy())
  q, _ = _resident(a)
  q.name = None
  want = _printed(want_state.dump, 'Current state')
  assert len(want.splitlines()) > 2
  assert _printed(q.dump) == want
  lazy = circuit._LazyPsi(q)                              # pylint: disable=protected-access
  assert _printed(lazy.dump, 'Current state') == want
  assert _printed(lazy.dump) == _printed(want_state.dump)
  assert _printed(lazy.dump, 'all', prob_only=False) == _printed(want_state.dump, 'all', prob_only=False)
  assert lazy._snap is None                               # pylint: disable=protected-access
  assert SelectOracle.downloads == 0


def test_support_top_ampls_probs_against_numpy(cpu_backend):
  a = _quadrant_state(8, 5, cpu_backend)
  q, _ = _resident(a)
  wide = a.astype(np.complex128)
  p = fma_probs(wide)
  for thr in (1e-5, 1e-3, 0.0, 2.0):
    got = q.support(thr)
    idx, amp, _ = np_select(wide, thr)
    assert [circuit.helper.bits2val(b) for b, _, _ in got] == idx.tolist()
    assert [len(b) for b, _, _ in got] == [8] * idx.size
    assert np.array_equal(np.array([x for _, x, _ in got], dtype=np.complex128), amp)
    np.testing.assert_allclose([pr for _, _, pr in got], p[idx.astype(np.int64)], rtol=1e-15, atol=0)
  for k in (0, 1, 7, 256, 300):
    got = q.top(k)
    idx, amp = np_topk(wide, k)
    assert [circuit.helper.bits2val(b) for b, _, _ in got] == idx.tolist()
    assert np.array_equal(np.array([x for _, x, _ in got], dtype=np.complex128), amp)
    assert all(pr > 0 for _, _, pr in got)
  assert len(q.top(300)) == int(np.count_nonzero(p)) < 256
  states = [0, 255, (1, 0, 1, 0, 1, 0, 1, 0), [0] * 7 + [1], np.int64(17), 17]
  want = wide[[0, 255, 0b10101010, 1, 17, 17]]
  assert np.array_equal(q.ampls(states), want)
  np.testing.assert_allclose(q.probs(states), np.abs(want) ** 2, rtol=1e-15)
  assert q.ampls([]).size == 0
  with pytest.raises(ValueError):
    q.ampls([256])
  with pytest.raises(ValueError):
    q.top(-1)
  assert SelectOracle.downloads == 0


def test_limit_overflow_names_count_and_weight(cpu_backend):
  a = _quadrant_state(8, 6, cpu_backend)
  q, _ = _resident(a)
  wide = a.astype(np.complex128)
  idx, _, w = np_select(wide, 1e-5)
  with pytest.raises(ValueError) as e:
    q.support(1e-5, limit=idx.size - 1)
  assert str(idx.size) in str(e.value) and f'{w:.6g}' in str(e.value)
  assert len(q.support(1e-5, limit=idx.size)) == idx.size
  # prob_only=False prints every basis state: refused above the default limit of 2^16, through _LazyPsi.dump itself, and
  # the refusal takes no snapshot; the thresholded form of the same 17-qubit state still prints
  big = np.zeros(1 << 17, dtype=np.complex128 if cpu_backend == 128 else np.complex64)
  big[[5, 70000]] = [0.6, -0.8j]
  q2, _ = _resident(big)
  lazy = circuit._LazyPsi(q2)                             # pylint: disable=protected-access
  with pytest.raises(ValueError) as e:
    lazy.dump(prob_only=False)
  assert '2^17' in str(e.value)
  text = _printed(lazy.dump, 'big')
  assert len(text.splitlines()) == 3 and '-0.00-0.80j' in text
  assert lazy._snap is None and SelectOracle.downloads == 0          # pylint: disable=protected-access


def test_devices_without_select_fall_back_to_numpy():
  tensor.set_tensor_width(128)
  backend.set_device_factory(fake_device.MeasureOracle)
  try:
    q = fake_device.readout_circuit(5, 3)
    q.maxprob()                                           # the state is on the device, which cannot select
    assert q._sparse_device() is None                     # pylint: disable=protected-access
    psi = np.asarray(q.psi).astype(np.complex128)
    p = np.abs(psi) ** 2
    thr = float(np.sort(p)[-6])
    assert [circuit.helper.bits2val(b) for b, _, _ in q.support(thr)] == np.flatnonzero(psi.real ** 2 + psi.imag ** 2 >= thr).tolist()
    assert [circuit.helper.bits2val(b) for b, _, _ in q.top(4)] == np.lexsort((np.arange(32), -(psi.real ** 2 + psi.imag ** 2)))[:4].tolist()
    assert np.array_equal(q.ampls([3, (1, 1, 1, 1, 1)]), psi[[3, 31]])
    with pytest.raises(ValueError):
      q.support(0.0, limit=8)
    q.name = None
    assert _printed(q.dump) == _printed(q.psi.dump, 'Current state')
    # a product state that never reached a device: qc.psi's route
    q2 = circuit.qc()
    q2.reg(3, 5)
    assert [(b, pr) for b, _, pr in q2.top(2)] == [([1, 0, 1], 1.0)]
    assert _printed(q2.dump) == _printed(q2.psi.dump, 'Current state')
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
  select_util.sharded_select_worker(
      rank, n, out_dir, lambda nbits, bw: sharded.ShardedDevice(nbits, bw, engine_factory=SelectShardEngine, chunk_amps=16))
  dist.barrier()
  dist.destroy_process_group()


@pytest.mark.parametrize('world,n', [(2, 6), (4, 7)])
def test_sharded_select_equals_single_process(tmp_path, world, n):
  mp.spawn(_sharded_worker, args=(world, _free_port(), n, str(tmp_path)), nprocs=world, join=True)
  select_util.check_sharded_select(tmp_path, world, n)
