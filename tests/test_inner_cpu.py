"""CPU tests of the two-state operations: the C-ABI symbols and their argument checks (NULL, planner-only handles), the host
side of qh_inner (qh_inner_plan on planner-only handles: insert positions and in-tile shuffle from two bit maps, checked
exhaustively against a NumPy model of the tile walk; the same code stand-alone under sanitizers), and qc.snapshot / restore /
overlap / fidelity over the NumPy stand-in device, which has none of clone / copy_from / inner."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from qcc_amd import device, native
from qcc_amd.lib import backend, circuit, tensor
from tests import fake_device, inner_util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the C-ABI ---------------------------------------------------------------------------------------------------------
def test_version_and_symbols_bound():
  lib = native.load()
  assert lib.qh_version() >= 110
  for name in ('qh_clone', 'qh_copy', 'qh_inner', 'qh_inner_plan'):
    assert name in native.SIGNATURES
    assert getattr(lib, name).argtypes == native.SIGNATURES[name][1]


def test_null_and_dry_handles_are_argument_errors():
  lib = native.load()
  d1, d2 = ctypes.c_void_p(), ctypes.c_void_p()
  native.check(lib.qh_create_dry(10, 128, ctypes.byref(d1)))
  native.check(lib.qh_create_dry(10, 128, ctypes.byref(d2)))
  try:
    out = (ctypes.c_double * 2)(7.0, 7.0)
    new = ctypes.c_void_p()
    assert lib.qh_clone(None, ctypes.byref(new)) == native.QH_ERR_ARG
    assert lib.qh_clone(d1, None) == native.QH_ERR_ARG
    assert lib.qh_clone(d1, ctypes.byref(new)) == native.QH_ERR_ARG and b'dry' in lib.qh_last_error()
    assert not new.value
    assert lib.qh_copy(None, d1) == native.QH_ERR_ARG
    assert lib.qh_copy(d1, None) == native.QH_ERR_ARG
    assert lib.qh_copy(d1, d2) == native.QH_ERR_ARG and b'dry' in lib.qh_last_error()
    assert lib.qh_inner(None, d1, out) == native.QH_ERR_ARG
    assert lib.qh_inner(d1, None, out) == native.QH_ERR_ARG
    assert lib.qh_inner(d1, d2, out) == native.QH_ERR_ARG and b'dry' in lib.qh_last_error()
    assert lib.qh_inner(d1, d1, out) == native.QH_ERR_ARG
    assert list(out) == [7.0, 7.0]
    assert lib.qh_inner_plan(d1, d2, None) == native.QH_ERR_ARG
    assert lib.qh_inner_plan(None, d2, ctypes.byref(native.QhInnerTiles())) == native.QH_ERR_ARG
  finally:
    lib.qh_destroy(d1)
    lib.qh_destroy(d2)


# ---- the tile planner ----------------------------------------------------------------------------------------------------
def _dry_pair(nloc, swaps_a, swaps_b, nglob=None):
  a, b = device.DeviceState(nloc, 128, dry=True), device.DeviceState(nloc, 128, dry=True)
  if nglob:
    a.set_shard(nglob, 1)
    b.set_shard(nglob, 1)
  for st, swaps in ((a, swaps_a), (b, swaps_b)):
    for x, y in swaps:
      st.remap_swap(x, y)
  return a, b


def _bitmap(st, n):
  bm = (ctypes.c_int32 * 64)()
  native.check(st.lib.qh_get_bitmap(st.h, bm))
  return list(bm)[:n]


def _check_plan(nloc, a, b):
  plan = a.inner_plan(b)
  pa, pb = _bitmap(a, nloc), _bitmap(b, nloc)
  want = inner_util.expected_pairs(pa, pb, nloc)
  assert plan['pos_b'][:nloc] == [pb[pa.index(p)] for p in range(nloc)]
  if pa == pb:
    assert plan['path'] == native.QH_INNER_LINEAR
  elif nloc < 8:
    assert plan['path'] == native.QH_INNER_GATHER
    got = inner_util.spread(np.arange(1 << nloc), plan['pos_b'][:nloc])
    assert np.array_equal(got, want)
  else:
    assert plan['path'] == native.QH_INNER_TILES
    # both tiles hold bits 0..3 (runs of 16 amplitudes in either state), b's contains a's low four
    assert plan['tile_a'][:4] == [0, 1, 2, 3] and plan['tile_b'][:4] == [0, 1, 2, 3]
    assert sorted(plan['tile_a']) == plan['tile_a'] and sorted(plan['tile_b']) == plan['tile_b']
    assert plan['free_a'] == sum(1 << p for p in plan['tile_a']) and plan['free_b'] == sum(1 << p for p in plan['tile_b'])
    assert {pa[pb.index(q)] for q in range(4)} <= set(plan['tile_a'])
    assert sorted(plan['rest_a'][:nloc - 8]) == plan['rest_a'][:nloc - 8]
    ia, ib = inner_util.tile_pairs(plan, nloc)
    # every index of each state exactly once, and paired as the bit maps say
    assert np.array_equal(np.sort(ia), np.arange(1 << nloc, dtype=np.uint64))
    assert np.array_equal(np.sort(ib), np.arange(1 << nloc, dtype=np.uint64))
    assert np.array_equal(want[ia.astype(np.int64)], ib)
  return plan


@pytest.mark.parametrize('nloc', [4, 7, 8, 9, 12, 16])
def test_plan_hand_made_maps(nloc):
  paths = set()
  for _name, sa, sb in [('same', [], [])] + inner_util.hand_maps(nloc):
    a, b = _dry_pair(nloc, sa, sb)
    try:
      paths.add(_check_plan(nloc, a, b)['path'])
      _check_plan(nloc, b, a)
    finally:
      a.close()
      b.close()
  assert paths == {native.QH_INNER_LINEAR, native.QH_INNER_GATHER if nloc < 8 else native.QH_INNER_TILES}


def test_plan_disjoint_and_padded_tiles():
  a, b = _dry_pair(12, [], [(k, 8 + k) for k in range(4)])
  plan = _check_plan(12, a, b)
  assert plan['tile_a'] == [0, 1, 2, 3, 8, 9, 10, 11] and plan['tile_b'] == plan['tile_a']        # t = 8: nothing to pad
  a.close()
  b.close()
  a, b = _dry_pair(12, [], [(0, 3), (1, 2)])
  plan = _check_plan(12, a, b)
  assert plan['tile_a'] == list(range(8)) and plan['tile_b'] == list(range(8))                     # t = 4, padded with 4..7
  a.close()
  b.close()


@pytest.mark.parametrize('nloc', range(8, 15))
def test_plan_random_permutations(nloc):
  """200 random pairs of layouts per size: the permutations are reached through swaps, as the engine's bit maps are"""
  rng = np.random.default_rng(1000 + nloc)
  a, b = _dry_pair(nloc, [], [])
  try:
    for _ in range(200):
      for st in (a, b):
        for p in range(nloc - 1, 0, -1):      # a Fisher-Yates shuffle of the positions, on top of the map the state has
          st.remap_swap(p, int(rng.integers(0, p + 1)))
      _check_plan(nloc, a, b)
  finally:
    a.close()
    b.close()


def test_plan_shard_bits():
  lib = native.load()
  t = native.QhInnerTiles()
  a, b = _dry_pair(10, [], [(2, 7)], nglob=12)
  try:
    assert _check_plan(10, a, b)['path'] == native.QH_INNER_TILES       # shard bits where they were: local bits anywhere
    b.remap_swap(3, 11)                                                  # one handle now holds another logical bit in the shard index
    assert lib.qh_inner_plan(a.h, b.h, ctypes.byref(t)) == native.QH_ERR_NONLOCAL
    assert b'exchange first' in lib.qh_last_error()
    b.remap_swap(3, 11)
    b.remap_swap(10, 11)                                                 # the same bits, at other shard positions
    assert lib.qh_inner_plan(a.h, b.h, ctypes.byref(t)) == native.QH_ERR_NONLOCAL
    b.remap_swap(10, 11)
    b.set_shard(12, 2)                                                   # another shard of the same state
    assert lib.qh_inner_plan(a.h, b.h, ctypes.byref(t)) == native.QH_ERR_NONLOCAL
    c = device.DeviceState(11, 128, dry=True)
    assert lib.qh_inner_plan(a.h, c.h, ctypes.byref(t)) == native.QH_ERR_ARG
    c.close()
  finally:
    a.close()
    b.close()


def test_planner_stand_alone_under_sanitizers(tmp_path):
  """qcc_amd/csrc/inner_plan.h is plain C++: the same permutations through a stand-alone program built with
  AddressSanitizer and UndefinedBehaviorSanitizer.  The sanitizer runtimes are linked statically, so the program runs in
  whatever environment this process has, unchanged (host code only; nothing is loaded into this process)."""
  cxx = shutil.which('g++') or shutil.which('clang++')
  assert cxx, 'no host C++ compiler'
  static = ['-static-libasan', '-static-libubsan'] if os.path.basename(cxx).startswith('g++') else ['-static-libsan']
  exe = str(tmp_path / 'inner_plan_check')
  subprocess.check_call([cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', *static,
                         os.path.join(ROOT, 'tools', 'inner_plan_check.cc'), '-o', exe])
  res = subprocess.run([exe, '40'], capture_output=True, text=True, timeout=120)
  assert res.returncode == 0, res.stdout + res.stderr
  assert 'ok' in res.stdout


# ---- qc.snapshot / restore / overlap / fidelity on the NumPy stand-in ----------------------------------------------------
@pytest.fixture(params=[128, 64])
def cpu_backend(request):
  tensor.set_tensor_width(request.param)
  backend.set_device_factory(fake_device.OracleDevice)
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


def test_fallback_overlap_and_fidelity(cpu_backend):
  tol = 1e-12 if cpu_backend == 128 else 1e-5
  a, b = _circuit(6, 1), _circuit(6, 2)
  assert not hasattr(a._ensure_device(), 'inner')
  pa, pb = np.asarray(a.psi).reshape(-1), np.asarray(b.psi).reshape(-1)
  want = complex(np.vdot(pa, pb))
  assert abs(a.overlap(b) - want) < tol
  assert abs(b.overlap(a) - np.conj(want)) < tol
  assert abs(a.overlap(a) - np.vdot(pa, pa)) < tol
  b.psi = np.asarray(pb) * 0.5                      # fidelity divides by both norms
  assert abs(b.fidelity(a) - abs(want) ** 2 / (np.vdot(pa, pa).real * np.vdot(pb, pb).real)) < 10 * tol
  assert abs(a.fidelity(a) - 1.0) < 10 * tol
  with pytest.raises(ValueError):
    a.overlap(_circuit(5, 3))
  with pytest.raises(ValueError):
    a.overlap(pa)
  with pytest.raises(ValueError):
    a.fidelity('psi')


def test_fallback_snapshot_restore(cpu_backend):
  tol = 1e-12 if cpu_backend == 128 else 1e-5
  q = _circuit(6, 4)
  before = np.array(q.psi).reshape(-1)
  with q.snapshot() as snap:
    assert isinstance(snap, circuit.Snapshot) and snap.nbits == 6 and snap.width == cpu_backend
    q.h(2)
    q.cx(1, 4)
    assert abs(q.overlap(snap) - np.vdot(np.asarray(q.psi).reshape(-1), before)) < tol
    assert abs(q.fidelity(snap) - abs(np.vdot(np.asarray(q.psi).reshape(-1), before)) ** 2) < 10 * tol
    q.measure([0, 3], seed=5)
    q.x(5)                                          # still queued on the host side when the snapshot comes back: dropped
    q.restore(snap)
    assert np.array_equal(np.asarray(q.psi).reshape(-1), before)
    q.h(0)                                          # the circuit goes on from the restored state
    q.h(0)
    assert np.allclose(np.asarray(q.psi).reshape(-1), before, atol=tol)
    with pytest.raises(ValueError):
      _circuit(5, 1).restore(snap)
    with pytest.raises(ValueError):
      q.restore(before)
  with pytest.raises(ValueError):
    q.restore(snap)                                 # closed
  with pytest.raises(ValueError):
    q.overlap(snap)
