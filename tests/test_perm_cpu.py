"""CPU tests of the register permutations: the NumPy reference of qh_apply_perm (checked against the CPU oracle on the tables
that are gates), the two C-ABI symbols and their argument checks on planner-only handles, qh_perm_plan executed with NumPy
tile by tile against the reference (exhaustive register placements up to 8 bits, sampled up to 18, both widths, shard bits),
the planner stand-alone under sanitizers, and qc.permutation / add_const / modadd / modmul / add over a NumPy stand-in device,
with order finding of 7 mod 15 end to end."""
import ctypes
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

from qcc_amd import device, native
from qcc_amd.lib import backend, circuit, tensor
from tests import fake_device, oracle_lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_ip = ctypes.POINTER(ctypes.c_int32)
_up = ctypes.POINTER(ctypes.c_uint32)
X = np.array([[0, 1], [1, 0]], dtype=np.complex128)


def perm_destinations(n, table, bits, ctl_mask=0):
  """where every index goes: i with the register (bit j of its value = bit bits[j] of i) replaced by table[value], for the
  indices that have every bit of ctl_mask set; the others stay"""
  idx = np.arange(1 << n, dtype=np.int64)
  s = np.zeros_like(idx)
  for j, b in enumerate(bits):
    s |= ((idx >> b) & 1) << j
  t = np.asarray(table, dtype=np.int64)[s]
  dst = idx.copy()
  for j, b in enumerate(bits):
    dst = (dst & ~(1 << b)) | (((t >> j) & 1) << b)
  return np.where((idx & ctl_mask) == ctl_mask, dst, idx)


def perm_reference(psi, n, table, bits, ctl_mask=0):
  """new[i with register := table[s(i)]] = old[i] where the controls are met: amplitudes are moved, in psi's own dtype."""
  psi = np.asarray(psi)
  out = np.empty_like(psi)
  out[perm_destinations(n, table, bits, ctl_mask)] = psi
  return out


def _rand_state(rng, n):
  v = rng.normal(size=1 << n) + 1j * rng.normal(size=1 << n)
  return v / np.linalg.norm(v)


# ---- the reference itself ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [2, 5, 9])
def test_reference_matches_oracle_on_tables_that_are_gates(n):
  rng = np.random.default_rng(n)
  o = oracle_lib.load()
  for _ in range(4):
    c, t = (int(v) for v in rng.permutation(n)[:2])          # reference qubits; logical bit = n - 1 - qubit
    psi = _rand_state(rng, n)
    want = psi.copy()
    o.apply1(want, X, n, t)
    assert np.array_equal(perm_reference(psi, n, [1, 0], [n - 1 - t]), want)                     # [1, 0] is X
    want = psi.copy()
    o.applyc(want, X, n, c, t)
    assert np.array_equal(perm_reference(psi, n, [0, 1, 3, 2], [n - 1 - t, n - 1 - c]), want)   # on (tgt, ctl): CNOT
    assert np.array_equal(perm_reference(psi, n, [1, 0], [n - 1 - t], 1 << (n - 1 - c)), want)  # ... and X under a control
    want = psi.copy()
    o.applyc(want, X, n, c, t)
    o.applyc(want, X, n, t, c)
    o.applyc(want, X, n, c, t)
    assert np.array_equal(perm_reference(psi, n, [0, 2, 1, 3], [n - 1 - t, n - 1 - c]), want)   # the swap table: three CNOTs


def test_reference_moves_every_amplitude_once():
  rng = np.random.default_rng(5)
  n, bits = 9, [7, 0, 4, 2]
  table = rng.permutation(16)
  dst = perm_destinations(n, table, bits, 0b100001000)
  assert np.array_equal(np.sort(dst), np.arange(1 << n))
  psi = _rand_state(rng, n).astype(np.complex64)
  out = perm_reference(psi, n, table, bits, 0b100001000)
  assert out.dtype == np.complex64 and np.array_equal(np.sort_complex(out), np.sort_complex(psi))
  inv = np.argsort(table)
  assert np.array_equal(perm_reference(out, n, inv, bits, 0b100001000), psi)


# ---- the C-ABI on planner-only handles -------------------------------------------------------------------------------------
@pytest.fixture
def dry():
  lib = native.load()
  handles = []

  def make(n, nglob=None, shard=0, bw=128):
    h = ctypes.c_void_p()
    native.check(lib.qh_create_dry(n, bw, ctypes.byref(h)))
    if nglob is not None:
      native.check(lib.qh_set_shard(h, nglob, shard))
    handles.append(h)
    return h
  yield make
  for h in handles:
    lib.qh_destroy(h)


def _perm(h, bits, ctl=0, k=None, table='identity'):
  lib = native.load()
  k = len(bits) if k is None else k
  b = (ctypes.c_int32 * max(1, len(bits)))(*bits)
  if table is None:
    return lib.qh_apply_perm(h, k, b, ctl, None)
  t = np.arange(1 << min(max(k, 0), 16), dtype=np.uint32) if isinstance(table, str) else np.asarray(table, dtype=np.uint32)
  return lib.qh_apply_perm(h, k, b, ctl, t.ctypes.data_as(_up))


def _plan(h, bits, ctl=0, k=None):
  lib = native.load()
  b = (ctypes.c_int32 * max(1, len(bits)))(*bits)
  return lib.qh_perm_plan(h, len(bits) if k is None else k, b, ctl, ctypes.byref(native.QhPermTiles()))


def test_symbols_exported_and_bound():
  lib = native.load()
  for name in ('qh_apply_perm', 'qh_perm_plan'):
    assert name in native.SIGNATURES
    assert getattr(lib, name).argtypes == native.SIGNATURES[name][1]
  assert lib.qh_version() >= 114
  assert native.QH_PERM_MAX_BITS == 16


def test_argument_errors_on_dry_handle(dry):
  lib = native.load()
  h = dry(20)
  one = np.arange(2, dtype=np.uint32)
  b1 = (ctypes.c_int32 * 1)(3)
  assert lib.qh_apply_perm(None, 1, b1, 0, one.ctypes.data_as(_up)) == native.QH_ERR_ARG
  assert lib.qh_apply_perm(h, 1, None, 0, one.ctypes.data_as(_up)) == native.QH_ERR_ARG
  assert _perm(h, [1, 2], table=None) == native.QH_ERR_ARG
  assert lib.qh_perm_plan(None, 1, b1, 0, ctypes.byref(native.QhPermTiles())) == native.QH_ERR_ARG
  assert lib.qh_perm_plan(h, 1, None, 0, ctypes.byref(native.QhPermTiles())) == native.QH_ERR_ARG
  assert lib.qh_perm_plan(h, 1, b1, 0, None) == native.QH_ERR_ARG
  for call in (_perm, _plan):
    assert call(h, [], k=0) == native.QH_ERR_ARG
    assert call(h, [], k=-1) == native.QH_ERR_ARG
    assert call(h, list(range(17)), k=17) == native.QH_ERR_ARG
    assert call(h, [0, 20]) == native.QH_ERR_BAD_QUBIT
    assert call(h, [-1, 3]) == native.QH_ERR_BAD_QUBIT
    assert call(h, [0, 3], ctl=1 << 20) == native.QH_ERR_BAD_QUBIT
    assert call(h, [3, 3]) == native.QH_ERR_SAME_QUBIT
    assert call(h, [5, 1, 5]) == native.QH_ERR_SAME_QUBIT
    assert call(h, [5, 5, 20]) == native.QH_ERR_BAD_QUBIT       # both faults: every bit's range is checked first
    assert call(h, [3, 4], ctl=1 << 4) == native.QH_ERR_SAME_QUBIT
  # valid calls: the plan is host arithmetic, the call itself has no state to work on
  assert _plan(h, [2, 5], ctl=1 << 7) == native.QH_OK
  assert _plan(h, list(range(4, 20))) == native.QH_OK
  for rc in (_perm(h, [2, 5]), _perm(h, [7]), _perm(h, list(range(4, 20)), ctl=0b1010)):
    assert rc == native.QH_ERR_ARG
    assert b'dry' in lib.qh_last_error()


def test_non_bijections_name_the_offending_entry(dry):
  lib = native.load()
  h = dry(12)
  assert _perm(h, [0, 5, 2], table=[0, 1, 2, 3, 8, 5, 6, 7]) == native.QH_ERR_ARG
  msg = lib.qh_last_error()
  assert b'table[4] = 8' in msg and b'dry' not in msg
  assert _perm(h, [0, 5, 2], table=[0, 1, 2, 3, 4, 2, 6, 2]) == native.QH_ERR_ARG
  msg = lib.qh_last_error()
  assert b'table[5] = 2' in msg and b'table[2]' in msg            # the first entry that repeats, and the one it repeats
  assert _perm(h, [3], table=[1, 1]) == native.QH_ERR_ARG
  assert b'table[1] = 1' in lib.qh_last_error()
  t = np.arange(1 << 12)
  t[4095] = 4094
  assert _perm(h, list(range(12)), table=t) == native.QH_ERR_ARG and b'table[4095] = 4094' in lib.qh_last_error()
  assert _perm(h, list(range(12)), table=np.arange(1 << 12)) == native.QH_ERR_ARG      # a bijection: only the dry handle is refused
  assert b'dry' in lib.qh_last_error()


def test_shard_bits_on_dry_handle(dry):
  lib = native.load()
  h = dry(10, nglob=12, shard=1)
  assert _perm(h, [3, 11]) == native.QH_ERR_NONLOCAL                # a register bit on the shard index
  assert b'exchange first' in lib.qh_last_error()
  assert _plan(h, [10, 4]) == native.QH_ERR_NONLOCAL
  t = native.QhPermTiles()
  b = (ctypes.c_int32 * 2)(3, 4)
  assert lib.qh_perm_plan(h, 2, b, (1 << 10) | (1 << 7), ctypes.byref(t)) == native.QH_OK
  assert t.ctl_met == 1 and t.ctl_in == 1 << 7 and t.ctl_out == 0   # shard index 1: bit 10 is 1 here, the control is dropped
  assert lib.qh_perm_plan(h, 2, b, (1 << 11) | (1 << 7), ctypes.byref(t)) == native.QH_OK
  assert t.ctl_met == 0                                             # bit 11 is 0 on this shard: the call would be a no-op
  assert _perm(h, [3, 4], ctl=1 << 11) == native.QH_ERR_ARG and b'dry' in lib.qh_last_error()


# ---- qh_perm_plan, executed with NumPy ---------------------------------------------------------------------------------------
LDS_BUDGET = 128 << 10


def _pdep(v, mask):
  """bit b of v (array or int) to the b-th lowest set position of mask"""
  out = np.zeros_like(np.asarray(v, dtype=np.int64))
  v = np.asarray(v, dtype=np.int64)
  b = 0
  for p in range(64):
    if (mask >> p) & 1:
      out |= ((v >> b) & 1) << p
      b += 1
  return out


def execute_plan(plan, phys, table, nloc):
  """What the kernels do with `plan` on the shard's amplitudes in PHYSICAL order: returns (new amplitudes, write counts).
  LDS path: load a tile, permute it in a scratch array, store it; tiles whose outside controls fail are left alone.
  Gather path: every amplitude written once from its source."""
  k = plan['k']
  table = np.asarray(table, dtype=np.int64)
  out = phys.copy()
  written = np.zeros(phys.size, dtype=np.int64)
  if not plan['ctl_met']:
    return out, written, 0
  if plan['path'] == native.QH_PERM_GATHER:
    i = np.arange(1 << nloc, dtype=np.int64)
    ctl = plan['ctl_in'] | plan['ctl_out']
    s = sum(((i >> plan['reg_pos'][j]) & 1) << j for j in range(k))
    t = table[s]
    dst = i.copy()
    for j in range(k):
      dst = (dst & ~(1 << plan['reg_pos'][j])) | (((t >> j) & 1) << plan['reg_pos'][j])
    dst = np.where((i & ctl) == ctl, dst, i)
    out = np.empty_like(phys)
    out[dst] = phys
    np.add.at(written, dst, 1)
    return out, written, 0
  m = plan['tile_bits']
  r = np.arange(1 << m, dtype=np.int64)
  off = _pdep(r, plan['tile_mask'])
  ranks = plan['reg_rank'][:k]
  s = sum(((r >> ranks[j]) & 1) << j for j in range(k))
  t = table[s]
  dest = r.copy()
  for j in range(k):
    dest = (dest & ~(1 << ranks[j])) | (((t >> j) & 1) << ranks[j])
  ctl_tile = 0
  for rank, p in enumerate(q for q in range(nloc) if (plan['tile_mask'] >> q) & 1):
    if (plan['ctl_in'] >> p) & 1:
      ctl_tile |= 1 << rank
  dest = np.where((r & ctl_tile) == ctl_tile, dest, r)
  rest = ((1 << nloc) - 1) & ~plan['tile_mask']
  skipped = 0
  for tile in range(plan['ntiles']):
    base = int(_pdep(tile, rest))
    if base & plan['ctl_out'] != plan['ctl_out']:
      skipped += 1
      continue
    lds = np.empty(1 << m, dtype=phys.dtype)
    lds[dest] = phys[base | off]
    out[base | off] = lds
    written[base | off] += 1
  return out, written, skipped


def _expected_tile(nloc, bw, reg_pos):
  line = min(3 if bw == 128 else 4, nloc)
  mask = (1 << line) - 1
  for p in reg_pos:
    mask |= 1 << p
  p = 0
  while bin(mask).count('1') < min(10, nloc):
    mask |= 1 << p
    p += 1
  return mask


def _bitmap(st, n):
  bm = (ctypes.c_int32 * 64)()
  native.check(st.lib.qh_get_bitmap(st.h, bm))
  return list(bm)[:n]


def _check_plan(st, nloc, nglob, shard, bits, ctl_mask, table, rng, paths=None):
  """plan on the handle's current bit map -> executed on this shard's amplitudes -> compared with the reference on the WHOLE
  logical state"""
  bw = st.bit_width
  plan = st.perm_plan(bits, ctl_mask)
  bm = _bitmap(st, nglob)
  k = len(bits)
  reg_pos = [bm[b] for b in bits]
  assert plan['k'] == k and plan['reg_pos'][:k] == reg_pos
  tile = _expected_tile(nloc, bw, reg_pos)
  assert plan['tile_mask'] == tile and plan['tile_bits'] == bin(tile).count('1')
  assert plan['reg_mask'] == sum(1 << p for p in reg_pos)
  assert plan['reg_rank'][:k] == [bin(tile & ((1 << p) - 1)).count('1') for p in reg_pos]
  ctl_phys = sum(1 << bm[b] for b in range(nglob) if (ctl_mask >> b) & 1)
  local = ctl_phys & ((1 << nloc) - 1)
  assert plan['ctl_in'] == local & tile and plan['ctl_out'] == local & ~tile
  assert plan['ctl_met'] == int((shard & (ctl_phys >> nloc)) == ctl_phys >> nloc)
  amp = 16 if bw == 128 else 8
  assert plan['lds_bytes'] == amp << plan['tile_bits']
  assert (plan['path'] == native.QH_PERM_LDS) == (plan['lds_bytes'] <= LDS_BUDGET)      # the LDS path exactly when the tile fits
  assert plan['ntiles'] == 1 << (nloc - plan['tile_bits'])
  if paths is not None:
    paths.add(plan['path'])
  # the whole logical state, this shard's part of it in physical order
  dtype = np.complex128 if bw == 128 else np.complex64
  psi = _rand_state(rng, nglob).astype(dtype)
  glob = np.arange(1 << nloc, dtype=np.int64) | (shard << nloc)
  logical = np.zeros_like(glob)
  for b in range(nglob):
    logical |= ((glob >> bm[b]) & 1) << b
  got, written, skipped = execute_plan(plan, psi[logical], table, nloc)
  want = perm_reference(psi, nglob, table, bits, ctl_mask)[logical]
  assert np.array_equal(got, want)
  if not plan['ctl_met']:
    assert not written.any()
  elif plan['path'] == native.QH_PERM_GATHER:
    assert np.all(written == 1)                                                          # every amplitude exactly once
  else:
    assert skipped == plan['tiles_skipped']
    run = (np.arange(1 << nloc) & plan['ctl_out']) == plan['ctl_out']
    assert np.array_equal(written, run.astype(np.int64))                                 # ... of the tiles that are not skipped
  return plan


def _shuffle_map(st, n, rng):
  for p in range(n - 1, 0, -1):
    st.remap_swap(p, int(rng.integers(0, p + 1)))


@pytest.mark.parametrize('bw', [128, 64])
@pytest.mark.parametrize('nloc', range(1, 9))
def test_plan_every_register_placement_up_to_8_bits(nloc, bw):
  """every non-empty set of positions as the register (in a random order), random controls inside and outside it, a
  random table, on a shuffled bit map"""
  rng = np.random.default_rng(100 * nloc + bw)
  st = device.DeviceState(nloc, bw, dry=True)
  try:
    for mask in range(1, 1 << nloc):
      if mask % 16 == 1:
        _shuffle_map(st, nloc, rng)
      bm = _bitmap(st, nloc)
      inv = {p: b for b, p in enumerate(bm)}
      reg = [inv[p] for p in range(nloc) if (mask >> p) & 1]
      rng.shuffle(reg)
      others = [b for b in range(nloc) if b not in reg]
      ctl = sum(1 << b for b in rng.permutation(others)[:int(rng.integers(0, 3))])
      _check_plan(st, nloc, nloc, 0, reg, ctl, rng.permutation(1 << len(reg)), rng)
  finally:
    st.close()


# (name, nloc, physical register positions in table-bit order, physical control positions)
_PLACED = [
    ('line_only', 14, [0, 1, 2], []),
    ('line_and_lane', 14, [1, 2, 3, 4, 5], [0]),
    ('lane', 14, [3, 4, 5, 6, 7, 8], [13, 1]),
    ('top', 14, [13, 12, 11, 10], [0, 5, 9]),                     # controls on a line bit, inside the padding, outside
    ('one_run', 18, list(range(5, 15)), [16]),
    ('one_run_reversed', 18, list(range(14, 4, -1)), [16, 17]),
    ('scattered', 18, [0, 3, 6, 9, 12, 15, 17], [1, 16]),
    ('k10_high', 18, list(range(8, 18)), [2]),                    # 13 tile bits: the largest complex128 tile
    ('k11_high', 18, list(range(7, 18)), []),                     # 14 (15) tile bits: fits complex64's line bits only ...
    ('k11_with_line', 18, [0, 1, 2, 3] + list(range(11, 18)), [5]),      # ... here: 11 + 0 extra bits at either width
    ('k14_all_line', 16, list(range(14)), [15]),                  # complex64: 14 bits = 128 KiB, complex128: gather
    ('k16', 16, list(range(15, -1, -1)), []),
    ('k13_scattered', 18, [0, 2, 3, 5, 6, 8, 9, 11, 12, 14, 15, 16, 17], [1]),
]


@pytest.mark.parametrize('bw', [128, 64])
@pytest.mark.parametrize('case', _PLACED, ids=[c[0] for c in _PLACED])
def test_plan_placed_by_physical_position(case, bw):
  _, nloc, regp, ctlp = case
  rng = np.random.default_rng(nloc + len(regp) + bw)
  st = device.DeviceState(nloc, bw, dry=True)
  try:
    _shuffle_map(st, nloc, rng)
    bm = _bitmap(st, nloc)
    inv = {p: b for b, p in enumerate(bm)}
    plan = _check_plan(st, nloc, nloc, 0, [inv[p] for p in regp], sum(1 << inv[p] for p in ctlp), rng.permutation(1 << len(regp)), rng)
    line = 3 if bw == 128 else 4
    extra = len([p for p in range(line) if p not in regp])
    assert plan['tile_bits'] == max(10, len(regp) + extra)
    assert (plan['path'] == native.QH_PERM_LDS) == (plan['tile_bits'] <= (13 if bw == 128 else 14))
  finally:
    st.close()


@pytest.mark.parametrize('nloc', [10, 12, 13, 14, 16, 18])
def test_plan_sampled_and_shard_bits(nloc):
  rng = np.random.default_rng(nloc)
  paths = set()
  for trial in range(12):
    bw = 128 if trial % 2 == 0 else 64
    nglob = nloc + (trial % 3)                                  # 0, 1 or 2 bits on the shard index
    shard = int(rng.integers(0, 1 << (nglob - nloc)))
    st = device.DeviceState(nloc, bw, dry=True)
    try:
      if nglob > nloc:
        st.set_shard(nglob, shard)
      _shuffle_map(st, nloc, rng)                               # local positions only: logical bits >= nloc stay on the shard index
      k = int(rng.integers(1, min(nloc, 16) + 1))
      local_bits = [int(b) for b in rng.permutation(nloc)]
      reg, rest = local_bits[:k], local_bits[k:] + list(range(nloc, nglob))
      ctl = sum(1 << b for b in rng.permutation(rest)[:int(rng.integers(0, 4))])
      _check_plan(st, nloc, nglob, shard, reg, ctl, rng.permutation(1 << k), rng, paths)
    finally:
      st.close()
  if nloc >= 16:
    assert paths == {native.QH_PERM_LDS, native.QH_PERM_GATHER}


def test_planner_stand_alone_under_sanitizers(tmp_path):
  """qcc_amd/csrc/perm_plan.h is plain C++: random bit maps, registers, controls and tables through a stand-alone program
  built with AddressSanitizer and UndefinedBehaviorSanitizer.  The sanitizer runtimes are linked statically, so the program
  runs in whatever environment this process has, unchanged (host code only; nothing is loaded into this process)."""
  cxx = shutil.which('g++') or shutil.which('clang++')
  assert cxx, 'no host C++ compiler'
  static = ['-static-libasan', '-static-libubsan'] if os.path.basename(cxx).startswith('g++') else ['-static-libsan']
  exe = str(tmp_path / 'perm_plan_check')
  subprocess.check_call([cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', *static,
                         os.path.join(ROOT, 'tools', 'perm_plan_check.cc'), '-o', exe])
  res = subprocess.run([exe, '40'], capture_output=True, text=True, timeout=120)
  assert res.returncode == 0, res.stdout + res.stderr
  assert 'ok' in res.stdout


# ---- qc routing and arithmetic on the NumPy stand-in ---------------------------------------------------------------------------
class PermOracle(fake_device.OracleDevice):
  """OracleDevice with apply_perm through the reference; records what it is asked."""
  calls_seen = []

  def apply_perm(self, table, bits, ctl_mask=0):
    t = np.array(table, dtype=np.int64)
    PermOracle.calls_seen.append((t, [int(b) for b in bits], int(ctl_mask), len(self.trace)))
    self.psi[:] = perm_reference(self.psi, self.nbits, t, list(bits), ctl_mask)


@pytest.fixture(params=[128, 64])
def cpu_backend(request):
  tensor.set_tensor_width(request.param)
  PermOracle.calls_seen = []
  backend.set_device_factory(PermOracle)
  yield request.param
  backend.set_device_factory(None)
  tensor.set_tensor_width(None)


def _prepared(n, seed):
  rng = np.random.default_rng(seed)
  q = circuit.qc('perm')
  q.reg(n, 0)
  for i in range(n):
    q.ry(i, float(rng.uniform(0.2, np.pi - 0.2)))
  q.cx(0, n - 1)
  return q


def _basis(n, qubit_values):
  q = circuit.qc('basis')
  q.reg(n, 0)
  for qb, v in qubit_values.items():
    if v:
      q.x(qb)
  return q


def _reg_value(n, qubits):
  """the value of the register `qubits` (first listed most significant) for every index"""
  idx = np.arange(1 << n)
  v = np.zeros_like(idx)
  for qb in qubits:
    v = (v << 1) | ((idx >> (n - 1 - qb)) & 1)
  return idx, v


def _moved(psi0, n, qubits, f, ctl=()):
  """psi0 with the register's value v replaced by f(v) (integer arithmetic on every index) where the controls are 1"""
  idx, v = _reg_value(n, qubits)
  w = f(v)
  dst = idx.copy()
  for j, qb in enumerate(reversed(qubits)):
    b = n - 1 - qb
    dst = (dst & ~(1 << b)) | (((w >> j) & 1) << b)
  on = np.ones_like(idx, dtype=bool)
  for c in ctl:
    on &= ((idx >> (n - 1 - c)) & 1) == 1
  dst = np.where(on, dst, idx)
  out = np.empty_like(psi0)
  out[dst] = psi0
  return out


def test_permutation_routes_logical_bits_and_table_order(cpu_backend):
  rng = np.random.default_rng(3)
  n = 7
  table = rng.permutation(8)
  q = _prepared(n, 1)
  psi0 = np.asarray(q.psi).copy()
  q.permutation(table, [5, 1, 3], ctl=[0, 6])
  t, bits, mask, _ = PermOracle.calls_seen[-1]
  assert bits == [n - 1 - 3, n - 1 - 1, n - 1 - 5] and mask == (1 << (n - 1 - 0)) | (1 << (n - 1 - 6))      # qubits[0] most significant
  assert np.array_equal(t, table)
  assert np.array_equal(np.asarray(q.psi), _moved(psi0, n, [5, 1, 3], lambda v: table[v], ctl=[0, 6]))
  # a callable is evaluated on the ints 0 .. 2^k - 1
  q.permutation(lambda s: s ^ 5, [2, 4, 6])
  assert np.array_equal(PermOracle.calls_seen[-1][0], np.arange(8) ^ 5)
  # basis states: |q5 q1 q3> = |1 0 1> = 5 -> table[5]
  qb = _basis(n, {5: 1, 3: 1, 2: 1})
  qb.permutation(table, [5, 1, 3])
  w = int(table[5])
  assert qb.prob(*[{5: w >> 2 & 1, 1: w >> 1 & 1, 3: w & 1, 2: 1}.get(i, 0) for i in range(n)]) == pytest.approx(1.0)


def test_arithmetic_matches_integer_arithmetic(cpu_backend):
  n, reg = 8, [6, 1, 4, 2, 7]                                    # 5 qubits, scattered, unordered
  size = 32
  q = _prepared(n, 2)
  for name, args, f in [
      ('add_const', (11,), lambda v: (v + 11) % size),
      ('add_const', (-3,), lambda v: (v - 3) % size),
      ('add_const', (size * 4 + 1,), lambda v: (v + 1) % size),
      ('modadd', (9, 21), lambda v: np.where(v < 21, (v + 9) % 21, v)),
      ('modadd', (-4, 32), lambda v: (v - 4) % 32),
      ('modmul', (5, 21), lambda v: np.where(v < 21, (v * 5) % 21, v)),
      ('modmul', (-2, 21), lambda v: np.where(v < 21, (v * 19) % 21, v)),
      ('modmul', (7, 32), lambda v: (v * 7) % 32),
  ]:
    for ctl in ((), (3,), (0, 5)):
      psi0 = np.asarray(q.psi).copy()
      getattr(q, name)(*args, reg, ctl)
      assert np.array_equal(np.asarray(q.psi), _moved(psi0, n, reg, f, ctl)), (name, args, ctl)
  # basis states through every method: 13 + 11 = 24; (13 + 9) mod 21 = 1; 5 * 13 mod 21 = 2; 25 >= 21 is left alone
  def run(start, call):
    qb = _basis(n, {qb_: (start >> (4 - j)) & 1 for j, qb_ in enumerate(reg)})
    call(qb)
    idx, p = qb.maxprob()
    assert p == pytest.approx(1.0)
    return int(''.join(str(idx[qb_]) for qb_ in reg), 2)
  assert run(13, lambda c: c.add_const(11, reg)) == 24
  assert run(13, lambda c: c.modadd(9, 21, reg)) == 1
  assert run(13, lambda c: c.modmul(5, 21, reg)) == 2
  assert run(25, lambda c: c.modmul(5, 21, reg)) == 25
  assert run(25, lambda c: c.modadd(9, 21, reg)) == 25


def test_add_of_two_registers(cpu_backend):
  n, src, dst = 9, [7, 0, 3], [5, 2, 8, 1]
  q = _prepared(n, 4)
  psi0 = np.asarray(q.psi).copy()
  q.add(src, dst)
  t, bits, mask, _ = PermOracle.calls_seen[-1]
  assert mask == 0 and bits == [n - 1 - qb for qb in reversed(src + dst)]
  # |a>|b> -> |a>|(a + b) mod 16> read off every index
  idx, a = _reg_value(n, src)
  _, b = _reg_value(n, dst)
  s = (a + b) % 16
  dest = idx.copy()
  for j, qb in enumerate(reversed(dst)):
    dest = (dest & ~(1 << (n - 1 - qb))) | (((s >> j) & 1) << (n - 1 - qb))
  want = np.empty_like(psi0)
  want[dest] = psi0
  assert np.array_equal(np.asarray(q.psi), want)
  qb = _basis(n, {7: 1, 3: 1, 5: 1, 2: 1, 1: 1})                  # a = 5, b = 13: 18 mod 16 = 2
  qb.add(src, dst)
  idx_bits, p = qb.maxprob()
  assert p == pytest.approx(1.0)
  assert [idx_bits[x] for x in src] == [1, 0, 1] and [idx_bits[x] for x in dst] == [0, 0, 1, 0]


def test_modmul_then_its_inverse_is_the_identity(cpu_backend):
  n, reg = 8, [1, 6, 3, 0, 5, 2]
  q = _prepared(n, 5)
  psi0 = np.asarray(q.psi).copy()
  for a, N in ((7, 15), (10, 63), (27, 64), (4, 61)):
    q.modmul(a, N, reg, ctl=[7])
    assert not np.array_equal(np.asarray(q.psi), psi0)
    q.modmul(pow(a, -1, N), N, reg, ctl=[7])
    assert np.array_equal(np.asarray(q.psi), psi0)                  # amplitudes are moved: exact


def test_queued_gates_are_drained_first(cpu_backend):
  q = circuit.qc('order')
  q.reg(4, 0)
  q.x(0)                                              # queued on the host side
  q.permutation([0, 1, 3, 2], [0, 1])                 # CNOT(0 -> 1) as a table
  assert PermOracle.calls_seen[-1][3] == 1            # the X had reached the device when the table arrived
  assert q.prob(1, 1, 0, 0) == pytest.approx(1.0)


def test_value_errors(cpu_backend):
  q = _prepared(6, 9)
  q.x(0)                                              # stays queued: a refused call drains nothing
  pending = len(q._q_ops)                             # pylint: disable=protected-access
  ident = list(range(4))
  with pytest.raises(ValueError):
    q.permutation([0, 1, 1, 3], [1, 2])               # a value hit twice
  with pytest.raises(ValueError):
    q.permutation([0, 1, 2, 4], [1, 2])               # out of range
  with pytest.raises(ValueError):
    q.permutation([0, -1, 2, 3], [1, 2])
  with pytest.raises(ValueError):
    q.permutation(lambda s: s // 2, [1, 2])           # a callable that is no bijection
  with pytest.raises(ValueError):
    q.permutation(ident, [1, 2, 3])                   # 4 entries for 3 qubits
  with pytest.raises(ValueError):
    q.permutation([], [])
  if pending:
    assert len(q._q_ops) == pending                   # pylint: disable=protected-access
  with pytest.raises(ValueError):
    q.permutation(ident, [1, 1])                      # a qubit twice
  with pytest.raises(ValueError):
    q.permutation(ident, [1, 6])                      # out of range
  with pytest.raises(ValueError):
    q.permutation(ident, [1, 2], ctl=[2])             # a control inside the register
  with pytest.raises(ValueError):
    q.permutation(ident, [1, 2], ctl=[7])
  with pytest.raises(ValueError):
    q.modmul(6, 15, [0, 1, 2, 3])                     # gcd(6, 15) = 3
  with pytest.raises(ValueError):
    q.modmul(3, 17, [0, 1, 2, 3])                     # N above 2^k
  with pytest.raises(ValueError):
    q.modmul(3, 0, [0, 1, 2, 3])
  with pytest.raises(ValueError):
    q.modadd(3, 17, [0, 1, 2, 3])
  with pytest.raises(ValueError):
    q.add_const(1, [0, 0])
  with pytest.raises(ValueError):
    q.add([0, 1], [1, 2])                             # the registers overlap
  with pytest.raises(ValueError):
    circuit.qc('wide').add(list(range(9)), list(range(9, 17)))      # 17 qubits in one table
  assert PermOracle.calls_seen == []


def test_devices_without_the_method_raise(cpu_backend):
  backend.set_device_factory(fake_device.OracleDevice)
  q = _prepared(4, 1)
  for call in (lambda: q.permutation([1, 0], [0]), lambda: q.add_const(1, [0, 1]), lambda: q.modadd(1, 3, [0, 1]),
               lambda: q.modmul(2, 3, [0, 1]), lambda: q.add([0], [1, 2])):
    with pytest.raises(NotImplementedError):
      call()


def order_finding_model(a, N, t, n):
  """P(m) of the exponent register after sum_x |x>|a^x mod N> / sqrt(2^t) and the inverse Fourier transform over x"""
  T = 1 << t
  amp = np.zeros((T, 1 << n), dtype=np.complex128)
  for x in range(T):
    amp[x, pow(a, x, N)] = 1 / math.sqrt(T)
  out = np.fft.fft(amp, axis=0) / math.sqrt(T)        # sum_x exp(-2 pi i x m / T) ...
  return np.sum(np.abs(out) ** 2, axis=1)


def order_finding_circuit(a, N, t, n):
  """exponent register on qubits 0 .. t-1 (qubit 0 most significant), work register on t .. t+n-1, initialised to 1: one
  controlled modmul per exponent bit, then the inverse Fourier transform without swaps -- its result sits bit-reversed, so
  the exponent register is read with qubit t-1 as the most significant bit"""
  q = circuit.qc('order')
  q.reg(t + n, 0)
  work = list(range(t, t + n))
  q.x(t + n - 1)
  for i in range(t):
    q.h(i)
  for i in range(t):
    q.modmul(pow(a, 1 << (t - 1 - i), N), N, work, ctl=[i])
  for i in range(t):
    q.h(i)
    for j in range(i + 1, t):
      q.cu1(j, i, -2 * np.pi / (1 << (j - i + 1)))
  return q, list(reversed(range(t)))


def test_order_finding_7_mod_15(cpu_backend):
  t, n = 8, 4
  q, read = order_finding_circuit(7, 15, t, n)
  p = q.probabilities(read)
  want = order_finding_model(7, 15, t, n)
  assert np.max(np.abs(p - want)) < (1e-12 if cpu_backend == 128 else 1e-5)
  peaks = np.flatnonzero(p > 0.2)
  assert list(peaks) == [0, 64, 128, 192]             # multiples of 2^t / r, r = 4 the order of 7 mod 15
  assert np.allclose(p[peaks], 0.25, atol=1e-5)
  assert len(PermOracle.calls_seen) == t
