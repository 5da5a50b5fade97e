"""CPU tests of the rank-one register updates: the NumPy reference of qh_apply_rank1 (against explicit Kronecker products,
against H-layer / 2|0><0| - I / H-layer through the CPU oracle, and against the reference project's dense reflections in
tests/golden/g16_reflections.npz), the two C-ABI symbols and their argument checks on planner-only handles, qh_rank1_plan
executed with NumPy -- the TILE path tile by tile through reg_rank, the pass-1 cut of the TWO_PASS path unit by unit -- against
the reference (every register placement up to 8 bits, sampled up to 18, both widths, shard bits), the planner stand-alone under
sanitizers, and qc.rank_one / reflect / diffusion / project_onto over a NumPy stand-in device with Grover search and amplitude
amplification against sin((2t + 1) theta)."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from qcc_amd import device, gates, native
from qcc_amd.lib import backend, circuit, tensor
from tests import fake_device, oracle_lib, rank1_util
from tests.rank1_util import Rank1Oracle, rand_state, rand_vector, rank1_parts, rank1_reference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_ip = ctypes.POINTER(ctypes.c_int32)
_dp = ctypes.POINTER(ctypes.c_double)
LDS_BUDGET = 128 << 10


# ---- the reference itself ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [1, 2, 4, 6])
def test_reference_matches_kronecker_products(n):
  """the operator as a dense matrix: the register permuted to the low bits, (I (x) (a I + b |u><v|)), permuted back, with
  projectors on the control bits"""
  rng = np.random.default_rng(n)
  for _ in range(6):
    k = int(rng.integers(1, n + 1))
    perm = [int(x) for x in rng.permutation(n)]
    bits, rest = perm[:k], perm[k:]
    ctl = sum(1 << x for x in rest[:int(rng.integers(0, min(3, len(rest) + 1)))])
    u, v = rand_vector(rng, k), rand_vector(rng, k)
    a, b = complex(*rng.normal(size=2)), complex(*rng.normal(size=2))
    op = a * np.eye(1 << k) + b * np.outer(u, np.conj(v))
    full = np.kron(np.eye(1 << (n - k)), op)             # register on bits 0..k-1 (bit j of the table index = bit j), rest above
    order = bits + rest                                   # bit j of `full`'s index is logical bit order[j]
    idx = np.arange(1 << n)
    moved = np.zeros_like(idx)
    for j, x in enumerate(order):
      moved |= ((idx >> x) & 1) << j
    mat = full[np.ix_(moved, moved)]                      # mat[i, i'] = full[moved(i), moved(i')]
    met = (idx & ctl) == ctl
    mat = np.where(met[:, None], mat, np.eye(1 << n))
    psi = rand_state(rng, n)
    assert np.allclose(rank1_reference(psi, n, bits, u, v, a, b, ctl), mat @ psi, atol=1e-13)
  psi = rand_state(rng, n)
  assert np.allclose(rank1_reference(psi, n, [0], None, None, -1.0, 2.0), rank1_reference(psi, n, [0], None, np.full(2, 0.5 ** 0.5), -1.0, 2.0))


@pytest.mark.parametrize('n', [3, 7])
def test_uniform_reflection_is_h_layer_zero_reflection_h_layer(n):
  rng = np.random.default_rng(n)
  o = oracle_lib.load()
  h_gate = np.asarray(gates.hadamard(), np.complex128)
  for qubits in ([0, n - 1], list(range(n)), [int(x) for x in rng.permutation(n)[:n - 1]]):
    psi = rand_state(rng, n)
    want = psi.copy()
    for q in qubits:
      o.apply1(want, h_gate, n, q)
    bits = [n - 1 - q for q in qubits]
    zero = (np.arange(1 << n) & sum(1 << x for x in bits)) == 0
    want = np.where(zero, want, -want)                    # 2|0><0| - I on the register
    for q in qubits:
      o.apply1(want, h_gate, n, q)
    assert np.allclose(rank1_reference(psi, n, bits, None, None, -1.0, 2.0), want, atol=1e-13)


def test_reference_matches_the_reference_projects_reflections():
  g = np.load(rank1_util.GOLDEN)
  assert sorted(g.files) == sorted([f'a{n}_{x}' for n in (3, 5, 8) for x in ('in', 'out')] + [f'b{n}_{x}' for n in (3, 6) for x in ('phi', 'in', 'out')])
  assert max(g[f].size for f in g.files) == 256
  for n in (3, 5, 8):
    for psi, want in zip(g[f'a{n}_in'], g[f'a{n}_out']):
      assert np.max(np.abs(rank1_reference(psi, n, list(range(n)), None, None, -1.0, 2.0) - want)) < 1e-13
  for n in (3, 6):
    phi = g[f'b{n}_phi']
    assert abs(np.linalg.norm(phi) - 1) < 1e-12
    for psi, want in zip(g[f'b{n}_in'], g[f'b{n}_out']):
      assert np.max(np.abs(rank1_reference(psi, n, list(range(n)), None, phi, -1.0, 2.0) - want)) < 1e-13


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


_ONE = np.array([1.0, 0.0])


def _apply(h, bits, ctl=0, k=None, v='ones', u=None, a=_ONE, b=_ONE):
  lib = native.load()
  k = len(bits) if k is None else k
  bb = (ctypes.c_int32 * max(1, len(bits)))(*bits)
  if isinstance(v, str):
    v = np.ones(1 << min(max(k, 0), 16), dtype=np.complex128)
  p = lambda t: None if t is None else np.ascontiguousarray(t).ctypes.data_as(_dp)
  return lib.qh_apply_rank1(h, k, bb, ctl, p(u), p(v), p(a), p(b), None)


def _plan(h, bits, ctl=0, k=None, uniform=0):
  lib = native.load()
  bb = (ctypes.c_int32 * max(1, len(bits)))(*bits)
  return lib.qh_rank1_plan(h, len(bits) if k is None else k, bb, ctl, uniform, ctypes.byref(native.QhRank1Info()))


def test_symbols_exported_and_bound():
  lib = native.load()
  for name in ('qh_apply_rank1', 'qh_rank1_plan'):
    assert name in native.SIGNATURES
    assert getattr(lib, name).argtypes == native.SIGNATURES[name][1]
  assert lib.qh_version() >= 120
  assert native.QH_RANK1_MAX_BITS == 16 and (native.QH_RANK1_TILE, native.QH_RANK1_TWO_PASS) == (0, 1)


def test_argument_errors_on_dry_handle(dry):
  lib = native.load()
  h = dry(20)
  b1 = (ctypes.c_int32 * 1)(3)
  two = np.ones(2, dtype=np.complex128)
  pd = lambda t: t.ctypes.data_as(_dp)
  assert lib.qh_apply_rank1(None, 1, b1, 0, None, pd(two), pd(_ONE), pd(_ONE), None) == native.QH_ERR_ARG
  assert lib.qh_apply_rank1(h, 1, None, 0, None, pd(two), pd(_ONE), pd(_ONE), None) == native.QH_ERR_ARG
  assert lib.qh_apply_rank1(h, 1, b1, 0, None, pd(two), None, pd(_ONE), None) == native.QH_ERR_ARG
  assert lib.qh_apply_rank1(h, 1, b1, 0, None, pd(two), pd(_ONE), None, None) == native.QH_ERR_ARG
  assert lib.qh_apply_rank1(h, 1, b1, 0, pd(two), None, pd(_ONE), pd(_ONE), None) == native.QH_ERR_ARG and b'u without v' in lib.qh_last_error()
  assert lib.qh_rank1_plan(None, 1, b1, 0, 0, ctypes.byref(native.QhRank1Info())) == native.QH_ERR_ARG
  assert lib.qh_rank1_plan(h, 1, None, 0, 0, ctypes.byref(native.QhRank1Info())) == native.QH_ERR_ARG
  assert lib.qh_rank1_plan(h, 1, b1, 0, 0, None) == native.QH_ERR_ARG
  for call in (_apply, _plan):
    assert call(h, [], k=0) == native.QH_ERR_ARG
    assert call(h, [], k=-1) == native.QH_ERR_ARG
    assert call(h, list(range(17)), k=17) == native.QH_ERR_ARG          # the table form stops at 16 bits
    assert call(h, [0, 20]) == native.QH_ERR_BAD_QUBIT
    assert call(h, [-1, 3]) == native.QH_ERR_BAD_QUBIT
    assert call(h, [0, 3], ctl=1 << 20) == native.QH_ERR_BAD_QUBIT
    assert call(h, [3, 3]) == native.QH_ERR_SAME_QUBIT
    assert call(h, [5, 5, 20]) == native.QH_ERR_BAD_QUBIT               # both faults: every bit's range is checked first
    assert call(h, [3, 4], ctl=1 << 4) == native.QH_ERR_SAME_QUBIT
  # the uniform form goes up to the local bits
  assert _plan(h, list(range(20)), uniform=1) == native.QH_OK and _plan(h, list(range(17)), uniform=1) == native.QH_OK
  hs = dry(10, nglob=12)
  assert _plan(hs, list(range(11)), uniform=1) == native.QH_ERR_ARG and _apply(hs, list(range(11)), v=None) == native.QH_ERR_ARG
  # non-finite coefficients and entries: the first offender is named, before the dry handle is refused
  bad = np.ones(8, dtype=np.complex128)
  bad[6] = complex(np.nan, 0)
  assert _apply(h, [1, 2, 3], v=bad) == native.QH_ERR_ARG and b'v[6]' in lib.qh_last_error()
  bad[2] = complex(0, np.inf)
  assert _apply(h, [1, 2, 3], u=bad, v=np.ones(8, dtype=np.complex128)) == native.QH_ERR_ARG
  assert b'u[2]' in lib.qh_last_error() and b'imaginary' in lib.qh_last_error()
  assert _apply(h, [1], a=np.array([0.0, np.nan])) == native.QH_ERR_ARG and b'a[1]' in lib.qh_last_error()
  assert _apply(h, [1], b=np.array([np.inf, 0.0])) == native.QH_ERR_ARG and b'b[0]' in lib.qh_last_error()
  # valid calls: the plan is host arithmetic, the call itself has no state to work on
  assert _plan(h, [2, 5], ctl=1 << 7) == native.QH_OK
  for rc in (_apply(h, [2, 5]), _apply(h, [7], v=None), _apply(h, list(range(4, 20)), ctl=0b1010), _apply(h, list(range(20)), v=None)):
    assert rc == native.QH_ERR_ARG
    assert b'dry' in lib.qh_last_error()


def test_shard_bits_on_dry_handle(dry):
  lib = native.load()
  h = dry(10, nglob=12, shard=1)
  assert _apply(h, [3, 11]) == native.QH_ERR_NONLOCAL and b'exchange first' in lib.qh_last_error()
  assert _plan(h, [10, 4]) == native.QH_ERR_NONLOCAL
  t = native.QhRank1Info()
  b = (ctypes.c_int32 * 2)(3, 4)
  assert lib.qh_rank1_plan(h, 2, b, (1 << 10) | (1 << 7), 0, ctypes.byref(t)) == native.QH_OK
  assert t.tile.ctl_met == 1 and t.tile.ctl_in == 1 << 7 and t.tile.ctl_out == 0   # bit 10 is 1 on shard 1: the control is dropped
  assert lib.qh_rank1_plan(h, 2, b, (1 << 11) | (1 << 7), 0, ctypes.byref(t)) == native.QH_OK
  assert t.tile.ctl_met == 0                                                       # bit 11 is 0 here: the call would be a no-op


# ---- qh_rank1_plan, executed with NumPy ---------------------------------------------------------------------------------------
def _pdep(v, mask):
  """bit b of v (array or int) to the b-th lowest set position of mask"""
  v = np.asarray(v, dtype=np.int64)
  out = np.zeros_like(v)
  b = 0
  for p in range(64):
    if (mask >> p) & 1:
      out |= ((v >> b) & 1) << p
      b += 1
  return out


def _pext(v, mask):
  v = np.asarray(v, dtype=np.int64)
  out = np.zeros_like(v)
  b = 0
  for p in range(64):
    if (mask >> p) & 1:
      out |= ((v >> p) & 1) << b
      b += 1
  return out


def execute_tile_plan(plan, phys, u, v, a, b, nloc):
  """The TILE path on the shard's amplitudes in PHYSICAL order: every tile whose outside controls are met is loaded, the
  register's value read through reg_rank, the fibre sums formed inside the tile, the tile stored.  Returns (new, written)."""
  t = plan['tile']
  k, m = t['k'], t['tile_bits']
  out, written = phys.astype(np.complex128), np.zeros(phys.size, dtype=np.int64)
  r = np.arange(1 << m, dtype=np.int64)
  off = _pdep(r, t['tile_mask'])
  ranks = t['reg_rank'][:k]
  s = sum(((r >> ranks[j]) & 1) << j for j in range(k))
  reg_tile = sum(1 << x for x in ranks)
  ctl_tile = 0
  for rank, p in enumerate(q for q in range(nloc) if (t['tile_mask'] >> q) & 1):
    if (t['ctl_in'] >> p) & 1:
      ctl_tile |= 1 << rank
  on = (r & ctl_tile) == ctl_tile
  fibre = r & ~reg_tile
  rest = ((1 << nloc) - 1) & ~t['tile_mask']
  for tile in range(t['ntiles']):
    base = int(_pdep(tile, rest))
    if base & t['ctl_out'] != t['ctl_out']:
      continue
    x = phys[base | off].astype(np.complex128)
    prod = np.conj(v[s]) * x
    mr = (np.bincount(fibre, weights=prod.real, minlength=1 << m) + 1j * np.bincount(fibre, weights=prod.imag, minlength=1 << m))[fibre]
    out[base | off] = np.where(on, a * x + b * u[s] * mr, x)
    written[(base | off)[on]] += 1
  return out, written


def execute_pass1(plan, phys, v_of_index, nloc):
  """Pass 1 of the TWO_PASS path as the plan cuts it: unit (group, segment) walks `walk` chunks and leaves fibres_per_chunk
  partial sums; the segments of a fibre are added in order.  v_of_index: conj(v[s(i)]) for every physical index i.  Returns m
  by fibre (the physical index with the register bits taken out) and how often every scratch entry was written."""
  t = plan['tile']
  cb, split, walk, fpc, nfib = plan['chunk_bits'], plan['split'], plan['walk'], plan['fibres_per_chunk'], plan['nfibres']
  low = (1 << cb) - 1
  reg_low, abv = t['reg_mask'] & low, t['reg_mask'] >> cb
  grp = (((1 << nloc) - 1) >> cb) & ~abv
  part = np.zeros((split, nfib), dtype=np.complex128)
  filled = np.zeros((split, nfib), dtype=np.int64)
  c = np.arange(1 << cb, dtype=np.int64)
  slot = _pext(c, low & ~reg_low)                          # the chunk-local index with the register bits taken out
  prod = v_of_index * phys.astype(np.complex128)
  for unit in range(plan['groups'] * split):
    g, seg = divmod(unit, split)
    acc = np.zeros(1 << cb, dtype=np.complex128)
    for wi in range(seg * walk, (seg + 1) * walk):
      chunk = int(_pdep(g, grp)) | int(_pdep(wi, abv))
      acc += prod[(chunk << cb) | c]
    sums = np.bincount(slot, weights=acc.real, minlength=fpc) + 1j * np.bincount(slot, weights=acc.imag, minlength=fpc)
    part[seg, g * fpc:(g + 1) * fpc] = sums
    filled[seg, g * fpc:(g + 1) * fpc] += 1
  return part.sum(axis=0), filled


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


def _check_plan(st, nloc, nglob, shard, bits, ctl_mask, uniform, rng, paths=None):
  """plan on the handle's current bit map -> invariants -> executed on this shard's amplitudes -> compared with the reference
  on the WHOLE logical state"""
  bw = st.bit_width
  plan = st.rank1_plan(bits, ctl_mask, uniform=uniform)
  t = plan['tile']
  bm = _bitmap(st, nglob)
  k = len(bits)
  reg_pos = [bm[x] for x in bits]
  tile = _expected_tile(nloc, bw, reg_pos)
  assert t['k'] == k and t['tile_mask'] == tile and t['tile_bits'] == bin(tile).count('1')       # the tile holds the register
  assert t['reg_mask'] == sum(1 << p for p in reg_pos) and t['reg_mask'] & ~tile == 0
  if k <= 16:
    assert t['reg_pos'][:k] == reg_pos and t['reg_rank'][:k] == [bin(tile & ((1 << p) - 1)).count('1') for p in reg_pos]
  ctl_phys = sum(1 << bm[x] for x in range(nglob) if (ctl_mask >> x) & 1)
  local = ctl_phys & ((1 << nloc) - 1)
  assert t['ctl_in'] == local & tile and t['ctl_out'] == local & ~tile
  assert t['ctl_met'] == int((shard & (ctl_phys >> nloc)) == ctl_phys >> nloc)
  amp = 16 if bw == 128 else 8
  assert t['lds_bytes'] == amp << t['tile_bits'] and t['ntiles'] == 1 << (nloc - t['tile_bits'])
  # the path follows from lds_bytes (and, for tables, from the 2^10 entries that fit behind the tile)
  assert (plan['path'] == native.QH_RANK1_TILE) == (t['lds_bytes'] <= LDS_BUDGET and (uniform or k <= 10))
  assert plan['nfibres'] == 1 << (nloc - k) and plan['uniform'] == int(uniform)
  state_bytes = amp << nloc
  if plan['path'] == native.QH_RANK1_TILE:
    assert plan['kernels'] == 1 and plan['scratch_bytes'] == 0
    assert plan['bytes_swept'] == 2 * state_bytes >> bin(t['ctl_out']).count('1')
  else:
    cb = min(nloc, 11 if bw == 128 else 12)
    assert plan['chunk_bits'] == cb and plan['reg_in_chunk'] == bin(t['reg_mask'] & ((1 << cb) - 1)).count('1')
    assert plan['reg_in_chunk'] + plan['reg_above'] == k
    assert plan['groups'] << (cb + plan['reg_above']) == 1 << nloc and plan['fibres_per_chunk'] << plan['reg_in_chunk'] == 1 << cb
    assert plan['walk'] * plan['split'] == 1 << plan['reg_above'] and 1 <= plan['split'] <= 256
    assert plan['kernels'] == (3 if plan['split'] > 1 else 2) and plan['bytes_swept'] == 3 * state_bytes
    assert plan['scratch_bytes'] == 16 * plan['nfibres'] * (1 + plan['split'] if plan['split'] > 1 else 1)
  if paths is not None:
    paths.add(plan['path'])
  # the whole logical state, this shard's part of it in physical order
  dtype = np.complex128 if bw == 128 else np.complex64
  psi = rand_state(rng, nglob).astype(dtype)
  glob = np.arange(1 << nloc, dtype=np.int64) | (shard << nloc)
  logical = np.zeros_like(glob)
  for x in range(nglob):
    logical |= ((glob >> bm[x]) & 1) << x
  if uniform:
    u = v = np.full(1 << k, 2.0 ** (-k / 2.0), dtype=np.complex128)
  else:
    u, v = rand_vector(rng, k), rand_vector(rng, k)
  a, b = complex(*rng.normal(size=2)), complex(*rng.normal(size=2))
  want, m, _ = rank1_parts(psi, nglob, bits, u, v, a, b, ctl_mask)
  want, m = want[logical], m[logical]
  phys = psi[logical]
  if not t['ctl_met']:
    assert np.array_equal(want, phys.astype(np.complex128))
    return plan
  if plan['path'] == native.QH_RANK1_TILE:
    got, written = execute_tile_plan(plan, phys, u, v, a, b, nloc)
    assert np.allclose(got, want, atol=1e-12)
    idx = np.arange(1 << nloc)
    assert np.array_equal(written, ((idx & local) == local).astype(np.int64))       # the met amplitudes, once each
  else:
    idx = np.arange(1 << nloc, dtype=np.int64)
    s = sum(((idx >> reg_pos[j]) & 1) << j for j in range(k))
    got_m, filled = execute_pass1(plan, phys, np.conj(v[s]), nloc)
    assert np.all(filled == 1)
    fibre = _pext(idx, ((1 << nloc) - 1) & ~t['reg_mask'])
    assert np.allclose(got_m[fibre], m, atol=1e-12)
  return plan


def _shuffle_map(st, n, rng):
  for p in range(n - 1, 0, -1):
    st.remap_swap(p, int(rng.integers(0, p + 1)))


@pytest.mark.parametrize('bw', [128, 64])
@pytest.mark.parametrize('nloc', range(1, 9))
def test_plan_every_register_placement_up_to_8_bits(nloc, bw):
  rng = np.random.default_rng(100 * nloc + bw)
  st = device.DeviceState(nloc, bw, dry=True)
  try:
    for mask in range(1, 1 << nloc):
      if mask % 16 == 1:
        _shuffle_map(st, nloc, rng)
      bm = _bitmap(st, nloc)
      inv = {p: x for x, p in enumerate(bm)}
      reg = [inv[p] for p in range(nloc) if (mask >> p) & 1]
      rng.shuffle(reg)
      others = [x for x in range(nloc) if x not in reg]
      ctl = sum(1 << x for x in rng.permutation(others)[:int(rng.integers(0, 3))])
      plan = _check_plan(st, nloc, nloc, 0, reg, ctl, bool(mask & 1), rng)
      assert plan['path'] == native.QH_RANK1_TILE
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
    uniform = trial % 4 >= 2
    st = device.DeviceState(nloc, bw, dry=True)
    try:
      if nglob > nloc:
        st.set_shard(nglob, shard)
      _shuffle_map(st, nloc, rng)                               # local positions only
      k = int(rng.integers(1, (nloc if uniform else min(nloc, 16)) + 1))
      if trial >= 8:
        k = min(nloc, 16) if not uniform else nloc - (trial % 2)      # wide registers: the second path
      local_bits = [int(x) for x in rng.permutation(nloc)]
      reg, rest = local_bits[:k], local_bits[k:] + list(range(nloc, nglob))
      ctl = sum(1 << x for x in rng.permutation(rest)[:int(rng.integers(0, 4))]) if rest else 0
      _check_plan(st, nloc, nglob, shard, reg, ctl, uniform, rng, paths)
    finally:
      st.close()
  if nloc >= 16:
    assert paths == {native.QH_RANK1_TILE, native.QH_RANK1_TWO_PASS}


def test_planner_stand_alone_under_sanitizers(tmp_path):
  """qcc_amd/csrc/rank1_plan.h is plain C++: random registers, controls and tables through a stand-alone program built with
  AddressSanitizer and UndefinedBehaviorSanitizer.  The sanitizer runtimes are linked statically, so the program runs in
  whatever environment this process has, unchanged (host code only; nothing is loaded into this process)."""
  cxx = shutil.which('g++') or shutil.which('clang++')
  assert cxx, 'no host C++ compiler'
  static = ['-static-libasan', '-static-libubsan'] if os.path.basename(cxx).startswith('g++') else ['-static-libsan']
  exe = str(tmp_path / 'rank1_plan_check')
  subprocess.check_call([cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', *static,
                         os.path.join(ROOT, 'tools', 'rank1_plan_check.cc'), '-o', exe])
  res = subprocess.run([exe, '24'], capture_output=True, text=True, timeout=120)
  assert res.returncode == 0, res.stdout + res.stderr
  assert 'ok' in res.stdout


# ---- qc routing on the NumPy stand-in ---------------------------------------------------------------------------------------------
@pytest.fixture(params=[128, 64])
def cpu_backend(request):
  tensor.set_tensor_width(request.param)
  Rank1Oracle.calls_seen = []
  backend.set_device_factory(Rank1Oracle)
  yield request.param
  backend.set_device_factory(None)
  tensor.set_tensor_width(None)


def _prepared(n, seed):
  rng = np.random.default_rng(seed)
  q = circuit.qc('rank1')
  q.reg(n, 0)
  for i in range(n):
    q.ry(i, float(rng.uniform(0.2, np.pi - 0.2)))
  q.cx(0, n - 1)
  return q


def test_rank_one_routes_logical_bits_and_table_order(cpu_backend):
  rng = np.random.default_rng(3)
  n = 7
  q = _prepared(n, 1)
  q.x(2)                                                 # queued on the host side: must reach the device first
  psi0 = np.asarray(q.psi).astype(np.complex128)
  u, v = rand_vector(rng, 3), rand_vector(rng, 3)
  q.rank_one([5, 1, 3], u, v, a=0.5, b=complex(0, 2), ctl=[0, 6])
  seen = Rank1Oracle.calls_seen[-1]
  assert seen['bits'] == [n - 1 - 3, n - 1 - 1, n - 1 - 5] and seen['ctl_mask'] == (1 << (n - 1)) | 1      # qubits[0] most significant
  assert np.array_equal(seen['u'], u) and np.array_equal(seen['v'], v) and (seen['a'], seen['b']) == (0.5, 2j)
  want = rank1_reference(psi0, n, seen['bits'], u, v, 0.5, 2j, seen['ctl_mask'])
  assert np.allclose(np.asarray(q.psi), want, atol=1e-6 if cpu_backend == 64 else 1e-13)
  q.rank_one([4], u[:2])                                 # v = None: |u><u|, a = 0, b = 1
  seen = Rank1Oracle.calls_seen[-1]
  assert seen['u'] is None and np.array_equal(seen['v'], u[:2]) and (seen['a'], seen['b']) == (0, 1)
  q.reflect([2, 6], [3.0, 0, 0, 4.0j])                   # normalised on the host
  seen = Rank1Oracle.calls_seen[-1]
  assert np.allclose(seen['v'], [0.6, 0, 0, 0.8j]) and (seen['a'], seen['b']) == (-1, 2)
  q.diffusion(list(range(n)))                            # the uniform form: no table, any number of qubits
  seen = Rank1Oracle.calls_seen[-1]
  assert seen['u'] is None and seen['v'] is None and seen['bits'] == list(range(n))


def test_value_errors_and_devices_without_the_method(cpu_backend):
  q = _prepared(6, 9)
  four = np.ones(4)
  for call in (lambda: q.rank_one([1, 2], np.ones(8)), lambda: q.rank_one([1, 2], four, np.ones(2)), lambda: q.rank_one([], [1.0]),
               lambda: q.rank_one([1, 1], four), lambda: q.rank_one([1, 6], four), lambda: q.rank_one([1, 2], four, ctl=[2]),
               lambda: q.rank_one([1, 2], [1, 2, np.nan, 4]), lambda: q.reflect([1, 2], np.zeros(4)), lambda: q.reflect([1, 1]),
               lambda: q.reflect([0, 7]), lambda: q.reflect([]), lambda: q.reflect([0], ctl=[0]),
               lambda: q.project_onto([1, 2], np.zeros(4)), lambda: q.project_onto([1, 2], np.ones(8))):
    with pytest.raises(ValueError):
      call()
  assert Rank1Oracle.calls_seen == []
  backend.set_device_factory(fake_device.OracleDevice)
  q2 = _prepared(4, 1)
  for call in (lambda: q2.rank_one([0], [1, 0]), lambda: q2.reflect([0, 1]), lambda: q2.diffusion([0, 1, 2]), lambda: q2.project_onto([1])):
    with pytest.raises(NotImplementedError):
      call()


def test_grover_search_on_10_qubits(cpu_backend):
  """phase_oracle + diffusion: the marked amplitude after t iterations is sin((2t + 1) theta), sin(theta) = 2^(-n/2)"""
  n, marked = 10, 0b1001101011
  q = circuit.qc('grover')
  q.reg(n, 0)
  for i in range(n):
    q.h(i)
  table = np.zeros(1 << n, dtype=np.int64)
  table[marked] = 1
  theta = np.arcsin(2.0 ** (-n / 2.0))
  atol = 1e-12 if cpu_backend == 128 else 2e-5
  for t in range(1, int(np.pi / (4 * theta)) + 1):
    q.phase_oracle(table, list(range(n)))
    q.diffusion(list(range(n)))
    amp = complex(np.asarray(q.psi)[marked])
    assert abs(amp - np.sin((2 * t + 1) * theta)) < atol
  assert abs(np.asarray(q.psi)[marked]) ** 2 > 0.999


def test_amplitude_amplification_about_a_random_state(cpu_backend):
  """Q = (2|phi><phi| - I)(I - 2|good><good|) on a 6-qubit register of a 7-qubit circuit, started in phi: the good amplitude
  after t rounds is sin((2t + 1) theta) with sin(theta) = |<good|phi>| (up to phi's phase there)"""
  rng = np.random.default_rng(17)
  n, reg = 7, [6, 0, 3, 4, 1, 5]
  k = len(reg)
  phi = rand_vector(rng, k)
  good = 37
  phi *= np.exp(-1j * np.angle(phi[good]))               # a real, positive overlap
  theta = np.arcsin(abs(phi[good]))
  q = circuit.qc('aa')
  q.reg(n, 0)
  bits = [n - 1 - r for r in reversed(reg)]
  idx, s = rank1_util.register_value(n, bits)
  start = np.where(((idx >> (n - 1 - 2)) & 1) == 0, phi[s], 0)      # |phi> on the register, qubit 2 at 0
  q.psi = start.astype(np.asarray(q.psi).dtype)
  table = np.zeros(1 << k, dtype=np.int64)
  table[good] = 1
  atol = 1e-12 if cpu_backend == 128 else 2e-5
  for t in range(1, 6):
    q.phase_oracle(table, reg)
    q.reflect(reg, phi * 2.5)
    psi = np.asarray(q.psi)
    amp = psi[(s == good) & (((idx >> (n - 1 - 2)) & 1) == 0)][0]
    assert abs(amp - np.sin((2 * t + 1) * theta)) < atol


def test_project_onto_probabilities(cpu_backend):
  rng = np.random.default_rng(23)
  n, reg = 6, [4, 1, 2]
  atol = 1e-12 if cpu_backend == 128 else 2e-6
  q = _prepared(n, 5)
  psi0 = np.asarray(q.psi).astype(np.complex128)
  bits = [n - 1 - r for r in reversed(reg)]
  phi = rand_vector(rng, 3)
  _, m, _ = rank1_parts(psi0, n, bits, None, phi, 0.0, 1.0)
  first = (np.arange(1 << n) & sum(1 << x for x in bits)) == 0
  want_p = float(np.sum(np.abs(m[first]) ** 2))
  p = q.project_onto(reg, 2.0 * phi, normalize=False)
  assert abs(p - want_p) < atol
  assert np.allclose(np.asarray(q.psi), rank1_reference(psi0, n, bits, None, phi, 0.0, 1.0), atol=atol)
  assert abs(q.project_onto(reg, phi) - want_p) < atol * 4         # a projector: applying it again changes nothing ...
  assert abs(float(np.vdot(np.asarray(q.psi), np.asarray(q.psi)).real) - 1) < 10 * atol      # ... and now the state is normalised
  # the uniform state, and a vanishing probability
  q2 = circuit.qc('zero')
  q2.reg(3, 0)
  q2.h(0)
  assert abs(q2.project_onto([1, 2], normalize=False) - 0.25) < atol
  q2.x(1)                                                # (queued gates are drained first)
  q3 = circuit.qc('orth')
  q3.reg(2, 0)
  with pytest.raises(ValueError):
    q3.project_onto([0, 1], [0, 1, 0, 0])                # |00> has no component along |01>
