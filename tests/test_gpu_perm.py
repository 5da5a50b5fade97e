"""qh_apply_perm on the MI355X: amplitudes moved by a table over up to 16 bits, against the NumPy reference of
tests/test_perm_cpu.py.

A permutation does no arithmetic, so the standard is BIT-FOR-BIT at both widths: sync, download, call, download, then
np.array_equal(after, perm_reference(before, ...)).  A tolerance (that of tests/test_gpu_mux.py::_check, one 2x2 per amplitude)
appears only where 2x2 gates of other calls run between two downloads.

Every tier at its smallest shapes, cases placed by physical position, a bit map left by relayout sweeps, inverses, attached and
host-mapped handles, shard handles, stats, and qc.modmul / qc.add / order finding end to end.
QH_ERR_NOMEM of the second path (no room for the scratch buffer) is not tested here: the owning buffer type
(qcc_amd/csrc/buffers.hip.h) has no fault-injection switch, and filling the device's memory to provoke the failure is not
something a test suite should do on a shared GPU; the path is a plain early return before anything is launched."""
import ctypes

import numpy as np
import pytest

from qcc_amd import device, gates, native
from qcc_amd.lib import backend, circuit, tensor
from tests import oracle_lib
from tests.test_perm_cpu import order_finding_circuit, order_finding_model, perm_reference

pytestmark = pytest.mark.gpu

_KS = [1, 2, 3, 5, 9, 10, 11, 13, 14, 16]      # straddle both LDS budgets (13 / 14 tile bits) and the switch to the gather path


def _rand_state(rng, n):
  v = rng.normal(size=1 << n) + 1j * rng.normal(size=1 << n)
  return v / np.linalg.norm(v)


def _bitmap(st, n):
  bm = (ctypes.c_int32 * 64)()
  native.check(st.lib.qh_get_bitmap(st.h, bm))
  return list(bm)[:n]


def _at(bm, phys):
  """logical bits that sit on the physical positions `phys` now"""
  inv = {p: b for b, p in enumerate(bm)}
  return [inv[p] for p in phys]


def _check(got, want, bw):
  got = np.asarray(got, dtype=np.complex128)
  if bw == 128:
    err = float(np.max(np.abs(got - want)))
    assert err < 1e-12, err
  else:
    err = float(np.linalg.norm(got - want) / np.linalg.norm(want))
    assert err < 1e-5, err


def _exact(st, n, table, bits, ctl=0):
  """sync, download, call, download: bit-for-bit"""
  st.sync()
  before = st.download()
  st.apply_perm(table, bits, ctl)
  after = st.download()
  assert after.dtype == before.dtype
  assert np.array_equal(after, perm_reference(before, n, table, bits, ctl))
  return before, after


@pytest.mark.parametrize('k', _KS)
@pytest.mark.parametrize('bw', [128, 64])
@pytest.mark.parametrize('fusion', [native.QH_FUSE_OFF, native.QH_FUSE_SWEEP])
def test_every_tier_smallest_shapes(bw, fusion, k):
  rng = np.random.default_rng(1000 * k + bw + 7 * fusion)
  o = oracle_lib.load()
  h_gate, ry = np.asarray(gates.hadamard(), np.complex128), np.asarray(gates.ry(0.7), np.complex128)
  dtype = np.complex128 if bw == 128 else np.complex64
  paths = set()
  for n in sorted({k, k + 1, k + 3, 13, 20}):
    if n < k:
      continue
    perm = [int(b) for b in rng.permutation(n)]
    reg = perm[:k]                                       # a random unordered subset
    ctl = (1 << perm[k]) if n > k and rng.integers(2) else 0
    table, table2 = rng.permutation(1 << k), rng.permutation(1 << k)
    psi = _rand_state(rng, n)
    with device.DeviceState(n, bw, fusion=fusion) as st:
      paths.add(st.perm_plan(reg, ctl)['path'])
      st.upload(psi.astype(dtype))
      st.apply1(h_gate, 0)
      _, after = _exact(st, n, table, reg, ctl)
      # gates queued (fusion on) before the call and after it
      want = after.astype(np.complex128)
      st.apply1(h_gate, n - 1)
      o.apply1(want, h_gate, n, n - 1)
      st.apply_perm(table2, reg, ctl)
      want = perm_reference(want, n, table2, reg, ctl)
      st.apply1(ry, 0)
      o.apply1(want, ry, n, 0)
      _check(st.download(), want, bw)
  if k <= 10:
    assert paths == {native.QH_PERM_LDS}
  if k >= 15:
    assert paths == {native.QH_PERM_GATHER}


# (name, n, physical register positions in table-bit order, physical control positions)
_PLACED = [
    ('line_only', 14, [0, 1, 2], []),
    ('line_only_c64', 14, [3, 0, 2, 1], [4]),
    ('line_and_lane', 14, [1, 2, 3, 4, 5], [0]),                  # a control on a line bit
    ('lane', 14, [3, 4, 5, 6, 7, 8], [13, 1]),
    ('lane_3_12', 20, list(range(3, 13)), [15]),
    ('top', 14, [13, 12, 11, 10], [0, 5, 9]),                     # controls on a line bit, inside the padding, outside the tile
    ('top_20', 20, list(range(10, 20)), [2, 9]),                  # 13 tile bits at complex128: 128 KiB of LDS
    ('one_run', 20, list(range(5, 15)), [16]),
    ('one_run_reversed', 20, list(range(14, 4, -1)), [16, 17]),
    ('scattered', 20, [0, 3, 6, 9, 12, 15, 19], [1, 16, 18]),
    ('small_register_many_tiles', 20, [4, 7], [11, 13]),          # 2^10 tiles, 3/4 of them skipped
    ('three_outside_controls', 20, [0, 5, 19], [12, 14, 17]),     # 2^9 tiles numbered, 2^6 run
    ('k11_high', 20, list(range(9, 20)), [3]),                    # 14 / 15 tile bits: the gather path at either width
    ('k11_with_line', 20, [0, 1, 2, 3] + list(range(13, 20)), [5]),      # 11 bits of tile at complex64, 11 at complex128: LDS
    ('k14_all_low', 16, list(range(14)), [15]),                   # complex64: 14 bits = 128 KiB of LDS; complex128: gather
    ('k13_c128_limit', 20, [0, 1, 2] + list(range(10, 20)), []),  # 13 bits: LDS at complex128, 14 bits at complex64: LDS
]


@pytest.mark.parametrize('bw', [128, 64])
@pytest.mark.parametrize('case', _PLACED, ids=[c[0] for c in _PLACED])
def test_placed_by_physical_position(case, bw):
  _, n, regp, ctlp = case
  rng = np.random.default_rng(len(regp) * 100 + n + bw)
  dtype = np.complex128 if bw == 128 else np.complex64
  psi = _rand_state(rng, n)
  with device.DeviceState(n, bw) as st:
    bm = _bitmap(st, n)
    reg, ctl = _at(bm, regp), sum(1 << b for b in _at(bm, ctlp))
    plan = st.perm_plan(reg, ctl)
    assert plan['reg_pos'][:len(regp)] == regp
    st.upload(psi.astype(dtype))
    for _ in range(2):
      _exact(st, n, rng.permutation(1 << len(regp)), reg, ctl)
    assert _bitmap(st, n) == bm


@pytest.mark.parametrize('bw', [128, 64])
def test_tile_count_that_is_not_a_multiple_of_the_grid(bw, monkeypatch):
  """Tile counts and the default grid are powers of two; QH_PERM_GRID caps the grid (read at every call), here at 5, 3 and 7
  blocks for 128, 64 and 64 tiles: blocks of one launch then walk different numbers of tiles, each with both barriers."""
  rng = np.random.default_rng(bw)
  n = 17
  with device.DeviceState(n, bw) as st:
    st.upload(_rand_state(rng, n).astype(st.dtype))
    bm = _bitmap(st, n)
    for grid, regp, ctlp in ((5, [2, 5, 9, 6], []), (3, [11, 4, 3], [16, 1]), (7, [1, 13, 12, 10, 14], [8])):
      monkeypatch.setenv('QH_PERM_GRID', str(grid))
      reg, ctl = _at(bm, regp), sum(1 << b for b in _at(bm, ctlp))
      assert st.perm_plan(reg, ctl)['path'] == native.QH_PERM_LDS
      _exact(st, n, rng.permutation(1 << len(regp)), reg, ctl)


def test_permuted_layout_left_by_relayout_sweeps():
  from tests.test_gpu_relayout import _high_bit_circuit   # (a circuit whose sweeps re-lay the state out)
  n = 20
  rng = np.random.default_rng(9)
  ops_, g8 = _high_bit_circuit(n, 7)
  with device.DeviceState(n, 128, fusion=native.QH_FUSE_SWEEP) as st:
    st.upload(_rand_state(rng, n))
    st.run_stream(ops_, g8)
    st.flush()
    bm = _bitmap(st, n)
    assert bm != list(range(n)), 'the sweeps should have left a permuted bit map'
    for reg, ctl in (([17, 0, 19, 2, 9, 13], 1 << 5), ([18, 1, 16, 3, 14, 5, 12, 7, 10, 9, 8], 0),
                     ([int(b) for b in rng.permutation(n)[:14]], 0)):
      plan = st.perm_plan(reg, ctl)
      assert plan['reg_pos'][:len(reg)] == [bm[b] for b in reg]
      table = rng.permutation(1 << len(reg))
      with st.clone() as snap:                           # (a download would bring st itself back to canonical order)
        before = snap.download()
      st.apply_perm(table, reg, ctl)
      assert _bitmap(st, n) == bm                        # the call works on the layout it finds
      with st.clone() as snap:
        assert np.array_equal(snap.download(), perm_reference(before, n, table, reg, ctl))


@pytest.mark.parametrize('bw', [128, 64])
def test_table_then_inverse_restores_the_state(bw):
  rng = np.random.default_rng(bw)
  n = 16
  dtype = np.complex128 if bw == 128 else np.complex64
  psi = _rand_state(rng, n).astype(dtype)
  with device.DeviceState(n, bw) as st:
    st.upload(psi)
    seen = set()
    for k, controlled in ((6, False), (10, True), (12, False), (15, True)):     # both paths
      perm = [int(b) for b in rng.permutation(n)]
      reg, ctl = perm[:k], (1 << perm[k]) if controlled else 0
      table = rng.permutation(1 << len(reg))
      seen.add(st.perm_plan(reg, ctl)['path'])
      st.apply_perm(table, reg, ctl)
      assert not np.array_equal(st.download(), psi)
      st.apply_perm(np.argsort(table), reg, ctl)
      assert np.array_equal(st.download(), psi)
    assert seen == {native.QH_PERM_LDS, native.QH_PERM_GATHER}


def test_back_to_back_tables_each_take_effect():
  rng = np.random.default_rng(5)
  n = 14
  psi = _rand_state(rng, n)
  want = psi.copy()
  with device.DeviceState(n, 128) as st:
    st.upload(psi)
    for k in [3, 9, 12, 1, 14, 5, 10, 11, 7, 13, 2]:       # the table buffer grows and is reused, both paths interleaved
      reg = np.asarray(rng.permutation(n)[:k], dtype=np.int32)
      table = np.ascontiguousarray(rng.permutation(1 << k), dtype=np.uint32)
      want = perm_reference(want, n, table.copy(), list(reg), 0)
      native.check(st.lib.qh_apply_perm(st.h, k, reg.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), 0,
                                        table.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))))
      table[:] = 0                                       # the caller's table is overwritten right away; no sync in between
    assert np.array_equal(st.download(), want)


@pytest.mark.parametrize('kind', ['attached', 'host_mapped'])
def test_device_pointer_stays_in_both_paths(kind):
  rng = np.random.default_rng(3)
  n = 16
  psi = _rand_state(rng, n)

  def run(st, read):
    ptr = st.device_ptr
    st.upload(psi)
    want = psi
    bm = _bitmap(st, n)
    for regp in ([9, 2, 14, 5, 0, 7, 11], [15, 3, 8] + list(range(4, 8)) + list(range(9, 15))):     # LDS, then the gather path with a borrowed second buffer
      k = len(regp)
      reg = _at(bm, regp)
      table = rng.permutation(1 << k)
      assert st.perm_plan(reg)['path'] == (native.QH_PERM_LDS if k == 7 else native.QH_PERM_GATHER)
      st.apply_perm(table, reg)
      want = perm_reference(want, n, table, reg)
      assert st.device_ptr == ptr
      st.sync()
      assert np.array_equal(read(), want)

  if kind == 'attached':
    with device.DeviceState(n, 128) as owner:
      with device.DeviceState(n, 128, device_ptr=owner.device_ptr) as att:
        run(att, owner.download)                         # the owner sees the result in ITS memory
  else:
    with device.DeviceState(n, 128, host_mapped=True) as st:
      run(st, lambda: st.host_array().copy())


def test_shard_handles():
  rng = np.random.default_rng(13)
  nl, n = 10, 12
  psi = _rand_state(rng, n)
  reg, table = [3, 0, 7, 9, 1], rng.permutation(32)
  h_gate = np.asarray(gates.hadamard(), np.complex128)
  for s in range(4):
    with device.DeviceState(nl, 128, fusion=native.QH_FUSE_SWEEP) as st:
      st.set_shard(n, s)
      mine = psi[s << nl:(s + 1) << nl]
      st.upload(mine)
      st.sync()
      st.reset_stats()
      # a control on a shard bit: dropped where met, a counted no-op where not
      st.apply_perm(table, reg, (1 << 10) | (1 << 5))
      want = perm_reference(psi, n, table, reg, (1 << 10) | (1 << 5))[s << nl:(s + 1) << nl]
      got = st.download()
      assert np.array_equal(got, want)
      stats = st.stats()
      if s & 1:
        assert stats['gates_noop'] == 0 and stats['kernels_launched'] == 1 and not np.array_equal(got, mine)
      else:
        assert stats['gates_noop'] == 1 and stats['kernels_launched'] == 0 and np.array_equal(got, mine)
      assert stats['gates_submitted'] == 1
      # a register bit on a shard bit: refused, the state and the pending queue as they were
      st.apply1(h_gate, n - 1 - 2)                       # (reference qubit numbers: logical bit 2) stays queued
      pending = ctypes.c_uint64()
      native.check(st.lib.qh_pending_gates(st.h, ctypes.byref(pending)))
      assert pending.value == 1
      with pytest.raises(native.QhError) as e:
        st.apply_perm(table, [3, 11, 7, 9, 1])
      assert e.value.code == native.QH_ERR_NONLOCAL
      native.check(st.lib.qh_pending_gates(st.h, ctypes.byref(pending)))
      assert pending.value == 1 and st.stats()['kernels_launched'] == stats['kernels_launched']
      native.check(st.lib.qh_discard_pending(st.h))
      assert np.array_equal(st.download(), want)


def test_stats_of_both_paths():
  n = 18
  rng = np.random.default_rng(2)
  with device.DeviceState(n, 128, fusion=native.QH_FUSE_SWEEP) as st:
    st.init_basis(5)
    st.sync()
    bm = _bitmap(st, n)
    state_bytes = 16 << n
    # LDS: register on positions 4-8, controls on position 1 (inside the tile) and 12, 15 (outside): a quarter of the tiles run
    reg, ctl = _at(bm, [4, 5, 6, 7, 8]), sum(1 << b for b in _at(bm, [1, 12, 15]))
    assert st.perm_plan(reg, ctl)['path'] == native.QH_PERM_LDS
    s0 = st.stats()
    st.apply_perm(rng.permutation(32), reg, ctl)
    s1 = st.stats()
    assert s1['kernels_launched'] - s0['kernels_launched'] == 1
    assert s1['gates_submitted'] - s0['gates_submitted'] == 1
    assert s1['bytes_algorithmic'] - s0['bytes_algorithmic'] == 2 * state_bytes // 8
    assert s1['bytes_swept'] - s0['bytes_swept'] == 2 * state_bytes // 4
    assert s1['sweeps'] == s0['sweeps'] and s1['gates_noop'] == s0['gates_noop']
    # gather: 12 high bits, one control: the kernel reads and writes the state once, the copy back once more
    reg, ctl = _at(bm, list(range(6, 18))), 1 << _at(bm, [2])[0]
    assert st.perm_plan(reg, ctl)['path'] == native.QH_PERM_GATHER
    st.apply_perm(rng.permutation(1 << 12), reg, ctl)
    s2 = st.stats()
    assert s2['kernels_launched'] - s1['kernels_launched'] == 1
    assert s2['gates_submitted'] - s1['gates_submitted'] == 1
    assert s2['bytes_algorithmic'] - s1['bytes_algorithmic'] == 2 * state_bytes // 2
    assert s2['bytes_swept'] - s1['bytes_swept'] == 4 * state_bytes
    assert abs(st.norm2() - 1) < 1e-15


# ---- through qc ------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def width128():
  tensor.set_tensor_width(128)
  yield
  tensor.set_tensor_width(None)
  backend.drop_device_pool()


def test_order_finding_7_mod_15(width128):
  t, n = 8, 4
  q, read = order_finding_circuit(7, 15, t, n)
  p = q.probabilities(read)
  assert np.max(np.abs(p - order_finding_model(7, 15, t, n))) < 1e-12
  assert list(np.flatnonzero(p > 0.2)) == [0, 64, 128, 192]
  q.close()


def test_modmul_under_a_control_at_16_qubits(width128):
  n = 16
  rng = np.random.default_rng(16)
  q = circuit.qc('modmul')
  q.reg(n, 0)
  for i in range(n):
    q.ry(i, float(rng.uniform(0.2, np.pi - 0.2)))
  q.cx(0, n - 1)
  reg, ctl = [int(x) for x in rng.permutation(np.arange(1, n))[:11]], 0
  before = np.asarray(q.psi).copy()
  a, N = 1234, 2039                                      # 2039 is prime, below 2^11
  q.modmul(a, N, reg, ctl=[ctl])
  after = np.asarray(q.psi).copy()
  x = np.arange(1 << 11)
  table = np.where(x < N, (x * a) % N, x)
  bits = [n - 1 - r for r in reversed(reg)]
  assert np.array_equal(after, perm_reference(before, n, table, bits, 1 << (n - 1 - ctl)))
  assert not np.array_equal(after, before)
  q.modmul(pow(a, -1, N), N, reg, ctl=[ctl])
  assert np.array_equal(np.asarray(q.psi), before)
  q.close()


def _fourier_adder(q, a, b):
  """a += b mod 2^len(a) from Hadamards and controlled phases (the Fourier-space adder the reference's arith_quantum is an
  instance of): a, b list their qubits LEAST significant first.  After the transform qubit a[j] carries the phase
  2 pi (a mod 2^(j+1)) / 2^(j+1); adding b is one controlled phase per pair (b[i], a[j]), i <= j."""
  m = len(a)
  for j in reversed(range(m)):
    q.h(a[j])
    for i in range(j):
      q.cu1(a[i], a[j], 2 * np.pi / (1 << (j - i + 1)))
  for j in range(m):
    for i in range(min(j, len(b) - 1) + 1):
      q.cu1(b[i], a[j], 2 * np.pi / (1 << (j - i + 1)))
  for j in range(m):
    for i in range(j):
      q.cu1(a[i], a[j], -2 * np.pi / (1 << (j - i + 1)))
    q.h(a[j])


def test_add_matches_the_fourier_space_adder(width128):
  n = 8
  rng = np.random.default_rng(8)
  q = circuit.qc('add')
  q.reg(n, 0)
  for i in range(n):
    q.ry(i, float(rng.uniform(0.2, np.pi - 0.2)))
  q.cx(1, 6)
  start = np.asarray(q.psi).copy()
  a, b = [0, 1, 2, 3], [4, 5, 6, 7]                      # least significant first, as the reference's registers are
  _fourier_adder(q, a, b)
  want = np.asarray(q.psi).copy()
  q.psi = start                                          # the same handle, the same start
  q.add(list(reversed(b)), list(reversed(a)))
  got = np.asarray(q.psi).copy()
  assert np.max(np.abs(got - want)) < 1e-10
  assert np.max(np.abs(got - start)) > 1e-3
  q.close()
