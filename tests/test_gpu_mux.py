"""qh_apply_mux / qh_apply_diag on the MI355X: gates selected by a table over up to 16 bits, against the NumPy references of
tests/test_mux_cpu.py.

Every tier of the kernels at its smallest shape (both widths, fusion off and on, 2x2 gates around the call), cases placed
by physical position, a permuted bit map left by relayout sweeps, exact cases, tables queued back to back, stats, sharded
and host-mapped handles, and two algorithms end to end through qc (Moettoenen state preparation, Grover).
Tolerances are those of tests/test_gpu_dense.py::_check (one 2x2 per amplitude)."""
import ctypes

import numpy as np
import pytest

from qcc_amd import device, gates, native
from qcc_amd.lib import backend, circuit, tensor
from tests import oracle_lib
from tests.test_mux_cpu import diag_reference, mux_reference_fast as mux_reference

pytestmark = pytest.mark.gpu

_KS = [0, 1, 2, 5, 9, 10, 11, 12, 13, 16]      # straddle the LDS limits of both calls (mux fits through 10, diag through 12)


def _rand_state(rng, n):
  v = rng.normal(size=1 << n) + 1j * rng.normal(size=1 << n)
  return v / np.linalg.norm(v)


def _rand_gates(rng, k, unitary):
  a = rng.normal(size=(1 << k, 2, 2)) + 1j * rng.normal(size=(1 << k, 2, 2))
  if unitary:
    a, _ = np.linalg.qr(a)
  return a


def _rand_values(rng, k, unitary):
  v = rng.normal(size=1 << k) + 1j * rng.normal(size=1 << k)
  return v / np.abs(v) if unitary else v


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


@pytest.mark.parametrize('k', _KS)
@pytest.mark.parametrize('bw', [128, 64])
@pytest.mark.parametrize('fusion', [native.QH_FUSE_OFF, native.QH_FUSE_SWEEP])
def test_every_tier_smallest_shapes(bw, fusion, k):
  rng = np.random.default_rng(1000 * k + bw + 7 * fusion)
  o = oracle_lib.load()
  h_gate, ry = np.asarray(gates.hadamard(), np.complex128), np.asarray(gates.ry(0.7), np.complex128)
  dtype = np.complex128 if bw == 128 else np.complex64
  for n in sorted({k + 1, k + 3, 13, 20}):
    if n < k + 1:
      continue
    perm = [int(b) for b in rng.permutation(n)]
    sel, tgt = perm[:k], perm[k]                       # a random unordered subset, the target a remaining bit
    unitary = bool(rng.integers(2))
    g, v = _rand_gates(rng, k, unitary), _rand_values(rng, k, unitary)
    psi = _rand_state(rng, n)
    for call in ('mux', 'diag'):
      want = psi.copy()
      with device.DeviceState(n, bw, fusion=fusion) as st:
        st.upload(psi.astype(dtype))
        st.apply1(h_gate, 0)                           # queued (fusion on) before the call
        o.apply1(want, h_gate, n, 0)
        if call == 'mux':
          st.apply_mux(g, sel, tgt)
          want = mux_reference(want, n, g, sel, tgt)
        else:
          st.apply_diag(v, sel)
          want = diag_reference(want, n, v, sel)
        st.apply1(ry, n - 1)                           # and after it
        o.apply1(want, ry, n, n - 1)
        _check(st.download(), want, bw)


def _at(bm, phys):
  """logical bits that sit on the physical positions `phys` now"""
  inv = {p: b for b, p in enumerate(bm)}
  return [inv[p] for p in phys]


# (name, n, physical selector positions, physical target positions tried for the mux)
_PLACED = [
    ('sel_mixed_tgt_everywhere', 14, [9, 1, 6, 12], [0, 2, 3, 4, 5, 13]),      # line, lane and top targets; LDS tier
    ('sel_all_high', 14, [10, 8, 13, 11], [0, 1, 2, 3, 5, 12]),                # wave-uniform tier, every kernel shape
    ('sel_above_lanes', 14, [7, 9], [6, 3]),                                   # wave-uniform for either target
    ('sel_on_bit_6', 14, [6, 9], [7, 3]),                                      # a target below 6 moves the lane positions up to bit 6
    ('sel_line_bits', 14, [0, 1, 2, 7], [3, 5, 13]),
    ('sel_line_bits_line_target', 14, [0, 2, 4, 9], [1]),
    ('sel_one_run', 14, [3, 4, 5, 6, 7, 8, 9], [1, 11]),                       # one contiguous run ...
    ('sel_one_run_reversed', 14, [9, 8, 7, 6, 5, 4, 3], [1, 11]),              # ... the same bits, no run longer than one
    ('sel_scattered', 14, [0, 2, 4, 6, 8, 10, 12], [1, 5, 13]),
    ('sel_high_big_table', 20, list(range(8, 19)), [19, 4, 0]),                # k = 11, wave-uniform: scalar loads of a 128 KiB table
    ('sel_low_big_table', 20, list(range(0, 11)), [19, 11]),                   # k = 11 through L2
]


@pytest.mark.parametrize('bw', [128, 64])
@pytest.mark.parametrize('case', _PLACED, ids=[c[0] for c in _PLACED])
def test_placed_by_physical_position(case, bw):
  _, n, selp, tgts = case
  rng = np.random.default_rng(len(selp) * 100 + n + bw)
  dtype = np.complex128 if bw == 128 else np.complex64
  k = len(selp)
  psi = _rand_state(rng, n)
  with device.DeviceState(n, bw) as st:
    bm = _bitmap(st, n)
    sel = _at(bm, selp)
    for tp in tgts:
      g = _rand_gates(rng, k, True)
      st.upload(psi.astype(dtype))
      st.apply_mux(g, sel, _at(bm, [tp])[0])
      _check(st.download(), mux_reference(psi, n, g, sel, _at(bm, [tp])[0]), bw)
    v = _rand_values(rng, k, False)
    st.upload(psi.astype(dtype))
    st.apply_diag(v, sel)
    _check(st.download(), diag_reference(psi, n, v, sel), bw)
    assert _bitmap(st, n) == bm


def test_permuted_layout_and_readers():
  from tests.test_gpu_relayout import _high_bit_circuit   # (a circuit whose sweeps re-lay the state out)
  n = 22
  rng = np.random.default_rng(9)
  ops_, g8 = _high_bit_circuit(n, 7)
  psi = _rand_state(rng, n)
  want = psi.copy()
  oracle_lib.load().run_stream(want, n, ops_, g8)
  sel, tgt = [17, 0, 21, 2, 9, 13], 5
  dbits = [20, 1, 18, 3, 16, 5, 14, 7, 12, 9, 10]
  g, v = _rand_gates(rng, 6, False), _rand_values(rng, 11, True)
  want = diag_reference(mux_reference(want, n, g, sel, tgt), n, v, dbits)
  with device.DeviceState(n, 128, fusion=native.QH_FUSE_SWEEP) as st:
    st.upload(psi)
    st.run_stream(ops_, g8)
    st.flush()
    bm = _bitmap(st, n)
    assert bm != list(range(n)), 'the sweeps should have left a permuted bit map'
    st.apply_mux(g, sel, tgt)
    st.apply_diag(v, dbits)
    assert _bitmap(st, n) == bm                        # the calls work on the layout they find
    for i in (0, 12345, (1 << n) - 1, int(np.argmax(np.abs(want)))):
      assert abs(st.amplitude(i) - want[i]) < 1e-12
    mb = [21, 0, 9, 5]
    idx = np.arange(1 << n)
    s = sum(((idx >> b) & 1) << j for j, b in enumerate(mb))
    assert np.max(np.abs(st.marginal(mb) - np.bincount(s, weights=np.abs(want) ** 2, minlength=16))) < 1e-12
    _check(st.download(), want, 128)


@pytest.fixture
def width128():
  tensor.set_tensor_width(128)
  yield
  tensor.set_tensor_width(None)
  backend.drop_device_pool()


def test_oracles_are_exact(width128):
  n, k = 14, 13
  rng = np.random.default_rng(14)
  q = circuit.qc('exact')
  q.reg(n, 0)
  for i in range(n):
    q.ry(i, float(rng.uniform(0, np.pi)))
  q.cx(0, n - 1)
  xs = [int(x) for x in rng.permutation(n)]
  xs, y = xs[:k], xs[k]
  table = rng.integers(0, 2, size=1 << k)
  before = np.asarray(q.psi).copy()
  q.oracle(table, xs, y)
  after = np.asarray(q.psi).copy()
  xi = np.stack([np.eye(2), np.eye(2)[::-1]])
  bits = [n - 1 - x for x in reversed(xs)]
  assert np.array_equal(after, mux_reference(before, n, xi[table], bits, n - 1 - y))
  assert not np.array_equal(after, before)
  ptable = rng.integers(0, 2, size=1 << k)
  q.phase_oracle(lambda b: int(ptable[int(''.join(str(v) for v in b), 2)]), xs)
  assert np.array_equal(np.asarray(q.psi), diag_reference(after, n, 1.0 - 2.0 * ptable, bits))
  q.close()


def test_back_to_back_tables_each_take_effect():
  rng = np.random.default_rng(5)
  n = 12
  psi = _rand_state(rng, n)
  want = psi.copy()
  ks = [3, 9, 0, 11, 5, 10, 1, 11, 7, 2, 6, 11, 4, 8, 10, 9, 0, 11, 3, 5]      # the table buffer grows and is reused
  with device.DeviceState(n, 128) as st:
    st.upload(psi)
    lib = st.lib
    for i, k in enumerate(ks):
      perm = np.asarray(rng.permutation(n), dtype=np.int32)
      sel = np.ascontiguousarray(perm[:k])
      sp = sel.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
      if i % 2 == 0:
        g = _rand_gates(rng, k, True)
        buf = g.copy()
        native.check(lib.qh_apply_mux(st.h, k, sp, int(perm[k]), buf.ctypes.data_as(ctypes.POINTER(ctypes.c_double))))
        want = mux_reference(want, n, g, list(sel), int(perm[k]))
      else:
        v = _rand_values(rng, k, True)
        buf = v.copy()
        native.check(lib.qh_apply_diag(st.h, k, sp, buf.ctypes.data_as(ctypes.POINTER(ctypes.c_double))))
        want = diag_reference(want, n, v, list(sel))
      buf[:] = np.nan                                  # the caller's table is overwritten right away; no sync in between
    _check(st.download(), want, 128)


@pytest.mark.parametrize('k', [0, 9, 16])
def test_stats_one_kernel_per_call(k):
  n = 18
  rng = np.random.default_rng(k)
  perm = [int(b) for b in rng.permutation(n)]
  with device.DeviceState(n, 128, fusion=native.QH_FUSE_SWEEP) as st:
    st.init_basis(5)
    st.sync()
    state_bytes = 2 * 16 << n
    for call in ('mux', 'diag'):
      s0 = st.stats()
      if call == 'mux':
        st.apply_mux(_rand_gates(rng, k, True), perm[:k], perm[k])
      else:
        st.apply_diag(_rand_values(rng, k, True), perm[:k])
      s1 = st.stats()
      assert s1['kernels_launched'] - s0['kernels_launched'] == 1
      assert s1['gates_submitted'] - s0['gates_submitted'] == 1
      assert s1['bytes_swept'] - s0['bytes_swept'] == state_bytes
      assert s1['bytes_algorithmic'] - s0['bytes_algorithmic'] == state_bytes
      assert s1['sweeps'] == s0['sweeps']
    assert abs(st.norm2() - 1) < 1e-12


def test_sharded_handles():
  rng = np.random.default_rng(13)
  nl, n = 10, 12
  psi = _rand_state(rng, n)
  sel, tgt = [3, 11, 0, 10, 7], 5                      # two selectors on the shard index
  dbits = [10, 2, 11, 9]
  dall = [11, 10]                                      # every bit on the shard index: one scale per shard
  g, v, v2 = _rand_gates(rng, 5, True), _rand_values(rng, 4, False), _rand_values(rng, 2, False)
  want = diag_reference(diag_reference(mux_reference(psi, n, g, sel, tgt), n, v, dbits), n, v2, dall)
  want = mux_reference(want, n, g[:4], [11, 10], 1)    # every selector on the shard index: one gate per shard
  for s in range(4):
    with device.DeviceState(nl, 128) as st:
      st.set_shard(n, s)
      mine = psi[s << nl:(s + 1) << nl]
      st.upload(mine)
      st.reset_stats()
      with pytest.raises(native.QhError) as e:
        st.apply_mux(g, [3, 1, 0, 2, 7], 11)           # a shard-bit target
      assert e.value.code == native.QH_ERR_NONLOCAL
      assert st.stats()['kernels_launched'] == 0 and np.array_equal(st.download(), mine)
      st.apply_mux(g, sel, tgt)
      st.apply_diag(v, dbits)
      st.apply_diag(v2, dall)
      st.apply_mux(g[:4], [11, 10], 1)
      assert st.stats()['kernels_launched'] == 4
      _check(st.download(), want[s << nl:(s + 1) << nl], 128)


@pytest.mark.parametrize('bw', [128, 64])
def test_host_mapped_handle(bw):
  rng = np.random.default_rng(3)
  n = 12
  dtype = np.complex128 if bw == 128 else np.complex64
  psi = _rand_state(rng, n)
  g, v = _rand_gates(rng, 4, True), _rand_values(rng, 6, True)
  sel, tgt, dbits = [7, 0, 11, 3], 1, [2, 9, 4, 0, 10, 6]
  with device.DeviceState(n, bw, host_mapped=True) as st:
    st.upload(psi.astype(dtype))
    st.apply_mux(g, sel, tgt)
    st.apply_diag(v, dbits)
    st.sync()
    _check(st.host_array().copy(), diag_reference(mux_reference(psi, n, g, sel, tgt), n, v, dbits), bw)


def test_mottonen_state_preparation(width128):
  """Qubit j gets a multiplexed Ry over qubits 0..j-1: k runs 0..11 and the target moves from the top index bit down to
  the line bits.  Twelve calls, twelve kernels."""
  n = 12
  rng = np.random.default_rng(12)
  target = np.abs(rng.normal(size=1 << n)) + 0.01
  target /= np.linalg.norm(target)
  q = circuit.qc('mottonen')
  q.reg(n, 0)
  q.sync()
  dev = q._ensure_device()                             # pylint: disable=protected-access
  dev.reset_stats()
  p = target ** 2
  for j in range(n):
    pj = p.reshape(1 << j, 2, -1).sum(axis=2)          # [prefix over qubits 0..j-1, value of qubit j]
    half = np.arctan2(np.sqrt(pj[:, 1]), np.sqrt(pj[:, 0]))
    c, s = np.cos(half), np.sin(half)
    q.multiplex(np.stack([np.stack([c, -s], axis=1), np.stack([s, c], axis=1)], axis=1), list(range(j)), j)
  q.sync()
  st = dev.stats()
  assert st['kernels_launched'] == 12 and st['gates_submitted'] == 12
  assert np.max(np.abs(np.asarray(q.psi) - target)) < 1e-12
  q.close()


def test_grover_with_phase_oracles(width128):
  n, marked = 12, 0xA57
  mark = np.zeros(1 << n, dtype=np.int64)
  mark[marked] = 1
  nonzero = np.ones(1 << n, dtype=np.int64)            # 2|0><0| - 1
  nonzero[0] = 0
  q = circuit.qc('grover')
  q.reg(n, 0)
  for i in range(n):
    q.h(i)
  for _ in range(int(np.pi / 4 * np.sqrt(1 << n))):
    q.phase_oracle(mark, list(range(n)))
    for i in range(n):
      q.h(i)
    q.phase_oracle(nonzero, list(range(n)))
    for i in range(n):
      q.h(i)
  bits, prob = q.maxprob()
  assert int(''.join(str(b) for b in bits), 2) == marked
  assert prob > 0.99
  q.close()
