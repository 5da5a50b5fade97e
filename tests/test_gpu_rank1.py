"""qh_apply_rank1 on the MI355X: a I + b |u><v| on a register, against the NumPy reference of tests/rank1_util.py.

Tolerance (rank1_util.tolerance), per component: with amax = max |psi_i| and B = |a| amax + |b| max|u_s| (sum_s |v_s|) amax,
a component carries at most a 2^k-term inner product in double plus a few products: (2^k + 8) 2^-52 B at complex128; complex64
adds one rounding to float, 2^-24 (|new| + B).  (The kernels sum pairwise over the bits inside a tile or chunk, so the real
error is far below the linear bound; the bound is kept as the issue states it.)  The reference is computed from the state as
downloaded right before the call, so nothing but the call lies between the two.  Amplitudes whose controls are 0 must keep
their bits.  A tolerance of the kind tests/test_gpu_mux.py uses appears only where 2x2 gates run between two downloads.

QH_ERR_NOMEM of the second path (no room for the fibre sums) is not provoked, for the reason tests/test_gpu_perm.py gives."""
import ctypes

import numpy as np
import pytest

from qcc_amd import device, gates, native
from qcc_amd.lib import backend, circuit, tensor
from tests import oracle_lib, rank1_util
from tests.rank1_util import rand_state, rand_vector, rank1_parts, tolerance

pytestmark = pytest.mark.gpu

_KS = [1, 2, 3, 5, 9, 10, 11, 13, 14, 16]
_dp = ctypes.POINTER(ctypes.c_double)
_ip = ctypes.POINTER(ctypes.c_int32)


def _bitmap(st, n):
  bm = (ctypes.c_int32 * 64)()
  native.check(st.lib.qh_get_bitmap(st.h, bm))
  return list(bm)[:n]


def _at(bm, phys):
  """logical bits that sit on the physical positions `phys` now"""
  inv = {p: b for b, p in enumerate(bm)}
  return [inv[p] for p in phys]


def _loose(got, want, bw):
  """where 2x2 gates of other calls lie between two downloads (tests/test_gpu_mux.py::_check)"""
  got = np.asarray(got, dtype=np.complex128)
  if bw == 128:
    assert float(np.max(np.abs(got - want))) < 1e-12
  else:
    assert float(np.linalg.norm(got - want) / np.linalg.norm(want)) < 1e-5


def _call(st, n, bits, u=None, v=None, a=-1.0, b=2.0, ctl=0, sums=True, before=None):
  """sync, download, call, download; the result against the reference within the derived tolerance, untouched amplitudes
  bit for bit, the two sums.  Returns (before, after, sums)."""
  if before is None:
    st.sync()
    before = st.download()
  out = st.apply_rank1(bits, u=u, v=v, a=a, b=b, ctl_mask=ctl, sums=sums)
  after = st.download()
  assert after.dtype == before.dtype
  want, m, met = rank1_parts(before, n, bits, u, v, a, b, ctl)
  k = len(bits)
  tol = tolerance(before, k, u, v, a, b, st.bit_width, new=want)
  err = float(np.max(np.abs(after.astype(np.complex128) - want)))
  print(f'n={n} k={k} bw={st.bit_width} err={err:.3e} tol={tol:.3e}')
  assert err <= tol, (err, tol)
  assert np.array_equal(after[~met], before[~met])             # a control at 0: the bits stay
  if sums:
    idx = np.arange(1 << n, dtype=np.int64)
    first = (idx & sum(1 << x for x in bits)) == 0
    want0, want1 = rank1_util.rank1_sums(after, n, bits, m, met)
    amax = float(np.max(np.abs(before.astype(np.complex128))))
    vsum = 2.0 ** (k / 2.0) if v is None else float(np.sum(np.abs(v)))
    dm = ((1 << k) + 8) * 2.0 ** -52 * vsum * amax
    t0, t1 = rank1_util.sums_tolerance(after, m, met, first, dm)
    print(f'   sums {out[0]!r} {out[1]!r} want {want0!r} {want1!r} tol {t0:.3e} {t1:.3e}')
    assert abs(out[0] - want0) <= t0 and abs(out[1] - want1) <= t1
  return before, after, out


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
    perm = [int(x) for x in rng.permutation(n)]
    reg = perm[:k]                                       # a random unordered subset
    ctl = (1 << perm[k]) if n > k and rng.integers(2) else 0
    u, v = rand_vector(rng, k), rand_vector(rng, k)
    a, b = complex(*rng.normal(size=2)), complex(*rng.normal(size=2))
    psi = rand_state(rng, n)
    with device.DeviceState(n, bw, fusion=fusion) as st:
      paths.add(st.rank1_plan(reg, ctl)['path'])
      st.upload(psi.astype(dtype))
      st.apply1(h_gate, 0)
      _, after, _ = _call(st, n, reg, u, v, a, b, ctl)
      # gates queued (fusion on) before the call and after it
      want = after.astype(np.complex128)
      st.apply1(h_gate, n - 1)
      o.apply1(want, h_gate, n, n - 1)
      st.apply_rank1(reg, u=u, v=v, a=b, b=a, ctl_mask=ctl)
      want = rank1_util.rank1_reference(want, n, reg, u, v, b, a, ctl)
      st.apply1(ry, 0)
      o.apply1(want, ry, n, 0)
      _loose(st.download(), want, bw)
  if k <= 10:
    assert paths == {native.QH_RANK1_TILE}
  if k >= 15:
    assert paths == {native.QH_RANK1_TWO_PASS}


@pytest.mark.parametrize('k', [1, 4, 10, 11, 14, 17, 20])
@pytest.mark.parametrize('bw', [128, 64])
def test_uniform_form(bw, k):
  rng = np.random.default_rng(77 * k + bw)
  dtype = np.complex128 if bw == 128 else np.complex64
  for n in sorted({k, 20, 22}):
    psi = rand_state(rng, n).astype(dtype)
    with device.DeviceState(n, bw) as st:
      st.upload(psi)
      bm = _bitmap(st, n)
      placements = [[int(x) for x in rng.permutation(n)[:k]]]
      if k < n <= 20 and k >= 10:
        placements.append(_at(bm, list(range(n - k, n))))          # the free bits lowest ...
        placements.append(_at(bm, list(range(k))))                 # ... and at the top
      for j, reg in enumerate(placements):
        ctl = 0
        if n > k and rng.integers(2):
          ctl = 1 << [x for x in range(n) if x not in reg][0]
        _call(st, n, reg, a=-1.0, b=2.0, ctl=ctl)
        if j == 0 and n <= 20:
          _call(st, n, reg, a=complex(0.3, -1.1), b=complex(-0.7, 0.2), ctl=ctl)


@pytest.mark.parametrize('bw', [128, 64])
def test_uniform_one_free_bit_bottom_and_top(bw):
  """k = n - 1: two fibres; the free bit on physical position 0 (inside every 16-byte item at complex64) and at the top"""
  rng = np.random.default_rng(bw)
  n = 18
  with device.DeviceState(n, bw) as st:
    st.upload(rand_state(rng, n).astype(st.dtype))
    bm = _bitmap(st, n)
    for free in (0, n - 1):
      reg = _at(bm, [p for p in range(n) if p != free])
      plan = st.rank1_plan(reg, uniform=True)
      assert plan['path'] == native.QH_RANK1_TWO_PASS and plan['nfibres'] == 2
      _call(st, n, reg)
      _call(st, n, reg, ctl=1 << _at(bm, [free])[0])


# (name, n, physical register positions in table-bit order, physical control positions)
_PLACED = [
    ('line_only', 14, [0, 1, 2], []),
    ('line_only_c64', 14, [3, 0, 2, 1], [4]),
    ('line_and_lane', 14, [1, 2, 3, 4, 5], [0]),                  # a control on a line bit
    ('lane', 14, [3, 4, 5, 6, 7, 8], [13, 1]),
    ('top', 14, [13, 12, 11, 10], [0, 5, 9]),                     # controls on a line bit, inside the padding, outside the tile
    ('top_20', 20, list(range(10, 20)), [2, 9]),                  # 13 tile bits at complex128, 14 at complex64: the LDS limits
    ('one_run_reversed', 20, list(range(14, 4, -1)), [16, 17]),
    ('scattered', 20, [0, 3, 6, 9, 12, 15, 19], [1, 16, 18]),
    ('small_register_many_tiles', 20, [4, 7], [11, 13]),
    ('k10_with_line', 20, [0, 1, 2] + list(range(13, 20)), [5]),  # 10 tile bits at complex128, 11 at complex64
    ('k11_high', 20, list(range(9, 20)), [3]),                    # the second path, controls inside a chunk
    ('k16_scattered', 20, [0, 1, 3, 4, 6, 7, 8, 10, 11, 12, 14, 15, 16, 17, 18, 19], [2, 13]),
    ('k11_low_unsplit', 22, list(range(10, -1, -1)), [14]),       # 2^10 / 2^11 fibre groups of one chunk: pass 1 writes m itself
]


@pytest.mark.parametrize('bw', [128, 64])
@pytest.mark.parametrize('case', _PLACED, ids=[c[0] for c in _PLACED])
def test_placed_by_physical_position(case, bw):
  name, n, regp, ctlp = case
  rng = np.random.default_rng(len(regp) * 100 + n + bw)
  k = len(regp)
  with device.DeviceState(n, bw) as st:
    bm = _bitmap(st, n)
    reg, ctl = _at(bm, regp), sum(1 << x for x in _at(bm, ctlp))
    plan = st.rank1_plan(reg, ctl)
    assert plan['tile']['reg_pos'][:k] == regp
    if name == 'top_20':
      assert plan['path'] == native.QH_RANK1_TILE and plan['tile']['lds_bytes'] == 128 << 10
    st.upload(rand_state(rng, n).astype(st.dtype))
    _call(st, n, reg, rand_vector(rng, k), rand_vector(rng, k), complex(0.2, 0.9), complex(-1.3, 0.4), ctl)
    _call(st, n, reg, None, rand_vector(rng, k), -1.0, 2.0, ctl)
    if k <= 14:
      _call(st, n, reg, a=-1.0, b=2.0, ctl=ctl)                    # the uniform form on the same bits
    assert _bitmap(st, n) == bm


@pytest.mark.parametrize('bw', [128, 64])
def test_tile_count_that_is_not_a_multiple_of_the_grid(bw, monkeypatch):
  """QH_RANK1_GRID caps the grid (read at every call): blocks of one launch walk different numbers of tiles, each with all
  its barriers, and every block's slab row enters the sums."""
  rng = np.random.default_rng(bw)
  n = 17
  with device.DeviceState(n, bw) as st:
    st.upload(rand_state(rng, n).astype(st.dtype))
    bm = _bitmap(st, n)
    for grid, regp, ctlp in ((5, [2, 5, 9, 6], []), (3, [11, 4, 3], [16, 1]), (7, [1, 13, 12, 10, 14], [8])):
      monkeypatch.setenv('QH_RANK1_GRID', str(grid))
      reg, ctl = _at(bm, regp), sum(1 << x for x in _at(bm, ctlp))
      assert st.rank1_plan(reg, ctl)['path'] == native.QH_RANK1_TILE
      _call(st, n, reg, rand_vector(rng, len(regp)), rand_vector(rng, len(regp)), 0.5, complex(0, 1.5), ctl)


def test_permuted_layout_left_by_relayout_sweeps():
  from tests.test_gpu_relayout import _high_bit_circuit   # (a circuit whose sweeps re-lay the state out)
  n = 20
  rng = np.random.default_rng(9)
  ops_, g8 = _high_bit_circuit(n, 7)
  with device.DeviceState(n, 128, fusion=native.QH_FUSE_SWEEP) as st:
    st.upload(rand_state(rng, n))
    st.run_stream(ops_, g8)
    st.flush()
    bm = _bitmap(st, n)
    assert bm != list(range(n)), 'the sweeps should have left a permuted bit map'
    for reg, ctl in (([17, 0, 19, 2, 9, 13], 1 << 5), ([18, 1, 16, 3, 14, 5, 12, 7, 10, 9, 8], 0),
                     ([int(x) for x in rng.permutation(n)[:14]], 0)):
      k = len(reg)
      plan = st.rank1_plan(reg, ctl)
      assert plan['tile']['reg_pos'][:k] == [bm[x] for x in reg]
      u, v = rand_vector(rng, k), rand_vector(rng, k)
      with st.clone() as snap:                           # (a download would bring st itself back to canonical order)
        before = snap.download()
      st.apply_rank1(reg, u=u, v=v, a=0.4, b=complex(1.0, -2.0), ctl_mask=ctl)
      assert _bitmap(st, n) == bm                        # the call works on the layout it finds
      want, _, met = rank1_parts(before, n, reg, u, v, 0.4, complex(1.0, -2.0), ctl)
      with st.clone() as snap:
        after = snap.download()
      assert float(np.max(np.abs(after - want))) <= tolerance(before, k, u, v, 0.4, complex(1.0, -2.0), 128)
      assert np.array_equal(after[~met], before[~met])


@pytest.mark.parametrize('kind', ['attached', 'host_mapped'])
def test_device_pointer_stays_in_both_paths(kind):
  rng = np.random.default_rng(3)
  n = 16
  psi = rand_state(rng, n)

  def run(st, read):
    ptr = st.device_ptr
    st.upload(psi)
    bm = _bitmap(st, n)
    for regp in ([9, 2, 14, 5, 0, 7, 11], [15, 3, 8] + list(range(4, 8)) + list(range(9, 15))):
      k = len(regp)
      reg = _at(bm, regp)
      assert st.rank1_plan(reg)['path'] == (native.QH_RANK1_TILE if k == 7 else native.QH_RANK1_TWO_PASS)
      st.sync()
      before = read()
      u, v = rand_vector(rng, k), rand_vector(rng, k)
      st.apply_rank1(reg, u=u, v=v, a=complex(0, 1), b=0.5)
      assert st.device_ptr == ptr
      st.sync()
      want = rank1_util.rank1_reference(before, n, reg, u, v, complex(0, 1), 0.5)
      assert float(np.max(np.abs(read() - want))) <= tolerance(before, k, u, v, complex(0, 1), 0.5, 128)

  if kind == 'attached':
    with device.DeviceState(n, 128) as owner:
      with device.DeviceState(n, 128, device_ptr=owner.device_ptr) as att:
        run(att, owner.download)                         # the owner sees the result in ITS memory
  else:
    with device.DeviceState(n, 128, host_mapped=True) as st:
      run(st, lambda: st.host_array().copy())


@pytest.mark.parametrize('bw', [128, 64])
def test_same_call_same_bits(bw):
  rng = np.random.default_rng(40 + bw)
  n = 18
  psi = rand_state(rng, n).astype(np.complex128 if bw == 128 else np.complex64)
  cases = [([3, 9, 0, 14, 6], 1 << 2, False), (list(range(5, 17)), 1 << 1, False), (list(range(n)), 0, True), ([1, 2, 4], 0, True)]
  for reg, ctl, uniform in cases:
    k = len(reg)
    u, v = (None, None) if uniform else (rand_vector(rng, k), rand_vector(rng, k))
    runs = []
    for _ in range(2):
      with device.DeviceState(n, bw) as st:
        st.upload(psi)
        s = st.apply_rank1(reg, u=u, v=v, a=complex(0.1, 0.2), b=complex(1.5, -0.5), ctl_mask=ctl, sums=True)
        runs.append((st.download(), s))
    assert np.array_equal(runs[0][0], runs[1][0]) and runs[0][1] == runs[1][1]


@pytest.mark.parametrize('bw', [128, 64])
def test_projector_sums_agree_and_reflection_twice_restores(bw):
  rng = np.random.default_rng(50 + bw)
  n = 16
  with device.DeviceState(n, bw) as st:
    for k, uniform in ((4, False), (10, False), (12, False), (6, True), (16, True)):
      reg = [int(x) for x in rng.permutation(n)[:k]]
      v = None if uniform else rand_vector(rng, k)
      psi = rand_state(rng, n).astype(st.dtype)
      st.upload(psi)
      # a reflection twice: the identity, within twice the tolerance
      st.apply_rank1(reg, v=v)
      mid = st.download()
      st.apply_rank1(reg, v=v)
      back = st.download()
      tol = 2 * max(tolerance(psi, k, None, v, -1.0, 2.0, bw), tolerance(mid, k, None, v, -1.0, 2.0, bw))
      assert float(np.max(np.abs(back.astype(np.complex128) - psi.astype(np.complex128)))) <= tol
      # the projector |v><v|, v normalised: psi'[s, r] = v_s m_r, so sum |psi'|^2 = sum |m_r|^2 up to the rounding of each
      # component: relative 2 * 2^-24 at complex64, and (2^k + 16) 2^-52 at complex128 (the norm of v and the products)
      s0, s1 = st.apply_rank1(reg, v=v, a=0.0, b=1.0, sums=True)
      rel = 4 * 2.0 ** -24 if bw == 64 else ((1 << k) + 16) * 2.0 ** -52
      assert abs(s0 - s1) <= rel * s1 and 0 < s1 <= 1 + 1e-6


def test_golden_reflections_of_the_reference():
  """the reference's dense reflections (tools/make_golden_rank1.py).  Its operator is a product of three 2^n x 2^n matrices and
  is applied by a fourth product, each with the error bound of one 2^n-term inner product: 4 x the tolerance of one call."""
  g = np.load(rank1_util.GOLDEN)
  for n in (3, 5, 8):
    with device.DeviceState(n, 128) as st:
      for psi, want in zip(g[f'a{n}_in'], g[f'a{n}_out']):
        st.upload(psi)
        st.apply_rank1(list(range(n)))                   # the uniform form on every bit: inversion about the mean
        assert float(np.max(np.abs(st.download() - want))) <= 4 * tolerance(psi, n, None, None, -1.0, 2.0, 128)
  for n in (3, 6):
    phi = g[f'b{n}_phi']
    with device.DeviceState(n, 128) as st:
      for psi, want in zip(g[f'b{n}_in'], g[f'b{n}_out']):
        st.upload(psi)
        st.apply_rank1(list(range(n)), v=phi)
        assert float(np.max(np.abs(st.download() - want))) <= 4 * tolerance(psi, n, None, phi, -1.0, 2.0, 128)


def test_shard_handles():
  rng = np.random.default_rng(13)
  nl, n = 10, 12
  psi = rand_state(rng, n)
  reg = [3, 0, 7, 9, 1]
  u, v = rand_vector(rng, 5), rand_vector(rng, 5)
  a, b = complex(0.3, 0.1), complex(-0.9, 1.2)
  h_gate = np.asarray(gates.hadamard(), np.complex128)
  ctl = (1 << 10) | (1 << 5)
  want_all, m_all, met_all = rank1_parts(psi, n, reg, u, v, a, b, ctl)
  for s in range(4):
    with device.DeviceState(nl, 128, fusion=native.QH_FUSE_SWEEP) as st:
      st.set_shard(n, s)
      mine = psi[s << nl:(s + 1) << nl]
      st.upload(mine)
      st.sync()
      st.reset_stats()
      # a control on a shard bit: dropped where met, a counted no-op where not
      sums = st.apply_rank1(reg, u=u, v=v, a=a, b=b, ctl_mask=ctl, sums=True)
      want = want_all[s << nl:(s + 1) << nl]
      got = st.download()
      assert float(np.max(np.abs(got - want))) <= tolerance(psi, 5, u, v, a, b, 128)
      stats = st.stats()
      if s & 1:
        assert stats['gates_noop'] == 0 and stats['kernels_launched'] == 1 and not np.array_equal(got, mine)
        assert sums[0] > 0 and sums[1] > 0
      else:
        assert stats['gates_noop'] == 1 and stats['kernels_launched'] == 0 and np.array_equal(got, mine)
        assert sums == (0.0, 0.0)
      assert stats['gates_submitted'] == 1
      # a register bit on a shard bit: refused, the state and the pending queue as they were
      st.apply1(h_gate, n - 1 - 2)                       # (reference qubit numbers: logical bit 2) stays queued
      pending = ctypes.c_uint64()
      native.check(st.lib.qh_pending_gates(st.h, ctypes.byref(pending)))
      assert pending.value == 1
      with pytest.raises(native.QhError) as e:
        st.apply_rank1([3, 11, 7, 9, 1], u=u, v=v)
      assert e.value.code == native.QH_ERR_NONLOCAL
      native.check(st.lib.qh_pending_gates(st.h, ctypes.byref(pending)))
      assert pending.value == 1 and st.stats()['kernels_launched'] == stats['kernels_launched']
      native.check(st.lib.qh_discard_pending(st.h))
      assert np.array_equal(st.download(), got)


# (n, physical register positions, physical control positions, uniform, path, kernels, state sweeps)
_STATS = [
    (18, [4, 5, 6, 7, 8], [1, 12, 15], False, native.QH_RANK1_TILE, 1, 0.5),      # a quarter of the tiles, read and written
    (18, list(range(6, 18)), [2], False, native.QH_RANK1_TWO_PASS, 3, 3),         # one fibre group: the walk is split
    (18, list(range(18)), [], True, native.QH_RANK1_TWO_PASS, 3, 3),              # one fibre
    (22, list(range(11)), [15], False, native.QH_RANK1_TWO_PASS, 2, 3),           # 2^11 groups of one chunk: no split
]


@pytest.mark.parametrize('case', _STATS, ids=[f'n{c[0]}k{len(c[1])}' for c in _STATS])
def test_stats_equal_the_plan_on_both_paths(case):
  n, regp, ctlp, uniform, path, kernels, sweeps = case
  rng = np.random.default_rng(2)
  with device.DeviceState(n, 128, fusion=native.QH_FUSE_SWEEP) as st:
    st.init_basis(5)
    st.sync()
    bm = _bitmap(st, n)
    state_bytes = 16 << n
    reg, ctl = _at(bm, regp), sum(1 << x for x in _at(bm, ctlp))
    k = len(reg)
    plan = st.rank1_plan(reg, ctl, uniform=uniform)
    assert plan['path'] == path and plan['kernels'] == kernels and plan['bytes_swept'] == int(sweeps * state_bytes)
    assert (plan['split'] > 1) == (kernels == 3)
    assert plan['scratch_bytes'] == (0 if path == native.QH_RANK1_TILE else 16 * plan['nfibres'] * (1 + plan['split'] if plan['split'] > 1 else 1))
    s0 = st.stats()
    st.apply_rank1(reg, v=None if uniform else rand_vector(rng, k), ctl_mask=ctl, sums=bool(uniform))
    s1 = st.stats()
    assert s1['kernels_launched'] - s0['kernels_launched'] == plan['kernels']
    assert s1['gates_submitted'] - s0['gates_submitted'] == 1
    assert s1['bytes_swept'] - s0['bytes_swept'] == plan['bytes_swept']
    assert s1['bytes_algorithmic'] - s0['bytes_algorithmic'] == 2 * state_bytes >> len(ctlp)
    assert s1['sweeps'] == s0['sweeps'] and s1['gates_noop'] == s0['gates_noop']
    assert abs(st.norm2() - 1) < 1e-12                   # a reflection


def test_error_paths_leave_the_state_as_it_was():
  rng = np.random.default_rng(6)
  n = 12
  psi = rand_state(rng, n)
  one = np.array([1.0, 0.0])
  with device.DeviceState(n, 128) as st:
    st.upload(psi)
    lib, h = st.lib, st.h
    v3 = np.ascontiguousarray(rand_vector(rng, 3))
    bad = v3.copy()
    bad[5] = complex(1.0, np.inf)
    b3 = (ctypes.c_int32 * 3)(1, 4, 7)

    def call(k=3, bits=b3, ctl=0, u=None, v=v3, a=one, b=one):
      p = lambda t: None if t is None else t.ctypes.data_as(_dp)
      return lib.qh_apply_rank1(h, k, bits, ctl, p(u), p(v), p(a), p(b), None)
    assert call(bits=None) == native.QH_ERR_ARG
    assert call(a=None) == native.QH_ERR_ARG and call(b=None) == native.QH_ERR_ARG
    assert call(u=v3, v=None) == native.QH_ERR_ARG
    assert call(k=0) == native.QH_ERR_ARG and call(k=17, bits=(ctypes.c_int32 * 17)(*range(17))) == native.QH_ERR_ARG
    assert call(k=13, bits=(ctypes.c_int32 * 13)(*range(13)), v=None) == native.QH_ERR_ARG      # uniform: k above the local bits
    assert call(v=bad) == native.QH_ERR_ARG and b'v[5]' in lib.qh_last_error()
    assert call(u=bad) == native.QH_ERR_ARG and b'u[5]' in lib.qh_last_error()
    assert call(a=np.array([np.nan, 0.0])) == native.QH_ERR_ARG and b'a[0]' in lib.qh_last_error()
    assert call(b=np.array([0.0, -np.inf])) == native.QH_ERR_ARG and b'b[1]' in lib.qh_last_error()
    assert call(bits=(ctypes.c_int32 * 3)(1, 12, 7)) == native.QH_ERR_BAD_QUBIT
    assert call(ctl=1 << 12) == native.QH_ERR_BAD_QUBIT
    assert call(bits=(ctypes.c_int32 * 3)(1, 4, 1)) == native.QH_ERR_SAME_QUBIT
    assert call(ctl=1 << 4) == native.QH_ERR_SAME_QUBIT
    assert np.array_equal(st.download(), psi)
    assert call() == native.QH_OK
    assert not np.array_equal(st.download(), psi)


# ---- through qc ------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def width128():
  tensor.set_tensor_width(128)
  yield
  tensor.set_tensor_width(None)
  backend.drop_device_pool()


def test_grover_on_12_qubits_through_qc(width128):
  n, marked = 12, 0b101100111010
  q = circuit.qc('grover')
  q.reg(n, 0)
  for i in range(n):
    q.h(i)
  reg = list(range(n))
  table = np.zeros(1 << n, dtype=np.int64)
  table[marked] = 1
  theta = np.arcsin(2.0 ** (-n / 2.0))
  iters = int(np.pi / (4 * theta))
  bits = [(marked >> (n - 1 - i)) & 1 for i in range(n)]
  # per iteration every amplitude moves by at most the tolerance of one call (amax <= 1: B <= 3), the oracle is exact; a
  # probability |x|^2 with |x| <= 1 moves by at most 2 |dx| + |dx|^2
  dx = ((1 << n) + 8) * 2.0 ** -52 * 3.0
  for t in range(1, iters + 1):
    q.phase_oracle(table, reg)
    q.diffusion(reg)
    if t in (1, 7, iters):
      d = t * dx + n * 2.0 ** -52                                # (+ the Hadamard layer)
      assert abs(q.prob(*bits) - np.sin((2 * t + 1) * theta) ** 2) <= 2 * d + d * d
  assert q.prob(*bits) > 0.999
  q.close()


def test_reflect_and_project_onto_through_qc(width128):
  rng = np.random.default_rng(21)
  n, reg = 10, [7, 2, 5, 0]
  q = circuit.qc('reflect')
  q.reg(n, 0)
  for i in range(n):
    q.ry(i, float(rng.uniform(0.2, np.pi - 0.2)))
  q.cx(0, n - 1)
  before = np.asarray(q.psi).copy()
  phi = rand_vector(rng, 4) * 3.0                                  # normalised on the host
  q.reflect(reg, phi, ctl=[9])
  bits = [n - 1 - r for r in reversed(reg)]
  unit = phi / np.linalg.norm(phi)
  want = rank1_util.rank1_reference(before, n, bits, None, unit, -1.0, 2.0, 1 << (n - 1 - 9))
  assert float(np.max(np.abs(np.asarray(q.psi) - want))) <= tolerance(before, 4, None, unit, -1.0, 2.0, 128)
  p = q.project_onto(reg, phi)
  _, m, met = rank1_parts(want, n, bits, None, unit, 0.0, 1.0)
  first = (np.arange(1 << n) & sum(1 << x for x in bits)) == 0
  assert abs(p - float(np.sum(np.abs(m[first]) ** 2))) < 1e-12
  assert abs(float(np.vdot(np.asarray(q.psi), np.asarray(q.psi)).real) - 1) < 1e-12
  q.close()
