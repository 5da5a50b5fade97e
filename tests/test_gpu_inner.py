"""Two states on the MI355X: qh_inner against np.vdot of both states brought into logical order on the host, qh_clone and
qh_copy, per-shard semantics on one GPU, qc.snapshot / restore / overlap / fidelity end to end, and one 30-qubit overlap
with an answer that does not come from the new kernels.

qh_download re-lays a permuted state out, so the handles under test are downloaded LAST; what they held before a call is
read from clones taken before it.

About "inner == norm2 bitwise" for a clone: qh_norm2 adds its block sums with atomic adds, in whatever order the blocks
finish, so its own low bits differ between two runs on a state of more than one block (256 amplitudes) and no fixed-order
sum can equal it bitwise.  The norm the bitwise assertions use is the one qh_inner defines, inner(a, a): inner(a, clone)
must equal it bit for bit in re, both with im == 0.0 exactly; qh_norm2 is held to 1e-12 of it."""
import ctypes
import cmath

import numpy as np
import pytest

from qcc_amd import device, gates, native, workloads
from qcc_amd.lib import circuit, tensor
from tests import inner_util, shard_util

pytestmark = pytest.mark.gpu

TOL = 1e-12      # readers that accumulate in double from the stored amplitudes, normalised states, both widths


def _logical_state(st, shard=0, nglob=None):
  """(logical indices, amplitudes as complex128) of everything the handle holds, whatever layout the download leaves"""
  phys = st.download().astype(np.complex128)
  lo = shard_util.phys_to_logical(st, shard, np.arange(phys.size), nglob or st.nbits).astype(np.int64)
  return lo, phys


def _logical(st):
  lo, phys = _logical_state(st)
  out = np.empty_like(phys)
  out[lo] = phys
  return out


def _random_state(n, seed):
  rng = np.random.default_rng(seed)
  v = rng.normal(size=1 << n) + 1j * rng.normal(size=1 << n)
  return v / np.linalg.norm(v)


def _uploaded(n, bw, seed, swaps=(), fusion=native.QH_FUSE_OFF):
  st = device.DeviceState(n, bw, fusion=fusion)
  st.upload(_random_state(n, seed))
  for x, y in swaps:
    st.remap_swap(x, y)
  return st


def _fused(n, bw, seed, depth=12):
  st = device.DeviceState(n, bw, fusion=native.QH_FUSE_SWEEP)
  ops, g8 = workloads.supremacy_stream(n, depth, seed=seed).arrays()
  st.init_basis(0)
  st.run_stream(ops, g8)
  st.flush()
  return st


def _fused_permuted(n, bw, first_seed=0):
  """a fused run whose relayout sweeps left a permuted bit map (which circuits do depends on the planner: the first of
  six seeds that does; 16 qubits is the smallest size of this file at which the supremacy circuits get one)"""
  for seed in range(first_seed, first_seed + 6):
    st = _fused(n, bw, seed)
    if shard_util.bitmap(st) != list(range(n)):
      return st
    st.close()
  raise AssertionError(f'no supremacy-{n} circuit of seeds {first_seed}..{first_seed + 5} left a permuted bit map')


def _raw_inner(a, b):
  out = (ctypes.c_double * 2)()
  native.check(a.lib.qh_inner(a.h, b.h, out))
  return out[0], out[1]


def _check_pair(a, b, what):
  """every property the issue lists for one pair of handles; returns |gpu - numpy|"""
  with a.clone() as ca, b.clone() as cb:
    bma, bmb = shard_util.bitmap(a), shard_util.bitmap(b)
    na, nb = a.marginal([]).tobytes(), b.marginal([]).tobytes()
    ka, kb = a.stats()['kernels_launched'], b.stats()['kernels_launched']
    v1 = _raw_inner(a, b)
    assert a.stats()['kernels_launched'] - ka == 1 and b.stats()['kernels_launched'] - kb == 0, what
    v2 = _raw_inner(a, b)
    assert v1 == v2, (what, v1, v2)                                                  # bitwise reproducible
    w = _raw_inner(b, a)
    print(f'{what}: <a|b> = {v1[0]:+.16f} {v1[1]:+.16f}i, <b|a> - conj = {abs(complex(*w) - complex(*v1).conjugate()):.2e}')
    assert abs(complex(*w) - complex(*v1).conjugate()) < TOL, what
    # reads only: bit maps, norms (bitwise: same state, same layout) and amplitudes of both handles as before
    assert shard_util.bitmap(a) == bma and shard_util.bitmap(b) == bmb, what
    assert a.marginal([]).tobytes() == na and b.marginal([]).tobytes() == nb, what
    la, lb = _logical(a), _logical(b)
    assert la.tobytes() == _logical(ca).tobytes() and lb.tobytes() == _logical(cb).tobytes(), what
  want = complex(np.vdot(la, lb))
  err = abs(complex(*v1) - want)
  print(f'{what}: |gpu - numpy| = {err:.3e}')
  assert err < TOL, (what, v1, want)
  return err


# ---- 1. small registers -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('bw', [128, 64])
@pytest.mark.parametrize('nloc', [4, 7, 8, 9, 12, 16])
def test_inner_clone_takes_the_linear_path(nloc, bw):
  swaps = inner_util.hand_maps(nloc)[3][2]      # a permuted map on BOTH sides is still the same layout
  with _uploaded(nloc, bw, 10 + nloc, swaps) as a, a.clone() as c:
    assert a.inner_plan(c)['path'] == native.QH_INNER_LINEAR and a.inner_plan(a)['path'] == native.QH_INNER_LINEAR
    ka, kc = a.stats()['kernels_launched'], c.stats()['kernels_launched']
    self_re, self_im = _raw_inner(a, a)
    assert a.stats()['kernels_launched'] - ka == 1
    re, im = _raw_inner(a, c)
    assert a.stats()['kernels_launched'] - ka == 2 and c.stats()['kernels_launched'] == kc
    assert self_im == 0.0 and im == 0.0
    assert re == self_re                                     # bit for bit the shard's norm as qh_inner defines it
    assert _raw_inner(c, a) == (re, im)
    print(f'nloc={nloc} bw={bw}: inner(a, a) = {self_re!r}, qh_norm2 = {a.norm2()!r}, marginal = {a.marginal([])[0]!r}')
    assert abs(a.norm2() - self_re) < TOL and abs(a.marginal([])[0] - self_re) < TOL
    _check_pair(a, c, f'clone nloc={nloc} bw={bw}')


@pytest.mark.parametrize('bw', [128, 64])
@pytest.mark.parametrize('nloc', [1, 2, 3])
def test_inner_tiny_registers(nloc, bw):
  """below the issue's sizes: a complex64 state of one 16-byte load (two amplitudes per lane on the linear path), partial
  chunks, and the gather on two and three bits"""
  with _uploaded(nloc, bw, 50 + nloc) as a, _uploaded(nloc, bw, 60 + nloc) as b:
    assert a.inner_plan(b)['path'] == native.QH_INNER_LINEAR
    _check_pair(a, b, f'tiny linear nloc={nloc} bw={bw}')
    re, im = _raw_inner(a, a)
    assert im == 0.0 and abs(re - a.marginal([])[0]) < TOL
    if nloc > 1:
      b.remap_swap(0, nloc - 1)
      assert a.inner_plan(b)['path'] == native.QH_INNER_GATHER
      _check_pair(a, b, f'tiny gather nloc={nloc} bw={bw}')


@pytest.mark.parametrize('bw', [128, 64])
@pytest.mark.parametrize('nloc', [4, 7, 8, 9, 12, 16])
def test_inner_hand_made_maps(nloc, bw):
  paths = set()
  for k, (name, sa, sb) in enumerate(inner_util.hand_maps(nloc)):
    with _uploaded(nloc, bw, 100 + k, sa) as a, _uploaded(nloc, bw, 200 + k, sb) as b:
      paths.add(a.inner_plan(b)['path'])
      _check_pair(a, b, f'{name} nloc={nloc} bw={bw}')
  assert (native.QH_INNER_GATHER if nloc < 8 else native.QH_INNER_TILES) in paths


@pytest.mark.parametrize('bw', [128, 64])
def test_inner_layouts_left_by_fused_flushes(bw):
  differ = []
  for nloc in (8, 9, 12, 16):
    with _fused(nloc, bw, seed=0) as a, _fused(nloc, bw, seed=1) as b:
      differ.append(shard_util.bitmap(a) != shard_util.bitmap(b))
      if differ[-1]:
        assert a.inner_plan(b)['path'] == native.QH_INNER_TILES
      _check_pair(a, b, f'fused nloc={nloc} bw={bw} maps differ={differ[-1]}')
  assert any(differ), differ      # or the test shows nothing


# ---- 2. qh_clone ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('bw', [128, 64])
def test_clone_copies_state_and_bit_map(bw):
  n = 16
  with _fused_permuted(n, bw) as a:
    bm = shard_util.bitmap(a)                               # relayout sweeps left a permuted map (and swapped the two buffers)
    with a.clone() as c:
      assert shard_util.bitmap(c) == bm and shard_util.bitmap(a) == bm
      assert c.stats() == dict.fromkeys(c.stats(), 0)
      pend = ctypes.c_uint64(9)
      native.check(c.lib.qh_pending_gates(c.h, ctypes.byref(pend)))
      assert pend.value == 0
      with c.clone() as ref:                                # (what a and c hold now, for the comparisons below)
        want = _logical(ref)
      # gates on the clone leave the source alone, and the other way round
      c.apply1(gates.hadamard(), 2)
      c.applyc(gates.pauli_x(), 0, n - 1)
      c.flush()
      with a.clone() as a2:
        assert _logical(a2).tobytes() == want.tobytes()
      with c.clone() as c2:
        moved = _logical(c2)
      assert moved.tobytes() != want.tobytes()
      a.apply1(gates.hadamard(), 5)
      a.flush()
      with c.clone() as c3:
        assert _logical(c3).tobytes() == moved.tobytes()
      assert _logical(a).tobytes() != want.tobytes()


def test_clone_runs_queued_gates_and_outlives_its_source():
  n = 10
  a = device.DeviceState(n, 128, fusion=native.QH_FUSE_SWEEP)
  a.init_basis(0)
  for q in range(n):
    a.apply1(gates.hadamard(), q)
  pend = ctypes.c_uint64()
  native.check(a.lib.qh_pending_gates(a.h, ctypes.byref(pend)))
  assert pend.value == n                                    # still queued when the clone is taken
  c = a.clone()
  native.check(a.lib.qh_pending_gates(a.h, ctypes.byref(pend)))
  assert pend.value == 0
  a.close()
  assert np.allclose(_logical(c), np.full(1 << n, 2.0 ** (-n / 2)), atol=1e-15)
  c.apply1(gates.hadamard(), 0)                             # the clone is a full handle: same fusion level, its own stream
  assert abs(c.prob_bit(n - 1, 1)) < 1e-15 and abs(c.inner(c) - 1.0) < TOL
  c.close()


@pytest.mark.parametrize('bw', [128, 64])
def test_clone_of_a_host_mapped_state_lives_in_hbm(bw):
  n = 9
  with device.DeviceState(n, bw, host_mapped=True) as a:
    a.upload(_random_state(n, 77))
    a.apply1(gates.hadamard(), 3)
    with a.clone() as c:
      p = ctypes.c_void_p(1)
      native.check(c.lib.qh_host_ptr(c.h, ctypes.byref(p)))
      assert not p.value
      native.check(a.lib.qh_host_ptr(a.h, ctypes.byref(p)))
      assert p.value                                        # the source is where it was
      a.sync()
      assert _logical(c).tobytes() == np.asarray(a.host_array()).astype(np.complex128).tobytes()
      _check_pair(a, c, f'host-mapped bw={bw}')


# ---- 3. qh_copy -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('bw', [128, 64])
def test_copy_restores_a_snapshot(bw):
  n = 16
  with _fused_permuted(n, bw) as a, a.clone() as snap:
    with snap.clone() as ref:
      want = _logical(ref)
    bm_snap = shard_util.bitmap(snap)
    ops, g8 = workloads.supremacy_stream(n, 6, seed=9).arrays()
    a.run_stream(ops, g8)
    a.flush()                                               # further gates: another state, most likely another layout
    a.apply1(gates.hadamard(), 1)                           # ... and one gate still queued: dropped by the restore, never run
    pend = ctypes.c_uint64()
    native.check(a.lib.qh_pending_gates(a.h, ctypes.byref(pend)))
    assert pend.value == 1
    a.copy_from(snap)
    native.check(a.lib.qh_pending_gates(a.h, ctypes.byref(pend)))
    assert pend.value == 0
    assert shard_util.bitmap(a) == bm_snap
    assert a.inner(snap) == snap.inner(snap)                # same layout, same amplitudes
    assert _logical(a).tobytes() == want.tobytes()
    a.apply1(gates.hadamard(), 0)                           # usable at once
    a.apply1(gates.hadamard(), 0)
    assert abs(a.inner(snap) - snap.inner(snap)) < 1e-6 if bw == 64 else abs(a.inner(snap) - snap.inner(snap)) < TOL


def test_copy_into_attached_memory_keeps_the_pointer():
  n = 16
  with device.DeviceState(n, 128) as owner, _fused_permuted(n, 128) as src:
    ptr = owner.device_ptr
    owner.init_basis(5)
    owner.sync()
    with device.DeviceState(n, 128, device_ptr=ptr, fusion=native.QH_FUSE_SWEEP) as att:
      assert abs(att.prob_bit(0, 1) - 1.0) < 1e-15 and abs(att.prob_bit(1, 1)) < 1e-15      # the attached handle sees |5>
      att.apply1(gates.hadamard(), 4)
      with src.clone() as ref:
        want = _logical(ref)
      att.copy_from(src)
      assert shard_util.bitmap(att) == shard_util.bitmap(src)
      assert att.inner(src) == src.inner(src)
      assert att.device_ptr == ptr                          # (brings att back to canonical order, inside the caller's memory)
      att.sync()
      assert owner.download().astype(np.complex128).tobytes() == want.tobytes()


def test_copy_argument_errors_change_nothing():
  lib = native.load()
  with _uploaded(8, 128, 1, [(0, 5)]) as a, _uploaded(9, 128, 2) as n9, _uploaded(8, 64, 3) as w64, _uploaded(8, 128, 4) as sh, \
       _uploaded(8, 128, 5) as sh1:
    sh.set_shard(10, 2)
    sh1.set_shard(10, 1)
    bm = shard_util.bitmap(a)
    with a.clone() as ref:
      want = _logical(ref)
    for dst, src in ((a, a), (a, n9), (n9, a), (a, w64), (a, sh), (sh, a), (sh, sh1), (sh1, sh)):
      assert lib.qh_copy(dst.h, src.h) == native.QH_ERR_ARG
    assert lib.qh_copy(a.h, None) == native.QH_ERR_ARG and lib.qh_copy(None, a.h) == native.QH_ERR_ARG
    out = (ctypes.c_double * 2)(7.0, 7.0)
    for x, y in ((a, n9), (a, w64)):
      assert lib.qh_inner(x.h, y.h, out) == native.QH_ERR_ARG
    assert lib.qh_inner(a.h, sh.h, out) == native.QH_ERR_ARG       # (another nbits_global)
    assert lib.qh_inner(sh.h, sh1.h, out) == native.QH_ERR_NONLOCAL    # another shard of the same register
    assert list(out) == [7.0, 7.0]
    assert shard_util.bitmap(a) == bm and _logical(a).tobytes() == want.tobytes()


# ---- 4. shards on one GPU ---------------------------------------------------------------------------------------------------------
def test_shard_inners_sum_to_the_full_overlap():
  nloc, nglob = 10, 12
  va, vb = _random_state(nglob, 41), _random_state(nglob, 42)
  total = 0j
  la, lb = np.zeros(1 << nglob, dtype=np.complex128), np.zeros(1 << nglob, dtype=np.complex128)
  for s in range(4):
    with device.DeviceState(nloc, 128) as a, device.DeviceState(nloc, 128) as b:
      for st, v in ((a, va), (b, vb)):
        st.set_shard(nglob, s)
        st.upload(v[s << nloc:(s + 1) << nloc])
      b.remap_swap(2, 7)                                    # local bits anywhere, on one side
      b.remap_swap(0, 9)
      assert a.inner_plan(b)['path'] == native.QH_INNER_TILES
      total += a.inner(b)
      out = (ctypes.c_double * 2)(7.0, 7.0)
      with b.clone() as c:
        c.remap_swap(3, 11)                                 # c now holds another logical bit in the shard index
        ka = a.stats()['kernels_launched']
        assert a.lib.qh_inner(a.h, c.h, out) == native.QH_ERR_NONLOCAL
        assert b'exchange first' in a.lib.qh_last_error()
        assert a.lib.qh_inner(c.h, a.h, out) == native.QH_ERR_NONLOCAL
        assert list(out) == [7.0, 7.0] and a.stats()['kernels_launched'] == ka
      for st, full in ((a, la), (b, lb)):
        lo, phys = _logical_state(st, s, nglob)
        full[lo] = phys
  want = complex(np.vdot(la, lb))
  print(f'4 shards of 10 of 12: |sum of qh_inner - vdot| = {abs(total - want):.3e}')
  assert abs(total - want) < TOL


# ---- 5. qc ------------------------------------------------------------------------------------------------------------------------
def _layers(q, nq, seed, depth):
  rng = np.random.default_rng(seed)
  for _ in range(depth):
    for i in range(nq):
      q.ry(i, float(rng.uniform(0, 3)))
    for i in range(nq - 1):
      q.cu1(i, i + 1, float(rng.uniform(0, 3)))
    q.cx(int(rng.integers(1, nq)), 0)


@pytest.fixture
def width128():
  tensor.set_tensor_width(128)
  yield
  tensor.set_tensor_width(None)


@pytest.mark.parametrize('nq,alias', [(10, True), (22, False)])
def test_qc_overlap_and_fidelity(width128, nq, alias):
  a, b = circuit.qc('a', alias_psi=alias), circuit.qc('b', alias_psi=alias)
  for q, seed in ((a, 1), (b, 2)):
    q.reg(nq, 0)
    _layers(q, nq, seed, 2)
  ov, fid, self_ov = a.overlap(b), a.fidelity(b), a.overlap(a)
  pa, pb = np.array(a.psi, dtype=np.complex128).reshape(-1), np.array(b.psi, dtype=np.complex128).reshape(-1)
  want = complex(np.vdot(pa, pb))
  print(f'qc {nq} qubits alias={alias}: |overlap - vdot| = {abs(ov - want):.3e}, fidelity {fid:.15f}')
  assert abs(ov - want) < TOL and abs(self_ov - 1.0) < TOL and self_ov.imag == 0.0
  assert abs(fid - abs(want) ** 2 / (np.vdot(pa, pa).real * np.vdot(pb, pb).real)) < TOL
  assert abs(b.overlap(a) - np.conj(want)) < TOL
  with pytest.raises(ValueError):
    c = circuit.qc('c')
    c.reg(nq - 1, 0)
    a.overlap(c)
  with pytest.raises(ValueError):
    a.overlap(pb)
  for q in (a, b):
    q.close()


@pytest.mark.parametrize('nq,alias', [(10, True), (14, False)])
def test_qc_snapshot_measure_restore(width128, nq, alias):
  q = circuit.qc('m', alias_psi=alias)
  q.reg(nq, 0)
  _layers(q, nq, 7, 2)
  regs = [[0, 1, 2], list(range(nq - 4, nq)), [5, 2, 8]]
  before = [q.probabilities(r) for r in regs]
  with q.snapshot() as snap:
    assert snap.nbits == nq and snap.width == 128
    if alias:
      assert type(snap._dev).__name__ == 'DeviceState'
      p = ctypes.c_void_p(1)
      native.check(snap._dev.lib.qh_host_ptr(snap._dev.h, ctypes.byref(p)))
      assert not p.value                                    # the copy of a host-mapped register lives in HBM
    value, prob = q.measure([1, 4, 6], seed=3, collapse=True)
    assert 0 < prob < 1
    assert abs(q.probabilities([1, 4, 6])[value] - 1.0) < 1e-12
    q.x(0)                                                  # queued when the snapshot comes back: dropped
    q.restore(snap)
    after = [q.probabilities(r) for r in regs]
    for x, y in zip(before, after):
      assert x.tobytes() == y.tobytes()                     # the very amplitudes in the very layout
    assert abs(q.overlap(snap) - 1.0) < TOL and abs(q.fidelity(snap) - 1.0) < TOL
    # what follows the snapshot, then its inverse: back at the snapshot
    sub = q.sub()
    _layers(sub, nq, 8, 2)
    q.qc(sub)
    assert abs(q.overlap(snap)) < 1.0 - 1e-3
    q.qc(sub.inverse())
    ov = q.overlap(snap)
    print(f'qc {nq} qubits alias={alias}: |<q|snapshot> - 1| after circuit + inverse = {abs(ov - 1.0):.3e}')
    assert abs(ov - 1.0) < TOL
    with pytest.raises(ValueError):
      small = circuit.qc('s')
      small.reg(nq - 1, 0)
      small.restore(snap)
  with pytest.raises(ValueError):
    q.overlap(snap)                                         # closed
  q.close()


# ---- 6. full size -------------------------------------------------------------------------------------------------------------------
def _adjoint_stream(ops, g8):
  """the inverse of a gate stream: reverse order, every 2x2 [a b c d] -> [a* c* b* d*]"""
  g = np.asarray(g8, dtype=np.float64).reshape(-1, 4, 2)[::-1]
  adj = g[:, [0, 2, 1, 3], :] * np.array([1.0, -1.0])
  return np.ascontiguousarray(np.asarray(ops)[::-1]), np.ascontiguousarray(adj.reshape(-1, 8))


def test_supremacy30_overlap_with_a_phase_rotated_clone():
  """<a|b> for b = u1(theta) on one qubit of a: p0 + e^{i theta} p1, with p0 and p1 from qh_prob_bit.  First on the layout
  the clone shares with a (after the u1 flush), then again after a fused block and its inverse have re-laid b out: the
  block is supremacy-30 depth 8 seed 1, run and flushed, then its adjoint stream, run and flushed."""
  n, theta, qubit = 30, 0.7366, 11
  bit = n - 1 - qubit
  ops, g8 = workloads.supremacy_stream(n, 20, seed=0).arrays()
  with device.DeviceState(n, 128, fusion=native.QH_FUSE_SWEEP) as a:
    a.init_basis(0)
    a.run_stream(ops, g8)
    a.flush()
    bm_a = shard_util.bitmap(a)
    assert bm_a != list(range(n))                           # a permuted layout
    p0, p1 = a.prob_bit(bit, 0), a.prob_bit(bit, 1)
    want = p0 + cmath.exp(1j * theta) * p1
    with a.clone() as b:
      b.apply1(gates.u1(theta), qubit)
      b.flush()
      first_path = a.inner_plan(b)['path']
      ov1 = a.inner(b)
      print(f'supremacy-30: path {first_path}, <a|b> = {ov1:.15f}, p0 + e^(i theta) p1 = {want:.15f}, |diff| = {abs(ov1 - want):.3e}')
      assert abs(ov1 - want) < 1e-10
      ops2, g82 = workloads.supremacy_stream(n, 8, seed=1).arrays()
      b.run_stream(ops2, g82)
      b.flush()
      b.run_stream(*_adjoint_stream(ops2, g82))
      b.flush()
      assert shard_util.bitmap(b) != bm_a and shard_util.bitmap(a) == bm_a
      assert a.inner_plan(b)['path'] == native.QH_INNER_TILES
      ka, kb = a.stats()['kernels_launched'], b.stats()['kernels_launched']
      ov2 = a.inner(b)
      assert a.stats()['kernels_launched'] - ka == 1 and b.stats()['kernels_launched'] == kb
      print(f'supremacy-30, b re-laid out: <a|b> = {ov2:.15f}, |diff| = {abs(ov2 - want):.3e}')
      assert abs(ov2 - want) < 1e-10
      assert abs(b.inner(a) - ov2.conjugate()) < 1e-10
      assert a.inner(b) == ov2
