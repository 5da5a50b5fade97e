"""Linear combinations of two states on the MI355X: qh_axpby (dst := alpha * dst + beta * src by LOGICAL index, written in
place in dst's layout) against NumPy on both states brought into logical order on the host, on every path of
qh_inner_plan(dst, src); the exact cases; the contract (what stays as it was, stats, the norm, queued gates); layouts left by
fused flushes; per-shard semantics on one GPU; blocks that walk more than one chunk, checked with the readers that were there
before; qc.combine / qc.project_out end to end.

qh_download re-lays a permuted state out, so the handles under test are downloaded LAST; what they held before a call is read
from clones taken before it."""
import ctypes

import numpy as np
import pytest

from qcc_amd import device, gates, native, workloads
from qcc_amd.lib import circuit, tensor
from tests import inner_util, shard_util

pytestmark = pytest.mark.gpu

TOL = 1e-12            # complex128: double arithmetic on normalised states, coefficients of order 1
EPS32 = 2.0 ** -23     # complex64: one rounding of a double result to float, per component, relative to the largest |want|
PATHS = {native.QH_INNER_LINEAR: 'linear', native.QH_INNER_TILES: 'tiles', native.QH_INNER_GATHER: 'gather'}
ALPHA, BETA = 0.8 - 0.3j, -0.4 + 0.5j


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


def _before(st):
  """what the handle holds, in logical order, without touching its layout"""
  with st.clone() as c:
    return _logical(c)


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


def _raw(dst, alpha, src, beta, norm=True):
  """qh_axpby through the C-ABI: the norm (or None)"""
  a, b = complex(alpha), complex(beta)
  out = ctypes.c_double(-1.0)
  native.check(dst.lib.qh_axpby(dst.h, (ctypes.c_double * 2)(a.real, a.imag), src.h, (ctypes.c_double * 2)(b.real, b.imag),
                                ctypes.byref(out) if norm else None))
  return out.value if norm else None


def _assert_close(got, want, bw, what):
  """all amplitudes: complex128 max |got - want| <= 1e-12; complex64 per component <= 2^-23 * max |want|"""
  if bw == 128:
    err, bound = float(np.max(np.abs(got - want))), TOL
  else:
    err = float(max(np.max(np.abs(got.real - want.real)), np.max(np.abs(got.imag - want.imag))))
    bound = EPS32 * float(np.max(np.abs(want)))
  print(f'{what}: error {err:.3e} (bound {bound:.3e})')
  assert err <= bound, (what, err, bound)


def _check_general(d, s, bw, what, alpha=ALPHA, beta=BETA):
  """dst := alpha dst + beta src on the handles as they lie: all amplitudes against NumPy, and what must stay as it was"""
  path = d.inner_plan(s)['path']
  dl, sl = _before(d), _before(s)
  bmd, bms = shard_util.bitmap(d), shard_util.bitmap(s)
  ms = s.marginal([]).tobytes()
  kd, ks = d.stats(), s.stats()
  n2 = _raw(d, alpha, s, beta)
  kd2, ks2 = d.stats(), s.stats()
  state_bytes = (1 << d.nbits) * (16 if bw == 128 else 8)
  assert kd2['kernels_launched'] - kd['kernels_launched'] == 1 and ks2 == ks, what
  assert kd2['bytes_swept'] - kd['bytes_swept'] == 3 * state_bytes, what
  assert kd2['bytes_algorithmic'] - kd['bytes_algorithmic'] == 3 * state_bytes, what
  assert shard_util.bitmap(d) == bmd and shard_util.bitmap(s) == bms, what
  assert d.inner_plan(s)['path'] == path, what
  assert s.marginal([]).tobytes() == ms, what
  self_norm = d.inner(d).real
  assert abs(n2 - self_norm) <= TOL, (what, n2, self_norm)
  assert _before(s).tobytes() == sl.tobytes(), what                  # src is read only
  got = _logical(d)
  assert shard_util.bitmap(s) == bms
  _assert_close(got, alpha * dl + beta * sl, bw, f'{what} [{PATHS[path]}]')
  return path


# ---- 1. paths at the smallest sizes ----------------------------------------------------------------------------------------
@pytest.mark.parametrize('bw', [128, 64])
@pytest.mark.parametrize('nloc', [1, 2, 3])
def test_axpby_tiny_registers(nloc, bw):
  """a complex64 state of one 16-byte item, partial chunks, and the gather on two and three bits"""
  with _uploaded(nloc, bw, 50 + nloc) as d, _uploaded(nloc, bw, 60 + nloc) as s:
    assert _check_general(d, s, bw, f'tiny nloc={nloc} bw={bw}') == native.QH_INNER_LINEAR
    if nloc > 1:
      s.remap_swap(0, nloc - 1)
      assert _check_general(d, s, bw, f'tiny nloc={nloc} bw={bw}') == native.QH_INNER_GATHER


@pytest.mark.parametrize('bw', [128, 64])
@pytest.mark.parametrize('nloc', [4, 7, 8, 9, 12, 16])
def test_axpby_hand_made_maps(nloc, bw):
  """every pair of inner_util.hand_maps, each way round (on the smallest registers some swaps fall away and leave equal
  layouts: those pairs take the linear path)"""
  want = native.QH_INNER_GATHER if nloc < 8 else native.QH_INNER_TILES
  paths = []
  for k, (name, sa, sb) in enumerate(inner_util.hand_maps(nloc)):
    same = inner_util.apply_swaps(range(nloc), sa) == inner_util.apply_swaps(range(nloc), sb)
    with _uploaded(nloc, bw, 100 + k, sa) as d, _uploaded(nloc, bw, 200 + k, sb) as s:
      paths.append(_check_general(d, s, bw, f'{name} nloc={nloc} bw={bw}'))
      assert paths[-1] == (native.QH_INNER_LINEAR if same else want)
    with _uploaded(nloc, bw, 300 + k, sb) as d, _uploaded(nloc, bw, 400 + k, sa) as s:      # the pair the other way round
      assert _check_general(d, s, bw, f'{name} reversed nloc={nloc} bw={bw}') == paths[-1]
  assert want in paths


@pytest.mark.parametrize('bw', [128, 64])
@pytest.mark.parametrize('nloc', [4, 7, 8, 9, 12, 16])
def test_axpby_same_layout_takes_the_linear_path(nloc, bw):
  swaps = inner_util.hand_maps(nloc)[3][2]      # a permuted map on BOTH sides is still the same layout
  with _uploaded(nloc, bw, 10 + nloc, swaps) as d, d.clone() as s:
    s.apply1(gates.hadamard(), 0)               # (per-gate kernels keep the layout)
    s.applyc(gates.pauli_x(), 0, nloc - 1)
    s.flush()
    assert _check_general(d, s, bw, f'clone nloc={nloc} bw={bw}') == native.QH_INNER_LINEAR


# ---- 2. exact cases on every path --------------------------------------------------------------------------------------------
def _pair_on_path(path, bw, seed):
  """(dst, src) of the smallest sizes that take `path` with more than one block or a partial chunk where there is one"""
  if path == native.QH_INNER_GATHER:
    nloc, sb = 5, inner_util.hand_maps(5)[3][2]
  elif path == native.QH_INNER_TILES:
    nloc, sb = 9, inner_util.hand_maps(9)[3][2]
  else:
    nloc, sb = 9, []
  d, s = _uploaded(nloc, bw, seed), _uploaded(nloc, bw, seed + 1, sb)
  assert d.inner_plan(s)['path'] == path
  return d, s


@pytest.mark.parametrize('bw', [128, 64])
@pytest.mark.parametrize('path', sorted(PATHS), ids=[PATHS[p] for p in sorted(PATHS)])
def test_axpby_exact_cases(path, bw):
  dt = np.complex128 if bw == 128 else np.complex64
  state_bytes = lambda st: (1 << st.nbits) * (16 if bw == 128 else 8)
  # alpha = 0, beta = 1 into a dst full of NaN: src by logical index, nothing of dst read
  d, s = _pair_on_path(path, bw, 1)
  with d, s:
    d.upload(np.full(1 << d.nbits, np.nan + 1j * np.nan))
    sl = _before(s)
    b0 = d.stats()['bytes_swept']
    n2 = _raw(d, 0.0, s, 1.0)
    assert d.stats()['bytes_swept'] - b0 == 2 * state_bytes(d)
    assert abs(n2 - s.inner(s).real) <= TOL
    assert np.array_equal(_logical(d), sl)
  # alpha = 1, beta = +-1: NumPy's d +- s at the handle's width
  for beta in (1.0, -1.0):
    d, s = _pair_on_path(path, bw, 3)
    with d, s:
      dl, sl = _before(d).astype(dt), _before(s).astype(dt)
      _raw(d, 1.0, s, beta, norm=False)
      want = (dl + sl if beta > 0 else dl - sl).astype(np.complex128)
      assert np.array_equal(_logical(d), want), (PATHS[path], bw, beta)
  # alpha = 1, beta = 0: nothing runs; the norm is still returned
  d, s = _pair_on_path(path, bw, 5)
  with d, s:
    dl = _before(d)
    st0 = d.stats()
    n2 = _raw(d, 1.0, s, 0.0)
    assert _raw(d, 1.0, s, 0.0, norm=False) is None
    assert d.stats() == st0
    assert abs(n2 - d.inner(d).real) <= TOL and n2 == _raw(d, 1.0, s, 0.0)
    assert _logical(d).tobytes() == dl.tobytes()
  # beta = 0: dst scaled, src not read (two streams); alpha = beta = 0: zeros (one stream)
  d, s = _pair_on_path(path, bw, 7)
  with d, s:
    dl = _before(d)
    k0 = d.stats()
    n2 = _raw(d, -1.0, s, 0.0)
    k1 = d.stats()
    assert k1['kernels_launched'] - k0['kernels_launched'] == 1 and k1['bytes_swept'] - k0['bytes_swept'] == 2 * state_bytes(d)
    assert abs(n2 - d.inner(d).real) <= TOL
    with d.clone() as c:
      assert np.array_equal(_logical(c), -dl)
    d.upload(np.full(1 << d.nbits, np.nan + 1j * np.nan))
    k1 = d.stats()
    n2 = _raw(d, 0.0, s, 0.0)
    k2 = d.stats()
    assert k2['kernels_launched'] - k1['kernels_launched'] == 1 and k2['bytes_swept'] - k1['bytes_swept'] == state_bytes(d)
    assert n2 == 0.0
    assert np.array_equal(_logical(d), np.zeros(1 << d.nbits))


# ---- 3. contract ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('bw', [128, 64])
@pytest.mark.parametrize('path', sorted(PATHS), ids=[PATHS[p] for p in sorted(PATHS)])
def test_axpby_norm_is_reproducible(path, bw):
  """the same states, layouts and coefficients give the same bits (two runs from clones), and the norm is the one the
  readers give for the result (the rest of the contract is asserted on every pair of section 1: _check_general)"""
  d, s = _pair_on_path(path, bw, 11)
  with d, s, d.clone() as d2:
    # (qh_device_ptr itself brings a handle to canonical order and ends its relayout: asked of a dst that is in canonical
    # order and owns no second buffer, where that changes nothing; _check_general leaves it alone)
    ptr, bm = d.device_ptr, shard_util.bitmap(d)
    n_a, n_b = _raw(d, ALPHA, s, BETA), _raw(d2, ALPHA, s, BETA)
    assert n_a == n_b, (n_a, n_b)
    assert shard_util.bitmap(d) == bm and d.device_ptr == ptr
    assert abs(n_a - d.inner(d).real) <= TOL
    assert _raw(d, 1.0, s, 0.0) == d.inner(d).real                     # the identity case: the readers' own sum
    assert d.inner(d2) == d.inner(d)                                    # bitwise the same amplitudes in the same layout


@pytest.mark.parametrize('bw', [128, 64])
def test_axpby_on_attached_and_host_mapped_memory_keeps_the_pointer(bw):
  n = 9
  with device.DeviceState(n, bw) as owner, _uploaded(n, bw, 21, inner_util.hand_maps(n)[0][2]) as s:
    ptr = owner.device_ptr
    owner.upload(_random_state(n, 22))
    owner.sync()
    with device.DeviceState(n, bw, device_ptr=ptr) as att:
      dl, sl = _before(att), _before(s)
      _raw(att, ALPHA, s, BETA)
      assert att.device_ptr == ptr
      _assert_close(_logical(att), ALPHA * dl + BETA * sl, bw, f'attached bw={bw}')
  with device.DeviceState(n, bw, host_mapped=True) as hm, _uploaded(n, bw, 23, inner_util.hand_maps(n)[3][2]) as s:
    hm.upload(_random_state(n, 24))
    dl, sl = _before(hm), _before(s)
    _raw(hm, ALPHA, s, BETA)
    hm.sync()
    p = ctypes.c_void_p()
    native.check(hm.lib.qh_host_ptr(hm.h, ctypes.byref(p)))
    assert p.value
    _assert_close(np.asarray(hm.host_array()).astype(np.complex128).reshape(-1), ALPHA * dl + BETA * sl, bw, f'host-mapped bw={bw}')


@pytest.mark.parametrize('bw', [128, 64])
def test_axpby_runs_what_dst_and_src_have_queued(bw):
  n = 12
  with _uploaded(n, bw, 31, fusion=native.QH_FUSE_SWEEP) as d, _uploaded(n, bw, 32, fusion=native.QH_FUSE_SWEEP) as s:
    dl, sl = _before(d), _before(s)
    d.apply1(gates.hadamard(), 3)            # reference qubit 3 = logical bit n - 1 - 3
    s.apply1(gates.hadamard(), 0)
    pend = ctypes.c_uint64()
    for st in (d, s):
      native.check(st.lib.qh_pending_gates(st.h, ctypes.byref(pend)))
      assert pend.value == 1                 # still queued when the call comes
    _raw(d, ALPHA, s, BETA)
    for st in (d, s):
      native.check(st.lib.qh_pending_gates(st.h, ctypes.byref(pend)))
      assert pend.value == 0

    def had(v, q):
      t = v.reshape(1 << q, 2, -1)
      return np.stack([t[:, 0] + t[:, 1], t[:, 0] - t[:, 1]], axis=1).reshape(-1) / np.sqrt(2.0)
    want = ALPHA * had(dl, 3) + BETA * had(sl, 0)
    got = _logical(d)
    # the gate itself rounds once more at complex64 (and a few ulps at complex128)
    if bw == 128:
      assert np.max(np.abs(got - want)) <= TOL
    else:
      assert max(np.max(np.abs(got.real - want.real)), np.max(np.abs(got.imag - want.imag))) <= 3 * EPS32 * np.max(np.abs(want))


def test_axpby_argument_errors_change_nothing():
  lib = native.load()
  one = (ctypes.c_double * 2)(1.0, 0.0)
  with _uploaded(8, 128, 1, [(0, 5)]) as a, _uploaded(9, 128, 2) as n9, _uploaded(8, 64, 3) as w64, _uploaded(8, 128, 4) as b:
    want, bm, st0 = _before(a), shard_util.bitmap(a), a.stats()
    n2 = ctypes.c_double(7.0)
    for dst, src in ((a, a), (a, n9), (n9, a), (a, w64), (w64, a)):
      assert lib.qh_axpby(dst.h, one, src.h, one, ctypes.byref(n2)) == native.QH_ERR_ARG
    assert lib.qh_axpby(a.h, one, a.h, one, None) == native.QH_ERR_ARG and b'qh_scale' in lib.qh_last_error()
    assert lib.qh_axpby(a.h, None, b.h, one, None) == native.QH_ERR_ARG
    assert lib.qh_axpby(a.h, one, b.h, None, None) == native.QH_ERR_ARG
    assert lib.qh_axpby(None, one, b.h, one, None) == native.QH_ERR_ARG
    assert lib.qh_axpby(a.h, one, None, one, None) == native.QH_ERR_ARG
    assert n2.value == 7.0 and a.stats() == st0
    assert shard_util.bitmap(a) == bm and _logical(a).tobytes() == want.tobytes()


# ---- 4. layouts left by fused flushes ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('bw', [128, 64])
def test_axpby_layouts_left_by_fused_flushes(bw):
  """dst and src from supremacy-16 runs of different seeds whose relayout sweeps left permuted, different bit maps (which
  circuits do depends on the planner: the first seeds that do)"""
  n = 16
  d = s = None
  for seed in range(6):
    d = _fused(n, bw, seed)
    if shard_util.bitmap(d) != list(range(n)):
      break
    d.close()
    d = None
  assert d is not None, 'no supremacy-16 circuit of seeds 0..5 left a permuted bit map'
  with d:
    for seed2 in range(seed + 1, seed + 7):
      s = _fused(n, bw, seed2)
      if shard_util.bitmap(s) not in (list(range(n)), shard_util.bitmap(d)):
        break
      s.close()
      s = None
    assert s is not None, 'no second supremacy-16 circuit left another permuted bit map'
    with s:
      assert _check_general(d, s, bw, f'fused-16 seeds {seed},{seed2} bw={bw}') == native.QH_INNER_TILES


# ---- 5. shards on one GPU -----------------------------------------------------------------------------------------------------------
def test_axpby_shard_semantics():
  nloc, nglob, shard = 10, 12, 2
  va, vb = _random_state(nglob, 41), _random_state(nglob, 42)
  one = (ctypes.c_double * 2)(1.0, 0.0)

  def full(st, sh):
    lo, phys = _logical_state(st, sh, nglob)
    out = np.zeros(1 << nglob, dtype=np.complex128)
    out[lo] = phys
    return out

  with device.DeviceState(nloc, 128) as d, device.DeviceState(nloc, 128) as s:
    for st, v in ((d, va), (s, vb)):
      st.set_shard(nglob, shard)
      st.upload(v[shard << nloc:(shard + 1) << nloc])
    s.remap_swap(2, 7)                                      # local bits anywhere, on one side
    s.remap_swap(0, 9)
    assert d.inner_plan(s)['path'] == native.QH_INNER_TILES
    with d.clone() as c, s.clone() as c2:
      dl, sl = full(c, shard), full(c2, shard)
    n2 = _raw(d, ALPHA, s, BETA)
    assert abs(n2 - d.inner(d).real) <= TOL
    with d.clone() as c:
      got = full(c, shard)
    assert np.max(np.abs(got - (ALPHA * dl + BETA * sl))) <= TOL
    # another shard index, or a shard bit held differently: refused, dst bitwise as before
    bm, st0 = shard_util.bitmap(d, nglob), d.stats()
    with s.clone() as other_shard, s.clone() as other_bit:
      other_shard.set_shard(nglob, 1)
      other_bit.remap_swap(3, 11)                           # now holds another logical bit in the shard index
      out = ctypes.c_double(7.0)
      for src in (other_shard, other_bit):
        assert d.lib.qh_axpby(d.h, one, src.h, one, ctypes.byref(out)) == native.QH_ERR_NONLOCAL
        assert b'exchange first' in d.lib.qh_last_error()
        assert src.lib.qh_axpby(src.h, one, d.h, one, ctypes.byref(out)) == native.QH_ERR_NONLOCAL
      assert out.value == 7.0 and d.stats() == st0 and shard_util.bitmap(d, nglob) == bm
    assert full(d, shard).tobytes() == got.tobytes()


# ---- 6. blocks that walk more than one chunk ---------------------------------------------------------------------------------------------
def _amp(st, index):
  out = (ctypes.c_double * 2)()
  native.check(st.lib.qh_amplitude(st.h, int(index), out))
  return complex(out[0], out[1])


def _check_with_readers(d, s, bw, what):
  """dst := ALPHA dst + BETA src, checked without a download, with qh_inner and qh_amplitude only"""
  n = d.nbits
  with d.clone() as c:
    cc, ss, cs = c.inner(c).real, s.inner(s).real, c.inner(s)
    kd, ks = d.stats()['kernels_launched'], s.stats()['kernels_launched']
    n2 = _raw(d, ALPHA, s, BETA)
    assert d.stats()['kernels_launched'] - kd == 1 and s.stats()['kernels_launched'] == ks
    want_n2 = abs(ALPHA) ** 2 * cc + abs(BETA) ** 2 * ss + 2.0 * (np.conj(ALPHA) * BETA * cs).real
    nd = np.sqrt(n2)

    def bound(x_norm2):      # an inner product with x: Cauchy-Schwarz on one float rounding per component of d'
      return TOL if bw == 128 else EPS32 * np.sqrt(x_norm2) * nd
    e_c = abs(c.inner(d) - (ALPHA * cc + BETA * cs))
    e_s = abs(s.inner(d) - (ALPHA * np.conj(cs) + BETA * ss))
    e_n = abs(n2 - want_n2)
    print(f'{what}: |<c|d\'> - want| = {e_c:.3e} (bound {bound(cc):.3e}), |<s|d\'> - want| = {e_s:.3e} (bound {bound(ss):.3e}), '
          f'|norm2 - want| = {e_n:.3e} (bound {bound(n2):.3e})')
    assert e_c <= bound(cc) and e_s <= bound(ss) and e_n <= bound(n2)
    assert abs(n2 - d.inner(d).real) <= TOL
    rng = np.random.default_rng(7)
    worst = 0.0
    for i in rng.integers(0, 1 << n, size=64):
      ci, si, got = _amp(c, i), _amp(s, i), _amp(d, i)
      want = ALPHA * ci + BETA * si
      lim = TOL if bw == 128 else EPS32 * max(abs(ALPHA * ci), abs(BETA * si))
      err = max(abs(got.real - want.real), abs(got.imag - want.imag))
      worst = max(worst, err / lim if lim else float(err > 0))
      assert err <= lim, (what, int(i), got, want, lim)
    print(f'{what}: 64 sampled amplitudes, worst error / bound = {worst:.3f}')


def test_axpby_linear_blocks_of_two_chunks():
  """qh_axpby keeps qh_inner's geometry (4096 blocks at most, chunks of 2^11 16-byte items): at 24 local bits of complex128
  every block of the linear walk takes two chunks.  src is a clone of dst advanced by a few unfused gates (same layout)."""
  n = 24
  with _fused(n, 128, seed=0, depth=8) as d, d.clone() as s:
    s.set_fusion(native.QH_FUSE_OFF)
    s.apply1(gates.hadamard(), 2)
    s.applyc(gates.pauli_x(), 0, n - 1)
    s.apply1(gates.u1(0.37), 11)
    s.flush()
    assert d.inner_plan(s)['path'] == native.QH_INNER_LINEAR
    _check_with_readers(d, s, 128, 'linear 24 bits complex128')


def test_axpby_tiles_blocks_of_two_chunks():
  """... and chunks of 2^6 tiles of 2^8 amplitudes: at 27 local bits every block of the tiles walk takes two chunks.  Run at
  complex64 (1 GiB per state); dst and src are fused supremacy-27 runs of two seeds, which leave different layouts."""
  n = 27
  with _fused(n, 64, seed=0, depth=8) as d:
    s = None
    for seed in range(1, 5):
      s = _fused(n, 64, seed=seed, depth=8)
      if d.inner_plan(s)['path'] == native.QH_INNER_TILES:
        break
      s.close()
      s = None
    assert s is not None, 'no supremacy-27 run of seeds 1..4 left a layout other than that of seed 0'
    with s:
      _check_with_readers(d, s, 64, f'tiles 27 bits complex64 (seeds 0, {seed})')


# ---- 7. qc ------------------------------------------------------------------------------------------------------------------------------
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


def _qc(nq, seed, eager):
  q = circuit.qc('q', eager=eager)
  q.reg(nq, 0)
  _layers(q, nq, seed, 2)
  if not eager:
    q.run()
  return q


def _amps(q):
  return np.array(q.psi, dtype=np.complex128).reshape(-1)


@pytest.mark.parametrize('eager', [True, False])
def test_qc_combine_and_project_out(width128, eager):
  nq = 12
  a, b = _qc(nq, 1, eager), _qc(nq, 2, eager)
  assert hasattr(a._ensure_device(), 'axpby')
  pa, pb = _amps(a), _amps(b)
  if eager:
    a.h(3)                                                  # queued on the host side when combine comes: runs first
    t = pa.reshape(1 << 3, 2, -1)
    pa = np.stack([t[:, 0] + t[:, 1], t[:, 0] - t[:, 1]], axis=1).reshape(-1) / np.sqrt(2.0)
  # against another qc
  n2 = a.combine(b, ALPHA, BETA)
  want = ALPHA * pa + BETA * pb
  assert abs(n2 - np.vdot(want, want).real) <= TOL
  assert np.max(np.abs(_amps(a) - want)) <= TOL and np.max(np.abs(_amps(b) - pb)) <= TOL
  # against a Snapshot, normalised
  with b.snapshot() as snap:
    b.x(0)                                                  # the snapshot keeps what b was
    n2 = a.combine(snap, normalize=True)
    want = want + pb
    assert abs(n2 - np.vdot(want, want).real) <= TOL
    want = want / np.sqrt(n2)
    assert np.max(np.abs(_amps(a) - want)) <= TOL and abs(a.overlap(a) - 1.0) <= TOL
    # one Gram-Schmidt step against the snapshot, then against the circuit
    c = a.project_out(snap)
    assert abs(c - np.vdot(pb, want) / np.vdot(pb, pb).real) <= TOL
    want = want - c * pb
    print(f'eager={eager}: |<snapshot|self>| after project_out = {abs(a.overlap(snap)):.3e}')
    assert abs(a.overlap(snap)) < 1e-10
    assert np.max(np.abs(_amps(a) - want)) <= TOL
  pb = _amps(b)
  c = a.project_out(b)
  assert abs(c - np.vdot(pb, want) / np.vdot(pb, pb).real) <= TOL
  assert abs(b.overlap(a)) < 1e-10 and abs(a.overlap(b)) < 1e-10
  assert np.max(np.abs(_amps(a) - (want - c * pb))) <= TOL
  a.h(0)                                                    # the circuit goes on
  a.h(0)
  assert np.max(np.abs(_amps(a) - (want - c * pb))) <= TOL
  with pytest.raises(ValueError):
    a.combine(_qc(nq - 1, 3, True))
  with pytest.raises(ValueError):
    a.combine(pb)
  with a.snapshot() as same:
    with pytest.raises(ValueError):
      a.combine(same, 1.0, -1.0, normalize=True)
  for q in (a, b):
    q.close()
