"""CPU tests of the linear combination of two states: the C-ABI symbol and its argument checks (NULL, planner-only handles),
qc.combine / qc.project_out over the NumPy stand-in device, which has no axpby (the host route), and a NumPy model of the
write walk: scattering alpha * d[ia] + beta * s[ib] to ia over the pairs of the tile walk must give the combination in
logical order -- the index contract k_two_tiles implements for qh_axpby."""
import ctypes

import numpy as np
import pytest

from qcc_amd import device, native
from qcc_amd.lib import backend, circuit, tensor
from tests import fake_device, inner_util


# ---- the C-ABI ---------------------------------------------------------------------------------------------------------
def test_version_and_symbol_bound():
  lib = native.load()
  assert lib.qh_version() >= 112
  assert 'qh_axpby' in native.SIGNATURES
  assert lib.qh_axpby.argtypes == native.SIGNATURES['qh_axpby'][1]
  assert hasattr(device.DeviceState, 'axpby')


def test_null_and_dry_handles_are_argument_errors():
  lib = native.load()
  d1, d2 = ctypes.c_void_p(), ctypes.c_void_p()
  native.check(lib.qh_create_dry(10, 128, ctypes.byref(d1)))
  native.check(lib.qh_create_dry(10, 128, ctypes.byref(d2)))
  try:
    one, zero = (ctypes.c_double * 2)(1.0, 0.0), (ctypes.c_double * 2)(0.0, 0.0)
    n2 = ctypes.c_double(7.0)
    assert lib.qh_axpby(None, one, d2, one, ctypes.byref(n2)) == native.QH_ERR_ARG
    assert lib.qh_axpby(d1, one, None, one, ctypes.byref(n2)) == native.QH_ERR_ARG
    assert lib.qh_axpby(d1, None, d2, one, ctypes.byref(n2)) == native.QH_ERR_ARG
    assert lib.qh_axpby(d1, one, d2, None, ctypes.byref(n2)) == native.QH_ERR_ARG
    assert lib.qh_axpby(d1, one, d2, one, ctypes.byref(n2)) == native.QH_ERR_ARG and b'dry' in lib.qh_last_error()
    assert lib.qh_axpby(d1, one, d2, zero, None) == native.QH_ERR_ARG       # (the identity case is checked like any other)
    assert lib.qh_axpby(d1, one, d1, one, ctypes.byref(n2)) == native.QH_ERR_ARG
    assert n2.value == 7.0
  finally:
    lib.qh_destroy(d1)
    lib.qh_destroy(d2)


# ---- the write walk --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('nloc', [8, 9, 12])
def test_numpy_model_of_the_write_walk(nloc):
  """dst keeps ITS layout: the new value of dst's physical index ia is alpha * d[ia] + beta * s[ib] for the pair (ia, ib) of
  the walk, and every ia is written exactly once"""
  rng = np.random.default_rng(nloc)
  alpha, beta = 0.3 - 0.8j, -1.1 + 0.2j
  logical = np.arange(1 << nloc, dtype=np.uint64)
  for name, sa, sb in inner_util.hand_maps(nloc):
    a, b = device.DeviceState(nloc, 128, dry=True), device.DeviceState(nloc, 128, dry=True)
    try:
      for st, swaps in ((a, sa), (b, sb)):
        for x, y in swaps:
          st.remap_swap(x, y)
      plan = a.inner_plan(b)
      assert plan['path'] == native.QH_INNER_TILES, name
    finally:
      a.close()
      b.close()
    pa, pb = inner_util.apply_swaps(range(nloc), sa), inner_util.apply_swaps(range(nloc), sb)
    dl = rng.normal(size=1 << nloc) + 1j * rng.normal(size=1 << nloc)      # both states in LOGICAL order ...
    sl = rng.normal(size=1 << nloc) + 1j * rng.normal(size=1 << nloc)
    d, s = np.empty_like(dl), np.empty_like(sl)                             # ... and as they lie
    d[inner_util.spread(logical, pa).astype(np.int64)] = dl
    s[inner_util.spread(logical, pb).astype(np.int64)] = sl
    ia, ib = (x.astype(np.int64) for x in inner_util.tile_pairs(plan, nloc))
    new = np.full(1 << nloc, np.nan + 0j)
    writes = np.zeros(1 << nloc, dtype=np.int64)
    np.add.at(writes, ia, 1)
    assert np.all(writes == 1), name
    new[ia] = alpha * d[ia] + beta * s[ib]
    got = new[inner_util.spread(logical, pa).astype(np.int64)]              # back in logical order, through dst's map
    assert np.array_equal(got, alpha * dl + beta * sl), name


# ---- qc.combine / qc.project_out on the NumPy stand-in -----------------------------------------------------------------------
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


def _amps(q):
  return np.array(q.psi).reshape(-1).astype(np.complex128)


def _eps(width):
  """one rounding of a double result to the width's component type, relative to the value: 1e-12 stands in at complex128
  (the bound of the device tests), 2^-23 at complex64"""
  return 1e-12 if width == 128 else 2.0 ** -23


@pytest.mark.parametrize('nq', [3, 4, 6])
def test_fallback_combine(cpu_backend, nq):
  eps = _eps(cpu_backend)
  a, b = _circuit(nq, 1), _circuit(nq, 2)
  assert not hasattr(a._ensure_device(), 'axpby')
  pa, pb = _amps(a), _amps(b)
  alpha, beta = 0.6 - 0.3j, -0.2 + 1.1j
  want = alpha * pa + beta * pb
  n2 = a.combine(b, alpha, beta)
  # the norm is summed in double from the stored values: it differs from |want|^2 by the rounding of the components only
  assert isinstance(n2, float) and abs(n2 - np.vdot(want, want).real) <= 4 * eps * np.vdot(want, want).real
  assert np.max(np.abs(_amps(a) - want)) <= eps * np.max(np.abs(want))
  assert np.max(np.abs(_amps(b) - pb)) == 0.0                      # other is read only
  # defaults: self + other; a Snapshot as the other side; normalize
  want = _amps(a)
  with b.snapshot() as snap:
    b.h(0)                                                          # the snapshot keeps the earlier state
    n2 = a.combine(snap, normalize=True)
    want2 = want + pb
    assert abs(n2 - np.vdot(want2, want2).real) <= 4 * eps * np.vdot(want2, want2).real
    want2 = want2 / np.sqrt(n2)
    assert np.max(np.abs(_amps(a) - want2)) <= 2 * eps * np.max(np.abs(want2))      # (the sum and the quotient each round)
    assert abs(np.vdot(_amps(a), _amps(a)).real - 1.0) <= 8 * eps
  a.h(1)                                                            # the circuit goes on from the combined state
  a.h(1)
  assert np.max(np.abs(_amps(a) - want2)) <= 16 * eps * np.max(np.abs(want2))


def test_fallback_combine_errors(cpu_backend):
  a = _circuit(5, 1)
  before = _amps(a)
  with pytest.raises(ValueError):
    a.combine(_circuit(4, 2))                                       # another size
  with pytest.raises(ValueError):
    a.combine(before)                                               # not a qc or a Snapshot
  with pytest.raises(ValueError):
    a.project_out('psi')
  snap = a.snapshot()
  snap.close()
  with pytest.raises(ValueError):
    a.combine(snap)                                                 # closed
  with pytest.raises(ValueError):
    a.project_out(snap)
  with a.snapshot() as same:
    with pytest.raises(ValueError):
      a.combine(same, 1.0, -1.0, normalize=True)                    # the result is 0
  other_width = 64 if cpu_backend == 128 else 128
  with a.snapshot() as snap:
    tensor.set_tensor_width(other_width)
    try:
      w = _circuit(5, 3)
      with pytest.raises(ValueError):
        w.combine(snap)                                             # another width
    finally:
      tensor.set_tensor_width(cpu_backend)
  zero = _circuit(5, 4)
  zero.psi = np.zeros(1 << 5, dtype=tensor.tensor_type())
  with pytest.raises(ValueError):
    _circuit(5, 5).project_out(zero)                                # <other|other> is 0


@pytest.mark.parametrize('nq', [3, 5, 6])
def test_fallback_project_out(cpu_backend, nq):
  """complex128: <other|self> ends below 1e-12.  complex64 cannot: the host route forms <other|self> with np.vdot on
  float32 components (2^nq products added in float32) and stores the result rounded to float32, so the residual overlap is
  bounded by (2^nq + 2) * 2^-24 * |other| * |self| (Cauchy-Schwarz over one float32 rounding per product, per partial sum
  and per stored component), and that is what is asserted there."""
  a, b = _circuit(nq, 6), _circuit(nq, 7)
  pa, pb = _amps(a), _amps(b)
  b.psi = (pb * 0.5).astype(tensor.tensor_type())                  # c divides by <other|other>
  pb = _amps(b)
  bound = 1e-12 if cpu_backend == 128 else ((1 << nq) + 2) * 2.0 ** -24 * np.linalg.norm(pb) * np.linalg.norm(pa)
  want_c = np.vdot(pb, pa) / np.vdot(pb, pb).real
  c = a.project_out(b)
  print(f'width {cpu_backend} nq={nq}: |c - numpy| = {abs(c - want_c):.3e}, |<other|self>| after = {abs(b.overlap(a)):.3e} (bound {bound:.3e})')
  assert abs(c - want_c) * np.vdot(pb, pb).real <= bound
  assert np.max(np.abs(_amps(a) - (pa - want_c * pb))) <= max(bound, _eps(cpu_backend)) * 4
  assert abs(np.vdot(pb, _amps(a))) < bound
  assert abs(b.overlap(a)) < bound
  with b.snapshot() as snap:                                        # against a Snapshot: the same coefficient, now ~0
    assert abs(a.project_out(snap)) * np.vdot(pb, pb).real < 2 * bound
