"""Z-polynomial operators without a GPU: the C-ABI's symbols and refusals on planner-only handles, qh_zpoly_plan (classes,
bit map, shard signs), the stand-alone plan check, the qc entry points on NumPy stand-in devices against
zpoly_util's model, and the reference's own MaxCut diagonal (tests/golden/g15_maxcut_diag.npz)."""
import ctypes
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

from qcc_amd import device, native
from qcc_amd.lib import backend, circuit, tensor
from tests import fake_device, zpoly_util as zu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_dp = ctypes.POINTER(ctypes.c_double)
_up = ctypes.POINTER(ctypes.c_uint64)
CONST, HIGH, LOW, STRADDLE = native.QH_ZPOLY_CONST, native.QH_ZPOLY_HIGH, native.QH_ZPOLY_LOW, native.QH_ZPOLY_STRADDLE
CHUNK_BITS = 11      # qcc_amd/csrc/pauli_plan.h: 256 threads x 8 items per chunk


class ZpolyOracle(fake_device.OracleDevice):
  """OracleDevice with the two calls in NumPy (logical order = the array's order)."""
  applied = 0

  def apply_zpoly(self, weights, zmasks, c, norm=False):
    ZpolyOracle.applied += 1
    self.psi[:] = zu.np_apply(self.psi, weights, zmasks, c).astype(self.dtype)
    return float(np.vdot(self.psi.astype(np.complex128), self.psi.astype(np.complex128)).real) if norm else None

  def expect_zpoly(self, weights, zmasks):
    ZpolyOracle.applied += 1
    return zu.np_moments(self.psi, weights, zmasks)


# ---- the model ---------------------------------------------------------------------------------------------------------------
def test_model_against_dense_z_strings():
  """f against np.kron of diag(1, -1), once, at 5 qubits"""
  rng = np.random.default_rng(118)
  n = 5
  ws = rng.normal(size=9)
  zs = [int(v) for v in rng.integers(0, 1 << n, size=9)]
  zs[3] = 0
  want = np.zeros(1 << n)
  for w, z in zip(ws, zs):
    d = np.ones(1)
    for b in reversed(range(n)):      # bit n - 1 is the first Kronecker factor
      d = np.kron(d, np.array([1.0, -1.0]) if (z >> b) & 1 else np.ones(2))
    want += w * d
  assert np.max(np.abs(zu.np_f(np.arange(1 << n), ws, zs) - want)) <= 1e-14
  psi = rng.normal(size=1 << n) + 1j * rng.normal(size=1 << n)
  assert np.max(np.abs(zu.np_apply(psi, ws, zs, 0.3 - 0.2j) - psi * np.exp((0.3 - 0.2j) * want))) <= 1e-13


def test_golden_maxcut_diagonal_of_the_reference():
  """the reference's graph_to_diagonal_h equals sum_edges w^2 (-1)^(b_u + b_v) with node q on bit n - 1 - q: the model on
  maxcut_terms with w^2, to the last bit"""
  g = np.load(os.path.join(ROOT, 'tests', 'golden', 'g15_maxcut_diag.npz'))
  assert list(g['nodes']) == [8, 10, 12]
  for n in (8, 10, 12):
    edges, diag = g[f'edges{n}'], g[f'diag{n}']
    assert diag.shape == (1 << n,) and edges.shape == (2 * n - 3, 3)
    terms = circuit.qc.maxcut_terms([(int(u), int(v), w * w) for u, v, w in edges])
    ws = [w for w, _ in terms]
    zs = [sum(1 << (n - 1 - q) for q in p) for _, p in terms]
    f = zu.np_f(np.arange(1 << n), ws, zs)
    assert np.max(np.abs(f - diag)) <= 4 * len(ws) * 2.0 ** -53 * zu.big_f(ws)
    assert int(np.argmin(f)) == int(np.argmin(diag))


# ---- the C-ABI ---------------------------------------------------------------------------------------------------------------
def test_version_symbols_and_structs():
  lib = native.load()
  assert lib.qh_version() >= 118
  for name in ('qh_apply_zpoly', 'qh_expect_zpoly', 'qh_zpoly_plan'):
    assert name in native.SIGNATURES
    assert getattr(lib, name).argtypes == native.SIGNATURES[name][1]
  header = open(os.path.join(ROOT, 'include', 'qcc_hip.h')).read()
  assert f'#define QH_ZPOLY_MAX_TERMS {native.QH_ZPOLY_MAX_TERMS}\n' in header and native.QH_ZPOLY_MAX_TERMS == 4096
  for name, v in zip(('CONST', 'HIGH', 'LOW', 'STRADDLE'), (CONST, HIGH, LOW, STRADDLE)):
    assert f'#define QH_ZPOLY_{name} {v}\n' in header
  t = native.QH_ZPOLY_MAX_TERMS
  assert ctypes.sizeof(native.QhZpolyInfo) == 7 * 8 + 4 * 4 + 3 * 8 * t + t


def _dry(n, bw=128, nglob=None, shard=0):
  st = device.DeviceState(n, bw, dry=True)
  if nglob is not None:
    st.set_shard(nglob, shard)
  return st


def _pending(st):
  pend = ctypes.c_uint64()
  native.check(st.lib.qh_pending_gates(st.h, ctypes.byref(pend)))
  return pend.value


def test_refusals_on_a_dry_handle():
  """every refusal of the three calls, none of which needs a state; the message names the first offending term; the outputs
  are untouched"""
  lib = native.load()
  st = _dry(10)
  try:
    n2 = ctypes.c_double(7.0)
    out = (ctypes.c_double * 3)(7.0, 7.0, 7.0)
    info = native.QhZpolyInfo()
    cc = (ctypes.c_double * 2)(0.0, -0.5)

    def arrays(ws, zs):
      w, z = np.asarray(ws, dtype=np.float64), np.asarray(zs, dtype=np.uint64)
      return (w, z), w.size, w.ctypes.data_as(_dp), z.ctypes.data_as(_up)

    calls = {'apply': lambda h, n, w, z: lib.qh_apply_zpoly(h, n, w, z, cc, ctypes.byref(n2)),
             'expect': lambda h, n, w, z: lib.qh_expect_zpoly(h, n, w, z, out),
             'plan': lambda h, n, w, z: lib.qh_zpoly_plan(h, n, w, z, ctypes.byref(info))}
    for what, call in calls.items():
      keep, n, w, z = arrays([1.0, 2.0, 3.0], [1, 2, 4])
      assert call(None, n, w, z) == native.QH_ERR_ARG, what
      assert call(st.h, n, None, z) == native.QH_ERR_ARG, what
      assert call(st.h, n, w, None) == native.QH_ERR_ARG, what
      big = arrays(np.ones(native.QH_ZPOLY_MAX_TERMS + 1), np.ones(native.QH_ZPOLY_MAX_TERMS + 1))
      assert call(st.h, *big[1:]) == native.QH_ERR_ARG and b'4097' in lib.qh_last_error(), what
      for bad in (np.inf, -np.inf, np.nan):
        k2 = arrays([1.0, 2.0, bad, np.nan], [1, 2, 4, 8])
        assert call(st.h, *k2[1:]) == native.QH_ERR_ARG, what
        assert b'term 2' in lib.qh_last_error() and b'non-finite' in lib.qh_last_error(), what
      k3 = arrays([1.0, 2.0, 3.0], [1, 1 << 10, 1 << 11])
      assert call(st.h, *k3[1:]) == native.QH_ERR_BAD_QUBIT and b'term 1' in lib.qh_last_error(), what
      if what != 'plan':      # a dry handle holds no state, not even for no terms
        assert call(st.h, n, w, z) == native.QH_ERR_ARG and b'dry' in lib.qh_last_error(), what
        assert call(st.h, 0, None, None) == native.QH_ERR_ARG and b'dry' in lib.qh_last_error(), what
      else:
        assert call(st.h, n, w, z) == native.QH_OK and call(st.h, 0, None, None) == native.QH_OK
    keep, n, w, z = arrays([1.0], [1])
    assert lib.qh_apply_zpoly(st.h, n, w, z, None, ctypes.byref(n2)) == native.QH_ERR_ARG
    for bad in ((np.inf, 0.0), (0.0, np.nan)):
      assert lib.qh_apply_zpoly(st.h, n, w, z, (ctypes.c_double * 2)(*bad), ctypes.byref(n2)) == native.QH_ERR_ARG
      assert b'not finite' in lib.qh_last_error()
    assert lib.qh_expect_zpoly(st.h, n, w, z, None) == native.QH_ERR_ARG
    assert lib.qh_zpoly_plan(st.h, n, w, z, None) == native.QH_ERR_ARG
    assert n2.value == 7.0 and list(out) == [7.0, 7.0, 7.0] and _pending(st) == 0
  finally:
    st.close()


def _want_class(pz, low_bits):
  lo, hi = pz & ((1 << low_bits) - 1), pz >> low_bits
  return CONST if pz == 0 else STRADDLE if (lo and hi) else HIGH if hi else LOW


def _to_phys(bitmap, z):
  return sum(1 << bitmap[b] for b in range(len(bitmap)) if (z >> b) & 1)


def _bitmap(st):
  bm = (ctypes.c_int32 * 64)()
  native.check(st.lib.qh_get_bitmap(st.h, bm))
  return [int(bm[b]) for b in range(st.nbits)]


def _check_plan(st, ws, zs, nglob=None, shard=0):
  n = st.nbits
  ab = 0 if st.bit_width == 128 else 1
  main = n - ab >= CHUNK_BITS
  low_bits = CHUNK_BITS + ab if main else n
  p = st.zpoly_plan(ws, zs)
  assert p['nterms'] == len(ws) and p['kernel'] == (native.QH_ZPOLY_KERNEL_MAIN if main else native.QH_ZPOLY_KERNEL_SMALL)
  assert p['low_bits'] == low_bits
  bm = _bitmap(st) + list(range(n, nglob or n))
  phys = [_to_phys(bm, z) for z in zs]
  assert p['pz'] == [z & ((1 << n) - 1) for z in phys]
  assert p['w'] == [-w if bin(shard & (z >> n)).count('1') % 2 else w for w, z in zip(ws, phys)]
  assert p['cls'] == [_want_class(z, low_bits) for z in p['pz']]
  counts = [p['nconst'], p['nhigh'], p['nlow'], p['nstraddle']]
  assert counts == [p['cls'].count(c) for c in (CONST, HIGH, LOW, STRADDLE)] and sum(counts) == len(ws)      # a partition
  groups = []
  for z, c in zip(p['pz'], p['cls']):
    if c == STRADDLE and (z & ((1 << low_bits) - 1)) not in groups:
      groups.append(z & ((1 << low_bits) - 1))
  assert p['group_mask'] == groups and p['ngroups'] == len(groups)
  if main:
    nchunks = 1 << (n - low_bits)
    assert p['nblk'] == min(nchunks, 4096) and p['cpb'] * p['nblk'] == nchunks
  else:
    assert p['nblk'] == ((1 << n) + 255) // 256
  return p


def test_plan_classes_on_dry_handles():
  rng = np.random.default_rng(7)
  for bw in (128, 64):
    ab = 0 if bw == 128 else 1
    for n in (1, 5, 10 + ab, 11 + ab, 14, 20, 30):
      st = _dry(n, bw)
      try:
        T = 40
        zs = [int(v) for v in rng.integers(0, 1 << n, size=T)]
        zs[5], zs[17] = 0, zs[3]                             # a constant and a duplicate
        if n >= 14:
          zs[:6] = [1, 1 << (n - 1), 1 | (1 << (n - 1)), 3 | (1 << (n - 2)), 1 | (3 << (n - 2)), 0]
        ws = [float(v) for v in rng.normal(size=T)]
        p = _check_plan(st, ws, zs)
        if n >= 14:
          assert p['cls'][:6] == [LOW, HIGH, STRADDLE, STRADDLE, STRADDLE, CONST]
          assert p['group_mask'][:2] == [1, 3]              # terms 2 and 4 share the low mask 1
        p0 = _check_plan(st, [], [])
        assert p0['nterms'] == 0 and p0['ngroups'] == 0
      finally:
        st.close()


def test_plan_moves_with_the_bit_map():
  for bw in (128, 64):
    ab = 0 if bw == 128 else 1
    st = _dry(16, bw)
    try:
      zs = [1 << 0, 1 << 15, (1 << 0) | (1 << 15), (1 << 3) | (1 << 4)]
      ws = [1.0, 2.0, 3.0, 4.0]
      assert _check_plan(st, ws, zs)['cls'] == [LOW, HIGH, STRADDLE, LOW]
      st.remap_swap(0, 14)                                   # logical 0 now sits in the chunk part, logical 14 in the low part
      p = _check_plan(st, ws, zs)
      assert p['cls'] == [HIGH, HIGH, HIGH, LOW] and p['pz'][0] == 1 << 14
      st.remap_swap(15, 3)
      p = _check_plan(st, ws, zs)
      assert p['cls'] == [HIGH, LOW, STRADDLE, STRADDLE] and p['group_mask'] == [1 << 3, 1 << 4]
      assert p['low_bits'] == CHUNK_BITS + ab
    finally:
      st.close()


def test_plan_folds_shard_signs():
  """a z bit held by the shard index negates the weight where the shard index has an odd number of ones under it"""
  for bw in (128, 64):
    for nloc, nglob in ((10, 12), (13, 15)):
      for shard in range(4):
        sh = _dry(nloc, bw, nglob=nglob, shard=shard)
        try:
          h0, h1 = 1 << nloc, 1 << (nloc + 1)
          zs = [h0, h1, h0 | h1, h0 | 1, h1 | (1 << (nloc - 1)) | 2, 5, 0]
          ws = [1.5, -2.5, 0.25, 3.0, 1.0, 2.0, -7.0]
          p = _check_plan(sh, ws, zs, nglob=nglob, shard=shard)
          negs = [shard & 1, shard >> 1, (shard & 1) ^ (shard >> 1), shard & 1, shard >> 1, 0, 0]
          assert p['w'] == [-w if s else w for w, s in zip(ws, negs)]
          assert p['pz'] == [0, 0, 0, 1, (1 << (nloc - 1)) | 2, 5, 0]
          assert p['cls'][:3] == [CONST] * 3               # only the sign is left of them
        finally:
          sh.close()


def test_plan_check_stand_alone():
  """tools/zpoly_plan_check.cc is plain C++ over zpoly_plan.h with its own main: the classes partition the terms, f rebuilt
  from the device block equals the popcount sum at every amplitude (integer weights: exact), the grid covers every item
  once; both widths, every size from 1 to 14 local bits.  A plain build; nothing is loaded into this process."""
  cxx = shutil.which('g++')
  assert cxx, 'no g++'
  import tempfile
  with tempfile.TemporaryDirectory() as tmp:
    exe = os.path.join(tmp, 'zpoly_plan_check')
    subprocess.check_call([cxx, '-std=c++17', '-O2', os.path.join(ROOT, 'tools', 'zpoly_plan_check.cc'), '-o', exe])
    res = subprocess.run([exe, '4'], capture_output=True, text=True, timeout=120)
  assert res.returncode == 0, res.stdout + res.stderr
  assert 'ok' in res.stdout


# ---- qc on NumPy devices -------------------------------------------------------------------------------------------------------
@pytest.fixture(params=[('apply_zpoly', 128), ('apply_zpoly', 64), ('fallback', 128), ('fallback', 64)], ids=lambda p: f'{p[0]}-{p[1]}')
def cpu_backend(request):
  kind, width = request.param
  tensor.set_tensor_width(width)
  backend.set_device_factory(ZpolyOracle if kind == 'apply_zpoly' else fake_device.OracleDevice)
  yield kind, width
  backend.set_device_factory(None)
  tensor.set_tensor_width(None)


def _circuit(nq, seed):
  rng = np.random.default_rng(seed)
  q = circuit.qc('z')
  q.reg(nq, 0)
  for _ in range(3 * nq):
    a = int(rng.integers(nq))
    q.ry(a, float(rng.random() * 3))
    b = int(rng.integers(nq))
    if b != a:
      q.cx(a, b)
    q.rz(int(rng.integers(nq)), float(rng.random() * 3))
  return q


def _amps(q):
  return np.asarray(q.psi).reshape(-1).astype(np.complex128)


def _masks(n, terms):
  return [float(w) for w, _ in terms], [sum(1 << (n - 1 - q) for q, p in paulis.items() if p == 'Z') for _, paulis in terms]


TERMS6 = [(0.7, {0: 'Z', 3: 'Z'}), (-1.1, {5: 'Z'}), (0.4, {}), (2.0, {1: 'Z', 2: 'Z', 4: 'Z'}), (0.7, {0: 'Z', 3: 'Z'}), (-0.3, {2: 'Z', 5: 'I'})]


def test_qc_entry_points_against_the_model(cpu_backend):
  kind, width = cpu_backend
  n = 6
  ws, zs = _masks(n, TERMS6)
  used = ZpolyOracle.applied
  q = _circuit(n, 3)
  psi = _amps(q)
  amax = float(np.max(np.abs(psi)))
  q.phase_polynomial(TERMS6, 0.37)
  got = _amps(q)
  assert np.max(np.abs(got - zu.np_apply(psi, ws, zs, -0.37j))) <= 2 * zu.apply_bound(width, ws, -0.37j, amax)
  mean, second = q.cost_expectation(TERMS6, moments=True)
  m = zu.np_moments(got, ws, zs)
  assert abs(mean - m[1]) <= zu.moment_bound(ws, 1, m[0]) and abs(second - m[2]) <= zu.moment_bound(ws, 2, m[0])
  assert q.cost_expectation(TERMS6) == mean
  want_e = q.expectation(TERMS6)
  assert abs(mean - want_e) <= (1e-12 if width == 128 else 1e-5) * zu.big_f(ws)
  # imaginary time
  n2 = q.cost_filter(TERMS6, 0.2, normalize=False)
  want = zu.np_apply(got, ws, zs, -0.2)
  assert np.max(np.abs(_amps(q) - want)) <= 2 * zu.apply_bound(width, ws, -0.2, amax)
  stored = _amps(q)
  assert abs(n2 - float(np.vdot(stored, stored).real)) <= 1e-12 * n2
  n2b = q.cost_filter(TERMS6, 0.1)
  assert abs(q.norm2() - 1.0) <= (1e-12 if width == 128 else 1e-6) and n2b > 0
  # a layer: the cost phase, then rx(2 beta) everywhere
  before = _amps(q)
  q.qaoa_layer(TERMS6, 0.3, 0.45)
  v = zu.np_apply(before, ws, zs, -0.3j)
  rx = np.array([[math.cos(0.45), -1j * math.sin(0.45)], [-1j * math.sin(0.45), math.cos(0.45)]])
  for k in range(n):
    t = v.reshape(1 << k, 2, -1)
    v = np.einsum('ab,xbr->xar', rx, t).reshape(-1)
  assert np.max(np.abs(_amps(q) - v)) <= (1e-13 if width == 128 else 2e-6)
  assert (ZpolyOracle.applied > used) == (kind == 'apply_zpoly')      # the device call where there is one, else the host formula


def test_qc_maxcut_terms_and_errors(cpu_backend):
  q = _circuit(5, 4)
  assert circuit.qc.maxcut_terms([(0, 1, 2.0), (3, 1, 0.5)]) == [(2.0, {0: 'Z', 1: 'Z'}), (0.5, {3: 'Z', 1: 'Z'})]
  assert q.maxcut_terms([]) == []
  with pytest.raises(ValueError):
    circuit.qc.maxcut_terms([(0, 1)])
  with pytest.raises(ValueError):
    circuit.qc.maxcut_terms([(2, 2, 1.0)])
  psi = _amps(q)
  for call in (lambda t: q.phase_polynomial(t, 0.1), lambda t: q.cost_filter(t, 0.1), lambda t: q.cost_expectation(t),
               lambda t: q.qaoa_layer(t, 0.1, 0.2)):
    for bad in ([(1.0, {0: 'X'})], [(1.0, {0: 'Z'}), (1.0, {1: 'Y', 2: 'Z'})], [(1.0 + 0.5j, {0: 'Z'})], [(1.0, {7: 'Z'})], [3.0]):
      with pytest.raises(ValueError):
        call(bad)
  assert np.array_equal(_amps(q), psi)                       # nothing was applied
  # a filter that leaves nothing: a zero state in, ValueError out
  z = circuit.qc('zero')
  z.reg(3, 0)
  z.psi = np.zeros(8, dtype=np.asarray(z.psi).dtype)
  with pytest.raises(ValueError):
    z.cost_filter([(1.0, {0: 'Z'})], 0.5)
  assert z.cost_filter([(1.0, {0: 'Z'})], 0.5, normalize=False) == 0.0
