"""CPU tests of the reduced density matrices: the golden matrices of the reference, the C-ABI symbols and their refusals on
planner-only handles, qh_density_plan's tables and geometry over many layouts, tools/density_plan_check.cc stand-alone under
ASan and UBSan, and qc.reduced_density / purity / entropy / schmidt_coefficients / mutual_information / bloch with the GPU
replaced by a NumPy stand-in that implements reduced_density and over the fallback that reads qc.psi.

The reference value everywhere is density_util.np_reduced_density: A @ A^H in complex128 NumPy."""
import ctypes
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

from qcc_amd import device, native
from qcc_amd.lib import backend, circuit, helper, ops, tensor
from tests import density_util as du, fake_device

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_dp = ctypes.POINTER(ctypes.c_double)
_ip = ctypes.POINTER(ctypes.c_int32)
KMAX = native.QH_DENSITY_MAX_BITS


class DensityOracle(fake_device.OracleDevice):
  """OracleDevice with reduced_density in NumPy (logical order = the array's order)."""
  reads = 0

  def reduced_density(self, bits):
    DensityOracle.reads += 1
    return du.np_reduced_density(self.psi, [int(b) for b in bits])


def _golden():
  g = np.load(os.path.join(ROOT, 'tests', 'golden', 'g14_reduced_density.npz'))
  off, at, recs = g['offsets'], 0, []
  for j in range(len(off) - 1):
    qubits = [int(q) for q in g['qubits'][off[j]:off[j + 1]]]
    d = 1 << len(qubits)
    recs.append((qubits, g['rho'][at:at + d * d].reshape(d, d)))
    at += d * d
  assert at == g['rho'].size
  return int(g['nbits']), g['psi'], recs


def test_golden_matrices_of_the_reference_against_the_formula():
  """tests/golden/g14_reduced_density.npz (tools/make_golden_reduced_density.py): ops.TraceOut(psi.density(), others) of the
  reference against the util formula; singles, pairs, 3-4 qubits and 6 are all there"""
  n, psi, recs = _golden()
  assert n == 8 and psi.shape == (256,)
  assert sorted({len(q) for q, _ in recs}) == [1, 2, 3, 4, 6] and len(recs) >= 18
  for qubits, want in recs:
    got = du.np_qubit_density(psi, qubits)
    assert np.max(np.abs(got - want)) <= 1e-14, qubits
    assert abs(np.trace(want).real - 1.0) <= 1e-13
  assert os.path.getsize(os.path.join(ROOT, 'tests', 'golden', 'g14_reduced_density.npz')) < 100_000


# ---- the C-ABI ---------------------------------------------------------------------------------------------------------
def test_version_symbols_and_struct():
  lib = native.load()
  assert lib.qh_version() >= 117
  for name in ('qh_reduced_density', 'qh_density_plan'):
    assert name in native.SIGNATURES
    assert getattr(lib, name).argtypes == native.SIGNATURES[name][1]
  assert KMAX == 8 and device.MAX_DENSITY_BITS == 8
  header = open(os.path.join(ROOT, 'include', 'qcc_hip.h')).read()
  assert '#define QH_DENSITY_MAX_BITS 8\n' in header
  for name, v in (('TILES', native.QH_DENSITY_TILES), ('GATHER', native.QH_DENSITY_GATHER)):
    assert f'#define QH_DENSITY_{name} {v} ' in header
  # the struct as the header lays it out: 8 u32, 3 u64, 8 + 8 + 16 + 40 bytes
  assert ctypes.sizeof(native.QhDensityTiles) == 8 * 4 + 3 * 8 + 8 + 8 + 16 + 40 == 128
  assert native.QhDensityTiles.chunks_per_wg.offset == 32 and native.QhDensityTiles.row_pos.offset == 56
  assert native.QhDensityTiles.rest_pos.offset == 88


def _dry(n, bw=128, nglob=None, shard=0):
  st = device.DeviceState(n, bw, dry=True)
  if nglob is not None:
    st.set_shard(nglob, shard)
  return st


SENTINEL = -7.25


def _rho_rc(st, bits, k=None, bits_null=False, out_null=False):
  """(status, out untouched) of qh_reduced_density"""
  lib = native.load()
  b = np.asarray(list(bits) + [0], dtype=np.int32)
  k = len(bits) if k is None else k
  out = np.full(2 << (2 * min(max(k, 0), KMAX)), SENTINEL, dtype=np.float64)
  rc = lib.qh_reduced_density(st.h if st else None, k, None if bits_null else b.ctypes.data_as(_ip),
                              None if out_null else out.ctypes.data_as(_dp))
  return rc, bool(np.all(out == SENTINEL))


def _plan_rc(st, bits, k=None, bits_null=False, out_null=False):
  lib = native.load()
  b = np.asarray(list(bits) + [0], dtype=np.int32)
  t = native.QhDensityTiles()
  t.path = 99
  rc = lib.qh_density_plan(st.h if st else None, len(bits) if k is None else k, None if bits_null else b.ctypes.data_as(_ip),
                           None if out_null else ctypes.byref(t))
  return rc, t.path == 99


@pytest.mark.parametrize('bw', [128, 64])
def test_refusals_on_planner_only_handles(bw):
  """every QH_ERR_ARG, QH_ERR_BAD_QUBIT and QH_ERR_SAME_QUBIT case of both calls; out keeps its sentinel"""
  lib = native.load()
  st, small = _dry(10, bw), _dry(5, bw)
  A, B, S = native.QH_ERR_ARG, native.QH_ERR_BAD_QUBIT, native.QH_ERR_SAME_QUBIT
  try:
    for call in (_rho_rc, _plan_rc):
      assert call(None, [1]) == (A, True)
      assert call(st, [1], bits_null=True) == (A, True)
      assert call(st, [1], out_null=True)[0] == A
      assert call(st, [], k=-1) == (A, True)
      assert call(st, list(range(9))) == (A, True)                       # k = 9 > QH_DENSITY_MAX_BITS
      assert call(small, list(range(6)), k=6) == (A, True)               # k = 6 > nbits_local = 5
      assert call(st, [0, 10]) == (B, True)
      assert call(st, [-1]) == (B, True)
      assert call(st, [3, 4, 3]) == (S, True)
      assert call(st, [10, 10]) == (B, True)                             # the range is checked first
    # a correct call on a planner-only handle: the plan answers, the matrix needs a state
    assert _plan_rc(st, [1, 2]) == (native.QH_OK, False)
    assert _plan_rc(st, [], bits_null=True) == (native.QH_OK, False)     # k = 0 needs no bits
    assert _rho_rc(st, [1, 2]) == (A, True)
    assert b'dry' in lib.qh_last_error()
    assert _rho_rc(st, [], bits_null=True) == (A, True)
    # the Python wrapper refuses k > 8 before sizing anything
    with pytest.raises(native.QhError) as e:
      st.reduced_density(list(range(9)))
    assert e.value.code == A
  finally:
    st.close()
    small.close()


def _pending(st):
  pend = ctypes.c_uint64()
  native.check(st.lib.qh_pending_gates(st.h, ctypes.byref(pend)))
  return pend.value


def _bitmap(st, n):
  bm = (ctypes.c_int32 * n)()
  native.check(st.lib.qh_get_bitmap(st.h, bm))
  return [int(b) for b in bm]


def _check_plan(st, nloc, bm, bits):
  """the plan of `bits` on st against the rules of include/qcc_hip.h, restated"""
  pl = st.density_plan(bits)
  k = len(bits)
  pos = [bm[b] for b in bits]
  gather = nloc < 8
  kt = k if gather else min(k, 6)
  assert pl['k'] == k and pl['tile_bits'] == kt
  assert pl['path'] == (native.QH_DENSITY_GATHER if gather else native.QH_DENSITY_TILES)      # gather exactly where no tile fits
  rows, cb, nrest = pl['row_pos'][:k], pl['chunk_bits'], pl['nrest']
  cols, rest = pl['col_pos'][:cb], pl['rest_pos'][:nrest]
  assert rows == sorted(pos) and [pos[t] for t in pl['row_bit'][:k]] == rows
  env = [p for p in range(nloc) if p not in pos]
  assert cols == env[:cb] and rest == env[cb:]                          # ascending, disjoint, the LOWEST free positions
  nb = 1 << (k - kt)
  assert pl['block_pairs'] == nb * (nb + 1) // 2 and pl['block_pairs'] in (1, 3, 10)
  assert pl['wg_per_pair'] * pl['chunks_per_wg'] * (1 << cb) == 1 << (nloc - k)      # the environment exactly once
  if gather:
    assert cb == 0 and pl['wg_per_pair'] == 1 and pl['slab_bytes'] == 0 and pl['amps_swept'] == 1 << nloc
  else:
    assert cb == min(nloc - k, 11 - kt - (1 if nb > 1 else 0))
    assert pl['slab_bytes'] == (16 << (2 * kt)) * pl['wg_per_pair'] * pl['block_pairs'] <= 32 << 20
    assert pl['wg_per_pair'] * pl['block_pairs'] <= 2048
    assert pl['amps_swept'] == nb << nloc
  return pl


@pytest.mark.parametrize('bw', [128, 64])
def test_plan_on_planner_only_handles(bw):
  rng = np.random.default_rng(3)
  had = np.array([1, 0, 1, 0, 1, 0, -1, 0], dtype=np.float64) / math.sqrt(2.0)
  paths = set()
  for n in range(1, 15):
    st = _dry(n, bw)
    try:
      for round_ in range(2):
        if round_ == 1:                                                   # a permuted bit map
          for _ in range(n):
            a, b = (int(v) for v in rng.integers(n, size=2))
            if a != b:
              st.remap_swap(a, b)
          native.check(st.lib.qh_set_fusion(st.h, native.QH_FUSE_SWEEP))   # a queued gate stays queued
          native.check(st.lib.qh_apply1(st.h, 0, had.ctypes.data_as(_dp)))
        bm = _bitmap(st, n)
        inv = {p: b for b, p in enumerate(bm)}
        for k in range(0, min(n, KMAX) + 1):
          low = [inv[p] for p in range(k)]                                # by PHYSICAL position: the lowest, the highest, mixed
          high = [inv[p] for p in range(n - k, n)]
          mixed = [inv[int(p)] for p in rng.permutation(n)[:k]]
          for bits in (low, high[::-1], mixed):
            pl = _check_plan(st, n, bm, bits)
            paths.add(pl['path'])
        if round_ == 1:
          assert _pending(st) == 1
    finally:
      st.close()
  assert paths == {native.QH_DENSITY_TILES, native.QH_DENSITY_GATHER}
  # geometry at a size where the grid caps bind: k = 6 is bounded by the slab, k = 8 has 10 pairs
  st = _dry(30, bw)
  try:
    pl = _check_plan(st, 30, list(range(30)), [0, 1, 2, 3, 4, 5])
    assert pl['wg_per_pair'] == 512 and pl['slab_bytes'] == 32 << 20 and pl['chunk_bits'] == 5
    pl = _check_plan(st, 30, list(range(30)), list(range(22, 30)))
    assert pl['block_pairs'] == 10 and pl['wg_per_pair'] == 32 and pl['chunk_bits'] == 4 and pl['amps_swept'] == 4 << 30
    pl = _check_plan(st, 30, list(range(30)), [7])
    assert pl['wg_per_pair'] == 2048 and pl['chunk_bits'] == 10 and pl['col_pos'][:10] == [0, 1, 2, 3, 4, 5, 6, 8, 9, 10]
  finally:
    st.close()


def test_plan_on_shard_handles():
  """a listed bit held by the shard index is QH_ERR_NONLOCAL for both calls; local ones plan as on an unsharded handle"""
  lib = native.load()
  for bw in (128, 64):
    sh = _dry(10, bw, nglob=12, shard=2)
    try:
      assert _plan_rc(sh, [0, 10]) == (native.QH_ERR_NONLOCAL, True)
      assert b'shard index' in lib.qh_last_error()
      assert _rho_rc(sh, [11]) == (native.QH_ERR_NONLOCAL, True)
      assert _plan_rc(sh, [12]) == (native.QH_ERR_BAD_QUBIT, True)
      _check_plan(sh, 10, list(range(12)), [9, 0, 4])
      sh.remap_swap(11, 0)                                               # logical 0 is now held, logical 11 local
      assert _plan_rc(sh, [0]) == (native.QH_ERR_NONLOCAL, True)
      bm = _bitmap(sh, 12)
      _check_plan(sh, 10, bm, [11, 3])
    finally:
      sh.close()


def test_plan_check_stand_alone_with_sanitizers(tmp_path):
  """tools/density_plan_check.cc is plain C++ over density_plan.h with its own main: for every size up to 12 local bits,
  every k and a sample of placements, the tables are consistent and every amplitude is visited once per block pair that
  needs it.  Built with ASan and UBSan, the runtimes linked statically; nothing is loaded into this process."""
  cxx = shutil.which('g++')
  assert cxx, 'no g++'
  exe = str(tmp_path / 'density_plan_check')
  subprocess.check_call([cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-static-libasan',
                         '-static-libubsan', os.path.join(ROOT, 'tools', 'density_plan_check.cc'), '-o', exe])
  res = subprocess.run([exe, '6', '12'], capture_output=True, text=True, timeout=120)
  assert res.returncode == 0, res.stdout + res.stderr
  assert 'ok' in res.stdout


# ---- qc on NumPy devices -------------------------------------------------------------------------------------------------
@pytest.fixture(params=[('reduced_density', 128), ('reduced_density', 64), ('fallback', 128), ('fallback', 64)],
                ids=lambda p: f'{p[0]}-{p[1]}')
def cpu_backend(request):
  kind, width = request.param
  tensor.set_tensor_width(width)
  backend.set_device_factory(DensityOracle if kind == 'reduced_density' else fake_device.OracleDevice)
  yield kind, width
  backend.set_device_factory(None)
  tensor.set_tensor_width(None)


def _eps(width):
  return 1e-12 if width == 128 else 4e-6


def _reg(n):
  q = circuit.qc('d')
  q.reg(n, 0)
  return q


def _random_circuit(nq, seed):
  rng = np.random.default_rng(seed)
  q = _reg(nq)
  for _ in range(3 * nq):
    a = int(rng.integers(nq))
    q.ry(a, float(rng.random() * 3))
    b = int(rng.integers(nq))
    if b != a:
      q.cx(a, b)
    q.rz(int(rng.integers(nq)), float(rng.random() * 3))
  return q


def test_golden_against_qc(cpu_backend):
  kind, width = cpu_backend
  n, psi, recs = _golden()
  q = _reg(n)
  q.psi = psi.astype(tensor.tensor_type())                                # current on the host only, not a product: uploaded
  reads = DensityOracle.reads
  for qubits, want in recs:
    got = q.reduced_density(qubits)
    assert isinstance(got, ops.Operator) and got.shape == want.shape
    assert np.max(np.abs(np.asarray(got) - want)) <= _eps(width), qubits
  if kind == 'reduced_density':
    assert DensityOracle.reads == reads + len(recs)


def test_bell_ghz_and_product_states(cpu_backend):
  _kind, width = cpu_backend
  eps = _eps(width)
  q = _reg(2)
  q.h(0)
  q.cx(0, 1)
  for qb in (0, 1):
    assert abs(q.entropy([qb]) - 1.0) <= 8 * eps
    assert abs(q.purity([qb]) - 0.5) <= 8 * eps
    assert np.max(np.abs(q.schmidt_coefficients([qb]) - [math.sqrt(0.5)] * 2)) <= 8 * eps
    assert np.max(np.abs(q.bloch(qb))) <= 8 * eps                       # maximally mixed: the centre of the ball
  assert abs(q.mutual_information([0], [1]) - 2.0) <= 32 * eps
  assert abs(q.entropy([0, 1])) <= (1e-9 if width == 128 else 1e-4)      # pure: 0 up to -x log x of an eigenvalue's rounding
  assert abs(q.entropy([0], base=math.e) - math.log(2.0)) <= 8 * eps
  g = _reg(5)
  g.h(0)
  for t in range(1, 5):
    g.cx(0, t)
  for sub in ([0], [4], [1, 3], [0, 1, 2], [1, 2, 3, 4], [4, 0]):
    assert abs(g.entropy(sub) - 1.0) <= 16 * eps, sub
    assert abs(g.purity(sub) - 0.5) <= 16 * eps
  p = _reg(4)
  for t in range(4):
    p.ry(t, 0.4 + t)
    p.rz(t, 1.1 * t)
  for sub in ([0], [2, 3], [3, 0, 1]):
    assert abs(p.purity(sub) - 1.0) <= 16 * eps
    assert abs(p.entropy(sub)) <= (1e-9 if width == 128 else 1e-4)
  assert abs(p.mutual_information([0], [2, 3])) <= (1e-9 if width == 128 else 3e-4)
  sc = p.schmidt_coefficients([1, 2])
  assert sc.shape == (4,) and abs(sc[0] - 1.0) <= 16 * eps and np.all(np.diff(sc) <= 0) and np.all(sc >= 0)


def test_bloch_is_qubit_to_bloch_on_product_states(cpu_backend):
  _kind, width = cpu_backend
  angles = [(0.3, 0.0), (1.2, 2.1), (2.9, -0.7)]
  q = _reg(3)
  for t, (a, b) in enumerate(angles):
    q.ry(t, a)
    q.rz(t, b)
  for t, (a, b) in enumerate(angles):
    one = _reg(1)
    one.ry(0, a)
    one.rz(0, b)
    want = helper.qubit_to_bloch(np.asarray(one.psi).reshape(-1).astype(np.complex128))
    got = q.bloch(t)
    assert len(got) == 3 and np.max(np.abs(np.asarray(got) - np.asarray(want))) <= 16 * _eps(width), t
    assert abs(sum(c * c for c in got) - 1.0) <= 32 * _eps(width)       # a pure qubit: on the sphere


def test_register_order_and_trace(cpu_backend):
  """non-ascending qubits give the permuted matrix; the result is not renormalised"""
  _kind, width = cpu_backend
  n = 6
  q = _random_circuit(n, 11)
  psi = np.asarray(q.psi).reshape(-1).astype(np.complex128)
  for qubits in ([1, 4], [4, 1], [5, 0, 2], [2, 5, 0], [3], list(range(6)), [], [5, 4, 3, 2, 1, 0]):
    got = np.asarray(q.reduced_density(qubits))
    assert np.max(np.abs(got - du.np_qubit_density(psi, qubits))) <= _eps(width), qubits
  a, b = np.asarray(q.reduced_density([1, 4])), np.asarray(q.reduced_density([4, 1]))
  swap = [0, 2, 1, 3]
  assert np.array_equal(b, a[np.ix_(swap, swap)])
  assert np.max(np.abs(a - b)) > 1e-3                                   # ... and the order matters on this state
  # against the 4^n route of this package, as the golden file was made
  want = ops.TraceOut(q.psi.density(), [0, 2, 3, 5])
  assert np.max(np.abs(a - np.asarray(want))) <= 4 * _eps(width)
  q.psi = (2.0 * psi).astype(tensor.tensor_type())
  q.x(0)
  q.x(0)
  assert abs(np.trace(np.asarray(q.reduced_density([0, 3]))).real - 4.0) <= 8 * _eps(width)
  assert abs(q.purity([0, 3]) - float(np.sum(np.abs(du.np_qubit_density(psi, [0, 3])) ** 2))) <= 8 * _eps(width)      # divided by the trace


def test_host_product_states_and_alias_mode_read_psi(cpu_backend):
  kind, width = cpu_backend
  reads = DensityOracle.reads
  q = _reg(3)                                                            # still a product state on the host
  assert np.asarray(q.reduced_density([1]))[0, 0] == 1.0
  backend.set_host_mapped_factory(DensityOracle)                         # alias mode: the state is the mapped buffer
  try:
    a = circuit.qc('a', alias_psi=True)
    a.reg(2, 0)
    a.h(0)
    a.cx(0, 1)
    assert abs(a.entropy([1]) - 1.0) <= 8 * _eps(width)
  finally:
    backend.set_host_mapped_factory(None)
  assert DensityOracle.reads == reads


def test_argument_errors(cpu_backend):
  q = _random_circuit(9, 2)
  psi = np.asarray(q.psi).copy()
  for bad in ([9], [-1], [0, 0], [1, 2, 1]):
    for method in (q.reduced_density, q.purity, q.entropy, q.schmidt_coefficients):
      with pytest.raises(ValueError):
        method(bad)
  with pytest.raises(ValueError, match='at most 8'):
    q.reduced_density(list(range(9)))
  with pytest.raises(ValueError):
    q.bloch(9)
  with pytest.raises(ValueError):
    q.mutual_information([0, 1], [1, 2])                                 # not disjoint
  with pytest.raises(ValueError, match='at most 8'):
    q.mutual_information([0, 1, 2, 3, 4], [5, 6, 7, 8])
  with pytest.raises(ValueError):
    q.mutual_information([0], [9])
  assert np.array_equal(np.asarray(q.psi), psi)
