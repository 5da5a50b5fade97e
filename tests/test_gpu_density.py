"""qh_reduced_density on the GPU against NumPy's complex128 A @ A^H on the DOWNLOADED state in logical order
(density_util.np_reduced_density), at both widths, in the permuted layouts relayout sweeps leave, with registers chosen by
PHYSICAL position through the bit map; its exact properties; the small shards of the gather path; one shape large enough
for the chunk and slab loops; attached, host-mapped and shard handles; and qc.entropy / purity / schmidt_coefficients /
mutual_information end to end.

Tolerance (derived, not measured): an entry is a sum of m = 2^(nbits_local - k) products formed in double from the stored
amplitudes; whatever the order, its error is at most 4 m 2^-53 sqrt(rho_rr rho_cc) (density_util.tolerance)."""
import ctypes

import numpy as np
import pytest

from qcc_amd import device, gates, native, workloads
from qcc_amd.lib import circuit, tensor
from tests import density_util as du

pytestmark = pytest.mark.gpu

_dp = ctypes.POINTER(ctypes.c_double)
_ip = ctypes.POINTER(ctypes.c_int32)
KMAX = native.QH_DENSITY_MAX_BITS


def _bitmap(st):
  bm = (ctypes.c_int32 * st.nbits)()
  native.check(st.lib.qh_get_bitmap(st.h, bm))
  return [int(b) for b in bm]


def _logical_state(st):
  """the whole state in LOGICAL order.  (A download brings the handle back to canonical order first: _reference below
  keeps the layout under test.)"""
  return du.logical_order(st.download().astype(np.complex128), _bitmap(st))


def _reference(st):
  """the state in logical order WITHOUT touching st's layout: the download of a clone"""
  with st.clone() as c:
    return _logical_state(c)


def _prepared(n, bw, fusion, seed):
  st = device.DeviceState(n, bw, fusion=fusion)
  ops, g8 = workloads.supremacy_stream(n, 12, seed=seed).arrays()
  st.init_basis(0)
  st.run_stream(ops, g8)
  st.flush()
  return st


def _random_state(n, seed):
  rng = np.random.default_rng(seed)
  v = rng.normal(size=1 << n) + 1j * rng.normal(size=1 << n)
  return v / np.linalg.norm(v)


def _check_exact(got):
  """rho[c][r] is the bitwise conjugate of rho[r][c]; diagonal imaginary parts are exactly +0.0"""
  off = ~np.eye(got.shape[0], dtype=bool)
  assert got.real.tobytes() == np.ascontiguousarray(got.real.T).tobytes()
  assert got.imag[off].tobytes() == (-got.imag.T)[off].tobytes()
  d = np.diag(got).imag
  assert np.all(d == 0.0) and not np.any(np.signbit(d))


def _check(st, psi, bits, what=''):
  """one call against NumPy on psi (the state in logical order), with every exact property; returns the matrix"""
  k = len(bits)
  k0 = st.stats()['kernels_launched']
  got = st.reduced_density(bits)
  assert st.stats()['kernels_launched'] == k0 + 1, (what, bits)
  want = du.np_reduced_density(psi, bits)
  tol = du.tolerance(want, 1 << (st.nbits - k))
  err = np.abs(got - want)
  assert np.all(err <= tol), (what, bits, float(np.max(err / np.maximum(tol, 1e-300))))
  _check_exact(got)
  again = st.reduced_density(bits)
  assert again.tobytes() == got.tobytes(), (what, bits)
  return got


def _placements(n, k, bm, rng):
  """registers by PHYSICAL position: the line bits, the lane positions, the top, a scattered mix; in shuffled list order"""
  inv = {p: b for b, p in enumerate(bm)}
  lane0 = min(3, n - k)
  sets = {'low': range(k), 'lane': range(lane0, lane0 + k), 'top': range(n - k, n), 'mix': sorted(int(p) for p in rng.permutation(n)[:k])}
  out = []
  for name, ps in sets.items():
    bits = [inv[p] for p in ps]
    if name != 'low':
      bits = [bits[j] for j in rng.permutation(k)]
    out.append((name, bits))
  return out


@pytest.mark.parametrize('fusion', [native.QH_FUSE_OFF, native.QH_FUSE_SWEEP])
@pytest.mark.parametrize('bw', [128, 64])
@pytest.mark.parametrize('n', [12, 16])
def test_every_k_and_placement(n, bw, fusion):
  rng = np.random.default_rng(100 * n + bw + fusion)
  with _prepared(n, bw, fusion, seed=n + fusion) as st:
    psi = _reference(st)
    bm = _bitmap(st)
    for k in range(KMAX + 1):
      for name, bits in _placements(n, k, bm, rng):
        got = _check(st, psi, bits, f'{name} k={k}')
        if k == 0:
          assert got.shape == (1, 1) and abs(got[0, 0].real - st.norm2()) <= 1e-12
    assert _bitmap(st) == bm and _logical_state(st).tobytes() == psi.tobytes()      # reads only: layout and state as before
  if fusion == native.QH_FUSE_SWEEP and n == 16:
    assert bm != list(range(n))                                              # relayout sweeps left a permuted bit map


@pytest.mark.parametrize('bw', [128, 64])
def test_runs_what_is_queued_first(bw):
  """gates still queued run first, and the walk is planned on the bit map that flush leaves, not on the one before it"""
  n = 16
  with device.DeviceState(n, bw, fusion=native.QH_FUSE_SWEEP) as st:
    ops, g8 = workloads.supremacy_stream(n, 12, seed=2).arrays()
    st.init_basis(0)
    st.run_stream(ops, g8)
    pend = ctypes.c_uint64()
    native.check(st.lib.qh_pending_gates(st.h, ctypes.byref(pend)))
    assert pend.value > 0
    before = _bitmap(st)
    bits = [15, 14, 13, 12, 11, 10, 9]
    got = st.reduced_density(bits)
    native.check(st.lib.qh_pending_gates(st.h, ctypes.byref(pend)))
    assert pend.value == 0 and _bitmap(st) != before
    want = du.np_reduced_density(_reference(st), bits)
    assert np.all(np.abs(got - want) <= du.tolerance(want, 1 << (n - 7)))


@pytest.mark.parametrize('bw', [128, 64])
def test_small_shards_gather_and_smallest_tiles(bw):
  """n = 1..9 with every k up to min(n, 8), k = n included: the gather path (n < 8) and the smallest tile shapes"""
  rng = np.random.default_rng(bw)
  paths = set()
  for n in range(1, 10):
    with device.DeviceState(n, bw) as st:
      st.upload(_random_state(n, 40 + n))
      if n >= 3:
        st.remap_swap(0, n - 1)                                              # a bit map that is not the identity
      psi = _reference(st)
      for k in range(min(n, KMAX) + 1):
        for _ in range(2):
          bits = [int(b) for b in rng.permutation(n)[:k]]
          paths.add(st.density_plan(bits)['path'])
          _check(st, psi, bits, f'n={n}')
  assert paths == {native.QH_DENSITY_TILES, native.QH_DENSITY_GATHER}


def _loop_size():
  """the smallest n in 20..24 at which, for k = 2, 6 and 8, a workgroup walks at least 2 chunks and a block pair has at
  least 2 slab rows -- read from qh_density_plan, not assumed"""
  for n in range(20, 25):
    with device.DeviceState(n, 128, dry=True) as st:
      plans = [st.density_plan(list(range(k))) for k in (2, 6, 8)]
    if all(p['chunks_per_wg'] >= 2 and p['wg_per_pair'] >= 2 for p in plans):
      return n
  return None


@pytest.mark.parametrize('bw', [128, 64])
def test_one_larger_shape_reaches_the_loops(bw):
  n = _loop_size()
  assert n is not None, 'no size in 20..24 walks two chunks per workgroup with two slab rows per pair'
  rng = np.random.default_rng(7)
  with _prepared(n, bw, native.QH_FUSE_SWEEP, seed=5) as st:
    psi = _reference(st)
    bm = _bitmap(st)
    assert bm != list(range(n))                                              # relayout sweeps left a permuted bit map
    inv = {p: b for b, p in enumerate(bm)}
    for k in (2, 6, 8):
      pos = sorted({0, 1} | {int(p) for p in rng.permutation(n)[:k]})[:k]     # line bits and a scattered rest
      bits = [inv[p] for p in pos]
      pl = st.density_plan(bits)
      assert pl['chunks_per_wg'] >= 2 and pl['wg_per_pair'] >= 2 and pl['block_pairs'] == (1, 1, 10)[(2, 6, 8).index(k)]
      s0 = st.stats()
      got = st.reduced_density(bits)
      s1 = st.stats()
      assert s1['kernels_launched'] == s0['kernels_launched'] + 1
      assert s1['bytes_algorithmic'] - s0['bytes_algorithmic'] == (16 if bw == 128 else 8) << n
      assert s1['bytes_swept'] - s0['bytes_swept'] == pl['amps_swept'] * (16 if bw == 128 else 8)
      want = du.np_reduced_density(psi, bits)
      assert np.all(np.abs(got - want) <= du.tolerance(want, 1 << (n - k))), k
      _check_exact(got)
      assert st.reduced_density(bits).tobytes() == got.tobytes()


@pytest.mark.parametrize('bw', [128, 64])
def test_exact_cases(bw):
  n = 13
  rng = np.random.default_rng(bw + 1)
  # a basis state: exactly one 1.0, zeros elsewhere
  with device.DeviceState(n, bw, fusion=native.QH_FUSE_SWEEP) as st:
    for j in (0, 1, 0b1011001110101, (1 << n) - 1):
      st.init_basis(j)
      for k in (0, 1, 3, 6, 7, 8):
        bits = [int(b) for b in rng.permutation(n)[:k]]
        got = st.reduced_density(bits)
        r = sum(((j >> b) & 1) << t for t, b in enumerate(bits))
        want = np.zeros((1 << k, 1 << k), dtype=np.complex128)
        want[r, r] = 1.0
        assert np.array_equal(got, want), (j, bits)
  with _prepared(n, bw, native.QH_FUSE_SWEEP, seed=9) as st:
    # the diagonal is the marginal, within the tolerance (the two sum in different orders)
    for k in (1, 4, 8):
      bits = [int(b) for b in rng.permutation(n)[:k]]
      got, marg = st.reduced_density(bits), st.marginal(bits)
      assert np.all(np.abs(np.diag(got).real - marg) <= 4.0 * (1 << (n - k)) * 2.0 ** -53 * marg), bits
    # projected on a register value and renormalised: rho is that projector
    bits = [int(b) for b in rng.permutation(n)[:5]]
    v = 0b10110
    mask = sum(1 << b for b in bits)
    value = sum(((v >> t) & 1) << b for t, b in enumerate(bits))
    p = st.marginal(bits)[v]
    assert p > 0
    st.project_bits(mask, value)
    st.scale(1.0 / np.sqrt(p))
    got = st.reduced_density(bits)
    want = np.zeros((32, 32))
    want[v, v] = 1.0
    assert np.array_equal(got != 0, want != 0)
    assert abs(got[v, v] - 1.0) <= (1e-12 if bw == 128 else 1e-6) and got[v, v].imag == 0.0


@pytest.mark.parametrize('kind', ['attached', 'host_mapped'])
def test_attached_and_host_mapped_handles(kind):
  n = 10
  v = _random_state(n, 3)
  bits = [9, 0, 4, 7, 2, 5, 8]

  def run(st, read):
    st.upload(v)
    st.apply1(gates.hadamard(), 3)
    st.sync()
    ptr = st.device_ptr
    held = read()
    psi = _reference(st)
    for k in (1, 3, 7):
      _check(st, psi, bits[:k], kind)
    assert st.device_ptr == ptr and read().tobytes() == held.tobytes()

  if kind == 'attached':
    with device.DeviceState(n, 128) as owner:
      with device.DeviceState(n, 128, device_ptr=owner.device_ptr) as att:
        run(att, owner.download)
  else:
    with device.DeviceState(n, 128, host_mapped=True) as st:
      run(st, lambda: st.host_array().copy())


@pytest.mark.parametrize('bw', [128, 64])
def test_shard_handles_on_one_gpu(bw):
  """four shards of a 12-qubit state behind four handles: with local registers the shards' results add up to the unsharded
  rho; a listed shard bit is QH_ERR_NONLOCAL and out keeps its sentinel"""
  nl, n = 10, 12
  v = _random_state(n, 21).astype(np.complex128 if bw == 128 else np.complex64)
  full = v.astype(np.complex128)
  lib = native.load()
  regs = [[0], [9, 3], [2, 7, 8, 1], [0, 1, 2, 3, 4, 5, 6, 9]]
  sums = [np.zeros((1 << len(r), 1 << len(r)), dtype=np.complex128) for r in regs]
  for shard in range(4):
    with device.DeviceState(nl, bw) as st:
      st.set_shard(n, shard)
      st.upload(v[shard << nl:(shard + 1) << nl])
      for s, r in zip(sums, regs):
        got = st.reduced_density(r)
        _check_exact(got)
        s += got
      k0 = st.stats()['kernels_launched']
      for bad in ([10], [3, 11], [11, 10, 0]):
        out = np.full(2 << (2 * len(bad)), -7.25)
        b = np.asarray(bad, dtype=np.int32)
        assert lib.qh_reduced_density(st.h, len(bad), b.ctypes.data_as(_ip), out.ctypes.data_as(_dp)) == native.QH_ERR_NONLOCAL
        assert np.all(out == -7.25)
      assert st.stats()['kernels_launched'] == k0
  for s, r in zip(sums, regs):
    want = du.np_reduced_density(full, r)
    assert np.all(np.abs(s - want) <= du.tolerance(want, 1 << (n - len(r)))), r


# ---- qc end to end -----------------------------------------------------------------------------------------------------
def _device_reads(q, fn):
  """fn() with nothing queued: (its result, the growth of kernels_launched on the circuit's device) -- 0 would mean that
  the circuit read qc.psi with NumPy instead"""
  q.norm2()                                                                    # (runs what is queued)
  dev = q._dev                                                                 # pylint: disable=protected-access
  k0 = dev.stats()['kernels_launched']
  out = fn()
  return out, q._dev.stats()['kernels_launched'] - k0                          # pylint: disable=protected-access


@pytest.mark.parametrize('width', [128, 64])
def test_qc_quantities_against_numpy_on_psi(width):
  tensor.set_tensor_width(width)
  try:
    n = 16
    rng = np.random.default_rng(31)
    q = circuit.qc('d')
    q.reg(n, 0)
    for _ in range(4 * n):
      a = int(rng.integers(n))
      q.ry(a, float(rng.random() * 3))
      b = int(rng.integers(n))
      if b != a:
        q.cx(a, b)
      q.rz(int(rng.integers(n)), float(rng.random() * 3))
    psi = np.asarray(q.psi).reshape(-1).astype(np.complex128)
    eps = 1e-10 if width == 128 else 2e-5
    for qubits in ([0], [15, 3], [4, 5, 6], [1, 14, 7, 9, 2], [0, 2, 4, 6, 8, 10, 12, 14]):
      rho = du.np_qubit_density(psi, qubits)
      rho /= np.trace(rho).real
      got, reads = _device_reads(q, lambda: np.asarray(q.reduced_density(qubits)))      # pylint: disable=cell-var-from-loop
      assert reads == 1                                                        # the device path, one read of the state
      assert np.max(np.abs(got * (1.0 / q.norm2()) - rho)) <= eps
      pur, reads = _device_reads(q, lambda: q.purity(qubits))                  # pylint: disable=cell-var-from-loop
      assert reads == 1 and abs(pur - float(np.sum(np.abs(rho) ** 2))) <= eps
      assert abs(q.entropy(qubits) - du.entropy(rho)) <= 100 * eps
      ev = np.sqrt(np.clip(np.linalg.eigvalsh(rho)[::-1], 0, None))
      assert np.max(np.abs(q.schmidt_coefficients(qubits) - ev)) <= (1e-7 if width == 128 else 1e-3)
    want = du.entropy(du.np_qubit_density(psi, [2, 3])) + du.entropy(du.np_qubit_density(psi, [11])) - du.entropy(du.np_qubit_density(psi, [2, 3, 11]))
    mi, reads = _device_reads(q, lambda: q.mutual_information([2, 3], [11]))
    assert reads == 3 and abs(mi - want) <= 300 * eps
    with pytest.raises(ValueError):
      q.reduced_density(list(range(9)))
  finally:
    tensor.set_tensor_width(None)


def test_qc_qft_on_half_of_a_bell_paired_register():
  """m Bell pairs (i, m + i), then a QFT on the first half: a unitary on one side of the cut leaves its entropy at m bits"""
  m = 7
  tensor.set_tensor_width(128)
  try:
    _bell_qft(m)
  finally:
    tensor.set_tensor_width(None)


def _bell_qft(m):
  q = circuit.qc('bell')
  q.reg(2 * m, 0)
  for i in range(m):
    q.h(i)
    q.cx(i, m + i)
  assert abs(q.mutual_information([1], [m + 1]) - 2.0) <= 1e-9 and abs(q.mutual_information([1], [m + 2])) <= 1e-9
  q.qft(list(range(m)))
  half = list(range(m))
  ent, reads = _device_reads(q, lambda: q.entropy(half))
  assert reads == 1 and abs(ent - m) <= 1e-9
  assert abs(q.purity(half) - 2.0 ** -m) <= 1e-12
  assert np.max(np.abs(q.schmidt_coefficients(half) - 2.0 ** (-m / 2))) <= 1e-9
  assert abs(q.entropy([0]) - 1.0) <= 1e-9 and abs(q.entropy([m + 2]) - 1.0) <= 1e-9
  assert np.max(np.abs(q.bloch(3))) <= 1e-12
