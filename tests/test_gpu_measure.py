"""Register readout on the MI355X: qh_marginal, qh_sample and qh_project_bits against NumPy on the downloaded state.

Small registers (n = 4-20, both widths, per-gate and fused runs that leave a permuted bit map), the exact inverse CDF in
physical order, a G-test of a seeded 2^20-shot histogram, qc.probabilities / sample / measure (host-mapped registers
too), and whole 30-qubit states: a k = 16 marginal of supremacy-30 against a chunked host reduction, the uniform
marginal of a QFT, GHZ shots, and readers that leave the state as it was."""
import math

import numpy as np
import pytest

from qcc_amd import device, gates, native, workloads
from qcc_amd.lib import circuit, tensor
from tests.shard_util import bitmap as _bitmap, check_exact_cdf, logical_of_phys as _logical_of_phys
from tests.test_dense_cpu import dense_reference
from tests.test_gpu_expect import _np_expect
from tests.test_mux_cpu import diag_reference

pytestmark = pytest.mark.gpu

def _logical_state(st):
  """the whole (small) state in LOGICAL order, whatever layout the download leaves"""
  phys = st.download().astype(np.complex128)
  out = np.empty_like(phys)
  out[_logical_of_phys(_bitmap(st), phys.size).astype(np.int64)] = phys
  return out


def _np_marginal(p, bits):
  idx = np.arange(p.size, dtype=np.uint64)
  j = np.zeros_like(idx)
  for t, b in enumerate(bits):
    j |= ((idx >> np.uint64(b)) & np.uint64(1)) << np.uint64(t)
  return np.bincount(j.astype(np.int64), weights=p, minlength=1 << len(bits))


def _check_marginal(got, want, bw):
  if bw == 128:
    assert float(np.max(np.abs(got - want))) < 1e-12
  else:
    assert float(np.max(np.abs(got - want))) <= 1e-6 * max(float(np.max(want)), 1e-30) + 1e-9


def _prepared(n, bw, fusion, seed):
  """a dense random state from a gate stream (fused runs leave a permuted bit map)"""
  st = device.DeviceState(n, bw, fusion=fusion)
  ops, g8 = workloads.supremacy_stream(n, 12, seed=seed).arrays()
  st.init_basis(0)
  st.run_stream(ops, g8)
  st.flush()
  return st


def _bit_sets(rng, n):
  sets = []
  for k in range(1, min(n, 16) + 1):
    sets.append([int(b) for b in rng.permutation(n)[:k]])
  sets.append([b for b in (0, 1, 2) if b < n])                       # line bits
  sets.append([b for b in range(3, 9) if b < n] or [0])              # lane bits
  sets.append(list(range(max(0, n - 3), n)))                         # top bits
  sets.append(sorted({0, n // 2, n - 1}))
  return sets


@pytest.mark.parametrize('bw', [128, 64])
@pytest.mark.parametrize('fusion', [native.QH_FUSE_OFF, native.QH_FUSE_SWEEP])
def test_marginal_small_registers(bw, fusion):
  rng = np.random.default_rng(bw + fusion)
  permuted = []
  for n in (4, 7, 12, 15, 20):
    with _prepared(n, bw, fusion, seed=n) as st:
      permuted.append(_bitmap(st) != list(range(n)))
      sets = _bit_sets(rng, n)
      got = [st.marginal(bits) for bits in sets]               # all in the layout the flush left
      again = [st.marginal(bits) for bits in sets]
      for a, b in zip(got, again):
        assert a.tobytes() == b.tobytes()                      # bitwise reproducible
      norm = st.marginal([])
      assert norm.shape == (1,)
      p = np.abs(_logical_state(st)) ** 2
    assert abs(norm[0] - p.sum()) < (1e-12 if bw == 128 else 1e-6)
    for bits, m in zip(sets, got):
      _check_marginal(m, _np_marginal(p, bits), bw)
  if fusion == native.QH_FUSE_SWEEP:
    assert any(permuted), permuted                      # relayout sweeps left a permuted bit map in some case


def test_marginal_argument_errors_on_a_real_handle():
  with device.DeviceState(8, 128) as st:
    st.init_basis(3)
    for bits, code in (([8], native.QH_ERR_BAD_QUBIT), ([1, 1], native.QH_ERR_SAME_QUBIT), (list(range(8)) * 3, native.QH_ERR_ARG)):
      with pytest.raises(native.QhError) as e:
        st.marginal(bits)
      assert e.value.code == code
    assert st.marginal([0, 1]).tolist() == [0.0, 0.0, 0.0, 1.0]


def _check_shots(bm, lstate, got, u):
  """shots `got` for the uniforms u against the inverse CDF of the state in physical order under the bit map bm"""
  lphys = _logical_of_phys(bm, lstate.size).astype(np.int64)       # logical index of each physical one
  pp = np.abs(lstate[lphys]) ** 2
  phys_of_logical = np.empty(lstate.size, dtype=np.int64)
  phys_of_logical[lphys] = np.arange(lstate.size)
  check_exact_cdf(pp, phys_of_logical[got.astype(np.int64)], u)


def _check_exact_cdf(st, u):
  """qh_sample against the inverse CDF of the state in the engine's physical order (bit map before the download)"""
  bm = _bitmap(st)
  got = st.sample(u)
  lstate = _logical_state(st)
  _check_shots(bm, lstate, got, u)
  return got, lstate


@pytest.mark.parametrize('bw', [128, 64])
@pytest.mark.parametrize('n', [5, 12, 17])
def test_sample_is_the_exact_inverse_cdf(bw, n):
  rng = np.random.default_rng(n * bw)
  with _prepared(n, bw, native.QH_FUSE_SWEEP, seed=100 + n) as st:
    u = np.sort(np.concatenate([rng.random(3000), [0.0, np.nextafter(1.0, 0.0), 0.5]]))
    _check_exact_cdf(st, u)
    assert st.sample(np.zeros(0)).size == 0
    for bad in ([0.5, 0.2], [1.0], [-0.1]):
      with pytest.raises(native.QhError):
        st.sample(np.asarray(bad))


def test_sample_basis_state_and_sparse_states():
  with device.DeviceState(13, 128, fusion=native.QH_FUSE_SWEEP) as st:
    st.init_basis(0x1a5b)
    got = st.sample(np.sort(np.random.default_rng(0).random(5000)))
    assert set(got.tolist()) == {0x1a5b}
    st.scale(0.0)
    with pytest.raises(native.QhError):
      st.sample(np.asarray([0.25]))
  # a sparse state: few nonzero amplitudes among zeros, edges of the CDF included
  with device.DeviceState(14, 64, fusion=native.QH_FUSE_OFF) as st:
    v = np.zeros(1 << 14, dtype=np.complex64)
    v[[3, 4097, 9000, 16383]] = [0.5, 0.5j, -0.5, 0.5]
    st.upload(v)
    u = np.sort(np.concatenate([np.random.default_rng(1).random(4000), [0.0, 0.25, 0.5, 0.75, np.nextafter(1.0, 0.0)]]))
    got, _ = _check_exact_cdf(st, u)
    assert set(got.tolist()) == {3, 4097, 9000, 16383}


@pytest.mark.parametrize('bw', [128, 64])
def test_readers_share_one_scratch_buffer_on_one_handle(bw):
  """The readers carve one scratch buffer whose required size goes up and down between calls, and the staged uploads of
  qh_apply_matrix (a ring) and qh_apply_diag (one slot) interleave: no region aliases another, no slot is overwritten early."""
  n = 12
  rng = np.random.default_rng(4000 + bw)
  full = (1 << n) - 1
  rnd = lambda: int(rng.integers(0, 1 << n))      # noqa: E731
  x0, x1 = rnd() | (1 << (n - 1)), rnd() & (full >> 1)          # two distinct x masks; 20 strings on the first: two batches
  xs = [x0] * 20 + [x1] * 12 + [rnd() for _ in range(8)]
  zs = [rnd() for _ in range(40)]
  u_many, u_few = np.sort(rng.random(4096)), np.sort(rng.random(3))
  b2, b11 = [int(b) for b in rng.permutation(n)[:2]], [int(b) for b in rng.permutation(n)[:11]]
  with _prepared(n, bw, native.QH_FUSE_SWEEP, seed=200 + bw) as st:
    bm = _bitmap(st)
    m2 = st.marginal(b2)
    s_many = st.sample(u_many)
    e40 = st.expect_pauli(xs, zs)
    m11 = st.marginal(b11)
    s_few = st.sample(u_few)
    e1 = st.expect_pauli(xs[-1:], zs[-1:])
    m0 = st.marginal([])
    assert _bitmap(st) == bm                                    # readers only: the layout they all ran on
    a = _logical_state(st)
    p = np.abs(a) ** 2
    _check_marginal(m2, _np_marginal(p, b2), bw)
    _check_marginal(m11, _np_marginal(p, b11), bw)
    assert m0.shape == (1,) and abs(m0[0] - p.sum()) < (1e-12 if bw == 128 else 1e-6)
    _check_shots(bm, a, s_many, u_many)
    _check_shots(bm, a, s_few, u_few)
    want = np.array([_np_expect(a, x, z) for x, z in zip(xs, zs)])
    assert float(np.max(np.abs(e40 - want))) < 1e-12            # (double accumulation at both widths: tests/test_gpu_expect.py)
    assert abs(e1[0] - want[-1]) < 1e-12
    # three matrices (k = 2) and three diagonals (k = 3), interleaved, nothing read in between
    for _ in range(3):
      mb, db = [int(b) for b in rng.permutation(n)[:2]], [int(b) for b in rng.permutation(n)[:3]]
      m, _r = np.linalg.qr(rng.normal(size=(4, 4)) + 1j * rng.normal(size=(4, 4)))
      v = np.exp(2j * np.pi * rng.random(8))
      st.apply_matrix(m, mb)
      st.apply_diag(v, db)
      a = diag_reference(dense_reference(a, n, m, mb), n, v, db)
    got = _logical_state(st)
  if bw == 128:                                                 # (tests/test_gpu_dense.py::_check)
    assert float(np.max(np.abs(got - a))) < 1e-12
  else:
    assert float(np.linalg.norm(got - a) / np.linalg.norm(a)) < 1e-5


def test_seeded_histogram_passes_a_g_test():
  n, shots = 10, 1 << 20
  rng = np.random.default_rng(20)
  v = rng.normal(size=1 << n) + 1j * rng.normal(size=1 << n)
  v /= np.linalg.norm(v)
  with device.DeviceState(n, 128) as st:
    st.upload(v)
    u = np.sort(np.random.default_rng(12345).random(shots))
    got = st.sample(u)
  obs = np.bincount(got.astype(np.int64), minlength=1 << n)
  exp = np.abs(v) ** 2 * shots
  nz = obs > 0
  g = 2.0 * float(np.sum(obs[nz] * np.log(obs[nz] / exp[nz])))
  df = (1 << n) - 1                       # chi-square tail by the Wilson-Hilferty cube-root normal approximation
  z = ((g / df) ** (1 / 3) - (1 - 2 / (9 * df))) / math.sqrt(2 / (9 * df))
  pval = 0.5 * math.erfc(z / math.sqrt(2))
  print(f'G = {g:.1f} on {(1 << n) - 1} dof, p = {pval:.3g}')
  assert pval > 1e-6


def _random_circuit(nq, seed, alias=False):
  rng = np.random.default_rng(seed)
  q = circuit.qc('m', alias_psi=alias)
  q.reg(nq, 0)
  for _ in range(4 * nq):
    a = int(rng.integers(nq))
    q.ry(a, float(rng.random() * 3))
    b = int(rng.integers(nq))
    if b != a:
      q.cx(a, b)
    q.rz(int(rng.integers(nq)), float(rng.random() * 3))
  return q


@pytest.mark.parametrize('alias', [False, True])
@pytest.mark.parametrize('nq', [3, 4, 6])
def test_qc_measure_collapses_like_numpy(nq, alias):
  tensor.set_tensor_width(128)
  try:
    rng = np.random.default_rng(nq)
    for trial in range(3):
      q = _random_circuit(nq, 10 * nq + trial, alias)
      psi = np.asarray(q.psi, dtype=np.complex128).copy()
      qubits = [int(x) for x in rng.permutation(nq)[:int(rng.integers(1, nq + 1))]]
      k = len(qubits)
      t = psi.reshape([2] * nq)
      pm = np.abs(np.moveaxis(t, qubits, list(range(k)))) ** 2
      probs = pm.reshape(1 << k, -1).sum(axis=1)
      np.testing.assert_allclose(q.probabilities(qubits), probs, atol=1e-12)
      value, prob = q.measure(qubits, seed=trial)
      assert abs(prob - probs[value]) < 1e-12
      idx = np.arange(1 << nq)
      keep = np.ones(1 << nq, dtype=bool)
      for j, qb in enumerate(qubits):
        keep &= ((idx >> (nq - 1 - qb)) & 1) == ((value >> (k - 1 - j)) & 1)
      want = np.where(keep, psi, 0) / np.sqrt(prob)
      got = np.asarray(q.psi, dtype=np.complex128)
      assert float(np.max(np.abs(got - want))) < 1e-12
      assert abs(float(np.vdot(got, got).real) - 1.0) < 1e-12
      q.close()
  finally:
    tensor.set_tensor_width(None)


def test_qc_sample_seeds_and_draw_order():
  tensor.set_tensor_width(128)
  try:
    q = _random_circuit(8, 77)
    a = q.sample(4000, [7, 0, 3], seed=5)
    b = q.sample(4000, [7, 0, 3], seed=5)
    assert a.tolist() == b.tolist()
    full = q.sample(4000, seed=5)                  # the same uniforms: the register is the bits of the full shot
    reg = ((full >> np.uint64(0)) & np.uint64(1)) << np.uint64(2) | ((full >> np.uint64(7)) & np.uint64(1)) << np.uint64(1) | \
        ((full >> np.uint64(4)) & np.uint64(1))
    assert reg.tolist() == a.tolist()
    np.random.seed(3)
    c = q.sample(100)
    np.random.seed(3)
    assert q.sample(100).tolist() == c.tolist()
    q.close()
  finally:
    tensor.set_tensor_width(None)


# ---- whole 30-qubit states ---------------------------------------------------------------------------------------------
def _host_marginal_chunked(st, bits, chunk_bits=26):
  """marginal of LOGICAL bits from qh_download, 2^chunk_bits amplitudes at a time"""
  n = st.nbits
  out = np.zeros(1 << len(bits))
  buf = np.empty(1 << chunk_bits, dtype=st.dtype)
  st.download(0, 1 << chunk_bits, out=buf)       # (a download may bring the layout back to canonical order first)
  bm = _bitmap(st)
  low = np.zeros(1 << chunk_bits, dtype=np.int64)
  i = np.arange(1 << chunk_bits, dtype=np.int64)
  for t, b in enumerate(bits):
    if bm[b] < chunk_bits:
      low |= ((i >> bm[b]) & 1) << t
  del i
  for c in range(1 << (n - chunk_bits)):
    if c:
      st.download(c << chunk_bits, 1 << chunk_bits, out=buf)
    hi = 0
    for t, b in enumerate(bits):
      if bm[b] >= chunk_bits and ((c << chunk_bits) >> bm[b]) & 1:
        hi |= 1 << t
    p = buf.real.astype(np.float64) ** 2 + buf.imag.astype(np.float64) ** 2
    out += np.bincount(low | hi, weights=p, minlength=out.size)
  return out


def test_supremacy30_marginal_and_readers_leave_the_state():
  n = 30
  ops, g8 = workloads.supremacy_stream(n, 20, seed=0).arrays()
  bits = [0, 1, 2, 4, 6, 8, 11, 13, 15, 17, 19, 21, 24, 26, 28, 29]
  with device.DeviceState(n, 128, fusion=native.QH_FUSE_SWEEP) as st:
    st.init_basis(0)
    st.run_stream(ops, g8)
    st.flush()
    assert _bitmap(st) != list(range(n))                # the readers below run on a permuted layout
    n0, a0, amps0 = st.marginal([]), st.argmax(), [st.amplitude(i) for i in (0, 12345, 1 << 29, (1 << 30) - 1)]
    m = st.marginal(bits)
    st.sample(np.sort(np.random.default_rng(0).random(100000)))
    st.marginal([3, 29])
    assert st.marginal([]).tobytes() == n0.tobytes()          # (norm2 and marginal([]) sum in different orders: compare to 1e-14)
    assert abs(st.norm2() - n0[0]) < 1e-14
    assert [st.amplitude(i) for i in (0, 12345, 1 << 29, (1 << 30) - 1)] == amps0
    assert st.argmax() == a0
    want = _host_marginal_chunked(st, bits)
  assert float(np.max(np.abs(m - want))) < 1e-12
  assert abs(m.sum() - 1.0) < 1e-12


def test_qft30_uniform_marginal_and_ghz30_shots():
  n = 30
  ops, g8 = workloads.qft_stream(range(n)).arrays()
  with device.DeviceState(n, 128, fusion=native.QH_FUSE_SWEEP) as st:
    st.init_basis(0x2345678)
    st.run_stream(ops, g8)
    st.flush()
    assert _bitmap(st) != list(range(n))
    m = st.marginal([0, 2, 5, 7, 9, 10, 12, 14, 16, 18, 20, 22, 25, 27, 28, 29])
    assert float(np.max(np.abs(m - 2.0 ** -16))) < 1e-15
    # GHZ: H on qubit 0, CNOT 0 -> every other qubit
    st.init_basis(0)
    st.apply1(gates.hadamard(), 0)
    for q in range(1, n):
      st.applyc(gates.pauli_x(), 0, q)
    got = st.sample(np.sort(np.random.default_rng(3).random(20000)))
    vals = set(got.tolist())
    assert vals == {0, (1 << n) - 1}
    frac = float(np.mean(got == 0))
    assert 0.45 < frac < 0.55
    np.testing.assert_allclose(st.marginal([0, 29, 15]), [0.5, 0, 0, 0, 0, 0, 0, 0.5], atol=1e-14)
    st.project_bits(1 << 29, 1 << 29)
    assert abs(st.norm2() - 0.5) < 1e-14
    assert st.amplitude(0) == 0

