"""Pauli-string expectations on the MI355X: qh_expect_pauli against the formula in NumPy on the downloaded state.

Small registers (n = 4-20, both widths, per-gate and fused runs that leave a permuted bit map; strings chosen by the
PHYSICAL position of their X bits), batching and the read counter, shard semantics on one GPU, qc.expectation end to end
(host-mapped registers too), and whole 30-qubit states: product states, GHZ, and supremacy-30 against qh_marginal."""
import ctypes
import math

import numpy as np
import pytest

from qcc_amd import device, gates, native, workloads
from qcc_amd.lib import circuit, tensor

pytestmark = pytest.mark.gpu

T = 16      # strings per read of the state (include/qcc_hip.h: qh_expect_pauli)


def _bitmap(st):
  bm = (ctypes.c_int32 * st.nbits)()
  native.check(st.lib.qh_get_bitmap(st.h, bm))
  return [int(b) for b in bm]


def _logical_state(st):
  """the whole (small) state in LOGICAL order, whatever layout the download leaves"""
  phys = st.download().astype(np.complex128)
  bm = _bitmap(st)
  i = np.arange(phys.size, dtype=np.uint64)
  lo = np.zeros_like(i)
  for b, p in enumerate(bm):
    lo |= ((i >> np.uint64(p)) & np.uint64(1)) << np.uint64(b)
  out = np.empty_like(phys)
  out[lo.astype(np.int64)] = phys
  return out


def _np_expect(a, x, z):
  """Re[(-i)^nY sum_i conj(a_i) (-1)^popcount(i & z) a_{i ^ x}] (the issue's formula), a in logical order"""
  idx = np.arange(a.size, dtype=np.uint64)
  par = np.zeros(a.size, dtype=np.uint64)
  for b in range(a.size.bit_length() - 1):
    if (int(z) >> b) & 1:
      par ^= (idx >> np.uint64(b)) & np.uint64(1)
  s = np.sum(np.conj(a) * (1.0 - 2.0 * par.astype(np.float64)) * a[(idx ^ np.uint64(x)).astype(np.int64)])
  return float(((-1j) ** (bin(int(x) & int(z)).count('1') % 4) * s).real)


def _reads(xs):
  """reads of the state the engine needs: per distinct x mask, ceil(terms / T)"""
  return sum(-(-list(xs).count(x) // T) for x in set(xs))


def _prepared(n, bw, fusion, seed):
  st = device.DeviceState(n, bw, fusion=fusion)
  ops, g8 = workloads.supremacy_stream(n, 12, seed=seed).arrays()
  st.init_basis(0)
  st.run_stream(ops, g8)
  st.flush()
  return st


def _mask(bits):
  m = 0
  for b in bits:
    m |= 1 << int(b)
  return m


def _string_sets(rng, n, bm):
  """(name, xmasks, zmasks) over LOGICAL bits; X positions picked by PHYSICAL position through the bit map bm"""
  full = (1 << n) - 1
  logical_of = {p: b for b, p in enumerate(bm)}
  phys = lambda ps: _mask(logical_of[p] for p in ps if p < n)      # noqa: E731
  rnd = lambda: int(rng.integers(0, 1 << n))                       # noqa: E731
  sets = [('random', [rnd() for _ in range(12)], [rnd() for _ in range(12)]),
          ('all-Z', [0] * 6, [full, 1, 1 << (n - 1), rnd(), rnd(), rnd()]),
          ('identity', [0], [0]),
          ('line', [phys([0]), phys([1]), phys([2]), phys([0, 1, 2]), phys([0, 2])], [0, rnd(), rnd(), full, phys([0])]),
          ('lane', [phys([3]), phys([4, 5]), phys([3, 4, 5]), phys([0, 5])], [rnd(), 0, full, rnd()]),
          ('top', [phys([n - 1]), phys([n - 1, n - 2, n - 3]), phys([n - 1, 0]), phys([n - 2, 3, 1])], [rnd(), full, rnd(), 0]),
          ('weight-n', [full, full, full, rnd() | 1], [0, full, rnd(), full])]
  xs = rnd() | (1 << (n - 1))
  sets.append(('shared-x', [xs] * (2 * T + 5), [rnd() for _ in range(2 * T + 5)]))      # more than T: batching is crossed
  sets.append(('shared-x0', [0] * (T + 3), [rnd() for _ in range(T + 3)]))
  many = sorted({rnd() for _ in range(24)})
  sets.append(('distinct-x', many + many[:7], [rnd() for _ in range(len(many) + 7)]))
  return sets


@pytest.mark.parametrize('bw', [128, 64])
@pytest.mark.parametrize('fusion', [native.QH_FUSE_OFF, native.QH_FUSE_SWEEP])
def test_expect_small_registers(bw, fusion):
  rng = np.random.default_rng(1000 + bw + fusion)
  permuted = []
  worst = 0.0
  for n in (4, 7, 12, 15, 20):
    with _prepared(n, bw, fusion, seed=n) as st:
      bm = _bitmap(st)
      permuted.append(bm != list(range(n)))
      sets = _string_sets(rng, n, bm)
      norm0 = st.marginal([])
      got = []
      for name, xs, zs in sets:
        k0 = st.stats()['kernels_launched']
        got.append(st.expect_pauli(xs, zs))
        assert st.stats()['kernels_launched'] - k0 == _reads(xs), name      # one read of the state per batch
      again = [st.expect_pauli(xs, zs) for _, xs, zs in sets]
      for a, b in zip(got, again):
        assert a.tobytes() == b.tobytes()                                     # bitwise reproducible
      ident = st.expect_pauli([0], [0])
      assert _bitmap(st) == bm                                                # reads only: bit map and norm as before
      assert st.marginal([]).tobytes() == norm0.tobytes()
      assert abs(ident[0] - norm0[0]) < 1e-12
      assert st.expect_pauli([], []).shape == (0,)
      a = _logical_state(st)
    for (name, xs, zs), g in zip(sets, got):
      want = np.array([_np_expect(a, x, z) for x, z in zip(xs, zs)])
      err = float(np.max(np.abs(g - want)))
      worst = max(worst, err)
      # the kernel accumulates in double from the stored amplitudes, as the NumPy sum does: both widths meet 1e-12
      assert err < 1e-12, (n, name, err)
  print(f'bw={bw} fusion={fusion}: max |gpu - numpy| = {worst:.3e}')
  if fusion == native.QH_FUSE_SWEEP:
    assert any(permuted), permuted                      # relayout sweeps left a permuted bit map in some case


def test_expect_leaves_the_state_bitwise():
  with _prepared(14, 128, native.QH_FUSE_SWEEP, seed=3) as st:
    rng = np.random.default_rng(5)
    before = _logical_state(st)
    st.expect_pauli([int(v) for v in rng.integers(0, 1 << 14, size=40)], [int(v) for v in rng.integers(0, 1 << 14, size=40)])
    after = _logical_state(st)
  assert before.tobytes() == after.tobytes()


def test_expect_argument_errors_on_a_real_handle():
  with device.DeviceState(8, 128) as st:
    st.init_basis(3)
    for xs, zs in (([1 << 8], [0]), ([0, 1], [0, 1 << 20])):
      with pytest.raises(native.QhError) as e:
        st.expect_pauli(xs, zs)
      assert e.value.code == native.QH_ERR_BAD_QUBIT
    assert st.expect_pauli([0, 0, 0], [1, 2, 4]).tolist() == [-1.0, -1.0, 1.0]       # |00000011>


def test_shard_semantics_on_one_gpu():
  n = 9
  rng = np.random.default_rng(9)
  v = rng.normal(size=1 << n) + 1j * rng.normal(size=1 << n)
  v /= np.linalg.norm(v)
  zs = [0, 0b101, (1 << n) - 1, 0b110011]
  xs = [0b11, 0b11, 1 << (n - 1), 0]
  for shard in range(4):
    with device.DeviceState(n, 128) as st:
      st.set_shard(n + 2, shard)
      st.upload(v)
      base = st.expect_pauli(xs, zs)
      np.testing.assert_allclose(base, [_np_expect(v, x, z) for x, z in zip(xs, zs)], atol=1e-12)
      lo = st.expect_pauli(xs, [z | (1 << n) for z in zs])                 # Z on shard bit 0: a sign on odd shards
      hi = st.expect_pauli(xs, [z | (3 << n) for z in zs])
      assert lo.tolist() == ((-base) if shard & 1 else base).tolist()
      assert hi.tolist() == ((-base) if bin(shard).count('1') & 1 else base).tolist()
      k0 = st.stats()['kernels_launched']
      with pytest.raises(native.QhError) as e:
        st.expect_pauli([1, 1 << n], [0, 0])                               # X on a shard bit: nothing is computed
      assert e.value.code == native.QH_ERR_NONLOCAL
      assert st.stats()['kernels_launched'] == k0


# ---- qc.expectation end to end ---------------------------------------------------------------------------------------------
def _random_circuit(nq, seed, alias=False):
  rng = np.random.default_rng(seed)
  q = circuit.qc('e', alias_psi=alias)
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
def test_qc_maxcut_sums_equal_diagonal_times_probabilities(alias):
  tensor.set_tensor_width(128)
  try:
    nq = 8
    q = _random_circuit(nq, 31, alias)
    rng = np.random.default_rng(2)
    edges = [(i, j, float(rng.random())) for i in range(nq) for j in range(i + 1, nq) if rng.random() < 0.6]
    got = q.expectation([(w, {i: 'Z', j: 'Z'}) for i, j, w in edges])
    probs = q.probabilities(list(range(nq)))             # register value v: qubit 0 is its most significant bit
    v = np.arange(1 << nq)
    diag = np.zeros(1 << nq)
    for i, j, w in edges:
      diag += w * (1 - 2 * ((v >> (nq - 1 - i)) & 1)) * (1 - 2 * ((v >> (nq - 1 - j)) & 1))
    assert abs(got - float(np.dot(diag, probs))) < 1e-12
    q.close()
  finally:
    tensor.set_tensor_width(None)


@pytest.mark.parametrize('alias', [False, True])
def test_qc_two_qubit_vqe_hamiltonian(alias):
  tensor.set_tensor_width(128)
  try:
    pauli = {'I': np.eye(2), 'X': np.array([[0, 1], [1, 0]]), 'Y': np.array([[0, -1j], [1j, 0]]), 'Z': np.diag([1.0, -1.0])}
    terms = [(0.4, 'ZI'), (-0.7, 'IZ'), (0.3, 'XX'), (0.25, 'YY'), (-0.15, 'ZZ'), (0.2, 'XZ'), (0.1, 'YI'), (1.1, 'II')]
    hmat = sum(c * np.kron(pauli[s[0]], pauli[s[1]]) for c, s in terms)
    evals = np.linalg.eigvalsh(hmat)
    for seed in range(4):
      q = _random_circuit(2, 50 + seed, alias)
      psi = np.asarray(q.psi, dtype=np.complex128).copy()
      e = q.expectation(terms)
      assert abs(e - float(np.vdot(psi, hmat @ psi).real)) < 1e-12
      assert evals[0] - 1e-12 <= e <= evals[-1] + 1e-12
      per = q.expectation(terms, per_term=True)
      for (c, s), p in zip(terms, per):
        assert abs(p - float(np.vdot(psi, np.kron(pauli[s[0]], pauli[s[1]]) @ psi).real)) < 1e-12
      q.close()
  finally:
    tensor.set_tensor_width(None)


# ---- whole 30-qubit states (one alive at a time) ---------------------------------------------------------------------------
def _signed(m):
  """sum_j (-1)^popcount(j) m[j]: the Z string on the marginal's bits"""
  j = np.arange(m.size)
  par = np.zeros(m.size, dtype=np.int64)
  for b in range(m.size.bit_length() - 1):
    par ^= (j >> b) & 1
  return float(np.sum((1.0 - 2.0 * par) * m))


def test_product_state_30():
  n = 30
  rng = np.random.default_rng(30)
  f = rng.normal(size=(n, 2)) + 1j * rng.normal(size=(n, 2))
  f /= np.linalg.norm(f, axis=1, keepdims=True)
  pauli = {'X': np.array([[0, 1], [1, 0]]), 'Y': np.array([[0, -1j], [1j, 0]]), 'Z': np.diag([1.0, -1.0])}
  one = {c: [float(np.vdot(f[q], m @ f[q]).real) for q in range(n)] for c, m in pauli.items()}     # factor q = qubit q
  strings = [{29: 'X'}, {28: 'Y'}, {27: 'Z'}, {25: 'X'}, {22: 'Y'}, {0: 'X'}, {1: 'Y'}, {0: 'Z'},          # line, lane, top
             {29: 'X', 27: 'Y', 24: 'Z', 10: 'X', 0: 'Y'}, {28: 'Z', 26: 'X', 23: 'X', 1: 'Z', 0: 'X'},
             {29: 'Y', 28: 'Y', 27: 'Y', 26: 'Y', 25: 'Y'},
             {q: 'XYZ'[q % 3] for q in range(n)}, {q: 'Y' for q in range(n)}, {q: 'ZXY'[(q * 7) % 3] for q in range(n)}]
  xs, zs = [], []
  for s in strings:
    xs.append(_mask(n - 1 - q for q, c in s.items() if c in 'XY'))
    zs.append(_mask(n - 1 - q for q, c in s.items() if c in 'ZY'))
  with device.DeviceState(n, 128) as st:
    st.init_product([(1, f[q]) for q in range(n)])
    got = st.expect_pauli(xs, zs)
    norm = st.expect_pauli([0], [0])[0]
  want = np.array([math.prod(one[c][q] for q, c in s.items()) for s in strings])
  err = float(np.max(np.abs(got - want)))
  print(f'product-30: max error {err:.3e}, norm {norm:.15f}')
  assert err < 1e-12 and abs(norm - 1.0) < 1e-12


def test_ghz_30():
  n = 30
  full = (1 << n) - 1
  with device.DeviceState(n, 128, fusion=native.QH_FUSE_SWEEP) as st:
    st.init_basis(0)
    st.apply1(gates.hadamard(), 0)
    for q in range(1, n):
      st.applyc(gates.pauli_x(), 0, q)
    xs = [0, 0, 0, 0, 0, full, full, 1, full ^ 1]
    zs = [(1 << 29) | 1, (1 << 13) | (1 << 2), 1, 1 << 29, 1 << 15, 0, full, 0, 0]
    got = st.expect_pauli(xs, zs)
  want = [1, 1, 0, 0, 0, 1, math.cos(30 * math.pi / 2), 0, 0]
  err = float(np.max(np.abs(got - np.array(want, dtype=np.float64))))
  print(f'GHZ-30: {got.tolist()}')
  assert err < 1e-12


def test_supremacy30_against_marginals():
  n = 30
  ops, g8 = workloads.supremacy_stream(n, 20, seed=0).arrays()
  zbits = [0, 1, 2, 4, 6, 8, 11, 13, 15, 17, 19, 21, 24, 26, 28, 29]
  x_sets = [[0, 1, 2], [3, 4, 5, 7], [27, 28, 29], [1, 9, 14, 22, 29], list(range(0, 30, 2))[:16]]
  with device.DeviceState(n, 128, fusion=native.QH_FUSE_SWEEP) as st:
    st.init_basis(0)
    st.run_stream(ops, g8)
    st.flush()
    bm = _bitmap(st)
    assert bm != list(range(n))                          # the expectations below run on a permuted layout
    n0 = st.marginal([])
    zsets = [zbits, zbits[:5], [29], [0], [12, 3]]
    gz = st.expect_pauli([0] * len(zsets), [_mask(b) for b in zsets])
    for bits, v in zip(zsets, gz):
      e = abs(v - _signed(st.marginal(bits)))
      print(f'supremacy-30 Z on {bits}: {v:+.15f} (|diff to marginal| {e:.2e})')
      assert e < 1e-12
    gx = st.expect_pauli([_mask(b) for b in x_sets], [0] * len(x_sets))
    assert st.expect_pauli([_mask(b) for b in x_sets], [0] * len(x_sets)).tobytes() == gx.tobytes()
    assert _bitmap(st) == bm and st.marginal([]).tobytes() == n0.tobytes()
    # <X_S>_psi = <Z_S>_{H psi}: H on every qubit of S (logical bit b is qubit n-1-b), then the signed marginal; undo
    for bits, v in zip(x_sets, gx):
      for b in bits:
        st.apply1(gates.hadamard(), n - 1 - b)
      e = abs(v - _signed(st.marginal(bits)))
      print(f'supremacy-30 X on {bits}: {v:+.15f} (|diff to H + marginal| {e:.2e})')
      assert e < 1e-12
      for b in bits:
        st.apply1(gates.hadamard(), n - 1 - b)
