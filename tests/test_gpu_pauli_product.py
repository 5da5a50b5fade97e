"""Pauli products on the MI355X: qh_apply_pauli_product (state := F_{n-1} ... F_0 state in place, F_t = a_t I + b_t P_t) against
pauli_product_util.np_pauli_product -- the factors one by one in complex128 NumPy on the amplitudes as stored -- at both
widths: single factors by the PHYSICAL position of their pivot on a layout a fused QFT flush has permuted, runs and their
order, the exact cases, every size of the small-state kernel and the first of the main shape, a block that walks two chunks,
the barrier, attached / host-mapped / shard handles, and qc.evolve / pauli_rot / imaginary_time / pauli_project end to end.

Tolerance (pauli_product_util.bound, derived, not measured): with M = prod_t (|a_t| + |b_t|) and amax = max |src_i|, per
component (4 nterms + 4) 2^-52 M amax at complex128, plus nruns * 2^-23 M amax at complex64.  Wherever the contract says
exact, ==.

qh_download re-lays a permuted state out, so what a handle under test holds is read from clones."""
import ctypes
import math

import numpy as np
import pytest

from qcc_amd import device, gates, native, workloads
from qcc_amd.lib import circuit, tensor
from tests import pauli_product_util as ppu, pauli_util, shard_util

pytestmark = pytest.mark.gpu

_dp = ctypes.POINTER(ctypes.c_double)
_up = ctypes.POINTER(ctypes.c_uint64)
BATCH = native.QH_PAULI_PRODUCT_BATCH
DIAG, PAIR, HALF = native.QH_PAULI_RUN_DIAG, native.QH_PAULI_RUN_PAIR, native.QH_PAULI_RUN_HALF
# the kernel's own constants (qcc_amd/csrc/pauli_plan.h): 256 threads x 8 numbers per chunk, 4096 blocks at most
CHUNK_BITS, BLOCK_CAP_BITS = 11, 12


def _amp_bits(bw):
  return 0 if bw == 128 else 1


def _dtype(bw):
  return np.complex128 if bw == 128 else np.complex64


def _logical_state(st, shard=0, nglob=None):
  phys = st.download().astype(np.complex128)
  lo = shard_util.phys_to_logical(st, shard, np.arange(phys.size), nglob or st.nbits).astype(np.int64)
  return lo, phys


def _logical(st):
  """the handle's amplitudes as stored, in logical order (re-lays the handle out)"""
  lo, phys = _logical_state(st)
  out = np.empty_like(phys)
  out[lo] = phys
  return out


def _held(st):
  """... read from a clone: the handle keeps its layout"""
  with st.clone() as c:
    return _logical(c)


def _random_state(n, seed):
  rng = np.random.default_rng(seed)
  v = rng.normal(size=1 << n) + 1j * rng.normal(size=1 << n)
  return v / np.linalg.norm(v)


def _permuted(n, bw, seed):
  """a random state taken through a fused QFT flush (relayout sweeps leave a permuted bit map), then two index-bit swaps so
  that the layout is permuted whatever the planner chose"""
  st = device.DeviceState(n, bw, fusion=native.QH_FUSE_SWEEP)
  st.upload(_random_state(n, seed))
  ops, g8 = workloads.qft_stream(range(n)).arrays()
  st.run_stream(ops, g8)
  st.flush()
  print(f'bit map after the QFT flush (n={n}, bw={bw}): {shard_util.bitmap(st)}')
  st.remap_swap(0, n - 1)
  st.remap_swap(2, n // 2)
  assert shard_util.bitmap(st) != list(range(n))
  return st


def _shard_bytes(st):
  return (1 << st.nbits) * (16 if st.bit_width == 128 else 8)


def _pending(st):
  pend = ctypes.c_uint64()
  native.check(st.lib.qh_pending_gates(st.h, ctypes.byref(pend)))
  return pend.value


def _maxerr(got, want):
  return float(max(np.max(np.abs(got.real - want.real)), np.max(np.abs(got.imag - want.imag))))


def _apply_checked(st, a, b, xs, zs, what, exact=False, nruns=None, kinds=None):
  """the product on st in place, with stats, bit map and norm2 checked (asking for the device pointer would bring the layout
  back to canonical order: the pointer is checked in test_attached_and_host_mapped_handles); the product is applied TWICE
  from the same start (restored from a clone) so that norm2 can be compared bit for bit.  Returns (before, after) in logical
  order."""
  bw = st.bit_width
  before = _held(st)
  _, runs = st.pauli_product_plan(xs, zs)
  if nruns is not None:
    assert len(runs) == nruns, (what, runs)
  if kinds is not None:
    assert [r['kind'] for r in runs] == kinds, (what, runs)
  assert [(r['first'], r['count'], r['px'], r['kind']) for r in runs] == \
      ppu.greedy_runs([t['px'] for t in st.pauli_product_plan(xs, zs)[0]], BATCH, _amp_bits(bw), (DIAG, PAIR, HALF)), what
  with st.clone() as keep:
    bm, s0 = shard_util.bitmap(st), st.stats()
    n2 = st.apply_pauli_product(a, b, xs, zs, norm=True)
    s1 = st.stats()
    sb = _shard_bytes(st)
    grow = dict(gates_submitted=len(xs), kernels_launched=len(runs), bytes_swept=2 * len(runs) * sb, bytes_algorithmic=2 * len(runs) * sb,
                sweeps=0, gates_noop=0)
    for k, v in grow.items():
      assert s1[k] - s0[k] == v, (what, k, s1[k] - s0[k], v)
    assert shard_util.bitmap(st) == bm and _pending(st) == 0, what
    got = _held(st)
    st.copy_from(keep)                                       # the same start again: the same bits
    assert shard_util.bitmap(st) == bm, what
    n2b = st.apply_pauli_product(a, b, xs, zs, norm=True)
    assert n2b == n2, (what, n2, n2b)
    assert _held(st).tobytes() == got.tobytes(), what
  want = ppu.np_pauli_product(before, a, b, xs, zs)
  amax = float(np.max(np.abs(before)))
  tol = ppu.bound(bw, a, b, amax, len(runs))
  err = _maxerr(got, want)
  n2_np = float(np.vdot(got, got).real)
  n2_want = float(np.vdot(want, want).real)
  n2_tol = 4 * ppu.magnitude(a, b) * amax * tol * got.size + 1e-12 * n2_want
  print(f'{what}: {len(runs)} runs, error {err:.3e} (bound {tol:.3e}); norm2 {n2:.17g}, NumPy {n2_want:.17g} (tolerance {n2_tol:.3e})')
  if exact:
    assert np.array_equal(got, want.astype(_dtype(bw)).astype(np.complex128)), what
  assert err <= tol, (what, err, tol)
  assert abs(n2 - n2_np) <= 1e-12 * max(1.0, n2_np) and abs(n2 - n2_want) <= n2_tol, (what, n2, n2_want, n2_np)
  return before, got


def _rot(theta):
  return math.cos(theta), -1j * math.sin(theta)


@pytest.fixture(scope='module', params=[128, 64])
def permuted14(request):
  """a handle at 14 qubits in a permuted layout; every test leaves a valid state in it"""
  bw = request.param
  st = _permuted(14, bw, 14 + bw)
  yield bw, st
  st.close()


# ---- 1. single factors by the physical position of the pivot --------------------------------------------------------------------
def _position_classes(n, bw):
  """physical AMPLITUDE-index positions of each class of the pair walk: sub-item (complex64: HALF), inside a 128-byte line, on
  a lane bit outside it, wave / register-index / chunk bits, the top bit"""
  ab = _amp_bits(bw)
  cls = {'line': ab + 1, 'lane': ab + 4, 'wave': ab + 7, 'register-index': ab + 9, 'chunk': ab + CHUNK_BITS, 'top': n - 1}
  if ab:
    cls['sub-item'] = 0
  assert cls['chunk'] < n - 1
  return cls


def test_single_factors_by_physical_position(permuted14):
  """One factor each with the top x bit, by PHYSICAL position in the layout the QFT flush left, on each class of index bit:
  as X, as Y, and as a multi-bit mask with extra x bits below the pivot and z bits on every part of the index.  Then one
  diagonal factor with z on every part."""
  bw, st = permuted14
  n = st.nbits
  cls = _position_classes(n, bw)
  bm = shard_util.bitmap(st)
  at = {name: 1 << bm.index(p) for name, p in cls.items()}
  zall = 0
  for bit in at.values():
    zall |= bit
  a, b = 0.6 - 0.3j, 0.2 + 0.7j
  for name, p in cls.items():
    bit = at[name]
    below = 0
    for q in range(p):                                       # every other physical position below the pivot
      if q % 2 == 0:
        below |= 1 << bm.index(q)
    kind = HALF if (name == 'sub-item') else PAIR
    _apply_checked(st, [a], [b], [bit], [0], f'X on the {name} bit, bw = {bw}', nruns=1, kinds=[kind])
    _apply_checked(st, [a], [b], [bit], [bit], f'Y on the {name} bit, bw = {bw}', nruns=1, kinds=[kind])
    if below:
      _apply_checked(st, [a], [b], [bit | below], [zall], f'pivot on the {name} bit, x below it, z everywhere, bw = {bw}', nruns=1, kinds=[PAIR])
    _apply_checked(st, [a, b], [b, a], [bit, 0], [zall & ~bit, zall], f'{name} bit with a diagonal factor, bw = {bw}', nruns=1, kinds=[kind])
  _apply_checked(st, [a], [b], [0], [zall], f'one diagonal factor, z everywhere, bw = {bw}', nruns=1, kinds=[DIAG])
  st.scale(1.0 / math.sqrt(st.norm2()))                      # (the factors are not unitary: keep the magnitudes near 1)


# ---- 2. runs ---------------------------------------------------------------------------------------------------------------------
def test_runs(permuted14):
  bw, st = permuted14
  n = st.nbits
  rng = np.random.default_rng(200 + bw)

  def angles(k):
    ab_ = [_rot(float(t)) for t in rng.uniform(-1.5, 1.5, size=k)]
    return [c for c, _ in ab_], [s for _, s in ab_]
  zs = lambda k: [int(v) for v in rng.integers(0, 1 << n, size=k)]      # noqa: E731
  # BATCH diagonal terms: one kernel; BATCH + 1: two
  a, b = angles(BATCH)
  _apply_checked(st, a, b, [0] * BATCH, zs(BATCH), f'{BATCH} diagonal terms, bw = {bw}', nruns=1, kinds=[DIAG])
  a, b = angles(BATCH + 1)
  _apply_checked(st, a, b, [0] * (BATCH + 1), zs(BATCH + 1), f'{BATCH + 1} diagonal terms, bw = {bw}', nruns=2, kinds=[DIAG, DIAG])
  # a full PAIR run, and the smaller instantiation (4 terms)
  X = int(rng.integers(2, 1 << n))
  a, b = angles(BATCH)
  _apply_checked(st, a, b, [X] * BATCH, zs(BATCH), f'{BATCH} terms of one x mask, bw = {bw}', nruns=1, kinds=[PAIR])
  a, b = angles(4)
  _apply_checked(st, a, b, [X, 0, X, X], zs(4), f'4 terms, bw = {bw}', nruns=1, kinds=[PAIR])
  # full runs of the other two walks: the pivot on the PHYSICAL line bit (in-wave, with an x bit below it), and X == 1
  # in complex64 (HALF); diagonal terms among them
  bm = shard_util.bitmap(st)
  ab_bits = _amp_bits(bw)
  line = (1 << bm.index(ab_bits + 1)) | (1 << bm.index(0))
  a, b = angles(BATCH)
  _apply_checked(st, a, b, [line if k % 3 else 0 for k in range(1, BATCH + 1)], zs(BATCH), f'{BATCH} terms, pivot inside the line, bw = {bw}',
                 nruns=1, kinds=[PAIR])
  if ab_bits:
    a, b = angles(BATCH)
    _apply_checked(st, a, b, [1 << bm.index(0) if k % 3 else 0 for k in range(1, BATCH + 1)], zs(BATCH), f'{BATCH} terms, X == 1, bw = {bw}',
                   nruns=1, kinds=[HALF])
  # an alternating X1, X2, X1 list: three kernels
  a, b = angles(3)
  _apply_checked(st, a, b, [6, 10, 6], zs(3), f'alternating x masks, bw = {bw}', nruns=3)
  # general coefficients: imaginary time, a projector, a plain string, anything
  a = [math.cosh(0.4), 0.5, 0.0, 0.3 - 1.1j]
  b = [-math.sinh(0.4), -0.5, 1.0, -0.8 + 0.2j]
  _apply_checked(st, a, b, [X, X, 0, X], zs(4), f'general coefficients, bw = {bw}', nruns=1)
  st.scale(1.0 / math.sqrt(st.norm2()))


def test_order_within_a_run_is_honoured(permuted14):
  """a run mixing px == 0 and px == X terms that do NOT commute (Z on a bit of X anticommutes with it); the same terms
  reversed give a result that differs by far more than the tolerance"""
  bw, st = permuted14
  n = st.nbits
  X = (1 << 5) | (1 << 9) | 1
  xs = [X, 0, X, 0, 0, X]
  zs = [1 << 2, 1 << 5, (1 << 9) | (1 << 3), (1 << 9) | (1 << 12), 1, 1 << 5]
  assert all(bin(X & z).count('1') % 2 == 1 for x, z in zip(xs, zs) if x == 0)      # each diagonal term anticommutes with X...
  ab = [_rot(0.3 + 0.2 * k) for k in range(len(xs))]
  a, b = [c for c, _ in ab], [s for _, s in ab]
  with st.clone() as keep:
    before, fwd = _apply_checked(st, a, b, xs, zs, f'mixed run, bw = {bw}', nruns=1, kinds=[PAIR])
    st.copy_from(keep)
    _, rev = _apply_checked(st, a[::-1], b[::-1], xs[::-1], zs[::-1], f'mixed run reversed, bw = {bw}', nruns=1, kinds=[PAIR])
    st.copy_from(keep)
  tol = ppu.bound(bw, a, b, float(np.max(np.abs(before))), 1)
  diff = float(np.max(np.abs(fwd - rev)))
  print(f'forward against reversed, bw = {bw}: {diff:.3e} (tolerance {tol:.3e})')
  assert diff > 1e3 * tol


# ---- 3. exact cases ----------------------------------------------------------------------------------------------------------------
def test_exact_cases(permuted14):
  """(0, 1) strings: == NumPy's moved and negated values; (1, 0): bits unchanged; P applied twice: == the original"""
  bw, st = permuted14
  n = st.nbits
  rng = np.random.default_rng(300 + bw)
  cls = _position_classes(n, bw)
  bm = shard_util.bitmap(st)
  masks = [(1 << bm.index(p), 0) for p in cls.values()] + [(1 << bm.index(p), 1 << bm.index(p)) for p in cls.values()]
  masks += [(0, int(rng.integers(1, 1 << n)))] + [(int(rng.integers(1, 1 << n)), int(rng.integers(0, 1 << n))) for _ in range(6)]
  letters = rng.integers(1, 4, size=n)                     # X, Z or Y on every qubit
  masks.append((sum(1 << q for q in range(n) if letters[q] & 1), sum(1 << q for q in range(n) if letters[q] & 2)))
  start = _held(st)
  for x, z in masks:
    ny = bin(x & z).count('1')
    _apply_checked(st, [0.0], [1.0], [x], [z], f'string x = {x:#x}, z = {z:#x} (nY = {ny}), bw = {bw}', exact=True, nruns=1)
    assert st.apply_pauli_product([0.0], [1.0], [x], [z]) is None      # P P = I: back to the bits before
    assert _held(st).tobytes() == start.tobytes(), (x, z)
  for b_unit in (-1.0, 1j, -1j):                             # b itself a power of i
    _apply_checked(st, [0.0], [b_unit], [masks[-1][0]], [masks[-1][1]], f'b = {b_unit}, bw = {bw}', exact=True, nruns=1)
  with st.clone() as keep:
    phys = keep.download().tobytes()
  for x, z in masks[:3] + masks[-2:]:
    s0 = st.stats()
    n2 = st.apply_pauli_product([1.0], [0.0], [x], [z], norm=True)      # the identity: one kernel, every bit as it was
    assert st.stats()['kernels_launched'] == s0['kernels_launched'] + 1
    with st.clone() as c:
      assert c.download().tobytes() == phys
    assert abs(n2 - st.norm2()) <= 1e-12 * n2
  st.scale(1.0 / math.sqrt(st.norm2()))


def test_no_terms_flushes_and_launches_nothing():
  with device.DeviceState(10, 128, fusion=native.QH_FUSE_SWEEP) as st:
    st.upload(_random_state(10, 3))
    st.apply1(gates.hadamard(), 2)
    assert _pending(st) == 1
    want = _had(_random_state(10, 3), 2)
    s0 = st.stats()
    n2 = st.apply_pauli_product([], [], [], [], norm=True)
    assert _pending(st) == 0 and st.stats()['gates_submitted'] == s0['gates_submitted']
    assert abs(n2 - 1.0) <= 1e-12 and abs(n2 - st.norm2()) <= 1e-14      # the qh_norm2 path
    assert st.apply_pauli_product([], [], [], []) is None
    assert np.max(np.abs(_held(st) - want)) <= 2.0 ** -50


# ---- 4. sizes ------------------------------------------------------------------------------------------------------------------------
def _random_list(rng, n, count):
  """count factors over at most two x masks with diagonal terms among them, rotations and general coefficients"""
  pool = [0] + [int(v) for v in rng.integers(1, 1 << n, size=2)]
  xs = [pool[int(k)] for k in rng.integers(0, 3, size=count)]
  zs = [int(v) for v in rng.integers(0, 1 << n, size=count)]
  a = [complex(*rng.normal(size=2)) for _ in range(count)]
  b = [complex(*rng.normal(size=2)) for _ in range(count)]
  a[0], b[0] = _rot(0.7)
  return a, b, xs, zs


@pytest.mark.parametrize('bw,n', [(128, n) for n in range(1, 13)] + [(64, n) for n in range(1, 14)])
def test_small_states(bw, n):
  """every local size from 1 to 12 bits (13 at complex64): the one-pair-per-thread kernel serves all of them but the last,
  which is the first of the main shape"""
  rng = np.random.default_rng(400 + n)
  with device.DeviceState(n, bw) as st:
    st.upload(_random_state(n, 30 + n))
    if n > 1:
      st.remap_swap(0, n - 1)
    a, b, xs, zs = _random_list(rng, n, 5)
    _apply_checked(st, a, b, xs, zs, f'n = {n}, 5 terms, bw = {bw}')
    st.scale(1.0 / math.sqrt(st.norm2()))
    x, z = int(rng.integers(1, 1 << n)), int(rng.integers(0, 1 << n))
    _apply_checked(st, [0.0], [1.0], [x], [z], f'n = {n}, a string, bw = {bw}', exact=True)
    _apply_checked(st, [0.0], [-1j], [0], [z], f'n = {n}, a diagonal string, bw = {bw}', exact=True)
    if bw == 64:
      low = 1 << shard_util.bitmap(st).index(0)             # the logical bit on physical bit 0
      _apply_checked(st, [0.3], [0.9j], [low], [z], f'n = {n}, X == 1 (physical), bw = {bw}', kinds=[HALF])


@pytest.mark.parametrize('bw,n', [(128, 12), (128, 13), (64, 13), (64, 14)])
def test_first_main_shape_sizes(bw, n):
  """the smallest states of the main shape: one chunk of pairs (two chunks of items), then two"""
  rng = np.random.default_rng(n + bw)
  with device.DeviceState(n, bw) as st:
    st.upload(_random_state(n, 50 + n))
    st.remap_swap(1, n - 2)
    a, b, xs, zs = _random_list(rng, n, 5)
    _apply_checked(st, a, b, xs, zs, f'main shape n = {n}, 5 terms, bw = {bw}')
    st.scale(1.0 / math.sqrt(st.norm2()))
    top = 1 << shard_util.bitmap(st).index(n - 1)
    _apply_checked(st, [0.5, 0.5], [0.5, -0.5j], [top | 1, 0], [3, top | 5], f'main shape n = {n}, top pivot, bw = {bw}', nruns=1, kinds=[PAIR])
    _apply_checked(st, [0.5], [0.5j], [0], [top | 6], f'main shape n = {n}, diagonal, bw = {bw}', nruns=1, kinds=[DIAG])
    if bw == 64:
      low = 1 << shard_util.bitmap(st).index(0)
      _apply_checked(st, [0.5], [0.5j], [low], [top | 7], f'main shape n = {n}, X == 1 (physical), bw = {bw}', nruns=1, kinds=[HALF])


def _model_on(idx, vals, a, b, xs, zs):
  """np_pauli_product on the amplitudes vals at the indices idx alone; idx must be closed under every x mask"""
  order = np.argsort(idx)
  idx, v = idx[order].astype(np.uint64), vals[order].astype(np.complex128)
  for at, bt, x, z in zip(a, b, xs, zs):
    pos = np.searchsorted(idx, idx ^ np.uint64(x))
    assert np.array_equal(idx[pos], idx ^ np.uint64(x))
    pv = np.where(pauli_util.parity(idx, z) == 1, -v[pos], v[pos])
    for _ in range(bin(int(x) & int(z)).count('1') % 4):      # times -i
      pv = pv.imag - 1j * pv.real
    v = complex(at) * v + complex(bt) * pv
  return idx, v


@pytest.mark.parametrize('bw', [128, 64])
def test_blocks_that_walk_two_chunks(bw):
  """25 qubits at complex128, 26 at complex64 (512 MiB): 2^24 pairs of items = 2^13 chunks of pairs over 4096 blocks, so a
  block of a pair walk goes through two chunks (an item walk through four) and the chunk number's lowest bit changes INSIDE a
  block.  Five terms -- a PAIR factor with its pivot inside the line (the in-wave walk over items), a diagonal factor (it
  joins that run), PAIR factors with the pivot on a lane bit outside the line and on a register-index bit (pair walks whose
  item0 is the pair number with a bit really inserted) and one with the top pivot -- then a diagonal factor alone (a DIAG
  run).  The layout is the identity, so the downloads are in logical order; NumPy checks a strided sample of 2^20 indices
  (closed under the x masks) and norm2."""
  ab = _amp_bits(bw)
  n = CHUNK_BITS + BLOCK_CAP_BITS + 2 + ab
  cb = CHUNK_BITS + ab                                       # the lowest bit of an ITEM walk's chunk number, as an amplitude bit
  rng = np.random.default_rng(25 + bw)
  host = (rng.random(2 << n, dtype=np.float32) - np.float32(0.5))
  host = host.astype(np.float64).view(np.complex128) if bw == 128 else host.view(np.complex64)

  def sumsq(flat):                                           # sum of squares in double, a slice at a time
    return float(sum(np.dot(part, part) for part in (flat[k:k + (1 << 22)].astype(np.float64) for k in range(0, flat.size, 1 << 22))))
  flat_t = np.float64 if bw == 128 else np.float32
  host *= flat_t(1.0 / math.sqrt(sumsq(host.view(flat_t))))
  low, top = (1 << (ab + 2)) | 1, (1 << (n - 1)) | (1 << 6)
  lane, reg = (1 << (ab + 4)) | (1 << ab) | 1, (1 << (ab + 9)) | (1 << (ab + 5)) | (1 << (ab + 1))      # pivots on item bits 4 and 9
  xs = [low, 0, lane, reg, top]
  zs = [(1 << cb) | (1 << (cb + 1)) | 1, (1 << (cb + 2)) | (1 << (n - 1)) | (1 << 9) | 1, (1 << (cb - 1)) | (1 << cb) | (1 << (ab + 4)) | (1 << 3) | 1,
        (1 << (cb - 1)) | (1 << (cb + 1)) | (1 << (ab + 9)) | (1 << (ab + 10)) | (1 << (n - 1)) | 1, (1 << cb) | (1 << (n - 1)) | (1 << 8) | 1]
  ab3 = [_rot(0.4), (0.8, 0.6j), _rot(0.9), _rot(-0.5), _rot(-1.1)]
  a, b = [c for c, _ in ab3], [s for _, s in ab3]
  xd, zd, ad, bd = [0], [(1 << cb) | (1 << (cb + 1)) | (1 << (n - 2)) | 1], [0.6], [-0.8j]
  with device.DeviceState(n, bw) as st:
    st.upload(host)
    _, runs = st.pauli_product_plan(xs, zs)
    assert [(r['count'], r['px'], r['kind']) for r in runs] == [(2, low, PAIR), (1, lane, PAIR), (1, reg, PAIR), (1, top, PAIR)]
    _, rund = st.pauli_product_plan(xd, zd)
    assert [(r['count'], r['kind']) for r in rund] == [(1, DIAG)]
    s0 = st.stats()
    n2a = st.apply_pauli_product(a, b, xs, zs, norm=True)
    n2 = st.apply_pauli_product(ad, bd, xd, zd, norm=True)
    s1 = st.stats()
    assert s1['kernels_launched'] - s0['kernels_launched'] == 5 and s1['gates_submitted'] - s0['gates_submitted'] == 6
    assert s1['bytes_swept'] - s0['bytes_swept'] == 10 * _shard_bytes(st)
    got = st.download()
  base = np.arange(0, 1 << n, (1 << n) >> 16, dtype=np.uint64) + rng.integers(0, (1 << n) >> 16, size=1 << 16).astype(np.uint64)
  span = [0]
  for x in (low, lane, reg, top):                            # the group the x masks generate: 16 masks
    span += [g ^ x for g in span]
  idx = np.unique(np.concatenate([base ^ np.uint64(g) for g in span]))
  sel = idx.astype(np.int64)
  idx2, want = _model_on(idx, host[sel], a + ad, b + bd, xs + xd, zs + zd)
  assert np.array_equal(idx2, idx)
  amax = float(np.max(np.abs(host)))
  tol = ppu.bound(bw, a + ad, b + bd, amax, 5)
  err = _maxerr(got[sel].astype(np.complex128), want)
  n2_np = sumsq(got.view(flat_t))
  print(f'{n} qubits, bw = {bw}: error {err:.3e} on {idx.size} indices (bound {tol:.3e}); norm2 {n2:.17g}, NumPy on the stored values {n2_np:.17g}; '
        f'after the unitary part {n2a:.17g}')
  assert err <= tol
  assert abs(n2 - n2_np) <= 1e-12 * n2_np
  assert abs(n2a - 1.0) <= (1e-12 if bw == 128 else 1e-6)   # rotations and a unit-modulus pair (0.8, 0.6i) keep the norm


# ---- 5. queue and barrier, handles ---------------------------------------------------------------------------------------------------
TERMS = ([_rot(0.3)[0], 0.5, 0.9 - 0.2j, _rot(-0.8)[0], 0.4], [_rot(0.3)[1], 0.5, 0.1 + 0.3j, _rot(-0.8)[1], 0.6j],
         [0b101, 0, 0b101, 1 << 8, 0b11 << 6], [0b11, 0b1001 << 3, 1 << 8, 0b111, 1 << 7])


def _had(v, q):
  t = v.reshape(1 << q, 2, -1)
  return np.stack([t[:, 0] + t[:, 1], t[:, 0] - t[:, 1]], axis=1).reshape(-1) / np.sqrt(2.0)


@pytest.mark.parametrize('bw', [128, 64])
def test_queue_and_barrier(bw):
  """gates left queued before the call run first; gates queued after it are applied on top; nothing is pending after it"""
  n = 12
  a, b, xs, zs = TERMS
  with _permuted(n, bw, 62) as st:
    relay = st.set_relayout(True)
    before = _held(st)
    st.apply1(gates.hadamard(), 3)                           # queued (reference qubit 3 = logical bit n - 1 - 3)
    assert _pending(st) == 1
    st.apply_pauli_product(a, b, xs, zs)
    assert _pending(st) == 0
    gate_eps = 2.0 ** -50 if bw == 128 else 2.0 ** -22      # the Hadamard itself: two roundings per component
    after_gate = _had(before, 3)
    want = ppu.np_pauli_product(after_gate, a, b, xs, zs)
    m, amax = ppu.magnitude(a, b), float(np.max(np.abs(after_gate)))
    _, runs = st.pauli_product_plan(xs, zs)
    tol = ppu.bound(bw, a, b, amax, len(runs)) + m * gate_eps * amax
    got = _held(st)
    assert _maxerr(got, want) <= tol
    assert st.set_relayout(True) == relay                    # relayout mode as before: fused gates afterwards still work
    st.apply1(gates.hadamard(), 0)
    st.apply1(gates.hadamard(), n - 1)
    assert _pending(st) == 2
    st.flush()
    want2 = _had(_had(got, 0), n - 1)
    assert np.max(np.abs(_held(st) - want2)) <= 4 * gate_eps * float(np.max(np.abs(got)))


@pytest.mark.parametrize('bw', [128, 64])
def test_attached_and_host_mapped_handles(bw):
  n = 12
  a, b, xs, zs = TERMS
  with device.DeviceState(n, bw) as owner:
    ptr = owner.device_ptr
    with device.DeviceState(n, bw, device_ptr=ptr) as att:
      att.upload(_random_state(n, 61))
      att.remap_swap(1, 9)
      _apply_checked(att, a, b, xs, zs, f'attached handle, bw = {bw}')
      assert att.device_ptr == ptr
  with device.DeviceState(n, bw, host_mapped=True) as hm:
    ptr = hm.device_ptr
    hm.upload(_random_state(n, 62))
    hm.remap_swap(1, 9)
    before, got = _apply_checked(hm, a, b, xs, zs, f'host-mapped handle, bw = {bw}')
    hm.sync()
    lo = shard_util.logical_of_phys(shard_util.bitmap(hm), 1 << n).astype(np.int64)      # the mapped memory itself, as it lies
    mapped = np.empty(1 << n, dtype=np.complex128)
    mapped[lo] = np.asarray(hm.host_array()).reshape(-1)
    assert mapped.tobytes() == got.tobytes()
    assert hm.device_ptr == ptr


def test_refusals_change_nothing():
  lib = native.load()
  with device.DeviceState(8, 128, fusion=native.QH_FUSE_SWEEP) as st:
    st.upload(_random_state(8, 1))
    st.remap_swap(0, 5)
    want, bm = _held(st), shard_util.bitmap(st)
    st.apply1(gates.hadamard(), 2)
    s0 = st.stats()
    n2 = ctypes.c_double(7.0)
    x, z = np.array([3, 5], dtype=np.uint64), np.array([5, 1], dtype=np.uint64)
    co = np.array([1.0, 0.0, 0.0, 1.0, 0.5, 0.0, 0.5, 0.0])
    args = (co.ctypes.data_as(_dp), x.ctypes.data_as(_up), z.ctypes.data_as(_up))
    assert lib.qh_apply_pauli_product(None, 2, *args, ctypes.byref(n2)) == native.QH_ERR_ARG
    assert lib.qh_apply_pauli_product(st.h, 2, None, *args[1:], ctypes.byref(n2)) == native.QH_ERR_ARG
    assert lib.qh_apply_pauli_product(st.h, 2, args[0], None, args[2], ctypes.byref(n2)) == native.QH_ERR_ARG
    big = np.array([3, 1 << 8], dtype=np.uint64)
    assert lib.qh_apply_pauli_product(st.h, 2, args[0], big.ctypes.data_as(_up), args[2], ctypes.byref(n2)) == native.QH_ERR_BAD_QUBIT
    assert b'term 1' in lib.qh_last_error()
    bad = co.copy()
    bad[6] = np.inf
    assert lib.qh_apply_pauli_product(st.h, 2, bad.ctypes.data_as(_dp), *args[1:], ctypes.byref(n2)) == native.QH_ERR_ARG
    assert b'term 1' in lib.qh_last_error() and b'non-finite' in lib.qh_last_error()
    assert n2.value == 7.0 and _pending(st) == 1 and st.stats() == s0 and shard_util.bitmap(st) == bm      # nothing flushed
    st.flush()
    assert np.max(np.abs(_held(st) - _had(want, 2))) <= 2.0 ** -50


@pytest.mark.parametrize('nloc,nglob', [(10, 12), (13, 15)])
@pytest.mark.parametrize('bw', [128, 64])
def test_shard_handles(bw, nloc, nglob):
  """qh_set_shard on one GPU, below and on the main shape: a z bit the shard index holds flips the sign per shard (folded
  into b on the host; a string whose shard sign makes b' = -1 on one shard and +1 on the other stays exact); an x bit there is
  QH_ERR_NONLOCAL, also for a later term, and state and stats are bitwise as before"""
  full = _random_state(nglob, 71).astype(_dtype(bw)).astype(np.complex128)      # as stored
  h0, h1 = 1 << nloc, 1 << (nloc + 1)
  ab5 = [_rot(0.5), (0.5, 0.5), (0.2 - 0.4j, 0.9j), _rot(-1.2), (math.cosh(0.3), -math.sinh(0.3))]
  a, b = [c for c, _ in ab5], [s for _, s in ab5]
  xs = [0b11, 0b11, 0, 1 << (nloc - 1), 1 << (nloc - 1)]
  zs = [h1, h0 | 4, h0 | h1 | (1 << (nloc - 1)), h0 | h1 | 1, h1 | (1 << (nloc - 1))]
  for shard in (1, 2):
    with device.DeviceState(nloc, bw) as s:
      s.set_shard(nglob, shard)
      s.upload(full[shard << nloc:(shard + 1) << nloc])
      s.remap_swap(2, 7)                                    # local bits anywhere (this relabels the state: read it back)
      with s.clone() as c:
        lo_s, phys_s = _logical_state(c, shard, nglob)
      held = np.zeros(1 << nglob, dtype=np.complex128)      # the global state with this shard's amplitudes only
      held[lo_s] = phys_s
      terms, runs = s.pauli_product_plan(xs, zs)
      assert [t['neg'] for t in terms] == [bin(shard & (z >> nloc)).count('1') % 2 for z in zs]
      with s.clone() as keep:
        n2 = s.apply_pauli_product(a, b, xs, zs, norm=True)
        with s.clone() as c:
          lo, phys = _logical_state(c, shard, nglob)
        assert np.all(lo >> nloc == shard) and np.array_equal(lo, lo_s)
        want = ppu.np_pauli_product(held, a, b, xs, zs)      # (x masks are local: partners stay on the shard)
        tol = ppu.bound(bw, a, b, float(np.max(np.abs(held))), len(runs))
        err = _maxerr(phys, want[lo])
        print(f'shard {shard} of {nglob - nloc} bits, nloc = {nloc}, bw = {bw}: error {err:.3e} (bound {tol:.3e})')
        assert err <= tol
        assert abs(n2 - float(np.vdot(phys, phys).real)) <= 1e-12 * n2
        # the string itself with z on a held bit: the shard's sign, exact
        s.copy_from(keep)
        s.apply_pauli_product([0.0], [1.0], [0b101], [h0 | 2])
        with s.clone() as c:
          _, phys1 = _logical_state(c, shard, nglob)
        want1 = ppu.np_pauli_product(held, [0.0], [1.0], [0b101], [h0 | 2])[lo]
        assert np.array_equal(phys1, want1)
        assert s.pauli_product_plan([0b101], [h0 | 2])[0][0]['neg'] == (shard & 1)
        s.copy_from(keep)
      # an x bit on a bit the shard index holds, in a LATER term: refused, everything as it is
      with s.clone() as c:
        bits = c.download().tobytes()
      st0 = s.stats()
      with pytest.raises(native.QhError) as e:
        s.apply_pauli_product(a[:3], b[:3], [1, 0, h0], [0, h1, 0])
      assert e.value.code == native.QH_ERR_NONLOCAL
      with pytest.raises(native.QhError) as e:
        s.apply_pauli_product([0.0], [1.0], [h1], [h1])
      assert e.value.code == native.QH_ERR_NONLOCAL
      assert s.stats() == st0
      with s.clone() as c:
        assert c.download().tobytes() == bits


# ---- 6. end to end through qc ---------------------------------------------------------------------------------------------------------
@pytest.fixture(params=[128, 64])
def width(request):
  tensor.set_tensor_width(request.param)
  yield request.param
  tensor.set_tensor_width(None)


def _amps(q):
  return np.array(q.psi).reshape(-1).astype(np.complex128)


def _layers(q, nq, seed):
  rng = np.random.default_rng(seed)
  for _ in range(2):
    for i in range(nq):
      q.ry(i, float(rng.uniform(0, 3)))
    for i in range(nq - 1):
      q.cu1(i, i + 1, float(rng.uniform(0, 3)))
    q.cx(int(rng.integers(1, nq)), 0)


def _masks(n, paulis):
  x = sum(1 << (n - 1 - q) for q, p in paulis.items() if p in 'XY')
  z = sum(1 << (n - 1 - q) for q, p in paulis.items() if p in 'ZY')
  return x, z


def test_qc_evolve_ising(width):
  """one and three first-order steps and one second-order step of a 10-qubit transverse-field Ising model against the model
  of the same factor list"""
  n, j, hx, t = 10, 1.0, 0.7, 0.35
  terms = [(-j, {q: 'Z', q + 1: 'Z'}) for q in range(n - 1)] + [(-hx, {q: 'X'}) for q in range(n)]
  eps = 2.0 ** -52 if width == 128 else 2.0 ** -23
  for steps, order in ((1, 1), (3, 1), (1, 2)):
    q = circuit.qc('ising')
    q.reg(n, 0)
    _layers(q, n, 5)
    assert hasattr(q._ensure_device(), 'apply_pauli_product')      # pylint: disable=protected-access
    psi = _amps(q)
    seq = list(range(len(terms)))
    dt = t / steps
    if order == 2:
      seq, dt = seq + seq[::-1], dt / 2
    seq = seq * steps
    ab_ = [_rot(dt * terms[k][0]) for k in seq]
    a, b = [c for c, _ in ab_], [s for _, s in ab_]
    xz = [_masks(n, terms[k][1]) for k in seq]
    want = ppu.np_pauli_product(psi, a, b, [x for x, _ in xz], [z for _, z in xz])
    q.evolve(terms, t, steps=steps, order=order)
    got = _amps(q)
    # every term may be a run of its own on some layout: nruns <= nterms
    tol = ppu.bound(width, a, b, float(np.max(np.abs(psi))), len(seq))
    err = _maxerr(got, want)
    print(f'evolve, {steps} steps of order {order}, width {width}: error {err:.3e} (bound {tol:.3e})')
    assert err <= tol
    assert abs(q.norm2() - 1.0) <= 64 * len(seq) * eps


def test_qc_pauli_rot_against_a_cx_ladder(width):
  """exp(-i theta/2 Z...Z) on 10 qubits as one call against the same rotation through the gate path: a CX ladder down to the
  last qubit, rz there, the ladder back.  The ladder is 18 CX (moves: exact) and one rz, a diagonal gate: one complex product
  per amplitude, two roundings per component -- 2 * 2^-52 amax (2^-23 at complex64: rounded to float once per fused pass at
  most three times) on top of the product's own bound."""
  n, theta = 10, 0.77
  eps = 2.0 ** -52 if width == 128 else 2.0 ** -23
  qa, qb = circuit.qc('rot'), circuit.qc('ladder')
  for q in (qa, qb):
    q.reg(n, 0)
    _layers(q, n, 6)
  psi = _amps(qa)
  qa.pauli_rot('Z' * n, theta)
  for i in range(n - 1):
    qb.cx(i, i + 1)
  qb.rz(n - 1, theta)
  for i in reversed(range(n - 1)):
    qb.cx(i, i + 1)
  a, b = _rot(theta / 2)
  amax = float(np.max(np.abs(psi)))
  tol = ppu.bound(width, [a], [b], amax, 1) + (2 + 3 * (width == 64)) * eps * amax
  err = _maxerr(_amps(qa), _amps(qb))
  print(f'pauli_rot against the ladder, width {width}: {err:.3e} (tolerance {tol:.3e})')
  assert err <= tol
  x, z = _masks(n, {k: 'Z' for k in range(n)})
  assert _maxerr(_amps(qa), ppu.np_pauli_product(psi, [a], [b], [x], [z])) <= ppu.bound(width, [a], [b], amax, 1)
  # a mixed weight-10 string against basis changes around the same ladder: h for X, (sdag, h) for Y -- a few more gates,
  # each two roundings per component
  s = 'XYZZYXXZYX'
  qa.pauli_rot(s, theta)
  pre = _amps(qb)
  for k, ch in enumerate(s):
    if ch == 'Y':
      qb.sdag(k)
    if ch in 'XY':
      qb.h(k)
  for i in range(n - 1):
    qb.cx(i, i + 1)
  qb.rz(n - 1, theta)
  for i in reversed(range(n - 1)):
    qb.cx(i, i + 1)
  for k, ch in enumerate(s):
    if ch in 'XY':
      qb.h(k)
    if ch == 'Y':
      qb.s(k)
  ngates = 2 * sum(ch in 'XY' for ch in s) + 2 * sum(ch == 'Y' for ch in s) + 1
  amax = float(np.max(np.abs(pre)))
  tol2 = tol + ppu.bound(width, [a], [b], amax, 1) + 4 * ngates * eps * 2 * amax
  err = _maxerr(_amps(qa), _amps(qb))
  print(f'mixed string against the ladder, width {width}: {err:.3e} (tolerance {tol2:.3e}, {ngates} rounding gates)')
  assert err <= tol2


def test_qc_imaginary_time_and_projection(width):
  n = 10
  terms = [(-1.0, {q: 'Z', q + 1: 'Z'}) for q in range(n - 1)] + [(-0.7, {q: 'X'}) for q in range(n)]
  q = circuit.qc('itime')
  q.reg(n, 0)
  _layers(q, n, 7)
  psi = _amps(q)
  norm2 = q.imaginary_time(terms, 0.4, steps=2, normalize=True)
  seq = list(range(len(terms))) * 2
  a = [math.cosh(0.2 * terms[k][0]) for k in seq]
  b = [-math.sinh(0.2 * terms[k][0]) for k in seq]
  xz = [_masks(n, terms[k][1]) for k in seq]
  want = ppu.np_pauli_product(psi, a, b, [x for x, _ in xz], [z for _, z in xz])
  n2_want = float(np.vdot(want, want).real)
  assert abs(norm2 - n2_want) <= (1e-12 if width == 128 else 1e-5) * n2_want
  assert abs(q.norm2() - 1.0) <= (1e-12 if width == 128 else 1e-6)
  tol = ppu.bound(width, a, b, float(np.max(np.abs(psi))), len(seq)) / math.sqrt(n2_want) + 4 * (2.0 ** -52 if width == 128 else 2.0 ** -23)
  assert _maxerr(_amps(q), want / math.sqrt(n2_want)) <= tol
  # GHZ: ZZ...Z (n even) has eigenvalue +1, XX...X too; (I - X...X)/2 annihilates it
  eps = 2.0 ** -52 if width == 128 else 2.0 ** -23
  g = circuit.qc('ghz')
  g.reg(n, 0)
  g.h(0)
  for i in range(n - 1):
    g.cx(i, i + 1)
  ghz = _amps(g)
  p = g.pauli_project('Z' * n, +1)
  assert abs(p - 1.0) <= 8 * eps and _maxerr(_amps(g), ghz) <= 8 * eps
  p = g.pauli_project('X' * n, +1)
  assert abs(p - 1.0) <= 8 * eps and _maxerr(_amps(g), ghz) <= 8 * eps
  p = g.pauli_project({0: 'Z'}, -1)                          # the |1...1> branch, probability 1/2
  assert abs(p - 0.5) <= 8 * eps
  got = _amps(g)
  assert abs(abs(got[-1]) - 1.0) <= 8 * eps and np.count_nonzero(np.abs(got) > 8 * eps) == 1
  g2 = circuit.qc('ghz2')
  g2.reg(n, 0)
  g2.h(0)
  for i in range(n - 1):
    g2.cx(i, i + 1)
  p = g2.pauli_project('X' * n, -1, normalize=False)
  assert p <= 8 * eps and float(np.max(np.abs(_amps(g2)))) <= 8 * eps
