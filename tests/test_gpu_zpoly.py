"""Z-polynomial operators on the MI355X: qh_apply_zpoly (a_i *= exp(c f(i))) and qh_expect_zpoly (sum |a_i|^2 (1, f, f^2)) against
zpoly_util's model -- f by popcount in float64, the factor in complex128 on the amplitudes as stored -- at both widths: term
classes by the PHYSICAL position of their bits on a layout a fused QFT flush has permuted, 4096 terms in one kernel, the exact
cases, every size of the small kernel and the first of the main shape, blocks that walk several chunks, the moments, the
barrier, attached / host-mapped / shard handles, and qc.phase_polynomial / cost_filter / cost_expectation / qaoa_layer end to
end, the last also on the reference's own MaxCut diagonal (tests/golden/g15_maxcut_diag.npz).

Tolerances are zpoly_util.apply_bound and moment_bound, derived in that module's docstring, not measured; every test prints
the largest error beside its bound.

qh_download re-lays a permuted state out, so what a handle under test holds is read from clones."""
import ctypes
import math
import os

import numpy as np
import pytest

from qcc_amd import device, gates, native, workloads
from qcc_amd.lib import circuit, helper, tensor
from tests import pauli_product_util as ppu, shard_util, zpoly_util as zu

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONST, HIGH, LOW, STRADDLE = native.QH_ZPOLY_CONST, native.QH_ZPOLY_HIGH, native.QH_ZPOLY_LOW, native.QH_ZPOLY_STRADDLE
MAIN, SMALL = native.QH_ZPOLY_KERNEL_MAIN, native.QH_ZPOLY_KERNEL_SMALL
# the kernel's own constants (qcc_amd/csrc/pauli_plan.h): 256 threads x 8 items per chunk, 4096 blocks at most
CHUNK_BITS, BLOCK_CAP_BITS = 11, 12
# qh_norm2 adds at most 4096 block sums atomically, in any order, after at most 72 serial and tree additions per block (2^26
# amplitudes at the most here): relative to the sum
NORM2_TOL = (4096 + 72) * 2.0 ** -53


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


def _held_bytes(st):
  with st.clone() as c:
    return c.download().tobytes()


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


def _grow(s0, s1, **want):
  base = dict(gates_submitted=0, kernels_launched=0, bytes_swept=0, bytes_algorithmic=0, sweeps=0, gates_noop=0)
  base.update(want)
  for k, v in base.items():
    assert s1[k] - s0[k] == v, (k, s1[k] - s0[k], v)


def _apply_checked(st, ws, zs, c, what):
  """a_i *= exp(c f(i)) on st in place, with stats, bit map and norm2 checked; applied TWICE from the same start (restored from
  a clone) so that norm2 and the amplitudes can be compared bit for bit.  Returns (before, after) in logical order."""
  bw = st.bit_width
  before = _held(st)
  with st.clone() as keep:
    bm, s0 = shard_util.bitmap(st), st.stats()
    n2 = st.apply_zpoly(ws, zs, c, norm=True)
    sb = _shard_bytes(st)
    _grow(s0, st.stats(), gates_submitted=1, kernels_launched=1, bytes_swept=2 * sb, bytes_algorithmic=2 * sb)
    assert shard_util.bitmap(st) == bm and _pending(st) == 0, what
    got = _held(st)
    st.copy_from(keep)                                       # the same start again: the same bits
    assert shard_util.bitmap(st) == bm, what
    n2b = st.apply_zpoly(ws, zs, c, norm=True)
    assert n2b == n2, (what, n2, n2b)
    assert _held(st).tobytes() == got.tobytes(), what
  want = zu.np_apply(before, ws, zs, c)
  tol = zu.apply_bound(bw, ws, c, float(np.max(np.abs(before))))
  err = _maxerr(got, want)
  n2_np = float(np.vdot(got, got).real)
  print(f'{what}: {len(ws)} terms, error {err:.3e} (bound {tol:.3e}, ratio {err / tol:.3f}); norm2 {n2:.17g}, NumPy on the stored values {n2_np:.17g}')
  assert err <= tol, (what, err, tol)
  assert abs(n2 - n2_np) <= 1e-12 * max(1.0, n2_np), (what, n2, n2_np)
  return before, got


def _expect_checked(st, ws, zs, what):
  """the three moments against the model, with stats, repeatability and the untouched state checked"""
  bits, bm, s0 = _held_bytes(st), shard_util.bitmap(st), st.stats()
  out = st.expect_zpoly(ws, zs)
  sb = _shard_bytes(st)
  _grow(s0, st.stats(), kernels_launched=1, bytes_swept=sb, bytes_algorithmic=sb)
  assert st.expect_zpoly(ws, zs) == out, what                # bitwise on a repeat
  assert shard_util.bitmap(st) == bm and _pending(st) == 0 and _held_bytes(st) == bits, what
  want = zu.np_moments(_held(st), ws, zs)
  for k in range(3):
    tol = zu.moment_bound(ws, k, want[0])
    err = abs(out[k] - want[k])
    print(f'{what}: moment {k}: {out[k]:.17g}, model {want[k]:.17g}, error {err:.3e} (bound {tol:.3e}, ratio {err / tol:.3f})')
    assert err <= tol, (what, k, err, tol)
  n2 = st.norm2()
  assert abs(out[0] - n2) <= zu.moment_bound(ws, 0, n2) + NORM2_TOL * n2, (what, out[0], n2)
  return out


@pytest.fixture(scope='module', params=[128, 64])
def permuted14(request):
  """a handle at 14 qubits in a permuted layout; every test leaves a valid state in it"""
  bw = request.param
  st = _permuted(14, bw, 14 + bw)
  yield bw, st
  st.close()


# ---- 1. term classes by physical position ----------------------------------------------------------------------------------------
def _position_classes(n, bw):
  """physical AMPLITUDE-index positions of each part of the walk: sub-item (complex64), inside a 128-byte line, a lane bit
  outside it, wave / register-index bits (all below the chunk part), the lowest chunk bit and the top bit"""
  ab = _amp_bits(bw)
  cls = {'line': ab + 1, 'lane': ab + 4, 'wave': ab + 7, 'register-index': ab + 9, 'chunk': ab + CHUNK_BITS, 'top': n - 1}
  if ab:
    cls['half'] = 0
  assert cls['chunk'] < n - 1
  return cls


def test_term_classes_by_physical_position(permuted14):
  bw, st = permuted14
  n = st.nbits
  pos = _position_classes(n, bw)
  bm = shard_util.bitmap(st)
  at = {name: 1 << bm.index(p) for name, p in pos.items()}      # the LOGICAL bit that sits on each position
  lows = [k for k in pos if k not in ('chunk', 'top')]
  c_im, c_gen = -0.7j, -0.05 + 0.3j
  # single terms, one per part of the index
  for name in pos:
    p = st.zpoly_plan([1.3], [at[name]])
    assert p['cls'] == [LOW if name in lows else HIGH] and p['kernel'] == MAIN and p['pz'] == [1 << pos[name]], name
    _apply_checked(st, [1.3], [at[name]], c_im, f'one term on the {name} bit, bw = {bw}')
  # one straddling term per low part
  for name in lows:
    z = at[name] | at['chunk']
    p = st.zpoly_plan([-0.8], [z])
    assert p['cls'] == [STRADDLE] and p['group_mask'] == [1 << pos[name]], name
    _apply_checked(st, [-0.8], [z], c_gen, f'{name} x chunk, bw = {bw}')
  # a mixture: every class, several groups, two terms in one group, a duplicate and a constant
  zs = [at['line'] | at['chunk'], at['lane'] | at['top'], at['wave'] | at['chunk'] | at['top'], at['register-index'] | at['chunk'],
        at['line'] | at['top'], at['line'] | at['lane'] | at['wave'] | at['top'], 0, at['chunk'], at['chunk'] | at['top'], at['line'] | at['wave'],
        at['register-index'], at['lane'] | at['top'], at['top']]
  if 'half' in at:
    zs += [at['half'] | at['top'], at['half'] | at['line'], at['half'] | at['lane'] | at['chunk']]
  rng = np.random.default_rng(100 + bw)
  ws = [float(v) for v in rng.uniform(-2, 2, size=len(zs))]
  p = st.zpoly_plan(ws, zs)
  assert p['nconst'] == 1 and p['nhigh'] == 3 and p['nlow'] >= 2 and p['nstraddle'] >= 7
  assert 3 <= p['ngroups'] < p['nstraddle']                 # G >= 3, and a group of more than one term
  assert len(set(p['group_mask'])) == p['ngroups']
  _apply_checked(st, ws, zs, c_im, f'every class, imaginary c, bw = {bw}')
  _apply_checked(st, ws, zs, c_gen, f'every class, complex c, bw = {bw}')
  _apply_checked(st, ws, zs, -0.1, f'every class, real c, bw = {bw}')
  _expect_checked(st, ws, zs, f'every class, bw = {bw}')
  st.scale(1.0 / math.sqrt(st.norm2()))                      # (real parts of c are not unitary: keep the magnitudes near 1)


# ---- 2. many terms ---------------------------------------------------------------------------------------------------------------
def test_many_terms_in_one_kernel(permuted14):
  bw, st = permuted14
  n = st.nbits
  rng = np.random.default_rng(4096 + bw)
  T = native.QH_ZPOLY_MAX_TERMS
  zs = []
  for _ in range(T):
    z = 0
    for b in rng.choice(n, size=int(rng.integers(1, 5)), replace=False):
      z |= 1 << int(b)
    zs.append(z)
  zs[7], zs[100], zs[4000] = 0, zs[99], zs[3]                # a constant term and duplicates
  ws = [float(v) for v in rng.uniform(-1, 1, size=T) * (36.0 / T) * 2]      # F about 36: |c| F <= 40 with |c| = 1
  assert zu.big_f(ws) <= 40
  p = st.zpoly_plan(ws, zs)
  assert p['nterms'] == T and p['ngroups'] > 64 and p['nstraddle'] > p['ngroups'] and p['nconst'] == 1
  _apply_checked(st, ws, zs, -1j, f'{T} terms, bw = {bw}')           # (its stats: one kernel)
  _expect_checked(st, ws, zs, f'{T} terms, bw = {bw}')
  # every mask with the top physical bit as well: all the terms straddle (or lie in the chunk part), more of them than the
  # kernel keeps in LDS (2048: qcc_amd/csrc/kernels_zpoly.hip.h), so the per-chunk sums read the device block itself
  top = 1 << shard_util.bitmap(st).index(n - 1)
  zs2 = [z | top for z in zs]
  p = st.zpoly_plan(ws, zs2)
  assert p['nconst'] + p['nhigh'] + p['nstraddle'] == T > 2048 and p['nlow'] == 0
  _apply_checked(st, ws, zs2, 0.01 - 1j, f'{T} terms in the chunk part, bw = {bw}')
  _expect_checked(st, ws, zs2, f'{T} terms in the chunk part, bw = {bw}')
  st.scale(1.0 / math.sqrt(st.norm2()))
  s0, bits = st.stats(), _held_bytes(st)
  for call in (lambda: st.apply_zpoly(ws + [0.5], zs + [1], -1j), lambda: st.expect_zpoly(ws + [0.5], zs + [1])):
    with pytest.raises(native.QhError) as e:
      call()
    assert e.value.code == native.QH_ERR_ARG
  assert st.stats() == s0 and _held_bytes(st) == bits


# ---- 3. exactness of the contract ----------------------------------------------------------------------------------------------------
def test_exact_cases(permuted14):
  bw, st = permuted14
  n = st.nbits
  ws, zs = [0.5, -1.5, 2.0], [3, 1 << (n - 1), 0]
  # c == 0 and no terms: nothing is launched and every bit stays; norm2 is qh_norm2's
  bits, s0 = _held_bytes(st), st.stats()
  n2 = st.norm2()
  s0 = st.stats()
  assert st.apply_zpoly(ws, zs, 0.0) is None and st.apply_zpoly([], [], 0.5) is None
  assert st.stats() == s0
  for got in (st.apply_zpoly(ws, zs, 0.0, norm=True), st.apply_zpoly([], [], -1j, norm=True)):      # (the same fixed-order sum: the same bits)
    assert got == n2, (got, n2)
  s1 = st.stats()
  assert s1['gates_submitted'] == s0['gates_submitted'] and s1['bytes_algorithmic'] == s0['bytes_algorithmic']
  assert _held_bytes(st) == bits
  out = st.expect_zpoly([], [])
  assert out == (n2, 0.0, 0.0), (out, n2)
  # a constant term alone with an imaginary c: one global phase.  On a uniform state every stored value is the same
  with device.DeviceState(n, bw) as u:
    u.upload(np.full(1 << n, 2.0 ** -(n / 2) * (0.6 + 0.8j)))
    assert u.zpoly_plan([1.7], [0])['cls'] == [CONST]
    u.apply_zpoly([1.7], [0], -0.9j)
    got = u.download()
    assert np.all(got == got[0])
    want = complex(np.complex128(_dtype(bw)(2.0 ** -(n / 2) * (0.6 + 0.8j)))) * np.exp(-0.9j * 1.7)
    assert abs(complex(got[0]) - want) <= zu.apply_bound(bw, [1.7], -0.9j, 2.0 ** -(n / 2))
  _apply_checked(st, [1.7], [0], -0.9j, f'a constant term, bw = {bw}')
  # apply(c) then apply(-c) returns the state within twice the bound
  before = _held(st)
  for c in (-0.8j, 0.1 - 0.4j):
    st.apply_zpoly(ws, zs, c)
    st.apply_zpoly(ws, zs, -c)
    back = _held(st)
    amax = float(np.max(np.abs(before)))
    grow = math.exp(abs(c.real) * zu.big_f(ws))              # the first error passes through the second factor
    tol = grow * zu.apply_bound(bw, ws, c, amax) + zu.apply_bound(bw, ws, c, amax * grow)
    err = _maxerr(back, before)
    print(f'apply({c}) then apply({-c}), bw = {bw}: {err:.3e} (twice the bound: {tol:.3e})')
    assert err <= tol
    before = back


# ---- 4. small states and the first main shapes -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('bw', [128, 64])
def test_small_states_and_first_main_shapes(bw):
  """every size of the small kernel (1 .. 10 + amp_bits local bits) and the first two of the main shape"""
  ab = _amp_bits(bw)
  for n in range(1, CHUNK_BITS + ab + 2):
    rng = np.random.default_rng(40 + n + bw)
    with device.DeviceState(n, bw) as st:
      st.upload(_random_state(n, 40 + n))
      if n >= 3:
        st.remap_swap(0, n - 1)
      T = 7
      zs = [int(v) for v in rng.integers(0, 1 << n, size=T)]
      zs[2], zs[5] = 0, (1 << n) - 1
      ws = [float(v) for v in rng.uniform(-2, 2, size=T)]
      p = st.zpoly_plan(ws, zs)
      assert p['kernel'] == (SMALL if n < CHUNK_BITS + ab else MAIN), n
      if p['kernel'] == MAIN:
        assert p['nblk'] == 1 << (n - CHUNK_BITS - ab) and p['cpb'] == 1
      _apply_checked(st, ws, zs, -0.6j, f'n = {n}, imaginary c, bw = {bw}')
      _apply_checked(st, ws, zs, 0.05 + 0.2j, f'n = {n}, complex c, bw = {bw}')
      _expect_checked(st, ws, zs, f'n = {n}, bw = {bw}')


# ---- 5. blocks that walk more than one chunk ---------------------------------------------------------------------------------------------
def _f_blocks(n, ws, zs, rows_bits=9):
  """f over ALL 2^n indices, a block of 2^(rows_bits + half) at a time: with the index split into a high and a low half of the
  bits, f = sum_t w_t s_t(high) s_t(low) is a matrix product of two sign tables.  Yields (start, f) in index order."""
  lo_bits = n // 2
  hi_bits = n - lo_bits
  lo_idx, hi_idx = np.arange(1 << lo_bits, dtype=np.uint64), np.arange(1 << hi_bits, dtype=np.uint64)
  s_lo = np.stack([1.0 - 2.0 * zu.parity(lo_idx, z & ((1 << lo_bits) - 1)).astype(np.float64) for z in zs])      # (T, 2^lo)
  s_hi = np.stack([(1.0 - 2.0 * zu.parity(hi_idx, z >> lo_bits).astype(np.float64)) * w for w, z in zip(ws, zs)], axis=1)      # (2^hi, T)
  rows = 1 << rows_bits
  for r in range(0, 1 << hi_bits, rows):
    yield r << lo_bits, (s_hi[r:r + rows] @ s_lo).reshape(-1)


@pytest.mark.parametrize('bw', [128, 64])
def test_blocks_that_walk_several_chunks(bw):
  """25 qubits at complex128, 26 at complex64 (512 MiB): 2^14 chunks over 4096 blocks, so a block walks four chunks and the two
  lowest bits of the chunk number change INSIDE a block.  Terms on those two bits, straddling terms on them (two of them in
  one group), top-bit, low-only and constant terms.  The layout is the identity, so the downloads are in logical order; NumPy
  checks a strided sample of 2^20 indices, and norm2 and the three moments over every amplitude, a slice at a time."""
  ab = _amp_bits(bw)
  n = CHUNK_BITS + BLOCK_CAP_BITS + 2 + ab
  cb = CHUNK_BITS + ab                                       # the lowest bit of the chunk number, as an amplitude bit
  rng = np.random.default_rng(25 + bw)
  host = (rng.random(2 << n, dtype=np.float32) - np.float32(0.5))
  host = host.astype(np.float64).view(np.complex128) if bw == 128 else host.view(np.complex64)
  flat_t = np.float64 if bw == 128 else np.float32

  def sumsq(flat):                                           # sum of squares in double, a slice at a time
    return float(sum(np.dot(part, part) for part in (flat[k:k + (1 << 22)].astype(np.float64) for k in range(0, flat.size, 1 << 22))))
  host *= flat_t(1.0 / math.sqrt(sumsq(host.view(flat_t))))
  top = 1 << (n - 1)
  zs = [1 << cb, (1 << cb) | (1 << (cb + 1)), top, (1 << cb) | 1, (1 << (cb + 1)) | (1 << (ab + 4)), top | (1 << (ab + 9)) | (1 << cb),
        (1 << (cb + 2)) | 1, 0b110, 0, (1 << (n - 2)) | (1 << (cb - 1)), (1 << (cb + 1)) | (1 << (ab + 7)) | 1]
  ws = [0.9, -1.3, 0.7, 1.1, -0.6, 1.7, 0.4, -2.1, 0.3, 1.2, -0.8]
  c = -0.9j
  with device.DeviceState(n, bw) as st:
    st.upload(host)
    p = st.zpoly_plan(ws, zs)
    assert p['kernel'] == MAIN and p['nblk'] == 4096 and p['cpb'] == 4
    assert (p['nconst'], p['nhigh'], p['nlow'], p['nstraddle'], p['ngroups']) == (1, 3, 1, 6, 5)
    s0 = st.stats()
    mom0 = st.expect_zpoly(ws, zs)
    n2 = st.apply_zpoly(ws, zs, c, norm=True)
    mom1 = st.expect_zpoly(ws, zs)
    sb = _shard_bytes(st)
    _grow(s0, st.stats(), gates_submitted=1, kernels_launched=3, bytes_swept=4 * sb, bytes_algorithmic=4 * sb)
    got = st.download()
  stride = (1 << n) >> 20
  idx = np.arange(0, 1 << n, stride, dtype=np.uint64) + rng.integers(0, stride, size=1 << 20).astype(np.uint64)
  sel = idx.astype(np.int64)
  want = zu.np_apply(host[sel], ws, zs, c, idx=idx)
  tol = zu.apply_bound(bw, ws, c, float(np.max(np.abs(host))))
  err = _maxerr(got[sel].astype(np.complex128), want)
  print(f'{n} qubits, bw = {bw}: error {err:.3e} on {idx.size} indices (bound {tol:.3e}, ratio {err / tol:.3f})')
  assert err <= tol
  # the sums over every amplitude: of the state before (moments) and after (norm2; |exp(c f)| = 1, so the moments again)
  m = np.zeros(3)
  n2_np = 0.0
  for start, f in _f_blocks(n, ws, zs):
    a = host[start:start + f.size].astype(np.complex128)
    pr = a.real * a.real + a.imag * a.imag
    m += [float(np.sum(pr)), float(np.dot(pr, f)), float(np.dot(pr, f * f))]
    g = got[start:start + f.size].astype(np.complex128)
    n2_np += float(np.sum(g.real * g.real + g.imag * g.imag))
  eps_w = 2.0 ** -52 if bw == 128 else 2.0 ** -23
  for k in range(3):
    tol_k = zu.moment_bound(ws, k, m[0])
    print(f'{n} qubits, bw = {bw}: moment {k}: {mom0[k]:.17g}, NumPy {m[k]:.17g}, error {abs(mom0[k] - m[k]):.3e} (bound {tol_k:.3e}, '
          f'ratio {abs(mom0[k] - m[k]) / tol_k:.3f}); after the phases {mom1[k]:.17g}')
    assert abs(mom0[k] - m[k]) <= tol_k
    # the stored result differs from the exact product by one rounding per component: 2 eps relative in each probability
    assert abs(mom1[k] - m[k]) <= tol_k + 4 * eps_w * zu.big_f(ws) ** k * m[0]
  print(f'{n} qubits, bw = {bw}: norm2 {n2:.17g}, NumPy on the stored values {n2_np:.17g}')
  assert abs(n2 - n2_np) <= zu.moment_bound(ws, 0, n2_np) and mom1[0] == pytest.approx(n2, rel=1e-12)


# ---- 6. the moments ---------------------------------------------------------------------------------------------------------------
def test_expect_against_the_model_and_expect_pauli(permuted14):
  bw, st = permuted14
  n = st.nbits
  rng = np.random.default_rng(600 + bw)
  T = 24
  zs = [int(v) for v in rng.integers(1, 1 << n, size=T)]
  zs[4] = zs[9]
  ws = [float(v) for v in rng.uniform(-1.5, 1.5, size=T)]
  out = _expect_checked(st, ws, zs, f'{T} random terms, bw = {bw}')
  # the same mean through qh_expect_pauli: sum_t w_t <Z_t>.  Each <Z_t> is a signed sum of probabilities in a fixed order of
  # fewer than 160 additions on any path: 160 * 2^-52 norm2; the dot product with w adds T roundings of at most F norm2
  zt = st.expect_pauli([0] * T, zs)
  mean_p = float(np.dot(np.asarray(ws), zt))
  tol = zu.moment_bound(ws, 1, out[0]) + (160 + T) * 2.0 ** -52 * zu.big_f(ws) * out[0]
  print(f'mean {out[1]:.17g}, through expect_pauli {mean_p:.17g}: {abs(out[1] - mean_p):.3e} (sum of both bounds {tol:.3e})')
  assert abs(out[1] - mean_p) <= tol
  # with a constant term the second moment is that of f + w0: <(f + w0)^2> = <f^2> + 2 w0 <f> + w0^2 norm2
  out2 = st.expect_zpoly(ws + [0.75], zs + [0])
  want2 = out[2] + 2 * 0.75 * out[1] + 0.75 ** 2 * out[0]
  assert abs(out2[2] - want2) <= 2 * zu.moment_bound(ws + [0.75], 2, out[0])


# ---- 7. queue and barrier, handles ---------------------------------------------------------------------------------------------------
TERMS = ([0.8, -1.2, 0.5, 0.3, 1.1, -0.4], [0b101, 1 << 9, (1 << 11) | 1, 0, (1 << 10) | (1 << 3), (1 << 11) | (1 << 10) | (1 << 6)])


def _had(v, q):
  t = v.reshape(1 << q, 2, -1)
  return np.stack([t[:, 0] + t[:, 1], t[:, 0] - t[:, 1]], axis=1).reshape(-1) / np.sqrt(2.0)


@pytest.mark.parametrize('bw', [128, 64])
def test_queue_and_barrier(bw):
  """gates left queued before either call run first; gates queued after it are applied on top; nothing is pending after it"""
  n = 12
  ws, zs = TERMS
  c = -0.45j
  with _permuted(n, bw, 62) as st:
    relay = st.set_relayout(True)
    before = _held(st)
    st.apply1(gates.hadamard(), 3)                           # queued (reference qubit 3 = logical bit n - 1 - 3)
    assert _pending(st) == 1
    st.apply_zpoly(ws, zs, c)
    assert _pending(st) == 0
    gate_eps = 2.0 ** -50 if bw == 128 else 2.0 ** -22      # the Hadamard itself: two roundings per component
    after_gate = _had(before, 3)
    want = zu.np_apply(after_gate, ws, zs, c)
    amax = float(np.max(np.abs(after_gate)))
    tol = zu.apply_bound(bw, ws, c, amax) + gate_eps * amax
    got = _held(st)
    print(f'queued gate then apply_zpoly, bw = {bw}: {_maxerr(got, want):.3e} (tolerance {tol:.3e})')
    assert _maxerr(got, want) <= tol
    assert st.set_relayout(True) == relay                    # relayout mode as before: fused gates afterwards still work
    st.apply1(gates.hadamard(), 0)
    assert _pending(st) == 1
    out = st.expect_zpoly(ws, zs)                            # a reader: the queued gate runs first
    assert _pending(st) == 0
    want2 = _had(got, 0)
    m = zu.np_moments(want2, ws, zs)
    for k in range(3):
      assert abs(out[k] - m[k]) <= zu.moment_bound(ws, k, m[0]) + 8 * gate_eps * zu.big_f(ws) ** k * m[0]
    assert np.max(np.abs(_held(st) - want2)) <= 4 * gate_eps * float(np.max(np.abs(got)))


@pytest.mark.parametrize('bw', [128, 64])
def test_attached_and_host_mapped_handles(bw):
  n = 12
  ws, zs = TERMS
  with device.DeviceState(n, bw) as owner:
    ptr = owner.device_ptr
    with device.DeviceState(n, bw, device_ptr=ptr) as att:
      att.upload(_random_state(n, 61))
      att.remap_swap(1, 9)
      _apply_checked(att, ws, zs, -0.5j, f'attached handle, bw = {bw}')
      _expect_checked(att, ws, zs, f'attached handle, bw = {bw}')
      assert att.device_ptr == ptr
  with device.DeviceState(n, bw, host_mapped=True) as hm:
    ptr = hm.device_ptr
    hm.upload(_random_state(n, 62))
    hm.remap_swap(1, 9)
    _, got = _apply_checked(hm, ws, zs, 0.1 - 0.5j, f'host-mapped handle, bw = {bw}')
    _expect_checked(hm, ws, zs, f'host-mapped handle, bw = {bw}')
    hm.sync()
    lo = shard_util.logical_of_phys(shard_util.bitmap(hm), 1 << n).astype(np.int64)      # the mapped memory itself, as it lies
    mapped = np.empty(1 << n, dtype=np.complex128)
    mapped[lo] = np.asarray(hm.host_array()).reshape(-1)
    assert mapped.tobytes() == got.tobytes()
    assert hm.device_ptr == ptr


def test_refusals_change_nothing():
  with device.DeviceState(8, 128, fusion=native.QH_FUSE_SWEEP) as st:
    st.upload(_random_state(8, 1))
    st.remap_swap(0, 5)
    want, bm = _held(st), shard_util.bitmap(st)
    st.apply1(gates.hadamard(), 2)
    s0 = st.stats()
    for call, code in ((lambda: st.apply_zpoly([1.0, np.inf], [1, 2], -1j, norm=True), native.QH_ERR_ARG),
                       (lambda: st.apply_zpoly([1.0, 2.0], [1, 1 << 8], -1j), native.QH_ERR_BAD_QUBIT),
                       (lambda: st.apply_zpoly([1.0, 2.0], [1, 2], complex(np.nan, 0.0)), native.QH_ERR_ARG),
                       (lambda: st.expect_zpoly([1.0, np.nan], [1, 2]), native.QH_ERR_ARG),
                       (lambda: st.expect_zpoly([1.0, 2.0], [1, 1 << 8]), native.QH_ERR_BAD_QUBIT)):
      with pytest.raises(native.QhError) as e:
        call()
      assert e.value.code == code
      assert 'term 1' in str(e.value) or 'not finite' in str(e.value)
    assert _pending(st) == 1 and st.stats() == s0 and shard_util.bitmap(st) == bm      # nothing flushed
    st.flush()
    assert np.max(np.abs(_held(st) - _had(want, 2))) <= 2.0 ** -50


# ---- 8. shard handles ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('nloc,nglob', [(10, 12), (13, 15)])
@pytest.mark.parametrize('bw', [128, 64])
def test_shard_handles(bw, nloc, nglob):
  """qh_set_shard on one GPU, below and on the main shape, every shard index: a z bit the shard index holds is a sign per
  shard, folded into the weight; terms on shard bits only, on local bits only and on both.  The shards are assembled and
  compared with the model on the GLOBAL state; the moments are summed over the shards."""
  full = _random_state(nglob, 71).astype(_dtype(bw)).astype(np.complex128)      # as stored
  h0, h1 = 1 << nloc, 1 << (nloc + 1)
  zs = [h0, h0 | h1, h1 | 1, h0 | (1 << (nloc - 1)) | 4, 0b1010, (1 << (nloc - 1)) | 1, 0, h0 | h1 | (1 << (nloc - 2)), 1 << (nloc - 1)]
  ws = [0.7, -1.1, 0.9, 1.3, -0.5, 0.6, 0.2, -1.4, 0.8]
  c = 0.05 - 0.6j
  got = np.zeros(1 << nglob, dtype=np.complex128)
  mom = np.zeros(3)
  for shard in range(1 << (nglob - nloc)):
    with device.DeviceState(nloc, bw) as s:
      s.set_shard(nglob, shard)
      s.upload(full[shard << nloc:(shard + 1) << nloc])
      s.remap_swap(2, 7)                                    # local bits anywhere (this relabels the state: read it back)
      with s.clone() as k:
        lo_s, phys_s = _logical_state(k, shard, nglob)
      assert np.all(lo_s >> nloc == shard)
      full[lo_s] = phys_s                                    # the global state as the shards really hold it
      p = s.zpoly_plan(ws, zs)
      assert p['w'] == [-w if bin(shard & (z >> nloc)).count('1') % 2 else w for w, z in zip(ws, zs)]
      assert p['cls'][:2] == [CONST, CONST] and p['nconst'] == 3
      s0 = s.stats()
      mom += s.expect_zpoly(ws, zs)
      n2 = s.apply_zpoly(ws, zs, c, norm=True)
      sb = _shard_bytes(s)
      _grow(s0, s.stats(), gates_submitted=1, kernels_launched=2, bytes_swept=3 * sb, bytes_algorithmic=3 * sb)
      with s.clone() as k:
        lo, phys = _logical_state(k, shard, nglob)
      assert np.array_equal(lo, lo_s)
      got[lo] = phys
      assert abs(n2 - float(np.vdot(phys, phys).real)) <= 1e-12 * n2
  want = zu.np_apply(full, ws, zs, c)
  tol = zu.apply_bound(bw, ws, c, float(np.max(np.abs(full))))
  err = _maxerr(got, want)
  print(f'{1 << (nglob - nloc)} shards of {nloc} bits, bw = {bw}: error {err:.3e} (bound {tol:.3e}, ratio {err / tol:.3f})')
  assert err <= tol
  m = zu.np_moments(full, ws, zs)
  for k in range(3):
    tol_k = zu.moment_bound(ws, k, m[0]) + 4 * 2.0 ** -52 * zu.big_f(ws) ** k * m[0]      # (and the sum over four shards)
    print(f'  moment {k} over the shards: {mom[k]:.17g}, model {m[k]:.17g} (bound {tol_k:.3e})')
    assert abs(mom[k] - m[k]) <= tol_k


# ---- 9. end to end through qc ---------------------------------------------------------------------------------------------------------
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


def _zmasks(n, terms):
  return [float(w) for w, _ in terms], [sum(1 << (n - 1 - q) for q, p in paulis.items() if p == 'Z') for _, paulis in terms]


def _graph(n, seed):
  rng = np.random.default_rng(seed)
  edges = [(q, (q + 1) % n, float(rng.uniform(0.2, 1.0))) for q in range(n)]
  edges += [(int(a), int(b), float(rng.uniform(0.2, 1.0))) for a, b in (rng.choice(n, size=2, replace=False) for _ in range(n // 2))]
  return edges


def test_qc_phase_polynomial_against_evolve(width):
  """exp(-i gamma C) in one pass against the same factors one by one through qc.evolve (qh_apply_pauli_product), within the sum
  of both bounds; each against the model as well"""
  n, gamma = 12, 0.37
  terms = circuit.qc.maxcut_terms(_graph(n, 3)) + [(0.4, {q: 'Z'}) for q in range(0, n, 3)] + [(-0.3, {})]
  ws, zs = _zmasks(n, terms)
  qa, qb = circuit.qc('zpoly'), circuit.qc('evolve')
  for q in (qa, qb):
    q.reg(n, 0)
    _layers(q, n, 5)
  assert hasattr(qa._ensure_device(), 'apply_zpoly')        # pylint: disable=protected-access
  psi = _amps(qa)
  amax = float(np.max(np.abs(psi)))
  qa.phase_polynomial(terms, gamma)
  qb.evolve(terms, gamma)
  a, b = [math.cos(gamma * w) for w in ws], [-1j * math.sin(gamma * w) for w in ws]
  tol_z, tol_e = zu.apply_bound(width, ws, -1j * gamma, amax), ppu.bound(width, a, b, amax, len(ws))
  err = _maxerr(_amps(qa), _amps(qb))
  err_m = _maxerr(_amps(qa), zu.np_apply(psi, ws, zs, -1j * gamma))
  print(f'phase_polynomial against evolve, width {width}: {err:.3e} (bounds {tol_z:.3e} + {tol_e:.3e}); against the model {err_m:.3e}')
  assert err <= tol_z + tol_e and err_m <= tol_z


def test_qc_cost_filter_and_expectation(width):
  n = 12
  terms = circuit.qc.maxcut_terms(_graph(n, 4)) + [(0.5, {1: 'Z', 4: 'Z', 7: 'Z'})]
  ws, zs = _zmasks(n, terms)
  q = circuit.qc('filter')
  q.reg(n, 0)
  _layers(q, n, 7)
  psi = _amps(q)
  mean, second = q.cost_expectation(terms, moments=True)
  m = zu.np_moments(psi, ws, zs)
  assert abs(mean - m[1]) <= zu.moment_bound(ws, 1, m[0]) and abs(second - m[2]) <= zu.moment_bound(ws, 2, m[0])
  via_pauli = q.expectation(terms)
  tol = zu.moment_bound(ws, 1, m[0]) + (160 + len(ws)) * 2.0 ** -52 * zu.big_f(ws) * m[0]
  print(f'cost_expectation {mean:.17g}, expectation {via_pauli:.17g}: {abs(mean - via_pauli):.3e} (sum of both bounds {tol:.3e})')
  assert abs(mean - via_pauli) <= tol and q.cost_expectation(terms) == mean
  tau = 0.15
  norm2 = q.cost_filter(terms, tau)
  want = zu.np_apply(psi, ws, zs, -tau)
  n2_want = float(np.vdot(want, want).real)
  assert abs(norm2 - n2_want) <= (1e-12 if width == 128 else 1e-5) * n2_want
  tol = zu.apply_bound(width, ws, -tau, float(np.max(np.abs(psi)))) / math.sqrt(n2_want) + 4 * (2.0 ** -52 if width == 128 else 2.0 ** -23)
  assert _maxerr(_amps(q), want / math.sqrt(n2_want)) <= tol
  assert abs(q.norm2() - 1.0) <= (1e-12 if width == 128 else 1e-6)
  lower = q.cost_expectation(terms)
  assert lower < mean                                        # the filter moved weight towards low cost
  # a filter that leaves nothing: exp(-800) underflows to 0 on every amplitude
  with pytest.raises(ValueError):
    q.cost_filter([(1.0, {})], 800.0)


def _np_rx_all(v, n, beta):
  rx = np.array([[math.cos(beta), -1j * math.sin(beta)], [-1j * math.sin(beta), math.cos(beta)]])
  for k in range(n):
    t = v.reshape(1 << k, 2, -1)
    v = np.einsum('ab,xbr->xar', rx, t).reshape(-1)
  return v


def test_qc_two_layer_qaoa(width):
  """two QAOA layers on a 12-node graph from the uniform superposition against NumPy.  The mixer is 12 one-qubit gates per
  layer through the normal queue, each two roundings per component in the handle's width"""
  n = 12
  edges = _graph(n, 8)
  terms = circuit.qc.maxcut_terms(edges)
  ws, zs = _zmasks(n, terms)
  q = circuit.qc('qaoa')
  q.reg(n, 0)
  for k in range(n):
    q.h(k)
  v = np.full(1 << n, 2.0 ** -(n / 2), dtype=np.complex128)
  eps = 2.0 ** -52 if width == 128 else 2.0 ** -23
  tol = 4 * n * eps * 2.0 ** -(n / 2)                        # the Hadamards
  for gamma, beta in ((0.31, 0.52), (0.47, 0.23)):
    q.qaoa_layer(terms, gamma, beta)
    v = _np_rx_all(zu.np_apply(v, ws, zs, -1j * gamma), n, beta)
    tol += zu.apply_bound(width, ws, -1j * gamma, float(np.max(np.abs(v)))) + 4 * n * eps * float(np.max(np.abs(v)))
  got = _amps(q)
  err = _maxerr(got, v)
  print(f'two QAOA layers, width {width}: {err:.3e} (tolerance {tol:.3e})')
  assert err <= tol
  e = q.cost_expectation(terms)
  m = zu.np_moments(v, ws, zs)
  assert abs(e - m[1]) <= zu.moment_bound(ws, 1, m[0]) + 2 * tol * zu.big_f(ws) * 2.0 ** (n / 2)


def test_golden_maxcut_of_the_reference(width):
  """the reference's MaxCut diagonals (graph_to_diagonal_h; the weight is w^2, node q on bit n - 1 - q): from the uniform
  superposition, phase_polynomial gives exp(-i gamma diag) / sqrt(2^n) at every amplitude, cost_expectation gives mean(diag)
  and mean(diag^2), and with gamma * sum w^2 < pi the phases do not wrap: the extreme phases qc.top finds sit on argmin and
  argmax of the diagonal"""
  g = np.load(os.path.join(ROOT, 'tests', 'golden', 'g15_maxcut_diag.npz'))
  for n in (8, 10, 12):
    edges, diag = g[f'edges{n}'], g[f'diag{n}']
    terms = circuit.qc.maxcut_terms([(int(u), int(v), w * w) for u, v, w in edges])
    ws, _ = _zmasks(n, terms)
    F = zu.big_f(ws)
    gamma = 3.0 / F
    assert gamma * F <= 40 and gamma * F < math.pi
    q = circuit.qc('maxcut')
    q.reg(n, 0)
    for k in range(n):
      q.h(k)
    amp0 = _amps(q)
    mean, second = q.cost_expectation(terms, moments=True)
    n2 = float(np.vdot(amp0, amp0).real)
    p0 = amp0.real ** 2 + amp0.imag ** 2
    assert abs(mean - float(np.dot(p0, diag))) <= zu.moment_bound(ws, 1, n2)
    assert abs(second - float(np.dot(p0, diag * diag))) <= zu.moment_bound(ws, 2, n2)
    eps = 2.0 ** -52 if width == 128 else 2.0 ** -23
    assert abs(mean - float(np.mean(diag))) <= zu.moment_bound(ws, 1, n2) + 4 * n * eps * F
    assert abs(second - float(np.mean(diag * diag))) <= zu.moment_bound(ws, 2, n2) + 4 * n * eps * F * F
    q.phase_polynomial(terms, gamma)
    got = _amps(q)
    tol = zu.apply_bound(width, ws, -1j * gamma, float(np.max(np.abs(amp0))))
    err = _maxerr(got, amp0 * np.exp(-1j * gamma * diag))
    err_u = _maxerr(got, np.exp(-1j * gamma * diag) / math.sqrt(1 << n))
    print(f'reference MaxCut diagonal, n = {n}, width {width}: {err:.3e} (bound {tol:.3e}, ratio {err / tol:.3f}); against 2^-n/2: {err_u:.3e}')
    assert err <= tol and err_u <= tol + 4 * n * eps * 2.0 ** -(n / 2)
    top = q.top(1 << n)
    assert len(top) == 1 << n
    idx = np.array([helper.bits2val(bits) for bits, _, _ in top])
    ang = np.array([np.angle(a) for _, a, _ in top])
    hi, lo = int(idx[np.argmax(ang)]), int(idx[np.argmin(ang)])
    mask = (1 << n) - 1                                      # a cut and its complement cost the same
    if width == 128:
      assert hi in (int(np.argmin(diag)), int(np.argmin(diag)) ^ mask) and lo in (int(np.argmax(diag)), int(np.argmax(diag)) ^ mask)
    delta = 16 * eps / gamma                                 # a stored amplitude's phase is good to a few eps: ties within that
    assert diag[hi] - np.min(diag) <= delta and np.max(diag) - diag[lo] <= delta
