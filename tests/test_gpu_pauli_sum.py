"""Pauli-sum operators on the MI355X: qh_apply_pauli_sum / qh_pauli_sum_new (dst := (sum_t c_t P_t) src, out of place)
against pauli_util.np_pauli_sum -- NumPy in complex128 on the amplitudes as stored -- at both widths: the exact cases on a
layout a fused QFT flush has permuted, batching and stats against qh_pauli_sum_plan, every size of the small-state kernel
and one where a block walks two chunks, the contract for both handles, shard handles on one GPU, and qc.hamiltonian_times /
variance / apply_hamiltonian end to end.

Tolerance (pauli_util.bound, derived, not measured): per component (nterms + 4) * 2^-52 * C * amax at complex128, plus
nbatches * 2^-23 * C * amax at complex64, with C = sum |c_t| and amax = max |src_i|.  Wherever the contract says exact, ==.

qh_download re-lays a permuted state out, so the handles under test are downloaded LAST; what they held before a call is read
from clones."""
import ctypes

import numpy as np
import pytest

from qcc_amd import device, gates, native, workloads
from qcc_amd.lib import circuit, tensor
from tests import pauli_util, shard_util

pytestmark = pytest.mark.gpu

_dp = ctypes.POINTER(ctypes.c_double)
_up = ctypes.POINTER(ctypes.c_uint64)
# the kernel's own constants (qcc_amd/csrc/pauli_plan.h): 256 threads x 8 items of 16 bytes per chunk, 4096 blocks at most
CHUNK_BITS, BLOCK_CAP_BITS = 11, 12


def _amp_bits(bw):
  return 0 if bw == 128 else 1


def _logical_state(st, shard=0, nglob=None):
  phys = st.download().astype(np.complex128)
  lo = shard_util.phys_to_logical(st, shard, np.arange(phys.size), nglob or st.nbits).astype(np.int64)
  return lo, phys


def _logical(st):
  """the handle's amplitudes as stored, in logical order (re-lays the handle out: last)"""
  lo, phys = _logical_state(st)
  out = np.empty_like(phys)
  out[lo] = phys
  return out


def _before(st):
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


def _logical_bit_at(st, phys):
  return shard_util.bitmap(st).index(phys)


def _shard_bytes(st):
  return (1 << st.nbits) * (16 if st.bit_width == 128 else 8)


def _predict(src, xs, zs):
  """what qh_pauli_sum_plan says dst's stats grow by"""
  _, batches = src.pauli_sum_plan(xs, zs)
  sb = _shard_bytes(src)
  if not batches:
    return dict(kernels_launched=1, bytes_swept=sb, bytes_algorithmic=sb), 1
  return dict(kernels_launched=len(batches), bytes_swept=sum(b['streams'] for b in batches) * sb, bytes_algorithmic=2 * sb), len(batches)


def _apply_checked(src, dst, coeffs, xs, zs, src_logical, what, exact=False):
  """dst := H src with stats and norm2 checked; returns (dst in logical order, norm2).  dst=None: qh_pauli_sum_new."""
  bw = src.bit_width
  bm, ks = shard_util.bitmap(src), src.stats()
  grow, nbatches = _predict(src, xs, zs)
  kd = dst.stats() if dst is not None else dict(kernels_launched=0, bytes_swept=0, bytes_algorithmic=0)
  new, n2 = src.apply_pauli_sum(coeffs, xs, zs, out=dst, norm=True)
  try:
    kd2 = new.stats()
    for k, v in grow.items():
      assert kd2[k] - kd[k] == v, (what, k, kd2[k] - kd[k], v)
    assert src.stats() == ks and shard_util.bitmap(src) == bm, what          # src: read only
    assert shard_util.bitmap(new) == bm, what                                  # dst takes src's bit map
    _, n2b = src.apply_pauli_sum(coeffs, xs, zs, out=new, norm=True)          # the same call again: the same bits
    assert n2b == n2, (what, n2, n2b)
    got = _logical(new)
  finally:
    if dst is None:
      new.close()
  want = pauli_util.np_pauli_sum(src_logical, coeffs, xs, zs)
  amax = float(np.max(np.abs(src_logical)))
  b = pauli_util.bound(bw, coeffs, amax, nbatches)
  csum = float(sum(abs(complex(c)) for c in coeffs))
  err = float(max(np.max(np.abs(got.real - want.real)), np.max(np.abs(got.imag - want.imag))))
  n2_np = float(np.vdot(got, got).real)
  n2_want = float(np.vdot(want, want).real)
  n2_tol = 4 * csum * amax * b * got.size
  print(f'{what}: error {err:.3e} (bound {b:.3e}); norm2 {n2:.17g}, NumPy {n2_want:.17g} (tolerance {n2_tol:.3e})')
  if exact:
    dt = np.complex128 if bw == 128 else np.complex64
    assert np.array_equal(got, want.astype(dt).astype(np.complex128)), what
  assert err <= b, (what, err, b)
  assert abs(n2 - n2_want) <= n2_tol and abs(n2 - n2_np) <= 1e-12 * max(1.0, n2_np), (what, n2, n2_want, n2_np)
  return got, n2


@pytest.fixture(scope='module', params=[128, 64])
def permuted14(request):
  """(bw, src handle at 14 qubits in a permuted layout, its amplitudes in logical order); the tests only read it"""
  bw = request.param
  st = _permuted(14, bw, 14 + bw)
  logical = _before(st)
  yield bw, st, logical
  st.close()


# ---- 1. exactness on a permuted layout ---------------------------------------------------------------------------------------
def _position_classes(n, bw):
  """physical AMPLITUDE-index positions of each class of the kernel's walk: sub-item (complex64), inside a 128-byte line, on
  a lane bit outside it, wave / register-index / chunk bits, the top bit"""
  ab = _amp_bits(bw)
  cls = {'line': ab + 1, 'lane': ab + 4, 'wave': ab + 7, 'register-index': ab + 9, 'chunk': ab + CHUNK_BITS, 'top': n - 1}
  if ab:
    cls['sub-item'] = 0
  assert cls['chunk'] < n - 1
  return cls


def test_single_terms_are_exact_on_a_permuted_layout(permuted14):
  """One term with coefficient 1, -1 and -i: == NumPy.  The x bit (then the z bit, then both: Y) sits, by PHYSICAL position
  in the layout the QFT flush left, on each class of index bit of the walk; then mixed masks and a weight-n XYZ string."""
  bw, src, logical = permuted14
  n = src.nbits
  cls = _position_classes(n, bw)
  at = {name: 1 << _logical_bit_at(src, p) for name, p in cls.items()}
  masks = []
  for name, bit in at.items():
    masks += [(f'X on the {name} bit', bit, 0), (f'Z on the {name} bit', 0, bit), (f'Y on the {name} bit', bit, bit)]
  mixed = at['line'] | at['wave'] | at['chunk'] | at['top'] | at.get('sub-item', 0)
  zmix = at['lane'] | at['register-index'] | at['chunk'] | at.get('sub-item', 0)
  masks += [('mixed X', mixed, 0), ('mixed Z (thread, register-index and chunk parts)', 0, zmix | at['wave']), ('mixed X and Z', mixed, zmix)]
  rng = np.random.default_rng(1)
  letters = rng.integers(1, 4, size=n)                     # X, Z or Y on every qubit
  masks.append(('weight-n XYZ string', sum(1 << b for b in range(n) if letters[b] & 1), sum(1 << b for b in range(n) if letters[b] & 2)))
  with device.DeviceState(n, bw) as dst:
    for k, (name, x, z) in enumerate(masks):
      for c in (1.0, -1.0, -1j):
        _apply_checked(src, dst if k % 2 else None, [c], [x], [z], logical, f'{name}, c = {c}, bw = {bw}', exact=True)


# ---- 2. batching and stats ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('count,nx', [(1, 1), (4, 1), (4, 3), (5, 1), (5, 3), (16, 1), (16, 3), (17, 1), (17, 3), (17, 17), (40, 1), (40, 3),
                                      (40, 20)])
def test_batches_values_stats_and_norm(permuted14, count, nx):
  """1, 4 (the small instantiation), 5, 16, 17 (a second, accumulating batch) and 40 terms over 1, 3 and 17+ distinct x
  masks in equal runs, so that a cut splits a group: values within the bound, kernels_launched / bytes_swept /
  bytes_algorithmic as qh_pauli_sum_plan predicts, norm2 against NumPy and bitwise equal on a repeated call."""
  bw, src, logical = permuted14
  n = src.nbits
  rng = np.random.default_rng(1000 * count + nx)
  xpool = [int(v) for v in rng.integers(0, 1 << n, size=nx)]
  xpool[0] = 0 if nx > 1 else xpool[0]                      # a diagonal group among them
  order = rng.permutation(count)                            # given unsorted
  xs = [xpool[(int(k) * nx) // count] for k in order]
  zs = [int(v) for v in rng.integers(0, 1 << n, size=count)]
  coeffs = [complex(a, b) for a, b in rng.normal(size=(count, 2))]
  _, batches = src.pauli_sum_plan(xs, zs)
  assert len(batches) == -(-count // 16)
  if count == 40 and nx == 3:
    assert sum(b['ngroups'] for b in batches) > len(set(xs))      # a group split by a cut
  with device.DeviceState(n, bw) as dst:
    dst.upload(np.full(1 << n, np.nan + 1j * np.nan))      # batch 0 does not read dst
    _apply_checked(src, dst, coeffs, xs, zs, logical, f'{count} terms, {nx} x masks, bw = {bw}')


def test_no_terms_is_one_kernel_of_zeros(permuted14):
  bw, src, logical = permuted14
  with device.DeviceState(src.nbits, bw) as dst:
    dst.upload(np.full(1 << src.nbits, np.nan + 1j * np.nan))
    got, n2 = _apply_checked(src, dst, [], [], [], logical, f'no terms, bw = {bw}', exact=True)
    assert n2 == 0.0 and not np.any(got)


# ---- 3. sizes ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('bw', [128, 64])
@pytest.mark.parametrize('n', range(1, 10))
def test_small_states(n, bw):
  """every local size from 1 to 9 qubits: the one-amplitude-per-thread kernel (one block up to 8 qubits, two at 9)"""
  rng = np.random.default_rng(n)
  with device.DeviceState(n, bw) as src, device.DeviceState(n, bw) as dst:
    src.upload(_random_state(n, 30 + n))
    if n > 1:
      src.remap_swap(0, n - 1)
    logical = _before(src)
    for count, exact in ((1, True), (5, False), (20, False)):
      xs = [int(v) for v in rng.integers(0, 1 << n, size=count)]
      zs = [int(v) for v in rng.integers(0, 1 << n, size=count)]
      coeffs = [-1j] if exact else [complex(a, b) for a, b in rng.normal(size=(count, 2))]
      _apply_checked(src, dst if count != 5 else None, coeffs, xs, zs, logical, f'n = {n}, {count} terms, bw = {bw}', exact=exact)
    _apply_checked(src, dst, [], [], [], logical, f'n = {n}, no terms, bw = {bw}', exact=True)


@pytest.mark.parametrize('bw,n', [(128, 11), (64, 12), (64, 11)])
def test_threshold_between_the_two_kernels(bw, n):
  """the smallest states of the main shape (one chunk: 2^11 16-byte items) and, at complex64, the largest small one"""
  rng = np.random.default_rng(n + bw)
  with device.DeviceState(n, bw) as src:
    src.upload(_random_state(n, 50 + n))
    src.remap_swap(1, n - 2)
    logical = _before(src)
    xs = [int(v) for v in rng.integers(0, 1 << n, size=3)] * 7
    zs = [int(v) for v in rng.integers(0, 1 << n, size=21)]
    coeffs = [complex(a, b) for a, b in rng.normal(size=(21, 2))]
    _apply_checked(src, None, coeffs, xs, zs, logical, f'threshold n = {n}, bw = {bw}')


def test_blocks_that_walk_two_chunks():
  """n = 24 = chunk bits (11) + log2(block cap) (12) + 1 at complex128, where an item is one amplitude: 2^13 chunks over 4096
  blocks, so every block walks two chunks and the chunk number's lowest bit changes INSIDE a block.  Run at complex128 only
  (256 MiB per state; complex64 would need 25 qubits for the same walk).  The layout is the identity, so the downloads are in
  logical order; NumPy checks 2^16 random amplitudes and the first and last two chunks."""
  n = CHUNK_BITS + BLOCK_CAP_BITS + 1
  rng = np.random.default_rng(24)
  host = (rng.random(2 << n, dtype=np.float32) - np.float32(0.5)).astype(np.float64).view(np.complex128)
  host *= 1.0 / np.sqrt(float(np.vdot(host, host).real))
  xs = [1 << (n - 1), (1 << CHUNK_BITS) | 5, (1 << CHUNK_BITS) | 5, 0]
  zs = [(1 << CHUNK_BITS) | (1 << (CHUNK_BITS + 1)), 1 << CHUNK_BITS, (1 << (n - 1)) | (1 << 9), (1 << CHUNK_BITS) | (1 << 7)]
  coeffs = [0.5 - 0.25j, 1.5, -0.75j, 0.3]
  with device.DeviceState(n, 128) as src:
    src.upload(host)
    grow, nbatches = _predict(src, xs, zs)
    new, n2 = src.apply_pauli_sum(coeffs, xs, zs, norm=True)
    with new:
      assert {k: new.stats()[k] for k in grow} == grow
      _, n2b = src.apply_pauli_sum(coeffs, xs, zs, out=new, norm=True)
      assert n2b == n2
      got = new.download()
  at = np.concatenate([rng.integers(0, 1 << n, size=1 << 16), np.arange(0, 2 << CHUNK_BITS), np.arange((1 << n) - (2 << CHUNK_BITS), 1 << n)])
  want = pauli_util.np_pauli_sum(host, coeffs, xs, zs, at=at)
  b = pauli_util.bound(128, coeffs, float(np.max(np.abs(host))), nbatches)
  err = float(max(np.max(np.abs(got[at].real - want.real)), np.max(np.abs(got[at].imag - want.imag))))
  n2_np = float(np.vdot(got, got).real)
  print(f'24 qubits complex128: error {err:.3e} (bound {b:.3e}); norm2 {n2:.17g}, NumPy on the stored values {n2_np:.17g}')
  assert err <= b
  assert abs(n2 - n2_np) <= 1e-12 * n2_np


# ---- 4. handles ----------------------------------------------------------------------------------------------------------------
TERMS = ([0.8 - 0.3j, -0.4, 0.5j, 1.25, -0.6 + 0.1j], [0b101, 0, 0b101, 1 << 8, 0b11 << 6], [0b11, 0b1001 << 3, 1 << 8, 0b111, 1 << 7])


def _had(v, q):
  t = v.reshape(1 << q, 2, -1)
  return np.stack([t[:, 0] + t[:, 1], t[:, 0] - t[:, 1]], axis=1).reshape(-1) / np.sqrt(2.0)


@pytest.mark.parametrize('bw', [128, 64])
def test_dst_attached_and_host_mapped_keeps_its_buffer(bw):
  n = 12
  coeffs, xs, zs = TERMS
  with _permuted(n, bw, 61) as src:
    logical = _before(src)
    with device.DeviceState(n, bw) as owner:
      ptr = owner.device_ptr
      with device.DeviceState(n, bw, device_ptr=ptr) as att:
        _apply_checked(src, att, coeffs, xs, zs, logical, f'attached dst, bw = {bw}')
        assert att.device_ptr == ptr
    with device.DeviceState(n, bw, host_mapped=True) as hm:
      src.apply_pauli_sum(coeffs, xs, zs, out=hm)
      hm.sync()
      lo = shard_util.logical_of_phys(shard_util.bitmap(hm), 1 << n).astype(np.int64)      # the mapped memory itself, as it lies
      got = np.empty(1 << n, dtype=np.complex128)
      got[lo] = np.asarray(hm.host_array()).reshape(-1)
      want = pauli_util.np_pauli_sum(logical, coeffs, xs, zs)
      assert np.max(np.abs(got - want)) <= np.sqrt(2.0) * pauli_util.bound(bw, coeffs, float(np.max(np.abs(logical))))
      _apply_checked(src, hm, coeffs, xs, zs, logical, f'host-mapped dst, bw = {bw}')


@pytest.mark.parametrize('bw', [128, 64])
def test_dst_with_relayout_on_and_gates_queued_src_with_gates_queued(bw):
  """dst keeps its relayout mode and second buffer (fused gates on it afterwards still work) and drops what it had queued;
  what src has queued runs first"""
  n = 12
  coeffs, xs, zs = TERMS
  pend = ctypes.c_uint64()
  with _permuted(n, bw, 62) as src, device.DeviceState(n, bw, fusion=native.QH_FUSE_SWEEP) as dst:
    dst.upload(_random_state(n, 63))
    relay = dst.set_relayout(True)
    dst.apply1(gates.hadamard(), 2)                        # queued on dst: dropped
    logical = _before(src)
    src.apply1(gates.hadamard(), 3)                        # queued on src (reference qubit 3 = logical bit n - 1 - 3): runs
    for st in (dst, src):
      native.check(st.lib.qh_pending_gates(st.h, ctypes.byref(pend)))
      assert pend.value == 1
    src.apply_pauli_sum(coeffs, xs, zs, out=dst)
    for st in (dst, src):
      native.check(st.lib.qh_pending_gates(st.h, ctypes.byref(pend)))
      assert pend.value == 0
    after_gate = _had(logical, 3)
    want = pauli_util.np_pauli_sum(after_gate, coeffs, xs, zs)
    gate_eps = 2.0 ** -50 if bw == 128 else 2.0 ** -22      # the Hadamard itself: two roundings per component of src
    amax = float(np.max(np.abs(after_gate)))
    csum = float(sum(abs(c) for c in coeffs))
    tol = pauli_util.bound(bw, coeffs, amax) + csum * gate_eps * amax
    with dst.clone() as c:
      got = _logical(c)
    assert max(np.max(np.abs(got.real - want.real)), np.max(np.abs(got.imag - want.imag))) <= tol
    # fused gates on dst afterwards: the relayout mode and the second buffer are as they were
    assert dst.set_relayout(True) == relay
    dst.apply1(gates.hadamard(), 0)
    dst.apply1(gates.hadamard(), n - 1)
    dst.flush()
    want2 = _had(_had(got, 0), n - 1)
    got2 = _logical(dst)
    assert np.max(np.abs(got2 - want2)) <= 4 * gate_eps * float(np.max(np.abs(got)))


def test_refusals_change_nothing():
  lib = native.load()
  co = np.array([1.0, 0.0])
  x, z = np.array([3], dtype=np.uint64), np.array([5], dtype=np.uint64)
  args = (1, co.ctypes.data_as(_dp), x.ctypes.data_as(_up), z.ctypes.data_as(_up))
  with device.DeviceState(8, 128) as a, device.DeviceState(9, 128) as n9, device.DeviceState(8, 64) as w64, device.DeviceState(8, 128) as b:
    for st, seed in ((a, 1), (n9, 2), (w64, 3), (b, 4)):
      st.upload(_random_state(st.nbits, seed))
    a.remap_swap(0, 5)
    want_a, want_b, bm, st_a, st_b = _before(a), _before(b), shard_util.bitmap(a), a.stats(), b.stats()
    n2 = ctypes.c_double(7.0)
    for dst, src in ((a, a), (a, n9), (n9, a), (a, w64), (w64, a)):
      assert lib.qh_apply_pauli_sum(dst.h, src.h, *args, ctypes.byref(n2)) == native.QH_ERR_ARG
    assert lib.qh_apply_pauli_sum(None, a.h, *args, None) == native.QH_ERR_ARG
    assert lib.qh_apply_pauli_sum(b.h, None, *args, None) == native.QH_ERR_ARG
    assert lib.qh_apply_pauli_sum(b.h, a.h, 1, None, *args[2:], None) == native.QH_ERR_ARG
    big = np.array([1 << 8], dtype=np.uint64)
    assert lib.qh_apply_pauli_sum(b.h, a.h, 1, args[1], big.ctypes.data_as(_up), args[3], None) == native.QH_ERR_BAD_QUBIT
    out = ctypes.c_void_p()
    assert lib.qh_pauli_sum_new(a.h, 1, args[1], big.ctypes.data_as(_up), args[3], None, ctypes.byref(out)) == native.QH_ERR_BAD_QUBIT
    assert out.value is None and n2.value == 7.0
    assert a.stats() == st_a and b.stats() == st_b and shard_util.bitmap(a) == bm and shard_util.bitmap(b) == list(range(8))
    assert _before(a).tobytes() == want_a.tobytes() and _before(b).tobytes() == want_b.tobytes()


@pytest.mark.parametrize('bw', [128, 64])
def test_shard_handles(bw):
  """qh_set_shard on one GPU: a z bit the shard index holds flips the sign per shard; an x bit there is QH_ERR_NONLOCAL and
  dst is untouched"""
  nloc, nglob = 10, 12
  full = _random_state(nglob, 71)
  dt = np.complex128 if bw == 128 else np.complex64
  full = full.astype(dt).astype(np.complex128)              # as stored
  coeffs = [1.0, 0.5 - 0.5j, -0.25, 2.0j]
  xs = [0b11, 0b11, 1 << 9, 0]
  zs = [1 << 11, (1 << 10) | 4, (3 << 10) | (1 << 9), (1 << 11) | (1 << 10) | 1]
  b = pauli_util.bound(bw, coeffs, float(np.max(np.abs(full))))
  for shard in (1, 2):
    with device.DeviceState(nloc, bw) as s, device.DeviceState(nloc, bw) as d:
      for st in (s, d):
        st.set_shard(nglob, shard)
      s.upload(full[shard << nloc:(shard + 1) << nloc])
      s.remap_swap(2, 7)                                    # local bits anywhere (this relabels the state: read it back)
      with s.clone() as c:
        lo_s, phys_s = _logical_state(c, shard, nglob)
      held_src = np.zeros(1 << nglob, dtype=np.complex128)    # the global state with this shard's amplitudes only
      held_src[lo_s] = phys_s
      want_full = pauli_util.np_pauli_sum(held_src, coeffs, xs, zs)      # (x masks are local: partners stay on the shard)
      d.upload(np.full(1 << nloc, 0.25))
      s.apply_pauli_sum(coeffs, xs, zs, out=d)
      assert shard_util.bitmap(d, nglob) == shard_util.bitmap(s, nglob)
      # an x bit on a bit the shard index holds: refused, dst as it is
      with d.clone() as c:
        held = c.download().tobytes()
      st0 = d.stats()
      with pytest.raises(native.QhError) as e:
        s.apply_pauli_sum([1.0], [1 << 10], [0], out=d)
      assert e.value.code == native.QH_ERR_NONLOCAL
      with pytest.raises(native.QhError) as e:
        s.apply_pauli_sum([1.0], [1 << 11], [1 << 11])
      assert e.value.code == native.QH_ERR_NONLOCAL
      assert d.stats() == st0
      with d.clone() as c:
        assert c.download().tobytes() == held
      lo, phys = _logical_state(d, shard, nglob)
      assert np.all(lo >> nloc == shard)
      err = float(max(np.max(np.abs(phys.real - want_full[lo].real)), np.max(np.abs(phys.imag - want_full[lo].imag))))
      print(f'shard {shard}, bw = {bw}: error {err:.3e} (bound {b:.3e})')
      assert err <= b


@pytest.mark.parametrize('bw', [128, 64])
def test_shard_handles_on_the_main_shape(bw):
  """13 local bits of 15: k_pauli_batch at both widths, with the sign the shard index gives folded into the coefficients.
  20 terms over three x masks: the first batch holds several x masks, the second accumulates; the z masks span the thread,
  register-index and chunk parts of the index and both held bits.  Then single terms with c = 1 whose shard sign gives
  c' = -1 on one shard and +1 on the other (the unit path entered through the shard sign), and a Y string whose nY makes c' a
  power of i: == NumPy."""
  nloc, nglob = 13, 15
  ab = _amp_bits(bw)
  dt = np.complex128 if bw == 128 else np.complex64
  full = _random_state(nglob, 72).astype(dt).astype(np.complex128)      # as stored
  rng = np.random.default_rng(73 + bw)
  thread, reg, chunk = 1 << (ab + 5), 1 << (ab + 9), 1 << (ab + CHUNK_BITS)      # (logical = physical but for bits 2 and 7)
  assert chunk < 1 << nloc
  xpool = [0, (1 << 12) | (1 << 7) | 1, (1 << 10) | (1 << 4) | 2]
  xs = [xpool[int(k) % 3] for k in rng.permutation(20)]      # given unsorted
  zs = [int(v) for v in rng.integers(0, 1 << nglob, size=20)]
  zs[0], zs[1], zs[2], zs[3] = thread | reg | chunk | (3 << nloc), chunk | (1 << nloc), reg | (2 << nloc) | 1, thread | 1
  coeffs = [complex(a, b) for a, b in rng.normal(size=(20, 2))]
  ystring = (0b111 << 3, (0b111 << 3) | (2 << nloc))        # nY = 3: (-i)^3 = i
  singles = [('c = 1, z on held bit 0', [1.0], [(1 << 11) | 5], [(1 << nloc) | chunk | 1]),
             ('c = 1, z on both held bits', [1.0], [1 << 9], [(3 << nloc) | thread]),
             ('a Y string with nY = 3', [1.0], [ystring[0]], [ystring[1]]),
             ('a Y string with nY = 3, c = -i', [-1j], [ystring[0]], [ystring[1]])]
  for shard in (1, 2):
    with device.DeviceState(nloc, bw) as s, device.DeviceState(nloc, bw) as d:
      for st in (s, d):
        st.set_shard(nglob, shard)
      s.upload(full[shard << nloc:(shard + 1) << nloc])
      s.remap_swap(2, 7)                                    # local bits anywhere (this relabels the state: read it back)
      with s.clone() as c:
        lo_s, phys_s = _logical_state(c, shard, nglob)
      held_src = np.zeros(1 << nglob, dtype=np.complex128)    # the global state with this shard's amplitudes only
      held_src[lo_s] = phys_s
      amax = float(np.max(np.abs(held_src)))
      terms, batches = s.pauli_sum_plan(xs, zs)
      assert len(batches) == 2 and batches[0]['ngroups'] > 1 and batches[1]['count'] == 4
      assert {t['neg'] for t in terms} == {0, 1}
      d.upload(np.full(1 << nloc, np.nan + 1j * np.nan))      # batch 0 does not read dst
      cases = [('20 terms', coeffs, xs, zs)] + singles
      for what, co, x, z in cases:
        s.apply_pauli_sum(co, x, z, out=d)
        assert shard_util.bitmap(d, nglob) == shard_util.bitmap(s, nglob)
        with d.clone() as c:
          lo, phys = _logical_state(c, shard, nglob)
        assert np.all(lo >> nloc == shard)
        want = pauli_util.np_pauli_sum(held_src, co, x, z)[lo]
        if len(co) == 1:
          tm = s.pauli_sum_plan(x, z)[0][0]
          print(f'shard {shard}, bw = {bw}, {what}: neg = {tm["neg"]}, ny = {tm["ny"]}')
          assert np.array_equal(phys, want.astype(dt).astype(np.complex128)), (what, shard)
        else:
          b = pauli_util.bound(bw, co, amax, len(batches))
          err = float(max(np.max(np.abs(phys.real - want.real)), np.max(np.abs(phys.imag - want.imag))))
          print(f'shard {shard}, bw = {bw}, {what}: error {err:.3e} (bound {b:.3e})')
          assert err <= b
      negs = [s.pauli_sum_plan(x, z)[0][0]['neg'] for _, _, x, z in singles[:2]]
      assert negs == ([1, 1] if shard == 1 else [0, 1])      # held bit 0 is 1 on shard 1 alone, held bit 1 on shard 2 alone


def test_blocks_that_walk_two_chunks_complex64():
  """n = 25 at complex64: an item is two amplitudes, so this is the walk of the complex128 case (2^13 chunks over 4096 blocks,
  every block walks two chunks) in the same 256 MiB per state.  The masks are those of that case moved up by the amplitude bit;
  x and z both hold amplitude bit 0 as well (the two halves of an item trade places, and the sign differs between them), and a
  z bit sits on the chunk number's lowest bit, which changes INSIDE a block.  NumPy checks 2^16 random amplitudes and the first
  and last two chunks."""
  n = CHUNK_BITS + BLOCK_CAP_BITS + 2
  cb = CHUNK_BITS + 1                                        # the chunk number's lowest bit, as an amplitude-index bit
  rng = np.random.default_rng(25)
  def sumsq(flat):                                           # sum of squares in double, a slice at a time
    return float(sum(np.dot(part, part) for part in (flat[k:k + (1 << 22)].astype(np.float64) for k in range(0, flat.size, 1 << 22))))
  host = (rng.random(2 << n, dtype=np.float32) - np.float32(0.5)).view(np.complex64)
  host *= np.float32(1.0 / np.sqrt(sumsq(host.view(np.float32))))
  xs = [1 << (n - 1), (1 << cb) | (5 << 1) | 1, (1 << cb) | (5 << 1) | 1, 0]
  zs = [(1 << cb) | (1 << (cb + 1)), (1 << cb) | 1, (1 << (n - 1)) | (1 << 10), (1 << cb) | (1 << 8) | 1]
  coeffs = [0.5 - 0.25j, 1.5, -0.75j, 0.3]
  with device.DeviceState(n, 64) as src:
    src.upload(host)
    terms, _ = src.pauli_sum_plan(xs, zs)
    assert any(t['px'] & 1 for t in terms) and any(t['pz'] & 1 for t in terms) and any((t['pz'] >> cb) & 1 for t in terms)
    grow, nbatches = _predict(src, xs, zs)
    new, n2 = src.apply_pauli_sum(coeffs, xs, zs, norm=True)
    with new:
      assert {k: new.stats()[k] for k in grow} == grow
      _, n2b = src.apply_pauli_sum(coeffs, xs, zs, out=new, norm=True)
      assert n2b == n2
      got = new.download()
  edge = 2 << cb                                             # two chunks of amplitudes
  at = np.concatenate([rng.integers(0, 1 << n, size=1 << 16), np.arange(0, edge), np.arange((1 << n) - edge, 1 << n)])
  want = pauli_util.np_pauli_sum(host, coeffs, xs, zs, at=at)
  amax = float(np.max(np.abs(host)))
  b = pauli_util.bound(64, coeffs, amax, nbatches)
  g = got[at].astype(np.complex128)
  err = float(max(np.max(np.abs(g.real - want.real)), np.max(np.abs(g.imag - want.imag))))
  n2_np = sumsq(got.view(np.float32))
  print(f'25 qubits complex64: error {err:.3e} (bound {b:.3e}); norm2 {n2:.17g}, NumPy on the stored values {n2_np:.17g}')
  assert err <= b
  assert abs(n2 - n2_np) <= 1e-12 * n2_np


# ---- 5. composition through qc ----------------------------------------------------------------------------------------------------
@pytest.fixture(params=[128, 64])
def width(request):
  tensor.set_tensor_width(request.param)
  yield request.param
  tensor.set_tensor_width(None)


def _ising(n, j=1.0, h=0.7):
  terms = [(-j, {q: 'Z', q + 1: 'Z'}) for q in range(n - 1)] + [(-h, {q: 'X'}) for q in range(n)]
  xs = [0] * (n - 1) + [1 << (n - 1 - q) for q in range(n)]
  zs = [(1 << (n - 1 - q)) | (1 << (n - 2 - q)) for q in range(n - 1)] + [0] * n
  return terms, [c for c, _ in terms], xs, zs


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


def test_qc_hamiltonian_times_variance_project_out_and_power_steps(width):
  """transverse-field Ising at 10 qubits (19 terms, 11 x masks: two batches).  w = H psi against NumPy; variance against
  NumPy; after project_out the overlap with psi is 0 within 3 x the bound; two normalised applications of H against the
  same two steps in NumPy."""
  n = 10
  terms, coeffs, xs, zs = _ising(n)
  csum = float(sum(abs(c) for c in coeffs))
  eps = 2.0 ** -52 if width == 128 else 2.0 ** -23
  q = circuit.qc('ising')
  q.reg(n, 0)
  _layers(q, n, 5)
  assert hasattr(q._ensure_device(), 'apply_pauli_sum')      # pylint: disable=protected-access
  psi = _amps(q)
  amax = float(np.max(np.abs(psi)))
  b = pauli_util.bound(width, coeffs, amax, 2)
  want = pauli_util.np_pauli_sum(psi, coeffs, xs, zs)
  with q.hamiltonian_times(terms) as w:
    assert np.array_equal(_amps(q), psi)
    with w._dev.clone() as c:                                # pylint: disable=protected-access
      got = _logical(c)
    err = float(max(np.max(np.abs(got.real - want.real)), np.max(np.abs(got.imag - want.imag))))
    print(f'H psi, width {width}: error {err:.3e} (bound {b:.3e})')
    assert err <= b
    # variance = |H psi|^2 - <H>^2: the norm within 4 C amax bound 2^n of NumPy's (as qh_apply_pauli_sum's norm2); <H> is a
    # sum of 2^n products formed in double from the same stored amplitudes on both sides: 2^n * 2^-52 * C per unit norm
    e_np = float(np.vdot(psi, want).real)
    var_np = float(np.vdot(want, want).real) - e_np ** 2
    var_tol = 4 * csum * amax * b * (1 << n) + 2 * abs(e_np) * (1 << n) * 2.0 ** -52 * csum * float(np.vdot(psi, psi).real)
    var = q.variance(terms)
    print(f'variance, width {width}: {var:.15g}, NumPy {var_np:.15g} (tolerance {var_tol:.3e})')
    assert abs(var - var_np) <= var_tol
    # one Gram-Schmidt step: phi = H psi - c psi is orthogonal to psi
    phi = circuit.qc('phi')
    phi.reg(n, 0)
    phi.restore(w)
    phi.project_out(q)
    ov = abs(phi.overlap(q))
    print(f'|<psi|phi>| after project_out, width {width}: {ov:.3e} (3 x bound {3 * b:.3e})')
    assert ov <= 3 * b
    phi.close()
  # psi <- H psi / |H psi|, twice.  Step k: the bound on its input's amax, divided by the norm, plus one rounding of the
  # scale; the error of step 1 goes through H (at most C times it) into step 2.
  v1 = want
  r1 = float(np.sqrt(np.vdot(v1, v1).real))
  p1 = v1 / r1
  v2 = pauli_util.np_pauli_sum(p1, coeffs, xs, zs)
  r2 = float(np.sqrt(np.vdot(v2, v2).real))
  p2 = v2 / r2
  e1 = b / r1 + 2 * eps * float(np.max(np.abs(p1)))
  e2 = (csum * e1 + pauli_util.bound(width, coeffs, float(np.max(np.abs(p1))) + e1, 2)) / r2 + 2 * eps * float(np.max(np.abs(p2)))
  n1 = q.apply_hamiltonian(terms, normalize=True)
  assert abs(n1 - r1 * r1) <= 4 * csum * amax * b * (1 << n)
  n2 = q.apply_hamiltonian(terms, normalize=True)
  got2 = _amps(q)
  err2 = float(max(np.max(np.abs(got2.real - p2.real)), np.max(np.abs(got2.imag - p2.imag))))
  print(f'two power steps, width {width}: error {err2:.3e} (bound {e2:.3e}); norms^2 {n1:.15g}, {n2:.15g} (NumPy {r1 * r1:.15g}, {r2 * r2:.15g})')
  assert err2 <= e2
  assert abs(n2 - r2 * r2) <= 2 * r2 * np.sqrt(1 << n) * (csum * e1 + b) + 4 * csum * b * (1 << n)
  q.h(0)                                                    # the circuit goes on
  q.h(0)
  assert np.max(np.abs(_amps(q) - got2)) <= 8 * eps
  with pytest.raises(ValueError, match='nothing to normalise'):
    q.apply_hamiltonian([(1.0, {0: 'Z'}), (-1.0, {0: 'Z'})], normalize=True)
  q.close()
