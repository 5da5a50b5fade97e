"""Matrix elements between two states on the MI355X: qh_transition_pauli against NumPy on the amplitudes as stored, brought
into logical order on the host (transition_util.np_transition), on every walk (gather, linear, tiles) with x and z bits on
every class of physical position, batches and their stats, the properties that tie it to qh_inner / qh_expect_pauli /
qh_apply_pauli_sum, shards on one GPU, refusals, one 30-qubit pair of product states with a closed form, and
qc.matrix_element / qc.rotation_gradients end to end.

qh_download re-lays a permuted state out, so the handles under test are downloaded LAST: a Pair collects the device's answers
first and compares them when the test is done with the handles."""
import ctypes
import itertools

import numpy as np
import pytest

from qcc_amd import device, gates, native, workloads
from qcc_amd.lib import circuit, tensor
from tests import shard_util, transition_util as tu

pytestmark = pytest.mark.gpu

TOL = 1e-12      # readers that sum in double from the stored amplitudes, normalised states, both widths
_dp = ctypes.POINTER(ctypes.c_double)
_up = ctypes.POINTER(ctypes.c_uint64)


def _logical(st, shard=0, nglob=None):
  """the amplitudes the handle holds as complex128, in (local) logical order, whatever layout the download leaves"""
  phys = st.download().astype(np.complex128)
  nglob = nglob or st.nbits
  lo = shard_util.phys_to_logical(st, shard, np.arange(phys.size), nglob).astype(np.int64)
  if nglob != st.nbits:
    return lo, phys
  out = np.empty_like(phys)
  out[lo] = phys
  return out


def _random_state(n, seed):
  rng = np.random.default_rng(seed)
  v = rng.standard_normal(1 << n) + 1j * rng.standard_normal(1 << n)
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


def _fused_permuted(n, bw, first_seed=0, other_than=None):
  """(state, seed): a fused run whose relayout sweeps left a permuted bit map (which circuits do depends on the planner: the
  first of six seeds that does), different from the map other_than where that is given"""
  for seed in range(first_seed, first_seed + 6):
    st = _fused(n, bw, seed)
    bm = shard_util.bitmap(st)
    if bm != list(range(n)) and bm != other_than:
      return st, seed
    st.close()
  raise AssertionError(f'no supremacy-{n} circuit of seeds {first_seed}..{first_seed + 5} left a permuted bit map')


def _logical_mask(st, phys_mask):
  """the LOGICAL mask whose bits sit at the physical positions phys_mask of st"""
  return int(st.phys_to_logical(int(phys_mask)))


def _raw(a, b, xs, zs, out=None):
  x, z = np.ascontiguousarray(xs, dtype=np.uint64), np.ascontiguousarray(zs, dtype=np.uint64)
  buf = np.zeros(2 * x.size, dtype=np.float64) if out is None else out
  rc = a.lib.qh_transition_pauli(a.h, b.h, int(x.size), x.ctypes.data_as(_up), z.ctypes.data_as(_up), buf.ctypes.data_as(_dp))
  return rc, buf


class Pair:
  """two handles, the device's answers collected now and compared with NumPy when the handles may be downloaded"""

  def __init__(self, a, b, what):
    self.a, self.b, self.what, self.calls = a, b, what, []

  def run(self, xs, zs, note=''):
    got = self.a.transition_pauli(self.b, xs, zs)
    assert got.dtype == np.complex128 and got.shape == (len(xs),)
    self.calls.append((list(xs), list(zs), got, note))
    return got

  def verify(self):
    la = _logical(self.a)
    lb = la if self.b is self.a else _logical(self.b)
    worst = 0.0
    for xs, zs, got, note in self.calls:
      for x, z, g in zip(xs, zs, got):
        err = abs(g - tu.np_transition(la, lb, x, z))
        worst = max(worst, err)
        assert err < TOL, (self.what, note, hex(x), hex(z), g, err)
    print(f'{self.what}: {sum(len(c[0]) for c in self.calls)} strings, max |gpu - numpy| = {worst:.3e}')
    return la, lb


def _position_strings(a, b, n, rng):
  """x alone, z alone and Y on every physical position (x by b's positions, z by a's), one weight-n string and one mixed"""
  xs, zs = [], []
  for p in range(n):
    xl, zl = _logical_mask(b, 1 << p), _logical_mask(a, 1 << p)
    xs += [xl, 0, xl]
    zs += [0, zl, xl]
  full = (1 << n) - 1
  wx = int(rng.integers(0, 1 << n))
  xs += [wx, int(rng.integers(0, 1 << n))]
  zs += [(full & ~wx) | int(rng.integers(0, 1 << n)), int(rng.integers(0, 1 << n))]      # X, Y or Z on every qubit; a mixed one
  return xs, zs


# ---- 1. the gather walk, and the smallest linear ones -----------------------------------------------------------------------
@pytest.mark.parametrize('bw', [128, 64])
@pytest.mark.parametrize('n', [1, 3, 7])
def test_gather_walk(n, bw):
  rng = np.random.default_rng(70 + n)
  if n <= 3:
    xs, zs = zip(*itertools.product(range(1 << n), repeat=2))      # every string: 4 at n = 1, 64 at n = 3
  else:
    xs, zs = rng.integers(0, 1 << n, size=40), rng.integers(0, 1 << n, size=40)
  xs, zs = [int(v) for v in xs], [int(v) for v in zs]
  with _uploaded(n, bw, 10 + n) as a, _uploaded(n, bw, 20 + n) as b:
    lin = Pair(a, b, f'linear n={n} bw={bw}')      # (one bit has one layout: the linear walk on a single item)
    assert a.transition_plan(b, xs[:1], zs[:1])[1][0]['walk'] == native.QH_INNER_LINEAR
    lin.run(xs, zs)
    if n == 1:
      lin.verify()
      return
    with b.clone() as c:
      c.remap_swap(0, n - 1)
      if n == 7:
        c.remap_swap(2, 4)
      gat = Pair(a, c, f'gather n={n} bw={bw}')
      assert a.transition_plan(c, xs[:1], zs[:1])[1][0]['walk'] == native.QH_INNER_GATHER
      gat.run(xs, zs)
      rev = Pair(c, a, f'gather (permuted a) n={n} bw={bw}')
      rev.run(xs, zs)
      rev.verify()
      gat.verify()
    lin.verify()


# ---- 2. the linear walk ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('bw', [128, 64])
@pytest.mark.parametrize('n', [8, 12, 16])
def test_linear_walk_every_position(n, bw):
  """x alone, z alone and Y on EVERY physical bit: bit 0 (inside a complex64 item), the lane bits, the thread bits 6 and 7,
  the register-index bits, the chunk bits (11 and up at complex128, 12 and up at complex64) and the top bit"""
  rng = np.random.default_rng(80 + n)
  with _uploaded(n, bw, 30 + n, [(0, n - 1), (3, 6)]) as a, _uploaded(n, bw, 40 + n, [(0, n - 1), (3, 6)]) as b:
    xs, zs = _position_strings(a, b, n, rng)
    assert all(p['walk'] == native.QH_INNER_LINEAR for p in a.transition_plan(b, xs, zs)[1])
    pair = Pair(a, b, f'linear n={n} bw={bw}')
    pair.run(xs, zs)
    pair.verify()


@pytest.mark.parametrize('bw,n', [(128, 24), (64, 25)])
def test_linear_walk_blocks_of_several_chunks(bw, n):
  """The linear walk has qh_inner's geometry: chunks of 2^11 16-byte items, at most 4096 blocks.  24 qubits at complex128 and
  25 at complex64 are 8192 chunks: the smallest sizes at which a block walks two."""
  rng = np.random.default_rng(n)
  with device.DeviceState(n, bw) as a, device.DeviceState(n, bw) as b:
    va, vb = _random_state(n, 1), _random_state(n, 2)
    a.upload(va)
    b.upload(vb)
    la, lb = a.download().astype(np.complex128), b.download().astype(np.complex128)      # as stored (canonical layouts)
    top, c0 = 1 << (n - 1), 1 << (n - 13)      # the top chunk bit; the lowest chunk bit (the one a block's two chunks differ in)
    xs = [0, c0 | 1, top | c0 | (1 << 9) | int(rng.integers(0, 1 << 8))]
    zs = [top | c0, top, c0 | 5 | int(rng.integers(0, 1 << n))]
    got = a.transition_pauli(b, xs, zs)
    for x, z, g in zip(xs, zs, got):
      err = abs(g - tu.np_transition(la, lb, x, z))
      print(f'n={n} bw={bw} x={x:#x} z={z:#x}: |gpu - numpy| = {err:.3e}')
      assert err < TOL


# ---- 3. the tiles walk ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('bw', [128, 64])
@pytest.mark.parametrize('n', [8, 10, 16])
def test_tiles_walk_every_position(n, bw):
  """b permuted (and, separately, a), a swap between a low in-tile bit and the top bit among them; x by b's physical positions
  and z by a's on every bit: in-tile bits below 4 and 4 to 7, the chunk-of-tiles bits and the higher tile-number bits"""
  rng = np.random.default_rng(90 + n)
  swaps = [(1, n - 1), (2, 5), (0, 6)]
  with _uploaded(n, bw, 50 + n) as a, _uploaded(n, bw, 60 + n, swaps) as b:
    pairs = []
    for first, second in ((a, b), (b, a)):
      xs, zs = _position_strings(first, second, n, rng)
      assert all(p['walk'] == native.QH_INNER_TILES for p in first.transition_plan(second, xs, zs)[1])
      pairs.append(Pair(first, second, f'tiles n={n} bw={bw} permuted {"b" if second is b else "a"}'))
      pairs[-1].run(xs, zs)
    with a.clone() as c:      # both permuted, differently
      c.remap_swap(3, n - 2)
      c.remap_swap(4, 7)
      xs, zs = _position_strings(c, b, n, rng)
      both = Pair(c, b, f'tiles n={n} bw={bw} both permuted')
      both.run(xs, zs)
      both.verify()
    for p in pairs:
      p.verify()


@pytest.mark.parametrize('bw', [128, 64])
def test_tiles_walk_on_layouts_left_by_fused_flushes(bw):
  n = 16
  rng = np.random.default_rng(16)
  a, seed = _fused_permuted(n, bw)
  b, _seed = _fused_permuted(n, bw, first_seed=seed + 1, other_than=shard_util.bitmap(a))
  with a, b:
    xs, zs = _position_strings(a, b, n, rng)
    assert all(p['walk'] == native.QH_INNER_TILES for p in a.transition_plan(b, xs, zs)[1])
    pair = Pair(a, b, f'fused supremacy-16 bw={bw}')
    pair.run(xs, zs)
    pair.verify()


# ---- 4. batches ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('bw', [128, 64])
@pytest.mark.parametrize('swaps', [(), ((0, 11), (3, 8))], ids=['linear', 'tiles'])
def test_batches_and_stats(swaps, bw):
  n, T = 12, native.QH_TRANSITION_BATCH
  rng = np.random.default_rng(5)
  state_bytes = (bw // 8) << n
  with _uploaded(n, bw, 1) as a, _uploaded(n, bw, 2, swaps) as b:
    pair = Pair(a, b, f'batches bw={bw} {"tiles" if swaps else "linear"}')
    lists = []
    for count in (T, T + 1, 2 * T + 3):
      lists.append(([0x2c5] * count, [int(v) for v in rng.integers(0, 1 << n, size=count)]))
    masks = [int(v) for v in rng.integers(0, 1 << n, size=7)]
    mixed_x = [masks[k % 7] for k in range(40)]
    rng.shuffle(mixed_x)
    lists.append(([int(v) for v in mixed_x], [int(v) for v in rng.integers(0, 1 << n, size=40)]))
    for xs, zs in lists:
      _terms, passes = a.transition_plan(b, xs, zs)
      batch = T if bw == 128 else T // 2
      counts = {x: xs.count(x) for x in set(xs)}
      assert len(passes) == sum(-(-c // batch) for c in counts.values())
      sa, sb = a.stats(), b.stats()
      got = pair.run(xs, zs, f'{len(xs)} strings')
      da, db = a.stats(), b.stats()
      assert da['kernels_launched'] - sa['kernels_launched'] == len(passes) and db == sb
      assert da['bytes_swept'] - sa['bytes_swept'] == 2 * state_bytes * len(passes)
      assert da['bytes_algorithmic'] - sa['bytes_algorithmic'] == 2 * state_bytes * len(passes)
      assert pair.run(xs, zs, 'again').tobytes() == got.tobytes()                # the same bits
    # two identical terms, far apart in the caller's list: identical bits, in the caller's order
    xs, zs = lists[2]
    xs, zs = xs + [xs[0]], zs + [zs[0]]
    got = pair.run(xs, zs, 'duplicate')
    assert got[0].tobytes() == got[-1].tobytes()
    pair.verify()


# ---- 5. properties ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('bw', [128, 64])
@pytest.mark.parametrize('n,swaps', [(12, ()), (12, ((1, 10), (2, 6))), (16, ()), (16, ((0, 15), (5, 9)))])
def test_properties(n, swaps, bw):
  rng = np.random.default_rng(n)
  xs = [0] + [int(v) for v in rng.integers(0, 1 << n, size=5)]
  zs = [0] + [int(v) for v in rng.integers(0, 1 << n, size=5)]
  with _uploaded(n, bw, 3) as a, _uploaded(n, bw, 4, swaps) as b, a.clone() as ca, b.clone() as cb:
    bma, bmb = shard_util.bitmap(a), shard_util.bitmap(b)
    pair = Pair(a, b, f'properties n={n} bw={bw} swaps={swaps}')
    ab = pair.run(xs, zs)
    assert pair.run(xs, zs).tobytes() == ab.tobytes()                             # two calls, the same bits
    assert abs(ab[0] - a.inner(b)) < TOL                                            # x = z = 0 is qh_inner
    ba = b.transition_pauli(a, xs, zs)
    assert np.max(np.abs(ab - np.conj(ba))) < TOL                                   # P is Hermitian
    aa = a.transition_pauli(a, xs, zs)
    assert np.max(np.abs(aa.real - a.expect_pauli(xs, zs))) < TOL and np.max(np.abs(aa.imag)) < TOL
    for x, z, v in zip(xs, zs, ab):                                                 # a device path none of the new code touches
      with b.apply_pauli_sum([1.0], [x], [z]) as w:
        assert abs(v - a.inner(w)) < TOL
    # reads only: bit maps and amplitudes of both handles as before
    assert shard_util.bitmap(a) == bma and shard_util.bitmap(b) == bmb
    la, lb = pair.verify()
    assert la.tobytes() == _logical(ca).tobytes() and lb.tobytes() == _logical(cb).tobytes()


def _hadamard_bits(v, bits):
  v = np.asarray(v, dtype=np.complex128).copy()
  for bit in bits:
    w = v.reshape(-1, 2, 1 << bit)
    lo, hi = w[:, 0, :].copy(), w[:, 1, :].copy()
    w[:, 0, :], w[:, 1, :] = (lo + hi) / np.sqrt(2), (lo - hi) / np.sqrt(2)
  return v


@pytest.mark.parametrize('bw', [128, 64])
def test_queued_gates_on_either_handle_run_first(bw):
  n = 12
  with _uploaded(n, bw, 5, fusion=native.QH_FUSE_SWEEP) as a, _uploaded(n, bw, 6, fusion=native.QH_FUSE_SWEEP) as b:
    sa, sb = a.download().astype(np.complex128), b.download().astype(np.complex128)      # as stored at this width
    for st, bits in ((a, (0, 7, 11)), (b, (3, 4))):
      for bit in bits:
        st.apply_bits(0, bit, gates.hadamard())
    pend = ctypes.c_uint64()
    for st, want in ((a, 3), (b, 2)):
      native.check(st.lib.qh_pending_gates(st.h, ctypes.byref(pend)))
      assert pend.value == want                                                     # still queued
    xs, zs = [0, 0x803, 0x803, 0x10], [0, 0x11, 0xf00, 0x10]
    got = a.transition_pauli(b, xs, zs)
    for st in (a, b):
      native.check(st.lib.qh_pending_gates(st.h, ctypes.byref(pend)))
      assert pend.value == 0
    ma, mb = _hadamard_bits(sa, (0, 7, 11)), _hadamard_bits(sb, (3, 4))
    tol = TOL if bw == 128 else 1e-6                                                # (the gates round to the state's width)
    for x, z, g in zip(xs, zs, got):
      assert abs(g - tu.np_transition(ma, mb, x, z)) < tol
    la, lb = _logical(a), _logical(b)
    for x, z, g in zip(xs, zs, got):
      assert abs(g - tu.np_transition(la, lb, x, z)) < TOL                          # and exactly what the handles hold now


@pytest.mark.parametrize('bw', [128, 64])
def test_attached_and_host_mapped_handles(bw):
  n = 10
  xs, zs = [0, 0x201, 0x3f], [0x155, 0x201, 0]
  with device.DeviceState(n, bw) as owner, _uploaded(n, bw, 8, [(0, 9)]) as b, device.DeviceState(n, bw, host_mapped=True) as hm:
    owner.upload(_random_state(n, 7))
    owner.sync()
    hm.upload(_random_state(n, 9))
    with device.DeviceState(n, bw, device_ptr=owner.device_ptr) as att:
      ptr = att.device_ptr
      p1, p2, p3 = Pair(att, b, f'attached a bw={bw}'), Pair(b, att, f'attached b bw={bw}'), Pair(hm, att, f'host-mapped a bw={bw}')
      p4 = Pair(b, hm, f'host-mapped b bw={bw}')
      for p in (p1, p2, p3, p4):
        p.run(xs, zs)
      assert att.device_ptr == ptr == owner.device_ptr
      hp = ctypes.c_void_p()
      native.check(hm.lib.qh_host_ptr(hm.h, ctypes.byref(hp)))
      assert hp.value
      for p in (p3, p4, p1, p2):
        p.verify()


# ---- 6. shards on one GPU -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('bw', [128, 64])
def test_shards_sum_to_the_global_value(bw):
  nloc, nglob = 10, 12
  va, vb = _random_state(nglob, 41), _random_state(nglob, 42)
  # logical bits 10 and 11 are the shard index; x stays on local bits, z anywhere
  xs = [0, 0x155, 0x155, 0x3ff, 0x002]
  zs = [1 << 10, 1 << 11, (3 << 10) | 0x0f3, (1 << 11) | 0x155, 0x002]
  total = np.zeros(len(xs), dtype=np.complex128)
  full_a, full_b = np.zeros(1 << nglob, dtype=np.complex128), np.zeros(1 << nglob, dtype=np.complex128)
  for s in range(4):
    with device.DeviceState(nloc, bw, fusion=native.QH_FUSE_SWEEP) as a, device.DeviceState(nloc, bw) as b:
      for st, v in ((a, va), (b, vb)):
        st.set_shard(nglob, s)
        st.upload(v[s << nloc:(s + 1) << nloc])
      b.remap_swap(2, 7)                                    # local bits anywhere, on one side
      b.remap_swap(0, 9)
      terms, passes = a.transition_plan(b, xs, zs)
      assert all(p['walk'] == native.QH_INNER_TILES for p in passes)
      assert {t['index']: t['neg'] for t in terms} == {0: s & 1, 1: s >> 1, 2: (s ^ (s >> 1)) & 1, 3: s >> 1, 4: 0}
      got = a.transition_pauli(b, xs, zs)
      total += got
      # per shard: the same sum with z's shard bits dropped, times the shard's sign
      plain = a.transition_pauli(b, xs, [z & 0x3ff for z in zs])
      signs = np.array([-1.0 if t else 1.0 for t in (s & 1, s >> 1, (s ^ (s >> 1)) & 1, s >> 1, 0)])
      assert (got == signs * plain).all()                                          # exact: a negation
      # refusals: nothing runs, out untouched, nothing flushed
      a.apply_bits(0, 1, gates.hadamard())
      a.apply_bits(0, 1, gates.hadamard())                                          # (H H: the state is what it was, to rounding)
      pend, ka = ctypes.c_uint64(), a.stats()['kernels_launched']
      buf = np.full(4, 7.0)
      rc, _ = _raw(a, b, [0x001, 1 << 10], [0, 0], out=buf)
      assert rc == native.QH_ERR_NONLOCAL and b'term 1 has X or Y on logical bit 10' in a.lib.qh_last_error()
      with b.clone() as c:
        c.set_shard(nglob, s ^ 1)
        rc2, _ = _raw(a, c, [0x001], [0], out=buf)
        assert rc2 == native.QH_ERR_NONLOCAL and b'exchange first' in a.lib.qh_last_error()
        c.set_shard(nglob, s)
        c.remap_swap(3, 11)                                 # c now holds another logical bit in the shard index
        rc3, _ = _raw(a, c, [0x001], [0], out=buf)
        assert rc3 == native.QH_ERR_NONLOCAL and b'exchange first' in a.lib.qh_last_error()
      native.check(a.lib.qh_pending_gates(a.h, ctypes.byref(pend)))
      assert list(buf) == [7.0] * 4 and pend.value == 2 and a.stats()['kernels_launched'] == ka
      native.check(a.lib.qh_discard_pending(a.h))
      for st, full in ((a, full_a), (b, full_b)):
        lo, phys = _logical(st, s, nglob)
        full[lo] = phys
  want = np.array([tu.np_transition(full_a, full_b, x, z) for x, z in zip(xs, zs)])
  print(f'4 shards of 10 of 12, bw={bw}: max |sum over shards - global| = {np.max(np.abs(total - want)):.3e}')
  assert np.max(np.abs(total - want)) < TOL


# ---- 7. refusals on live handles ---------------------------------------------------------------------------------------------
def test_refusals_and_the_empty_list():
  with _uploaded(8, 128, 1, [(0, 5)]) as a, _uploaded(9, 128, 2) as n9, _uploaded(8, 64, 3) as w64, _uploaded(8, 128, 4) as b:
    with a.clone() as ref:
      want = _logical(ref)
    buf = np.full(2, 7.0)
    for x, y in ((a, n9), (n9, a), (a, w64), (w64, a)):
      rc, _ = _raw(x, y, [1], [0], out=buf)
      assert rc == native.QH_ERR_ARG
    rc, _ = _raw(a, b, [1 << 8], [0], out=buf)
    assert rc == native.QH_ERR_BAD_QUBIT
    assert a.lib.qh_transition_pauli(a.h, b.h, 1, None, None, buf.ctypes.data_as(_dp)) == native.QH_ERR_ARG
    a.apply_bits(0, 2, gates.pauli_x())
    a.set_fusion(native.QH_FUSE_SWEEP)
    a.apply_bits(0, 2, gates.pauli_x())                                             # queued: the empty list flushes it
    kb = b.stats()
    launched = a.stats()['kernels_launched']
    assert a.lib.qh_transition_pauli(a.h, b.h, 0, None, None, None) == native.QH_OK
    pend = ctypes.c_uint64(9)
    native.check(a.lib.qh_pending_gates(a.h, ctypes.byref(pend)))
    assert pend.value == 0 and b.stats() == kb
    assert a.transition_pauli(b, [], []).shape == (0,)
    assert list(buf) == [7.0, 7.0]
    assert a.stats()['kernels_launched'] - launched == 1                              # the queued gate, and nothing else
    assert _logical(a).tobytes() == want.tobytes()


# ---- 8. full size: two 30-qubit product states ----------------------------------------------------------------------------
def test_product_states_30_qubits_closed_form():
  """<a|P|b> of two product states is the product of 30 single-qubit matrix elements: nothing from the new kernels enters
  the expected value, and the top bits exercise the 64-bit index arithmetic (2^30 amplitudes of 16 bytes)."""
  n = 30
  rng = np.random.default_rng(30)

  def factors():
    t, p = rng.uniform(0.2, 1.3, size=n), rng.uniform(0, 2 * np.pi, size=n)
    return [np.array([np.cos(t[q]), np.exp(1j * p[q]) * np.sin(t[q])]) for q in range(n)]      # factor q: logical bit n - 1 - q
  fa, fb = factors(), factors()
  mats = {(0, 0): np.eye(2), (1, 0): np.array([[0, 1], [1, 0]]), (1, 1): np.array([[0, -1j], [1j, 0]]), (0, 1): np.diag([1.0, -1.0])}

  def closed_form(x, z):
    v = 1.0 + 0j
    for q in range(n):
      bit = n - 1 - q
      v *= np.vdot(fa[q], mats[((x >> bit) & 1, (z >> bit) & 1)] @ fb[q])
    return complex(v)
  full = (1 << n) - 1
  wx = int(rng.integers(0, 1 << n)) | (1 << 29) | 1
  xs = [0, 0, 1 << 0, 1 << 7, 1 << 11, 1 << 29, wx]
  zs = [0, 1 << 0, 0, 0, 0, 0, (full & ~wx) | int(rng.integers(0, 1 << n))]
  with device.DeviceState(n, 128) as a, device.DeviceState(n, 128) as b:
    a.init_product([(1, f) for f in fa])
    b.init_product([(1, f) for f in fb])
    assert shard_util.bitmap(a) == list(range(n)) and shard_util.bitmap(b) == list(range(n))      # physical bit = logical bit
    ka = a.stats()['kernels_launched']
    got = a.transition_pauli(b, xs, zs)
    assert a.stats()['kernels_launched'] - ka == 6                                  # six x masks
    for x, z, g in zip(xs, zs, got):
      want = closed_form(x, z)
      print(f'30 qubits x={x:#011x} z={z:#011x}: gpu {g:.15f} closed form {want:.15f} |diff| = {abs(g - want):.3e}')
      assert abs(g - want) < TOL
    assert abs(a.inner(b) - got[0]) < TOL


# ---- 9. qc ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def width128():
  tensor.set_tensor_width(128)
  yield
  tensor.set_tensor_width(None)


def _layers(q, nq, seed, depth):
  rng = np.random.default_rng(seed)
  for _ in range(depth):
    for i in range(nq):
      q.ry(i, float(rng.uniform(0, 3)))
    for i in range(nq - 1):
      q.cu1(i, i + 1, float(rng.uniform(0, 3)))
    q.cx(int(rng.integers(1, nq)), 0)


def test_qc_matrix_element(width128):
  nq = 12
  a, b = circuit.qc('a'), circuit.qc('b')
  for q, seed in ((a, 1), (b, 2)):
    q.reg(nq, 0)
    _layers(q, nq, seed, 2)
  ham = [(-1.0, {q: 'Z', q + 1: 'Z'}) for q in range(nq - 1)] + [(0.7, {q: 'X'}) for q in range(nq)] + [(0.3, {0: 'Y', 5: 'y', 11: 'Z'})]
  assert type(a._ensure_device()).__name__ == 'DeviceState'
  got, per = a.matrix_element(b, ham), a.matrix_element(b, ham, per_term=True)
  with b.snapshot() as snap:
    b.h(3)
    from_snap = a.matrix_element(snap, ham)
    b.h(3)
  self_me = a.matrix_element(a, ham)
  assert abs(self_me.real - a.expectation(ham)) < TOL and abs(self_me.imag) < TOL
  assert abs(b.matrix_element(a, ham) - np.conj(got)) < TOL
  pa, pb = np.array(a.psi, dtype=np.complex128).reshape(-1), np.array(b.psi, dtype=np.complex128).reshape(-1)
  want = np.array([tu.np_transition(pa, pb, *a._pauli_masks(p)) for _c, p in ham])
  print(f'qc.matrix_element, 12 qubits: max |per term - numpy| = {np.max(np.abs(per - want)):.3e}')
  assert np.max(np.abs(per - want)) < TOL
  total = complex(np.dot([c for c, _p in ham], want))
  assert abs(got - total) < 1e-11 and abs(from_snap - total) < 1e-11                # (24 terms of size <= 1, each to TOL)
  for q in (a, b):
    q.close()


def test_qc_rotation_gradients(width128, monkeypatch):
  """10 qubits, complex128, 8 rotations (four distinct x masks, two repeated strings), a transverse-field Ising H, against
  the parameter-shift rule on fresh circuits.  Tolerance 1e-10: eight un-evolutions of double rounding, each O(1e-16), times
  |H| <= 2 n."""
  nq = 10
  rots = ['XIIIIIIIIZ', 'IYYIIIIIII', 'ZZIIIIIIII', 'XIIIIIIIIZ', 'IXYIIIZIII', 'IIIIIXIIII', 'IYYIIIIIII', 'IIIIZIIIIZ']
  assert len({tu.masks_of(s)[0] for s in rots}) == 4 and len(set(rots)) == 6
  thetas = [float(t) for t in np.random.default_rng(10).uniform(-3, 3, size=len(rots))]
  ham = [(-1.0, {q: 'Z', q + 1: 'Z'}) for q in range(nq - 1)] + [(-0.8, {q: 'X'}) for q in range(nq)]

  def prepared():
    q = circuit.qc('g')
    q.reg(nq, 0)
    _layers(q, nq, 3, 1)
    return q

  def energy_of(angles):
    q = prepared()
    for s, t in zip(rots, angles):
      q.pauli_rot(s, t)
    e = q.expectation(ham)
    q.close()
    return e

  made = []      # every device state made beside the circuit's own during the call
  for name in ('clone', '_sibling'):
    orig = getattr(device.DeviceState, name)

    def wrapped(self, *args, _orig=orig, **kw):
      new = _orig(self, *args, **kw)
      made.append(new)
      return new
    monkeypatch.setattr(device.DeviceState, name, wrapped)
  q = prepared()
  energy, grad = q.rotation_gradients(list(zip(rots, thetas)), ham)
  assert len(made) == 2 and all(st.h is None for st in made)                        # lam and phi, both closed
  want = tu.parameter_shift(energy_of, thetas)
  print(f'rotation_gradients, 10 qubits: E = {energy:.12f}, max |adjoint - parameter shift| = {np.max(np.abs(grad - want)):.3e}')
  assert abs(energy - energy_of(thetas)) < TOL * 2 * nq
  assert np.max(np.abs(grad - want)) < 1e-10
  q.close()
