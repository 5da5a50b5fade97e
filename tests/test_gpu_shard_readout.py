"""Readout, projection and initialisation on SHARD handles (qh_set_shard: nglob > nloc), on the GPU, at sizes where every
amplitude can be checked: one GPU holds all 2^g shards of an n <= 18 qubit state at once, each behind its own handle, and
every entry point that resolves a bit held by the shard index with host arithmetic around its kernel (qh_marginal,
qh_sample, qh_project_bits / qh_project_bit, qh_prob_bit_value, qh_amplitude, qh_argmax, qh_init_basis, qh_init_product,
qh_upload / qh_download) is compared with NumPy on the full 2^n state in logical order.

Layouts: 'canonical' (right after the upload, per-gate handles), 'sweep' (fused handles after a flushed stream of dense
gates on high local bits with controls and diagonal targets on held bits; from nloc = 14 on relayout sweeps leave the local
bits permuted, which the fixture asserts), 'mid3' and 'midhalf' (qh_remap_swap of held bits with local bit 3 / the bits
around nloc / 2: held bits in the middle of the logical register and local bits out of ascending order without any flush;
per-gate and fused handles).  Sizes: nloc = 5 (below a measurement chunk and below the sweeps), 10 (one chunk), 14 (outer
bits in k_marginal_bins, several chunks in k_chunk_locate), 16 (tile maxima for qh_argmax); g = 1, 2 (3 at nloc = 14).

The reference of every reader is `before`: what the handles hold, exactly, as one complex128 array in logical order -- the
uploaded (rounded) state, or, behind a stream, the download of a twin set of handles that ran the same calls, itself
compared with the oracle's run of the stream on the full state."""
import contextlib
import ctypes

import numpy as np
import pytest

from qcc_amd import device, gates, native
from tests import oracle_lib, shard_util
from tests.fake_device import np_keep, np_marginal
from tests.oracle_lib import NO_CTL

pytestmark = pytest.mark.gpu

SIZES = [(5, 1), (5, 2), (10, 1), (10, 2), (14, 1), (14, 2), (14, 3), (16, 1), (16, 2)]
LAYOUTS = ['canonical', 'sweep', 'mid3', 'midhalf']
CASES = [pytest.param(nloc, g, bw, lay, id=f'{nloc}+{g}-c{bw}-{lay}')
         for nloc, g in SIZES for bw in (128, 64) for lay in LAYOUTS]
every_case = pytest.mark.parametrize('nloc,g,bw,layout', CASES)
PERMUTED_FROM = 14        # relayout sweeps run on shards of 2^14 amplitudes and more


def _dtype(bw):
  return np.complex128 if bw == 128 else np.complex64


def _amp_tol(bw):
  return 1e-12 if bw == 128 else 5e-6


def _close(got, want, bw):
  """sums of probabilities: test_gpu_measure's rule (_check_marginal)"""
  got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
  if bw == 128:
    assert float(np.max(np.abs(got - want))) < 1e-12, (got, want)
  else:
    assert float(np.max(np.abs(got - want))) <= 1e-6 * max(float(np.max(want)), 1e-30) + 1e-9, (got, want)


def _prob(a):
  a = np.asarray(a, dtype=np.complex128)
  return a.real ** 2 + a.imag ** 2


def _phys_of(bm, logical):
  logical = np.asarray(logical, dtype=np.uint64)
  out = np.zeros_like(logical)
  for b, p in enumerate(bm):
    out |= ((logical >> np.uint64(b)) & np.uint64(1)) << np.uint64(p)
  return out


def _swaps(nloc, g, layout):
  """qh_remap_swap calls (physical positions) of the layouts that put a held bit in the middle of the register"""
  if layout == 'mid3':
    return [(nloc, 3)]
  if layout == 'midhalf':
    return [(nloc + k, nloc // 2 - k) for k in range(g)]
  return []


def _fusion_of(layout):
  return native.QH_FUSE_SWEEP if layout in ('sweep', 'midhalf') else native.QH_FUSE_OFF


def _arrays(ops, gs):
  return np.array(ops, dtype=np.int32).reshape(-1, 2), np.array(gs, dtype=np.complex128).reshape(-1, 4).view(np.float64).reshape(-1, 8)


def _shard_stream(n, g, seed, count=60):
  """What a shard can execute, in the style of test_gpu_relayout._high_bit_circuit: dense gates on HIGH local bits
  (scattered tiles), some under a control on a held bit, mixed with controlled phases anywhere (held targets included).
  Reference qubit numbers: qubit q is logical bit n - 1 - q."""
  rng = np.random.default_rng(seed)
  nloc = n - g
  pool = [gates.hadamard(), gates.vgate(), gates.yroot(), gates.ry(0.4), gates.rx(0.7)]
  ops, gs = [], []
  for _ in range(count):
    if rng.random() < 0.5:
      t = int(rng.integers(nloc // 2, nloc))
      c = NO_CTL if rng.random() < 0.6 else n - 1 - int(rng.integers(nloc, n))
      ops.append((c, n - 1 - t))
      gs.append(np.asarray(pool[int(rng.integers(len(pool)))], dtype=np.complex128).reshape(4))
    else:
      c, t = (int(v) for v in rng.choice(n, size=2, replace=False))
      ops.append((n - 1 - c, n - 1 - t))
      gs.append(np.asarray(gates.u1(float(rng.uniform(0, 3))), dtype=np.complex128).reshape(4))
  return _arrays(ops, gs)


def _exact_stream(n, local, held, seed, count=60):
  """Permutations and quarter-turn phases only (the two peaks of test_argmax stay exactly equal wherever they go): X on
  the logical bits `local`, some under a control on one of `held`, and controlled phases anywhere."""
  rng = np.random.default_rng(seed)
  xg = np.array([0, 1, 1, 0], dtype=np.complex128)
  ops, gs = [], []
  for _ in range(count):
    if rng.random() < 0.5:
      t = int(local[int(rng.integers(len(local)))])
      c = NO_CTL if rng.random() < 0.6 else n - 1 - int(held[int(rng.integers(len(held)))])
      ops.append((c, n - 1 - t))
      gs.append(xg)
    else:
      c, t = (int(v) for v in rng.choice(n, size=2, replace=False))
      ops.append((n - 1 - c, n - 1 - t))
      gs.append(np.array([1, 0, 0, (1, 1j, -1, -1j)[int(rng.integers(0, 4))]], dtype=np.complex128))
  return _arrays(ops, gs)


class Shards:
  """2^g handles of nloc bits on one GPU, shard s of an n-qubit state behind handle s."""

  def __init__(self, n, g, bw, sts):
    self.n, self.g, self.nloc, self.bw, self.sts = n, g, n - g, bw, sts
    self.before = self.ref = None

  def bm(self, s):
    return shard_util.bitmap(self.sts[s], self.n)

  def held(self, s=0):
    """logical bits the shard index holds, by physical position"""
    bm = self.bm(s)
    return sorted((b for b in range(self.n) if bm[b] >= self.nloc), key=lambda b: bm[b])

  def local(self, s=0):
    """logical bits that are index bits of the shard's amplitudes, by physical position"""
    bm = self.bm(s)
    return sorted((b for b in range(self.n) if bm[b] < self.nloc), key=lambda b: bm[b])

  def held_value(self, s, b):
    return (s >> (self.bm(s)[b] - self.nloc)) & 1

  def logical(self, s):
    """global logical index of every local amplitude of shard s, in its physical order, as the layout is NOW"""
    return shard_util.phys_to_logical(self.sts[s], s, np.arange(1 << self.nloc, dtype=np.uint64), self.n).astype(np.int64)

  def gather(self):
    """every shard's download mapped back through its own bit map (a download may re-order the local bits first)"""
    out = np.zeros(1 << self.n, dtype=np.complex128)
    seen = np.zeros(1 << self.n, dtype=np.int64)
    for s, st in enumerate(self.sts):
      a = st.download()
      idx = self.logical(s)
      out[idx] = a
      seen[idx] += 1
    assert np.all(seen == 1)          # the shards' maps partition the logical index range
    return out

  def close(self):
    for st in self.sts:
      st.close()


def _make(n, g, bw, layout, psi, fusion, stream, tail):
  """the handles, laid out and loaded: psi (logical order) is cut by the map the swaps will leave and uploaded BEFORE them
  (the swap relabels and moves no data), then the stream runs and is flushed, then the tail is queued"""
  nloc = n - g
  F = Shards(n, g, bw, [])
  try:
    swaps = _swaps(nloc, g, layout)
    bm = list(range(n))
    for a, b in swaps:
      la, lb = bm.index(a), bm.index(b)
      bm[la], bm[lb] = bm[lb], bm[la]
    local = np.arange(1 << nloc, dtype=np.uint64)
    for s in range(1 << g):
      st = device.DeviceState(nloc, bw, fusion=fusion)
      F.sts.append(st)
      st.set_shard(n, s)
      st.upload(psi[shard_util.logical_of(bm, (np.uint64(s) << np.uint64(nloc)) | local).astype(np.int64)].astype(_dtype(bw)))
      for a, b in swaps:
        st.remap_swap(a, b)
      assert F.bm(s) == bm
      if stream is not None:
        st.run_stream(*stream)
        st.flush()
      if tail is not None:
        st.run_stream(*tail)
    return F
  except BaseException:
    F.close()
    raise


@contextlib.contextmanager
def shards(nloc, g, bw, layout, seed, psi=None, fusion=None, stream=None, tail=None, permuted=None):
  n = nloc + g
  if psi is None:
    rng = np.random.default_rng(seed)
    psi = rng.standard_normal(1 << n) + 1j * rng.standard_normal(1 << n)
    psi /= np.linalg.norm(psi)
  psi = psi.astype(_dtype(bw)).astype(np.complex128)       # what the handles hold, exactly
  fusion = _fusion_of(layout) if fusion is None else fusion
  if layout == 'sweep' and stream is None:
    stream = _shard_stream(n, g, 41)
    permuted = nloc >= PERMUTED_FROM
  F = _make(n, g, bw, layout, psi, fusion, stream, tail)
  try:
    F.ref = psi.copy()
    for part in (stream, tail):
      if part is not None:
        oracle_lib.load().run_stream(F.ref, n, part[0], part[1])
    if stream is None and tail is None:
      F.before = psi
    else:
      twin = _make(n, g, bw, layout, psi, fusion, stream, tail)
      try:
        F.before = twin.gather()
      finally:
        twin.close()
      assert float(np.max(np.abs(F.before - F.ref))) < _amp_tol(bw)
    if permuted:
      ident = list(range(n))
      assert any(F.bm(s) != ident for s in range(1 << g)), 'no relayout sweep ran: this case would not test a permuted layout'
    yield F
  finally:
    F.close()


# ---- norms, single-bit probabilities, the bit map's accessors, scale ------------------------------------------------------
@every_case
def test_norm_prob_bit_maps_and_scale(nloc, g, bw, layout):
  n = nloc + g
  rng = np.random.default_rng(5)
  with shards(nloc, g, bw, layout, seed=100 + nloc + g) as F:
    norms = []
    for s, st in enumerate(F.sts):
      L = F.logical(s)
      p = _prob(F.before[L])
      nl, ng = ctypes.c_int(-1), ctypes.c_int(-1)
      native.check(st.lib.qh_nbits(st.h, ctypes.byref(nl), ctypes.byref(ng)))
      assert (nl.value, ng.value) == (nloc, n)
      norms.append(st.norm2())
      _close(norms[-1], p.sum(), bw)
      held, local = F.held(s), F.local(s)
      for b in [local[0], local[nloc // 2], local[-1]] + held:
        for v in (0, 1):
          got = st.prob_bit(b, v)
          if b in held and F.held_value(s, b) != v:
            assert got == 0.0                                  # the shard index says otherwise: exactly nothing
          else:
            _close(got, p[((L >> b) & 1) == v].sum(), bw)
        p1 = ctypes.c_double(-1.0)
        native.check(st.lib.qh_prob_bit(st.h, b, ctypes.byref(p1)))
        _close(p1.value, p[((L >> b) & 1) == 1].sum(), bw)
      bm = F.bm(s)
      for i in [0, (1 << n) - 1] + [int(v) for v in rng.integers(0, 1 << n, size=6)]:
        ph = int(_phys_of(bm, [i])[0])
        assert st.logical_to_phys(i) == ph and st.phys_to_logical(ph) == i
    _close(sum(norms), 1.0, bw)
    z = 0.5 - 0.25j
    for s, st in enumerate(F.sts):
      st.scale(z)
      _close(st.norm2(), norms[s] * abs(z) ** 2, bw)
    assert float(np.max(np.abs(F.gather() - F.before * z))) < _amp_tol(bw)


# ---- projection ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('which', ['local', 'held', 'span', 'bit_local', 'bit_held'])
@every_case
def test_projection_zeroes_exactly_and_keeps_bitwise(nloc, g, bw, layout, which):
  n = nloc + g
  with shards(nloc, g, bw, layout, seed=200 + nloc + g) as F:
    held, local = F.held(), F.local()
    lo, mid, hi = local[0], local[nloc // 2], local[-1]
    if which == 'local':
      mask, value = (1 << lo) | (1 << hi), 1 << lo
    elif which == 'held':        # every held bit: ONE shard agrees with the value, the others contradict it and end all-zero
      mask, value = sum(1 << b for b in held), 1 << held[0]
    elif which == 'span':
      mask, value = (1 << held[0]) | (1 << lo) | (1 << mid), 1 << mid
    elif which == 'bit_local':
      mask, value = 1 << hi, 1 << hi
    else:
      mask, value = 1 << held[-1], 0
    contradicts = [any(((mask >> b) & 1) and F.held_value(s, b) != ((value >> b) & 1) for b in F.held(s)) for s in range(1 << g)]
    assert any(contradicts) == (which in ('held', 'span', 'bit_held')) and not all(contradicts)
    for st in F.sts:
      if which.startswith('bit_'):
        st.project_bit(mask.bit_length() - 1, 1 if value else 0)
      else:
        st.project_bits(mask, value)
    for s, st in enumerate(F.sts):
      if contradicts[s]:
        assert st.norm2() == 0.0
    keep = np_keep(1 << n, mask, value)
    after = F.gather()
    assert np.array_equal(after, np.where(keep, F.before, 0))      # zeros are zeros, kept amplitudes are bitwise the same
    for s, st in enumerate(F.sts):
      if contradicts[s]:
        assert not st.download().any()


# ---- marginals -----------------------------------------------------------------------------------------------------------------
def _marginal_at(p, idx, bits):
  """np_marginal for amplitudes at the (scattered) logical indices idx"""
  j = np.zeros_like(idx)
  for t, b in enumerate(bits):
    j |= ((idx >> b) & 1) << t
  return np.bincount(j, weights=p, minlength=1 << len(bits))


@every_case
def test_marginal_resolves_held_bits_in_output_space(nloc, g, bw, layout):
  rng = np.random.default_rng(7)
  with shards(nloc, g, bw, layout, seed=300 + nloc + g) as F:
    bm, held, local = F.bm(0), F.held(), F.local()
    inner = [b for b in local if bm[b] < 12]          # below kMeasChunkBits: folded in LDS
    outer = [b for b in local if bm[b] >= 12]         # chunk index bits
    sets = [[], list(held), list(held)[::-1],
            [inner[0], held[0], inner[-1]],            # a held bit at output position 1 ...
            [held[-1]] + inner[1:4],                   # ... at 0 ...
            inner[:2] + held]                          # ... and on top
    if outer:
      sets += [[outer[0], held[0], inner[2], outer[-1]], [held[-1]] + outer[::-1] + [inner[3]]]
    if nloc == 16:
      sets.append(held + [int(b) for b in rng.permutation(local)[:16 - g]])            # k = 16, held bits at the bottom
      sets.append([int(b) for b in rng.permutation(held + local[:16 - g])])             # ... and anywhere
    total = [np.zeros(1 << len(bits)) for bits in sets]
    for s, st in enumerate(F.sts):
      L = F.logical(s)
      p = _prob(F.before[L])
      for k, bits in enumerate(sets):
        got = st.marginal(bits)
        assert got.shape == (1 << len(bits),)
        assert st.marginal(bits).tobytes() == got.tobytes()             # bitwise reproducible
        _close(got, _marginal_at(p, L, bits), bw)
        total[k] += got
    for bits, t in zip(sets, total):
      _close(t, np_marginal(F.before, bits), bw)


# ---- sampling ------------------------------------------------------------------------------------------------------------------
@every_case
def test_sample_is_the_shards_inverse_cdf_with_its_held_bits(nloc, g, bw, layout):
  rng = np.random.default_rng(11)
  u = np.sort(np.concatenate([rng.random(4093), [0.0, 0.5, np.nextafter(1.0, 0.0)]]))
  with shards(nloc, g, bw, layout, seed=400 + nloc + g) as F:
    for s, st in enumerate(F.sts):
      bm = F.bm(s)
      pp = _prob(F.before[F.logical(s)])                # the shard's amplitudes in ITS physical order; u is scaled by ITS norm
      got = st.sample(u)
      assert got.dtype == np.uint64 and got.shape == u.shape
      phys = _phys_of(bm, got)
      assert np.all((phys >> np.uint64(nloc)) == np.uint64(s))            # global logical indices that carry the shard's held bits
      shard_util.check_exact_cdf(pp, (phys & np.uint64((1 << nloc) - 1)).astype(np.int64), u)
    b = F.held()[0]
    F.sts[0].project_bits(1 << b, (1 - F.held_value(0, b)) << b)          # shard 0 contradicts: emptied
    with pytest.raises(native.QhError) as e:
      F.sts[0].sample(u)
    assert e.value.code == native.QH_ERR_ARG and "the shard's norm is 0" in str(e.value)
    assert F.sts[1].sample(u[:16]).size == 16


# ---- single amplitudes ---------------------------------------------------------------------------------------------------------
@every_case
def test_amplitude_only_on_the_owning_shard(nloc, g, bw, layout):
  n = nloc + g
  rng = np.random.default_rng(13)
  with shards(nloc, g, bw, layout, seed=500 + nloc + g) as F:
    for i in [0, (1 << n) - 1, 1 << nloc, (1 << nloc) - 1] + [int(v) for v in rng.integers(0, 1 << n, size=6)]:
      owners = 0
      for s, st in enumerate(F.sts):
        if int(_phys_of(F.bm(s), [i])[0]) >> nloc == s:
          owners += 1
          assert complex(st.amplitude(i)) == complex(F.before[i])
        else:
          with pytest.raises(native.QhError) as e:
            st.amplitude(i)
          assert e.value.code == native.QH_ERR_NONLOCAL
      assert owners == 1


# ---- argmax --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('fused', ['1', '0'])
@every_case
def test_argmax_reports_global_indices_and_breaks_ties_logically(nloc, g, bw, layout, fused, monkeypatch):
  """Two exactly equal peaks per shard over a small background; every gate is a permutation or a quarter-turn phase, so
  the peaks stay exactly equal wherever they go.  Fused handles still have gates queued when qh_argmax is called: with
  QH_FUSED_ARGMAX=1 the flush in front of the reader leaves tile maxima (nloc = 16), with 0 the full pass decides."""
  monkeypatch.setenv('QH_FUSED_ARGMAX', fused)
  n = nloc + g
  rng = np.random.default_rng(600 + nloc + g)
  psi = rng.standard_normal(1 << n) + 1j * rng.standard_normal(1 << n)
  psi *= 0.1 / np.linalg.norm(psi)
  local_mask = (1 << nloc) - 1
  for s in range(1 << g):                       # (under 'canonical' and 'sweep' the held bits are the top logical bits; the
    a, b = (int(v) for v in rng.choice(1 << nloc, 2, replace=False))   #  swaps of the other layouts relabel: peaks per SHARD below)
    psi[(s << nloc) | a] = 0.5
    psi[(s << nloc) | b] = -0.5j
  bm = list(range(n))
  for x, y in _swaps(nloc, g, layout):
    lx, ly = bm.index(x), bm.index(y)
    bm[lx], bm[ly] = bm[ly], bm[lx]
  psi = psi[_phys_of(bm, np.arange(1 << n, dtype=np.uint64)).astype(np.int64)]      # two peaks on every shard under bm
  fusion = _fusion_of(layout)
  held = [b for b in range(n) if bm[b] >= nloc]
  local = [b for b in range(n) if bm[b] < nloc]
  stream = _exact_stream(n, local, held, 17) if layout == 'sweep' else None
  tail = _exact_stream(n, local, held, 19, 24) if fusion == native.QH_FUSE_SWEEP else None
  with shards(nloc, g, bw, layout, seed=0, psi=psi, stream=stream, tail=tail, permuted=layout == 'sweep' and nloc == 16) as F:
    for s, st in enumerate(F.sts):
      if tail is not None:
        pending = ctypes.c_uint64(0)
        native.check(st.lib.qh_pending_gates(st.h, ctypes.byref(pending)))
        assert pending.value > 0
      idx, p = st.argmax()
      L = F.logical(s)
      pr = _prob(F.before[L])
      peaks = L[pr == pr.max()]
      assert len(peaks) == 2 and pr.max() == 0.25
      assert (idx, p) == (int(peaks.min()), 0.25), (s, idx, peaks)


# ---- initialisation ------------------------------------------------------------------------------------------------------------
@every_case
def test_init_basis_lands_on_one_shard(nloc, g, bw, layout):
  n = nloc + g
  rng = np.random.default_rng(19)
  with shards(nloc, g, bw, layout, seed=700 + nloc + g) as F:
    xs = [int(v) for v in rng.integers(0, 1 << n, size=3)] + [0, (1 << n) - 1]
    for x in xs:
      for st in F.sts:
        st.init_basis(x)
      norms = [st.norm2() for st in F.sts]
      assert sorted(norms) == [0.0] * ((1 << g) - 1) + [1.0]
      owner = norms.index(1.0)
      assert int(_phys_of(F.bm(owner), [x])[0]) >> nloc == owner
      assert complex(F.sts[owner].amplitude(x)) == 1.0
    got = F.gather()
    want = np.zeros(1 << n, dtype=np.complex128)
    want[xs[-1]] = 1
    assert np.array_equal(got, want)
    for s, st in enumerate(F.sts):
      if s != norms.index(1.0):
        assert not st.download().any()


def _table(rng, k):
  t = rng.standard_normal(1 << k) + 1j * rng.standard_normal(1 << k)
  return t / np.linalg.norm(t)


@pytest.mark.parametrize('which', ['at_nloc', 'across_nloc', 'all_basis'])
@every_case
def test_init_product_builds_every_shards_slice(nloc, g, bw, layout, which):
  n = nloc + g
  rng = np.random.default_rng(800 + nloc + g)
  if which == 'at_nloc':            # a factor boundary between the held and the local bits of the canonical layout
    f = [(g, _table(rng, g)), (nloc - 3, int(rng.integers(0, 1 << (nloc - 3)))), (3, _table(rng, 3))]
  elif which == 'across_nloc':      # a table that spans held and local bits
    f = [(g + 2, _table(rng, g + 2)), (nloc - 4, int(rng.integers(0, 1 << (nloc - 4)))), (2, _table(rng, 2))]
  else:                             # one basis state: the qh_init_basis shortcut
    f = [(g, int(rng.integers(0, 1 << g))), (nloc - 2, int(rng.integers(0, 1 << (nloc - 2)))), (2, 3)]
  want = np.ones(1, dtype=np.complex128)
  for k, x in f:
    want = np.kron(want, np.eye(1 << k)[x] if isinstance(x, int) else x)
  with shards(nloc, g, bw, layout, seed=800 + nloc + g) as F:
    for st in F.sts:
      st.init_product(f)
    _close(sum(st.norm2() for st in F.sts), 1.0, bw)
    for i in (int(np.argmax(np.abs(want))), 0):          # through the map as it is, before any download re-orders it
      owner = [s for s in range(1 << g) if int(_phys_of(F.bm(s), [i])[0]) >> nloc == s]
      assert len(owner) == 1 and abs(complex(F.sts[owner[0]].amplitude(i)) - want[i]) < _amp_tol(bw)
    got = F.gather()
    if which == 'all_basis':
      assert np.array_equal(got, want)
    else:
      assert float(np.max(np.abs(got - want))) < _amp_tol(bw)


# ---- whole-shard upload and download under a map whose local bits are out of order ------------------------------------------
@pytest.mark.parametrize('mode', ['per_gate', 'fused_unflushed', 'fused_no_relayout'])
@pytest.mark.parametrize('layout', ['mid3', 'midhalf'])
@pytest.mark.parametrize('nloc,g,bw', [(5, 1, 128), (10, 2, 64), (14, 3, 128), (16, 2, 64)])
def test_upload_download_round_trip_without_a_second_buffer(nloc, g, bw, layout, mode, monkeypatch):
  """qh_remap_swap alone leaves the local bits out of ascending order; the handle has no second buffer yet (or never gets
  one): qh_upload / qh_download must still bring the layout back to canonical order and move the data."""
  if mode == 'fused_no_relayout':
    monkeypatch.setenv('QH_RELAYOUT', '0')
  fusion = native.QH_FUSE_OFF if mode == 'per_gate' else native.QH_FUSE_SWEEP
  rng = np.random.default_rng(900 + nloc)
  with shards(nloc, g, bw, layout, seed=900 + nloc + g, fusion=fusion) as F:
    last = len(F.sts) - 1
    first = F.sts[last].download(3, 9)        # a window: canonical order comes first, the amplitudes move with it
    assert F.local(last) == sorted(F.local(last))
    assert np.array_equal(first.astype(np.complex128), F.before[F.logical(last)[3:12]])
    data = (rng.standard_normal(1 << nloc) + 1j * rng.standard_normal(1 << nloc)).astype(_dtype(bw))
    F.sts[0].upload(data)                     # the whole shard, on a handle still in the swapped layout
    assert F.local(0) == sorted(F.local(0))
    assert np.array_equal(F.sts[0].download(), data)
    got = F.gather()                          # the other shards are as they were
    want = F.before.copy()
    want[F.logical(0)] = data
    assert np.array_equal(got, want)
