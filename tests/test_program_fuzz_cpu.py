"""The program fuzzer without a GPU (tests/program_model.py): every fixed program passes run_program on the NumPy stand-in,
the runner FAILS on stand-ins that break one promise of include/qcc_hip.h each, and the fixed programs cover what they are
there for (the table is printed with -s)."""
import numpy as np
import pytest

from tests import program_model as pm
from tests.fake_device import np_marginal

WIDTHS = (128, 64)
_PROGRAMS, _CHECKS, _DRAWS, _ZDRAWS = {}, {}, {}, {}


def program(mode, seed, bw):
  key = (mode, seed, bw)
  if key not in _PROGRAMS:
    _PROGRAMS[key], draws = pm.gen_program_draws(seed, bw, mode)
    _DRAWS[key], _ZDRAWS[key] = draws['pauli_product'], draws['zpoly']
  return _PROGRAMS[key]


def run_on(cls, mode, seed, bw):
  return pm.run_program(program(mode, seed, bw), lambda nloc, w, kind: cls(nloc, w, kind), pm.Check(bw))


def checks():
  """every fixed program on NumpyDevice, once per session"""
  for bw in WIDTHS:
    for mode, seed in pm.FIXED:
      if (mode, seed, bw) not in _CHECKS:
        _CHECKS[mode, seed, bw] = run_on(pm.NumpyDevice, mode, seed, bw)
  return _CHECKS


def test_generator_is_deterministic_and_sized():
  for mode in ('own', 'shard', 'attached', 'mapped'):
    a, b = pm.gen_program(3, 64, mode), pm.gen_program(3, 64, mode)
    assert [pm.describe(s) for s in a] == [pm.describe(s) for s in b]
    assert 30 <= len(a) - 1 <= 60 and a[0]['nloc'] in pm.NLOCS
    assert sum(s['op'] == 'refused' for s in a) <= 2
    for x, y in zip(a, b):
      if x['op'] == 'gates':
        assert 5 <= len(x['gates']) <= 40 and all(np.array_equal(g, h) for (_, _, g), (_, _, h) in zip(x['gates'], y['gates']))
  assert pm.gen_program(0, 64, 'mapped')[0]['nloc'] <= 12


def test_pauli_product_draws_keep_their_conditions_and_are_rarely_rejected():
  """every emitted 'pauli_product' step has M = prod (|a_t| + |b_t|) <= 8 (pauli_product_util.bound stays near the real rounding;
  the norm range is the generator's own trial), and the budgeted draw misses M or the norm range in at most one call in ten:
  over the fixed programs and seeds 0..199 (the four modes in turn) at both widths"""
  modes = ('own', 'shard', 'attached', 'mapped')
  keys = [(mode, seed, bw) for bw in WIDTHS for mode, seed in pm.FIXED]
  keys += [key for key in ((modes[seed % 4], seed, bw) for seed in range(200) for bw in WIDTHS) if key not in keys]
  calls = rejected = steps = 0
  for key in keys:
    if key in _PROGRAMS:
      prog = program(*key)
      c, r = _DRAWS[key]
    else:
      prog, draws = pm.gen_program_draws(key[1], key[2], key[0])      # (not kept: 400 programs)
      c, r = draws['pauli_product']
    calls, rejected = calls + c, rejected + r
    for s in prog:
      if s['op'] == 'pauli_product':
        steps += 1
        assert len(s['a']) == len(s['b']) == len(s['x']) == len(s['z']) <= 3 * pm.PAULI_PRODUCT_BATCH
        assert pm.ppu.magnitude(s['a'], s['b']) <= 8.0, (key, pm.describe(s))
  print(f'k_pauli_product: {calls} draws in {len(keys)} programs, {rejected} rejected ({rejected / calls:.2%}), {steps} steps emitted')
  assert steps == calls - rejected and 10 * rejected <= calls


def test_zpoly_draws_keep_their_budget_and_are_rarely_rejected():
  """every emitted 'zpoly' step has E = exp(|c.re| F) <= 8, F = sum |w_t| (zpoly_util.apply_bound stays near the real rounding),
  its weights and c are finite and nterms * 2^nloc <= 2^25, and the drawer's trial leaves the norm range in at most one call in
  ten: over the fixed programs and seeds 0..199 (the four modes in turn) at both widths"""
  modes = ('own', 'shard', 'attached', 'mapped')
  keys = [(mode, seed, bw) for bw in WIDTHS for mode, seed in pm.FIXED]
  keys += [key for key in ((modes[seed % 4], seed, bw) for seed in range(200) for bw in WIDTHS) if key not in keys]
  calls = rejected = steps = 0
  for key in keys:
    if key in _PROGRAMS:
      prog = program(*key)
      c, r = _ZDRAWS[key]
    else:
      prog, draws = pm.gen_program_draws(key[1], key[2], key[0])      # (not kept: 400 programs)
      c, r = draws['zpoly']
    calls, rejected = calls + c, rejected + r
    for s in prog:
      if s['op'] in ('zpoly', 'expect_zpoly'):
        assert len(s['w']) == len(s['z']) <= pm.ZPOLY_MAX_TERMS and bool(np.all(np.isfinite(s['w']))), (key, pm.describe(s))
        assert len(s['z']) << s['nloc'] <= pm.ZPOLY_MODEL_BUDGET, (key, pm.describe(s))
      if s['op'] == 'zpoly':
        steps += 1
        assert np.isfinite(s['c'].real) and np.isfinite(s['c'].imag)
        assert np.exp(abs(s['c'].real) * pm.zu.big_f(s['w'])) <= 8.0, (key, pm.describe(s))
  print(f'k_zpoly: {calls} draws in {len(keys)} programs, {rejected} rejected ({rejected / calls:.2%}), {steps} steps emitted')
  assert steps == calls - rejected and 10 * rejected <= calls


def test_fixed_programs_pass_on_the_numpy_device():
  for (mode, seed, bw), c in checks().items():
    assert c.chain_err <= c.chain_tol, (mode, seed, bw)
    if bw == 64:
      assert c.chain_tol == max(pm.amp_tol(64), 4 * c.chain_d)


# ---- mutants: NumpyDevice with one method that breaks one promise ---------------------------------------------------------------
class QueueBehindBarrier(pm.NumpyDevice):
  """1. a barrier operation that does not run the queue first"""
  def _barrier(self, fn, kernels=1):
    self.store(fn(self.to_logical()))
    self.flush()
    self.kernels += kernels                                # (counted as ever: only the order is broken)


class CopyKeepsQueue(pm.NumpyDevice):
  """2. copy_from keeps the destination's queue"""
  def _copy_queue(self):
    pass


class CopyDropsBitmap(pm.NumpyDevice):
  """3. copy_from / clone copy the amplitudes but hand on a canonical bit map"""
  def _clone_bitmap(self):
    loc = [b for b in range(self.nbits_global) if self.bm[b] < self.nbits]
    bm = list(self.bm)
    for b, p in zip(loc, sorted(self.bm[b] for b in loc)):
      bm[b] = p
    return bm


class ReleaseKeepsLogicalNumbers(pm.NumpyDevice):
  """4. release renumbers the physical positions but not the logical bits"""
  def _release_bitmap(self, bits):
    gone = sorted(self.bm[b] for b in bits)
    new = {b: p - sum(1 for r in gone if r < p) for b, p in enumerate(self.bm) if b not in bits}
    size = len(new)
    left = [new[b] for b in sorted(new) if b >= size]
    return [new[b] if b in new else left.pop(0) for b in range(size)]


class ExtendOnTop(pm.NumpyDevice):
  """5. extend puts the new bits at the top of the logical register"""
  def _extend_vec(self, vec, f):
    return np.kron(f, vec)


class MuxSelectorsReversed(pm.NumpyDevice):
  """6. mux selector bits read in reversed order"""
  def _sel(self, sel_bits):
    return [int(b) for b in sel_bits][::-1]


class TopkTiesByPhysicalIndex(pm.NumpyDevice):
  """7. topk breaks ties by physical index"""
  def _topk(self, m, k):
    mine, a, p = m._probs(0)
    where = np.empty(1 << self.nbits_global, dtype=np.int64)
    where[self._lidx()] = np.arange(1 << self.nbits)
    order = np.lexsort((where[mine.astype(np.int64)], -p))
    order = order[p[order] > 0][:k]
    return mine[order], a[order]


class AxpbyReadsDstAnyway(pm.NumpyDevice):
  """8. axpby with alpha == 0 still adds 0 * old value (NaN stays NaN)"""
  def _axpby(self, d, alpha, s, beta):
    return complex(alpha) * d + complex(beta) * s


class SelectInPhysicalOrder(pm.NumpyDevice):
  """9. select returns its entries in physical order"""
  def _select(self, m, threshold):
    idx, amp, n, w = m._select({'h': 0, 'threshold': threshold})
    where = np.empty(1 << self.nbits_global, dtype=np.int64)
    where[self._lidx()] = np.arange(1 << self.nbits)
    order = np.argsort(where[idx.astype(np.int64)], kind='stable')
    return idx[order], amp[order], n, w


class ReaderCanonicalises(pm.NumpyDevice):
  """10. a reader leaves the layout canonicalised"""
  def _read(self, kernels=1):
    vec = super()._read(kernels)
    self._canonicalize()
    return vec


class MarginalIgnoresHeldBits(pm.NumpyDevice):
  """11. marginal ignores the fixed value of a bit the shard index holds"""
  def _marginal(self, vec, bits):
    held = self.held()
    local = [b for b in bits if b not in held]
    small = np_marginal(vec, local)
    j = np.arange(1 << len(bits))
    at = np.zeros_like(j)
    for t, b in enumerate(bits):
      if b in local:
        at |= ((j >> t) & 1) << local.index(b)
    return small[at]


class RoundsTwice(pm.NumpyDevice):
  """12. complex64 amplitudes rounded twice, through a perturbed intermediate: beyond the per-step bound"""
  # What this shows and what it does not: the intermediate is off by a relative 3e-5, some 250 float32 ulps, so that a barrier
  # step's result misses _amp_tol(64) = 5e-6.  A true second rounding moves an amplitude by about 6e-8 and passes: the
  # per-step bound is the one the operations' own test files use, not an ulp bound.  The chain bound max(5e-6, 4 d) is the
  # same 5e-6 for every fixed program (d is at most 3.1e-7), 10 to 1000 times the error the GPU shows.
  def _barrier(self, fn, kernels=1):
    if self.dtype == np.complex64:
      inner = fn
      fn = lambda v: (inner(v).astype(np.complex64) * np.float32(1 + 3e-5)).astype(np.complex128)      # noqa: E731
    super()._barrier(fn, kernels)


class ReaderTurnsRelayoutOn(pm.NumpyDevice):
  """13. a reader switches the relayout mode on (on attached memory, or behind set_relayout(0))"""
  def _read(self, kernels=1):
    vec = super()._read(kernels)
    self.relayout = 1
    return vec


# -- register permutations.  Which check of the runner catches which (found by deleting each check in turn: the mutant named
#    "only" then passes every fixed program, the other five are still caught)
#      14, 15  the amplitudes behind the step: bit for bit on a quiet step, _amp_tol behind a queue
#      16      the same where the table moves something; gates_noop + 1 where it does not (the first catch: an identity table)
#      17      only the bit map: it may not move in a step with nothing to flush, nor behind a flush whose relayout mode is off
#      18      only the stats of a quiet step: kernels_launched + 0, gates_noop + 1 where a held control is 0 on the shard
#      19      only the BYTES of a quiet step: the values are equal as numbers, array_equal and the chain see nothing
#      20      the amplitudes behind a step with a queue (_amp_tol), as for every other barrier
class PermTableBackwards(pm.NumpyDevice):
  """14. apply_perm applies the inverse table"""
  def _perm_apply(self, vec, table, bits, ctl_mask):
    return super()._perm_apply(vec, np.argsort(table), bits, ctl_mask)


class PermBitsAscending(pm.NumpyDevice):
  """15. apply_perm reads the register bits in ascending logical order, not in the order listed"""
  def _perm_apply(self, vec, table, bits, ctl_mask):
    return super()._perm_apply(vec, table, sorted(bits), ctl_mask)


class PermHeldControlMet(pm.NumpyDevice):
  """16. apply_perm treats a control the shard index holds as met"""
  def _perm_controls(self, ctl_mask):
    return True, ctl_mask & ~sum(1 << b for b in self.held())


class PermCanonicalises(pm.NumpyDevice):
  """17. apply_perm leaves the local bits in canonical order"""
  def _perm_layout(self):
    self._canonicalize()


class PermNoopCountsAKernel(pm.NumpyDevice):
  """18. apply_perm under a held control that is 0 on this shard counts a kernel"""
  def _perm_noop_kernels(self):
    return 1


class PermComputes(pm.NumpyDevice):
  """19. apply_perm passes the amplitudes through arithmetic (x + 0): a negative zero loses its sign"""
  def _perm_apply(self, vec, table, bits, ctl_mask):
    return super()._perm_apply(vec, table, bits, ctl_mask) + 0.0


class PermBeforeItsQueue(pm.NumpyDevice):
  """20. apply_perm runs before what is queued: mutant 1, for this call alone (it goes through _barrier like the others)"""
  def apply_perm(self, table, bits, ctl_mask=0):
    self._barrier = lambda fn, kernels=1: QueueBehindBarrier._barrier(self, fn, kernels)
    try:
      super().apply_perm(table, bits, ctl_mask)
    finally:
      del self._barrier


# -- Pauli-sum operators.  Which check of _Runner.run_pauli_sum catches which (the mutants named "only" pass every fixed program
#    once that one check is deleted; each deletion was tried once, HISTORY.md T3)
#      21, 22  the amplitudes of the destination: exact for one unit term, within pauli_util.bound otherwise (21 on a shard whose
#              held z bits have odd parity, 22 where x & z has an odd number of bits); norm2 cannot see a sign or a phase
#      23      only the bit map: "the destination's bit map is not the source's" -- the amplitudes lie in the map dst kept, so
#              every value read through that map is right
#      24      only the pending count behind the step (the queue that survives holds gates the model has dropped; the
#              amplitudes are read through a clone, which would run them -- the count is asked first)
#      25      the amplitudes behind a step with a queue on src (bound + C _amp_tol), then norm2 against the model
#      26      the amplitudes of a step with 17 terms or more; norm2 against the model where the first batch weighs enough
#      27      the amplitudes (NaN) and norm2 (NaN) of a step on a poisoned destination
#      28      only the stats: kernels_launched + 1 for no terms (on a new handle also the totals)
#      29      only the BYTES of a quiet one-term step with c' = 1: equal as numbers, array_equal and norm2 see nothing
#      30      only norm2 against the amplitudes read back, 1e-12 relative (complex64; the model's norm is 1e-7 away and passes)
class PauliIgnoresHeldZ(pm.NumpyDevice):
  """21. apply_pauli_sum ignores the z bits the shard index holds (no shard sign)"""
  def _pauli_neg(self, term):
    return 0


class PauliPlusI(pm.NumpyDevice):
  """22. apply_pauli_sum multiplies by (+i)^nY instead of (-i)^nY"""
  def _pauli_ny(self, term):
    return -term['ny'] & 3


class PauliDstKeepsBitmap(pm.NumpyDevice):
  """23. apply_pauli_sum writes the result in the layout dst had: dst keeps its own bit map"""
  def _pauli_bitmap(self, out):
    return list(out.bm)


class PauliDstKeepsQueue(pm.NumpyDevice):
  """24. apply_pauli_sum leaves what dst has queued in place"""
  def _pauli_drop_queue(self):
    pass


class PauliBeforeSrcQueue(pm.NumpyDevice):
  """25. apply_pauli_sum reads src before what src has queued has run (the queue runs behind the call)"""
  def apply_pauli_sum(self, coeffs, xmasks, zmasks, out=None, norm=False):
    self._pauli_enter = lambda: None
    try:
      res = super().apply_pauli_sum(coeffs, xmasks, zmasks, out, norm)
    finally:
      del self._pauli_enter
    self.flush()
    return res


class PauliLaterBatchOverwrites(pm.NumpyDevice):
  """26. a later batch of apply_pauli_sum overwrites dst instead of adding to it"""
  def _pauli_accumulate(self, b, old, part):
    return part


class PauliFirstBatchReadsDst(pm.NumpyDevice):
  """27. the first batch of apply_pauli_sum adds 0 * dst's old value (NaN stays NaN)"""
  def _pauli_accumulate(self, b, old, part):
    return (0.0 * old if b == 0 else old) + part


class PauliZeroTermsCountNothing(pm.NumpyDevice):
  """28. apply_pauli_sum with no terms counts no kernel"""
  def _pauli_zero_kernels(self):
    return 0


class PauliUnitComputes(pm.NumpyDevice):
  """29. a one-term batch with c' = 1 passes the amplitudes through arithmetic (x + 0): a negative zero loses its sign"""
  def _pauli_unit(self, part):
    return part + 0.0


class PauliNormUnrounded(pm.NumpyDevice):
  """30. at complex64 norm2 is summed from the double values before they are rounded to the handle's width"""
  def _pauli_norm2(self, stored, unrounded):
    return float(np.vdot(unrounded, unrounded).real) if self.dtype == np.complex64 else super()._pauli_norm2(stored, unrounded)


# -- Pauli products.  Which check of _Runner.run_pauli_product catches which (the mutants named "only" pass every fixed program once
#    that one check is deleted; each deletion was tried once, HISTORY.md T4)
#      31, 32  the amplitudes within pauli_product_util.bound: a run whose terms do not commute, a list whose x masks alternate
#      33, 34  the amplitudes (33 on a shard whose held z bits have odd parity, 34 where x & z has an odd number of bits)
#      35      the amplitudes of a run with an exchanging term whose z mask shares an odd number of bits with X
#      36      the amplitudes behind a step with a queue (bound + M _amp_tol)
#      37      the pending count of a REFUSED step on a handle with a queue: the list is checked whole before anything is flushed
#      38      the bit map: it may not move in a step with nothing to flush, nor behind a flush whose relayout mode is off; without
#              those checks, the plan asked before a quiet call against the plan asked behind it
#      39      the plan against the run rule (the engine launches from the plan), then the stats
#      40      only the stats of a quiet step: kernels_launched + 0 for no terms ("only": passes once that check is deleted)
#      41      the pending count behind a step of no terms on a handle with a queue
#      42, 43  only the BYTES of a quiet one-term step on an exact path: equal as numbers, the bound and norm2 see nothing
#      44      only norm2 against the amplitudes read back, 1e-12 relative (complex64)
#      45      norm2 against the amplitudes read back on a list of several runs; without that check, norm2 against the model
#      46      only the stats of a quiet step of several runs: both byte counters + 2 x the shard's bytes PER RUN
class ProductTermsReversed(pm.NumpyDevice):
  """31. apply_pauli_product applies the terms of a run in reverse order"""
  def _pprod_order_run(self, pairs):
    return pairs[::-1]


class ProductSortsByX(pm.NumpyDevice):
  """32. apply_pauli_product sorts the terms stably by x mask first, as the sum does"""
  def _pprod_order_list(self, terms):
    return sorted(terms, key=lambda t: t['px'])


class ProductIgnoresHeldZ(pm.NumpyDevice):
  """33. apply_pauli_product ignores the z bits the shard index holds (no shard sign)"""
  def _pprod_neg(self, term):
    return 0


class ProductPlusI(pm.NumpyDevice):
  """34. apply_pauli_product multiplies by (+i)^nY instead of (-i)^nY"""
  def _pprod_ny(self, term):
    return -term['ny'] & 3


class ProductNeverFlips(pm.NumpyDevice):
  """35. the partner's sign is never flipped: both amplitudes of a pair take the sign of the one whose pivot bit is clear"""
  def _pprod_own_index(self, idx, x):
    if not x:
      return idx
    pivot = np.uint64(1 << (int(x).bit_length() - 1))
    return np.where(idx & pivot != 0, idx ^ np.uint64(x), idx)


class ProductBeforeItsQueue(pm.NumpyDevice):
  """36. apply_pauli_product works before what is queued has run (the queue runs behind the call)"""
  def apply_pauli_product(self, a, b, xmasks, zmasks, norm=False):
    self._pprod_enter = lambda nterms: None
    try:
      res = super().apply_pauli_product(a, b, xmasks, zmasks, norm)
    finally:
      del self._pprod_enter
    self.flush()
    return res


class ProductChecksLateTermsLate(pm.NumpyDevice):
  """37. apply_pauli_product checks the first term, flushes, and refuses a bad later term only then"""
  def _pprod_check(self, av, bv, xs, zs, upto, late=False):
    super()._pprod_check(av, bv, xs, zs, upto if late else min(upto, 1))


class ProductCanonicalises(pm.NumpyDevice):
  """38. apply_pauli_product leaves the local bits in canonical order"""
  def _pprod_layout(self):
    self._canonicalize()


class ProductRunsOf16(pm.NumpyDevice):
  """39. apply_pauli_product cuts its runs every 16 terms"""
  def _pprod_batch(self):
    return 16


class ProductZeroTermsCountAKernel(pm.NumpyDevice):
  """40. apply_pauli_product with no terms counts a kernel"""
  def _pprod_zero_kernels(self):
    return 1


class ProductZeroTermsDoNotFlush(pm.NumpyDevice):
  """41. apply_pauli_product with no terms leaves what is queued in place"""
  def _pprod_enter(self, nterms):
    if nterms:
      self.flush()


class ProductUnitComputes(pm.NumpyDevice):
  """42. a run of one unit string is computed as 0 * x + 1 * P x: a negative zero loses its sign"""
  def _pprod_unit(self, vec, moved):
    return 0.0 * vec + 1.0 * moved


class ProductIdentityComputes(pm.NumpyDevice):
  """43. a run of one factor (1, 0) is computed as 1 * x + 0 * P x: a negative zero loses its sign"""
  def _pprod_identity(self, vec, x, z):
    return 1.0 * vec + 0.0 * self._pprod_partner(vec, x, z)


class ProductNormUnrounded(pm.NumpyDevice):
  """44. at complex64 norm2 is summed from the double values before they are rounded to the handle's width"""
  def _pprod_norm2(self, stored, unrounded, first_stored):
    return float(np.vdot(unrounded, unrounded).real) if self.dtype == np.complex64 else super()._pprod_norm2(stored, unrounded, first_stored)


class ProductNormByFirstRun(pm.NumpyDevice):
  """45. norm2 is summed by the first run of the list, not by the last"""
  def _pprod_norm2(self, stored, unrounded, first_stored):
    return float(np.vdot(first_stored, first_stored).real)


class ProductBytesOncePerCall(pm.NumpyDevice):
  """46. the byte counters grow by 2 x the shard's bytes once per call, not once per run"""
  def _pprod_bytes(self, nruns, shard_bytes):
    return 2 * shard_bytes


# -- reduced densities (47-56, 72, 73, 78) and Z-polynomials (57-71, 74-77, 79-81): one mutant per hook of NumpyDevice, and one
#    for every family of runner checks that none of those needed.  HISTORY.md T5 has the table: for every mutant the family of
#    checks of _Runner.run_reduced_density / run_zpoly / run_expect_zpoly / the refused frame that catches it first, and what
#    catches it once that family is deleted, and so on until it passes every fixed program or a check outside the new code
#    (the next step's pending count, the final chain) takes over
class DensityRowsReversed(pm.NumpyDevice):
  """47. reduced_density takes bits[k-1-t], not bits[t], for bit t of a row number"""
  def _dens_rows(self, bits):
    return bits[::-1]


class DensityTransposed(pm.NumpyDevice):
  """48. reduced_density returns rho transposed (sum_e conj(a(r,e)) a(c,e))"""
  def _dens_orient(self, rho):
    return rho.T.copy()


class DensityNormalised(pm.NumpyDevice):
  """49. reduced_density divides by the trace"""
  def _dens_scale(self, rho):
    t = float(np.trace(rho).real)
    return rho / t if t > 0 else rho


class DensityHeldBitAccepted(pm.NumpyDevice):
  """50. reduced_density drops a listed bit that the shard index holds instead of refusing the call"""
  def _dens_local(self, b):
    return True


class DensityFoldCounted(pm.NumpyDevice):
  """51. reduced_density counts its fold kernel"""
  def _dens_kernels(self):
    return 2


class DensityDoesNotFlush(pm.NumpyDevice):
  """52. reduced_density reads the state without running what is queued"""
  def _dens_enter(self):
    pass


class DensityBothTrianglesComputed(pm.NumpyDevice):
  """53. reduced_density computes the lower triangle on its own: an ulp away from the mirror of the upper one"""
  def _dens_mirror(self, rho):
    return np.triu(rho) + np.tril(rho, -1) * (1 + 2.0 ** -52)


class DensityCanonicalises(pm.NumpyDevice):
  """54. reduced_density leaves the local bits in canonical order"""
  def _dens_layout(self):
    self._canonicalize()


class DensitySweptIsTheShard(pm.NumpyDevice):
  """55. bytes_swept grows by the shard's bytes, not by the bytes the kernel requests (k = 7, 8 read the state 2, 4 times)"""
  def _dens_swept(self, plan, amp_bytes):
    return (1 << self.nbits) * amp_bytes


class DensityRefusalFlushes(pm.NumpyDevice):
  """56. reduced_density runs what is queued before it checks its arguments"""
  def _dens_check(self, who, bits):
    if who == 'reduced_density':
      self.flush()
    super()._dens_check(who, bits)


class ZpolySignFlipped(pm.NumpyDevice):
  """57. a term counts -w where the parity of i & z is even"""
  def _zp_parity(self, w, z):
    return -w if z else w


class ZpolyConstantDropped(pm.NumpyDevice):
  """58. a constant term (no local z bit) is dropped"""
  def _zp_terms(self, terms):
    return [(w, z) for w, z in terms if z]


class ZpolyHeldSignNotFolded(pm.NumpyDevice):
  """59. the sign the shard index gives a held z bit is not folded into the weight"""
  def _zp_fold(self, w, z, held):
    return w


class ZpolyConjugatesC(pm.NumpyDevice):
  """60. apply_zpoly multiplies by exp(conj(c) f)"""
  def _zp_c(self, c):
    return c.conjugate()


class ZpolyLeavesOutExp(pm.NumpyDevice):
  """61. apply_zpoly leaves exp(c.re f) out: the phase alone"""
  def _zp_factor(self, c, f):
    return np.cos(c.imag * f) + 1j * np.sin(c.imag * f)


class ZpolyNormBeforeTheApply(pm.NumpyDevice):
  """62. norm2 of apply_zpoly is summed from the amplitudes as they were before the call"""
  def _zp_norm2(self, first, stored):
    return first


class ZpolyNoopCountsAKernel(pm.NumpyDevice):
  """63. apply_zpoly with no terms or c == (0, 0) counts a kernel"""
  def _zp_noop_kernels(self):
    return 1


class ZpolyCanonicalises(pm.NumpyDevice):
  """64. apply_zpoly leaves the local bits in canonical order"""
  def _zp_layout(self):
    self._canonicalize()


class ZpolyRefusalFlushes(pm.NumpyDevice):
  """65. apply_zpoly / expect_zpoly run what is queued before they check their arguments"""
  def _zp_check(self, who, ws, zs, c=None):
    if who != 'zpoly_plan':
      self.flush()
    super()._zp_check(who, ws, zs, c)


class ZpolyDoesNotFlush(pm.NumpyDevice):
  """66. apply_zpoly works on the state without running what is queued"""
  def _zp_enter(self):
    pass


class ZpolyBytesOnce(pm.NumpyDevice):
  """67. the byte counters of apply_zpoly grow by 1 x the shard's bytes"""
  def _zp_bytes(self, shard_bytes):
    return shard_bytes


class ExpectSecondIsMeanSquared(pm.NumpyDevice):
  """68. the third sum of expect_zpoly is (sum p f)^2 / sum p"""
  def _ezp_second(self, p, f):
    return float(np.dot(p, f)) ** 2 / float(np.sum(p))


class ExpectDoesNotFlush(pm.NumpyDevice):
  """69. expect_zpoly reads the state without running what is queued"""
  def _ezp_enter(self):
    pass


class ExpectCanonicalises(pm.NumpyDevice):
  """70. expect_zpoly leaves the local bits in canonical order"""
  def _ezp_layout(self):
    self._canonicalize()


class ExpectBytesTwice(pm.NumpyDevice):
  """71. the byte counters of expect_zpoly grow by 2 x the shard's bytes"""
  def _ezp_bytes(self, shard_bytes):
    return 2 * shard_bytes


class DensityNotRepeatable(pm.NumpyDevice):
  """72. every second call of reduced_density sums in another order: an ulp away in one entry"""
  def reduced_density(self, bits):
    rho = super().reduced_density(bits)
    self._dens_calls = getattr(self, '_dens_calls', 0) + 1
    if self._dens_calls % 2 == 0 and rho.size > 1:
      rho[0, 1] *= 1 + 2.0 ** -52
      rho[1, 0] = np.conj(rho[0, 1])
    elif self._dens_calls % 2 == 0:
      rho[0, 0] *= 1 + 2.0 ** -52
    return rho


class DensityRefusalTouchesTheState(pm.NumpyDevice):
  """73. a refused reduced_density negates the first stored amplitude"""
  def _dens_check(self, who, bits):
    try:
      super()._dens_check(who, bits)
    except pm.native.QhError:
      if who == 'reduced_density':
        self.phys[0] = -self.phys[0]
      raise


class ZpolyNotRepeatable(pm.NumpyDevice):
  """74. every second apply_zpoly sums its norm2 in another order: an ulp away"""
  def _zp_norm2(self, first, stored):
    self._zp_calls = getattr(self, '_zp_calls', 0) + 1
    return super()._zp_norm2(first, stored) * (1 + 2.0 ** -52 * (self._zp_calls % 2 == 0))


class ZpolyRefusalCountsAGate(pm.NumpyDevice):
  """75. a refused apply_zpoly / expect_zpoly counts gates_submitted + 1"""
  def _zp_check(self, who, ws, zs, c=None):
    try:
      super()._zp_check(who, ws, zs, c)
    except pm.native.QhError:
      self.submitted += who != 'zpoly_plan'
      raise


class ExpectNotRepeatable(pm.NumpyDevice):
  """76. every second expect_zpoly sums in another order: the second moment an ulp away"""
  def _ezp_second(self, p, f):
    self._ezp_calls = getattr(self, '_ezp_calls', 0) + 1
    return super()._ezp_second(p, f) * (1 + 2.0 ** -52 * (self._ezp_calls % 2 == 0))


class ExpectZeroTermsSumApart(pm.NumpyDevice):
  """77. expect_zpoly with no terms sums |a|^2 in an order of its own: an ulp away from norm2"""
  def expect_zpoly(self, weights, zmasks):
    out = super().expect_zpoly(weights, zmasks)
    return out if len(zmasks) else (out[0] * (1 + 2.0 ** -52), out[1], out[2])


class DensityTouchesTheState(pm.NumpyDevice):
  """78. reduced_density negates the first stored amplitude on its way out"""
  def _dens_layout(self):
    self.phys[0] = -self.phys[0]


class ExpectTouchesTheState(pm.NumpyDevice):
  """79. expect_zpoly negates the first stored amplitude on its way out"""
  def _ezp_layout(self):
    self.phys[0] = -self.phys[0]


class ZpolyNoopNormSumsApart(pm.NumpyDevice):
  """80. apply_zpoly with no terms or c == (0, 0) sums its norm2 in an order of its own: an ulp away from norm2"""
  def apply_zpoly(self, weights, zmasks, c, norm=False):
    n2 = super().apply_zpoly(weights, zmasks, c, norm)
    return n2 * (1 + 2.0 ** -52) if norm and (not len(zmasks) or complex(c) == 0) else n2


class ZpolyNamesAnotherTerm(pm.NumpyDevice):
  """81. a refused apply_zpoly / expect_zpoly names the last term of the list, not the first offending one"""
  def _zp_check(self, who, ws, zs, c=None):
    try:
      super()._zp_check(who, ws, zs, c)
    except pm.native.QhError as e:
      raise pm.native.QhError(e.code, f'{who}: term {len(zs) - 1} has a non-finite weight') if 'non-finite weight' in str(e) else e


DENSITY_MUTANTS = [DensityRowsReversed, DensityTransposed, DensityNormalised, DensityHeldBitAccepted, DensityFoldCounted, DensityDoesNotFlush,
                   DensityBothTrianglesComputed, DensityCanonicalises, DensitySweptIsTheShard, DensityRefusalFlushes,
                   DensityNotRepeatable, DensityRefusalTouchesTheState, DensityTouchesTheState]
ZPOLY_MUTANTS = [ZpolySignFlipped, ZpolyConstantDropped, ZpolyHeldSignNotFolded, ZpolyConjugatesC, ZpolyLeavesOutExp, ZpolyNormBeforeTheApply,
                 ZpolyNoopCountsAKernel, ZpolyCanonicalises, ZpolyRefusalFlushes, ZpolyDoesNotFlush, ZpolyBytesOnce, ExpectSecondIsMeanSquared,
                 ExpectDoesNotFlush, ExpectCanonicalises, ExpectBytesTwice, ZpolyNotRepeatable, ZpolyRefusalCountsAGate, ExpectNotRepeatable,
                 ExpectZeroTermsSumApart, ExpectTouchesTheState, ZpolyNoopNormSumsApart, ZpolyNamesAnotherTerm]
MUTANTS = [QueueBehindBarrier, CopyKeepsQueue, CopyDropsBitmap, ReleaseKeepsLogicalNumbers, ExtendOnTop, MuxSelectorsReversed,
           TopkTiesByPhysicalIndex, AxpbyReadsDstAnyway, SelectInPhysicalOrder, ReaderCanonicalises, MarginalIgnoresHeldBits,
           RoundsTwice, ReaderTurnsRelayoutOn, PermTableBackwards, PermBitsAscending, PermHeldControlMet, PermCanonicalises,
           PermNoopCountsAKernel, PermComputes, PermBeforeItsQueue, PauliIgnoresHeldZ, PauliPlusI, PauliDstKeepsBitmap,
           PauliDstKeepsQueue, PauliBeforeSrcQueue, PauliLaterBatchOverwrites, PauliFirstBatchReadsDst, PauliZeroTermsCountNothing,
           PauliUnitComputes, PauliNormUnrounded, ProductTermsReversed, ProductSortsByX, ProductIgnoresHeldZ, ProductPlusI,
           ProductNeverFlips, ProductBeforeItsQueue, ProductChecksLateTermsLate, ProductCanonicalises, ProductRunsOf16,
           ProductZeroTermsCountAKernel, ProductZeroTermsDoNotFlush, ProductUnitComputes, ProductIdentityComputes, ProductNormUnrounded,
           ProductNormByFirstRun, ProductBytesOncePerCall] + DENSITY_MUTANTS + ZPOLY_MUTANTS
PERM_MUTANTS = MUTANTS[13:20]
PAULI_MUTANTS = MUTANTS[20:30]
PRODUCT_MUTANTS = MUTANTS[30:46]


def _product_step(s):
  """a 'pauli_product' step, or a call of apply_pauli_product that is to be refused"""
  return s['op'] == 'pauli_product' or (s['op'] == 'refused' and s['what'].startswith('pauli_product_'))


def _density_step(s):
  """a 'reduced_density' step, or a call of reduced_density that is to be refused"""
  return s['op'] == 'reduced_density' or (s['op'] == 'refused' and s['what'].startswith('density_'))


def _zpoly_step(s, ops=('zpoly', 'expect_zpoly')):
  """a 'zpoly' / 'expect_zpoly' step, or a call of apply_zpoly / expect_zpoly that is to be refused"""
  return s['op'] in ops or (s['op'] == 'refused' and s['what'].startswith(tuple(op + '_' for op in ops)))


@pytest.mark.parametrize('mutant', MUTANTS, ids=[m.__name__ for m in MUTANTS])
def test_the_runner_fails_on_a_broken_device(mutant):
  order = sorted(((mode, seed, bw) for bw in WIDTHS for mode, seed in pm.FIXED), key=lambda k: len(program(*k)[0]['slots']) << program(*k)[0]['nloc'])
  if mutant in PERM_MUTANTS:                                  # (they differ from NumpyDevice in apply_perm alone)
    order = [key for key in order if any(s['op'] == 'perm' for s in program(*key))]
    if mutant in (PermHeldControlMet, PermNoopCountsAKernel):                       # ... and these on a shard alone
      order = [key for key in order if key[0] == 'shard']
  if mutant in PAULI_MUTANTS:                                 # (they differ from NumpyDevice in apply_pauli_sum alone)
    order = [key for key in order if any(s['op'] == 'pauli_sum' for s in program(*key))]
    if mutant is PauliIgnoresHeldZ:
      order = [key for key in order if key[0] == 'shard']
    if mutant is PauliNormUnrounded:
      order = [key for key in order if key[2] == 64]
  if mutant in PRODUCT_MUTANTS:                               # (they differ from NumpyDevice in apply_pauli_product alone)
    order = [key for key in order if any(_product_step(s) for s in program(*key))]
    if mutant is ProductIgnoresHeldZ:
      order = [key for key in order if key[0] == 'shard']
    if mutant is ProductNormUnrounded:
      order = [key for key in order if key[2] == 64]
    if mutant is ProductZeroTermsDoNotFlush:                  # (it differs on a list of no terms alone)
      order = [key for key in order if any(s['op'] == 'pauli_product' and not s['x'] for s in program(*key))]
  if mutant in DENSITY_MUTANTS:                               # (they differ from NumpyDevice in reduced_density alone)
    order = [key for key in order if any(_density_step(s) for s in program(*key))]
    if mutant is DensityHeldBitAccepted:
      order = [key for key in order if key[0] == 'shard']
    if mutant is DensitySweptIsTheShard:                      # (it differs where the state is read more than once alone)
      order = [key for key in order if any(s['op'] == 'reduced_density' and len(s['bits']) >= 7 for s in program(*key))]
  if mutant in ZPOLY_MUTANTS:                                 # (they differ from NumpyDevice in apply_zpoly / expect_zpoly alone)
    ops = ('expect_zpoly',) if mutant.__name__.startswith('Expect') else \
        ('zpoly',) if (mutant in ZPOLY_MUTANTS[3:11] and mutant is not ZpolyRefusalFlushes) or mutant in (ZpolyNotRepeatable, ZpolyNoopNormSumsApart) else ('zpoly', 'expect_zpoly')
    order = [key for key in order if any(_zpoly_step(s, ops) for s in program(*key))]
    if mutant is ZpolyHeldSignNotFolded:
      order = [key for key in order if key[0] == 'shard']
  for key in order:
    try:
      run_on(mutant, *key)
    except pm.StepFailure as e:
      print(f'{mutant.__name__}: {key}: {e}'[:400])
      assert f'step {e.index} ' in str(e) and 0 <= e.index <= len(program(*key))      # the assertion names the step
      if mutant in PERM_MUTANTS:                                                      # ... and it is a permutation that breaks them
        assert e.step['op'] == 'perm', e.step['op']
      if mutant in PAULI_MUTANTS:                                                     # ... or a Pauli sum
        assert e.step['op'] == 'pauli_sum', e.step['op']
      if mutant in PRODUCT_MUTANTS:                                                   # ... or a Pauli product (applied or refused)
        assert _product_step(e.step), e.step
      if mutant in DENSITY_MUTANTS:                                                   # ... or a reduced density
        assert _density_step(e.step), e.step
      if mutant in ZPOLY_MUTANTS:                                                     # ... or a Z-polynomial
        assert _zpoly_step(e.step), e.step
      return
  raise AssertionError(f'{mutant.__name__} ({mutant.__doc__}) passes every fixed program')


# ---- coverage of the fixed programs ------------------------------------------------------------------------------------------------
def coverage(bw):
  kinds = dict.fromkeys(pm.KINDS, 0)
  permuted = dict.fromkeys(pm.BARRIERS + pm.READERS, 0)
  queued = dict.fromkeys(pm.BARRIERS + pm.READERS + ('clone', 'copy', 'extend', 'release', 'inner', 'axpby', 'pauli_sum', 'pauli_product', 'zpoly', 'remap'), 0)
  paths = {(op, p): 0 for op in pm.TWO_STATE for p in (pm.LINEAR, pm.TILES, pm.GATHER)}
  for (mode, seed, w), c in checks().items():
    if w != bw:
      continue
    for _, op, perm, q, path, _ in c.events:
      kinds[op] += 1
      if op in permuted and perm:
        permuted[op] += 1
      if op in queued and q:
        queued[op] += 1
      if path is not None:
        paths[op, path] += 1
  return kinds, permuted, queued, paths


def perm_coverage(bw):
  """what the 'perm' steps of the fixed programs met, from the path NumpyDevice.perm_plan predicts on its own bit map; a path
  counts where the call ran a kernel (a held control that is 0 on the shard runs none)"""
  lds, gather = pm.native.QH_PERM_LDS, pm.native.QH_PERM_GATHER
  names = ('lds', 'gather', 'gather, relayout buffer', 'gather, temporary', 'layout band', 'layout band, queued, relayout on', 'local control',
           'held control met', 'held control unmet', 'k == nloc', 'nloc < 10', 'gather on a shard', 'shard, held bit inside the register') + tuple('band ' + b for b in pm.PERM_BANDS)
  n = dict.fromkeys(names, 0)
  for (mode, seed, w), c in checks().items():
    for _, op, _, q, _, r in c.events:
      if w != bw or op != 'perm':
        continue
      ran = r['ctl_met'] == 1
      n['lds'] += ran and r['path'] == lds
      n['gather'] += ran and r['path'] == gather
      n['gather, relayout buffer'] += ran and r['path'] == gather and r['relayout_on']
      n['gather, temporary'] += ran and r['path'] == gather and not r['relayout_on']
      n['band ' + r['band']] += 1
      n['layout band'] += r['band'] == 'layout'
      n['layout band, queued, relayout on'] += r['band'] == 'layout' and q and r['relayout_on']
      n['local control'] += r['ctl_local']
      n['held control met'] += mode == 'shard' and r['ctl_held'] and ran
      n['held control unmet'] += mode == 'shard' and r['ctl_held'] and not ran
      n['k == nloc'] += r['k'] == r['nloc']
      n['nloc < 10'] += r['nloc'] < 10
      n['gather on a shard'] += ran and r['path'] == gather and r['shard']
      n['shard, held bit inside the register'] += ran and r['held_inside']      # (the 'mid3' / 'midhalf' starts)
  for (mode, seed, w) in checks():                             # the refusals of apply_perm, from the programs themselves
    for s in program(mode, seed, w):
      if w == bw and s['op'] == 'refused' and s['what'].startswith('perm_'):
        n['refused: ' + s['what']] = n.get('refused: ' + s['what'], 0) + 1
  return {k: int(v) for k, v in n.items()}


PERM_AT_LEAST = {'lds': 3, 'gather': 2, 'gather, relayout buffer': 1, 'gather, temporary': 1, 'layout band': 2,
                 'layout band, queued, relayout on': 1, 'local control': 3, 'held control met': 1, 'held control unmet': 1, 'k == nloc': 1,
                 'nloc < 10': 1, 'gather on a shard': 1, 'shard, held bit inside the register': 1, 'refused: perm_not_bijection': 1,
                 'refused: perm_control_in_register': 1, 'refused: perm_register_held': 1}


def pauli_counts(records, bw):
  """what 'pauli_sum' steps met, from (mode, non-identity local map, record of _Runner.run_pauli_sum); shared with the closing
  item of tests/test_gpu_program_fuzz.py, which counts what the real qh_pauli_sum_plan and qh_get_bitmap said"""
  n = {}
  def count(name, cond):
    n[name] = n.get(name, 0) + bool(cond)
  for mode, permuted, r in records:
    classes = set(r['classes']) if r['main'] else set()
    count('k_pauli_small shape', not r['main'])
    count('main shape', r['main'])
    for slots in ('few', 'many'):
      for groups in ('one', 'several'):
        count(f'main shape: {slots} term slots, {groups} x mask{"s" if groups == "several" else ""}', (slots, groups) in classes)
    count('an accumulating batch (17 or more terms)', r['nbatches'] >= 2)
    count('an accumulating batch on the main shape', r['nbatches'] >= 2 and r['main'])
    count('zero terms', r['zero'])
    count("a unit term with c' == 1", r['unit'] == 0)
    count("a unit term with c' != c", r['unit'] is not None and r['changed'])
    count('into a new handle', r['new'])
    count('into an existing handle', not r['new'])
    count('dst with a queue dropped', r['dst_queued'])
    count('dst poisoned', r['poisoned'])
    count('src with a burst queued and relayout on, at 14 or more local bits', r['queued'] and r['relayout_on'] and r['nloc'] >= 14)
    count("on a non-identity local map its own flush left", r['relaid'])
    count('on a non-identity local map', permuted)
    count('shard: a held z bit with neg set', r['shard'] and r['held_z'] and r['neg'])
    count('shard: main shape', r['shard'] and r['main'])
    count('shard: main shape with neg set', r['shard'] and r['main'] and r['neg'])
    count("'attached' programs: dst the attached handle", mode == 'attached' and r['dst_fixed'])
    count("'mapped' programs: dst the mapped handle", mode == 'mapped' and r['dst_fixed'])
    if bw == 64:
      count('complex64: px bit 0 set', r['px0'])
      count('complex64: pz bit 0 set', r['pz0'])
  return n


def pauli_coverage(bw):
  """what the 'pauli_sum' steps of the fixed programs met, from the plan NumpyDevice.pauli_sum_plan gives on its own bit map"""
  n = pauli_counts([(mode, e[2], e[5]) for (mode, seed, w), c in checks().items() if w == bw for e in c.events if e[1] == 'pauli_sum'], bw)
  for (mode, seed, w) in checks():                             # the refusals of apply_pauli_sum, from the programs themselves
    for s in program(mode, seed, w):
      if w == bw and s['op'] == 'refused' and s['what'].startswith('pauli_sum_'):
        n['refused: ' + s['what']] = n.get('refused: ' + s['what'], 0) + 1
  return n


PAULI_AT_LEAST = {'k_pauli_small shape': 2, 'main shape': 3, 'main shape: few term slots, one x mask': 1,
                  'main shape: few term slots, several x masks': 1, 'main shape: many term slots, one x mask': 1,
                  'main shape: many term slots, several x masks': 1, 'an accumulating batch (17 or more terms)': 2, 'zero terms': 1,
                  "a unit term with c' == 1": 1, "a unit term with c' != c": 1, 'into a new handle': 2, 'into an existing handle': 2,
                  'dst with a queue dropped': 1, 'dst poisoned': 1, 'src with a burst queued and relayout on, at 14 or more local bits': 1,
                  'on a non-identity local map': 3, 'shard: a held z bit with neg set': 1, 'shard: main shape': 1,
                  "'attached' programs: dst the attached handle": 1, "'mapped' programs: dst the mapped handle": 1,
                  'refused: pauli_sum_self': 1, 'refused: pauli_sum_bad_qubit': 1, 'refused: pauli_sum_x_held': 1}
PAULI_AT_LEAST_64 = {'complex64: px bit 0 set': 2, 'complex64: pz bit 0 set': 2}


PRODUCT_WALKS = ('diag', 'lane', 'pair', 'half')           # program_model.pauli_product_walk on the main shape ('half': complex64 alone)


def pauli_product_counts(records, bw):
  """what 'pauli_product' steps met, from (mode, non-identity local map, record of _Runner.run_pauli_product); shared with the
  closing item of tests/test_gpu_program_fuzz.py, which counts what the real qh_pauli_product_plan and qh_get_bitmap said"""
  n = {}
  def count(name, cond):
    n[name] = n.get(name, 0) + bool(cond)
  for mode, permuted, r in records:
    runs = r['runs']
    count('k_pauli_product_small shape', not r['main'] and not r['zero'])
    count('main shape', r['main'] and not r['zero'])
    for walk in PRODUCT_WALKS[:4 if bw == 64 else 3]:
      for slots in ('few', 'many'):
        count(f'main shape: {walk} walk, {slots} term slots', any(x['walk'] == walk and x['slots'] == slots for x in runs))
    count('three or more runs', r['nruns'] >= 3)
    count('three or more runs on the main shape', r['nruns'] >= 3 and r['main'])
    count('several runs, norm2 asked', r['nruns'] >= 2 and r['norm'])
    count('several runs, norm2 not asked', r['nruns'] >= 2 and not r['norm'])
    count('a run with flip set', any(x['flip'] for x in runs))
    count('a run with flip set on the main shape', r['main'] and any(x['flip'] and x['kind'] != pm.native.QH_PAULI_RUN_DIAG for x in runs))
    count('a run mixing diagonal and exchanging terms', any(x['mixed'] for x in runs))
    count('exact path: one unit string', any(x['exact'] == 'string' for x in runs))
    count('exact path: the factor (1, 0)', any(x['exact'] == 'identity' for x in runs))
    count('zero terms', r['zero'])
    count('zero terms behind a queue', r['zero'] and r['queued'])
    count('behind a queued burst', r['queued'])
    count('behind a queued burst with relayout on, at 14 or more local bits', r['queued'] and r['relayout_on'] and r['nloc'] >= 14)
    count('on a non-identity local map its own flush left', r['relaid'])
    count('on a non-identity local map', permuted)
    count('shard: a held z bit with neg set', r['shard'] and r['held_z'] and r['neg'])
    count('shard: main shape with neg set', r['shard'] and r['main'] and r['neg'])
    count('on an attached handle', mode == 'attached' and r['fixed'])
    count('on a host-mapped handle', mode == 'mapped' and r['fixed'])
    if bw == 64:
      count('complex64: physical bit 0 in X of a pair or lane run', any(x['px0'] and x['walk'] in ('pair', 'lane') for x in runs))
      count('complex64: physical bit 0 in a z mask', r['pz0'])
  return n


def pauli_product_coverage(bw):
  """what the 'pauli_product' steps of the fixed programs met, from the plan NumpyDevice.pauli_product_plan gives on its own bit map"""
  n = pauli_product_counts([(mode, e[2], e[5]) for (mode, seed, w), c in checks().items() if w == bw for e in c.events if e[1] == 'pauli_product'], bw)
  for (mode, seed, w) in checks():                             # the refusals of apply_pauli_product, from the programs themselves
    for s in program(mode, seed, w):
      if w == bw and s['op'] == 'refused' and s['what'].startswith('pauli_product_'):
        n['refused: ' + s['what']] = n.get('refused: ' + s['what'], 0) + 1
        n['refused on a handle with a queue'] = n.get('refused on a handle with a queue', 0) + bool(s['queued'])
  return n


PAULI_PRODUCT_AT_LEAST = dict({'k_pauli_product_small shape': 3, 'main shape': 3, 'three or more runs': 3, 'three or more runs on the main shape': 1,
                               'several runs, norm2 asked': 2, 'several runs, norm2 not asked': 2, 'a run with flip set': 3,
                               'a run with flip set on the main shape': 1, 'a run mixing diagonal and exchanging terms': 2,
                               'exact path: one unit string': 2, 'exact path: the factor (1, 0)': 1, 'zero terms': 1, 'zero terms behind a queue': 1,
                               'behind a queued burst': 3, 'behind a queued burst with relayout on, at 14 or more local bits': 1,
                               'on a non-identity local map': 3, 'shard: a held z bit with neg set': 1, 'shard: main shape with neg set': 1,
                               'on an attached handle': 1, 'on a host-mapped handle': 1, 'refused: pauli_product_nonfinite': 1,
                               'refused: pauli_product_bad_qubit': 1, 'refused: pauli_product_x_held': 1, 'refused on a handle with a queue': 1},
                              **{f'main shape: {walk} walk, {slots} term slots': 1 for walk in PRODUCT_WALKS[:3] for slots in ('few', 'many')})
PAULI_PRODUCT_AT_LEAST_64 = {'main shape: half walk, few term slots': 1, 'main shape: half walk, many term slots': 1,
                             'complex64: physical bit 0 in X of a pair or lane run': 1, 'complex64: physical bit 0 in a z mask': 2}


def density_counts(records, bw):
  """what 'reduced_density' steps met, from (mode, non-identity local map, record of _Runner.run_reduced_density); shared with the
  closing item of tests/test_gpu_program_fuzz.py, which counts what the real qh_density_plan and qh_get_bitmap said"""
  n = {}
  def count(name, cond):
    n[name] = n.get(name, 0) + bool(cond)
  for mode, permuted, r in records:
    tiles = r['path'] == pm.native.QH_DENSITY_TILES
    count('GATHER path', not tiles)
    count('TILES path', tiles)
    count('k = 0', r['k'] == 0)
    count('k in 1-2', 1 <= r['k'] <= 2)
    count('k in 3-5', 3 <= r['k'] <= 5)
    count('k = 6', r['k'] == 6)
    count('k = 7 (3 block pairs)', r['k'] == 7 and r['block_pairs'] == 3)
    count('k = 8 (10 block pairs)', r['k'] == 8 and r['block_pairs'] == 10)
    count('k = nloc', r['k'] == r['nloc'])
    count('row_bit not the identity', not r['row_identity'])
    count('the register holds physical position 0', r['pos0'])
    count('the register holds physical positions 0 and 1', r['pos01'])
    count('chunk_bits cut short by the environment', tiles and r['nrest'] == 0)      # cb == ne
    count('chunks_per_wg > 1', tiles and r['chunks_per_wg'] > 1)
    count('behind a queued burst', r['queued'])
    count('on a non-identity local map its own flush left', r['relaid'])
    count('on a non-identity local map', permuted)
    count('on a shard', r['shard'])
    count('on an attached handle', mode == 'attached' and r['fixed'])
    count('on a host-mapped handle', mode == 'mapped' and r['fixed'])
    count('right behind extend, release or copy', r['fresh'] is not None)
  return n


DENSITY_LINES = ('GATHER path', 'TILES path', 'k = 0', 'k in 1-2', 'k in 3-5', 'k = 6', 'k = 7 (3 block pairs)', 'k = 8 (10 block pairs)', 'k = nloc',
                 'row_bit not the identity', 'the register holds physical position 0', 'the register holds physical positions 0 and 1',
                 'chunk_bits cut short by the environment', 'behind a queued burst', 'on a non-identity local map its own flush left', 'on a shard',
                 'on an attached handle', 'on a host-mapped handle', 'right behind extend, release or copy')      # ('chunks_per_wg > 1': at either width)
DENSITY_AT_LEAST = dict({k: 1 for k in DENSITY_LINES}, **{'GATHER path': 2, 'TILES path': 3, 'row_bit not the identity': 3, 'behind a queued burst': 3,
                                                          'on a non-identity local map': 3, 'refused: density_nonlocal': 1, 'refused: density_same_qubit': 1,
                                                          'refused: density_bad_qubit': 1, 'refused: density_k_range': 1})


def zpoly_counts(records, bw):
  """what 'zpoly' or 'expect_zpoly' steps met, from (mode, non-identity local map, record of _Runner.run_zpoly / run_expect_zpoly);
  shared with the closing item of tests/test_gpu_program_fuzz.py, which counts what the real qh_zpoly_plan and qh_get_bitmap said"""
  n = {}
  def count(name, cond):
    n[name] = n.get(name, 0) + bool(cond)
  for mode, permuted, r in records:
    count('small kernel', not r['main'] and r['nterms'])
    count('main kernel', r['main'] and r['nterms'])
    for c in pm.ZPOLY_CLASSES.values():
      count(f'main kernel: a {c} term', c in r['classes'])
    for kd in pm.ZPOLY_GROUP_KINDS:
      count(f'a {kd} group', r['group_kinds'][kd] >= 1)
    count('two or more groups of one kind', any(v >= 2 for v in r['group_kinds'].values()))
    count('a segment with more than 64 terms', r['seg_over_64'])
    count('a segment with 2 to 63 terms', r['seg_2_to_63'])
    count('4096 terms', r['nterms'] == pm.ZPOLY_MAX_TERMS)
    count('duplicate masks', r['duplicates'])
    count('zero terms', r['nterms'] == 0)
    count('zero terms behind a queue', r['nterms'] == 0 and r['queued'])
    count('behind a queued burst', r['queued'])
    count('shard: a held bit in a mask where the sign is negative', r['shard'] and r['neg_held'])
    count('on a non-identity local map its own flush left', r['relaid'])
    count('on a non-identity local map', permuted)
    count('on an attached handle', mode == 'attached' and r['fixed'])
    count('on a host-mapped handle', mode == 'mapped' and r['fixed'])
    if r['c'] is not None:                                   # apply_zpoly alone
      for kind, name in (('re0', 'c.re == 0'), ('im0', 'c.im == 0'), ('general', 'general c'), ('zero', 'c == (0, 0)')):
        count(name, r['c'] == kind)
      count('norm2 asked', r['norm'])
      count('norm2 not asked', not r['norm'])
    if bw == 64:
      count('complex64: physical bit 0 in a mask', r['pz0'])
  return n


ZPOLY_LINES = ('small kernel', 'main kernel') + tuple(f'main kernel: a {c} term' for c in pm.ZPOLY_CLASSES.values()) + \
    tuple(f'a {kd} group' for kd in pm.ZPOLY_GROUP_KINDS) + ('two or more groups of one kind', 'a segment with more than 64 terms', 'a segment with 2 to 63 terms',
                                                            '4096 terms', 'duplicate masks', 'shard: a held bit in a mask where the sign is negative',
                                                            'on a non-identity local map its own flush left', 'on an attached handle', 'on a host-mapped handle')
ZPOLY_APPLY_LINES = ZPOLY_LINES + ('c.re == 0', 'c.im == 0', 'general c', 'c == (0, 0)', 'zero terms behind a queue', 'norm2 asked', 'norm2 not asked')
ZPOLY_LINES_64 = ('complex64: physical bit 0 in a mask',)
ZPOLY_AT_LEAST = dict({k: 1 for k in ZPOLY_APPLY_LINES}, **{'small kernel': 3, 'main kernel': 3, 'behind a queued burst': 3, 'on a non-identity local map': 3,
                                                            'refused: zpoly_nonfinite': 1, 'refused: zpoly_bad_qubit': 1, 'refused: zpoly_too_many': 1})
EXPECT_ZPOLY_AT_LEAST = dict({k: 1 for k in ZPOLY_LINES}, **{'small kernel': 3, 'main kernel': 3, 'zero terms': 1, 'behind a queued burst': 3,
                                                             'on a non-identity local map': 3, 'refused: expect_zpoly_nonfinite': 1,
                                                             'refused: expect_zpoly_bad_qubit': 1, 'refused: expect_zpoly_too_many': 1})


def new_kind_coverage(op, bw):
  """what the steps of one of the three kinds met in the fixed programs, from the plans NumpyDevice gives on its own bit map, and
  the refusals of its call from the programs themselves"""
  records = [(mode, e[2], e[5]) for (mode, seed, w), c in checks().items() if w == bw for e in c.events if e[1] == op]
  n = density_counts(records, bw) if op == 'reduced_density' else zpoly_counts(records, bw)
  prefix = 'density_' if op == 'reduced_density' else op + '_'
  for (mode, seed, w) in checks():
    for s in program(mode, seed, w):
      if w == bw and s['op'] == 'refused' and s['what'].startswith(prefix):
        n['refused: ' + s['what']] = n.get('refused: ' + s['what'], 0) + 1
        n['refused on a handle with a queue'] = n.get('refused on a handle with a queue', 0) + bool(s['queued'])
  return n


@pytest.mark.parametrize('bw', WIDTHS)
def test_coverage_of_the_fixed_programs(bw):
  kinds, permuted, queued, paths = coverage(bw)
  print(f'\ncoverage of the {len(pm.FIXED)} fixed programs at complex{bw}: step kind: times met / on a non-identity local map / behind a queued burst')
  for k in pm.KINDS:
    print(f'  {k:13s} {kinds[k]:4d} {permuted.get(k, "-"):>4} {queued.get(k, "-"):>4}')
  names = {pm.LINEAR: 'linear', pm.TILES: 'tiles', pm.GATHER: 'gather'}
  print('  two-state paths: ' + ', '.join(f'{op} {names[p]} {n}' for (op, p), n in paths.items()))
  assert all(n >= 8 for n in kinds.values()), kinds
  assert all(n >= 3 for n in permuted.values()), permuted
  assert all(n >= 2 for n in paths.values()), paths
  assert all(n >= 2 for n in queued.values()), queued        # (every barrier mutator, and every other step that runs a queue)
  perms = perm_coverage(bw)
  print('  perm steps: ' + ', '.join(f'{k} {n}' + (f' (>= {PERM_AT_LEAST[k]})' if k in PERM_AT_LEAST else '') for k, n in perms.items()))
  assert all(perms.get(k, 0) >= least for k, least in PERM_AT_LEAST.items()), perms
  least = dict(PAULI_AT_LEAST, **(PAULI_AT_LEAST_64 if bw == 64 else {}))
  paulis = pauli_coverage(bw)
  print('  pauli_sum steps: ' + ', '.join(f'{k} {n}' + (f' (>= {least[k]})' if k in least else '') for k, n in paulis.items()))
  assert all(paulis.get(k, 0) >= v for k, v in least.items()), {k: paulis.get(k, 0) for k, v in least.items() if paulis.get(k, 0) < v}
  least = dict(PAULI_PRODUCT_AT_LEAST, **(PAULI_PRODUCT_AT_LEAST_64 if bw == 64 else {}))
  products = pauli_product_coverage(bw)
  print('  pauli_product steps: ' + ', '.join(f'{k} {n}' + (f' (>= {least[k]})' if k in least else '') for k, n in products.items()))
  assert all(products.get(k, 0) >= v for k, v in least.items()), {k: products.get(k, 0) for k, v in least.items() if products.get(k, 0) < v}
  for op, table in (('reduced_density', DENSITY_AT_LEAST), ('zpoly', ZPOLY_AT_LEAST), ('expect_zpoly', EXPECT_ZPOLY_AT_LEAST)):
    least = dict(table, **({k: 1 for k in ZPOLY_LINES_64} if bw == 64 and op != 'reduced_density' else {}))
    met = new_kind_coverage(op, bw)
    print(f'  {op} steps: ' + ', '.join(f'{k} {n}' + (f' (>= {least[k]})' if k in least else '') for k, n in met.items()))
    assert all(met.get(k, 0) >= v for k, v in least.items()), (op, {k: met.get(k, 0) for k, v in least.items() if met.get(k, 0) < v})
  both = sum(new_kind_coverage('reduced_density', w).get('chunks_per_wg > 1', 0) for w in WIDTHS)
  print(f'  reduced_density steps with chunks_per_wg > 1, both widths together: {both}')
  assert both >= 1
  ratios = {}
  for (mode, seed, w), c in checks().items():
    if w == bw:
      for k, v in c.ratios.items():
        ratios[k] = max(ratios.get(k, 0.0), v)
  print('  largest error as a fraction of its derived bound: ' + ', '.join(f'{k} {v:.3g}' for k, v in sorted(ratios.items())))


def test_the_long_running_tool_ends_at_the_first_failure(monkeypatch, capsys):
  """tools/fuzz_programs.py on a stand-in that breaks its first barrier: one FAIL line, the summary, exit status 1 -- and no
  program started behind the one that failed (on the GPU a failure may be a fault)"""
  import json
  import fuzz_programs                                       # (tools/ is on sys.path: tests/program_model.py put it there)
  def make(nloc, w, kind):
    return QueueBehindBarrier(nloc, w, kind)
  monkeypatch.setattr('sys.argv', ['fuzz_programs.py', '3600', '1', 'all'])
  with pytest.raises(SystemExit) as e:
    fuzz_programs.main(make_state=make)
  assert e.value.code == 1
  lines = [json.loads(x) for x in capsys.readouterr().out.splitlines() if x.startswith('{')]
  assert len(lines) == 2 and lines[0]['FAIL'] == 1 and lines[0]['step_index'] is not None
  first = (lines[0]['mode'], lines[0]['bw'])
  order = [(md, w) for md in ('own', 'shard', 'attached', 'mapped') for w in (128, 64)]
  assert lines[1] == dict(lines[1], programs=order.index(first) + 1, failures=1, next_seed=2, mode='all')
