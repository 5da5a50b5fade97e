"""TEST-ONLY: random PROGRAMS over the whole device API (include/qcc_hip.h) and a NumPy model of them.  Host only.

  gen_program(seed, bw, mode)   a deterministic list of steps (dicts) that interleaves queued gate bursts, barrier mutators,
                                readers, handle steps, two-state steps and layout steps on a pool of handles
  ModelState                    every step in plain NumPy on one complex128 vector per handle, in LOGICAL order
  run_program(program, make_state, check)   drives any object with qcc_amd.device.DeviceState's interface through a program
                                and compares every step with the model; the only place that compares
  NumpyDevice                   a stand-in with DeviceState's interface (physical array + bit map + queue per handle) that
                                re-lays its local bits out at a flush of >= 14 local bits, as relayout sweeps do

A handle of a SHARD (qh_set_shard) is modelled as a vector of the GLOBAL size that is zero outside the indices the shard
holds: gates on local bits, controls / diagonals / selectors / z masks on held bits and every per-shard reader then are the
plain operation on that vector.  Bits are LOGICAL everywhere; a step never names a physical position (remap_swap names the
two logical bits whose positions are exchanged, the runner looks the positions up).

References are imported, not copied: tests/oracle_lib (gates), fake_device.np_marginal / np_keep, resize_util.np_extend /
np_release, select_util.np_select / np_topk / fma_probs, test_dense_cpu.dense_reference, test_mux_cpu.mux_reference_fast /
diag_reference, test_expect_cpu.np_expect, test_perm_cpu.perm_reference (and the tile rule of qh_perm_plan it states),
pauli_util.np_pauli_sum and pauli_util.bound (qh_apply_pauli_sum and its derived error bound),
pauli_product_util.np_pauli_product, bound and greedy_runs (qh_apply_pauli_product, its derived bound and its run rule),
shard_util.check_exact_cdf (the inverse CDF of qh_sample in physical order), density_util.np_reduced_density and
density_util.tolerance (qh_reduced_density and its derived bound), zpoly_util.np_apply, np_moments, apply_bound and moment_bound
(qh_apply_zpoly / qh_expect_zpoly and their derived bounds)."""
import os
import sys

import numpy as np

from qcc_amd import native
from tests import density_util as du, oracle_lib, pauli_product_util as ppu, pauli_util, shard_util, zpoly_util as zu
from tests.fake_device import np_keep, np_marginal
from tests.resize_util import np_extend, np_release
from tests.select_util import fma_probs, np_select, np_topk
from tests.test_dense_cpu import dense_reference
from tests.test_expect_cpu import np_expect
from tests.test_mux_cpu import diag_reference, mux_reference_fast
from tests.test_perm_cpu import LDS_BUDGET, _expected_tile, perm_reference

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))
import fuzz_parity  # noqa: E402  (the gate pools and the control-density logic of the gate fuzzer)

NLOCS = (3, 6, 8, 9, 12, 14, 15, 16, 17)
SWEEPS_FROM = 8               # fused sweeps (and with them relayout) exist from 8 local bits on (sweep_supported)
PERMUTED_FROM = 14            # tests/test_gpu_shard_readout.py: relayout sweeps permute local bits from here on
MAX_BITS = 20                 # the largest state of a program: 2^20 amplitudes
MAX_LIVE = 4
LINEAR, TILES, GATHER = native.QH_INNER_LINEAR, native.QH_INNER_TILES, native.QH_INNER_GATHER

BARRIERS = ('matrix', 'mux', 'diag', 'perm', 'scale', 'project_bit', 'project_bits')
READERS = ('norm2', 'prob_bit', 'marginal', 'sample', 'expect', 'argmax', 'amplitude', 'amplitudes', 'select', 'topk', 'reduced_density',
           'expect_zpoly')
HANDLE_STEPS = ('clone', 'copy', 'extend', 'release', 'close')
TWO_STATE = ('inner', 'axpby')
# pauli_sum reads one handle and replaces another whole (or makes a new one); pauli_product works in place, in runs of kernels;
# zpoly works in place in one kernel
OPERATOR_STEPS = ('pauli_sum', 'pauli_product', 'zpoly')
LAYOUT_STEPS = ('flush', 'set_relayout', 'remap')
KINDS = ('gates',) + BARRIERS + READERS + HANDLE_STEPS + TWO_STATE + OPERATOR_STEPS + LAYOUT_STEPS + ('refused',)


# the fixed programs of the suite (tests/test_program_fuzz_cpu.py on NumpyDevice, tests/test_gpu_program_fuzz.py on the GPU),
# each at both widths; the coverage table of the CPU test is what this seed list was chosen by
# (re-chosen when 'perm' and then 'pauli_sum' became kinds: one stream draws the kinds, so a new kind changes every program of
# every seed; no seed has left the list.  With 'pauli_product': own 44, 82, shard 25, 32, 64, attached 176 and mapped 56, 73 joined, each for
# a condition of the coverage tables that the other programs no longer or never met -- HISTORY.md T4 names them.  With 'reduced_density',
# 'expect_zpoly' and 'zpoly': own 86, 138, shard 8, 67 and attached 29, 99, 235, 278 joined, likewise -- HISTORY.md T5 names them)
FIXED = [('own', seed) for seed in list(range(21)) + [42, 44, 48, 60, 82, 86, 88, 92, 138, 139]] + \
        [('shard', seed) for seed in list(range(6)) + [8, 15, 22, 24, 25, 32, 34, 54, 64, 67]] + \
        [('attached', seed) for seed in list(range(4)) + [5, 7, 11, 29, 99, 176, 235, 278]] + [('mapped', seed) for seed in list(range(4)) + [15, 42, 56, 73]]
# planner variants of tests/test_gpu_fuzz.py, each on 'own' programs whose first handle is large enough for sweeps
ENV_VARIANTS = [{'QH_RELAYOUT': '0'}, {'QH_WAVE_BITS': '2', 'QH_LANE_VALU': '2'}, {'QH_SEATS': '2', 'QH_WAVE_BITS': '1'}]


# ---- tolerances: the constants of the operations' own GPU test files ------------------------------------------------------
def amp_tol(bw):
  """amplitudes: _amp_tol of tests/test_gpu_shard_readout.py"""
  return 1e-12 if bw == 128 else 5e-6


def close(got, want, bw):
  """sums of probabilities: _close of tests/test_gpu_shard_readout.py; returns the message of a miss or None"""
  got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
  err = float(np.max(np.abs(got - want))) if got.size else 0.0
  lim = 1e-12 if bw == 128 else 1e-6 * max(float(np.max(want)) if want.size else 0.0, 1e-30) + 1e-9
  return None if err <= lim else f'off by {err:.3e} (limit {lim:.3e})'


# ---- register permutations: which path a register of k bits can take (plan_perm_tiles of perm_plan.h) -------------------------
# The tile is the register's positions plus the positions inside a 128-byte line (3 at complex128, 4 at complex64), padded to
# min(10, nloc) bits; it goes through LDS while amp_bytes << tile_bits <= 128 KiB, i.e. up to 13 (14) tile bits.  So k <= 10 is
# always LDS, k >= 14 (15) always gather, and in between the path depends on how many line positions hold register bits.
PERM_MAX_BITS = native.QH_PERM_MAX_BITS
PERM_BANDS = ('small', 'lds_edge', 'layout', 'gather')


def perm_sure_gather(bw):
  """the smallest k that takes the gather path on every layout"""
  return 14 if bw == 128 else 15


def perm_band(k, bw):
  return 'small' if k <= 6 else 'lds_edge' if k <= 10 else 'layout' if k < perm_sure_gather(bw) else 'gather'


def perm_tiles(nloc, bw, bm, shard, bits, ctl_mask):
  """path, tile_bits, ctl_met and reg_pos of qh_perm_plan from a bit map, by the tile rule tests/test_perm_cpu.py states"""
  reg_pos = [bm[b] for b in bits]
  tile_bits = bin(_expected_tile(nloc, bw, reg_pos)).count('1')
  path = native.QH_PERM_LDS if ((16 if bw == 128 else 8) << tile_bits) <= LDS_BUDGET else native.QH_PERM_GATHER
  held = sum(1 << (bm[b] - nloc) for b in range(len(bm)) if (ctl_mask >> b) & 1 and bm[b] >= nloc)
  return {'path': path, 'tile_bits': tile_bits, 'ctl_met': int((shard & held) == held), 'k': len(bits), 'reg_pos': reg_pos}


# ---- Pauli-sum operators: what qh_pauli_sum_plan must say of a bit map (plan_pauli / pauli_cut of the engine) ---------------------
PAULI_BATCH = native.QH_PAULI_SUM_BATCH
PAULI_FEW = 4                 # kPauliSmallT of pauli_plan.h: a batch of up to 4 terms takes the instantiation with 4 term slots
PAULI_CHUNK_BITS = 11         # kPauliChunkBits: the main shape needs nloc - amp_bits >= 11, smaller states take k_pauli_small


def _popcount(v):
  return bin(int(v)).count('1')


def pauli_main_shape(nloc, bw):
  return nloc - (0 if bw == 128 else 1) >= PAULI_CHUNK_BITS


def pauli_plan_rule(nloc, bm, shard, xmasks, zmasks):
  """(terms, batches) of qh_pauli_sum_plan from a bit map, as include/qcc_hip.h states it: px / pz are the logical masks
  mapped through the map and cut to the local bits, neg is the parity of shard & the held z bits, ny = popcount(x & z) & 3;
  the terms are stably sorted by px and cut every 16; a batch counts its distinct x masks and asks for that many + 1 streams,
  + 1 more behind the first batch"""
  def local(mask):
    return sum(1 << bm[b] for b in range(len(bm)) if (mask >> b) & 1 and bm[b] < nloc)
  def held(mask):
    return sum(1 << (bm[b] - nloc) for b in range(len(bm)) if (mask >> b) & 1 and bm[b] >= nloc)
  terms = [{'index': t, 'px': local(x), 'pz': local(z), 'neg': _popcount(shard & held(z)) & 1, 'ny': _popcount(int(x) & int(z)) & 3}
           for t, (x, z) in enumerate(zip(xmasks, zmasks))]
  terms.sort(key=lambda t: t['px'])                         # (list.sort is stable)
  batches = []
  for first in range(0, len(terms), PAULI_BATCH):
    part = terms[first:first + PAULI_BATCH]
    groups = 1 + sum(part[k]['px'] != part[k - 1]['px'] for k in range(1, len(part)))
    batches.append({'first': first, 'count': len(part), 'ngroups': groups, 'streams': groups + 1 + (first > 0)})
  return terms, batches


def pauli_coef(c, ny, neg):
  """c' = c (-i)^ny (shard sign), by swaps and negations only (pauli_coef of pauli_plan.h)"""
  re, im = complex(c).real, complex(c).imag
  for _ in range(ny & 3):
    re, im = im, -re
  return complex(-re, -im) if neg else complex(re, im)


def pauli_unit(c):
  """k with c == i^k exactly, or None"""
  return {(1.0, 0.0): 0, (0.0, 1.0): 1, (-1.0, 0.0): 2, (0.0, -1.0): 3}.get((complex(c).real, complex(c).imag))


def pauli_rotated(vec, n, x, z, k):
  """i^k (-1)^popcount(i & z) vec[i ^ x] by negations and swaps of the stored components alone: the bits a batch of one unit
  term stores (k = 0 and z = 0: the source's bits; a zero that is negated becomes a negative zero)"""
  idx = np.arange(1 << n, dtype=np.uint64)
  p = np.asarray(vec, dtype=np.complex128)[(idx ^ np.uint64(x)).astype(np.int64)]
  re, im = p.real.copy(), p.imag.copy()
  if k & 1:
    re, im = -im, re
  neg = (pauli_util.parity(idx, z) == 1) ^ bool(k & 2)
  out = np.empty(1 << n, dtype=np.complex128)
  out.real, out.imag = np.where(neg, -re, re), np.where(neg, -im, im)
  return out


# ---- Pauli products: what qh_pauli_product_plan must say of a bit map (plan_pauli_product / pauli_product_cut of the engine) ------
PAULI_PRODUCT_BATCH = native.QH_PAULI_PRODUCT_BATCH
PAULI_PRODUCT_FEW = 4         # kPauliProdSmallT of pauli_product_plan.h: a run of up to 4 terms takes the instantiation with 4 slots
PAULI_LANE_PIVOT_MAX = 2      # kPauliLanePivotMax: a PAIR run whose pivot is an item bit <= 2 (inside a 128-byte line) walks items
PAULI_RUN_KINDS = (native.QH_PAULI_RUN_DIAG, native.QH_PAULI_RUN_PAIR, native.QH_PAULI_RUN_HALF)


def pauli_product_main_shape(nloc, bw):
  """pauli_product_main_shape: a whole chunk of PAIRS; smaller states take k_pauli_product_small"""
  return nloc - (0 if bw == 128 else 1) - 1 >= PAULI_CHUNK_BITS


def pauli_product_rule(nloc, bw, bm, shard, xmasks, zmasks, batch=PAULI_PRODUCT_BATCH):
  """(terms, runs) of qh_pauli_product_plan from a bit map, as include/qcc_hip.h states it: the terms of pauli_plan_rule in the
  CALLER'S order, cut into runs by the greedy rule (pauli_product_util.greedy_runs)"""
  def local(mask):
    return sum(1 << bm[b] for b in range(len(bm)) if (mask >> b) & 1 and bm[b] < nloc)
  def held(mask):
    return sum(1 << (bm[b] - nloc) for b in range(len(bm)) if (mask >> b) & 1 and bm[b] >= nloc)
  terms = [{'index': t, 'px': local(x), 'pz': local(z), 'neg': _popcount(shard & held(z)) & 1, 'ny': _popcount(int(x) & int(z)) & 3}
           for t, (x, z) in enumerate(zip(xmasks, zmasks))]
  runs = [{'first': f, 'count': c, 'px': X, 'kind': k}
          for f, c, X, k in ppu.greedy_runs([t['px'] for t in terms], batch, 0 if bw == 128 else 1, PAULI_RUN_KINDS)]
  return terms, runs


def pauli_product_walk(nloc, bw, run):
  """how launch_pauli_run walks a run: 'small' below the main shape; on it 'diag' and 'half' walk items, a PAIR run walks items
  too ('lane': the partner comes by a lane exchange) where the top bit of its PHYSICAL X >> amp_bits is an item bit <=
  kPauliLanePivotMax (pauli_pair_in_wave), and pair numbers otherwise ('pair').  The plan does not say which: it says PAIR."""
  ab = 0 if bw == 128 else 1
  if not pauli_product_main_shape(nloc, bw):
    return 'small'
  if run['kind'] != native.QH_PAULI_RUN_PAIR:
    return 'diag' if run['kind'] == native.QH_PAULI_RUN_DIAG else 'half'
  xi = run['px'] >> ab
  return 'lane' if xi and xi.bit_length() - 1 <= PAULI_LANE_PIVOT_MAX else 'pair'


# ---- reduced density matrices: what qh_density_plan must say of a bit map (plan_density of density_plan.h) -----------------------
DENSITY_MAX_BITS = native.QH_DENSITY_MAX_BITS
DENSITY_TILE_BITS = 6         # kDensityTileBits: a tile has at most 64 rows; k = 7, 8 are cut into 2, 4 blocks of 64 rows
DENSITY_LDS_BITS = 11         # kDensityLdsBits: amplitudes of (tiles x chunk) a workgroup keeps in LDS
DENSITY_GATHER_BELOW = 8      # kDensityGatherBelow: fewer local bits take QH_DENSITY_GATHER
DENSITY_MAX_WGS, DENSITY_SLAB_BYTES = 2048, 32 << 20
DENSITY_TABLES = ('row_pos', 'row_bit', 'col_pos', 'rest_pos')


def density_rule(nloc, bm, bits):
  """qh_density_plan from a bit map, as include/qcc_hip.h states it: the register's positions ascending (row_pos) and which
  listed bit each holds (row_bit); the environment's positions ascending, the lowest chunk_bits of them the columns of a chunk,
  the others the chunk number; min(k, 6) row bits per tile, nb (nb + 1) / 2 block pairs of nb = 2^(k - tile_bits) row blocks;
  the workgroups per pair a power of two bounded by the chunks, by 2048 workgroups and by 32 MiB of slab in all"""
  k, pos = len(bits), [bm[b] for b in bits]
  rows = sorted(pos)
  env = [p for p in range(nloc) if p not in pos]
  out = {'k': k, 'row_pos': rows, 'row_bit': [pos.index(p) for p in rows]}
  if nloc < DENSITY_GATHER_BELOW:
    out.update(path=native.QH_DENSITY_GATHER, tile_bits=k, chunk_bits=0, nrest=len(env), block_pairs=1, wg_per_pair=1,
               chunks_per_wg=1 << len(env), slab_bytes=0, amps_swept=1 << nloc, col_pos=[], rest_pos=env)
    return out
  kt = min(k, DENSITY_TILE_BITS)
  nb = 1 << (k - kt)
  pairs = nb * (nb + 1) // 2
  cb = min(DENSITY_LDS_BITS - kt - (1 if nb > 1 else 0), len(env))
  nchunks, row_bytes = 1 << (len(env) - cb), 16 << (2 * kt)
  cap = min(DENSITY_SLAB_BYTES // row_bytes, DENSITY_MAX_WGS) // pairs
  wg = 1
  while wg * 2 <= cap and wg * 2 <= nchunks:
    wg *= 2
  out.update(path=native.QH_DENSITY_TILES, tile_bits=kt, chunk_bits=cb, nrest=len(env) - cb, block_pairs=pairs, wg_per_pair=wg,
             chunks_per_wg=nchunks // wg, slab_bytes=row_bytes * wg * pairs, amps_swept=1 << (nloc + k - kt), col_pos=env[:cb], rest_pos=env[cb:])
  return out


def density_plan_view(plan):
  """a plan of qh_density_plan (QhDensityTiles.as_dict) with its four position tables cut to their lengths"""
  out = dict(plan)
  for name, count in zip(DENSITY_TABLES, (plan['k'], plan['k'], plan['chunk_bits'], plan['nrest'])):
    out[name] = [int(x) for x in plan[name][:count]]
  return out


def local_view(vec, n, held):
  """a shard's amplitudes in the logical order of its LOCAL bits (held bits dropped from the index), and the number every local
  logical bit has there: what density_util.np_reduced_density takes for a shard"""
  loc = [b for b in range(n) if b not in held]
  return np.asarray(vec)[mine_of(n, held).astype(np.int64)], {b: j for j, b in enumerate(loc)}


# ---- Z-polynomials: what qh_zpoly_plan must say of a bit map (zpoly_plan of zpoly_plan.h) ----------------------------------------
ZPOLY_MAX_TERMS = native.QH_ZPOLY_MAX_TERMS
ZPOLY_LANES = 64              # the kernels deal a segment's terms to 64 lanes before an xor tree
ZPOLY_BLOCKS = 4096           # kPauliBlocks: blocks at most, each a contiguous run of chunks
ZPOLY_MODEL_BUDGET = 1 << 25  # nterms * 2^nloc of a drawn step: the NumPy model evaluates f term by term
ZPOLY_CLASSES = {native.QH_ZPOLY_CONST: 'CONST', native.QH_ZPOLY_HIGH: 'HIGH', native.QH_ZPOLY_LOW: 'LOW', native.QH_ZPOLY_STRADDLE: 'STRADDLE'}
ZPOLY_GROUP_KINDS = ('thread-only', 'register-index/half-only', 'mixed')


def zpoly_main_shape(nloc, bw):
  return pauli_main_shape(nloc, bw)                          # whole chunks of 2^11 items; smaller states take k_zpoly_small


def zpoly_rule(nloc, bw, bm, shard, weights, zmasks):
  """qh_zpoly_plan from a bit map, as include/qcc_hip.h states it: per term the physical local mask, the weight negated where
  the parity of shard & (the held z bits) is odd, and the class by where the mask lies about low_bits (11 item bits + the
  half bit at complex64 on the main kernel, every local bit on the small one); the distinct low masks of the straddling terms
  in order of first appearance; the grid of pauli_grid"""
  ab = 0 if bw == 128 else 1
  main = zpoly_main_shape(nloc, bw)
  low_bits = PAULI_CHUNK_BITS + ab if main else nloc
  pz, w, cls, groups = [], [], [], []
  for wt, z in zip(weights, zmasks):
    local = sum(1 << bm[b] for b in range(len(bm)) if (int(z) >> b) & 1 and bm[b] < nloc)
    held = sum(1 << (bm[b] - nloc) for b in range(len(bm)) if (int(z) >> b) & 1 and bm[b] >= nloc)
    lo, hi = local & ((1 << low_bits) - 1), local >> low_bits
    c = native.QH_ZPOLY_CONST if local == 0 else native.QH_ZPOLY_STRADDLE if lo and hi else native.QH_ZPOLY_HIGH if hi else native.QH_ZPOLY_LOW
    pz.append(local)
    w.append(-float(wt) if _popcount(shard & held) & 1 else float(wt))
    cls.append(c)
    if c == native.QH_ZPOLY_STRADDLE and lo not in groups:
      groups.append(lo)
  nchunks = 1 << (nloc - low_bits) if main else 0
  nblk = min(nchunks, ZPOLY_BLOCKS) if main else ((1 << nloc) + 255) // 256
  return {'nterms': len(pz), 'nconst': cls.count(native.QH_ZPOLY_CONST), 'nhigh': cls.count(native.QH_ZPOLY_HIGH),
          'nlow': cls.count(native.QH_ZPOLY_LOW), 'nstraddle': cls.count(native.QH_ZPOLY_STRADDLE), 'ngroups': len(groups), 'nblk': nblk,
          'kernel': native.QH_ZPOLY_KERNEL_MAIN if main else native.QH_ZPOLY_KERNEL_SMALL, 'low_bits': low_bits, 'cpb': nchunks // nblk if main else 0,
          'group_mask': groups, 'pz': pz, 'w': w, 'cls': cls}


def zpoly_group_kind(low_mask, bw):
  """where a group's low mask lies: on thread bits only (item bits 0-7), on register-index / half bits only, or on both"""
  thread = 255 << (0 if bw == 128 else 1)
  return ZPOLY_GROUP_KINDS[0 if not low_mask & ~thread else 1 if not low_mask & thread else 2]


def zpoly_segments(plan):
  """the term counts of the main kernel's segments: segment 0 the CONST and HIGH terms, then one per group"""
  lowm = (1 << plan['low_bits']) - 1
  seg = [plan['nconst'] + plan['nhigh']] + [0] * plan['ngroups']
  for z, c in zip(plan['pz'], plan['cls']):
    if c == native.QH_ZPOLY_STRADDLE:
      seg[1 + plan['group_mask'].index(z & lowm)] += 1
  return seg


_ZPOLY_F = []                 # the last few (key, f): a step's f is asked by the generator's trial, the models and the runner


def zpoly_f(n, held, weights, zmasks):
  """zpoly_util.np_f at the global logical indices the shard holds (ascending), kept for the next caller that asks the same"""
  key = (n, tuple(sorted(held.items())), np.asarray(weights, dtype=np.float64).tobytes(), tuple(int(z) for z in zmasks))
  for k, f in _ZPOLY_F:
    if k == key:
      return f
  f = zu.np_f(mine_of(n, held), weights, zmasks)
  f.setflags(write=False)
  _ZPOLY_F.insert(0, (key, f))
  del _ZPOLY_F[3:]
  return f


def zpoly_c_kind(c):
  c = complex(c)
  return 'zero' if c == 0 else 're0' if c.real == 0 else 'im0' if c.imag == 0 else 'general'


TOL = 1e-12                   # TOL of tests/test_gpu_inner.py: readers that accumulate in double from the stored amplitudes
CHAIN_TOL_128 = 2e-11         # tools/fuzz_parity.py, complex128


_ORACLE = []


def _oracle():
  if not _ORACLE:
    _ORACLE.append(oracle_lib.load())
  return _ORACLE[0]


def apply_gate(vec, n, ctl_mask, tgt, g):
  """one qh_apply_bits gate on a vector of 2^n amplitudes in logical order, in place, in the vector's own precision"""
  orc = _oracle()
  ctl = [b for b in range(n) if (ctl_mask >> b) & 1]
  gq = np.asarray(g, dtype=vec.dtype).reshape(4)
  if not ctl:
    orc.apply1(vec, gq, n, n - 1 - tgt)
  elif len(ctl) == 1:
    orc.applyc(vec, gq, n, n - 1 - ctl[0], n - 1 - tgt)
  else:                                           # (as tools/fuzz_parity.py: the gate where every control is 1)
    idx = np.arange(1 << n, dtype=np.uint64)
    on = (idx & np.uint64(ctl_mask)) == np.uint64(ctl_mask)
    tmp = vec.copy()
    orc.apply1(tmp, gq, n, n - 1 - tgt)
    vec[on] = tmp[on]


def swap_logical_bits(vec, n, a, b):
  if a == b:
    return vec.copy()
  return np.ascontiguousarray(np.swapaxes(vec.reshape([2] * n), n - 1 - a, n - 1 - b)).reshape(-1)


def held_mask_value(held):
  return sum(1 << b for b in held), sum(v << b for b, v in held.items())


def mine_of(n, held):
  """the global logical indices a shard holds, ascending"""
  mask, value = held_mask_value(held)
  return np.flatnonzero(np_keep(1 << n, mask, value)).astype(np.uint64)


def axpby_ref(d, alpha, s, beta):
  """alpha * d + beta * s as qh_axpby defines it: a coefficient that is exactly 0 leaves its state unread"""
  alpha, beta = complex(alpha), complex(beta)
  out = np.zeros_like(d)
  if alpha != 0:
    out = out + alpha * d
  if beta != 0:
    out = out + beta * s
  return out


def init_vector(s):
  """the GLOBAL state an 'init' step describes, complex128, logical order"""
  n = s['nloc'] + s['g']
  if s['how'] == 'basis':
    v = np.zeros(1 << n, dtype=np.complex128)
    v[s['index']] = 1
  elif s['how'] == 'product':
    v = np.ones(1, dtype=np.complex128)
    for k, x in s['factors']:
      if isinstance(x, (int, np.integer)):
        t = np.zeros(1 << k, dtype=np.complex128)
        t[int(x)] = 1
      else:
        t = np.asarray(x, dtype=np.complex128)
      v = np.kron(v, t)
  else:
    rng = np.random.default_rng(s['seed'])
    v = rng.standard_normal(1 << n) + 1j * rng.standard_normal(1 << n)
    v /= np.linalg.norm(v)
  return v


def init_bitmap(s):
  """physical position of every logical bit after the initial remap_swaps of a shard program"""
  bm = list(range(s['nloc'] + s['g']))
  for a, b in s['swaps']:
    la, lb = bm.index(a), bm.index(b)
    bm[la], bm[lb] = bm[lb], bm[la]
  return bm


class ModelState:
  """Every live handle as one vector in logical order.  A burst of gates is applied at once but remembered as queued: the
  vector BEFORE the burst is kept, so that a step that DROPS the queue (copy_from on the destination) finds it."""

  def __init__(self, dtype=np.complex128):
    self.dtype = dtype
    self.v, self.base, self.q, self.n, self.held = {}, {}, {}, {}, {}
    # relayout mode as include/qcc_hip.h describes it: -1 undecided (decided by the first fused flush), 0 off, 1 on; and
    # whether the handle owns HBM memory (attached and host-mapped ones do not: they never re-lay out)
    self.mode, self.owns = {}, {}
    # the bit map a handle would have if no relayout sweep ever moved it: what the generator aims physical positions by (the
    # runner reads the real one; nothing is compared with this)
    self.bm = {}

  def _rnd(self, x):
    return np.ascontiguousarray(x, dtype=np.complex128).astype(self.dtype) if self.dtype != np.complex128 else np.ascontiguousarray(x, dtype=np.complex128)

  def wide(self, h):
    return self.v[h].astype(np.complex128)

  def put(self, h, vec, n=None, held=None):
    self.v[h] = self.base[h] = self._rnd(vec)
    self.q[h] = 0
    if n is not None:
      self.n[h], self.held[h] = n, dict(held)
      self.mode[h], self.owns[h] = -1, True                # a new handle: undecided, memory of its own

  def eligible(self, h):
    """relayout_eligible of the engine: QH_RELAYOUT (read when asked), memory of its own, a size that has sweeps"""
    return bool(self.owns[h] and int(os.environ.get('QH_RELAYOUT', '1')) != 0 and self.nloc(h) >= SWEEPS_FROM)

  def wanted(self, h):
    """would a flush of this handle re-lay it out (relayout_wanted of the engine)"""
    return self.eligible(h) if self.mode[h] < 0 else self.mode[h] == 1

  def run(self, h):
    if self.q[h] and self.mode[h] < 0 and self.nloc(h) >= SWEEPS_FROM:
      self.mode[h] = int(self.eligible(h))                 # the first fused flush decides
    self.base[h] = self.v[h]
    self.q[h] = 0

  def queued(self, h, ahead, count):
    """a burst of `count` gates was queued: `ahead` is the state with it applied, the state before it is kept"""
    if self.q[h] == 0:
      self.base[h] = self.v[h]
    self.v[h] = ahead
    self.q[h] += count

  def drop(self, h):
    self.v[h] = self.base[h]
    self.q[h] = 0

  def nloc(self, h):
    return self.n[h] - len(self.held[h])

  def local_bits(self, h):
    return [b for b in range(self.n[h]) if b not in self.held[h]]

  def norm(self, h):
    w = self.wide(h)
    return float(np.vdot(w, w).real)

  def step(self, s):
    return getattr(self, '_' + s['op'])(s)

  # -- start ------------------------------------------------------------------------------------------------------------------
  def _init(self, s):
    n, nloc = s['nloc'] + s['g'], s['nloc']
    psi, bm = init_vector(s), init_bitmap(s)
    for shard, h in enumerate(s['slots']):
      held = {b: (shard >> (bm[b] - nloc)) & 1 for b in range(n) if bm[b] >= nloc}
      mask, value = held_mask_value(held)
      self.put(h, np.where(np_keep(1 << n, mask, value), psi, 0), n, held)
      self.bm[h] = list(bm)
      if s['mode'] in ('attached', 'mapped'):
        self.mode[h], self.owns[h] = 0, False

  # -- gates --------------------------------------------------------------------------------------------------------------------
  def _gates(self, s):
    h = s['h']
    ahead = self.v[h].copy()
    for cm, t, g in s['gates']:
      apply_gate(ahead, self.n[h], cm, t, g)
    self.queued(h, ahead, len(s['gates']))

  def _mut(self, h, fn):
    self.run(h)
    self.put(h, fn(self.wide(h)))

  def _matrix(self, s):
    self._mut(s['h'], lambda v: dense_reference(v, self.n[s['h']], s['m'], s['bits'], s['ctl']))

  def _mux(self, s):
    self._mut(s['h'], lambda v: mux_reference_fast(v, self.n[s['h']], s['gates'], s['sel'], s['tgt']))

  def _diag(self, s):
    self._mut(s['h'], lambda v: diag_reference(v, self.n[s['h']], s['values'], s['bits']))

  def _perm(self, s):
    # (on the vector of the GLOBAL size with the full control mask: a shard's vector is zero wherever a held control is 0)
    self._mut(s['h'], lambda v: perm_reference(v, self.n[s['h']], s['table'], s['bits'], s['ctl']))

  def _scale(self, s):
    self._mut(s['h'], lambda v: v * complex(s['z']))

  def _project_bit(self, s):
    self._mut(s['h'], lambda v: np.where(np_keep(v.size, 1 << s['bit'], s['value'] << s['bit']), v, 0))

  def _project_bits(self, s):
    self._mut(s['h'], lambda v: np.where(np_keep(v.size, s['mask'], s['value']), v, 0))

  # -- readers ------------------------------------------------------------------------------------------------------------------
  def _norm2(self, s):
    self.run(s['h'])
    return self.norm(s['h'])

  def _prob_bit(self, s):
    self.run(s['h'])
    w = self.wide(s['h'])
    sel = np_keep(w.size, 1 << s['bit'], s['value'] << s['bit'])
    return float(np.vdot(w[sel], w[sel]).real)

  def _marginal(self, s):
    self.run(s['h'])
    return np_marginal(self.wide(s['h']), s['bits'])

  def _sample(self, s):
    self.run(s['h'])              # (the answer depends on the physical order: the runner checks it there)

  def _expect(self, s):
    self.run(s['h'])
    w = self.wide(s['h'])
    return np.array([np_expect(w, x, z) for x, z in zip(s['x'], s['z'])], dtype=np.float64)

  def _reduced_density(self, s):
    h = s['h']
    self.run(h)
    psi, number = local_view(self.wide(h), self.n[h], self.held[h])
    return du.np_reduced_density(psi, [number[b] for b in s['bits']])

  def _expect_zpoly(self, s):
    h = s['h']
    self.run(h)
    mine = mine_of(self.n[h], self.held[h]).astype(np.int64)
    return zu.np_moments(self.wide(h)[mine], s['w'], s['z'], f=zpoly_f(self.n[h], self.held[h], s['w'], s['z']))

  def _probs(self, h):
    mine = mine_of(self.n[h], self.held[h])
    a = self.wide(h)[mine.astype(np.int64)]
    return mine, a, fma_probs(a)

  def _argmax(self, s):
    self.run(s['h'])
    mine, _, p = self._probs(s['h'])
    k = int(np.argmax(p))
    return int(mine[k]), float(p[k])

  def _amplitude(self, s):
    self.run(s['h'])
    return complex(self.wide(s['h'])[s['index']])

  def _amplitudes(self, s):
    self.run(s['h'])
    return self.wide(s['h'])[np.asarray(s['indices'], dtype=np.int64)]

  def _select(self, s):
    self.run(s['h'])
    mine, a, p = self._probs(s['h'])
    idx, amp, w = np_select(a, s['threshold'], probs=p)
    return mine[idx.astype(np.int64)], amp, int(idx.size), w

  def _topk(self, s):
    self.run(s['h'])
    mine, a, p = self._probs(s['h'])
    idx, amp = np_topk(a, s['k'], probs=p)
    return mine[idx.astype(np.int64)], amp

  # -- handles ------------------------------------------------------------------------------------------------------------------
  def _clone(self, s):
    self.run(s['h'])
    self.put(s['new'], self.v[s['h']].copy(), self.n[s['h']], self.held[s['h']])
    self.bm[s['new']] = list(self.bm[s['h']])

  def _copy(self, s):
    self.run(s['src'])
    self.drop(s['h'])
    self.put(s['h'], self.v[s['src']].copy())
    self.bm[s['h']] = list(self.bm[s['src']])

  def _extend(self, s):
    h, k = s['h'], s['k']
    self.run(h)
    if s['amps'] is None:
      f = np.zeros(1 << k, dtype=np.complex128)
      f[s['basis']] = 1
    else:
      f = np.asarray(s['amps'], dtype=np.complex128)
    self.put(s['new'], np_extend(self.wide(h), f), self.n[h] + k, {b + k: v for b, v in self.held[h].items()})
    nl = self.nloc(h)
    self.bm[s['new']] = list(range(nl, nl + k)) + [p if p < nl else p + k for p in self.bm[h]]

  def _release(self, s):
    h, bits = s['h'], s['bits']
    self.run(h)
    small, kept, dropped = np_release(self.wide(h), bits, s['value'])
    held = {b - sum(1 for x in bits if x < b): v for b, v in self.held[h].items()}
    self.put(s['new'], small, self.n[h] - len(bits), held)
    gone = sorted(self.bm[h][b] for b in bits)
    self.bm[s['new']] = [p - sum(1 for r in gone if r < p) for b, p in enumerate(self.bm[h]) if b not in bits]
    return kept, dropped

  def _close(self, s):
    for d in (self.v, self.base, self.q, self.n, self.held, self.mode, self.owns, self.bm):
      d.pop(s['h'])

  # -- two states ----------------------------------------------------------------------------------------------------------------
  def _inner(self, s):
    self.run(s['h'])
    self.run(s['other'])
    return complex(np.vdot(self.wide(s['h']), self.wide(s['other'])))

  def _axpby(self, s):
    h = s['h']
    self.run(h)
    self.run(s['other'])
    self.put(h, axpby_ref(self.wide(h), s['alpha'], self.wide(s['other']), s['beta']))
    return self.norm(h)

  def _pauli_sum(self, s):
    """h is the SOURCE; the result goes into the existing handle `dst` (whose queue is dropped, never run, and whose relayout
    mode stays) or into the new slot `new`.  x masks are local, so partners stay on the shard and the vector of the global
    size needs nothing more: a held z bit is the plain sign of the global index."""
    src = s['h']
    self.run(src)
    out = pauli_util.np_pauli_sum(self.wide(src), s['coeffs'], s['x'], s['z'])
    if s['dst'] is None:
      d = s['new']
      self.put(d, out, self.n[src], self.held[src])
    else:
      d = s['dst']
      self.drop(d)
      self.put(d, out)
    self.bm[d] = list(self.bm[src])
    return self.norm(d)

  def _pauli_product(self, s):
    """prod_t (a_t I + b_t P_t) in place, term 0 first, on the handle as stored; x masks are local, so the vector of the global
    size needs nothing more (a held z bit is the plain sign of the global index)"""
    h = s['h']
    self.run(h)
    self.put(h, ppu.np_pauli_product(self.wide(h), s['a'], s['b'], s['x'], s['z']))
    return self.norm(h)

  def _zpoly(self, s):
    """a_i *= exp(c f(i)) in place on the amplitudes the shard holds, f over the GLOBAL logical index (a held z bit is the plain
    sign of that index); no terms or c == (0, 0): nothing is touched"""
    h = s['h']
    self.run(h)
    if len(s['z']) and complex(s['c']) != 0:
      mine = mine_of(self.n[h], self.held[h]).astype(np.int64)
      out = np.zeros(1 << self.n[h], dtype=np.complex128)
      out[mine] = zu.np_apply(self.wide(h)[mine], s['w'], s['z'], s['c'], f=zpoly_f(self.n[h], self.held[h], s['w'], s['z']))
      self.put(h, out)
    return self.norm(h)

  # -- layout -------------------------------------------------------------------------------------------------------------------
  def _flush(self, s):
    self.run(s['h'])

  def _set_relayout(self, s):
    h = s['h']
    if not s['on']:
      self.run(h)
      self.mode[h] = 0
    elif self.mode[h] != 1:
      self.mode[h] = int(self.eligible(h))
    return self.mode[h] == 1

  def _remap(self, s):
    h = s['h']
    self.run(h)
    self.put(h, swap_logical_bits(self.v[h], self.n[h], s['a'], s['b']))
    bm = self.bm[h]
    bm[s['a']], bm[s['b']] = bm[s['b']], bm[s['a']]

  def _refused(self, s):
    pass


# ---- the generator ------------------------------------------------------------------------------------------------------------
def _rand_op(rng, k, unitary):
  a = rng.standard_normal((1 << k, 1 << k)) + 1j * rng.standard_normal((1 << k, 1 << k))
  if unitary:
    a, _ = np.linalg.qr(a)
  else:
    a /= np.linalg.norm(a, 2)
  return a


def _rand_table(rng, k):
  t = rng.standard_normal(1 << k) + 1j * rng.standard_normal(1 << k)
  return t / np.linalg.norm(t)


def _rand_perm_table(rng, k):
  """mostly a random bijection; now and then one with structure (long cycles, fixed points) that a random one rarely has"""
  size, r = 1 << k, rng.random()
  x = np.arange(size, dtype=np.int64)
  if r < 0.7:
    t = rng.permutation(size)
  elif r < 0.8 or k == 1:
    t = (x + int(rng.integers(1, size))) % size             # x + c mod 2^k: one cycle of length 2^k / gcd
  elif r < 0.9:
    big = int(rng.integers(3, size + 1))                     # a * x mod N below N, the identity from N on
    a = int(rng.integers(1, big))
    while np.gcd(a, big) != 1:
      a = int(rng.integers(1, big))
    t = np.where(x < big, (a * x) % big, x)
  else:
    t = sum(((x >> j) & 1) << (k - 1 - j) for j in range(k))   # bit reversal: 2^ceil(k/2) fixed points, the rest in pairs
  return np.asarray(t, dtype=np.uint32)


class _Gen:
  def __init__(self, seed, bw, mode):
    self.rng = np.random.default_rng([int(seed), bw, ('own', 'attached', 'mapped', 'shard').index(mode)])
    self.bw, self.mode = bw, mode
    self.m = ModelState()
    self.steps = []
    self.next_slot = 0
    self.refused = 0
    self.pp_calls = self.pp_rejected = 0                     # k_pauli_product: draws made, draws that missed M <= 8 or the norm range
    self.zp_calls = self.zp_rejected = 0                     # k_zpoly: draws made, draws whose trial left the norm range

  def live(self):
    return sorted(self.m.v)

  def emit(self, s):
    self.steps.append(s)
    out = self.m.step(s)
    if s['op'] in ('gates', 'close', 'refused', 'init') or s.get('poison'):
      return out
    for h in [x for x in (s.get('new'), s.get('dst'), s.get('h')) if x is not None and x in self.m.v]:
      nv = self.m.norm(h)
      if self.m.q[h] == 0 and np.isfinite(nv) and nv > 0 and not 0.25 <= nv <= 4:      # norm control
        z = {'op': 'scale', 'h': h, 'z': complex(1 / np.sqrt(nv))}
        self.steps.append(z)
        self.m.step(z)
    return out

  def start(self):
    rng, mode = self.rng, self.mode
    g = int(rng.integers(1, 3)) if mode == 'shard' else 0
    pool = [x for x in NLOCS if (mode != 'mapped' or x <= 12) and x + g <= MAX_BITS - 1]
    nloc = int(pool[int(rng.integers(len(pool)))])
    n = nloc + g
    swaps = []
    if g and rng.random() < 0.5:                       # 'mid3' / 'midhalf' of tests/test_gpu_shard_readout.py
      swaps = [(nloc, 3 if nloc > 3 else 1)] if rng.random() < 0.5 else [(nloc + k, nloc // 2 - k) for k in range(g)]
    s = {'op': 'init', 'bw': self.bw, 'mode': mode, 'nloc': nloc, 'g': g, 'swaps': swaps, 'slots': list(range(1 << g))}
    how = ('basis', 'product', 'upload')[int(rng.integers(3))]
    s['how'] = how
    if how == 'basis':
      s['index'] = int(rng.integers(1 << n))
    elif how == 'product':
      fac, left = [], n
      while left:
        k = int(min(left, rng.integers(1, 5)))
        r = rng.random()
        fac.append((k, int(rng.integers(1 << k)) if r < 0.3 else (np.full(1 << k, 2.0 ** (-k / 2), dtype=np.complex128) if r < 0.6
                                                                else _rand_table(rng, k))))
        left -= k
      s['factors'] = fac
    else:
      s['seed'] = int(rng.integers(1 << 30))
    self.next_slot = 1 << g
    self.max_live = MAX_LIVE + (1 << g) - 1
    self.emit(s)

  def new_slot(self):
    self.next_slot += 1
    return self.next_slot - 1

  # -- one step of every kind; each returns False where the pool offers no valid instance -------------------------------------
  def pick(self, cond=lambda h: True):
    c = [h for h in self.live() if cond(h)]
    return c[int(self.rng.integers(len(c)))] if c else None

  def partner(self, h):
    """another live handle of the same shape and shard index"""
    m = self.m
    c = [x for x in self.live() if x != h and m.n[x] == m.n[h] and m.held[x] == m.held[h]]
    return c[int(self.rng.integers(len(c)))] if c else None

  def usable(self, h):
    nv = self.m.norm(h)
    return np.isfinite(nv) and nv > 0

  def k_gates(self):
    rng, m = self.rng, self.m
    h = self.pick(self.usable)
    if h is None:
      return False
    n, loc = m.n[h], m.local_bits(h)
    w = rng.dirichlet([1, 1, 1, 1])
    pctl, pmulti = rng.uniform(0, 0.8), rng.uniform(0, 0.3)
    focus = rng.random() < 0.4
    hot = rng.choice(n, size=max(2, n // 3), replace=False)
    bf, diag, real, gen = fuzz_parity.pools(rng)
    want = int(rng.integers(5, 41))
    trial = m.v[h].copy()
    out = []
    for _ in range(4 * want):
      if len(out) == want:
        break
      kind = int(rng.choice(4, p=w))
      pool = [bf, diag, real, gen][kind]
      g = np.asarray(pool[int(rng.integers(len(pool)))], dtype=np.complex128).reshape(4)
      t = int(rng.choice(hot)) if focus and rng.random() < 0.8 else int(rng.integers(n))
      if t not in loc and not (g[1] == 0 and g[2] == 0):
        t = loc[t % len(loc)]                              # dense gates stay on local bits
      cm = 0
      if rng.random() < pctl:
        k = 1 + (int(rng.integers(1, 4)) if rng.random() < pmulti else 0)
        others = [q for q in range(n) if q != t]
        for c in rng.choice(others, size=min(k, len(others)), replace=False):
          cm |= 1 << int(c)
      g2 = g.reshape(2, 2)
      if np.allclose(g2.conj().T @ g2, np.eye(2), rtol=0, atol=1e-12):
        apply_gate(trial, n, cm, t, g)                     # unitary: the norm stays where it is
      else:
        nxt = trial.copy()
        apply_gate(nxt, n, cm, t, g)
        nv = float(np.vdot(nxt, nxt).real)
        if not 0.25 <= nv <= 4:                            # a non-unitary operator that would take the norm out of range
          continue
        trial = nxt
      out.append((cm, t, g))
    if len(out) < 5:
      return False
    self.steps.append({'op': 'gates', 'h': h, 'gates': out})
    m.queued(h, trial, len(out))                           # (what ModelState._gates computes, without applying the burst twice)
    return True

  def k_matrix(self):
    rng, m = self.rng, self.m
    h = self.pick(self.usable)
    loc = m.local_bits(h) if h is not None else []
    if not loc:
      return False
    k = int(rng.integers(1, min(6, len(loc)) + 1))
    bits = [int(b) for b in rng.choice(loc, size=k, replace=False)]
    ctl = 0
    others = [b for b in range(m.n[h]) if b not in bits]
    if others and rng.random() < 0.5:
      for c in rng.choice(others, size=min(len(others), int(rng.integers(1, 4))), replace=False):
        ctl |= 1 << int(c)
    self.emit({'op': 'matrix', 'h': h, 'bits': bits, 'ctl': ctl, 'm': _rand_op(rng, k, rng.random() < 0.7)})
    return True

  def k_mux(self):
    rng, m = self.rng, self.m
    h = self.pick(self.usable)
    if h is None:
      return False
    loc, n = m.local_bits(h), m.n[h]
    tgt = int(loc[int(rng.integers(len(loc)))])
    k = int(rng.integers(0, min(10, len(loc) - 1) + 1))
    sel = [int(b) for b in rng.choice([b for b in range(n) if b != tgt], size=k, replace=False)]
    gs = np.stack([_rand_op(rng, 1, rng.random() < 0.8) for _ in range(1 << k)])
    self.emit({'op': 'mux', 'h': h, 'sel': sel, 'tgt': tgt, 'gates': gs})
    return True

  def k_diag(self):
    rng, m = self.rng, self.m
    h = self.pick(self.usable)
    if h is None:
      return False
    n = m.n[h]
    k = int(rng.integers(0, min(12, m.nloc(h)) + 1))
    bits = [int(b) for b in rng.choice(n, size=k, replace=False)]
    vals = np.exp(1j * rng.uniform(0, 6.28, 1 << k)) * (rng.uniform(0.8, 1.25, 1 << k) if rng.random() < 0.3 else 1.0)
    self.emit({'op': 'diag', 'h': h, 'bits': bits, 'values': vals})
    return True

  def k_perm(self):
    rng, m = self.rng, self.m
    h = self.pick(self.usable)
    if h is None:
      return False
    loc, n = m.local_bits(h), m.n[h]
    kmax, sure = min(PERM_MAX_BITS, len(loc)), perm_sure_gather(self.bw)
    # the bands of perm_band, with equal weight where the handle is large enough for them; and the register that is the whole
    # shard (one tile, no bit left to number the tiles)
    bands = [(lo, min(hi, kmax)) for lo, hi in ((1, 6), (7, 10), (11, sure - 1), (sure, PERM_MAX_BITS)) if lo <= kmax]
    if len(loc) <= PERM_MAX_BITS and rng.random() < 0.15:
      k = len(loc)
    else:
      lo, hi = bands[int(rng.integers(len(bands)))]
      k = int(rng.integers(lo, hi + 1))
    bits = [int(b) for b in rng.choice(loc, size=k, replace=False)]
    ctl = 0
    others = [b for b in range(n) if b not in bits]          # (held bits included: dropped where met, a no-op where not)
    if others and rng.random() < 0.5:
      for c in rng.choice(others, size=min(len(others), int(rng.integers(1, 4))), replace=False):
        ctl |= 1 << int(c)
    held = sorted(m.held[h])
    if held and rng.random() < 0.4:
      ctl |= 1 << held[int(rng.integers(len(held)))]
    self.emit({'op': 'perm', 'h': h, 'bits': bits, 'ctl': ctl, 'table': _rand_perm_table(rng, k)})
    return True

  def k_scale(self):
    h = self.pick(self.usable)
    if h is None:
      return False
    self.emit({'op': 'scale', 'h': h, 'z': complex(self.rng.uniform(0.8, 1.25) * np.exp(1j * self.rng.uniform(0, 6.28)))})
    return True

  def _renorm(self, h):
    nv = self.m.norm(h)
    self.emit({'op': 'scale', 'h': h, 'z': complex(1 / np.sqrt(nv))})

  def k_project_bit(self):
    rng, m = self.rng, self.m
    h = self.pick(self.usable)
    if h is None:
      return False
    bit, value = int(rng.integers(m.n[h])), int(rng.integers(2))
    if m._prob_bit({'h': h, 'bit': bit, 'value': value}) < 1e-3 * m.norm(h):
      value ^= 1
    self.emit({'op': 'project_bit', 'h': h, 'bit': bit, 'value': value})
    self._renorm(h)
    return True

  def k_project_bits(self):
    rng, m = self.rng, self.m
    h = self.pick(self.usable)
    if h is None:
      return False
    n = m.n[h]
    bits = [int(b) for b in rng.choice(n, size=int(rng.integers(1, min(4, n) + 1)), replace=False)]
    p = m._marginal({'h': h, 'bits': bits})
    j = int(rng.choice(np.flatnonzero(p >= 0.5 * p.max())))
    mask = sum(1 << b for b in bits)
    value = sum(((j >> t) & 1) << b for t, b in enumerate(bits))
    self.emit({'op': 'project_bits', 'h': h, 'mask': mask, 'value': value})
    self._renorm(h)
    return True

  def k_norm2(self):
    h = self.pick()
    self.emit({'op': 'norm2', 'h': h})
    return True

  def k_prob_bit(self):
    h = self.pick(self.usable)
    if h is None:
      return False
    self.emit({'op': 'prob_bit', 'h': h, 'bit': int(self.rng.integers(self.m.n[h])), 'value': int(self.rng.integers(2))})
    return True

  def k_marginal(self):
    rng = self.rng
    h = self.pick(self.usable)
    if h is None:
      return False
    n = self.m.n[h]
    self.emit({'op': 'marginal', 'h': h, 'bits': [int(b) for b in rng.choice(n, size=int(rng.integers(0, min(8, n) + 1)), replace=False)]})
    return True

  def k_sample(self):
    h = self.pick(self.usable)
    if h is None:
      return False
    u = np.sort(self.rng.random(int(self.rng.integers(1, 65))))
    self.emit({'op': 'sample', 'h': h, 'u': u})
    return True

  def k_expect(self):
    rng, m = self.rng, self.m
    h = self.pick(self.usable)
    if h is None:
      return False
    n, loc = m.n[h], m.local_bits(h)
    xs = []
    for _ in range(int(rng.integers(1, 4))):
      x = 0
      for b in rng.choice(loc, size=int(rng.integers(0, min(4, len(loc)) + 1)), replace=False):
        x |= 1 << int(b)
      xs.append(x)
    nt = int(rng.integers(1, 21))
    x = [xs[int(rng.integers(len(xs)))] for _ in range(nt)]
    if rng.random() < 0.3:
      x = [xs[0]] * nt                                     # up to 20 terms on ONE x mask: two reads of 16
    z = [int(rng.integers(1 << n)) if rng.random() < 0.8 else 0 for _ in range(nt)]
    self.emit({'op': 'expect', 'h': h, 'x': x, 'z': z})
    return True

  def k_argmax(self):
    h = self.pick(self.usable)
    if h is None:
      return False
    self.emit({'op': 'argmax', 'h': h})
    return True

  def _held_index(self, h, count):
    mine = mine_of(self.m.n[h], self.m.held[h])
    return mine[self.rng.integers(mine.size, size=count)]

  def k_amplitude(self):
    h = self.pick(self.usable)
    if h is None:
      return False
    self.emit({'op': 'amplitude', 'h': h, 'index': int(self._held_index(h, 1)[0])})
    return True

  def k_amplitudes(self):
    rng = self.rng
    h = self.pick(self.usable)
    if h is None:
      return False
    idx = rng.integers(1 << self.m.n[h], size=int(rng.integers(0, 40)))           # (other shards' indices: exact zeros)
    idx = np.concatenate([idx, idx[:idx.size // 3], self._held_index(h, 3)]).astype(np.uint64)
    self.emit({'op': 'amplitudes', 'h': h, 'indices': rng.permutation(idx)})
    return True

  def k_select(self):
    rng = self.rng
    h = self.pick(self.usable)
    if h is None:
      return False
    _, _, p = self.m._probs(h)
    ps = np.sort(p)
    r = rng.random()
    if r < 0.25:
      thr = 0.0                                            # everything
    elif r < 0.45:
      thr = float(ps[-1]) * 2 + 1.0                        # nothing
    elif r < 0.8:
      thr = float(ps[-min(ps.size, int(rng.integers(1, 9)))])   # a few (ties with the threshold included)
    else:
      thr = float(ps[ps.size // 2])
    self.emit({'op': 'select', 'h': h, 'threshold': thr})
    return True

  def k_topk(self):
    h = self.pick(self.usable)
    if h is None:
      return False
    self.emit({'op': 'topk', 'h': h, 'k': int(self.rng.choice([1, 5, 64]))})
    return True

  def room(self):
    return len(self.live()) < self.max_live

  def k_clone(self):
    h = self.pick(self.usable)
    if h is None or not self.room():
      return False
    self.emit({'op': 'clone', 'h': h, 'new': self.new_slot()})
    return True

  def k_copy(self):
    rng, m = self.rng, self.m
    pairs = [(d, s) for d in self.live() for s in self.live() if d != s and m.n[d] == m.n[s] and m.held[d] == m.held[s] and self.usable(s)]
    if not pairs:
      return False
    pairs.sort(key=lambda p: -m.q[p[0]])                   # prefer a destination with gates queued
    d, s = pairs[0] if m.q[pairs[0][0]] and rng.random() < 0.7 else pairs[int(rng.integers(len(pairs)))]
    self.emit({'op': 'copy', 'h': d, 'src': s})
    return True

  def k_extend(self):
    rng, m = self.rng, self.m
    h = self.pick(lambda x: self.usable(x) and m.n[x] < MAX_BITS)
    if h is None or not self.room():
      return False
    k = int(rng.integers(1, min(3, MAX_BITS - m.n[h]) + 1))
    if m.n[h] + k > 17 and rng.random() < 0.5:
      return False                                         # (keep the largest states rare: they cost host time)
    amps, basis = (None, int(rng.integers(1 << k))) if rng.random() < 0.4 else (_rand_table(rng, k), 0)
    self.emit({'op': 'extend', 'h': h, 'k': k, 'amps': amps, 'basis': basis, 'new': self.new_slot()})
    return True

  def k_release(self):
    rng, m = self.rng, self.m
    h = self.pick(lambda x: self.usable(x) and m.nloc(x) >= 3)
    if h is None or not self.room():
      return False
    loc = m.local_bits(h)
    k = int(rng.integers(1, min(3, len(loc) - 2) + 1))
    bits = [int(b) for b in rng.choice(loc, size=k, replace=False)]
    p = m._marginal({'h': h, 'bits': bits})
    value = int(rng.choice(np.flatnonzero(p >= 0.5 * p.max())))
    new = self.new_slot()
    self.emit({'op': 'release', 'h': h, 'bits': bits, 'value': value, 'new': new})
    self._renorm(new)
    return True

  def k_close(self):
    m = self.m
    c = self.live()
    if len(c) < 2:                                         # never the last handle
      return False
    big = [h for h in c if m.n[h] >= 18]                   # (the largest states first: they cost host time)
    h = big[0] if big else c[int(self.rng.integers(len(c)))]
    self.emit({'op': 'close', 'h': h})
    return True

  def unalign(self, o, h):
    """in a third of the two-state steps one side's local bits are swapped first, so that the two layouts differ whether or
    not a sweep has re-laid one of them out (below 14 local bits nothing else would)"""
    if o != h and self.m.nloc(o) >= 2 and self.rng.random() < 0.35:
      a, b = (int(x) for x in self.rng.choice(self.m.local_bits(o), size=2, replace=False))
      self.emit({'op': 'remap', 'h': o, 'a': a, 'b': b})

  def k_inner(self):
    h = self.pick(self.usable)
    if h is None:
      return False
    o = self.partner(h)
    if o is None or (self.rng.random() < 0.15):
      o = h
    if not self.usable(o):
      return False
    self.unalign(o, h)
    self.emit({'op': 'inner', 'h': h, 'other': o})
    return True

  def k_axpby(self):
    rng = self.rng
    h = self.pick()
    o = self.partner(h) if h is not None else None
    if o is None or not self.usable(o):
      return False
    self.unalign(o, h)
    r = rng.random()
    cz = lambda: complex(rng.uniform(-1, 1), rng.uniform(-1, 1))      # noqa: E731
    exact = [(0, cz()), (cz(), 0), (0, 0), (1, 0), (1, 1), (1, -1), (-1, 1), (0, 1)]
    alpha, beta = (cz(), cz()) if r < 0.45 else exact[int(rng.integers(len(exact)))]
    if complex(alpha) != 0 and not self.usable(h):
      return False
    if complex(alpha) == 0 and complex(beta) != 0 and rng.random() < 0.5:
      # the header: alpha == 0 exactly, dst's old values are not read -- NaN in them does not propagate
      self.emit({'op': 'scale', 'h': h, 'z': complex(np.nan, 0), 'poison': True})
    trial = axpby_ref(self.m.wide(h), alpha, self.m.wide(o), beta)
    nv = float(np.vdot(trial, trial).real)
    if not (complex(alpha) == 0 and complex(beta) == 0) and not 1e-3 <= nv <= 100:
      if self.steps[-1].get('poison'):
        alpha, beta = 0, 1
      else:
        return False
    self.emit({'op': 'axpby', 'h': h, 'other': o, 'alpha': complex(alpha), 'beta': complex(beta)})
    if complex(alpha) == 0 and complex(beta) == 0:         # a state of zeros: give it content again
      self.emit({'op': 'copy', 'h': h, 'src': o})
    return True

  def k_pauli_sum(self):
    """dst := (sum_t c_t P_t) src into a new slot or into a partner of src in whatever condition the program left it"""
    rng, m = self.rng, self.m
    src = self.pick(self.usable)
    if src is None:
      return False
    dst = None
    if not self.room() or rng.random() < 0.5:
      c = sorted((x for x in self.live() if x != src and m.n[x] == m.n[src] and m.held[x] == m.held[src]), key=lambda x: -m.q[x])
      if not c:
        return False
      dst = c[0] if m.q[c[0]] and rng.random() < 0.7 else c[int(rng.integers(len(c)))]      # prefer a destination with gates queued
    n, loc, held = m.n[src], m.local_bits(src), m.held[src]
    lo, hi = ((0, 0), (1, 1), (2, 4), (5, 16), (17, 40))[int(rng.choice(5, p=[0.08, 0.27, 0.2, 0.2, 0.25]))]
    nt = int(rng.integers(lo, hi + 1))
    def xmask():                                             # local bits only, of any weight from 0 to all of them
      return sum(1 << int(b) for b in rng.choice(loc, size=int(rng.integers(0, len(loc) + 1)), replace=False))
    shape = int(rng.integers(3))
    if shape == 0:
      x = [xmask()] * nt                                     # one shared mask
    elif shape == 1:                                         # 2-3 masks in runs, given unsorted
      pool = [xmask() for _ in range(int(rng.integers(2, 4)))]
      x = [pool[(int(k) * len(pool)) // nt] for k in rng.permutation(nt)]
    else:
      x = [xmask() for _ in range(nt)]                       # all drawn apart
    z = [int(rng.integers(1 << n)) if rng.random() < 0.8 else 0 for _ in range(nt)]      # all global bits, held ones included
    kind = int(rng.choice(3, p=[0.6, 0.2, 0.2] if nt == 1 else [0.2, 0.3, 0.5]))
    if kind == 0:
      coeffs = [(1, -1, 1j, -1j)[int(k)] for k in rng.integers(4, size=nt)]      # one term: the exact paths
      if nt == 1 and rng.random() < 0.4:                     # the c that makes c' = c (-i)^nY (shard sign) == 1: the source's bits
        neg = sum(v for b, v in held.items() if (z[0] >> b) & 1) & 1
        coeffs = [c for c in (1, -1, 1j, -1j) if pauli_coef(c, _popcount(x[0] & z[0]), neg) == 1]
    elif kind == 1:
      coeffs = [float(v) for v in rng.uniform(-1, 1, nt)]
    else:
      coeffs = [complex(a, b) for a, b in rng.uniform(-1, 1, (nt, 2))]
    coeffs = np.asarray(coeffs, dtype=np.complex128).reshape(nt)
    csum = float(np.sum(np.abs(coeffs)))
    if csum > 4:
      coeffs = coeffs * (4 / csum)                           # C = sum |c_t| <= 4
    self.unalign(src if dst is None else dst, None if dst is None else src)      # (a remap relabels: the trial comes after it)
    if nt:
      trial = pauli_util.np_pauli_sum(m.wide(src), coeffs, x, z)
      if not 1e-3 <= float(np.vdot(trial, trial).real) <= 100:
        return False
    s = {'op': 'pauli_sum', 'h': src, 'dst': dst, 'coeffs': coeffs, 'x': x, 'z': z, 'poisoned': False}
    if dst is None:
      s['new'] = self.new_slot()
    else:
      if rng.random() < (0.15 if m.q[dst] else 0.35):        # the header: batch 0 does not read dst
        self.emit({'op': 'scale', 'h': dst, 'z': complex(np.nan, 0), 'poison': True})
        s['poisoned'] = True
    self.emit(s)
    if nt == 0:                                              # a state of zeros: give it content again
      self.emit({'op': 'copy', 'h': s['new'] if dst is None else dst, 'src': src})
    return True

  PP_BUDGET = 8.0              # M = prod_t (|a_t| + |b_t|) <= 8 on every emitted step: pauli_product_util.bound stays near the real rounding

  def _pp_factor(self, kind, share):
    """one factor (a, b) of the given kind with log(|a| + |b|) <= share: the angle or the magnitude is shrunk into the share"""
    rng = self.rng
    if kind == 'rotation':                                   # exp(-i t P)
      t = float(rng.uniform(-np.pi, np.pi))
      while np.log(abs(np.cos(t)) + abs(np.sin(t))) > share:
        t *= 0.5
      return complex(np.cos(t)), complex(0, -np.sin(t))
    if kind == 'imaginary':                                  # exp(-t P): cosh t + |sinh t| = e^|t|
      t = float(rng.uniform(-0.5, 0.5))
      while abs(t) > share:
        t *= 0.5
      return complex(np.cosh(t)), complex(-np.sinh(t))
    if kind == 'projector':
      return 0.5 + 0j, complex(0.5 * (1 - 2 * int(rng.integers(2))))
    if kind == 'string':
      return 0j, (1 + 0j, 1j, -1 + 0j, -1j)[int(rng.integers(4))]
    if kind == 'identity':
      return 1 + 0j, 0j
    a, b = complex(*rng.uniform(-1, 1, 2)), complex(*rng.uniform(-1, 1, 2))
    size = abs(a) + abs(b)
    if size > np.exp(share):
      a, b = a * (np.exp(share) / size * (1 - 1e-12)), b * (np.exp(share) / size * (1 - 1e-12))
    return a, b

  def k_pauli_product(self):
    """h := F_{n-1} ... F_0 h in place, F_t = a_t I + b_t P_t, on a usable handle in whatever condition the program left it"""
    rng, m = self.rng, self.m
    c = [x for x in self.live() if self.usable(x)]
    if not c:
      return False
    queued = [x for x in c if m.q[x]]
    h = queued[int(rng.integers(len(queued)))] if queued and rng.random() < 0.5 else c[int(rng.integers(len(c)))]      # a queue about half the time
    n, loc, held = m.n[h], m.local_bits(h), m.held[h]
    # the bands: the edges are kPauliProdSmallT (the smaller instantiation) and QH_PAULI_PRODUCT_BATCH (a full run)
    lo, hi = ((0, 0), (1, 1), (2, PAULI_PRODUCT_FEW), (PAULI_PRODUCT_FEW + 1, PAULI_PRODUCT_BATCH),
              (PAULI_PRODUCT_BATCH + 1, 3 * PAULI_PRODUCT_BATCH))[int(rng.choice(5, p=[0.06, 0.27, 0.22, 0.2, 0.25]))]
    nt = int(rng.integers(lo, hi + 1))
    def xmask():
      # local bits only, never 0.  One time in three of weight 1 or 2: only then can HALF and the in-wave walk occur whatever the
      # layout -- and half of those among the four lowest local bits, one in four of them the lowest alone: where the local map
      # is still the identity these are the in-wave walk and (complex64) HALF
      if rng.random() < 1 / 3:
        r = rng.random()
        pool = loc[:1] if r < 0.125 else loc[:4] if r < 0.5 else loc
        return sum(1 << int(b) for b in rng.choice(pool, size=int(rng.integers(1, min(2, len(pool)) + 1)), replace=False))
      return sum(1 << int(b) for b in rng.choice(loc, size=int(rng.integers(1, len(loc) + 1)), replace=False))
    shape = int(rng.integers(4))
    if shape == 0:                                           # one shared X, diagonal terms interleaved: one run per 8 terms
      X = xmask()
      x = [X if rng.random() < 0.6 else 0 for _ in range(nt)]
    elif shape == 1:                                         # two or three masks alternating: a new run at almost every term
      pool = [xmask() for _ in range(int(rng.integers(2, 4)))]
      x = [pool[t % len(pool)] for t in range(nt)]
    elif shape == 2:
      x = [xmask() for _ in range(nt)]                       # every mask drawn apart
    else:
      x = [0] * nt                                           # diagonal throughout
    z = [int(rng.integers(1 << n)) if rng.random() < 0.8 else 0 for _ in range(nt)]      # all global bits, held ones included
    runs = ppu.greedy_runs(x, PAULI_PRODUCT_BATCH, 0, PAULI_RUN_KINDS)                    # (logical masks cut as physical ones are)
    for f, cnt, X, _ in runs:                                # half the runs that exchange: one z mask with an odd overlap with X ('flip')
      if X and rng.random() < 0.5:
        t = f + int(rng.integers(cnt))
        if not _popcount(X & z[t]) & 1:
          z[t] ^= X & -X
    kinds = ('rotation', 'imaginary', 'projector', 'string', 'identity', 'general')
    p = [0.1, 0.08, 0.07, 0.45, 0.15, 0.15] if nt == 1 else [0.3, 0.15, 0.1, 0.2, 0.05, 0.2]      # one term: the exact paths in 6 of 10
    a, b, left = [], [], float(np.log(self.PP_BUDGET)) - 1e-9
    for t in range(nt):                                      # each term an equal share of what is left of log M
      at, bt = self._pp_factor(kinds[int(rng.choice(6, p=p))], max(left, 0.0) / (nt - t))
      if nt == 1 and at == 0 and rng.random() < 0.4:         # the b that makes b' = b (-i)^nY (shard sign) == 1: the stored bits
        neg = sum(v for hb, v in held.items() if (z[0] >> hb) & 1) & 1
        bt = [u for u in (1 + 0j, 1j, -1 + 0j, -1j) if pauli_coef(u, _popcount(x[0] & z[0]), neg) == 1][0]
      left -= float(np.log(abs(at) + abs(bt)))
      a.append(at)
      b.append(bt)
    a, b = np.asarray(a, dtype=np.complex128).reshape(nt), np.asarray(b, dtype=np.complex128).reshape(nt)
    self.pp_calls += 1
    if nt:
      trial = ppu.np_pauli_product(m.wide(h), a, b, x, z)
      if not (ppu.magnitude(a, b) <= self.PP_BUDGET and 1e-3 <= float(np.vdot(trial, trial).real) <= 100):
        self.pp_rejected += 1                                # (a zero result, of projectors mostly, is rejected here too)
        return False
    # (emit follows the step with a scale where the norm has left [0.25, 4])
    self.emit({'op': 'pauli_product', 'h': h, 'a': a, 'b': b, 'x': x, 'z': z, 'norm': bool(rng.integers(2))})
    return True

  def pick_half_queued(self):
    """a usable handle in whatever condition the program left it, half the time one with a burst queued"""
    rng, m = self.rng, self.m
    c = [x for x in self.live() if self.usable(x)]
    if not c:
      return None
    queued = [x for x in c if m.q[x]]
    return queued[int(rng.integers(len(queued)))] if queued and rng.random() < 0.5 else c[int(rng.integers(len(c)))]

  def k_reduced_density(self):
    """rho of k local logical bits in random list order; k from the bands whose edges are the kernels' (k <= 2 straight from memory,
    k < 6 folded groups, 6 one tile, 7 and 8 three and ten block pairs) and the whole shard"""
    rng, m = self.rng, self.m
    h = self.pick_half_queued()
    if h is None:
      return False
    last = self.steps[-1]                                    # half the time right behind extend or copy_from, on the handle they made or filled
    fresh = last.get('new') if last['op'] == 'extend' else last['h'] if last['op'] == 'copy' else None
    if fresh is not None and self.usable(fresh) and rng.random() < 0.5:
      h = fresh
    loc = m.local_bits(h)                                    # on a shard: only bits the shard index does not hold
    nloc, kmax = len(loc), min(DENSITY_MAX_BITS, len(loc))
    bands = [(lo, min(hi, kmax)) for lo, hi in ((0, 0), (1, 2), (3, 5), (6, 6), (7, 7), (8, 8)) if lo <= kmax]
    if nloc <= DENSITY_MAX_BITS:
      bands.append((nloc, nloc))                             # k = nloc: the outer product of the shard's state
    lo, hi = bands[int(rng.integers(len(bands)))]
    k = int(rng.integers(lo, hi + 1))
    if nloc >= 18 and rng.random() < 0.6:
      k = 8                                                  # with k = 7 from 19 bits on the only way to chunks_per_wg > 1 below MAX_BITS
    if rng.random() < 1 / 3:                                 # the bits that sit lowest in the map (as far as the model knows it) among them
      low = sorted(loc, key=lambda b: m.bm[h][b])[:min(k, int(rng.integers(1, 3)))]
      rest = [b for b in loc if b not in low]
      bits = low + [int(b) for b in rng.choice(rest, size=k - len(low), replace=False)]
      bits = [int(bits[j]) for j in rng.permutation(len(bits))]
    else:
      bits = [int(b) for b in rng.choice(loc, size=k, replace=False)]      # in random order, not ascending: row_bit is no identity
    self.emit({'op': 'reduced_density', 'h': h, 'bits': bits})
    return True

  ZP_BUDGET = 8.0              # E = exp(|c.re| F) <= 8, F = sum |w_t|, on every emitted 'zpoly' step: zpoly_util.apply_bound stays near the real rounding

  def _zp_terms(self, h):
    """(weights, z masks) of a cost function on handle h: the term counts about the 64 lanes a segment's terms are dealt to, the
    masks in the shapes that make the planner's classes and groups -- aimed by the map as far as the model knows it"""
    rng, m = self.rng, self.m
    n, loc, held = m.n[h], m.local_bits(h), sorted(m.held[h])
    nloc, bm = len(loc), m.bm[h]
    lo, hi = ((0, 0), (1, 1), (2, 8), (9, 63), (64, 200), (ZPOLY_MAX_TERMS, ZPOLY_MAX_TERMS))[int(rng.choice(6, p=[0.06, 0.1, 0.28, 0.26, 0.24, 0.06]))]
    nt = min(int(rng.integers(lo, hi + 1)), ZPOLY_MODEL_BUDGET >> nloc)      # the NumPy model evaluates f term by term
    low_bits = PAULI_CHUNK_BITS + (0 if self.bw == 128 else 1)
    below = [b for b in loc if bm[b] < low_bits]             # the low part of the index and the chunk part, in logical bits
    above = [b for b in loc if bm[b] >= low_bits]
    def mask(pool, lo_w, hi_w):
      hi_w = min(hi_w, len(pool))
      return sum(1 << int(b) for b in rng.choice(pool, size=int(rng.integers(min(lo_w, hi_w), hi_w + 1)), replace=False))
    everything = list(range(n))
    def any_shape():
      r = rng.random()
      if r < 0.08:
        return 0                                             # a constant term
      if r < 0.33:
        return mask(everything, 1, 1)
      if r < 0.63:
        return mask(everything, 2, 2)                        # an edge
      if r < 0.83:
        return mask(everything, 3, n)
      if r < 0.9 or not held:
        return (1 << n) - 1 if r < 0.88 else sum(1 << b for b in loc)      # the full register, global or local
      return mask(everything, 0, 3) | (1 << held[int(rng.integers(len(held)))])      # a held shard bit among them
    shape = int(rng.integers(4)) if above and below else int(rng.integers(2))
    if shape == 0:
      z = [any_shape() for _ in range(nt)]
    elif shape == 1:                                         # the edge list of a random graph, with fields on some vertices
      z = [mask(everything, 2, 2) if rng.random() < 0.8 else mask(everything, 1, 1) for _ in range(nt)]
    elif shape == 2:                                         # 1-4 low masks, each with several masks above it: as many groups
      lows = [mask(below, 1, 3) for _ in range(int(rng.integers(1, 5)))]
      z = [lows[int(rng.integers(len(lows)))] | mask(above, 1, 3) for _ in range(nt)]
      z = [0 if rng.random() < 0.05 else v for v in z]
    else:                                                    # constants and the chunk part alone: one long segment, wherever the bits lie
      z = [0 if rng.random() < 0.5 else mask(above, 1, 3) for _ in range(nt)]
    if held and rng.random() < 0.5:                          # held shard bits in a third of the masks: signs folded into the weights
      z = [v | (1 << held[int(rng.integers(len(held)))]) if rng.random() < 1 / 3 else v for v in z]
    if nt >= 2 and rng.random() < 0.3:                       # the same mask twice: equal masks are not merged
      a, b = (int(x) for x in rng.choice(nt, size=2, replace=False))
      z[a] = z[b]
    w = rng.choice([-1.0, 1.0], size=nt) * 10.0 ** rng.uniform(-2.5, 0.5, size=nt)      # both signs, mixed magnitudes
    return np.asarray(w, dtype=np.float64).reshape(nt), [int(v) for v in z]

  def k_expect_zpoly(self):
    h = self.pick_half_queued()
    if h is None:
      return False
    w, z = self._zp_terms(h)
    self.emit({'op': 'expect_zpoly', 'h': h, 'w': w, 'z': z, 'nloc': self.m.nloc(h)})
    return True

  def k_zpoly(self):
    """h := exp(c f) h in place: c purely imaginary (no exp in the kernel), purely real, general or exactly (0, 0); c.re is drawn
    inside the budget exp(|c.re| F) <= 8 as the Pauli products' factors are drawn inside M <= 8"""
    rng, m = self.rng, self.m
    h = self.pick_half_queued()
    if h is None:
      return False
    w, z = self._zp_terms(h)
    big_f = zu.big_f(w)
    re = float(rng.uniform(-1, 1)) * float(np.log(self.ZP_BUDGET)) * (1 - 1e-9) / big_f if big_f > 0 else float(rng.uniform(-1, 1))
    im = float(rng.uniform(-np.pi, np.pi)) / (big_f if big_f > 1 and rng.random() < 0.5 else 1.0)
    kind = int(rng.choice(4, p=[0.35, 0.25, 0.3, 0.1]))
    c = (complex(0, im), complex(re, 0), complex(re, im), 0j)[kind]
    self.zp_calls += 1
    if len(z) and c != 0:
      mine = mine_of(m.n[h], m.held[h]).astype(np.int64)
      trial = zu.np_apply(m.wide(h)[mine], w, z, c, f=zpoly_f(m.n[h], m.held[h], w, z))
      if not (np.exp(abs(c.real) * big_f) <= self.ZP_BUDGET and 1e-3 <= float(np.vdot(trial, trial).real) <= 100):
        self.zp_rejected += 1
        return False
    # (emit follows the step with a scale where the norm has left [0.25, 4])
    self.emit({'op': 'zpoly', 'h': h, 'w': w, 'z': z, 'c': c, 'norm': bool(rng.integers(2)), 'nloc': m.nloc(h)})
    return True

  def k_flush(self):
    h = self.pick(lambda x: self.m.q[x] > 0) or self.pick()
    self.emit({'op': 'flush', 'h': h})
    return True

  def k_set_relayout(self):
    h = self.pick()
    self.emit({'op': 'set_relayout', 'h': h, 'on': int(self.rng.integers(2))})
    return True

  def k_remap(self):
    m = self.m
    h = self.pick(lambda x: m.nloc(x) >= 2)
    if h is None:
      return False
    a, b = (int(x) for x in self.rng.choice(m.local_bits(h), size=2, replace=False))
    self.emit({'op': 'remap', 'h': h, 'a': a, 'b': b})
    return True

  def k_refused(self):
    """one host-side refusal from the header's lists; nothing is launched, nothing changes"""
    rng, m = self.rng, self.m
    if self.refused >= 2:
      return False
    h = self.pick(lambda x: m.nloc(x) >= 2)
    if h is None:
      return False
    loc = m.local_bits(h)
    whats = ['matrix_twice', 'mux_target_selected', 'marginal_twice', 'sample_descending', 'copy_self', 'axpby_self',
             'extend_basis', 'release_value', 'perm_not_bijection', 'perm_control_in_register', 'pauli_sum_self', 'pauli_sum_bad_qubit',
             'pauli_product_nonfinite', 'pauli_product_bad_qubit', 'density_same_qubit', 'density_bad_qubit', 'density_k_range',
             'zpoly_nonfinite', 'zpoly_bad_qubit', 'zpoly_too_many', 'expect_zpoly_nonfinite', 'expect_zpoly_bad_qubit', 'expect_zpoly_too_many']
    if m.held[h]:
      whats.append('density_nonlocal')                       # (a listed bit on the shard index: nothing runs, nothing is flushed)
      whats.append('perm_register_held')                     # (a register bit on the shard index: nothing is flushed)
      whats.append('pauli_sum_x_held')                       # (an x bit there: nothing runs, no handle comes into being)
      whats.append('pauli_product_x_held')                   # (likewise: the whole list is checked before anything is flushed)
    what = whats[int(rng.integers(len(whats)))]
    if m.held[h] and rng.random() < 0.4:                     # (the four that only a shard can draw, and few programs are shards)
      what = whats[len(whats) - 4 + int(rng.integers(4))]
    late = ('pauli_product_', 'density_', 'zpoly_', 'expect_zpoly_')      # calls that check everything before anything is flushed
    if what.startswith(late) and rng.random() < 0.5:
      # half of them on a handle with a burst queued, where the pool has one: the checks of a refused step then show that nothing was flushed
      c = [x for x in self.live() if m.q[x] and m.nloc(x) >= 2 and bool(m.held[x]) == bool(m.held[h])]
      if c:
        h = c[int(rng.integers(len(c)))]
        loc = m.local_bits(h)
    code = native.QH_ERR_SAME_QUBIT if what in ('matrix_twice', 'mux_target_selected', 'marginal_twice', 'perm_control_in_register', 'density_same_qubit') \
        else native.QH_ERR_NONLOCAL if what in ('perm_register_held', 'pauli_sum_x_held', 'pauli_product_x_held', 'density_nonlocal') \
        else native.QH_ERR_BAD_QUBIT if what.endswith('_bad_qubit') else native.QH_ERR_ARG
    s = {'op': 'refused', 'h': h, 'what': what, 'code': code, 'bits': [int(loc[0]), int(loc[1])]}
    if what.startswith(('density_', 'zpoly_', 'expect_zpoly_')):
      s['nbits'], s['queued'] = m.n[h], bool(m.q[h])
    if what == 'density_k_range':                            # k = 9, and k = nloc + 1 on a handle of fewer than 8 local bits
      s['k'] = min(DENSITY_MAX_BITS, len(loc)) + 1
    if what.endswith('zpoly_nonfinite'):                     # NaN or an infinity in a weight of term 1 or 2 of 3 (and sometimes in the
      s['term'], s['value'] = int(rng.integers(1, 3)), ('nan', 'inf', '-inf')[int(rng.integers(3))]      # next one too), or in c
      s['also_next'], s['in_c'] = bool(rng.integers(2)), what == 'zpoly_nonfinite' and rng.random() < 0.3
      s['says'] = 'c = ' if s['in_c'] else f"term {s['term']} "      # qh_last_error names the first offending term
    if what.endswith('zpoly_bad_qubit'):
      s['term'] = int(rng.integers(1, 3))
    if what in ('perm_register_held', 'pauli_sum_x_held', 'pauli_product_x_held', 'density_nonlocal'):
      s['held'] = int(sorted(m.held[h])[int(rng.integers(len(m.held[h])))])
    if what.startswith('pauli_product_'):
      s['nbits'], s['queued'] = m.n[h], bool(m.q[h])
      s['in_x'] = bool(rng.integers(2))                      # bad_qubit: the bit beyond the register in the x mask or in the z mask
      if what == 'pauli_product_nonfinite':                  # NaN or an infinity in one of the four numbers of term 1 or 2 of 3
        s['term'], s['slot'], s['value'] = int(rng.integers(1, 3)), int(rng.integers(4)), ('nan', 'inf', '-inf')[int(rng.integers(3))]
        s['says'] = f"term {s['term']} "                      # qh_last_error names the first offending term
    if what.startswith('pauli_sum_'):
      s['nbits'] = m.n[h]
      o = self.partner(h) if what != 'pauli_sum_self' else None
      if o is not None:
        s['other'] = o                                       # also through an existing destination, which stays as it is
    self.refused += 1
    self.emit(s)
    return True

  WEIGHTS = {'gates': 9.0, 'close': 0.6, 'refused': 2.0, 'remap': 1.6, 'flush': 0.7, 'clone': 1.3, 'inner': 1.8, 'axpby': 1.8, 'copy': 1.3,
             'pauli_sum': 2.5, 'pauli_product': 2.5, 'reduced_density': 2.0, 'expect_zpoly': 1.5, 'zpoly': 2.5}

  def run(self):
    self.start()
    nsteps = int(self.rng.integers(30, 56))              # fixed by the seed, never by a clock; a kind adds at most 5 steps
    kinds = list(KINDS)
    w = np.array([self.WEIGHTS.get(k, 1.0) for k in kinds])
    w /= w.sum()
    tries = 0
    while len(self.steps) - 1 < nsteps and tries < 40 * nsteps:
      tries += 1
      getattr(self, 'k_' + kinds[int(self.rng.choice(len(kinds), p=w))])()
    assert 30 <= len(self.steps) - 1 <= 60, len(self.steps)
    return self.steps


def gen_program(seed, bw, mode='own'):
  """the steps of program `seed` at width bw in mode 'own' | 'attached' | 'mapped' | 'shard': the same list every time"""
  assert bw in (128, 64) and mode in ('own', 'attached', 'mapped', 'shard')
  return _Gen(seed, bw, mode).run()


def gen_program_draws(seed, bw, mode='own'):
  """(the steps of gen_program, {kind: (draws made, draws rejected)} of the two budgeted drawers k_pauli_product and k_zpoly)"""
  g = _Gen(seed, bw, mode)
  return g.run(), {'pauli_product': (g.pp_calls, g.pp_rejected), 'zpoly': (g.zp_calls, g.zp_rejected)}


def describe(s):
  """a step as a short JSON-able dict (tables and matrices by shape)"""
  out = {}
  for k, v in s.items():
    if isinstance(v, np.ndarray) and np.iscomplexobj(v) and v.ndim == 1 and v.size <= 40:
      out[k] = [[float(c.real), float(c.imag)] for c in v]   # (the coefficients of a Pauli sum: enough to replay the step)
    elif isinstance(v, np.ndarray):
      out[k] = v.tolist() if v.size <= 8 else f'<{v.dtype} {list(v.shape)}>'
    elif k == 'gates' and s['op'] == 'gates':
      out[k] = f'<{len(v)} gates>'
    elif k == 'factors':
      out[k] = [(n, x if isinstance(x, int) else f'<table {len(x)}>') for n, x in v]
    elif isinstance(v, complex):
      out[k] = ['nan' if np.isnan(x) else x for x in (v.real, v.imag)]      # (a poison step: NaN does not equal itself)
    else:
      out[k] = v
  return out


# ---- the runner -----------------------------------------------------------------------------------------------------------------
class StepFailure(AssertionError):
  def __init__(self, index, step, what):
    super().__init__(f'step {index} {describe(step)}: {what}')
    self.index, self.step, self.what = index, step, what


class Check:
  """What a run of run_program is held to and what it saw: the width's tolerances, one event per step (for the coverage
  table) and the figures of the chain comparison."""

  def __init__(self, bw):
    self.bw = bw
    # (index, op, local bits out of canonical order, a queued burst ran in the step, inner path or None, the record of a
    # 'perm' step or None: what qh_perm_plan said of the layout the call worked on, and what kind of handle it was; for a
    # 'pauli_sum' step the record of _Runner.run_pauli_sum: what qh_pauli_sum_plan said, and what src and dst were; likewise the
    # records of run_pauli_product, run_reduced_density, run_zpoly and run_expect_zpoly)
    self.events = []
    self.relaid = 0             # barrier / reader steps whose own flush re-laid the handle out
    self.chain_err = self.chain_d = self.chain_tol = None
    self.ratios = {}            # family of derived bound -> the largest error seen as a fraction of it
    self.nloc0 = None


def _bitmap(st):
  return st.bitmap() if hasattr(st, 'bitmap') else shard_util.bitmap(st)


def _pending(st):
  if hasattr(st, 'pending_gates'):
    return st.pending_gates()
  import ctypes
  c = ctypes.c_uint64()
  native.check(st.lib.qh_pending_gates(st.h, ctypes.byref(c)))
  return int(c.value)


def _plans_relayout(st):
  """does the plan of what the handle has QUEUED re-lay it out: qh_plan_json's per-sweep relayout field, which goes through
  the engine's relayout_wanted and neither launches nor allocates (an empty queue has no sweeps and says nothing)"""
  if hasattr(st, 'plans_relayout'):
    return st.plans_relayout()
  return '"relayout":1' in st.plan_json()


def _canonical(bm, nloc):
  pos = [p for p in bm if p < nloc]
  return pos == sorted(pos)


_LOGICAL_CACHE = {}


def _logical_index(bm, shard, nloc):
  """global logical index of every local physical index of a shard under the bit map bm"""
  key = (tuple(bm), shard, nloc)
  if key not in _LOGICAL_CACHE:
    if len(_LOGICAL_CACHE) > 64:
      _LOGICAL_CACHE.clear()
    phys = (np.uint64(shard) << np.uint64(nloc)) | np.arange(1 << nloc, dtype=np.uint64)
    _LOGICAL_CACHE[key] = shard_util.logical_of(list(bm), phys).astype(np.int64)
  return _LOGICAL_CACHE[key]


class _Runner:
  def __init__(self, program, make_state, check):
    self.prog, self.make, self.check = program, make_state, check
    self.bw = program[0]['bw']
    self.dev, self.shard, self.fixed_ptr = {}, {}, {}
    self.m = ModelState()                                   # step-local: re-read from the device after every step
    self.chain = ModelState()                               # never re-read
    self.chain_r = ModelState(np.complex64) if self.bw == 64 else None
    self.i, self.s = 0, None
    self.fresh = {}                                         # handle -> 'extend' | 'release' | 'copy' while nothing else has touched it since

  def note(self, s):
    """which handles are as extend / release made them or copy_from filled them, with no step on them since"""
    if s['op'] in ('refused', 'init'):
      return
    for x in (s.get('h'), s.get('other'), s.get('src'), s.get('dst')):
      self.fresh.pop(x, None)
    if s['op'] in ('extend', 'release'):
      self.fresh[s['new']] = s['op']
    elif s['op'] == 'copy':
      self.fresh[s['h']] = 'copy'

  def fail(self, what):
    raise StepFailure(self.i, self.s, what)

  def need(self, cond, what):
    if not cond:
      self.fail(what)

  # -- reading a handle exactly: a clone's download through the clone's bit map (qh_download re-lays a permuted state out, so
  # the handle under test is never downloaded before the end; _logical of tests/test_gpu_inner.py)
  def read(self, h):
    st = self.dev[h]
    c = st.clone()
    try:
      self.need(_bitmap(c) == _bitmap(st), 'a clone does not carry its source\'s bit map')
      phys = c.download().astype(np.complex128)
      bm = _bitmap(c)                                        # (the download may have re-laid the clone out)
    finally:
      c.close()
    out = np.zeros(1 << self.m.n[h], dtype=np.complex128)
    out[_logical_index(bm, self.shard[h], st.nbits)] = phys
    return out

  def own_download(self, h):
    st = self.dev[h]
    phys = st.download().astype(np.complex128)
    out = np.zeros(1 << self.m.n[h], dtype=np.complex128)
    out[_logical_index(_bitmap(st), self.shard[h], st.nbits)] = phys
    return out

  def kernels(self, h):
    return self.dev[h].stats()['kernels_launched']

  def check_ptr(self, h, always=False):
    # (qh_device_ptr brings a permuted layout back to canonical order: between steps it is only asked where that moves nothing)
    if h in self.fixed_ptr and h in self.dev and (always or self.fixed_ptr[h][2] or _canonical(_bitmap(self.dev[h]), self.dev[h].nbits)):
      self.need(self.fixed_ptr[h][0]() == self.fixed_ptr[h][1], 'the pointer of an attached / host-mapped handle moved')

  def check_raw(self, h, vec, bm):
    """the state of an attached / host-mapped handle lies in the caller's memory, in the handle's current layout: read there
    (no call into the engine, so nothing is re-laid out) it is what the clone gave"""
    st = self.dev[h]
    if h in self.fixed_ptr and bm is not None and getattr(st, 'raw_view', None) is not None:
      raw = np.asarray(st.raw_view()).astype(np.complex128)
      self.need(np.array_equal(raw, vec[_logical_index(bm, self.shard[h], st.nbits)], equal_nan=True),
                'the caller\'s memory does not hold the state of the attached / host-mapped handle')

  def held_of(self, h):
    st, bm = self.dev[h], _bitmap(self.dev[h])
    return {b: (self.shard[h] >> (bm[b] - st.nbits)) & 1 for b in range(len(bm)) if bm[b] >= st.nbits}

  # -- the start ---------------------------------------------------------------------------------------------------------------
  def do_init(self, s):
    nloc, g, n = s['nloc'], s['g'], s['nloc'] + s['g']
    self.check.nloc0 = nloc
    psi, bm = init_vector(s), init_bitmap(s)
    dt = np.complex128 if self.bw == 128 else np.complex64
    for shard, h in enumerate(s['slots']):
      st = self.make(nloc, self.bw, s['mode'] if s['mode'] != 'shard' else 'own')
      self.dev[h], self.shard[h] = st, shard
      if g:
        st.set_shard(n, shard)
      if s['how'] == 'upload':                               # _make of tests/test_gpu_shard_readout.py: the swap relabels, so the
        st.upload(psi[_logical_index(bm, shard, nloc)].astype(dt))      # data goes up in the order the swaps will give it
      for a, b in s['swaps']:
        st.remap_swap(a, b)
      if s['how'] == 'basis':
        st.init_basis(s['index'])
      elif s['how'] == 'product':
        st.init_product(s['factors'])
      self.need(_bitmap(st) == bm, f'bit map {_bitmap(st)} after the start, expected {bm}')
      if s['mode'] == 'attached':
        self.fixed_ptr[h] = ((lambda st=st: st.device_ptr), st.device_ptr, False)
      elif s['mode'] == 'mapped':                            # (qh_host_ptr moves nothing: asked after every step)
        self.fixed_ptr[h] = ((lambda st=st: st.host_array().ctypes.data), st.host_array().ctypes.data, True)
    for mdl in (self.m, self.chain, self.chain_r):
      if mdl is not None:
        mdl.step(s)
    for h in s['slots']:
      got = self.read(h)
      err = float(np.max(np.abs(got - self.m.wide(h))))
      self.need(err <= amp_tol(self.bw), f'initial state off by {err:.3e}')        # _amp_tol
      self.need(self.held_of(h) == self.m.held[h], 'held bits differ from the model\'s')
      self.m.put(h, got)
      if s['how'] == 'upload':                               # an upload is exact: the chain starts from what the device holds
        for mdl in (self.chain, self.chain_r):
          if mdl is not None:
            mdl.put(h, got)

  # -- running one step on the device -------------------------------------------------------------------------------------------
  def _call(self, s):
    op, st = s['op'], self.dev[s['h']]
    if op == 'gates':
      for cm, t, g in s['gates']:
        st.apply_bits(cm, t, g)
    elif op == 'matrix':
      st.apply_matrix(s['m'], s['bits'], s['ctl'])
    elif op == 'mux':
      st.apply_mux(s['gates'], s['sel'], s['tgt'])
    elif op == 'diag':
      st.apply_diag(s['values'], s['bits'])
    elif op == 'perm':
      st.apply_perm(s['table'], s['bits'], s['ctl'])
    elif op == 'scale':
      st.scale(s['z'])
    elif op == 'project_bit':
      st.project_bit(s['bit'], s['value'])
    elif op == 'project_bits':
      st.project_bits(s['mask'], s['value'])
    elif op == 'norm2':
      return st.norm2()
    elif op == 'prob_bit':
      return st.prob_bit(s['bit'], s['value'])
    elif op == 'marginal':
      return st.marginal(s['bits'])
    elif op == 'sample':
      return st.sample(s['u'])
    elif op == 'expect':
      return st.expect_pauli(s['x'], s['z'])
    elif op == 'argmax':
      return st.argmax()
    elif op == 'amplitude':
      return complex(st.amplitude(s['index']))
    elif op == 'amplitudes':
      return st.amplitudes(s['indices'])
    elif op == 'select':
      return st.select(s['threshold'], cap=1 << 20)
    elif op == 'topk':
      return st.topk(s['k'])
    elif op == 'clone':
      self.dev[s['new']] = st.clone()
    elif op == 'copy':
      st.copy_from(self.dev[s['src']])
    elif op == 'extend':
      self.dev[s['new']] = st.extend(s['k'], s['amps'], s['basis'])
    elif op == 'release':
      self.dev[s['new']], kept, dropped = st.release(s['bits'], s['value'])
      return kept, dropped
    elif op == 'close':
      st.close()
      del self.dev[s['h']]
    elif op == 'inner':
      return st.inner(self.dev[s['other']])
    elif op == 'axpby':
      return st.axpby(s['alpha'], self.dev[s['other']], s['beta'], norm=True)
    elif op == 'flush':
      st.flush()
    elif op == 'set_relayout':
      return st.set_relayout(s['on'])
    elif op == 'remap':
      st.flush()                                           # positions are physical: those the queued sweeps leave
      bm = _bitmap(st)
      st.remap_swap(bm[s['a']], bm[s['b']])
      return bm
    return None

  def call(self, s):
    """a valid step the engine refuses is a failure of that step, named like any other"""
    try:
      return self._call(s)
    except native.QhError as e:
      self.fail(f'the engine refused a valid step: {e}')

  def refused(self, s):
    st, (a, b) = self.dev[s['h']], s['bits']
    calls = {
        'matrix_twice': lambda: st.apply_matrix(np.eye(4), [a, a]),
        'mux_target_selected': lambda: st.apply_mux(np.stack([np.eye(2)] * 2), [a], a),
        'marginal_twice': lambda: st.marginal([a, b, a]),
        'sample_descending': lambda: st.sample([0.5, 0.25]),
        'copy_self': lambda: st.copy_from(st),
        'axpby_self': lambda: st.axpby(1, st, 1),
        'extend_basis': lambda: st.extend(1, None, 2),
        'release_value': lambda: st.release([a], 2),
        'perm_not_bijection': lambda: st.apply_perm([0, 1, 1, 3], [a, b]),
        'perm_control_in_register': lambda: st.apply_perm([0, 1, 2, 3], [a, b], 1 << b),
        'perm_register_held': lambda: st.apply_perm([0, 1, 2, 3], [a, s.get('held')]),
        'pauli_sum_self': lambda out: st.apply_pauli_sum([1.0], [1 << a], [1 << b], out=st),
        'pauli_sum_bad_qubit': lambda out: st.apply_pauli_sum([1.0, 0.5], [1 << a, 0], [0, 1 << s.get('nbits', 0)], out=out),
        'pauli_sum_x_held': lambda out: st.apply_pauli_sum([0.5, 1.0], [1 << a, (1 << s.get('held', 0)) | (1 << b)], [0, 0], out=out),
    }
    if s['what'].startswith('pauli_product_'):               # three terms, the offending one never the first
      bad, high = float(s.get('value', 'nan')), 1 << s['nbits']
      ab = [[0.6, 0.0, 0.0, -0.8] for _ in range(3)]
      ab[s.get('term', 1)][s.get('slot', 0)] = bad
      ok_x, ok_z = [1 << a, 0, 1 << b], [1 << b, 1 << a, 0]
      calls['pauli_product_nonfinite'] = lambda: st.apply_pauli_product([complex(*t[:2]) for t in ab], [complex(*t[2:]) for t in ab], ok_x, ok_z)
      calls['pauli_product_bad_qubit'] = lambda: st.apply_pauli_product([0.6] * 3, [-0.8j] * 3, ok_x[:2] + [ok_x[2] | (high if s['in_x'] else 0)],
                                                                        ok_z[:2] + [ok_z[2] | (0 if s['in_x'] else high)], norm=True)
      calls['pauli_product_x_held'] = lambda: st.apply_pauli_product([0.6] * 3, [-0.8j] * 3, ok_x[:2] + [ok_x[2] | (1 << s.get('held', 0))], ok_z)
    if s['what'].startswith('density_'):
      k, high, loc = s.get('k', 0), s['nbits'], self.m.local_bits(s['h'])
      calls['density_same_qubit'] = lambda: st.reduced_density([a, a])
      calls['density_bad_qubit'] = lambda: st.reduced_density([a, high])
      calls['density_k_range'] = lambda: st.reduced_density((loc * (DENSITY_MAX_BITS + 1))[:k])      # (k is checked before the list)
      calls['density_nonlocal'] = lambda: st.reduced_density([a, s.get('held')])
    if 'zpoly_' in s['what']:                                # three terms, the offending one never the first; 4097 for too many
      ws, zs, t = [0.5, -0.25, 2.0], [1 << a, (1 << a) | (1 << b), 0], s.get('term', 1)
      if s['what'].endswith('nonfinite') and not s['in_c']:
        ws[t] = float(s['value'])
        if s['also_next'] and t + 1 < 3:
          ws[t + 1] = float('nan')
      if s['what'].endswith('bad_qubit'):
        zs[t] |= 1 << s['nbits']
      if s['what'].endswith('too_many'):
        ws, zs = [0.0] * (ZPOLY_MAX_TERMS + 1), [1 << a] * (ZPOLY_MAX_TERMS + 1)
      c = complex(float(s['value']), 0.5) if s.get('in_c') else complex(0.25, -0.5)
      calls[s['what']] = (lambda: st.expect_zpoly(ws, zs)) if s['what'].startswith('expect_') else (lambda: st.apply_zpoly(ws, zs, c, norm=True))
    # a refused Pauli sum: into a new handle (none may come into being) and, where the pool has one, into an existing one
    outs = [None] + ([self.dev[s['other']]] if s.get('other') is not None else []) if s['what'].startswith('pauli_sum_') else [()]
    for out in outs:
      try:
        made = calls[s['what']](*(() if out == () else (out,)))
      except native.QhError as e:
        self.need(e.code == s['code'], f'error code {e.code}, expected {s["code"]}')
        self.need(s.get('says', '') in str(e), f'the error message does not say "{s.get("says")}": {e}')
        continue
      if s['what'].startswith('pauli_sum_') and made is not None and made is not out and hasattr(made, 'close'):
        made.close()                                         # (the handle that should not exist)
      self.fail('the call was not refused')

  # -- one step ------------------------------------------------------------------------------------------------------------------
  def run_step(self, s):
    op, h, bw, m = s['op'], s['h'], self.bw, self.m
    involved = [x for x in (h, s.get('other'), s.get('src'), s.get('dst')) if x is not None]
    involved = list(dict.fromkeys(involved))
    for x in involved:
      self.need(_pending(self.dev[x]) == m.q[x], f'handle {x}: {_pending(self.dev[x])} gates pending before the step, expected {m.q[x]}')
    q_before = {x: m.q[x] for x in involved}
    quiet = not any(q_before.values())                     # nothing queued: stats, bit maps and amplitudes can be held exactly
    bm_before = {x: _bitmap(self.dev[x]) for x in involved}
    if op == 'gates':
      self.call(s)
      for mdl in (m, self.chain, self.chain_r):
        if mdl is not None:
          mdl.step(s)
      self.need(_pending(self.dev[h]) == m.q[h], f'{_pending(self.dev[h])} gates pending behind the burst, expected {m.q[h]}')
      self.need(_bitmap(self.dev[h]) == bm_before[h], 'queueing gates changed the bit map')
      self.check.events.append((self.i, op, not _canonical(bm_before[h], self.dev[h].nbits), False, None, None))
      return
    if op == 'refused':
      k0 = {x: self.kernels(x) for x in involved}
      stats0 = self.dev[h].stats()
      self.refused(s)
      for x in involved:                                     # (the handle, and the destination a refused Pauli sum was given)
        self.need(_pending(self.dev[x]) == q_before[x] and _bitmap(self.dev[x]) == bm_before[x] and self.kernels(x) == k0[x],
                  f'handle {x}: a refused call changed the queue, the bit map or launched a kernel')
        if q_before[x] == 0:
          self.need(self.read(x).tobytes() == m.wide(x).tobytes(), f'handle {x}: a refused call changed the state')
      if s['what'].startswith(('density_', 'zpoly_', 'expect_zpoly_')):      # "nothing runs, nothing changes, nothing is flushed"
        self.need(self.dev[h].stats() == stats0, f'a refused call changed the stats: {self.dev[h].stats()}, before {stats0}')
        if q_before[h] == 0:                                 # (asking an attached handle for its pointer runs what is queued)
          self.check_ptr(h)
      self.check.events.append((self.i, op, False, False, None, None))
      return
    for x in involved:                                     # the mode, read without changing it, where a plan exists to show it
      if q_before[x] and self.dev[x].nbits >= SWEEPS_FROM and not m.wanted(x):
        self.need(not _plans_relayout(self.dev[x]), f'handle {x}: the queued burst is planned with relayout sweeps, its relayout mode is off')
    if op == 'pauli_sum':
      self.run_pauli_sum(s, q_before, bm_before)
      return
    if op == 'pauli_product':
      self.run_pauli_product(s, q_before[h], bm_before[h])
      return
    if op in ('reduced_density', 'expect_zpoly', 'zpoly'):
      getattr(self, 'run_' + op)(s, q_before[h], bm_before[h])
      return
    k_before = {x: self.kernels(x) for x in involved}
    n0 = {x: self.dev[x].marginal([]).tobytes() for x in involved} if quiet and op in READERS + ('inner',) else {}
    if n0:
      k_before = {x: self.kernels(x) for x in involved}
    path = None
    if op in TWO_STATE and quiet:
      path = self.dev[h].inner_plan(self.dev[s['other']])['path']
    stats0 = self.dev[h].stats() if op == 'perm' else None
    got = self.call(s)
    dk = {x: self.kernels(x) - k_before[x] for x in involved if x in self.dev}
    want = m.step(s)
    perm = self.perm_record(s, q_before[h], bm_before[h]) if op == 'perm' else None      # (no call between: m is the model)
    for mdl in (self.chain, self.chain_r):
      if mdl is not None:
        mdl.step(s)
    if op == 'close':
      self.check.events.append((self.i, op, False, False, None, None))
      return
    if op == 'set_relayout' and s['on'] and q_before[h]:   # allocates, runs nothing: the burst stays queued (and unread)
      self.need(_pending(self.dev[h]) == q_before[h] and _bitmap(self.dev[h]) == bm_before[h], 'set_relayout(1) ran the queue')
      self.need(bool(got) == bool(want), f'set_relayout(1) answered {got}, the mode should be {int(want)}')
      self.check.events.append((self.i, op, not _canonical(bm_before[h], self.dev[h].nbits), False, None, None))
      return
    # every barrier: nothing is left queued -- on the destination of a copy because its queue was dropped
    for x in involved:
      self.need(_pending(self.dev[x]) == 0, f'handle {x}: {_pending(self.dev[x])} gates pending behind a barrier step')
    new = s.get('new')
    if new is not None:
      self.shard[new] = self.shard[h]
      self.need(_pending(self.dev[new]) == 0, 'a new handle with gates queued')
      self.need(self.dev[new].stats()['kernels_launched'] == 0, 'a new handle whose stats are not zero')
    if op in TWO_STATE and path is None:
      path = self.dev[h].inner_plan(self.dev[s['other']])['path']
    bm_after = {x: _bitmap(self.dev[x]) for x in involved}
    # -- bit maps ------------------------------------------------------------------------------------------------------------
    for x in involved:
      moved = bm_after[x] != bm_before[x]
      if op == 'copy' and x == h:
        self.need(bm_after[h] == bm_after[s['src']], 'copy_from: the destination\'s bit map is not the source\'s')
      elif op == 'remap' and x == h:
        a, b = s['a'], s['b']
        exp = list(got)                                    # (the map behind remap_swap's own flush)
        self.need(exp == bm_before[h] or (q_before[h] and m.mode[h] == 1), 'remap_swap: its flush moved a bit map that relayout may not touch')
        exp[a], exp[b] = exp[b], exp[a]
        self.need(bm_after[h] == exp, f'remap_swap: bit map {bm_after[h]}, expected {exp}')
      elif op == 'set_relayout' and not s['on']:
        self.need(_canonical(bm_after[x], self.dev[x].nbits), 'set_relayout(0) left the local bits out of order')
      elif q_before[x] == 0:
        self.need(not moved, f'handle {x}: the bit map moved in a step that had nothing to flush')
      elif moved:                                          # only relayout sweeps do that, and only where the mode is on
        self.need(m.mode[x] == 1, f'handle {x}: a flush re-laid the handle out, its relayout mode is {m.mode[x]}')
        if op in BARRIERS + READERS:
          self.check.relaid += 1                           # relayout sweeps left a permuted map in front of this very call
      self.need({b for b, p in enumerate(bm_after[x]) if p >= self.dev[x].nbits} == set(m.held[x]), 'the held bits changed')
      self.check_ptr(x)
    if op == 'set_relayout':
      self.need(bool(got) == bool(want), f'set_relayout({s["on"]}) answered {got}, the mode should be {int(want)}')
    if op == 'clone':
      self.need(_bitmap(self.dev[new]) == bm_after[h], 'clone: the bit map is not the source\'s')
    if op == 'extend':
      nl, k = self.dev[h].nbits, s['k']
      exp = list(range(nl, nl + k)) + [p if p < nl else p + k for p in bm_after[h]]
      self.need(_bitmap(self.dev[new]) == exp, f'extend: bit map {_bitmap(self.dev[new])}, expected {exp}')
    if op == 'release':
      gone = sorted(bm_after[h][b] for b in s['bits'])
      exp = [p - sum(1 for r in gone if r < p) for b, p in enumerate(bm_after[h]) if b not in s['bits']]
      self.need(_bitmap(self.dev[new]) == exp, f'release: bit map {_bitmap(self.dev[new])}, expected {exp}')
    # -- amplitudes: what every touched handle holds now, exactly, against the model's step from what it held before ------------
    touched = involved + ([new] if new is not None else [])
    exact_ops = READERS + ('clone', 'copy', 'release', 'flush', 'set_relayout', 'remap', 'inner', 'project_bit', 'project_bits')
    after = {}
    for x in touched:
      after[x] = self.read(x)
      w = m.wide(x)
      if s.get('poison'):
        self.need(bool(np.all(np.isnan(after[x][mine_of(m.n[x], m.held[x]).astype(np.int64)]))), 'scale by NaN left numbers')
        continue
      exact = quiet and (op in exact_ops or (op == 'extend' and (x == h or s['amps'] is None)) or
                         (op == 'axpby' and (x != h or (s['alpha'] == 1 and s['beta'] == 0))))
      if op == 'perm' and quiet:                           # "moved as stored": the same bytes, the sign of a zero included
        self.need(after[x].tobytes() == w.tobytes(), f'handle {x}: a permutation did not move the amplitudes bit for bit '
                  f'(max diff {float(np.max(np.abs(after[x] - w))):.3e}, {int(np.sum(np.signbit(after[x].view(np.float64)) != np.signbit(w.view(np.float64))))} signs differ)')
      elif exact:     # zero tolerance (array_equal: equal as numbers, the sign of a zero may differ)
        self.need(np.array_equal(after[x], w), f'handle {x}: amplitudes changed where the header promises them as stored '
                  f'(max diff {float(np.max(np.abs(after[x] - w))):.3e})')
      else:
        err = float(np.max(np.abs(after[x] - w)))
        self.need(err <= amp_tol(bw), f'handle {x}: amplitudes off by {err:.3e} (limit {amp_tol(bw):.1e})')      # _amp_tol
      if op in ('project_bit', 'project_bits') and x == h:
        keep = np_keep(w.size, *((1 << s['bit'], s['value'] << s['bit']) if op == 'project_bit' else (s['mask'], s['value'])))
        self.need(not np.any(after[x][~keep]), 'a projection left something where it writes zeros')
      m.put(x, after[x])
      self.check_raw(x, after[x], bm_after.get(x))
    if op in ('clone', 'copy'):
      a, b = (new, h) if op == 'clone' else (h, s['src'])
      self.need(after[a].tobytes() == after[b].tobytes(), f'{op}: the two states differ')
    # -- results, from what the handle holds now (a reader changes nothing: the model's answer on the exact state) --------------
    if op in READERS or op == 'inner':
      want = m.step(s)
      self.results(s, got, want, after, bm_after)
      for x, b in n0.items():
        self.need(self.dev[x].marginal([]).tobytes() == b, f'handle {x}: marginal([]) changed its bits across a reader')
    elif op == 'release':
      # from what src holds now (release leaves src as it is), as the readers' answers: behind a queued burst the model's own
      # weights carry the burst's rounding, which _amp_tol allows per amplitude and _close does not allow for a sum
      _, *want = np_release(after[h], s['bits'], s['value'])
      for name, g_, w_ in (('kept', got[0], want[0]), ('dropped', got[1], want[1])):
        miss = close(g_, w_, bw)                           # _close
        self.need(miss is None, f'release: weight {name} {miss}')
    elif op == 'axpby' and not np.isnan(want):
      want = m.norm(h)
      miss = close(got, want, bw)                          # _close
      self.need(miss is None, f'axpby: norm2 {miss}')
    # -- stats, where the header gives an exact number ---------------------------------------------------------------------------
    if quiet:
      exp = None
      if op in ('mux', 'diag', 'select'):
        exp = {h: 1}
      elif op == 'amplitudes':
        exp = {h: 0}
      elif op == 'expect':
        xs = {}
        for x in s['x']:
          xs[x] = xs.get(x, 0) + 1
        exp = {h: sum(-(-c // 16) for c in xs.values())}
      elif op == 'inner':
        exp = {h: 1, s['other']: 0} if s['other'] != h else {h: 1}
      elif op == 'axpby':
        exp = {h: 0 if s['alpha'] == 1 and s['beta'] == 0 else 1, s['other']: 0}
      elif op in ('extend', 'release'):
        exp = {h: 1}
      elif op == 'perm':                                   # one kernel on either path; a held control that is 0 here: none
        exp = {h: perm['ctl_met']}
        ds = {k: perm['stats'][k] - stats0[k] for k in ('gates_submitted', 'gates_noop')}
        self.need(ds == {'gates_submitted': 1, 'gates_noop': 1 - perm['ctl_met']},
                  f'apply_perm with ctl_met = {perm["ctl_met"]}: {ds}, the header says gates_submitted + 1 and gates_noop + {1 - perm["ctl_met"]}')
      if exp is not None:
        for x, e in exp.items():
          self.need(dk[x] == e, f'handle {x}: kernels_launched grew by {dk[x]}, the header says {e}')
    local_perm = not _canonical(bm_after[h], self.dev[h].nbits)
    self.check.events.append((self.i, op, local_perm, bool(q_before[h]), path, perm))

  PAULI_STATS = ('kernels_launched', 'bytes_swept', 'bytes_algorithmic')

  def run_pauli_sum(self, s, q_before, bm_before):
    """One 'pauli_sum' step: h is the source, the result replaces the handle `dst` or becomes the new handle `new`.  A step
    is QUIET where the source has nothing queued (what the destination has queued is dropped and runs nothing): then the
    source, the amplitudes, the plan and norm2 are held exactly.  The destination's stats are held on every step -- the
    source's flush is not counted there."""
    m, bw = self.m, self.bw
    src, dst, new = s['h'], s['dst'], s.get('new')
    st = self.dev[src]
    coeffs, xs, zs = s['coeffs'], s['x'], s['z']
    nt, n = len(xs), m.n[src]
    quiet = q_before[src] == 0
    csum = float(np.sum(np.abs(coeffs)))
    mine = mine_of(n, m.held[src]).astype(np.int64)
    if s['poisoned']:
      self.need(bool(np.all(np.isnan(m.wide(dst)[mine]))), 'the destination of this step was to hold NaN')
    plan0 = st.pauli_sum_plan(xs, zs) if quiet else None    # asked on src right before the call
    src_stats0 = st.stats()
    d_stats0 = self.dev[dst].stats() if dst is not None else dict.fromkeys(self.PAULI_STATS, 0)
    try:
      out, n2 = st.apply_pauli_sum(coeffs, xs, zs, out=None if dst is None else self.dev[dst], norm=True)
    except native.QhError as e:
      self.fail(f'the engine refused a valid step: {e}')
    d = new if dst is None else dst
    if dst is None:
      self.dev[new], self.shard[new] = out, self.shard[src]
    dv = self.dev[d]
    self.need(out is dv, 'apply_pauli_sum did not return the destination it was given')
    terms, batches = st.pauli_sum_plan(xs, zs)              # right behind the call: the layout the call's own flush left
    bm_src, bm_dst = _bitmap(st), _bitmap(dv)
    want_n2 = m.step(s)
    for mdl in (self.chain, self.chain_r):
      if mdl is not None:
        mdl.step(s)
    for x in (src, d):                                      # src's queue ran, dst's was dropped
      self.need(_pending(self.dev[x]) == 0, f'handle {x}: {_pending(self.dev[x])} gates pending behind a Pauli sum')
    # -- bit maps: dst takes src's; src's moves only behind a flush whose relayout mode is on --------------------------------
    self.need(bm_dst == bm_src, f'the destination\'s bit map {bm_dst} is not the source\'s {bm_src}')
    moved = bm_src != bm_before[src]
    if quiet:
      self.need(not moved, 'the source\'s bit map moved in a step that had nothing to flush')
    elif moved:
      self.need(m.mode[src] == 1, f'a flush re-laid the source out, its relayout mode is {m.mode[src]}')
      self.check.relaid += 1
    for x in (src, d):
      self.need({b for b, p in enumerate(_bitmap(self.dev[x])) if p >= self.dev[x].nbits} == set(m.held[x]), 'the held bits changed')
      self.check_ptr(x)
    # -- the plan, held to the bit map by the rule stated in Python ----------------------------------------------------------------
    want_plan = pauli_plan_rule(st.nbits, bm_src, self.shard[src], xs, zs)
    self.need((terms, batches) == want_plan, f'qh_pauli_sum_plan says {(terms, batches)}, the rule on bit map {bm_src} gives {want_plan}')
    if quiet:
      self.need(plan0 == (terms, batches), 'the plan asked before a quiet call differs from the plan asked behind it')
    # -- norm2 twice on a quiet step: the same bits --------------------------------------------------------------------------------
    calls = 1
    if quiet:
      _, again = st.apply_pauli_sum(coeffs, xs, zs, out=dv, norm=True)
      calls = 2
      self.need(again == n2, f'norm2 {n2!r}, from the same call repeated {again!r}')
      self.need(_bitmap(dv) == bm_src and _bitmap(st) == bm_src and _pending(dv) == 0, 'the repeated call moved a bit map or queued something')
      self.need(st.stats() == src_stats0, 'the source\'s stats changed')
    # -- stats of the destination, as the header gives them from the plan ---------------------------------------------------------
    sb = (1 << st.nbits) * (16 if bw == 128 else 8)
    grow = {'kernels_launched': max(1, len(batches)), 'bytes_swept': (sum(b['streams'] for b in batches) if batches else 1) * sb,
            'bytes_algorithmic': (2 if nt else 1) * sb}
    d_stats = dv.stats()
    for k in self.PAULI_STATS:
      self.need(d_stats[k] - d_stats0[k] == calls * grow[k], f'the destination\'s {k} grew by {d_stats[k] - d_stats0[k]}, the header says {calls} x {grow[k]}')
    if dst is None:                                         # a new handle starts with zeroed stats, which then count this call
      self.need(all(v == calls * grow.get(k, 0) for k, v in d_stats.items()), f'a new handle whose stats are not those of this call: {d_stats}')
    # -- amplitudes -------------------------------------------------------------------------------------------------------------------
    after_src, after_d = self.read(src), self.read(d)
    w_src = m.wide(src)
    if quiet:
      self.need(np.array_equal(after_src, w_src), 'the source\'s amplitudes changed')
    else:
      err = float(np.max(np.abs(after_src - w_src)))
      self.need(err <= amp_tol(bw), f'the source behind its queue: amplitudes off by {err:.3e} (limit {amp_tol(bw):.1e})')      # _amp_tol
    m.put(src, after_src)
    want = m.wide(d)                                        # the model's step from what src held
    amax = float(np.max(np.abs(after_src)))                 # src as stored
    b = pauli_util.bound(bw, coeffs, amax, len(batches))
    if not quiet:
      b += csum * amp_tol(bw)                               # the burst's own error passes through at most C
    cps = [pauli_coef(coeffs[t['index']], t['ny'], t['neg']) for t in terms]
    unit = pauli_unit(cps[0]) if nt == 1 else None
    if nt == 0:
      self.need(not np.any(after_d), 'no terms: the destination is not all zeros')
    elif unit is not None and quiet:
      self.need(np.array_equal(after_d, want), f'one term with c\' = i^{unit}: the amplitudes are not exact (max diff {float(np.max(np.abs(after_d - want))):.3e})')
      if unit == 0:                                         # the same bytes, the sign of a zero included
        local = sum(1 << b_ for b_ in m.local_bits(src))
        exp = np.zeros(1 << n, dtype=np.complex128)
        exp[mine] = pauli_rotated(w_src, n, xs[0], zs[0] & local, 0)[mine]
        self.need(after_d.tobytes() == exp.tobytes(), f'one term with c\' = 1: not the source\'s bits '
                  f'({int(np.sum(np.signbit(after_d.view(np.float64)) != np.signbit(exp.view(np.float64))))} signs differ)')
    else:
      err = float(max(np.max(np.abs(after_d.real - want.real)), np.max(np.abs(after_d.imag - want.imag))))
      self.need(err <= b, f'amplitudes off by {err:.3e} per component (bound {b:.3e}, {len(batches)} batches, C = {csum:.3g})')
    m.put(d, after_d)
    self.check_raw(src, after_src, bm_src)
    self.check_raw(d, after_d, bm_dst)
    # -- norm2 --------------------------------------------------------------------------------------------------------------------------
    n2_np = float(np.vdot(after_d, after_d).real)
    self.need(abs(n2 - n2_np) <= 1e-12 * n2_np, f'norm2 {n2!r}, the amplitudes read back give {n2_np!r}')
    n2_tol = 4 * csum * amax * b * (1 << st.nbits)          # (as _apply_checked of tests/test_gpu_pauli_sum.py)
    self.need(abs(n2 - want_n2) <= n2_tol, f'norm2 {n2!r}, the model gives {want_n2!r} (tolerance {n2_tol:.3e})')
    # -- the record ---------------------------------------------------------------------------------------------------------------------
    ab = 0 if bw == 128 else 1
    rec = {'nloc': st.nbits, 'main': pauli_main_shape(st.nbits, bw), 'nbatches': len(batches), 'zero': nt == 0, 'unit': unit,
           'classes': [('few' if bt['count'] <= PAULI_FEW else 'many', 'one' if bt['ngroups'] == 1 else 'several') for bt in batches],
           'changed': unit is not None and cps[0] != complex(coeffs[0]),
           'shard': bool(m.held[src]), 'held_z': any((z >> hb) & 1 for z in zs for hb in m.held[src]), 'neg': any(t['neg'] for t in terms),
           'new': dst is None, 'dst_queued': dst is not None and bool(q_before[dst]), 'poisoned': bool(s['poisoned']),
           'dst_fixed': d in self.fixed_ptr, 'queued': not quiet, 'relayout_on': m.mode[src] == 1,
           'relaid': not quiet and moved and not _canonical(bm_src, st.nbits),
           'px0': bool(ab) and any(t['px'] & 1 for t in terms), 'pz0': bool(ab) and any(t['pz'] & 1 for t in terms)}
    self.check.events.append((self.i, 'pauli_sum', not _canonical(bm_src, st.nbits), not quiet, None, rec))

  def run_pauli_product(self, s, queued, bm_before):
    """One 'pauli_product' step, in place on h in whatever condition the program left it: every check of _apply_checked of
    tests/test_gpu_pauli_product.py and those of run_pauli_sum that apply.  A step is QUIET where h has nothing queued: then
    the plan, the bit map, the stats and the exact cases are held exactly, and the call is repeated from the same start
    (restored from a clone) for the same norm2 bits and the same amplitude bytes."""
    m, bw = self.m, self.bw
    h, st = s['h'], self.dev[s['h']]
    a, b, xs, zs = s['a'], s['b'], s['x'], s['z']
    nt, n, nloc = len(xs), m.n[h], st.nbits
    quiet = queued == 0
    mag = ppu.magnitude(a, b)                               # M
    mine = mine_of(n, m.held[h]).astype(np.int64)
    local = sum(1 << x for x in m.local_bits(h))
    plan0 = st.pauli_product_plan(xs, zs) if quiet else None      # asked right before the call
    keep = st.clone() if quiet and nt else None              # the start, for the repeat
    try:
      stats0 = st.stats()
      try:
        n2 = st.apply_pauli_product(a, b, xs, zs, norm=s['norm'])
      except native.QhError as e:
        self.fail(f'the engine refused a valid step: {e}')
      stats1 = st.stats()
      terms, runs = st.pauli_product_plan(xs, zs)             # right behind the call: the layout the call's own flush left
      bm = _bitmap(st)
      m.run(h)
      before = m.wide(h)                                      # quiet: what the handle held, bit for bit; else the model behind the burst
      want_n2 = m.step(s)
      for mdl in (self.chain, self.chain_r):
        if mdl is not None:
          mdl.step(s)
      self.need(_pending(st) == 0, f'{_pending(st)} gates pending behind a Pauli product')
      # -- bit map: as the call found it; behind a queue it moves only where the relayout mode is on -----------------------------
      moved = bm != bm_before
      if quiet:
        self.need(not moved, 'the bit map moved in a step that had nothing to flush')
      elif moved:
        self.need(m.mode[h] == 1, f'a flush re-laid the handle out, its relayout mode is {m.mode[h]}')
        self.check.relaid += 1
      self.need({x for x, p in enumerate(bm) if p >= nloc} == set(m.held[h]), 'the held bits changed')
      self.check_ptr(h)
      # -- the plan, held to the bit map by the rule stated in Python ------------------------------------------------------------------
      want_plan = pauli_product_rule(nloc, bw, bm, self.shard[h], xs, zs)
      self.need((terms, runs) == want_plan, f'qh_pauli_product_plan says {(terms, runs)}, the rule on bit map {bm} gives {want_plan}')
      if quiet:
        self.need(plan0 == (terms, runs), 'the plan asked before a quiet call differs from the plan asked behind it')
      # -- stats of a quiet step, as the header gives them from the plan ----------------------------------------------------------------
      sb = (1 << nloc) * (16 if bw == 128 else 8)
      if quiet:
        grow = {'gates_submitted': nt, 'kernels_launched': len(runs), 'bytes_swept': 2 * len(runs) * sb, 'bytes_algorithmic': 2 * len(runs) * sb}
        for k in stats0:
          self.need(stats1[k] - stats0[k] == grow.get(k, 0), f'{k} grew by {stats1[k] - stats0[k]}, the header says {grow.get(k, 0)} ({len(runs)} runs)')
      # -- amplitudes ---------------------------------------------------------------------------------------------------------------------
      after = self.read(h)
      self.need(_bitmap(st) == bm, 'reading the handle through a clone moved its bit map')
      want = m.wide(h)                                        # np_pauli_product of what the handle held
      amax = float(np.max(np.abs(before)))
      bound = ppu.bound(bw, a, b, amax, len(runs))
      if not quiet:
        bound += mag * amp_tol(bw)                            # the burst's own rounding passes through the factors and grows by at most M
      bps = [pauli_coef(b[t['index']], t['ny'], t['neg']) for t in terms]
      unit = pauli_unit(bps[0]) if nt == 1 and complex(a[0]) == 0 else None
      ident = nt == 1 and complex(a[0]) == 1 and complex(b[0]) == 0
      signs = lambda got, exp: int(np.sum(np.signbit(got.view(np.float64)) != np.signbit(exp.view(np.float64))))      # noqa: E731
      if quiet and nt == 0:
        self.need(after.tobytes() == before.tobytes(), 'no terms: the amplitudes changed')
      elif quiet and unit is not None:                        # the stored bits moved: the same bytes, the sign of a zero included
        exp = np.zeros(1 << n, dtype=np.complex128)
        exp[mine] = pauli_rotated(before, n, xs[0], zs[0] & local, unit)[mine]
        self.need(after.tobytes() == exp.tobytes(), f'one string with a == 0 and b\' = i^{unit}: not the stored bits moved '
                  f'(max diff {float(np.max(np.abs(after - exp))):.3e}, {signs(after, exp)} signs differ)')
      elif quiet and ident:
        self.need(after.tobytes() == before.tobytes(), f'the factor (1, 0): not every bit as it was (max diff '
                  f'{float(np.max(np.abs(after - before))):.3e}, {signs(after, before)} signs differ)')
      else:
        err = float(max(np.max(np.abs(after.real - want.real)), np.max(np.abs(after.imag - want.imag))))
        self.need(err <= bound, f'amplitudes off by {err:.3e} per component (bound {bound:.3e}, {len(runs)} runs, M = {mag:.3g})')
      m.put(h, after)
      self.check_raw(h, after, bm)
      # -- norm2 --------------------------------------------------------------------------------------------------------------------------
      if s['norm']:
        n2_np = float(np.vdot(after, after).real)
        self.need(abs(n2 - n2_np) <= 1e-12 * n2_np, f'norm2 {n2!r}, the amplitudes read back give {n2_np!r}')
        n2_tol = 4 * mag * amax * bound * (1 << nloc) + 1e-12 * want_n2      # (as _apply_checked of tests/test_gpu_pauli_product.py)
        self.need(abs(n2 - want_n2) <= n2_tol, f'norm2 {n2!r}, the model gives {want_n2!r} (tolerance {n2_tol:.3e})')
      else:
        self.need(n2 is None, f'norm2 was not asked for, the call returned {n2!r}')
      # -- the same start again: the same bits --------------------------------------------------------------------------------------------
      if keep is not None:
        st.copy_from(keep)
        self.need(_bitmap(st) == bm, 'copy_from a clone of the handle itself moved the bit map')
        again = st.apply_pauli_product(a, b, xs, zs, norm=s['norm'])
        self.need(again == n2, f'norm2 {n2!r}, from the same call repeated {again!r}')
        self.need(_bitmap(st) == bm and _pending(st) == 0, 'the repeated call moved the bit map or queued something')
        self.need(self.read(h).tobytes() == after.tobytes(), 'the same call from the same start gave other amplitude bytes')
    finally:
      if keep is not None:
        keep.close()
    # -- the record ---------------------------------------------------------------------------------------------------------------------
    ab = 0 if bw == 128 else 1
    rec_runs = []
    for r in runs:
      tl = terms[r['first']:r['first'] + r['count']]
      one = tl[0]['index'] if r['count'] == 1 else None
      exact = None if one is None else 'string' if complex(a[one]) == 0 and pauli_unit(bps[r['first']]) is not None \
          else 'identity' if complex(a[one]) == 1 and complex(b[one]) == 0 else None
      rec_runs.append({'kind': r['kind'], 'walk': pauli_product_walk(nloc, bw, r), 'slots': 'few' if r['count'] <= PAULI_PRODUCT_FEW else 'many',
                       'exact': exact, 'flip': any(_popcount(r['px'] & t['pz']) & 1 for t in tl),
                       'mixed': any(t['px'] for t in tl) and not all(t['px'] for t in tl), 'px0': bool(ab) and bool(r['px'] & 1)})
    rec = {'nloc': nloc, 'main': pauli_product_main_shape(nloc, bw), 'nruns': len(runs), 'zero': nt == 0, 'norm': bool(s['norm']), 'runs': rec_runs,
           'shard': bool(m.held[h]), 'held_z': any((z >> hb) & 1 for z in zs for hb in m.held[h]), 'neg': any(t['neg'] for t in terms),
           'queued': not quiet, 'relayout_on': m.mode[h] == 1, 'relaid': not quiet and moved and not _canonical(bm, nloc),
           'fixed': h in self.fixed_ptr, 'pz0': bool(ab) and any(t['pz'] & 1 for t in terms)}
    self.check.events.append((self.i, 'pauli_product', not _canonical(bm, nloc), not quiet, None, rec))

  # -- reduced densities and Z-polynomials: the frame the three steps share -----------------------------------------------------------
  def _behind(self, h, queued, bm_before, what):
    """behind a call that runs what is queued and leaves the layout as it finds it: nothing pending, the bit map moved only by a
    flush whose relayout mode is on, the held bits and the pointer as before.  Returns (bit map, moved)."""
    st, m = self.dev[h], self.m
    bm = _bitmap(st)
    self.need(_pending(st) == 0, f'{_pending(st)} gates pending behind {what}')
    moved = bm != bm_before
    if not queued:
      self.need(not moved, 'the bit map moved in a step that had nothing to flush')
    elif moved:
      self.need(m.mode[h] == 1, f'a flush re-laid the handle out, its relayout mode is {m.mode[h]}')
      self.check.relaid += 1
    self.need({x for x, p in enumerate(bm) if p >= st.nbits} == set(m.held[h]), 'the held bits changed')
    self.check_ptr(h)
    return bm, moved

  def _read_behind_reader(self, h, quiet, bm):
    """the amplitudes behind a reader, through a clone: as stored on a quiet step, within _amp_tol of the model behind a burst"""
    m, st = self.m, self.dev[h]
    after = self.read(h)
    self.need(_bitmap(st) == bm, 'reading the handle through a clone moved its bit map')
    w = m.wide(h)
    if quiet:
      self.need(np.array_equal(after, w), f'a reader changed the amplitudes (max diff {float(np.max(np.abs(after - w))):.3e})')
    else:
      err = float(np.max(np.abs(after - w)))
      self.need(err <= amp_tol(self.bw), f'behind its queue: amplitudes off by {err:.3e} (limit {amp_tol(self.bw):.1e})')      # _amp_tol
    m.put(h, after)
    self.check_raw(h, after, bm)
    return after

  def _stats_grew(self, stats0, stats1, grow, what):
    for k in stats0:
      self.need(stats1[k] - stats0[k] == grow.get(k, 0), f'{k} grew by {stats1[k] - stats0[k]}, the header says {grow.get(k, 0)} for {what}')

  def _ratio(self, family, err, bound):
    """the largest error seen as a fraction of its bound, per family (HISTORY.md T5 records it)"""
    r = float(np.max(np.where(bound > 0, err / np.maximum(bound, 1e-300), np.where(err > 0, np.inf, 0.0))))
    self.check.ratios[family] = max(self.check.ratios.get(family, 0.0), r)

  def run_reduced_density(self, s, queued, bm_before):
    """One 'reduced_density' step: a reader on h in whatever condition the program left it.  The matrix is held to
    density_util.np_reduced_density of the amplitudes read back behind the step, within density_util.tolerance."""
    m, bw = self.m, self.bw
    h, st, bits = s['h'], self.dev[s['h']], s['bits']
    k, n, nloc = len(bits), m.n[h], st.nbits
    quiet = queued == 0
    stats0 = st.stats()
    try:
      rho = st.reduced_density(bits)
    except native.QhError as e:
      self.fail(f'the engine refused a valid step: {e}')
    stats1 = st.stats()
    plan = density_plan_view(st.density_plan(bits))          # right behind the call: the layout the call's own flush left
    for mdl in (m, self.chain, self.chain_r):
      if mdl is not None:
        mdl.run(h)
    bm, moved = self._behind(h, queued, bm_before, 'a reduced density')
    # -- the plan, held to the bit map by the rule stated in Python ------------------------------------------------------------------
    want_plan = density_rule(nloc, bm, bits)
    self.need(plan == want_plan, f'qh_density_plan says {plan}, the rule on bit map {bm} gives {want_plan}')
    # -- stats of a quiet step: one kernel (the fold is not counted), the shard once, the bytes the kernel requests -----------------
    ab = 16 if bw == 128 else 8
    if quiet:
      self._stats_grew(stats0, stats1, {'kernels_launched': 1, 'bytes_algorithmic': (1 << nloc) * ab, 'bytes_swept': want_plan['amps_swept'] * ab},
                       'a reduced density')
    # -- the state: unchanged ------------------------------------------------------------------------------------------------------------
    after = self._read_behind_reader(h, quiet, bm)
    # -- the matrix ------------------------------------------------------------------------------------------------------------------------
    self.need(rho.shape == (1 << k, 1 << k) and rho.dtype == np.complex128, f'the result has shape {rho.shape} and type {rho.dtype}')
    psi, number = local_view(after, n, m.held[h])
    want = du.np_reduced_density(psi, [number[b] for b in bits])
    tol = du.tolerance(want, 1 << (nloc - k))
    err = np.abs(rho - want)
    self._ratio('reduced_density', err, tol)
    self.need(bool(np.all(err <= tol)), f'rho off by up to {float(np.max(err / np.maximum(tol, 1e-300))):.3g} x density_util.tolerance '
              f'(max error {float(np.max(err)):.3e}, k = {k}, {plan["block_pairs"]} block pairs, path {plan["path"]})')
    # -- bit for bit: one triangle mirrored, a real diagonal ----------------------------------------------------------------------------------
    off = ~np.eye(1 << k, dtype=bool)
    self.need(rho.real.tobytes() == np.ascontiguousarray(rho.real.T).tobytes() and rho.imag[off].tobytes() == (-rho.imag.T)[off].tobytes(),
              'rho[c][r] is not the bitwise conjugate of rho[r][c]')
    d = np.diag(rho)
    self.need(bool(np.all(d.imag == 0.0)) and not np.any(np.signbit(d.imag)), 'a diagonal imaginary part is not 0.0')
    # -- the diagonal against marginal on the same bits, the trace against norm2 (k = 0: the norm itself) ------------------------------------
    # (the bound holds each of two sums of m products to the exact value: rho_rr and the marginal, which sums the same m
    # probabilities in another order, are each within it, so they lie within twice the bound of each other)
    dtol = np.diag(tol)
    p = st.marginal(bits)
    self.need(bool(np.all(np.abs(d.real - p) <= 2 * dtol)),
              f'the diagonal differs from marginal on the same bits by up to {float(np.max(np.abs(d.real - p))):.3e}')
    n2 = st.norm2()
    self.need(abs(float(np.sum(d.real)) - n2) <= float(np.sum(dtol)) + TOL * n2,      # (+ TOL: norm2 and this sum of the diagonal round on their own)
              f'the trace {float(np.sum(d.real))!r} differs from norm2 {n2!r}')
    if quiet:
      self.need(st.reduced_density(bits).tobytes() == rho.tobytes(), 'two calls on the same state and layout, two answers')
    self.need(_bitmap(st) == bm and _pending(st) == 0, 'the readers behind the step moved the bit map or queued something')
    # -- the record ---------------------------------------------------------------------------------------------------------------------
    rows = plan['row_pos']
    rec = {'nloc': nloc, 'k': k, 'path': plan['path'], 'tile_bits': plan['tile_bits'], 'chunk_bits': plan['chunk_bits'], 'nrest': plan['nrest'],
           'block_pairs': plan['block_pairs'], 'chunks_per_wg': plan['chunks_per_wg'], 'row_identity': plan['row_bit'] == list(range(k)),
           'pos0': 0 in rows, 'pos01': 0 in rows and 1 in rows, 'queued': not quiet, 'relayout_on': m.mode[h] == 1,
           'relaid': not quiet and moved and not _canonical(bm, nloc), 'shard': bool(m.held[h]), 'fixed': h in self.fixed_ptr,
           'fresh': self.fresh.get(h)}
    self.check.events.append((self.i, 'reduced_density', not _canonical(bm, nloc), not quiet, None, rec))

  def _zpoly_record(self, s, plan, quiet, moved, bm):
    m, bw, h = self.m, self.bw, s['h']
    nloc = self.dev[h].nbits
    main = plan['kernel'] == native.QH_ZPOLY_KERNEL_MAIN
    segs = zpoly_segments(plan) if main else []
    kinds = [zpoly_group_kind(g, bw) for g in plan['group_mask']] if main else []
    return {'nloc': nloc, 'main': main, 'nterms': plan['nterms'], 'classes': sorted({ZPOLY_CLASSES[c] for c in plan['cls']}) if main else [],
            'group_kinds': {kd: kinds.count(kd) for kd in ZPOLY_GROUP_KINDS}, 'seg_over_64': any(c > ZPOLY_LANES for c in segs),
            'seg_2_to_63': any(2 <= c < ZPOLY_LANES for c in segs), 'duplicates': len(set(s['z'])) < len(s['z']),
            'pz0': bw == 64 and any(z & 1 for z in plan['pz']), 'c': zpoly_c_kind(s['c']) if 'c' in s else None, 'norm': s.get('norm'),
            'shard': bool(m.held[h]), 'neg_held': any(a != float(b) and (a or b) for a, b in zip(plan['w'], s['w'])),
            'queued': not quiet, 'relayout_on': m.mode[h] == 1, 'relaid': not quiet and moved and not _canonical(bm, nloc),
            'fixed': h in self.fixed_ptr}

  def _zpoly_plan(self, st, s, bm, h):
    """qh_zpoly_plan right now, held to the rule on the bit map"""
    plan = st.zpoly_plan(s['w'], s['z'])
    want = zpoly_rule(st.nbits, self.bw, bm, self.shard[h], s['w'], s['z'])
    self.need(plan == want, f'qh_zpoly_plan differs from the rule on bit map {bm} in {[k for k in want if plan.get(k) != want[k]]}: '
              f'{ {k: plan.get(k) for k in want if plan.get(k) != want[k] and k not in ("pz", "w", "cls")} }')
    return plan

  def run_expect_zpoly(self, s, queued, bm_before):
    """One 'expect_zpoly' step: a reader; the three sums are held to zpoly_util.np_moments of the amplitudes read back behind the
    step at the global logical indices the shard holds, within zpoly_util.moment_bound"""
    m, bw = self.m, self.bw
    h, st, ws, zs = s['h'], self.dev[s['h']], s['w'], s['z']
    nt, n, nloc = len(zs), m.n[h], st.nbits
    quiet = queued == 0
    stats0 = st.stats()
    try:
      got = st.expect_zpoly(ws, zs)
    except native.QhError as e:
      self.fail(f'the engine refused a valid step: {e}')
    stats1 = st.stats()
    for mdl in (m, self.chain, self.chain_r):
      if mdl is not None:
        mdl.run(h)
    bm, moved = self._behind(h, queued, bm_before, 'expect_zpoly')
    plan = self._zpoly_plan(st, s, bm, h)                    # right behind the call: the layout the call's own flush left
    sb = (1 << nloc) * (16 if bw == 128 else 8)
    if quiet:                                                # one kernel and one read of the shard; no terms: the reader norm2, which counts nothing
      self._stats_grew(stats0, stats1, {'kernels_launched': 1, 'bytes_swept': sb, 'bytes_algorithmic': sb} if nt else {}, f'expect_zpoly of {nt} terms')
    after = self._read_behind_reader(h, quiet, bm)
    mine = mine_of(n, m.held[h]).astype(np.int64)
    want = zu.np_moments(after[mine], ws, zs, f=zpoly_f(n, m.held[h], ws, zs))
    self.need(len(got) == 3, f'expect_zpoly returned {got!r}')
    for k in range(3):
      bound = zu.moment_bound(ws, k, want[0])
      err = abs(got[k] - want[k])
      self._ratio(f'expect_zpoly moment {k}', np.float64(err), np.float64(bound))
      self.need(err <= bound, f'moment {k}: {got[k]!r}, the model gives {want[k]!r}: off by {err:.3e} (zpoly_util.moment_bound {bound:.3e}, {nt} terms)')
    if nt == 0:
      n2 = st.norm2()
      self.need((got[1], got[2]) == (0.0, 0.0) and got[0] == n2, f'no terms: {got!r}, norm2 called next gives {n2!r}')
    if quiet:
      again = st.expect_zpoly(ws, zs)
      self.need(tuple(again) == tuple(got), f'two calls on the same state and layout, two answers: {got!r}, {again!r}')
    self.need(_bitmap(st) == bm and _pending(st) == 0, 'the readers behind the step moved the bit map or queued something')
    self.check.events.append((self.i, 'expect_zpoly', not _canonical(bm, nloc), not quiet, None, self._zpoly_record(s, plan, quiet, moved, bm)))

  def run_zpoly(self, s, queued, bm_before):
    """One 'zpoly' step, in place on h in whatever condition the program left it: every check of _apply_checked of
    tests/test_gpu_zpoly.py and those of run_pauli_product that apply.  On a QUIET step the plan is asked before the call too, the
    stats are held exactly and the call is repeated from the same start (restored from a clone)."""
    m, bw = self.m, self.bw
    h, st, ws, zs, c = s['h'], self.dev[s['h']], s['w'], s['z'], complex(s['c'])
    nt, n, nloc = len(zs), m.n[h], st.nbits
    quiet = queued == 0
    noop = nt == 0 or c == 0                                 # flushes and launches nothing; norm2 is then qh_norm2's
    mine = mine_of(n, m.held[h]).astype(np.int64)
    plan0 = self._zpoly_plan(st, s, bm_before, h) if quiet else None      # asked right before the call
    keep = st.clone() if quiet and not noop else None        # the start, for the repeat
    try:
      stats0 = st.stats()
      try:
        n2 = st.apply_zpoly(ws, zs, c, norm=s['norm'])
      except native.QhError as e:
        self.fail(f'the engine refused a valid step: {e}')
      stats1 = st.stats()
      m.run(h)
      before = m.wide(h)                                     # quiet: what the handle held, bit for bit; else the model behind the burst
      want_n2 = m.step(s)
      for mdl in (self.chain, self.chain_r):
        if mdl is not None:
          mdl.step(s)
      bm, moved = self._behind(h, queued, bm_before, 'a Z-polynomial')
      plan = self._zpoly_plan(st, s, bm, h)                  # right behind the call: the layout the call's own flush left
      if quiet:
        self.need(plan0 == plan, 'the plan asked before a quiet call differs from the plan asked behind it')
      sb = (1 << nloc) * (16 if bw == 128 else 8)
      if quiet:
        grow = {} if noop else {'gates_submitted': 1, 'kernels_launched': 1, 'bytes_swept': 2 * sb, 'bytes_algorithmic': 2 * sb}
        self._stats_grew(stats0, stats1, grow, f'apply_zpoly of {nt} terms with c = {c}')
      # -- amplitudes ---------------------------------------------------------------------------------------------------------------------
      after = self.read(h)
      self.need(_bitmap(st) == bm, 'reading the handle through a clone moved its bit map')
      want = m.wide(h)                                       # zpoly_util.np_apply of what the handle held
      amax = float(np.max(np.abs(before)))
      big_e = float(np.exp(abs(c.real) * zu.big_f(ws)))      # E
      bound = zu.apply_bound(bw, ws, c, amax)
      if not quiet:
        bound += big_e * amp_tol(bw)                         # the burst's own rounding passes through the factor and grows by at most E
      if quiet and noop:
        self.need(after.tobytes() == before.tobytes(), 'no terms or c == (0, 0): the amplitudes changed')
      else:
        err = float(max(np.max(np.abs(after.real - want.real)), np.max(np.abs(after.imag - want.imag))))
        self._ratio('zpoly' if quiet else 'zpoly behind a burst', np.float64(err), np.float64(bound))
        self.need(err <= bound, f'amplitudes off by {err:.3e} per component (bound {bound:.3e}, {nt} terms, E = {big_e:.3g})')
      self.need(not np.any(after[np.setdiff1d(np.arange(1 << n), mine)]), 'amplitudes another shard holds are not zero in what was read')
      m.put(h, after)
      self.check_raw(h, after, bm)
      # -- norm2 --------------------------------------------------------------------------------------------------------------------------
      if s['norm']:
        n2_np = float(np.vdot(after, after).real)
        self.need(abs(n2 - n2_np) <= TOL * n2_np, f'norm2 {n2!r}, the amplitudes read back give {n2_np!r}')
        # against the model: every component within `bound` of the model's, so |sum |got|^2 - sum |want|^2| <= sum (2 |want_i| d + d^2)
        # with d = sqrt(2) bound per amplitude, and sum |want_i| <= sqrt(N want_n2) (Cauchy-Schwarz); + the reader's own TOL
        size = float(1 << nloc)
        n2_tol = 2 * np.sqrt(2.0) * bound * np.sqrt(size * want_n2) + 2 * bound * bound * size + TOL * want_n2
        self.need(abs(n2 - want_n2) <= n2_tol, f'norm2 {n2!r}, the model gives {want_n2!r} (tolerance {n2_tol:.3e})')
        if noop:
          nr = st.norm2()
          self.need(n2 == nr, f'no terms or c == (0, 0): norm2 {n2!r}, qh_norm2 gives {nr!r}')
      else:
        self.need(n2 is None, f'norm2 was not asked for, the call returned {n2!r}')
      # -- the same start again: the same bits --------------------------------------------------------------------------------------------
      if keep is not None:
        st.copy_from(keep)
        self.need(_bitmap(st) == bm, 'copy_from a clone of the handle itself moved the bit map')
        again = st.apply_zpoly(ws, zs, c, norm=s['norm'])
        self.need(again == n2, f'norm2 {n2!r}, from the same call repeated {again!r}')
        self.need(_bitmap(st) == bm and _pending(st) == 0, 'the repeated call moved the bit map or queued something')
        self.need(self.read(h).tobytes() == after.tobytes(), 'the same call from the same start gave other amplitude bytes')
    finally:
      if keep is not None:
        keep.close()
    self.check.events.append((self.i, 'zpoly', not _canonical(bm, nloc), not quiet, None, self._zpoly_record(s, plan, quiet, moved, bm)))

  def perm_record(self, s, queued, bm_before):
    """What qh_perm_plan says of the step's bits right behind the call: the call does not move the bit map, so this is the
    layout it worked on (the one its own flush left).  The plan is held to the bit map by the tile rule."""
    h, st, m = s['h'], self.dev[s['h']], self.m
    plan, bm = st.perm_plan(s['bits'], s['ctl']), _bitmap(st)
    want = perm_tiles(st.nbits, self.bw, bm, self.shard[h], s['bits'], s['ctl'])
    got = {k: (list(plan[k])[:len(s['bits'])] if k == 'reg_pos' else int(plan[k])) for k in want}
    self.need(got == want, f'qh_perm_plan says {got}, the tile rule on bit map {bm} gives {want}')
    ctl_held = sum(1 << b for b in m.held[h] if (s['ctl'] >> b) & 1)
    return {'k': len(s['bits']), 'nloc': st.nbits, 'band': perm_band(len(s['bits']), self.bw), 'path': want['path'],
            'tile_bits': want['tile_bits'], 'ctl_met': want['ctl_met'], 'ctl_local': bool(s['ctl'] & ~ctl_held), 'ctl_held': bool(ctl_held),
            'shard': bool(m.held[h]), 'held_inside': bool(m.held[h]) and min(m.held[h]) < m.n[h] - len(m.held[h]),
            'relayout_on': m.mode[h] == 1, 'relaid': bool(queued) and bm != bm_before and not _canonical(bm, st.nbits), 'stats': st.stats()}

  def results(self, s, got, want, after, bm_after):
    op, h, bw, st = s['op'], s['h'], self.bw, self.dev[s['h']]
    if op in ('norm2', 'prob_bit', 'marginal'):
      miss = close(got, want, bw)                           # _close
      self.need(miss is None, f'{op}: {miss}')
      if op == 'marginal':
        self.need(st.marginal(s['bits']).tobytes() == np.asarray(got).tobytes(), 'marginal: two calls, two answers')
    elif op == 'expect':
      err = float(np.max(np.abs(got - want))) if len(want) else 0.0
      # TOL of tests/test_gpu_inner.py is for normalised states; a program's norms lie in [0.25, 4] and these sums are
      # quadratic in the amplitudes, so the bound is TOL times the norm where that is above 1 (at most 4e-12)
      self.need(err < TOL * max(1.0, self.m.norm(h)), f'expect_pauli off by {err:.3e}')
      self.need(st.expect_pauli(s['x'], s['z']).tobytes() == got.tobytes(), 'expect_pauli: two calls, two answers')
    elif op == 'inner':
      err = abs(got - want)
      scale = max(1.0, float(np.sqrt(self.m.norm(h) * self.m.norm(s['other']))))      # (TOL scaled as for expect_pauli)
      self.need(err < TOL * scale, f'inner off by {err:.3e}')
      if s['other'] == h:
        self.need(got.imag == 0.0, f'inner(a, a) has imaginary part {got.imag!r}')
      again = st.inner(self.dev[s['other']])
      self.need((again.real, again.imag) == (got.real, got.imag), 'inner: two calls, two answers')
    elif op == 'argmax':
      mine, _, p = self.m._probs(h)
      top = float(p.max())
      where = np.flatnonzero(mine == np.uint64(got[0]))
      eps = 1e-6 if bw == 64 else 4e-16                     # tools/fuzz_parity.py's argmax rule
      self.need(where.size == 1 and p[where[0]] >= top * (1 - eps) - 1e-300 and abs(got[1] - top) <= eps * top + 1e-300,
                f'argmax {got}, the largest probability is {top!r} at {want[0]}')
    elif op == 'amplitude':
      self.need(got == want, f'amplitude {got!r}, stored {want!r}')
    elif op == 'amplitudes':
      self.need(np.array_equal(got, want), 'amplitudes: entries differ from what is stored')
    elif op == 'select':
      idx, amp, cnt, w = got
      self.need(cnt == want[2], f'select: count {cnt}, expected {want[2]}')
      self.need(np.array_equal(idx, want[0]) and np.array_equal(amp, want[1]), 'select: entries differ (ascending logical index, as stored)')
      miss = close(w, want[3], bw)                          # _close
      self.need(miss is None, f'select: weight {miss}')
      self.need(st.select(s['threshold'], cap=0)[3] == w, 'select: two calls, two weights')
    elif op == 'topk':
      self.need(np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]),
                f'topk: indices {got[0][:8].tolist()}..., expected {want[0][:8].tolist()}...')
    elif op == 'sample':
      nloc = st.nbits
      lidx = _logical_index(bm_after[h], self.shard[h], nloc)
      a = after[h][lidx]
      pp = a.real ** 2 + a.imag ** 2                        # physical order
      inv = np.full(1 << self.m.n[h], -1, dtype=np.int64)
      inv[lidx] = np.arange(lidx.size)
      g = inv[np.asarray(got, dtype=np.int64)]
      self.need(bool(np.all(g >= 0)), 'sample: an index another shard holds')
      try:
        shard_util.check_exact_cdf(pp, g, np.asarray(s['u']))
      except AssertionError as e:
        self.fail(f'sample: not the inverse CDF in physical order {e}')

  # -- the whole program ---------------------------------------------------------------------------------------------------------
  def run(self):
    try:
      for self.i, self.s in enumerate(self.prog):
        if self.s['op'] == 'init':
          self.do_init(self.s)
        else:
          self.run_step(self.s)
          self.note(self.s)
      self.finish()
    finally:
      for st in self.dev.values():
        st.close()
      self.dev = {}

  def finish(self):
    """the chain: every live handle's OWN download against a model that never looked at the device"""
    self.i, self.s = len(self.prog), {'op': 'final download', 'h': None}
    err = d = 0.0
    for h in sorted(self.dev):
      self.chain.run(h)
      got = self.own_download(h)
      self.check_ptr(h, always=True)
      self.need(got.tobytes() == self.m.wide(h).tobytes() if self.m.q[h] == 0 else True,
                f'handle {h}: its own download differs from what its clone gave')
      w = self.chain.wide(h)
      if np.all(np.isfinite(w)):
        err = max(err, float(np.max(np.abs(got - w))))
        if self.chain_r is not None:
          d = max(d, float(np.max(np.abs(self.chain_r.wide(h) - w))))
      else:
        self.need(np.array_equal(np.isfinite(got), np.isfinite(w)), f'handle {h}: NaN where the model has numbers')
    # complex128: tools/fuzz_parity.py's bound.  complex64: d = how far the same program drifts on the CPU when the state is
    # rounded to complex64 after every gate and every step (the per-gate engine's worst case); the engine may order its
    # roundings differently, never more often per gate: max(_amp_tol(64), 4 d)
    tol = CHAIN_TOL_128 if self.bw == 128 else max(amp_tol(64), 4 * d)
    self.check.chain_err, self.check.chain_d, self.check.chain_tol = err, d, tol
    print(f'chain: bw={self.bw} nloc0={self.check.nloc0} steps={len(self.prog) - 1} d={d:.3e} gpu_err={err:.3e} tol={tol:.3e}')
    self.need(err <= tol, f'chain: the final states are off by {err:.3e} (limit {tol:.3e}, d = {d:.3e})')


def run_program(program, make_state, check):
  """Runs `program` on handles made by make_state(nloc, bw, kind) (kind 'own' | 'attached' | 'mapped'; fused: gates queue)
  and holds every step to the model.  Raises StepFailure (an AssertionError that names the step)."""
  _Runner(program, make_state, check).run()
  return check


def make_device_state(nloc, bw, kind):
  """make_state for the real engine: a fused qcc_amd.device.DeviceState that owns HBM memory ('own'), works on a torch
  allocation ('attached') or on pinned host memory ('mapped'); raw_view reads the caller's memory without the engine"""
  from qcc_amd import device  # pylint: disable=import-outside-toplevel
  dt = np.complex128 if bw == 128 else np.complex64
  if kind == 'mapped':
    st = device.DeviceState(nloc, bw, fusion=native.QH_FUSE_SWEEP, host_mapped=True)
    st.raw_view = lambda: np.array(st.host_array())
    return st
  if kind == 'attached':
    import torch  # pylint: disable=import-outside-toplevel
    buf = torch.zeros(2 << nloc, dtype=torch.float64 if bw == 128 else torch.float32, device='cuda')
    torch.cuda.synchronize()
    st = device.DeviceState(nloc, bw, fusion=native.QH_FUSE_SWEEP, device_ptr=buf.data_ptr())
    st.raw_view = lambda: buf.cpu().numpy().view(dt)        # (the allocation lives as long as the handle object)
    return st
  return device.DeviceState(nloc, bw, fusion=native.QH_FUSE_SWEEP)


# ---- the NumPy stand-in ---------------------------------------------------------------------------------------------------------
class NumpyDevice:
  """DeviceState's interface on a physical array, a bit map (physical position of every logical bit) and a gate queue per
  handle.  Operations run the model's functions on the logical vector and store the result back through the bit map.  A flush
  of a queue on >= PERMUTED_FROM local bits re-lays the local bits out pseudo-randomly, standing in for relayout sweeps
  (handles that own their memory and have not been told set_relayout(0))."""
  _serial = [0]

  def __init__(self, nbits, bit_width=128, kind='own'):
    self.nbits = self.nbits_global = int(nbits)
    self.bit_width = bit_width
    self.dtype = np.complex128 if bit_width == 128 else np.complex64
    self.phys = np.zeros(1 << nbits, dtype=self.dtype)
    self.bm = list(range(nbits))
    self.shard = 0
    self.queue = []
    self.kind = kind
    self.relayout = -1                                     # undecided: the first fused flush decides (attached / mapped: off)
    self.kernels = self.submitted = self.noop = 0          # (submitted / noop: counted for apply_perm only)
    self.swept = self.algorithmic = 0                      # (bytes: counted for apply_pauli_sum only)
    NumpyDevice._serial[0] += 1
    self.device_ptr = 0x1000 * NumpyDevice._serial[0]
    self.rng = np.random.default_rng(NumpyDevice._serial[0])

  # -- plumbing ----------------------------------------------------------------------------------------------------------------
  def _lidx(self):
    return _logical_index(self.bm, self.shard, self.nbits)

  def to_logical(self):
    out = np.zeros(1 << self.nbits_global, dtype=np.complex128)
    out[self._lidx()] = self.phys
    return out

  def store(self, vec):
    self.phys = np.asarray(vec)[self._lidx()].astype(self.dtype)

  def held(self):
    return {b: (self.shard >> (p - self.nbits)) & 1 for b, p in enumerate(self.bm) if p >= self.nbits}

  def _move_local(self, new_pos):
    """local logical bit b goes to position new_pos[b]; the data follows"""
    vec = self.to_logical()
    for b, p in new_pos.items():
      self.bm[b] = p
    self.store(vec)

  def _canonicalize(self):
    loc = [b for b in range(self.nbits_global) if self.bm[b] < self.nbits]
    if [self.bm[b] for b in loc] != sorted(self.bm[b] for b in loc):
      self._move_local(dict(zip(loc, sorted(self.bm[b] for b in loc))))

  def bitmap(self):
    return list(self.bm)

  def pending_gates(self):
    return len(self.queue)

  def stats(self):
    return {'kernels_launched': self.kernels, 'gates_submitted': self.submitted, 'gates_noop': self.noop,
            'bytes_swept': self.swept, 'bytes_algorithmic': self.algorithmic}

  def host_array(self):
    if not hasattr(self, '_host'):
      self._host = np.empty(1)                             # (its address stands for the host pointer: a constant)
    return self._host

  def close(self):
    self.phys = None

  def set_shard(self, nbits_global, shard_index):
    self.nbits_global, self.shard = int(nbits_global), int(shard_index)
    self.bm = list(range(self.nbits_global))

  def flush(self):
    if not self.queue:
      return
    q, self.queue = self.queue, []
    vec = self.to_logical().astype(self.dtype)
    for cm, t, g in q:
      apply_gate(vec, self.nbits_global, cm, t, g)
    self.kernels += 1
    self.store(vec)
    if self.relayout < 0 and self.nbits >= SWEEPS_FROM:
      self.relayout = int(self._eligible())
    if self.nbits >= PERMUTED_FROM and self.relayout == 1:
      loc = [b for b in range(self.nbits_global) if self.bm[b] < self.nbits]
      self._move_local(dict(zip(loc, self.rng.permutation([self.bm[b] for b in loc]).tolist())))

  sync = flush

  def _eligible(self):
    return self.kind == 'own' and int(os.environ.get('QH_RELAYOUT', '1')) != 0 and self.nbits >= SWEEPS_FROM

  def plans_relayout(self):
    want = self._eligible() if self.relayout < 0 else self.relayout == 1
    return bool(self.queue) and want

  @property
  def raw_view(self):
    return (lambda: self.phys) if self.kind != 'own' else None

  def set_relayout(self, on):
    if on:
      if self.relayout != 1:
        self.relayout = int(self._eligible())
    else:
      self.flush()
      self._canonicalize()
      self.relayout = 0
    return self.relayout == 1

  def remap_swap(self, a, b):
    self.flush()
    la, lb = self.bm.index(a), self.bm.index(b)
    self.bm[la], self.bm[lb] = self.bm[lb], self.bm[la]

  # -- initialisation / IO -------------------------------------------------------------------------------------------------------
  def _fresh(self):
    self.queue = []
    if self.nbits_global == self.nbits:
      self.bm = list(range(self.nbits))

  def init_basis(self, index=0):
    self._fresh()
    v = np.zeros(1 << self.nbits_global, dtype=np.complex128)
    v[index] = 1
    self.store(v)

  def init_product(self, factors):
    self._fresh()
    self.store(init_vector({'how': 'product', 'factors': factors, 'nloc': self.nbits_global, 'g': 0}))

  def upload(self, host, offset=0):
    assert offset == 0
    self._fresh()
    self._canonicalize()
    self.phys = np.asarray(host).astype(self.dtype).copy()

  def download(self, offset=0, count=None, out=None):
    self.flush()
    self._canonicalize()
    return self.phys.copy()

  # -- gates and barrier mutators --------------------------------------------------------------------------------------------------
  def apply_bits(self, ctl_mask, tgt_bit, gate):
    self.queue.append((int(ctl_mask), int(tgt_bit), np.asarray(gate, dtype=np.complex128).reshape(4)))

  def _barrier(self, fn, kernels=1):
    self.flush()
    self.store(fn(self.to_logical()))
    self.kernels += kernels

  def apply_matrix(self, matrix, bits, ctl_mask=0):
    bits = [int(b) for b in bits]
    if len(set(bits)) != len(bits) or any((ctl_mask >> b) & 1 for b in bits):
      raise native.QhError(native.QH_ERR_SAME_QUBIT, 'apply_matrix: a bit twice')
    self._barrier(lambda v: dense_reference(v, self.nbits_global, np.asarray(matrix, dtype=np.complex128), bits, ctl_mask))

  def _sel(self, sel_bits):
    return [int(b) for b in sel_bits]

  def apply_mux(self, gates, sel_bits, tgt_bit):
    sel = self._sel(sel_bits)
    if len(set(sel)) != len(sel) or tgt_bit in sel:
      raise native.QhError(native.QH_ERR_SAME_QUBIT, 'apply_mux: the target among the selectors')
    self._barrier(lambda v: mux_reference_fast(v, self.nbits_global, gates, sel, tgt_bit))

  def apply_diag(self, values, bits):
    self._barrier(lambda v: diag_reference(v, self.nbits_global, values, [int(b) for b in bits]))

  def perm_plan(self, bits, ctl_mask=0):
    return perm_tiles(self.nbits, self.bit_width, self.bm, self.shard, [int(b) for b in bits], int(ctl_mask))

  def apply_perm(self, table, bits, ctl_mask=0):
    bits, ctl_mask, table = [int(b) for b in bits], int(ctl_mask), np.asarray(table, dtype=np.int64)
    if len(set(bits)) != len(bits) or any((ctl_mask >> b) & 1 for b in bits):
      raise native.QhError(native.QH_ERR_SAME_QUBIT, 'apply_perm: a bit twice, or a control in the register')
    if any(self.bm[b] >= self.nbits for b in bits):
      raise native.QhError(native.QH_ERR_NONLOCAL, 'apply_perm: a register bit held by the shard index')
    if not np.array_equal(np.sort(table), np.arange(1 << len(bits))):
      raise native.QhError(native.QH_ERR_ARG, 'apply_perm: not a bijection')
    met, mask = self._perm_controls(ctl_mask)
    self.submitted += 1
    if not met:                                            # a barrier all the same: the queue runs, then nothing
      self.flush()
      self.noop += 1
      self.kernels += self._perm_noop_kernels()
      return
    self._barrier(lambda v: self._perm_apply(v, table, bits, mask))
    self._perm_layout()

  def _perm_controls(self, ctl_mask):
    """(are the controls the shard index holds all 1 here, the mask to apply: on the vector of the global size the whole mask)"""
    return all(v for b, v in self.held().items() if (ctl_mask >> b) & 1), ctl_mask

  def _perm_apply(self, vec, table, bits, ctl_mask):
    return perm_reference(vec, self.nbits_global, table, bits, ctl_mask)

  def _perm_noop_kernels(self):
    return 0

  def _perm_layout(self):
    pass

  def scale(self, z):
    self._barrier(lambda v: v * complex(z))

  def project_bit(self, logical_bit, value):
    self.project_bits(1 << logical_bit, value << logical_bit)

  def project_bits(self, mask, value):
    self._barrier(lambda v: np.where(np_keep(v.size, mask, value), v, 0))

  # -- readers -------------------------------------------------------------------------------------------------------------------
  def _read(self, kernels=1):
    self.flush()
    self.kernels += kernels
    return self.to_logical()

  def _model(self, vec=None):
    m = ModelState()
    m.put(0, self._read(0) if vec is None else vec, self.nbits_global, self.held())
    return m

  def norm2(self):
    return self._model(self._read()).norm(0)

  def prob_bit(self, logical_bit, value=1):
    return self._model(self._read())._prob_bit({'h': 0, 'bit': logical_bit, 'value': value})

  def marginal(self, bits):
    bits = [int(b) for b in bits]
    if len(set(bits)) != len(bits):
      raise native.QhError(native.QH_ERR_SAME_QUBIT, 'marginal: a bit twice')
    return self._marginal(self._read(), bits)

  def _marginal(self, vec, bits):
    return np_marginal(vec, bits)

  def sample(self, u):
    u = np.asarray(u, dtype=np.float64)
    if np.any(np.diff(u) < 0):
      raise native.QhError(native.QH_ERR_ARG, 'sample: u is not ascending')
    self.flush()
    self.kernels += 2
    a = self.phys.astype(np.complex128)
    p = a.real ** 2 + a.imag ** 2
    cdf = np.cumsum(p)
    i = np.minimum(np.searchsorted(cdf, u * cdf[-1], side='right'), np.flatnonzero(p)[-1])
    return self._lidx()[i].astype(np.uint64)

  def expect_pauli(self, xmasks, zmasks):
    reads = {}
    for x in xmasks:
      reads[int(x)] = reads.get(int(x), 0) + 1
    vec = self._read(sum(-(-c // 16) for c in reads.values()))
    return np.array([np_expect(vec, x, z) for x, z in zip(xmasks, zmasks)], dtype=np.float64)

  def argmax(self):
    return self._model(self._read())._argmax({'h': 0})

  def amplitude(self, logical_index):
    return self.dtype(self._read(0)[int(logical_index)])

  def amplitudes(self, indices, nlocal=False):
    return self._read(0)[np.asarray(indices, dtype=np.int64)]

  def select(self, threshold, cap=1 << 16):
    idx, amp, n, w = self._select(self._model(self._read()), threshold)
    if n > cap:
      return np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=np.complex128), n, w
    return idx, amp, n, w

  def _select(self, m, threshold):
    return m._select({'h': 0, 'threshold': threshold})

  def topk(self, k):
    return self._topk(self._model(self._read(2)), k)

  def _topk(self, m, k):
    return m._topk({'h': 0, 'k': k})

  # -- handles -------------------------------------------------------------------------------------------------------------------
  def _sibling(self, nbits, nglob, bm, vec):
    o = NumpyDevice(nbits, self.bit_width)
    o.__class__ = self.__class__                           # (a mutant's handles are mutants)
    o.nbits_global, o.shard, o.bm = nglob, self.shard, list(bm)
    o.store(vec)
    return o

  def clone(self):
    self.flush()
    o = self._sibling(self.nbits, self.nbits_global, self._clone_bitmap(), np.zeros(1 << self.nbits_global))
    o.phys = self.phys.copy()
    return o

  def _clone_bitmap(self):
    return self.bm

  def copy_from(self, other):
    if other is self:
      raise native.QhError(native.QH_ERR_ARG, 'copy: dst == src')
    other.flush()
    self._copy_queue()
    self.phys, self.bm = other.phys.copy(), list(other._clone_bitmap())

  def _copy_queue(self):
    self.queue = []

  def extend(self, nqubits, amps=None, basis=0):
    k = int(nqubits)
    if amps is None and basis >= 1 << k:
      raise native.QhError(native.QH_ERR_ARG, 'extend: basis state out of range')
    self.flush()
    f = np.zeros(1 << k, dtype=np.complex128)
    if amps is None:
      f[basis] = 1
    else:
      f[:] = amps
    self.kernels += 1
    return self._sibling(self.nbits + k, self.nbits_global + k, self._extend_bitmap(k), self._extend_vec(self.to_logical(), f))

  def _extend_vec(self, vec, f):
    return np_extend(vec, f)

  def _extend_bitmap(self, k):
    return list(range(self.nbits, self.nbits + k)) + [p if p < self.nbits else p + k for p in self.bm]

  def release(self, bits, value=0):
    bits = [int(b) for b in bits]
    if value >= 1 << len(bits):
      raise native.QhError(native.QH_ERR_ARG, 'release: value out of range')
    self.flush()
    small, kept, dropped = np_release(self.to_logical(), bits, value)
    self.kernels += 1
    return self._sibling(self.nbits - len(bits), self.nbits_global - len(bits), self._release_bitmap(bits), small), kept, dropped

  def _release_bitmap(self, bits):
    gone = sorted(self.bm[b] for b in bits)
    return [p - sum(1 for r in gone if r < p) for b, p in enumerate(self.bm) if b not in bits]

  # -- two states ------------------------------------------------------------------------------------------------------------------
  def inner_plan(self, other):
    if self.bm == other.bm:
      return {'path': LINEAR}
    return {'path': TILES if self.nbits >= 8 else GATHER}

  def inner(self, other):
    self.flush()
    other.flush()
    self.kernels += 1
    return complex(np.vdot(self.to_logical(), other.to_logical()))

  def axpby(self, alpha, other, beta, norm=False):
    if other is self:
      raise native.QhError(native.QH_ERR_ARG, 'axpby: dst == src')
    self.flush()
    other.flush()
    if not (complex(alpha) == 1 and complex(beta) == 0):
      self.store(self._axpby(self.to_logical(), alpha, other.to_logical(), beta))
      self.kernels += 1
    a = self.phys.astype(np.complex128)
    return float(np.vdot(a, a).real) if norm else None

  def _axpby(self, d, alpha, s, beta):
    return axpby_ref(d, alpha, s, beta)

  # -- Pauli-sum operators: batch by batch as the header describes them, through hooks a mutant overrides one at a time ----------
  def _pauli_check(self, who, out, xmasks, zmasks):
    if out is self:
      raise native.QhError(native.QH_ERR_ARG, f'{who}: dst == src')
    if any((x | z) >> self.nbits_global for x, z in zip(xmasks, zmasks)):
      raise native.QhError(native.QH_ERR_BAD_QUBIT, f'{who}: a mask bit >= nbits_global')
    if any((x >> b) & 1 for x in xmasks for b in self.held()):
      raise native.QhError(native.QH_ERR_NONLOCAL, f'{who}: X or Y on a bit held by the shard index')

  def pauli_sum_plan(self, xmasks, zmasks):
    xs, zs = [int(x) for x in xmasks], [int(z) for z in zmasks]
    self._pauli_check('pauli_sum_plan', None, xs, zs)
    return pauli_plan_rule(self.nbits, self.bm, self.shard, xs, zs)

  def apply_pauli_sum(self, coeffs, xmasks, zmasks, out=None, norm=False):
    cs, xs, zs = [complex(c) for c in coeffs], [int(x) for x in xmasks], [int(z) for z in zmasks]
    self._pauli_check('apply_pauli_sum', out, xs, zs)
    self._pauli_enter()
    terms, batches = self.pauli_sum_plan(xs, zs)
    if out is None:
      out = self._sibling(self.nbits, self.nbits_global, self.bm, np.zeros(1 << self.nbits_global))
    out._pauli_drop_queue()
    n, src = self.nbits_global, self.to_logical()
    mine = self._lidx()
    local = sum(1 << b for b in range(n) if self.bm[b] < self.nbits)
    old = out.to_logical()                                   # (read by the batches behind the first alone)
    exact = new = np.zeros(1 << n, dtype=np.complex128)
    for b, bt in enumerate(batches):
      tl = terms[bt['first']:bt['first'] + bt['count']]
      cps = [pauli_coef(cs[t['index']], self._pauli_ny(t), self._pauli_neg(t)) for t in tl]
      unit = pauli_unit(cps[0]) if len(tl) == 1 and b == 0 else None
      if unit is not None:                                  # stored as it is, negated and / or with its components swapped
        part = self._pauli_unit(pauli_rotated(src, n, xs[tl[0]['index']], zs[tl[0]['index']] & local, unit))
      else:
        part = np.zeros(1 << n, dtype=np.complex128)
        for t, c in zip(tl, cps):
          part += c * pauli_rotated(src, n, xs[t['index']], zs[t['index']] & local, 0)
      exact = new = out._pauli_accumulate(b, old, part)
      old = new = self._round(new)                          # rounded once per batch to the handle's width
    out.bm = self._pauli_bitmap(out)                        # written in src's physical layout: dst takes src's bit map
    keep = np.zeros(1 << n, dtype=np.complex128)
    keep[mine] = new[mine]
    out.store(keep)
    out.kernels += len(batches) if batches else self._pauli_zero_kernels()
    sb = (1 << self.nbits) * (16 if self.bit_width == 128 else 8)
    out.swept += (sum(bt['streams'] for bt in batches) if batches else 1) * sb
    out.algorithmic += (2 if batches else 1) * sb
    n2 = self._pauli_norm2(out.phys.astype(np.complex128), exact[mine])
    return (out, n2) if norm else out

  def _round(self, vec):
    return vec.astype(self.dtype).astype(np.complex128)

  def _pauli_enter(self):
    self.flush()                                             # what src has queued runs first

  def _pauli_drop_queue(self):
    self.queue = []                                          # dst is replaced whole: what it has queued is dropped

  def _pauli_ny(self, term):
    return term['ny']

  def _pauli_neg(self, term):
    return term['neg']

  def _pauli_unit(self, part):
    return part

  def _pauli_accumulate(self, b, old, part):
    return part if b == 0 else old + part                   # the first batch does not read dst

  def _pauli_bitmap(self, out):
    return list(self.bm)

  def _pauli_zero_kernels(self):
    return 1

  def _pauli_norm2(self, stored, unrounded):
    return float(np.vdot(stored, stored).real)

  # -- Pauli products: run by run as the header describes them, through hooks a mutant overrides one at a time ----------------------
  def pauli_product_plan(self, xmasks, zmasks):
    xs, zs = [int(x) for x in xmasks], [int(z) for z in zmasks]
    self._pauli_check('pauli_product_plan', None, xs, zs)
    return pauli_product_rule(self.nbits, self.bit_width, self.bm, self.shard, xs, zs, self._pprod_batch())

  def apply_pauli_product(self, a, b, xmasks, zmasks, norm=False):
    av, bv = [complex(v) for v in a], [complex(v) for v in b]
    xs, zs = [int(x) for x in xmasks], [int(z) for z in zmasks]
    self._pprod_check(av, bv, xs, zs, len(xs))               # the WHOLE list, before anything is flushed
    self._pprod_enter(len(xs))
    self._pprod_check(av, bv, xs, zs, len(xs), late=True)
    if not xs:                                               # nothing is launched; norm2 is the reader's
      self.kernels += self._pprod_zero_kernels()
      return self._model(self._read(0)).norm(0) if norm else None      # (the reader's sum; the call counts no kernel)
    terms, _ = self.pauli_product_plan(xs, zs)
    terms = self._pprod_order_list(terms)
    runs = ppu.greedy_runs([t['px'] for t in terms], self._pprod_batch(), 0 if self.bit_width == 128 else 1, PAULI_RUN_KINDS)
    n, mine = self.nbits_global, self._lidx()
    local = sum(1 << q for q in range(n) if self.bm[q] < self.nbits)
    vec = exact = self.to_logical()
    first_stored = None
    for first, count, _, _ in runs:
      tl = terms[first:first + count]
      t0 = tl[0]['index']
      bps = [pauli_coef(bv[t['index']], self._pprod_ny(t), self._pprod_neg(t)) for t in tl]
      if count == 1 and av[t0] == 0 and pauli_unit(bps[0]) is not None:      # the stored bits moved, negated and / or swapped
        vec = self._pprod_unit(vec, pauli_rotated(vec, n, xs[t0], zs[t0] & local, pauli_unit(bps[0])))
      elif count == 1 and av[t0] == 1 and bv[t0] == 0:                       # every bit as it was
        vec = self._pprod_identity(vec, xs[t0], zs[t0] & local)
      else:
        for t, bp in self._pprod_order_run(list(zip(tl, bps))):
          vec = av[t['index']] * vec + bp * self._pprod_partner(vec, xs[t['index']], zs[t['index']] & local)
      exact = vec
      vec = self._round(vec)                                  # rounded once per run to the handle's width
      if first_stored is None:
        first_stored = vec[mine]
    keep = np.zeros(1 << n, dtype=np.complex128)
    keep[mine] = vec[mine]
    self.store(keep)
    self._pprod_layout()
    sb = (1 << self.nbits) * (16 if self.bit_width == 128 else 8)
    self.submitted += len(xs)
    self.kernels += len(runs)
    self.swept += self._pprod_bytes(len(runs), sb)
    self.algorithmic += self._pprod_bytes(len(runs), sb)
    return self._pprod_norm2(self.phys.astype(np.complex128), exact[mine], first_stored) if norm else None

  def _pprod_check(self, av, bv, xs, zs, upto, late=False):
    if late:
      return
    for t in range(upto):
      if not all(np.isfinite(v) for v in (av[t].real, av[t].imag, bv[t].real, bv[t].imag)):
        raise native.QhError(native.QH_ERR_ARG, f'apply_pauli_product: term {t} has a non-finite coefficient')
    self._pauli_check('apply_pauli_product', None, xs[:upto], zs[:upto])

  def _pprod_enter(self, nterms):
    self.flush()                                             # a barrier: what is queued runs first

  def _pprod_batch(self):
    return PAULI_PRODUCT_BATCH

  def _pprod_zero_kernels(self):
    return 0

  def _pprod_order_list(self, terms):
    return terms                                             # the caller's order is never changed

  def _pprod_order_run(self, pairs):
    return pairs

  def _pprod_ny(self, term):
    return term['ny']

  def _pprod_neg(self, term):
    return term['neg']

  def _pprod_unit(self, vec, moved):
    return moved

  def _pprod_identity(self, vec, x, z):
    return vec

  def _pprod_own_index(self, idx, x):
    return idx                                               # the index whose z parity signs what arrives at idx: its own

  def _pprod_partner(self, vec, x, z):
    """(-1)^popcount(i & z) vec[i ^ x]"""
    idx = np.arange(vec.size, dtype=np.uint64)
    sign = 1.0 - 2.0 * pauli_util.parity(self._pprod_own_index(idx, x), z).astype(np.float64)
    return sign * vec[(idx ^ np.uint64(x)).astype(np.int64)]

  def _pprod_layout(self):
    pass                                                     # the bit map is as the call found it

  def _pprod_bytes(self, nruns, shard_bytes):
    return 2 * nruns * shard_bytes

  def _pprod_norm2(self, stored, unrounded, first_stored):
    return float(np.vdot(stored, stored).real)               # of the final amplitudes as stored, summed by the last run

  # -- reduced density matrices: clause by clause as the header describes them, through hooks a mutant overrides one at a time -----
  def _dens_check(self, who, bits):
    """k out of range, then the list (a bit beyond the register, a bit twice), then a listed bit the shard index holds"""
    kmax = min(DENSITY_MAX_BITS, self.nbits)
    if len(bits) > kmax:
      raise native.QhError(native.QH_ERR_ARG, f'{who}: k = {len(bits)} outside [0,{kmax}]')
    if any(not 0 <= b < self.nbits_global for b in bits):
      raise native.QhError(native.QH_ERR_BAD_QUBIT, f'{who}: a bit beyond the register')
    if len(set(bits)) != len(bits):
      raise native.QhError(native.QH_ERR_SAME_QUBIT, f'{who}: a bit twice')
    if any(not self._dens_local(b) for b in bits):
      raise native.QhError(native.QH_ERR_NONLOCAL, f'{who}: a listed bit is held by the shard index; exchange first')

  def density_plan(self, bits):
    bits = [int(b) for b in bits]
    self._dens_check('density_plan', bits)
    return density_rule(self.nbits, self.bm, bits)

  def reduced_density(self, bits):
    bits = [int(b) for b in bits]
    self._dens_check('reduced_density', bits)                # before anything is flushed
    self._dens_enter()
    plan = self.density_plan([b for b in bits if self._dens_is_local(b)])
    vec = self.to_logical()
    psi, number = local_view(vec, self.nbits_global, self.held())
    rho = du.np_reduced_density(psi, self._dens_rows([number[b] for b in bits if b in number]))
    rho = self._dens_mirror(self._dens_scale(self._dens_orient(rho)))
    self._dens_layout()
    ab = 16 if self.bit_width == 128 else 8
    self.kernels += self._dens_kernels()
    self.algorithmic += (1 << self.nbits) * ab
    self.swept += self._dens_swept(plan, ab)
    return rho

  def _dens_is_local(self, b):
    return self.bm[b] < self.nbits

  def _dens_local(self, b):
    return self._dens_is_local(b)                            # the refusal's view of it

  def _dens_enter(self):
    self.flush()                                             # a reader: what is queued runs first

  def _dens_rows(self, bits):
    return bits                                              # bits[t] is bit t of a row number

  def _dens_orient(self, rho):
    return rho                                               # rho[r][c] = sum_e a(r,e) conj(a(c,e))

  def _dens_scale(self, rho):
    return rho                                               # not normalised: the trace is the shard's norm

  def _dens_mirror(self, rho):
    """one triangle is computed, the other mirrored; the diagonal's imaginary parts are exactly 0.0"""
    out = np.array(rho, dtype=np.complex128)
    lower = np.tril_indices(out.shape[0], -1)
    out[lower] = np.conj(out.T[lower])                       # (a negation of the imaginary part: the sign of a zero included)
    d = np.diag_indices(out.shape[0])
    out[d] = out[d].real
    return out

  def _dens_layout(self):
    pass                                                     # reads only: the bit map is as the call found it

  def _dens_kernels(self):
    return 1                                                 # the fold is not counted

  def _dens_swept(self, plan, amp_bytes):
    return plan['amps_swept'] * amp_bytes                    # the bytes the kernel requests

  # -- Z-polynomials: clause by clause as the header describes them, through hooks a mutant overrides one at a time -------------------
  def _zp_check(self, who, ws, zs, c=None):
    """the whole list, before anything is flushed"""
    if len(zs) > ZPOLY_MAX_TERMS:
      raise native.QhError(native.QH_ERR_ARG, f'{who}: {len(zs)} terms (at most {ZPOLY_MAX_TERMS})')
    for t, (w, z) in enumerate(zip(ws, zs)):
      if not np.isfinite(w):
        raise native.QhError(native.QH_ERR_ARG, f'{who}: term {t} has a non-finite weight ({w})')
      if z >> self.nbits_global:
        raise native.QhError(native.QH_ERR_BAD_QUBIT, f'{who}: term {t} has bits >= {self.nbits_global}')
    if c is not None and not (np.isfinite(c.real) and np.isfinite(c.imag)):
      raise native.QhError(native.QH_ERR_ARG, f'{who}: c = {c} is not finite')

  def zpoly_plan(self, weights, zmasks):
    ws, zs = [float(w) for w in weights], [int(z) for z in zmasks]
    self._zp_check('zpoly_plan', ws, zs)
    return zpoly_rule(self.nbits, self.bit_width, self.bm, self.shard, ws, zs)

  def _zp_f(self, ws, zs):
    """f at the global logical indices the shard holds, from the terms as the kernels get them: masks cut to the local bits, the
    sign the shard index gives a held z bit folded into the weight"""
    held = self.held()
    local = sum(1 << b for b in range(self.nbits_global) if b not in held)
    terms = self._zp_terms([(self._zp_fold(w, z, held), z & local) for w, z in zip(ws, zs)])
    return zpoly_f(self.nbits_global, held, [self._zp_parity(w, z) for w, z in terms], [z for _, z in terms])

  def _zp_fold(self, w, z, held):
    return -w if sum(v for b, v in held.items() if (z >> b) & 1) & 1 else w      # an exact negation

  def _zp_terms(self, terms):
    return terms                                             # as given: a constant term is applied, equal masks are not merged

  def _zp_parity(self, w, z):
    return w                                                 # w (-1)^popcount(i & z): + where the parity is even

  def apply_zpoly(self, weights, zmasks, c, norm=False):
    ws, zs, c = [float(w) for w in weights], [int(z) for z in zmasks], complex(c)
    self._zp_check('apply_zpoly', ws, zs, c)
    self._zp_enter()
    if not zs or c == 0:                                     # flushes and launches nothing; norm2 is then the reader's
      self.kernels += self._zp_noop_kernels()
      return self._model(self._read(0)).norm(0) if norm else None
    mine = mine_of(self.nbits_global, self.held()).astype(np.int64)
    vec = self.to_logical()
    first = float(np.vdot(self.phys.astype(np.complex128), self.phys.astype(np.complex128)).real)
    cc = self._zp_c(c)
    out = np.zeros_like(vec)
    out[mine] = vec[mine] * self._zp_factor(cc, self._zp_f(ws, zs))
    self.store(out)                                          # rounded once to the handle's width
    self._zp_layout()
    sb = (1 << self.nbits) * (16 if self.bit_width == 128 else 8)
    self.submitted += 1
    self.kernels += 1
    self.swept += self._zp_bytes(sb)
    self.algorithmic += self._zp_bytes(sb)
    return self._zp_norm2(first, self.phys.astype(np.complex128)) if norm else None

  def _zp_enter(self):
    self.flush()                                             # a barrier: what is queued runs first

  def _zp_noop_kernels(self):
    return 0

  def _zp_c(self, c):
    return c

  def _zp_factor(self, c, f):
    return np.exp(c.real * f) * (np.cos(c.imag * f) + 1j * np.sin(c.imag * f))      # exp(c.re f) * (cos(c.im f), sin(c.im f))

  def _zp_layout(self):
    pass                                                     # the bit map is as the call found it

  def _zp_bytes(self, shard_bytes):
    return 2 * shard_bytes                                   # one read and one write of the state

  def _zp_norm2(self, first, stored):
    return float(np.vdot(stored, stored).real)               # of the final amplitudes as stored

  def expect_zpoly(self, weights, zmasks):
    ws, zs = [float(w) for w in weights], [int(z) for z in zmasks]
    self._zp_check('expect_zpoly', ws, zs)
    self._ezp_enter()
    if not zs:
      return self._model(self._read(0)).norm(0), 0.0, 0.0     # (the reader's sum; the call counts no kernel)
    mine = mine_of(self.nbits_global, self.held()).astype(np.int64)
    a = self.to_logical()[mine]
    p, f = a.real * a.real + a.imag * a.imag, self._zp_f(ws, zs)
    self._ezp_layout()
    sb = (1 << self.nbits) * (16 if self.bit_width == 128 else 8)
    self.kernels += 1
    self.swept += self._ezp_bytes(sb)
    self.algorithmic += self._ezp_bytes(sb)
    return float(np.sum(p)), float(np.dot(p, f)), self._ezp_second(p, f)

  def _ezp_enter(self):
    self.flush()                                             # a reader: what is queued runs first

  def _ezp_layout(self):
    pass

  def _ezp_bytes(self, shard_bytes):
    return shard_bytes                                       # one read of the state

  def _ezp_second(self, p, f):
    return float(np.dot(p, f * f))                           # sum |a_i|^2 f(i)^2, not normalised
