"""The corpus of tests/handler_corpus.py reaches every handler of every sweep island, proved without a GPU.

The handler space of an island is enumerated from the NUMBERING (sweep_handlers.inc, kernels_sweep.hip.h op_handler_id /
reg_mask_number / group_handler_bits) -- never from the island assembly; what a case reaches is what qh_plan_handlers
reports for it on a planner-only handle under the case's switches.  tests/test_gpu_handlers.py then runs the same cases
on the GPU and checks first that the live handle plans the same words."""
import numpy as np
import pytest

from tests import handler_corpus as hc
from tests import plan_interp

ISLAND_IDS = [hc.island_id(i) for i in hc.ISLANDS]


def _mask_numbers(rb):
  """reg_mask_number over every register mask of an island: 1-bit masks, 2-bit masks (b0 major), 15 = any other"""
  out = set(range(rb))
  idx = rb
  for b0 in range(rb):
    for b1 in range(b0 + 1, rb):
      out.add(min(idx, 15))
      idx += 1
  if rb >= 3:
    out.add(15)
  return out


def handler_space(bw, rb):
  """every op slot and group handler the numbering defines for this island, and the paths inside them the corpus must take"""
  k = hc.handler_numbers()
  ops = {k['kHidDiag'], k['kHidDense'], k['kHidWswap'], k['kHidBflyLane'], k['kHidBflyLaneDpp']}
  ops |= {k['kHidLswap'] + 2 * reg + (lane - 4) for reg in range(rb) for lane in (4, 5)}
  ops |= {k['kHidBflyReg'] + 8 * v + b for v in range(5) for b in range(rb)}
  if bw == 128:     # fused rotations and single groups folded into the op header: complex128 islands only
    ops |= {k['kHidBflyRot'] + 8 * (5 * rot + v) + b for rot in (0, 1) for v in range(5) for b in range(rb)}
    ops |= {k['kHidDiag1'] + 16 * cls + m for cls in range(3) for m in _mask_numbers(rb)}
  assert all(o < k['kNumOpHandlers'] for o in ops)
  # group_handler_bits: mask ids 0 (no register mask), 1-bit, 2-bit, any other; classes general / sign flip / uniform /
  # lane-masked; factor trees per register bit on the general path and from the header; sign-flip outside terms
  n_masks = 1 + rb + rb * (rb - 1) // 2 + 1
  mask_ids = set(range(n_masks - 1)) | ({n_masks - 1} if rb >= 3 else set())
  grp = set()
  for m in mask_ids:
    grp.add(4 | (m << 8))                                     # general
    grp.add((m + n_masks + rb) << 8)                          # factor -1
    grp.add((m + 2 * n_masks + rb) << 8)                      # uniform factor
    grp.add((m + 3 * n_masks + rb) << 8)                      # lane-masked factor
    grp.add(16 | ((m + n_masks + rb) << 8))                   # sign-flip outside terms
  for j in range(rb):
    grp.add(4 | ((n_masks + j) << 8))                         # factor tree, base from the general path
    grp.add((4 * n_masks + rb + j) << 8)                      # factor tree, base from the header
  feats = {'nwave0', 'nwave1', 'nwave2', 'store_inplace', 'store_relayout', 'diag_signflip_c', 'diag_general_c',
           'group_lane_table', 'group_chunk_table', 'group_outside_terms', 'dpp_bfly_plain', 'dpp_bfly_swap_ri',
           'dense_reg_general', 'dense_reg_real', 'dense_lane_general', 'dense_lane_real', 'dense_lane_real_dpp', 'dense_lane_use_c',
           'dense_reg_ctl_reg_one', 'dense_reg_ctl_reg_zero', 'dense_reg_ctl_thread',
           'dense_lane_ctl_reg_one', 'dense_lane_ctl_reg_zero', 'dense_lane_ctl_thread'}
  return {f'op:{o}' for o in ops} | {f'grp:{g}' for g in grp} | {f'feat:{f}' for f in feats}


def describe(island, key):
  """a handler key in words (messages only)"""
  bw, rb = island
  k = hc.handler_numbers()
  what, v = key.split(':')
  if what == 'feat':
    return key
  v = int(v)
  if what == 'op':
    if v >= k['kHidDiag1']:
      return f'{key}=d1(class {(v - k["kHidDiag1"]) // 16}, mask no {(v - k["kHidDiag1"]) % 16})'
    if v >= k['kHidBflyRot']:
      w = v - k['kHidBflyRot']
      return f'{key}=bfly_rot({"pm"[w // 40]}, variant {w // 8 % 5}, reg bit {w % 8})'
    if v >= k['kHidBflyReg']:
      return f'{key}=bfly_reg(variant {(v - k["kHidBflyReg"]) // 8}, reg bit {(v - k["kHidBflyReg"]) % 8})'
    if v >= k['kHidLswap']:
      return f'{key}=lswap(reg bit {(v - k["kHidLswap"]) // 2}, lane bit {4 + (v - k["kHidLswap"]) % 2})'
    return f'{key}=' + {k['kHidDiag']: 'diag', k['kHidDense']: 'dense', k['kHidWswap']: 'wswap', k['kHidBflyLane']: 'bfly_lane',
                        k['kHidBflyLaneDpp']: 'bfly_lane_dpp'}.get(v, '?')
  n_masks = 1 + rb + rb * (rb - 1) // 2 + 1
  hid, general, sot = v >> 8, bool(v & 4), bool(v & 16)
  if sot:
    return f'{key}=group(sign-flip outside terms, mask id {hid - n_masks - rb})'
  if general:
    return f'{key}=group(general, mask id {hid})' if hid < n_masks else f'{key}=group(factor tree general, reg bit {hid - n_masks})'
  if hid >= 4 * n_masks + rb:
    return f'{key}=group(factor tree header, reg bit {hid - 4 * n_masks - rb})'
  cls = (hid - rb) // n_masks
  return f'{key}=group({["?", "factor -1", "uniform", "lane-masked"][cls]}, mask id {(hid - rb) % n_masks})'


# Handlers the numbering defines but the planner cannot emit, under any switch setting: (island, key) -> the planner line
# that excludes it.  Candidates for removal from the generator; the test fails if the corpus ever plans one.
_NO_TREE_AT_RB2 = ('planner.h fuse_bit_factors, "if (best_n < (base >= 0 ? 2 : 3)) return;": a factor tree needs two scalar groups on two '
                   'register bits {i, j} in ONE DIAG op; with two register bits there is one such mask, and flush_diag keeps one group '
                   'per (lane mask, register mask)')
DEAD = {}
for _bw in (128, 64):
  _nm = 1 + 2 + 1 + 1        # n_masks at rb = 2
  for _j in range(2):
    DEAD[((_bw, 2), f'grp:{4 | ((_nm + _j) << 8)}')] = _NO_TREE_AT_RB2            # factor tree, base from the general path
    DEAD[((_bw, 2), f'grp:{(4 * _nm + 2 + _j) << 8}')] = _NO_TREE_AT_RB2          # factor tree, base from the header


def _dead(island):
  return {key for (isl, key) in DEAD if isl == island}


@pytest.fixture(scope='module')
def plans():
  """{case name: (handler words, exported plan, reached)} -- planned once, shared, never modified"""
  out = {}
  for c in hc.CASES:
    words, sweeps = hc.dry_plan(c)
    out[c.name] = (words, sweeps, hc.reached(c, words, sweeps))
  return out


@pytest.fixture(scope='module')
def claims():
  return hc.load_claims()


def test_the_corpus_is_small_and_named(claims):
  assert sorted(claims) == sorted(c.name for c in hc.CASES), 'tests/golden/handler_claims.json is not about these cases'
  for c in hc.CASES:
    assert len(c.gates) <= 48 and 6 + c.island[1] <= c.n <= 16, c.name
    assert claims[c.name], (c.name, 'claims nothing')


@pytest.mark.parametrize('island', hc.ISLANDS, ids=ISLAND_IDS)
def test_corpus_reaches_the_whole_handler_space(plans, claims, island):
  space, dead = handler_space(*island), _dead(island)
  assert dead <= space
  got, claimed = set(), set()
  for c in hc.CASES:
    if c.island == island:
      got |= set(plans[c.name][2])
      claimed |= claims[c.name]
  planned_dead = sorted(got & dead)
  assert not planned_dead, ('DEAD entries the corpus plans', [describe(island, k) for k in planned_dead])
  missing = sorted((space - dead) - got)
  assert not missing, ('never planned', [describe(island, k) for k in missing])
  unclaimed = sorted((space - dead) - claimed)
  assert not unclaimed, ('claimed by no case', [describe(island, k) for k in unclaimed])
  outside = sorted(k for k in got - space if not k.startswith('feat:'))
  assert not outside, ('planned, but not in the space the numbering defines', [describe(island, k) for k in outside])


def test_claimed_is_reached(plans, claims):
  for c in hc.CASES:
    lost = sorted(claims[c.name] - set(plans[c.name][2]))
    assert not lost, (c.name, 'claims what its plan does not dispatch', [describe(c.island, k) for k in lost])


@pytest.mark.parametrize('island', hc.ISLANDS, ids=ISLAND_IDS)
def test_plans_equal_the_oracle_and_claimed_ops_are_visible(oracle, plans, claims, island):
  for c in hc.CASES:
    if c.island != island:
      continue
    words, sweeps, r = plans[c.name]
    psi0 = hc.case_state(c)
    want = hc.oracle_apply(oracle, psi0.copy(), c)
    base = plan_interp.run_plan(psi0.copy(), sweeps, c.n)
    err = float(np.max(np.abs(base - want)))
    assert err < 1e-11, (c.name, err)           # (the bound of tests/test_planner_semantics_cpu.py)
    for key in sorted(claims[c.name]):
      assert hc.visible_instances(c, sweeps, r[key][:3], psi0, base), \
          (c.name, describe(c.island, key), 'deleting the op / group does not move the result: it would run on the GPU and change nothing')
