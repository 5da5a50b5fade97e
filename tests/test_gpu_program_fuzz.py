"""Random programs over the whole device API on the MI355X (tests/program_model.py): every fixed program, one per test item,
in this process.  run_program holds every step to the NumPy model -- amplitudes read through a clone before and after the
step, results, bit maps, pending counts, kernel counts -- and the final downloads to a model that never looked at the device.

The last item reads what the earlier ones recorded from the real qh_get_bitmap / qh_inner_plan: relayout sweeps did leave a
permuted local map in front of a barrier step or a reader in at least a third of the 'own' programs that start at 14 local
bits or more, and all three paths of the two-state kernels were taken.  Of the register permutations it reads what the real
qh_perm_plan said right behind each call: at both widths the LDS path and the gather path ran, the gather path on a handle
that keeps a relayout buffer (which it borrows), on one that keeps none (a temporary) and on a shard, and a permutation ran on a
non-identity local map that its own flush had left.  Of the Pauli-sum operators it reads what the real qh_pauli_sum_plan and
qh_get_bitmap said right behind each call: at both widths k_pauli_small and k_pauli_batch ran, the latter in all four
instantiation classes (few or many term slots, one x mask or several) and with an accumulating batch, on a shard with the shard
sign set, on a non-identity local map that the call's own flush had left, into a destination whose queue was dropped and into
one that held NaN; at complex64 with physical bit 0 in an x mask and in a z mask.  Of the Pauli products it reads what the real
qh_pauli_product_plan and qh_get_bitmap said right behind each call: at both widths k_pauli_product_small ran and k_pauli_product
in each of its walks (items of a diagonal run, items with a lane exchange, pair numbers, and at complex64 the two halves of an
item), each with few and with many term slots, on lists of three runs or more, with norm2 asked and not asked on several runs,
with the partner's sign flipped, with diagonal and exchanging terms in one run, on both exact paths, with no terms behind a queue,
on a shard with the shard sign set, on a non-identity local map that the call's own flush had left, on an attached and on a
host-mapped handle; at complex64 with physical bit 0 in the X of a pair or lane run and in a z mask.  Of the reduced density
matrices it reads what the real qh_density_plan and qh_get_bitmap said right behind each call: at both widths the gather path and
the tiles path ran, with k = 0, 1-2, 3-5, 6, 7 (three block pairs), 8 (ten) and the whole shard, with row_bit not the identity, with
the register on physical position 0 and on positions 0 and 1, with the chunk cut short by the environment, behind a queued burst,
on a non-identity local map that the call's own flush had left, on a shard, on an attached and on a host-mapped handle, and right
behind extend, release or copy_from with no flush between; at one width at least with several chunks per workgroup.  Of the
Z-polynomials it reads what the real qh_zpoly_plan and qh_get_bitmap said right behind each call, qh_apply_zpoly and
qh_expect_zpoly counted apart: at both widths the small kernel and the main kernel ran, the latter with terms of all four classes,
with groups of all three kinds and several of one kind, with a segment of more than 64 terms and one of 2 to 63, with 4096 terms,
with duplicate masks, on a shard with a held bit in a mask where the sign is negative, on a non-identity local map that the
call's own flush had left, on an attached and on a host-mapped handle; the apply with c.re == 0, c.im == 0, a general c, c == (0, 0),
no terms behind a queue, norm2 asked and not asked; at complex64 with physical bit 0 in a mask.  The CPU table
(tests/test_program_fuzz_cpu.py) only predicts this.

The figures recorded when the file was added (time, chain errors per program) are in HISTORY.md, section T1; those of the
register permutations in section T2, those of the Pauli-sum operators in section T3, those of the Pauli products in section T4,
those of the reduced densities and the Z-polynomials in section T5.
"""
import pytest

from qcc_amd import native
from tests import program_model as pm
from tests.test_program_fuzz_cpu import (DENSITY_LINES, PRODUCT_WALKS, ZPOLY_APPLY_LINES, ZPOLY_LINES, ZPOLY_LINES_64, density_counts, pauli_counts,
                                         pauli_product_counts, zpoly_counts)

pytestmark = pytest.mark.gpu

SEEN = {'own': 0, 'own_big': 0, 'own_big_relaid': 0, 'paths': set(), 'gather_relayout_0': 0}
PERMS = []                    # (mode, width, the record of a 'perm' step: program_model._Runner.perm_record), fixed programs only
PAULIS = []                   # (mode, width, non-identity local map, the record of a 'pauli_sum' step: _Runner.run_pauli_sum), likewise
VARIANT_PAULIS = {}           # planner variant (its index in pm.ENV_VARIANTS) -> 'pauli_sum' steps on the main shape under it
PRODUCTS = []                 # (mode, width, non-identity local map, the record of a 'pauli_product' step: _Runner.run_pauli_product), fixed programs only
VARIANT_PRODUCTS = {}         # planner variant -> 'pauli_product' steps on the main shape under it
NEW_KINDS = ('reduced_density', 'zpoly', 'expect_zpoly')
NEW_STEPS = {op: [] for op in NEW_KINDS}      # op -> (mode, width, non-identity local map, the record of _Runner.run_<op>), fixed programs only
VARIANT_NEW = {}              # planner variant -> [zpoly steps on the main kernel, reduced_density steps on the TILES path] under it
RATIOS = {}                   # family of derived bound -> the largest error seen as a fraction of it (printed by the closing item)
# the 'own' programs that run again under a planner variant: (seed, width) whose first handle has sweeps that re-lay out and
# which hold a register permutation (checked below, so that a change of the generator cannot quietly empty the list); of
# the four under QH_RELAYOUT=0 the last two were added for a register wide enough for the gather path, there through a
# temporary on a handle that owns its memory.  Under each variant at least one program holds a Pauli sum on the main shape
# and a Pauli product on the main shape (checked by the closing item): own-18 at complex64 no longer held a 'perm' step when
# 'pauli_sum' became a kind and gave way to own-92, which lost its own when 'pauli_product' did and gave way to own-11.  With the
# reduced densities and the Z-polynomials own-4 and own-8 at complex64 lost their 'perm' steps and gave way to own-82 (whose register
# of 15 bits is now the one that takes the gather path under QH_RELAYOUT=0) and own-92; under each variant a listed program holds a
# 'zpoly' step on the main kernel and a 'reduced_density' step on the TILES path (checked by the closing item).
VARIANT_PROGRAMS = [(env, seed, bw) for env, pair in zip(pm.ENV_VARIANTS, ([(1, 128), (82, 64), (8, 128), (15, 64)], [(15, 128), (11, 64)], [(6, 128), (92, 64)]))
                    for seed, bw in pair]


def _run(mode, seed, bw):
  prog = pm.gen_program(seed, bw, mode)
  print(f'\n{mode}-{seed}-c{bw} ', end='')                  # (with -s: the chain figures of run_program follow on this line)
  check = pm.run_program(prog, pm.make_device_state, pm.Check(bw))
  for k, v in check.ratios.items():
    RATIOS[k, bw] = max(RATIOS.get((k, bw), 0.0), v)
  return prog, check


@pytest.mark.parametrize('bw', [128, 64])
@pytest.mark.parametrize('mode,seed', pm.FIXED, ids=[f'{m}-{s}' for m, s in pm.FIXED])
def test_program(mode, seed, bw):
  prog, check = _run(mode, seed, bw)
  PERMS.extend((mode, bw, e[5]) for e in check.events if e[1] == 'perm')
  PAULIS.extend((mode, bw, e[2], e[5]) for e in check.events if e[1] == 'pauli_sum')
  PRODUCTS.extend((mode, bw, e[2], e[5]) for e in check.events if e[1] == 'pauli_product')
  for op in NEW_KINDS:
    NEW_STEPS[op].extend((mode, bw, e[2], e[5]) for e in check.events if e[1] == op)
  if mode == 'own':
    SEEN['own'] += 1
    SEEN['paths'] |= {e[4] for e in check.events if e[4] is not None}
    if prog[0]['nloc'] >= pm.PERMUTED_FROM:
      SEEN['own_big'] += 1
      SEEN['own_big_relaid'] += check.relaid > 0


@pytest.mark.parametrize('env,seed,bw', VARIANT_PROGRAMS,
                         ids=['-'.join(f'{k}={v}' for k, v in e.items()) + f'-{sd}-c{w}' for e, sd, w in VARIANT_PROGRAMS])
def test_program_under_planner_variants(env, seed, bw, monkeypatch):
  for k, v in env.items():
    monkeypatch.setenv(k, v)                                # (the planner reads its switches at every flush)
  prog, check = _run('own', seed, bw)
  assert prog[0]['nloc'] >= pm.PERMUTED_FROM and any(s['op'] == 'perm' for s in prog)
  which = pm.ENV_VARIANTS.index(env)
  VARIANT_PAULIS[which] = VARIANT_PAULIS.get(which, 0) + sum(1 for e in check.events if e[1] == 'pauli_sum' and e[5]['main'])
  VARIANT_PRODUCTS[which] = VARIANT_PRODUCTS.get(which, 0) + sum(1 for e in check.events if e[1] == 'pauli_product' and e[5]['main'] and not e[5]['zero'])
  seen = VARIANT_NEW.setdefault(which, [0, 0])
  seen[0] += sum(1 for e in check.events if e[1] == 'zpoly' and e[5]['main'] and e[5]['nterms'] and e[5]['c'] != 'zero')
  seen[1] += sum(1 for e in check.events if e[1] == 'reduced_density' and e[5]['path'] == native.QH_DENSITY_TILES)
  if env.get('QH_RELAYOUT') == '0':
    assert check.relaid == 0                                # no flush re-laid a handle out: clones and siblings decide as told
    perms = [e[5] for e in check.events if e[1] == 'perm']
    assert not any(r['relayout_on'] for r in perms)
    SEEN['gather_relayout_0'] += sum(1 for r in perms if r['ctl_met'] and r['path'] == native.QH_PERM_GATHER)


def test_zz_relayout_and_inner_paths_were_met():
  if not SEEN['own']:
    pytest.skip('reads what the program items of this file recorded: run the file as a whole')
  print(f"'own' programs from {pm.PERMUTED_FROM} local bits: {SEEN['own_big']}, re-laid out in front of a barrier or reader: "
        f"{SEEN['own_big_relaid']}; inner paths {sorted(SEEN['paths'])}")
  assert 3 * SEEN['own_big_relaid'] >= SEEN['own_big'] > 0
  assert SEEN['paths'] == {native.QH_INNER_LINEAR, native.QH_INNER_TILES, native.QH_INNER_GATHER}
  for bw in (128, 64):
    ran = [(mode, r) for mode, w, r in PERMS if w == bw and r['ctl_met']]       # (a held control that is 0 on the shard runs nothing)
    gather = [(mode, r) for mode, r in ran if r['path'] == native.QH_PERM_GATHER]
    n = {'lds': len(ran) - len(gather), 'gather': len(gather),
         'gather, own handle, relayout buffer': sum(1 for mode, r in gather if mode in ('own', 'shard') and r['relayout_on']),
         'gather, temporary': sum(1 for mode, r in gather if not r['relayout_on']),
         'gather on a shard': sum(1 for mode, r in gather if r['shard']),
         'permuted map behind its own flush': sum(1 for mode, r in ran if r['relaid']),
         'no-op (held control 0)': sum(1 for mode, w, r in PERMS if w == bw and not r['ctl_met'])}
    by_kind = {m: [sum(1 for mode, r in ran if mode == m and r['path'] == p) for p in (native.QH_PERM_LDS, native.QH_PERM_GATHER)]
               for m in ('own', 'shard', 'attached', 'mapped')}
    print(f'perm steps at complex{bw}: {n}; [lds, gather] by program kind: {by_kind}')
    assert n['lds'] and n['gather'] and n['gather, own handle, relayout buffer'] and n['gather, temporary'], n
    assert n['permuted map behind its own flush'] and n['gather on a shard'], n
  print(f"gather-path perm steps under QH_RELAYOUT=0 (a temporary on a handle that owns its memory): {SEEN['gather_relayout_0']}")
  assert SEEN['gather_relayout_0']
  # the Pauli-sum operators, from what the real qh_pauli_sum_plan and qh_get_bitmap said right behind each call
  for bw in (128, 64):
    n = pauli_counts([(mode, permuted, r) for mode, w, permuted, r in PAULIS if w == bw], bw)
    print(f'pauli_sum steps at complex{bw}: {n}')
    for k in ('k_pauli_small shape', 'main shape', 'main shape: few term slots, one x mask', 'main shape: few term slots, several x masks',
              'main shape: many term slots, one x mask', 'main shape: many term slots, several x masks', 'an accumulating batch on the main shape',
              'shard: main shape with neg set', 'on a non-identity local map its own flush left', 'dst with a queue dropped', 'dst poisoned') + \
             (('complex64: px bit 0 set', 'complex64: pz bit 0 set') if bw == 64 else ()):
      assert n.get(k, 0) >= 1, (bw, k, n)
  print(f'pauli_sum steps on the main shape under the planner variants: {VARIANT_PAULIS}')
  assert all(VARIANT_PAULIS.get(which, 0) >= 1 for which in range(len(pm.ENV_VARIANTS))), VARIANT_PAULIS
  # the Pauli products, from what the real qh_pauli_product_plan and qh_get_bitmap said right behind each call
  for bw in (128, 64):
    n = pauli_product_counts([(mode, permuted, r) for mode, w, permuted, r in PRODUCTS if w == bw], bw)
    print(f'pauli_product steps at complex{bw}: {n}')
    walks = [f'main shape: {walk} walk, {slots} term slots' for walk in PRODUCT_WALKS[:4 if bw == 64 else 3] for slots in ('few', 'many')]
    for k in ['k_pauli_product_small shape', 'main shape'] + walks + \
             ['three or more runs', 'several runs, norm2 asked', 'several runs, norm2 not asked', 'a run with flip set', 'a run with flip set on the main shape',
              'a run mixing diagonal and exchanging terms', 'exact path: one unit string', 'exact path: the factor (1, 0)', 'zero terms behind a queue',
              'shard: main shape with neg set', 'on a non-identity local map its own flush left', 'on an attached handle', 'on a host-mapped handle'] + \
             (['complex64: physical bit 0 in X of a pair or lane run', 'complex64: physical bit 0 in a z mask'] if bw == 64 else []):
      assert n.get(k, 0) >= 1, (bw, k, n)
  print(f'pauli_product steps on the main shape under the planner variants: {VARIANT_PRODUCTS}')
  assert all(VARIANT_PRODUCTS.get(which, 0) >= 1 for which in range(len(pm.ENV_VARIANTS))), VARIANT_PRODUCTS
  # the reduced density matrices, from what the real qh_density_plan and qh_get_bitmap said right behind each call
  several = 0
  for bw in (128, 64):
    n = density_counts([(mode, permuted, r) for mode, w, permuted, r in NEW_STEPS['reduced_density'] if w == bw], bw)
    print(f'reduced_density steps at complex{bw}: {n}')
    several += n.get('chunks_per_wg > 1', 0)
    for k in DENSITY_LINES:
      assert n.get(k, 0) >= 1, (bw, k, n)
  assert several >= 1                                       # (k = 8 from 18 local bits on, k = 7 from 19: either width will do)
  # the Z-polynomials, from what the real qh_zpoly_plan and qh_get_bitmap said right behind each call
  for op, lines in (('zpoly', ZPOLY_APPLY_LINES), ('expect_zpoly', ZPOLY_LINES)):
    for bw in (128, 64):
      n = zpoly_counts([(mode, permuted, r) for mode, w, permuted, r in NEW_STEPS[op] if w == bw], bw)
      print(f'{op} steps at complex{bw}: {n}')
      for k in lines + (ZPOLY_LINES_64 if bw == 64 else ()):
        assert n.get(k, 0) >= 1, (op, bw, k, n)
  print(f'[zpoly steps on the main kernel, reduced_density steps on the TILES path] under the planner variants: {VARIANT_NEW}')
  assert all(min(VARIANT_NEW.get(which, [0, 0])) >= 1 for which in range(len(pm.ENV_VARIANTS))), VARIANT_NEW
  print('largest error as a fraction of its derived bound: ' + ', '.join(f'{k} at complex{w} {v:.3g}' for (k, w), v in sorted(RATIOS.items())))
