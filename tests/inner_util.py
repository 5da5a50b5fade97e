"""Shared by tests/test_inner_cpu.py and tests/test_gpu_inner.py: the hand-made layout pairs for qh_inner and a NumPy model
of how k_two_tiles walks two states from a qh_inner_tiles plan."""
import numpy as np


def hand_maps(nloc):
  """[(name, swaps on a, swaps on b)]: lists of (x, y) for qh_remap_swap, chosen by PHYSICAL position.  A swap of a position
  with itself is left out, so the smallest registers keep fewer distinct pairs."""
  def sw(pairs):
    return [(x, y) for x, y in pairs if x != y and 0 <= x < nloc and 0 <= y < nloc]
  top4 = sw([(k, nloc - 4 + k) for k in range(4)])
  two = sw([(0, nloc - 1), (1, nloc - 2)])
  low = sw([(0, 3), (1, 2), (0, 1)])
  rev = sw([(k, nloc - 1 - k) for k in range(nloc // 2)])
  return [('low4<->top4', [], top4), ('bits01<->high', [], two), ('inside0..3', [], low), ('reversal', [], rev),
          ('both', low + two, rev + top4)]


def apply_swaps(perm, swaps):
  """perm[l] = physical position of logical bit l after the swaps (what qh_remap_swap does to the bit map)."""
  perm = list(perm)
  for x, y in swaps:
    lx, ly = perm.index(x), perm.index(y)
    perm[lx], perm[ly] = perm[ly], perm[lx]
  return perm


def spread(idx, positions):
  """sum_k bit_k(idx) << positions[k], on uint64 arrays"""
  idx = np.asarray(idx, dtype=np.uint64)
  out = np.zeros(idx.shape, dtype=np.uint64)
  for k, p in enumerate(positions):
    out |= ((idx >> np.uint64(k)) & np.uint64(1)) << np.uint64(p)
  return out


def tile_pairs(plan, nloc):
  """(a index, b index) of every pair the tile walk forms, in walk order: tile by tile, thread r of 256 holding a's in-tile
  index r and picking b's value from LDS slot shuffle(r), which the thread of that number loaded in b's enumeration."""
  nrest = plan['nrest']
  assert nrest == nloc - 8
  tiles = np.arange(1 << nrest, dtype=np.uint64)
  base_a, base_b = spread(tiles, plan['rest_a'][:nrest]), spread(tiles, plan['rest_b'][:nrest])
  r = np.arange(256, dtype=np.uint64)
  da, db = spread(r, plan['tile_a']), spread(r, plan['tile_b'])
  slot = spread(r, plan['shuffle']).astype(np.int64)
  ia = (base_a[:, None] | da[None, :]).reshape(-1)
  ib = (base_b[:, None] | db[slot][None, :]).reshape(-1)
  return ia, ib


def expected_pairs(perm_a, perm_b, nloc):
  """b's physical index of every physical index of a, from the two bit maps (local bits only)"""
  logical = np.arange(1 << nloc, dtype=np.uint64)
  pa, pb = spread(logical, perm_a[:nloc]), spread(logical, perm_b[:nloc])
  want = np.zeros(1 << nloc, dtype=np.uint64)
  want[pa.astype(np.int64)] = pb
  return want
