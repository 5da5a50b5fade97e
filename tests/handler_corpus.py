"""A deterministic corpus of short circuits that, together, make the sweep planner emit every op handler and every
DIAG-group handler of the nine sweep islands (sweep_island[_f32]_rb*.inc): TEST INFRASTRUCTURE, a plain module.

Which handlers a circuit reaches is never worked out here: it is read from qh_plan_handlers -- the device copy of the
plan, numbered by the function a flush numbers its upload with.  A case only CLAIMS handlers (tests/golden/
handler_claims.json, written once by `python -m tests.handler_corpus --write-claims` and reviewed like code);
tests/test_handler_coverage_cpu.py proves claimed = reached, that the claims cover the whole handler space, that the plans
compute the circuits and that every claimed op changes the result; tests/test_gpu_handlers.py runs the cases on the GPU.

A case: name, island (bit width, register bits), n, planner switches, a gate stream of (control mask, target bit, 2x2
matrix) in index-bit numbers (qh_apply_bits).  Cases are built by construction -- every register bit x every butterfly
variant x both rotations, every register mask x every factor class, ... -- at the smallest sizes an island can be chosen:
n = 6 + rb (the tile is the state), up to 6 + rb + 2 where wave bits, outside bits or a relayout store are wanted.

Handler keys (strings): 'op:<number>' (the branch-table slot, sweep_handlers.inc), 'grp:<flags & 0xff14>' (the group's
device flags: handler number in bits 8..15, general path bit 2, sign-flip outside terms bit 4), and 'feat:<name>' for the
paths inside one handler that the issue lists (dense op shapes, DPP with / without exchanged partner, DIAG flag bit 9,
group tables, wave bits, store kinds)."""
import collections
import ctypes
import itertools
import json
import os
import zlib

import numpy as np

from qcc_amd import native
from tests import plan_interp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLAIMS_PATH = os.path.join(ROOT, 'tests', 'golden', 'handler_claims.json')
ISLANDS = [(128, 2), (128, 3), (128, 4), (128, 5), (64, 2), (64, 3), (64, 4), (64, 5), (64, 6)]
MAGIC = 0x51484831
_dp = ctypes.POINTER(ctypes.c_double)

Case = collections.namedtuple('Case', 'name island n env gates')


def island_id(island):
  return f'c{island[0]}_rb{island[1]}'


# ---- gates --------------------------------------------------------------------------------------
_S = 1.0 / np.sqrt(2.0)
# c * M with unit entries (planner.h butterfly_variant): h, yroot, yroot^+, v, v^+ up to their scalars
BF = [np.array(m, dtype=np.complex128) * _S for m in
      ([[1, 1], [1, -1]], [[1, -1], [1, 1]], [[1, 1], [-1, 1]], [[1, -1j], [-1j, 1]], [[1, 1j], [1j, 1]])]
Z = np.diag([1.0, -1.0]).astype(np.complex128)
X = np.array([[0, 1], [1, 0]], dtype=np.complex128)


def ph(theta):
  return np.diag([1.0, np.exp(1j * theta)])


def t_pow(k):      # T^k: k odd -> a phase c (1 +- i), fused into the butterfly behind it (OPF_ROT_P / OPF_ROT_M)
  s = np.sqrt(0.5)
  return np.diag([1.0, complex(*{1: (s, s), 3: (-s, s), 5: (-s, -s), 7: (s, -s)}[k % 8])])


def ru(rng):       # a random unitary: the general dense path
  m = rng.standard_normal((2, 2)) + 1j * rng.standard_normal((2, 2))
  q, r = np.linalg.qr(m)
  return q * (np.diag(r) / np.abs(np.diag(r)))


def rr(rng):       # a random real rotation: OPF_REAL
  a = float(rng.uniform(0.3, 2.8))
  return np.array([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]], dtype=np.complex128)


def mask_of(bits):
  m = 0
  for b in bits:
    m |= 1 << b
  return m


def diag_on(bits, phase):
  """diag gate: `phase` where every bit of `bits` is set."""
  bits = sorted(bits)
  g = np.diag([1.0, phase]).astype(np.complex128)
  return (mask_of(bits[1:]), bits[0], g)


# ---- the cases -----------------------------------------------------------------------------------
def _chunks(seq, size):
  seq = list(seq)
  k = max(1, -(-len(seq) // size))
  per = -(-len(seq) // k)
  return [seq[i:i + per] for i in range(0, len(seq), per)]


def _reg_masks(rb):
  """register-bit sets: every 1-bit and 2-bit mask, and (rb >= 3) masks of three and more bits"""
  out = [(a,) for a in range(rb)] + list(itertools.combinations(range(rb), 2))
  if rb >= 3:
    out.append((0, 1, 2))
    out.append(tuple(range(rb - 3, rb)) if rb > 3 else (0, 1, 2))
    if rb >= 4:
      out.append(tuple(range(rb)))
  return list(dict.fromkeys(out))


def _island_cases(bw, rb):
  isl = (bw, rb)
  max_rb = 5 if bw == 128 else 6
  base_env = {} if rb == max_rb else {'QH_SWEEP_RB': str(rb)}
  n0 = 6 + rb
  R = list(range(6, 6 + rb))            # at n0 the register bits are index bits 6.. in order
  cases = []

  def add(name, n, env, gates):
    full = f'{island_id(isl)}:{name}'
    e = dict(base_env)
    e.update(env)
    cases.append(Case(full, isl, n, e, gates))

  def rng_for(name):
    return np.random.default_rng(zlib.crc32(f'{bw}/{rb}/{name}'.encode()))

  # register butterflies: every variant x every register bit
  add('bfr', n0, {}, [(0, b, BF[v]) for v in range(5) for b in R])
  # ... behind a T^k on their target (fused on complex128: both rotations, both signs of the scale)
  for rot, ks in (('p', (1, 5)), ('m', (7, 3))):
    for vs in ((0, 1, 2), (3, 4)):
      g = []
      for v in vs:
        for i, b in enumerate(R):
          g += [(0, b, t_pow(ks[(i + v) % 2])), (0, b, BF[v])]
      add(f'rot_{rot}_v{"".join(map(str, vs))}', n0, {}, g)
  # lane butterflies: DPP moves (lane bits 0..3; partner re/im exchanged for variants 3, 4), through LDS, and lane
  # bits 4 / 5 exchanged with every register bit (the victim is the one register bit no later gate targets; the controls on
  # bits 4 and 5 keep those gates behind the butterflies)
  add('lane_dpp', n0, {'QH_LANE_VALU': '2'}, [(0, l, BF[v]) for v in range(5) for l in range(4)])
  add('lane_lds', n0, {'QH_LANE_VALU': '0'}, [(0, l, BF[v]) for v in range(5) for l in (0, 3, 4, 5)][:16] +
      [(0, R[0], BF[0])])
  for r in range(rb):
    rng = rng_for(f'lswap{r}')
    add(f'lswap_r{r}', n0, {'QH_LANE_VALU': '2'},
        [(0, 4, BF[r % 5]), (0, 5, BF[(r + 3) % 5])] + [(1 << 4 | 1 << 5, R[k], ru(rng)) for k in range(rb) if k != r])
  # dense 2x2: register / lane target, general / real, register controls (one, zero), thread controls
  rng = rng_for('dense')
  c1 = R[1]
  add('dense', n0, {}, [
      (0, R[0], ru(rng)), (0, R[1], rr(rng)), (0, 1, ru(rng)), (0, 2, rr(rng)), (0, 5, ru(rng)), (0, 4, rr(rng)),
      (1 << c1, R[0], ru(rng)), (1 << c1, R[0], rr(rng)),                                  # register control
      (0, c1, X), (1 << c1, R[0], ru(rng)), (1 << c1, 3, rr(rng)), (0, c1, X),             # ... required to be zero
      (1 << 3, R[0], ru(rng)), (1 << 0, R[1], rr(rng)), (1 << R[0], 2, ru(rng)), (1 << 3, 1, ru(rng)),   # lane-bit (thread) controls
      (0, 2, X), (1 << 2, R[1], ru(rng)), (0, 2, X),                                       # ... required to be zero
      (0, 1, ph(0.7)), (0, 1, ru(rng)),                                                    # phase folded into a lane op's matrix
      (0, 0, Z), (0, 0, ru(rng)), (0, R[0], ru(rng))])
  add('dense_dpp', n0, {'QH_LANE_VALU': '2'}, [(0, l, rr(rng)) for l in range(6)] + [(1 << R[0], l, rr(rng)) for l in (0, 2)] +
      [(0, R[0], ru(rng))])
  # DIAG ops of one group: factor class x register mask (complex128: folded into the op header; complex64: the group handlers)
  masks = _reg_masks(rb)
  for cls in ('neg', 'uni', 'lane'):
    for ci, chunk in enumerate(_chunks(masks, 16)):
      rng = rng_for(f'd1{cls}{ci}')
      g = []
      for k, m in enumerate(chunk):
        bits = [R[i] for i in m] + ([k % 6] if cls == 'lane' else [])
        g += [diag_on(bits, -1.0 if cls == 'neg' else np.exp(1j * (0.4 + 0.37 * k))), (0, R[m[k % len(m)]], ru(rng))]
      add(f'd1_{cls}_{ci}', n0, {}, g)
  # ... and of two groups (every width dispatches those through the group handlers): the same, beside a companion term
  for cls in ('neg', 'uni', 'lane'):
    for ci, chunk in enumerate(_chunks(masks, 12)):
      rng = rng_for(f'grp{cls}{ci}')
      g = []
      for k, m in enumerate(chunk):
        t = m[k % len(m)]
        bits = [R[i] for i in m] + ([1 + k % 5] if cls == 'lane' else [])
        comp = [R[t], R[(t + 1) % rb], 0] if len(m) == 1 else [R[t], 0]
        g += [diag_on(bits, -1.0 if cls == 'neg' else np.exp(1j * (0.5 + 0.29 * k))), diag_on(comp, np.exp(0.9j + 0.1j * k)),
              (0, R[t], ru(rng))]
      add(f'grp_{cls}_{ci}', n0, {}, g)
  # groups without register mask: a sign flip / a phase on lane bits, a global phase; flag bit 9 of the op set and unset
  rng = rng_for('grp0')
  add('grp_nomask', n0, {}, [(0, 1, Z), (0, 1, ru(rng)), (0, 2, ph(0.8)), (0, 2, rr(rng)), diag_on([3, 4], -1.0), diag_on([3, R[0]], -1.0),
                             (0, 3, rr(rng)), (0, R[0], np.exp(0.3j) * np.eye(2)), (0, R[0], ru(rng)), diag_on([0, 5], np.exp(0.2j)),
                             (0, 5, Z), (0, 5, ru(rng))])
  # general groups: a lane table on every register mask (and none) ...
  for ci, chunk in enumerate(_chunks([()] + masks, 12)):
    rng = rng_for(f'ltab{ci}')
    g = []
    for k, m in enumerate(chunk):
      t = R[m[k % len(m)]] if m else 2
      regs = [R[i] for i in m]
      l0, l1 = (0, 1) if m else (0, 1)
      g += [diag_on(regs + [l0] + ([] if m else [2]), np.exp(1j * (0.3 + 0.2 * k))), diag_on(regs + [l1] + ([] if m else [2]), np.exp(1j * (1.1 + 0.1 * k))),
            (0, t, ru(rng))]
    add(f'grp_ltab_{ci}', n0, {}, g)
  # ... chunk tables, outside terms and sign-flip outside terms (bits outside the tile: n0 + 2, nothing dense on the top bits)
  n2 = n0 + 2
  while (n2 - 1 - (3 if bw == 128 else 4)) // 8 != (n2 - 2 - (3 if bw == 128 else 4)) // 8:
    n2 += 1          # (a chunk table covers eight index bits from the line bits up: both outside bits in one window)
  o1, o2 = n2 - 1, n2 - 2
  for kind in ('tab', 'oterm', 'sot'):
    for ci, chunk in enumerate(_chunks([()] + masks, 12)):
      rng = rng_for(f'{kind}{ci}')
      g = [(0, b, ru(rng)) for b in R[:1]]
      for k, m in enumerate(chunk):
        regs = [R[i] for i in m] if m else [1]
        t = regs[k % len(regs)]
        if kind == 'tab':
          g += [diag_on(regs + [o1], np.exp(1j * (0.3 + 0.2 * k))), diag_on(regs + [o2], np.exp(1j * (0.7 + 0.1 * k)))]
        elif kind == 'oterm':
          g += [diag_on(regs + [o1 if k % 2 else o2], np.exp(1j * (0.3 + 0.2 * k)))] + ([diag_on(regs + [o1, o2], np.exp(0.45j))] if k % 3 == 0 else [])
        else:
          g += [diag_on(regs + [o1 if k % 2 else o2], -1.0)] + ([diag_on(regs + [o1, o2], -1.0)] if k % 3 == 0 else [])
        g += [(0, t, ru(rng))]
      add(f'grp_{kind}_{ci}', n2, {}, g)
  # factor trees: the controlled phases between one register bit and the others (a QFT's ladder), base factor from the
  # header and from the general path (a lane table on the same register bit)
  if rb >= 3:
    for gen in (False, True):
      for ci, chunk in enumerate(_chunks(range(rb), 3 if gen else 4)):
        rng = rng_for(f'bitfac{gen}{ci}')
        g = []
        for j in chunk:
          g += [diag_on([R[j]], np.exp(0.21j * (j + 1)))]
          g += [diag_on([R[j], R[i]], np.exp(1j * np.pi / 2 ** (1 + abs(i - j)))) for i in range(rb) if i != j]
          if gen:
            g += [diag_on([R[j], 0], np.exp(0.33j)), diag_on([R[j], 1], np.exp(0.44j))]
          g += [(0, R[j], ru(rng) if j % 2 else BF[0])]
        if not any(np.count_nonzero(x[2]) == 4 and abs(abs(x[2][0, 0]) - _S) > 1e-9 for x in g):
          g += [(0, 0, ru(rng))]
        add(f'bitfac_{"gen" if gen else "hdr"}_{ci}', n0, {}, g)
  # wave bits (OP_WSWAP): one and two, stored in place and re-laid out; fixed bits
  for nw in (1, 2):
    n = n0 + nw
    rng = rng_for(f'wave{nw}')
    hi = list(range(6, n))
    g = [(0, b, [BF[0], ru(rng), BF[3], rr(rng)][i % 4]) for i, b in enumerate(hi)]
    g += [diag_on([hi[-1], hi[0]], np.exp(0.4j)), diag_on([hi[-1], 2], -1.0), (0, hi[-1], BF[1]), (0, hi[0], ru(rng)), (1 << hi[-1], hi[1], ru(rng)),
          (0, 4, BF[2]), (0, hi[-2], ru(rng))]
    add(f'wave{nw}', n, {'QH_WAVE_BITS': str(nw)}, g)
    add(f'wave{nw}_norelayout', n + 1, {'QH_WAVE_BITS': str(nw), 'QH_RELAYOUT': '0'},
        [(c, t + 1 if t >= 6 else t, m) for c, t, m in g if not c] + [diag_on([6, n], np.exp(0.3j)), (0, n, ru(rng))])
    add(f'wave{nw}_relayout', n + 1, {'QH_WAVE_BITS': str(nw)},
        [(c, t + 1 if t >= 6 else t, m) for c, t, m in g if not c] + [diag_on([6, n], np.exp(0.3j)), (0, n, ru(rng))])
  rng = rng_for('fixed')
  top = n0
  add('fixed', n0 + 1, {}, [(1 << top, R[0], ru(rng)), (1 << top, R[1], BF[0]), (1 << top | 1 << R[0], R[1], Z), (1 << top, 2, rr(rng)),
                            (1 << top, R[1], ru(rng))])
  return cases


def build_cases():
  out = []
  for bw, rb in ISLANDS:
    out += _island_cases(bw, rb)
  names = [c.name for c in out]
  assert len(set(names)) == len(names)
  return out


CASES = build_cases()


def load_claims():
  with open(CLAIMS_PATH) as f:
    return {k: set(v) for k, v in json.load(f).items()}


# ---- what a case reaches: read from the engine ---------------------------------------------------------
def queue_case(lib, handle, case):
  for cm, t, g in case.gates:
    g8 = np.ascontiguousarray(np.asarray(g, dtype=np.complex128).reshape(4)).view(np.float64)
    native.check(lib.qh_apply_bits(handle, int(cm), int(t), g8.ctypes.data_as(_dp)))


def plan_handlers(lib, handle):
  """qh_plan_handlers, parsed: [{bw, rb, nwave, relayout, ops: [(kind, flags)], groups: [flags]}]"""
  need = ctypes.c_uint64()
  native.check(lib.qh_plan_handlers(handle, None, 0, ctypes.byref(need)))
  buf = np.zeros(need.value // 4, dtype=np.uint32)
  native.check(lib.qh_plan_handlers(handle, buf.ctypes.data, need.value, None))
  assert int(buf[0]) == MAGIC
  pos, out = 2, []
  for _ in range(int(buf[1])):
    bw, rb, nwave, relayout, n_ops, n_groups = (int(x) for x in buf[pos:pos + 6])
    pos += 6
    ops = [(int(buf[pos + 2 * k]), int(buf[pos + 2 * k + 1])) for k in range(n_ops)]
    pos += 2 * n_ops
    groups = [int(x) for x in buf[pos:pos + n_groups]]
    pos += n_groups
    out.append({'bw': bw, 'rb': rb, 'nwave': nwave, 'relayout': relayout, 'ops': ops, 'groups': groups})
  assert pos in (buf.size, buf.size - 1)
  return out


class EnvPatch:
  """the planner reads its switches from the environment at every planning call"""

  def __init__(self, env):
    self.env = env

  def __enter__(self):
    self.old = {k: os.environ.get(k) for k in self.env}
    os.environ.update(self.env)

  def __exit__(self, *a):
    for k, v in self.old.items():
      if v is None:
        os.environ.pop(k, None)
      else:
        os.environ[k] = v


def dry_plan(case):
  """(handler words, exported plan) of the case on a planner-only handle, under the case's switches"""
  lib = native.load()
  h = ctypes.c_void_p()
  native.check(lib.qh_create_dry(case.n, case.island[0], ctypes.byref(h)))
  try:
    native.check(lib.qh_set_fusion(h, native.QH_FUSE_SWEEP))
    queue_case(lib, h, case)
    with EnvPatch(case.env):
      words = plan_handlers(lib, h)
      sweeps, _ = plan_interp.export_plan(h)
  finally:
    lib.qh_destroy(h)
  return words, sweeps


GROUP_KEY_BITS = 0xff14      # handler number, general path, sign-flip outside terms


def handler_numbers():
  """the constants of qcc_amd/csrc/sweep_handlers.inc (kHidDiag, kHidBflyReg, ...), by name"""
  import re
  text = open(os.path.join(ROOT, 'qcc_amd', 'csrc', 'sweep_handlers.inc')).read()
  text = re.sub(r'//.*', '', text)
  return {k: int(v) for k, v in re.findall(r'\b(k[A-Z][A-Za-z0-9]*)\s*=\s*(\d+)', text)}


def reached(case, words, sweeps):
  """{key: [(sweep, 'op' | 'grp', index)]}: the handlers of the case's island its plan dispatches, and where.  Handler numbers
  and group flags are the device words of qh_plan_handlers; the exported plan only says which groups belong to which op
  (a DIAG op folded into its header dispatches no group) and which tables a group carries."""
  out = collections.defaultdict(list)
  diag_hid = handler_numbers()['kHidDiag']
  assert len(words) == len(sweeps)
  for si, (w, sp) in enumerate(zip(words, sweeps)):
    assert w['rb'] == sp['rb'] and len(w['ops']) == len(sp['ops']) and len(w['groups']) == len(sp['groups'])
    if (w['bw'], w['rb']) != tuple(case.island):
      continue
    out[f'feat:nwave{w["nwave"]}'].append((si, 'sweep', 0))
    out['feat:store_relayout' if w['relayout'] else 'feat:store_inplace'].append((si, 'sweep', 0))
    for oi, ((kind, flags), op) in enumerate(zip(w['ops'], sp['ops'])):
      hid, k = kind >> 16, kind & 0xffff
      assert k == int(op['kind'])
      out[f'op:{hid}'].append((si, 'op', oi))
      if k == plan_interp.OP_DIAG:
        out['feat:diag_signflip_c' if flags & (1 << 9) else 'feat:diag_general_c'].append((si, 'op', oi))
        if hid != diag_hid:
          continue
        for gi in range(int(op['group_off']), int(op['group_off']) + int(op['n_groups'])):
          gf, g = w['groups'][gi], sp['groups'][gi]
          out[f'grp:{gf & GROUP_KEY_BITS}'].append((si, 'grp', gi))
          if int(g['flags']) & plan_interp.DG_LTAB:
            out['feat:group_lane_table'].append((si, 'grp', gi))
          if int(g['ntab']):
            out['feat:group_chunk_table'].append((si, 'grp', gi))
          if int(g['n_oterms']):
            out['feat:group_outside_terms'].append((si, 'grp', gi))
      elif k in (plan_interp.OP_DENSE_REG, plan_interp.OP_DENSE_LANE):
        where = 'lane' if k == plan_interp.OP_DENSE_LANE else 'reg'
        if flags & plan_interp.OPF_BFLY:
          if flags & plan_interp.OPF_LANE_DPP:
            out['feat:dpp_bfly_swap_ri' if flags & plan_interp.OPF_SWAP_RI else 'feat:dpp_bfly_plain'].append((si, 'op', oi))
          continue
        out[f'feat:dense_{where}_{"real" if flags & plan_interp.OPF_REAL else "general"}'].append((si, 'op', oi))
        if flags & plan_interp.OPF_LANE_DPP:
          out['feat:dense_lane_real_dpp'].append((si, 'op', oi))
        if flags & 2:
          out['feat:dense_lane_use_c'].append((si, 'op', oi))
        cm_reg, cmt = int(op['cm_reg']), int(op['cm_thread'])
        if cm_reg & 0x3f:
          out[f'feat:dense_{where}_ctl_reg_one'].append((si, 'op', oi))
        if (cm_reg >> 8) & 0x3f:
          out[f'feat:dense_{where}_ctl_reg_zero'].append((si, 'op', oi))
        if cmt:
          out[f'feat:dense_{where}_ctl_thread'].append((si, 'op', oi))
  return out


def without(sweeps, where):
  """the exported plan with one op deleted / one group made neutral"""
  si, what, idx = where
  sp = dict(sweeps[si])
  if what == 'op':
    sp['ops'] = np.delete(sp['ops'], idx)
  else:
    groups = sp['groups'].copy()
    g = np.zeros((), dtype=plan_interp.GROUP_DT)
    g['re'] = 1.0
    groups[idx] = g
    sp['groups'] = groups
  return sweeps[:si] + [sp] + sweeps[si + 1:]


def case_state(case):
  rng = np.random.default_rng(zlib.crc32(case.name.encode()) ^ 0x5eed)
  p = rng.standard_normal(1 << case.n) + 1j * rng.standard_normal(1 << case.n)
  return (p / np.linalg.norm(p)).astype(np.complex128)


def oracle_apply(oracle, psi, case):
  """the case's stream on `psi` (complex128 or complex64) through the CPU oracle"""
  n = case.n
  idx = None
  for cm, t, g in case.gates:
    ctl = [b for b in range(n) if (cm >> b) & 1]
    if not ctl:
      oracle.apply1(psi, g, n, n - 1 - t)
    elif len(ctl) == 1:
      oracle.applyc(psi, g, n, n - 1 - ctl[0], n - 1 - t)
    else:
      if idx is None:
        idx = np.arange(1 << n, dtype=np.uint64)
      sel = (idx & np.uint64(cm)) == np.uint64(cm)
      tmp = psi.copy()
      oracle.apply1(tmp, g, n, n - 1 - t)
      psi[sel] = tmp[sel]
  return psi


VISIBLE_MIN = 1e-6
EXEMPT_KINDS = (plan_interp.OP_LSWAP, plan_interp.OP_WSWAP)    # bookkeeping in the interpreter


def visible_instances(case, sweeps, instances, psi0, base, first_only=True):
  """the instances (the first one only, by default) whose deletion moves the interpreted result by more than VISIBLE_MIN"""
  out = []
  for where in instances:
    si, what, idx = where
    if what == 'sweep' or (what == 'op' and int(sweeps[si]['ops'][idx]['kind']) in EXEMPT_KINDS):
      out.append(where)
    elif float(np.max(np.abs(plan_interp.run_plan(psi0.copy(), without(sweeps, where), case.n) - base))) > VISIBLE_MIN:
      out.append(where)
    if out and first_only:
      break
  return out


def compute_claims(case):
  words, sweeps = dry_plan(case)
  r = reached(case, words, sweeps)
  psi0 = case_state(case)
  base = plan_interp.run_plan(psi0.copy(), sweeps, case.n)
  claims = []
  for key, inst in sorted(r.items()):
    if visible_instances(case, sweeps, inst[:3], psi0, base):
      claims.append(key)
  return claims


if __name__ == '__main__':
  import sys
  if '--write-claims' in sys.argv:
    native.build()
    data = {c.name: compute_claims(c) for c in CASES}
    with open(CLAIMS_PATH, 'w') as f:
      json.dump(data, f, indent=0, sort_keys=True)
    print(f'{len(CASES)} cases, {sum(len(v) for v in data.values())} claims -> {CLAIMS_PATH}')
