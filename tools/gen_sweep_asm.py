#!/usr/bin/env python3
"""Generates qcc_amd/csrc/sweep_island_rb{2..5}.inc: the per-tile body of the
fused sweep kernel (kernels_sweep.hip.h) as gfx950 assembly with FIXED physical
registers.

Why assembly: the tile (2^RB complex128 amplitudes per lane = up to 128 VGPRs)
must stay in the same registers across an interpreter loop over queued gate ops.
hipcc's register allocator copies the whole tile at every op-kind branch (2x the
VGPRs, spills at RB=5, one v_mov per amplitude per op), so the loop is written
by hand: every op updates the tile in place.

Two element types: complex128 (sweep_island_rb*.inc, a real number = a VGPR
pair) and complex64 (sweep_island_f32_rb*.inc, one VGPR per real number; the op
stream -- matrices, phase factors, tables -- stays double precision in memory and
is converted with v_cvt_f32_f64 as it is read).

Structure: an Island holds what one (rb, wide, prof, nomem) fixes -- the element-type helpers, the width-dependent
temporaries, the unique-label counter -- and has one method per section of the island; each returns its own Asm.
gen() is the table of contents: it builds the sections in emission order and hands them to layout(), which decides
what goes in front of the entry.  The branch table, sweep_handlers.inc and the register-mask order all come from
OP_FAMILIES / group_handlers() / reg_masks() below.

Register map (island-private, declared as clobbers to the compiler), complex128:
  v[T0+4k .. T0+4k+3]   tile slot k: x = v[+0:+1], y = v[+2:+3]; T0 = 40
  v16..v39              24 temporaries, reused per op kind (see "VGPR temporaries by context" below)
                        => 168 VGPRs at RB=5: THREE waves per SIMD
  s36..s99              scalar state: the roles that outlive a few instructions are named under "SGPR roles" below
                        (parameter block, op header OP_*, gate matrix / group header G_*, cursors); the rest is scratch
  NEXT_HDR              header of the NEXT op (prefetched); TAB = address of the handler table
                        during the op loop (ops and DIAG-group apply code are reached by s_setpc_b64
                        into a table of s_branch instructions; the host numbers the handlers: see OP_FAMILIES),
                        store base at the end
Operands supplied by the C++ kernel: see "inline-asm operands" below.
Data layouts must match planner.h (SweepOp 96 B, DGroup 64 B, OTerm 24 B) and
kernels_sweep.hip.h (SweepParams: slot byte offsets at +0x40).
"""
import os
import sys

# streaming tile loads/stores are non-temporal (each byte is touched once per sweep).  Round 3 tried the other cache-policy
# bits on loads and stores separately, a window on the loads in flight per wave and 4 / 16 slot offsets per scalar round
# trip (profiles/r03/cache_policy_ab.txt): nothing beat `nt` on both, 8 offsets per round trip; the switches are gone.
NT = ' nt'
LD_BITS = ST_BITS = NT
T0 = 40
TEMP_LO, TEMP_HI = 16, 39
# Measurement variants (arguments of gen(); main() takes them from the environment):
# prof (QH_ISLAND_PROF=1): a measurement build of the complex128 RB=5 island (sweep_island_prof_rb5.inc, compiled
# only with -DQH_PROF, tools/probes/prof_island.sh): sampled waves write s_memtime at the start, after the
# tile has arrived, at the head of every op, after the stores are issued and after they have completed.
# nomem (QH_ISLAND_NOMEM=1 / 2): TIMING experiments only (wrong results): islands without their tile loads AND stores /
# without the stores -- what a sweep costs when nothing but the op stream runs (tools/probes/r04_nomem.sh)

# --- inline-asm operands ---------------------------------------------------------------------
BLO, BHI = '%[blo]', '%[bhi]'          # tile base address lo, hi (SGPR)
PRM = '%[prm]'                         # SweepParams* (SGPR pair)
TIDX = '%[tidx]'                       # tile index (idx_high|base) (SGPR pair, for outside-bit predicates)
VOFF = '%[voff]'                       # this lane's byte offset inside a tile (VGPR)
LANE = '%[lane]'                       # lane id (VGPR)
ITLO, ITHI = '%[itlo]', '%[ithi]'      # thread index lo, hi (VGPR)
WAVE, LDS, LTAB = '%[wave]', '%[lds]', '%[ltab]'     # wave of the workgroup, LDS exchange buffer, lane tables in LDS (SGPR)
SBLO, SBHI, SVOFF = '%[sblo]', '%[sbhi]', '%[svoff]'   # the store's base and lane offset
NLT, WGTHR, TENT, PROW = '%[nlt]', '%[wgthr]', '%[tent]', '%[prow]'

# --- SGPR roles ------------------------------------------------------------------------------
# parameter block (SweepParams +0x0 .. +0x1f)
OPS, OPS_LO, OPS_HI = 's[36:37]', 's36', 's37'        # cursor: the op that runs
GROUPS_LO, GROUPS_HI = 's38', 's39'                   # groups base
OTERMS_LO, OTERMS_HI = 's40', 's41'                   # oterms base
TABLES_REL = 's43'                                    # tables - groups (bytes); s42 = number of ops (unused: a sentinel ends the list)
NEXT_HDR = 's[16:23]'                                 # header of the next op
TAB, TAB_LO, TAB_HI = 's[24:25]', 's24', 's25'        # handler table (store base at the end)
# op header (device copy of SweepOp words 0..7): kind tb cm_reg n_groups cm_thread(2) group_off flags
OP_KIND, OP_TB, OP_CM_REG, OP_NGROUPS, OP_CMT_LO, OP_CMT_HI, OP_GROUP_OFF, OP_FLAGS = (f's{44 + i}' for i in range(8))
OP_CM_THREAD = 's[48:49]'
OP_W23 = 's[46:47]'                                   # words cm_reg / n_groups as a pair (fused rotations, inlined DIAG factor)
# group header (DGroup): lane_mask reg_mask oterm_off n_oterms re(2) im(2) flags ltab_off ntab tab_shift tab_off[4];
# a dense op keeps its matrix g[8] in the same registers
G_HDR, MAT0 = 's[52:67]', 52


def G(i):
  """Double i of a dense op's matrix g[8] (g0r g0i g1r g1i g2r g2i g3r g3i) as it sits in the SGPRs."""
  return f's[{MAT0 + 2 * i}:{MAT0 + 2 * i + 1}]'


G_LANE_MASK, G_REG_MASK, G_OTERM_OFF, G_N_OTERMS = 's52', 's53', 's54', 's55'
G_PHI0_RE, G_PHI0_IM, G_PHI0_DW = 's[56:57]', 's[58:59]', ('s56', 's57', 's58', 's59')
G_FLAGS, G_LTAB_OFF, G_NTAB, G_TAB_SHIFT = 's60', 's61', 's62', 's63'
G_TAB_OFF = ('s64', 's65', 's66', 's67')
GRP, GRP_LO, GRP_HI = 's[92:93]', 's92', 's93'        # cursor: the group whose header is loaded
# flag bits the islands test (planner.h OPF_* / DG_*, as bit positions; *_FIELD: s_bfe operand, width << 16 | position)
OPF_DEFER_C, OPF_USE_C, OPF_REAL, OPF_LANE_DPP, OPF_C_SIGN = 0, 1, 2, 7, 9      # (C_SIGN: device copy only)
OPF_BFLY_FIELD, OPF_SWAP_RI_FIELD = 0x30004, 0x10008                             # variant; partner's re/im exchanged
DG_LTAB, DG_LTAB_LDS, DG_GENERAL, DG_SIGN_OTERMS = 0, 1, 2, 4                    # (GENERAL, SIGN_OTERMS: device copy only)
DG_HANDLER_FIELD = 0x80008


# --- handlers: ONE description of the islands' branch table -------------------------------------
# The host writes a handler number into the device copy of every op and group (through the generated sweep_handlers.inc).
# What must agree with this description in kernels_sweep.hip.h:
#   op_handler_id       the op families below: constant + offset
#   reg_mask_number     the position of a register mask in reg_masks() (kHidDiag1: + 16 * class + that number, 15 = any other)
#   group_handler_bits  the order of group_handlers(), whose entries follow the NHID op handlers in the table
def reg_masks(rb):
  """Register masks with straight-line apply code, in handler order: the 1-bit masks, then the 2-bit masks (b0 < b1, b0 major).
  (kernels_sweep.hip.h knows this list as d1_masks and the first numbers of OP_FAMILIES as HID_*.)"""
  return [1 << b for b in range(rb)] + [(1 << b0) | (1 << b1) for b0 in range(rb) for b1 in range(b0 + 1, rb)]


BFLY_VARIANTS, ROTATIONS, D1_CLASSES = range(5), range(2), 'nul'
# (constant of sweep_handlers.inc, first number, rb -> {offset: label}, complex128 only)
OP_FAMILIES = (
    ('kHidDiag', 0, lambda rb: {0: 'L_diag'}, False),
    ('kHidDense', 1, lambda rb: {0: 'L_dense'}, False),
    ('kHidWswap', 2, lambda rb: {0: 'L_wswap'}, False),
    ('kHidBflyLane', 3, lambda rb: {0: 'L_bfl_e'}, False),
    ('kHidBflyLaneDpp', 4, lambda rb: {0: 'L_dpp'}, False),
    ('kHidDone', 5, lambda rb: {0: 'L_done'}, False),
    ('kHidLswap', 8, lambda rb: {2 * r + w: f'L_lswap{16 << w}_r{r}' for r in range(rb) for w in range(2)}, False),
    ('kHidBflyReg', 24, lambda rb: {8 * v + b: f'L_bf{v}_{b}' for v in BFLY_VARIANTS for b in range(rb)}, False),
    ('kHidBflyRot', 64, lambda rb: {8 * (5 * r + v) + b: f'L_bfr{r}{v}_{b}'
                                    for r in ROTATIONS for v in BFLY_VARIANTS for b in range(rb)}, True),
    ('kHidDiag1', 144, lambda rb: {16 * c + mi: f'L_d1{cls}{m}' for c, cls in enumerate(D1_CLASSES)
                                   for mi, m in list(enumerate(reg_masks(rb))) + [(15, 'x')]}, True),
)
NHID = 192


def op_handlers(rb, wide):
  """Label of every op handler number (unused numbers go on to the next op)."""
  targets = ['L_next'] * NHID
  for _, first, labels, wide_only in OP_FAMILIES:
    if wide or not wide_only:
      for off, label in labels(rb).items():
        targets[first + off] = label
  return targets


def group_handlers(rb):
  """Apply handlers of DIAG groups, in table order: per class (vector factor, factor -1, uniform factor, lane-masked factor)
  no mask, reg_masks(), any other mask; the factor trees (one per register bit) follow the classes that have them."""
  out = []
  for cls, tree in (('m', 'L_gbf'), ('n', None), ('u', None), ('l', 'L_gbl')):
    out += [f'L_g{cls}0'] + [f'L_g{cls}{m}' for m in reg_masks(rb)] + [f'L_g{cls}x']
    if tree:
      out += [f'{tree}{j}' for j in range(rb)]
  return out


def handlers_header():
  consts = [f'{name} = {first}' for name, first, _, _ in OP_FAMILIES] + [f'kNumOpHandlers = {NHID}']
  pad = ' ' * len('constexpr uint32_t ')
  return ('// GENERATED by tools/gen_sweep_asm.py -- do not edit: handler numbers of the sweep islands\' branch table.\n'
          '// LSWAP: + 2 * register bit + (lane bit - 4); register butterfly: + 8 * variant + register bit;\n'
          '// register butterfly behind a (1 +- i) x scale phase on its target (OPF_ROT_P / OPF_ROT_M): + 8 * (5 * rotation + variant) + register bit.\n'
          'constexpr uint32_t ' + ', '.join(consts[0:4]) + ',\n' +
          pad + ', '.join(consts[4:8]) + ',\n'
          '// DIAG op of ONE simple group with a register mask, inlined into its header (kernels_sweep.hip.h inline_single_group):\n'
          '// + 16 * class (0 factor -1, 1 uniform factor, 2 lane-masked factor) + mask number (1-bit masks, 2-bit masks, 15 = any other).\n' +
          pad + ', '.join(consts[8:]) + ';\n')


class Asm:
  """One section of an island.  front: laid out before the entry; cut: the part of the body that moves in front of the
  dispatcher (see layout) may end where this section starts; falls_into: the one section it may run on into."""

  def __init__(self, name, front=False, cut=False, falls_into=None):
    self.name, self.front, self.cut, self.falls_into = name, front, cut, falls_into
    self.lines = []

  def __call__(self, s):
    self.lines.append(s)

  def label(self, name):
    self.lines.append(f'{name}_%=:')

  def ends_in_jump(self):
    return bool(self.lines) and self.lines[-1].startswith(('s_branch ', 's_setpc_b64 '))


def L(name):
  return f'{name}_%='


def pairs(b, nr):
  """Slot pairs (k0, k1) a gate on register bit b acts on: k1 = k0 | 1 << b."""
  out = []
  for h in range(nr // 2):
    k0 = ((h >> b) << (b + 1)) | (h & ((1 << b) - 1))
    out.append((k0, k0 | (1 << b)))
  return out


# --- VGPR temporaries by context -------------------------------------------------------
# common
V_A, V_B = 16, 17
# dense register op: 4 result temporaries
R_T = [30, 32, 34, 36]
# dense lane op
LN_ADDR = 16
LN_TMP = 17
LN_COEF = {'car': 18, 'cai': 20, 'cbr': 22, 'cbi': 24}
LN_BUF = [26, 30]          # two shuffle buffers of 4 dwords
LN_T = [34, 36]
# diagonal op: c, the wave-uniform u and the per-lane factor f depend on the element type (Island.D_C, D_U, D_F)
D_TMP = [30, 32, 34, 36]   # cmul temporaries (4 slots interleaved)
D_LTAB = 34                # lane-table entry lands in v[34:37] (free until the apply phase)

# --- unit-entry butterflies (OPF_BFLY): the gate is c*M with M's entries in {1,-1,i,-i};
# the planner moved c into another op of the sweep, so M costs adds only, in place.
#   variant (flags bits 4..6): 0  [[1, 1],[ 1,-1]]  (h)        1  [[1,-1],[1,1]]  (yroot)
#   2  [[1,1],[-1,1]] (yroot^+)   3  [[1,-i],[-i,1]] (v, sqrt-x)   4  [[1,i],[i,1]] (v^+)
# On a pair (a, b), components 0 = re, 1 = im:
#   first   a'[dst] = a[dst] +- b[src]                 as (dst, src, sign)
#   second  b'[dst] = +-2 b[dst] +- a'[src]            as (dst, sign of the 2, sign of a', src)
#   pk1, pk2   complex64: the same two steps as ONE packed add / fma each ((re, im) of a slot = one 64-bit register pair;
#              K = (2, 2), signs and the re/im exchange of the v gates by neg_* / op_sel)
BFLY = {
    0: dict(first=((0, 0, ''), (1, 1, '')), second=((0, '-', '', 0), (1, '-', '', 1)),             # a' = a + b ; b' = a - b = a' - 2b
            pk1='', pk2=' neg_lo:[0,1,0] neg_hi:[0,1,0]'),
    1: dict(first=((0, 0, '-'), (1, 1, '-')), second=((0, '', '', 0), (1, '', '', 1)),             # a' = a - b ; b' = a + b = a' + 2b
            pk1=' neg_lo:[0,1] neg_hi:[0,1]', pk2=''),
    2: dict(first=((0, 0, ''), (1, 1, '')), second=((0, '', '-', 0), (1, '', '-', 1)),             # a' = a + b ; b' = b - a = 2b - a'
            pk1='', pk2=' neg_lo:[0,0,1] neg_hi:[0,0,1]'),
    3: dict(first=((0, 1, ''), (1, 0, '-')), second=((1, '', '-', 0), (0, '', '', 1)),             # a' = a - i b ; b' = b - i a:
            pk1=' op_sel:[0,1] op_sel_hi:[1,0] neg_hi:[0,1]',                                      #   a' = (ar + bi, ai - br)
            pk2=' op_sel:[0,0,1] op_sel_hi:[1,1,0] neg_hi:[0,0,1]'),                               #   b' = (2br + ai', 2bi - ar')
    4: dict(first=((0, 1, '-'), (1, 0, '')), second=((1, '', '', 0), (0, '', '-', 1)),             # a' = a + i b ; b' = b + i a:
            pk1=' op_sel:[0,1] op_sel_hi:[1,0] neg_lo:[0,1]',                                      #   a' = (ar - bi, ai + br)
            pk2=' op_sel:[0,0,1] op_sel_hi:[1,1,0] neg_lo:[0,0,1]'),                               #   b' = (2br - ai', 2bi + ar')
}
# lane-bit butterflies fetch the partner with DPP moves when the bit is 0..3
DPP1 = {0: ['quad_perm:[1,0,3,2]'], 1: ['quad_perm:[2,3,0,1]'],
        2: ['row_half_mirror', 'quad_perm:[3,2,1,0]'], 3: ['row_ror:8']}


def vpair(r):
  """'v26' -> 'v[26:27]'"""
  n = int(r[1:])
  return f'v[{n}:{n + 1}]'


def pk_cmul(a, dst, src, f, tmp):
  """complex64, packed: dst = src * f (register pairs (re, im); dst may be src; tmp another pair)."""
  a(f'v_pk_mul_f32 {tmp}, {src}, {f} op_sel_hi:[1,0]')                                    # (x fr, y fr)
  a(f'v_pk_fma_f32 {dst}, {src}, {f}, {tmp} op_sel:[1,1,0] op_sel_hi:[0,1,1] neg_lo:[0,1,0]')   # (x fr - y fi, y fr + x fi)


def ctl_skip(a, k, skip):
  """Register-bit controls of a dense op (s76: bits that must be one, s77: that must be zero): slot k is skipped when it misses one."""
  a(f's_andn2_b32 s74, s76, {k}')
  a(f's_and_b32 s75, s77, {k}')
  a('s_or_b32 s74, s74, s75')
  a('s_cmp_eq_u32 s74, 0')
  a(f's_cbranch_scc0 {L(skip)}')


def mask_skip(a, k, skip):
  """Register mask of a DIAG group in s72: slot k is skipped unless its index holds every bit of it."""
  a(f's_andn2_b32 s74, s72, {k}')
  a('s_cmp_eq_u32 s74, 0')
  a(f's_cbranch_scc0 {L(skip)}')


def sel64(a, v, lo, hi):
  """v[v:v+1] = vcc ? s[hi:hi+1] : s[lo:lo+1] (doubles, per lane)."""
  for d in range(2):
    a(f'v_mov_b32 v{v + d}, s{lo + d}')
    a(f'v_mov_b32 v{LN_TMP}, s{hi + d}')
    a(f'v_cndmask_b32 v{v + d}, v{v + d}, v{LN_TMP}, vcc')


def dpp_fetch(a, q, tq, src, steps):
  """v[q..] = the dwords `src` of the partner lane, by one DPP move each or two through v[tq..]."""
  nd = len(src)
  if len(steps) == 1:
    for d in range(nd):
      a(f'v_mov_b32_dpp v{q + d}, v{src[d]} {steps[0]} row_mask:0xf bank_mask:0xf')
  else:
    for d in range(nd):
      a(f'v_mov_b32_dpp v{tq + d}, v{src[d]} {steps[0]} row_mask:0xf bank_mask:0xf')
    if nd < 3:
      a('s_nop 1')
    for d in range(nd):
      a(f'v_mov_b32_dpp v{q + d}, v{tq + d} {steps[1]} row_mask:0xf bank_mask:0xf')


class Island:
  """One island: everything (rb, wide, prof, nomem) fixes, and one method per section."""

  def __init__(self, rb, wide=True, prof=False, nomem=0):
    self.rb, self.wide, self.prof, self.nomem = rb, wide, prof, nomem
    self.nr = 1 << rb
    self.batch = min(8, self.nr)      # slots whose byte offsets are fetched (s_load) per round trip of the tile load / store
    self.W = w = 2 if wide else 1     # VGPRs per real number
    self.MUL, self.FMA, self.MOV = ('v_mul_f64', 'v_fma_f64', 'v_mov_b64') if wide else ('v_mul_f32', 'v_fma_f32', 'v_mov_b32')
    # (re, im) of a temporary complex number sit in ADJACENT registers: complex64 multiplies by them with
    # packed FP32 instructions (v_pk_mul_f32 / v_pk_fma_f32 take 64-bit register pairs)
    self.D_C, self.D_U, self.D_F = (18, 18 + w), (22, 22 + w), (26, 26 + w)   # c = cr + i ci; wave-uniform u; per-lane factor f
    self.cr, self.ci = self.V2(self.D_C[0]), self.V2(self.D_C[1])
    self.ur, self.ui = self.V2(self.D_U[0]), self.V2(self.D_U[1])
    self.fr, self.fi = self.V2(self.D_F[0]), self.V2(self.D_F[1])
    self.dt = self.V2(D_TMP[0])
    # the matrix of a dense op: complex128 reads it from the SGPRs, complex64 converts it first (load_matrix_f32)
    gnames = ['g0r', 'g0i', 'g1r', 'g1i', 'g2r', 'g2i', 'g3r', 'g3i']
    self.g = {nm: G(i) if wide else f'v{16 + i}' for i, nm in enumerate(gnames)}
    self.counters = {}

  # ---- element type ------------------------------------------------------------------------
  def T(self, k):
    return T0 + 2 * self.W * k

  def V2(self, i):
    """The real number held at temp index i (a VGPR pair for f64, one VGPR for f32)."""
    return f'v[{i}:{i + 1}]' if self.wide else f'v{i}'

  def X(self, k):
    return self.V2(self.T(k))

  def Y(self, k):
    return self.V2(self.T(k) + self.W)

  def XY(self, k):
    """Slot k as a register range (complex64: the pair the packed instructions take)."""
    return f'v[{self.T(k)}:{self.T(k) + 2 * self.W - 1}]'

  def ADDS(self, d, x, y, neg=False):
    """d = x + y (neg: d = x - y)."""
    if self.wide:
      return f'v_add_f64 {d}, {x}, {"-" if neg else ""}{y}'
    return f'{"v_sub_f32" if neg else "v_add_f32"} {d}, {x}, {y}'

  def uniq(self, prefix):
    """prefix1, prefix2, .. in emission order."""
    self.counters[prefix] = n = self.counters.get(prefix, 0) + 1
    return f'{prefix}{n}'

  def slots_of(self, m):
    return [k for k in range(self.nr) if (k & m) == m]

  def cmul_slots(self, a, slots, fr, fi, temps=None):
    """slot *= (fr,fi) for 1..4 slots, interleaved to hide the FP64 latency (temps: one temporary per slot, D_TMP if None;
    complex64 with the factor in an adjacent VGPR pair: packed arithmetic, the temporaries are register pairs)."""
    X, Y, XY, MUL, FMA = self.X, self.Y, self.XY, self.MUL, self.FMA
    packed = not self.wide and fr[0] == 'v' and fi == f'v{int(fr[1:]) + 1}'
    tm = temps or [f'v[{t}:{t + 1}]' if packed else self.V2(t) for t in D_TMP]
    assert len(slots) <= len(tm)
    if packed:
      f = vpair(fr)
      for t, k in zip(tm, slots):
        a(f'v_pk_mul_f32 {t}, {XY(k)}, {f} op_sel_hi:[1,0]')
      for t, k in zip(tm, slots):
        a(f'v_pk_fma_f32 {XY(k)}, {XY(k)}, {f}, {t} op_sel:[1,1,0] op_sel_hi:[0,1,1] neg_lo:[0,1,0]')
      return
    # t = y*fi ; y = y*fr ; y += x*fi ; x = x*fr - t   (4 FP64 ops, result in place)
    for t, k in zip(tm, slots):
      a(f'{MUL} {t}, {Y(k)}, {fi}')
    for t, k in zip(tm, slots):
      a(f'{MUL} {Y(k)}, {Y(k)}, {fr}')
    for t, k in zip(tm, slots):
      a(f'{FMA} {Y(k)}, {X(k)}, {fi}, {Y(k)}')
    for t, k in zip(tm, slots):
      a(f'{FMA} {X(k)}, {X(k)}, {fr}, -{t}')

  def cmul_vv(self, a, xr, xi, fr, fi, tmp):
    """(xr,xi) *= (fr,fi), all 64-bit register pairs (VGPR or SGPR factor)."""
    a(f'{self.MUL} {tmp}, {xi}, {fi}')
    a(f'{self.MUL} {xi}, {xi}, {fr}')
    a(f'{self.FMA} {xi}, {xr}, {fi}, {xi}')
    a(f'{self.FMA} {xr}, {xr}, {fr}, -{tmp}')

  def load_matrix_f32(self, a, first=16):
    """complex64 tile: the op's double-precision matrix -> 8 floats in v[first..first+7]."""
    if not self.wide:
      for i in range(8):
        a(f'v_cvt_f32_f64 v{first + i}, {G(i)}')

  # ---- pieces every section uses -------------------------------------------------------------
  def prof_rec(self, a, wait_stores=False, real_at=None):
    """s[30:31] = this wave's row of the profile buffer (0: not sampled), s101 = byte offset of the next record."""
    if not self.prof:
      return
    skip = self.uniq('L_prof')
    a('s_cmp_eq_u64 s[30:31], 0')
    a(f's_cbranch_scc1 {L(skip)}')
    if wait_stores:
      a('s_waitcnt vmcnt(0)')
    a('s_memtime s[28:29]')
    a('s_waitcnt lgkmcnt(0)')
    a('v_mov_b32 v30, s28')
    a('v_mov_b32 v31, s29')
    a('v_mov_b32 v32, s101')
    a('global_store_dwordx2 v32, v[30:31], s[30:31]')
    a('s_add_u32 s101, s101, 8')
    a('s_and_b32 s101, s101, 0x3ff')              # 128 records per row
    if real_at is not None:                       # the 100 MHz counter beside it: records 126 / 127 of the row
      a('s_memrealtime s[28:29]')
      a('s_waitcnt lgkmcnt(0)')
      a('v_mov_b32 v30, s28')
      a('v_mov_b32 v31, s29')
      a(f'v_mov_b32 v32, {real_at * 8}')
      a('global_store_dwordx2 v32, v[30:31], s[30:31]')
    a.label(skip)

  # The 32-byte op header (kind tb cm_reg n_groups cm_thread(2) group_off flags) of op i+1 is
  # fetched into NEXT_HDR while op i runs: the scalar-load latency (hundreds of cycles behind
  # the tile stream) is off the critical path.  The 64-byte matrix g[8] is loaded only by the
  # op kinds that read it (most ops of a QFT or supremacy sweep do not).
  # Dispatch: the host puts a handler number into the upper half of `kind` (kernels_sweep.hip.h op_handler_id);
  # TAB holds the address of a table of s_branch instructions, one per handler.  A taken branch
  # costs a wave ~50 cycles (the instruction buffer refills), and the compare-and-branch chains this
  # replaces took 3-5 of them per op plus 5-10 not-taken ones: ~400 cycles of the ~650 a 64-instruction
  # register butterfly held its wave (tools/probes/prof_island.sh).  Every handler ends with its own copy
  # of the loop head (next_op), so an op costs two jumps: s_setpc_b64 into the table, s_branch to the code.
  # The op list ends with a sentinel whose handler is the store (kHidDone): no counter, no end test.
  def op_head(self, a):
    self.prof_rec(a)
    a('s_waitcnt lgkmcnt(0)')
    a('s_mov_b64 s[44:45], s[16:17]')              # NEXT_HDR -> OP_KIND .. OP_FLAGS
    a(f's_mov_b64 {OP_W23}, s[18:19]')
    a(f's_mov_b64 {OP_CM_THREAD}, s[20:21]')
    a('s_mov_b64 s[50:51], s[22:23]')
    a(f's_load_dwordx8 {NEXT_HDR}, {OPS}, 0x60')   # next op's header (the buffer is padded: reading one past the end is harmless)
    a(f's_lshr_b32 s74, {OP_KIND}, 16')            # handler number
    a(f's_and_b32 {OP_KIND}, {OP_KIND}, 0xffff')   # kind
    a('s_lshl_b32 s74, s74, 2')
    a(f's_add_u32 s72, {TAB_LO}, s74')
    a(f's_addc_u32 s73, {TAB_HI}, 0')
    a('s_setpc_b64 s[72:73]')

  def next_op(self, a):
    a('s_mov_b64 exec, -1')                     # (waves are always full: 64 x k threads per block)
    a(f's_add_u32 {OPS_LO}, {OPS_LO}, 96')
    a(f's_addc_u32 {OPS_HI}, {OPS_HI}, 0')
    self.op_head(a)

  def lane_pipeline(self, a, first_buf, depth, combine_slot):
    """Partner values of slot k arrive by ds_bpermute `depth` slots ahead of their use
    (the shuffle latency, not its issue rate, bounds a lane op: SQ_WAIT_INST_LDS was 42%
    of the wave time with one slot of lookahead)."""
    nr, w2 = self.nr, 2 * self.W
    bufs = [first_buf + w2 * j for j in range(depth)]
    assert bufs[-1] + w2 - 1 <= TEMP_HI and (depth - 1) * w2 <= 15
    for k in range(min(depth, nr)):
      self.shuf(a, k, bufs[k % depth])
    for k in range(nr):
      ahead = min(k + depth - 1, nr - 1) - k
      a(f's_waitcnt lgkmcnt({ahead * w2})')
      buf = bufs[k % depth]
      combine_slot(k, self.V2(buf), self.V2(buf + self.W))
      if k + depth < nr:
        self.shuf(a, k + depth, buf)

  def shuf(self, a, k, buf):
    """v[buf..] = slot k of the partner lane (byte address in v[LN_ADDR])."""
    for d in range(2 * self.W):
      a(f'ds_bpermute_b32 v{buf + d}, v{LN_ADDR}, v{self.T(k) + d}')

  def lane_partner(self, a, m):
    """s<m> = 1 << tb: the partner lane's bpermute byte address, vcc = this lane holds the "1" element of the pair."""
    a(f's_lshl_b32 {m}, 1, {OP_TB}')
    a(f'v_xor_b32 v{LN_ADDR}, {m}, {LANE}')
    a(f'v_lshlrev_b32 v{LN_ADDR}, 2, v{LN_ADDR}')
    a(f'v_and_b32 v{LN_TMP}, {m}, {LANE}')
    a(f'v_cmp_ne_u32 vcc, 0, v{LN_TMP}')

  # ---- lane tables -> LDS, overlapped with the tile load ---------------------------------------------------
  # The first n_lt lane tables of the sweep (1 KiB each) live in LDS for the op loop.  Until round 3 the C++
  # prologue copied them (global loads from L2, ds writes, __syncthreads) BEFORE the island issued its tile loads:
  # ~1 us per workgroup = per tile with nothing in flight (complex64, whose tiles live half as long: 6 % of a sweep).
  # Now the waves of the workgroup share the tables out -- wave w takes tables w, w + W, .. -- and fetch each with ONE
  # global_load_lds_dwordx4 (gfx950: 64 lanes x 16 bytes = one table, straight from L2 into LDS at M0 + lane * 16, no
  # VGPRs), FIRST; the tile loads follow at once, and since loads complete in order `s_waitcnt vmcnt(<tile loads issued
  # since>)` says when the tables are in LDS: one barrier there, while the tile is still on its way.
  LT_MAX = 16                                      # (kernels_sweep.hip.h ltab_lds_count: at most 16 tables in LDS)

  def ltab_begin(self, a):
    a('s_waitcnt lgkmcnt(0)')                      # s[36:43]: groups base, tables - groups
    a(f's_mov_b32 s74, {NLT}')                     # tables to fetch (0: none, or not this turn of the wave's loop)
    a(f's_mov_b32 {TAB_LO}, m0')                   # (M0 is the compiler's: given back below)
    a('s_cmp_eq_u32 s74, 0')
    a(f's_cbranch_scc1 {L("L_lt_none")}')
    a(f's_add_u32 s72, {GROUPS_LO}, {TABLES_REL}')
    a(f's_addc_u32 s73, {GROUPS_HI}, 0')           # lane tables = the start of the sweep's tables
    a(f'v_lshlrev_b32 v{V_A}, 4, {LANE}')          # lane * 16
    a(f's_lshr_b32 s75, {WGTHR}, 6')               # W = waves of the workgroup
    a(f's_mov_b32 s76, {WAVE}')                    # table = wave, wave + W, ..
    for k in range(self.LT_MAX):
      a('s_cmp_ge_u32 s76, s74')
      a(f's_cbranch_scc1 {L("L_lt_none")}')
      a('s_lshl_b32 s77, s76, 10')
      a('s_add_u32 s78, s72, s77')
      a('s_addc_u32 s79, s73, 0')
      a(f's_add_u32 m0, {LTAB}, s77')
      a(f'global_load_lds_dwordx4 v{V_A}, s[78:79]')
      a('s_add_u32 s76, s76, s75')
    a.label('L_lt_none')
    a(f's_mov_b32 m0, {TAB_LO}')

  def ltab_after(self, a, loads_since):
    """Tile loads issued since the table loads: `loads_since` (<= 32: vmcnt counts to 63)."""
    a('s_cmp_eq_u32 s74, 0')
    a(f's_cbranch_scc1 {L("L_lt_done")}')
    a(f's_waitcnt vmcnt({loads_since})')
    a('s_barrier')
    a.label('L_lt_done')

  def tile_io(self, a, store, after_batch=None, before_first=None):
    # the store uses its own slot offsets (+0x240) and a base corrected by the index bits
    # OP_WSWAP moved between the wave id and the registers (they are not swapped back)
    # Slot byte offsets come from the sweep's parameter block, 8 per scalar load (s_load_dwordx16), into two register
    # sets in turn: the loads for batches 0 and 1 are issued together with everything else the phase needs, batch j + 2
    # is requested as soon as batch j's registers are consumed -- ONE scalar round trip in front of the first tile
    # load / store instead of one per batch (each cost the wave 500-700 cycles behind a saturated memory system:
    # profiles/r04/op_timeline_*.txt, "tile load" / "store issue" before and after).
    batch, nomem = self.batch, self.nomem
    blo, bhi, table = (TAB_LO, TAB_HI, 0x240) if store else (BLO, BHI, 0x40)
    nb = self.nr // batch
    sets = (52, 80)

    def fetch(j):
      base = sets[j & 1]
      a(f's_load_dwordx{2 * batch} s[{base}:{base + 2 * batch - 1}], {PRM}, {table + 8 * batch * j}')

    fetch(0)
    if nb > 1:
      fetch(1)
    if store:
      # in place: the load address corrected by the index bits OP_WSWAP moved (mask = ~0);
      # relayout sweep: the tile's own contiguous block of the second buffer (mask = 0, the
      # kernel passes that block's address and lane offsets as the store operands)
      a(f's_load_dwordx2 s[74:75], {PRM}, 0x28')  # SweepParams::store_delta_mask
      a(f's_mov_b64 s[72:73], {TIDX}')
      a(f's_sub_u32 {TAB_LO}, s72, s26')          # tile index now - tile index at load time
      a(f's_subb_u32 {TAB_HI}, s73, s27')
      a('s_waitcnt lgkmcnt(0)')
      a(f's_and_b64 {TAB}, {TAB}, s[74:75]')
      a(f's_lshl_b64 {TAB}, {TAB}, {2 + self.W}')
      a(f's_add_u32 {TAB_LO}, {TAB_LO}, {SBLO}')
      a(f's_addc_u32 {TAB_HI}, {TAB_HI}, {SBHI}')
    assert store or before_first                  # (someone has waited for batches 0 and 1 by now)
    if before_first:
      before_first()                              # (starts with s_waitcnt lgkmcnt(0))
    dw = 'dwordx4' if self.wide else 'dwordx2'
    for j in range(nb):
      if j >= 2:
        a('s_waitcnt lgkmcnt(0)')
      base = sets[j & 1]
      for i in range(batch):
        k = batch * j + i
        a(f's_add_u32 s98, {blo}, s{base + 2 * i}')
        a(f's_addc_u32 s99, {bhi}, s{base + 1 + 2 * i}')
        if store:
          if not nomem:
            a(f'global_store_{dw} {SVOFF}, {self.XY(k)}, s[98:99]' + ST_BITS)
        elif nomem != 1:
          a(f'global_load_{dw} {self.XY(k)}, {VOFF}, s[98:99]' + LD_BITS)
      if j + 2 < nb:
        fetch(j + 2)
      if after_batch:
        after_batch(batch * (j + 1))

  # ---- prologue: parameters, then one 1-KiB global_load_dwordx4 per slot ------------
  def prologue(self):
    a = Asm('prologue', falls_into='dispatcher')
    if self.prof:
      a(f's_mov_b64 s[30:31], {PROW}')
      a('s_mov_b32 s101, 0')
      self.prof_rec(a, real_at=126)
    a(f's_load_dwordx4 s[36:39], {PRM}, 0x0')   # ops cursor, groups base
    a(f's_load_dwordx2 s[40:41], {PRM}, 0x10')  # oterms base
    a(f's_load_dwordx2 s[42:43], {PRM}, 0x18')  # number of ops, tables - groups (bytes)
    lt_at = min(self.nr, 32)                    # (vmcnt counts to 63: complex64 RB=6 lands its tables after 32 of its 64 loads)
    self.tile_io(a, store=False, after_batch=lambda issued: self.ltab_after(a, issued) if issued == lt_at else None,
                 before_first=lambda: self.ltab_begin(a))
    a(f's_mov_b64 s[26:27], {TIDX}')                # tile index at load time (see the store)
    a(f's_load_dwordx8 {NEXT_HDR}, {OPS}, 0x0')     # header of the first op
    a('s_waitcnt vmcnt(0)')
    self.prof_rec(a)
    return a

  # ---- op loop: the handler table, the loop head, the generic dense op's way to its code ---------------------------
  def dispatcher(self):
    a, rb = Asm('dispatcher'), self.rb
    a(f's_getpc_b64 {TAB}')                       # address of the next instruction; the table starts 12 bytes on
    a(f's_add_u32 {TAB_LO}, {TAB_LO}, 12')
    a(f's_addc_u32 {TAB_HI}, {TAB_HI}, 0')
    a(f's_branch {L("L_op")}')
    for t in op_handlers(rb, self.wide) + group_handlers(rb):      # (apply handlers of DIAG groups: see L_diag)
      a(f's_branch {L(t)}')
    a.label('L_op')
    self.op_head(a)
    a.label('L_dense')
    a(f's_load_dwordx16 {G_HDR}, {OPS}, 0x20')     # g[8]
    # control predicate of this thread: (it & cm_thread) == cm_thread  -> s[68:69]
    # (zero-controls: header words n_groups / group_off of a dense op hold the bits of cm_thread
    # that must be 0; bits 8..12 of cm_reg the register bits that must be 0)
    a(f's_andn2_b32 s74, {OP_CMT_LO}, {OP_NGROUPS}')
    a(f's_andn2_b32 s75, {OP_CMT_HI}, {OP_GROUP_OFF}')
    a(f's_and_b32 s76, {OP_CM_REG}, {(1 << rb) - 1:#x}')      # register bits that must be one
    a(f's_bfe_u32 s77, {OP_CM_REG}, {(rb << 16) | 8:#x}')      # ... that must be zero (bits 8.. of cm_reg)
    a(f'v_and_b32 v{V_A}, {OP_CMT_LO}, {ITLO}')
    a(f'v_and_b32 v{V_B}, {OP_CMT_HI}, {ITHI}')
    a(f'v_cmp_eq_u32 vcc, s74, v{V_A}')
    a(f'v_cmp_eq_u32_e64 s[72:73], s75, v{V_B}')
    a('s_nop 1')
    a('s_and_b64 s[68:69], vcc, s[72:73]')
    a('s_waitcnt lgkmcnt(0)')                   # g[8] (and the header prefetch)
    # REAL fast paths: all four matrix entries real (x, ry, cx, ccx ...) and no REGISTER-bit
    # control.  Lane / outside-bit controls just narrow EXEC: the real paths update in place,
    # so disabled lanes keep their amplitudes (a gate pair always shares its predicate).
    a(f's_bitcmp1_b32 {OP_FLAGS}, {OPF_REAL}')
    a(f's_cbranch_scc0 {L("L_generic")}')
    a(f's_bitcmp1_b32 {OP_FLAGS}, {OPF_LANE_DPP}')   # on a real lane op: partner by DPP, no LDS
    a(f's_cbranch_scc1 {L("L_lrd")}')
    a('s_and_b64 exec, exec, s[68:69]')
    a(f's_cbranch_execz {L("L_next")}')
    a(f's_cmp_eq_u32 {OP_CM_REG}, 0')
    a(f's_cbranch_scc1 {L("L_real")}')
    # register-bit controls (ccx, ladders of multi_control): same in-place real arithmetic,
    # slots whose index misses a control bit are skipped one by one
    self.by_target(a, 'L_lane_real_c', 'L_rrc')
    self.next_op(a)
    a.label('L_generic')
    self.by_target(a, 'L_lane', 'L_reg')
    a.label('L_next')
    self.next_op(a)
    return a

  def by_target(self, a, lane, reg):
    """A dense op's code: `lane` for a lane bit (kind 1), `reg`<tb> for a register bit."""
    a(f's_cmp_eq_u32 {OP_KIND}, 1')
    a(f's_cbranch_scc1 {L(lane)}')
    for b in range(self.rb):
      a(f's_cmp_eq_u32 {OP_TB}, {b}')
      a(f's_cbranch_scc1 {L(f"{reg}{b}")}')

  # ---- dense 2x2 on register bit b: in-place butterflies ----------------------------
  def reg_dense(self):
    a, g, X, Y, MUL, FMA, MOV = Asm('reg_dense'), self.g, self.X, self.Y, self.MUL, self.FMA, self.MOV
    t0, t1, t2, t3 = (self.V2(t) for t in R_T)
    for b in range(self.rb):
      a.label(f'L_reg{b}')
      self.load_matrix_f32(a)
      for h, (k0, k1) in enumerate(pairs(b, self.nr)):
        skip = f'L_r{b}_{h}'
        ctl_skip(a, k0, skip)                   # control bits (register part) not set in k0
        ar, ai, br, bi = X(k0), Y(k0), X(k1), Y(k1)
        a(f'{MUL} {t0}, {g["g0r"]}, {ar}')
        a(f'{MUL} {t1}, {g["g0r"]}, {ai}')
        a(f'{MUL} {t2}, {g["g2r"]}, {ar}')
        a(f'{MUL} {t3}, {g["g2r"]}, {ai}')
        a(f'{FMA} {t0}, -{g["g0i"]}, {ai}, {t0}')
        a(f'{FMA} {t1}, {g["g0i"]}, {ar}, {t1}')
        a(f'{FMA} {t2}, -{g["g2i"]}, {ai}, {t2}')
        a(f'{FMA} {t3}, {g["g2i"]}, {ar}, {t3}')
        a(f'{FMA} {t0}, {g["g1r"]}, {br}, {t0}')
        a(f'{FMA} {t1}, {g["g1r"]}, {bi}, {t1}')
        a(f'{FMA} {t2}, {g["g3r"]}, {br}, {t2}')
        a(f'{FMA} {t3}, {g["g3r"]}, {bi}, {t3}')
        a(f'{FMA} {t0}, -{g["g1i"]}, {bi}, {t0}')
        a(f'{FMA} {t1}, {g["g1i"]}, {br}, {t1}')
        a(f'{FMA} {t2}, -{g["g3i"]}, {bi}, {t2}')
        a(f'{FMA} {t3}, {g["g3i"]}, {br}, {t3}')
        a('s_and_saveexec_b64 s[70:71], s[68:69]')
        a(f'{MOV} {ar}, {t0}')
        a(f'{MOV} {ai}, {t1}')
        a(f'{MOV} {br}, {t2}')
        a(f'{MOV} {bi}, {t3}')
        a('s_mov_b64 exec, s[70:71]')
        a.label(skip)
      self.next_op(a)
    return a

  def real_pairs(self, a, grp):
    """Real 2x2 on 1..2 slot pairs, interleaved (two temporaries each), results in place."""
    g, X, Y, MUL, FMA, MOV = self.g, self.X, self.Y, self.MUL, self.FMA, self.MOV
    tmps = [(self.V2(R_T[2 * j]), self.V2(R_T[2 * j + 1])) for j in range(len(grp))]
    for (k0, k1), (ta, tb) in zip(grp, tmps):
      a(f'{MUL} {ta}, {g["g0r"]}, {X(k0)}')
      a(f'{MUL} {tb}, {g["g0r"]}, {Y(k0)}')
    for (k0, k1), (ta, tb) in zip(grp, tmps):
      a(f'{FMA} {ta}, {g["g1r"]}, {X(k1)}, {ta}')
      a(f'{FMA} {tb}, {g["g1r"]}, {Y(k1)}, {tb}')
    for (k0, k1), (ta, tb) in zip(grp, tmps):
      a(f'{MUL} {X(k1)}, {g["g3r"]}, {X(k1)}')
      a(f'{MUL} {Y(k1)}, {g["g3r"]}, {Y(k1)}')
    for (k0, k1), (ta, tb) in zip(grp, tmps):
      a(f'{FMA} {X(k1)}, {g["g2r"]}, {X(k0)}, {X(k1)}')
      a(f'{FMA} {Y(k1)}, {g["g2r"]}, {Y(k0)}, {Y(k1)}')
    for (k0, k1), (ta, tb) in zip(grp, tmps):
      a(f'{MOV} {X(k0)}, {ta}')
      a(f'{MOV} {Y(k0)}, {tb}')

  # ---- REAL uncontrolled dense ops: half the arithmetic, results in place ---------------
  def real_dense(self):
    a = Asm('real_dense', cut=True)
    a.label('L_real')
    self.by_target(a, 'L_lane_real', 'L_rr')
    self.next_op(a)
    for b in range(self.rb):
      a.label(f'L_rr{b}')
      self.load_matrix_f32(a)
      ps = pairs(b, self.nr)
      for i in range(0, len(ps), 2):            # two pairs interleaved (4 temporaries)
        self.real_pairs(a, ps[i:i + 2])
      self.next_op(a)
    return a

  def real_controlled(self):
    a = Asm('real_controlled', cut=True)
    for b in range(self.rb):                    # real gate on register bit b under register controls
      a.label(f'L_rrc{b}')
      self.load_matrix_f32(a)
      for h, (k0, k1) in enumerate(pairs(b, self.nr)):
        skip = f'L_rrc{b}_{h}'
        ctl_skip(a, k0, skip)
        self.real_pairs(a, [(k0, k1)])
        a.label(skip)
      self.next_op(a)
    return a

  # lane bit, real: new = ca*mine + cb*other with real per-lane ca, cb -- 4 FP64 ops per slot
  def lane_real(self):
    a, X, Y, MUL, FMA = Asm('lane_real', cut=True), self.X, self.Y, self.MUL, self.FMA
    a.label('L_lane_real')
    a.label('L_lane_real_c')
    self.lane_partner(a, 's74')
    a(f's_bitcmp1_b32 {OP_FLAGS}, {OPF_USE_C}')      # needs complex coefficients: generic path
    a(f's_cbranch_scc1 {L("L_lane_c1")}')
    if self.wide:
      sel64(a, LN_COEF['car'], MAT0, MAT0 + 12)
      sel64(a, LN_COEF['cbr'], MAT0 + 4, MAT0 + 8)
    else:
      self.load_matrix_f32(a, 26)                  # g0r g0i g1r g1i g2r g2i g3r g3i -> v26..v33
      a(f'v_cndmask_b32 v{LN_COEF["car"]}, v26, v32, vcc')   # hi ? g3r : g0r
      a(f'v_cndmask_b32 v{LN_COEF["cbr"]}, v28, v30, vcc')   # hi ? g2r : g1r
    rca, rcb = self.V2(LN_COEF['car']), self.V2(LN_COEF['cbr'])

    def comb_real(k, pr, pi):
      a(f'{MUL} {X(k)}, {rca}, {X(k)}')
      a(f'{MUL} {Y(k)}, {rca}, {Y(k)}')
      a(f'{FMA} {X(k)}, {rcb}, {pr}, {X(k)}')
      a(f'{FMA} {Y(k)}, {rcb}, {pi}, {Y(k)}')

    def comb_real_c(k, pr, pi):                    # register-bit controls: combine only the selected slots
      skip = f'L_lrc_{k}'
      ctl_skip(a, k, skip)
      comb_real(k, pr, pi)
      a.label(skip)
    a(f's_cmp_eq_u32 {OP_CM_REG}, 0')
    a(f's_cbranch_scc0 {L("L_lane_real_cc")}')
    self.lane_pipeline(a, 24, 4, comb_real)
    self.next_op(a)
    a.label('L_lane_real_cc')
    self.lane_pipeline(a, 24, 4, comb_real_c)      # (all slots are shuffled: the pipeline's wait counts stay static)
    self.next_op(a)
    return a

  # ---- unit-entry butterflies on a register bit (BFLY above) -------------------------------------------------------
  def bfly_pairs(self, a, v, grp, scale=None):
    """complex128: butterfly `v` on the slot pairs `grp`, interleaved; scale = (c, 2c): b counts c times (fused rotations)."""
    R = lambda k, comp: self.Y(k) if comp else self.X(k)
    for k0, k1 in grp:
      for dst, src, sg in BFLY[v]['first']:
        if scale:
          a(f'v_fma_f64 {R(k0, dst)}, {sg}{scale[0]}, {R(k1, src)}, {R(k0, dst)}')
        else:
          a(f'v_add_f64 {R(k0, dst)}, {R(k0, dst)}, {sg}{R(k1, src)}')
    for k0, k1 in grp:
      for dst, s2, sa, src in BFLY[v]['second']:
        a(f'v_fma_f64 {R(k1, dst)}, {s2}{scale[1] if scale else "2.0"}, {R(k1, dst)}, {sa}{R(k0, src)}')

  def reg_butterflies(self):
    a, XY = Asm('reg_butterflies', cut=True), self.XY
    a.label('L_bf')                               # (section marker; handlers are reached through the table)
    for v in BFLY_VARIANTS:
      for b in range(self.rb):
        a.label(f'L_bf{v}_{b}')
        ps = pairs(b, self.nr)
        if self.wide:
          for i in range(0, len(ps), 4):          # four pairs interleaved: 8 independent chains
            self.bfly_pairs(a, v, ps[i:i + 4])
        else:
          a('v_mov_b32 v16, 2.0')
          a('v_mov_b32 v17, 2.0')
          for i in range(0, len(ps), 8):
            for k0, k1 in ps[i:i + 8]:
              a(f'v_pk_add_f32 {XY(k0)}, {XY(k0)}, {XY(k1)}{BFLY[v]["pk1"]}')
            for k0, k1 in ps[i:i + 8]:
              a(f'v_pk_fma_f32 {XY(k1)}, {XY(k1)}, v[16:17], {XY(k0)}{BFLY[v]["pk2"]}')
        self.next_op(a)
    return a

  # ---- register butterfly behind a phase on its own target (round 4) ---------------------------------------------
  # A layered circuit puts a T in front of most of its sqrt-gates: diag(1, e^{i pi/4}) on the butterfly's target, which the
  # planner emits right before that butterfly (phases are placed lazily).  As a DIAG op that was one op and one group
  # dispatch plus a complex product on the 2^(RB-1) slots of the bit (64 FP64 instructions at RB = 5).  Fused: b is the
  # slot with the bit set, e^{i pi/4} b = c (1 + i) b with c = 1/sqrt 2:  (1 +- i) b costs an addition and an fma in place,
  # and the real scale c rides on the butterfly's own additions as fma constants -- c in OP_CM_THREAD, 2c in OP_W23 (header
  # words cm_thread and cm_reg / n_groups of the device copy: kernels_sweep.hip.h) --: 32 + 64 instructions, one dispatch.
  # rotation 0: (1 + i) b; 1: (1 - i) b; the sign of c covers the other two odd multiples of pi/4.  complex128 only.
  def rot_butterflies(self):
    a, X, Y = Asm('rot_butterflies', front=True), self.X, self.Y
    if not self.wide:
      return a
    for r in ROTATIONS:
      for v in BFLY_VARIANTS:
        for b in range(self.rb):
          a.label(f'L_bfr{r}{v}_{b}')
          ps = pairs(b, self.nr)
          for i in range(0, len(ps), 4):
            grp = ps[i:i + 4]
            for k0, k1 in grp:                      # b = (1 +- i) b
              a(f'v_add_f64 {X(k1)}, {X(k1)}, {"-" if r == 0 else ""}{Y(k1)}')
            for k0, k1 in grp:
              a(f'v_fma_f64 {Y(k1)}, 2.0, {Y(k1)}, {"" if r == 0 else "-"}{X(k1)}')
            self.bfly_pairs(a, v, grp, scale=(OP_CM_THREAD, OP_W23))
          self.next_op(a)
    return a

  # ---- butterfly on a lane bit: partner p via ds_bpermute, own value o -------------------------------------------------
  def lane_butterflies(self):
    a, X, Y, FMA = Asm('lane_butterflies', cut=True), self.X, self.Y, self.FMA
    a.label('L_bfl_e')
    a(f's_bfe_u32 s74, {OP_FLAGS}, {OPF_BFLY_FIELD:#x}')      # butterfly variant
    a.label('L_bfl')
    a(f's_bitcmp1_b32 {OP_FLAGS}, {OPF_LANE_DPP}')            # partner values by DPP moves (VALU), not LDS
    a(f's_cbranch_scc1 {L("L_dpp")}')
    self.lane_partner(a, 's75')
    coef = self.V2(LN_COEF['car'])
    for v, lab in ((0, 'L_bfl_a'), (1, 'L_bfl_b'), (2, 'L_bfl_b'), (3, 'L_bfl_v'), (4, 'L_bfl_w')):
      a(f's_cmp_eq_u32 s74, {v}')
      a(f's_cbranch_scc1 {L(lab)}')
    self.next_op(a)

    def comb_a(k, pr, pi):       # new = alpha*o + p
      a(f'{FMA} {X(k)}, {coef}, {X(k)}, {pr}')
      a(f'{FMA} {Y(k)}, {coef}, {Y(k)}, {pi}')

    def comb_b(k, pr, pi):       # new = o + beta*p
      a(f'{FMA} {X(k)}, {coef}, {pr}, {X(k)}')
      a(f'{FMA} {Y(k)}, {coef}, {pi}, {Y(k)}')

    def comb_first(v):           # new = o -+ i p: the first step of variant v with the partner as b
      def comb(k, pr, pi):
        own = (X(k), Y(k))
        for dst, src, sg in BFLY[v]['first']:
          a(self.ADDS(own[dst], own[dst], (pr, pi)[src], neg=sg == '-'))
      return comb

    c0 = LN_COEF['car']
    a.label('L_bfl_a')                               # h: alpha = +1 on the 0-lane, -1 on the 1-lane
    if self.wide:
      a(f'v_mov_b32 v{c0}, 0')
      a(f'v_mov_b32 v{c0 + 1}, 0x3ff00000')
      a(f'v_mov_b32 v{LN_TMP}, 0xbff00000')
      a(f'v_cndmask_b32 v{c0 + 1}, v{c0 + 1}, v{LN_TMP}, vcc')
    else:
      a(f'v_mov_b32 v{LN_TMP}, -1.0')
      a(f'v_cndmask_b32 v{c0}, 1.0, v{LN_TMP}, vcc')
    self.lane_pipeline(a, 20, 4, comb_a)
    self.next_op(a)
    a.label('L_bfl_b')                               # yroot / yroot^+: beta = g[0] on the 0-lane, g[1] on the 1-lane
    a(f's_load_dwordx4 s[{MAT0}:{MAT0 + 3}], {OPS}, 0x20')
    a('s_waitcnt lgkmcnt(0)')
    if self.wide:
      sel64(a, c0, MAT0, MAT0 + 2)
    else:
      a(f'v_cvt_f32_f64 v{c0}, {G(0)}')
      a(f'v_cvt_f32_f64 v{LN_TMP}, {G(1)}')
      a(f'v_cndmask_b32 v{c0}, v{c0}, v{LN_TMP}, vcc')
    self.lane_pipeline(a, 20, 4, comb_b)
    self.next_op(a)
    for lab, v in (('L_bfl_v', 3), ('L_bfl_w', 4)):
      a.label(lab)
      self.lane_pipeline(a, 20, 4, comb_first(v))
      self.next_op(a)
    return a

  # ---- OP_LSWAP: lane bit tb (4 or 5) <-> register bit r (header field cm_reg), in place --
  # v_permlane{16,32}_swap exchanges the odd rows / upper half of one register with the even
  # rows / lower half of another: applied to slots (k, k^1) it moves the pair a lane-bit gate
  # acts on into ONE lane (registers k and k^1), i.e. afterwards that index bit is register
  # bit r and the old register bit r is the lane bit.  The planner emits the gate as a
  # register op in between and swaps back (the op is an involution).  No LDS traffic:
  # ds_bpermute issues once per ~6 cycles per CU, these run at VALU rate.
  def lswap(self):
    a, T = Asm('lswap', cut=True), self.T
    a.label('L_lswap')                            # (section marker)
    for r in range(self.rb):
      for name, ins in ((f'L_lswap16_r{r}', 'v_permlane16_swap_b32'), (f'L_lswap32_r{r}', 'v_permlane32_swap_b32')):
        a.label(name)
        for k0, k1 in pairs(r, self.nr):
          for d in range(2 * self.W):
            a(f'{ins} v{T(k0) + d}, v{T(k1) + d}')
        # the thread's own bit moves with the exchange: header n_groups = the lane bit's index position,
        # cm_thread = that bit | the register bit's position (which holds 0 in a thread index)
        a(f's_lshl_b64 s[72:73], 1, {OP_NGROUPS}')
        a(f'v_and_b32 v{V_A}, s72, {ITLO}')
        a(f'v_and_b32 v{V_B}, s73, {ITHI}')
        a(f'v_or_b32 v{V_A}, v{V_A}, v{V_B}')
        a(f'v_cmp_ne_u32 vcc, 0, v{V_A}')
        a(f'v_xor_b32 v{V_A}, {OP_CMT_LO}, {ITLO}')
        a(f'v_xor_b32 v{V_B}, {OP_CMT_HI}, {ITHI}')
        a(f'v_cndmask_b32 {ITLO}, {ITLO}, v{V_A}, vcc')
        a(f'v_cndmask_b32 {ITHI}, {ITHI}, v{V_B}, vcc')
        self.next_op(a)
    return a

  # ---- OP_WSWAP: wave bit tb <-> register bit r (header field cm_reg) --------------------
  # The 2^W waves of a workgroup hold the tiles of ONE super-tile: they differ in W chosen
  # index bits ("wave bits").  A dense gate on such a bit pairs amplitudes of two waves; the
  # exchange below transposes that bit with register bit r: the wave whose bit is 0 hands its
  # slots with bit r set to the partner wave and receives the partner's other slots into them (and vice
  # versa), through a 2^W x (half x 16 lines) LDS buffer, `half` slots per pass, two barriers
  # per pass.  Afterwards the gate is a register op; the planner swaps back before the store.
  # The wave's own index bits change with the layout: header field cm_thread holds
  # (1 << old wave-bit position) | (1 << position of register bit r); it is XORed into the
  # tile index and the thread index when this wave's bit is 1.
  def wswap(self):
    a, nr, rb, XY = Asm('wswap', cut=True), self.nr, self.rb, self.XY
    a.label('L_wswap')
    half = min(8, nr // 2)
    slot_bytes = 64 * 2 * self.W * 4              # bytes one slot of one wave takes (64 lanes x complex)
    region = half * slot_bytes
    a(f's_lshr_b32 s74, {WAVE}, {OP_TB}')
    a('s_and_b32 s74, s74, 1')                    # x = this wave's bit
    a(f's_lshl_b32 s75, 1, {OP_TB}')
    a(f's_xor_b32 s75, {WAVE}, s75')              # partner wave
    a(f's_mul_i32 s72, {WAVE}, {region}')
    a(f's_add_u32 s72, s72, {LDS}')
    a(f's_mul_i32 s73, s75, {region}')
    a(f's_add_u32 s73, s73, {LDS}')
    a(f'v_lshlrev_b32 v16, {2 + self.W}, {LANE}')   # lane * bytes per amplitude
    a('v_add_u32 v17, s72, v16')                  # where this wave writes
    a('v_add_u32 v18, s73, v16')                  # where the partner wrote
    wr = 'ds_write_b128' if self.wide else 'ds_write_b64'
    rd = 'ds_read_b128' if self.wide else 'ds_read_b64'
    for r in range(rb):
      a(f's_cmp_eq_u32 {OP_CM_REG}, {r}')
      a(f's_cbranch_scc1 {L(f"L_wswap_r{r}")}')
    self.next_op(a)
    for r in range(rb):
      a.label(f'L_wswap_r{r}')
      a('s_cmp_eq_u32 s74, 0')
      a(f's_cbranch_scc0 {L(f"L_wswap_even_r{r}")}')
      for name, parity in ((f'L_wswap_odd_r{r}', 1), (f'L_wswap_even_r{r}', 0)):
        a.label(name)
        slots = [k for k in range(nr) if ((k >> r) & 1) == parity]
        for p0 in range(0, len(slots), half):
          part = slots[p0:p0 + half]
          for j, k in enumerate(part):
            a(f'{wr} v17, {XY(k)} offset:{j * slot_bytes}')
          a('s_waitcnt lgkmcnt(0)')
          a('s_barrier')
          for j, k in enumerate(part):
            a(f'{rd} {XY(k)}, v18 offset:{j * slot_bytes}')
          a('s_waitcnt lgkmcnt(0)')
          a('s_barrier')
        if parity == 0:            # (bit 0: index bits unchanged, both positions hold 0)
          a(f's_xor_b64 {TIDX}, {TIDX}, {OP_CM_THREAD}')
          a(f'v_xor_b32 {ITLO}, {OP_CMT_LO}, {ITLO}')
          a(f'v_xor_b32 {ITHI}, {OP_CMT_HI}, {ITHI}')
        self.next_op(a)
    return a

  # ---- butterfly on lane bit 0..3 with DPP partner fetch (OPF_LANE_DPP) -------------------
  # new.re = o.re + beta_re * q.re ; new.im = o.im + beta_im * q.im, q = partner value, or the
  # partner with re/im exchanged (flags bit 8; v / v^+).  beta = +-1 per lane: g[0..3] =
  # beta_re(0-lane), beta_re(1-lane), beta_im(0-lane), beta_im(1-lane).
  def dpp_butterfly(self):
    a, W, T, X, Y, XY, V2 = Asm('dpp_butterfly', cut=True), self.W, self.T, self.X, self.Y, self.XY, self.V2
    a.label('L_dpp')
    a(f's_load_dwordx8 s[{MAT0}:{MAT0 + 7}], {OPS}, 0x20')      # beta_re, beta_im per lane half
    a(f's_lshl_b32 s75, 1, {OP_TB}')
    a(f'v_and_b32 v{LN_TMP}, s75, {LANE}')
    a(f'v_cmp_ne_u32 vcc, 0, v{LN_TMP}')
    BRE, BIM, Q, TQ = 18, (22 if self.wide else 19), 24, 28     # complex64: (beta_re, beta_im) adjacent for the packed fma
    a('s_waitcnt lgkmcnt(0)')
    for v, lo in ((BRE, MAT0), (BIM, MAT0 + 4)):
      if self.wide:
        sel64(a, v, lo, lo + 2)
      else:
        a(f'v_cvt_f32_f64 v{v}, s[{lo}:{lo + 1}]')
        a(f'v_cvt_f32_f64 v{LN_TMP}, s[{lo + 2}:{lo + 3}]')
        a(f'v_cndmask_b32 v{v}, v{v}, v{LN_TMP}, vcc')
    a(f's_bfe_u32 s75, {OP_FLAGS}, {OPF_SWAP_RI_FIELD:#x}')     # 1: partner's re/im exchanged
    a('s_lshl_b32 s75, s75, 2')
    a(f's_add_u32 s75, s75, {OP_TB}')             # 4*exchanged + tb
    for code in range(8):
      a(f's_cmp_eq_u32 s75, {code}')
      a(f's_cbranch_scc1 {L(f"L_dpp{code}")}')
    self.next_op(a)
    for code in range(8):
      tbv, exch = code & 3, code >> 2
      a.label(f'L_dpp{code}')
      a('s_nop 1')
      for k in range(self.nr):
        # source dwords: q.re from the partner's re (or im when exchanged), q.im likewise
        src = [T(k) + d for d in range(2 * W)]
        if exch:
          src = src[W:] + src[:W]
        dpp_fetch(a, Q, TQ, src, DPP1[tbv])
        if self.wide:
          a(f'{self.FMA} {X(k)}, {V2(BRE)}, {V2(Q)}, {X(k)}')
          a(f'{self.FMA} {Y(k)}, {V2(BIM)}, {V2(Q + W)}, {Y(k)}')
        else:
          a(f'v_pk_fma_f32 {XY(k)}, v[{BRE}:{BRE + 1}], v[{Q}:{Q + 1}], {XY(k)}')
      self.next_op(a)
    return a

  # ---- real 2x2 on lane bit 0..3, partner by DPP moves (OPF_LANE_DPP on a REAL lane op) ------
  # new = ca*own + cb*partner; the control predicate is folded into the coefficients
  # (ca = 1, cb = 0 where it fails), so EXEC stays full and the two-step DPP moves may pass
  # through lanes the gate does not act on.
  def dpp_real(self):
    a, W, T, X, Y, V2, MUL, FMA = Asm('dpp_real', cut=True), self.W, self.T, self.X, self.Y, self.V2, self.MUL, self.FMA
    a.label('L_lrd')
    a(f's_lshl_b32 s74, 1, {OP_TB}')
    a(f'v_and_b32 v{LN_TMP}, s74, {LANE}')
    a(f'v_cmp_ne_u32 vcc, 0, v{LN_TMP}')
    CA, CB, Q, TQ = 18, 18 + 2 * W, 24, 28
    if self.wide:
      sel64(a, CA, MAT0, MAT0 + 12)
      sel64(a, CB, MAT0 + 4, MAT0 + 8)
      # predicate fails: ca = 1.0, cb = 0.0
      a(f'v_mov_b32 v{LN_TMP}, 0x3ff00000')
      a(f'v_cndmask_b32 v{CA}, 0, v{CA}, s[68:69]')
      a(f'v_cndmask_b32 v{CA + 1}, v{LN_TMP}, v{CA + 1}, s[68:69]')
      a(f'v_cndmask_b32 v{CB}, 0, v{CB}, s[68:69]')
      a(f'v_cndmask_b32 v{CB + 1}, 0, v{CB + 1}, s[68:69]')
    else:
      a(f'v_cvt_f32_f64 v{CA}, {G(0)}')
      a(f'v_cvt_f32_f64 v{LN_TMP}, {G(6)}')
      a(f'v_cndmask_b32 v{CA}, v{CA}, v{LN_TMP}, vcc')
      a(f'v_cvt_f32_f64 v{CB}, {G(2)}')
      a(f'v_cvt_f32_f64 v{LN_TMP}, {G(4)}')
      a(f'v_cndmask_b32 v{CB}, v{CB}, v{LN_TMP}, vcc')
      a(f'v_cndmask_b32 v{CA}, 1.0, v{CA}, s[68:69]')
      a(f'v_cndmask_b32 v{CB}, 0, v{CB}, s[68:69]')
    for tbv in range(4):
      a(f's_cmp_eq_u32 {OP_TB}, {tbv}')
      a(f's_cbranch_scc1 {L(f"L_lrd{tbv}")}')
    self.next_op(a)
    for tbv in range(4):
      a.label(f'L_lrd{tbv}')
      a('s_nop 1')
      for k in range(self.nr):
        skip = f'L_lrd{tbv}_{k}'
        ctl_skip(a, k, skip)                        # register-bit controls: skip the slots they exclude
        dpp_fetch(a, Q, TQ, [T(k) + d for d in range(2 * W)], DPP1[tbv])
        a(f'{MUL} {X(k)}, {V2(CA)}, {X(k)}')
        a(f'{MUL} {Y(k)}, {V2(CA)}, {Y(k)}')
        a(f'{FMA} {X(k)}, {V2(CB)}, {V2(Q)}, {X(k)}')
        a(f'{FMA} {Y(k)}, {V2(CB)}, {V2(Q + W)}, {Y(k)}')
        a.label(skip)
      self.next_op(a)
    return a

  # ---- dense 2x2 on a lane bit: partner via ds_bpermute -------------------------------
  def lane_dense(self):
    a, W, nr, X, Y, V2, MUL, FMA, MOV = Asm('lane_dense', cut=True), self.W, self.nr, self.X, self.Y, self.V2, self.MUL, self.FMA, self.MOV
    a.label('L_lane')
    self.lane_partner(a, 's74')
    a.label('L_lane_c1')
    # deferred factor c of the preceding DIAG op lives in v[18:21] = the coefficient
    # registers: move it to v[34:37] and fetch the partner lane's c into v[26:29] first
    a(f's_bitcmp1_b32 {OP_FLAGS}, {OPF_USE_C}')
    a(f's_cbranch_scc0 {L("L_lane_c0")}')
    cc = 34 if self.wide else 38                      # f64: v[34:35], v[36:37]; f32: v38, v39
    a(f'{MOV} {V2(cc)}, {self.cr}')
    a(f'{MOV} {V2(cc + W)}, {self.ci}')
    for d in range(2 * W):
      a(f'ds_bpermute_b32 v{LN_BUF[0] + d}, v{LN_ADDR}, v{cc + d}')
    a.label('L_lane_c0')
    # new = ca*mine + cb*other ; ca = hi ? g3 : g0 ; cb = hi ? g2 : g1
    src = {'car': (52, 64), 'cai': (54, 66), 'cbr': (56, 60), 'cbi': (58, 62)}
    if self.wide:
      for name, v in LN_COEF.items():
        sel64(a, v, *src[name])
    else:
      # the partner's c (USE_C) may be arriving in v26,v27: convert the matrix into the
      # cmul temporaries' neighbourhood instead (v30..v37), then select per lane
      self.load_matrix_f32(a, 30)
      a(f'v_cndmask_b32 v{LN_COEF["car"]}, v30, v36, vcc')   # hi ? g3r : g0r
      a(f'v_cndmask_b32 v{LN_COEF["cai"]}, v31, v37, vcc')   # hi ? g3i : g0i
      a(f'v_cndmask_b32 v{LN_COEF["cbr"]}, v32, v34, vcc')   # hi ? g2r : g1r
      a(f'v_cndmask_b32 v{LN_COEF["cbi"]}, v33, v35, vcc')   # hi ? g2i : g1i
    car, cai, cbr, cbi = (V2(LN_COEF[n]) for n in ('car', 'cai', 'cbr', 'cbi'))
    # USE_C (flags bit 1): the preceding DIAG op left its per-lane factor c un-applied;
    # H.diag(c) acts as  new = (ca c_mine) mine + (cb c_other) other  -- two complex
    # products per LANE instead of one per amplitude.
    a(f's_bitcmp1_b32 {OP_FLAGS}, {OPF_USE_C}')
    a(f's_cbranch_scc0 {L("L_lane_nc")}')
    a('s_waitcnt lgkmcnt(0)')
    self.cmul_vv(a, car, cai, V2(cc), V2(cc + W), V2(LN_BUF[1]))
    self.cmul_vv(a, cbr, cbi, V2(LN_BUF[0]), V2(LN_BUF[0] + W), V2(LN_BUF[1]))
    a.label('L_lane_nc')

    def combine(k, buf):
      orr, oi = V2(buf), V2(buf + W)
      u0, u1 = V2(LN_T[0]), V2(LN_T[1])
      a(f'{MUL} {u0}, {car}, {X(k)}')
      a(f'{MUL} {u1}, {car}, {Y(k)}')
      a(f'{FMA} {u0}, -{cai}, {Y(k)}, {u0}')
      a(f'{FMA} {u1}, {cai}, {X(k)}, {u1}')
      a(f'{FMA} {u0}, {cbr}, {orr}, {u0}')
      a(f'{FMA} {u1}, {cbr}, {oi}, {u1}')
      a(f'{FMA} {u0}, -{cbi}, {oi}, {u0}')
      a(f'{FMA} {u1}, {cbi}, {orr}, {u1}')
      a('s_and_saveexec_b64 s[70:71], s[68:69]')
      a(f'{MOV} {X(k)}, {u0}')
      a(f'{MOV} {Y(k)}, {u1}')
      a('s_mov_b64 exec, s[70:71]')

    a(f's_cmp_eq_u32 {OP_CM_REG}, 0')
    a(f's_cbranch_scc0 {L("L_lane_ctl")}')
    # fast path (no register-bit controls): shuffles of slot k+1 in flight while slot k combines
    self.shuf(a, 0, LN_BUF[0])
    for k in range(nr):
      if k + 1 < nr:
        self.shuf(a, k + 1, LN_BUF[(k + 1) & 1])
        a(f's_waitcnt lgkmcnt({2 * W})')
      else:
        a('s_waitcnt lgkmcnt(0)')
      combine(k, LN_BUF[k & 1])
    self.next_op(a)
    a.label('L_lane_ctl')
    for k in range(nr):
      skip = f'L_l_{k}'
      ctl_skip(a, k, skip)
      self.shuf(a, k, LN_BUF[0])
      a('s_waitcnt lgkmcnt(0)')
      combine(k, LN_BUF[0])
      a.label(skip)
    self.next_op(a)
    return a

  # ---- diagonal op: groups of phase factors -------------------------------------------
  # SGPRs here: OP_CM_THREAD tables base, G_HDR group header, s[76:91] chunk-table entries / oterm scratch, GRP group
  # cursor, s96 counter, s75 = "c was modified", and of the group being applied (its header registers are already being
  # refilled with the NEXT group's header during the apply phase): s72 reg_mask, s73 tab_off[3], s97 lane_mask,
  # s[84:87] phi0.
  # Control flow (a taken branch costs a wave ~50 cycles, see the op dispatch above): the host marks a
  # group GENERAL (flags bit 2) when it has a lane table, chunk tables or outside terms; every other
  # group -- f = phi0 on the lanes that satisfy lane_mask -- runs straight through.  The apply code is
  # reached through the handler table (entries NHID.., number in flags bits 8..15: group_handlers()), and every apply
  # handler ends with its own copy of the group head: two jumps per group instead of eight.
  def cmul_su(self, a, sre, sim):
    """u *= the double-precision factor held in two SGPR pairs."""
    if self.wide:
      self.cmul_vv(a, self.ur, self.ui, sre, sim, self.dt)
    else:
      a(f'v_cvt_f32_f64 v38, {sre}')          # v34..v37 may be receiving a lane-table entry
      a(f'v_cvt_f32_f64 v39, {sim}')
      self.cmul_vv(a, self.ur, self.ui, 'v38', 'v39', self.dt)

  def lane_ok(self, a, lane_mask):
    """vcc = this lane satisfies lane_mask."""
    a(f'v_and_b32 v{V_A}, {lane_mask}, {LANE}')
    a(f'v_cmp_eq_u32 vcc, {lane_mask}, v{V_A}')

  def f_from_u(self, a):
    """f = vcc ? u : 1"""
    D_U, D_F = self.D_U, self.D_F
    if self.wide:
      a(f'v_mov_b32 v{V_B}, 0x3ff00000')
      a(f'v_cndmask_b32 v{D_F[0]}, 0, v{D_U[0]}, vcc')
      a(f'v_cndmask_b32 v{D_F[0] + 1}, v{V_B}, v{D_U[0] + 1}, vcc')
      a(f'v_cndmask_b32 v{D_F[1]}, 0, v{D_U[1]}, vcc')
      a(f'v_cndmask_b32 v{D_F[1] + 1}, 0, v{D_U[1] + 1}, vcc')
    else:
      a(f'v_cndmask_b32 v{D_F[0]}, 1.0, v{D_U[0]}, vcc')
      a(f'v_cndmask_b32 v{D_F[1]}, 0, v{D_U[1]}, vcc')

  def u_from_sgprs(self, a, dwords):
    """u = the double-precision complex number in four SGPRs (a wave-uniform value held in VGPRs)."""
    D_U = self.D_U
    if self.wide:
      for v, s in zip((D_U[0], D_U[0] + 1, D_U[1], D_U[1] + 1), dwords):
        a(f'v_mov_b32 v{v}, {s}')
    else:
      a(f'v_cvt_f32_f64 v{D_U[0]}, s[{dwords[0][1:]}:{dwords[1][1:]}]')
      a(f'v_cvt_f32_f64 v{D_U[1]}, s[{dwords[2][1:]}:{dwords[3][1:]}]')

  def grp_dispatch(self, a):
    # the header is consumed: remember reg_mask, advance, prefetch the NEXT group's header into the same
    # SGPRs (one past the last group is readable memory: oterms / tables follow) and jump to the apply code
    a(f's_mov_b32 s72, {G_REG_MASK}')
    a(f's_mov_b32 s73, {G_TAB_OFF[3]}')          # the bit factors of a DG_BITFAC group
    a(f's_mov_b32 s97, {G_LANE_MASK}')           # the sign-flip handlers of factor -1 build their own lane predicate
    a(f's_bfe_u32 s74, {G_FLAGS}, {DG_HANDLER_FIELD:#x}')
    self.grp_advance(a)
    a('s_lshl_b32 s74, s74, 2')
    a(f's_add_u32 s74, s74, {4 * NHID}')
    a(f's_add_u32 s98, {TAB_LO}, s74')
    a(f's_addc_u32 s99, {TAB_HI}, 0')
    a('s_setpc_b64 s[98:99]')

  def grp_advance(self, a):
    a(f's_add_u32 {GRP_LO}, {GRP_LO}, 64')
    a(f's_addc_u32 {GRP_HI}, {GRP_HI}, 0')
    a('s_add_u32 s96, s96, 1')
    a(f's_load_dwordx16 {G_HDR}, {GRP}, 0x0')

  def grp_body(self, a):
    # Classes (the host numbers the apply handler accordingly: kernels_sweep.hip.h group_handler_bits).  GENERAL groups
    # (lane table, chunk tables, outside terms, bit factors) assemble f in VGPRs first (L_grp_gen) and apply it with the
    # L_gm* handlers.  Every other group is dispatched at once with phi0 in s[84:87] and lane_mask in s97:
    #   L_gn*  factor -1: sign flips, no factor registers at all
    #   L_gu*  lane_mask == 0 (T, S, Rz on a register bit, global scalars: most groups of a layered circuit): the
    #          products take phi0 straight from the SGPRs -- no per-group VALU prologue (11 instructions until round 4)
    #   L_gl*  lane-masked factor: f = lane_ok ? phi0 : 1 built in the handler, then the L_gm* body
    a('s_waitcnt lgkmcnt(0)')
    a(f's_bitcmp1_b32 {G_FLAGS}, {DG_SIGN_OTERMS}')   # sign group under outside-bit conditions: see L_grp_sot
    a(f's_cbranch_scc1 {L("L_grp_sot")}')
    a(f's_bitcmp1_b32 {G_FLAGS}, {DG_GENERAL}')
    a(f's_cbranch_scc1 {L("L_grp_gen")}')
    a(f's_mov_b64 s[84:85], {G_PHI0_RE}')          # phi0 (the header registers are refilled by the dispatch)
    a(f's_mov_b64 s[86:87], {G_PHI0_IM}')
    self.grp_dispatch(a)

  def grp_tail(self, a):
    a('s_mov_b64 exec, -1')                        # (lane-masked factors are applied under an EXEC mask, see L_gl*)
    a(f's_cmp_lt_u32 s96, {OP_NGROUPS}')
    a(f's_cbranch_scc0 {L("L_diag_end")}')
    self.grp_body(a)

  def c_init(self, a):
    D_C = self.D_C
    if self.wide:
      a(f'v_mov_b32 v{D_C[0]}, 0')
      a(f'v_mov_b32 v{D_C[0] + 1}, 0x3ff00000')   # c = 1.0 + 0.0i
      a(f'v_mov_b32 v{D_C[1]}, 0')
      a(f'v_mov_b32 v{D_C[1] + 1}, 0')
    else:
      a(f'v_mov_b32 v{D_C[0]}, 1.0')
      a(f'v_mov_b32 v{D_C[1]}, 0')

  def c_ensure(self, a):
    """c = 1 before the first factor joins it (most DIAG ops of a layered circuit have no factor for c at all: the
    unconditional initialisation cost them four moves each)."""
    skip = self.uniq('L_ci')
    a('s_cmp_lg_u32 s75, 0')
    a(f's_cbranch_scc1 {L(skip)}')
    self.c_init(a)
    a.label(skip)

  def on_mask(self, a, m, body, per=1, skip=None):
    """body(slots) on the slots whose index holds every bit of the register mask m, `per` at a time; m == 'x': the mask is in
    s72 and every slot is tested (skip(k): the label that jumps over slot k)."""
    if m == 'x':
      for k in range(self.nr):
        lab = skip(k)
        mask_skip(a, k, lab)
        body([k])
        a.label(lab)
    else:
      slots = self.slots_of(m)
      for i in range(0, len(slots), per):
        body(slots[i:i + per])

  def cmul_mask(self, a, m, fr, fi, skip=None):
    self.on_mask(a, m, lambda ks: self.cmul_slots(a, ks, fr, fi), per=4, skip=skip)

  # Factor -1 (cz and friends: a third of the groups of a supremacy sweep): the host picks these handlers for a
  # group without tables whose factor is exactly -1; a sign flip is ONE 32-bit xor per real number instead of
  # the four FP64 instructions of a complex product.  v16 = sign bit on the lanes that satisfy lane_mask.
  def neg_mask_vgpr(self, a):
    self.lane_ok(a, 's97')
    a(f'v_mov_b32 v{V_B}, 0x80000000')
    a(f'v_cndmask_b32 v{V_A}, 0, v{V_B}, vcc')

  def neg_slot(self, a, k):
    hi, T, W = self.W - 1, self.T, self.W        # hi: the dword that holds the sign of a real number
    a(f'v_xor_b32 v{T(k) + hi}, v{V_A}, v{T(k) + hi}')
    a(f'v_xor_b32 v{T(k) + W + hi}, v{V_A}, v{T(k) + W + hi}')

  def neg_mask(self, a, m, skip=None):
    self.on_mask(a, m, lambda ks: self.neg_slot(a, ks[0]), skip=skip)

  def exec_from_lane_mask(self, a):
    self.lane_ok(a, 's97')
    a('s_nop 1')
    a('s_and_b64 exec, exec, vcc')

  def diag_groups(self):
    """The group loop of a DIAG op and the apply handlers of its four classes (the pieces follow; one section because they
    run on into one another only by jumps, and nothing may be laid out between them and the op's entry)."""
    a = Asm('diag_groups', cut=True)
    self.diag_entry(a)
    self.grp_sign_oterms(a)
    self.grp_general(a)
    self.apply_vector(a)
    self.apply_sign(a)
    self.apply_uniform(a)
    self.apply_lane_masked(a)
    return a

  def diag_entry(self, a):
    a.label('L_diag')
    a(f's_bitcmp1_b32 {OP_FLAGS}, {OPF_DEFER_C}')   # (rare): the next op reads c whatever happened to it -> L_diag_ci, out of line
    a(f's_cbranch_scc1 {L("L_diag_ci")}')
    a.label('L_diag_nc')
    a('s_mov_b32 s75, 0')                        # c modified?
    a(f's_cmp_eq_u32 {OP_NGROUPS}, 0')
    a(f's_cbranch_scc1 {L("L_next")}')
    a(f's_add_u32 {OP_CMT_LO}, {GROUPS_LO}, {TABLES_REL}')   # tables base = groups base + rel
    a(f's_addc_u32 {OP_CMT_HI}, {GROUPS_HI}, 0')
    a(f's_lshl_b32 s74, {OP_GROUP_OFF}, 6')      # group_off * sizeof(DGroup)=64
    a(f's_add_u32 {GRP_LO}, {GROUPS_LO}, s74')
    a(f's_addc_u32 {GRP_HI}, {GROUPS_HI}, 0')
    a('s_mov_b32 s96, 0')
    a(f's_load_dwordx16 {G_HDR}, {GRP}, 0x0')
    self.grp_body(a)

  def oterm_cursor(self, a):
    a(f's_mul_i32 s74, {G_OTERM_OFF}, 24')       # oterm_off * sizeof(OTerm)
    a(f's_add_u32 s94, {OTERMS_LO}, s74')
    a(f's_addc_u32 s95, {OTERMS_HI}, 0')

  # A factor -1 whose condition includes bits OUTSIDE the tile (a cz between a register / lane bit and a far bit):
  # phi0 = 1 and every outside term is -1 on its mask.  The outside bits are wave-uniform, so the parity of the terms
  # that apply is a scalar: even -> the group does nothing for this tile (skipped: no vector instruction at all), odd ->
  # the sign-flip handler of its register mask.  (Until round 4: u = +-1 built in VGPRs, then a complex product per slot.)
  def grp_sign_oterms(self, a):
    a.label('L_grp_sot')
    self.oterm_cursor(a)
    a('s_mov_b32 s98, 0')                        # parity
    a('s_mov_b32 s99, 0')                        # counter
    a.label('L_sot')
    a('s_load_dwordx2 s[84:85], s[94:95], 0x0')
    a('s_waitcnt lgkmcnt(0)')
    a(f's_and_b64 s[72:73], {TIDX}, s[84:85]')
    a('s_cmp_eq_u64 s[72:73], s[84:85]')
    a('s_cselect_b32 s74, 1, 0')
    a('s_xor_b32 s98, s98, s74')
    a('s_add_u32 s94, s94, 24')
    a('s_addc_u32 s95, s95, 0')
    a('s_add_u32 s99, s99, 1')
    a(f's_cmp_lt_u32 s99, {G_N_OTERMS}')
    a(f's_cbranch_scc1 {L("L_sot")}')
    a('s_cmp_eq_u32 s98, 0')
    a(f's_cbranch_scc0 {L("L_sot_odd")}')
    self.grp_advance(a)                          # even: next group (as grp_dispatch, without an apply handler)
    self.grp_tail(a)
    a.label('L_sot_odd')
    self.grp_dispatch(a)                         # (the host numbered the handler L_gn<mask>)

  def grp_general(self, a):
    """General group: lane table, chunk tables, outside terms."""
    MUL, FMA, V2, fr, fi, ur, ui = self.MUL, self.FMA, self.V2, self.fr, self.fi, self.ur, self.ui
    a.label('L_grp_gen')
    self.u_from_sgprs(a, G_PHI0_DW)
    a(f's_bitcmp1_b32 {G_FLAGS}, {DG_LTAB}')     # start the 1-KiB lane-table load early
    a(f's_cbranch_scc0 {L("L_g1")}')
    a(f's_lshl_b32 s74, {G_LTAB_OFF}, 4')
    a(f'v_lshlrev_b32 v{V_A}, 4, {LANE}')        # 16-byte table entries, indexed by the LANE id
    a(f's_bitcmp1_b32 {G_FLAGS}, {DG_LTAB_LDS}')   # the kernel copied the lane tables to LDS
    a(f's_cbranch_scc0 {L("L_g0g")}')
    a(f's_add_u32 s74, s74, {LTAB}')
    a(f'v_add_u32 v{V_A}, s74, v{V_A}')
    a(f'ds_read_b128 v[{D_LTAB}:{D_LTAB + 3}], v{V_A}')
    a(f's_branch {L("L_g1")}')
    a.label('L_g0g')
    a(f's_add_u32 s98, {OP_CMT_LO}, s74')
    a(f's_addc_u32 s99, {OP_CMT_HI}, 0')
    a(f'global_load_dwordx4 v[{D_LTAB}:{D_LTAB + 3}], v{V_A}, s[98:99]')
    a.label('L_g1')
    a(f's_cmp_eq_u32 {G_NTAB}, 0')
    a(f's_cbranch_scc1 {L("L_g2")}')
    for t in range(4):                           # issue all chunk-table lookups, then one wait
      if t:
        a(f's_cmp_le_u32 {G_NTAB}, {t}')
        a(f's_cbranch_scc1 {L("L_g1w")}')
      a(f's_bfe_u32 s74, {G_TAB_SHIFT}, {(8 << 16) | (8 * t)}')
      a(f's_lshr_b64 s[72:73], {TIDX}, s74')
      a('s_and_b32 s72, s72, 0xff')
      a(f's_add_u32 s72, s72, {G_TAB_OFF[t]}')
      a('s_lshl_b32 s72, s72, 4')
      a(f's_load_dwordx4 s[{76 + 4 * t}:{79 + 4 * t}], {OP_CM_THREAD}, s72')
    a.label('L_g1w')
    a('s_waitcnt lgkmcnt(0)')
    for t in range(4):
      if t:
        a(f's_cmp_le_u32 {G_NTAB}, {t}')
        a(f's_cbranch_scc1 {L("L_g2")}')
      self.cmul_su(a, f's[{76 + 4 * t}:{77 + 4 * t}]', f's[{78 + 4 * t}:{79 + 4 * t}]')
    a.label('L_g2')
    a(f's_cmp_eq_u32 {G_N_OTERMS}, 0')
    a(f's_cbranch_scc1 {L("L_grp_f")}')
    self.oterm_cursor(a)
    a('s_mov_b32 s97, 0')
    a.label('L_ot')
    a('s_load_dwordx2 s[84:85], s[94:95], 0x0')
    a('s_load_dwordx4 s[88:91], s[94:95], 0x8')
    a('s_waitcnt lgkmcnt(0)')
    a(f's_and_b64 s[72:73], {TIDX}, s[84:85]')
    a('s_cmp_eq_u64 s[72:73], s[84:85]')
    a(f's_cbranch_scc0 {L("L_ot_n")}')
    self.cmul_su(a, 's[88:89]', 's[90:91]')
    a.label('L_ot_n')
    a('s_add_u32 s94, s94, 24')
    a('s_addc_u32 s95, s95, 0')
    a('s_add_u32 s97, s97, 1')
    a(f's_cmp_lt_u32 s97, {G_N_OTERMS}')
    a(f's_cbranch_scc1 {L("L_ot")}')
    a.label('L_grp_f')
    a(f's_bitcmp1_b32 {G_FLAGS}, {DG_LTAB}')
    a(f's_cbranch_scc0 {L("L_g3")}')
    a('s_waitcnt vmcnt(0) lgkmcnt(0)')           # f = ltab[lane] * u
    if self.wide:
      lt_r, lt_i = V2(D_LTAB), V2(D_LTAB + 2)
    else:
      a(f'v_cvt_f32_f64 v38, v[{D_LTAB}:{D_LTAB + 1}]')
      a(f'v_cvt_f32_f64 v39, v[{D_LTAB + 2}:{D_LTAB + 3}]')
      lt_r, lt_i = 'v38', 'v39'
    a(f'{MUL} {fr}, {lt_r}, {ur}')
    a(f'{MUL} {fi}, {lt_r}, {ui}')
    a(f'{FMA} {fr}, -{lt_i}, {ui}, {fr}')
    a(f'{FMA} {fi}, {lt_i}, {ur}, {fi}')
    self.grp_dispatch(a)
    a.label('L_g3')
    self.lane_ok(a, G_LANE_MASK)                 # f = lane_ok ? u : 1
    self.f_from_u(a)
    self.grp_dispatch(a)

  def c_times(self, a, fr, fi):
    """reg_mask == 0: c *= f"""
    self.c_ensure(a)
    self.cmul_vv(a, self.cr, self.ci, fr, fi, self.dt)
    a('s_mov_b32 s75, 1')
    self.grp_tail(a)

  def apply_vector(self, a):
    """L_gm*: the factor f is in VGPRs."""
    a.label('L_gm0')
    self.c_times(a, self.fr, self.fi)
    for m in reg_masks(self.rb) + ['x']:         # 1- and 2-bit register masks: straight-line code; x: any other register mask
      a.label(f'L_gm{m}')
      self.cmul_mask(a, m, self.fr, self.fi, skip=lambda k: f'L_g_{k}')
      self.grp_tail(a)

  def apply_sign(self, a):
    """L_gn*: factor -1 (see neg_mask_vgpr)."""
    D_C, hi = self.D_C, self.W - 1
    a.label('L_gn0')                               # no register mask: c = -c on those lanes
    self.c_ensure(a)
    self.neg_mask_vgpr(a)
    a(f'v_xor_b32 v{D_C[0] + hi}, v{V_A}, v{D_C[0] + hi}')
    a(f'v_xor_b32 v{D_C[1] + hi}, v{V_A}, v{D_C[1] + hi}')
    a('s_mov_b32 s75, 1')
    self.grp_tail(a)
    for m in reg_masks(self.rb) + ['x']:
      a.label(f'L_gn{m}')
      self.neg_mask_vgpr(a)
      self.neg_mask(a, m, skip=lambda k: f'L_gn_{k}')
      self.grp_tail(a)

  def apply_uniform(self, a):
    """L_gu*: uniform groups (lane_mask == 0, no tables): phi0 sits in s[84:87].  complex128: the complex products read it
    from there (one SGPR pair per instruction: within the constant-bus limit); complex64: two conversions, then the L_gm body."""
    sfr, sfi = 's[84:85]', 's[86:87]'
    for m in [0] + reg_masks(self.rb) + ['x']:
      a.label(f'L_gu{m}')
      if not self.wide:
        a(f'v_cvt_f32_f64 v{self.D_F[0]}, {sfr}')
        a(f'v_cvt_f32_f64 v{self.D_F[1]}, {sfi}')
        a(f's_branch {L(f"L_gm{m}")}')
      elif m == 0:                                 # reg_mask == 0: c *= phi0 on every lane
        self.c_times(a, sfr, sfi)
      else:
        self.cmul_mask(a, m, sfr, sfi, skip=lambda k: f'L_gu_{k}')
        self.grp_tail(a)

  def apply_lane_masked(self, a):
    """L_gl*: lane-masked groups without tables: f = (lane & lane_mask) == lane_mask ? phi0 : 1, then the vector-factor body.
    Round 4 (the socket sits at its 1 400 W limit under these sweeps: profiles/r04/smi_trace_*.csv, so ENERGY is what a
    sweep pays in): on a register mask the factor is not blended with 1 into a per-lane f -- eleven instructions, then
    complex products in which half the lanes multiply by one --; the lanes that satisfy lane_mask are the EXEC mask and
    the products take phi0 from the SGPRs (the L_gu* bodies; grp_tail restores EXEC).  complex128; c (no register mask)
    and factor trees keep the blended f."""
    rb = self.rb
    for name, target, utarget in ([('L_gl0', 'L_gm0', None)] + [(f'L_gl{m}', f'L_gm{m}', f'L_gu{m}') for m in reg_masks(rb) + ['x']] +
                                  [(f'L_gbl{j}', f'L_gbf{j}', None) for j in range(rb)]):   # (a factor tree whose base factor has no tables)
      a.label(name)
      if self.wide and utarget:
        self.exec_from_lane_mask(a)
        a(f's_branch {L(utarget)}')
        continue
      self.lane_ok(a, 's97')
      self.u_from_sgprs(a, ('s84', 's85', 's86', 's87'))
      self.f_from_u(a)
      a(f's_branch {L(target)}')

  # ---- DIAG ops of ONE simple group, inlined into the op header (round 4) ---------------------------------------------
  # Most DIAG ops of a layered circuit carry a single group without tables or outside terms on a register mask (a cz
  # between tile bits, a T / S / Rz on a register bit): 60 of the 93 DIAG ops of supremacy-30.  Through the group machinery
  # such an op costs an op dispatch, an UNPREFETCHED 64-byte group header (a scalar round trip, 250-300 cycles behind the
  # tile stream), a group dispatch and the way out through L_diag_end -- 650-850 cycles of a wave for 20-64 VALU
  # instructions (profiles/r04/op_timeline_sup30.txt).  The host folds the group into the device copy of the op header
  # instead (kernels_sweep.hip.h inline_single_group: tb = lane_mask | reg_mask << 8, words 2-5 = the factor) and numbers
  # a handler of its own: one dispatch, no load, straight on to the next op.  complex128 only; c is not touched.
  def diag_inline(self):
    a = Asm('diag_inline', front=True)
    if not self.wide:
      return a
    skip = lambda k: self.uniq('L_d1s')
    for cls in D1_CLASSES:
      for m in reg_masks(self.rb) + ['x']:
        a.label(f'L_d1{cls}{m}')
        if cls != 'u':                              # n, l: the lanes that satisfy lane_mask
          a(f's_and_b32 s97, {OP_TB}, 0xff')
        if cls == 'n':                              # factor -1: sign flips on those lanes
          self.neg_mask_vgpr(a)
        elif cls == 'l':                            # lane-masked factor: those lanes are the EXEC mask (see L_gl*)
          self.exec_from_lane_mask(a)
        if m == 'x':
          a(f's_bfe_u32 s72, {OP_TB}, 0x80008')     # reg_mask
        if cls == 'n':
          self.neg_mask(a, m, skip=skip)
        else:                                       # u, l: the products read the factor from the header's SGPRs
          self.cmul_mask(a, m, OP_W23, OP_CM_THREAD, skip=skip)
        self.next_op(a)
    return a

  # DG_BITFAC (planner.h): slots with register bit j set take f x the factors w_k of their other set bits;
  # the subsets of those bits are walked as a tree, parent factor x w_k -> child factor (kept in VGPRs for
  # the inner nodes: three levels), so every slot costs two complex products at most.
  def bitfac_trees(self):
    a = Asm('bitfac_trees')
    for j in range(self.rb):
      a.label(f'L_gbf{j}')
      self.bitfac(a, j)
      self.grp_tail(a)
    return a

  def bitfac(self, a, j):
    rb, V2, MUL, FMA = self.rb, self.V2, self.MUL, self.FMA
    others = [b for b in range(rb) if b != j][:4]
    free = [b for b in range(rb) if b != j and b not in others]
    a('s_lshl_b32 s73, s73, 4')
    a(f's_load_dwordx16 s[76:91], {OP_CM_THREAD}, s73')
    if self.wide:
      wv = [(f's[{76 + 4 * t}:{77 + 4 * t}]', f's[{78 + 4 * t}:{79 + 4 * t}]') for t in range(4)]
      levels = [(V2(22), V2(24)), (V2(30), V2(32)), (V2(34), V2(36))]
      temps = [V2(16), V2(38)]
    else:
      # complex64: factors as (re, im) register pairs, packed arithmetic.  v18 v19 = c, v26 v27 = f.
      wv = [('v20', 'v21'), ('v22', 'v23'), ('v24', 'v25'), ('v28', 'v29')]
      levels = [('v30', 'v31'), ('v32', 'v33'), ('v34', 'v35')]
      temps = ['v[16:17]', 'v[36:37]', 'v[38:39]']

    def expand(slot):
      out = [slot]
      for b in free:
        out += [x | (1 << b) for x in out]
      return out

    def cmul_by(slots, pr, pi):
      for i in range(0, len(slots), len(temps)):
        self.cmul_slots(a, slots[i:i + len(temps)], pr, pi, temps)

    waited = [False]

    def need_w():
      if not waited[0]:
        a('s_waitcnt lgkmcnt(0)')
        if not self.wide:
          for t in range(4):
            a(f'v_cvt_f32_f64 {wv[t][0]}, s[{76 + 4 * t}:{77 + 4 * t}]')
            a(f'v_cvt_f32_f64 {wv[t][1]}, s[{78 + 4 * t}:{79 + 4 * t}]')
        waited[0] = True

    def visit(F, rem, slot, level):
      last = rem[-1] if rem else None
      mine = expand(slot)
      leaf = expand(slot | (1 << others[last])) if rem else []
      cmul_by(mine + leaf, F[0], F[1])
      if rem:
        need_w()
        cmul_by(leaf, wv[last][0], wv[last][1])
      for idx, t in enumerate(rem[:-1]):
        need_w()
        C = levels[level]
        if self.wide:
          a(f'{MUL} {C[0]}, {F[0]}, {wv[t][0]}')
          a(f'{MUL} {C[1]}, {F[0]}, {wv[t][1]}')
          a(f'{FMA} {C[0]}, -{F[1]}, {wv[t][1]}, {C[0]}')
          a(f'{FMA} {C[1]}, {F[1]}, {wv[t][0]}, {C[1]}')
        else:
          pk_cmul(a, vpair(C[0]), vpair(F[0]), vpair(wv[t][0]), temps[0])
        visit(C, rem[idx + 1:], slot | (1 << others[t]), level + 1)

    visit((self.fr, self.fi), list(range(len(others))), 1 << j, 0)

  def diag_end(self):
    a = Asm('diag_end')
    a.label('L_diag_ci')                           # (a taken branch costs a wave ~50 cycles: the common path falls through)
    self.c_init(a)
    a(f's_branch {L("L_diag_nc")}')

    a.label('L_diag_end')
    a('s_cmp_eq_u32 s75, 0')
    a(f's_cbranch_scc1 {L("L_next")}')
    a(f's_bitcmp1_b32 {OP_FLAGS}, {OPF_DEFER_C}')  # the next (lane) op folds c into its matrix
    a(f's_cbranch_scc1 {L("L_next")}')
    a(f's_bitcmp1_b32 {OP_FLAGS}, {OPF_C_SIGN}')   # every factor that went into c is -1: c = +-1 per lane
    a(f's_cbranch_scc1 {L("L_c_sign")}')
    if self.wide:                                  # lanes whose c is exactly one sit the products out (energy, see L_gl*)
      a(f'v_cmp_neq_f64 vcc, 1.0, {self.cr}')
      a(f'v_cmp_neq_f64 s[72:73], 0, {self.ci}')
      a('s_nop 1')
      a('s_or_b64 vcc, vcc, s[72:73]')
      a('s_and_b64 exec, exec, vcc')
    self.cmul_mask(a, 0, self.cr, self.ci)
    self.next_op(a)
    a.label('L_c_sign')                            # ... so applying it is a sign flip: the sign bit of re(c), per lane
    a(f'v_and_b32 v{V_A}, 0x80000000, v{self.D_C[0] + self.W - 1}')
    self.neg_mask(a, 0)
    self.next_op(a)
    return a

  # ---- store the tile -------------------------------------------------------------------
  def store(self):
    a, X, Y = Asm('store'), self.X, self.Y
    a.label('L_done')
    self.tile_io(a, store=True)
    self.prof_rec(a)
    self.prof_rec(a, wait_stores=True, real_at=127)
    # ---- optional epilogue: the largest |amplitude|^2 of the tile (qh_argmax right behind a flush) ----------------
    # The reader that follows most circuits (maxprob: state.py:60-78) is a full pass over the state (2.9 ms at 30 qubits,
    # 45 ms at 34).  When the flush that precedes it ends in a sweep that touches every amplitude, the LAST sweep leaves
    # the maximum of every unit it stores in SweepParams::tilemax[unit] (+0x38, 0 = off): re^2 + im^2 per slot, v_max over
    # the slots, four DPP steps over the 16 lanes of a row, one 64-bit unsigned atomic max per row (non-negative doubles
    # order like their bit patterns).  The engine then looks only at the units that hold the maximum (engine.hip
    # argmax_from_tilemax).  ~110 VALU instructions per complex128 tile, ~340 per complex64 tile of 64 amplitudes per lane (two
    # conversions per amplitude: the probabilities are doubles either way, exactly those of the full pass).
    a(f's_load_dwordx2 s[74:75], {PRM}, 0x38')
    a('s_waitcnt lgkmcnt(0)')
    a('s_cmp_eq_u64 s[74:75], 0')
    a(f's_cbranch_scc1 {L("L_tmax_end")}')
    for k in range(self.nr):
      d = 'v[16:17]' if k == 0 else 'v[18:19]'
      if self.wide:
        a(f'v_mul_f64 {d}, {X(k)}, {X(k)}')
        a(f'v_fma_f64 {d}, {Y(k)}, {Y(k)}, {d}')
      else:               # complex64 tiles: the probability in double precision, as the full pass computes it
        a(f'v_cvt_f64_f32 {d}, {X(k)}')
        a(f'v_cvt_f64_f32 v[20:21], {Y(k)}')
        a(f'v_mul_f64 {d}, {d}, {d}')
        a(f'v_fma_f64 {d}, v[20:21], v[20:21], {d}')
      if k:
        a('v_max_f64 v[16:17], v[16:17], v[18:19]')
    for ctl in ('quad_perm:[1,0,3,2]', 'quad_perm:[2,3,0,1]', 'row_half_mirror', 'row_mirror'):
      a('s_nop 1')                                  # (a DPP read of a VGPR a VALU instruction has just written)
      a(f'v_mov_b32_dpp v18, v16 {ctl} row_mask:0xf bank_mask:0xf')
      a(f'v_mov_b32_dpp v19, v17 {ctl} row_mask:0xf bank_mask:0xf')
      a('v_max_f64 v[16:17], v[16:17], v[18:19]')
    a(f's_lshl_b32 s76, {TENT}, 3')
    a('s_add_u32 s74, s74, s76')
    a('s_addc_u32 s75, s75, 0')
    a('v_mov_b32 v20, 0')
    a('s_mov_b64 s[76:77], exec')
    a('s_mov_b32 s78, 0x00010001')
    a('s_mov_b32 s79, 0x00010001')
    a('s_mov_b64 exec, s[78:79]')                   # lanes 0, 16, 32, 48: one per row
    a('s_nop 1')
    a('global_atomic_umax_x2 v20, v[16:17], s[74:75]')
    a('s_mov_b64 exec, s[76:77]')
    a.label('L_tmax_end')
    a('s_nop 0')
    return a

  def wrap(self, lines):
    """The island as the C++ kernel includes it: one asm volatile statement with its operands and clobbers."""
    clob = ([f'v{i}' for i in range(TEMP_LO, T0 + 2 * self.W * self.nr)] + [f's{i}' for i in range(16, 28)] + [f's{i}' for i in range(36, 100)] +
            (['s28', 's29', 's30', 's31', 's101'] if self.prof else []) + ['vcc', 'scc', 'memory'])
    body = '\n'.join(f'    "{ln}\\n\\t"' for ln in lines)
    cl = ', '.join(f'"{c}"' for c in clob)
    return (f'// GENERATED by tools/gen_sweep_asm.py (RB={self.rb}, {"complex128" if self.wide else "complex64"}) -- do not edit.\n'
            f'asm volatile(\n{body}\n'
            '    : [tidx] "+s"(tile_idx), [itlo] "+v"(it_lo), [ithi] "+v"(it_hi)\n'
            '    : [blo] "s"(base_lo), [bhi] "s"(base_hi), [prm] "s"(prm), [voff] "v"(voff), [lane] "v"(lane_u),\n'
            '      [wave] "s"(wave_s), [lds] "s"(lds_base), [ltab] "s"(lds_ltab),\n'
            '      [sblo] "s"(sbase_lo), [sbhi] "s"(sbase_hi), [svoff] "v"(svoff), [nlt] "s"(nlt_now), [wgthr] "s"(wg_threads),\n'
            '      [tent] "s"(tmax_entry)' + (', [prow] "s"(prof_row)' if self.prof else '') + '\n'
            f'    : {cl});\n')


# s_branch / s_cbranch reach +-32 Ki dwords (128 KiB).  The complex64 RB=6 island is ~180 KiB of code:
# its op sections are laid out on BOTH sides of the dispatcher (entry jumps over the first half), so
# that every section is within reach of L_op / L_next / L_done and of the sections it jumps into.
# (the complex128 RB=5 island -- 21 000 lines, ~120 KiB -- still assembles in the linear layout, and runs the QFT 2 % faster
# in it: the dispatcher and the handlers a sweep uses stay close together)
# The fused butterflies of round 4 sit in FRONT of the entry (which jumps over them): the dispatcher and every older
# handler keep their distances -- the complex128 RB=5 island was within 5 KiB of the reach of a branch already.
REACH_LINES = 21500      # (~125 KiB: beyond it the assembler refuses branches across the island)


def layout(sections):
  """The island's lines from its sections in emission order: front sections before L_entry; when the body is beyond the
  reach of a branch, the sections from reg_dense up to the first `cut` section at or past the middle of the op code
  (reg_dense .. store) go in front of the dispatcher too."""
  front = [s for s in sections if s.front and s.lines]
  body = [s for s in sections if not s.front]
  if sum(len(s.lines) for s in body) > REACH_LINES:
    at, starts = 0, []
    for s in body:
      starts.append(at)
      at += len(s.lines)
    names = [s.name for s in body]
    first, last = names.index('reg_dense'), names.index('store')
    mid = (starts[first] + starts[last]) // 2
    cuts = [i for i in range(first + 1, last) if body[i].cut]
    cut = min((i for i in cuts if starts[i] >= mid), default=cuts[-1])
    front, body = front + body[first:cut], body[:first] + body[cut:]
  order = front + [None] + body if front else body
  for s, nxt in zip(order, order[1:]):             # no section falls through into whatever the layout put behind it
    assert s is None or s.ends_in_jump() or (nxt is not None and s.falls_into == nxt.name), (s.name, nxt and nxt.name)
  lines = [f's_branch {L("L_entry")}'] if front else []
  for s in order:
    lines += [f'{L("L_entry")}:'] if s is None else s.lines
  return lines


def gen(rb, wide=True, prof=False, nomem=0):
  """The island of 2^rb amplitudes per lane, complex128 (wide) or complex64, as the text of its .inc file."""
  isl = Island(rb, wide, prof, nomem)
  return isl.wrap(layout([                       # (emission order: it numbers the unique labels)
      isl.prologue(), isl.dispatcher(),
      isl.reg_dense(), isl.real_dense(), isl.real_controlled(), isl.lane_real(),
      isl.reg_butterflies(), isl.rot_butterflies(), isl.lane_butterflies(),
      isl.lswap(), isl.wswap(), isl.dpp_butterfly(), isl.dpp_real(), isl.lane_dense(),
      isl.diag_groups(), isl.diag_inline(), isl.bitfac_trees(), isl.diag_end(),
      isl.store()]))


def main():
  out = os.environ.get('QH_ISLAND_OUT') or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'qcc_amd', 'csrc')
  nomem = int(os.environ.get('QH_ISLAND_NOMEM', '0'))
  if os.environ.get('QH_ISLAND_PROF') == '1':
    path = os.path.join(out, 'sweep_island_prof_rb5.inc')
    with open(path, 'w') as f:
      f.write(gen(5, True, prof=True, nomem=nomem))
    print('wrote', path)
    return 0
  with open(os.path.join(out, 'sweep_handlers.inc'), 'w') as f:
    f.write(handlers_header())
  for wide in (True, False):
    for rb in (2, 3, 4, 5) + (() if wide else (6,)):     # complex64: 64 amplitudes per lane fit the same 128 VGPRs
      path = os.path.join(out, f'sweep_island_rb{rb}.inc' if wide else f'sweep_island_f32_rb{rb}.inc')
      with open(path, 'w') as f:
        f.write(gen(rb, wide, nomem=nomem))
      print('wrote', path, sum(1 for _ in open(path)), 'lines')


if __name__ == '__main__':
  sys.exit(main())
