"""CPU tests of the Pauli products: the C-ABI symbols and their argument checks on planner-only handles,
qh_pauli_product_plan's runs against the greedy rule restated in Python, qc.pauli_rot / apply_pauli / evolve / imaginary_time /
pauli_project with the GPU replaced by a NumPy stand-in that implements apply_pauli_product and over the fallback that reads
qc.psi, the golden rotations of the reference, and tools/pauli_product_plan_check.cc stand-alone under ASan and UBSan.

The reference value everywhere is pauli_product_util.np_pauli_product: the factors a_t I + b_t P_t one by one in complex128
NumPy, term 0 first, with pauli_util's (P v)_i = (-i)^nY (-1)^popcount(i & z) v_{i ^ x}; it is cross-checked once against
np.kron of qcc_amd.lib.ops Paulis."""
import ctypes
import functools
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

from qcc_amd import device, native
from qcc_amd.lib import backend, circuit, ops, tensor
from tests import fake_device, pauli_product_util as ppu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_dp = ctypes.POINTER(ctypes.c_double)
_up = ctypes.POINTER(ctypes.c_uint64)
BATCH = native.QH_PAULI_PRODUCT_BATCH
KINDS = (native.QH_PAULI_RUN_DIAG, native.QH_PAULI_RUN_PAIR, native.QH_PAULI_RUN_HALF)


class ProductOracle(fake_device.OracleDevice):
  """OracleDevice with apply_pauli_product in NumPy (logical order = the array's order)."""
  applied = 0

  def apply_pauli_product(self, a, b, xmasks, zmasks, norm=False):
    ProductOracle.applied += 1
    self.psi[:] = ppu.np_pauli_product(self.psi, a, b, xmasks, zmasks).astype(self.dtype)
    return float(np.vdot(self.psi.astype(np.complex128), self.psi.astype(np.complex128)).real) if norm else None


MATS = {'I': np.eye(2, dtype=np.complex128), 'X': np.asarray(ops.PauliX(), dtype=np.complex128),
        'Y': np.asarray(ops.PauliY(), dtype=np.complex128), 'Z': np.asarray(ops.PauliZ(), dtype=np.complex128)}


def kron_string(s):
  """one Pauli string as a dense matrix: np.kron of qcc_amd.lib.ops Paulis, letter q on qubit q"""
  return functools.reduce(np.kron, [MATS[ch] for ch in s])


def string_masks(s):
  n = len(s)
  x = sum(1 << (n - 1 - q) for q, ch in enumerate(s) if ch in 'XY')
  z = sum(1 << (n - 1 - q) for q, ch in enumerate(s) if ch in 'ZY')
  return x, z


def expm_string(s, theta):
  """exp(-i theta P) = cos(theta) I - i sin(theta) P, dense"""
  return math.cos(theta) * np.eye(1 << len(s)) - 1j * math.sin(theta) * kron_string(s)


def test_reference_formula_against_kron():
  """The formula every other test trusts, once against dense matrices at 6 qubits: a product of 12 factors with random
  complex a, b over random strings, in order (the factors do not commute), and the order reversed gives something else."""
  rng = np.random.default_rng(16)
  n = 6
  psi = rng.normal(size=1 << n) + 1j * rng.normal(size=1 << n)
  strings = [''.join(rng.choice(list('IXYZ'), size=n)) for _ in range(12)]
  a = [complex(*rng.normal(size=2)) for _ in strings]
  b = [complex(*rng.normal(size=2)) for _ in strings]
  xs, zs = zip(*[string_masks(s) for s in strings])
  want = psi.copy()
  for at, bt, s in zip(a, b, strings):
    want = (at * np.eye(1 << n) + bt * kron_string(s)) @ want
  got = ppu.np_pauli_product(psi, a, b, xs, zs)
  np.testing.assert_allclose(got, want, atol=1e-10 * float(np.max(np.abs(want))))
  rev = ppu.np_pauli_product(psi, a[::-1], b[::-1], xs[::-1], zs[::-1])
  assert np.max(np.abs(rev - want)) > 1e-3 * float(np.max(np.abs(want)))
  y = ppu.np_pauli_product(np.array([2.0, 3.0]), [0.0], [1.0], [1], [1])      # (Y v)_0 = -i v_1, (Y v)_1 = i v_0
  assert y[0] == -3j and y[1] == 2j


def test_golden_rotations_of_the_reference():
  """tests/golden/g13_pauli_rot.npz (tools/make_golden_pauli_rot.py): (cos t I - i sin t P) psi from the reference's own
  Pauli Kronecker products, against the util formula"""
  g = np.load(os.path.join(ROOT, 'tests', 'golden', 'g13_pauli_rot.npz'))
  psi = g['psi']
  assert int(g['nbits']) == 8 and psi.shape == (256,) and len(g['strings']) >= 12
  letters = set()
  for s, t, want in zip(g['strings'], g['thetas'], g['rotated']):
    s = str(s)
    letters |= set(s)
    x, z = string_masks(s)
    got = ppu.np_pauli_product(psi, [math.cos(t)], [-1j * math.sin(t)], [x], [z])
    assert np.max(np.abs(got - want)) <= 1e-13, s
  assert letters == set('IXYZ')


# ---- the C-ABI ---------------------------------------------------------------------------------------------------------
def test_version_symbols_and_structs():
  lib = native.load()
  assert lib.qh_version() >= 116
  for name in ('qh_apply_pauli_product', 'qh_pauli_product_plan'):
    assert name in native.SIGNATURES
    assert getattr(lib, name).argtypes == native.SIGNATURES[name][1]
  assert BATCH in (8, 16)
  assert len(set(KINDS)) == 3
  assert ctypes.sizeof(native.QhPauliRun) == 32 and ctypes.sizeof(native.QhPauliTerm) == 32
  header = open(os.path.join(ROOT, 'include', 'qcc_hip.h')).read()
  assert f'#define QH_PAULI_PRODUCT_BATCH {BATCH}\n' in header
  for name, v in zip(('DIAG', 'PAIR', 'HALF'), KINDS):
    assert f'#define QH_PAULI_RUN_{name} {v}\n' in header


def _dry(n, bw=128, nglob=None, shard=0):
  st = device.DeviceState(n, bw, dry=True)
  if nglob is not None:
    st.set_shard(nglob, shard)
  return st


def _pending(st):
  pend = ctypes.c_uint64()
  native.check(st.lib.qh_pending_gates(st.h, ctypes.byref(pend)))
  return pend.value


def test_apply_argument_errors():
  """every refusal that needs no state: null handle and arrays, a dry handle, non-finite coefficients (the message names the
  first offending term); norm2 is untouched"""
  lib = native.load()
  st = _dry(10)
  try:
    n2 = ctypes.c_double(7.0)

    def call(h, ab, xs, zs, abp=True, xp=True, zp=True):
      x, z = np.asarray(xs, dtype=np.uint64), np.asarray(zs, dtype=np.uint64)
      co = np.asarray(ab, dtype=np.float64)
      return lib.qh_apply_pauli_product(h.h if h else None, x.size, co.ctypes.data_as(_dp) if abp else None,
                                        x.ctypes.data_as(_up) if xp else None, z.ctypes.data_as(_up) if zp else None, ctypes.byref(n2))
    ok = [1.0, 0.0, 0.0, 1.0]
    assert call(None, ok, [1], [0]) == native.QH_ERR_ARG
    assert call(st, ok, [1], [0], abp=False) == native.QH_ERR_ARG
    assert call(st, ok, [1], [0], xp=False) == native.QH_ERR_ARG
    assert call(st, ok, [1], [0], zp=False) == native.QH_ERR_ARG
    assert call(st, ok, [1], [0]) == native.QH_ERR_ARG                  # dry handles hold no state
    assert b'dry' in lib.qh_last_error()
    assert call(st, [], [], [], abp=False, xp=False, zp=False) == native.QH_ERR_ARG      # ... not even for no terms
    assert n2.value == 7.0
  finally:
    st.close()


def _plan_rc(st, xs, zs, xp=True, zp=True, nrp=True, cap=64, rp=True):
  lib = native.load()
  x, z = np.asarray(xs, dtype=np.uint64), np.asarray(zs, dtype=np.uint64)
  runs = (native.QhPauliRun * max(cap, 1))()
  nr = ctypes.c_uint64(99)
  rc = lib.qh_pauli_product_plan(st.h if st else None, x.size, x.ctypes.data_as(_up) if xp else None, z.ctypes.data_as(_up) if zp else None,
                                 None, runs if rp else None, cap, ctypes.byref(nr) if nrp else None)
  return rc, nr.value


def test_plan_argument_errors_on_planner_only_handles():
  """qh_pauli_product_plan makes every check of qh_apply_pauli_product that needs no state, on planner-only handles: null
  pointers, mask bits at or above nbits_global, and X or Y on a bit the shard index holds -- also for a LATER term, with
  nothing flushed"""
  lib = native.load()
  st, sh = _dry(10), _dry(10, nglob=12, shard=2)
  had = np.array([1, 0, 1, 0, 1, 0, -1, 0], dtype=np.float64) / math.sqrt(2.0)
  try:
    assert _plan_rc(None, [1], [0])[0] == native.QH_ERR_ARG
    assert _plan_rc(st, [1], [0], xp=False)[0] == native.QH_ERR_ARG
    assert _plan_rc(st, [1], [0], zp=False)[0] == native.QH_ERR_ARG
    assert _plan_rc(st, [1], [0], nrp=False)[0] == native.QH_ERR_ARG
    assert _plan_rc(st, [1], [0], rp=False)[0] == native.QH_ERR_ARG
    assert _plan_rc(st, [1], [0], rp=False, cap=0) == (native.QH_OK, 1)            # the count-only form
    assert _plan_rc(st, [1, 2, 1], [0, 0, 0], cap=1) == (native.QH_OK, 3)           # cap smaller than the number of runs
    assert _plan_rc(st, [1, 1 << 10], [0, 0])[0] == native.QH_ERR_BAD_QUBIT
    assert _plan_rc(st, [1, 2], [0, 1 << 63])[0] == native.QH_ERR_BAD_QUBIT
    assert _plan_rc(sh, [1], [1 << 12])[0] == native.QH_ERR_BAD_QUBIT
    assert _plan_rc(st, [], [], xp=False, zp=False) == (native.QH_OK, 0)            # nterms == 0: no run
    for h in (st, sh):                                                             # gates queued stay queued
      native.check(lib.qh_set_fusion(h.h, native.QH_FUSE_SWEEP))
      native.check(lib.qh_apply1(h.h, 3, had.ctypes.data_as(_dp)))
      assert _pending(h) == 1
    assert _plan_rc(sh, [1, 2, 1 << 11], [0, 0, 0])[0] == native.QH_ERR_NONLOCAL   # a LATER term: x on a held bit
    assert b'shard index' in lib.qh_last_error() and b'term 2' in lib.qh_last_error()
    assert _plan_rc(sh, [1, 3], [1 << 11, 1 << 10]) == (native.QH_OK, 2)           # z there is a sign
    assert _pending(sh) == 1 and _pending(st) == 1
    # the apply call makes the same checks, in the same order, before it looks at the state (so they show on planner-only
    # handles): refused for the later term before anything is flushed, norm2 untouched
    n2 = ctypes.c_double(7.0)
    x, z = np.array([1, 2, 1 << 11], dtype=np.uint64), np.zeros(3, dtype=np.uint64)
    co = np.tile([1.0, 0.0, 0.0, 1.0], 3)
    bad = np.array([1, 2, 1 << 13], dtype=np.uint64)

    def apply(h, c, xm):
      return lib.qh_apply_pauli_product(h.h, 3, c.ctypes.data_as(_dp), xm.ctypes.data_as(_up), z.ctypes.data_as(_up), ctypes.byref(n2))
    assert apply(sh, co, x) == native.QH_ERR_NONLOCAL and b'term 2' in lib.qh_last_error()
    assert apply(sh, co, bad) == native.QH_ERR_BAD_QUBIT and b'term 2' in lib.qh_last_error()
    assert apply(st, co, x) == native.QH_ERR_BAD_QUBIT                            # bit 11 of a 10-qubit state
    for nonfinite in (np.nan, np.inf, -np.inf):
      for slot in range(4):
        c2 = co.copy()
        c2[4 + slot] = nonfinite
        c2[8 + slot] = nonfinite
        assert apply(sh, c2, x) == native.QH_ERR_ARG
        assert b'term 1 ' in lib.qh_last_error() and b'non-finite' in lib.qh_last_error()      # the FIRST offending term
    assert n2.value == 7.0 and _pending(sh) == 1 and _pending(st) == 1
    sh.remap_swap(11, 0)                                                           # logical 0 is now held, logical 11 local
    assert _plan_rc(sh, [1 << 11], [0]) == (native.QH_OK, 1)
    assert _plan_rc(sh, [1 << 11, 1], [0, 0])[0] == native.QH_ERR_NONLOCAL
    assert _plan_rc(sh, bad, [0, 0, 0])[0] == native.QH_ERR_BAD_QUBIT
  finally:
    st.close()
    sh.close()


def _check_plan(st, xs, zs, amp_bits, phys=None):
  """the plan of (xs, zs) on st against the restated rule; phys maps a logical mask to the physical one"""
  phys = phys or (lambda m: m)
  terms, runs = st.pauli_product_plan(xs, zs)
  assert [t['index'] for t in terms] == list(range(len(xs)))                       # the caller's order
  assert [t['px'] for t in terms] == [phys(x) for x in xs]
  assert [t['ny'] for t in terms] == [bin(x & z).count('1') % 4 for x, z in zip(xs, zs)]
  want = ppu.greedy_runs([t['px'] for t in terms], BATCH, amp_bits, KINDS)
  assert [(r['first'], r['count'], r['px'], r['kind']) for r in runs] == want
  return terms, runs


def test_plan_runs_against_the_greedy_rule():
  rng = np.random.default_rng(7)
  for bw, ab in ((128, 0), (64, 1)):
    st = _dry(12, bw)
    try:
      D, P, H = KINDS
      # hand-made lists
      _, runs = _check_plan(st, [0] * (3 * BATCH), list(range(3 * BATCH)), ab)      # a long diagonal stretch
      assert [r['count'] for r in runs] == [BATCH] * 3 and all(r['kind'] == D for r in runs)
      _, runs = _check_plan(st, [6] * BATCH, [0] * BATCH, ab)                       # exactly BATCH
      assert len(runs) == 1 and runs[0]['kind'] == P
      _, runs = _check_plan(st, [6] * (BATCH + 1), [0] * (BATCH + 1), ab)           # and one more
      assert [r['count'] for r in runs] == [BATCH, 1]
      _, runs = _check_plan(st, [2, 4, 2, 4, 2], [1] * 5, ab)                       # alternating masks
      assert len(runs) == 5
      _, runs = _check_plan(st, [0, 0, 6, 0, 6, 0, 4, 0], [3] * 8, ab)              # diagonal terms join either side
      assert [(r['first'], r['count'], r['px']) for r in runs] == [(0, 6, 6), (6, 2, 4)]
      _, runs = _check_plan(st, [1, 0, 1], [0, 5, 1], ab)                           # X == 1: inside one item at complex64
      assert len(runs) == 1 and runs[0]['kind'] == (H if ab else P)
      _, runs = _check_plan(st, [3], [0], ab)
      assert runs[0]['kind'] == P
      # random lists: few masks, stretches of one mask with diagonal terms among them
      for _ in range(60):
        n = int(rng.integers(1, 70))
        pool = [int(v) for v in rng.integers(1, 1 << 12, size=int(rng.integers(1, 4)))] + [1]
        xs, cur = [], pool[0]
        for _t in range(n):
          if rng.random() < 0.15:
            cur = pool[int(rng.integers(len(pool)))]
          xs.append(0 if rng.random() < 0.3 else cur)
        _check_plan(st, xs, [int(v) for v in rng.integers(0, 1 << 12, size=n)], ab)
      # after qh_remap_swap the masks are physical
      st.remap_swap(0, 11)
      st.remap_swap(3, 4)
      swap = {0: 11, 11: 0, 3: 4, 4: 3}
      phys = lambda m: sum(1 << swap.get(b, b) for b in range(12) if (m >> b) & 1)      # noqa: E731
      terms, runs = _check_plan(st, [1, 1 << 11, 1 << 11, 0, 1 << 3], [1 << 4, 1, 9, 1 << 11, 0], ab, phys)
      assert [t['pz'] for t in terms] == [1 << 3, 1 << 11, (1 << 11) | (1 << 4), 1, 0]
      assert runs[1]['px'] == 1 and runs[1]['kind'] == (H if ab else P)             # logical bit 11 sits on physical bit 0
    finally:
      st.close()


def test_plan_on_shard_handles():
  """A z bit held by the shard index is the sign `neg`, as it is on this shard; the local part of the masks remains and
  the runs are those of the local x masks."""
  for bw, ab in ((128, 0), (64, 1)):
    for shard, negs in [(0, [0, 0, 0, 0]), (1, [1, 0, 1, 0]), (2, [0, 1, 1, 0]), (3, [1, 1, 0, 0])]:
      sh = _dry(10, bw, nglob=12, shard=shard)
      try:
        terms, runs = _check_plan(sh, [3, 0, 3, 1], [(1 << 10) | 1, (1 << 11) | 2, (3 << 10) | 4, 7], ab)
        assert [t['neg'] for t in terms] == negs
        assert [t['pz'] for t in terms] == [1, 2, 4, 7]
        assert [(r['first'], r['count'], r['px']) for r in runs] == [(0, 3, 3), (3, 1, 1)]
      finally:
        sh.close()


def test_plan_check_stand_alone_with_sanitizers(tmp_path):
  """tools/pauli_product_plan_check.cc is plain C++ over pauli_product_plan.h with its own main: the runs partition the terms
  in order, every item is visited exactly once and the split signs equal the popcount signs, at both widths and every size
  from 1 to 14 local bits.  Built with ASan and UBSan, the runtimes linked statically; nothing is loaded into this process."""
  cxx = shutil.which('g++')
  assert cxx, 'no g++'
  exe = str(tmp_path / 'pauli_product_plan_check')
  subprocess.check_call([cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-static-libasan',
                         '-static-libubsan', os.path.join(ROOT, 'tools', 'pauli_product_plan_check.cc'), '-o', exe])
  res = subprocess.run([exe, '6'], capture_output=True, text=True, timeout=120)
  assert res.returncode == 0, res.stdout + res.stderr
  assert 'ok' in res.stdout


# ---- qc on NumPy devices -------------------------------------------------------------------------------------------------
@pytest.fixture(params=[('apply_pauli_product', 128), ('apply_pauli_product', 64), ('fallback', 128), ('fallback', 64)],
                ids=lambda p: f'{p[0]}-{p[1]}')
def cpu_backend(request):
  kind, width = request.param
  tensor.set_tensor_width(width)
  backend.set_device_factory(ProductOracle if kind == 'apply_pauli_product' else fake_device.OracleDevice)
  yield kind, width
  backend.set_device_factory(None)
  tensor.set_tensor_width(None)


def _circuit(nq, seed):
  rng = np.random.default_rng(seed)
  q = circuit.qc('p')
  q.reg(nq, 0)
  for _ in range(3 * nq):
    a = int(rng.integers(nq))
    q.ry(a, float(rng.random() * 3))
    b = int(rng.integers(nq))
    if b != a:
      q.cx(a, b)
    q.rz(int(rng.integers(nq)), float(rng.random() * 3))
  return q


def _amps(q):
  return np.asarray(q.psi).reshape(-1).astype(np.complex128)


def _eps(width):
  return 1e-13 if width == 128 else 2e-6


def test_pauli_rot_is_rx_ry_rz(cpu_backend):
  kind, width = cpu_backend
  n = 4
  for letter, gate in (('X', 'rx'), ('Y', 'ry'), ('Z', 'rz')):
    for qb in range(n):
      theta = 0.3 + qb + 0.1 * ord(letter)
      q, ref = _circuit(n, 3), _circuit(n, 3)
      applied = ProductOracle.applied
      q.pauli_rot({qb: letter}, theta)
      getattr(ref, gate)(qb, theta)
      if kind == 'apply_pauli_product':
        assert ProductOracle.applied == applied + 1
      assert np.max(np.abs(_amps(q) - _amps(ref))) <= _eps(width), (letter, qb)
  # a str string, and against the dense exponential
  q = _circuit(n, 4)
  psi = _amps(q)
  q.pauli_rot('XYIZ', 1.1)
  assert np.max(np.abs(_amps(q) - expm_string('XYIZ', 0.55) @ psi)) <= _eps(width)
  q.h(0)                                                     # gates afterwards act on the new state
  ref = circuit.qc('r')
  ref.reg(n, 0)
  ref.psi = (expm_string('XYIZ', 0.55) @ psi).astype(np.asarray(q.psi).dtype)
  ref.h(0)
  assert np.max(np.abs(_amps(q) - _amps(ref))) <= 2 * _eps(width)


def test_apply_pauli_is_the_dense_string_exactly(cpu_backend):
  _kind, _width = cpu_backend
  n = 5
  rng = np.random.default_rng(2)
  for s in ['XXXXX', 'YYYYY', 'ZZZZZ', 'IIYII', 'XYZIY'] + [''.join(rng.choice(list('IXYZ'), size=n)) for _ in range(5)]:
    q = _circuit(n, 5)
    stored = np.asarray(q.psi).reshape(-1).copy()
    q.apply_pauli(s)
    want = (kron_string(s) @ stored.astype(np.complex128)).astype(stored.dtype)      # moves, negations, swaps: exact
    assert np.array_equal(np.asarray(q.psi).reshape(-1), want), s
    q.apply_pauli({k: ch for k, ch in enumerate(s)})                                # P P = I, exactly
    assert np.array_equal(np.asarray(q.psi).reshape(-1), stored), s


def test_evolve_commuting_terms_and_order_two(cpu_backend):
  kind, width = cpu_backend
  n = 5
  # mutually commuting terms: exp(-i t sum c P) = prod exp(-i t c P), whatever the steps
  terms = [(0.7, 'ZZIII'), (-0.4, 'IIZZI'), (1.3, 'IIIZI'), (0.25, 'IIZIZ'), (0.9, 'XXIII'), (-0.6, 'YYIII')]
  t = 0.83
  for steps in (1, 3):
    q = _circuit(n, 6)
    psi = _amps(q)
    applied = ProductOracle.applied
    q.evolve(terms, t, steps=steps)
    if kind == 'apply_pauli_product':
      assert ProductOracle.applied == applied + 1          # all steps in one call
    want = psi
    for c, s in terms:
      want = expm_string(s, t * c) @ want
    assert np.max(np.abs(_amps(q) - want)) <= 4 * steps * _eps(width)
  # terms that do not commute: order 1 is the product in the caller's order, order 2 its explicit palindrome
  terms = [(0.7, 'ZZIII'), (-0.4, {1: 'X'}), (1.3, 'IYZII'), (0.25, 'XIIIX')]
  strs = ['ZZIII', 'IXIII', 'IYZII', 'XIIIX']
  cs = [c for c, _ in terms]
  for steps in (1, 2):
    dt = t / steps
    q = _circuit(n, 7)
    psi = _amps(q)
    q.evolve(terms, t, steps=steps)
    want = psi
    for _ in range(steps):
      for c, s in zip(cs, strs):
        want = expm_string(s, dt * c) @ want
    assert np.max(np.abs(_amps(q) - want)) <= 8 * steps * _eps(width)
    q2, q3 = _circuit(n, 7), _circuit(n, 7)
    q2.evolve(terms, t, steps=steps, order=2)
    want2 = psi
    for _ in range(steps):
      for c, s in list(zip(cs, strs)) + list(zip(cs, strs))[::-1]:
        want2 = expm_string(s, dt * c / 2) @ want2
        q3.pauli_rot(s, dt * c)                            # pauli_rot takes theta / 2: the half angle
    assert np.max(np.abs(_amps(q2) - want2)) <= 16 * steps * _eps(width)
    assert np.max(np.abs(_amps(q2) - _amps(q3))) <= 16 * steps * _eps(width)
    assert np.max(np.abs(want2 - want)) > 1e-3              # ... and it is not the first-order product
  q = _circuit(n, 7)
  psi = np.asarray(q.psi).copy()
  q.evolve([], 1.0)                                         # no terms: nothing happens
  assert np.array_equal(np.asarray(q.psi), psi)


def test_imaginary_time_and_projection(cpu_backend):
  _kind, width = cpu_backend
  n = 4
  terms = [(0.8, 'ZZII'), (-0.5, 'IXII'), (0.3, 'IIYZ')]
  tau = 0.6
  for normalize in (False, True):
    q = _circuit(n, 8)
    psi = _amps(q)
    norm2 = q.imaginary_time(terms, tau, steps=2, normalize=normalize)
    want = psi
    for _ in range(2):
      for c, s in terms:
        want = (math.cosh(tau / 2 * c) * np.eye(1 << n) - math.sinh(tau / 2 * c) * kron_string(s)) @ want
    n2 = float(np.vdot(want, want).real)
    assert isinstance(norm2, float) and abs(norm2 - n2) <= 1e-5 * n2          # before normalisation
    if normalize:
      want = want / math.sqrt(n2)
      assert abs(q.norm2() - 1.0) <= 4 * _eps(width)
    assert np.max(np.abs(_amps(q) - want)) <= 16 * _eps(width) * max(1.0, math.sqrt(n2))
  # projections: probabilities of the two outcomes add up to the norm, the projected state is an eigenstate
  for s in ('ZIII', 'XXII', 'YZXI'):
    p = {}
    for ev in (+1, -1):
      q = _circuit(n, 9)
      psi = _amps(q)
      p[ev] = q.pauli_project(s, ev)
      want = 0.5 * (psi + ev * (kron_string(s) @ psi))
      assert abs(p[ev] - float(np.vdot(want, want).real)) <= 8 * _eps(width)
      assert np.max(np.abs(_amps(q) - want / math.sqrt(p[ev]))) <= 8 * _eps(width)
      assert abs(q.norm2() - 1.0) <= 8 * _eps(width)
      got = _amps(q)
      assert np.max(np.abs(kron_string(s) @ got - ev * got)) <= 16 * _eps(width)
    assert abs(p[+1] + p[-1] - 1.0) <= 16 * _eps(width)
    q = _circuit(n, 9)
    psi = _amps(q)
    pr = q.pauli_project(s, -1, normalize=False)
    assert np.max(np.abs(_amps(q) - 0.5 * (psi - kron_string(s) @ psi))) <= 8 * _eps(width) and abs(pr - p[-1]) <= 8 * _eps(width)
  # a zero result: |0000> has no -1 component of ZIII
  q = circuit.qc('z')
  q.reg(n, 0)
  with pytest.raises(ValueError, match='nothing to normalise'):
    q.pauli_project('ZIII', -1)
  assert not np.any(np.asarray(q.psi))
  q = circuit.qc('z')
  q.reg(n, 0)
  assert q.pauli_project('ZIII', +1) == 1.0 and np.asarray(q.psi).reshape(-1)[0] == 1.0


def test_argument_errors(cpu_backend):
  q = _circuit(4, 2)
  psi = np.asarray(q.psi).copy()
  for bad in ('XYZ', 'XYZII', 'XAZI', {4: 'X'}, {-1: 'Z'}, {0: 'Q'}, 17):
    with pytest.raises(ValueError):
      q.pauli_rot(bad, 0.3)
    with pytest.raises(ValueError):
      q.apply_pauli(bad)
    with pytest.raises(ValueError):
      q.pauli_project(bad)
    for method in (q.evolve, q.imaginary_time):
      with pytest.raises(ValueError):
        method([(1.0, bad)], 0.5)
  for method in (q.evolve, q.imaginary_time):
    with pytest.raises(ValueError):
      method([1.0], 0.5)
    with pytest.raises(ValueError, match='real coefficients'):
      method([(1j, 'ZIII')], 0.5)
    for steps in (0, -1, 1.5, True):
      with pytest.raises(ValueError, match='steps'):
        method([(1.0, 'ZIII')], 0.5, steps=steps)
  with pytest.raises(ValueError, match='order'):
    q.evolve([(1.0, 'ZIII')], 0.5, order=3)
  for ev in (0, 2, 0.5, 1j):
    with pytest.raises(ValueError, match='eigenvalue'):
      q.pauli_project('ZIII', ev)
  assert np.array_equal(np.asarray(q.psi), psi)
