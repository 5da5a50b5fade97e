"""The full-state reference of tests/torch_reference.py checked on the host, before the GPU tests lean on it:
apply_stream against the C oracle, qft_closed_form against workloads.qft_analytic (up to 40 qubits, where an
overflowing phase product would show), and the comparator's sensitivity to the faults it exists to catch."""
import math

import numpy as np
import pytest
import torch

from qcc_amd import gates, workloads
from tests import torch_reference as tr
from tests.oracle_lib import NO_CTL


def _rand_unitary(rng):
  m = rng.standard_normal((2, 2)) + 1j * rng.standard_normal((2, 2))
  q, r = np.linalg.qr(m)
  return q * (np.diag(r) / np.abs(np.diag(r)))


def _random_stream(rng, n, ngates):
  ops, gs = [], []
  for _ in range(ngates):
    kind = rng.random()
    t = int(rng.integers(0, n))
    if kind < 0.2:
      g = np.diag([np.exp(1j * rng.uniform(0, 6.28)), np.exp(1j * rng.uniform(0, 6.28))])   # diagonal shortcut
    elif kind < 0.3:
      g = gates.pauli_x()
    else:
      g = _rand_unitary(rng)
    if n > 1 and rng.random() < 0.45:
      c = int((t + 1 + rng.integers(0, n - 1)) % n)
      ops.append((c, t))
    else:
      ops.append((NO_CTL, t))
    gs.append(np.asarray(g, dtype=np.complex128).reshape(4))
  return np.array(ops, dtype=np.int32).reshape(-1, 2), np.array(gs).view(np.float64).reshape(-1, 8)


def _rand_state(rng, n):
  p = rng.standard_normal(1 << n) + 1j * rng.standard_normal(1 << n)
  return p / np.linalg.norm(p)


def _both(oracle, psi0, n, ops, g8, chunk=tr.PAIR_CHUNK):
  want = psi0.copy()
  oracle.run_stream(want, n, ops, g8)
  got = tr.apply_stream(torch.from_numpy(psi0.copy()), n, ops, g8, chunk=chunk).numpy()
  return got, want


@pytest.mark.parametrize('n', list(range(1, 13)))
def test_apply_stream_random_streams_vs_oracle(oracle, n):
  rng = np.random.default_rng(100 + n)
  ops, g8 = _random_stream(rng, n, 40 + 10 * n)
  psi0 = _rand_state(rng, n)
  got, want = _both(oracle, psi0, n, ops, g8)
  assert np.max(np.abs(got - want)) <= 1e-13
  # the chunked path (blocks smaller than a gate's pair set) gives the same state
  got_small, _ = _both(oracle, psi0, n, ops, g8, chunk=2)
  assert np.max(np.abs(got_small - want)) <= 1e-13


def test_apply_stream_every_ordered_pair_n6(oracle):
  n = 6
  rng = np.random.default_rng(6)
  for c in range(n):
    for t in range(n):
      if c == t:
        continue
      u = _rand_unitary(rng)
      ops = np.array([(c, t)], dtype=np.int32)
      g8 = np.asarray(u, dtype=np.complex128).reshape(1, 4).view(np.float64)
      psi0 = _rand_state(rng, n)
      for chunk in (tr.PAIR_CHUNK, 1):
        got, want = _both(oracle, psi0, n, ops, g8, chunk=chunk)
        assert np.max(np.abs(got - want)) <= 1e-13, (c, t, chunk)
      assert np.max(np.abs(got - psi0)) > 1e-3, (c, t)        # the gate did something


def test_apply_stream_control_equal_to_target_is_the_oracles_no_op(oracle):
  n = 5
  psi0 = _rand_state(np.random.default_rng(5), n)
  ops = np.array([(2, 2)], dtype=np.int32)
  g8 = np.asarray(_rand_unitary(np.random.default_rng(1)), dtype=np.complex128).reshape(1, 4).view(np.float64)
  got, want = _both(oracle, psi0, n, ops, g8)
  assert np.array_equal(got, want) and np.array_equal(got, psi0)


@pytest.mark.parametrize('ctl', [-1, -7, 6, 40])
def test_apply_stream_rejects_out_of_range_controls(ctl):
  psi = torch.zeros(1 << 6, dtype=torch.complex128)
  with pytest.raises(ValueError):
    tr.apply_stream(psi, 6, np.array([(ctl, 1)], dtype=np.int32), np.zeros((1, 8)))
  with pytest.raises(ValueError):
    tr.apply_stream(psi, 6, np.array([(NO_CTL, 6)], dtype=np.int32), np.zeros((1, 8)))


@pytest.mark.parametrize('name', ['qft', 'supremacy', 'grover'])
@pytest.mark.parametrize('n', [6, 9, 12])
def test_apply_stream_workloads_vs_oracle(oracle, name, n):
  if name == 'qft':
    ops, g8 = workloads.qft_stream(range(n)).arrays()
    init = 0xB5A & ((1 << n) - 1)
  elif name == 'supremacy':
    ops, g8 = workloads.supremacy_stream(n, 12, seed=n).arrays()
    init = 0
  else:
    nb = n // 2
    ops, g8 = workloads.grover_stream(nb, [1, 0] * (nb // 2) + [1] * (nb % 2), iterations=1).arrays()
    init = workloads.grover_initial_index(nb)
  psi0 = np.zeros(1 << n, dtype=np.complex128)
  psi0[init] = 1
  got, want = _both(oracle, psi0, n, ops, g8)
  assert np.max(np.abs(got - want)) <= 1e-13
  if name == 'qft':
    closed = tr.qft_closed_form(n, init, 0, 1 << n).numpy()
    assert np.max(np.abs(got - closed)) <= 1e-13


@pytest.mark.parametrize('n', [1, 2, 7, 16, 30, 31, 33, 37, 40])
def test_qft_closed_form_matches_qft_analytic(n):
  rng = np.random.default_rng(n)
  top = (1 << n) - 1
  for x in sorted({top, 0, 1, int(rng.integers(0, top + 1)), 0x1B2CB9A5E3 & top}):
    idx = sorted({0, top, 1 << (n - 1), top - 1} | {int(v) for v in rng.integers(0, top + 1, size=200)})
    want = workloads.qft_analytic(n, x, idx)
    got = np.array([complex(tr.qft_closed_form(n, x, i, 1)[0]) for i in idx[:8]])
    assert np.max(np.abs(got - want[:8])) <= 4e-16 * 2.0 ** (-n / 2), (n, x)
    # a contiguous run through the same code path as the GPU tests, ending at 2^n - 1
    cnt = min(1 << n, 4096)
    run = tr.qft_closed_form(n, x, (1 << n) - cnt, cnt).numpy()
    want_run = workloads.qft_analytic(n, x, np.arange((1 << n) - cnt, 1 << n, dtype=np.uint64))
    assert np.max(np.abs(run - want_run)) <= 4e-16 * 2.0 ** (-n / 2), (n, x)


def test_qft_closed_form_phase_numerator_is_exact_at_40_qubits():
  """k = 2^40 - 1, x with every bit set: bitrev(x) k ~ 2^80 -- (bitrev(x) k mod 2^40) must come out exactly."""
  n = 40
  x = (1 << n) - 1
  k = (1 << n) - 1
  num = (x * k) % (1 << n)                   # = 1
  a = complex(tr.qft_closed_form(n, x, k, 1)[0])
  want = complex(math.cos(2 * math.pi * num / 2 ** n), math.sin(2 * math.pi * num / 2 ** n)) / 2 ** 20
  assert abs(a - want) <= 1e-22
  assert abs(np.angle(a) - 2 * math.pi * 2.0 ** -40) <= 1e-25      # the phase of numerator 1, not of a wrapped product


def _old_30q_samples():
  """The indices tests/test_gpu_parity.py::test_full_size_30q_properties read before this file existed."""
  n = 30
  idx = np.random.default_rng(30).integers(0, 1 << n, size=512)
  win = np.arange((1 << 29) + 12345, (1 << 29) + 12345 + 4096)
  return np.concatenate([idx, win])


def test_comparator_flags_two_swapped_blocks():
  """Two blocks of 2^9 amplitudes swapped (a misplaced tile): flagged by every metric of compare().  At 30 qubits the
  same fault at these positions lies between every amplitude the old sampled checks read.  (A QFT state is periodic in k
  with period 2^n / 2^v, 2^v the lowest set bit of bitrev(x): x's top bit is set here, so no swap of distinct blocks is
  invisible.)"""
  n, x, blk = 16, 0xDA3C, 1 << 9
  ref = lambda off, cnt: tr.qft_closed_form(n, x, off, cnt)      # noqa: E731
  good = ref(0, 1 << n)
  assert tr.compare_tensor(good, ref, chunk=1 << 12)['max_abs'] == 0.0
  bad = good.clone()
  i, j = 37 * blk, 101 * blk
  bad[i:i + blk], bad[j:j + blk] = good[j:j + blk].clone(), good[i:i + blk].clone()
  r = tr.compare_tensor(bad, ref, chunk=1 << 12)
  assert r['max_abs'] > 1e-10 and r['rel_l2'] > 1e-12
  assert i <= r['worst'] < i + blk or j <= r['worst'] < j + blk
  # scaled to 30 qubits: the same two blocks at 2^14 times the offsets hold none of the old test's sampled indices
  s = np.sort(_old_30q_samples())
  for lo in (i << 14, j << 14):
    assert np.searchsorted(s, lo) == np.searchsorted(s, lo + blk)


def test_comparator_flags_a_1e9_rad_error_in_one_cu1_angle():
  """One CU1 angle of the QFT off by 1e-9 rad: the normwise metric (bound 1e-12) flags it at any size -- a fixed fraction
  of the amplitudes carry it -- while max |got - ref| falls with the amplitude modulus 2^(-n/2): 4e-12 here, 3e-14 at 30
  qubits, far under the 1e-10 max-abs bound that alone would have passed it.  (The mutated stream is the one a reviewer
  can send to the engine instead: the full-state GPU tests then fail on the normwise bound.)"""
  n, x = 16, 0x5A3C
  ops, g8 = workloads.qft_stream(range(n)).arrays()
  ref = lambda off, cnt: tr.qft_closed_form(n, x, off, cnt)      # noqa: E731
  good = tr.apply_stream(tr.basis_state(n, x, 'cpu'), n, ops, g8)
  r0 = tr.compare_tensor(good, ref, chunk=1 << 12)
  assert r0['max_abs'] <= 1e-10 * 2.0 ** -8 and r0['rel_l2'] <= 1e-14
  k = next(i for i, (c, _t) in enumerate(ops) if c != NO_CTL and c < n // 2)
  g = g8.copy().view(np.complex128)
  g[k] = gates.u1(np.angle(g[k, 3]) + 1e-9).reshape(4)
  bad = tr.apply_stream(tr.basis_state(n, x, 'cpu'), n, ops, g.view(np.float64))
  r = tr.compare_tensor(bad, ref, chunk=1 << 12)
  assert r['rel_l2'] > 1e-12 * 100                 # 5e-10: flagged with room to spare
  assert 2e-10 < r['rel_l2'] < 1e-9                # a fixed fraction of the state off by ~1e-9 rad: size-independent
  assert r['max_abs'] < 1e-10                      # max-abs alone misses it already at 16 qubits ...
  assert r['max_abs'] * 2.0 ** ((n - 30) / 2) < 1e-10 / 1000      # ... and by far at 30 (same angle, modulus 2^-15)
