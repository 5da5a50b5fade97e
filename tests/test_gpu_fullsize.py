"""BASELINE.json configs 3 and 4 at full size on one MI355X.

The reference cannot run these sizes (32-bit indices stop at 30 qubits and a
30-qubit gate takes seconds on its single thread), so parity rests on
size-independent properties plus the chain of trust
GPU == oracle == reference established at <= 22 qubits:
  * two independent GPU implementations (per-gate kernels vs fused sweeps) agree
    amplitude by amplitude on sampled windows; the same circuit family at 28 qubits
    against the CPU oracle itself (all host cores, seconds);
  * circuit followed by its inverse returns the basis state; norm stays 1;
  * closed forms: the Grover 4-amplitude recurrence.
Every amplitude of the 30-33 qubit QFT and of supremacy-30 against an independent reference: test_gpu_fullstate.py."""
import math

import numpy as np
import pytest

from qcc_amd import device, native, workloads

pytestmark = pytest.mark.gpu


def _inverse(ops, g8):
  inv_ops = ops[::-1].copy()
  c = g8[::-1].copy().reshape(-1, 4, 2)
  z = (c[..., 0] + 1j * c[..., 1]).reshape(-1, 2, 2)
  zi = np.conj(z.transpose(0, 2, 1)).reshape(-1, 4)
  return inv_ops, np.ascontiguousarray(zi).view(np.float64).reshape(-1, 8)


@pytest.mark.parametrize('seed', [0, 1, 2, 3, 4, 5])
def test_config3_supremacy_30q_depth20(seed, monkeypatch):
  """BASELINE config 3 at full size, SURVEY 8(d)'s seeds 0, 1, 2 (the bench line carries all three since round 6) and three
  more: the fused sweeps (4 4 4 4 4 5 of them since the level search, planner.h search_levels: the minimum under 13-bit
  tiles for each) against the per-gate kernels on sampled windows at 1e-10, and the inverse circuit through the fused path
  back to |0>."""
  n = 30
  monkeypatch.setenv('QH_PLAN_SEARCH_STREAMS', '6')      # (the default follows the host's usable cores: pinned for the sweep counts below)
  ops, g8 = workloads.supremacy_stream(n, 20, seed=seed).arrays()
  if seed == 0:
    assert len(ops) == 342                    # 30 H, 117 V/Yroot, 80 T, 115 CZ
  rng = np.random.default_rng(3)
  offs = [int(o) for o in rng.integers(0, (1 << n) - 4096, size=6)] + [0, (1 << n) - 4096]
  windows = {}
  for fusion in (native.QH_FUSE_SWEEP, native.QH_FUSE_OFF):
    with device.DeviceState(n, 128, fusion=fusion) as st:
      st.init_basis(0)
      st.run_stream(ops, g8)
      assert abs(st.norm2() - 1.0) < 1e-10
      windows[fusion] = np.concatenate([st.download(o, 4096) for o in offs])
      if fusion == native.QH_FUSE_SWEEP:
        assert st.stats()['sweeps'] == (4, 4, 4, 4, 4, 5)[seed]
        st.run_stream(*_inverse(ops, g8))
        i, p = st.argmax()
        assert i == 0 and abs(p - 1.0) < 1e-9
  a, b = windows[native.QH_FUSE_SWEEP], windows[native.QH_FUSE_OFF]
  assert np.max(np.abs(a)) > 1e-6             # a dense, non-trivial state
  assert np.max(np.abs(a - b)) <= 1e-10


@pytest.mark.parametrize('seed', [0, 1])
def test_config3_supremacy_28q_against_the_oracle(seed):
  """(seed 1: VERDICT r05 #4 -- SURVEY 8(d) names seeds 0, 1, 2; since round 6 these instances plan with two wave bits, 13-bit
  tiles found by the level search, 4 sweeps.)  Config 3's circuit family against the CPU ORACLE at a size the host finishes in seconds (VERDICT r2, next #6:
  the 30-qubit run above is GPU-vs-GPU plus inverse; the largest oracle comparison of a random circuit was 20
  qubits).  supremacy.py:123-158,208-253 at 28 qubits, depth 20, random.seed(0): every gate through
  oracle/xgates_oracle.c's restatement of xgates.cc:23-67 on all host cores (2^28 amplitudes, 4 GiB), the fused
  GPU result compared amplitude by amplitude on 64 windows of 2^14 (plus the ends) at 1e-10."""
  import time
  from tests import oracle_lib
  n = 28
  ops, g8 = workloads.supremacy_stream(n, 20, seed=seed).arrays()
  assert len(ops) > 300
  omp = oracle_lib.load(omp=True)
  want = np.empty(1 << n, dtype=np.complex128)
  omp.init_basis_mt(want, n, 0)
  t0 = time.perf_counter()
  omp.run_stream_mt(want, n, ops, g8)
  t_cpu = time.perf_counter() - t0
  rng = np.random.default_rng(28)
  width = 1 << 14
  offs = [0, (1 << n) - width] + [int(o) for o in rng.integers(0, (1 << n) - width, size=64)]
  with device.DeviceState(n, 128, fusion=native.QH_FUSE_SWEEP) as st:
    st.init_basis(0)
    st.run_stream(ops, g8)
    st.flush()
    sweeps = st.stats()['sweeps']
    assert abs(st.norm2() - 1.0) < 1e-10
    got = [st.download(o, width) for o in offs]
  worst = max(float(np.max(np.abs(g - want[o:o + width]))) for g, o in zip(got, offs))
  print(f'supremacy-28 seed {seed} ({len(ops)} gates): oracle {t_cpu:.1f} s on the host cores, {sweeps} sweeps on the GPU, max |gpu - oracle| = {worst:.2e}')
  assert float(np.max(np.abs(want[:width]))) > 1e-7          # dense state
  assert worst <= 1e-10


def test_config4_grover_34q_one_iteration():
  nb = 17
  n = 2 * nb
  marked = [1, 0] * 8 + [1]
  ops, g8 = workloads.grover_stream(nb, marked, iterations=1).arrays()
  try:
    st = device.DeviceState(n, 128, fusion=native.QH_FUSE_SWEEP)
  except native.QhError as e:
    if e.code == native.QH_ERR_NOMEM:
      pytest.skip(f'cannot allocate the 256 GiB state on this box: {e}')
    raise
  with st:
    st.init_basis(workloads.grover_initial_index(nb))
    st.run_stream(ops, g8)
    assert abs(st.norm2() - 1.0) < 1e-9
    cm0, cm1, cu0, cu1 = workloads.grover_recurrence(nb, 1)
    x = int(''.join(map(str, marked)), 2)
    anc = 1 << (nb - 1)
    rng = np.random.default_rng(4)
    others = [int(v) for v in rng.integers(0, 1 << nb, size=8) if int(v) != x]
    for xx, (c0, c1) in [(x, (cm0, cm1))] + [(o, (cu0, cu1)) for o in others]:
      assert abs(st.amplitude((xx << nb) | 0) - c0) < 1e-12
      assert abs(st.amplitude((xx << nb) | anc) - c1) < 1e-12
      assert abs(st.amplitude((xx << nb) | 1)) < 1e-14        # aux != 0 stays empty
      assert abs(st.amplitude((xx << nb) | anc | 5)) < 1e-14
    s = st.stats()
    assert s['gates_submitted'] == len(ops)


@pytest.mark.parametrize('n,bw', [(31, 128), (32, 128), (31, 64), (33, 128)])
def test_qft_between_the_configs_closed_form(n, bw):
  """31 / 32 / 33-qubit QFT on one GPU (plans with two wave bits, relayout between two 32-128 GiB buffers,
  64-bit indices past the reference's 30-qubit limit): closed form on sampled amplitudes, norm, and the
  inverse circuit on the re-laid-out state returns the basis state.  (Every amplitude of 31 and 33:
  tests/test_gpu_fullstate.py.)"""
  ops, g8 = workloads.qft_stream(range(n)).arrays()
  x = 0x1B2CB9A5E3 & ((1 << n) - 1)
  try:
    st = device.DeviceState(n, bw, fusion=native.QH_FUSE_SWEEP)
  except native.QhError as e:
    if e.code == native.QH_ERR_NOMEM:
      pytest.skip(str(e))
    raise
  tol = (1e-12 if bw == 128 else 3e-5) * 2.0 ** (-n / 2)     # relative to the amplitude modulus, as test_qft_fused_analytic
  with st:
    st.init_basis(x)
    st.run_stream(ops, g8)
    assert abs(st.norm2() - 1.0) < (1e-9 if bw == 128 else 1e-4)
    rng = np.random.default_rng(n)
    idx = [0, (1 << n) - 1] + [int(v) for v in rng.integers(0, 1 << n, size=40)]
    want = workloads.qft_analytic(n, x, idx)
    got = np.array([st.amplitude(i) for i in idx])
    assert np.max(np.abs(got - want)) <= tol
    st.run_stream(*_inverse(ops, g8))
    i, p = st.argmax()
    assert i == x and abs(p - 1.0) < (1e-9 if bw == 128 else 1e-4)
    assert abs(st.amplitude(x) - 1.0) < (1e-9 if bw == 128 else 1e-4)
