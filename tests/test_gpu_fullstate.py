"""Every amplitude of the 30-33 qubit runs against an independent reference (tests/torch_reference.py), on the device.

The sampled checks of tests/test_gpu_fullsize.py and test_gpu_parity.py read ~3e-5 of these states, and an absolute
bound of 1e-10 against amplitudes of modulus 2^-15 lets a relative error of 3e-6 through.  Here the whole state is
compared, in HBM, against
  * the QFT's closed form (no gate stream involved), or
  * the gate stream applied by plain torch ops on the GPU (apply_stream; checked against the C oracle first, below),
with two bounds for complex128 -- max |got - ref| <= 1e-10 (BASELINE.json north star) and |got - ref|_2 / |ref|_2 <=
1e-12 -- and for complex64 normwise <= 1e-5 and per amplitude |got - ref| <= 3e-5 2^(-n/2) + 3e-5 |ref|.

The readers are checked first, while the layout the last flush left is still live (qh_device_ptr and qh_download both
canonicalise): norm2, prob_bit_value for every bit and value, argmax (supremacy: from the last sweep's tile maxima) and
three single amplitudes.  Every test prints one line with the measured errors, whether the bit map was permuted, and the
torch memory it used."""
import ctypes
import gc
import time

import numpy as np
import pytest
import torch

from qcc_amd import device, native, workloads
from tests import torch_reference as tr

pytestmark = pytest.mark.gpu
DEV = 'cuda'
GiB = 1 << 30
QFT_X = 0x1B2CB9A5E3
PERMUTED = {}


@pytest.fixture(scope='module', autouse=True)
def _torch_memory_is_returned():
  """test_gpu_fullsize.py runs next: its Grover-34 state needs 256 GiB of the device."""
  yield
  gc.collect()
  torch.cuda.empty_cache()
  assert torch.cuda.memory_reserved() == 0


@pytest.fixture(autouse=True)
def _free_torch_memory():
  gc.collect()
  torch.cuda.empty_cache()
  torch.cuda.reset_peak_memory_stats()
  yield
  gc.collect()
  torch.cuda.empty_cache()


def _bitmap(st):
  bm = (ctypes.c_int32 * st.nbits)()
  native.check(st.lib.qh_get_bitmap(st.h, bm))
  return list(bm)


def _amp_bound(n, bw):
  """(atol, rtol) per amplitude.  complex64: 3e-5 2^(-n/2) (the bound test_qft_fused_analytic holds at 27 qubits) plus
  3e-5 |ref| for states whose moduli spread; complex128: 1e-11 of the same scale (reported, and held by the readers)."""
  return (3e-5 * 2.0 ** (-n / 2), 3e-5) if bw == 64 else (1e-11 * 2.0 ** (-n / 2), 1e-11)


def _check_readers(st, ref_fn, n, bw, check_argmax):
  """Readers against the reference, in the layout the flush left (call before device_ptr / download)."""
  bm = _bitmap(st)
  permuted = bm != list(range(n))
  if check_argmax:                        # first: right behind the flush, from the last sweep's tile maxima
    idx, p = st.argmax()
  norm_ref, prob_ref, pmax = tr.ref_readers(ref_fn, n)
  tol = 1e-11 if bw == 128 else 1e-5
  assert abs(st.norm2() - norm_ref) <= tol
  worst_prob = 0.0
  for b in range(n):
    for v in (0, 1):
      worst_prob = max(worst_prob, abs(st.prob_bit(b, v) - prob_ref[b, v]))
  assert worst_prob <= tol, worst_prob
  if check_argmax:                        # (complex64: the probabilities of float amplitudes, ~1e-7 relative)
    rel = 1e-9 if bw == 128 else 1e-5
    r = complex(ref_fn(idx, 1)[0])
    p_at = r.real * r.real + r.imag * r.imag
    assert p_at >= pmax * (1 - rel), (idx, p_at, pmax)
    assert abs(p - pmax) <= rel * pmax, (p, pmax)
  atol, rtol = _amp_bound(n, bw)
  for i in (0, (1 << n) - 1, 1 << (n - 1)):
    want = complex(ref_fn(i, 1)[0])
    assert abs(complex(st.amplitude(i)) - want) <= atol + rtol * abs(want), (i, st.amplitude(i), want)
  return bm, permuted, worst_prob


def _assert_bounds(r, n, bw):
  if bw == 128:
    assert r['max_abs'] <= 1e-10, r
    assert r['rel_l2'] <= 1e-12, r
  else:
    assert r['rel_l2'] <= 1e-5, r
    assert r['bound_ratio'] <= 1.0, r


def _report(case, r, permuted, worst_prob, t0, extra=''):
  print(f'\n[fullstate] {case}: max_abs={r["max_abs"]:.3e} rel_l2={r["rel_l2"]:.3e} worst={r["worst"]} '
        f'amp_bound_ratio={r["bound_ratio"]:.3e} prob_bit_err={worst_prob:.2e} permuted={permuted} '
        f'torch_peak_alloc={torch.cuda.max_memory_allocated() / GiB:.2f}GiB '
        f'torch_peak_reserved={torch.cuda.max_memory_reserved() / GiB:.2f}GiB wall={time.perf_counter() - t0:.1f}s {extra}')


# ---- the reference itself on the device ------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [16, 20])
def test_apply_stream_on_the_gpu_matches_the_oracle(oracle, n):
  rng = np.random.default_rng(n)
  ops, gs = [], []
  for _ in range(200):
    t = int(rng.integers(0, n))
    m = rng.standard_normal((2, 2)) + 1j * rng.standard_normal((2, 2))
    q = np.linalg.qr(m)[0]
    if rng.random() < 0.4:
      ops.append((int((t + 1 + rng.integers(0, n - 1)) % n), t))
      gs.append(q if rng.random() < 0.5 else np.diag([1.0, np.exp(1j * rng.uniform(0, 6.28))]))
    else:
      ops.append((tr.NO_CTL, t))
      gs.append(q)
  ops = np.array(ops, dtype=np.int32)
  g8 = np.array([np.asarray(g, dtype=np.complex128).reshape(4) for g in gs]).view(np.float64).reshape(-1, 8)
  sops, sg8 = workloads.supremacy_stream(n, 20, seed=n).arrays()
  for o, g in ((ops, g8), (sops, sg8)):
    psi0 = rng.standard_normal(1 << n) + 1j * rng.standard_normal(1 << n)
    psi0 /= np.linalg.norm(psi0)
    want = psi0.copy()
    oracle.run_stream(want, n, o, g)
    got = tr.apply_stream(torch.from_numpy(psi0).to(DEV), n, o, g, chunk=1 << (n - 4))   # several blocks per gate
    assert float((got.cpu() - torch.from_numpy(want)).abs().max()) <= 1e-13
    del got


# ---- QFT: closed form ----------------------------------------------------------------------------------------------------
_QFT_CASES = [(30, 128, native.QH_FUSE_SWEEP), (30, 128, native.QH_FUSE_OFF), (30, 64, native.QH_FUSE_SWEEP),
              (31, 128, native.QH_FUSE_SWEEP), (31, 64, native.QH_FUSE_SWEEP), (33, 128, native.QH_FUSE_SWEEP)]


@pytest.mark.parametrize('n,bw,fusion', _QFT_CASES, ids=[f'{n}q-c{bw}-{"fused" if f else "off"}' for n, bw, f in _QFT_CASES])
def test_qft_full_state_closed_form(n, bw, fusion):
  """QFT of |x> against exp(2 pi i bitrev(x) k / 2^n) / 2^(n/2) at every k (31: indices cross 2^31, 33: 2^32).
  QFT-30 complex128 fused is also compared through qh_download, whose own canonicalisation runs then."""
  t0 = time.perf_counter()
  x = (QFT_X & ((1 << n) - 1)) | 1 << (n - 1)    # bitrev(x) odd: amplitude k and k + 2^m differ for every m < n
  ops, g8 = workloads.qft_stream(range(n)).arrays()
  ref_fn = lambda off, cnt: tr.qft_closed_form(n, x, off, cnt, DEV)      # noqa: E731
  try:
    st = device.DeviceState(n, bw, fusion=fusion)
  except native.QhError as e:
    if e.code == native.QH_ERR_NOMEM:
      pytest.skip(str(e))
    raise
  atol, rtol = _amp_bound(n, bw)
  with st:
    st.init_basis(x)
    st.run_stream(ops, g8)
    st.flush()
    sweeps = st.stats()['sweeps']
    _bm, permuted, worst_prob = _check_readers(st, ref_fn, n, bw, check_argmax=False)
    PERMUTED[f'qft{n}-c{bw}-{fusion}'] = permuted
    extra = ''
    if (n, bw, fusion) == (30, 128, native.QH_FUSE_SWEEP):
      rh = tr.compare_download(st, ref_fn, atol=atol, rtol=rtol)
      _assert_bounds(rh, n, bw)
      extra = f'download: max_abs={rh["max_abs"]:.3e} rel_l2={rh["rel_l2"]:.3e}'
    r = tr.compare(st, ref_fn, atol=atol, rtol=rtol)
  _report(f'qft{n} c{bw} fusion={fusion} sweeps={sweeps}', r, permuted, worst_prob, t0, extra)
  _assert_bounds(r, n, bw)
  limit = 2 * GiB if n >= 33 else 4 * GiB
  assert torch.cuda.max_memory_allocated() <= limit


# ---- supremacy: the stream through plain torch ops on the GPU ------------------------------------------------------------
_SUP_CASES = {0: [(128, native.QH_FUSE_SWEEP), (128, native.QH_FUSE_OFF), (64, native.QH_FUSE_SWEEP)],
              1: [(128, native.QH_FUSE_SWEEP)],
              2: [(128, native.QH_FUSE_SWEEP)]}


@pytest.mark.parametrize('seed', [0, 1, 2])
def test_supremacy30_full_state(seed, monkeypatch):
  """BASELINE config 3 (30 qubits, depth 20, SURVEY 8(d)'s seeds): the engine against apply_stream on the GPU, every
  amplitude; seed 0 also per-gate kernels and complex64 against the same reference."""
  n = 30
  monkeypatch.setenv('QH_PLAN_SEARCH_STREAMS', '6')      # (pinned as in test_gpu_fullsize.py, for the sweep counts)
  ops, g8 = workloads.supremacy_stream(n, 20, seed=seed).arrays()
  t0 = time.perf_counter()
  ref = tr.apply_stream(tr.basis_state(n, 0, DEV), n, ops, g8)
  torch.cuda.synchronize()
  t_ref = time.perf_counter() - t0
  ref_fn = lambda off, cnt: ref[off:off + cnt]      # noqa: E731
  for bw, fusion in _SUP_CASES[seed]:
    t0 = time.perf_counter()
    atol, rtol = _amp_bound(n, bw)
    with device.DeviceState(n, bw, fusion=fusion) as st:
      st.init_basis(0)
      st.run_stream(ops, g8)
      st.flush()
      sweeps = st.stats()['sweeps']
      if fusion == native.QH_FUSE_SWEEP and bw == 128:
        assert sweeps == 4
      _bm, permuted, worst_prob = _check_readers(st, ref_fn, n, bw, check_argmax=True)
      PERMUTED[f'sup{seed}-c{bw}-{fusion}'] = permuted
      r = tr.compare(st, ref_fn, atol=atol, rtol=rtol)
    _report(f'supremacy30 seed={seed} c{bw} fusion={fusion} sweeps={sweeps}', r, permuted, worst_prob, t0,
            f'(reference {t_ref:.1f}s)')
    _assert_bounds(r, n, bw)
  assert float(ref[:1 << 20].abs().max()) > 1e-6           # a dense, non-trivial state
  del ref, ref_fn
  assert torch.cuda.max_memory_allocated() <= 20 * GiB


def test_a_full_state_case_ran_in_a_permuted_layout():
  """The relayout sweeps and the canonicalisation behind device_ptr / download were really exercised above."""
  if not PERMUTED:
    pytest.skip('no full-state case ran in this selection')
  print(f'\n[fullstate] permuted bit maps: {PERMUTED}')
  assert any(PERMUTED.values()), PERMUTED
