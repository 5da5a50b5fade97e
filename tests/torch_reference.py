"""Plain full-state reference for the 30-33 qubit checks.  TEST-ONLY.

Everything here is written with ordinary torch tensor ops on views, so it runs the same on the CPU and on the GPU and
shares no code with the engine: neither qcc_amd's kernels nor the C oracle produce a reference value here.

  apply_stream      the project's (ctl | NO_CTL, tgt) / 8-double gate streams on a complex128 tensor, with the semantics of
                    oracle/xgates_oracle.c (qubit q is index bit nbits-1-q; both new values of a pair from the old ones)
  qft_closed_form   amplitudes of the QFT of a basis state from the closed form, no gate stream involved
  compare           every amplitude of an engine state against a reference, chunk by chunk on the device
  compare_download  the same through qh_download (the host path), for the one case that covers its canonicalisation
  ref_readers       what the engine's readers (norm2, prob_bit_value, argmax) must return, summed from the reference

Nothing under qcc_amd/ may import this module.
"""
import ctypes
import itertools
import math

import numpy as np
import torch

NO_CTL = -(2 ** 31)
PAIR_CHUNK = 1 << 25          # pairs per step of apply_stream: one 512 MiB temporary for a complex128 state
CMP_CHUNK = 1 << 24           # amplitudes per step of compare / ref_readers


# ---- apply_stream -------------------------------------------------------------------------------------------------------
def _blocks(shape, limit):
  """Index tuples that cut a tensor of `shape` into blocks of at most `limit` elements (every extent a power of two)."""
  d, suffix = len(shape), 1
  while d > 0 and suffix * shape[d - 1] <= limit:
    d -= 1
    suffix *= shape[d]
  if d == 0:
    yield ()
    return
  step = max(1, limit // suffix)
  for lead in itertools.product(*(range(s) for s in shape[:d - 1])):
    for s0 in range(0, shape[d - 1], step):
      yield lead + (slice(s0, s0 + step),)


def _pair_views(psi, nbits, c, p):
  """(a, b): views of the amplitudes with target bit p = 0 and = 1 (and control bit c = 1 when c is not None)."""
  if c is None:
    v = psi.view(1 << (nbits - 1 - p), 2, 1 << p)
    return v[:, 0], v[:, 1]
  if c > p:
    v = psi.view(1 << (nbits - 1 - c), 2, 1 << (c - p - 1), 2, 1 << p)[:, 1]
    return v[:, :, 0], v[:, :, 1]
  v = psi.view(1 << (nbits - 1 - p), 2, 1 << (p - c - 1), 2, 1 << c)[:, :, :, 1]
  return v[:, 0], v[:, 1]


def apply_gate(psi, nbits, ctl, tgt, g, chunk=PAIR_CHUNK):
  """One gate, in place: g = (g0, g1, g2, g3) row-major; ctl = NO_CTL or a qubit number."""
  if not 0 <= tgt < nbits:
    raise ValueError(f'target qubit {tgt} out of range for {nbits} qubits')
  if ctl != NO_CTL and not 0 <= ctl < nbits:
    raise ValueError(f'control qubit {ctl} out of range for {nbits} qubits (out-of-range controls: the C oracle)')
  p = nbits - 1 - tgt
  c = None if ctl == NO_CTL else nbits - 1 - ctl
  if c == p:                     # xgates_oracle.c: the control is read on the pair's first index, whose bit p is 0
    return
  g0, g1, g2, g3 = (complex(v) for v in g)
  a_all, b_all = _pair_views(psi, nbits, c, p)
  for ix in _blocks(tuple(a_all.shape), chunk):
    a, b = a_all[ix], b_all[ix]
    if g1 == 0 and g2 == 0:      # diagonal: the off-diagonal products are exact zeros
      if g0 != 1:
        a.mul_(g0)
      if g3 != 1:
        b.mul_(g3)
      continue
    t = torch.mul(a, g0).add_(b, alpha=g1)       # new a = g0 a + g1 b
    b.mul_(g3).add_(a, alpha=g2)                 # new b = g2 a + g3 b, a still old
    a.copy_(t)
    del t


def apply_stream(psi, nbits, ops, gates8, chunk=PAIR_CHUNK):
  """psi: complex128 tensor of 2^nbits amplitudes (any device), updated in place.  ops int32[G,2], gates8 float64[G,8]."""
  assert psi.dtype == torch.complex128 and psi.is_contiguous() and psi.numel() == 1 << nbits
  ops = np.asarray(ops, dtype=np.int64).reshape(-1, 2)
  g = np.ascontiguousarray(gates8, dtype=np.float64).reshape(-1, 8).view(np.complex128)
  assert len(ops) == len(g)
  for (ctl, tgt), gk in zip(ops, g):
    apply_gate(psi, nbits, int(ctl), int(tgt), gk, chunk)
  return psi


def basis_state(nbits, index, device):
  psi = torch.zeros(1 << nbits, dtype=torch.complex128, device=device)
  psi[index] = 1
  return psi


# ---- the QFT's closed form ----------------------------------------------------------------------------------------------
def bitrev(x, nbits):
  return int(format(x, f'0{nbits}b')[::-1], 2)


def qft_closed_form(nbits, x, offset, count, device='cpu'):
  """Amplitudes offset .. offset+count-1 of QFT|x>: exp(2 pi i (bitrev(x) k mod 2^n) / 2^n) / 2^(n/2).
  The phase numerator is exact: k = k1 2^20 + k0, every int64 product stays below 2^61 for n <= 40."""
  if not 1 <= nbits <= 40:
    raise ValueError('qft_closed_form: 1 <= nbits <= 40')
  mask = (1 << nbits) - 1
  xr = bitrev(x, nbits)
  k = torch.arange(offset, offset + count, dtype=torch.int64, device=device)
  k0, k1 = k & ((1 << 20) - 1), k >> 20                 # k1 < 2^20
  num = (((k1 * xr) & mask) << 20) + k0 * xr            # < 2^60 + 2^60
  num &= mask
  theta = num.to(torch.float64) * (2 * math.pi / (1 << nbits))     # = fl(2 pi) * num / 2^n, as qft_analytic
  s = math.sqrt(1 << nbits)
  return torch.complex(torch.cos(theta) / s, torch.sin(theta) / s)


# ---- comparison -----------------------------------------------------------------------------------------------------------
_hip = None


def _hip_runtime():
  """The HIP runtime already mapped (torch's, which the engine binds to when torch is imported first)."""
  global _hip
  if _hip is None:
    _hip = ctypes.CDLL('libamdhip64.so.7')
    _hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    _hip.hipMemcpy.restype = ctypes.c_int
  return _hip


class _Acc:
  """max |got - ref| (and where), sum |got - ref|^2, sum |ref|^2, max |got - ref| / (atol + rtol |ref|)."""

  def __init__(self, atol, rtol):
    self.atol, self.rtol = atol, rtol
    self.max_abs, self.worst, self.err2, self.ref2, self.ratio = 0.0, -1, 0.0, 0.0, 0.0

  def add(self, off, got, ref):
    d = (got.to(torch.complex128) - ref).abs()
    m, i = torch.max(d, 0)
    m = float(m)
    if m > self.max_abs or self.worst < 0:
      self.max_abs, self.worst = m, off + int(i)
    self.err2 += float(torch.sum(d * d))
    self.ref2 += float(torch.sum(ref.real * ref.real + ref.imag * ref.imag))
    if self.atol or self.rtol:
      self.ratio = max(self.ratio, float(torch.max(d / (self.atol + self.rtol * ref.abs()))))

  def result(self):
    return {'max_abs': self.max_abs, 'rel_l2': math.sqrt(self.err2 / self.ref2), 'worst': self.worst,
            'bound_ratio': self.ratio}


def compare(st, ref_fn, bw=None, chunk=CMP_CHUNK, atol=0.0, rtol=0.0):
  """Every amplitude of DeviceState st against ref_fn(offset, count) (complex128 tensor on the GPU), without copying the
  state to the host: the canonical pointer (qh_device_ptr), chunks copied device-to-device into one reused buffer.
  Returns max_abs, rel_l2 = |got - ref|_2 / |ref|_2, worst (logical index of max_abs) and bound_ratio =
  max |got - ref| / (atol + rtol |ref|) (0 unless a bound is given)."""
  bw = bw or st.bit_width
  total = 1 << st.nbits
  chunk = min(chunk, total)
  assert total % chunk == 0
  elem = 16 if bw == 128 else 8
  ptr = st.device_ptr                 # flushes, canonicalises; valid for the handle's life
  st.sync()
  hip = _hip_runtime()
  buf = torch.empty(chunk, dtype=torch.complex128 if bw == 128 else torch.complex64, device='cuda')
  acc = _Acc(atol, rtol)
  for off in range(0, total, chunk):
    torch.cuda.synchronize()          # the previous chunk's reads of buf are done
    rc = hip.hipMemcpy(ctypes.c_void_p(buf.data_ptr()), ctypes.c_void_p(ptr + off * elem), chunk * elem, 3)  # D2D
    assert rc == 0, f'hipMemcpy rc={rc}'
    acc.add(off, buf, ref_fn(off, chunk))
  del buf
  return acc.result()


def compare_tensor(got, ref_fn, chunk=CMP_CHUNK, atol=0.0, rtol=0.0):
  """compare() for a state that is already a tensor (the comparator's own tests, on host data)."""
  total = got.numel()
  chunk = min(chunk, total)
  acc = _Acc(atol, rtol)
  for off in range(0, total, chunk):
    acc.add(off, got[off:off + chunk], ref_fn(off, chunk))
  return acc.result()


def compare_download(st, ref_fn, chunk=CMP_CHUNK, atol=0.0, rtol=0.0):
  """compare() through DeviceState.download (qh_download: its own flush and canonicalisation) in chunks."""
  total = 1 << st.nbits
  chunk = min(chunk, total)
  host = np.empty(chunk, dtype=st.dtype)
  acc = _Acc(atol, rtol)
  for off in range(0, total, chunk):
    st.download(off, chunk, out=host)
    acc.add(off, torch.from_numpy(host).to('cuda'), ref_fn(off, chunk))
  return acc.result()


def ref_readers(ref_fn, nbits, chunk=CMP_CHUNK):
  """From the reference: norm2, prob[b][v] = sum |a|^2 over indices whose bit b is v, and the largest |a|^2."""
  total = 1 << nbits
  chunk = min(chunk, total)
  cb = chunk.bit_length() - 1
  norm = None
  prob = None
  pmax = 0.0
  for off in range(0, total, chunk):
    r = ref_fn(off, chunk)
    p = r.real * r.real + r.imag * r.imag
    del r
    s = p.sum()
    if prob is None:
      norm = torch.zeros((), dtype=torch.float64, device=p.device)
      prob = torch.zeros((nbits, 2), dtype=torch.float64, device=p.device)
    norm += s
    for b in range(nbits):
      if b < cb:
        prob[b] += p.view(-1, 2, 1 << b).sum(dim=(0, 2))
      else:
        prob[b, (off >> b) & 1] += s
    pmax = max(pmax, float(p.max()))
    del p
  return float(norm), prob.cpu().numpy(), pmax
