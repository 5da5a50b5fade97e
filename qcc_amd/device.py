"""DeviceState: a 2^n amplitude vector resident in MI355X HBM behind the C-ABI.

Host-side mirror of the native half of the reference boundary: the methods
apply1/applyc take the same arguments, in the same order and meaning, as
State.apply1 / State.applyc (src/lib/state.py:80,102) and the libxgates entry
points (src/lib/xgates.cc:89-145): reference (big-endian) qubit numbers and a
2x2 (or flattened) complex gate.
"""
import ctypes

import numpy as np

from qcc_amd import gates as _gates
from qcc_amd import native

_dp = ctypes.POINTER(ctypes.c_double)
MAX_MARGINAL_BITS = 16     # qh_marginal: k <= 16
MAX_DENSITY_BITS = native.QH_DENSITY_MAX_BITS     # qh_reduced_density: k <= 8


def _g8(gate):
  g = _gates.as8(gate)
  return g, g.ctypes.data_as(_dp)


def merge_factors(factors, table_bits=12, max_factors=32):
  """Adjacent factors are merged on the host while that is cheap (basis with basis;
  tables up to 2^table_bits amplitudes), so that the device sees few factors."""
  out = []
  for n, x in factors:
    n = int(n)
    if n == 0:
      continue
    is_int = isinstance(x, (int, np.integer))
    if out:
      pn, px = out[-1]
      p_int = isinstance(px, (int, np.integer))
      if is_int and p_int and pn + n <= 63:
        out[-1] = (pn + n, (int(px) << n) | int(x))
        continue
      if not (is_int and p_int) and pn + n <= table_bits:
        def table(m, v):
          if isinstance(v, (int, np.integer)):
            t = np.zeros(1 << m, dtype=np.complex128)
            t[int(v)] = 1
            return t
          return np.asarray(v, dtype=np.complex128).reshape(-1)
        out[-1] = (pn + n, np.kron(table(pn, px), table(n, x)))
        continue
    out.append((n, int(x) if is_int else np.asarray(x, dtype=np.complex128).reshape(-1)))
  while len(out) > max_factors:      # pathological: many large tables; merge the smallest neighbours
    sizes = [out[i][0] + out[i + 1][0] for i in range(len(out) - 1)]
    i = int(np.argmin(sizes))
    (n0, x0), (n1, x1) = out[i], out[i + 1]
    def tab(m, v):
      if isinstance(v, (int, np.integer)):
        t = np.zeros(1 << m, dtype=np.complex128)
        t[int(v)] = 1
        return t
      return v
    out[i:i + 2] = [(n0 + n1, np.kron(tab(n0, x0), tab(n1, x1)))]
  return out


class DeviceState:
  """Owns a qh_handle.  complex128 (bit_width=128) or complex64 (64)."""

  def __init__(self, nbits, bit_width=128, device=0, fusion=native.QH_FUSE_OFF, *,
               device_ptr=None, stream=None, host_mapped=False, dry=False):
    self.lib = native.load()
    self.nbits = int(nbits)
    self.bit_width = int(bit_width)
    self.dtype = np.complex128 if bit_width == 128 else np.complex64
    h = ctypes.c_void_p()
    if dry:        # planner-only handle (qh_create_dry): gates queue, plans and exchange geometry can be inspected, no device
      native.check(self.lib.qh_create_dry(self.nbits, self.bit_width, ctypes.byref(h)))
    elif host_mapped:
      native.check(self.lib.qh_create_host_mapped(self.nbits, self.bit_width, device, ctypes.byref(h)))
    elif device_ptr is None:
      rc = self.lib.qh_create(self.nbits, self.bit_width, device, ctypes.byref(h))
      if rc == native.QH_ERR_NOMEM:
        # device states parked by finished circuits (qcc_amd.lib.backend's pool) may be in the way: free them, try again
        from qcc_amd.lib import backend  # pylint: disable=import-outside-toplevel
        backend.drop_device_pool()
        rc = self.lib.qh_create(self.nbits, self.bit_width, device, ctypes.byref(h))
      native.check(rc)
    else:
      native.check(self.lib.qh_attach(self.nbits, self.bit_width, device,
                                      ctypes.c_void_p(device_ptr),
                                      ctypes.c_void_p(stream or 0), ctypes.byref(h)))
    self.h = h
    self.nbits_global = self.nbits
    if fusion != native.QH_FUSE_OFF:
      self.set_fusion(fusion)

  # -- lifetime ---------------------------------------------------------------
  def close(self):
    if getattr(self, 'h', None):
      self.lib.qh_destroy(self.h)
      self.h = None

  def __del__(self):
    # A state parked in qcc_amd.lib.backend's pool belongs to the pool: when a circuit and its state are collected in one
    # pass of the cycle collector, BOTH finalizers run -- the circuit's parks the state (and so resurrects it), this one must
    # then leave the handle alone.  The pool closes what it evicts or drops explicitly.
    if getattr(self, '_parked', False):
      return
    try:
      self.close()
    except Exception:  # pylint: disable=broad-except
      pass

  def __enter__(self):
    return self

  def __exit__(self, *a):
    self.close()

  # -- configuration ------------------------------------------------------------
  def set_fusion(self, level):
    native.check(self.lib.qh_set_fusion(self.h, int(level)))

  def set_relayout(self, on):
    """Relayout sweeps on/off (qh_set_relayout); returns the resulting mode."""
    actual = ctypes.c_int(0)
    native.check(self.lib.qh_set_relayout(self.h, 1 if on else 0, ctypes.byref(actual)))
    return bool(actual.value)

  def set_shard(self, nbits_global, shard_index):
    native.check(self.lib.qh_set_shard(self.h, int(nbits_global), int(shard_index)))
    self.nbits_global = int(nbits_global)

  def host_array(self):
    """NumPy view of a host-mapped state (qh_create_host_mapped): the very memory the GPU works on.
    Call sync() before reading."""
    p = ctypes.c_void_p()
    native.check(self.lib.qh_host_ptr(self.h, ctypes.byref(p)))
    if not p.value:
      raise ValueError('this state lives in HBM (create it with host_mapped=True)')
    real = ctypes.c_double if self.bit_width == 128 else ctypes.c_float
    flat = np.ctypeslib.as_array(ctypes.cast(p, ctypes.POINTER(real)), shape=(2 << self.nbits,))
    return flat.view(self.dtype)

  @property
  def device_ptr(self):
    p = ctypes.c_void_p()
    native.check(self.lib.qh_device_ptr(self.h, ctypes.byref(p)))
    return p.value

  # -- initialisation / IO ------------------------------------------------------
  def init_basis(self, index=0):
    native.check(self.lib.qh_init_basis(self.h, int(index)))

  def init_product(self, factors):
    """State := f_0 (x) f_1 (x) ... built on the device.  factors: [(nqubits, x)], x an
    int (basis state |x>) or 2^nqubits amplitudes; f_0 holds the most significant qubits."""
    factors = merge_factors(factors)
    k = len(factors)
    nq = (ctypes.c_int32 * k)(*[int(f[0]) for f in factors])
    basis = (ctypes.c_uint64 * k)()
    ptrs = (ctypes.c_void_p * k)()
    keep = []
    for j, (n, x) in enumerate(factors):
      if isinstance(x, (int, np.integer)):
        basis[j] = int(x)
      else:
        a = np.ascontiguousarray(x, dtype=np.complex128).reshape(-1)
        if a.size != 1 << n:
          raise ValueError(f'factor {j}: {a.size} amplitudes for {n} qubits')
        keep.append(a)
        ptrs[j] = a.ctypes.data
    native.check(self.lib.qh_init_product(self.h, k, nq, ptrs, basis))

  def upload(self, host, offset=0):
    a = np.ascontiguousarray(host, dtype=self.dtype)
    native.check(self.lib.qh_upload(self.h, a.ctypes.data, int(offset), a.size))

  def download(self, offset=0, count=None, out=None):
    count = (1 << self.nbits) - offset if count is None else count
    if out is None:
      out = np.empty(count, dtype=self.dtype)
    assert out.dtype == self.dtype and out.flags.c_contiguous and out.size >= count
    native.check(self.lib.qh_download(self.h, out.ctypes.data, int(offset), int(count)))
    return out

  # -- the hot path ---------------------------------------------------------------
  def apply1(self, gate, index):
    _keep, p = _g8(gate)
    native.check(self.lib.qh_apply1(self.h, int(index), p))

  def applyc(self, gate, control, target):
    _keep, p = _g8(gate)
    native.check(self.lib.qh_applyc(self.h, int(control), int(target), p))

  def apply_bits(self, ctl_mask, tgt_bit, gate):
    _keep, p = _g8(gate)
    native.check(self.lib.qh_apply_bits(self.h, int(ctl_mask), int(tgt_bit), p))

  def apply_matrix(self, matrix, bits, ctl_mask=0):
    """Dense (2^k, 2^k) matrix, 1 <= k <= 6, on LOGICAL bits (as apply_bits): bit j of the matrix's row / column index is
    logical bit bits[j], bits[0] the least significant; applied where every bit of ctl_mask is 1 (qh_apply_matrix)."""
    m = np.ascontiguousarray(matrix, dtype=np.complex128)
    bits = np.ascontiguousarray([int(b) for b in bits], dtype=np.int32)
    k = len(bits)
    if m.shape != (1 << k, 1 << k):
      raise ValueError(f'apply_matrix: a {m.shape} matrix for {k} bits')
    native.check(self.lib.qh_apply_matrix(self.h, k, bits.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), int(ctl_mask),
                                          m.ctypes.data_as(_dp)))

  def apply_mux(self, gates, sel_bits, tgt_bit):
    """Multiplexed 2x2 (qh_apply_mux): `gates` of shape (2^k, 2, 2); for every index, s = the value of the LOGICAL
    selection bits (sel_bits[0] the least significant bit of s) and gates[s] is applied to LOGICAL bit tgt_bit.
    0 <= k <= 16; one read and one write of the state for any k."""
    sel = np.ascontiguousarray([int(b) for b in sel_bits], dtype=np.int32)
    k = len(sel)
    g = np.ascontiguousarray(gates, dtype=np.complex128)
    if g.shape != (1 << k, 2, 2):
      raise ValueError(f'apply_mux: gates of shape {g.shape} for {k} selection bits (want ({1 << k}, 2, 2))')
    native.check(self.lib.qh_apply_mux(self.h, k, sel.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), int(tgt_bit),
                                       g.ctypes.data_as(_dp)))

  def apply_diag(self, values, bits):
    """a_i *= values[s(i)] (qh_apply_diag): 2^k complex values, s gathered from the LOGICAL bits `bits` (bits[0] the
    least significant bit of s).  0 <= k <= 16."""
    b = np.ascontiguousarray([int(x) for x in bits], dtype=np.int32)
    k = len(b)
    v = np.ascontiguousarray(values, dtype=np.complex128)
    if v.shape != (1 << k,):
      raise ValueError(f'apply_diag: values of shape {v.shape} for {k} bits (want ({1 << k},))')
    native.check(self.lib.qh_apply_diag(self.h, k, b.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), v.ctypes.data_as(_dp)))

  def apply_perm(self, table, bits, ctl_mask=0):
    """|s> -> |table[s]> on the register of LOGICAL bits `bits` (bits[0] the least significant bit of s) where every bit of
    ctl_mask is 1 (qh_apply_perm): `table` is a bijection of range(2^k), 1 <= k <= 16.  Amplitudes are moved, not computed."""
    b = np.ascontiguousarray([int(x) for x in bits], dtype=np.int32)
    k = len(b)
    t = np.asarray(table)
    if t.shape != (1 << k,) or np.any(t < 0) or np.any(t >= 1 << 32):
      raise ValueError(f'apply_perm: a table of shape {t.shape} for {k} bits (want ({1 << k},) of non-negative integers)')
    t = np.ascontiguousarray(t, dtype=np.uint32)
    native.check(self.lib.qh_apply_perm(self.h, k, b.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), int(ctl_mask),
                                        t.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))))

  def perm_plan(self, bits, ctl_mask=0):
    """How apply_perm on these bits would walk the state right now (qh_perm_plan), as a dict."""
    b = np.ascontiguousarray([int(x) for x in bits], dtype=np.int32)
    t = native.QhPermTiles()
    native.check(self.lib.qh_perm_plan(self.h, len(b), b.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), int(ctl_mask), ctypes.byref(t)))
    return t.as_dict()

  def apply_rank1(self, bits, u=None, v=None, a=-1.0, b=2.0, ctl_mask=0, sums=False):
    """a I + b |u><v| on the register of LOGICAL bits `bits` (bits[0] the least significant bit of the table index) where every
    bit of ctl_mask is 1 (qh_apply_rank1).  u, v: 2^k complex numbers, k <= 16; u=None means u = v; v=None (then u must be None)
    is the uniform vector 2^(-k/2), any k up to the local bits.  The defaults a = -1, b = 2 are the reflection 2|v><v| - I.
    sums=True returns (sum |psi'|^2 over the amplitudes whose controls are met, sum |<v|psi_r>|^2 over those fibres)."""
    bb = np.ascontiguousarray([int(x) for x in bits], dtype=np.int32)
    k = len(bb)
    if v is None and u is not None:
      raise ValueError('apply_rank1: u without v (v=None is the uniform form)')

    def table(t, name):
      if t is None:
        return None
      t = np.ascontiguousarray(t, dtype=np.complex128)
      if t.shape != (1 << k,):
        raise ValueError(f'apply_rank1: {name} of shape {t.shape} for {k} bits (want ({1 << k},))')
      return t
    tu, tv = table(u, 'u'), table(v, 'v')
    ab = np.array([complex(a), complex(b)], dtype=np.complex128)
    out = np.zeros(2, dtype=np.float64)
    native.check(self.lib.qh_apply_rank1(self.h, k, bb.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), int(ctl_mask),
                                         tu.ctypes.data_as(_dp) if tu is not None else None,
                                         tv.ctypes.data_as(_dp) if tv is not None else None,
                                         ab[0:1].ctypes.data_as(_dp), ab[1:2].ctypes.data_as(_dp),
                                         out.ctypes.data_as(_dp) if sums else None))
    return (float(out[0]), float(out[1])) if sums else None

  def rank1_plan(self, bits, ctl_mask=0, uniform=False):
    """How apply_rank1 on these bits would run right now (qh_rank1_plan), as a dict."""
    b = np.ascontiguousarray([int(x) for x in bits], dtype=np.int32)
    t = native.QhRank1Info()
    native.check(self.lib.qh_rank1_plan(self.h, len(b), b.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), int(ctl_mask),
                                        1 if uniform else 0, ctypes.byref(t)))
    return t.as_dict()

  def apply_bits_raw(self, ctl_mask, tgt_bit, addr):
    """apply_bits with the gate given as the address of 8 contiguous doubles."""
    rc = self.lib.qh_apply_bits(self.h, ctl_mask, tgt_bit, ctypes.cast(addr, _dp))
    if rc:
      native.check(rc)

  def run_stream(self, ops, gates8):
    """ops int32[G,2] (ctl or NO_CTL, tgt), gates8 float64[G,8] -- reference qubit numbers."""
    ops = np.ascontiguousarray(ops, dtype=np.int32).reshape(-1, 2)
    gates8 = np.ascontiguousarray(gates8, dtype=np.float64).reshape(-1, 8)
    assert len(ops) == len(gates8)
    # one FFI call for the stream: exactly len(ops) qh_apply1 / qh_applyc calls inside (include/qcc_hip.h)
    native.check(self.lib.qh_apply_stream(self.h, len(ops), ops.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                          gates8.ctypes.data_as(_dp)))

  def flush(self):
    native.check(self.lib.qh_flush(self.h))

  def sync(self):
    native.check(self.lib.qh_sync(self.h))

  # -- multi-GPU exchange (include/qcc_hip.h: qh_comm_* / qh_exchange_*) ------------
  @staticmethod
  def comm_unique_id():
    buf = ctypes.create_string_buffer(128)
    native.check(native.load().qh_comm_unique_id(buf))
    return buf.raw

  def comm_init(self, nranks, rank, unique_id):
    """RCCL transport: send/recv over xGMI on the engine's exchange stream."""
    assert len(unique_id) == 128
    native.check(self.lib.qh_comm_init(self.h, int(nranks), int(rank), ctypes.c_char_p(unique_id)))

  def comm_init_custom(self, nranks, rank, round_fn):
    """Host-staged transport: round_fn(peers, send_arrays, recv_arrays) moves one round (uint8 views of
    the engine's pinned buffers); used with gloo when several ranks share one GPU (tests)."""
    def _cb(_user, npeers, peers, send, recv, nbytes):
      try:
        ps = [peers[i] for i in range(npeers)]
        sv = [np.ctypeslib.as_array(ctypes.cast(send[i], ctypes.POINTER(ctypes.c_uint8)), shape=(nbytes,)) for i in range(npeers)]
        rv = [np.ctypeslib.as_array(ctypes.cast(recv[i], ctypes.POINTER(ctypes.c_uint8)), shape=(nbytes,)) for i in range(npeers)]
        round_fn(ps, sv, rv)
        return 0
      except Exception:  # pylint: disable=broad-except
        import traceback
        traceback.print_exc()
        return 1
    self._round_cb = native.ROUND_FN(_cb)     # keep the trampoline alive as long as the handle
    native.check(self.lib.qh_comm_init_custom(self.h, int(nranks), int(rank), self._round_cb, None))

  def comm_destroy(self):
    native.check(self.lib.qh_comm_destroy(self.h))

  def exchange_alltoall(self, base_bit, chunk_amps=0):
    native.check(self.lib.qh_exchange_alltoall(self.h, int(base_bit), int(chunk_amps)))

  def exchange_pair(self, shard_bit, local_bit, chunk_amps=0):
    native.check(self.lib.qh_exchange_pair(self.h, int(shard_bit), int(local_bit), int(chunk_amps)))

  def exchange_loopback(self, local_bit, chunk_amps=0):
    native.check(self.lib.qh_exchange_loopback(self.h, int(local_bit), int(chunk_amps)))

  def exchange_wait(self):
    native.check(self.lib.qh_exchange_wait(self.h))

  def comm_init_dry(self, nranks, rank):
    """Planner-only handles: qh_exchange_* decide slabs / rounds / path like rank `rank` of `nranks` would; nothing moves."""
    native.check(self.lib.qh_comm_init_dry(self.h, int(nranks), int(rank)))

  def exchange_geometry(self):
    """How the last exchange was cut (qh_xgeom): equal on every rank by construction, compared before data moves."""
    g = native.QhXGeom()
    native.check(self.lib.qh_exchange_geometry(self.h, ctypes.byref(g)))
    return g.as_dict()

  def exchange_stats(self):
    s = native.QhXStats()
    native.check(self.lib.qh_exchange_stats(self.h, ctypes.byref(s)))
    return s.as_dict()

  def allreduce_sum(self, values):
    a = np.ascontiguousarray(values, dtype=np.float64).copy()
    native.check(self.lib.qh_comm_allreduce_sum(self.h, a.ctypes.data_as(_dp), a.size))
    return a

  # -- readers --------------------------------------------------------------------
  def norm2(self):
    v = ctypes.c_double()
    native.check(self.lib.qh_norm2(self.h, ctypes.byref(v)))
    return v.value

  def argmax(self):
    i, p = ctypes.c_uint64(), ctypes.c_double()
    native.check(self.lib.qh_argmax(self.h, ctypes.byref(i), ctypes.byref(p)))
    return self.phys_to_logical(i.value), p.value

  def prob_bit(self, logical_bit, value=1):
    v = ctypes.c_double()
    native.check(self.lib.qh_prob_bit_value(self.h, int(logical_bit), int(value), ctypes.byref(v)))
    return v.value

  def scale(self, z):
    z = complex(z)
    native.check(self.lib.qh_scale(self.h, z.real, z.imag))

  def project_bit(self, logical_bit, value):
    native.check(self.lib.qh_project_bit(self.h, int(logical_bit), int(value)))

  def marginal(self, bits):
    """(2^k,) float64: entry j = sum |a|^2 over the indices whose LOGICAL bit bits[t] equals bit t of j (qh_marginal;
    0 <= k <= 16, not normalised, bitwise reproducible)."""
    b = np.ascontiguousarray([int(x) for x in bits], dtype=np.int32)
    if b.size > MAX_MARGINAL_BITS:      # (before sizing the 2^k result: the engine would refuse it anyway)
      raise native.QhError(native.QH_ERR_ARG, f'marginal: k = {b.size} outside [0,{MAX_MARGINAL_BITS}]')
    out = np.zeros(1 << b.size, dtype=np.float64)
    native.check(self.lib.qh_marginal(self.h, int(b.size), b.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                      out.ctypes.data_as(_dp)))
    return out

  def reduced_density(self, bits):
    """(2^k, 2^k) complex128: rho[r][c] = sum_e a(r,e) conj(a(c,e)) over this shard, where the LOGICAL bit bits[t] of a(r,e)'s
    index is bit t of r (qh_reduced_density; 0 <= k <= 8, not normalised, bitwise Hermitian and reproducible)."""
    b = np.ascontiguousarray([int(x) for x in bits], dtype=np.int32)
    if b.size > MAX_DENSITY_BITS:      # (before sizing the 4^k result: the engine would refuse it anyway)
      raise native.QhError(native.QH_ERR_ARG, f'reduced_density: k = {b.size} outside [0,{MAX_DENSITY_BITS}]')
    out = np.zeros((1 << b.size, 1 << b.size), dtype=np.complex128)
    native.check(self.lib.qh_reduced_density(self.h, int(b.size), b.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                             out.ctypes.data_as(_dp)))
    return out

  def density_plan(self, bits):
    """How reduced_density(bits) would walk the state right now (qh_density_plan), as a dict."""
    b = np.ascontiguousarray([int(x) for x in bits], dtype=np.int32)
    t = native.QhDensityTiles()
    native.check(self.lib.qh_density_plan(self.h, int(b.size), b.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), ctypes.byref(t)))
    return t.as_dict()

  def sample(self, u):
    """LOGICAL indices drawn by inverse CDF for the ascending uniforms u in [0, 1) (qh_sample)."""
    u = np.ascontiguousarray(u, dtype=np.float64).reshape(-1)
    out = np.zeros(u.size, dtype=np.uint64)
    native.check(self.lib.qh_sample(self.h, int(u.size), u.ctypes.data_as(_dp),
                                    out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))))
    return out

  def expect_pauli(self, xmasks, zmasks):
    """(T,) float64: Re <psi|P_t|psi> of the Pauli strings given as LOGICAL bit masks (x: X or Y on the bit, z: Z or Y),
    summed over this shard, not normalised (qh_expect_pauli: strings that share an x mask share a read of the state)."""
    x = np.ascontiguousarray([int(v) for v in xmasks], dtype=np.uint64)
    z = np.ascontiguousarray([int(v) for v in zmasks], dtype=np.uint64)
    if x.size != z.size:
      raise ValueError(f'expect_pauli: {x.size} x masks, {z.size} z masks')
    out = np.zeros(x.size, dtype=np.float64)
    u64p = ctypes.POINTER(ctypes.c_uint64)
    native.check(self.lib.qh_expect_pauli(self.h, int(x.size), x.ctypes.data_as(u64p), z.ctypes.data_as(u64p),
                                          out.ctypes.data_as(_dp)))
    return out

  # -- sparse readout ------------------------------------------------------------
  @staticmethod
  def _entries(buf, count):
    """(idx uint64, amp complex128) of the first `count` qh_entry records of a ctypes array."""
    if not count:
      return np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=np.complex128)
    rec = np.frombuffer(buf, dtype=np.dtype([('index', np.uint64), ('re', np.float64), ('im', np.float64)]), count=count)
    amp = np.empty(count, dtype=np.complex128)      # (component by component: re + 1j * im would lose the sign of a zero)
    amp.real, amp.imag = rec['re'], rec['im']
    return rec['index'].copy(), amp

  def select(self, threshold, cap=1 << 16):
    """(idx uint64, amp complex128, count, weight): the amplitudes of this shard with probability >= threshold, by ascending
    GLOBAL LOGICAL index, their exact number and the sum of their probabilities (qh_select: one read of the state).  More
    than cap of them: the arrays are empty, count and weight still hold.  cap = 0 counts only."""
    cap = int(cap)
    buf = (native.QhEntry * cap)() if cap else None
    n, w = ctypes.c_uint64(), ctypes.c_double()
    native.check(self.lib.qh_select(self.h, float(threshold), cap, buf, ctypes.byref(n), ctypes.byref(w)))
    idx, amp = self._entries(buf, n.value if n.value <= cap else 0)
    return idx, amp, int(n.value), float(w.value)

  def topk(self, k):
    """(idx uint64, amp complex128): the k most probable amplitudes of this shard, most probable first, ties by ascending
    GLOBAL LOGICAL index; never one of probability 0, so fewer than k where the support is smaller (qh_topk)."""
    k = int(k)
    buf = (native.QhEntry * k)() if k else None
    n = ctypes.c_uint64()
    native.check(self.lib.qh_topk(self.h, k, buf, ctypes.byref(n)))
    return self._entries(buf, n.value)

  def amplitudes(self, indices, nlocal=False):
    """complex128 array: the amplitudes at the GLOBAL LOGICAL indices given, exact zeros where another shard holds them
    (qh_amplitudes: one gather, one copy back).  nlocal=True: (array, how many this shard holds)."""
    idx = np.ascontiguousarray(indices, dtype=np.uint64).reshape(-1)
    out = np.zeros(idx.size, dtype=np.complex128)
    n = ctypes.c_uint64()
    native.check(self.lib.qh_amplitudes(self.h, int(idx.size), idx.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)),
                                        out.ctypes.data_as(_dp), ctypes.byref(n)))
    return (out, int(n.value)) if nlocal else out

  # -- two states ---------------------------------------------------------------
  def clone(self):
    """A new DeviceState holding a copy of this one as it lies -- amplitudes, bit map, shard geometry, fusion level --
    in HBM memory of its own (qh_clone); queued gates run first."""
    h = ctypes.c_void_p()
    native.check(self.lib.qh_clone(self.h, ctypes.byref(h)))
    other = object.__new__(DeviceState)
    other.lib, other.nbits, other.bit_width, other.dtype = self.lib, self.nbits, self.bit_width, self.dtype
    other.h, other.nbits_global = h, self.nbits_global
    return other

  def _sibling(self, call, nbits_delta):
    """Wraps the handle a qh_extend / qh_release call makes (call(out) -> status), the way clone() wraps its own; on
    QH_ERR_NOMEM the parked device states are dropped and the call is tried once more, as in __init__."""
    h = ctypes.c_void_p()
    rc = call(ctypes.byref(h))
    if rc == native.QH_ERR_NOMEM:
      from qcc_amd.lib import backend  # pylint: disable=import-outside-toplevel
      backend.drop_device_pool()
      rc = call(ctypes.byref(h))
    native.check(rc)
    other = object.__new__(DeviceState)
    other.lib, other.bit_width, other.dtype, other.h = self.lib, self.bit_width, self.dtype, h
    other.nbits, other.nbits_global = self.nbits + nbits_delta, self.nbits_global + nbits_delta
    return other

  def extend(self, nqubits, amps=None, basis=0):
    """A new DeviceState holding self (x) f (np.kron order: the nqubits new qubits are the least significant logical bits),
    built on the device (qh_extend); f = amps (2^nqubits amplitudes) or, where amps is None, the basis state |basis>.
    1 <= nqubits <= 16.  This state is left as clone() leaves it."""
    k = int(nqubits)
    tab = None
    if amps is not None:
      tab = np.ascontiguousarray(amps, dtype=np.complex128).reshape(-1)
      if not 1 <= k <= 16 or tab.size != 1 << k:
        raise ValueError(f'extend: {tab.size} amplitudes for {k} qubits')
    ptr = tab.ctypes.data_as(_dp) if tab is not None else None
    return self._sibling(lambda out: self.lib.qh_extend(self.h, k, ptr, int(basis), out), k)

  def release(self, bits, value=0):
    """(new DeviceState, kept, dropped): the slice of this state where LOGICAL bit bits[j] equals bit j of value, as a state
    of len(bits) fewer qubits (qh_release: the remaining bits keep their order and are renumbered from 0), with the sums of
    |a|^2 of the amplitudes kept and dropped (per shard, not normalised).  Nothing is rescaled.  This state is left as
    clone() leaves it."""
    b = np.ascontiguousarray([int(x) for x in bits], dtype=np.int32)
    w = (ctypes.c_double * 2)()
    bp = b.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    new = self._sibling(lambda out: self.lib.qh_release(self.h, int(b.size), bp, int(value), w, out), -int(b.size))
    return new, float(w[0]), float(w[1])

  def copy_from(self, other):
    """This state := other's, amplitudes and bit map (qh_copy); what this state has queued is dropped."""
    native.check(self.lib.qh_copy(self.h, other.h))

  def inner(self, other):
    """complex <self|other> = sum_i conj(self_i) other_i by LOGICAL index, over this shard, not normalised (qh_inner:
    both states are read where they lie, whatever their layouts)."""
    out = (ctypes.c_double * 2)()
    native.check(self.lib.qh_inner(self.h, other.h, out))
    return complex(out[0], out[1])

  def axpby(self, alpha, other, beta, norm=False):
    """self := alpha * self + beta * other by LOGICAL index, in place, in this state's layout (qh_axpby: both states are
    read where they lie; other is read only).  norm=True returns sum |a|^2 of the new amplitudes over this shard (a float,
    summed in a fixed order on the device), otherwise None."""
    a, b = complex(alpha), complex(beta)
    out = ctypes.c_double() if norm else None
    native.check(self.lib.qh_axpby(self.h, (ctypes.c_double * 2)(a.real, a.imag), other.h, (ctypes.c_double * 2)(b.real, b.imag),
                                   ctypes.byref(out) if norm else None))
    return out.value if norm else None

  # -- Pauli-sum operators ------------------------------------------------------
  @staticmethod
  def _pauli_arrays(coeffs, xmasks, zmasks):
    c = np.ascontiguousarray([complex(v) for v in coeffs], dtype=np.complex128)
    x = np.ascontiguousarray([int(v) for v in xmasks], dtype=np.uint64)
    z = np.ascontiguousarray([int(v) for v in zmasks], dtype=np.uint64)
    if not c.size == x.size == z.size:
      raise ValueError(f'apply_pauli_sum: {c.size} coefficients, {x.size} x masks, {z.size} z masks')
    u64p = ctypes.POINTER(ctypes.c_uint64)
    return (c, x, z), c.view(np.float64).ctypes.data_as(_dp), x.ctypes.data_as(u64p), z.ctypes.data_as(u64p)

  def apply_pauli_sum(self, coeffs, xmasks, zmasks, out=None, norm=False):
    """(sum_t c_t P_t) self as a state of its own (qh_apply_pauli_sum): complex coefficients and Pauli strings as LOGICAL
    bit masks (x: X or Y on the bit, z: Z or Y), as in expect_pauli.  This state is read only (queued gates run first).
    out=None: a new DeviceState (qh_pauli_sum_new); otherwise the result replaces out's state, which takes this state's
    bit map, and out is returned.  norm=True returns (state, sum |a|^2 of the result over this shard)."""
    keep, cp, xp, zp = self._pauli_arrays(coeffs, xmasks, zmasks)
    n = int(keep[0].size)
    n2 = ctypes.c_double() if norm else None
    n2p = ctypes.byref(n2) if norm else None
    if out is None:
      out = self._sibling(lambda h: self.lib.qh_pauli_sum_new(self.h, n, cp, xp, zp, n2p, h), 0)
    else:
      native.check(self.lib.qh_apply_pauli_sum(out.h, self.h, n, cp, xp, zp, n2p))
    return (out, n2.value) if norm else out

  def pauli_sum_plan(self, xmasks, zmasks):
    """How apply_pauli_sum would batch these strings right now (qh_pauli_sum_plan): (terms, batches), lists of dicts."""
    keep, _cp, xp, zp = self._pauli_arrays([0] * len(xmasks), xmasks, zmasks)
    n = int(keep[0].size)
    terms = (native.QhPauliTerm * max(n, 1))()
    cap = n // native.QH_PAULI_SUM_BATCH + 1
    batches = (native.QhPauliBatch * cap)()
    nb = ctypes.c_uint64()
    native.check(self.lib.qh_pauli_sum_plan(self.h, n, xp, zp, terms, batches, cap, ctypes.byref(nb)))
    tl = [{k: int(getattr(terms[j], k)) for k, _ in native.QhPauliTerm._fields_} for j in range(n)]
    return tl, [batches[b].as_dict() for b in range(nb.value)]

  # -- Pauli products -------------------------------------------------------------
  @staticmethod
  def _pauli_product_arrays(a, b, xmasks, zmasks):
    ab = np.ascontiguousarray([[complex(u), complex(v)] for u, v in zip(a, b)], dtype=np.complex128).reshape(-1, 2)
    x = np.ascontiguousarray([int(v) for v in xmasks], dtype=np.uint64)
    z = np.ascontiguousarray([int(v) for v in zmasks], dtype=np.uint64)
    if not len(a) == len(b) == x.size == z.size:
      raise ValueError(f'apply_pauli_product: {len(a)} a, {len(b)} b, {x.size} x masks, {z.size} z masks')
    u64p = ctypes.POINTER(ctypes.c_uint64)
    return (ab, x, z), ab.view(np.float64).ctypes.data_as(_dp), x.ctypes.data_as(u64p), z.ctypes.data_as(u64p)

  def apply_pauli_product(self, a, b, xmasks, zmasks, norm=False):
    """state := F_{n-1} ... F_0 state in place, F_t = a[t] I + b[t] P_t (qh_apply_pauli_product): complex a, b and Pauli
    strings as LOGICAL bit masks (x: X or Y on the bit, z: Z or Y), as in expect_pauli.  Term 0 is applied first.  Queued
    gates run first.  norm=True returns sum |a|^2 of the result over this shard, otherwise None."""
    keep, abp, xp, zp = self._pauli_product_arrays(list(a), list(b), xmasks, zmasks)
    n2 = ctypes.c_double() if norm else None
    native.check(self.lib.qh_apply_pauli_product(self.h, int(keep[1].size), abp, xp, zp, ctypes.byref(n2) if norm else None))
    return n2.value if norm else None

  def pauli_product_plan(self, xmasks, zmasks):
    """How apply_pauli_product would cut these strings into runs right now (qh_pauli_product_plan): (terms, runs), lists of
    dicts; the terms are in the caller's order."""
    keep, _abp, xp, zp = self._pauli_product_arrays([0] * len(xmasks), [0] * len(xmasks), xmasks, zmasks)
    n = int(keep[1].size)
    terms = (native.QhPauliTerm * max(n, 1))()
    cap = max(n, 1)
    runs = (native.QhPauliRun * cap)()
    nr = ctypes.c_uint64()
    native.check(self.lib.qh_pauli_product_plan(self.h, n, xp, zp, terms, runs, cap, ctypes.byref(nr)))
    tl = [{k: int(getattr(terms[j], k)) for k, _ in native.QhPauliTerm._fields_} for j in range(n)]
    return tl, [runs[r].as_dict() for r in range(nr.value)]

  # -- Z-polynomial operators ------------------------------------------------------
  @staticmethod
  def _zpoly_arrays(weights, zmasks):
    w = np.ascontiguousarray([float(v) for v in weights], dtype=np.float64)
    z = np.ascontiguousarray([int(v) for v in zmasks], dtype=np.uint64)
    if w.size != z.size:
      raise ValueError(f'zpoly: {w.size} weights, {z.size} z masks')
    return (w, z), w.ctypes.data_as(_dp), z.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))

  def apply_zpoly(self, weights, zmasks, c, norm=False):
    """a_i *= exp(c f(i)) in place, f(i) = sum_t weights[t] (-1)^popcount(i & zmasks[t]) over LOGICAL bits, complex c
    (qh_apply_zpoly: one pass over the state for any number of terms).  Queued gates run first.  norm=True returns
    sum |a|^2 of the result over this shard, otherwise None."""
    keep, wp, zp = self._zpoly_arrays(weights, zmasks)
    c = complex(c)
    cc = (ctypes.c_double * 2)(c.real, c.imag)
    n2 = ctypes.c_double() if norm else None
    native.check(self.lib.qh_apply_zpoly(self.h, int(keep[0].size), wp, zp, cc, ctypes.byref(n2) if norm else None))
    return n2.value if norm else None

  def expect_zpoly(self, weights, zmasks):
    """(norm2, mean, second) = sum |a_i|^2 (1, f(i), f(i)^2) over this shard, not normalised (qh_expect_zpoly: one read of
    the state for any number of terms)."""
    keep, wp, zp = self._zpoly_arrays(weights, zmasks)
    out = (ctypes.c_double * 3)()
    native.check(self.lib.qh_expect_zpoly(self.h, int(keep[0].size), wp, zp, out))
    return float(out[0]), float(out[1]), float(out[2])

  def zpoly_plan(self, weights, zmasks):
    """How the terms fall on the layout right now (qh_zpoly_plan), as a dict: counts by class, per-term physical masks,
    folded weights and classes, the groups' low masks, the kernel and its grid."""
    keep, wp, zp = self._zpoly_arrays(weights, zmasks)
    info = native.QhZpolyInfo()
    native.check(self.lib.qh_zpoly_plan(self.h, int(keep[0].size), wp, zp, ctypes.byref(info)))
    return info.as_dict()

  def inner_plan(self, other):
    """How inner(other) would walk the two states right now (qh_inner_plan), as a dict."""
    t = native.QhInnerTiles()
    native.check(self.lib.qh_inner_plan(self.h, other.h, ctypes.byref(t)))
    return t.as_dict()

  # -- matrix elements between two states -------------------------------------------
  @staticmethod
  def _mask_arrays(who, xmasks, zmasks):
    x = np.ascontiguousarray([int(v) for v in xmasks], dtype=np.uint64)
    z = np.ascontiguousarray([int(v) for v in zmasks], dtype=np.uint64)
    if x.size != z.size:
      raise ValueError(f'{who}: {x.size} x masks, {z.size} z masks')
    u64p = ctypes.POINTER(ctypes.c_uint64)
    return (x, z), x.ctypes.data_as(u64p), z.ctypes.data_as(u64p)

  def transition_pauli(self, other, xmasks, zmasks):
    """(T,) complex128: <self|P_t|other> of the Pauli strings given as LOGICAL bit masks (x: X or Y on the bit, z: Z or Y),
    as in expect_pauli, summed over this shard by LOGICAL index, not normalised (qh_transition_pauli: both states are read
    where they lie, strings that share an x mask share a read of them)."""
    keep, xp, zp = self._mask_arrays('transition_pauli', xmasks, zmasks)
    out = np.zeros(keep[0].size, dtype=np.complex128)
    native.check(self.lib.qh_transition_pauli(self.h, other.h, int(keep[0].size), xp, zp, out.view(np.float64).ctypes.data_as(_dp)))
    return out

  def transition_plan(self, other, xmasks, zmasks):
    """How transition_pauli(other, ...) would run these strings right now (qh_transition_plan): (terms, passes), lists of
    dicts; px is in other's physical positions, pz in this state's."""
    keep, xp, zp = self._mask_arrays('transition_plan', xmasks, zmasks)
    n = int(keep[0].size)
    terms = (native.QhPauliTerm * max(n, 1))()
    cap = max(n, 1)
    passes = (native.QhTransitionPass * cap)()
    npass = ctypes.c_uint64()
    native.check(self.lib.qh_transition_plan(self.h, other.h, n, xp, zp, terms, passes, cap, ctypes.byref(npass)))
    tl = [{k: int(getattr(terms[j], k)) for k, _ in native.QhPauliTerm._fields_} for j in range(n)]
    return tl, [passes[p].as_dict() for p in range(npass.value)]

  def project_bits(self, mask, value):
    """Zero every amplitude whose LOGICAL bits under mask differ from value (qh_project_bits); renormalise with scale."""
    native.check(self.lib.qh_project_bits(self.h, int(mask), int(value)))

  def phys_to_logical(self, i):
    o = ctypes.c_uint64()
    native.check(self.lib.qh_phys_to_logical(self.h, int(i), ctypes.byref(o)))
    return o.value

  def logical_to_phys(self, i):
    o = ctypes.c_uint64()
    native.check(self.lib.qh_logical_to_phys(self.h, int(i), ctypes.byref(o)))
    return o.value

  def remap_swap(self, a, b):
    native.check(self.lib.qh_remap_swap(self.h, int(a), int(b)))

  def amplitude(self, logical_index):
    """One amplitude by LOGICAL (local) index -- 16-byte D2H."""
    out = (ctypes.c_double * 2)()
    native.check(self.lib.qh_amplitude(self.h, int(logical_index), out))
    return self.dtype(complex(out[0], out[1]))

  # -- engine measurement ---------------------------------------------------------
  def stats(self):
    s = native.QhStats()
    native.check(self.lib.qh_get_stats(self.h, ctypes.byref(s)))
    return s.as_dict()

  def reset_stats(self):
    native.check(self.lib.qh_reset_stats(self.h))

  def timer_begin(self):
    native.check(self.lib.qh_timer_begin(self.h))

  def timer_end(self):
    ms = ctypes.c_float()
    native.check(self.lib.qh_timer_end(self.h, ctypes.byref(ms)))
    return ms.value

  def timer_lap(self):
    native.check(self.lib.qh_timer_lap(self.h))

  def timer_laps(self, cap=4096):
    """Milliseconds between consecutive timer_lap() marks (waits for the last one)."""
    buf = (ctypes.c_float * cap)()
    n = ctypes.c_int(0)
    native.check(self.lib.qh_timer_laps(self.h, buf, cap, ctypes.byref(n)))
    return [float(buf[k]) for k in range(min(n.value, cap))]

  def plan_json(self):
    need = ctypes.c_uint64()
    native.check(self.lib.qh_plan_json(self.h, None, 0, ctypes.byref(need)))
    buf = ctypes.create_string_buffer(need.value)
    native.check(self.lib.qh_plan_json(self.h, buf, need.value, None))
    return buf.value.decode()


NO_CTL = -(2 ** 31)
