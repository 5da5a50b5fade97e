"""TEST-ONLY stand-ins for the GPU, used by the CPU ("not gpu") host-logic tests.

OracleDevice implements the interface circuit.qc needs from
qcc_amd.device.DeviceState with NumPy + the CPU oracle; OracleHostExecutor is
the host-buffer counterpart.  Installed through qcc_amd.lib.backend's test
seams; product code never imports this module.
"""
import numpy as np

from tests import oracle_lib


class OracleDevice:
  calls = 0

  def __init__(self, nbits, bit_width):
    self.nbits, self.bit_width = nbits, bit_width
    self.dtype = np.complex128 if bit_width == 128 else np.complex64
    self.psi = np.zeros(1 << nbits, dtype=self.dtype)
    self.o = oracle_lib.load()
    self.trace = []

  def close(self):
    pass

  def host_array(self):
    """stand-in for a host-mapped state (device.DeviceState.host_array): THE buffer gates work on"""
    return self.psi

  def init_basis(self, index=0):
    self.psi[:] = 0
    self.psi[index] = 1

  def init_product(self, factors):
    v = np.ones(1, dtype=np.complex128)
    for n, x in factors:
      if isinstance(x, (int, np.integer)):
        t = np.zeros(1 << n, dtype=np.complex128)
        t[int(x)] = 1
      else:
        t = np.asarray(x, dtype=np.complex128).reshape(-1)
      v = np.kron(v, t)
    self.psi[:] = v.astype(self.dtype)

  def upload(self, host, offset=0):
    host = np.asarray(host, dtype=self.dtype)
    self.psi[offset:offset + host.size] = host

  def download(self, offset=0, count=None, out=None):
    count = self.psi.size - offset if count is None else count
    if out is not None:
      out[:count] = self.psi[offset:offset + count]
      return out
    return self.psi[offset:offset + count].copy()

  def apply1(self, gate, index):
    OracleDevice.calls += 1
    self.trace.append((None, int(index), np.asarray(gate, dtype=np.complex128).reshape(4).copy()))
    self.o.apply1(self.psi, gate, self.nbits, index)

  def applyc(self, gate, control, target):
    OracleDevice.calls += 1
    self.trace.append((int(control), int(target), np.asarray(gate, dtype=np.complex128).reshape(4).copy()))
    self.o.applyc(self.psi, gate, self.nbits, control, target)

  def sync(self):
    pass

  def flush(self):
    pass

  def norm2(self):
    return float(np.vdot(self.psi, self.psi).real)

  def argmax(self):
    i = int(np.argmax(np.abs(self.psi)))
    return i, float(np.abs(self.psi[i]) ** 2)

  def prob_bit(self, bit, value=1):
    sel = ((np.arange(self.psi.size) >> bit) & 1) == value
    return float(np.vdot(self.psi[sel], self.psi[sel]).real)

  def project_bit(self, bit, value):
    sel = ((np.arange(self.psi.size) >> bit) & 1) != value
    self.psi[sel] = 0

  def scale(self, z):
    self.psi *= z

  def amplitude(self, index):
    return self.psi[index]


class PlanDevice(OracleDevice):
  """Like OracleDevice, but the queued gates go through the REAL planner: at every flush the
  queue is planned by the engine library (dry handle, qh_plan_export) and the plan is executed
  with NumPy (tests/plan_interp.py).  States below 8 qubits (no sweeps) use the oracle."""
  planned_flushes = 0

  def __init__(self, nbits, bit_width):
    super().__init__(nbits, bit_width)
    self.queue = []

  def apply1(self, gate, index):
    self.queue.append((None, int(index), np.asarray(gate, dtype=np.complex128).reshape(4).copy()))

  def applyc(self, gate, control, target):
    self.queue.append((int(control), int(target), np.asarray(gate, dtype=np.complex128).reshape(4).copy()))

  def flush(self):
    import ctypes
    from qcc_amd import native
    from tests import plan_interp
    q, self.queue = self.queue, []
    if not q:
      return
    n = self.nbits
    in_range = all(c is None or 0 <= c < n for c, _, _ in q)
    if n < 8 or not in_range:          # no sweeps / the reference's out-of-range control quirk: oracle semantics
      for c, t, g in q:
        if c is None:
          super().apply1(g, t)
        else:
          super().applyc(g, c, t)
      return
    lib = native.load()
    h = ctypes.c_void_p()
    native.check(lib.qh_create_dry(n, 128, ctypes.byref(h)))
    native.check(lib.qh_set_fusion(h, native.QH_FUSE_SWEEP))
    dp = ctypes.POINTER(ctypes.c_double)
    for c, t, g in q:
      g8 = np.ascontiguousarray(g).view(np.float64)
      if c is None:
        native.check(lib.qh_apply1(h, t, g8.ctypes.data_as(dp)))
      else:
        native.check(lib.qh_applyc(h, c, t, g8.ctypes.data_as(dp)))
    sweeps, _ = plan_interp.export_plan(h)
    lib.qh_destroy(h)
    work = self.psi.astype(np.complex128)
    plan_interp.run_plan(work, sweeps, n)
    self.psi[:] = work.astype(self.dtype)
    PlanDevice.planned_flushes += 1

  sync = flush

  def download(self, offset=0, count=None, out=None):
    self.flush()
    return super().download(offset, count, out)

  def upload(self, host, offset=0):
    self.flush()
    super().upload(host, offset)

  def init_basis(self, index=0):
    self.queue = []
    super().init_basis(index)

  def init_product(self, factors):
    self.queue = []
    super().init_product(factors)

  def norm2(self):
    self.flush()
    return super().norm2()

  def argmax(self):
    self.flush()
    return super().argmax()

  def prob_bit(self, bit, value=1):
    self.flush()
    return super().prob_bit(bit, value)

  def project_bit(self, bit, value):
    self.flush()
    super().project_bit(bit, value)

  def scale(self, z):
    self.flush()
    super().scale(z)

  def amplitude(self, index):
    self.flush()
    return super().amplitude(index)


class OracleHostExecutor:
  def __init__(self):
    self.o = oracle_lib.load()

  def apply1(self, psi, gate, nbits, tgt, bit_width=128):
    self.o.apply1(psi, gate, nbits, tgt)

  def applyc(self, psi, gate, nbits, ctl, tgt, bit_width=128):
    self.o.applyc(psi, gate, nbits, ctl, tgt)


class NumpyShardEngine:
  """CPU stand-in for the per-rank engine of qcc_amd.sharded.ShardedState, with the interface of
  qcc_amd.device.DeviceState as that layer uses it: the engine knows its shard (set_shard) and resolves shard-bit
  controls / diagonal gates on shard bits itself, builds states in place, and runs the exchange as host-staged
  ROUNDS through the callback ShardedState hands it (comm_init_custom) -- the same protocol the HIP engine speaks
  when several ranks share one GPU.  NumPy only; TEST INFRASTRUCTURE."""

  def __init__(self, nloc, bit_width=128):
    self.nbits = nloc
    self.nbits_global = nloc
    self.shard = 0
    self.bit_width = bit_width
    self.psi = np.zeros(1 << nloc, dtype=np.complex128)
    self.n_gates = 0
    self._round_fn = None
    self._x = {'exchanges': 0, 'rounds': 0, 'bytes_sent': 0, 'slabs': 0, 'sweeps_overlapped': 0, 'span_ms': 0.0, 'rounds_packed': 0}

  # -- configuration ------------------------------------------------------------------
  def set_shard(self, nbits_global, shard_index):
    self.nbits_global, self.shard = int(nbits_global), int(shard_index)

  def set_relayout(self, on):
    return False                       # one buffer: nothing to re-lay out

  # -- state construction / IO -----------------------------------------------------------
  def init_basis(self, index=0):
    self.psi[:] = 0
    if (int(index) >> self.nbits) == self.shard:
      self.psi[int(index) & ((1 << self.nbits) - 1)] = 1

  def init_product(self, factors):
    idx = (np.uint64(self.shard) << np.uint64(self.nbits)) | np.arange(1 << self.nbits, dtype=np.uint64)
    out = np.ones(idx.shape, dtype=np.complex128)
    shift = self.nbits_global
    for n, x in factors:
      shift -= n
      v = ((idx >> np.uint64(shift)) & np.uint64((1 << n) - 1)).astype(np.int64)
      if isinstance(x, (int, np.integer)):
        out *= (v == int(x))
      else:
        out *= np.asarray(x, dtype=np.complex128).reshape(-1)[v]
    self.psi[:] = out

  def upload(self, host, offset=0):
    host = np.asarray(host, dtype=np.complex128).reshape(-1)
    self.psi[offset:offset + host.size] = host

  def download(self, offset=0, count=None, out=None):
    count = self.psi.size - offset if count is None else count
    return self.psi[offset:offset + count].copy()

  # -- gates (GLOBAL bit positions: bits >= nbits are the shard index) ----------------------
  def apply_bits(self, ctl_mask, tgt_bit, gate):
    g = np.asarray(gate, dtype=np.complex128).reshape(2, 2)
    self.n_gates += 1
    nloc = self.nbits
    hi = int(ctl_mask) >> nloc
    if (self.shard & hi) != hi:
      return                                       # a control lives in the shard index and is 0 here
    cm = int(ctl_mask) & ((1 << nloc) - 1)
    idx = np.arange(self.psi.size)
    on = (idx & cm) == cm
    if tgt_bit >= nloc:                            # diagonal gate on a shard bit: a rank-dependent factor
      assert g[0, 1] == 0 and g[1, 0] == 0, 'dense gate on a shard bit: exchange first'
      f = g[1, 1] if (self.shard >> (tgt_bit - nloc)) & 1 else g[0, 0]
      self.psi[on] *= f
      return
    sel = on & (((idx >> tgt_bit) & 1) == 0)
    lo = idx[sel]
    hi_ = lo | (1 << tgt_bit)
    a, b = self.psi[lo].copy(), self.psi[hi_].copy()
    self.psi[lo] = g[0, 0] * a + g[0, 1] * b
    self.psi[hi_] = g[1, 0] * a + g[1, 1] * b

  def apply_bits_raw(self, ctl_mask, tgt_bit, addr):
    import ctypes
    g = np.ctypeslib.as_array(ctypes.cast(addr, ctypes.POINTER(ctypes.c_double)), shape=(8,)).copy()
    self.apply_bits(ctl_mask, tgt_bit, g.view(np.complex128))

  # -- the exchange: host-staged rounds (qcc_hip.h qh_round_fn semantics) ------------------------
  def comm_init_custom(self, nranks, rank, round_fn):
    self._nranks, self._rank, self._round_fn = int(nranks), int(rank), round_fn

  def comm_destroy(self):
    self._round_fn = None

  def _swap_blocks(self, moves, base, gbits, chunk_amps):
    """moves: [(peer, block value sent, block value where the peer's data lands)] of the gbits local bits at base."""
    run, nruns = 1 << base, 1 << (self.nbits - base - gbits)
    view = self.psi.reshape(nruns, 1 << gbits, run)
    send = [np.ascontiguousarray(view[:, blk, :]).reshape(-1) for _, blk, _ in moves]
    recv = [np.empty_like(s_) for s_ in send]
    chunk = max(1, int(chunk_amps) or send[0].size)
    for off in range(0, send[0].size, chunk):
      self._round_fn([p for p, _, _ in moves], [s_[off:off + chunk].view(np.uint8) for s_ in send],
                     [r_[off:off + chunk].view(np.uint8) for r_ in recv])
      self._x['rounds'] += 1
    for (_, _, land), r_ in zip(moves, recv):
      view[:, land, :] = r_.reshape(nruns, run)
    self._x['exchanges'] += 1
    self._x['bytes_sent'] += sum(s_.nbytes for s_ in send)

  def exchange_alltoall(self, base_bit, chunk_amps=0):
    g = self._nranks.bit_length() - 1
    self._swap_blocks([(j, j, j) for j in range(self._nranks) if j != self._rank], int(base_bit), g, chunk_amps)

  def exchange_pair(self, shard_bit, local_bit, chunk_amps=0):
    mybit = (self._rank >> shard_bit) & 1
    self._swap_blocks([(self._rank ^ (1 << shard_bit), 1 - mybit, 1 - mybit)], int(local_bit), 1, chunk_amps)

  def exchange_stats(self):
    return dict(self._x)

  # -- readers ---------------------------------------------------------------------------------------
  def sync(self):
    pass

  def flush(self):
    pass

  def close(self):
    pass

  def norm2(self):
    return float(np.vdot(self.psi, self.psi).real)

  def argmax(self):
    i = int(np.argmax(np.abs(self.psi)))
    return (self.shard << self.nbits) | i, float(np.abs(self.psi[i]) ** 2)

  def amplitude(self, global_index):
    assert (int(global_index) >> self.nbits) == self.shard
    return self.psi[int(global_index) & ((1 << self.nbits) - 1)]

  def prob_bit(self, bit, value=1):
    sel = ((np.arange(self.psi.size) >> bit) & 1) == value
    return float(np.vdot(self.psi[sel], self.psi[sel]).real)

  def project_bit(self, bit, value):
    self.psi[((np.arange(self.psi.size) >> bit) & 1) != value] = 0

  def scale(self, z):
    self.psi *= complex(z)

  def stats(self):
    return {'gates_submitted': self.n_gates}

  def reset_stats(self):
    self.n_gates = 0


# ---- register readout: NumPy references and stand-ins with marginal / sample / project_bits ---------------------------
def np_marginal(psi, bits, base=0):
  """marginal of the logical bits; psi holds indices base .. base + size - 1"""
  p = np.abs(np.asarray(psi, dtype=np.complex128)) ** 2
  idx = np.uint64(base) + np.arange(p.size, dtype=np.uint64)
  j = np.zeros_like(idx)
  for t, b in enumerate(bits):
    j |= ((idx >> np.uint64(b)) & np.uint64(1)) << np.uint64(t)
  return np.bincount(j.astype(np.int64), weights=p, minlength=1 << len(bits))


def np_sample(psi, u, base=0):
  p = np.abs(np.asarray(psi, dtype=np.complex128)) ** 2
  cdf = np.cumsum(p)
  assert cdf[-1] > 0
  i = np.minimum(np.searchsorted(cdf, np.asarray(u) * cdf[-1], side='right'), np.flatnonzero(p)[-1])
  return (np.uint64(base) + i.astype(np.uint64)).astype(np.uint64)


def np_keep(size, mask, value, base=0):
  idx = np.uint64(base) + np.arange(size, dtype=np.uint64)
  return (idx & np.uint64(mask)) == np.uint64(value)


class MeasureOracle(OracleDevice):
  """OracleDevice with the three readout methods, in NumPy (logical order = the array's order)."""

  def marginal(self, bits):
    return np_marginal(self.psi, bits)

  def sample(self, u):
    return np_sample(self.psi, u)

  def project_bits(self, mask, value):
    self.psi[~np_keep(self.psi.size, mask, value)] = 0


class MeasureShardEngine(NumpyShardEngine):
  """NumpyShardEngine with the readout methods, shard bits resolved as qh_marginal / qh_sample / qh_project_bits do
  (tests/test_gpu_shard_readout.py holds the HIP engine to the same answers)."""

  def marginal(self, bits):
    return np_marginal(self.psi, bits, self.shard << self.nbits)

  def sample(self, u):
    return np_sample(self.psi, u, self.shard << self.nbits)

  def project_bits(self, mask, value):
    self.psi[~np_keep(self.psi.size, mask, value, self.shard << self.nbits)] = 0


def readout_circuit(nq, seed):
  from qcc_amd.lib import circuit
  rng = np.random.default_rng(seed)
  q = circuit.qc('m')
  q.reg(nq, 0)
  for _ in range(3 * nq):
    a = int(rng.integers(nq))
    q.ry(a, float(rng.random() * 3))
    b = int(rng.integers(nq))
    if b != a:
      q.cx(a, b)
    q.rz(int(rng.integers(nq)), float(rng.random() * 3))
  return q


def _shard_qubits(q):
  """qubits whose logical bit the shard index holds now (the router's map), after the queued gates have been routed"""
  st = q._ensure_device().st                             # pylint: disable=protected-access
  return [qb for qb in range(q.nbits) if st.perm[q.nbits - 1 - qb] >= st.nloc]


def sharded_readout_worker(rank, n, out_dir, device_factory, layer=False):
  """One rank of the sharded readout test, inside an initialised process group: qc.probabilities / sample / measure
  through qcc_amd.sharded.ShardedDevice over whatever engine device_factory builds it on (the NumPy stand-in for the CPU
  test, the HIP engine on the GPU); what it saw goes to out_dir/r<rank>.npz for check_sharded_readout.  layer=True: the
  layer's other readers too (prob_bit / project_bit on a held and on a local bit, amplitude, argmax, init_product)."""
  import os
  from qcc_amd.lib import backend, tensor
  tensor.set_tensor_width(128)
  backend.set_device_factory(device_factory)
  q = readout_circuit(n, 5)
  q.h(0)                                                  # dense gates on the top qubits: shard bits get exchanged
  q.cx(0, n - 1)
  res = {'psi': np.asarray(q.psi).copy()}
  sq = _shard_qubits(q)                                   # registers that include qubits held by the shard index
  local = [qb for qb in range(n) if qb not in sq]
  regs = {'shard': sq, 'mixed': [local[0], sq[0], local[-1]], 'local': local[:2]}
  for name, qubits in regs.items():
    res['q_' + name] = np.array(qubits)
    res['p_' + name] = q.probabilities(qubits)
  res['shots'] = q.sample(3000, [0, 2, n - 1], seed=9)
  res['full'] = q.sample(3000, seed=9)
  # seed=None: every rank's global stream differs; the ranks still agree (rank 0's draws)
  np.random.seed(100 + rank)
  res['shots_none'] = q.sample(2000, [1, n - 1])
  res['mq'] = np.array(regs['mixed'])
  res['shard_before_measure'] = np.array(_shard_qubits(q))
  res['m1'] = np.array(q.measure(regs['mixed']))
  res['after'] = np.asarray(q.psi).copy()
  if layer:
    dev = q._ensure_device()                              # pylint: disable=protected-access
    st = dev.st
    hb = [b for b in range(n) if st.perm[b] >= st.nloc][0]       # LOGICAL bits, one held by the shard index, one local
    lb = [b for b in range(n) if st.perm[b] < st.nloc][n // 2]
    res['bits'] = np.array([hb, lb])
    res['prob_bit'] = np.array([dev.prob_bit(b, v) for b in (hb, lb) for v in (0, 1)])
    res['argmax'] = np.array(dev.argmax())
    res['amp_idx'] = np.array([0, (1 << n) - 1, int(res['argmax'][0]), 0x2A5A5 & ((1 << n) - 1)])
    res['amps'] = np.array([dev.amplitude(int(i)) for i in res['amp_idx']])
    res['perm_held'] = np.array([st.perm[hb], st.nloc])
    dev.project_bit(lb, 1)
    res['proj_local'] = np.asarray(dev.download()).copy()
    dev.project_bit(hb, 0)
    res['proj_held'] = np.asarray(dev.download()).copy()
    rng = np.random.default_rng(3)
    tabs = [rng.standard_normal(1 << k) + 1j * rng.standard_normal(1 << k) for k in (3, 2)]
    tabs = [t / np.linalg.norm(t) for t in tabs]
    dev.init_product([(3, tabs[0]), (n - 5, 0b1011), (2, tabs[1])])
    res['product'] = np.asarray(dev.download()).copy()
    res['product_want'] = np.kron(np.kron(tabs[0], np.eye(1 << (n - 5))[0b1011]), tabs[1])
  np.savez(os.path.join(out_dir, f'r{rank}.npz'), **res)


def _project(psi, n, qubits, value):
  idx = np.arange(1 << n)
  keep = np.ones(1 << n, dtype=bool)
  for t, qb in enumerate(qubits):
    keep &= ((idx >> (n - 1 - qb)) & 1) == ((value >> (len(qubits) - 1 - t)) & 1)
  return np.where(keep, psi, 0)


def check_sharded_readout(out_dir, world, n, atol, layer=False):
  """What the ranks of sharded_readout_worker saw against the single-process NumPy answer."""
  import os
  from qcc_amd.lib import backend, circuit, tensor
  res = [dict(np.load(os.path.join(out_dir, f'r{r}.npz'))) for r in range(world)]
  for r in res[1:]:
    for k, v in res[0].items():
      assert np.array_equal(v, r[k]), k                  # every rank returns the same, seed=None included
  r0 = res[0]
  psi = r0['psi']
  g = world.bit_length() - 1
  assert len(r0['q_shard']) == g                          # the shard-bit paths of engine and router ran
  assert set(r0['mq'].tolist()) & set(r0['shard_before_measure'].tolist())
  tensor.set_tensor_width(128)
  backend.set_device_factory(MeasureOracle)
  try:
    q = circuit.qc('single')
    q.psi = psi
    for name in ('shard', 'mixed', 'local'):
      np.testing.assert_allclose(r0['p_' + name], q.probabilities(r0['q_' + name].tolist()), atol=atol)
    # the CDF runs in the sharded layout's physical order (rank order, then the router's bit map): the shots follow the
    # single-process distribution, not its exact sequence
    p_full = np.abs(psi) ** 2
    assert np.all(p_full[r0['full'].astype(np.int64)] > 0)
    freq = np.bincount(r0['full'].astype(np.int64), minlength=1 << n) / 3000
    assert np.max(np.abs(freq - p_full)) < 0.05
    reg = (((r0['full'] >> np.uint64(n - 1)) & np.uint64(1)) << np.uint64(2)) | \
        (((r0['full'] >> np.uint64(n - 3)) & np.uint64(1)) << np.uint64(1)) | (r0['full'] & np.uint64(1))
    assert reg.tolist() == r0['shots'].tolist()            # the same uniforms: the register is the bits of the full shot
    pn = q.probabilities([1, n - 1])
    assert np.all(pn[r0['shots_none'].astype(np.int64)] > 0)
    mq = r0['mq'].tolist()
    value, prob = int(r0['m1'][0]), float(r0['m1'][1])
    assert abs(prob - q.probabilities(mq)[value]) < atol and prob > 0
    np.testing.assert_allclose(r0['after'], _project(psi, n, mq, value) / np.sqrt(prob), atol=atol)
  finally:
    backend.set_device_factory(None)
    tensor.set_tensor_width(None)
  if layer:
    after = r0['after']
    hb, lb = (int(b) for b in r0['bits'])
    assert int(r0['perm_held'][0]) >= int(r0['perm_held'][1])
    idx = np.arange(1 << n)
    pa = np.abs(after) ** 2
    want = [float(pa[((idx >> b) & 1) == v].sum()) for b in (hb, lb) for v in (0, 1)]
    np.testing.assert_allclose(r0['prob_bit'], want, atol=atol)
    k = int(np.argmax(pa))
    assert int(r0['argmax'][0]) == k and abs(float(r0['argmax'][1]) - pa[k]) < atol
    np.testing.assert_allclose(r0['amps'], after[r0['amp_idx'].astype(np.int64)], atol=atol)
    proj = np.where(((idx >> lb) & 1) == 1, after, 0)
    assert np.array_equal(r0['proj_local'], proj)           # zeros are zeros, the rest is untouched
    assert np.array_equal(r0['proj_held'], np.where(((idx >> hb) & 1) == 0, proj, 0))
    np.testing.assert_allclose(r0['product'], r0['product_want'], atol=atol)
