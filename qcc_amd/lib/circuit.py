"""class qc -- the circuit front-end, with the state resident in MI355X HBM.

API mirror of /root/reference/src/lib/circuit.py (class qc :68-534): same method
names, argument order and meaning, so the reference's algorithms run unchanged.
The difference is below ``apply1``/``applyc``: instead of calling the
``libxgates`` CPU extension on a NumPy buffer per gate (circuit.py:196,213) the
gates are queued on a device state (qcc_amd.device.DeviceState -> C-ABI ->
fused HIP sweeps) and the host only sees amplitudes when it asks for them.

Host-visible state contract:
  * ``qc.psi`` returns a READ-ONLY host snapshot (a ``state.State``); it is
    downloaded lazily, only when the device state changed since the last read.
    A snapshot taken earlier is never mutated by later gates.
  * ``qc.psi = some_state`` replaces the state (uploaded before the next gate).
  * readers that do not need all amplitudes (maxprob, prob/ampl of one basis
    state, measure_bit, norm) have device-side equivalents on ``qc`` that move
    a few bytes instead of 2^n amplitudes: ``qc.maxprob()``, ``qc.ampl()``,
    ``qc.prob()``, ``qc.measure_bit()``.
  * registers created with ``reg``/``zeros``/``ones``/``bitstring`` on a circuit
    that is still a basis state never materialise 2^n amplitudes on the host
    (the reference does: circuit.py:121-129 -> np.kron).
  * ``qc(..., alias_psi=True)`` (or QCC_ALIAS_PSI=1), registers up to 26 qubits: the reference's contract
    LITERALLY -- the state lives in pinned host memory the GPU works on in place (qh_create_host_mapped),
    ``qc.psi`` is a writable State over that very memory, every gate is complete when its call returns,
    and ``p = qc.psi; qc.h(0)`` changes ``p`` (src/lib/xgates.cc:37-38).  Every gate crosses PCIe and is
    waited for: for code that depends on the aliasing, not for speed.
"""
import math
import weakref

import numpy as np

from qcc_amd import gates as _gates
from qcc_amd.lib import backend
from qcc_amd.lib import helper
from qcc_amd.lib import ir
from qcc_amd.lib import ops
from qcc_amd.lib import state
from qcc_amd.lib import tensor

try:
    from absl import flags as _flags
    for _name in ('libq', 'qasm', 'cirq', 'text', 'latex'):
        try:
            _flags.DEFINE_string(_name, '', f'Generate {_name} output file, or empty')
        except Exception:  # pylint: disable=broad-except
            pass
except Exception:  # pylint: disable=broad-except
    _flags = None

_SNAPSHOT_LIMIT_BITS = 31  # above this a full host snapshot is refused (>= 32 GiB)
_MEASURE_SNAPSHOT_BITS = 20  # measure_bit returns the real State up to here (16 MiB per call), a lazy handle above: loops of
                             # repeated measurements at 22-26 qubits would otherwise download up to 1 GiB per iteration
_QUEUE_FLUSH_GATES = 4096    # eager gates queued on the host side are handed to the engine in batches of this size, so the GPU starts
                             # working while a long circuit is still being written down
_ALIAS_LIMIT_BITS = 26     # alias_psi: registers up to this size live in host-mapped memory
_NO_CTL = -(2 ** 31)       # "no control" in a gate stream (include/qcc_hip.h QH_NO_CTL)

_U1_CACHE = {}


def _u1_operator(value):
    """ops.U1(value), built once per angle and width (a QFT asks for the same n - 1 angles n / 2 times each: two Operator
    constructions per gate were 40 % of what `qc.qft` costs in Python).  Read-only: the queue copies what it keeps."""
    key = (float(value), tensor.tensor_width())
    op = _U1_CACHE.get(key)
    if op is None:
        if len(_U1_CACHE) > 4096:
            _U1_CACHE.clear()
        op = ops.U1(value)
        op.flags.writeable = False
        _U1_CACHE[key] = op
    return op



_DENSE_MAX_BITS = 6        # qh_apply_matrix: dense operators on up to 6 qubits run on the device
_TABLE_MAX_BITS = 16       # qh_apply_mux / qh_apply_diag: tables over up to 16 qubits
_MARGINAL_MAX_BITS = 16    # qh_marginal: registers of up to 16 qubits (2^16 probabilities)
_DENSITY_MAX_BITS = 8      # qh_reduced_density: registers of up to 8 qubits (a 256 x 256 matrix)
_EXTEND_MAX_BITS = 16      # qh_extend / qh_release: up to 16 qubits added or given back per call


def _dense_bits(op):
    """k if op is a square 2^k x 2^k matrix with 1 <= k <= 6, else 0."""
    shape = np.shape(op)
    if len(shape) != 2 or shape[0] != shape[1] or shape[0] < 2 or shape[0] & (shape[0] - 1):
        return 0
    k = int(shape[0]).bit_length() - 1
    return k if k <= _DENSE_MAX_BITS else 0


def _dump_flags_set():
    if _flags is None:
        return False
    try:
        f = _flags.FLAGS
        return bool(f.libq + f.qasm + f.cirq + f.text + f.latex)
    except Exception:  # pylint: disable=broad-except
        return False


def _sqrt2x2(u):
    """Principal square root of a 2x2 matrix, closed form (the reference calls
    scipy.linalg.sqrtm per Toffoli, circuit.py:238; same matrix to ~1e-16)."""
    u = np.asarray(u, dtype=np.complex128)
    s = np.sqrt(u[0, 0] * u[1, 1] - u[0, 1] * u[1, 0])
    t = np.sqrt(u[0, 0] + u[1, 1] + 2 * s)
    if abs(t) < 1e-12:
        s = -s
        t = np.sqrt(u[0, 0] + u[1, 1] + 2 * s)
    return (u + s * np.eye(2)) / t


class _LazyPsi(np.lib.mixins.NDArrayOperatorsMixin):
    """What measure_bit() hands back as the state of a LARGE register (circuit.py:287-297 returns
    (prob, psi)): most callers only want the probability, so nothing is copied from the device until the
    caller actually looks.  The first look takes a snapshot (a real, read-only State) and every later
    look sees that same snapshot -- the value does not drift when more gates follow.  It is a snapshot of
    the state AT THE TIME OF THE FIRST LOOK; registers of <= 26 qubits get the real State at measurement
    time instead (see measure_bit).  Arithmetic, comparisons and ufuncs work as on the State."""

    def __init__(self, owner):
        self._owner = owner
        self._snap = None

    def _get(self):
        if self._snap is None:
            self._snap = self._owner.psi
            self._owner = None
        return self._snap

    def __array__(self, dtype=None, copy=None):
        a = np.asarray(self._get())
        return a.astype(dtype) if dtype is not None else a

    def __array_ufunc__(self, ufunc, method, *inputs, **kwargs):
        inputs = tuple(x._get() if isinstance(x, _LazyPsi) else x for x in inputs)
        if 'out' in kwargs:
            kwargs['out'] = tuple(x._get() if isinstance(x, _LazyPsi) else x for x in kwargs['out'])
        return getattr(ufunc, method)(*inputs, **kwargs)

    def __matmul__(self, other):
        return self._get() @ (other._get() if isinstance(other, _LazyPsi) else other)

    def __rmatmul__(self, other):
        return other @ self._get()

    def __getattr__(self, name):
        return getattr(self._get(), name)

    def dump(self, desc=None, prob_only=True):
        """State.dump without the snapshot: while nobody has looked yet and the owner's state lives on a device that can
        select, the rows come from there (the state as it is NOW).  prob_only=False prints every basis state and is refused
        above 2^16 of them."""
        if self._snap is None:
            dev = self._owner._sparse_device()      # pylint: disable=protected-access
            if dev is not None:
                self._owner._dump_state(dev, desc, prob_only)      # pylint: disable=protected-access
                return
        self._get().dump(desc, prob_only)

    def __getitem__(self, key):
        return self._get()[key]

    def __len__(self):
        return len(self._get())

    def __iter__(self):
        return iter(self._get())

    def __repr__(self):
        return repr(self._get())


def _alive(ref):
    circ = ref()
    if circ is None:      # (a gate method kept beyond its circuit: `f = qc.h; del qc; f(0)`)
        raise ReferenceError('this gate method belongs to a circuit that has been released')
    return circ


class Snapshot:
    """A copy of a circuit's state at one moment (qc.snapshot): a device state of its own in HBM (or, with a device that
    cannot clone, the amplitudes on the host), the number of qubits and the width.  qc.restore() puts it back,
    qc.overlap() / qc.fidelity() compare against it.  close() (or leaving a `with` block, or collection) releases it."""

    def __init__(self, nbits, width, dev=None, host=None):
        self.nbits, self.width = int(nbits), int(width)
        self._dev, self._host = dev, host

    def close(self):
        dev, self._dev, self._host = self._dev, None, None
        if dev is not None:
            dev.close()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:  # pylint: disable=broad-except
            pass


class qc:
    """State + gate application + (optional) IR recording."""

    def __init__(self, name=None, eager=True, alias_psi=None):
        self.name = name
        import os as _os
        self._alias = bool(_os.environ.get('QCC_ALIAS_PSI') == '1' if alias_psi is None else alias_psi)
        self.ir = ir.Ir()
        self.eager = eager
        self.build_ir = not eager
        self.global_reg = 0
        self.sub_circuits = 0
        # state bookkeeping: exactly one of (_factors, _host, _dev) is authoritative
        self._nbits = 0
        # while no gate has run the state is a tensor product of the pieces handed to
        # reg()/qubit()/bitstring()/state(): [(nqubits, basis index | amplitudes)], most
        # significant first.  It is built ON THE DEVICE (qh_init_product) when the first
        # gate arrives -- the reference np.kron's on the host at every call
        # (circuit.py:121-123).
        self._factors = []
        self._product_flag = True  # (_is_product) True until something non-trivial happens
        self._host = None        # State snapshot (valid iff _host_ok)
        self._host_ok = False
        self._dev = None         # device state (valid iff _dev_ok)
        self._dev_ok = False
        # eager gates wait HERE, as (control | NO_CTL, target) + matrix, until something reads the state: they then
        # reach the engine through ONE native call (qh_apply_stream) instead of one FFI round trip per gate
        # (ctypes + NumPy conversions cost ~25 us per gate, the reference's own Python overhead is 6.5 us: SURVEY 8a A5)
        self._q_ops = []
        self._q_gates = []
        if _dump_flags_set():
            self.eager = False

        for gname, gate in (('h', ops.Hadamard()), ('s', ops.Sgate()), ('t', ops.Tgate()),
                            ('v', ops.Vgate()), ('x', ops.PauliX()), ('y', ops.PauliY()),
                            ('z', ops.PauliZ()), ('yroot', ops.Yroot())):
            self.add_single(gname, gate)
            self.add_single(gname + 'dag', gate.adjoint())
            self.add_ctl('c' + gname, gate)
            self.add_ctl('c' + gname + 'dag', gate.adjoint())

    # ------------------------------------------------------------------ state plumbing
    @property
    def _is_product(self):
        """Still the tensor product of the pieces handed in?  (Asking submits the gates queued on the host side
        first: whoever asks is about to read or rebuild the state.)"""
        if self._q_ops:
            self._drain()
        return self._product_flag

    @_is_product.setter
    def _is_product(self, value):
        self._product_flag = bool(value)

    @property
    def nbits(self):
        return self._nbits

    def _width(self):
        return tensor.tensor_width()

    def _ensure_device(self):
        """Make the device copy authoritative-capable and current (queued gates submitted)."""
        dev = self._device_ready()
        if self._q_ops:
            self._drain()
        return dev

    def _drain(self):
        """Hand the gates queued on the host side to the engine, in order."""
        if not self._q_ops:
            return
        dev = self._device_ready()        # (may raise -- no memory, width change above the snapshot limit: the queue is kept)
        ops_, gs = self._q_ops, self._q_gates
        self._q_ops, self._q_gates = [], []
        # from here on the engine owns the gates: whatever happens, neither the product description nor a host snapshot
        # describes the state any more
        self._product_flag = False
        self._host_ok = False
        if hasattr(dev, 'run_stream'):
            dev.run_stream(np.array(ops_, dtype=np.int32).reshape(-1, 2),
                           np.array(gs, dtype=np.complex128).reshape(-1, 4).view(np.float64).reshape(-1, 8))
        else:
            for (c, t), g in zip(ops_, gs):
                if c == _NO_CTL:
                    dev.apply1(g, t)
                else:
                    dev.applyc(g, c, t)
        self._gate_done()

    def flush(self):
        """Submit everything queued so far (host side and engine side) without waiting for it."""
        if self._nbits:
            dev = self._ensure_device()
            if hasattr(dev, 'flush'):
                dev.flush()

    def _device_ready(self):
        if self._nbits == 0:
            raise ValueError('circuit has no qubits yet')
        if self._dev is not None and (self._dev.nbits != self._nbits or self._dev.bit_width != self._width()):
            if (self._dev_ok and not self._host_ok and not self._product_flag and self._dev.nbits == self._nbits):
                # the tensor width changed under a live state (the reference silently stops applying gates then,
                # SURVEY appendix B Q1): carry the amplitudes over through the host
                if self._nbits > _SNAPSHOT_LIMIT_BITS:
                    raise ValueError(f'tensor width changed to {self._width()} while a {self._nbits}-qubit state is '
                                     f'resident at width {self._dev.bit_width}')
                self._host, self._host_ok = state.State(self._dev.download()), True
            if not self._alias:
                backend.release_device_state(self._dev)     # (alias mode: State views handed out keep the mapped memory alive)
            self._dev, self._dev_ok = None, False
        if self._dev is None:
            if self._alias and self._nbits <= _ALIAS_LIMIT_BITS:
                self._dev = backend.make_host_mapped_state(self._nbits, self._width())
            else:
                self._dev = backend.make_device_state(self._nbits, self._width())
        if not self._dev_ok:
            if self._product_flag:          # (the raw flag: queued gates run right after, on this very state)
                self._dev.init_product(self._factors)
            else:
                assert self._host_ok, 'no valid copy of the state'
                self._dev.upload(np.asarray(tensor.host_current(self._host)))
            self._dev_ok = True
            if self._aliased():
                self._host, self._host_ok = None, False   # from now on THE state is the mapped buffer
        return self._dev

    def _aliased(self):
        return self._alias and self._nbits and self._nbits <= _ALIAS_LIMIT_BITS

    @property
    def psi(self):
        if self._nbits == 0:
            return state.State(1.0)
        if self._q_ops:
            self._drain()
        if self._aliased():
            dev = self._ensure_device()
            dev.sync()
            if self._host is None or not self._host_ok:
                view = state.State(dev.host_array())      # zero copy: the mapped memory itself
                view._keepalive = dev                     # pylint: disable=protected-access
                self._host, self._host_ok = view, True
            return self._host
        if not self._host_ok:
            if self._nbits > _SNAPSHOT_LIMIT_BITS:
                raise MemoryError(f'qc.psi would copy 2^{self._nbits} amplitudes to the host; use qc.maxprob(), '
                                  'qc.ampl(), qc.prob(), qc.measure_bit() (device-side readers) instead')
            if self._dev_ok:
                host = state.State(self._dev.download())
            else:  # still a product state that never reached the device
                vec = np.ones(1, dtype=tensor.tensor_type())
                for n, x in self._factors:
                    if isinstance(x, (int, np.integer)):
                        t = np.zeros(1 << n, dtype=tensor.tensor_type())
                        t[int(x)] = 1
                    else:
                        t = np.asarray(x, dtype=tensor.tensor_type())
                    vec = np.kron(vec, t)
                host = state.State(vec)
            host.flags.writeable = False
            self._host, self._host_ok = host, True
        return self._host

    @psi.setter
    def psi(self, value):
        if self._q_ops:
            self._drain()
        host = tensor.host_current(value) if isinstance(value, state.State) else state.State(value)
        if host.dtype != tensor.tensor_type():
            host = state.State(host)
        if (self._aliased() and self._dev is not None and self._dev_ok and host.ndim and host.nbits == self._nbits
                and self._dev.bit_width == self._width()):
            self._dev.sync()
            np.copyto(self._dev.host_array(), np.asarray(host))     # same register: the mapped buffer stays THE state
            self._is_product = False
            return
        self._nbits = host.nbits if host.ndim else 0
        self._host, self._host_ok = host, True
        self._dev_ok = False
        self._is_product = False
        self._factors = []

    def _tprod(self, new_state, nqubits):
        """psi <- psi (x) new_state (circuit.py:121-123)."""
        if self._is_product:
            idx = getattr(new_state, 'basis_index', None)
            self._append_factor(nqubits, idx if idx is not None else np.array(tensor.host_current(new_state), dtype=np.complex128))
            return
        dev = self._dev
        if (self._dev_ok and dev is not None and not self._alias and hasattr(dev, 'extend') and 1 <= nqubits <= _EXTEND_MAX_BITS
                and dev.nbits == self._nbits and dev.bit_width == self._width()):
            # a live state in HBM: the product is built there (qh_extend), in a buffer of its own; the old one goes back
            idx = getattr(new_state, 'basis_index', None)
            if idx is not None:
                grown = dev.extend(nqubits, basis=int(idx))
            else:
                grown = dev.extend(nqubits, amps=np.array(tensor.host_current(new_state), dtype=np.complex128).reshape(-1))
            self._dev = grown
            backend.release_device_state(dev)
            self._nbits += nqubits
            self.global_reg += nqubits
            self._host, self._host_ok = None, False
            self._factors = []
            return
        cur = self.psi if self._nbits else state.State(1.0)
        self.psi = cur * new_state
        self.global_reg += nqubits

    def _append_factor(self, nqubits, what):
        self._factors.append((int(nqubits), what))
        self._nbits += nqubits
        self.global_reg += nqubits
        self._host_ok = self._dev_ok = False

    def _tprod_basis(self, nqubits, index):
        self._append_factor(nqubits, int(index))

    class scope:
        """Context manager grouping gates into a named IR section."""

        def __init__(self, ir_param, desc):
            self.ir, self.desc = ir_param, desc

        def __enter__(self):
            self.ir.section(self.desc)

        def __exit__(self, t, value, traceback):
            self.ir.end_section()

    # ------------------------------------------------------------------ state builders
    def reg(self, size, it=0, *, name=None):
        ret = state.Reg(size, it, self.global_reg)
        if self._is_product:
            self._tprod_basis(size, helper.bits2val(ret.val))
        else:
            self._tprod(ret.psi(), size)
        self.ir.reg(size, name, ret)
        return ret

    def qubit(self, alpha=None, beta=None):
        self._tprod(state.qubit(alpha, beta), 1)

    def zeros(self, n):
        self._tprod(state.zeros(n), n) if not self._is_product else self._tprod_basis(n, 0)

    def ones(self, n):
        self._tprod(state.ones(n), n) if not self._is_product else self._tprod_basis(n, 2 ** n - 1)

    def bitstring(self, *bits):
        if self._is_product:
            arr = np.asarray(bits)
            assert len(arr) and ((arr == 1) | (arr == 0)).all(), 'Bits must be 0 or 1'
            self._tprod_basis(len(bits), helper.bits2val(bits))
        else:
            self._tprod(state.bitstring(*bits), len(bits))

    def rand_bits(self, n):
        self._tprod(state.rand_bits(n), n)

    def arange(self, n):
        self.psi = state.State([float(i) for i in range(2 ** n)])
        self.global_reg += n

    def random(self, n=1):
        from scipy.stats import unitary_group  # pylint: disable=import-outside-toplevel
        self.psi = ops.Operator(unitary_group.rvs(1 << n))(state.zeros(n))

    def state(self, t):
        psi = state.State(t)
        ret = state.Reg(t.nbits, 0, self.global_reg)
        self._tprod(psi, psi.nbits)
        self.ir.reg(t.nbits, 'state', ret)
        return ret

    @staticmethod
    def _ctl_by_0(ctl):
        """[q] means "controlled by |0>" (circuit.py:166-169)."""
        if isinstance(ctl, (int, np.integer)):
            return int(ctl), False
        return ctl[0], True

    # ------------------------------------------------------------------ gates
    # The generated gate methods are instance attributes (as in the reference, circuit.py:97-101).  They reach the circuit
    # through a WEAK reference: a closure over `self` stored on `self` is a cycle, and a circuit in a cycle keeps its
    # device state -- two 16-GiB buffers at 30 qubits -- until the cycle collector happens to run; `del qc` (or the name
    # going out of scope) must give the state back to the pool at once (backend.release_device_state).
    def add_single(self, name, gate):
        ref = weakref.ref(self)
        setattr(self, name, lambda idx, cond=True: _alive(ref).apply1(gate, idx, name) if cond else None)

    def add_ctl(self, name, gate):
        ref = weakref.ref(self)
        setattr(self, name, lambda idx0, idx1, cond=True: _alive(ref).applyc(gate, idx0, idx1, name) if cond else None)

    def apply1(self, gate, idx_set, name=None, *, val=None):
        """Apply a single-qubit gate to one index or to each index of a list/Reg."""
        if isinstance(idx_set, (int, np.integer)):
            indices = [int(idx_set)]
        elif isinstance(idx_set, (state.Reg, list)):
            indices = list(idx_set)
        else:
            indices = []  # the reference silently ignores other types (quirk Q10)
        for idx in indices:
            if self.build_ir:
                self.ir.single(name, idx, gate, val)
            if self.eager:
                assert idx < self._nbits, 'Invalid qubit index'
                if self._aliased():
                    self._ensure_device().apply1(np.asarray(gate).reshape(4), idx)
                else:
                    if idx < 0:
                        raise ValueError(f'apply1: qubit {idx} out of range for {self._nbits} qubits')
                    self._q_ops.append((_NO_CTL, int(idx)))
                    self._q_gates.append(np.array(gate, dtype=np.complex128).reshape(4))
                    if len(self._q_ops) >= _QUEUE_FLUSH_GATES:
                        self._drain()
                    continue
                self._gate_done()

    def applyc(self, gate, ctl, idx, name=None, *, val=None):
        """Apply `gate` on `idx` controlled by `ctl` ([ctl] = controlled by |0>)."""
        if isinstance(idx, state.Reg):
            assert len(idx) == 1, 'Controlled n-qbit register not supported'
            idx = idx[0]
        ctl_qubit, by_0 = self._ctl_by_0(ctl)
        self.x(ctl_qubit, by_0)
        if self.build_ir:
            self.ir.controlled(name, ctl_qubit, idx, gate, val)
        if self.eager:
            assert idx < self._nbits, 'Invalid qubit index'
            if self._aliased():
                self._ensure_device().applyc(np.asarray(gate).reshape(4), ctl_qubit, idx)
            else:
                if idx < 0 or ctl_qubit >= self._nbits:
                    raise ValueError(f'applyc: qubits ({ctl_qubit}, {idx}) out of range for {self._nbits} qubits')
                if ctl_qubit == idx:
                    raise ValueError(f'applyc: control == target (qubit {idx})')
                self._q_ops.append((int(ctl_qubit), int(idx)))
                self._q_gates.append(np.array(gate, dtype=np.complex128).reshape(4))
                if len(self._q_ops) >= _QUEUE_FLUSH_GATES:
                    self._drain()
            if self._aliased():
                self._gate_done()
        self.x(ctl_qubit, by_0)

    def _gate_done(self):
        self._is_product = False
        if self._aliased():
            self._dev.sync()          # the reference's calls are synchronous: holders of qc.psi see the gate now
        else:
            self._host_ok = False

    def cx0(self, idx0, idx1):
        xgate = ops.PauliX()
        self.apply1(xgate, idx0, 'x')
        self.applyc(ops.PauliX(), idx0, idx1, 'cx')
        self.apply1(xgate, idx0, 'x')

    def cu(self, idx0, idx1, op, desc=None):
        assert op.shape[0] == 2, 'cu only supports 2x2 operators'
        self.applyc(op, idx0, idx1, desc)

    def ccu(self, idx0, idx1, idx2, op, desc=''):
        """Doubly-controlled U by the Sleator-Weinfurter construction (circuit.py:227-246)."""
        i0, c0_by_0 = self._ctl_by_0(idx0)
        i1, c1_by_0 = self._ctl_by_0(idx1)
        with self.scope(self.ir, f'CC{op.name}\\{desc}({idx0},{idx1},{idx2})'):
            self.x(i0, c0_by_0)
            self.x(i1, c1_by_0)
            v = ops.Operator(_sqrt2x2(op))
            self.cu(i0, idx2, v, (op.name or '') + '^{1/2}')
            self.cx(i0, i1)
            self.cu(i1, idx2, v.adjoint(), (op.name or '') + '^t')
            self.cx(i0, i1)
            self.cu(i1, idx2, v, (op.name or '') + '^{1/2}')
            self.x(i1, c1_by_0)
            self.x(i0, c0_by_0)

    def ccx(self, idx0, idx1, idx2):
        self.ccu(idx0, idx1, idx2, ops.PauliX(), 'ccx')

    def toffoli(self, idx0, idx1, idx2):
        self.ccu(idx0, idx1, idx2, ops.PauliX(), 'ccx')

    def u1(self, idx, val):
        self.apply1(ops.U1(val), idx, 'u1', val=val)

    def cu1(self, idx0, idx1, value):
        self.applyc(_u1_operator(value), idx0, idx1, 'cu1', val=value)

    def ccu1(self, idx0, idx1, tgt, value):
        self.ccu(idx0, idx1, tgt, ops.U1(value))

    def rx(self, idx, theta):
        self.apply1(ops.RotationX(theta), idx, 'rx', val=theta)

    def ry(self, idx, theta):
        self.apply1(ops.RotationY(theta), idx, 'ry', val=theta)

    def rz(self, idx, theta):
        self.apply1(ops.RotationZ(theta), idx, 'rz', val=theta)

    def crx(self, ctl, idx, theta):
        self.applyc(ops.RotationX(theta), ctl, idx, 'crx', val=theta)

    def cry(self, ctl, idx, theta):
        self.applyc(ops.RotationY(theta), ctl, idx, 'cry', val=theta)

    def crz(self, ctl, idx, theta):
        self.applyc(ops.RotationZ(theta), ctl, idx, 'crz', val=theta)

    def unitary(self, op, idx):
        """Multi-qubit operator on qubits idx .. idx+k-1 (qubit idx the matrix's most significant bit, np.kron order).
        Up to 6 qubits in range it runs on the device (qh_apply_matrix: no download, no 2^n x 2^n matrix); anything
        else, and devices without apply_matrix, take the reference's route through the full matrix on the host."""
        k = _dense_bits(op)
        if k and isinstance(idx, (int, np.integer)) and 0 <= idx and idx + k <= self._nbits:
            dev = self._ensure_device()
            if hasattr(dev, 'apply_matrix'):
                n = self._nbits
                dev.apply_matrix(np.asarray(ops.Operator(op)), [n - int(idx) - k + j for j in range(k)])
                self._gate_done()
                return
        self.psi = ops.Operator(op)(self.psi, idx)

    def apply_matrix(self, op, qubits, ctl=()):
        """Dense (2^k, 2^k) operator, 1 <= k <= 6, on the qubits `qubits` (any order, not necessarily adjacent;
        qubits[0] is the matrix's most significant bit), applied where every qubit of `ctl` is 1.  An extension: the
        reference has no such method; qc.unitary(op, idx) is apply_matrix(op, range(idx, idx + k))."""
        k = _dense_bits(op)
        qubits, ctl = [int(q) for q in qubits], [int(c) for c in ctl]
        if not k or len(qubits) != k:
            raise ValueError(f'apply_matrix: a {np.shape(op)} operator for {len(qubits)} qubits (want 2^k x 2^k, 1 <= k <= 6)')
        every = qubits + ctl
        if any(q < 0 or q >= self._nbits for q in every):
            raise ValueError(f'apply_matrix: qubits {every} out of range for {self._nbits} qubits')
        if len(set(every)) != len(every):
            raise ValueError(f'apply_matrix: a qubit appears twice among targets {qubits} and controls {ctl}')
        dev = self._ensure_device()
        if not hasattr(dev, 'apply_matrix'):
            raise NotImplementedError(f'apply_matrix: {type(dev).__name__} has no dense-matrix kernel')
        n = self._nbits
        mask = 0
        for c in ctl:
            mask |= 1 << (n - 1 - c)
        dev.apply_matrix(np.asarray(ops.Operator(op)), [n - 1 - q for q in reversed(qubits)], mask)
        self._gate_done()

    # table-selected gates (extensions with the standing of apply_matrix: eager, one kernel each on the device).  In all
    # four the FIRST listed qubit is the most significant bit of the table index (np.kron order, as apply_matrix).
    def _table_device(self, who, method, qubits, nentries, tgt=None, ctl=()):
        """Checks the qubit lists, drains what is queued and returns (device, logical bits, least significant first)."""
        qubits = [int(q) for q in qubits]
        every = qubits + ([int(tgt)] if tgt is not None else []) + [int(c) for c in ctl]
        if len(qubits) > _TABLE_MAX_BITS:
            raise ValueError(f'{who}: {len(qubits)} selection qubits (at most {_TABLE_MAX_BITS})')
        if nentries != 1 << len(qubits):
            raise ValueError(f'{who}: a table of {nentries} entries for {len(qubits)} qubits (want {1 << len(qubits)})')
        if any(q < 0 or q >= self._nbits for q in every):
            raise ValueError(f'{who}: qubits {every} out of range for {self._nbits} qubits')
        if len(set(every)) != len(every):
            raise ValueError(f'{who}: a qubit appears twice in {every}')
        dev = self._ensure_device()
        if not hasattr(dev, method):
            raise NotImplementedError(f'{who}: {type(dev).__name__} has no {method}')
        n = self._nbits
        return dev, [n - 1 - q for q in reversed(qubits)]

    def multiplex(self, gates, sel, tgt):
        """Uniformly controlled gate: gates[s] (2^k operators of shape (2, 2)) on qubit `tgt`, s the value of the
        qubits `sel` (sel[0] the most significant bit of s).  One pass over the state for any k <= 16."""
        g = np.asarray(gates, dtype=np.complex128)
        if g.ndim != 3 or g.shape[1:] != (2, 2):
            raise ValueError(f'multiplex: gates of shape {g.shape} (want (2^k, 2, 2))')
        dev, bits = self._table_device('multiplex', 'apply_mux', sel, g.shape[0], tgt)
        dev.apply_mux(g, bits, self._nbits - 1 - int(tgt))
        self._gate_done()

    def diagonal(self, values, qubits):
        """Multiplies every amplitude by values[s], s the value of `qubits` (qubits[0] the most significant bit)."""
        v = np.asarray(values, dtype=np.complex128)
        if v.ndim != 1:
            raise ValueError(f'diagonal: values of shape {v.shape} (want (2^k,))')
        dev, bits = self._table_device('diagonal', 'apply_diag', qubits, v.shape[0])
        dev.apply_diag(v, bits)
        self._gate_done()

    @staticmethod
    def _truth_table(f, k):
        """f as 2^k values 0/1, entry s for the bits of s with xs[0] the most significant: a callable with OracleUf's
        convention (a list of bits, bits[0] the value of qubit xs[0]; evaluated 2^k times on the host) or a sequence."""
        if callable(f):
            return np.array([1 if f(helper.val2bits(s, k)) else 0 for s in range(1 << k)], dtype=np.int64)
        t = np.asarray(f).reshape(-1)
        if t.shape[0] != 1 << k or np.any((t != 0) & (t != 1)):
            raise ValueError(f'oracle: a table of {t.shape[0]} entries for {k} qubits (want {1 << k} values 0/1)')
        return t.astype(np.int64)

    def oracle(self, f, xs, y):
        """Bit oracle |x>|y> -> |x>|y xor f(x)> as a multiplexed X / I on qubit y selected by the qubits xs."""
        xs = list(xs)
        if len(xs) > _TABLE_MAX_BITS:
            raise ValueError(f'oracle: {len(xs)} input qubits (at most {_TABLE_MAX_BITS})')
        t = self._truth_table(f, len(xs))
        xi = np.stack([np.eye(2), np.array([[0.0, 1.0], [1.0, 0.0]])]).astype(np.complex128)
        self.multiplex(xi[t], xs, y)

    def phase_oracle(self, f, xs):
        """The diagonal (-1)^f(x) over the qubits xs."""
        xs = list(xs)
        if len(xs) > _TABLE_MAX_BITS:
            raise ValueError(f'phase_oracle: {len(xs)} input qubits (at most {_TABLE_MAX_BITS})')
        t = self._truth_table(f, len(xs))
        self.diagonal(1.0 - 2.0 * t, xs)

    # register permutations (reversible classical arithmetic): amplitudes moved by a table, one call each, exact to the bit
    def permutation(self, table, qubits, ctl=()):
        """|s> -> |table[s]> on the register `qubits` (qubits[0] the most significant bit of s) where every qubit of `ctl`
        is 1.  table: a bijection of range(2^k) as a sequence, or a callable on ints evaluated 2^k times on the host."""
        qubits, ctl = list(qubits), list(ctl)
        k = len(qubits)
        if not 1 <= k <= _TABLE_MAX_BITS:
            raise ValueError(f'permutation: {k} register qubits (1 to {_TABLE_MAX_BITS})')
        t = np.array([int(table(s)) for s in range(1 << k)] if callable(table) else [int(v) for v in table], dtype=np.int64)
        if t.shape != (1 << k,):
            raise ValueError(f'permutation: a table of {t.shape[0]} entries for {k} qubits (want {1 << k})')
        if np.any(t < 0) or np.any(t >= 1 << k) or np.unique(t).shape[0] != 1 << k:
            seen = {}
            for s, v in enumerate(t.tolist()):
                if not 0 <= v < 1 << k or v in seen:
                    raise ValueError(f'permutation: table[{s}] = {v} is out of range or already hit: not a bijection of range({1 << k})')
                seen[v] = s
        dev, bits = self._table_device('permutation', 'apply_perm', qubits, t.shape[0], ctl=ctl)
        mask = 0
        for c in ctl:
            mask |= 1 << (self._nbits - 1 - int(c))
        dev.apply_perm(t, bits, mask)
        self._gate_done()

    def add_const(self, a, reg, ctl=()):
        """x -> (x + a) mod 2^k on the register `reg` (reg[0] most significant); a may be negative."""
        size = 1 << len(list(reg))
        self.permutation((np.arange(size, dtype=np.int64) + int(a)) % size, reg, ctl)

    def modadd(self, a, N, reg, ctl=()):
        """x -> (x + a) mod N for x < N, identity for x >= N."""
        reg = list(reg)
        a, N, size = int(a), int(N), 1 << len(reg)
        if not 1 <= N <= size:
            raise ValueError(f'modadd: N = {N} outside [1, 2^{len(reg)}]')
        x = np.arange(size, dtype=np.int64)
        self.permutation(np.where(x < N, (x + a) % N, x), reg, ctl)

    def modmul(self, a, N, reg, ctl=()):
        """x -> a x mod N for x < N, identity for x >= N; gcd(a, N) must be 1 and N at most 2^k."""
        reg = list(reg)
        a, N, size = int(a), int(N), 1 << len(reg)
        if not 1 <= N <= size:
            raise ValueError(f'modmul: N = {N} outside [1, 2^{len(reg)}]')
        if math.gcd(a, N) != 1:
            raise ValueError(f'modmul: gcd({a}, {N}) != 1: x -> {a} x mod {N} is not reversible')
        x = np.arange(size, dtype=np.int64)
        self.permutation(np.where(x < N, (x * (a % N)) % N, x), reg, ctl)

    def add(self, src, dst):
        """|a>|b> -> |a>|(a + b) mod 2^len(dst)>, a on the qubits `src`, b on `dst`: one permutation of both registers."""
        src, dst = list(src), list(dst)
        if len(src) + len(dst) > _TABLE_MAX_BITS:
            raise ValueError(f'add: {len(src)} + {len(dst)} qubits (at most {_TABLE_MAX_BITS})')
        s = np.arange(1 << (len(src) + len(dst)), dtype=np.int64)
        a, b = s >> len(dst), s & ((1 << len(dst)) - 1)
        self.permutation((a << len(dst)) | ((a + b) & ((1 << len(dst)) - 1)), src + dst)

    # rank-one register updates (the standing of permutation: eager, one call each): a I + b |u><v| on a register, identity on
    # the rest -- reflections, Householder steps, projections onto a register state -- without ever forming a matrix
    def _rank1(self, who, qubits, u, v, a, b, ctl, sums=False):
        qubits, ctl = [int(q) for q in qubits], [int(c) for c in ctl]
        k = len(qubits)
        if v is None:                    # the uniform form: any number of qubits
            every = qubits + ctl
            if k < 1:
                raise ValueError(f'{who}: no register qubits')
            if any(q < 0 or q >= self._nbits for q in every):
                raise ValueError(f'{who}: qubits {every} out of range for {self._nbits} qubits')
            if len(set(every)) != len(every):
                raise ValueError(f'{who}: a qubit appears twice in {every}')
            dev = self._ensure_device()
            if not hasattr(dev, 'apply_rank1'):
                raise NotImplementedError(f'{who}: {type(dev).__name__} has no apply_rank1')
            bits = [self._nbits - 1 - q for q in reversed(qubits)]
        else:
            if k < 1:
                raise ValueError(f'{who}: no register qubits')
            dev, bits = self._table_device(who, 'apply_rank1', qubits, np.shape(v)[0], ctl=ctl)
        mask = 0
        for c in ctl:
            mask |= 1 << (self._nbits - 1 - c)
        out = dev.apply_rank1(bits, u=u, v=v, a=a, b=b, ctl_mask=mask, sums=sums)
        self._gate_done()
        return out

    @staticmethod
    def _rank1_vector(who, name, vec, k):
        t = np.asarray(vec, dtype=np.complex128)
        if t.shape != (1 << k,):
            raise ValueError(f'{who}: {name} of shape {t.shape} for {k} qubits (want ({1 << k},))')
        if not np.all(np.isfinite(t.real) & np.isfinite(t.imag)):
            raise ValueError(f'{who}: {name} has a non-finite entry')
        return t

    def rank_one(self, qubits, u, v=None, a=0.0, b=1.0, ctl=()):
        """a I + b |u><v| on the register `qubits` (qubits[0] the most significant bit of the vectors' index, as in diagonal)
        where every qubit of `ctl` is 1.  v=None means v = u.  Any complex a, b and any vectors: nothing is normalised."""
        qubits = list(qubits)
        tu = self._rank1_vector('rank_one', 'u', u, len(qubits))
        tv = tu if v is None else self._rank1_vector('rank_one', 'v', v, len(qubits))
        self._rank1('rank_one', qubits, None if v is None else tu, tv, complex(a), complex(b), ctl)

    def reflect(self, qubits, state=None, ctl=()):
        """The reflection 2|phi><phi| - I about a register state phi (normalised here; state=None: the uniform state) on the
        register `qubits`, where every qubit of `ctl` is 1."""
        qubits = list(qubits)
        if state is None:
            self._rank1('reflect', qubits, None, None, -1.0, 2.0, ctl)
            return
        phi = self._rank1_vector('reflect', 'state', state, len(qubits))
        nrm = float(np.linalg.norm(phi))
        if not nrm > 0:
            raise ValueError('reflect: the state is the zero vector')
        self._rank1('reflect', qubits, None, phi / nrm, -1.0, 2.0, ctl)

    def diffusion(self, reg):
        """Grover's inversion about the mean on the register `reg`: reflect(reg), i.e. H^k (2|0><0| - I) H^k."""
        self.reflect(reg)

    def project_onto(self, qubits, state=None, *, normalize=True):
        """The projector |phi><phi| (x) I for a register state phi (normalised here; state=None: the uniform state): post-
        selection of the register onto phi.  Returns the probability of finding it there (for a normalised state);
        normalize=True then rescales to norm 1 and raises ValueError where the probability is 0."""
        qubits = list(qubits)
        phi = None
        if state is not None:
            phi = self._rank1_vector('project_onto', 'state', state, len(qubits))
            nrm = float(np.linalg.norm(phi))
            if not nrm > 0:
                raise ValueError('project_onto: the state is the zero vector')
            phi = phi / nrm
        norm2, _overlap = self._rank1('project_onto', qubits, None, phi, 0.0, 1.0, (), sums=True)
        if normalize:
            self._rescale(norm2, 'project_onto')
        return float(norm2)

    # ------------------------------------------------------------------ readers / measurement
    def maxprob(self):
        """(bits, probability) of the likeliest basis state, reduced on the device."""
        if self._q_ops:
            self._drain()
        if not self._dev_ok:
            return self.psi.maxprob()
        idx, p = self._dev.argmax()
        return helper.val2bits(idx, self._nbits), p

    def ampl(self, *bits):
        if self._q_ops:
            self._drain()
        if not self._dev_ok:
            return self.psi.ampl(*bits)
        return self._dev.amplitude(helper.bits2val(bits))

    def prob(self, *bits):
        a = self.ampl(*bits)
        return np.real(np.conj(a) * a)

    def norm2(self):
        return self._ensure_device().norm2()

    # Sparse readout (extensions): short lists of (bits, amplitude, probability) straight from the device (qh_select,
    # qh_topk, qh_amplitudes) -- nothing is downloaded, so they work at sizes where qc.psi raises.  Devices without
    # select / topk / amplitudes, states still a product on the host and alias mode read qc.psi with NumPy instead.
    def _sparse_device(self):
        if self._q_ops:
            self._drain()
        dev = self._dev
        if (self._dev_ok and not self._aliased() and hasattr(dev, 'select') and hasattr(dev, 'topk')
                and hasattr(dev, 'amplitudes')):
            return dev
        return None

    @staticmethod
    def _select_checked(dev, threshold, limit, what):
        idx, amp, count, weight = dev.select(threshold, limit)
        if count > limit:
            raise ValueError(f'{what}: {count} basis states have probability >= {threshold:g} (total weight {weight:.6g}), '
                             f'more than limit = {limit}; raise the threshold or the limit')
        return np.asarray(idx, dtype=np.uint64), np.asarray(amp, dtype=np.complex128)

    def _triples(self, idx, amp):
        n = self._nbits
        return [(helper.val2bits(i, n), complex(a), float((a.conjugate() * a).real)) for i, a in zip(idx.tolist(), amp.tolist())]

    def support(self, threshold=1e-5, limit=1 << 16):
        """[(bits, amplitude, probability)] of every basis state with probability >= threshold, in index order.  More than
        `limit` of them: ValueError that names their number and total weight."""
        limit = int(limit)
        dev = self._sparse_device()
        if dev is not None:
            return self._triples(*self._select_checked(dev, float(threshold), limit, 'support'))
        a = np.asarray(self.psi, dtype=np.complex128).reshape(-1)
        p = a.real * a.real + a.imag * a.imag
        idx = np.flatnonzero(p >= threshold)
        if idx.size > limit:
            raise ValueError(f'support: {idx.size} basis states have probability >= {threshold:g} (total weight '
                             f'{float(p[idx].sum()):.6g}), more than limit = {limit}; raise the threshold or the limit')
        return self._triples(idx, a[idx])

    def top(self, k):
        """The k most probable basis states as [(bits, amplitude, probability)], most probable first, ties by ascending
        index; never one of probability 0."""
        k = int(k)
        if k < 0:
            raise ValueError(f'top: k = {k}')
        dev = self._sparse_device()
        if dev is not None:
            idx, amp = dev.topk(k)
            return self._triples(np.asarray(idx, dtype=np.uint64), np.asarray(amp, dtype=np.complex128))
        a = np.asarray(self.psi, dtype=np.complex128).reshape(-1)
        p = a.real * a.real + a.imag * a.imag
        order = np.lexsort((np.arange(p.size), -p))[:k]
        order = order[p[order] > 0]
        return self._triples(order, a[order])

    def _indices(self, states):
        n = self._nbits
        out = []
        for s in states:
            i = int(s) if isinstance(s, (int, np.integer)) else helper.bits2val(s)
            if i < 0 or i >> n:
                raise ValueError(f'basis state {s} out of range for {n} qubits')
            out.append(i)
        return np.array(out, dtype=np.uint64)

    def ampls(self, states):
        """complex128 array: the amplitudes of the basis states given as bit tuples (as qc.ampl takes them) or integer
        indices, fetched in one device call."""
        idx = self._indices(states)
        dev = self._sparse_device()
        if dev is not None:
            return np.asarray(dev.amplitudes(idx), dtype=np.complex128)
        return np.asarray(self.psi, dtype=np.complex128).reshape(-1)[idx.astype(np.int64)]

    def probs(self, states):
        """float64 array: the probabilities of those basis states."""
        a = self.ampls(states)
        return a.real * a.real + a.imag * a.imag

    def _dump_state(self, dev, desc, prob_only, limit=1 << 16):
        """What State.dump(desc, prob_only) prints, from a device selection: the same header, rows, formats and order."""
        n = self._nbits
        if not prob_only and (1 << n) > limit:
            raise ValueError(f'dump: prob_only=False would print 2^{n} basis states, more than limit = {limit}')
        # a little under State.dump's threshold, which is then applied to each row exactly as State.dump applies it (at
        # the state's own width)
        idx, amp = self._select_checked(dev, 0.99 * state.DUMP_MIN_PROB if prob_only else 0.0, limit, 'dump')
        rows = []
        for i, a in zip(idx.tolist(), amp.astype(tensor.tensor_type())):
            if prob_only and np.real(a.conj() * a) < state.DUMP_MIN_PROB:
                continue
            rows.append(state.dump_row(n, i, a))
        if desc:
            print(state.dump_header(n, desc))
        print(*rows, sep='\n')

    def measure_bit(self, idx, tostate=0, collapse=True):
        """P(qubit idx == tostate); with collapse, project and renormalise in place.

        Device-side reduction + projection kernels (the reference builds a 4^n
        density matrix: ops.py:426-460)."""
        dev = self._ensure_device()
        bit = self._nbits - 1 - idx
        prob = dev.prob_bit(bit, 1 if tostate else 0)
        if collapse:
            assert prob > 1e-20, 'Measurement collapses to 0.0.'
            dev.project_bit(bit, 1 if tostate else 0)
            dev.scale(1.0 / math.sqrt(prob))
            self._gate_done()
        # circuit.py:291-297 returns the State itself: small registers (and aliased ones, whose psi is the
        # device's own memory) get exactly that, isinstance(psi, State) included; larger ones a lazy handle
        if self._nbits <= _MEASURE_SNAPSHOT_BITS or self._aliased():
            return prob, self.psi
        return prob, _LazyPsi(self)

    # Register readout (extensions: the reference loops psi.prob(*bits) over basis states).  qubits[0] is the most
    # significant bit of a register value (np.kron order, helper.bits2val); the engine takes LOGICAL bits (qubit q is
    # bit n-1-q).  Devices without marginal / sample / project_bits read qc.psi on the host instead.
    def _register(self, qubits, what, at_most=None):
        n = self._nbits
        qubits = list(range(n)) if qubits is None else [int(q) for q in qubits]
        if any(q < 0 or q >= n for q in qubits):
            raise ValueError(f'{what}: qubits {qubits} out of range for {n} qubits')
        if len(set(qubits)) != len(qubits):
            raise ValueError(f'{what}: a qubit appears twice in {qubits}')
        if at_most is not None and len(qubits) > at_most:
            raise ValueError(f'{what}: {len(qubits)} qubits (at most {at_most})')
        return qubits

    def _register_values(self, idx, qubits):
        """Register values (uint64) of full basis indices idx."""
        n, k = self._nbits, len(qubits)
        idx = np.asarray(idx, dtype=np.uint64)
        val = np.zeros(idx.shape, dtype=np.uint64)
        for t, q in enumerate(qubits):
            val |= ((idx >> np.uint64(n - 1 - q)) & np.uint64(1)) << np.uint64(k - 1 - t)
        return val

    def probabilities(self, qubits):
        """(2^k,) float64: P(register == v) for every value v of the qubits `qubits` (k <= 16), one read of the state
        on the device (qh_marginal).  Not renormalised."""
        qubits = self._register(qubits, 'probabilities')
        n, k = self._nbits, len(qubits)
        if k > _MARGINAL_MAX_BITS:
            raise ValueError(f'probabilities: {k} qubits (at most {_MARGINAL_MAX_BITS})')
        dev = self._ensure_device()
        if hasattr(dev, 'marginal'):
            return np.asarray(dev.marginal([n - 1 - q for q in reversed(qubits)]), dtype=np.float64)
        p = np.abs(np.asarray(self.psi, dtype=np.complex128).reshape(-1)) ** 2
        out = np.zeros(1 << k, dtype=np.float64)
        np.add.at(out, self._register_values(np.arange(p.size, dtype=np.uint64), qubits).astype(np.int64), p)
        return out

    # Reduced density matrices (extensions: the reference traces a 4^n matrix, ops.TraceOut(psi.density(), ...)).  One call
    # of qh_reduced_density gives the 2^k x 2^k matrix of up to 8 qubits without downloading the state; the derived
    # quantities are host NumPy on that small matrix, divided by its trace.  A state that is still a product on the host and
    # alias mode read qc.psi with NumPy instead, and so do devices without reduced_density; any other state that is current
    # on the host only is uploaded first, as probabilities does.
    def _rho(self, qubits, what):
        """(2^k, 2^k) complex128, not normalised."""
        qubits = self._register(qubits, what, at_most=_DENSITY_MAX_BITS)
        n, k = self._nbits, len(qubits)
        if self._q_ops:
            self._drain()
        if not self._aliased() and not (self._is_product and not self._dev_ok):
            dev = self._ensure_device()
            if hasattr(dev, 'reduced_density'):
                return np.asarray(dev.reduced_density([n - 1 - q for q in reversed(qubits)]), dtype=np.complex128)
        a = np.asarray(self.psi, dtype=np.complex128).reshape((2,) * n)
        a = np.moveaxis(a, qubits, list(range(k))).reshape(1 << k, -1)
        return a @ a.conj().T

    def reduced_density(self, qubits):
        """ops.Operator (2^k, 2^k): rho = Tr_rest |psi><psi| of the qubits `qubits` (k <= 8); qubits[0] is the most
        significant bit of a row or column number, so for ascending qubits it is ops.TraceOut(psi.density(), [the other
        qubits]).  Not renormalised: the trace is the state's norm.  (An Operator has the tensor width; the quantities
        below work on the complex128 matrix.)"""
        return ops.Operator(self._rho(qubits, 'reduced_density'))

    def _unit_density(self, qubits, what):
        rho = self._rho(qubits, what)
        tr = float(np.trace(rho).real)
        if not tr > 0:
            raise ValueError(f'{what}: the state has norm 0')
        return rho / tr

    def purity(self, qubits):
        """Tr rho^2 of the qubits' reduced state (1 for a pure one, 2^-k for the maximally mixed one)."""
        rho = self._unit_density(qubits, 'purity')
        return float(np.sum(np.abs(rho) ** 2))

    def entropy(self, qubits, base=2):
        """Von Neumann entropy -Tr rho log rho of the qubits' reduced state: for a pure global state, the entanglement
        entropy between `qubits` and the rest.  Eigenvalues <= 0 contribute 0."""
        ev = np.linalg.eigvalsh(self._unit_density(qubits, 'entropy'))
        ev = ev[ev > 0]
        return float(max(0.0, -np.sum(ev * np.log(ev)) / math.log(base)))

    def schmidt_coefficients(self, qubits):
        """The Schmidt coefficients of the cut `qubits` | rest, descending: square roots of rho's eigenvalues (clipped at 0)."""
        ev = np.linalg.eigvalsh(self._unit_density(qubits, 'schmidt_coefficients'))
        return np.sqrt(np.clip(ev[::-1], 0.0, None))

    def mutual_information(self, a, b, base=2):
        """S(a) + S(b) - S(a u b) for two disjoint registers of at most 8 qubits together."""
        a, b = self._register(a, 'mutual_information'), self._register(b, 'mutual_information')
        both = self._register(a + b, 'mutual_information', at_most=_DENSITY_MAX_BITS)
        return self.entropy(a, base) + self.entropy(b, base) - self.entropy(both, base)

    def bloch(self, qubit):
        """(x, y, z) of one qubit's reduced state (helper.density_to_cartesian)."""
        return helper.density_to_cartesian(self._unit_density([qubit], 'bloch'))

    @staticmethod
    def _uniforms(count, seed, dev):
        """`count` uniforms in [0, 1): np.random.default_rng(seed), or the legacy global np.random stream for seed=None.
        A device that spans several processes (ShardedDevice) hands every rank rank 0's draws."""
        u = np.random.random_sample(count) if seed is None else np.random.default_rng(seed).random(count)
        if hasattr(dev, 'from_rank0'):
            u = np.asarray(dev.from_rank0(u), dtype=np.float64)
        return u

    def sample(self, shots, qubits=None, seed=None):
        """`shots` register values (uint64, in draw order) of the qubits `qubits` (None: all), sampled by inverse CDF on
        the device (qh_sample).  The uniforms come from np.random.default_rng(seed); seed=None draws from the legacy
        global np.random stream, so np.random.seed(...) reproduces a run."""
        qubits = self._register(qubits, 'sample')
        shots = int(shots)
        if shots < 0:
            raise ValueError(f'sample: {shots} shots')
        dev = self._ensure_device()
        u = self._uniforms(shots, seed, dev)
        order = np.argsort(u, kind='stable')
        if hasattr(dev, 'sample'):
            idx = np.asarray(dev.sample(u[order]), dtype=np.uint64)
        else:
            p = np.abs(np.asarray(self.psi, dtype=np.complex128).reshape(-1)) ** 2
            cdf = np.cumsum(p)
            if not cdf[-1] > 0:
                raise ValueError('sample: the state has norm 0')
            idx = np.minimum(np.searchsorted(cdf, u[order] * cdf[-1], side='right'), np.flatnonzero(p)[-1]).astype(np.uint64)
        out = np.empty(shots, dtype=np.uint64)
        out[order] = self._register_values(idx, qubits)
        return out

    def measure(self, qubits, *, seed=None, collapse=True):
        """One shot of the register `qubits` (k <= 16): (value, probability).  One marginal (qh_marginal: one read of the
        state) gives the register's distribution; the value is its inverse CDF, in register-value order, at one uniform
        drawn as in sample().  With collapse the state is projected on the outcome and renormalised in place
        (qh_project_bits + qh_scale)."""
        qubits = self._register(qubits, 'measure')
        n, k = self._nbits, len(qubits)
        if k > _MARGINAL_MAX_BITS:
            raise ValueError(f'measure: {k} qubits (at most {_MARGINAL_MAX_BITS})')
        probs = self.probabilities(qubits)
        nz = np.flatnonzero(probs > 0)
        if not nz.size:
            raise ValueError('measure: the state has norm 0')
        cdf = np.cumsum(probs)
        u = float(self._uniforms(1, seed, self._ensure_device())[0])
        value = int(min(int(np.searchsorted(cdf, u * cdf[-1], side='right')), int(nz[-1])))
        if probs[value] == 0:                    # (rounding at a boundary: the next value that has weight)
            value = int(nz[np.searchsorted(nz, value)])
        prob = float(probs[value])
        if collapse:
            assert prob > 1e-20, 'Measurement collapses to 0.0.'
            dev = self._ensure_device()
            mask = vbits = 0
            for t, q in enumerate(qubits):
                mask |= 1 << (n - 1 - q)
                if (value >> (k - 1 - t)) & 1:
                    vbits |= 1 << (n - 1 - q)
            if hasattr(dev, 'project_bits'):
                dev.project_bits(mask, vbits)
            else:
                for q in qubits:
                    dev.project_bit(n - 1 - q, (vbits >> (n - 1 - q)) & 1)
            dev.scale(1.0 / math.sqrt(prob))
            self._gate_done()
        return value, prob

    def release(self, qubits, value=0, *, tol=1e-9, normalize=False):
        """Give the qubits `qubits` back: the state becomes its slice at register value `value` (an int in register order,
        qubits[0] most significant, as measure() returns it -- `v, _ = qc.measure(qs); qc.release(qs, v)` -- or a sequence of
        bits), a state of len(qubits) fewer qubits, on the device (qh_release).  Returns (kept, dropped): the sums of |a|^2
        of the amplitudes kept and dropped.  The remaining qubits keep their order and are renumbered from 0: Reg objects
        handed out earlier are stale.  If tol is not None and dropped > tol * (kept + dropped) -- the qubits were not in
        |value> -- ValueError is raised and the state is as before; tol=None is post-selection.  normalize=True scales the
        result by 1/sqrt(kept).  Not recorded in the IR, like measure.  With a device that cannot release (and in aliased
        mode) the same result comes from qc.psi on the host."""
        qubits = self._register(qubits, 'release')
        n, k = self._nbits, len(qubits)
        if k < 1 or k >= n:
            raise ValueError(f'release: {k} of {n} qubits (at least one is released, at least one remains)')
        if not isinstance(value, (int, np.integer)):
            bits = [int(b) for b in value]
            if len(bits) != k or any(b not in (0, 1) for b in bits):
                raise ValueError(f'release: value {value!r} is not {k} bits')
            value = helper.bits2val(bits)
        value = int(value)
        if value < 0 or value >> k:
            raise ValueError(f'release: value {value} of {k} qubits')
        dev = self._ensure_device()
        on_device = hasattr(dev, 'release') and k <= _EXTEND_MAX_BITS and not self._alias
        if on_device:
            small, kept, dropped = dev.release([n - 1 - q for q in reversed(qubits)], value)
        else:
            amps = np.asarray(self.psi).reshape(-1)
            keep = self._register_values(np.arange(amps.size, dtype=np.uint64), qubits) == np.uint64(value)
            w = np.abs(amps.astype(np.complex128)) ** 2
            kept, dropped = float(w[keep].sum()), float(w[~keep].sum())
        if tol is not None and dropped > tol * (kept + dropped):
            if on_device:
                small.close()
            raise ValueError(f'release: qubits {qubits} are not in |{value}>: weight {dropped:.3e} of {kept + dropped:.3e} would be dropped')
        if normalize and not kept > 0:
            if on_device:
                small.close()
            raise ValueError('release: nothing is kept, nothing to normalise')
        if on_device:
            self._dev = small
            backend.release_device_state(dev)
            self._nbits = n - k
            self._host, self._host_ok = None, False
            self._factors = []
            self._product_flag = False
            if normalize:
                small.scale(1.0 / math.sqrt(kept))
        else:
            self.psi = amps[keep] / math.sqrt(kept) if normalize else amps[keep]
        self.global_reg -= k
        return kept, dropped

    def _pauli_masks(self, paulis):
        """(x, z) masks over LOGICAL bits of one Pauli string: a str over IXYZ of length nbits (character q = qubit q)
        or a dict {qubit: 'X' | 'Y' | 'Z' | 'I'}."""
        n = self._nbits
        if isinstance(paulis, str):
            if len(paulis) != n:
                raise ValueError(f'expectation: string {paulis!r} has {len(paulis)} letters for {n} qubits')
            items = enumerate(paulis)
        elif isinstance(paulis, dict):
            items = paulis.items()
        else:
            raise ValueError(f'expectation: a Pauli string is a str or a dict, not {type(paulis).__name__}')
        x = z = 0
        for q, p in items:
            if isinstance(q, bool) or not isinstance(q, (int, np.integer)) or q < 0 or q >= n:
                raise ValueError(f'expectation: qubit {q!r} out of range for {n} qubits')
            if not isinstance(p, str) or p.upper() not in ('I', 'X', 'Y', 'Z'):
                raise ValueError(f'expectation: {p!r} on qubit {q} is not one of I, X, Y, Z')
            bit = 1 << (n - 1 - int(q))
            if p.upper() in 'XY':
                x |= bit
            if p.upper() in 'ZY':
                z |= bit
        return x, z

    def expectation(self, terms, *, per_term=False):
        """sum_t c_t <psi|P_t|psi> for terms = [(c_t, paulis_t), ...] (paulis: see _pauli_masks), on the device
        (qh_expect_pauli: strings with the same X/Y positions share one read of the state).  Real coefficients give a
        float, complex ones a complex; per_term=True returns the float64 array of the <P_t> instead.  Not divided by
        the norm: like probabilities, it reports what the state holds."""
        coeffs, xs, zs = [], [], []
        for term in terms:
            try:
                c, paulis = term
            except (TypeError, ValueError):
                raise ValueError(f'expectation: term {term!r} is not a (coefficient, paulis) pair') from None
            x, z = self._pauli_masks(paulis)
            coeffs.append(complex(c))
            xs.append(x)
            zs.append(z)
        dev = self._ensure_device()
        if not xs:
            vals = np.zeros(0, dtype=np.float64)
        elif hasattr(dev, 'expect_pauli'):
            vals = np.asarray(dev.expect_pauli(xs, zs), dtype=np.float64)
        else:
            a = np.asarray(self.psi, dtype=np.complex128).reshape(-1)
            idx = np.arange(a.size, dtype=np.uint64)
            vals = np.zeros(len(xs), dtype=np.float64)
            for t, (x, z) in enumerate(zip(xs, zs)):
                par = np.zeros(a.size, dtype=np.uint64)
                for b in range(self._nbits):
                    if (z >> b) & 1:
                        par ^= (idx >> np.uint64(b)) & np.uint64(1)
                s = np.vdot(a, (1.0 - 2.0 * par.astype(np.float64)) * a[idx ^ np.uint64(x)])
                vals[t] = ((-1j) ** (bin(x & z).count('1') % 4) * s).real
        if per_term:
            return vals
        c = np.asarray(coeffs, dtype=np.complex128)
        total = complex(np.dot(c, vals)) if len(coeffs) else 0j
        return total if np.any(c.imag != 0) else float(total.real)

    # Pauli-sum operators (extensions; the reference applies an operator as a dense matrix, ops.Operator.__call__).  With a
    # device that cannot apply_pauli_sum (and in aliased mode) the same formula runs over qc.psi on the host.
    def _pauli_terms(self, terms, what):
        coeffs, xs, zs = [], [], []
        for term in terms:
            try:
                c, paulis = term
            except (TypeError, ValueError):
                raise ValueError(f'{what}: term {term!r} is not a (coefficient, paulis) pair') from None
            x, z = self._pauli_masks(paulis)
            coeffs.append(complex(c))
            xs.append(x)
            zs.append(z)
        return coeffs, xs, zs

    def _pauli_sum_host(self, coeffs, xs, zs):
        """H|psi> from qc.psi: complex128 sums, rounded once to the state's width."""
        amps = np.asarray(self.psi).reshape(-1)
        a = amps.astype(np.complex128)
        idx = np.arange(a.size, dtype=np.uint64)
        out = np.zeros(a.size, dtype=np.complex128)
        for c, x, z in zip(coeffs, xs, zs):
            par = np.zeros(a.size, dtype=np.uint64)
            for b in range(self._nbits):
                if (z >> b) & 1:
                    par ^= (idx >> np.uint64(b)) & np.uint64(1)
            out += (c * (-1j) ** (bin(x & z).count('1') % 4)) * (1.0 - 2.0 * par.astype(np.float64)) * a[idx ^ np.uint64(x)]
        return out.astype(amps.dtype)

    def _pauli_on_device(self, dev):
        return hasattr(dev, 'apply_pauli_sum') and not self._alias

    def apply_hamiltonian(self, terms, *, normalize=False):
        """self := H self for H = sum_t c_t P_t, terms = [(c_t, paulis_t), ...] as in expectation(), on the device
        (qh_pauli_sum_new: the result is a device state of its own that takes this circuit's place).  Gates queued run
        first.  Returns the norm^2 of the result, before any normalisation; normalize=True follows with
        scale(1 / sqrt(norm^2)) and raises ValueError where the result is 0 (the state is then that result).  Not recorded
        in the IR, like combine."""
        coeffs, xs, zs = self._pauli_terms(terms, 'apply_hamiltonian')
        dev = self._ensure_device()
        if self._pauli_on_device(dev):
            new, norm2 = dev.apply_pauli_sum(coeffs, xs, zs, norm=True)
            norm2 = float(norm2)
            self._dev = new
            backend.release_device_state(dev)
            self._host, self._host_ok = None, False
            self._factors = []
            self._product_flag = False
            if normalize:
                if not norm2 > 0:
                    raise ValueError('apply_hamiltonian: the result is 0, nothing to normalise')
                new.scale(1.0 / math.sqrt(norm2))
                self._gate_done()
            return norm2
        new = self._pauli_sum_host(coeffs, xs, zs)
        norm2 = float(np.vdot(new.astype(np.complex128), new.astype(np.complex128)).real)      # of the values as stored
        if normalize and not norm2 > 0:
            self.psi = new
            raise ValueError('apply_hamiltonian: the result is 0, nothing to normalise')
        self.psi = new / math.sqrt(norm2) if normalize else new
        return norm2

    def hamiltonian_times(self, terms):
        """A Snapshot holding H|self> (terms as in apply_hamiltonian); this circuit's state is unchanged.  For overlap,
        combine, project_out and restore: a Krylov step, a residual, a variance."""
        coeffs, xs, zs = self._pauli_terms(terms, 'hamiltonian_times')
        dev = self._ensure_device()
        if self._pauli_on_device(dev):
            return Snapshot(self._nbits, self._width(), dev=dev.apply_pauli_sum(coeffs, xs, zs))
        return Snapshot(self._nbits, self._width(), host=self._pauli_sum_host(coeffs, xs, zs))

    def variance(self, terms):
        """<H^2> - <H>^2 = norm2(H psi) - expectation(terms)^2 for real coefficients (ValueError otherwise).  Not divided
        by the norm: exact for a normalised state."""
        terms = list(terms)
        coeffs, xs, zs = self._pauli_terms(terms, 'variance')
        if any(c.imag != 0 for c in coeffs):
            raise ValueError('variance: real coefficients only (H must be Hermitian)')
        dev = self._ensure_device()
        if self._pauli_on_device(dev):
            w, norm2 = dev.apply_pauli_sum(coeffs, xs, zs, norm=True)
            w.close()
        else:
            new = self._pauli_sum_host(coeffs, xs, zs).astype(np.complex128)
            norm2 = float(np.vdot(new, new).real)
        return float(norm2) - float(self.expectation(terms)) ** 2

    # Pauli products (eager extensions with the standing of diagonal and permutation: not recorded in the IR).  A product of
    # factors a_t I + b_t P_t is applied in place, term 0 first (qh_apply_pauli_product: consecutive factors that act on the
    # same amplitude pairs share one pass over the state).  With a device that cannot apply_pauli_product (and in aliased
    # mode) the same factors run over qc.psi on the host.
    def _pauli_product_host(self, a, b, xs, zs):
        """prod_t (a_t I + b_t P_t) |psi> from qc.psi: complex128, rounded once to the state's width."""
        amps = np.asarray(self.psi).reshape(-1)
        v = amps.astype(np.complex128)
        idx = np.arange(v.size, dtype=np.uint64)
        for at, bt, x, z in zip(a, b, xs, zs):
            par = np.zeros(v.size, dtype=np.uint64)
            for bit in range(self._nbits):
                if (z >> bit) & 1:
                    par ^= (idx >> np.uint64(bit)) & np.uint64(1)
            v = at * v + (bt * (-1j) ** (bin(x & z).count('1') % 4)) * (1.0 - 2.0 * par.astype(np.float64)) * v[idx ^ np.uint64(x)]
        return v.astype(amps.dtype)

    def _pauli_product(self, a, b, xs, zs, norm=False):
        """Applies the factors; norm=True returns the norm^2 of the result as stored (the device then sums it in the last
        pass and the host waits for it; without it the call is queued on the stream like a gate)."""
        dev = self._ensure_device()
        if hasattr(dev, 'apply_pauli_product') and not self._alias:
            norm2 = dev.apply_pauli_product(a, b, xs, zs, norm=norm)
            self._gate_done()
            return float(norm2) if norm else None
        new = self._pauli_product_host(a, b, xs, zs)
        self.psi = new
        return float(np.vdot(new.astype(np.complex128), new.astype(np.complex128)).real) if norm else None

    def _rescale(self, norm2, what):
        if not norm2 > 0:
            raise ValueError(f'{what}: the result is 0, nothing to normalise')
        dev = self._ensure_device()
        if hasattr(dev, 'scale') and not self._alias:
            dev.scale(1.0 / math.sqrt(norm2))
            self._gate_done()
        else:
            self.psi = np.asarray(self.psi).reshape(-1) / math.sqrt(norm2)

    def pauli_rot(self, paulis, theta):
        """exp(-i theta/2 P) for one Pauli string (see _pauli_masks), the convention of rx / ry / rz:
        pauli_rot({q: 'X'}, t) is rx(q, t).  One pass over the state whatever the weight of the string."""
        x, z = self._pauli_masks(paulis)
        theta = float(theta)
        self._pauli_product([math.cos(theta / 2)], [-1j * math.sin(theta / 2)], [x], [z])

    def apply_pauli(self, paulis):
        """The Pauli string itself: amplitudes are moved, negated and multiplied by +-i only, so the result is exact."""
        x, z = self._pauli_masks(paulis)
        self._pauli_product([0.0], [1.0], [x], [z])

    def evolve(self, terms, t, *, steps=1, order=1):
        """prod_t exp(-i (t / steps) c_t P_t), repeated `steps` times, for terms = [(c_t, paulis_t), ...] with real c_t: a
        Trotter step of H = sum_t c_t P_t.  The terms stay in the caller's order (the first is applied first); order=2 is
        the palindromic sequence with half angles.  All steps go to the device in one call."""
        coeffs, xs, zs = self._pauli_terms(terms, 'evolve')
        if any(c.imag != 0 for c in coeffs):
            raise ValueError('evolve: real coefficients only (H must be Hermitian)')
        if isinstance(steps, bool) or not isinstance(steps, (int, np.integer)) or steps < 1:
            raise ValueError(f'evolve: steps = {steps!r} (want an int >= 1)')
        if order not in (1, 2):
            raise ValueError(f'evolve: order = {order!r} (want 1 or 2)')
        dt = float(t) / int(steps)
        seq = list(range(len(coeffs)))
        if order == 2:
            seq, dt = seq + seq[::-1], dt / 2
        seq = seq * int(steps)
        a = [math.cos(dt * coeffs[k].real) for k in seq]
        b = [-1j * math.sin(dt * coeffs[k].real) for k in seq]
        self._pauli_product(a, b, [xs[k] for k in seq], [zs[k] for k in seq])

    def imaginary_time(self, terms, tau, *, steps=1, normalize=True):
        """prod_t exp(-(tau / steps) c_t P_t), repeated `steps` times (factors cosh - sinh P; real c_t).  Returns the
        norm^2 of the result before any normalisation; normalize=True follows with scale(1 / sqrt(norm^2)) and raises
        ValueError where the result is 0."""
        coeffs, xs, zs = self._pauli_terms(terms, 'imaginary_time')
        if any(c.imag != 0 for c in coeffs):
            raise ValueError('imaginary_time: real coefficients only (H must be Hermitian)')
        if isinstance(steps, bool) or not isinstance(steps, (int, np.integer)) or steps < 1:
            raise ValueError(f'imaginary_time: steps = {steps!r} (want an int >= 1)')
        dt = float(tau) / int(steps)
        seq = list(range(len(coeffs))) * int(steps)
        norm2 = self._pauli_product([math.cosh(dt * coeffs[k].real) for k in seq], [-math.sinh(dt * coeffs[k].real) for k in seq],
                                    [xs[k] for k in seq], [zs[k] for k in seq], norm=True)
        if normalize:
            self._rescale(norm2, 'imaginary_time')
        return norm2

    def pauli_project(self, paulis, eigenvalue=+1, *, normalize=True):
        """The projector (I + eigenvalue P) / 2 onto an eigenspace of one Pauli string: a stabiliser measurement with a
        chosen outcome.  Returns the norm^2 of the projected state -- the probability of that outcome for a normalised
        state; normalize=True then rescales to norm 1 and raises ValueError where the probability is 0."""
        if eigenvalue not in (1, -1):
            raise ValueError(f'pauli_project: eigenvalue = {eigenvalue!r} (want +1 or -1)')
        x, z = self._pauli_masks(paulis)
        norm2 = self._pauli_product([0.5], [0.5 * int(eigenvalue)], [x], [z], norm=True)
        if normalize:
            self._rescale(norm2, 'pauli_project')
        return norm2

    # Diagonal Z-polynomial operators (eager extensions with the standing of diagonal and evolve: not recorded in the IR).  A
    # classical cost function C = sum_t w_t Z..Z is one multiplication per amplitude (qh_apply_zpoly) and one read for
    # <C> and <C^2> (qh_expect_zpoly), whatever the number of terms.  With a device that has no apply_zpoly (and in aliased
    # mode) the same formula runs over qc.psi on the host.
    def _zpoly_terms(self, terms, what):
        coeffs, xs, zs = self._pauli_terms(terms, what)
        if any(x for x in xs):
            raise ValueError(f'{what}: Z and I only (a cost function is diagonal)')
        if any(c.imag != 0 for c in coeffs):
            raise ValueError(f'{what}: real weights only')
        return [c.real for c in coeffs], zs

    def _zpoly_host_f(self, ws, zs):
        """f(i) over every index, float64"""
        idx = np.arange(1 << self._nbits, dtype=np.uint64)
        f = np.zeros(idx.size, dtype=np.float64)
        for w, z in zip(ws, zs):
            par = np.zeros(idx.size, dtype=np.uint64)
            for bit in range(self._nbits):
                if (z >> bit) & 1:
                    par ^= (idx >> np.uint64(bit)) & np.uint64(1)
            f += w * (1.0 - 2.0 * par.astype(np.float64))
        return f

    def _zpoly(self, ws, zs, c, norm=False):
        dev = self._ensure_device()
        if hasattr(dev, 'apply_zpoly') and not self._alias:
            norm2 = dev.apply_zpoly(ws, zs, c, norm=norm)
            self._gate_done()
            return float(norm2) if norm else None
        amps = np.asarray(self.psi).reshape(-1)
        new = (amps.astype(np.complex128) * np.exp(complex(c) * self._zpoly_host_f(ws, zs))).astype(amps.dtype)
        self.psi = new
        return float(np.vdot(new.astype(np.complex128), new.astype(np.complex128)).real) if norm else None

    def phase_polynomial(self, terms, gamma):
        """exp(-i gamma C) for C = sum_t w_t P_t, terms = [(w_t, paulis_t), ...] with Z and I only and real w_t: the QAOA
        cost layer, one pass over the state."""
        ws, zs = self._zpoly_terms(terms, 'phase_polynomial')
        self._zpoly(ws, zs, complex(0.0, -float(gamma)))

    def cost_filter(self, terms, tau, normalize=True):
        """exp(-tau C): imaginary time under a classical cost.  Returns the norm^2 of the result before any normalisation;
        normalize=True follows with scale(1 / sqrt(norm^2)) and raises ValueError where the result is 0."""
        ws, zs = self._zpoly_terms(terms, 'cost_filter')
        norm2 = self._zpoly(ws, zs, complex(-float(tau), 0.0), norm=True)
        if normalize:
            self._rescale(norm2, 'cost_filter')
        return norm2

    def cost_expectation(self, terms, moments=False):
        """<C>, or (<C>, <C^2>) with moments=True, in one read of the state.  Not divided by the norm, like expectation."""
        ws, zs = self._zpoly_terms(terms, 'cost_expectation')
        dev = self._ensure_device()
        if hasattr(dev, 'expect_zpoly') and not self._alias:
            _, mean, second = dev.expect_zpoly(ws, zs)
        else:
            a = np.asarray(self.psi).reshape(-1).astype(np.complex128)
            p, f = a.real * a.real + a.imag * a.imag, self._zpoly_host_f(ws, zs)
            mean, second = float(np.dot(p, f)), float(np.dot(p, f * f))
        return (float(mean), float(second)) if moments else float(mean)

    @staticmethod
    def maxcut_terms(edges):
        """[(u, v, w), ...] -> the terms w Z_u Z_v of a MaxCut cost function"""
        terms = []
        for e in edges:
            try:
                u, v, w = e
            except (TypeError, ValueError):
                raise ValueError(f'maxcut_terms: edge {e!r} is not (u, v, w)') from None
            if u == v:
                raise ValueError(f'maxcut_terms: edge {e!r} joins a node to itself')
            terms.append((float(w), {int(u): 'Z', int(v): 'Z'}))
        return terms

    def qaoa_layer(self, terms, gamma, beta):
        """One QAOA layer: exp(-i gamma C), then the mixer rx(q, 2 beta) = exp(-i beta X_q) on every qubit through the
        normal queue."""
        self.phase_polynomial(terms, gamma)
        for q in range(self._nbits):
            self.rx(q, 2.0 * float(beta))

    # Two states (extensions; the reference compares states on the host: State.diff, the swap and Hadamard tests).  With a
    # device that cannot clone / copy_from / inner, the amplitudes go through qc.psi on the host instead.
    def snapshot(self):
        """A Snapshot of the state as it is now (qh_clone: queued gates run first, one device-to-device copy)."""
        dev = self._ensure_device()
        if hasattr(dev, 'clone'):
            return Snapshot(self._nbits, self._width(), dev=dev.clone())
        return Snapshot(self._nbits, self._width(), host=np.array(self.psi, dtype=tensor.tensor_type()).reshape(-1))

    def _same_shape(self, other, what):
        if not isinstance(other, (qc, Snapshot)):
            raise ValueError(f'{what}: a qc or a Snapshot, not {type(other).__name__}')
        width = other.width if isinstance(other, Snapshot) else other._width()      # pylint: disable=protected-access
        if other.nbits != self._nbits or width != self._width() or self._nbits == 0:
            raise ValueError(f'{what}: {other.nbits} qubits at width {width} against {self._nbits} at width {self._width()}')
        if isinstance(other, Snapshot) and other._dev is None and other._host is None:      # pylint: disable=protected-access
            raise ValueError(f'{what}: the snapshot has been closed')

    def restore(self, snap):
        """The state := the snapshot's (qh_copy).  Gates still queued, on the host side or in the engine, are dropped."""
        if not isinstance(snap, Snapshot):
            raise ValueError(f'restore: a Snapshot, not {type(snap).__name__}')
        self._same_shape(snap, 'restore')
        self._q_ops, self._q_gates = [], []
        dev = self._ensure_device()
        if snap._dev is not None and hasattr(dev, 'copy_from'):      # pylint: disable=protected-access
            dev.copy_from(snap._dev)                                   # pylint: disable=protected-access
        else:
            host = snap._host if snap._host is not None else snap._dev.download()      # pylint: disable=protected-access
            dev.upload(np.asarray(host))
        # neither the product description nor a host copy describes the state any more (as _drain)
        self._product_flag = False
        self._host_ok = False
        if self._aliased():
            self._dev.sync()

    @staticmethod
    def _host_amps(other):
        if isinstance(other, qc):
            return np.asarray(other.psi).reshape(-1)
        if other._host is not None:      # pylint: disable=protected-access
            return other._host           # pylint: disable=protected-access
        return other._dev.download()     # pylint: disable=protected-access

    def overlap(self, other):
        """complex <self|other> for another circuit or a Snapshot of the same size and width, on the device (qh_inner:
        both states are read where they lie).  Not divided by the norms."""
        self._same_shape(other, 'overlap')
        dev = self._ensure_device()
        odev = other._ensure_device() if isinstance(other, qc) else other._dev      # pylint: disable=protected-access
        if hasattr(dev, 'inner') and odev is not None and hasattr(odev, 'inner'):
            return complex(dev.inner(odev))
        return complex(np.vdot(np.asarray(self.psi).reshape(-1), self._host_amps(other)))

    def fidelity(self, other):
        """|<self|other>|^2 / (|self|^2 |other|^2)."""
        ov = self.overlap(other)
        na = self.overlap(self).real
        if isinstance(other, qc):
            nb = other.overlap(other).real
        elif other._dev is not None and hasattr(other._dev, 'inner'):      # pylint: disable=protected-access
            nb = other._dev.inner(other._dev).real                          # pylint: disable=protected-access
        else:
            nb = float(np.vdot(self._host_amps(other), self._host_amps(other)).real)
        return float(abs(ov) ** 2 / (na * nb))

    def combine(self, other, alpha=1.0, beta=1.0, *, normalize=False):
        """self := alpha * self + beta * other for another circuit or a Snapshot of the same size and width, on the device
        (qh_axpby: in place, both states read where they lie; other is unchanged).  Gates queued on either side run first.
        Returns the norm^2 of the result, before any normalisation; normalize=True follows with scale(1 / sqrt(norm^2)) and
        raises ValueError where the result is 0 (the state is then that result).  Not recorded in the IR, like restore."""
        self._same_shape(other, 'combine')
        if other is self:
            raise ValueError('combine: other is this circuit (scale it instead)')
        alpha, beta = complex(alpha), complex(beta)
        dev = self._ensure_device()
        odev = other._ensure_device() if isinstance(other, qc) else other._dev      # pylint: disable=protected-access
        if hasattr(dev, 'axpby') and odev is not None and hasattr(odev, 'axpby'):
            norm2 = float(dev.axpby(alpha, odev, beta, norm=True))
            # neither the product description nor a host copy describes the state any more (as restore)
            self._product_flag = False
            self._host_ok = False
            if self._aliased():
                self._dev.sync()
            if normalize:
                if not norm2 > 0:
                    raise ValueError('combine: the result is 0, nothing to normalise')
                dev.scale(1.0 / math.sqrt(norm2))
                self._gate_done()
            return norm2
        amps = np.asarray(self.psi).reshape(-1)
        new = (alpha * amps.astype(np.complex128) + beta * np.asarray(self._host_amps(other)).reshape(-1).astype(np.complex128)).astype(amps.dtype)
        norm2 = float(np.vdot(new.astype(np.complex128), new.astype(np.complex128)).real)      # of the values as stored, in double
        if normalize and not norm2 > 0:
            self.psi = new
            raise ValueError('combine: the result is 0, nothing to normalise')
        self.psi = new / math.sqrt(norm2) if normalize else new
        return norm2

    def project_out(self, other):
        """Remove other's component from this state (one Gram-Schmidt step): c = <other|self> / <other|other>,
        self -= c * other; returns c.  ValueError where <other|other> is 0."""
        self._same_shape(other, 'project_out')
        if other is self:
            raise ValueError('project_out: other is this circuit')
        if isinstance(other, qc):
            ov, nn = other.overlap(self), other.overlap(other).real
        else:
            ov = complex(np.conj(self.overlap(other)))
            if other._dev is not None and hasattr(other._dev, 'inner'):      # pylint: disable=protected-access
                nn = other._dev.inner(other._dev).real                          # pylint: disable=protected-access
            else:
                nn = float(np.vdot(self._host_amps(other), self._host_amps(other)).real)
        if not nn > 0:
            raise ValueError('project_out: <other|other> is 0')
        c = ov / nn
        self.combine(other, 1.0, -c)
        return c

    # Matrix elements between two states (extensions).  <a|P|b> for a Pauli string between two states that both live in HBM
    # is one read of each (qh_transition_pauli); without the call on the device, and in aliased mode, the same formula runs
    # on the host.
    @staticmethod
    def _pauli_string_host(v, x, z):
        """P v for one Pauli string as (x, z) masks over LOGICAL bits: (P v)_i = (-i)^nY (-1)^popcount(i & z) v_{i ^ x},
        complex128."""
        v = np.asarray(v).reshape(-1).astype(np.complex128)
        idx = np.arange(v.size, dtype=np.uint64)
        par = np.zeros(v.size, dtype=np.uint64)
        for bit in range(max(int(z).bit_length(), 1)):
            if (z >> bit) & 1:
                par ^= (idx >> np.uint64(bit)) & np.uint64(1)
        return (-1j) ** (bin(x & z).count('1') % 4) * (1.0 - 2.0 * par.astype(np.float64)) * v[idx ^ np.uint64(x)]

    def matrix_element(self, other, terms, *, per_term=False):
        """complex sum_t c_t <self|P_t|other> for terms = [(c_t, paulis_t), ...] as in expectation() and another circuit or
        a Snapshot of the same size and width (other may be this circuit), in one device call for the whole list
        (qh_transition_pauli: both states are read where they lie, strings with the same X/Y positions share a read).
        per_term=True returns the complex128 array of the <self|P_t|other> instead.  Not divided by the norms."""
        self._same_shape(other, 'matrix_element')
        coeffs, xs, zs = self._pauli_terms(terms, 'matrix_element')
        dev = self._ensure_device()
        if other is self:
            odev = dev
        else:
            odev = other._ensure_device() if isinstance(other, qc) else other._dev      # pylint: disable=protected-access
        aliased = self._alias or (isinstance(other, qc) and other._alias)      # pylint: disable=protected-access
        on_device = odev is not None and not aliased
        if not xs:
            vals = np.zeros(0, dtype=np.complex128)
        elif on_device and hasattr(dev, 'transition_pauli') and hasattr(odev, 'transition_pauli'):
            vals = np.asarray(dev.transition_pauli(odev, xs, zs), dtype=np.complex128)
        elif on_device and hasattr(dev, 'inner') and hasattr(odev, 'inner') and hasattr(odev, 'apply_pauli_sum'):
            vals = np.zeros(len(xs), dtype=np.complex128)
            for t, (x, z) in enumerate(zip(xs, zs)):
                w = odev.apply_pauli_sum([1.0], [x], [z])
                try:
                    vals[t] = complex(dev.inner(w))
                finally:
                    w.close()
        else:
            a = np.asarray(self.psi).reshape(-1).astype(np.complex128)
            b = a if other is self else np.asarray(self._host_amps(other)).reshape(-1)
            vals = np.array([np.vdot(a, self._pauli_string_host(b, x, z)) for x, z in zip(xs, zs)], dtype=np.complex128)
        if per_term:
            return vals
        return complex(np.dot(np.asarray(coeffs, dtype=np.complex128), vals)) if coeffs else 0j

    def rotation_gradients(self, rotations, terms):
        """Applies exp(-i theta_k/2 P_k) for rotations = [(paulis_k, theta_k), ...] in order, exactly as pauli_rot would, and
        returns (E, grad): E = expectation(terms) on the rotated state, which the circuit keeps, and the float64 array
        grad[k] = dE/dtheta_k, by the adjoint method.  terms is a Hamiltonian with real coefficients (ValueError otherwise).

        With phi_k the state after rotation k and lam_k = (U_{K-1} ... U_{k+1})^+ H |phi_{K-1}>,
            dE/dtheta_k = 2 Re <lam_k| (-i/2) P_k |phi_k> = Im <lam_k|P_k|phi_k>.
        lam := hamiltonian_times(terms) and phi := snapshot() are un-evolved in step, exp(+i theta_k/2 P_k) on both, from
        k = K - 1 down: one matrix element and two in-place passes per rotation, against the 2K circuit executions of the
        parameter-shift rule.  The two scratch states are closed before returning.  Not recorded in the IR, like evolve."""
        terms = list(terms)
        coeffs, hx, hz = self._pauli_terms(terms, 'rotation_gradients')
        if any(c.imag != 0 for c in coeffs):
            raise ValueError('rotation_gradients: real coefficients only (H must be Hermitian)')
        rots = []
        for rot in rotations:
            try:
                paulis, theta = rot
            except (TypeError, ValueError):
                raise ValueError(f'rotation_gradients: rotation {rot!r} is not a (paulis, theta) pair') from None
            rots.append(self._pauli_masks(paulis) + (float(theta),))
        for x, z, theta in rots:
            self._pauli_product([math.cos(theta / 2)], [-1j * math.sin(theta / 2)], [x], [z])
        energy = self.expectation(terms)
        grad = np.zeros(len(rots), dtype=np.float64)
        dev = self._ensure_device()
        if not self._alias and all(hasattr(dev, m) for m in ('transition_pauli', 'apply_pauli_sum', 'apply_pauli_product', 'clone')):
            lam = dev.apply_pauli_sum(coeffs, hx, hz)
            phi = None
            try:
                phi = dev.clone()
                for k in range(len(rots) - 1, -1, -1):
                    x, z, theta = rots[k]
                    grad[k] = complex(lam.transition_pauli(phi, [x], [z])[0]).imag
                    if k:
                        a, b = [math.cos(theta / 2)], [1j * math.sin(theta / 2)]
                        lam.apply_pauli_product(a, b, [x], [z])
                        phi.apply_pauli_product(a, b, [x], [z])
            finally:
                lam.close()
                if phi is not None:
                    phi.close()
            return energy, grad
        phi = np.asarray(self.psi).reshape(-1).astype(np.complex128)
        lam = np.zeros(phi.size, dtype=np.complex128)
        for c, x, z in zip(coeffs, hx, hz):
            lam += c * self._pauli_string_host(phi, x, z)
        for k in range(len(rots) - 1, -1, -1):
            x, z, theta = rots[k]
            grad[k] = complex(np.vdot(lam, self._pauli_string_host(phi, x, z))).imag
            if k:
                a, b = math.cos(theta / 2), 1j * math.sin(theta / 2)
                lam = a * lam + b * self._pauli_string_host(lam, x, z)
                phi = a * phi + b * self._pauli_string_host(phi, x, z)
        return energy, grad

    def pauli_expectation(self, idx):
        p0, _ = self.measure_bit(idx, 0, False)
        return p0 - (1 - p0)

    # ------------------------------------------------------------------ composite gates
    def swap(self, idx0, idx1):
        # pylint: disable=arguments-out-of-order
        with self.scope(self.ir, f'swap({idx0}, {idx1})'):
            self.cx(idx1, idx0)
            self.cx(idx0, idx1)
            self.cx(idx1, idx0)

    def cswap(self, ctl, idx0, idx1):
        with self.scope(self.ir, f'cswap({ctl}, {idx0}, {idx1})'):
            self.cx(idx1, idx0)
            self.ccx(ctl, idx0, idx1)
            self.cx(idx1, idx0)

    def qft(self, reg, with_swaps=False):
        """Quantum Fourier transform over `reg` (gate order of circuit.py:320-328)."""
        for i in reversed(range(len(reg))):
            self.h(reg[i])
            for j in reversed(range(i)):
                self.cu1(reg[i], reg[j], np.pi / 2 ** (i - j))
        if with_swaps:
            self.flip(reg)

    def inverse_qft(self, reg, with_swaps=False):
        if with_swaps:
            self.flip(reg)
        last = len(reg) - 1
        for pos, r in enumerate(reg):
            self.h(r)
            if pos != last:
                for y in range(pos, -1, -1):
                    self.cu1(reg[pos + 1], reg[y], -np.pi / 2 ** (pos + 1 - y))

    def multi_control(self, ctl, idx1, aux, gate, desc=''):
        """Gate on idx1 controlled by all of ctl, using len(ctl)-1 ancillae (circuit.py:341-392)."""
        if aux:
            assert len(aux) >= len(ctl) - 1, 'Incorrect number of ancilla qubits.'
        with self.scope(self.ir, f'multi-{gate.name}({ctl}, {idx1}) # {desc})'):
            if not ctl:
                self.apply1(gate, idx1, desc)
                return
            ctl = list(ctl)
            if len(ctl) == 1:
                self.applyc(gate, ctl[0], idx1, desc)
                return
            if len(ctl) == 2:
                self.ccu(ctl[0], ctl[1], idx1, gate, desc)
                return
            # AND the controls into the ancilla ladder, fire, then uncompute
            self.ccx(ctl[0], ctl[1], aux[0])
            top = 0
            for c in ctl[2:]:
                self.ccx(c, aux[top], aux[top + 1])
                top += 1
            self.applyc(gate, aux[top], idx1, desc)
            for c in reversed(ctl[2:]):
                top -= 1
                self.ccx(c, aux[top], aux[top + 1])
            self.ccx(ctl[0], ctl[1], aux[0])

    def flip(self, reg):
        for i in range(len(reg) // 2):
            self.swap(reg[i], reg[len(reg) - 1 - i])

    # ------------------------------------------------------------------ circuits of circuits
    def qc(self, qc_parm, offset=0):
        """Replay another circuit's IR on this circuit, shifted by `offset`."""
        for node in qc_parm.ir.gates:
            if node.is_single():
                self.apply1(node.gate, node.idx0 + offset, node.name, val=node.val)
            if node.is_ctl():
                self.applyc(node.gate, node.ctl + offset, node.idx1 + offset, node.name, val=node.val)

    def run(self):
        """Execute the recorded IR now (without recording it again)."""
        saved = self.build_ir, self.eager
        self.build_ir, self.eager = False, True
        self.qc(self)
        self.build_ir, self.eager = saved

    def inverse(self):
        """A new non-eager circuit with the adjoint gates in reverse order."""
        newqc = qc(self.name, eager=False)
        for node in reversed(self.ir.gates):
            val = -node.val if node.val else None
            if node.is_single():
                newqc.apply1(node.gate.adjoint(), node.idx0, node.name + '*', val=val)
            if node.is_ctl():
                newqc.applyc(node.gate.adjoint(), node.ctl, node.idx1, node.name + '*', val=val)
        return newqc

    def control_by(self, ctl):
        """Make every recorded gate additionally controlled by qubit `ctl`."""
        assert not self.eager, 'control_by() used in non-eager circuit.'
        res = ir.Ir()
        for node in self.ir.gates:
            if node.is_single():
                node.to_ctl(ctl)
                res.add_node(node)
            elif node.is_ctl():
                sub = qc('multi', eager=False)
                sub.multi_control([ctl, node.ctl], node.idx1, None, node.gate, node.desc)
                for inner in sub.ir.gates:
                    res.add_node(inner)
        self.ir = res

    def sub(self, name=''):
        made = qc(f'inner_{self.sub_circuits}{name}', eager=False)
        self.sub_circuits += 1
        return made

    # ------------------------------------------------------------------ debug / output
    def stats(self):
        return f'Circuit Statistics\n  Qubits: {self.nbits}\n  Gates : {self.ir.ngates}\n'

    def dump_to_file(self):
        """Text emitters (qasm/libq/cirq/latex) are outside the accelerated path."""
        if _dump_flags_set():
            raise NotImplementedError('circuit text dumpers are not part of qcc_amd (hot path only)')

    def dump(self, *, desc=None, draw=False, pstate=True):
        if desc:
            print(desc)
        if self.name:
            print(f'Circuit: {self.name}, Gates: {len(self.ir.gates)}, QBits: {self.nbits}')
        print(self.ir, end='')
        if pstate:
            dev = self._sparse_device() if self._nbits else None
            if dev is not None:
                self._dump_state(dev, 'Current state', True)
            else:
                self.psi.dump('Current state')

    def sync(self):
        """Wait for all queued device work (for timing)."""
        if self._q_ops:
            self._drain()
        if self._dev is not None:
            self._dev.sync()

    def close(self):
        """Give the device state back (to the per-process pool of qcc_amd.lib.backend: the next circuit of the same
        shape reuses its buffers instead of allocating 2 x 16 GiB again).  Also runs when the circuit is collected."""
        self._q_ops, self._q_gates = [], []
        if self._dev is not None:
            if not self._alias:
                backend.release_device_state(self._dev)
            self._dev, self._dev_ok = None, False

    def __del__(self):
        try:
            self.close()
        except Exception:  # pylint: disable=broad-except
            pass
