/*
 * qcc_hip.h -- C-ABI of the MI355X (gfx950) state-vector gate-application engine.
 *
 * This is the drop-in boundary for the hot path of qcc4cp/qcc: the two native
 * entry points of the reference's `libxgates` CPython extension
 *
 *     apply1(psi, gate, nbits, tgt, bit_width)        src/lib/xgates.cc:89-107
 *     applyc(psi, gate, nbits, ctl, tgt, bit_width)   src/lib/xgates.cc:126-145
 *
 * (templates apply1<> :23-41 and applyc<> :45-67; only callers are
 * qc.apply1/qc.applyc, src/lib/circuit.py:180-215).  Everything here is plain
 * C: opaque handle, raw pointers, sizes and ints.  No torch / numpy / Python
 * types cross this boundary.  INTEGRATION.md shows the binding a maintainer of
 * the reference adds (a `libxgates` module over ctypes).
 *
 * Conventions kept from the reference
 *   - amplitudes are interleaved (re,im), C-contiguous, length 2^nbits,
 *     complex128 when bit_width==128, complex64 when bit_width==64
 *     (src/lib/tensor.py:42-46); gates are 4 complex numbers, row-major
 *     [a b c d] (xgates.cc:18-21), ALWAYS passed here as 8 doubles;
 *   - qubit numbers in qh_apply1/qh_applyc/qh_host_* are the reference's
 *     big-endian qubit indices: qubit q is index bit (nbits-1-q)
 *     (xgates.cc:26,48-49);
 *   - updates are in place.
 * Deliberate differences
 *   - 64-bit indices (reference: int, breaks at 31 qubits, xgates.cc:27,33);
 *   - errors are returned as status codes + qh_last_error(), never exit()
 *     (reference: exit(EXIT_FAILURE), xgates.cc:28-32);
 *   - the state may live in HBM behind a handle across calls (the reference
 *     borrows a host NumPy buffer per call); qh_host_apply1/applyc keep the
 *     borrow-a-host-buffer contract for literal drop-in use.
 *
 * Threading: one host thread per handle.  Work is asynchronous on the handle's
 * HIP stream; qh_sync() waits.  All readers synchronise internally.
 */
#ifndef QCC_HIP_H_
#define QCC_HIP_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct qh_state_s *qh_handle;

/* status codes */
#define QH_OK 0
#define QH_ERR_BAD_QUBIT 1      /* qubit / bit position out of range            */
#define QH_ERR_SAME_QUBIT 2     /* control == target                            */
#define QH_ERR_BAD_DTYPE 3      /* bit_width not 64 / 128                       */
#define QH_ERR_HIP 4            /* a HIP runtime call failed (see last_error)   */
#define QH_ERR_ARG 5            /* NULL pointer, bad size, bad handle           */
#define QH_ERR_NOMEM 6          /* device allocation failed                     */
#define QH_ERR_NO_DEVICE 7      /* no gfx950 device visible                     */
#define QH_ERR_NONLOCAL 8       /* non-diagonal gate targets a bit held by the
                                   shard index: exchange first (qh_exchange_*)  */
#define QH_ERR_COMM 9           /* RCCL / transport failure (see last_error)    */

/* fusion levels for qh_set_fusion */
#define QH_FUSE_OFF 0           /* one kernel per gate, launched immediately    */
#define QH_FUSE_SWEEP 1         /* queue gates, plan register-tile sweeps       */

const char *qh_last_error(void);
int qh_version(void);
int qh_device_count(int *count);

/* ---- state lifetime ----------------------------------------------------- */
/* Allocate 2^nbits amplitudes in HBM on `device` (own HIP stream).           */
int qh_create(int nbits, int bit_width, int device, qh_handle *out);
/* Use caller-owned device memory / stream (e.g. a torch allocation and
 * torch's current stream, passed as raw pointers).  stream may be NULL
 * (engine creates its own).                                                  */
int qh_attach(int nbits, int bit_width, int device, void *device_ptr,
              void *hip_stream, qh_handle *out);
/* The state in pinned host memory the GPU works on directly (zero copy): for SMALL registers whose
 * owner wants the reference's contract literally -- apply1/applyc mutate the caller-visible buffer in
 * place (xgates.cc:37-38) and every holder of that buffer sees it.  qh_host_ptr gives the host
 * address (valid until qh_destroy; read it after qh_sync).  Every gate crosses PCIe: <= 28 qubits.   */
int qh_create_host_mapped(int nbits, int bit_width, int device, qh_handle *out);
int qh_host_ptr(qh_handle h, void **host_ptr);   /* NULL for states that live in HBM */
/* Planner-only handle: no device, no memory.  Gates can be queued and the
 * plan inspected with qh_plan_json (used by CPU-side tests).                 */
int qh_create_dry(int nbits, int bit_width, qh_handle *out);
int qh_destroy(qh_handle h);

/* Multi-GPU sharding: this handle holds the 2^nbits amplitudes whose global
 * index has high bits == shard_index, out of a 2^nbits_global state.  Gates
 * are then addressed in GLOBAL qubit numbers / bit positions.               */
int qh_set_shard(qh_handle h, int nbits_global, uint64_t shard_index);
/* Device pointer of the shard, amplitudes in physical order.  A handle that owns its memory may
 * re-lay the state out between two buffers while sweeps run (planner.h, relayout): this call
 * brings it back to canonical order first and, from then on, keeps the state in that one buffer
 * (as qh_set_relayout(h, 0) does): the pointer stays valid for the life of the handle.        */
int qh_device_ptr(qh_handle h, void **ptr);
/* Relayout sweeps (a second buffer of the state's size; planner.h): on = 1 allocates it now, on = 0 runs what is
 * queued, returns the layout to canonical order and frees it.  *actual (may be NULL) = the resulting mode.
 * Default: decided at the first flush (on if the handle owns its memory and the buffer fits).  A handle with a
 * communicator of SEVERAL ranks starts with relayout off: every rank must hold the same layout when they exchange,
 * so the caller turns it on only after all ranks report that they can (qcc_amd/sharded.py).                  */
int qh_set_relayout(qh_handle h, int on, int *actual);
int qh_stream(qh_handle h, void **stream);
int qh_nbits(qh_handle h, int *nbits_local, int *nbits_global);

/* ---- initialisation and host <-> device --------------------------------- */
/* |index> in global logical index space (zero elsewhere).                    */
int qh_init_basis(qh_handle h, uint64_t index);
/* Product state f_0 (x) f_1 (x) ... (x) f_{k-1} (np.kron order: f_0 on the most significant
 * qubits), built on the device -- what qc.reg/qubit/bitstring/state() build with
 * np.kron on the host (src/lib/circuit.py:121-164, state.py:185-246).
 * Factor j spans nq[j] qubits (sum == nbits_global) and is a table of 2^nq[j]
 * complex128 amplitudes (amps[j], interleaved re,im; nq[j] <= 24) or, where amps is NULL
 * or amps[j] is NULL, the basis state |basis[j]>.  At most 32 factors.           */
int qh_init_product(qh_handle h, int nfactors, const int *nq, const double *const *amps,
                    const uint64_t *basis);
/* offset/count in amplitudes of the LOCAL shard, physical order.             */
int qh_upload(qh_handle h, const void *host, uint64_t offset, uint64_t count);
int qh_download(qh_handle h, void *host, uint64_t offset, uint64_t count);

/* ---- the hot path -------------------------------------------------------- */
/* Reference semantics (xgates.cc:23-41): 2x2 `gate` on qubit `tgt`.          */
int qh_apply1(qh_handle h, int tgt, const double gate[8]);
/* Reference semantics (xgates.cc:45-67): `gate` on `tgt` where qubit `ctl` is 1. */
int qh_applyc(qh_handle h, int ctl, int tgt, const double gate[8]);
/* Generalisation in LOGICAL bit positions (bit 0 = least significant index
 * bit = reference qubit nbits-1): gate on bit `tgt_bit` for indices having
 * all bits of `ctl_mask` set.  Used by the multi-GPU layer and by native
 * multi-controlled gates.                                                    */
int qh_apply_bits(qh_handle h, uint64_t ctl_mask, int tgt_bit,
                  const double gate[8]);
/* Dense 2^k x 2^k complex matrix (row-major, 2*4^k doubles, interleaved re,im) on LOGICAL bits bits[0..k-1];
 * bit j of the matrix's row/column index is logical bit bits[j] (bits[0] least significant); applied where every
 * bit of ctl_mask is 1.  1 <= k <= 6.  The caller's matrix is not referenced after the call returns.
 * Any matrix, unitary or not.  A barrier: what is queued runs first (one kernel of its own, never fused).
 * Errors: QH_ERR_ARG (null pointer, k out of range, k + local controls above 15, dry handle), QH_ERR_BAD_QUBIT,
 * QH_ERR_SAME_QUBIT (a bit twice, a control that is also a target), QH_ERR_NONLOCAL (a target held by the shard
 * index: nothing changes).  A control on a shard bit is dropped where met, and the call is a counted no-op where not. */
int qh_apply_matrix(qh_handle h, int k, const int32_t *bits, uint64_t ctl_mask, const double *matrix);

/* Gates selected by a table (kernels_mux.hip.h): one read and one write of the state for any k, 0 <= k <= 16.
 * gates: 2^k gates of 8 doubles (row-major a b c d, as everywhere).  For every index, s = the value of the selection
 * bits (bit j of s = LOGICAL bit sel_bits[j], sel_bits[0] least significant); gates[s] is applied to LOGICAL bit tgt_bit.
 * k = 0 (sel_bits may be NULL) is a plain uncontrolled gate.  Any matrices, unitary or not.  A barrier: what is queued runs
 * first, and the call works on the layout it finds (no re-layout).  The caller's table is not referenced after the call
 * returns.  One kernel, counted as one gate; bytes_swept = bytes_algorithmic = the state once read and once written.
 * A selection bit held by the shard index is fixed per shard: only the entries that agree with the shard index are used.
 * Errors: QH_ERR_ARG (null pointer, k out of range, dry handle), QH_ERR_BAD_QUBIT, QH_ERR_SAME_QUBIT (a bit twice, the
 * target among the selectors), QH_ERR_NONLOCAL (the target held by the shard index: nothing changes, nothing is flushed). */
int qh_apply_mux(qh_handle h, int k, const int32_t *sel_bits, int tgt_bit, const double *gates);
/* values: 2^k complex numbers (interleaved re,im); a_i *= values[s(i)], s gathered from bits[] the same way (any bit may
 * be held by the shard index).  k = 0 is qh_scale.  Otherwise as qh_apply_mux.                                        */
int qh_apply_diag(qh_handle h, int k, const int32_t *bits, const double *values);

/* Register permutation (kernels_perm.hip.h): |s> -> |table[s]> on the register made of LOGICAL bits bits[0..k-1] (bits[0]
 * least significant, as in qh_apply_diag), 1 <= k <= QH_PERM_MAX_BITS.  table: 2^k entries, a bijection of [0, 2^k).  For
 * every index i whose bits under ctl_mask are all 1, with register value s(i): new[i with register := table[s]] = old[i];
 * every other amplitude stays where it is.  Amplitudes are moved as stored: no arithmetic, bit-for-bit at both widths.
 * A barrier like qh_apply_mux: what is queued runs first, and the call works on the layout it finds.  The caller's table is
 * not referenced after the call returns.  Bit map, relayout mode and device pointer are as before.
 * Two paths (qh_perm_tiles below): tiles that fit LDS are permuted in place, one read and one write of the tiles whose
 * controls are met; larger tiles go through a second buffer of the state's size (the relayout buffer where the handle has
 * one, otherwise a temporary: QH_ERR_NOMEM, state unchanged, when there is no room) and are copied back.
 * qh_stats: gates_submitted + 1, kernels_launched + 1, bytes_algorithmic + 2 x the shard's bytes / 2^(local controls),
 * bytes_swept + what was read and written (the second path: the state twice read and twice written).
 * A control on a shard bit is dropped where met, and the call is a counted no-op (gates_noop) where not.
 * Errors, nothing runs and nothing changes: QH_ERR_ARG (null pointer, k out of range, dry handle, a table entry >= 2^k or a
 * value hit twice: qh_last_error names the first offending entry), QH_ERR_BAD_QUBIT, QH_ERR_SAME_QUBIT (a bit twice, a
 * control that is also a register bit), QH_ERR_NONLOCAL (a register bit held by the shard index: nothing is flushed).     */
#define QH_PERM_MAX_BITS 16
int qh_apply_perm(qh_handle h, int k, const int32_t *bits, uint64_t ctl_mask, const uint32_t *table);
/* How qh_apply_perm would walk the state right now (nothing runs, nothing is flushed; planner-only handles too).  Positions
 * are physical, local.  A tile is the amplitudes that agree outside tile_mask: the register's positions, the positions inside
 * a 128-byte line, padded with the lowest positions left to 10 bits; bit r of an in-tile index is the r-th lowest position of
 * tile_mask, the remaining positions, ascending, number the tiles.  Controls inside the tile (ctl_in) are a predicate per
 * amplitude; the tiles where a control outside it (ctl_out) is 0 are skipped.  QH_PERM_GATHER walks every amplitude of the
 * state instead: there the tile only says why (lds_bytes above 128 KiB).  ctl_met = 0: a control held by the shard index is 0
 * on this shard and the call would be a no-op.  Errors as qh_apply_perm, without those of the table and of dry handles.  */
#define QH_PERM_LDS 0           /* in place, tile by tile through LDS                          */
#define QH_PERM_GATHER 1        /* out of place: linear writes, gathered reads, copied back    */
typedef struct {
  uint32_t path;               /* QH_PERM_*                                                   */
  uint32_t tile_bits;          /* bits of an in-tile index                                    */
  uint64_t tile_mask;          /* positions of a tile's free bits                             */
  uint64_t reg_mask;           /* positions of the register (all inside tile_mask)            */
  uint64_t ctl_in, ctl_out;    /* positions of the local controls inside / outside the tile   */
  uint64_t ntiles;             /* 2^(nbits_local - tile_bits)                                 */
  uint64_t tiles_skipped;      /* of those, the tiles where a control of ctl_out is 0         */
  uint64_t lds_bytes;          /* amplitudes of one tile, in bytes                            */
  uint32_t ctl_met;            /* controls held by the shard index are all 1 on this shard    */
  uint32_t k;
  uint8_t reg_pos[QH_PERM_MAX_BITS];    /* position of register bit j                         */
  uint8_t reg_rank[QH_PERM_MAX_BITS];   /* the bit of the in-tile index that stands for it    */
} qh_perm_tiles;
int qh_perm_plan(qh_handle h, int k, const int32_t *bits, uint64_t ctl_mask, qh_perm_tiles *out);

/* Rank-one register update (kernels_rank1.hip.h): a I + b |u><v| on the register made of LOGICAL bits bits[0..k-1] (bits[0]
 * least significant, as in qh_apply_diag), identity on every other bit.  A fibre r is one setting of all other bits; for every
 * fibre whose bits under ctl_mask are all 1
 *     m_r = sum_s conj(v[s]) psi[s, r],      psi'[s, r] = a psi[s, r] + b u[s] m_r.
 * u, v: 2^k complex numbers each (interleaved re,im).  u == NULL means u = v.  v == NULL (then u must be NULL too) is the
 * UNIFORM form: u = v = the vector of 2^(-k/2).  Table form: 1 <= k <= QH_RANK1_MAX_BITS; uniform form: 1 <= k <= nbits_local.
 * a = -1, b = 2 with a normalised v is the reflection 2|v><v| - I (uniform form: Grover's inversion about the mean), a = 0,
 * b = 1 the projector |v><v|.  Any finite complex a and b and any finite tables: neither unitarity nor normalisation is checked.
 * A barrier like qh_apply_perm: what is queued runs first, and the call works on the layout it finds.  Bit map, relayout mode
 * and device pointer are as before; the caller's arrays are not referenced after the call returns.  Attached, host-mapped and
 * shard handles, from one local bit up, at both widths.
 * Arithmetic: in double, from the amplitudes as stored (complex64 widened unrounded); the tables are used as conj(v) and the
 * double-precision products b * u.  m_r is summed in a fixed order that depends only on the plan and the layout (a pairwise
 * tree over the register bits inside a tile or chunk, ascending position; the chunks of a fibre group in ascending order; the
 * segments of a split walk in order), without atomics; every new component is rounded once to the handle's width.  Amplitudes
 * where a control is 0 keep their bits.  The same state, layout and arguments give the same bits.
 * sums (may be NULL): sums[0] = the sum of |psi'|^2 over the amplitudes whose controls are met, as stored; sums[1] = the sum of
 * |m_r|^2 over those fibres (for a normalised v: the probability of finding the register in v).  This shard only, in double,
 * in the readers' fixed order, bitwise reproducible.  With sums the call waits for the stream.
 * Two paths (qh_rank1_info below): QH_RANK1_TILE, in place, one read and one write of the tiles whose out-of-tile controls are
 * met; QH_RANK1_TWO_PASS, two reads and one write of the shard, m_r kept in a scratch buffer of scratch_bytes (QH_ERR_NOMEM,
 * state unchanged, when there is no room).
 * qh_stats: gates_submitted + 1, kernels_launched + the plan's kernels (the fold of sums is not counted), bytes_swept + the
 * plan's bytes_swept, bytes_algorithmic + 2 x the shard's bytes / 2^(local controls).
 * A control on a shard bit is dropped where met, and the call is a counted no-op (gates_noop; sums = 0, 0) where not.
 * Errors, nothing runs, nothing changes, nothing is flushed: QH_ERR_ARG (null handle, bits, a or b; u without v; k out of range
 * for the form; a non-finite coefficient or table entry: qh_last_error names the first offending entry; dry handle),
 * QH_ERR_BAD_QUBIT, QH_ERR_SAME_QUBIT (a bit twice, a control inside the register), QH_ERR_NONLOCAL (a register bit held by
 * the shard index), QH_ERR_NOMEM.                                                                                          */
#define QH_RANK1_MAX_BITS 16
int qh_apply_rank1(qh_handle h, int k, const int32_t *bits, uint64_t ctl_mask, const double *u, const double *v,
                   const double a[2], const double b[2], double *sums /* may be NULL: 2 doubles */);
/* How qh_apply_rank1 would run right now (nothing runs, nothing is flushed; planner-only handles too; uniform != 0: the
 * uniform form).  tile: the tile of qh_perm_plan on the register's positions (its path field says only whether it fits LDS;
 * reg_pos and reg_rank are filled for k <= QH_PERM_MAX_BITS).  QH_RANK1_TILE when tile.lds_bytes <= 128 KiB and, in the table form,
 * k <= 10 (the tables are staged in LDS behind the tile's products).  Otherwise pass 1
 * cuts the shard into chunks of 2^chunk_bits consecutive amplitudes; reg_in_chunk register bits lie below chunk_bits and are
 * summed inside a block, the 2^reg_above chunks that differ only in the other register bits form one of `groups` fibre groups
 * of fibres_per_chunk fibres each and are walked in ascending order, by `split` blocks of `walk` chunks each; split > 1 adds a
 * kernel that folds the partial sums in segment order.  Fibre f of the scratch is the physical index with the register bits
 * taken out.  The engine launches from this very function.  Errors as qh_apply_rank1, without those of tables, coefficients
 * and dry handles.                                                                                                          */
#define QH_RANK1_TILE 0         /* in place, tile by tile: registers, fibre sums through LDS   */
#define QH_RANK1_TWO_PASS 1     /* m_r into scratch, then one update stream                    */
typedef struct {
  uint32_t path;               /* QH_RANK1_*                                                  */
  uint32_t uniform;
  qh_perm_tiles tile;
  uint64_t scratch_bytes;      /* TWO_PASS: 16 x nfibres x (1, or 1 + split when split > 1)   */
  uint64_t bytes_swept;        /* bytes the kernels request                                   */
  uint64_t nfibres;            /* 2^(nbits_local - k)                                         */
  uint64_t groups, fibres_per_chunk, walk;      /* pass 1 (0 on the TILE path)                */
  uint32_t kernels;            /* kernels the call launches                                   */
  uint32_t chunk_bits, reg_in_chunk, reg_above, split, pad;
} qh_rank1_info;
int qh_rank1_plan(qh_handle h, int k, const int32_t *bits, uint64_t ctl_mask, int uniform, qh_rank1_info *out);

/* The whole stream in one call: ops[2k] = control qubit of gate k or QH_NO_CTL (then qh_apply1), ops[2k+1] =
 * target qubit, gates + 8k = its 8 doubles -- exactly `count` qh_apply1/qh_applyc calls (xgates.cc:89-145), without
 * the per-call cost of the host language's FFI (ctypes: ~3 us per gate).  Stops at the first error.          */
#define QH_NO_CTL INT32_MIN
int qh_apply_stream(qh_handle h, uint64_t count, const int32_t *ops, const double *gates);

int qh_set_fusion(qh_handle h, int level);
/* Launch everything queued (no-op with QH_FUSE_OFF).                         */
int qh_flush(qh_handle h);
/* qh_flush + wait for the stream.                                            */
int qh_sync(qh_handle h);
/* Gates accepted but not yet executed.  After a failed flush these are the gates
 * that did NOT run (a planning/allocation failure keeps the whole queue; a failed
 * per-gate launch keeps that gate and every later one): the caller may change the
 * fusion level and flush again, or drop them.  (The reference has no counterpart:
 * xgates.cc:23-67 runs every gate synchronously or exits.)                    */
int qh_pending_gates(qh_handle h, uint64_t *count);
int qh_discard_pending(qh_handle h);

/* ---- logical -> physical bit map (global<->local qubit swaps) ----------- */
/* Records that the DATA of physical bits a and b has been exchanged (by the
 * communication layer for a >= nbits_local).  Later
 * gates are routed through the map; readers report physical indices, convert
 * with qh_phys_to_logical.                                                   */
int qh_remap_swap(qh_handle h, int phys_bit_a, int phys_bit_b);
int qh_get_bitmap(qh_handle h, int32_t *phys_of_logical /* [nbits_global] */);
int qh_phys_to_logical(qh_handle h, uint64_t phys_index, uint64_t *logical);
int qh_logical_to_phys(qh_handle h, uint64_t logical_index, uint64_t *phys);

/* ---- multi-GPU exchange (the reference has no distributed path) --------------
 * One process per GPU, each with one handle on its shard (qh_set_shard).  A dense gate whose
 * target is a shard bit needs the exchange below first; gates on local bits, controls on shard
 * bits and diagonal gates on shard bits never communicate.  Transport: RCCL send/recv over xGMI
 * on a second HIP stream (qh_comm_init), or a host-staged callback (qh_comm_init_custom: tests
 * with several ranks on one GPU, fabrics without peer access).
 *
 * qh_exchange_* first run the queued gates, then enqueue the exchange and RETURN: the exchange
 * proceeds in slabs, slab k leaving as soon as the part of the last queued sweep that writes it
 * has finished, and the first sweep submitted afterwards starts on slab k as soon as slab k has
 * arrived (HIP events between the handle's stream and the exchange streams; no host wait).
 * Every other entry point that touches the state waits for the arrivals first.
 * The bit map is NOT changed here: the caller records the swap (qh_remap_swap, or its own map). */
#define QH_COMM_ID_BYTES 128
/* One round of the host-staged transport: send bytes from send_host[i] to rank peers[i] and
 * receive the same number of bytes from it into recv_host[i], for all i at once; 0 = ok.   */
typedef int (*qh_round_fn)(void *user, int npeers, const int *peers, void *const *send_host,
                           void *const *recv_host, uint64_t bytes);
typedef struct {
  uint64_t exchanges;        /* qh_exchange_* calls                                        */
  uint64_t rounds;           /* grouped send/recv rounds                                   */
  uint64_t bytes_sent;       /* bytes this rank sent (== bytes received)                   */
  uint64_t slabs;            /* slabs the exchanges were cut into                          */
  uint64_t sweeps_overlapped;/* sweeps launched slab-wise around exchanges                 */
  double span_ms;            /* HIP-event time from the first send to the last landing     */
  uint64_t rounds_packed;    /* rounds moved through the gather / scatter kernels (blocks
                                without long contiguous runs: after relayout sweeps)       */
  uint64_t geometry_checks;  /* exchange geometries whose signature was compared with every
                                peer's and found equal (0 with one rank)                   */
  uint32_t comm_ranks;       /* size and ...                                               */
  uint32_t comm_rank;        /* ... rank as the TRANSPORT reports them (ncclCommCount /
                                ncclCommUserRank; the caller's arguments on the host-staged
                                transport)                                                 */
} qh_xstats;
/* How the last qh_exchange_* call of a handle was cut.  Every field must be the same on every rank (the planner keeps
 * rank-dependent gates as ghosts so that it is; `signature` is what the ranks compare before data moves): tools and tests
 * read it, on real handles and -- without any device -- on planner-only ones (qh_create_dry + qh_comm_init_dry).        */
typedef struct {
  uint64_t signature;        /* 64-bit hash of everything below + the bit map + planner switches + build            */
  uint64_t slab_mask;        /* local index bits whose values number the slabs (layout after the queued sweeps)     */
  uint64_t block_bits;       /* local index bits that select the block a peer gets                                  */
  uint64_t rounds_per_slab;  /* grouped send/recv rounds per slab                                                   */
  uint64_t staging_bytes;    /* staging area this exchange needs (receive halves + send halves of packed rounds)    */
  uint32_t slabs;            /* 2^popcount(slab_mask)                                                               */
  uint32_t chunk_bits;       /* log2(amplitudes per peer and round)                                                 */
  uint32_t packed;           /* 1: rounds go through the gather / scatter kernels, 0: sent from where they lie      */
  uint32_t peers;            /* peers per round                                                                     */
  uint32_t sweeps_before;    /* sweeps the queued gates were planned into (the last one precedes the exchange)      */
  uint32_t last_sweep_split; /* 1: that last sweep was launched slab by slab (overlaps the exchange)                */
} qh_xgeom;
int qh_exchange_geometry(qh_handle h, qh_xgeom *out);
/* Planner-only counterpart of qh_comm_init for handles made by qh_create_dry: qh_exchange_* then plan the queued gates,
 * decide slabs, rounds, chunk size and path exactly as a real handle of that rank would, and move nothing.          */
int qh_comm_init_dry(qh_handle h, int nranks, int rank);
int qh_comm_unique_id(void *id /* QH_COMM_ID_BYTES, rank 0; broadcast by the caller */);
int qh_comm_init(qh_handle h, int nranks, int rank, const void *id);
int qh_comm_init_custom(qh_handle h, int nranks, int rank, qh_round_fn fn, void *user);
int qh_comm_destroy(qh_handle h);
/* All g = log2(nranks) shard bits <-> local bits [base_bit, base_bit+g): rank r sends block j of
 * its shard to rank j and receives rank j's block r in its place (all peers at once).
 * chunk_amps: amplitudes per peer and round (0 = default 2^22).                             */
int qh_exchange_alltoall(qh_handle h, int base_bit, uint64_t chunk_amps);
/* Shard bit k (0..g-1) <-> local_bit: the half of the shard whose local_bit differs from this
 * rank's shard bit k is swapped with rank (r ^ 2^k)'s (one peer, one link).                 */
int qh_exchange_pair(qh_handle h, int shard_bit, int local_bit, uint64_t chunk_amps);
/* Self test of the transport on one rank: the two halves of the shard selected by local_bit are
 * sent to this rank itself and land exchanged (== an X gate on that bit), through the same
 * rounds / staging / slabs as a real exchange.                                              */
int qh_exchange_loopback(qh_handle h, int local_bit, uint64_t chunk_amps);
int qh_exchange_wait(qh_handle h);                 /* host wait for all arrivals             */
/* Host waits of a handle whose communicator has several ranks are bounded: if the stream has not drained within
 * QH_COMM_TIMEOUT_MS (default 300000) -- a peer is missing, or the ranks disagree about a round -- the call returns
 * QH_ERR_COMM instead of hanging, and the handle refuses further work.  Before data moves the ranks compare a signature
 * of the exchange geometry (every geometry a communicator has not seen yet; QH_EXCHANGE_VERIFY=1 every exchange, =0
 * never): a disagreement is QH_ERR_COMM with both signatures in qh_last_error().                                    */
int qh_exchange_stats(qh_handle h, qh_xstats *out);
/* sum over ranks of `count` doubles, in place (RCCL transport only): norms, probabilities    */
int qh_comm_allreduce_sum(qh_handle h, double *inout, int count);

/* ---- device-side readers (state.py:24-78) ------------------ */
int qh_norm2(qh_handle h, double *out);                       /* sum |a|^2 of the shard, in the readers' fixed order: same state and layout, same bits */
/* One amplitude by LOGICAL index (state.py:31-40 ampl/prob), read where it lives now: no
 * re-layout, 16 bytes over PCIe.  QH_ERR_NONLOCAL if another shard holds it.                */
int qh_amplitude(qh_handle h, uint64_t logical_index, double out[2]);
int qh_argmax(qh_handle h, uint64_t *phys_index, double *prob); /* max |a|^2 of the shard */
int qh_prob_bit(qh_handle h, int logical_bit, double *p1);    /* sum |a|^2 with bit set (shard) */
int qh_prob_bit_value(qh_handle h, int logical_bit, int value, double *p); /* ... with bit == value */
int qh_scale(qh_handle h, double re, double im);              /* a *= (re + i im) */
/* Project on logical_bit == value (zero the rest); caller renormalises with qh_scale. */
int qh_project_bit(qh_handle h, int logical_bit, int value);
/* Register readout (kernels_measure.hip.h).  Bits are LOGICAL (bit 0 = least significant index bit = reference qubit
 * nbits-1); every call is per shard and runs what is queued first.
 * out[j] = sum |a_i|^2 over the shard's indices i whose bit bits[t] equals bit t of j, for 0 <= j < 2^k.
 * 0 <= k <= 16 (k = 0: out[0] = the shard's norm).  Bits may sit anywhere in the current layout, shard bits included
 * (fixed per shard: every j whose shard-bit part disagrees gets 0).  Not normalised.  Bitwise reproducible for a
 * given state and layout: one read of the state, fixed-order sums in double.
 * Errors: QH_ERR_ARG (null, k out of range, dry handle), QH_ERR_BAD_QUBIT, QH_ERR_SAME_QUBIT.                     */
int qh_marginal(qh_handle h, int k, const int32_t *bits, double *out);
/* Inverse-CDF sampling: for each u[s] (ascending, 0 <= u < 1), the LOGICAL index of the first amplitude, in the
 * engine's current physical order, at which the running sum of |a|^2 exceeds u[s] * (shard norm).  Never returns
 * an index whose amplitude is exactly 0.  count = 0 is allowed.  At most two reads of the state + O(count).
 * QH_ERR_ARG if u is not ascending or out of [0,1), or if the shard's norm is 0.                                  */
int qh_sample(qh_handle h, uint64_t count, const double *u, uint64_t *logical_out);
/* Zero every amplitude whose logical bits under `mask` differ from `value` (value & ~mask must be 0: QH_ERR_ARG); the
 * caller renormalises with qh_scale.  Shard bits in the mask: a shard that disagrees is zeroed whole (as
 * qh_project_bit).  Writes zeros only.  QH_ERR_BAD_QUBIT for mask bits >= nbits_global.                           */
int qh_project_bits(qh_handle h, uint64_t mask, uint64_t value);
/* Pauli-string expectations (kernels_expect.hip.h).  Term t is two masks over LOGICAL bits: xmask (X or Y on the bit) and
 * zmask (Z or Y).  out[t] = Re sum over the shard's i of conj(a_i) (P_t a)_i: per shard, not normalised (x = z = 0 gives
 * the shard's norm).  Runs what is queued first; reads only (state, bit map and relayout mode are as before).  Terms that
 * share an x mask share a read of the state, 16 at a time: qh_stats.kernels_launched grows by the number of reads,
 * sum over distinct x masks of ceil(terms / 16).  A z bit held by the shard index is a sign fixed per shard; an x bit
 * held by the shard index is QH_ERR_NONLOCAL (nothing computed, out untouched).  Bitwise reproducible for a given state
 * and layout.  nterms = 0 is allowed.  Errors: QH_ERR_ARG (null, dry handle), QH_ERR_BAD_QUBIT (mask bits >= nbits_global). */
int qh_expect_pauli(qh_handle h, uint64_t nterms, const uint64_t *xmask, const uint64_t *zmask, double *out);
/* Sparse readout (kernels_select.hip.h): a short list of (logical index, amplitude) entries instead of a reduction.  All
 * three calls are per shard, run what is queued first and read only (state, bit map, relayout mode and device pointer are
 * as before); they work at either width (complex64 amplitudes are widened to double, unrounded), in whatever layout the
 * last flush left, on attached and host-mapped handles, from 1 local bit up.  index is the GLOBAL LOGICAL index, the bits
 * the shard index holds included.  A probability is fma(im, im, re * re) in double, as qh_argmax computes it.  Dry handles:
 * QH_ERR_ARG.                                                                                                            */
typedef struct { uint64_t index; double re, im; } qh_entry;
#define QH_SELECT_MAX (1u << 20)
#define QH_TOPK_MAX 4096
/* Every amplitude of the shard with probability >= threshold.  *count = their exact number, whatever cap is; *weight (may
 * be NULL) = the sum of their probabilities, in double, in a fixed order without float atomics: bitwise reproducible for a
 * given state and layout.  If *count <= cap, out[0..*count) holds them in ascending index, amplitudes bit for bit as
 * stored; otherwise out is not written and the call is still QH_OK (raise the threshold or the cap).  cap == 0 with
 * out == NULL is the count-only form; threshold == 0 selects everything.  One read of the state: a stream compaction with
 * one returning 64-bit atomic add per wave and chunk that has hits (none once the count has passed cap);
 * qh_stats.kernels_launched grows by 1, bytes_swept and bytes_algorithmic by the bytes of the state.
 * Errors, nothing written: QH_ERR_ARG (null handle or count, threshold negative or NaN, cap > QH_SELECT_MAX, out == NULL
 * with cap > 0).                                                                                                         */
int qh_select(qh_handle h, double threshold, uint64_t cap, qh_entry *out, uint64_t *count, double *weight);
/* The k entries of largest probability, most probable first, ties by ascending index -- at the cut too: the smallest
 * indices get in.  Entries of probability 0 are never returned: *count = min(k, nonzero amplitudes of the shard).
 * qh_topk(h, 1, ...) names the amplitude qh_argmax names.  A radix select on the bit pattern of the probability: one
 * histogram read of the top key bits, then one compaction read from the lower edge of the bin that holds the k-th entry (a
 * peaked state: kernels_launched + 2).  One compaction hands the host at most max(4 k, QH_TOPK_MAX) candidates; a boundary
 * bin that holds more is histogrammed again on its next 12 key bits (at most 6 histogram reads: then the bin is one value),
 * and one value with that many ties -- a flat state, or the near-flat output of a QFT -- is finished by scanning ranges of
 * the LOGICAL index space for it (each scan counts as a kernel; bytes_swept grows by what it read).  Exact.  k == 0 is
 * allowed; NaN amplitudes: unspecified.
 * Errors: QH_ERR_ARG (null, k > QH_TOPK_MAX).                                                                             */
int qh_topk(qh_handle h, uint64_t k, qh_entry *out, uint64_t *count);
/* out[2j], out[2j+1] = the amplitude at global LOGICAL index logical[j]; exactly (0, 0) where another shard holds it, so
 * the sum over ranks is the answer.  *nlocal (may be NULL) = how many of the entries this shard holds.  One gather kernel
 * and one copy back, no read of the state (kernels_launched is unchanged).  Duplicates and count == 0 are allowed.
 * Errors, nothing written: QH_ERR_ARG (null, count > 2^24, an index >= 2^nbits_global).                                   */
int qh_amplitudes(qh_handle h, uint64_t count, const uint64_t *logical, double *out, uint64_t *nlocal);
/* Reduced density matrix of k listed LOGICAL bits (kernels_density.hip.h): rho = Tr_rest |psi><psi| of this shard.
 * out[2 (r 2^k + c)], out[2 (r 2^k + c) + 1] = (re, im) of rho[r][c] = sum_e a(r,e) conj(a(c,e)), where a(r,e) is the shard's
 * amplitude whose logical bit bits[t] equals bit t of r (the bit convention of qh_marginal) and whose remaining local bits
 * spell e.  Per shard and not normalised: the trace is the shard's norm.  The output is always complex128: complex64
 * amplitudes are widened unrounded, every product and sum is formed in double.
 * 0 <= k <= min(QH_DENSITY_MAX_BITS, nbits_local): k = 0 gives the norm, k = nbits_local the outer product of the shard's
 * state.  Works from 1 local bit up, at either width, on attached and host-mapped handles, in whatever layout the last flush
 * left; the bits may sit at any physical positions.  Runs what is queued first; reads only (state, bit map, relayout mode
 * and device pointer are as before).
 * Exact properties: rho[c][r] is the bitwise conjugate of rho[r][c] (one triangle is computed, the other mirrored); every
 * diagonal imaginary part is exactly 0.0; sums run in a fixed order without float atomics, so two calls on the same state
 * and layout return the same bits; a basis state gives exactly one 1.0 and zeros elsewhere.  The diagonal agrees with
 * qh_marginal to rounding (the summation orders differ).
 * A listed bit held by the shard index is QH_ERR_NONLOCAL (nothing runs, out untouched: the off-diagonal blocks would live
 * on other shards; exchange first, as for an x bit of qh_expect_pauli).  With every listed bit local, the sum of the shards'
 * results is the global rho.
 * The walk (qh_density_tiles below is what the engine launches from): a 256-thread workgroup owns a tile of up to 64 x 64
 * entries, a thread a 4 x 4 block of complex accumulators; the workgroup walks its share of the remaining (environment)
 * bits in chunks of columns that go into LDS once, with 16-byte loads in physical order.  k < 6: the 256 threads form groups
 * that take different columns and are folded through LDS in a fixed order (k <= 2: one tile per thread, straight from
 * memory).  k = 7, 8: the matrix is cut into blocks of 64 rows and one launch covers the block pairs (R, C >= R), 3 or 10 of
 * them; a pair reads the rows of both blocks, so the state is read 2 or 4 times.  Every workgroup writes its partial tile
 * to a slab row; a fold kernel adds the rows of a pair in workgroup order and scatters to out, mirroring the conjugate.
 * Fewer than 8 local bits: one workgroup gathers amplitude by amplitude.
 * qh_stats: kernels_launched + 1 (the fold is not counted), bytes_algorithmic + the shard's bytes, bytes_swept + the bytes
 * the kernel requests (qh_density_tiles.amps_swept amplitudes).
 * Errors, nothing runs and out is untouched: QH_ERR_ARG (null pointers, k out of range, dry handle), QH_ERR_BAD_QUBIT,
 * QH_ERR_SAME_QUBIT, QH_ERR_NONLOCAL as above.                                                                            */
#define QH_DENSITY_MAX_BITS 8
int qh_reduced_density(qh_handle h, int k, const int32_t *bits, double *out /* 2 * 4^k doubles */);
/* How qh_reduced_density would walk the state right now (density_plan.h: host arithmetic on the bit map only; nothing runs,
 * nothing is flushed; planner-only handles too).  Positions are physical, local, ascending in every table.
 *   row_pos[j], j < k       the register's positions; bit j of a row number as the kernels count it.  The first tile_bits
 *                           of them number the rows of a tile, the others (k = 7, 8: the highest) number the row blocks.
 *   row_bit[j]              row_pos[j] holds bits[row_bit[j]]: bit j of a kernel row number is bit row_bit[j] of r in out.
 *   col_pos[c], c < chunk_bits   the columns of a chunk: the LOWEST positions the register does not hold.
 *   rest_pos[q], q < nrest  the other environment positions: bit q of a chunk number.
 * A launch has block_pairs * wg_per_pair workgroups; a workgroup walks chunks_per_wg consecutive chunks of 2^chunk_bits
 * columns: wg_per_pair * chunks_per_wg * 2^chunk_bits = 2^(nbits_local - k), the environment exactly once per pair.
 * Errors: QH_ERR_ARG (null, k out of range), QH_ERR_BAD_QUBIT, QH_ERR_SAME_QUBIT, QH_ERR_NONLOCAL as qh_reduced_density.    */
#define QH_DENSITY_TILES 0      /* tiles of min(k, 6) row bits, chunks of columns                    */
#define QH_DENSITY_GATHER 1     /* fewer than 8 local bits: one workgroup, amplitude by amplitude    */
typedef struct {
  uint32_t path;               /* QH_DENSITY_*                                                */
  uint32_t k;                  /* register bits                                               */
  uint32_t tile_bits;          /* row bits of a tile: min(k, 6); QH_DENSITY_GATHER: k          */
  uint32_t chunk_bits;         /* column bits of a chunk                                      */
  uint32_t nrest;              /* chunk-number bits: nbits_local - k - chunk_bits             */
  uint32_t block_pairs;        /* 1, 3 (k = 7) or 10 (k = 8)                                  */
  uint32_t wg_per_pair;        /* workgroups, = slab rows, per block pair                     */
  uint32_t pad;
  uint64_t chunks_per_wg;
  uint64_t slab_bytes;         /* block_pairs * wg_per_pair rows of 4^tile_bits complex128    */
  uint64_t amps_swept;         /* amplitudes the kernel requests: 2^(nbits_local + k - tile_bits) */
  uint8_t row_pos[8], row_bit[8];
  uint8_t col_pos[16];
  uint8_t rest_pos[40];
} qh_density_tiles;
int qh_density_plan(qh_handle h, int k, const int32_t *bits, qh_density_tiles *out);

/* ---- two states (kernels_two_state.hip.h) ------------------------------------ */
/* A new handle on src's device holding a copy of src's state: what src has queued runs first, then one device-to-device
 * copy of the buffer as it lies, with nbits (local and global), width, shard index, fusion level and the bit map as it is
 * (no canonical order; src's pointer, layout and relayout mode are as before).  The clone always owns HBM memory and its own
 * stream, also when src is attached or host-mapped; it starts with zeroed stats, nothing queued, relayout mode undecided and
 * no communicator.  The copy is complete when the call returns.
 * Errors: QH_ERR_ARG (null, dry handle), QH_ERR_NOMEM (no room: nothing is created; src's STATE is unchanged, but what it
 * had queued has run, and a flush may re-lay it out).                                                                     */
int qh_clone(qh_handle src, qh_handle *out);
/* dst's state := src's, amplitudes and bit map together (restore a snapshot).  What src has queued runs first; what dst has
 * queued is dropped, as by qh_init_basis.  Waits for dst's outstanding exchange arrivals and stream work, then copies into
 * dst's CURRENT buffer: the pointer of an attached or host-mapped dst stays valid, dst's relayout mode and second buffer stay
 * as they are.  The host waits for the copy: after return either handle may be used at once.
 * Errors: QH_ERR_ARG (null, dry handle, dst == src, another device, different nbits (local or global), width or shard
 * index): nothing changes.                                                                                              */
int qh_copy(qh_handle dst, qh_handle src);
/* out = sum_i conj(a_i) b_i as (re, im) over this shard's amplitudes, matched by LOGICAL index: per shard, not normalised;
 * qh_inner(a, a, out) is the shard's norm with out[1] == 0.0 exactly.  Runs what both handles have queued; a's stream waits
 * for b's flushed work (an event), the read runs on a's stream and the host waits for it: on return b is free again.  Reads
 * only: state, bit map, relayout mode and device pointer of both handles are as before, wherever their local bits sit --
 * equal layouts are read as two linear streams (16 bytes per lane and load at either width), different ones tile by tile
 * (qh_inner_tiles below), each state in runs of 16 amplitudes.  Sums in double from the stored amplitudes, in a fixed order: bitwise reproducible for given states and
 * layouts.  a's qh_stats.kernels_launched grows by 1 (one read of the two states), b's by 0.
 * Both handles must hold the same logical bits in the shard index, at the same positions, with the same shard index:
 * otherwise QH_ERR_NONLOCAL (exchange first; out untouched).
 * Errors: QH_ERR_ARG (null, dry handle, another device, different nbits (local or global) or width).                     */
int qh_inner(qh_handle a, qh_handle b, double out[2]);
/* How qh_inner would walk a and b right now (nothing runs, nothing is flushed; planner-only handles too).  Positions are
 * physical, local.  QH_INNER_TILES: bit k of an in-tile index is position tile_a[k] in a's enumeration and tile_b[k] in
 * b's (both ascending, both start 0,1,2,3); a's amplitude at in-tile index r pairs with b's at sum_k bit_k(r) << shuffle[k];
 * bit k of a tile number is position rest_a[k] in a and rest_b[k] in b.  Host arithmetic on the two bit maps only: dry
 * handles are allowed and the handles' devices are not compared.  Errors: QH_ERR_ARG (null, different nbits (local or
 * global) or width), QH_ERR_NONLOCAL as qh_inner.                                                                         */
#define QH_INNER_LINEAR 0       /* same layout: both states front to back                      */
#define QH_INNER_TILES 1        /* tiles of 2^8 amplitudes, b's crossing through LDS           */
#define QH_INNER_GATHER 2       /* fewer than 8 local bits: one amplitude at a time            */
typedef struct {
  uint32_t path;               /* QH_INNER_*                                                  */
  uint32_t nrest;              /* tile-number bits: nbits_local - 8                           */
  uint64_t free_a, free_b;     /* a tile's free bits, in a's and in b's positions             */
  uint8_t tile_a[8], tile_b[8], shuffle[8];
  uint8_t rest_a[56], rest_b[56];
  uint8_t pos_b[64];           /* b's position of the logical bit a keeps at position p       */
} qh_inner_tiles;
int qh_inner_plan(qh_handle a, qh_handle b, qh_inner_tiles *out);
/* dst := alpha*dst + beta*src, amplitude by amplitude, matched by LOGICAL index.  alpha, beta: (re, im).  Written in place
 * into dst's current buffer in dst's current layout: bit map, relayout mode, second buffer and device pointer of dst are as
 * before (attached and host-mapped handles too); src is read only.  What both handles have queued runs first (dst's queue is
 * flushed, not dropped; dst's exchange arrivals are waited for); dst's stream waits for src's flushed work (an event), the
 * kernel runs on dst's stream and the host waits for it: on return either handle may be used at once.
 * The two states are walked as qh_inner_plan(dst, src) says: equal layouts as linear streams of 16 bytes per lane, different
 * ones tile by tile with src's values crossing through LDS, fewer than 8 local bits as a gather.
 * Each component of a new amplitude is formed in double from the stored amplitudes and rounded once to the handle's width;
 * a coefficient component that is exactly 0 contributes 0 whatever the amplitude holds, so coefficients made of 0, 1 and -1
 * give d + s, d - s, s ... equal as numbers to the sums formed at the handle's width (the sign of a zero may differ).
 * alpha == 0 exactly: dst's old values are not read (NaN or Inf in them does not propagate; two streams).  beta == 0 exactly:
 * src is not read, whatever its layout.  Both 0: one stream of zeros.  alpha == 1 and beta == 0: no kernel.
 * norm2 (may be NULL): sum |a|^2 of dst's NEW amplitudes as stored, over this shard, in double, in a fixed order without
 * atomics: the same states, layouts and coefficients give the same bits.  Without a kernel it is qh_inner(dst, dst)'s sum.
 * dst's qh_stats: kernels_launched + 1 (+ 0 without a kernel), bytes_swept and bytes_algorithmic + (streams touched: the
 * write, dst's read unless alpha == 0, src's read unless beta == 0) x the bytes of the state.  src's stats are unchanged.
 * Errors, nothing runs and nothing changes: QH_ERR_ARG (null handle or coefficient pointer, dry handle, dst == src -- use
 * qh_scale --, another device, different nbits (local or global) or width); QH_ERR_NONLOCAL as qh_inner (another shard index,
 * or a logical bit one handle keeps in the shard index and the other elsewhere; exchange first).                          */
int qh_axpby(qh_handle dst, const double alpha[2], qh_handle src, const double beta[2], double *norm2);

/* ---- Pauli-sum operators (kernels_pauli.hip.h, pauli_plan.h) ------------------ */
/* dst := (sum_t c_t P_t) src, out of place.  Term t is a coefficient coeffs[2t], coeffs[2t+1] = (re, im) and two masks over
 * LOGICAL bits as in qh_expect_pauli (xmask: X or Y on the bit, zmask: Z or Y), nY = popcount(x & z):
 *   (P a)_i = (-i)^nY (-1)^popcount(i & z) a_{i ^ x},   dst_i = sum_t c_t (P_t src)_i.
 * Any coefficients are accepted (Hermitian or not is the caller's business); terms are taken as given, never merged or dropped.
 * Handles: what src has queued runs first and src is read only (state, bit map, relayout mode and pointer as before).  dst is
 * replaced whole, as by qh_copy: what it has queued is dropped, a poisoned flag is cleared, its exchange arrivals and stream
 * are waited for; the result goes into dst's CURRENT buffer (attached and host-mapped handles too; relayout mode and second
 * buffer stay) in src's physical layout, so dst takes src's bit map.  dst's stream waits for src's flushed work (an event),
 * the kernels run on dst's stream and the host waits: on return both handles are free.
 * Batches: masks go through the bit map as in qh_expect_pauli; a z bit held by the shard index is a sign folded into the
 * coefficient on the host, an x bit there is QH_ERR_NONLOCAL (nothing runs, dst untouched).  c'_t = c_t (-i)^nY (shard sign)
 * is formed on the host by exact swaps and negations.  The terms are stably sorted by physical x mask and cut every
 * QH_PAULI_SUM_BATCH terms (a batch may hold several x masks; G_b = the distinct ones in batch b); one kernel per batch, the
 * first writes dst without reading it, the later ones read dst and add to it.  Within a batch every component is formed in
 * double from the stored amplitudes (complex64 widened unrounded; plus dst's stored value after the first batch) and rounded
 * once to the handle's width.  A batch of one term with c' = 1 stores the source amplitude bit for bit; c' in {-1, i, -i}
 * gives it exactly as a number.  nterms == 0: dst becomes zeros in one kernel.
 * norm2 (may be NULL): sum |a|^2 of dst's FINAL amplitudes as stored, over this shard, in double, in a fixed order without
 * atomics: bitwise reproducible for given states, layout and terms.
 * dst's qh_stats (src's are unchanged): kernels_launched + the number of batches (+ 1 for nterms == 0); bytes_swept + the sum
 * over batches of (G_b + 1 + [b > 0]) x the shard's bytes -- what the kernels request, an upper bound on HBM traffic;
 * bytes_algorithmic + 2 x the shard's bytes (1 x for nterms == 0).  Works from 1 local bit up, at either width.
 * Errors, nothing runs and nothing changes: QH_ERR_ARG (null handle, null arrays with nterms > 0, dry handle, dst == src,
 * another device, different nbits (local or global), width or shard index), QH_ERR_BAD_QUBIT (mask bits >= nbits_global),
 * QH_ERR_NONLOCAL as above.                                                                                                */
#define QH_PAULI_SUM_BATCH 16
int qh_apply_pauli_sum(qh_handle dst, qh_handle src, uint64_t nterms, const double *coeffs /* 2 per term */,
                       const uint64_t *xmask, const uint64_t *zmask, double *norm2 /* may be NULL */);
/* The same into a NEW handle made beside src as qh_clone makes its own (without the copy): it owns HBM memory and a stream,
 * starts with zeroed stats -- which then count this call -- and takes src's bit map.  QH_ERR_NOMEM: nothing is created.    */
int qh_pauli_sum_new(qh_handle src, uint64_t nterms, const double *coeffs, const uint64_t *xmask,
                     const uint64_t *zmask, double *norm2, qh_handle *out);
/* How qh_apply_pauli_sum would batch these terms on src right now: runs nothing, flushes nothing, planner-only handles too.
 * terms (may be NULL): the nterms terms in sorted order -- index of the caller's term, physical local masks, the sign the
 * shard index gives (1: negative) and nY mod 4.  batches: at most cap are written, *nbatches is always set; batch b holds
 * terms [first, first + count), ngroups distinct x masks, and asks for streams = ngroups + 1 + [b > 0] passes over the shard.
 * The engine launches from this very function.  Errors: QH_ERR_ARG (null), QH_ERR_BAD_QUBIT, QH_ERR_NONLOCAL as above.      */
typedef struct { uint64_t index, px, pz; uint32_t neg, ny; } qh_pauli_term;
typedef struct { uint64_t first, count, ngroups, streams; } qh_pauli_batch;
int qh_pauli_sum_plan(qh_handle src, uint64_t nterms, const uint64_t *xmask, const uint64_t *zmask,
                      qh_pauli_term *terms /* nterms, sorted order; may be NULL */,
                      qh_pauli_batch *batches, uint64_t cap, uint64_t *nbatches);

/* ---- Pauli products (kernels_pauli_product.hip.h, pauli_product_plan.h) -------- */
/* state := F_{n-1} ... F_1 F_0 state in place, F_t = a_t I + b_t P_t: term 0 is applied first and the caller's order is never
 * changed.  ab holds (a.re, a.im, b.re, b.im) per term; the masks and P are those of qh_expect_pauli and qh_apply_pauli_sum,
 *   (P v)_i = (-i)^nY (-1)^popcount(i & z) v_{i ^ x}   over LOGICAL bits.
 * Any finite complex a, b: a rotation exp(-i t P) is (cos t, -i sin t), imaginary time (cosh t, -sinh t), a projector
 * (1/2, +-1/2), the string itself (0, 1).
 * A barrier, as qh_apply_mux and qh_apply_perm: what is queued runs first and the call works on the layout it finds; bit map,
 * relayout mode and device pointer are as before.  Attached, host-mapped and shard handles, from 1 local bit up, at either
 * width.  The caller's arrays are not referenced after the call returns.
 * Shards: a z bit held by the shard index is a sign, folded into b on the host together with (-i)^nY (b', swaps and negations
 * only); an x bit there is QH_ERR_NONLOCAL.  The WHOLE term list is checked before anything is flushed or run.
 * Runs: the terms are walked in order, keeping the current run's pair mask X (physical, local; 0 while every term so far is
 * diagonal).  Term t (physical x mask px_t) joins the run if the run has fewer than QH_PAULI_PRODUCT_BATCH terms and px_t == 0,
 * X == 0 or px_t == X; otherwise a new run starts.  One kernel per run: one read and one write of the state, whatever the
 * weight of the strings.  (The batch is 8: measured at 30 qubits, a 16-term run cost more per term than two of 8;
 * DESIGN.md "Pauli products".)  kind: QH_PAULI_RUN_DIAG (every px == 0), QH_PAULI_RUN_HALF (complex64 and X == 1: the pair lies
 * inside one 16-byte item), QH_PAULI_RUN_PAIR (otherwise).
 * Arithmetic: every term of a run is applied in registers, in double, to the amplitudes as stored (complex64 widened
 * unrounded); the result is rounded once per run to the handle's width.  A run of ONE term with a == 0 and b' a power of i
 * moves the stored bits (negated and / or with the components swapped): exact at both widths.  A run of one term with a == 1,
 * b == 0 leaves every bit as it was.
 * norm2 (may be NULL): sum |v|^2 of the FINAL amplitudes as stored, over this shard, summed by the last run in the readers'
 * fixed order without atomics: bitwise reproducible.  nterms == 0 flushes and launches no kernel; norm2 is then qh_norm2's.
 * qh_stats: gates_submitted + nterms, kernels_launched + the number of runs, bytes_swept and bytes_algorithmic + 2 x the
 * shard's bytes per run.
 * Errors, nothing runs, nothing changes, nothing is flushed: QH_ERR_ARG (null handle, null arrays with nterms > 0, dry handle,
 * a non-finite coefficient: qh_last_error names the first offending term), QH_ERR_BAD_QUBIT (mask bits >= nbits_global),
 * QH_ERR_NONLOCAL as above.                                                                                                 */
#define QH_PAULI_PRODUCT_BATCH 8
#define QH_PAULI_RUN_DIAG 0
#define QH_PAULI_RUN_PAIR 1
#define QH_PAULI_RUN_HALF 2
int qh_apply_pauli_product(qh_handle h, uint64_t nterms, const double *ab /* 4 per term: a.re a.im b.re b.im */,
                           const uint64_t *xmask, const uint64_t *zmask, double *norm2 /* may be NULL */);
/* How qh_apply_pauli_product would cut these terms into runs on h right now: runs nothing, flushes nothing, planner-only
 * handles too.  terms (may be NULL): the nterms terms in the caller's order, as qh_pauli_sum_plan reports them.  runs: at most
 * cap are written, *nruns is always set; run r holds terms [first, first + count), pair mask px (0: diagonal) and its kind.
 * The engine launches from this very function.  Errors: QH_ERR_ARG (null), QH_ERR_BAD_QUBIT, QH_ERR_NONLOCAL as above.      */
typedef struct { uint64_t first, count, px; uint32_t kind, pad; } qh_pauli_run;
int qh_pauli_product_plan(qh_handle h, uint64_t nterms, const uint64_t *xmask, const uint64_t *zmask,
                          qh_pauli_term *terms /* nterms, caller's order; may be NULL */,
                          qh_pauli_run *runs, uint64_t cap, uint64_t *nruns);

/* ---- diagonal Z-polynomial operators (kernels_zpoly.hip.h, zpoly_plan.h) ------- */
/* A classical cost function of the basis state as a polynomial in Z, over LOGICAL bits:
 *   f(i) = sum_t w[t] * (-1)^popcount(i & zmask[t]),   zmask == 0: a constant term.
 * qh_apply_zpoly: a_i *= exp(c * f(i)) in place for any finite complex c = (re, im): c = (0, -gamma) is the QAOA cost layer
 * exp(-i gamma C), c = (-tau, 0) imaginary time under C.  A constant term is applied, not dropped (imaginary c: a global
 * phase).  Terms are taken as given: equal masks are not merged.
 * A barrier, as qh_apply_diag and qh_apply_pauli_product: what is queued runs first and the call works on the layout it finds;
 * bit map, relayout mode and device pointer are as before.  Attached, host-mapped and shard handles, from 1 local bit up, at
 * either width.  The caller's arrays are not referenced after the call returns.
 * ONE kernel, one read and one write of the state, for any nterms <= QH_ZPOLY_MAX_TERMS.  On the layout as it is, the amplitude
 * index splits into a chunk part (item bits 11 and up; an item is 16 bytes) and a low part below it.  A term wholly in the chunk
 * part (or constant) is a scalar per chunk; a term wholly in the low part is a constant of the thread for the whole kernel; a
 * term that straddles is sign_chunk * sign_low, and all straddling terms with the same low mask form one GROUP, one scalar per
 * chunk.  A group whose low mask lies on thread bits only is added once per thread and chunk, one on register-index / half
 * bits only once per chunk; per amplitude that leaves two adds (one more per group of mixed low mask; a 2-local cost function
 * has none), one sincos (and one exp unless c.re == 0), one complex product.  States below one chunk take a
 * one-amplitude-per-thread kernel that sums f by popcount.
 * Shards: a z bit held by the shard index is a sign fixed per shard, folded into w[t] on the host as an exact negation: no
 * Z-polynomial is non-local.
 * Arithmetic: f is summed in double in a fixed order (the chunk scalar and the thread-only groups, + the thread's low sum, + the
 * register-index / half groups, + the mixed groups; groups of a kind in order of first appearance; inside a scalar, the terms in
 * the caller's order dealt to 64 lanes, then an xor tree).  The factor is
 * exp(c.re f) * (cos(c.im f), sin(c.im f)) from the precise device sincos / exp; the product with the amplitude as stored is
 * taken in double (complex64 widened unrounded) and rounded once to the handle's width.
 * norm2 (may be NULL): sum |v|^2 of the final amplitudes as stored, over this shard, in the readers' fixed order without
 * atomics: bitwise reproducible for a given state, layout and term list.
 * nterms == 0 or c == (0, 0): flushes and launches nothing; norm2 is then qh_norm2's.
 * qh_stats: gates_submitted + 1, kernels_launched + 1, bytes_swept and bytes_algorithmic + 2 x the shard's bytes.
 * Errors, nothing runs, nothing changes, nothing is flushed, the whole list is checked first: QH_ERR_ARG (null handle, null
 * arrays with nterms > 0, null c, nterms > QH_ZPOLY_MAX_TERMS, a non-finite weight or c: qh_last_error names the first
 * offending term, dry handle), QH_ERR_BAD_QUBIT (mask bits >= nbits_global).                                               */
#define QH_ZPOLY_MAX_TERMS 4096
int qh_apply_zpoly(qh_handle h, uint64_t nterms, const double *w, const uint64_t *zmask, const double c[2],
                   double *norm2 /* may be NULL */);
/* out[0] = sum |a_i|^2, out[1] = sum |a_i|^2 f(i), out[2] = sum |a_i|^2 f(i)^2 over this shard, not normalised: the norm,
 * <C> and <C^2> of a cost function in ONE kernel and one read of the state for any nterms.  Runs what is queued first and
 * reads only.  The same fixed-order f; three sums in the readers' fixed order: bitwise reproducible.  nterms == 0 gives
 * (qh_norm2, 0, 0).  qh_stats: kernels_launched + 1, bytes_swept and bytes_algorithmic + 1 x the shard's bytes.  Errors as
 * above (null out: QH_ERR_ARG).                                                                                            */
int qh_expect_zpoly(qh_handle h, uint64_t nterms, const double *w, const uint64_t *zmask, double out[3]);
/* How the terms fall on h's layout right now: runs nothing, flushes nothing, planner-only handles too.  Per term, in the
 * caller's order: the physical local mask pz, the weight with the shard's sign folded in, and its class.  low_bits: the
 * amplitude-index bits below the chunk part (the small kernel: all local bits, so every term is constant or low).
 * group_mask[g], g < ngroups: the distinct low masks among the straddling terms, in physical positions, in order of first
 * appearance.  kernel: which kernel would run, on nblk blocks of 256 threads (main: cpb chunks each).  The engine launches
 * from this very function.  Errors: QH_ERR_ARG (null, too many terms, non-finite weight), QH_ERR_BAD_QUBIT.               */
#define QH_ZPOLY_CONST 0
#define QH_ZPOLY_HIGH 1
#define QH_ZPOLY_LOW 2
#define QH_ZPOLY_STRADDLE 3
#define QH_ZPOLY_KERNEL_MAIN 0
#define QH_ZPOLY_KERNEL_SMALL 1
typedef struct {
  uint64_t nterms, nconst, nhigh, nlow, nstraddle, ngroups, nblk;
  uint32_t kernel, low_bits, cpb, pad;
  uint64_t group_mask[QH_ZPOLY_MAX_TERMS];
  uint64_t pz[QH_ZPOLY_MAX_TERMS];
  double w[QH_ZPOLY_MAX_TERMS];
  uint8_t cls[QH_ZPOLY_MAX_TERMS];
} qh_zpoly_info;
int qh_zpoly_plan(qh_handle h, uint64_t nterms, const double *w, const uint64_t *zmask, qh_zpoly_info *out);

/* ---- matrix elements between two states (kernels_transition.hip.h) -------- */
/* out[2t], out[2t + 1] = Re, Im of <a|P_t|b> for Pauli strings given as in qh_expect_pauli, over LOGICAL bits:
 *   <a|P|b> = (-i)^nY * sum_i (-1)^popcount(i & z) * conj(a_i) * b_{i ^ x},   nY = popcount(x & z)
 * summed over this shard's amplitudes matched by logical index, not normalised, in the caller's term order.  x = z = 0 is
 * qh_inner(a, b); a == b is allowed (the real part is then what qh_expect_pauli returns).
 * Handles as in qh_inner: what both have queued runs first, a's stream waits for b's flushed work, the reads run on a's
 * stream and the host waits; nothing of either handle changes.  Both states are read where they lie, through the walk
 * qh_inner_plan(a, b) names, b's index XORed with x in b's physical positions, the sign taken from a's physical index.  No
 * allocation proportional to the state.
 * Shards: as qh_inner, the handles must hold the same logical bits in the shard index, at the same positions, with the same
 * shard index (QH_ERR_NONLOCAL).  A z bit the shard index holds is a sign fixed on this shard, folded in on the host; an x
 * bit there is QH_ERR_NONLOCAL.
 * Passes: terms are stably sorted by x mask and every group is cut each QH_TRANSITION_BATCH terms at complex128, each
 * QH_TRANSITION_BATCH / 2 at complex64 (qh_transition_plan reports the passes actually cut); one kernel per pass, one pass
 * reads each state once.  a's qh_stats: kernels_launched += passes (the folds are not counted), bytes_swept and
 * bytes_algorithmic += 2 x the shard's bytes per pass; b's are unchanged.
 * Every product and sum is formed in double from the amplitudes as stored, in a fixed order without float atomics: the same
 * states, layouts and term list give the same bits.  (-i)^nY and the shard sign are swaps and negations.  nterms = 0 flushes
 * both handles and launches nothing.
 * Errors, nothing runs, out untouched, the whole list checked first: QH_ERR_ARG (null handle, null arrays or out with
 * nterms > 0, dry handle, another device, different nbits (local or global) or width), QH_ERR_BAD_QUBIT (mask bits >=
 * nbits_global; checked before the dry-handle refusal), QH_ERR_NONLOCAL as above (nothing is flushed).                    */
#define QH_TRANSITION_BATCH 16
int qh_transition_pauli(qh_handle a, qh_handle b, uint64_t nterms, const uint64_t *xmask, const uint64_t *zmask,
                        double *out /* 2 per term: re, im */);
/* How qh_transition_pauli would run these strings right now: host arithmetic on the two bit maps, runs nothing, flushes
 * nothing, planner-only handles are allowed and the devices are not compared.  terms (sorted order; may be NULL): px is the x
 * mask in B's physical local positions, pz the z mask in A's, neg the shard sign, ny = nY mod 4, index the caller's term.
 * passes (at most cap are written, *npasses is their number): terms [first, first + count) in one kernel, px their common x
 * mask, walk the QH_INNER_* path.  The engine launches from this very function.  Errors: QH_ERR_ARG (null, different nbits
 * or width), QH_ERR_BAD_QUBIT, QH_ERR_NONLOCAL as above.                                                                   */
typedef struct { uint64_t first, count, px; uint32_t walk /* QH_INNER_* */, pad; } qh_transition_pass;
int qh_transition_plan(qh_handle a, qh_handle b, uint64_t nterms, const uint64_t *xmask, const uint64_t *zmask,
                       qh_pauli_term *terms /* nterms, sorted order; may be NULL */,
                       qh_transition_pass *passes, uint64_t cap, uint64_t *npasses);

/* ---- growing and shrinking a state (kernels_resize.hip.h) ----------------- */
/* Both calls make a NEW handle and leave src as qh_clone leaves it: what src has queued runs first (exchange arrivals are
 * waited for); src keeps its amplitudes, bit map, relayout mode and device pointer.  The new handle lives on src's device with
 * src's width, shard index and fusion level, always owns HBM memory and a stream of its own (also beside an attached or
 * host-mapped src), starts with zeroed stats, nothing queued, relayout mode undecided and no communicator, and is complete
 * when the call returns.  src's qh_stats.kernels_launched grows by 1, bytes_algorithmic and bytes_swept by the bytes of src
 * (read once) plus the bytes of the new state (written once).  Beside a planner-only src the new handle is planner-only: the
 * new sizes and bit map, no data, weight untouched.
 * Errors of both: QH_ERR_ARG (null pointer, k outside [1,16], a resulting local size outside [1,40] or global size above
 * 62), QH_ERR_NOMEM (nothing is created).
 *
 * qh_extend: new state = src (x) f in np.kron order.  The k new qubits are the k least significant LOGICAL bits; logical bit
 * b of src becomes b + k.  f = amps, 2^k complex128 values (interleaved re,im, as in qh_init_product; not referenced after
 * the call returns), or, where amps is NULL, the basis state |basis> (basis >= 2^k: QH_ERR_ARG).  Nothing of src is re-laid
 * out: the new bits sit at physical positions nbits_local .. nbits_local + k - 1, every local bit of src keeps its position,
 * every bit held by the shard index moves up by k: new[(j << nbits_local) | p] = f[j] * src[p], one read of src, 2^k linear
 * writes (zeros where f[j] is 0).  One complex product per amplitude in the handle's width; entries that are exactly 0 or 1
 * give 0 or the stored amplitude, equal as numbers.  Shard handles: the new bits are local on every shard.               */
int qh_extend(qh_handle src, int k, const double *amps, uint64_t basis, qh_handle *out);
/* qh_release: new state = the slice of src where LOGICAL bit bits[j] has the value of bit j of `value`, for the k distinct bits
 * listed (value >= 2^k: QH_ERR_ARG; QH_ERR_BAD_QUBIT, QH_ERR_SAME_QUBIT; at least one local qubit must remain).  A listed bit
 * held by the shard index is QH_ERR_NONLOCAL: nothing is created, weight untouched.  The remaining bits keep their order,
 * logically and physically, and are renumbered densely: logical l becomes l - (listed bits below l), physical p becomes
 * p - (released positions below p).  Amplitudes are copied as stored; nothing is rescaled (qh_scale).  weight (may be NULL):
 * weight[0] = sum |a|^2 of the amplitudes kept, weight[1] = of those dropped, over this shard, not normalised, summed in
 * double in a fixed order (bitwise reproducible for a given state and layout).  One kernel, one read of src.              */
int qh_release(qh_handle src, int k, const int32_t *bits, uint64_t value, double weight[2], qh_handle *out);

/* ---- measurement of the engine itself ----------------------------------- */
typedef struct {
  uint64_t gates_submitted;   /* qh_apply* calls accepted                      */
  uint64_t kernels_launched;  /* gate/sweep kernels launched                   */
  uint64_t sweeps;            /* fused sweep launches                          */
  uint64_t bytes_algorithmic; /* minimal-touch bytes of the gates  */
  uint64_t bytes_swept;       /* bytes the launched kernels had to move        */
  uint64_t gates_noop;        /* gates skipped by shard-bit predicate          */
} qh_stats;
int qh_get_stats(qh_handle h, qh_stats *out);
int qh_reset_stats(qh_handle h);
/* hipEvent pair on the handle's stream.                                      */
int qh_timer_begin(qh_handle h);
int qh_timer_end(qh_handle h, float *milliseconds);
/* Lap marks: qh_timer_lap flushes what is queued and records an event on the stream (no host wait);
 * qh_timer_laps waits for the last mark, writes the milliseconds between consecutive marks (at most cap),
 * sets *count to the number of intervals and forgets the marks.  Per-step times of a loop without stalling it. */
int qh_timer_lap(qh_handle h);
int qh_timer_laps(qh_handle h, float *milliseconds, int cap, int *count);
/* JSON text of the sweeps the planner would launch for the current queue
 * (does not launch or clear).  Returns bytes needed; writes at most cap.     */
int qh_plan_json(qh_handle h, char *buf, uint64_t cap, uint64_t *needed);

/* The same plan in binary form, complete (ops, phase groups, tables): 3 x u64 (magic
 * 0x51485033, sweeps, gates dropped as no-ops), 64 bytes final_pos (position after the flush of
 * the index bit at each position before it), then per sweep 28 x i64 (rb, regpos[6],
 * regpos_store[6], lanehi[3], nwave, wavepos[2], fixed_ones, ntiles, #ops, #groups, #oterms,
 * #table doubles, #lane tables, lane_low, relayout), 64 bytes dest_pos, 20 x i64 (seat[6]: the index
 * bit on each lane bit when the tile is loaded, seat_store[6]: when it is stored, seat_dest[6]: the
 * position 0..5 a relayout store sends it to, wavepos at store time [2]), 25 x i64 (relayout store as the kernel gets it: reg_dest[6], wave_dest[2], number of
 * unit-index runs, 8 masks, 8 shifts), followed by the SweepOp / DGroup / OTerm / table arrays of
 * qcc_amd/csrc/planner.h, each padded to 8 bytes.  For tools and tests that check a plan
 * without a GPU (tests/plan_interp.py executes it with NumPy).                 */
int qh_plan_export(qh_handle h, void *buf, uint64_t cap, uint64_t *needed);

/* What the sweep kernels would DISPATCH for the current queue: the plan of qh_plan_export as a flush hands it to
 * the device (does not launch or clear; planner-only and live handles alike).  Same calling convention.  u32 words:
 * magic 0x51484831, number of sweeps, then per sweep bit_width, rb, nwave, relayout, n_ops, n_groups, the device
 * `kind` and `flags` words of every op (kind: OP_* | handler number << 16; the sentinel that ends the list is left
 * out) and the device `flags` word of every group (handler in bits 8..15, general path bit 2, sign-flip outside
 * terms bit 4); padded to 8 bytes.  Built by the function the flush builds its upload with
 * (qcc_amd/csrc/kernels_sweep.hip.h build_device_copy): tests use it to say which island handlers a circuit runs. */
int qh_plan_handlers(qh_handle h, void *buf, uint64_t cap, uint64_t *needed);

/* ---- literal drop-in on host buffers (what `libxgates` binds) ----------- */
/* psi: host pointer to 2^nbits complex numbers of width bit_width, updated in
 * place (H2D, kernel, D2H -- PCIe inclusive).  gate: 8 doubles.              */
int qh_host_apply1(void *psi, const double gate[8], int nbits, int tgt,
                   int bit_width);
int qh_host_applyc(void *psi, const double gate[8], int nbits, int ctl, int tgt,
                   int bit_width);
/* The two calls above keep device scratch per calling thread (the two most recent register
 * shapes); this frees the calling thread's.  Safe to call at any time, from any thread.       */
int qh_host_release(void);

#ifdef __cplusplus
}
#endif
#endif /* QCC_HIP_H_ */
