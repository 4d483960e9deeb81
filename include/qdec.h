/*
 * qdec.h -- C ABI of libqdec_hip.so, the MI355X (gfx950) BP + small-set-flip
 * syndrome decoder.
 *
 * This is the drop-in boundary for the reference's decoding hot path.  In the
 * reference (qldpc/exp_ldpc @ 2025-02-21) that boundary is the third-party
 * `ldpc` v1 decoder-object API, called only from python/qldpc/misc/_experiment.py:
 *   - construction  bposd_decoder(H, error_rate=.., **opts)     _experiment.py:23-27, 96-100
 *                   bposd_decoder(H, channel_probs=.., **opts)  _experiment.py:37-40
 *                   bposd_decoder(H, channel_prior=.., **opts)  _experiment.py:77
 *                   bp_decoder(H, channel_probs=.., **opts)     _experiment.py:110-113, 137-140
 *   - decode        .decode(syndrome) -> ndarray[n]             _experiment.py:51, 59, 82, 117, 125, 149
 *   - per-shot logical check  any(GF2(Lz) @ GF2(readout))       _experiment.py:209
 * Each entry point below names the reference interface it replaces.  The Python
 * binding (exp_ldpc_amd/_abi.py, ctypes) and the ldpc-v1-compatible classes are
 * described in INTEGRATION.md.
 *
 * Conventions: plain pointers and sizes; no C++ exceptions cross the ABI; status
 * 0 = OK, negative = error (message via qd_last_error(), thread-local).  The
 * library owns device copies of the graph; the caller owns every buffer it
 * passes.  A handle is used from one host thread at a time; one handle per
 * device for multi-GPU.  Device-buffer decodes on one handle may be enqueued on
 * different streams: the handle's SSF queue and message scratch are shared, so
 * the library chains such calls with an event (a call waits for the previous
 * call's kernels) and frees a grown buffer only after its last use completed.
 * Calls on one handle therefore never run concurrently; use one handle per
 * stream for concurrent decodes.
 */
#ifndef QDEC_H
#define QDEC_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define QDEC_ABI_VERSION 1

typedef struct qd_graph qd_graph;

enum qd_method { QD_PRODUCT_SUM = 0, QD_MIN_SUM = 1 };      /* ldpc bp_method 'ps' / 'ms','msl' */
enum qd_precision { QD_F64 = 0, QD_F32 = 1 };               /* message arithmetic */
/* syn_flags bits.  QD_INPUT_PACKED: the decode's syn / base / readout inputs are
 * bit-packed rows of little-endian u64 words instead of one byte per bit:
 * syn [B][ceil(m/64)], base / readout [B][ceil(n_data/64)], bit j of word w =
 * element 64 w + j, padding bits ignored, 8-B aligned.  Byte for byte this is
 * Stim's sample(bit_packed=True) layout (the reference sampler,
 * _experiment.py:196-197) with each row zero-padded to a multiple of 8 bytes.
 * Outputs keep their layouts. */
enum qd_syn_flags { QD_SYN_ADD_BASE = 1, QD_SYN_ADD_READOUT = 2, QD_INPUT_PACKED = 16 };
enum qd_status_bits { QD_ST_BP_CONVERGED = 1, QD_ST_SATISFIED = 2 };

typedef struct qd_params {
    int32_t max_iter;      /* <= 0 -> n (ldpc v1: max_iter=0 means n) */
    int32_t method;        /* enum qd_method */
    int32_t precision;     /* enum qd_precision */
    int32_t ssf;           /* 1: small-set-flip on shots BP did not converge (needs flip sets) */
    int32_t ssf_max_steps; /* <= 0: unbounded (terminates: |residual| strictly decreases) */
    int32_t syn_flags;     /* enum qd_syn_flags: syndrome ^= H[:, :n_data] (base ^ readout) */
    double ms_scaling;     /* 0 -> alpha_t = 1 - 2^-t (ldpc ms_scaling_factor=0) */
} qd_params;

/* Version / device discovery. */
int qd_abi_version(void);
int qd_device_count(void);
const char* qd_last_error(void);

/* Replaces the ldpc constructor's copy of H into mod2sparse (_experiment.py:23,
 * 37, 77, 96, 110, 137).  H is m x n CSR with column indices sorted within each
 * row (row_ptr[m+1], col_idx[row_ptr[m]]).  Columns t*n_data + q (t <
 * fold_blocks) fold onto data qubit q (SpacetimeCode.final_correction,
 * spacetime_code.py:81-84); fold_blocks = 1, n_data = n for a plain code.  The
 * graph is uploaded to `device` (HIP ordinal). */
int qd_graph_create(int32_t m, int32_t n, const int32_t* row_ptr, const int32_t* col_idx,
                    int32_t n_data, int32_t fold_blocks, int32_t device, qd_graph** out);
int qd_graph_destroy(qd_graph* g);

/* Host-only graph: the same validation and host tables as qd_graph_create
 * (kernel layouts and anneals, flip-set and logical tables, priors) with no
 * device and no HIP call; the tables are kept in host memory.  For CPU tests
 * and sanitizer runs (tools/sanitize.sh); decode calls on it fail.
 * qd_graph_table_digest returns an FNV-1a digest and the byte count of every
 * table built so far.  No reference counterpart. */
int qd_graph_create_host(int32_t m, int32_t n, const int32_t* row_ptr, const int32_t* col_idx, int32_t n_data,
                         int32_t fold_blocks, qd_graph** out);
int qd_graph_table_digest(const qd_graph* g, uint64_t* digest, int64_t* bytes);

/* Flip sets for small-set-flip: generator rows (CSR over H's columns; for the
 * storage experiment the X-check rows of Hx).  Each generator must have <= 8
 * qubits whose checks in H number <= 32.  No reference counterpart (SSF is
 * absent from the reference). */
int qd_graph_set_flipsets(qd_graph* g, int32_t n_gen, const int32_t* gen_ptr, const int32_t* gen_idx);

/* Logical operators for the fused failure check, dense 0/1 k x n_data (the `LZ`
 * rows of the qecc file; replaces GF2(logicals.z) @ GF2(readout) at
 * _experiment.py:209). */
int qd_graph_set_logicals(qd_graph* g, int32_t k, const uint8_t* lz);

/* The same logicals as a CSR over data qubits (row r = the support of logical r,
 * lz_ptr[k+1], lz_idx[nnz] in [0, n_data), duplicates cancel mod 2).  For codes
 * with many sparse logicals (the PSL(2,16) Cayley-graph LP code of config 5:
 * k = 4080 of weight 3, n = 53,040) where the dense k x n_data form is hundreds
 * of MB; the workgroup kernels then test each logical on its support only. */
int qd_graph_set_logicals_csr(qd_graph* g, int32_t k, const int32_t* lz_ptr, const int32_t* lz_idx);

/* Per-column error probabilities (ldpc `error_rate` broadcast / `channel_probs`;
 * reference call sites _experiment.py:23-27, 37-40, 74-77, 106-113).  Converted
 * on the host to the ldpc initial messages log((1-p)/p) (min-sum) and p/(1-p)
 * (product-sum) in both precisions, and to the fault sampler's thresholds
 * (qd_sample_faults_device).  Probabilities lie in [0, 1] (-51 otherwise); a 0
 * or a 1 among them leaves a graph that samples but does not decode (BP has no
 * finite message for it: decodes return -51). */
int qd_graph_set_priors(qd_graph* g, const double* channel_probs);

/* Batched replacement of B calls to .decode(syndrome) (_experiment.py:82, 117,
 * 125, ...), plus the fused fold and logical check.  Host buffers; synchronous.
 *   syn       uint8 [B][m]       syndrome bits (nullable when syn_flags set)
 *   base      uint8 [B][n_data]  xor-ed into corr_out (and into the syndrome with
 *                                QD_SYN_ADD_BASE); nullable
 *   readout   uint8 [B][n_data]  data readout for the failure flag (and the
 *                                syndrome with QD_SYN_ADD_READOUT); nullable
 * outputs (each nullable):
 *   x_out     uint8 [B][n]       decoding (BP hard decision, SSF applied) = ldpc .decode() result
 *   corr_out  uint8 [B][n_data]  base ^ fold(x_out)
 *   llr_out   [B][n] float (QD_F32) or double (QD_F64): ldpc .log_prob_ratios
 *   iters     int32 [B]          ldpc .iter
 *   status    uint8 [B]          QD_ST_BP_CONVERGED (= ldpc .converge) | QD_ST_SATISFIED
 *   ssf_steps int32 [B]          flips applied by SSF
 *   fail      uint8 [B]          any(Lz (readout ^ corr_out)) mod 2 (needs logicals+readout) */
int qd_decode_batch(qd_graph* g, const qd_params* prm, int64_t B,
                    const uint8_t* syn, const uint8_t* base, const uint8_t* readout,
                    uint8_t* x_out, uint8_t* corr_out, void* llr_out,
                    int32_t* iters, uint8_t* status, int32_t* ssf_steps, uint8_t* fail);

/* Same contract on device-resident buffers (HBM), enqueued on `stream`
 * (hipStream_t; NULL = default stream); returns after the launch. */
int qd_decode_batch_device(qd_graph* g, const qd_params* prm, int64_t B,
                           const uint8_t* syn, const uint8_t* base, const uint8_t* readout,
                           uint8_t* x_out, uint8_t* corr_out, void* llr_out,
                           int32_t* iters, uint8_t* status, int32_t* ssf_steps, uint8_t* fail,
                           void* stream);

/* Replaces Stim's compile_sampler().sample(B) + StorageSim slicing +
 * _spacetime_syndrome (_experiment.py:196-207, storage_sim.py:187-196,
 * spacetime_code.py:98-119) for the storage experiment under
 * depolarizing_noise(p_data, pm=p_meas) (noise_model.py:117-123).  The graph must
 * be a plain code (fold_blocks = 1): H = Hz.  Writes, on device:
 *   syn     uint8 [B][(rounds+1)*m]  spacetime (difference) syndrome
 *   readout uint8 [B][n]             transversal Z readout
 * Philox4x32-10 keyed (seed, stream_id), counter (word, event, shot): results
 * do not depend on how shots are split across calls or devices. */
int qd_sample_storage_device(qd_graph* g, int32_t rounds, double p_data, double p_meas,
                             uint32_t seed, uint32_t stream_id, int64_t shot0, int64_t B,
                             uint8_t* syn, uint8_t* readout, void* stream);
/* The same shots, written bit-packed (the QD_INPUT_PACKED layout):
 *   syn     uint64 [B][ceil((rounds+1)*m/64)]   readout uint64 [B][ceil(n/64)]
 * 8-B aligned buffers.  With rounds = 0 the rows feed qd_decode_batch_device
 * with QD_INPUT_PACKED directly (42 B per shot at n = 225 instead of 333). */
int qd_sample_storage_packed_device(qd_graph* g, int32_t rounds, double p_data, double p_meas,
                                    uint32_t seed, uint32_t stream_id, int64_t shot0, int64_t B,
                                    uint64_t* syn, uint64_t* readout, void* stream);

/* Draw B shots of the graph's own faults: column j fires with the probability last
 * given to qd_graph_set_priors.  Replaces Stim's compile_detector_sampler().sample
 * (_experiment.py:193-194) for a DEM whose fault check matrix is this graph.
 *   det    [B][m] u8, or with QD_INPUT_PACKED in flags u64 [B][ceil(m/64)]: H e
 *   faults [B][n] u8 / u64 [B][ceil(n/64)]: e itself (nullable) -- pass it as the
 *          decode's `readout`: with the fault map as logicals, fail = any(obs ^ F x)
 *   obs    [B][k] u8: F e (nullable; needs logicals)
 * Fault j fires when u < thr[j]: u = lane j % 4 of the Philox4x32-10 block with
 * key (seed, stream_id) and counter (j / 4, 0, shot), shot = shot0 + row (64
 * bits); thr[j] = floor(p_j 2^32) clamped to 2^32 - 1 (0 for p_j = 0), the
 * storage sampler's conversion.  Results do not depend on how shots are split
 * across calls, streams or devices.  Padding bits of packed rows are written 0.
 * For sampling, qd_graph_set_priors takes probabilities in [0, 1]; a graph whose
 * priors hold a 0 or a 1 can be sampled but not decoded (-51).  B = 0 returns 0
 * and writes nothing.  Errors: -16 host-only graph, -60 B < 0 or unknown flags,
 * -63 priors never set, -64 folded graph (fold_blocks != 1 or n_data != n),
 * -65 obs without logicals, -66 det null, -67 packed buffer not 8-B aligned. */
int qd_sample_faults_device(qd_graph* g, uint32_t seed, uint32_t stream_id, int64_t shot0, int64_t B,
                            int32_t flags, void* det, void* faults, uint8_t* obs, void* stream);
/* Host-only graphs, for tests: the sampler's tables, thr[n] (above) and crow[nnz]
 * (the row of each edge in column-major order: column j's rows, ascending, at
 * crow[colptr[j] .. colptr[j+1])).  Either may be NULL.  -63 before the first
 * qd_graph_set_priors. */
int qd_graph_sample_tables_copy(const qd_graph* g, uint32_t* thr, int32_t* crow);

/* Pauli-frame sampling of a compiled circuit: replaces Stim's
 * compile_sampler().sample / compile_detector_sampler().sample (_experiment.py:
 * 193-197) for circuits of the storage experiment's gate set under any noise
 * rewriter (noise_model.py:117-151).  A circuit is not a graph and has a handle
 * of its own.  The program (built by exp_ldpc_amd/circuit.py):
 *   ops      int32 [n_ops][4]: opcode, first target, target count, first
 *            argument (0 unless the opcode takes arguments).  Opcodes:
 *            0 H, 1 CX, 2 CZ, 3 R, 4 RX, 5 M, 6 MX, 7 X_ERROR, 8 Y_ERROR,
 *            9 Z_ERROR, 10 DEPOLARIZE1, 11 DEPOLARIZE2, 12 PAULI_CHANNEL_1,
 *            13 PAULI_CHANNEL_2 (CX, CZ, DEPOLARIZE2, PAULI_CHANNEL_2: targets in
 *            pairs).  MR / MRX are an M / MX followed by an R / RX.
 *   targets  int32 [n_targets]: qubit indices; a measurement target with bit 30
 *            set has its record inverted (a reference sample of 1)
 *   probs    double [n_ops]: the probability of a noise instruction, the record
 *            flip probability of a measurement, 0 otherwise; converted to u32
 *            thresholds as in qd_sample_faults_device
 *   args     double [n_args] (qd_circuit_create_args / _create_host_args only):
 *            PAULI_CHANNEL_1 reads 3 entries from its first argument on, the
 *            probabilities of X, Y, Z; PAULI_CHANNEL_2 reads 15, those of the
 *            two-qubit codes 1 .. 15 (Stim's order IX, IY, IZ, XI, .. ZZ: first
 *            qubit's Pauli = code >> 2, second's = code & 3; 0 I, 1 X, 2 Y, 3 Z).
 *            Its entry of probs is their sum c_{K-1}, with c_k = c_{k-1} + a_k
 *            in double, left to right
 *   groups   up to 4 output groups; group g has group_rows[g] rows, each the
 *            parity of a set of measurement records: one CSR over absolute
 *            record indices, the groups' rows concatenated (row_ptr[rows + 1],
 *            rec_idx[row_ptr[rows]]); duplicates in a row cancel mod 2
 * The targets of one H / CX / CZ / R / RX / M / MX instruction are applied in
 * parallel and must be pairwise disjoint (the compiler splits Stim's in-order
 * target lists into such groups).  The number of measurements M is the total
 * target count of the M / MX instructions, record i being the i-th such target.
 * Create validates every index and refuses a bad program: -71 malformed arrays
 * (sizes, opcode, target range, odd pair count, CSR bounds), -72 qubit index out
 * of range, -73 record reference outside [0, M), -74 a qubit twice in one
 * parallel group, -75 probability outside [0, 1], -76 the circuit needs more
 * than 160 KiB of LDS (16 B per qubit + 8 B per measurement), -15 device
 * ordinal.  qd_circuit_create_host validates only and makes no HIP call.
 * qd_circuit_create_args / qd_circuit_create_host_args are qd_circuit_create_placed
 * / _create_host_placed with the argument array in front of `out`; only they take
 * opcodes 12 and 13 (the four others refuse them as unknown, -71).  Further
 * refusals: -71 n_args < 0, an instruction's arguments outside the array, or a
 * non-zero first argument on any other opcode; -75 an argument outside [0, 1], a
 * sum above 1 + 1e-12, or an entry of probs further than 1e-12 from the sum.
 * qd_circuit_info: out[10] = qubits, measurements, rows of groups 0..3, LDS
 * bytes (16 Q + 8 M under every placement), instructions, Bernoulli / Pauli draw
 * sites, randomisation sites.
 *
 * Frame placement.  The kernels keep the frame (x[Q], z[Q], rec[M], a u64 word
 * per 64 shots) either in LDS or, per resident workgroup, in a slot of 16 Q + 8 M
 * bytes of a scratch in device memory the handle owns.  Both placements give the
 * same bits.  qd_circuit_create_placed / qd_circuit_create_host_placed take the
 * placement in front of the arguments of qd_circuit_create / _create_host:
 *   QD_FRAME_LDS   the two entry points above, -76 included
 *   QD_FRAME_HBM   always the HBM kernels, at any size
 *   QD_FRAME_AUTO  LDS when 16 Q + 8 M <= 160 KiB, else HBM
 * Validation and its codes are the same; -96 for any other placement.  The int32
 * limits hold under every placement (-71): fewer than 2^31 draw sites and
 * randomisation sites, 2^28 records, 2^30 noise faults.
 * qd_circuit_set_frame_slots: slots (resident workgroups) of the HBM kernels'
 * launches; 0 = the default, 8 per compute unit; a launch uses min(slots, 64-shot
 * words).  -98 for slots < 0 or > 2^20.  Results do not depend on it.
 * qd_circuit_frame_info: out[4] = the placement in effect (QD_FRAME_LDS or
 * QD_FRAME_HBM), bytes per slot (16 Q + 8 M), slots of the last HBM launch,
 * scratch bytes held.
 * qd_circuit_op_flags_copy: dup[n_ops] = 1 for a noise instruction that names a
 * qubit more than once (legal: X_ERROR 0 1 0), else 0.  The HBM sampler applies
 * the sites of such an instruction one after the other, every other noise
 * instruction 64 sites at a time; site numbers are the same either way.
 * The scratch is allocated at the first HBM launch and grown when a launch wants
 * more slots.  When the allocation fails the slot count is halved down to one;
 * only then the launch fails with -97.  Launches on one handle from different
 * streams are chained with an event (the second waits for the first), so no two
 * share live slots. */
#define QD_FRAME_LDS 0
#define QD_FRAME_HBM 1
#define QD_FRAME_AUTO 2
typedef struct qd_circuit qd_circuit;
int qd_circuit_create(int32_t device, int32_t num_qubits, int32_t n_ops, const int32_t* ops, int32_t n_targets,
                      const int32_t* targets, const double* probs, int32_t n_groups, const int32_t* group_rows,
                      const int32_t* row_ptr, const int32_t* rec_idx, qd_circuit** out);
int qd_circuit_create_host(int32_t num_qubits, int32_t n_ops, const int32_t* ops, int32_t n_targets,
                           const int32_t* targets, const double* probs, int32_t n_groups, const int32_t* group_rows,
                           const int32_t* row_ptr, const int32_t* rec_idx, qd_circuit** out);
int qd_circuit_create_placed(int32_t placement, int32_t device, int32_t num_qubits, int32_t n_ops,
                             const int32_t* ops, int32_t n_targets, const int32_t* targets, const double* probs,
                             int32_t n_groups, const int32_t* group_rows, const int32_t* row_ptr,
                             const int32_t* rec_idx, qd_circuit** out);
int qd_circuit_create_host_placed(int32_t placement, int32_t num_qubits, int32_t n_ops, const int32_t* ops,
                                  int32_t n_targets, const int32_t* targets, const double* probs, int32_t n_groups,
                                  const int32_t* group_rows, const int32_t* row_ptr, const int32_t* rec_idx,
                                  qd_circuit** out);
int qd_circuit_create_args(int32_t placement, int32_t device, int32_t num_qubits, int32_t n_ops, const int32_t* ops,
                           int32_t n_targets, const int32_t* targets, const double* probs, int32_t n_groups,
                           const int32_t* group_rows, const int32_t* row_ptr, const int32_t* rec_idx, int32_t n_args,
                           const double* args, qd_circuit** out);
int qd_circuit_create_host_args(int32_t placement, int32_t num_qubits, int32_t n_ops, const int32_t* ops,
                                int32_t n_targets, const int32_t* targets, const double* probs, int32_t n_groups,
                                const int32_t* group_rows, const int32_t* row_ptr, const int32_t* rec_idx,
                                int32_t n_args, const double* args, qd_circuit** out);
int qd_circuit_set_frame_slots(qd_circuit* c, int64_t slots);
int qd_circuit_frame_info(const qd_circuit* c, int64_t out[4]);
int qd_circuit_op_flags_copy(const qd_circuit* c, int32_t* dup);
int qd_circuit_destroy(qd_circuit* c);
int qd_circuit_info(const qd_circuit* c, int64_t out[10]);
/* B shots, global indices shot0 .. shot0 + B, enqueued on `stream`.  outs[g]:
 * group g's rows, u8 [B][rows_g], or with QD_INPUT_PACKED in flags u64
 * [B][ceil(rows_g / 64)] (the decode's packed layout, padding bits written 0,
 * 8-B aligned); NULL skips the group.  Frame rules (Stim's frame simulator, bits
 * (x, z) per qubit and shot): H swaps x and z; CX c t: x_t ^= x_c, z_c ^= z_t;
 * CZ a b: z_a ^= x_b, z_b ^= x_a; M q: record = x_q ^ flip (^ invert), then
 * z_q ^= a random bit; MX q: record = z_q ^ flip, then x_q ^= a random bit;
 * R q: x_q = 0, z_q = a random bit; RX q: z_q = 0, x_q = a random bit; qubits
 * start with x = z = 0.  The record is the flip against the noiseless reference
 * sample, taken as all zero unless a target's invert bit says otherwise.
 * Draws, Philox4x32-10 keyed (seed, stream_id):
 *   Bernoulli / Pauli site s, shot g: u = lane s % 4 of the block with counter
 *     (s / 4, 0, g_lo, g_hi); the site fires when u < T.  DEPOLARIZE1 applies
 *     Pauli 1 + floor(3 u / T) (1 X, 2 Y, 3 Z); DEPOLARIZE2 draws code 1 +
 *     floor(15 u / T) and applies Pauli code >> 2 to the pair's first qubit and
 *     code & 3 to its second (0 I).  PAULI_CHANNEL_1 / 2 with arguments a_0 ..
 *     a_{K-1} (K = 3 / 15): C_k = the u32 threshold of c_k; T = C_{K-1}; a fired
 *     site applies Pauli (PAULI_CHANNEL_1) or code (PAULI_CHANNEL_2, as
 *     DEPOLARIZE2) 1 + #{j < K : C_j <= u}, so an outcome whose argument is 0 never
 *     occurs.  Sites number the targets (pairs for DEPOLARIZE2 and
 *     PAULI_CHANNEL_2) of the noise and measurement instructions in program order,
 *     each instruction starting at the next multiple of 4.
 *   randomisation site r, shot g: bit g % 32 of lane (g / 32) % 4 of the block
 *     with counter (r, 1, (g / 128)_lo, (g / 128)_hi); sites number the targets
 *     of R, RX, M, MX in program order.
 * Results therefore do not depend on shot0, on how shots are split across
 * calls, streams or devices, or on alignment.  B = 0 returns 0 and writes
 * nothing.  Errors: -77 B < 0, unknown flags or a buffer for a group the circuit
 * lacks, -78 packed buffer not 8-B aligned, -79 host-only circuit, -97 no memory
 * for one frame slot (HBM placement). */
int qd_circuit_sample_device(qd_circuit* c, uint32_t seed, uint32_t stream_id, int64_t shot0, int64_t B,
                             int32_t flags, void* const outs[4], void* stream);

/* Fault propagation through a compiled circuit: what Stim's
 * circuit.detector_error_model() (_experiment.py:174) starts from.  The library
 * derives the circuit's elementary faults from the program; their numbering does
 * not depend on the probabilities (instructions with p = 0 are numbered too).
 *   noise faults (kind 0), in program order:
 *     X_ERROR / Y_ERROR / Z_ERROR: one per target, the named Pauli (Y: x and z);
 *     DEPOLARIZE1: two per target, fault 2e = X on target e, 2e + 1 = Z;
 *     DEPOLARIZE2: four per pair: X_a, Z_a, X_b, Z_b;
 *     PAULI_CHANNEL_1 / PAULI_CHANNEL_2: as DEPOLARIZE1 / DEPOLARIZE2;
 *     M / MX: one per target, a flip of that record (MR(p) is an M(p) then an R).
 *   gauge faults (kind 1): one per randomisation site in the sampler's site order
 *     (the targets of R, RX, M, MX, the opening R included); the injected bit is
 *     the component the sampler randomises there: z after R and M, x after RX
 *     and MX.
 * qd_circuit_fault_info: out[4] = noise faults, gauge faults, 0, 0.
 * qd_circuit_fault_table: per fault of `kind` the instruction index, the index
 * into `targets` and the component (1 x, 2 z, 3 both, 4 a record flip); arrays
 * of the kind's fault count.  Both are host-only (no HIP call).
 * qd_circuit_faults_device: faults f0 .. f0 + F of one kind, enqueued on
 * `stream`; outs[g] as in qd_circuit_sample_device with a fault where that call
 * has a shot: u8 [F][rows_g], or with QD_INPUT_PACKED u64 [F][ceil(rows_g / 64)],
 * padding bits 0.  Row f is the symptom of fault f alone: the record flips it
 * causes in an otherwise noiseless run.  Frame rules as the sampler's without any
 * randomisation: qubits start with x = z = 0; R and RX clear both components;
 * M q: record = x_q, MX q: record = z_q, the other component is left alone; invert
 * bits do not apply (a flip is not inverted).  A fault is injected after its own
 * instruction's work: a record flip XORs the record just written, a gauge fault
 * the component just reset or measured against.  Every argument is checked
 * before anything is enqueued, in this order: -87 kind outside {0, 1}, -88 f0 < 0
 * or F < 0, -89 f0 + F beyond the kind's fault count, -77 unknown flags, -79
 * host-only circuit, -77 a buffer for a group the circuit lacks, -78 packed
 * buffer not 8-B aligned.  F = 0 returns 0 and writes nothing. */
int qd_circuit_fault_info(const qd_circuit* c, int64_t out[4]);
int qd_circuit_fault_table(const qd_circuit* c, int32_t kind, int32_t* op, int32_t* target, int32_t* comp);
int qd_circuit_faults_device(qd_circuit* c, int32_t kind, int64_t f0, int64_t F, int32_t flags, void* const outs[4],
                             void* stream);

/* Ordered-statistics decoding of shots BP did not converge on (the OSD stage of
 * ldpc v1 bposd_decoder; reference _experiment.py:23-27, 37-40, 77, 96-100).  Host
 * buffers; runs on the host cores (nthreads <= 0: all).  method: 0 = osd0,
 * 1 = osd_e, 2 = osd_cs; order = osd_order.  llr = BP log-probability ratios
 * (qd_decode_batch llr_out widened to double).  Outputs osd0 and the best
 * higher-order solution (ldpc .osd0_decoding / .osdw_decoding), uint8 [B][n]. */
int qd_osd_batch(int32_t m, int32_t n, const int32_t* row_ptr, const int32_t* col_idx, int32_t method,
                 int32_t order, int64_t B, const uint8_t* syn, const double* llr, uint8_t* osd0_out,
                 uint8_t* osdw_out, int32_t nthreads);
const char* qd_osd_last_error(void);

/* The same OSD on the GPU, on device-resident buffers, enqueued on `stream`
 * (hipStream_t).  Graph = the BP graph handle (H, fold and logicals).  Shots with
 * status bit QD_ST_BP_CONVERGED set are skipped (status nullable: all shots).
 * llr: [B][n] float (QD_F32) or double (QD_F64), the BP .log_prob_ratios; the
 * syndrome is syn (^ H[:, :n_data] base/readout per syn_flags, as in
 * qd_decode_batch).  Outputs for processed shots (each nullable): osd0_out,
 * osdw_out [B][n] (ldpc .osd0_decoding / .osdw_decoding), corr_out = base ^
 * fold(osdw), fail = any(Lz (readout ^ corr_out)).  Bit-identical to
 * qd_osd_batch.  Needs a graph a device kernel holds (qd_osd_device_supported):
 * m <= 384 and n < 1024 for the register kernel, an LDS image of at most 160 KiB
 * for the workgroup kernel; otherwise -85. */
int qd_osd_device_supported(const qd_graph* g);
/* Which kernel qd_osd_batch_device launches for the graph, decided by the code
 * the launch itself uses; no HIP call, so host-only graphs (qd_graph_create_host)
 * answer too.  out[0] = RS and out[1] = W of osd_wave_kernel<RS, W> (RS = 0: the
 * workgroup kernel, W = its words per row), out[2] = the launch's dynamic LDS
 * bytes.  Returns 1, or 0 (out all zero) when no device kernel holds the graph. */
int qd_osd_kernel_info(const qd_graph* g, int32_t out[3]);
int qd_osd_batch_device(qd_graph* g, int32_t method, int32_t order, int64_t B, const uint8_t* syn, int32_t syn_flags,
                        const void* llr, int32_t llr_precision, const uint8_t* status, const uint8_t* base,
                        const uint8_t* readout, uint8_t* osd0_out, uint8_t* osdw_out, uint8_t* corr_out, uint8_t* fail,
                        void* stream);

/* Where the OSD stage keeps the augmented rows [H_sorted | s].  On chip
 * (registers or LDS) is the selection above.  In HBM, osd_hbm_kernel gives every
 * workgroup a slot of a scratch the graph handle owns: the rows (m x ceil((n +
 * 1) / 64) words), the sort keys and indices, and the solution; indices are
 * 32-bit, so circuit detector error models (648 x 25,684: 2 MiB of rows) and
 * deep spacetime graphs are decoded on the device.  Same spec and outputs,
 * bit-identical to qd_osd_batch.  The HBM kernel holds a graph while its LDS
 * part (m hit flags, four row buffers, 64 transformed columns) fits 160 KiB and
 * k <= 256 (-48 otherwise).
 *
 * The scratch is allocated at the first HBM launch and grown on demand: num_cus
 * x 8 slots by default (qd_osd_set_slots: any count; -47 for slots < 0 or >
 * 2^20), at most B, at most a quarter of the free device memory (-45 when that
 * does not hold one slot).  On an allocation failure the slot count is halved
 * down to one; only then the launch fails with -46.  Launches on one handle from
 * different streams are chained through an event of the handle; a regrow and
 * qd_graph_destroy wait for it.  Results never depend on the slot count. */
#define QD_OSD_ONCHIP 0 /* qd_osd_batch_device's selection, -85 beyond it */
#define QD_OSD_HBM 1    /* always the HBM kernel */
#define QD_OSD_AUTO 2   /* on chip where a kernel holds the graph, else HBM */
/* qd_osd_batch_device with a placement (-44 for any other value; -16 on a
 * host-only graph); qd_osd_batch_device is this call with QD_OSD_ONCHIP. */
int qd_osd_batch_device_placed(qd_graph* g, int32_t method, int32_t order, int64_t B, const uint8_t* syn,
                               int32_t syn_flags, const void* llr, int32_t llr_precision, const uint8_t* status,
                               const uint8_t* base, const uint8_t* readout, uint8_t* osd0_out, uint8_t* osdw_out,
                               uint8_t* corr_out, uint8_t* fail, void* stream, int32_t placement);
/* The kernel a placement launches; no HIP call, host-only graphs answer.  out[0] =
 * kind (0 register kernel, 1 workgroup kernel, 2 HBM kernel), out[1] = RS (0 unless
 * kind 0), out[2] = W, out[3] = dynamic LDS bytes (kinds 0, 1) or bytes per slot
 * (kind 2).  Returns 1, 0 (out all zero) when the placement has no kernel for the
 * graph, -44 for an unknown placement. */
int qd_osd_kernel_info_placed(const qd_graph* g, int32_t placement, int64_t out[4]);
/* Slots of the next HBM launches (0 = the default). */
int qd_osd_set_slots(qd_graph* g, int64_t slots);
/* out[0] = bytes per slot (0: the HBM kernel does not hold the graph), out[1] =
 * slots of the last HBM launch, out[2] = scratch bytes held. */
int qd_osd_hbm_info(const qd_graph* g, int64_t out[3]);

/* Relay-BP: a post-processor made of message passing alone, for the shots plain
 * BP leaves open on graphs without flip sets (circuit detector error models),
 * where OSD's elimination is the slow stage.  An ensemble of min-sum "legs"
 * with per-variable memory strengths gamma_j: each leg starts from the previous
 * leg's marginals, and the lowest-weight solution found is kept.  No reference
 * counterpart (the reference has no decoder of its own): the algorithm is
 * build-defined, fixed to the last rounding in DESIGN 3.6d, with
 * tests/relay_model.py as its model.  All arithmetic in T = float or double,
 * no contraction.
 *
 * qd_graph_set_relay: the stage's tables.  Leg 0 runs up to pre_iter iterations
 * with gamma_j = gamma0, leg r = 1 .. num_sets up to set_max_iter with row r - 1
 * of gammas [num_sets][n] (doubles, rounded once to T; NULL with num_sets = 0);
 * alpha is the fixed min-sum scaling factor, clip (2^64 by default in the Python
 * binding) the bound of marginals and messages, stop_nconv the number of
 * converged legs after which a shot stops.  Solution weights are llrint(prior
 * 2^16) of the f64 min-sum priors.  Works on host-only graphs; the tables are
 * rebuilt by every later qd_graph_set_priors.  Errors: -52 a parameter out of
 * range (alpha not finite or <= 0, clip not > 0 (+inf: no clamp), gamma0 or a
 * gamma not finite, pre_iter, set_max_iter, stop_nconv < 1, num_sets < 0, gammas
 * NULL with num_sets > 0; qd_relay_set_slots: slots outside 0 .. 2^20), -53 (num_sets + 1) n above 2^23 table entries, -5
 * priors never set, -51 priors holding a 0 or a 1.
 *
 * qd_relay_batch_device: B shots on device buffers, enqueued on `stream`.
 * Inputs as qd_decode_batch_device's byte rows (syn_flags: QD_SYN_ADD_BASE /
 * _READOUT; QD_INPUT_PACKED is refused).  Outputs (each nullable):
 *   x_out    uint8 [B][n]      the best solution, or the last hard decision
 *   corr_out uint8 [B][n_data] base ^ fold(x_out)
 *   llr_out  [B][n] float / double: the marginals after the last iteration run
 *   iters    int32 [B]         all iterations run
 *   legs     int32 [B]         legs run
 *   status   uint8 [B]         3 (QD_ST_BP_CONVERGED | QD_ST_SATISFIED) when a
 *                              solution was found, else 0
 *   fail     uint8 [B]         any(Lz (readout ^ corr_out)) (logicals + readout)
 * With only_failed != 0, status is read first: a shot whose QD_ST_BP_CONVERGED
 * bit is set is skipped and none of its outputs is touched.  placement: where a
 * workgroup keeps v2c, c2v and the marginals --
 *   QD_RELAY_LDS   dynamic LDS with the shot state (-56 above 160 KiB)
 *   QD_RELAY_HBM   a slot of a scratch the handle owns; bytes and bits stay in
 *                  LDS (-56 when that part alone exceeds 160 KiB)
 *   QD_RELAY_AUTO  LDS where it fits, else HBM
 * Both give the same bits.  The scratch follows the OSD scratch's policy: grown
 * on demand within a quarter of the free device memory (-59 when that holds no
 * slot), halved on a refusal down to one slot (-58).  Launches on one handle
 * from different streams are chained through an event.  Errors: -4 precision,
 * -8 B < 0, -55 placement, -57 inputs the stage does not take (packed rows,
 * unknown syn_flags, a failure check over more than 256 logicals), -54
 * qd_graph_set_relay not called, -5 / -51 priors, -7 no syndrome source, -56,
 * -16 host-only graph.  B = 0 returns 0 and writes nothing.
 * qd_relay_batch: the same on host buffers, synchronous.
 * qd_relay_set_slots: workgroups of later launches in both placements (0 = the
 * default: 2 per compute unit in HBM, what fits in LDS); a launch uses at most
 * B.  Results do not depend on it.
 * qd_relay_info: out[4] = kind (QD_RELAY_LDS or QD_RELAY_HBM) the placement
 * launches, its dynamic LDS bytes, bytes per slot (0 for LDS), workgroups of
 * the last launch.  No HIP call; host-only graphs answer.  -56 when the
 * placement has no kernel for the graph.
 * qd_relay_kernel_names: as qd_kernel_table_names for the relay kernels' own
 * table (which that list does not include). */
#define QD_RELAY_LDS 0
#define QD_RELAY_HBM 1
#define QD_RELAY_AUTO 2
typedef struct qd_relay_params {
    double gamma0;
    double alpha;
    double clip;
    int32_t pre_iter;
    int32_t num_sets;
    int32_t set_max_iter;
    int32_t stop_nconv;
} qd_relay_params;
int qd_graph_set_relay(qd_graph* g, const qd_relay_params* prm, const double* gammas);
int qd_relay_batch_device(qd_graph* g, int32_t precision, int64_t B, const uint8_t* syn, int32_t syn_flags,
                          const uint8_t* base, const uint8_t* readout, uint8_t* x_out, uint8_t* corr_out,
                          void* llr_out, int32_t* iters, int32_t* legs, uint8_t* status, uint8_t* fail,
                          int32_t only_failed, int32_t placement, void* stream);
int qd_relay_batch(qd_graph* g, int32_t precision, int64_t B, const uint8_t* syn, int32_t syn_flags,
                   const uint8_t* base, const uint8_t* readout, uint8_t* x_out, uint8_t* corr_out, void* llr_out,
                   int32_t* iters, int32_t* legs, uint8_t* status, uint8_t* fail, int32_t only_failed,
                   int32_t placement);
int qd_relay_set_slots(qd_graph* g, int64_t slots);
int qd_relay_info(const qd_graph* g, int32_t precision, int32_t placement, int64_t out[4]);
int64_t qd_relay_kernel_names(char* buf, int64_t cap);

/* Layered (check-serial) min-sum BP: the rows of H are processed in ascending
 * order and the posteriors are updated after each row, so information crosses
 * the graph within an iteration; on the graphs here it leaves fewer shots open
 * than the flooding schedule in about half the iterations.  The
 * kernel runs one wave per shot with its lanes along the row, the access
 * pattern wide rows (circuit detector error models) want.  Build-defined, fixed
 * to the last rounding in DESIGN 3.6f with tests/layered_model.py as its model:
 *   P_j = prior_j, R_e = 0; for t = 1 .. max_iter, for every row i in order,
 *   over its edges e = (i, j): q_e = P_j - R_e; m1 <= m2 the two smallest |q_e|;
 *   par = s_i ^ parity(q_e <= 0); y_e = min(|q_e| == m1 ? m2 a_t : m1 a_t, clip);
 *   R_e = par ^ (q_e <= 0) ? -y_e : y_e; P_j = clamp(q_e + R_e, -clip, clip);
 *   after the last row x_j = (P_j <= 0), and a shot with H x = s stops.
 * a_t = ms_scaling, or 1 - 2^-t when ms_scaling = 0.  All arithmetic in T =
 * float or double, no contraction.  The graph's min-sum priors are used.
 *
 * qd_layered_batch_device: B shots on device buffers, enqueued on `stream`.
 * Inputs as qd_decode_batch_device's byte rows (syn_flags: QD_SYN_ADD_BASE /
 * _READOUT).  Outputs (each nullable), with the meaning they have after
 * qd_decode_batch_device, so the OSD and relay stages follow unchanged:
 *   x_out    uint8 [B][n]      the hard decision after the last iteration run
 *   corr_out uint8 [B][n_data] base ^ fold(x_out)
 *   llr_out  [B][n] float / double: P as it stands
 *   iters    int32 [B]         iterations run
 *   status   uint8 [B]         3 (QD_ST_BP_CONVERGED | QD_ST_SATISFIED) when
 *                              H x = s, else 0
 *   fail     uint8 [B]         any(Lz (readout ^ corr_out)) (logicals + readout)
 * placement: where a workgroup keeps P[n] and R[E] --
 *   QD_LAYERED_LDS   dynamic LDS (-111 above 160 KiB)
 *   QD_LAYERED_HBM   a slot of a scratch the handle owns, (E + n) sizeof(T)
 *                    rounded to 256 B; the syndrome and the hard decision stay
 *                    in LDS (-111 when they alone exceed 160 KiB)
 *   QD_LAYERED_AUTO  LDS while eight workgroups fit a compute unit's 160 KiB,
 *                    else HBM
 * Both give the same bits.  The scratch follows the relay scratch's policy:
 * grown on demand within a quarter of the free device memory (-113 when that
 * holds no slot), halved on a refusal down to one slot (-112).  Launches on one
 * handle from different streams are chained through an event.  Errors, in this
 * order: -1 null handle, -4 precision, -8 B < 0, -68 placement, -49 a parameter
 * out of range (null, max_iter < 1, ms_scaling not finite or < 0, clip not
 * finite or <= 0; qd_layered_set_slots: slots outside 0 .. 2^20), -69 inputs
 * the kernel does not take (QD_INPUT_PACKED, unknown syn_flags, a failure check
 * over more than 256 logicals), -5 priors never set, -51 priors holding a 0 or
 * a 1, -7 no syndrome source, -111, -16 host-only graph.  B = 0 returns 0 and
 * writes nothing.
 * qd_layered_batch: the same on host buffers, synchronous.
 * qd_layered_set_slots: workgroups of later launches in both placements (0 =
 * the default: 16 per compute unit in LDS or what its LDS holds, 8 in HBM); a
 * launch uses at most B.
 * Results do not depend on it.
 * qd_layered_info: out[4] = kind (QD_LAYERED_LDS or QD_LAYERED_HBM) the
 * placement launches, its dynamic LDS bytes, bytes per slot (0 for LDS),
 * workgroups of the last launch.  No HIP call; host-only graphs answer.
 * qd_layered_kernel_names: as qd_kernel_table_names for the layered kernels'
 * own table (which that list does not include). */
#define QD_LAYERED_LDS 0
#define QD_LAYERED_HBM 1
#define QD_LAYERED_AUTO 2
typedef struct qd_layered_params {
    int32_t max_iter;
    double ms_scaling;
    double clip;
} qd_layered_params;
int qd_layered_batch_device(qd_graph* g, const qd_layered_params* prm, int32_t precision, int64_t B,
                            const uint8_t* syn, int32_t syn_flags, const uint8_t* base, const uint8_t* readout,
                            uint8_t* x_out, uint8_t* corr_out, void* llr_out, int32_t* iters, uint8_t* status,
                            uint8_t* fail, int32_t placement, void* stream);
int qd_layered_batch(qd_graph* g, const qd_layered_params* prm, int32_t precision, int64_t B, const uint8_t* syn,
                     int32_t syn_flags, const uint8_t* base, const uint8_t* readout, uint8_t* x_out,
                     uint8_t* corr_out, void* llr_out, int32_t* iters, uint8_t* status, uint8_t* fail,
                     int32_t placement);
int qd_layered_set_slots(qd_graph* g, int64_t slots);
int qd_layered_info(const qd_graph* g, int32_t precision, int32_t placement, int64_t out[4]);
int64_t qd_layered_kernel_names(char* buf, int64_t cap);

/* ---- sliding-window decoding: the step between two windows ----------------
 * (csrc/qdec_window.hip; no reference counterpart: the reference
 * left it as a stub, spacetime_code.py:95-96).  A layered graph is decoded
 * window by window; a qd_window is one boundary: what the window's committed
 * columns do to the rows of the full syndrome that later windows read (the
 * carry table), what they add to an accumulator (the fold of a spacetime code,
 * the observables of a detector error model), and which rows of the full
 * syndrome the next window takes.
 *
 * Tables (copied): carry row i is global row carry_rows[i] (strictly ascending,
 * inside [0, m_total)) and reads the window-local columns carry_cols[
 * carry_ptr[i] .. carry_ptr[i + 1]); accumulator row i reads acc_cols[
 * acc_ptr[i] .. acc_ptr[i + 1]).  A column that is not committed is simply not
 * listed.  Refusals, before anything is copied or enqueued: -26 a null handle,
 * output or array, a negative size, n_w < 1 or above 2^19; -25 row0 + m_next >
 * m_total (or either negative); -24 a pointer array that does not start at 0 or
 * decreases; -22 carry rows unsorted, repeated or out of range; -23 a column
 * outside [0, n_w); -15 device ordinal.  qd_window_create_host validates the
 * same way and makes no HIP call (its handle refuses to run, -16).
 *
 * qd_window_advance_device, per shot b (all buffers uint8, one byte per bit;
 * bit 0 of an x byte counts), enqueued on `stream`:
 *   syn_full[b][carry_rows[i]] ^= xor_{c in carry row i} x[b][c]
 *   acc_out[b][i]              ^= xor_{c in acc row i} x[b][c]      (acc_out may be NULL)
 *   syn_next[b][i]              = syn_full[b][row0 + i], after the carry (syn_next may be NULL)
 * x = NULL: no carry and no accumulate, only the copy (it stages the first
 * window).  syn_full [B][m_total] is updated in place -- a column that spans
 * more layers than a window commits carries into windows after the next one --
 * and no other byte of it is written.  -28 B < 0 or a NULL syn_full that would
 * be read.  B = 0 returns 0 and writes nothing.
 * qd_window_set_blocks: workgroups of later launches (0 = the default, 8 per
 * compute unit; a launch uses at most B; -29 outside 0 .. 2^20).  Results do
 * not depend on it. */
typedef struct qd_window qd_window;
int qd_window_create(int32_t device, int32_t n_w, int32_t m_total, int32_t n_carry, const int32_t* carry_rows,
                     const int32_t* carry_ptr, const int32_t* carry_cols, int32_t k_acc, const int32_t* acc_ptr,
                     const int32_t* acc_cols, int32_t row0, int32_t m_next, qd_window** out);
int qd_window_create_host(int32_t n_w, int32_t m_total, int32_t n_carry, const int32_t* carry_rows,
                          const int32_t* carry_ptr, const int32_t* carry_cols, int32_t k_acc, const int32_t* acc_ptr,
                          const int32_t* acc_cols, int32_t row0, int32_t m_next, qd_window** out);
int qd_window_advance_device(qd_window* w, int64_t B, const uint8_t* x, uint8_t* syn_full, uint8_t* acc_out,
                             uint8_t* syn_next, void* stream);
int qd_window_set_blocks(qd_window* w, int64_t blocks);
int qd_window_destroy(qd_window* w);

/* Kernel timing for measurement: with capacity > 0, the next `capacity` decode
 * calls record HIP events on their launch stream immediately before the BP kernel,
 * after it and after the SSF kernel.  qd_graph_read_timing returns the per-call
 * BP and SSF kernel durations (ms) and resets the ring.  No reference
 * counterpart (the reference only reports whole-sweep walltime,
 * misc/p_sweep.py:26-33). */
int qd_graph_set_timing(qd_graph* g, int32_t capacity);

/* Route the SSF kernel of later qd_decode_batch_device calls (wave-kernel graphs)
 * to `ssf_stream` (hipStream_t; NULL = the decode's own stream, the default):
 * it runs behind an event recorded after the BP kernel on the decode stream.
 * Outputs the SSF stage writes (status, ssf_steps, fail, x/corr of BP-failed
 * shots) are complete when `ssf_stream` has passed that point; the caller
 * synchronises with it.  Split decodes alternate between two SSF queues (and
 * their control words), so a decode waits for the SSF kernel of the decode two
 * back on this handle, not the previous one: the handle's next triage and BP
 * run while this SSF kernel is still on `ssf_stream`.  Replaces nothing in the
 * reference (its decode is one synchronous call per shot). */
int qd_graph_set_ssf_stream(qd_graph* g, void* ssf_stream);

/* Occupancy of the wave BP kernels (one wave per shot, persistent grid) in waves
 * per CU: 0 = the default (f64: 8, measured fastest for a lone decode; f32: the
 * hardware maximum), N > 0 = N, bounded by what the kernel's LDS and registers
 * allow and rounded down to a multiple of 4 (equal waves per SIMD).  For
 * several decodes running concurrently on different streams: the bench's
 * 9-stream sweep measured 82-83 M shots/s at 12 f64 waves per CU against 80 M
 * at 8, while a lone f64 decode at 12 is slower (p = 0.1: 9.3 vs 7.1 ms per 2^18
 * shots).  A request above 8 f64 waves per CU launches the kernel's build for
 * 3 waves per SIMD (the f64 LEAN kernel otherwise needs 172 VGPRs, which fit
 * only 2).  Results are identical at every setting.  No reference counterpart. */
int qd_graph_set_wave_occupancy(qd_graph* g, int32_t waves_per_cu);
int qd_graph_read_timing(qd_graph* g, float* bp_ms, float* ssf_ms, int32_t max_calls, int32_t* n_calls);
/* The same ring split finer: per recorded call the BP stage's pre-pass (the
 * lean launches' shot triage; 0 when none ran), the BP kernel alone, the SSF
 * kernel (ms), and `listed` = the number of shots the triage left to the BP
 * kernel (-1 when the call did not run the two-pass path).  Resets the ring
 * like qd_graph_read_timing.  Any output may be NULL.  No reference
 * counterpart. */
int qd_graph_read_timing_detail(qd_graph* g, float* pre_ms, float* bp_ms, float* ssf_ms, int64_t* listed,
                                int32_t max_calls, int32_t* n_calls);

/* Names of the BP and SSF kernels the last decode call on `g` launched, and of
 * the pass run before the BP kernel inside the BP timing (the lean launches'
 * shot triage), as rocprofv3 spells them (template arguments included; "" when
 * a stage did not run or has no recorded name), NUL-terminated and truncated to
 * the buffer lengths.  Lets a measurement match a rocprof / PMC entry to the
 * exact instantiation it timed.  No reference counterpart. */
int qd_graph_last_kernels(qd_graph* g, char* bp, int32_t bp_len, char* ssf, int32_t ssf_len, char* pre,
                          int32_t pre_len);

/* Kernel choices of one handle, for A/B measurements and for tests that keep
 * every kernel path covered.  Results are identical under every setting (each
 * path is parity-tested against the oracle).  Returns -2 for an unknown option
 * or an out-of-range value.  No reference counterpart: ldpc has one decoder
 * implementation.
 *   QD_OPT_COMPACT       1 (default): lean min-sum decodes on wave graphs run the
 *                        shot triage + compact-list kernel; 0: the one-pass kernel.
 *   QD_OPT_TRIAGE_IT1    1 (default): the triage runs min-sum iteration 1
 *                        bit-sliced (default alpha schedule, positive priors); 0: off.
 *   QD_OPT_SSF           SSF kernels: QD_SSF_AUTO (default: the table-driven
 *                        wave kernel, or table scoring in the workgroup kernel,
 *                        when the graph's tables qualify, else the scanning
 *                        kernels), QD_SSF_SCAN (scanning kernel / subset search,
 *                        incremental local syndromes), QD_SSF_SCAN_GATHER (scanning
 *                        kernel, local syndromes re-gathered every step),
 *                        QD_SSF_SCAN_NOSPLIT (scanning, one lane per generator).
 *   QD_OPT_LDS_KERNEL    -1 (default) automatic, 0 never, 1 forced: the
 *                        LDS-resident min-sum workgroup kernels (f32: every
 *                        message in LDS; f64: v2c in registers, check states
 *                        by LDS atomics).
 *   QD_OPT_GROUP_KERNEL  -1 (default) automatic, 0 never, 1 forced: the slot-group
 *                        HBM-streaming kernel.
 *   QD_OPT_SSF_INC       1 (default): incremental workgroup SSF; 0: re-scanning.
 *   QD_OPT_BLOCK_WG      0 (default) automatic, N > 0: workgroups per CU of the
 *                        HBM-slice workgroup BP kernel.
 *   QD_OPT_GROUP_MB      0 (default): a quarter of the free HBM, N > 0: N MiB for
 *                        the slot-group kernel's message scratch.
 *   QD_OPT_SSF_FUSE      0 (default): BP-failed shots of two-pass min-sum decodes
 *                        are queued for ssf_lut_kernel; 1: the compact BP kernel
 *                        runs the same table-driven SSF itself right after a
 *                        shot's BP fails (no queue, no second launch; its tables
 *                        come through the caches, not LDS: measured slower). */
#define QD_OPT_COMPACT 1
#define QD_OPT_TRIAGE_IT1 2
#define QD_OPT_SSF 3
#define QD_OPT_LDS_KERNEL 4
#define QD_OPT_GROUP_KERNEL 5
#define QD_OPT_SSF_INC 6
#define QD_OPT_BLOCK_WG 7
#define QD_OPT_GROUP_MB 8
#define QD_OPT_SSF_FUSE 9
#define QD_SSF_AUTO 0
#define QD_SSF_SCAN 1
#define QD_SSF_SCAN_GATHER 2
#define QD_SSF_SCAN_NOSPLIT 3
int qd_graph_set_option(qd_graph* g, int32_t option, int32_t value);
int qd_graph_get_option(const qd_graph* g, int32_t option, int32_t* value);

/* Which table-driven SSF the handle's graph qualifies for: 1 when the wave
 * kernel's tables were built (ssf_lut_kernel: QD_SSF_AUTO then runs it), 2 when
 * only the score tables were (graphs beyond the wave shapes: the workgroup SSF
 * kernel scores generators by table lookup), 0 otherwise.  *lut_bytes
 * (nullable) = bytes of the score tables.  No reference counterpart. */
int qd_graph_ssf_tables(const qd_graph* g, int32_t* has_lut, int64_t* lut_bytes);
/* Copies of the table-driven SSF kernel's tables, for host-only graphs
 * (qd_graph_create_host; tests emulate the kernel's steps on them): lut
 * [lut_bytes / 4], off [g_pad], lcw [4][g_pad], tog [m_pad + 1][64] (u32 each; the
 * layouts of DevGraph::s_lut / s_off / s_lcw / s_tog in qdec_internal.h);
 * *g_pad and *m_pad receive the strides.  Any output may be NULL. */
/* Host-side layout of the handle's queue scratch for a batch of B shots (the
 * workspace attach_queue allocates; tests check its alignment and capacities
 * on host-only graphs): out[8] = total bytes, offsets of the shot-index array,
 * the hard-decision / packed-entry region, the residual region, the compact
 * lists' 2 x 64 segment counters (light, then heavy) and their entries, the
 * entries per segment, the
 * bytes per entry.  No reference counterpart. */
int qd_graph_queue_layout(const qd_graph* g, int64_t B, int64_t* out);

/* The launch plan of a decode of B shots with these parameters (diagnostic; also
 * on host-only graphs): which kernels the call would run and which library
 * buffers it would attach, decided by the same function the decode entry points
 * use (plan_decode, qdec_internal.h).  `present`: the QD_PLAN_* bit of every
 * optional buffer the call would pass, plus QD_PLAN_ROWS_ALIGNED when syn and
 * readout meet the triage's alignment (16 B for byte rows, 8 B for packed
 * rows; a packed decode refuses anything less).  out[8] = BP path (QD_BP_*),
 * SSF / finalize path (QD_FIN_*), two_pass, expand_packed (packed inputs go
 * through the byte expansion), fuse (0 / 1 / 2), q_rpar, placement of the
 * workgroup kernel's state (3: messages and shot state in LDS, 2: messages in
 * HBM, 0: both in HBM), buffers (bit 0 SSF queue, 1 compact lists, 2 unpack
 * buffer, 3 HBM scratch).  No reference counterpart. */
#define QD_PLAN_SYN 1u
#define QD_PLAN_BASE 2u
#define QD_PLAN_READOUT 4u
#define QD_PLAN_X 8u
#define QD_PLAN_CORR 16u
#define QD_PLAN_LLR 32u
#define QD_PLAN_FAIL 64u
#define QD_PLAN_ROWS_ALIGNED 128u
#define QD_BP_WAVE 0      /* bp_wave_kernel (product-sum on a wave graph) */
#define QD_BP_MS_WAVE 1   /* bp_ms_wave_kernel */
#define QD_BP_TWO_PASS 2  /* ms_triage_kernel + bp_ms_cmp_kernel */
#define QD_BP_GROUP 3     /* bp_group_kernel */
#define QD_BP_LDS 4       /* bp_ms_lds_kernel (f32) / bp_ms_lds64_kernel (f64) */
#define QD_BP_BLOCK 5     /* bp_block_kernel */
#define QD_FIN_NONE 0
#define QD_FIN_FUSED 1          /* inside bp_ms_cmp_kernel */
#define QD_FIN_LUT 2            /* ssf_lut_kernel */
#define QD_FIN_SCAN 3           /* ssf_wave_kernel */
#define QD_FIN_SCAN_GATHER 4
#define QD_FIN_SCAN_NOSPLIT 5
#define QD_FIN_INC_BLOCK 6      /* ssf_inc_block_kernel */
#define QD_FIN_BLOCK_LDS 7      /* ssf_block_kernel, shot state in LDS */
#define QD_FIN_BLOCK_HBM 8      /* ssf_block_kernel, shot state in HBM */
int qd_graph_plan(const qd_graph* g, const qd_params* p, int64_t B, uint32_t present, int32_t* out);
/* The instantiations that plan holds, by name: the three strings
 * qd_graph_last_kernels returns after the same decode (the plan picks every
 * stage's entry of the kernel tables, the launchers record what they enqueue
 * from it), also on host-only graphs.  A decode whose instantiation the library
 * does not build fails here and in qd_graph_plan with -17.  No reference
 * counterpart. */
int qd_graph_plan_names(const qd_graph* g, const qd_params* p, int64_t B, uint32_t present, char* bp,
                        int32_t bp_len, char* ssf, int32_t ssf_len, char* pre, int32_t pre_len);
/* The same plan's entries whether or not qd_graph_last_kernels records them:
 * as qd_graph_plan_names, except that a stage whose entry is not reported after
 * a launch (bp_block_kernel, the workgroup SSF kernels) is written under the name
 * qd_kernel_table_names lists it by ("" only for a stage without an entry).  No
 * HIP call; also on host-only graphs.  No reference counterpart. */
int qd_graph_plan_entries(const qd_graph* g, const qd_params* p, int64_t B, uint32_t present, char* bp,
                          int32_t bp_len, char* ssf, int32_t ssf_len, char* pre, int32_t pre_len);
/* Every instantiation the library builds for the decode kernel families: the
 * names of all entries of the kernel tables the plan picks from (wave graphs
 * first, then workgroup graphs; table order), each followed by '\n', spelled as
 * qd_graph_plan_names spells them; the workgroup SSF kernels, which the plan
 * reports as "", are listed under their own names.  Returns the length of the
 * list; copies it into buf (NUL-terminated, cut to cap) when buf is given.  No
 * HIP call.  For tests that keep a ledger of which instantiations they launch.
 * No reference counterpart. */
int64_t qd_kernel_table_names(char* buf, int64_t cap);

/* Copies of the triage's iteration-1 tables (host-only graphs): lut[n_pad]
 * (bit b = column j's hard decision after min-sum iteration 1 under syndrome
 * pattern b of its checks, in the kernels' precision and summation order) and
 * vchk[n_pad] (the checks of column j's edges, 4 x u16, pad = m).  Fails when
 * the precision has no tables (a prior <= 0).  No reference counterpart. */
int qd_graph_it1_tables_copy(const qd_graph* g, int32_t precision, uint16_t* lut, uint64_t* vchk, int32_t* n_pad);
/* Host-only graphs: the first check state of the compact min-sum kernel,
 * state[m_pad][2] of the precision's float type: the (m1, m2) pair check lane i
 * writes in the first check pass (rows holding the priors, syndrome bit 0: the
 * two smallest |prior| of the row, 1e308 / 1e30f where it has fewer, both
 * negated on odd parity; f64 uses the sign-bit rule for rows holding a zero),
 * and sslot[m_pad], the state slot of check lane i.  Either may be NULL.  -39
 * when the graph has no wave shape or no BP priors.  No reference counterpart. */
int qd_graph_ms_state0_copy(const qd_graph* g, int32_t precision, void* state, uint16_t* sslot, int32_t* m_pad);
/* Host-only graphs: the f64 LDS-resident kernel's check-state slots (m64_layout):
 * etab uint16 [4][n] (slot of edge k of column j, 0xffff pad), check_of_slot
 * uint16 [m].  -38 when the graph has none.  For tests. */
int qd_graph_lds64_slots_copy(const qd_graph* g, uint16_t* etab, uint16_t* check_of_slot);

int qd_graph_ssf_tables_copy(const qd_graph* g, uint32_t* lut, uint32_t* off, uint32_t* lcw, uint32_t* tog,
                             int32_t* g_pad, int32_t* m_pad);

/* Hypergraph-product kernel (qdec_hgp.cpp, qdec_hgp_kernel.hip).  When H =
 * [I_a0 (x) B | A (x) I_b0] (the Z checks of hgp.py homological_product, e.g.
 * biregular_hgp, reference python/qldpc/hypergraph_product_code.py:7-35), the
 * library generates an f64 min-sum BP kernel with B's and A's Tanner graphs as
 * compile-time tables and compiles it with hipRTC.  qd_graph_hgp_info: 1 and
 * out8 = {a0, a1, b0, b1, shot slots per workgroup, left waves, right waves,
 * workgroups per CU (0 before the first decode)} for such a graph, 0 otherwise.
 * qd_graph_hgp_source: the generated source (its length; copied into buf).
 * qd_graph_hgp_compile: compile only (no device needed).  No reference
 * counterpart (the reference decodes with ldpc's generic BpDecoder). */
int qd_graph_hgp_info(qd_graph* g, int32_t* out8);
/* Re-plan with `slots` shot slots per workgroup (0: the library's choice);
 * -95 when no workgroup shape holds `slots` (the previous plan stays). */
int qd_graph_hgp_set_slots(qd_graph* g, int32_t slots);
int64_t qd_graph_hgp_source(qd_graph* g, char* buf, int64_t cap);
int qd_graph_hgp_compile(qd_graph* g);
/* (Development builds with -DQDEC_DEV_HOOKS also export
 * qd_graph_hgp_replace_source(g, src), which recompiles an edited kernel
 * source; the product library does not.) */
/* BP only (f64 min-sum, ldpc v1 semantics as qd_decode_batch_device with
 * method QD_MIN_SUM, precision QD_F64, no SSF): device buffers syn [B][m],
 * x_out [B][n] (or null), iters [B], status [B] (bit 0: converged). */
int qd_graph_hgp_decode_bp(qd_graph* g, int64_t B, const uint8_t* syn, uint8_t* x_out, int32_t* iters,
                           uint8_t* status, int32_t max_iter, double ms_scaling, void* stream);

/* Device-side sum of a uint8 flag array (failure / status counts) into *out
 * (device int64, accumulated: caller zeroes it).  `mask` selects bits. */
int qd_count_flags_device(const uint8_t* flags, int64_t B, uint8_t mask, int64_t* out, void* stream);

/* GF(2) elimination on bit-packed rows (uint64 words, bit j at word j/64), host
 * cores.  Offline code-construction support for the logical operators the fused
 * failure check consumes; replaces galois row_reduce / null_space /
 * column_space in the reference's get_logicals
 * (python/qldpc/homological_product_code.py:6-60).
 * qd_gf2_rref: in-place reduced row echelon form over columns [0, ncols); the
 * first `rank` rows are the pivot rows, pivots[r] = their pivot columns
 * (nullable).  Returns rank, or < 0 on bad arguments.
 * qd_gf2_extend_basis: reduce each candidate row against an echelon basis (row b
 * has its lowest set bit at basis_lead[b]) plus the candidates accepted so far;
 * accepted[c] = 1 for candidates outside that span (at most max_accept when >= 0).
 * Returns the number accepted (homological_product_code.py:15-21). */
int64_t qd_gf2_rref(uint64_t* rows, int64_t nrows, int64_t words, int64_t ncols, int64_t* pivots, int32_t nthreads);
int64_t qd_gf2_extend_basis(const uint64_t* basis, int64_t nbasis, const int64_t* basis_lead, const uint64_t* cand,
                            int64_t ncand, int64_t words, int64_t ncols, uint8_t* accepted, int64_t max_accept);

#ifdef __cplusplus
}
#endif
#endif
