/*
 * commpy_amd.h -- C-ABI of libcommpy_amd.so, the MI355X (gfx950) decoding engine.
 *
 * The reference (veeresht/CommPy 0.8.0, pure Python) has no FFI/plugin layer: its boundary for the
 * hot path is the set of Python callables exported by commpy/channelcoding/__init__.py:65-71 and
 * commpy/modulation.py:35-36.  Each entry point below replaces the BODY of one of those callables;
 * the Python mirror in commpy_amd/ keeps the reference signatures and reaches these symbols with
 * ctypes (see INTEGRATION.md for the stub a CommPy maintainer would add).
 *
 * Conventions
 *   - extern "C", plain pointers and sizes, no C++/torch types.
 *   - every function returns 0 on success, <0 on error (CPX_E*); cpx_last_error() gives a
 *     thread-local message.  The Python layer maps errors to the reference's exception types.
 *   - "host" entry points take caller-owned host buffers (C-contiguous NumPy memory), copy
 *     H2D/D2H themselves on the library's stream and return after completion.
 *   - "_dev" entry points take DEVICE pointers and a hipStream_t (as void*; NULL = the library's
 *     own stream), enqueue the kernels and return immediately (asynchronous); used by bench.py and
 *     the multi-GPU path where inputs are already resident in HBM.
 *   - handles (cpx_trellis/cpx_ldpc/cpx_modem) own small device-side tables; they belong to the
 *     device that was current at creation and are freed by the matching *_destroy.
 *   - no CPU fallback exists: without a usable HIP device every compute entry point fails.
 */
#ifndef COMMPY_AMD_H
#define COMMPY_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* the library is built with -fvisibility=hidden: what this header declares is ALL it exports */
#pragma GCC visibility push(default)

#define CPX_OK 0
#define CPX_EINVAL (-1)   /* bad argument (Python: ValueError) */
#define CPX_EHIP (-2)     /* HIP runtime error (Python: RuntimeError) */
#define CPX_ENOMEM (-3)   /* allocation failure */
#define CPX_ENODEV (-4)   /* no usable gfx950 device */
#define CPX_ELIMIT (-5)   /* argument exceeds a documented engine limit */

typedef struct cpx_trellis cpx_trellis;
typedef struct cpx_ldpc cpx_ldpc;
typedef struct cpx_modem cpx_modem;

/* ---- runtime ---------------------------------------------------------------------------------*/
const char *cpx_last_error(void);
int cpx_version(void);
/* "full:<sha16>;viterbi:<sha16>" -- digests of the sources this library was compiled from (commpy_amd/build.py).  Measurement
 * files (profiles/...pmc.json) carry the id of the library that produced them; bench.py only quotes their counters when the
 * "viterbi" part equals the loaded library's. */
const char *cpx_build_id(void);
int cpx_device_count(int *n);
int cpx_set_device(int device);
int cpx_get_device(int *device);
/* Name of the (dominant) kernel the last decoder call of the calling thread launched, e.g.
 * "viterbi_cw_fused_kernel<6,0155,0117,soft,28>": benchmarks and tests report what really ran.  Decoders with a "detect and redo"
 * path append "; redo: n of N ..." -- n is written by the redo kernel itself, so that suffix is only valid once the issuing stream
 * has been synchronised (the host-buffer entry points return synchronised; after a *_dev call, cpx_stream_sync first). */
int cpx_last_kernel(char *name, int cap);
/* Precision mode of the process ("fp64-parity default vs fp32-fast"), initial value from the environment variable
 * CPX_PRECISION.  "fp64-parity" (default): every kernel computes in float64 in the reference's operation order -- the mode all
 * parity claims are made in.  "fp32-fast": kernels that have a float32 variant use it -- the fused codeword-per-lane Viterbi
 * kernel (float32 path metrics, correlation branch metric; measured mismatch rate in DESIGN.md 4.1) and the LDS-resident LDPC
 * kernels (float32 messages, hardware exp2 / log2 / reciprocal for sum-product; same decoded words and frame error rate on the
 * measured workloads) and soft demodulation (float32 log-sum-exp, |dLLR| <= 3.4e-5 + 35 * 2^-24 * max_a |y - c_a|^2 /
 * noise_var at every finite input -- within 2e-5 + 4e-6 |LLR| for samples a few noise standard deviations from a constellation
 * point, NOT far from the constellation --, finite where the reference's sums underflow) -- NOT bit-exact and NOT
 * under the 1e-5 LLR criterion; every other kernel is unaffected.  Viterbi and min-sum are exact against a float32 model of the same
 * operations, sum-product and the demodulator within bounds (tests/fp32_model.py).
 * cpx_last_kernel shows "f32" in the name when a variant ran. */
int cpx_set_precision(const char *mode);
int cpx_get_precision(void);   /* 0 fp64-parity, 1 fp32-fast */
int cpx_device_info(char *name, int name_cap, int *compute_units, int64_t *hbm_bytes);
int cpx_malloc(void **dptr, size_t bytes);
int cpx_free(void *dptr);
/* cpx_memset / cpx_memcpy_h2d / cpx_memcpy_d2h are synchronous AND ordered with the library stream: they run after every `_dev`
 * call that was given stream = NULL has finished (work on a caller's own stream needs cpx_stream_sync first). */
int cpx_memset(void *dptr, int value, size_t bytes);
int cpx_memcpy_h2d(void *dst, const void *src, size_t bytes);
int cpx_memcpy_d2h(void *dst, const void *src, size_t bytes);
int cpx_memcpy_h2d_async(void *dst, const void *src, size_t bytes, void *stream);
int cpx_memcpy_d2h_async(void *dst, const void *src, size_t bytes, void *stream);
int cpx_memcpy_d2d_async(void *dst, const void *src, size_t bytes, void *stream);
int cpx_stream_create(void **stream);       /* a non-blocking hipStream_t on the current device */
int cpx_stream_destroy(void *stream);
int cpx_stream_sync(void *stream);          /* NULL = the library's stream */
int cpx_release_workspace(void);            /* free the per-stream scratch arenas the decoders keep between calls */
void *cpx_default_stream(void);             /* the library's own hipStream_t */
/* HIP-event timer on a stream (bench.py times the kernels on the stream they are launched on) */
int cpx_timer_create(void **timer);
int cpx_timer_start(void *timer, void *stream);
int cpx_timer_stop(void *timer, void *stream);
int cpx_timer_elapsed_ms(void *timer, float *ms);   /* synchronises on the stop event */
int cpx_timer_destroy(void *timer);
/* Shader-clock probe (round 5; measurement support, no reference counterpart): cpx_sclk_probe_start launches one mostly sleeping
 * wavefront on a stream of its own for `spin_ms` milliseconds of the constant-rate device clock; cpx_sclk_probe_read waits for it
 * and returns the average shader clock (MHz) over the interval it really covered (`interval_ms`) -- the clock the kernels on the
 * OTHER streams ran at meanwhile -- and frees the probe.  bench.py records it next to its per-launch times.  Every outstanding
 * probe owns one of 16 result slots of its device (a 17th start: CPX_ELIMIT); cpx_sclk_probe_destroy gives back a probe that is never
 * read (it waits for the probe's wavefront first). */
int cpx_sclk_probe_start(void **probe, double spin_ms);
int cpx_sclk_probe_read(void *probe, double *sclk_mhz, double *interval_ms);
int cpx_sclk_probe_destroy(void *probe);

/* ---- convolutional codes: Viterbi ---------------------------------------------------------------
 * cpx_trellis_create: device copy of the code description built by the host Trellis class.
 *   Replaces nothing by itself; it carries Trellis.next_state_table / output_table
 *   (reference commpy/channelcoding/convcode.py:117-255) to the device.  Tables are [S][I]
 *   row-major int32.  Predecessor lists are derived in np.where order (convcode.py:561-572), which
 *   defines the ACS tie-break.  Limits: S = 2^m <= 65536, I = 2^k <= 256, n <= 16; every state needs exactly I incoming branches
 *   (the reference indexes pmetrics[number_inputs], convcode.py:604-629).  The specialised kernels serve S <= 128, k <= 2, n <= 6;
 *   the general kernels (viterbi_generic.hip, bcjr_exact.hip) the rest.
 */
int cpx_trellis_create(int k, int n, int n_states, int n_inputs, const int32_t *next_state_table,
                       const int32_t *output_table, cpx_trellis **out);
int cpx_trellis_destroy(cpx_trellis *t);

/* decoding_type */
#define CPX_VIT_HARD 0
#define CPX_VIT_SOFT 1
#define CPX_VIT_UNQUANTIZED 2

/* cpx_viterbi_decode_batch replaces the body of
 *   viterbi_decode(coded_bits, trellis, tb_depth, decoding_type)   convcode.py:661-749
 * (with _acs_traceback :590-657, _compute_branch_metrics :575-587) for B independent codewords.
 *   coded      [B][len] float64 (hard: 0/1 values; soft: LLR log P1/P0, clipped to +-500 inside;
 *              unquantized: real symbols)
 *   L          number of decoded bits per codeword = int(len*k/n)  (convcode.py:698)
 *   n_steps    trellis steps actually run = int((L+total_memory)/k) - 1  (convcode.py:721)
 *   tb_depth   traceback depth (>= 2), the caller resolves the default min(5*m, L)
 *   bits       [B][L] uint8 decoded bits, tail included (convcode.py:749)
 * Decision rule: the bit(s) of step s come from the survivor of the
 * first-minimum state at step min(s+tb_depth-2, n_steps), ties -> lowest index.
 * Kernel selection is internal and does not change a single output bit: batches of >= 0.45 * (SIMDs of the device) * 64
 * codewords of a rate-1/2 shift-register code of 4 .. 64 states run one codeword per lane (csrc/viterbi_cw.hip): a single fused
 * kernel with the generators compiled in -- K = 7 (133,171), (171,133) in both polynomial formats and Wifi80211's (5,43) for
 * tb_depth <= 48; K = 3 (5,7) and K = 5 (23,35) at their default depth -- or, for any other pair whose generators both tap the
 * input and the oldest register bit, with a run-time code table (default depth 5 * memory); an add-compare-select + a traceback kernel with a 9 B per codeword-step device workspace beyond that;
 * every other trellis of up to 128 states, k <= 2, n <= 6 runs one trellis state per lane (csrc/viterbi.hip); the rest of the
 * reference's argument domain (up to 65536 states, k <= 8, n <= 16, any traceback depth) one workgroup per codeword
 * (csrc/viterbi_generic.hip: slow, complete).  A NaN among 'soft' inputs is handled as the reference
 * handles it (convcode.py:719 lets it through the clip): flagged codewords are decoded again by a NaN-exact instantiation.
 * cpx_viterbi_set_path (or the environment variable CPX_VITERBI_PATH = wave | cw | cw! | cw2 | cw2! | general at load time)
 * overrides the choice (tests, benchmarks); cpx_last_kernel reports which kernel ran.
 */
int cpx_viterbi_decode_batch(const cpx_trellis *t, const double *coded, int64_t B, int64_t len,
                             int64_t L, int64_t n_steps, int tb_depth, int decoding_type, uint8_t *bits);
int cpx_viterbi_decode_batch_dev(const cpx_trellis *t, const double *d_coded, int64_t B, int64_t len,
                                 int64_t L, int64_t n_steps, int tb_depth, int decoding_type,
                                 uint8_t *d_bits, void *stream);
/* Kernel-path override for tests and benchmarks (initial value: environment variable CPX_VITERBI_PATH):
 * NULL / "" / "auto" = automatic, "wave", "cw", "cw!", "cw2", "cw2!" as described above, "general" = the general kernel. */
int cpx_viterbi_set_path(const char *mode);
/* Per-pair code objects for the codeword-per-lane kernels (round 6).  A rate-1/2 code of full constraint length that is not one of
 * the built-in generator pairs runs the TABLE-DRIVEN fused kernel (branch metric selected by VGPR index mode: 1.78 ms on the config-2
 * geometry where a built-in pair takes 1.55).  The same source file compiled with the pair as template arguments
 *     hipcc --offload-arch=gfx950 --cuda-device-only --no-gpu-bundle-output -O3 -std=c++17 -ffp-contract=off \
 *           -DCPX_VIT_SPEC_LG=<lg> -DCPX_VIT_SPEC_G0=<g0>u -DCPX_VIT_SPEC_G1=<g1>u -c commpy_amd/csrc/viterbi_cw.hip
 * gives a code object with the six fused kernels of THAT pair; commpy_amd/jit.py builds and caches it by (generators, build id).
 *   cpx_trellis_viterbi_spec_query   *lg = log2(states) and the generators in the kernel template's convention when the trellis would
 *                                    gain from such an object (else *lg = 0: built-in pair, other structure, or already attached)
 *   cpx_trellis_attach_viterbi_code  loads the image (hipModuleLoadData) and looks its kernels up BY THIS TRELLIS'S GENERATORS: an
 *                                    image of another pair or of other sources is refused (CPX_EINVAL), the trellis stays as it was;
 *                                    afterwards viterbi_decode batches that take the codeword-per-lane path launch the module's
 *                                    kernels (cpx_last_kernel: "... (code object of this pair)"); results are bit-identical
 *   cpx_trellis_detach_viterbi_code  back to the table-driven kernel (tests) */
int cpx_trellis_viterbi_spec_query(const cpx_trellis *t, int *lg, unsigned *g0, unsigned *g1);
int cpx_trellis_attach_viterbi_code(cpx_trellis *t, const void *image, size_t bytes);
int cpx_trellis_detach_viterbi_code(cpx_trellis *t);
int cpx_trellis_has_viterbi_code(const cpx_trellis *t);   /* 1: a code object is attached */
/* Fused hard demodulation + hard-decision Viterbi: replaces the pair
 *   bits = modem.demodulate(y, 'hard')            commpy/modulation.py:121-123
 *   viterbi_decode(bits, trellis, tb_depth, 'hard')  commpy/channelcoding/convcode.py:578-580, 661-749
 * for B codewords of nsym symbols each (y [B][nsym][2] float64 = complex128).  The kernel takes the hard decisions
 * itself while it prepares the branch metrics: the int8 bits are never written to (or re-read from) HBM -- 16 B in per
 * symbol instead of 16 B in + nb B out + 8 nb B in.  Output identical to the two calls.  len = nsym * bits-per-symbol
 * takes the place of len(coded_bits); trellises above 64 states return CPX_ELIMIT (use the two calls). */
int cpx_demod_hard_viterbi_batch(const cpx_modem *m, const cpx_trellis *t, const double *y_re_im, int64_t B,
                                 int64_t nsym, int64_t L, int64_t n_steps, int tb_depth, uint8_t *bits);
int cpx_demod_hard_viterbi_batch_dev(const cpx_modem *m, const cpx_trellis *t, const double *d_y_re_im, int64_t B,
                                     int64_t nsym, int64_t L, int64_t n_steps, int tb_depth, uint8_t *d_bits,
                                     void *stream);
/* Same as cpx_viterbi_decode_batch with the result widened to the reference's return type (`decoded_bits` is an
 * int array, convcode.py:711/749): bits64 [B][L] int64.  The compact bits cross PCIe, host threads widen them
 * straight into the caller's array: a single-threaded astype of 67 M bits costs more than decoding them. */
int cpx_viterbi_decode_batch_i64(const cpx_trellis *t, const double *coded, int64_t B, int64_t len,
                                 int64_t L, int64_t n_steps, int tb_depth, int decoding_type, int64_t *bits64);

/* ---- turbo codes: BCJR / MAP ---------------------------------------------------------------------
 * cpx_map_decode_batch replaces map_decode(sys, non_sys, trellis, noise_variance, L_int, mode)
 *   commpy/channelcoding/turbo.py:163-251 (+ _backward_recursion :78-111,
 *   _forward_recursion_decoding :114-158, _compute_branch_prob :62-76) for B codewords.
 *   sys, par, L_int [B][N] float64; L_ext [B][N] float64 (= L_int + log(app1/app0), turbo.py:145);
 *   bits [B][N] uint8 (all zero unless want_bits, i.e. mode == 'decode').
 * cpx_turbo_decode_batch replaces turbo_decode(...) turbo.py:254-333: n_iter x (MAP1, interleave,
 *   MAP2, de-interleave); perm = interleaver.p_array (interleavers.py:13-47), shared by the batch;
 *   L_int may be NULL (zeros).  bits [B][N] uint8, already de-interleaved.
 * Limits: k = 1 (I == 2, like the reference's priors[2]), n >= 2; N < 2^24 (map), N < 2^21 (turbo).  2 .. 16 states run the
 *   wave-pair kernels of bcjr.hip; larger trellises the literal kernel of bcjr_exact.hip alone (one codeword per lane, scratch
 *   (N + 1) * S doubles per lane: CPX_ELIMIT only beyond 4 GB for 64 lanes).
 * Inputs for which the reference's absolute-scale recursion underflows (turbo.py:62-76, :238-240: symbol amplitudes of 5 - 20 at
 *   sigma^2 <= 0.1, priors of e^-200) or that are not finite give what the reference gives -- NaN / +-inf LLRs, their decisions --:
 *   the fast kernels flag such codewords and a literal absolute-scale kernel decodes them again (blocks up to the scratch limit of
 *   that path).
 */
int cpx_map_decode_batch(const cpx_trellis *t, const double *sys, const double *par, const double *L_int,
                         int64_t B, int64_t N, double noise_variance, int want_bits, double *L_ext,
                         uint8_t *bits);
int cpx_map_decode_batch_dev(const cpx_trellis *t, const double *d_sys, const double *d_par,
                             const double *d_L_int, int64_t B, int64_t N, double noise_variance,
                             int want_bits, double *d_L_ext, uint8_t *d_bits, void *stream);
int cpx_turbo_decode_batch(const cpx_trellis *t, const double *sys, const double *p1, const double *p2,
                           const double *L_int_or_null, const int32_t *perm, int64_t B, int64_t N,
                           double noise_variance, int n_iter, uint8_t *bits);
int cpx_turbo_decode_batch_dev(const cpx_trellis *t, const double *d_sys, const double *d_p1,
                               const double *d_p2, const double *d_L_int_or_null, const int32_t *d_perm,
                               int64_t B, int64_t N, double noise_variance, int n_iter, uint8_t *d_bits,
                               void *stream);

/* ---- LDPC belief propagation ---------------------------------------------------------------------
 * cpx_ldpc_create: device copy of the Tanner graph produced by get_ldpc_code_params
 *   (commpy/channelcoding/ldpc.py:51-141): the edge list sorted by (check, variable) -- the
 *   row-major order SciPy keeps `message_matrix` in, which fixes the summation orders of
 *   ldpc.py:217-219 and :243.
 * cpx_ldpc_bp_decode_batch replaces ldpc_bp_decode(llr_vec, params, alg, n_iters) ldpc.py:144-254.
 *   llr       [B][n_v] float64, positive = bit 0 (ldpc.py:193); CLIPPED IN PLACE to +-500 (:186)
 *   alg       0 'SPA', 1 'MSA'
 *   dec_word  [n_v][B] int8 and out_llrs [n_v][B] float64: one block per COLUMN, the reference's
 *             output layout (ldpc.py:251-253)
 *   iters_done[B] int32 executed iterations per block (early exit ldpc.py:205-206), may be NULL
 * Limits (CPX_ELIMIT): n_v, n_c < 2^24.  Checks of up to 32 edges run the LDS-resident / tiled kernels (a row lives in registers
 * / one 32-bit sign mask); a code with a larger check is decoded by the literal kernel (ldpc_exact_kernel) alone.
 */
#define CPX_LDPC_SPA 0
#define CPX_LDPC_MSA 1
int cpx_ldpc_create(int n_vnodes, int n_cnodes, int64_t n_edges, const int32_t *edge_check,
                    const int32_t *edge_var, cpx_ldpc **out);
int cpx_ldpc_destroy(cpx_ldpc *c);
/* Compiled design ("blob"): the device tables of a Tanner graph -- sorted edge list, row / column
 * pointers, the variable-major view and the padded node tables the passes read -- in one position-independent,
 * checksummed byte string, so that a design file (ldpc.py:51-141 / write_ldpc_params :257-299) is compiled ONCE and the
 * result cached under the file's hash instead of being re-derived per code object.
 *   cpx_ldpc_blob_build        host only (no device needed); blob == NULL queries the size into *need;
 *                              blob must be 8-byte aligned
 *   cpx_ldpc_blob_info         validates a blob (magic, sizes, checksum, every index in range) and returns its dimensions
 *   cpx_ldpc_create_from_blob  validates, then uploads; cpx_ldpc_create == blob_build + create_from_blob */
int cpx_ldpc_blob_build(int n_vnodes, int n_cnodes, int64_t n_edges, const int32_t *edge_check, const int32_t *edge_var,
                        void *blob, size_t cap, size_t *need);
int cpx_ldpc_blob_info(const void *blob, size_t nbytes, int *n_vnodes, int *n_cnodes, int64_t *n_edges,
                       int *max_cnode_deg, int *max_vnode_deg);
int cpx_ldpc_create_from_blob(const void *blob, size_t nbytes, cpx_ldpc **out);
int cpx_ldpc_bp_decode_batch(const cpx_ldpc *c, double *llr, int64_t B, int alg, int n_iters,
                             int8_t *dec_word, double *out_llrs, int32_t *iters_done);
int cpx_ldpc_bp_decode_batch_dev(const cpx_ldpc *c, double *d_llr, int64_t B, int alg, int n_iters,
                                 int8_t *d_dec_word, double *d_out_llrs, int32_t *d_iters_done,
                                 void *stream);
/* The same decode with BLOCK-MAJOR outputs: dec_word [B][n_v] int8 and out_llrs [B][n_v] float64, one block per ROW.  This
 * is the memory the reference's own results live in: ldpc.py:251-253 returns `x.reshape(-1, n_blocks, order='F')`, an
 * F-ordered (n_v, n_blocks) VIEW of a buffer in which every block is contiguous -- so the Python layer wraps these arrays as
 * `dec.T` / `out.T` and returns objects with the reference's shape, dtype, values AND strides, and no transposition pass exists
 * anywhere (the [n_v][B] entry points above cost one: a staging buffer written, read back and written again).  HBM traffic of a
 * block is then SURVEY 8d's resident model exactly: llr in, out_llrs and dec_word out, 17 n_v bytes. */
int cpx_ldpc_bp_decode_batch_bm(const cpx_ldpc *c, double *llr, int64_t B, int alg, int n_iters,
                                int8_t *dec_word, double *out_llrs, int32_t *iters_done);
int cpx_ldpc_bp_decode_batch_bm_dev(const cpx_ldpc *c, double *d_llr, int64_t B, int alg, int n_iters,
                                    int8_t *d_dec_word, double *d_out_llrs, int32_t *d_iters_done,
                                    void *stream);
/* Two implementations: the LDS-resident path (csrc/ldpc_resident.hip: the decoder state of a block lives in the LDS of one
 * compute unit, one persistent launch, blocks retire and are replaced individually) whenever that state fits, else the tiled
 * HBM path (csrc/ldpc.hip).  Min-sum: the same arithmetic, identical results.  Sum-product: the tiled path and "resident-log"
 * share the log-domain row (identical results); the default resident kernel keeps the state as likelihood ratios -- no exp / log
 * inside an iteration, same dec_word, iteration counts and out_llrs contract, blocks it cannot carry (a NaN, an
 * iteration saturated in more than half of its rows) decoded again in place with the log-domain row (tests/test_ldpc_resident_gpu.py).
 * cpx_ldpc_set_path("auto" | "tiled" | "resident" | "resident-log") forces one (initial value: environment variable
 * CPX_LDPC_PATH); the "resident" modes fail with CPX_EINVAL instead of falling back.  cpx_last_kernel names what ran. */
int cpx_ldpc_set_path(const char *mode);

/* ---- PSK/QAM demodulation ------------------------------------------------------------------------
 * cpx_modem_create: device copy of Modem.constellation (commpy/modulation.py:68-77,159-172),
 *   M = 2^nbits complex points as [M][2] float64 (re, im), index = Gray-reordered symbol label.
 * cpx_demod_soft replaces Modem.demodulate(y, 'soft', noise_var) modulation.py:125-137:
 *   llr[i*nb + nb-1-b] = log( sum_{m:(m>>b)&1} e^{-|y_i-c_m|^2/noise_var} / sum_{m:!..} ... ),
 *   positive = bit 1, sums in increasing m.
 * cpx_demod_hard replaces Modem.demodulate(y, 'hard') modulation.py:121-123: first-min nearest
 *   point, MSB-first int8 bits.
 *   y [Ns][2] float64 (complex128 memory), llr [Ns*nb] float64, bits [Ns*nb] int8.
 */
int cpx_modem_create(const double *constellation_re_im, int M, cpx_modem **out);
int cpx_modem_destroy(cpx_modem *m);
/* Implementation choice of the soft demodulator for tests and A/B runs (initial value: environment variable CPX_DEMOD):
 * NULL / "auto": square QAM of 64 points and more takes the geometric-progression form (equally spaced Gray-labelled levels:
 * TWO exponentials and one division per axis, every other level by two multiplications) with table-driven exp / log (32-entry
 * tables in LDS); PSK and arbitrary constellations take the table-driven point-by-point kernel (round 6).  Both store a wave's LLRs
 * as one contiguous run of 16-byte stores: an output pointer that is only 8-byte aligned is served by the literal kernel instead.
 * "libm": the same forms with the library's exp / log (generic constellations: the literal kernel); "plain": one exponential per
 * level everywhere.
 * All are within 1e-5 of modulation.py:125-137 (measured: 1e-13); symbols near the underflow range are decided point by
 * point in the reference's order either way. */
int cpx_demod_set_path(const char *mode);
int cpx_demod_soft(const cpx_modem *m, const double *y_re_im, int64_t Ns, double noise_var, double *llr);
int cpx_demod_soft_dev(const cpx_modem *m, const double *d_y_re_im, int64_t Ns, double noise_var,
                       double *d_llr, void *stream);
/* the same with every LLR multiplied by `scale` on its way out: scale = -1 is the sign flip between Modem.demodulate (log P1/P0)
 * and ldpc_bp_decode (log P0/P1), test_ldpc.py:53-54, without a second pass over the LLRs; scale = 1 is cpx_demod_soft_dev */
int cpx_demod_soft_scaled_dev(const cpx_modem *m, const double *d_y_re_im, int64_t Ns, double noise_var, double scale,
                              double *d_llr, void *stream);
int cpx_demod_hard(const cpx_modem *m, const double *y_re_im, int64_t Ns, int8_t *bits);
int cpx_demod_hard_dev(const cpx_modem *m, const double *d_y_re_im, int64_t Ns, int8_t *d_bits,
                       void *stream);

/* ---- OFDM transmit / receive -------------------------------------------------------
 * ofdm_tx / ofdm_rx, commpy/modulation.py:265-296, with h = nsc / 2, float64 only (cpx_set_precision does not apply):
 *   TX, symbol i:  F = zeros(nfft); F[1:h+1] = x_i[h:]; F[nfft-h:] = x_i[:h] -- where the two ranges overlap (nsc > nfft - 1)
 *                  the second write wins; t = ifft(F) (1/nfft scaling); the block is t[nfft-P:] followed by t, where
 *                  P = cp_length if 0 < cp_length < nfft and P = nfft otherwise: the reference's t[-cp_length:] takes the whole
 *                  symbol for cp_length = 0 and for cp_length >= nfft, and that is reproduced, not corrected.
 *   RX, symbol i:  S = nfft + cp_length, X = fft(y[i S + cp_length : i S + cp_length + nfft]); x_hat_i = X[nfft-h:] ++ X[1:h+1];
 *                  ny / S symbols per row, leftover samples at the end are ignored.
 * cpx_ofdm_create: the plan of one (nfft, nsc, cp_length) on the current device: the twiddles (host-computed in long double from
 *   exactly reduced angles), the bin map and the kernel: power-of-two nfft up to 8192 take an LDS-resident Stockham FFT, every
 *   other size a direct DFT.  CPX_EINVAL for nfft < 2, nsc odd or < 2, h > nfft - 1, cp_length < 0; CPX_ELIMIT for nfft > 65536.
 * cpx_ofdm_tx:  x [B][nsym][nsc] complex128 (symbol-major: a modulated bit stream reshaped) -> out [B][nsym (P + nfft)].
 * cpx_ofdm_rx:  y [B][ny] complex128 -> out [B][ny / S][nsc].
 * Every symbol's output is bit-identical whatever the batch size, its place in the batch or the stream.
 */
typedef struct cpx_ofdm cpx_ofdm;
int cpx_ofdm_create(int nfft, int nsc, int cp_length, cpx_ofdm **out);
int cpx_ofdm_destroy(cpx_ofdm *plan);
int cpx_ofdm_tx(const cpx_ofdm *plan, const double *x_re_im, int64_t B, int64_t nsym, double *out_re_im);
int cpx_ofdm_tx_dev(const cpx_ofdm *plan, const double *d_x_re_im, int64_t B, int64_t nsym, double *d_out_re_im, void *stream);
int cpx_ofdm_rx(const cpx_ofdm *plan, const double *y_re_im, int64_t B, int64_t ny, double *out_re_im);
int cpx_ofdm_rx_dev(const cpx_ofdm *plan, const double *d_y_re_im, int64_t B, int64_t ny, double *d_out_re_im, void *stream);

/* ---- FIR filtering and frequency offset of sampled waveforms ------------------------------
 * What commpy/filters.py, utilities.upsample and impairments.py leave to numpy.convolve and numpy.exp, batched; complex128 data,
 * float64 arithmetic only (cpx_set_precision does not apply).
 * cpx_fir_create: a plan holding `ntaps` taps on the current device, real (taps_complex = 0: ntaps doubles) or complex
 *   (taps_complex = 1: ntaps interleaved re/im pairs).  1 <= ntaps <= 8192 (CPX_ELIMIT above); taps must be finite.
 * cpx_fir_interp:  x [B][n] -> out [B][n sps + ntaps - 1], row b = convolve(upsample(x[b], sps), taps), polyphase (the zeros
 *   between symbols are never formed); sps >= 1, sps = 1 is a plain full convolution.
 * cpx_fir_decim:   y [B][n] -> out [B][ceil((n + ntaps - 1 - offset) / sps)], row b = convolve(y[b], taps)[offset::sps] for
 *   0 <= offset < n + ntaps - 1; only the kept samples are computed.
 * cpx_freq_offset: out[b][k] = x[b][k] (cos t + i sin t), t = step k rounded once to float64, step = step[0] for the whole batch
 *   (step_batched = 0) or step[b] per row (step_batched = 1); the caller computes step = (2 pi)(delta_f / Fs).  In the _dev form
 *   `d_step` is a DEVICE pointer like the data, and out == x (in place) is allowed.
 * B = 0 succeeds without touching the device; n = 0 with B > 0 is CPX_EINVAL for the filters (numpy.convolve refuses an empty
 * operand).  Every output sample is summed over its taps in ascending tap index by fused multiply-adds: bit-identical whatever
 * the batch size, the row's place in the batch or the stream.
 */
typedef struct cpx_fir cpx_fir;
int cpx_fir_create(const double *taps, int ntaps, int taps_complex, cpx_fir **out);
int cpx_fir_destroy(cpx_fir *plan);
int cpx_fir_interp(const cpx_fir *plan, const double *x_re_im, int64_t B, int64_t n, int sps, double *out_re_im);
int cpx_fir_interp_dev(const cpx_fir *plan, const double *d_x_re_im, int64_t B, int64_t n, int sps, double *d_out_re_im, void *stream);
int cpx_fir_decim(const cpx_fir *plan, const double *y_re_im, int64_t B, int64_t n, int sps, int64_t offset, double *out_re_im);
int cpx_fir_decim_dev(const cpx_fir *plan, const double *d_y_re_im, int64_t B, int64_t n, int sps, int64_t offset,
                      double *d_out_re_im, void *stream);
int cpx_freq_offset(const double *x_re_im, int64_t B, int64_t n, const double *step, int step_batched, double *out_re_im);
int cpx_freq_offset_dev(const double *d_x_re_im, int64_t B, int64_t n, const double *d_step, int step_batched, double *d_out_re_im,
                        void *stream);

/* ---- Multipath channel and pilot-aided OFDM channel estimation ----------------------------
 * Not in the reference.  complex128 data, float64 arithmetic only (cpx_set_precision does not apply); B = 0 succeeds without a launch.
 * cpx_multipath:  x [B][nt][n], g [B][nr][nt][L] (g_batched = 1) or [nr][nt][L] shared by all rows (g_batched = 0) ->
 *   y [B][nr][n + L - 1], y[b][r] = sum_t convolve(x[b][t], g[b][r][t]): full length, which cpx_ofdm_rx takes as it is (it ignores
 *   trailing samples).  Every sample is one chain of fused multiply-adds from +0 over t ascending, then tap index ascending:
 *   bit-identical whatever the batch size, the row's place, the stream, and whether g is shared or replicated.  Taps are expected
 *   to be finite.  CPX_EINVAL: nt, nr or L < 1, n < 1 with B > 0, null pointers; CPX_ELIMIT: L > 1024 or nr nt L > 2048 (one
 *   row's taps are staged in 32 KB of LDS).  Noise: cpx_awgn_dev.
 * The entry points of a pilot plan are named cpx_pilots_*: the cpx_ofdm_* family is the transform of DESIGN.md 4.9 alone.
 * cpx_pilots_create: the pilot plan of a frame of nsym OFDM symbols x nsc used subcarriers (cpx_ofdm_tx's input order =
 *   cpx_ofdm_rx's output order) of nt transmit antennas.  Pilot i puts pil_val[i] on resource element (pil_sym[i], pil_sc[i]) of
 *   antenna pil_tx[i]; every other antenna is silent there; a resource element appears at most once.  All remaining resource
 *   elements carry data and are numbered d = 0 .. ndata - 1 (ndata = nsym nsc - npil), symbol-major, then subcarrier ascending.
 *   With k_0 < ... < k_{np_t - 1} the distinct pilot subcarriers of antenna t, `w_re_im` holds, antenna after antenna, the
 *   interpolation matrix W_t [nsc][np_t], complex, row-major; the engine does not interpret it.  CPX_EINVAL: nsc odd or < 2;
 *   nsym, nt or npil < 1; an index out of range; a repeated resource element; an antenna without a pilot; a pilot value that is
 *   zero or not finite; a W entry that is not finite.  CPX_ELIMIT: nt > 1024, or nsym nsc >= 2^30.
 * cpx_pilots_map:  data [B][ndata][nt] (vector-major, the layout of the MIMO detectors' symbols) -> grid [B][nt][nsym][nsc]: data at
 *   the data elements, pilots at their antenna's pilot elements, exact zeros elsewhere.  grid viewed as [B nt][nsym][nsc] is
 *   cpx_ofdm_tx's input, whose output is cpx_multipath's x.
 * cpx_pilots_estimate:  Y [B][nr][nsym][nsc] (cpx_ofdm_rx's output for B nr rows; fading constant over the frame -- a channel that
 *   moves inside the frame is followed by cpx_pilots_create_tv + cpx_pilots_estimate_tv below).
 *   LS[b][r][t][j] = (sum_s Y[b][r][s][k_j] conj(p_s) / |p_s|^2) / count over antenna t's pilots on subcarrier k_j in ascending
 *   symbol order; H^[b][k][r][t] = sum_j W_t[k][j] LS[b][r][t][j], an fma chain from +0 over ascending j.  Outputs, each nullable
 *   (at least one must be given): h_sc [B][nsc][nr][nt] = H^; y_data [B][ndata][nr] = Y at the data elements; h_data
 *   [B][ndata][nr][nt] = H^ of each data element's subcarrier -- (y_data, h_data) with V = B ndata vectors and h_batched = 1 are
 *   what cpx_mimo_ml, cpx_kbest_*, cpx_best_first, cpx_mimo_linear and cpx_mimo_list_* take.  A non-finite sample of Y makes NaNs
 *   in its own frame only; results are bit-identical whatever the batch size, the frame's place, the stream, the form (host or
 *   device) and the outputs requested.  CPX_EINVAL: nr < 1, no output; CPX_ELIMIT: nr > 1024.
 * Time-varying channels: a separable estimator, frequency first (W_t, as above), then time.
 * cpx_pilots_create_tv: cpx_pilots_create's arguments and checks, the same handle type, plus the time matrices.  With s_0 < ... <
 *   s_{ns_t - 1} the distinct pilot symbols of antenna t, the pattern must be a rectangle per antenna: on every one of those symbols
 *   antenna t has pilots on exactly its pilot subcarriers k_0 < ... < k_{np_t - 1} (comb and block patterns are; a staggered one is
 *   CPX_EINVAL, the message names the antenna and the symbol).  `v_re_im` holds, antenna after antenna, V_t [nsym][ns_t], complex,
 *   row-major: it spreads the estimates at the antenna's pilot symbols over all symbols, and the engine does not interpret it (linear,
 *   hold, Wiener and polynomial tracking are all "a matrix").  CPX_EINVAL also: v_re_im null, a V entry that is not finite.  The
 *   handle serves cpx_pilots_map and cpx_pilots_estimate as one of cpx_pilots_create does, bit for bit.
 * cpx_pilots_estimate_tv:  Y [B][nr][nsym][nsc] as above.
 *   LSp[b][r][t][i][j] = Y[b][r][s_i][k_j] c, c = conj(p) / |p|^2 of that pilot formed on the host: one complex multiply-add from +0,
 *     no averaging;
 *   Hp[b][i][k][r][t] = sum_j W_t[k][j] LSp[b][r][t][i][j], an fma chain from +0 over ascending j (cpx_pilots_estimate's, per pilot symbol);
 *   H^[b][s][k][r][t] = sum_i V_t[s][i] Hp[b][i][k][r][t], a chain of complex multiply-adds (re += vr hr, re -= vi hi, im += vr hi,
 *     im += vi hr, four fma) from +0 over ascending i.
 *   Outputs, each nullable (at least one must be given): h_sym [B][nsym][nsc][nr][nt] = H^; y_data [B][ndata][nr], exactly
 *   cpx_pilots_estimate's; h_data [B][ndata][nr][nt] = H^ at each data element's (symbol, subcarrier).  (y_data, h_data) feed the
 *   detectors with V = B ndata and h_batched = 1 as above.  A non-finite sample of Y stays in its own frame; results are bit-identical
 *   whatever the batch size, the frame's place, the stream, the form (host or device) and the outputs requested; B = 0 succeeds
 *   without a launch.  CPX_EINVAL: a plan made by cpx_pilots_create (no time matrices), nr < 1, no output; CPX_ELIMIT: nr > 1024.
 */
typedef struct cpx_ofdm_pilots cpx_ofdm_pilots;
int cpx_multipath(const double *x_re_im, const double *g_re_im, int g_batched, int64_t B, int nt, int nr, int64_t n, int L,
                  double *y_re_im);
int cpx_multipath_dev(const double *d_x_re_im, const double *d_g_re_im, int g_batched, int64_t B, int nt, int nr, int64_t n, int L,
                      double *d_y_re_im, void *stream);
int cpx_pilots_create(int nsc, int nsym, int nt, int64_t npil, const int32_t *pil_sym, const int32_t *pil_sc,
                           const int32_t *pil_tx, const double *pil_val_re_im, const double *w_re_im, cpx_ofdm_pilots **out);
int cpx_pilots_destroy(cpx_ofdm_pilots *plan);
int cpx_pilots_map(const cpx_ofdm_pilots *plan, const double *data_re_im, int64_t B, double *grid_re_im);
int cpx_pilots_map_dev(const cpx_ofdm_pilots *plan, const double *d_data_re_im, int64_t B, double *d_grid_re_im, void *stream);
int cpx_pilots_estimate(const cpx_ofdm_pilots *plan, const double *Y_re_im, int64_t B, int nr, double *h_sc, double *y_data,
                      double *h_data);
int cpx_pilots_estimate_dev(const cpx_ofdm_pilots *plan, const double *d_Y_re_im, int64_t B, int nr, double *d_h_sc, double *d_y_data,
                          double *d_h_data, void *stream);
int cpx_pilots_create_tv(int nsc, int nsym, int nt, int64_t npil, const int32_t *pil_sym, const int32_t *pil_sc,
                         const int32_t *pil_tx, const double *pil_val_re_im, const double *w_re_im, const double *v_re_im,
                         cpx_ofdm_pilots **out);
int cpx_pilots_estimate_tv(const cpx_ofdm_pilots *plan, const double *Y_re_im, int64_t B, int nr, double *h_sym, double *y_data,
                           double *h_data);
int cpx_pilots_estimate_tv_dev(const cpx_ofdm_pilots *plan, const double *d_Y_re_im, int64_t B, int nr, double *d_h_sym,
                               double *d_y_data, double *d_h_data, void *stream);

/* ---- OFDM timing and frequency-offset synchronisation ---------------------------------------
 * Not in the reference.  complex128 data, float64 arithmetic only (cpx_set_precision does not apply, no path switch); B = 0 succeeds
 * without a launch.  With y [B][nr][n], a lag D >= 1, a window W >= 1 and nd = n - D - W + 1:
 *   q[b][i] = sum_r conj(y[b][r][i]) y[b][r][i+D],  e[b][i] = 1/2 sum_r (|y[b][r][i]|^2 + |y[b][r][i+D]|^2),
 *   P[b][d] = sum_{i=d}^{d+W-1} q[b][i],  E[b][d] likewise from e,  M[b][d] = |P|^2 / E^2 where E > 0, +0 where E == 0, NaN where E
 *   is NaN.  M <= 1 up to rounding; the antennas of a row are combined before the modulus.  D = W = nfft / 2 is the Schmidl-Cox
 *   search on a two-halves preamble, D = nfft with W = cp_length the cyclic-prefix correlator.
 * Sums: the q axis is cut into tiles of 1024 anchored at multiples of 1024 within the row; every P[d], E[d] is assembled from
 *   in-tile prefix sums and whole-tile totals (csrc/sync.hip), so that the cost per output does not grow with W, no rounding involves
 *   a product further than 1023 positions from the window, and |P - exact| <= 2 (W + 2048 + 8) 2^-53 sqrt(2) sum |y_i| |y_{i+D}| over
 *   r and i in [d - 2048, d + W + 2048) within the row (E: the same with e under the sum).  Each value depends on the row's samples
 *   and (n, D, W, d) alone: bit-identical whatever the batch size, the row's place, the stream, the form (host or device) and the
 *   outputs requested.  A NaN or an infinity spoils windows of its own row only (those that share a tile sum with it).
 * cpx_sync_metric:    P [B][nd] complex, E [B][nd], M [B][nd]; each nullable, at least one must be given.
 * cpx_sync_estimate:  the fused search, nothing [B][nd] is written.  d_hat[b] = the smallest d in [d_lo, d_hi) n [0, nd) whose M is
 *   the largest of the range's non-NaN values, peak[b] = M[b][d_hat], step[b] = -atan2(Im P, Re P) / D at d_hat in radians per
 *   sample: what cpx_freq_offset and cpx_sync_align take to remove the offset.  A row without a non-NaN M: d_hat = -1, peak = step =
 *   NaN.  d_lo = 0, d_hi = INT64_MAX searches the whole row.  M and P are bit for bit those of cpx_sync_metric.
 * cpx_sync_align:     out[b][r][k] = s (cos t + i sin t), k < nout, with s = y[b][r][start[b] + offset + k], or exact +0 where that
 *   index is outside [0, n), and t = step[b] k rounded once: the rotation of cpx_freq_offset, bit for bit (start = 0, offset = 0,
 *   nout = n is cpx_freq_offset with step_batched = 1 on the B nr rows).  step == NULL: a pure gather, zeros are +0.  start [B] may
 *   be negative; in the _dev form start and step are DEVICE arrays, so cpx_sync_estimate_dev's outputs feed it without a host stage
 *   (offset = -cp_length turns the preamble's d_hat into the start of its cyclic prefix).  out must not alias y.
 * CPX_EINVAL: nr, D or W < 1; nd < 1 with B > 0; nout < 1; null pointers; no output requested; an empty search range (d_lo >= d_hi,
 *   or none of [0, nd) in it).  CPX_ELIMIT: nr > 1024; D or W > 2^20.
 */
int cpx_sync_metric(const double *y_re_im, int64_t B, int nr, int64_t n, int64_t D, int64_t W, double *P_re_im, double *E, double *M);
int cpx_sync_metric_dev(const double *d_y_re_im, int64_t B, int nr, int64_t n, int64_t D, int64_t W, double *d_P_re_im, double *d_E,
                        double *d_M, void *stream);
int cpx_sync_estimate(const double *y_re_im, int64_t B, int nr, int64_t n, int64_t D, int64_t W, int64_t d_lo, int64_t d_hi,
                      int64_t *d_hat, double *peak, double *step);
int cpx_sync_estimate_dev(const double *d_y_re_im, int64_t B, int nr, int64_t n, int64_t D, int64_t W, int64_t d_lo, int64_t d_hi,
                          int64_t *d_d_hat, double *d_peak, double *d_step, void *stream);
int cpx_sync_align(const double *y_re_im, int64_t B, int nr, int64_t n, const int64_t *start, const double *step, int64_t offset,
                   int64_t nout, double *out_re_im);
int cpx_sync_align_dev(const double *d_y_re_im, int64_t B, int nr, int64_t n, const int64_t *d_start, const double *d_step, int64_t offset,
                       int64_t nout, double *d_out_re_im, void *stream);

/* ---- MIMO detection ------------------------------------------------------------------------------
 * Replace mimo_ml / kbest of commpy/modulation.py:299-406 (with max_log_approx :599-646 for the soft output) for a batch of B
 * received vectors.  The constellation is the modem's (cpx_modem_create), float64 throughout.
 *   y [B][nr] complex (re, im); h [nr][nt] complex shared by the batch (h_batched = 0) or [B][nr][nt] (h_batched = 1);
 *   outputs are constellation INDICES.
 * cpx_mimo_ml:    idx [B][nt] of the first minimum of |y - H x|^2 over all m^nt hypotheses, antenna 0 the most significant
 *                 base-m digit (modulation.py:314-317).  CPX_EINVAL above 2^31 hypotheses per vector; CPX_ELIMIT when nr is
 *                 so large that one vector's H and residuals exceed 64 KB of LDS.
 * cpx_kbest_*:    K-best breadth-first search after a Householder QR of each H; the K smallest accumulated distances survive
 *                 each antenna, ties broken by the lowest child position (point index * nb_can + parent).  nt > nr: CPX_EINVAL.
 *   _hard         idx [B][nt] of the best surviving candidate;
 *   _soft         llr [B][nt * log2 m]: max-log LLRs over the final list on the original y and H, bit k of a candidate = the
 *                 MSB-first bits of its indices (the modem's labels), value (min_1 - min_0) / (2 noise_var), +-inf where no
 *                 candidate carries a bit value, IEEE results for noise_var = 0;
 *   _list         cand [B][Ke][nt] the final candidates in ascending distance (rows past count[b] hold -1), count [B];
 *                 Ke = min(K, m^nt).
 * States up to 64 KB per vector run LDS-resident; larger ones, or all after cpx_kbest_set_path("general") (initial value:
 * environment variable CPX_KBEST_PATH), take the same search with its state in a global workspace.  cpx_last_kernel names
 * what ran. */
int cpx_kbest_set_path(const char *mode);
int cpx_mimo_ml(const cpx_modem *m, const double *y_re_im, const double *h_re_im, int h_batched, int64_t B, int nr, int nt,
                int32_t *idx);
int cpx_mimo_ml_dev(const cpx_modem *m, const double *d_y_re_im, const double *d_h_re_im, int h_batched, int64_t B, int nr, int nt,
                    int32_t *d_idx, void *stream);
int cpx_kbest_hard(const cpx_modem *m, const double *y_re_im, const double *h_re_im, int h_batched, int64_t B, int nr, int nt,
                   int K, int32_t *idx);
int cpx_kbest_hard_dev(const cpx_modem *m, const double *d_y_re_im, const double *d_h_re_im, int h_batched, int64_t B, int nr,
                       int nt, int K, int32_t *d_idx, void *stream);
int cpx_kbest_soft(const cpx_modem *m, const double *y_re_im, const double *h_re_im, int h_batched, int64_t B, int nr, int nt,
                   int K, double noise_var, double *llr);
int cpx_kbest_soft_dev(const cpx_modem *m, const double *d_y_re_im, const double *d_h_re_im, int h_batched, int64_t B, int nr,
                       int nt, int K, double noise_var, double *d_llr, void *stream);
int cpx_kbest_list(const cpx_modem *m, const double *y_re_im, const double *h_re_im, int h_batched, int64_t B, int nr, int nt,
                   int K, int32_t *cand, int32_t *count);
int cpx_kbest_list_dev(const cpx_modem *m, const double *d_y_re_im, const double *d_h_re_im, int h_batched, int64_t B, int nr,
                       int nt, int K, int32_t *d_cand, int32_t *d_count, void *stream);

/* cpx_best_first: the soft-output best-first stack search of commpy/modulation.py:422-565 after a Householder QR of [H | y]:
 *   nr stacks (one per receive antenna, as the reference's nb_tx, nb_rx = h.shape), stack i truncated to stack_size[i-1]
 *   records after every iteration (stack_size has nr - 1 entries, further entries are ignored), LLR clipping at llr_max.
 *   llr [B][nr * log2 m] = (map metric - counter metric) * (+1 / -1 for the MAP's bit), position after position, bits in the
 *   label order of `labels` [m][log2 m] (0/1 bytes; null: the index bits, MSB first -- what Modem.demodulate(., 'hard')
 *   gives).  A vector that reaches no leaf (NaN / inf input) gets NaN LLRs.  Children of equal metric are taken in
 *   ascending constellation index.  CPX_EINVAL: nr < 2, nr > nt (the reference then reaches no leaf), a stack size < 1, a
 *   label entry other than 0 / 1; CPX_ELIMIT: nr > 64.  The iterations are capped at the number of tree nodes
 *   (sum_{c=1..nr} m^c), which the search cannot exceed: a vector that hits the cap is an engine fault (cpx_best_first:
 *   CPX_EHIP; _dev: iters[b] = -1 and NaN LLRs).  noise_var of the reference is not an argument: it does not use it.
 * cpx_best_first_dev: device pointers (labels too, nullable) on `stream`, except stack_size (host);
 *   d_iters [B] (nullable) receives the number of search iterations of each vector.
 * States up to 64 KB per vector run LDS-resident; larger ones, or all after cpx_best_first_set_path("general") (initial
 * value: environment variable CPX_BEST_FIRST_PATH), take the same search with its state in a global workspace. */
int cpx_best_first_set_path(const char *mode);
int cpx_best_first(const cpx_modem *m, const double *y_re_im, const double *h_re_im, int h_batched, int64_t B, int nr, int nt,
                   const int32_t *stack_size, double llr_max, const uint8_t *labels, double *llr);
int cpx_best_first_dev(const cpx_modem *m, const double *d_y_re_im, const double *d_h_re_im, int h_batched, int64_t B, int nr,
                       int nt, const int32_t *stack_size, double llr_max, const uint8_t *d_labels, double *d_llr,
                       int32_t *d_iters, void *stream);

/* ---- linear MIMO detection: zero forcing and MMSE (csrc/mimo_linear.hip) -----------------------------------------
 * Not in the reference.  y, h, h_batched, B, nr, nt and the modem as for the detectors above; any nr >= 1 and nt >= 1 (nt > nr too);
 * the modem must have m = 2^nbits points.  float64 only: cpx_set_precision is ignored and there is no path switch, nt picks the kernel
 * (nt <= 8: one vector per lane, registers; above: one wave per vector, LDS).  Per vector, with a regulariser reg >= 0:
 *   A = H^H H + reg I = L L^H (Cholesky),  z = A^-1 H^H y,  a_i = (A^-1)_ii,  g_i = 1 - reg a_i
 *   xhat [B][nt] complex  = z_i / g_i, the unbiased estimate;  nu [B][nt] = noise_var a_i / g_i, its noise variance.
 *   reg = 0 is zero forcing (xhat = H^+ y, nu_i = noise_var a_i), reg = N0 / Es unbiased MMSE: one kernel, only reg differs.
 *   idx [B][nt]           the first minimum of |xhat_i - s|^2 over the points in index order (strict <: a tie goes to the lowest
 *                         index, a NaN estimate to index 0, as cpx_mimo_ml's all-NaN metric);
 *   llr [B][nt * nbits]   (min_{s: bit k = 1} |xhat_i - s|^2 - min_{s: bit k = 0} |xhat_i - s|^2) / (2 nu_i) at [i * nbits + k], bit k
 *                         of a point = the MSB-first bits of its index (the modem's labels); positive: bit 0; the factor 2 is
 *                         cpx_kbest_soft's, so that either output feeds the same decoder.
 * Each output is nullable; at least one must be given.  A vector FAILS when a Cholesky pivot is not a positive finite number
 * (singular H under zero forcing, nt > nr with reg = 0, NaN / inf in H; positive in float64's terms: the pivot of column j must
 * exceed 4 (nr + nt) 2^-52 A_jj, what rounding can leave of an exactly singular matrix's pivot), when H^H y is not finite (NaN / inf in y) or when some g_i is
 * not positive: its xhat, nu and llr are NaN and its idx 0; no other vector is affected.  Every vector goes through the same
 * operations in the same order: outputs are bit-identical across batch sizes, positions in the batch, streams, shared / replicated H,
 * the host and device forms and whichever outputs are requested.
 * CPX_EINVAL: reg negative or NaN, noise_var NaN, no output requested, then a null modem / another device's modem / B < 0 / nr < 1 /
 * nt < 1, a modem without 2^nbits points, null y or h with B > 0; CPX_ELIMIT: a constellation (nt <= 8) or the state of one vector
 * (nt >= 9) above 64 KB of LDS.  B = 0 returns CPX_OK without a launch.  cpx_last_kernel names what ran, with nt, nr and m.
 * cpx_mimo_linear_dev: device pointers, asynchronous on `stream`. */
int cpx_mimo_linear(const cpx_modem *m, const double *y_re_im, const double *h_re_im, int h_batched, int64_t B, int nr, int nt,
                    double reg, double noise_var, int32_t *idx, double *llr, double *xhat_re_im, double *nu);
int cpx_mimo_linear_dev(const cpx_modem *m, const double *d_y_re_im, const double *d_h_re_im, int h_batched, int64_t B, int nr, int nt,
                        double reg, double noise_var, int32_t *d_idx, double *d_llr, double *d_xhat_re_im, double *d_nu, void *stream);

/* ---- list detection with a-priori LLRs, iterative detection and decoding (csrc/mimo_idd.hip) -------------------------------
 * A max-log soft MIMO detector over a candidate list that accepts priors, and the detector / decoder exchange of
 * commpy/links.py:345-407 (idd_decoder) on device buffers.  The list -- cand [B][Ke][nt] int32 constellation indices and count [B],
 * exactly what cpx_kbest_list writes -- is searched once on the channel metric; the priors reweigh it, they do not re-run the
 * tree search.  float64 only: cpx_set_precision is ignored and there is no path switch.  Bits are the modem's labels, MSB first,
 * antenna after antenna; an LLR is positive for bit 0.
 *   cpx_mimo_list_dist  dist [B][Ke] = norm(y - H x_c)^2 of every candidate (+inf past count[b]), summed as cpx_kbest_soft sums it:
 *                       per receive antenna r ascending, hx = 0 + sum_t H[r][t] x[t] (t ascending), s = 0 + sum_r |y_r - hx|^2,
 *                       sqrt(s) squared.  One thread per candidate: the order depends on nothing else.
 *   cpx_mimo_list_llr   with La_k = the prior clipped to [-clip, clip] (null: no prior) and S_c = the sum of La_k over the bits 1 of
 *                       candidate c (k ascending), cost_c = dist_c + 2 noise_var S_c and
 *                       llr_k = -(min_{c: b_k = 0} cost_c - min_{c: b_k = 1} cost_c) / (2 noise_var), clipped to [-clip, clip]; a bit
 *                       value no candidate carries counts as +inf (llr = +-clip).  This is min_{b_k = 1} - min_{b_k = 0} of
 *                       dist_c / (2 noise_var) + S_c, scaled by 2 noise_var so that a null or zero prior with clip = inf reproduces
 *                       cpx_kbest_soft bit for bit.  A NaN in a vector's y, H or prior makes all LLRs of that vector NaN.
 *   cpx_mimo_idd_exchange_dev   one IDD round in one launch: ext = dec_out - dec_in (the decoder's extrinsic LLRs),
 *                       post = the detector above with prior ext, dec_in <- post - ext (last != 0: dec_in <- post, what the
 *                       decision receives).  dec_in is the block-major buffer cpx_ldpc_bp_decode_batch_bm_dev clipped in place,
 *                       dec_out its out_llrs; both [B][nt nbits] seen per vector.
 *   cpx_mimo_llr_hard_dev       bits[i] = signbit(llr[i]) (int8), the hard decision on final LLRs.
 * CPX_EINVAL: clip <= 0 or NaN, noise_var not positive and finite, Ke < 1, a null pointer with B > 0, a modem without 2^nbits points; CPX_ELIMIT:
 * nt * nbits > 64 bits per vector, or a list whose costs and labels exceed 64 KB of LDS (Ke > 4064).  Ke is the row count of
 * cand, min(K, m^nt) for a list from cpx_kbest_list.  cpx_last_kernel names what ran. */
int cpx_mimo_list_dist(const cpx_modem *m, const double *y_re_im, const double *h_re_im, int h_batched, int64_t B, int nr, int nt,
                       const int32_t *cand, const int32_t *count, int Ke, double *dist);
int cpx_mimo_list_dist_dev(const cpx_modem *m, const double *d_y_re_im, const double *d_h_re_im, int h_batched, int64_t B, int nr,
                           int nt, const int32_t *d_cand, const int32_t *d_count, int Ke, double *d_dist, void *stream);
int cpx_mimo_list_llr(const cpx_modem *m, const int32_t *cand, const int32_t *count, const double *dist, int64_t B, int nt, int Ke,
                      const double *prior_or_null, double noise_var, double clip, double *llr);
int cpx_mimo_list_llr_dev(const cpx_modem *m, const int32_t *d_cand, const int32_t *d_count, const double *d_dist, int64_t B, int nt,
                          int Ke, const double *d_prior_or_null, double noise_var, double clip, double *d_llr, void *stream);
int cpx_mimo_idd_exchange_dev(const cpx_modem *m, const int32_t *d_cand, const int32_t *d_count, const double *d_dist, int64_t B,
                              int nt, int Ke, double *d_dec_in_inout, const double *d_dec_out, double noise_var, double clip,
                              int last, void *stream);
int cpx_mimo_llr_hard_dev(const double *d_llr, int64_t n, int8_t *d_bits, void *stream);

/* ---- MIMO link stages on the device ---------------------------------------------------
 * The MIMO flat-fading channel of commpy/channels.py:242-330 (MIMOFlatChannel.propagate, Kronecker model) and the hard-decision
 * error count of a MIMO link, so that a Monte-Carlo MIMO point never leaves HBM.  Device pointers, asynchronous on `stream`.
 *   cpx_mimo_channel_create   HOST matrices, complex (re, im), row-major: sqrt_rr = sqrtm(Rr) [nr][nr], sqrt_rt_T = sqrtm(Rt).T [nt][nt],
 *                             mean [nr][nt] -- the three matrices propagate uses (fading_param); an exact identity sqrt_rr / sqrt_rt_T
 *                             (the uncorrelated case) skips its product.  Non-finite entries: CPX_EINVAL.
 *   cpx_mimo_channel_run_dev  V vectors of nt symbols: d_bits [V][nt][nb] uint8 (the modem's labels, MSB first: modulate_kernel and
 *                             the reference's row-major reshape(nb_vect, nb_tx)) -> d_h_re_im [V][nr][nt] = A G Bt + mean with G of
 *                             i.i.d. CN(0, 1) entries (N(0, 1/2) per component) and d_y_re_im [V][nr] = H x + noise_scale (n_re + j n_im),
 *                             n ~ N(0, 1).  Philox streams keyed by (seed, stream_fading, (first_vector + v) nr nt + r nt + a) for G and
 *                             (seed, stream_noise, (first_vector + v) nr + r) for the noise (cpx_awgn_dev's draws), so a batch split
 *                             into launches at any vector gives the same bytes.  Sums run in ascending index order from 0: T = A G
 *                             (over q), H = T Bt (over p) + mean, y = H x (over a) + noise.  Any nr, nt >= 1.
 *   cpx_mimo_hard_errors_dev  errs [T] int32: bits of msg [T][bits_per_tx] uint8 that differ from the MSB-first nb-bit labels of the
 *                             detected indices d_idx (symbol s of transmission t = d_idx[t bits_per_tx / nb + s], i.e. [V][nt] with
 *                             whole vectors per transmission): what mimo_receiver's hard path and LinkModel count on the host.
 *                             bits_per_tx must be a multiple of nb (CPX_EINVAL).
 * The handle belongs to the device that was current at cpx_mimo_channel_create.
 */
typedef struct cpx_mimo_channel cpx_mimo_channel;
int cpx_mimo_channel_create(int nr, int nt, const double *sqrt_rr, const double *sqrt_rt_T, const double *mean, cpx_mimo_channel **out);
int cpx_mimo_channel_destroy(cpx_mimo_channel *ch);
int cpx_mimo_channel_run_dev(const cpx_mimo_channel *ch, const cpx_modem *m, const uint8_t *d_bits, int64_t V, uint64_t first_vector,
                             double noise_scale, uint64_t seed, uint64_t stream_fading, uint64_t stream_noise, double *d_y_re_im,
                             double *d_h_re_im, void *stream);
int cpx_mimo_hard_errors_dev(const int32_t *d_idx, int nb, const uint8_t *d_msg, int64_t T, int64_t bits_per_tx, int32_t *d_errs,
                             void *stream);

/* ---- link-simulation stages around the decoders ("next" rows) ---------------------------
 * Device-resident (all pointers are device pointers, asynchronous on `stream`), so that a Monte-Carlo
 * BER sweep (commpy/links.py:155-267, commpy/wifi80211.py:132-216) never leaves HBM.
 *   cpx_random_bits_dev       message bits (links.py:229); Philox4x32-10 counter stream (seed, stream_id)
 *   cpx_conv_encode_batch_dev conv_encode(msg, trellis, termination) convcode.py:475-558 for B rows:
 *                             msg [B][nmsg] uint8 -> coded [B][nout] uint8 (nout as the reference computes
 *                             number_outbits; rsc = code_type == 'rsc'; terminate = (termination == 'term') for
 *                             recursive codes -- the only case whose tail is clocked, convcode.py:538 -- and
 *                             (termination != 'cont') otherwise; positions past the clocked steps are zero)
 *   cpx_gather_u8_dev         out[b][j] = in[b][idx[j]]: puncturing (convcode.py:752-774) with the kept
 *                             positions as idx
 *   cpx_gather_f64_dev        out[b][j] = idx[j] >= 0 ? in[b][idx[j]] : 0: depuncturing (convcode.py:777-804)
 *   cpx_modulate_dev          Modem.modulate modulation.py:79-98: nb bits MSB-first -> constellation point
 *   cpx_awgn_dev              y = x + scale_re*n_re + 1j*scale_im*n_im, n ~ N(0,1) (channels.py:37-55)
 *   cpx_bsc_dev / cpx_bec_dev bsc(input_bits, p_t) commpy/channels.py:652-673 / bec(input_bits, p_e) :630-649: one uniform
 *                             draw per bit (Philox stream (seed, stream_id)), flipped / erased to -1 where the draw is
 *                             <= p.  Outputs: int8 (the reference's integer bits) and / or float64 (what
 *                             viterbi_decode(..., 'hard') takes, BASELINE config 1); either may be NULL.  p outside
 *                             [0, 1] (or NaN): CPX_EINVAL
 *   cpx_count_errors_dev      errs[b][c] = sum(msg[b, chunk c] ^ dec[b, chunk c]) (links.py:252-256)
 *   cpx_scale_f64_dev         y = a*x, e.g. the sign flip between Modem.demodulate (log P1/P0) and ldpc_bp_decode
 *                             (log P0/P1), test_ldpc.py:53-54
 *
 * Random streams (csrc/cpx_rng.h; modelled by tests/rng_model.py).  The draws are not NumPy's MT19937 stream: every one is an exactly
 * specified function of (seed, stream_id, element index i), so a kernel may regenerate any of them anywhere.
 *   words      (w0, w1, w2, w3) = Philox4x32-10 (Salmon et al., SC'11) of the counter (c0, c1, c2, c3) = (i lo, i hi, stream_id lo,
 *              stream_id hi) under the key (k0, k1) = (seed lo, seed hi): every 64-bit value is split low 32-bit word first.
 *   uniform    u01(hi, lo) = m 2^-53 with m = ((hi >> 5) << 26 | lo >> 6) + 1 in [1, 2^53]: the top 27 bits of `hi` above the top 26
 *              bits of `lo`; u01 is in (0, 1] and exact in float64.
 *   bits       cpx_random_bits_dev: message bit 16 i + j is bit j (LSB first) of the low 16 bits of w0 at counter i.
 *   bsc / bec  two draws per counter: position 2 i from u01(w0, w1), position 2 i + 1 from u01(w2, w3), both at counter i; a position
 *              is flipped / erased where (m - 1) 2^-53 <= p, the [0, 1) draw of the reference's `random(n) <= p`.
 *   awgn       element i: u1 = u01(w0, w1), u2 = u01(w2, w3), rad = sqrt(-2 log u1),
 *              y.re = x.re + (scale_re * rad) * cos(2 pi u2), y.im = x.im + (scale_im * rad) * sin(2 pi u2), float64 without FMA
 *              contraction in that order; a zero scale leaves its component of x bit-identical.  log, sqrt and sincospi are the
 *              device library's: the result is within a few ulp of the noise term of the model's.
 */
int cpx_random_bits_dev(uint8_t *d_bits, int64_t n, uint64_t seed, uint64_t stream_id, void *stream);
int cpx_conv_encode_batch_dev(const cpx_trellis *t, const uint8_t *d_msg, int64_t B, int64_t nmsg, int terminate,
                              int rsc, uint8_t *d_coded, int64_t nout, void *stream);
int cpx_gather_u8_dev(const uint8_t *d_in, int64_t B, int64_t nin, const int32_t *d_idx, int64_t nout,
                      uint8_t *d_out, void *stream);
int cpx_gather_f64_dev(const double *d_in, int64_t B, int64_t nin, const int32_t *d_idx, int64_t nout,
                       double *d_out, void *stream);
int cpx_modulate_dev(const cpx_modem *m, const uint8_t *d_bits, int64_t nsym, double *d_sym_re_im, void *stream);
int cpx_awgn_dev(const double *d_x_re_im, int64_t n, double scale_re, double scale_im, uint64_t seed,
                 uint64_t stream_id, double *d_y_re_im, void *stream);
int cpx_scale_f64_dev(const double *d_x, int64_t n, double a, double *d_y, void *stream);
int cpx_bsc_dev(const uint8_t *d_bits, int64_t n, double p_t, uint64_t seed, uint64_t stream_id, int8_t *d_out_i8,
                double *d_out_f64, void *stream);
int cpx_bec_dev(const uint8_t *d_bits, int64_t n, double p_e, uint64_t seed, uint64_t stream_id, int8_t *d_out_i8,
                double *d_out_f64, void *stream);
int cpx_count_errors_dev(const uint8_t *d_msg, int64_t msg_stride, const uint8_t *d_dec, int64_t dec_stride,
                         int64_t B, int64_t nchunks, int64_t chunk, int32_t *d_errs, void *stream);

/* ---- Doppler-fading multipath channel: time-varying taps (csrc/fading.hip; modelled by tests/fading_model.py) -------
 * Not in the reference.  A tapped delay line whose tap gains follow Clarke's model (a sum of Ns sinusoids per path, Jakes Doppler
 * spectrum), Rayleigh or Rician per tap, drawn from the random streams above.  complex128 data, float64 arithmetic only
 * (cpx_set_precision does not apply, no path switch, no environment variable); B = 0 succeeds without a launch.
 * Parameters.  fd: maximum Doppler in cycles per sample, 0 <= fd <= 0.5.  n_sin = Ns: sinusoids per path, 1 <= Ns <= 256.  pdp[L]:
 *   linear tap powers, finite and >= 0.  kf[L]: Rician K factor per tap, finite and >= 0, or NULL for all zero.  fd_los: Doppler of
 *   the line-of-sight component in cycles per sample, |fd_los| <= 0.5.  hold >= 1: samples per gain block.  t0 >= 0: the time of a
 *   row's output sample 0.  first_row: the row number of b = 0 (as first_vector of cpx_mimo_channel_run_dev), so that rows [0, B) in
 *   one call or in several give the same bytes.  pdp and kf are HOST arrays in both forms (they are read before the call returns).
 * Counters.  Path p = (((first_row + b) nr + r) nt + t) L + l, modulo 2^64.  Sinusoid s < Ns of path p uses counter p (Ns + 1) + s,
 *   counter p (Ns + 1) + Ns belongs to the path's line of sight (all modulo 2^64).  From a counter's words: u_a = u01(w0, w1),
 *   u_b = u01(w2, w3).
 * Sinusoid parameters.  nu_s = fd * cospi(2 u_a) (one cospi, one multiply), phi_s = u_b.  Line of sight: nu = fd_los, phi = u_b of
 *   its counter; its u_a is unused.
 * Gain of block j.  tau = t0 + j hold, exact in float64: t0 + nblk hold >= 2^52 is CPX_EINVAL.  Per sinusoid psi = fma(nu_s, tau,
 *   phi_s), rho = psi - rint(psi) (exact), (sn, cs) = sincospi(2 rho).  S = the sum of (cs, sn) over s ascending, plain adds from +0.
 *   G = a_l S with a_l = sqrt(pdp[l] / ((1 + kf[l]) Ns)) formed on the host (G.re = a_l S.re, G.im = a_l S.im).  Where kf[l] > 0, and
 *   only there, the line of sight is added: G.re = fma(c_l, cs_los, G.re), G.im = fma(c_l, sn_los, G.im) with c_l = sqrt(pdp[l] kf[l]
 *   / (1 + kf[l])).  pdp[l] == 0 gives exact +0.  The antenna pairs are independent (no spatial correlation).  No recurrence runs
 *   along time: a gain does not depend on where a call starts, on the batch or on the stream.  cospi and sincospi are the device
 *   library's: nu and the gains are within a few ulp of the model's.
 * Layout.  G [B][nblk][nr][nt][L]: a cpx_multipath tap set per block; nblk = ceil((n + L - 1) / hold) where G belongs to a
 *   convolution.
 * Convolution.  y[b][r][m] = sum_t sum_l G[b][m div hold][r][t][l] x[b][t][m - l] for m < n + L - 1: cpx_multipath's chain (one
 *   chain of fused multiply-adds from +0 over t ascending, then l ascending, the four fmas of a tap in the same order; terms outside
 *   the row are skipped or meet zeros), so with gains that do not change from block to block it is cpx_multipath bit for bit, for
 *   every hold.  Limits as cpx_multipath: L <= 1024, nr nt L <= 2048.
 * cpx_fading_params:    (nu, phi) of every sinusoid and of the line of sight, [B][nr][nt][L][Ns + 1][2] float64.
 * cpx_fading_gains:     G for nblk blocks from t0.
 * cpx_fading_convolve:  the convolution with the caller's G [B][nblk][nr][nt][L] (g_batched = 1) or [nblk][nr][nt][L] shared by all
 *   rows (g_batched = 0).
 * cpx_fading_channel:   gains, then the convolution, in one call: y [B][nr][n + L - 1] and / or G (each nullable, at least one must
 *   be given; x may be NULL where y is).  Without G the gains live in the scratch arena, in chunks of whole rows or, where one row's
 *   gains are larger than the budget, of whole blocks of one row: never more than CPX_FADING_SCRATCH_BYTES (plus 16 KB for the tap
 *   scales, which every gains call keeps there); the result is bit-identical to cpx_fading_gains followed by cpx_fading_convolve.
 * CPX_EINVAL: the parameter ranges above, nr, nt or L < 1, n < 1 with B > 0, nblk < 1, null pointers, no output requested, sizes that
 *   overflow.  CPX_ELIMIT: L > 1024, nr nt L > 2048, Ns > 256.  All are reported before a device is looked for.
 */
#define CPX_FADING_SCRATCH_BYTES 67108864   /* 64 MiB */
int cpx_fading_params(int64_t B, int nr, int nt, int L, int n_sin, double fd, double fd_los, uint64_t seed, uint64_t stream_id,
                      uint64_t first_row, double *params);
int cpx_fading_params_dev(int64_t B, int nr, int nt, int L, int n_sin, double fd, double fd_los, uint64_t seed, uint64_t stream_id,
                          uint64_t first_row, double *d_params, void *stream);
int cpx_fading_gains(int64_t B, int nr, int nt, int L, const double *pdp, const double *kf, int n_sin, double fd, double fd_los,
                     int64_t hold, int64_t t0, int64_t nblk, uint64_t seed, uint64_t stream_id, uint64_t first_row, double *G_re_im);
int cpx_fading_gains_dev(int64_t B, int nr, int nt, int L, const double *pdp, const double *kf, int n_sin, double fd, double fd_los,
                         int64_t hold, int64_t t0, int64_t nblk, uint64_t seed, uint64_t stream_id, uint64_t first_row,
                         double *d_G_re_im, void *stream);
int cpx_fading_convolve(const double *x_re_im, const double *G_re_im, int g_batched, int64_t B, int nt, int nr, int64_t n, int L,
                        int64_t hold, double *y_re_im);
int cpx_fading_convolve_dev(const double *d_x_re_im, const double *d_G_re_im, int g_batched, int64_t B, int nt, int nr, int64_t n, int L,
                            int64_t hold, double *d_y_re_im, void *stream);
int cpx_fading_channel(const double *x_re_im, int64_t B, int nt, int nr, int64_t n, int L, const double *pdp, const double *kf, int n_sin,
                       double fd, double fd_los, int64_t hold, int64_t t0, uint64_t seed, uint64_t stream_id, uint64_t first_row,
                       double *y_re_im, double *G_re_im);
int cpx_fading_channel_dev(const double *d_x_re_im, int64_t B, int nt, int nr, int64_t n, int L, const double *pdp, const double *kf,
                           int n_sin, double fd, double fd_los, int64_t hold, int64_t t0, uint64_t seed, uint64_t stream_id,
                           uint64_t first_row, double *d_y_re_im, double *d_G_re_im, void *stream);

/* ---- the stages of one Monte-Carlo point in front of the decoder as ONE kernel (round 6; same SURVEY 8f rows) ----------------------
 * random bits -> conv_encode ('cont') -> puncturing -> Modem.modulate -> AWGN -> Modem.demodulate('soft') -> depuncturing
 * (links.py:229-250, wifi80211.py:178-206, convcode.py:475-558, :752-804, modulation.py:79-141, channels.py:37-55) for T
 * transmissions of `nbits` message bits, without the five intermediate arrays: every lane produces one symbol's LLRs from its index
 * and the counter-based streams (seed, stream_bits) / (seed, stream_noise).  The results equal those of the staged calls
 * cpx_random_bits_dev(d_msg, T*nbits, seed, stream_bits) ... cpx_gather_f64_dev bit for bit.
 *   cpx_link_front_create   HOST tables: keep_idx[ntx] = coded position of transmitted bit t (NULL: no puncturing), pos_idx[ntx] =
 *                           decoder-input position of transmitted bit t among nde (NULL: t; the others are set to 0.0), both
 *                           increasing.  CPX_ELIMIT when the combination is not what the kernel is built for (feed-forward k = 1
 *                           trellis of <= 64 states, square QAM of 4..256 points with equally spaced Gray levels, a symbol depending on
 *                           <= 49 message bits): the caller keeps the staged calls.  The handle refers to `t` and `m`: destroy it first.
 *   cpx_link_front_run_dev  d_msg [T][nbits] uint8, d_llr [T][nde] float64 (LLR * llr_scale), d_rx_re_im optional [T][ntx/nb][2]
 *                           noisy symbols (NULL: not stored).  scale_re / scale_im as cpx_awgn_dev.  CPX_ELIMIT in the non-default
 *                           demodulator modes (cpx_demod_set_path, fp32-fast) and when 1 / noise_var is not a normal number.
 */
typedef struct cpx_link_front cpx_link_front;
int cpx_link_front_create(const cpx_trellis *t, const cpx_modem *m, int64_t nbits, const int32_t *keep_idx, int64_t ntx,
                          const int32_t *pos_idx, int64_t nde, cpx_link_front **out);
int cpx_link_front_destroy(cpx_link_front *lf);
int cpx_link_front_run_dev(const cpx_link_front *lf, int64_t T, double noise_var, double scale_re, double scale_im,
                           double llr_scale, uint64_t seed, uint64_t stream_bits, uint64_t stream_noise, uint8_t *d_msg,
                           double *d_llr, double *d_rx_re_im, void *stream);

/* ---- channel encoders on the device ("next" rows) --------------------------------
 * Device pointers, asynchronous on `stream`; bit-exact integer work.
 *   cpx_turbo_encode_batch_dev  turbo_encode(msg, trellis1, trellis2, interleaver) commpy/channelcoding/turbo.py:14-59
 *       for B rows: msg [B][N] uint8 -> sys [B][N], p1 [B][N], p2 [B][np2] (np2 >= N; entries past N are 0:
 *       turbo.py:47,53 pass 'rsc' as the termination argument, so conv_encode (convcode.py:538) clocks no
 *       tail and leaves the tail of its output zero; the reference returns len(p2) = 2(N+m2)-m2).
 *       Component codes must be rate 1/2 (the [::2] / [1::2] split of turbo.py:48-49).  perm = the
 *       interleaver's p_array (interleavers.py:45: out[i] = in[p[i]]), int32 [N], 16-byte aligned.
 *       mode: 0 auto, 1 one-codeword-per-lane walk, 2 wave-per-codeword state-map scan (<= 16 states).
 *   cpx_ldpc_encoder_create     packs a GF(2) generator: gen_bits [m][k] uint8 (0/1), parity = gen . msg mod 2 --
 *       `generator_matrix` of build_matrix (ldpc.py:44-48) reduced mod 2; k <= 8192.
 *   cpx_ldpc_encode_batch_dev   triang_ldpc_systematic_encode (ldpc.py:302-354) for B blocks: msg [B][k] uint8 ->
 *       code [B][k+m] uint8, systematic part first (:354); row b is column b of the reference's result.
 */
typedef struct cpx_ldpc_encoder cpx_ldpc_encoder;
int cpx_turbo_encode_batch_dev(const cpx_trellis *t1, const cpx_trellis *t2, const uint8_t *d_msg, int64_t B, int64_t N,
                               const int32_t *d_perm, uint8_t *d_sys, uint8_t *d_p1, uint8_t *d_p2, int64_t np2,
                               int mode, void *stream);
int cpx_ldpc_encoder_create(const uint8_t *gen_bits, int64_t m, int64_t k, cpx_ldpc_encoder **out);
int cpx_ldpc_encoder_destroy(cpx_ldpc_encoder *e);
int cpx_ldpc_encode_batch_dev(const cpx_ldpc_encoder *e, const uint8_t *d_msg, int64_t B, uint8_t *d_code,
                              void *stream);

/* ---- polar codes: encoder, successive cancellation and CRC-aided list decoding (csrc/polar.hip) --------
 * x = u F^{(x)n} over GF(2), F = [[1,0],[1,1]], natural order (no bit reversal), N = 2^n <= 8192.  The K positions with frozen[i] = 0
 * carry the information bits, in increasing position; with a CRC of crc_bits = c bits (1 <= c <= 32, c < K) these are A = K - c message
 * bits followed by the CRC bits, most significant first, else A = K.  crc_table [K] uint32: entry k = x^(K-1-k) mod g (NULL and
 * crc_bits = 0: no CRC); a word passes iff the XOR of the entries of its one bits is 0.
 *   cpx_polar_create      validates the mask and the table (CPX_EINVAL, before a device is looked for) and uploads them.
 *   cpx_polar_encode      msg [B][A] uint8 -> x [B][N] uint8 (CRC appended on the device).
 *   cpx_polar_decode      llr [B][N] float64, positive = bit 0.  L = 1: successive cancellation; L in {2, 4, 8, 16, 32}: list decoding,
 *                         min-sum f and exact g in float64, the list sorted stably by path metric at every information bit; the chosen
 *                         path is the lowest rank that passes the CRC (rank 0 and crc_ok = 0 if none does; rank 0 and crc_ok = 1 without
 *                         a CRC).  L * N <= 8192, else CPX_ELIMIT.  Every output may be NULL (not all of them): bits [B][A] uint8,
 *                         crc_ok [B] uint8, metric [B] float64 (of the chosen path), u_llr [B][N] float64 (the decision LLR of every
 *                         position; L = 1 only, else CPX_EINVAL), list_bits [B][L][K] uint8 (information bits by rank), list_metric
 *                         [B][L] float64, list_live [B] int32 (paths alive at the end = min(L, 2^K)); rows past the live count hold
 *                         zeros and metrics of +inf.  Bit-identical to tests/polar_model.py; the precision mode has no effect.
 * The _dev forms take device pointers and a stream and are asynchronous; the others take host pointers and return synchronised.
 * B = 0 returns CPX_OK without a launch. */
typedef struct cpx_polar cpx_polar;
int cpx_polar_create(int N, const uint8_t *frozen, int crc_bits, const uint32_t *crc_table, cpx_polar **out);
int cpx_polar_destroy(cpx_polar *p);
int cpx_polar_encode(const cpx_polar *p, const uint8_t *msg, int64_t B, uint8_t *x);
int cpx_polar_encode_dev(const cpx_polar *p, const uint8_t *d_msg, int64_t B, uint8_t *d_x, void *stream);
int cpx_polar_decode(const cpx_polar *p, const double *llr, int64_t B, int L, uint8_t *bits, uint8_t *crc_ok, double *metric,
                     double *u_llr, uint8_t *list_bits, double *list_metric, int32_t *list_live);
int cpx_polar_decode_dev(const cpx_polar *p, const double *d_llr, int64_t B, int L, uint8_t *d_bits, uint8_t *d_crc_ok, double *d_metric,
                         double *d_u_llr, uint8_t *d_list_bits, double *d_list_metric, int32_t *d_list_live, void *stream);

/* ---- binary BCH codes: systematic encoder and bounded-distance decoder (csrc/bch.hip) -------------------
 * Narrow-sense code of length n <= 2^m - 1 (shortened below that) over GF(2^m), 3 <= m <= 14, correcting t <= 32 errors.  A word is n
 * bytes 0 / 1; byte i is the coefficient of x^(n-1-i): k = n - deg g message bits, then the n - k bits of x^(n-k) m(x) mod g(x).
 *   cpx_bch_create   prim_poly: the field's polynomial with its leading term (bit i = coefficient of x^i); genpoly_bits [degree + 1]
 *                    uint8, entry i = coefficient of x^i of the generator.  Checked before a device is looked for: m, t, n and a degree
 *                    above 448 (CPX_ELIMIT); prim_poly of degree m under which x generates the multiplicative group, 1 <= degree < n,
 *                    leading and constant coefficient 1, g(alpha^j) = 0 for j = 1 .. 2t (CPX_EINVAL).  Any such g is encoded and decoded.
 *   cpx_bch_encode   msg [B][k] uint8 (bit 0 of a byte counts) -> word [B][n] uint8.
 *   cpx_bch_decode   in [B][n] uint8 hard decisions (non-zero = 1).  S_1 .. S_2t all zero: accepted, 0 errors.  Else Berlekamp-Massey
 *                    over the 2t syndromes gives sigma of length L; the word is corrected iff L <= t, sigma's coefficient of x^L is
 *                    non-zero and sigma has exactly L roots among the inverse locators of the positions 0 .. n - 1 (a root in the
 *                    shortened-away positions is a failure).  Outputs, each may be NULL (not all): bits [B][k] uint8, word [B][n]
 *                    uint8, errors [B] int32 = the number of corrected bits, -1 after a failure (bits and word then hold the received
 *                    word as 0 / 1).  Equal to tests/bch_model.py byte for byte.
 * The _dev forms take device pointers and a stream and are asynchronous; the others take host pointers and return synchronised.
 * B = 0 returns CPX_OK without a launch. */
typedef struct cpx_bch cpx_bch;
int cpx_bch_create(int m, uint32_t prim_poly, int n, int t, const uint8_t *genpoly_bits, int genpoly_degree, cpx_bch **out);
int cpx_bch_destroy(cpx_bch *p);
int cpx_bch_encode(const cpx_bch *p, const uint8_t *msg, int64_t B, uint8_t *word);
int cpx_bch_encode_dev(const cpx_bch *p, const uint8_t *d_msg, int64_t B, uint8_t *d_word, void *stream);
int cpx_bch_decode(const cpx_bch *p, const uint8_t *in, int64_t B, uint8_t *bits, uint8_t *word, int32_t *errors);
int cpx_bch_decode_dev(const cpx_bch *p, const uint8_t *d_in, int64_t B, uint8_t *d_bits, uint8_t *d_word, int32_t *d_errors,
                       void *stream);

/* ---- Chase-II soft-decision BCH decoding with Pyndiah's soft output (csrc/bch_chase.hip) ----------------
 * Works on a cpx_bch handle.  Per word of n float64 values x_i = llr_i, or fl(llr_i + fl(alpha prior_i)) with a prior (positive = bit
 * 0): hard decisions h_i = (x_i < 0), reliabilities |x_i|; the p least reliable positions by (|x_i|, i) ascending, 1 <= p <= min(8, n);
 * each of the 2^p test patterns tau (bit j flips the j-th of them) is decoded by the rule of cpx_bch_decode; a success is a candidate
 * with the metric M = sum of |x_i| over the positions where it differs from h, added serially in ascending position order.  The
 * decision D is the candidate of least metric (ties: lowest tau); without a candidate D = h, metric = +inf, extrinsic = 0.
 * extrinsic_i = s_i (M_C - M_D) - x_i, s_i = +1 for d_i = 0 and -1 otherwise, M_C the least metric of the candidates that differ from
 * D at i; s_i beta where there is none (beta >= 0, finite).  A word holding a non-finite x_i is rejected on its own: candidates = -1,
 * metric = +inf, the hard decisions (NaN: bit 0), extrinsic 0.  Equal to tests/chase_model.py bit for bit.
 *   cpx_chase_bch_dev  words (b, j), b < B, j < J; element i of word (b, j) of llr, prior, extrinsic and codeword is at
 *                      b sb + j sj + i si (in elements): rows and columns of a block decode in place; a flat batch is J = 1, sb = n,
 *                      si = 1.  The words must not overlap (CPX_EINVAL): either sj > (n-1) si or si > (J-1) sj, and sb above both
 *                      spans.  bits is dense and nested as the input: [B][J][k] in the first case (and for J = 1), [B][k][J] in the
 *                      second.  metric and candidates are [B][J].  prior may be NULL; extrinsic may be prior (a wave reads its word
 *                      before it writes it).  Outputs may be NULL, not all of them.
 *   cpx_chase_bch      the flat batch in host buffers: llr, prior, extrinsic [B][n], bits [B][k], codeword [B][n], metric, candidates [B].
 * Checked before any device call: the arguments (CPX_EINVAL), and the LDS one word needs beside the field tables -- 8.25 n bytes and
 * 2^p (2 (p + t) + 10) -- against 160 KiB (CPX_ELIMIT, the message names the byte count).  B = 0 returns CPX_OK without a launch. */
int cpx_chase_bch_dev(const cpx_bch *p, const double *d_llr, const double *d_prior, double alpha, double beta, int test_positions, int64_t B,
                      int64_t J, int64_t sb, int64_t sj, int64_t si, uint8_t *d_bits, uint8_t *d_codeword, double *d_extrinsic,
                      double *d_metric, int32_t *d_candidates, void *stream);
int cpx_chase_bch(const cpx_bch *p, const double *llr, const double *prior, double alpha, double beta, int test_positions, int64_t B,
                  uint8_t *bits, uint8_t *codeword, double *extrinsic, double *metric, int32_t *candidates);

/* ---- Reed-Solomon codes: systematic encoder and errors-and-erasures decoder (csrc/rs.hip) ---------------
 * Code of length n <= 2^m - 1 (shortened below that) over GF(2^m), 3 <= m <= 14, with r = n - k <= 63 parity symbols and the generator
 * g(x) = prod_{j<r} (x - alpha^(fcr+j)).  A word is n uint16 symbols in tuple form (bit i = coefficient of alpha^i), of which only the
 * low m bits count (the kernels mask them); symbol i is the coefficient of x^(n-1-i): k message symbols, then the r symbols of
 * x^r m(x) mod g(x).
 *   cpx_rs_create    prim_poly as for cpx_bch_create; genpoly [n - k + 1] field elements, lowest degree first.  Checked before a device
 *                    is looked for: m, n, n - k above 63 (CPX_ELIMIT); k, fcr in 0 .. 2^m - 2, prim_poly of degree m under which x
 *                    generates the multiplicative group, entries below 2^m, genpoly[n - k] = 1, g(alpha^(fcr+j)) = 0 for j < r
 *                    (CPX_EINVAL).
 *   cpx_rs_encode    msg [B][k] -> word [B][n].
 *   cpx_rs_decode    in [B][n]; erased [B][n] uint8, non-zero = the position is flagged (NULL: none).  With f flagged positions:
 *                    f > r fails.  S_j = R(alpha^(fcr+j)), j < r, from the symbols as given; all zero: accepted, 0 errors.  Else
 *                    Gamma = prod (1 - alpha^d x) over the flagged degrees d, and Berlekamp-Massey on rho = f .. r - 1 started with
 *                    C = B = Gamma, L = f (length change when 2 L <= rho + f, to rho + 1 - L + f) gives Lambda of length L.  Failure if
 *                    2 (L - f) + f > r, if Lambda_L = 0 or if Lambda has not exactly L roots among alpha^-d, d = 0 .. n - 1.  Otherwise
 *                    Omega = S Lambda mod x^r and Y = alpha^(d (1 - fcr)) Omega(alpha^-d) / Lambda'(alpha^-d) is XORed into the symbol
 *                    at every root.  Outputs, each may be NULL (not all): symbols [B][k], word [B][n], errors [B] int32 = L - f, the
 *                    corrected unflagged positions, -1 after a failure (symbols and word then hold the received word, masked to m
 *                    bits).  Equal to tests/rs_model.py symbol for symbol.
 * The _dev forms take device pointers and a stream and are asynchronous; the others take host pointers and return synchronised.
 * B = 0 returns CPX_OK without a launch. */
typedef struct cpx_rs cpx_rs;
int cpx_rs_create(int m, uint32_t prim_poly, int n, int k, int fcr, const uint16_t *genpoly, cpx_rs **out);
int cpx_rs_destroy(cpx_rs *p);
int cpx_rs_encode(const cpx_rs *p, const uint16_t *msg, int64_t B, uint16_t *word);
int cpx_rs_encode_dev(const cpx_rs *p, const uint16_t *d_msg, int64_t B, uint16_t *d_word, void *stream);
int cpx_rs_decode(const cpx_rs *p, const uint16_t *in, const uint8_t *erased, int64_t B, uint16_t *symbols, uint16_t *word,
                  int32_t *errors);
int cpx_rs_decode_dev(const cpx_rs *p, const uint16_t *d_in, const uint8_t *d_erased, int64_t B, uint16_t *d_symbols, uint16_t *d_word,
                      int32_t *d_errors, void *stream);

/* ---- tail-biting convolutional codes: encoder and wrap-around Viterbi decoder (csrc/tbcc.hip) ----------
 * A block is T trellis steps of the code of a cpx_trellis; it has no tail: the encoder starts in the state in which it ends.  Limits
 * (CPX_ELIMIT, naming the limit): the number of states is a power of two from 2 to 64; k <= 2 and n <= 6; T >= 1 and T k <= 8192 (the
 * block's decisions stay in LDS); 1 <= max_wraps <= 32.
 *   cpx_tbcc_encode  msg [B][T k] uint8 (bit 0 of a byte counts) -> word [B][T n] uint8: the encoder walks the message once from state
 *                    0, starts again in the state it ended in and emits that second walk.  closed [B] uint8 (may be NULL): 1 = the
 *                    second walk ended where it began (0: a recursive trellis, or a message shorter than the encoder memory).
 *   cpx_tbcc_decode  coded [B][T n] float64, read per decoding_type (CPX_VIT_*) as cpx_viterbi_decode_batch reads it, 'soft' clipped to
 *                    +-500.  float64, sums in the order written: bm_t[c] = the sum over the n bits, MSB first and starting from 0.0, of
 *                    the Viterbi decoder's per-bit metric for step t; M[s] = 0 for every state before the first trip.  On trip
 *                    w = 1 .. max_wraps: (1) M_start = M.  (2) Steps t = 0 .. T - 1: every state takes its candidates in np.where
 *                    order, cand_j = M[pred_j] + bm_t[code_j], and keeps the first minimum (a later candidate replaces it only if
 *                    strictly smaller); metrics run on across trips without rescaling.  (3) origin[s] = the state in which the survivor
 *                    ending in s began this trip, net[s] = M[s] - M_start[origin[s]].  (4) s* = the first state of minimum M; if
 *                    origin[s*] == s*: that path, wraps = w, tailbiting = 1, metric = net[s*].  (5) Otherwise c, the first state of
 *                    minimum net among the states with origin[s] == s, replaces the remembered candidate only if its net is strictly
 *                    smaller; a remembered candidate keeps its bits.  (6) After the last trip: the remembered candidate, wraps =
 *                    max_wraps, tailbiting = 1; none: the path of the last s*, tailbiting = 0, metric = net[s*].  A row that holds a
 *                    NaN, or +-inf under 'hard' / 'unquantized', is rejected and not decoded: zero bits, wraps = 0, tailbiting = 0,
 *                    metric = NaN; no other row is affected.  Outputs, each may be NULL (not all): bits [B][T k] uint8, wraps [B]
 *                    int32, tailbiting [B] uint8, metric [B] float64.  Equal to tests/tbcc_model.py bit for bit.
 * The _dev forms take device pointers and a stream and are asynchronous; the others take host pointers and return synchronised.
 * B = 0 returns CPX_OK without a launch. */
int cpx_tbcc_encode(const cpx_trellis *t, const uint8_t *msg, int64_t B, int64_t T, uint8_t *word, uint8_t *closed);
int cpx_tbcc_encode_dev(const cpx_trellis *t, const uint8_t *d_msg, int64_t B, int64_t T, uint8_t *d_word, uint8_t *d_closed, void *stream);
int cpx_tbcc_decode(const cpx_trellis *t, const double *coded, int64_t B, int64_t T, int decoding_type, int max_wraps, uint8_t *bits,
                    int32_t *wraps, uint8_t *tailbiting, double *metric);
int cpx_tbcc_decode_dev(const cpx_trellis *t, const double *d_coded, int64_t B, int64_t T, int decoding_type, int max_wraps, uint8_t *d_bits,
                        int32_t *d_wraps, uint8_t *d_tailbiting, double *d_metric, void *stream);

/* ---- layered normalised / offset min-sum LDPC decoding (csrc/ldpc_layered.hip) -----------------------
 * The code is the edge list of cpx_ldpc_create, sorted by (check, variable).  A schedule is an ordered list of layers; a layer is a list
 * of checks; every check appears exactly once and no two checks of one layer share a variable: layer l holds
 * layer_checks[layer_start[l] .. layer_start[l + 1]), layer_start[0] = 0, layer_start[n_layers] = n_c.
 * The rule (float64, operations in the order written, no fused multiply-add); LLRs are positive for bit 0:
 *   Start.       Q[v] = min(max(llr[v], -llr_clip), llr_clip) on a copy (the caller's array is not modified); R[e] = +0.0 for every edge.
 *   Iterations.  it = 1 .. n_iters; within an iteration the layers in order; for every check c of the layer, its edges j in stored order:
 *                  m_j  = Q[v_j] - R_cj
 *                  a_j  = min over i != j of |m_i|
 *                  g_j  = max(alpha * a_j - beta, 0.0)        two roundings: the product, then the difference
 *                  s_j  = XOR over i != j of signbit(m_i)     the sign BIT: -0.0 counts as negative
 *                  R_cj = s_j ? -g_j : g_j
 *                  Q[v_j] = m_j + R_cj
 *                No variable is touched twice within a layer, so the order of its checks cannot matter.
 *   Decision.    After the last layer of an iteration bit[v] = signbit(Q[v]).  With early_stop: if every check's parity of bits is even
 *                the block stops with iters = it, converged = 1; a block that never stops has iters = n_iters, converged = 0.  Without
 *                early_stop iters = n_iters and converged is the parity test on the final bits.
 *   Rejection.   A block with a NaN anywhere in its LLRs is rejected on its own: bits all zero, the llr output all NaN, iters = 0,
 *                converged = 0.  +-inf is no reason to reject: the clip maps it to +-llr_clip.
 * Equal to tests/ldpc_layered_model.py bit for bit, whatever the batch size, the block's place, the stream and the outputs requested.
 * Limits (CPX_ELIMIT, naming the limit, checked before a device is looked for): every check degree 2 .. 32; a schedule that is a
 * conflict-free partition of the checks; the state of one block in LDS, 8 n_v + 24 n_c bytes, at most 163 840 (there is no HBM path);
 * n_iters >= 1; alpha > 0, beta >= 0, llr_clip > 0, all finite.  CPX_EINVAL: null pointers, an edge out of range, an edge list that is
 * not sorted or repeats an edge, no output requested.
 *   cpx_ldpc_layered_decode  llr [B][n_v] float64, one block per row.  Outputs, each may be NULL (not all): bits [B][n_v] int8,
 *                            llr_out [B][n_v] float64 (the final Q), iters [B] int32, converged [B] uint8.
 * The _dev form takes device pointers and a stream and is asynchronous; the other takes host pointers and returns synchronised.
 * B = 0 returns CPX_OK without a launch.  cpx_last_kernel names the kernel, the blocks per workgroup, its LDS, the workgroups per compute
 * unit that the runtime's occupancy query reports and the blocks resident on the device. */
typedef struct cpx_ldpc_layered cpx_ldpc_layered;
int cpx_ldpc_layered_create(int n_v, int n_c, int64_t n_edges, const int32_t *edge_check, const int32_t *edge_var, int n_layers,
                            const int32_t *layer_start, const int32_t *layer_checks, cpx_ldpc_layered **out);
int cpx_ldpc_layered_destroy(cpx_ldpc_layered *c);
int cpx_ldpc_layered_decode(const cpx_ldpc_layered *c, const double *llr, int64_t B, int n_iters, double alpha, double beta, int early_stop,
                            double llr_clip, int8_t *bits, double *llr_out, int32_t *iters, uint8_t *converged);
int cpx_ldpc_layered_decode_dev(const cpx_ldpc_layered *c, const double *d_llr, int64_t B, int n_iters, double alpha, double beta,
                                int early_stop, double llr_clip, int8_t *d_bits, double *d_llr_out, int32_t *d_iters, uint8_t *d_converged,
                                void *stream);

/* ---- trellis equalisation of a known multipath channel: MLSE and max-log MAP (csrc/mlse.hip) ----------
 * A block of n symbols with labels a_0 .. a_{n-1} and values c[a] (the points of a cpx_modem, label = position) is sent in silence
 * through L taps: y_t = sum_l h_l c[a_{t-l}] + w_t, the terms with t - l < 0 or t - l >= n absent.  With tail != 0 a row holds
 * n + L - 1 samples (what cpx_multipath returns), else the first n.
 * The rule (float64, real and imaginary parts separate doubles, every product rounded before it is added, sums in the order written):
 *   State.      After step t: s' = a_t M^(L-2) + ... + a_{t-L+2}.  Candidates into s' in the order old = 0 .. M-1,
 *               pred = (s' mod M^(L-2)) M + old.
 *   Branch.     xh = sum_{l=0}^{L-1} h_l c[a_{t-l}], l ascending from 0.0, a product is (hr cr - hi ci, hr ci + hi cr), the terms with
 *               t - l < 0 skipped; e = y_t - xh; d = er er + ei ei.
 *   Prior.      P_t[a] = noise_var (sum of La over the bits 1 of a, MSB first, from 0.0); 0.0 without a prior.  LLRs are positive for bit 0.
 *   Forward.    alpha_0 = 0; alpha_{t+1}[s'] = (first minimum over old of alpha_t[pred] + d) + P_t[a_t]; a later candidate wins only if
 *               strictly smaller; the winning old is the decision.
 *   Tail.       beta_n[s] = sum_{j=0}^{L-2} |y_{n+j} - xh_j(s)|^2, j ascending from 0.0, xh_j(s) over l = j+1 .. L-1 (and n + j - l >= 0);
 *               beta_n = 0 with tail == 0.
 *   Hard.       s* = the first minimum of alpha_n + beta_n; that minimum is the metric; the indices from s* and the decisions.
 *   Soft.       beta_t[s] = min over a of (d_t(s, a) + (P_t[a] + beta_{t+1}[s'])); Lambda_t[s'] = alpha_{t+1}[s'] + beta_{t+1}[s'];
 *               llr[t m + i] = (min over the s' whose a_t has bit i = 1 of Lambda_t - the same with bit i = 0) / noise_var.
 *   Rejection.  A row whose y, h, prior or noise_var holds a NaN or +-inf, or whose noise_var is not positive, is rejected on its own:
 *               zero indices and bits, NaN metric and LLRs.
 * Equal to tests/mlse_model.py bit for bit, whatever the batch size, the row's place, the stream and the outputs requested.
 * Limits (CPX_EINVAL, naming the limit, checked before a device is looked for): L >= 2; M a power of two from 2 to 16;
 * M^(L-1) <= 256 states; 1 <= n <= 4096; noise_var given when llr or prior is.
 *   cpx_mlse  y [B][n_y][2] float64 (re, im); h [L][2] or, with h_batched, [B][L][2]; noise_var NULL, one value or, with nv_batched,
 *             [B]; prior NULL or [B][n m].  Outputs, each may be NULL (not all): indices [B][n] int32, bits [B][n m] uint8 (MSB
 *             first), metric [B] float64, llr [B][n m] float64 (posterior; extrinsic = llr - prior).
 * The _dev form takes device pointers (noise_var included) and a stream and is asynchronous; the other takes host pointers and returns
 * synchronised.  B = 0 returns CPX_OK without a launch.  cpx_last_kernel names the kernel's (M, S) class, the rows per workgroup, the
 * grid's cap and where the decisions are kept. */
int cpx_mlse(const cpx_modem *md, const double *y, const double *h, int h_batched, int64_t B, int64_t n, int L, int tail,
             const double *noise_var, int nv_batched, const double *prior, int32_t *indices, uint8_t *bits, double *metric, double *llr);
int cpx_mlse_dev(const cpx_modem *md, const double *d_y, const double *d_h, int h_batched, int64_t B, int64_t n, int L, int tail,
                 const double *d_noise_var, int nv_batched, const double *d_prior, int32_t *d_indices, uint8_t *d_bits, double *d_metric,
                 double *d_llr, void *stream);

/* ---- MMSE linear and decision-feedback equalisation of a known multipath channel (csrc/equalize.hip) ----------
 * y_t = sum_l h_l x_{t-l} + w_t, x_t = c[a_t] for 0 <= t < n and 0 elsewhere (the points of a cpx_modem, label = position); es is the
 * mean symbol energy, N0 = noise_var, d = delay, nf feed-forward taps, nb feedback taps (0: the linear equaliser).  With tail != 0 a
 * row holds n + L - 1 samples (what cpx_multipath returns), else the first n.
 * The rule (float64, real and imaginary parts separate doubles, every product rounded before it is added, every sum from 0.0 in
 * ascending index order; a b = (ar br - ai bi, ar bi + ai br), a conj(b) = (ar br + ai bi, ai br - ar bi)):
 *   Design.     H[i][k] = h_{k-i} for 0 <= k-i < L (i < nf); K = all columns but d+1 .. d+nb.  For j <= i:
 *               S[i][j] = sum over k in K, i <= k < j+L, of h_{k-i} conj(h_{k-j}); R[i][j] = es S[i][j], and + N0 on the diagonal,
 *               whose imaginary part is never computed.  p_i = es h_{d-i} (0 outside the taps).
 *   L D L^H.    Column j: g_k = (D_k Lr[j][k], -(D_k Li[j][k])) for k < j; v_i = R[i][j] - sum_{k<j} L[i][k] g_k for i >= j;
 *               D_j = Re v_j; L[i][j] = (vr / D_j, vi / D_j) for i > j.  No square root.
 *   Solve.      a_i = p_i - sum_{k<i} L[i][k] a_k; b_i = (ar / D_i, ai / D_i); u_i = b_i - sum_{k>i} u_k conj(L[k][i]), i descending,
 *               every sum over k ascending.
 *   Taps.       ff_i = conj(u_i); fb_j = sum_i ff_i h_{d+j-i} over the i with 0 <= d+j-i < L, j = 1 .. nb;
 *               gain = sum_i (ffr hr - ffi hi) of h_{d-i} over the i with 0 <= d-i < L; nu = (es (1 - gain)) / gain.
 *   Equalise.   z_t = sum_{i<nf} ff_i y_{t+d-i} - sum_{j=1..nb, t-j>=0} fb_j c[a^_{t-j}], the two sums formed separately, a sample
 *               outside the row read as 0.0 and multiplied like any other; x^_t = (zr / gain, zi / gain); a^_t = the first minimum
 *               over a ascending of e = x^_t - c[a], er er + ei ei, a later point winning only if strictly smaller.
 *   Soft.       llr[t m + i] = (min over the a with bit i = 1 - min over the a with bit i = 0 of that distance) / nu, bits MSB first,
 *               positive = bit 0; each minimum from +inf over a ascending, replaced only by a strictly smaller value.  With
 *               feedback this takes the past decisions for correct.
 *   Rejection.  A row whose y, h or noise_var holds a NaN or +-inf (or a noise_var <= 0), one of whose pivots D_j is not positive
 *               and finite, or whose gain is not a finite number in (0, 1) -- an all-zero h gives gain 0 -- is rejected on its own:
 *               zero indices and bits, NaN everything else.
 * Equal to tests/equalize_model.py bit for bit, whatever the batch size, the row's place, the stream, the outputs requested and
 * whether h is shared or repeated per row.
 * Limits (CPX_EINVAL, naming the limit, checked before a device is looked for): 1 <= L <= 64; 1 <= nf <= 64; 0 <= nb <= 64;
 * 0 <= delay; delay + nb <= nf + L - 2; 2 <= M <= 256; M a power of two when bits or llr is asked for; 1 <= n <= 2^30; noise_var
 * given; es positive and finite.
 *   cpx_mmse_equalize  y [B][n_y][2] float64 (re, im); h [L][2] or, with h_batched, [B][L][2]; noise_var one value or, with
 *             nv_batched, [B].  Outputs, each may be NULL (not all): indices [B][n] int32, bits [B][n m] uint8 (MSB first),
 *             estimate [B][n][2] (the unbiased x^), llr [B][n m], noise [B] (nu), ff [B][nf][2], fb [B][nb][2], gain [B].
 * The _dev form takes device pointers (noise_var included) and a stream and is asynchronous; the other takes host pointers and returns
 * synchronised.  B = 0 returns CPX_OK without a launch.  cpx_last_kernel names the last kernel of the call (eq_filter_kernel<LGM> for
 * nb = 0, eq_dfe_kernel<LGM> with feedback, eq_design_kernel when only the design is asked for; LGM = m with llr, else 0), nf, nb,
 * the number of designs solved and the grid caps of the three kernels.  With feedback the call takes 16 B n bytes of workspace. */
int cpx_mmse_equalize(const cpx_modem *md, double es, const double *y, const double *h, int h_batched, int64_t B, int64_t n, int L,
                      int tail, const double *noise_var, int nv_batched, int nf, int nb, int delay, int32_t *indices, uint8_t *bits,
                      double *estimate, double *llr, double *noise, double *ff, double *fb, double *gain);
int cpx_mmse_equalize_dev(const cpx_modem *md, double es, const double *d_y, const double *d_h, int h_batched, int64_t B, int64_t n,
                          int L, int tail, const double *d_noise_var, int nv_batched, int nf, int nb, int delay, int32_t *d_indices,
                          uint8_t *d_bits, double *d_estimate, double *d_llr, double *d_noise, double *d_ff, double *d_fb,
                          double *d_gain, void *stream);

/* ---- adaptive linear and decision-feedback equalisation: LMS, normalised LMS, RLS (csrc/adaptive.hip) ----------
 * The equaliser learns its taps from the known first nt symbols of a row (training labels) and then tracks on its own decisions.
 * y holds sps samples per symbol; the nf feed-forward taps are one sample apart (T/sps spacing), the nb feedback taps one symbol apart
 * (0: the linear equaliser); d = delay in samples, N = nf + nb, c the points of a cpx_modem (label = position), theta = (ff, fb).
 * algorithm: 0 = LMS, 1 = normalised LMS (both take step = mu, nlms also eps), 2 = RLS (takes forgetting = lambda and delta).
 * The rule (float64, real and imaginary parts separate doubles, every product rounded before it is added, every sum from 0.0 in
 * ascending index order; a b = (ar br - ai bi, ar bi + ai br), a conj(b) = (ar br + ai bi, ai br - ar bi)), for t = 0 .. n-1:
 *   Regressor.  x[i] = y[t sps + d - i] for i < nf, a sample outside the row read as 0.0 and multiplied like any other;
 *               x[nf + j - 1] = -r_{t-j} (each part negated) for j = 1 .. nb, and 0.0 where t - j < 0, multiplied like any other.
 *   Output.     z_t = (sum_{k<nf} theta_k x_k) + (sum_{nf<=k<N} theta_k x_k), no conjugate, the two sums formed separately.
 *   Decision.   a^_t = the first minimum over a ascending of e = z_t - c[a], er er + ei ei, a later point winning only if strictly
 *               smaller.  It is indices[t] at every t, training included.
 *   Reference.  r_t = c[training[t]] for t < nt, else c[a^_t]; e_t = r_t - z_t (the a-priori error).
 *   LMS.        w = (mu er, mu ei); theta_k <- theta_k + w conj(x_k).
 *   NLMS.       The same with mu_t = mu / (eps + sum_{k<N} (xr xr + xi xi)) in place of mu.
 *   RLS.        P = I / delta = (1.0 / delta) on the diagonal before the first step of every call.  g_i = sum_{j<N} P[i][j] conj(x_j);
 *               den = lambda + sum_{k<N} (xr gr - xi gi); kappa_i = (gr_i / den, gi_i / den); theta_i <- theta_i + kappa_i e_t;
 *               P[i][j] <- ((Pr - qr) / lambda, (Pi - qi) / lambda) with q = kappa_i conj(g_j).
 *   Rejection.  A row whose y (all n_y samples), ff0, fb0, step, forgetting, delta or eps holds a NaN or +-inf or lies outside its
 *               range, one of whose training labels is negative or >= M, one of whose z_t is not finite (a diverged LMS), or one of
 *               whose den is not positive and finite is rejected on its own: zero indices and bits, NaN everything else.
 * Equal to tests/adaptive_model.py bit for bit, whatever the batch size, the row's place, the stream and the outputs requested.
 * Limits (CPX_EINVAL, naming the limit, checked before a device is looked for): algorithm 0 .. 2; 1 <= nf <= 64; 0 <= nb <= 64;
 * nf + nb <= 32 with RLS; 0 <= delay; 1 <= sps <= 8; 2 <= M <= 256; M a power of two when bits is asked for; 1 <= n <= 2^30;
 * 0 <= n_y <= 2^33; 0 <= nt <= n; step given for LMS and NLMS and NULL for RLS; forgetting and delta given for RLS (ignored
 * otherwise); eps >= 0; and, where the values are host values, step > 0, 0 < forgetting <= 1, delta > 0 (a NaN passes and rejects
 * its row; the _dev form leaves these three to the kernels, which reject the rows).
 *   cpx_adaptive_equalize  y [B][n_y][2] float64 (re, im); training [nt] int32 or, with tr_batched, [B][nt]; step, forgetting, delta
 *             one value each or, with their _batched flag, [B]; ff0 [nf][2] or [B][nf][2], fb0 [nb][2] or [B][nb][2], the initial
 *             taps, NULL = zeros.  Outputs, each may be NULL (not all): indices [B][n] int32, bits [B][n m] uint8 (MSB first),
 *             estimate [B][n][2] (z), error [B][n][2] (e), ff [B][nf][2], fb [B][nb][2], the taps after the last symbol.
 * The _dev form takes device pointers and a stream and is asynchronous; the other takes host pointers and returns synchronised.
 * B = 0 returns CPX_OK without a launch.  cpx_last_kernel names the kernel (ad_lms_kernel for LMS and NLMS, ad_rls_kernel), nf, nb,
 * the rows per wave and the grid cap (lms_cap / rls_cap, in workgroups).  No workspace is taken. */
int cpx_adaptive_equalize(const cpx_modem *md, const double *y, int64_t B, int64_t n_y, int64_t n, int sps, const int32_t *training,
                          int tr_batched, int64_t nt, int nf, int nb, int delay, int algorithm, const double *step, int step_batched,
                          const double *forgetting, int fg_batched, const double *delta, int dl_batched, double eps, const double *ff0,
                          int ff0_batched, const double *fb0, int fb0_batched, int32_t *indices, uint8_t *bits, double *estimate,
                          double *error, double *ff, double *fb);
int cpx_adaptive_equalize_dev(const cpx_modem *md, const double *d_y, int64_t B, int64_t n_y, int64_t n, int sps,
                              const int32_t *d_training, int tr_batched, int64_t nt, int nf, int nb, int delay, int algorithm,
                              const double *d_step, int step_batched, const double *d_forgetting, int fg_batched, const double *d_delta,
                              int dl_batched, double eps, const double *d_ff0, int ff0_batched, const double *d_fb0, int fb0_batched,
                              int32_t *d_indices, uint8_t *d_bits, double *d_estimate, double *d_error, double *d_ff, double *d_fb,
                              void *stream);

/* ---- symbol-timing and carrier recovery of a single-carrier burst (csrc/recovery.hip) ---------------------------
 * The interpolator / timing-error detector / loop filter / controller loop on rows of matched-filter output at nominally sps samples
 * per symbol, with an optional decision-directed carrier PLL on the strobes; one row = one independent loop.  md may be NULL for the
 * Gardner detector without carrier loop, training, indices and bits; c = the points of md (label = position).
 * ted: 0 = Gardner (non-data-aided), 1 = Mueller-Mueller (decision-directed).  interp: 0 = linear, 1 = cubic (4-sample Lagrange, Farrow).
 * The rule (float64, real and imaginary parts separate doubles, every product rounded before it is added, no fused multiply-add; a
 * sample index outside [0, n_y) reads 0.0 and is used like any other).  State of a row: the position m (int64) and mu, from m0 and mu0;
 * v = 0.0; the period w = (double)sps; phi = phase0 and f = 0.0; the previous strobe and reference.  For k = 0 .. n-1:
 *   Interpolate.  z_k = I(m, mu), each part on its own.  Linear: x0 + mu (x1 - x0), x0 = y[m], x1 = y[m+1].  Cubic, with xm = y[m-1],
 *                 x0 = y[m], x1 = y[m+1], x2 = y[m+2], S = 0.16666666666666666: v3 = ((x2 - xm) + 3.0 (x0 - x1)) S;
 *                 v2 = ((x1 + xm) 0.5) - x0; v1 = ((6.0 x1 - x2) - (3.0 x0 + 2.0 xm)) S; I = ((v3 mu + v2) mu + v1) mu + x0.
 *   Derotate.     With the carrier loop (c, s) = unit_phasor(phi) (csrc/cpx_phasor.h: a fixed float64 polynomial, no sincos) and
 *                 z'_k = (zr c + zi s, zi c - zr s); without it z' = z.
 *   Decide.       With md, a^_k = the first minimum over a ascending of e = z'_k - c[a], er er + ei ei, a later point winning only if
 *                 strictly smaller; r_k = c[training[k]] for k < nt, else c[a^_k].
 *   Timing error. e_0 = 0.0, no midpoint is read at k = 0.  Gardner: t = mu - 0.5 w, fl = floor(t), zm = I(m + fl, t - fl),
 *                 e_k = (zr_{k-1} - zr_k) zmr + (zi_{k-1} - zi_k) zmi on the unrotated strobes.
 *                 Mueller-Mueller: e_k = (rr_{k-1} z'r_k + ri_{k-1} z'i_k) - (rr_k z'r_{k-1} + ri_k z'i_{k-1}).
 *   Carrier.      ep = z'i_k rr_k - z'r_k ri_k; f <- f + kc2 ep; phi <- phi + (f + kc1 ep); phi <- phi - rint(phi); the row is rejected
 *                 unless |phi| <= 0.5 (a NaN fails).
 *   Loop filter.  v <- v + k2 e_k; w = sps + (v + k1 e_k); the row is rejected unless 0.5 sps < w < 1.5 sps.
 *   Controller.   t = mu + w, fl = floor(t), m <- m + fl, mu <- t - fl.
 *   Rejection.    A row whose y (all n_y samples), k1, k2, kc1, kc2, mu0 or phase0 holds a NaN or +-inf or lies outside its range, whose
 *                 m0 is outside [0, n_y), one of whose training labels is negative or >= M, or one of whose w or phi fails its test is
 *                 rejected on its own: zero integers, NaN floats.
 * Equal to tests/recovery_model.py bit for bit, whatever the batch size, the row's place, the stream and the outputs requested.
 * Limits (CPX_EINVAL, naming the limit, checked before a device is looked for): ted and interp 0 or 1; 2 <= sps <= 8; 1 <= n <= 2^30;
 * 1 <= n_y <= 2^33; k1, k2, m0, mu0, phase0 given; kc1 and kc2 both given (the carrier loop) or both NULL; md given for ted = 1, the
 * carrier loop, nt > 0, indices and bits; 2 <= M <= 256; M a power of two when bits is asked for; phase only with the carrier loop;
 * 0 <= nt <= n; and, where the values are host values, k1, k2, kc1, kc2 >= 0, 0 <= mu0 < 1, |phase0| <= 0.5, 0 <= m0 < n_y (a NaN passes
 * and rejects its row; the _dev form leaves these to the kernel, which rejects the rows).
 *   cpx_timing_recover  y [B][n_y][2] float64 (re, im); k1, k2, kc1, kc2, mu0, phase0 (float64) and m0 (int64): one value each or, with
 *             their _batched flag, [B]; training [nt] int32 or, with tr_batched, [B][nt].  Outputs, each may be NULL (not all):
 *             symbols [B][n][2] (z'), indices [B][n] int32, bits [B][n m] uint8 (MSB first), position [B][n] ((double)m + mu at the
 *             strobe), error [B][n] (e_k), phase [B][n] (phi after the strobe's update, turns), count [B] int32 (the strobes all of
 *             whose interpolator reads lay inside the row).
 * The _dev form takes device pointers and a stream and is asynchronous; the other takes host pointers and returns synchronised.
 * B = 0 returns CPX_OK without a launch.  cpx_last_kernel names tr_loop_kernel, the detector, the interpolator, carrier=0/1, sps, M and
 * the grid cap (tr_cap, in workgroups).  No workspace is taken. */
int cpx_timing_recover(const cpx_modem *md, const double *y, int64_t B, int64_t n_y, int64_t n, int sps, int ted, int interp,
                       const double *k1, int k1_batched, const double *k2, int k2_batched, const double *kc1, int kc1_batched,
                       const double *kc2, int kc2_batched, const int32_t *training, int tr_batched, int64_t nt, const int64_t *m0,
                       int m0_batched, const double *mu0, int mu0_batched, const double *phase0, int phase0_batched, double *symbols,
                       int32_t *indices, uint8_t *bits, double *position, double *error, double *phase, int32_t *count);
int cpx_timing_recover_dev(const cpx_modem *md, const double *d_y, int64_t B, int64_t n_y, int64_t n, int sps, int ted, int interp,
                           const double *d_k1, int k1_batched, const double *d_k2, int k2_batched, const double *d_kc1, int kc1_batched,
                           const double *d_kc2, int kc2_batched, const int32_t *d_training, int tr_batched, int64_t nt, const int64_t *d_m0,
                           int m0_batched, const double *d_mu0, int mu0_batched, const double *d_phase0, int phase0_batched,
                           double *d_symbols, int32_t *d_indices, uint8_t *d_bits, double *d_position, double *d_error, double *d_phase,
                           int32_t *d_count, void *stream);

/* ---- multi-GPU: RCCL collectives of the sharded decode ------------------------------------
 * The path shards by codeword (contiguous blocks of B/G codewords per GPU, tables replicated) and has no exchange
 * step inside a decoder.  Two collectives exist around it:
 *   all-gather of decoded bits (uint8)   -- every GPU ends with the whole [B][L] result, the array the reference
 *                                           returns from viterbi_decode / ldpc_bp_decode (convcode.py:749, ldpc.py:251-254)
 *   all-reduce (sum / max) of int64 / float64 counters -- the error and bit counters of a Monte-Carlo sweep,
 *                                           commpy/links.py:252-260
 * A communicator is formed either by ONE process for several devices (cpx_comm_init_all = ncclCommInitAll; every
 * collective then takes one buffer per local device, in the order of `devices`, issued inside one ncclGroup) or by one
 * process per GPU (cpx_comm_unique_id on rank 0, the 128-byte id handed to the others by the launcher plumbing,
 * cpx_comm_init_rank on every rank with its device current).  librccl.so.1 is dlopen()ed at the first communicator.
 * d_send / d_recv / streams are arrays of nlocal pointers (nlocal = 1 for init_rank); streams == NULL or a NULL entry =
 * the library's stream of that device.  All calls are asynchronous on those streams.
 *   cpx_comm_allgather_u8: d_recv[i] holds nranks * bytes_per_rank bytes, rank r's block at r * bytes_per_rank
 *                          (ragged shards: the caller pads to the largest shard, commpy_amd/parallel.py)
 *   op: 0 = sum, 1 = max */
typedef struct cpx_comm cpx_comm;
int cpx_comm_unique_id(void *id128);
int cpx_comm_init_rank(const void *id128, int nranks, int rank, cpx_comm **out);
int cpx_comm_init_all(const int *devices, int ndev, cpx_comm **out);
int cpx_comm_info(const cpx_comm *c, int *nranks, int *nlocal, int *first_rank);
int cpx_comm_destroy(cpx_comm *c);
int cpx_comm_allgather_u8(cpx_comm *c, const void *const *d_send, void *const *d_recv, size_t bytes_per_rank,
                          void *const *streams);
int cpx_comm_allreduce_i64(cpx_comm *c, const void *const *d_send, void *const *d_recv, size_t count, int op,
                           void *const *streams);
int cpx_comm_allreduce_f64(cpx_comm *c, const void *const *d_send, void *const *d_recv, size_t count, int op,
                           void *const *streams);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* COMMPY_AMD_H */
