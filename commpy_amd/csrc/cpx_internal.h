// Internal helpers shared by the HIP translation units of libcommpy_amd.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "commpy_amd.h"

namespace cpx {

void set_error(const char *fmt, ...);
hipStream_t lib_stream();   // lazily created per-process stream of the current device
// name of the (dominant) kernel the last decoder call of this thread launched -- read back by cpx_last_kernel(), so
// that benchmarks and tests report what really ran instead of re-deriving the dispatch rules
void note_kernel(const char *fmt, ...);
const char *last_kernel_name();
// redo counter of "detect and redo" paths: `dev` = two device words {count, workgroups done}, zero between launches; `host` = a pinned
// host word.  The redo kernel adds its flagged items to dev[0] and calls redo_finish() at its end: the last workgroup publishes the
// count to *host and zeroes the device words.  note_redo() AFTER the final note_kernel() makes cpx_last_kernel append
// "redo: <host word> of <total> <what>" (pointers null: no counter available)
struct RedoCounter { unsigned *dev, *host; };
class Scratch;
RedoCounter redo_counter(Scratch &sc, hipStream_t st);
#ifdef __HIPCC__
// collective over the workgroup (one __syncthreads); `mine` = this workgroup's contribution, added by thread 0
__device__ __forceinline__ void redo_finish(RedoCounter rc, unsigned mine) {
    __syncthreads();
    if (threadIdx.x == 0 && rc.dev) {
        if (mine) atomicAdd(&rc.dev[0], mine);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        const unsigned prev = atomicAdd(&rc.dev[1], 1u);
        if (prev == gridDim.x - 1) {                              // the last workgroup of the launch
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            const unsigned total = atomicExch(&rc.dev[0], 0u);
            atomicExch(&rc.dev[1], 0u);
            __hip_atomic_store(rc.host, total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
}
#endif
void note_redo(long long total, const char *what);
// CPX_EINVAL unless the current device is the one the handle's tables were created on
int check_handle_device(int handle_device, const char *what);
int ensure_device();        // CPX_OK if a HIP device is usable
int device_cus();           // compute units of the current device (256 on MI355X)
// workgroups of `fn` (block size `threads`, no dynamic LDS) resident on the whole device at once -- the size of a
// persistent grid; cached per kernel
int resident_blocks(const void *fn, int threads);
#define CPX_HIP(call)                                                                          \
    do {                                                                                       \
        hipError_t _e = (call);                                                                \
        if (_e != hipSuccess) {                                                                \
            cpx::set_error("%s failed: %s (%s:%d)", #call, hipGetErrorString(_e), __FILE__, __LINE__); \
            return CPX_EHIP;                                                                   \
        }                                                                                      \
    } while (0)

#define CPX_REQUIRE(cond, code, ...)            \
    do {                                        \
        if (!(cond)) {                          \
            cpx::set_error(__VA_ARGS__);        \
            return (code);                      \
        }                                       \
    } while (0)

// What the Viterbi dispatch needs to know about a trellis: worked out once, by cpx_trellis_create (viterbi.hip)
struct TrellisClass {
    int lgS = 0;                     // S = 1 << lgS
    // feed-forward, k = 1: predecessor j of state s is ((s << 1) & (S - 1)) | j, its input s >> (lgS - 1) => arithmetic traceback
    bool shift_register = false;
    // ... of rate 1/2 and 4 .. 64 states, AND a linear code: g0, g1 = its generators in the kernel template's convention (bit lgS taps
    // the input, viterbi_cw.hip SrCode); what the compiled-in pairs and the per-pair code objects are keyed by
    bool linear_half = false;
    unsigned g0 = 0, g1 = 0;
    // ... of rate 1/2 and 4 .. 64 states whose butterflies have the form (c, c ^ 3, c ^ 3, c) -- both generators tap the input and the
    // oldest register bit: the table-driven fused kernel (cw_step, G0 = G1 = 0).  goff: field j = 2 c_j of butterfly j
    bool end_tap = false;
    unsigned goff[4] = {0u, 0u, 0u, 0u};
};

// The codeword-per-lane path runs in rounds of one wavefront of 64 codewords per SIMD (65536 codewords on 256 CUs), each as long as a
// full one; the state-per-lane kernels' time is proportional to the batch.  A round filled below 45 % is cheaper on the latter (config
// 2: 54 us per 1000 codewords against 1.55 ms per round, break-even at 0.44 of a round -- scripts/micro/split_probe.py: 30 000
// codewords 1.63 ms on the wave kernels, 1.53 ms as a round; 99 536: 3.59 ms as round + wave kernels, 3.01 as two rounds)
inline int64_t viterbi_round() { return (int64_t)device_cus() * 4 * 64; }
inline bool viterbi_round_pays(int64_t codewords, int64_t round) { return 20 * codewords >= 9 * round; }

// codeword-per-lane Viterbi path (viterbi_cw.hip): what it launched, if anything
enum class CwFlavour { none, mirrored, deep, lean, small, code_object, table, two_kernels };
struct CwResult {
    bool handled = false;            // false: the caller uses the state-per-lane kernels
    int rc = CPX_OK;                 // handled: the call's status
    CwFlavour flavour = CwFlavour::none;
};
// any_batch_size: take this path whatever the batch size (a chunk of the host-buffer pipeline: its round costs the same however full
// it is and hides behind the next chunk's upload; the fused kernel -- and with it the precision mode -- then serves the host API exactly
// as it serves the device API).  lean_ring: the 64-state built-in pairs take the ring stored once where that flavour exists ('soft',
// default depth, float64): the caller runs a remainder beside the round(s).
// nanflags ('soft' only, else null): [B] bytes, set to 1 for every codeword that received a NaN (viterbi.hip re-decodes those)
CwResult viterbi_codeword_path(const ::cpx_trellis *t, const double *d_coded, int64_t B, int64_t len, int64_t L, int64_t T, int tb,
                               int type, uint8_t *d_bits, uint8_t *nanflags, Scratch &sc, hipStream_t st, bool any_batch_size, bool lean_ring);

// LDS-resident LDPC path (ldpc_resident.hip): true when it handled the call (*rc = status)
int ldpc_resident_tables(::cpx_ldpc *c, const int32_t *row_ptr, const int32_t *row_pad, const int32_t *col_ptr,
                         const int32_t *col_pad_cj);
void ldpc_resident_free(::cpx_ldpc *c);
// nanflags (min-sum only, else null): [B] bytes, written for every block: 1 = a NaN among its LLRs (ldpc.hip decodes it again)
// block_major: d_dec / d_out are [B][n_v] (one block per row) instead of [n_v][B]
bool ldpc_resident_path(const ::cpx_ldpc *c, double *d_llr, int64_t B, int alg, int n_iters, int8_t *d_dec, double *d_out,
                        int block_major, int32_t *d_iters, int *d_clipped, uint8_t *nanflags, Scratch &sc, hipStream_t st, int *rc);

// absolute-scale BCJR / turbo decoder for trellises above 16 states (bcjr_exact.hip; CPX_EINVAL for any other): every codeword of the
// batch, one per lane
int bcjr_exact_map(const ::cpx_trellis *t, const double *sys, const double *par, const double *Lin, int64_t B, int64_t N, double nv2,
                   int want_bits, double *Lout, uint8_t *bits, Scratch &sc, hipStream_t st);
int bcjr_exact_turbo(const ::cpx_trellis *t, const double *sys, const double *p1, const double *p2, const double *Lint_or_null,
                     const int32_t *perm, int64_t B, int64_t N, double nv2, int n_iter, uint8_t *bits, Scratch &sc, hipStream_t st);

// Scratch arena keyed by (device, stream, slot): grown with hipMalloc on demand, reused by later calls and released by
// cpx_release_workspace / cpx_stream_destroy.  Kernels of one stream serialise, so one arena per stream is safe ACROSS calls; within
// one call two live buffers must not share a slot (the second request returns the same block, or frees it when it grows).
// (Stream-ordered hipMallocAsync/hipFreeAsync was measured to hand out memory that is still in use on this
//  stack -- 45/120 corrupted LDPC decodes -- so the engine never uses it.)
// One enumerator per slot: who takes it and what it holds; for a slot with several users, why no two of them are live in one call.
enum class Slot : int {
    // ldpc.hip tiled slab (R, Q, L, tables) | ldpc_resident.hip staging + queue + e0 | bcjr.hip map checkpoint rows | bcjr.hip turbo
    // checkpoint rows | viterbi_cw.hip two-kernel decisions.  One per call: the three decoders are separate entry points; the LDPC slab is
    // taken only once ldpc_resident_path has declined (returned false, before its own request); map and turbo are separate entry points
    state,
    // bcjr.hip turbo time-major slab (larr) | viterbi_cw.hip two-kernel best states: separate entry points
    state2,
    ldpc_pack,           // encoders.hip: packed message words of the LDPC encoder
    // NaN / "detect and redo" flag bytes, one per codeword or work item: bcjr.hip map | bcjr.hip turbo | viterbi.hip 'soft'
    // (viterbi_dispatch, read by the codeword path and launch_redo): separate entry points, each takes it once per call
    redo_flags,
    ldpc_nan_flags,      // ldpc.hip: min-sum NaN flag bytes, one per block (live together with exact_redo, hence a slot of its own)
    // per-lane / per-workgroup float64 state of the literal kernels: ldpc.hip ldpc_exact_kernel (general path or min-sum redo: the general
    // path returns before the redo exists) | bcjr_exact.hip map | bcjr_exact.hip turbo (the only decoder of trellises above 16
    // states, not a redo: the entry point returns right behind it, before any other request): one launch per call
    exact_redo,
    vit_host_in,         // viterbi.hip cpx_viterbi_decode_batch_i64: device copy of the host input (library stream, see there)
    vit_host_out,        // ... and of the decoded bits
    vit_gen_ring,        // viterbi_generic.hip: decision ring, per workgroup
    vit_gen_best,        // viterbi_generic.hip: best state per ring step, per workgroup
    vit_gen_pm,          // viterbi_generic.hip: path metrics of trellises above 2048 states
    turbo_tables,        // bcjr.hip turbo: inverse-permutation and identity row tables
    redo_counter,        // runtime.hip redo_counter: the stream's two counter words, zeroed when the block is created
    kbest_state,         // mimo.hip K-best: per-workgroup detector state that does not fit LDS
    best_first_state,    // mimo.hip best-first: per-workgroup stacks that do not fit LDS
    mimo_channel_state,  // mimo_channel.hip: per-wave scratch above 64 KB
    ofdm_ls,             // ofdm_chan.hip: least-squares estimates at the pilots
    ofdm_hsc,            // ofdm_chan.hip: the channel at every subcarrier, where the caller does not ask for it
    ofdm_lsp,            // ofdm_chan.hip cpx_pilots_estimate_tv_dev: least-squares estimates per pilot (no averaging over symbols)
    ofdm_hp,             // ofdm_chan.hip cpx_pilots_estimate_tv_dev: the channel at every subcarrier of every pilot symbol
    sync_totals,         // sync.hip windows_setup: per-tile totals of the window sums
    sync_parts,          // sync.hip cpx_sync_estimate_dev: per-tile partial results of the peak search
    fading_taps,         // fading.hip launch_taps: the power-delay profile's taps
    fading_gains,        // fading.hip cpx_fading_channel_dev: a chunk of tap gains, where the caller does not ask for them
    mlse_dec,            // mlse.hip: per-workgroup decision words of blocks too long for LDS
    mlse_alpha,          // mlse.hip: per-workgroup forward metrics of every step, soft output only (live together with mlse_dec)
    eq_design,           // equalize.hip: rejection flags, and the taps, gain and noise of every design that the caller does not ask for
    eq_sums,             // equalize.hip: feed-forward sums of a chunk of rows, feedback equaliser only (live together with eq_design)
    count
};

// The device's issue lock for the lifetime of the object, and the only way to arena memory.  Host threads may call into the library
// concurrently (ctypes drops the GIL).  Between get() handing out a block and the launches that use it, another thread growing the same
// (device, stream, slot) would free it (the grow path synchronises the stream first -- which only protects work that has already been
// issued).  An entry point therefore declares a Scratch before its first request and keeps it until its launches are queued; internal
// functions that take arena memory receive the caller's by reference.  The lock is recursive per device (host-buffer entry points call
// the device ones); the constructor touches no stream.
class Scratch {
public:
    Scratch();
    ~Scratch();
    Scratch(const Scratch &) = delete;  Scratch &operator=(const Scratch &) = delete;
    // *out = at least `bytes` bytes of `slot` on `st` (a zero-byte request still gets 8); fresh: the block was (re)allocated by this call
    template <class T> int get(hipStream_t st, Slot slot, size_t bytes, T **out, bool *fresh = nullptr) {
        void *p = nullptr;
        const int rc = block(st, slot, bytes, &p, fresh);
        *out = static_cast<T *>(p);
        return rc;
    }
private:
    static int block(hipStream_t st, Slot slot, size_t bytes, void **out, bool *fresh);   // runtime.hip
    int dev_;
};

// blocking download into pageable host memory through pinned staging + host threads (runtime.hip)
int d2h_pageable(void *dst, const void *d_src, size_t bytes, hipStream_t st);
void issue_lock(int dev, bool lock);     // cpx_release_workspace takes all of them

// roctx range for the lifetime of the object when CPX_TRACE=1 (runtime.hip); a no-op otherwise
struct TraceRange {
    explicit TraceRange(const char *name);
    ~TraceRange();
    TraceRange(const TraceRange &) = delete;
    TraceRange &operator=(const TraceRange &) = delete;
    bool on;
};
bool trace_enabled();
#define CPX_TRACE_CAT2(a, b) a##b
#define CPX_TRACE_CAT(a, b) CPX_TRACE_CAT2(a, b)
#define CPX_TRACE(name) cpx::TraceRange CPX_TRACE_CAT(cpx_trace_, __LINE__)(name)

// Kernel-path switches: one process-wide table in runtime.hip holds, per switch, its environment variable, its public setter
// and the mode names it accepts.
enum class Switch { precision, viterbi_path, ldpc_path, demod, kbest_path, best_first_path, ldpc_spa, viterbi_overlap, count };
int mode_of(Switch s);                      // the current mode: one relaxed atomic load once the environment has been read
int set_mode(Switch s, const char *name);   // null, "" and the default's names reset; CPX_EINVAL for a name not in the switch's row

// cpx_set_precision / CPX_PRECISION: false = fp64-parity (default), true = fp32-fast
inline bool precision_fast() { return mode_of(Switch::precision) == 1; }
// cpx_ldpc_set_path / CPX_LDPC_PATH: 0 auto, 1 'tiled', 2 'resident', 3 'resident-log' (forced modes never substitute another kernel)
inline int ldpc_forced_path() { return mode_of(Switch::ldpc_path); }
// CPX_LDPC_SPA=exact: sum-product check rows always by the exact-order sequence (ldpc_dev.h)
inline bool ldpc_spa_exact() { return mode_of(Switch::ldpc_spa) == 1; }

// cpx_viterbi_set_path / CPX_VITERBI_PATH: bit 0 wave only, bit 1 codeword path forced, bit 2 strict ("!": fail instead of
// falling back), bit 3 two-kernel form even where the fused kernel applies, bit 4 general kernel (viterbi_generic.hip)
inline int viterbi_path_flags() { return mode_of(Switch::viterbi_path); }
// the general Viterbi kernel (viterbi_generic.hip): any trellis cpx_trellis_create accepts, any traceback depth
int viterbi_generic(const ::cpx_trellis *t, const double *d_coded, int64_t B, int64_t len, int64_t L, int64_t T, int tb, int type,
                    uint8_t *d_bits, Scratch &sc, hipStream_t st);

inline hipStream_t pick_stream(void *s) { return s ? reinterpret_cast<hipStream_t>(s) : lib_stream(); }

// a handle's device table: hipMalloc + hipMemcpy of `bytes` into *d ("<what>: ..." set, CPX_ENOMEM / CPX_EHIP, on failure; *d stays
// null if the allocation failed, so the handle's own destroy releases what was built)
int upload(void **d, const void *h, size_t bytes, const char *what);

// a HIP event (no timing) for the lifetime of the object; e is null if it could not be created
struct Event {
    hipEvent_t e = nullptr;
    Event() { if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) e = nullptr; }
    ~Event() { if (e) (void)hipEventDestroy(e); }
    Event(const Event &) = delete;
    Event &operator=(const Event &) = delete;
};

// Device staging of the host-buffer entry points, on the library stream: `in` allocates and queues the upload of `host`, `out`
// allocates, `get` downloads (blocking, through d2h_pageable; nothing for zero bytes); the destructor frees every buffer.  Allocations
// are fresh per call (a zero-byte request still gets 8 bytes); copies run inside CPX_TRACE ranges, and with tracing on an upload is
// waited for so that the ranges do not overlap.  The optional outputs of an entry point are one array of `Out`, in the order of its
// arguments: `out(outs)` allocates `dev` for every entry whose `host` is non-null, `get(outs)` downloads the same entries in order;
// a null `host` keeps a null `dev`, which is what the `_dev` entry point takes for "not wanted".
class HostStage {
public:
    struct Out {
        void *host;
        size_t bytes;
        void *dev = nullptr;
        template <class T> T *as() const { return static_cast<T *>(dev); }
    };
    const hipStream_t st = lib_stream();
    HostStage() = default;
    HostStage(const HostStage &) = delete;
    HostStage &operator=(const HostStage &) = delete;
    ~HostStage() { for (void *p : bufs_) (void)hipFree(p); }
    template <class T> int out(size_t bytes, T **d) {
        void *p;
        int rc = alloc(bytes, &p);
        *d = static_cast<T *>(p);
        return rc;
    }
    template <class T> int in(const void *host, size_t bytes, T **d) {
        CPX_TRACE("H2D");
        void *p;
        if (int rc = alloc(bytes, &p)) return rc;
        *d = static_cast<T *>(p);
        CPX_HIP(hipMemcpyAsync(p, host, bytes, hipMemcpyHostToDevice, st));
        if (trace_enabled()) CPX_HIP(hipStreamSynchronize(st));
        return CPX_OK;
    }
    int get(void *host, const void *d, size_t bytes) {
        if (bytes == 0) return CPX_OK;
        CPX_TRACE("D2H");
        return d2h_pageable(host, d, bytes, st);
    }
    template <size_t N> int out(Out (&outs)[N]) {
        for (Out &o : outs)
            if (o.host)
                if (int rc = alloc(o.bytes, &o.dev)) return rc;
        return CPX_OK;
    }
    template <size_t N> int get(Out (&outs)[N]) {
        for (Out &o : outs)
            if (o.host)
                if (int rc = get(o.host, o.dev, o.bytes)) return rc;
        return CPX_OK;
    }
private:
    int alloc(size_t bytes, void **d) {
        if (bytes == 0) bytes = 8;
        hipError_t e = hipMalloc(d, bytes);
        if (e != hipSuccess) { set_error("hipMalloc(%zu) failed: %s", bytes, hipGetErrorString(e)); *d = nullptr; return CPX_ENOMEM; }
        bufs_.push_back(*d);
        return CPX_OK;
    }
    std::vector<void *> bufs_;
};

// the MIMO entry points' shared checks and staging (mimo.hip; also used by mimo_linear.hip)
int mimo_check(const ::cpx_modem *md, int64_t B, int nr, int nt, const char *what);   // handle, device and sizes
// the host-buffer wrappers' checks, ensure_device() first
int mimo_host_check(const double *y, const double *h, int64_t B, int nr, int nt, const void *out);
// y and H staged; an empty batch stages neither
int mimo_in(HostStage &s, const double *y, const double *h, int h_batched, int64_t B, int nr, int nt, const double **dy,
            const double **dh);

}  // namespace cpx

// ---- handles -----------------------------------------------------------------------------------
#define CPX_MAX_STATES 65536   // the specialised kernels stop at 128; viterbi_generic.hip / bcjr_exact.hip serve the rest
#define CPX_MAX_INPUTS 4
#define CPX_MAX_N 6

struct cpx_trellis {
    __attribute__((visibility("hidden"))) ~cpx_trellis() = default;   // (the handle types are declared in the public header, i.e. with
                                                                      //  default visibility: keep their implicit members out of the ABI)
    int k, n, S, I;
    int device;
    // host copies
    std::vector<int32_t> next_state, output;
    std::vector<int32_t> pred_state, pred_input, pred_code;  // [S][I] in np.where order
    // device tables (int32)
    int32_t *d_next = nullptr, *d_out = nullptr;             // [S][I]
    int32_t *d_pred_state = nullptr, *d_pred_input = nullptr, *d_pred_code = nullptr;  // [S][I]
    // the fused codeword-per-lane Viterbi kernels compiled for THIS code's generators (cpx_trellis_attach_viterbi_code, round 6):
    // [decoding type][run-time hop count]; null module: none attached (built-in pair or table-driven kernel)
    hipModule_t spec_mod = nullptr;
    hipFunction_t spec_fn[3][2] = {{nullptr, nullptr}, {nullptr, nullptr}, {nullptr, nullptr}};
    int spec_lg = 0;
    unsigned spec_g0 = 0, spec_g1 = 0;
    cpx::TrellisClass cls;                                   // filled by cpx_trellis_create, read by the Viterbi dispatch
};

struct cpx_ldpc {
    int n_v, n_c;
    int64_t n_edges;
    int device;
    int max_cdeg, max_vdeg;
    // check-major edge list (sorted by check, then variable)
    int32_t *d_edge_var = nullptr;    // [E] variable of edge e
    int32_t *d_row_ptr = nullptr;     // [n_c+1]
    // variable-major view: for each variable its edges in increasing check order
    int32_t *d_col_ptr = nullptr;     // [n_v+1]
    int32_t *d_col_edge = nullptr;    // [E] edge ids
    int32_t *d_col_cj = nullptr;      // [E] (check << 5) | position of the edge in its check's row (min-sum records)
    // padded copies (row/column stride cpad/vpad): their address depends on the node index only, so the
    // scalar loads of a work item issue together with row_ptr/col_ptr instead of after them
    int cpad = 0, vpad = 0;
    int32_t *d_row_pad = nullptr;     // [n_c][cpad] variable of the j-th edge of check c
    int32_t *d_col_pad_edge = nullptr;  // [n_v][vpad] edge id of the q-th edge of variable v
    int32_t *d_col_pad_cj = nullptr;    // [n_v][vpad] (check << 5) | position
    // LDS-resident path (ldpc_resident.hip): tables of pre-scaled LDS byte offsets, null when the state of one block
    // does not fit the LDS of a compute unit
    int32_t *d_res_row_deg = nullptr;   // [n_c] check degree
    int32_t *d_res_row_q = nullptr;     // [n_c][cpad] offset of Q[variable]; padding -> a +inf slot
    int32_t *d_res_col_r = nullptr;     // [n_v][vpad] offset of R[check][position], increasing check; padding -> a +0.0 slot
    int32_t *d_res_row_q32 = nullptr;   // the same two tables with 4-byte offsets (fp32-fast mode)
    int32_t *d_res_col_r32 = nullptr;
    int32_t *d_res_vgrp = nullptr;      // [ceil(n_v/64)] chunks of four entries per group of 64 variables
};

struct cpx_modem {
    // M and nbits stay the first two members, in this order: tests/test_adaptive_host.py checks the limits of cpx_adaptive_equalize
    // without a device on a stand-in that holds just these two ints (check_adaptive reads nothing else of the handle)
    int M, nbits;
    int device;
    double *d_const = nullptr;  // [M][2]
    // axis-separable square constellations (QAMModem): label = (a << nbits/2) | b, point = xs[a] + 1j*ys[b]
    bool separable = false;
    double *d_axes = nullptr;   // [2][sqrt(M)]: xs then ys
    // ... whose levels are equally spaced and labelled in reflected Gray order (QAMModem): level j = axes[0] + j * gp_step has
    // label j ^ (j >> 1) -- the soft demodulator then needs four exp per axis (demod.hip, GP)
    bool gp = false;
    double gp_step[2] = {0.0, 0.0};
};
