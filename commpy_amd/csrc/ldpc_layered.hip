// Layered (row-serial) normalised / offset min-sum LDPC decoding: cpx_ldpc_layered_*.
//
// The code is the edge list of cpx_ldpc_create, sorted by (check, variable).  A schedule is an ordered list of layers; a layer is a list of
// checks; every check appears exactly once and no two checks of one layer share a variable.  The rule (float64, operations in the order
// written, no fused multiply-add: -ffp-contract=off and the pragma in ll_scale); LLRs are positive for bit 0:
//   Start.       Q[v] = min(max(llr[v], -llr_clip), llr_clip) on a copy (the caller's array is not modified); R[e] = +0.0 for every edge.
//   Iterations.  it = 1 .. n_iters; within an iteration the layers in order; for every check c of the layer, its edges j in stored order:
//                  m_j  = Q[v_j] - R_cj
//                  a_j  = min over i != j of |m_i|
//                  g_j  = max(alpha * a_j - beta, 0.0)        two roundings: the product, then the difference
//                  s_j  = XOR over i != j of signbit(m_i)     the sign BIT: -0.0 counts as negative
//                  R_cj = s_j ? -g_j : g_j
//                  Q[v_j] = m_j + R_cj
//                No variable is touched twice within a layer, so the order of its checks cannot matter.
//   Decision.    After the last layer of an iteration bit[v] = signbit(Q[v]).  With early_stop: if every check's parity of bits is even the
//                block stops with iters = it, converged = 1; a block that never stops has iters = n_iters, converged = 0.  Without
//                early_stop iters = n_iters and converged is the parity test on the final bits.
//   Rejection.   A block with a NaN anywhere in its LLRs is rejected on its own: bits all zero, the llr output all NaN, iters = 0,
//                converged = 0.  +-inf is no reason to reject: the clip maps it to +-llr_clip.
//   Ties need no rule: when two magnitudes tie for the minimum every a_j has the same value whichever of them is called first.
//
// ldpc_layered_kernel<CAP>: one block per WAVE, lane = check.  A layer of n checks is cut into ceil(n / 64) passes; in a pass lane l owns
//   the check in schedule position first + l, gathers its Q values from LDS, and writes them back.  The waves of a workgroup share nothing
//   and never meet: a block is owned by one wave, LDS operations of a wave complete in order, so a layer needs no barrier -- only the
//   wave's own LDS counter is waited for where a layer ends (wave_sync).  Blocks retire as they finish: a wave that is done with its
//   block writes it out and takes the next index from a global queue (one atomic per block), so blocks that stop after 2 iterations
//   and blocks that run all 50 share the machine without a scan.
//   LDS per block: Q, 8 n_v bytes, and ONE RECORD PER CHECK instead of a message per edge, 24 n_c bytes: the two smallest magnitudes
//   (min1, min2), and a word holding the position of the smallest (8 bits) and the sign bits of m_j (32 bits).  The messages are
//   regenerated from it: R_cj = +-ll_scale(j == pos ? min2 : min1), the very operations (and so the very float64 values) that produced
//   the stored message; the record of all-zero magnitudes and signs regenerates the initial +0.0.  The records are indexed by schedule
//   position, so the lanes of a pass read and write consecutive words.  (1944,1296): 15.2 + 15.2 KiB, five blocks per compute unit.
//   The code's tables are read from global memory (L2 / vector L1; every wave reads the same ones): per pass and lane, CAP / 4 words of
//   four 16-bit variable indices laid out [pass][word][lane] (coalesced) and one word with the degree (0: the lane has no check), the
//   check's schedule position and a flag where a layer begins.  A pass's words are
//   requested one pass ahead.  CAP (8, 12, 16, 24, 32: the smallest that holds the largest check) bounds the unrolled row: its m_j stay
//   in registers, entries at and past the degree are computed on a valid address and discarded by selects, not by branches.
//   The syndrome pass after an iteration walks the same tables and reads the high dword (the sign) of each Q only.
//   Everything is written with vector stores; there are no atomics but the queue's.
#include "cpx_internal.h"
#include "cpx_wave.h"

#include <algorithm>
#include <cmath>

using namespace cpx;

#define CPX_LL_MIN_DEG 2
#define CPX_LL_MAX_DEG 32
#define CPX_LL_LDS_MAX (160 * 1024)        // one block's state: 8 n_v + 24 n_c bytes
#define LL_MAX_WAVES 8                     // blocks (waves) per workgroup

struct cpx_ldpc_layered {
    __attribute__((visibility("hidden"))) ~cpx_ldpc_layered() = default;
    int n_v = 0, n_c = 0, n_layers = 0, n_pass = 0, cap = 0, device = 0;
    int64_t n_edges = 0;
    unsigned block_lds = 0;              // bytes of LDS per block
    int waves = 0, per_cu = 0;           // blocks per workgroup; workgroups per compute unit as the runtime's occupancy query reports them
    // [n_pass][64] bits 0 .. 7: degree of the lane's check, 0 = none; bits 8 .. 29: its schedule position (none: that of lane 0's check);
    // bit 30: the pass begins a layer
    int32_t *d_deg = nullptr;
    uint2 *d_tab = nullptr;              // [n_pass][cap / 4][64] four 16-bit variable indices per word
};

namespace {

struct LlArgs {
    const double *llr;                   // [B][n_v]
    const int32_t *deg;
    const uint2 *tab;
    int *queue;                          // next block to hand out
    int B, n_v, n_c, n_pass, n_iters, early_stop;
    unsigned block_lds;
    double alpha, beta, clip;
    int8_t *bits;                        // [B][n_v] or null
    double *out;                         // [B][n_v] or null
    int32_t *iters;                      // [B] or null
    uint8_t *converged;                  // [B] or null
};

// orders this wave's LDS writes before its later reads (the waves of a workgroup never meet).  LDS only: a fence would also wait for the
// global loads in flight, i.e. for the next pass's table words
__device__ __forceinline__ void wave_sync() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
}

// g = max(alpha a - beta, 0.0): the product is rounded, then the difference
__device__ __forceinline__ double ll_scale(double a, double alpha, double beta) {
#pragma clang fp contract(off)
    const double prod = alpha * a;
    const double x = prod - beta;
    return x > 0.0 ? x : 0.0;
}

template <int U>
__device__ __forceinline__ int ll_idx(const uint2 (&w)[U], int j) {
    const unsigned x = (j & 2) ? w[j >> 2].y : w[j >> 2].x;
    return (int)((j & 1) ? x >> 16 : x & 0xffffu);
}

// s ? -g : g for g >= +0.0 and s = 0 / 1: the sign bit is set, which is what negation does (a -0.0 included)
__device__ __forceinline__ double ll_signed(double g, unsigned s) {
    return __hiloint2double(__double2hiint(g) ^ (int)(s << 31), __double2loint(g));
}

// one check: the row's messages regenerated from its record, the new record, the new Q.  deg = 0: the lane has no check (slot is then a
// valid one that is read and not written)
template <int CAP>
__device__ __forceinline__ void ll_check(double *Q, double *M1, double *M2, unsigned long long *MT, int slot, int deg, const uint2 (&w)[CAP / 4],
                                         double alpha, double beta) {
    const double o1 = M1[slot], o2 = M2[slot];
    const unsigned long long ot = MT[slot];
    double m[CAP];
#pragma unroll
    for (int j = 0; j < CAP; j++) m[j] = Q[ll_idx(w, j)];
    const double g1 = ll_scale(o1, alpha, beta), g2 = ll_scale(o2, alpha, beta);
    const int opos = (int)(ot & 0xffull);
    const unsigned osg = (unsigned)(ot >> 8), opar = (unsigned)__popc(osg) & 1u;
    double n1 = __builtin_huge_val(), n2 = __builtin_huge_val();
    int pos = 0;
    unsigned sg = 0u;
#pragma unroll
    for (int j = 0; j < CAP; j++) {
        m[j] = m[j] - ll_signed(j == opos ? g2 : g1, (opar ^ (osg >> j)) & 1u);
        const bool in = j < deg;
        const double am = in ? __builtin_fabs(m[j]) : __builtin_huge_val();
        // the two smallest so far: am < n1 moves n1 to n2, else am < n2 replaces n2 -- as minima and a maximum (no NaN, no -0.0 here)
        pos = am < n1 ? j : pos;
        n2 = __builtin_fmin(n2, __builtin_fmax(n1, am));
        n1 = __builtin_fmin(n1, am);
        sg |= ((unsigned)__double2hiint(m[j]) >> 31) << j;
    }
    sg &= deg >= 32 ? ~0u : (1u << deg) - 1u;                    // the entries past the degree have no sign
    const double h1 = ll_scale(n1, alpha, beta), h2 = ll_scale(n2, alpha, beta);
    const unsigned par = (unsigned)__popc(sg) & 1u;
#pragma unroll
    for (int j = 0; j < CAP; j++)
        if (j < deg) Q[ll_idx(w, j)] = m[j] + ll_signed(j == pos ? h2 : h1, (par ^ (sg >> j)) & 1u);
    if (deg > 0) {
        M1[slot] = n1;
        M2[slot] = n2;
        MT[slot] = (unsigned long long)(unsigned)pos | ((unsigned long long)sg << 8);
    }
}

template <int CAP>
__global__ __launch_bounds__(LL_MAX_WAVES * 64) void ldpc_layered_kernel(LlArgs a) {
    extern __shared__ __align__(16) char lds[];
    constexpr int U = CAP / 4;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n_v = a.n_v, n_c = a.n_c, P = a.n_pass;
    double *Q = reinterpret_cast<double *>(lds + (size_t)wave * a.block_lds);
    double *M1 = Q + n_v, *M2 = M1 + n_c;
    unsigned long long *MT = reinterpret_cast<unsigned long long *>(M2 + n_c);
    const unsigned *Qw = reinterpret_cast<const unsigned *>(Q);
    const double alpha = a.alpha, beta = a.beta, clip = a.clip;
    auto load_pass = [&](int p, uint2 (&w)[U], int &deg) {
#pragma unroll
        for (int k = 0; k < U; k++) w[k] = a.tab[((size_t)p * U + k) * 64 + lane];
        deg = a.deg[p * 64 + lane];
    };
    // Control flow round the block loop is kept UNIFORM on purpose: nothing in it is under `if (lane == 0)`.  With lane-0 blocks at the end
    // of the body (the block's scalar results) and at its start (the queue) the structuriser turned the loop inside out: lane 0 left for
    // an outer loop that held the stores and the atomic while lanes 1 .. 63 went round again, read the block index from lane 1 (where
    // it is 0) and decoded block 0 for ever.  So every lane takes part in the atomic (lane 0 adds 1, the others 0: lane 0's return
    // value is the block's index) and every lane stores the block's scalar results (one address, one value).
    for (;;) {
        const int t = atomicAdd(a.queue, lane == 0 ? 1 : 0);
        const int b = __builtin_amdgcn_readfirstlane(t);
        if (b >= a.B) break;
        const int64_t row = (int64_t)b * n_v;
        const double *__restrict__ in = a.llr + row;
        wave_sync();                                             // the block before this one has been read out of LDS
        bool bad = false;
        for (int v0 = lane; v0 < n_v; v0 += 256) {               // four requests in flight per lane
            double x[4];
#pragma unroll
            for (int u = 0; u < 4; u++) x[u] = in[v0 + 64 * u < n_v ? v0 + 64 * u : v0];
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const int v = v0 + 64 * u;
                if (v < n_v) {
                    bad |= x[u] != x[u];
                    const double lo = x[u] < -clip ? -clip : x[u];
                    Q[v] = lo > clip ? clip : lo;
                }
            }
        }
        for (int s = lane; s < n_c; s += 64) {                   // the record that regenerates R = +0.0 on every edge
            M1[s] = 0.0;
            M2[s] = 0.0;
            MT[s] = 0ull;
        }
        const bool rejected = __ballot(bad) != 0ull;             // a NaN: the block is rejected on its own, no iteration runs
        const int n_iters = rejected ? 0 : a.n_iters;
        uint2 cw[U], nw[U];
        int cd, nd;
        load_pass(0, cw, cd);
        int it = 0, conv = 0;
        while (it < n_iters) {
            it++;
            for (int p = 0; p < P; p++) {
                load_pass(p + 1 < P ? p + 1 : 0, nw, nd);
                if (__builtin_amdgcn_readfirstlane(cd) & (1 << 30)) wave_sync();      // a layer begins: the layer before it is in LDS
                ll_check<CAP>(Q, M1, M2, MT, (cd >> 8) & 0x3fffff, cd & 0xff, cw, alpha, beta);
#pragma unroll
                for (int k = 0; k < U; k++) cw[k] = nw[k];
                cd = nd;
            }
            wave_sync();
            if (a.early_stop || it == n_iters) {
                bool odd = false;
                for (int p = 0; p < P; p++) {
                    load_pass(p + 1 < P ? p + 1 : 0, nw, nd);
                    unsigned par = 0u;
#pragma unroll
                    for (int j = 0; j < CAP; j++) {
                        const unsigned hi = Qw[2 * ll_idx(cw, j) + 1];
                        par ^= j < (cd & 0xff) ? hi >> 31 : 0u;
                    }
                    odd |= par != 0u;
#pragma unroll
                    for (int k = 0; k < U; k++) cw[k] = nw[k];
                    cd = nd;
                }
                conv = __ballot(odd) == 0ull ? 1 : 0;
                if (conv) break;
            }
        }
        for (int v = lane; v < n_v; v += 64) {
            const double x = rejected ? __builtin_nan("") : Q[v];
            if (a.out) a.out[row + v] = x;
            if (a.bits) a.bits[row + v] = (int8_t)(!rejected && __builtin_signbit(x) ? 1 : 0);
        }
        if (a.iters) a.iters[b] = it;                            // every lane: see above
        if (a.converged) a.converged[b] = (uint8_t)conv;
    }
}

int cap_of(int max_deg) { return max_deg <= 8 ? 8 : max_deg <= 12 ? 12 : max_deg <= 16 ? 16 : max_deg <= 24 ? 24 : 32; }

const void *kernel_of(int cap) {
    switch (cap) {
    case 8: return (const void *)ldpc_layered_kernel<8>;
    case 12: return (const void *)ldpc_layered_kernel<12>;
    case 16: return (const void *)ldpc_layered_kernel<16>;
    case 24: return (const void *)ldpc_layered_kernel<24>;
    default: return (const void *)ldpc_layered_kernel<32>;
    }
}

int check_decode(const cpx_ldpc_layered *c, int64_t B, int n_iters, double alpha, double beta, double llr_clip, bool any_output) {
    CPX_REQUIRE(c, CPX_EINVAL, "ldpc_layered_decode: null pointer");
    CPX_REQUIRE(B >= 0, CPX_EINVAL, "ldpc_layered_decode: B = %lld", (long long)B);
    CPX_REQUIRE(B <= 0x7fff0000ll, CPX_ELIMIT, "ldpc_layered_decode: B = %lld, the limit is %lld blocks per call", (long long)B, 0x7fff0000ll);
    CPX_REQUIRE(n_iters >= 1, CPX_ELIMIT, "ldpc_layered_decode: n_iters = %d, the limit is n_iters >= 1", n_iters);
    CPX_REQUIRE(std::isfinite(alpha) && alpha > 0.0, CPX_ELIMIT, "ldpc_layered_decode: alpha = %g, the limit is alpha > 0 and finite", alpha);
    CPX_REQUIRE(std::isfinite(beta) && beta >= 0.0, CPX_ELIMIT, "ldpc_layered_decode: beta = %g, the limit is beta >= 0 and finite", beta);
    CPX_REQUIRE(std::isfinite(llr_clip) && llr_clip > 0.0, CPX_ELIMIT, "ldpc_layered_decode: llr_clip = %g, the limit is llr_clip > 0 and finite",
                llr_clip);
    CPX_REQUIRE(any_output, CPX_EINVAL, "ldpc_layered_decode: no output requested");
    return CPX_OK;
}

}  // namespace

extern "C" {

int cpx_ldpc_layered_create(int n_v, int n_c, int64_t n_edges, const int32_t *edge_check, const int32_t *edge_var, int n_layers,
                            const int32_t *layer_start, const int32_t *layer_checks, cpx_ldpc_layered **out) {
    CPX_TRACE("cpx_ldpc_layered_create");
    CPX_REQUIRE(out, CPX_EINVAL, "ldpc_layered: null pointer");
    *out = nullptr;
    CPX_REQUIRE(edge_check && edge_var && layer_start && layer_checks, CPX_EINVAL, "ldpc_layered: null pointer");
    CPX_REQUIRE(n_v >= 1 && n_c >= 1 && n_edges >= 1 && n_edges <= (int64_t)n_c * CPX_LL_MAX_DEG, CPX_EINVAL,
                "ldpc_layered: n_v = %d, n_c = %d, n_edges = %lld", n_v, n_c, (long long)n_edges);
    const size_t block_lds = 8 * (size_t)n_v + 24 * (size_t)n_c;
    CPX_REQUIRE(block_lds <= CPX_LL_LDS_MAX, CPX_ELIMIT,
                "ldpc_layered: the state of one block, 8 n_v + 24 n_c = %zu bytes, is above the kernel's LDS budget of %d bytes", block_lds,
                CPX_LL_LDS_MAX);
    std::vector<int> row_ptr((size_t)n_c + 1, 0);
    for (int64_t e = 0; e < n_edges; e++) {
        const int c = edge_check[e], v = edge_var[e];
        CPX_REQUIRE(c >= 0 && c < n_c && v >= 0 && v < n_v, CPX_EINVAL, "ldpc_layered: edge %lld = (%d, %d) is out of range", (long long)e, c, v);
        CPX_REQUIRE(e == 0 || c > edge_check[e - 1] || (c == edge_check[e - 1] && v > edge_var[e - 1]), CPX_EINVAL,
                    "ldpc_layered: the edge list is not sorted by (check, variable) without repeats at edge %lld", (long long)e);
        row_ptr[(size_t)c + 1]++;
    }
    int max_deg = 0;
    for (int c = 0; c < n_c; c++) {
        const int d = row_ptr[(size_t)c + 1];
        CPX_REQUIRE(d >= CPX_LL_MIN_DEG && d <= CPX_LL_MAX_DEG, CPX_ELIMIT, "ldpc_layered: check %d has degree %d, the limit is %d .. %d", c, d,
                    CPX_LL_MIN_DEG, CPX_LL_MAX_DEG);
        max_deg = std::max(max_deg, d);
        row_ptr[(size_t)c + 1] += row_ptr[c];
    }
    CPX_REQUIRE(n_layers >= 1 && n_layers <= n_c && layer_start[0] == 0 && layer_start[n_layers] == n_c, CPX_ELIMIT,
                "ldpc_layered: the schedule is not a partition of the %d checks into 1 .. %d layers", n_c, n_c);
    std::vector<char> seen((size_t)n_c, 0);
    std::vector<int> stamp((size_t)n_v, -1);
    int n_pass = 0;
    for (int l = 0; l < n_layers; l++) {
        const int s0 = layer_start[l], s1 = layer_start[l + 1];
        CPX_REQUIRE(s0 >= 0 && s1 > s0 && s1 <= n_c, CPX_ELIMIT, "ldpc_layered: the schedule is not a partition of the checks: layer %d is empty or out of range", l);
        for (int s = s0; s < s1; s++) {
            const int c = layer_checks[s];
            CPX_REQUIRE(c >= 0 && c < n_c && !seen[c], CPX_ELIMIT, "ldpc_layered: the schedule is not a partition of the checks: entry %d of layer %d", s - s0,
                        l);
            seen[c] = 1;
            for (int e = row_ptr[c]; e < row_ptr[(size_t)c + 1]; e++) {
                CPX_REQUIRE(stamp[edge_var[e]] != l, CPX_ELIMIT, "ldpc_layered: the schedule is not conflict-free: layer %d holds two checks with variable %d", l,
                            edge_var[e]);
                stamp[edge_var[e]] = l;
            }
        }
        n_pass += (s1 - s0 + 63) / 64;
    }
    if (int rc = ensure_device()) return rc;
    const int cap = cap_of(max_deg), U = cap / 4;
    std::vector<int32_t> deg((size_t)n_pass * 64, 0);
    std::vector<uint2> tab((size_t)n_pass * U * 64, make_uint2(0u, 0u));
    int p = 0;
    for (int l = 0; l < n_layers; l++) {
        for (int s0 = layer_start[l]; s0 < layer_start[l + 1]; s0 += 64, p++) {
            for (int lane = 0; lane < 64; lane++) {
                const bool has = s0 + lane < layer_start[l + 1];
                const int c = layer_checks[has ? s0 + lane : s0];           // a lane without a check reads the first one's variables
                const int d = row_ptr[(size_t)c + 1] - row_ptr[c];
                deg[(size_t)p * 64 + lane] = (has ? d : 0) | ((has ? s0 + lane : s0) << 8) | (s0 == layer_start[l] ? 1 << 30 : 0);
                for (int j = 0; j < cap; j++) {
                    const unsigned v = (unsigned)edge_var[row_ptr[c] + (j < d ? j : 0)];      // past the degree: the row's first variable
                    uint2 &w = tab[((size_t)p * U + (j >> 2)) * 64 + lane];
                    unsigned &half = (j & 2) ? w.y : w.x;
                    half |= (j & 1) ? v << 16 : v;
                }
            }
        }
    }
    cpx_ldpc_layered *c = new cpx_ldpc_layered;
    c->n_v = n_v; c->n_c = n_c; c->n_layers = n_layers; c->n_pass = n_pass; c->cap = cap; c->n_edges = n_edges;
    c->block_lds = (unsigned)block_lds;
    auto fail = [&](int rc) { cpx_ldpc_layered_destroy(c); return rc; };
    if (hipGetDevice(&c->device) != hipSuccess) { set_error("ldpc_layered: hipGetDevice failed"); return fail(CPX_EHIP); }
    int rc;
    if ((rc = upload((void **)&c->d_deg, deg.data(), deg.size() * sizeof(int32_t), "ldpc_layered")) ||
        (rc = upload((void **)&c->d_tab, tab.data(), tab.size() * sizeof(uint2), "ldpc_layered")))
        return fail(rc);
    // blocks per workgroup: as many as the LDS of a compute unit holds, eight at the most (smaller codes share it between workgroups)
    c->waves = std::min<int>(LL_MAX_WAVES, (int)(CPX_LL_LDS_MAX / block_lds));
    const void *fn = kernel_of(cap);
    const unsigned lds = c->block_lds * (unsigned)c->waves;
    if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, CPX_LL_LDS_MAX) != hipSuccess ||
        hipOccupancyMaxActiveBlocksPerMultiprocessor(&c->per_cu, fn, c->waves * 64, lds) != hipSuccess || c->per_cu < 1) {
        set_error("ldpc_layered: the runtime's occupancy query failed for %d waves and %u bytes of LDS", c->waves, lds);
        return fail(CPX_EHIP);
    }
    *out = c;
    return CPX_OK;
}

int cpx_ldpc_layered_destroy(cpx_ldpc_layered *c) {
    if (!c) return CPX_OK;
    (void)hipFree(c->d_deg); (void)hipFree(c->d_tab);
    delete c;
    return CPX_OK;
}

int cpx_ldpc_layered_decode_dev(const cpx_ldpc_layered *c, const double *d_llr, int64_t B, int n_iters, double alpha, double beta,
                                int early_stop, double llr_clip, int8_t *d_bits, double *d_llr_out, int32_t *d_iters, uint8_t *d_converged,
                                void *stream) {
    CPX_TRACE("cpx_ldpc_layered_decode_dev");
    if (int rc = check_decode(c, B, n_iters, alpha, beta, llr_clip, d_bits || d_llr_out || d_iters || d_converged)) return rc;
    if (B == 0) return CPX_OK;
    CPX_REQUIRE(d_llr, CPX_EINVAL, "ldpc_layered_decode: null pointer");
    if (int rcd = check_handle_device(c->device, "ldpc_layered_decode")) return rcd;
    hipStream_t st = pick_stream(stream);
    Scratch sc;
    int *queue;
    // (Slot::state: this entry point's only request; the other decoders that take the slot are separate entry points)
    if (int rc = sc.get(st, Slot::state, sizeof(int), &queue)) return rc;
    CPX_HIP(hipMemsetAsync(queue, 0, sizeof(int), st));
    LlArgs a{d_llr, c->d_deg, c->d_tab, queue, (int)B, c->n_v, c->n_c, c->n_pass, n_iters, early_stop ? 1 : 0, c->block_lds,
             alpha, beta, llr_clip, d_bits, d_llr_out, d_iters, d_converged};
    const int resident = device_cus() * c->per_cu;              // workgroups: the persistent grid
    const int64_t wgs = (B + c->waves - 1) / c->waves;
    const unsigned lds = c->block_lds * (unsigned)c->waves;
    const dim3 grid(grid_of(wgs, resident)), block((unsigned)c->waves * 64);
    switch (c->cap) {
    case 8: hipLaunchKernelGGL(ldpc_layered_kernel<8>, grid, block, lds, st, a); break;
    case 12: hipLaunchKernelGGL(ldpc_layered_kernel<12>, grid, block, lds, st, a); break;
    case 16: hipLaunchKernelGGL(ldpc_layered_kernel<16>, grid, block, lds, st, a); break;
    case 24: hipLaunchKernelGGL(ldpc_layered_kernel<24>, grid, block, lds, st, a); break;
    default: hipLaunchKernelGGL(ldpc_layered_kernel<32>, grid, block, lds, st, a); break;
    }
    CPX_HIP(hipGetLastError());
    note_kernel("ldpc_layered_kernel<%d> waves=%d lds=%u per_cu=%d resident=%d passes=%d", c->cap, c->waves, lds, c->per_cu,
                resident * c->waves, c->n_pass);
    return CPX_OK;
}

int cpx_ldpc_layered_decode(const cpx_ldpc_layered *c, const double *llr, int64_t B, int n_iters, double alpha, double beta, int early_stop,
                            double llr_clip, int8_t *bits, double *llr_out, int32_t *iters, uint8_t *converged) {
    CPX_TRACE("cpx_ldpc_layered_decode");
    if (int rc = check_decode(c, B, n_iters, alpha, beta, llr_clip, bits || llr_out || iters || converged)) return rc;
    if (B == 0) return CPX_OK;
    CPX_REQUIRE(llr, CPX_EINVAL, "ldpc_layered_decode: null pointer");
    int rc = ensure_device();
    if (rc) return rc;
    const size_t b = (size_t)B, nv = (size_t)c->n_v;
    HostStage::Out outs[4] = {{bits, b * nv}, {llr_out, 8 * b * nv}, {iters, 4 * b}, {converged, b}};
    HostStage s;
    const double *din;
    if ((rc = s.in(llr, 8 * b * nv, &din)) || (rc = s.out(outs))) return rc;
    if ((rc = cpx_ldpc_layered_decode_dev(c, din, B, n_iters, alpha, beta, early_stop, llr_clip, outs[0].as<int8_t>(), outs[1].as<double>(),
                                          outs[2].as<int32_t>(), outs[3].as<uint8_t>(), s.st)))
        return rc;
    return s.get(outs);
}

}  // extern "C"
