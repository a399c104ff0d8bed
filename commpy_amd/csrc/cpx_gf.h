// What the algebraic codecs (bch.hip, bch_chase.hip, rs.hip) share.  On the host: the limits, the checks and the exp / log tables of
// GF(2^m) as a handle builds them, and the launch helpers of the decoders.  On the device: GF(2^m) arithmetic on the LDS-staged tables and
// the two stages every decoder runs, one wave on one word -- Berlekamp-Massey and the Chien search.  bch_decode_kernel, bch_chase_kernel
// and rs_decode_kernel call this one copy, so a failure rule ("leading coefficient zero", "root in the shortened region") is stated once.
#pragma once
#include "cpx_internal.h"
#include "cpx_wave.h"

#include <mutex>
#include <set>
#include <utility>
#include <vector>

#define CPX_GF_MIN_M 3
#define CPX_GF_MAX_M 14
#define CPX_GF_LDS_MAX (160 * 1024)
#define CPX_GF_MAX_WAVES 16
#define CPX_GF_NONE 0xFFFFu                // "logarithm" of a zero coefficient

namespace cpx {

// tab = [2][2^m] uint16: exp[e] = alpha^e (e = 0 .. N, N = 2^m - 1, alpha = x), then log[v] (log[0] = 0).  CPX_EINVAL with "<who>: ..."
// unless x generates the multiplicative group under prim_poly (whose degree the caller has checked).
inline int gf_tables(const char *who, int m, uint32_t prim_poly, std::vector<uint16_t> &tab) {
    const int N = (1 << m) - 1;
    tab.assign((size_t)2 << m, 0);
    uint16_t *ex = tab.data(), *lg = ex + ((size_t)1 << m);
    unsigned v = 1;
    for (int e = 0; e < N; ++e) {
        CPX_REQUIRE(e == 0 || v != 1u, CPX_EINVAL, "%s: prim_poly = %u is not primitive (x has order %d, not %d)", who, prim_poly, e, N);
        ex[e] = (uint16_t)v;
        lg[v] = (uint16_t)e;
        v <<= 1;
        if (v >> m) v ^= prim_poly;
    }
    CPX_REQUIRE(v == 1u, CPX_EINVAL, "%s: prim_poly = %u is not primitive (x does not return to 1 after %d steps)", who, prim_poly, N);
    ex[N] = 1;
    return CPX_OK;
}

// the field and the length of a code of `who` ("bch", "rs"), checked, and the tables of gf_tables
inline int gf_field(const char *who, int m, uint32_t prim_poly, int n, std::vector<uint16_t> &tab) {
    CPX_REQUIRE(m >= CPX_GF_MIN_M && m <= CPX_GF_MAX_M, CPX_ELIMIT, "%s: m = %d is outside the engine's range %d .. %d", who, m, CPX_GF_MIN_M,
                CPX_GF_MAX_M);
    const int N = (1 << m) - 1;
    CPX_REQUIRE(n >= 2 && n <= N, CPX_ELIMIT, "%s: n = %d is outside 2 .. 2^m - 1 = %d", who, n, N);
    CPX_REQUIRE((prim_poly >> m) == 1u, CPX_EINVAL, "%s: prim_poly = %u has not degree m = %d", who, prim_poly, m);
    return gf_tables(who, m, prim_poly, tab);
}

// g(alpha^x), by Horner, for g of degree deg with the coefficients c[0 .. deg] (field elements; 0 / 1 for a binary code), 0 <= x
template <typename T>
inline unsigned gf_eval(const std::vector<uint16_t> &tab, int m, const T *c, int deg, int x) {
    const uint16_t *ex = tab.data(), *lg = ex + ((size_t)1 << m);
    const int N = (1 << m) - 1;
    unsigned acc = 0;
    for (int i = deg; i >= 0; --i) {
        if (acc) acc = ex[(lg[acc] + x) % N];
        acc ^= c[i];
    }
    return acc;
}

inline int check_batch(const void *handle, int64_t B, const char *what) {
    CPX_REQUIRE(handle, CPX_EINVAL, "%s: null handle", what);
    CPX_REQUIRE(B >= 0, CPX_EINVAL, "%s: B = %lld", what, (long long)B);
    return CPX_OK;
}

__host__ __device__ inline unsigned gf_tab_lds(int m) { return 4u << m; }      // bytes of the two tables

// waves per workgroup of a decoder: small tables leave room for several workgroups per compute unit
inline int gf_waves(int m) { return m <= 8 ? 4 : m <= 11 ? 8 : CPX_GF_MAX_WAVES; }

// dynamic LDS above 64 KiB has to be allowed once per kernel and device
inline int raise_lds(const void *fn, int bytes, int device, const char *who) {
    static std::mutex mu;
    static std::set<std::pair<const void *, int>> raised;
    CPX_REQUIRE(device >= 0 && device < 64, CPX_ELIMIT, "%s: device index %d is outside 0 .. 63", who, device);
    std::lock_guard<std::mutex> lk(mu);
    if (!raised.count({fn, device})) {
        CPX_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
        raised.insert({fn, device});
    }
    return CPX_OK;
}

// workgroups of `waves` waves and `lds` bytes that a compute unit holds at once: what the LDS allows, at most 32 waves
inline int wgs_per_cu(uint64_t lds, int waves) {
    const int by_lds = (int)(CPX_GF_LDS_MAX / lds), by_waves = 32 / waves;
    return by_lds < by_waves ? by_lds : by_waves;
}

// the grid of a kernel whose workgroups stride over `wgs` items of work: no more workgroups than are resident at once
inline unsigned resident_grid(int64_t wgs, unsigned lds, int waves) { return grid_of(wgs, (int64_t)device_cus() * wgs_per_cu(lds, waves)); }

#ifdef __HIPCC__
// orders this wave's LDS writes before its later reads (the waves never meet after the staging barrier)
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ unsigned wave_xor(unsigned v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v ^= (unsigned)__shfl_xor((int)v, d);
    return v;
}

// the tables in LDS; every index a caller forms must lie in 0 .. 2^m - 1
struct Gf {
    const uint16_t *ex, *lg;
    int N;
    __device__ __forceinline__ unsigned mul(unsigned a, unsigned b) const {
        if (a == 0u || b == 0u) return 0u;
        int e = (int)lg[a] + (int)lg[b];
        if (e >= N) e -= N;
        return ex[e];
    }
};

// the exp and log tables of the handle into LDS at `base` (2^(m+2) bytes), by the whole workgroup; ends with the only block barrier
__device__ __forceinline__ Gf stage_tables(unsigned char *base, const uint16_t *tab, int m, int N) {
    uint32_t *dst = reinterpret_cast<uint32_t *>(base);
    const uint32_t *src = reinterpret_cast<const uint32_t *>(tab);
    for (int i = threadIdx.x; i < (1 << m); i += blockDim.x) dst[i] = src[i];
    __syncthreads();
    Gf gf;
    gf.ex = reinterpret_cast<const uint16_t *>(base);
    gf.lg = gf.ex + (1 << m);
    gf.N = N;
    return gf;
}

// Berlekamp-Massey over synd[0 .. nsyn), started at rho = f with length f from the polynomial the caller passes in sigma (lane q holds
// the coefficient of x^q): 1 and f = 0 for errors alone, the erasure locator of f flagged positions otherwise.  Lane q ends with the
// locator's coefficient C_q in sigma, `length` is its length L.  The length changes when 2 L <= rho + f, to rho + 1 - L + f; L only
// grows, so the first length with 2 L - f > nsyn is a failure at once (nsyn = 2t, f = 0: L > t).  The discrepancy is an XOR across the
// wave.  Returns true for a failure: that, or a locator of a lower degree than its length (fewer than L roots).
__device__ __forceinline__ bool berlekamp_massey(const Gf &gf, const uint16_t *synd, int nsyn, int f, int lane, unsigned &sigma, int &length) {
    const int N = gf.N;
    // C the connection polynomial, Bp the one before the last length change, b its discrepancy, sh the shift
    unsigned C = sigma, Bp = C, b = 1u;
    int L = f, sh = 1;
    bool fail = false;
    for (int rho = f; rho < nsyn; ++rho) {
        const unsigned d = wave_xor(lane <= L ? gf.mul(C, synd[rho - lane]) : 0u);       // L <= rho
        if (d == 0u) { ++sh; continue; }
        int e = (int)gf.lg[d] - (int)gf.lg[b];
        if (e < 0) e += N;
        const unsigned coef = gf.ex[e];
        const unsigned moved = (unsigned)__shfl((int)Bp, lane >= sh ? lane - sh : lane);
        const unsigned next = C ^ gf.mul(coef, lane >= sh ? moved : 0u);
        if (2 * L <= rho + f) {
            L = rho + 1 - L + f;
            if (2 * L - f > nsyn) { fail = true; break; }
            Bp = C;
            b = d;
            sh = 1;
        } else {
            ++sh;
        }
        C = next;
    }
    if (!fail && __shfl((int)C, L) == 0) fail = true;
    sigma = C;
    length = L;
    return fail;
}

// Chien search of the locator (lane q <= L holds C_q, C_0 = 1) over the positions 0 .. n - 1, four chunks at a time: the lane of degree
// d evaluates it at alpha^-d; returns the number of roots.  MASK: the ballot of a chunk's roots goes to mask[c] (nw 64-bit words).  LIST:
// the positions of the roots go to list, ascending (64 uint16: the locator has at most L <= 63 roots).  clog receives the logarithms of
// the 64 lanes' coefficients, CPX_GF_NONE above L and for a zero coefficient; visible to the wave on return, like mask and list after the
// caller's next wave_sync.
template <bool MASK, bool LIST>
__device__ __forceinline__ int chien_search(const Gf &gf, unsigned C, int L, uint16_t *clog, unsigned long long *mask, uint16_t *list, int n,
                                            int nw, int lane) {
    const int N = gf.N;
    int count = 0;
    clog[lane] = lane <= L && C ? gf.lg[C] : (uint16_t)CPX_GF_NONE;
    wave_sync();
    for (int c0 = 0; c0 < nw; c0 += 4) {                          // four chunks share the read of clog[q]; their gathers are independent
        int kk[4], qk[4];
        unsigned v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int d = n - 1 - ((c0 + u) * 64 + lane);
            kk[u] = d > 0 ? N - d : 0;                            // -d mod N; a lane past the word's end computes a value nobody reads
            qk[u] = 0;
            v[u] = 1u;                                            // C_0 = 1
        }
        for (int q = 1; q <= L; ++q) {
            const int cl = clog[q];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                qk[u] += kk[u];
                if (qk[u] >= N) qk[u] -= N;
            }
            if (cl != (int)CPX_GF_NONE) {
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    int e = cl + qk[u];
                    if (e >= N) e -= N;
                    v[u] ^= gf.ex[e];
                }
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int i = (c0 + u) * 64 + lane;
            const unsigned long long roots = __ballot(i < n && v[u] == 0u);
            if (MASK && lane == 0 && c0 + u < nw) mask[c0 + u] = roots;
            if (LIST) {
                const int at = count + __popcll(roots & ((1ull << lane) - 1ull));
                if (((roots >> lane) & 1ull) && at < 64) list[at] = (uint16_t)i;
            }
            count += __popcll(roots);
        }
    }
    return count;
}
#endif  // __HIPCC__

}  // namespace cpx
