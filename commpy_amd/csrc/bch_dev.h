// What the BCH kernels share (bch.hip: bounded-distance decoding of hard decisions, bch_chase.hip: Chase-II soft decoding): the handle,
// GF(2^m) arithmetic on the LDS-staged tables, and the three stages of the algebraic decoder -- syndromes, Berlekamp-Massey, Chien
// search -- each executed by one wave on one word.  Both kernels call this code, so a test pattern of the Chase decoder is decoded by
// exactly the rule of bch_decode_kernel, its failure conditions included.
#pragma once
#include "cpx_gf.h"
#include "cpx_internal.h"
#include "cpx_wave.h"

#define CPX_BCH_MIN_M 3
#define CPX_BCH_MAX_M 14
#define CPX_BCH_MAX_T 32
#define CPX_BCH_MAX_GEN_WORDS 7            // 64-bit words of a remainder: deg g <= 14 * 32 = 448
#define CPX_BCH_LDS_MAX (160 * 1024)
#define BCH_MAX_WAVES 16

struct cpx_bch {
    __attribute__((visibility("hidden"))) ~cpx_bch() = default;
    int m, N, n, k, t, deg, device;
    uint64_t gen[CPX_BCH_MAX_GEN_WORDS];   // g without its leading term, bit j of word w = coefficient of x^(64 w + j)
    uint16_t *d_tab = nullptr;             // [2][2^m]: exp then log
};

namespace cpx {

__host__ __device__ inline unsigned bch_tab_lds(int m) { return 4u << m; }

// waves per workgroup: small tables leave room for several workgroups per compute unit
inline int bch_waves(int m) { return m <= 8 ? 4 : m <= 11 ? 8 : BCH_MAX_WAVES; }

#ifdef __HIPCC__
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ unsigned wave_xor(unsigned v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v ^= (unsigned)__shfl_xor((int)v, d);
    return v;
}

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

// S_j for the G odd indices j0, j0 + 2, ...: synd[j - 1] = XOR over the set bits of alpha^(j d), d the degree of the position
template <int G>
__device__ __forceinline__ void syndrome_group(const Gf &gf, const unsigned long long *rw, uint16_t *synd, int nw, int j0, int d0, int lane) {
    const int N = gf.N;
    int e[G], step[G];
    unsigned acc[G];
#pragma unroll
    for (int u = 0; u < G; ++u) {
        const int j = j0 + 2 * u;
        step[u] = (64 * j) % N;
        e[u] = d0 > 0 ? (int)((unsigned)(j * d0) % (unsigned)N) : 0;        // j d0 < 64 * 2^14
        acc[u] = 0u;
    }
    for (int c = 0; c < nw; ++c) {
        const unsigned take = 0u - (unsigned)((rw[c] >> lane) & 1ull);
#pragma unroll
        for (int u = 0; u < G; ++u) {
            acc[u] ^= gf.ex[e[u]] & take;                         // e stays in 0 .. N - 1 on every lane: the gather needs no mask
            e[u] -= step[u];
            if (e[u] < 0) e[u] += N;
        }
    }
#pragma unroll
    for (int u = 0; u < G; ++u) {
        const unsigned s = wave_xor(acc[u]);
        if (lane == 0) synd[j0 + 2 * u - 1] = (uint16_t)s;
    }
}

// synd[0 .. 2t) = S_1 .. S_2t of the word held as ballot words rw[0 .. nw) (the caller has made rw visible): the odd indices four (then
// two, then one) at a time -- one read of rw and independent gathers per chunk --, S_2j = S_j^2 by repeated squaring on the lane of the
// odd j.  Visible to the wave on return.
__device__ __forceinline__ void syndromes(const Gf &gf, const unsigned long long *rw, uint16_t *synd, int n, int nw, int t, int lane) {
    const int d0 = n - 1 - lane;                                  // the degree of this lane's position in chunk 0; negative: no position
    {
        int j = 1;
        for (; j + 6 < 2 * t; j += 8) syndrome_group<4>(gf, rw, synd, nw, j, d0, lane);
        if (j + 2 < 2 * t) { syndrome_group<2>(gf, rw, synd, nw, j, d0, lane); j += 4; }
        if (j < 2 * t) syndrome_group<1>(gf, rw, synd, nw, j, d0, lane);
    }
    wave_sync();
    if ((lane & 1) && lane < 2 * t) {                              // lane = odd j: S_2j, S_4j, ...
        unsigned v = synd[lane - 1];
        for (int jj = 2 * lane; jj <= 2 * t; jj *= 2) {
            v = gf.mul(v, v);
            synd[jj - 1] = (uint16_t)v;
        }
    }
    wave_sync();
}

// Berlekamp-Massey over synd[0 .. 2t): lane i ends with sigma's coefficient C_i, L is its length (degrees stay <= t <= 32: the first
// length above t is a failure at once); the discrepancy is an XOR across the wave.  Returns true for a failure: L > t, or sigma of a
// lower degree than its length (fewer than L roots).
__device__ __forceinline__ bool berlekamp_massey(const Gf &gf, const uint16_t *synd, int t, int lane, unsigned &sigma, int &length) {
    const int N = gf.N;
    // C the connection polynomial, Bp the one before the last length change, b its discrepancy, sh the shift
    unsigned C = lane == 0 ? 1u : 0u, Bp = C, b = 1u;
    int L = 0, sh = 1;
    bool fail = false;
    for (int r = 0; r < 2 * t; ++r) {
        const unsigned d = wave_xor(lane <= L ? gf.mul(C, synd[r - lane]) : 0u);
        if (d == 0u) { ++sh; continue; }
        int e = (int)gf.lg[d] - (int)gf.lg[b];
        if (e < 0) e += N;
        const unsigned coef = gf.ex[e];
        const unsigned moved = (unsigned)__shfl((int)Bp, lane >= sh ? lane - sh : lane);
        const unsigned next = C ^ gf.mul(coef, lane >= sh ? moved : 0u);
        if (2 * L <= r) {
            L = r + 1 - L;
            if (L > t) { fail = true; break; }
            Bp = C;
            b = d;
            sh = 1;
        } else {
            ++sh;
        }
        C = next;
    }
    if (!fail && __shfl((int)C, L) == 0) fail = true;             // sigma of a lower degree than its length: fewer than L roots
    sigma = C;
    length = L;
    return fail;
}

// Chien search of sigma (lane i <= L holds C_i) over the positions 0 .. n - 1, four chunks at a time: the lane of degree d evaluates
// sigma(alpha^-d); returns the number of roots.  LIST false: the ballot of a chunk's roots is its flip mask out[c] (64-bit words).
// LIST true: the positions of the roots go to out as uint16, ascending (at most L of them: sigma has degree L).  clog: 64 uint16 of
// scratch.
template <bool LIST>
__device__ __forceinline__ int chien_search(const Gf &gf, unsigned C, int L, uint16_t *clog, void *out, int n, int nw, int lane) {
    const int N = gf.N;
    int count = 0;
    if (lane <= L) clog[lane] = C ? gf.lg[C] : (uint16_t)0xFFFF;
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
            if (cl != 0xFFFF) {
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
            if (LIST) {
                const int at = count + __popcll(roots & ((1ull << lane) - 1ull));
                if (((roots >> lane) & 1ull) && at < 64) static_cast<uint16_t *>(out)[at] = (uint16_t)i;
            } else {
                if (lane == 0 && c0 + u < nw) static_cast<unsigned long long *>(out)[c0 + u] = roots;
            }
            count += __popcll(roots);
        }
    }
    return count;
}
#endif  // __HIPCC__

}  // namespace cpx
