// What the BCH kernels share (bch.hip: bounded-distance decoding of hard decisions, bch_chase.hip: Chase-II soft decoding) and
// Reed-Solomon codes have no use for: the handle, the limits, and the syndromes of a binary word, whose S_2j = S_j^2 halves the work.
// The field arithmetic, Berlekamp-Massey and the Chien search are those of cpx_gf.h.  Both kernels call this code, so a test pattern of
// the Chase decoder is decoded by exactly the rule of bch_decode_kernel, its failure conditions included.
#pragma once
#include "cpx_gf.h"

#define CPX_BCH_MAX_T 32
#define CPX_BCH_MAX_GEN_WORDS 7            // 64-bit words of a remainder: deg g <= 14 * 32 = 448

struct cpx_bch {
    __attribute__((visibility("hidden"))) ~cpx_bch() = default;
    int m, N, n, k, t, deg, device;
    uint64_t gen[CPX_BCH_MAX_GEN_WORDS];   // g without its leading term, bit j of word w = coefficient of x^(64 w + j)
    uint16_t *d_tab = nullptr;             // [2][2^m]: exp then log
};

namespace cpx {

#ifdef __HIPCC__
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
#endif  // __HIPCC__

}  // namespace cpx
