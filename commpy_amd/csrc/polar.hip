// Polar codes: encoder, successive cancellation (SC) and CRC-aided successive-cancellation list (SCL) decoding.
//
// Code: x = u F^{(x)n} over GF(2), F = [[1,0],[1,1]], natural order: x = (enc(u_a) ^ enc(u_b), enc(u_b)) for the two halves of u.  A decoder
// node with the LLRs l[0 .. 2M) therefore hands f(l[i], l[i + M]) to its left child, and g(l[i], l[i + M], xa[i]) to its right child once
// the left one has returned its re-encoded bits xa.  f is min-sum, g exact; both are float64 comparisons and one addition, and the
// library is built with -ffp-contract=off: every output equals tests/polar_model.py bit for bit.
//
// polar_decode_kernel<L>: one codeword per workgroup of four waves, all state in LDS (polar_lds below).
//   level s holds 2^s LLRs per path; level n = the channel LLRs, shared; level 0 = the decision LLR, kept in a register.
//   Bit phi recomputes the levels ctz(phi) .. 0 (all of them for phi = 0): level s from level s + 1, by g where bit s of phi is set.
//   Levels 1 .. n - 2 are stored (N / 2 - 2 values per path).  Level n - 1 -- half of what a path would need -- changes twice per word
//   and is read four times: it is recomputed from the channel LLRs wherever it is read (load_pair), by the same operations.
//   xl level s holds the 2^s re-encoded bits of the left child of the level-(s+1) node the walk is in.  After bit phi, with t' its number
//   of trailing ones, xl[t'] = the re-encoding of the last 2^t' bits: built in place, from u and xl[0 .. t').
//   Path r writes slot r of every level it recomputes; lidx / xidx say for each (level, path) which slot the path reads -- a fork copies
//   these bytes (two copies, flipped at every information bit), never an LLR array.
//   The bits of a path are not copied either: every information bit stores (parent rank, u) per rank, and the end walks back.
//   Levels with L 2^s >= 256 items run on all four waves with a workgroup barrier each; everything below -- most steps -- runs on wave 0
//   alone, ordered by LDS fences (a wave's LDS operations complete in order), while the other waves wait at the next barrier.
//   The list sort: candidate c = 2 rank + u sits on lane c; its rank is the number of candidates with a smaller (key, c), where key is
//   the metric's bit pattern mapped to an unsigned total order (NaN last).  (key, c) pairs are distinct, so the ranks are a permutation
//   whatever the LLRs are.
// polar_encode_kernel: one codeword per wave, bit-packed: u is gathered 64 positions at a time by ballot, the stages of span < 64 are
//   shifts and masks inside a word, the wider ones exchange words across lanes (and between a lane's two words at N = 8192).
#include "cpx_internal.h"
#include "cpx_wave.h"

#include <mutex>

using namespace cpx;

#define CPX_POLAR_MAX_N 8192        // and L * N <= 8192: 64 KiB of path LLRs
#define CPX_POLAR_MAX_L 32
#define CPX_POLAR_LDS_MAX (160 * 1024)
#define POLAR_THREADS 256
#define POLAR_ENC_THREADS 64

struct cpx_polar {
    __attribute__((visibility("hidden"))) ~cpx_polar() = default;
    int N, n, K, A, crc_bits, device;
    uint64_t *d_frozen = nullptr;    // [max(N / 64, 1)] bit i of the mask at bit (i & 63) of word i >> 6
    int32_t *d_rank = nullptr;       // [N] index of the information bit at this position, -1: frozen
    uint32_t *d_crc = nullptr;       // [K] x^(K-1-k) mod g; null without a CRC
};

namespace {

struct PolarArgs {
    const double *llr;               // [B][N]
    const uint64_t *frozen;
    const uint32_t *crc;
    int64_t B;
    int N, n, K, A, crc_bits;
    uint8_t *bits, *crc_ok;          // [B][A], [B]
    double *metric, *u_llr;          // [B], [B][N]
    uint8_t *list_bits;              // [B][L][K]
    double *list_metric;             // [B][L]
    int32_t *list_live;              // [B]
};

// byte offsets of the decoder's LDS arrays
struct PolarLds {
    unsigned chan, llr, pm, npm, fz, crcacc, hist, xl, lidx, xidx, npar, nbit, total;
};
__host__ __device__ inline PolarLds polar_lds(int N, int n, int K, int L) {
    PolarLds o;
    unsigned at = 0;
    o.chan = at;   at += 8u * N;                    // channel LLRs
    o.llr = at;    at += N > 4 ? 8u * L * (N / 2 - 2) : 0u;   // levels 1 .. n - 2: level s at L (2^s - 2), slot r at r 2^s
    o.pm = at;     at += 8u * L;                    // path metrics by rank
    o.npm = at;    at += 8u * L;                    // ... of the sorted candidates
    o.fz = at;     at += 8u * ((N + 63) / 64);      // frozen mask
    o.crcacc = at; at += 4u * L;                    // CRC remainder per rank
    o.hist = at;   at += (unsigned)K * L;           // [K][L] parent rank | u << 7; after the walk back: the bits of rank r
    o.xl = at;     at += (unsigned)L * (N - 1);     // level s at L (2^s - 1), slot r at r 2^s
    o.lidx = at;   at += 2u * n * L;                // [2][n][L]
    o.xidx = at;   at += 2u * n * L;
    o.npar = at;   at += L;
    o.nbit = at;   at += L;
    o.total = (at + 15u) & ~15u;
    return o;
}

__device__ __forceinline__ double polar_f(double a, double b) {
    const double fa = fabs(a), fb = fabs(b);
    const double m = (fa < fb || fa != fa) ? fa : fb;          // min that keeps a NaN of either side
    return ((a < 0.0) != (b < 0.0)) ? -m : m;
}
__device__ __forceinline__ double polar_g(double a, double b, int u) { return u ? b - a : b + a; }

// unsigned key with the order of the float64 values, -0.0 below +0.0 and every NaN last
__device__ __forceinline__ unsigned long long polar_key(double m) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(m);
    if (m != m) return ~0ull;
    return (b >> 63) ? ~b : (b | (1ull << 63));
}

// the LDS operations of this wave issued so far are complete and visible to its other lanes
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __builtin_amdgcn_wave_barrier();
}

struct PolarState {
    double *chan, *llr, *pm;
    uint8_t *xl, *lidx, *xidx;       // lidx / xidx: the current copy
    int n;
};

// the slot a path reads at a level; the only path of L = 1 lives in slot 0 and keeps no table
template <int L>
__device__ __forceinline__ int slot_of(const uint8_t *idx, int at) { return L == 1 ? 0 : (int)idx[at]; }

// the values i and i + 2^(lvl - 1) of level lvl (1 <= lvl <= n) of path r.  Level n - 1 is not stored: it is f, or g with xl[n - 1], of
// the channel LLRs, computed here by the same operations whenever level n - 2 (or, for N = 4, the decision) is.
// SRC says which case lvl is, so that the stored levels -- nearly every call -- carry no test: 0 stored, 1 level n - 1, 2 the channel.
template <int L, int SRC>
__device__ __forceinline__ void load_pair(const PolarState &st, int lvl, int r, int i, int phi, double &a, double &b) {
    const int half = 1 << (lvl - 1);
    if (SRC == 2) {
        a = st.chan[i];
        b = st.chan[i + half];
    } else if (SRC == 1) {
        const int H = 1 << lvl;
        const double a0 = st.chan[i], b0 = st.chan[i + H], a1 = st.chan[i + half], b1 = st.chan[i + half + H];
        if ((phi >> lvl) & 1) {
            const uint8_t *x = st.xl + L * (H - 1) + (slot_of<L>(st.xidx, lvl * L + r) << lvl);
            a = polar_g(a0, b0, x[i]);
            b = polar_g(a1, b1, x[i + half]);
        } else {
            a = polar_f(a0, b0);
            b = polar_f(a1, b1);
        }
    } else {
        const double *src = st.llr + L * (2 * half - 2) + (slot_of<L>(st.lidx, lvl * L + r) << lvl);
        a = src[i];
        b = src[i + half];
    }
}

// level s (1 <= s <= n - 2) of every live path from level s + 1, by the threads tid, tid + nthr, ...
template <int L, int SRC>
__device__ __forceinline__ void llr_level(const PolarState &st, int s, int phi, int live, int tid, int nthr) {
    const int half = 1 << s, items = live << s, use_g = (phi >> s) & 1;
    for (int it = tid; it < items; it += nthr) {
        const int r = it >> s, i = it & (half - 1);
        double a, b;
        load_pair<L, SRC>(st, s + 1, r, i, phi, a, b);
        double v;
        if (use_g) v = polar_g(a, b, st.xl[L * (half - 1) + (slot_of<L>(st.xidx, s * L + r) << s) + i]);
        else v = polar_f(a, b);
        st.llr[L * (half - 2) + (r << s) + i] = v;
        if (L > 1 && i == 0) st.lidx[s * L + r] = (uint8_t)r;
    }
}

// step s of building xl[tp] in place: (x[0 .. 2^s)) -> (xl[s] ^ x, x)
template <int L>
__device__ __forceinline__ void xl_step(const PolarState &st, int s, int tp, int live, int tid, int nthr) {
    const int half = 1 << s, items = live << s;
    for (int it = tid; it < items; it += nthr) {
        const int r = it >> s, i = it & (half - 1);
        uint8_t *dst = st.xl + L * ((1 << tp) - 1) + (r << tp);
        const uint8_t x = dst[i];
        const uint8_t l = st.xl[L * (half - 1) + (slot_of<L>(st.xidx, s * L + r) << s) + i];
        dst[i] = l ^ x;
        dst[i + half] = x;
    }
}

template <int L>
__global__ __launch_bounds__(POLAR_THREADS) void polar_decode_kernel(PolarArgs a) {
    extern __shared__ double2 polar_lds_raw[];
    unsigned char *base = reinterpret_cast<unsigned char *>(polar_lds_raw);
    const int N = a.N, n = a.n, K = a.K, A = a.A;
    const PolarLds o = polar_lds(N, n, K, L);
    double *chan = reinterpret_cast<double *>(base + o.chan), *pm = reinterpret_cast<double *>(base + o.pm);
    double *npm = reinterpret_cast<double *>(base + o.npm);
    uint64_t *fz = reinterpret_cast<uint64_t *>(base + o.fz);
    unsigned *crcacc = reinterpret_cast<unsigned *>(base + o.crcacc);
    uint8_t *hist = base + o.hist, *npar = base + o.npar, *nbit = base + o.nbit;
    const int tid = threadIdx.x;
    const bool w0 = tid < 64;
    constexpr int WIDE = POLAR_THREADS;                           // a level of L 2^s >= WIDE items runs on every wave

    for (int64_t cw = blockIdx.x; cw < a.B; cw += gridDim.x) {
        __syncthreads();                                          // the previous codeword's outputs have been read
        for (int i = tid; i < N; i += POLAR_THREADS) chan[i] = a.llr[cw * N + i];
        for (int i = tid; i < (N + 63) / 64; i += POLAR_THREADS) fz[i] = a.frozen[i];
        if (tid < L) { pm[tid] = 0.0; crcacc[tid] = 0u; }
        __syncthreads();
        PolarState st;
        st.chan = chan;
        st.llr = reinterpret_cast<double *>(base + o.llr);
        st.pm = pm;
        st.xl = base + o.xl;
        st.n = n;
        int live = 1, k = 0, cur = 0;
        uint64_t fw = 0;
        for (int phi = 0; phi < N; ++phi) {
            if ((phi & 63) == 0) fw = fz[phi >> 6];
            const bool frozen = (fw >> (phi & 63)) & 1;
            st.lidx = base + o.lidx + cur * n * L;
            st.xidx = base + o.xidx + cur * n * L;
            int s = phi ? __builtin_ctz((unsigned)phi) : n - 1;
            if (s > n - 2) s = n - 2;                             // level n - 1 is computed in flight (load_pair)
            for (; s >= 1 && (L << s) >= WIDE; --s) {
                if (s == n - 2) llr_level<L, 1>(st, s, phi, live, tid, POLAR_THREADS);
                else llr_level<L, 0>(st, s, phi, live, tid, POLAR_THREADS);
                __syncthreads();
            }
            const int tp = __builtin_ctz(~(unsigned)phi);         // trailing ones of phi = ctz(phi + 1)
            const int newlive = (frozen || 2 * live > L) ? (frozen ? live : L) : 2 * live;
            if (w0) {
                for (; s >= 1; --s) {
                    if (s == n - 2) llr_level<L, 1>(st, s, phi, live, tid, 64);
                    else llr_level<L, 0>(st, s, phi, live, tid, 64);
                    wave_sync();
                }
                // the decision LLR of path r on lanes 2r and 2r + 1
                const int c = tid, r = c >> 1, u = c & 1;
                const bool act = c < 2 * live;
                double lam = 0.0;
                if (act) {
                    double x, y;
                    if (n > 2) load_pair<L, 0>(st, 1, r, 0, phi, x, y);
                    else if (n == 2) load_pair<L, 1>(st, 1, r, 0, phi, x, y);
                    else load_pair<L, 2>(st, 1, r, 0, phi, x, y);
                    lam = (phi & 1) ? polar_g(x, y, st.xl[slot_of<L>(st.xidx, r)]) : polar_f(x, y);
                    if (L == 1 && a.u_llr && c == 0) a.u_llr[cw * N + phi] = lam;
                }
                const bool hard = lam < 0.0;
                int mybit = 0;                                    // the bit of the new path of rank tid
                if (frozen) {
                    if (act && u == 0 && hard) pm[r] = pm[r] + fabs(lam);
                } else if (L == 1) {
                    mybit = hard;                                 // lane 0: the only path
                    if (c == 0) hist[k] = hard;
                } else {
                    const double m = act ? pm[r] : 0.0;
                    const double cm = (u != (int)hard) ? m + fabs(lam) : m;
                    const unsigned long long key = act ? polar_key(cm) : ~0ull;
                    // lanes past 2 live hold the last key and a higher index: they count for nobody
                    const int klo = (int)(unsigned)key, khi = (int)(unsigned)(key >> 32);
                    int rank = 0;
#pragma unroll
                    for (int j = 0; j < 2 * L; ++j) {
                        const unsigned long long kj = ((unsigned long long)(unsigned)__builtin_amdgcn_readlane(khi, j) << 32) |
                                                      (unsigned)__builtin_amdgcn_readlane(klo, j);
                        rank += (kj < key || (kj == key && j < c)) ? 1 : 0;
                    }
                    if (act && rank < newlive) { npar[rank] = (uint8_t)r; nbit[rank] = (uint8_t)u; npm[rank] = cm; }
                    wave_sync();
                    if (c < newlive) {
                        mybit = nbit[c];
                        pm[c] = npm[c];
                        hist[k * L + c] = (uint8_t)(npar[c] | (mybit << 7));
                    }
                    uint8_t *nl = base + o.lidx + (cur ^ 1) * n * L, *nx = base + o.xidx + (cur ^ 1) * n * L;
                    for (int it = c; it < n * L; it += 64) {
                        const int rr = it & (L - 1);
                        if (rr < newlive) {
                            const int src = (it - rr) + npar[rr];
                            nl[it] = st.lidx[src];
                            nx[it] = st.xidx[src];
                        }
                    }
                    st.lidx = nl;
                    st.xidx = nx;
                }
                // xl[tp] of every new path: its bit (in slot tid, behind the copied table entry), then the narrow steps
                if (tp < n && tid < newlive) {
                    st.xl[L * ((1 << tp) - 1) + (tid << tp)] = (uint8_t)mybit;
                    if (L > 1) st.xidx[tp * L + tid] = (uint8_t)tid;
                }
                wave_sync();
                for (int q = 0; q < tp && tp < n && (L << q) < WIDE; ++q) {
                    xl_step<L>(st, q, tp, newlive, tid, 64);
                    wave_sync();
                }
            }
            if (!frozen) {
                ++k;
                if (L > 1) cur ^= 1;
            }
            live = newlive;
            st.lidx = base + o.lidx + cur * n * L;
            st.xidx = base + o.xidx + cur * n * L;
            if (phi + 1 < N && (L << tp) >= WIDE) {               // wide work follows: the rest of xl[tp], or level tp of bit phi + 1
                __syncthreads();
                int q = 0;
                while ((L << q) < WIDE) ++q;
                for (; q < tp; ++q) {
                    xl_step<L>(st, q, tp, live, tid, POLAR_THREADS);
                    __syncthreads();
                }
            }
        }
        // walk back: row k of hist becomes the k-th information bit of every rank
        if (w0 && L > 1) {
            int at = tid;
            for (int kk = K - 1; kk >= 0; --kk) {
                const int h = tid < live ? hist[kk * L + at] : 0;
                wave_sync();
                if (tid < live) hist[kk * L + tid] = (uint8_t)(h >> 7);
                at = h & (L - 1);
            }
        }
        __syncthreads();
        if (a.crc_bits) {
            const int r = tid & (L - 1);
            unsigned acc = 0;
            for (int kk = tid / L; kk < K; kk += POLAR_THREADS / L)
                if (r < live && hist[kk * L + r]) acc ^= a.crc[kk];
            if (acc) atomicXor(&crcacc[r], acc);
            __syncthreads();
        }
        int chosen = 0, ok = 1;
        if (a.crc_bits) {
            ok = 0;
            for (int r = live - 1; r >= 0; --r)
                if (crcacc[r] == 0u) { chosen = r; ok = 1; }
        }
        if (a.bits)
            for (int kk = tid; kk < A; kk += POLAR_THREADS) a.bits[cw * A + kk] = hist[kk * L + chosen];
        if (tid == 0) {
            if (a.crc_ok) a.crc_ok[cw] = (uint8_t)ok;
            if (a.metric) a.metric[cw] = pm[chosen];
            if (a.list_live) a.list_live[cw] = live;
        }
        if (a.list_metric && tid < L) a.list_metric[cw * L + tid] = tid < live ? pm[tid] : __builtin_inf();
        if (a.list_bits)
            for (int it = tid; it < L * K; it += POLAR_THREADS) {
                const int r = it / K, kk = it - r * K;
                a.list_bits[(cw * L + r) * K + kk] = r < live ? hist[kk * L + r] : (uint8_t)0;
            }
    }
}

struct PolarEncArgs {
    const uint8_t *msg;              // [B][A]
    const int32_t *rank;
    const uint32_t *crc;
    uint8_t *x;                      // [B][N]
    int64_t B;
    int N, K, A, crc_bits;
};

__global__ __launch_bounds__(POLAR_ENC_THREADS) void polar_encode_kernel(PolarEncArgs a) {
    const int lane = threadIdx.x, N = a.N, K = a.K, A = a.A;
    const int W = (N + 63) / 64;                                  // words of a codeword: lane j holds words j and j + 64
    for (int64_t cw = blockIdx.x; cw < a.B; cw += gridDim.x) {
        const uint8_t *m = a.msg + cw * A;
        unsigned crc = 0;
        if (a.crc_bits) {
            for (int k = lane; k < A; k += 64)
                if (m[k] & 1) crc ^= a.crc[k];
            for (int d = 32; d >= 1; d >>= 1) crc ^= (unsigned)__shfl_xor((int)crc, d);
        }
        unsigned long long x[2] = {0ull, 0ull};
        for (int w = 0; w < W; ++w) {
            const int i = w * 64 + lane;
            int bit = 0;
            if (i < N) {
                const int rk = a.rank[i];
                if (rk >= 0) bit = rk < A ? (m[rk] & 1) : (int)((crc >> (K - 1 - rk)) & 1u);
            }
            const unsigned long long word = __ballot(bit);
            if ((w & 63) == lane) x[w >> 6] = word;
        }
        for (int q = 0; q < 2; ++q) {
            unsigned long long v = x[q];
            v ^= (v >> 1) & 0x5555555555555555ull;
            v ^= (v >> 2) & 0x3333333333333333ull;
            v ^= (v >> 4) & 0x0F0F0F0F0F0F0F0Full;
            v ^= (v >> 8) & 0x00FF00FF00FF00FFull;
            v ^= (v >> 16) & 0x0000FFFF0000FFFFull;
            v ^= (v >> 32) & 0x00000000FFFFFFFFull;
            x[q] = v;
        }
        for (int d = 1; d < W && d < 64; d <<= 1)
            for (int q = 0; q < 2; ++q) {
                const unsigned long long v = __shfl_xor(x[q], d);
                if (!(lane & d)) x[q] ^= v;
            }
        if (W > 64) x[0] ^= x[1];
        uint8_t *out = a.x + cw * N;
        for (int w = 0; w < W; ++w) {
            const unsigned long long word = __shfl(x[w >> 6], w & 63);
            const int i = w * 64 + lane;
            if (i < N) out[i] = (uint8_t)((word >> lane) & 1ull);
        }
    }
}

template <int L>
int launch_decode(const PolarArgs &a, unsigned lds, hipStream_t st) {
    static std::mutex raised_mu;
    static bool raised[64] = {};
    int dev = 0;
    (void)hipGetDevice(&dev);
    {
        std::lock_guard<std::mutex> lk(raised_mu);
        if (dev >= 0 && dev < 64 && !raised[dev]) {
            CPX_HIP(hipFuncSetAttribute((const void *)polar_decode_kernel<L>, hipFuncAttributeMaxDynamicSharedMemorySize, CPX_POLAR_LDS_MAX));
            raised[dev] = true;
        }
    }
    hipLaunchKernelGGL(polar_decode_kernel<L>, dim3(grid_of(a.B, (int64_t)device_cus() * 8)), dim3(POLAR_THREADS), lds, st, a);
    CPX_HIP(hipGetLastError());
    note_kernel("polar_decode_kernel<%d>", L);
    return CPX_OK;
}

int decode_check(const cpx_polar *p, int64_t B, int L, const void *u_llr, bool any_out) {
    CPX_REQUIRE(p, CPX_EINVAL, "polar_decode: null handle");
    CPX_REQUIRE(B >= 0, CPX_EINVAL, "polar_decode: B = %lld", (long long)B);
    CPX_REQUIRE(L >= 1 && (L & (L - 1)) == 0, CPX_EINVAL, "polar_decode: list size %d, need a power of two", L);
    CPX_REQUIRE(L <= CPX_POLAR_MAX_L, CPX_ELIMIT, "polar_decode: list size %d is above the engine's limit of %d", L, CPX_POLAR_MAX_L);
    CPX_REQUIRE(L * p->N <= CPX_POLAR_MAX_N, CPX_ELIMIT, "polar_decode: L * N = %d * %d is above the engine's limit of %d", L, p->N,
                CPX_POLAR_MAX_N);
    CPX_REQUIRE(polar_lds(p->N, p->n, p->K, L).total <= CPX_POLAR_LDS_MAX, CPX_ELIMIT, "polar_decode: N = %d, L = %d needs %u bytes of LDS",
                p->N, L, polar_lds(p->N, p->n, p->K, L).total);
    CPX_REQUIRE(!u_llr || L == 1, CPX_EINVAL, "polar_decode: u_llr is defined for L = 1 only");
    CPX_REQUIRE(any_out, CPX_EINVAL, "polar_decode: no output requested");
    return CPX_OK;
}

int encode_check(const cpx_polar *p, int64_t B) {
    CPX_REQUIRE(p, CPX_EINVAL, "polar_encode: null handle");
    CPX_REQUIRE(B >= 0, CPX_EINVAL, "polar_encode: B = %lld", (long long)B);
    return CPX_OK;
}

}  // namespace

extern "C" {

int cpx_polar_create(int N, const uint8_t *frozen, int crc_bits, const uint32_t *crc_table, cpx_polar **out) {
    CPX_TRACE("cpx_polar_create");
    CPX_REQUIRE(out, CPX_EINVAL, "polar: null pointer");
    *out = nullptr;
    CPX_REQUIRE(N >= 2 && (N & (N - 1)) == 0, CPX_EINVAL, "polar: N = %d, need a power of two >= 2", N);
    CPX_REQUIRE(N <= CPX_POLAR_MAX_N, CPX_ELIMIT, "polar: N = %d is above the engine's limit of %d", N, CPX_POLAR_MAX_N);
    CPX_REQUIRE(frozen, CPX_EINVAL, "polar: null pointer");
    std::vector<uint64_t> words((size_t)(N + 63) / 64, 0);
    std::vector<int32_t> rank((size_t)N, -1);
    int K = 0;
    for (int i = 0; i < N; ++i) {
        CPX_REQUIRE(frozen[i] <= 1, CPX_EINVAL, "polar: frozen[%d] = %d, need 0 or 1", i, (int)frozen[i]);
        if (frozen[i]) words[(size_t)i >> 6] |= 1ull << (i & 63);
        else rank[(size_t)i] = K++;
    }
    CPX_REQUIRE(K >= 1, CPX_EINVAL, "polar: every position is frozen");
    CPX_REQUIRE(crc_bits >= 0 && crc_bits <= 32, CPX_EINVAL, "polar: crc_bits = %d, need 0 .. 32", crc_bits);
    CPX_REQUIRE(crc_bits < K, CPX_EINVAL, "polar: crc_bits = %d, need fewer than the K = %d information bits", crc_bits, K);
    CPX_REQUIRE((crc_bits > 0) == (crc_table != nullptr), CPX_EINVAL, "polar: a CRC table goes with crc_bits > 0, and only with it");
    for (int k = 0; k < K && crc_bits; ++k) {
        const uint32_t v = crc_table[k];
        CPX_REQUIRE(v != 0 && (crc_bits == 32 || (v >> crc_bits) == 0), CPX_EINVAL, "polar: crc_table[%d] = 0x%x is no remainder of degree < %d",
                    k, v, crc_bits);
        CPX_REQUIRE(k < K - crc_bits || v == (1u << (K - 1 - k)), CPX_EINVAL, "polar: crc_table[%d] = 0x%x, need x^%d = 0x%x", k, v, K - 1 - k,
                    1u << (K - 1 - k));
    }
    int rc = ensure_device();
    if (rc) return rc;
    cpx_polar *p = new cpx_polar();
    p->N = N;
    p->n = __builtin_ctz((unsigned)N);
    p->K = K;
    p->A = K - crc_bits;
    p->crc_bits = crc_bits;
    (void)hipGetDevice(&p->device);
    if ((rc = upload((void **)&p->d_frozen, words.data(), sizeof(uint64_t) * words.size(), "polar")) ||
        (rc = upload((void **)&p->d_rank, rank.data(), sizeof(int32_t) * rank.size(), "polar")) ||
        (crc_bits && (rc = upload((void **)&p->d_crc, crc_table, sizeof(uint32_t) * (size_t)K, "polar")))) {
        cpx_polar_destroy(p);
        return rc;
    }
    *out = p;
    return CPX_OK;
}

int cpx_polar_destroy(cpx_polar *p) {
    if (!p) return CPX_OK;
    (void)hipFree(p->d_frozen);
    (void)hipFree(p->d_rank);
    (void)hipFree(p->d_crc);
    delete p;
    return CPX_OK;
}

int cpx_polar_encode_dev(const cpx_polar *p, const uint8_t *d_msg, int64_t B, uint8_t *d_x, void *stream) {
    CPX_TRACE("cpx_polar_encode_dev");
    if (int rc = encode_check(p, B)) return rc;
    if (B == 0) return CPX_OK;
    CPX_REQUIRE(d_msg && d_x, CPX_EINVAL, "polar_encode: null pointer");
    if (int rcd = check_handle_device(p->device, "polar_encode")) return rcd;
    PolarEncArgs a{d_msg, p->d_rank, p->d_crc, d_x, B, p->N, p->K, p->A, p->crc_bits};
    hipLaunchKernelGGL(polar_encode_kernel, dim3(grid_of(B, (int64_t)device_cus() * 32)), dim3(POLAR_ENC_THREADS), 0, pick_stream(stream), a);
    CPX_HIP(hipGetLastError());
    note_kernel("polar_encode_kernel");
    return CPX_OK;
}

int cpx_polar_encode(const cpx_polar *p, const uint8_t *msg, int64_t B, uint8_t *x) {
    CPX_TRACE("cpx_polar_encode");
    if (int rc = encode_check(p, B)) return rc;
    if (B == 0) return CPX_OK;
    CPX_REQUIRE(msg && x, CPX_EINVAL, "polar_encode: null pointer");
    int rc = ensure_device();
    if (rc) return rc;
    const size_t in_bytes = (size_t)B * (size_t)p->A, out_bytes = (size_t)B * (size_t)p->N;
    HostStage s;
    const uint8_t *din;
    uint8_t *dout;
    if ((rc = s.in(msg, in_bytes, &din)) || (rc = s.out(out_bytes, &dout)) || (rc = cpx_polar_encode_dev(p, din, B, dout, s.st))) return rc;
    return s.get(x, dout, out_bytes);
}

int cpx_polar_decode_dev(const cpx_polar *p, const double *d_llr, int64_t B, int L, uint8_t *d_bits, uint8_t *d_crc_ok, double *d_metric,
                         double *d_u_llr, uint8_t *d_list_bits, double *d_list_metric, int32_t *d_list_live, void *stream) {
    CPX_TRACE("cpx_polar_decode_dev");
    if (int rc = decode_check(p, B, L, d_u_llr, d_bits || d_crc_ok || d_metric || d_u_llr || d_list_bits || d_list_metric || d_list_live))
        return rc;
    if (B == 0) return CPX_OK;
    CPX_REQUIRE(d_llr, CPX_EINVAL, "polar_decode: null pointer");
    if (int rcd = check_handle_device(p->device, "polar_decode")) return rcd;
    PolarArgs a{d_llr, p->d_frozen, p->d_crc, B, p->N, p->n, p->K, p->A, p->crc_bits, d_bits, d_crc_ok, d_metric, d_u_llr, d_list_bits,
                d_list_metric, d_list_live};
    const unsigned lds = polar_lds(p->N, p->n, p->K, L).total;
    hipStream_t st = pick_stream(stream);
    switch (L) {
    case 1: return launch_decode<1>(a, lds, st);
    case 2: return launch_decode<2>(a, lds, st);
    case 4: return launch_decode<4>(a, lds, st);
    case 8: return launch_decode<8>(a, lds, st);
    case 16: return launch_decode<16>(a, lds, st);
    default: return launch_decode<32>(a, lds, st);
    }
}

int cpx_polar_decode(const cpx_polar *p, const double *llr, int64_t B, int L, uint8_t *bits, uint8_t *crc_ok, double *metric, double *u_llr,
                     uint8_t *list_bits, double *list_metric, int32_t *list_live) {
    CPX_TRACE("cpx_polar_decode");
    if (int rc = decode_check(p, B, L, u_llr, bits || crc_ok || metric || u_llr || list_bits || list_metric || list_live)) return rc;
    if (B == 0) return CPX_OK;
    CPX_REQUIRE(llr, CPX_EINVAL, "polar_decode: null pointer");
    int rc = ensure_device();
    if (rc) return rc;
    const size_t b = (size_t)B;
    HostStage::Out outs[7] = {{bits, b * (size_t)p->A},
                              {crc_ok, b},
                              {metric, 8 * b},
                              {u_llr, 8 * b * (size_t)p->N},
                              {list_bits, b * (size_t)L * (size_t)p->K},
                              {list_metric, 8 * b * (size_t)L},
                              {list_live, 4 * b}};
    HostStage s;
    const double *din;
    if ((rc = s.in(llr, 8 * b * (size_t)p->N, &din)) || (rc = s.out(outs))) return rc;
    if ((rc = cpx_polar_decode_dev(p, din, B, L, outs[0].as<uint8_t>(), outs[1].as<uint8_t>(), outs[2].as<double>(), outs[3].as<double>(),
                                   outs[4].as<uint8_t>(), outs[5].as<double>(), outs[6].as<int32_t>(), s.st)))
        return rc;
    return s.get(outs);
}

}  // extern "C"
