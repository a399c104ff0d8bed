// OFDM transmit / receive (ofdm_tx / ofdm_rx, commpy/modulation.py:265-296), batched, float64 only.
//
//   TX, per symbol s:  F = zeros(N); F[1:h+1] = x[s][h:]; F[N-h:] = x[s][:h] (the second write wins where they overlap);
//                      t = ifft(F); out[s] = t[N-P:] ++ t, with P = cp if 0 < cp < N else N (the reference's t[-cp:])
//   RX, per symbol s:  X = fft(y[s S + cp : s S + cp + N]), S = N + cp; out[s] = X[N-h:] ++ X[1:h+1]
//
// Two kernels, chosen by the plan (no process-wide switch):
//   ofdm_fast_kernel<LOGN, TX>  power-of-two N from 2 to 8192.  A Stockham (autosort) FFT whose passes do radix-8 butterflies
//       in registers (radix 16 at N = 8192; the first pass takes the radix left over), so a symbol crosses the LDS once per
//       pass.  The first pass reads its operands from HBM through the bin map (TX) or past the prefix (RX).  The last pass
//       stores to the LDS, from where the workgroup writes its symbols' outputs as one contiguous run (TX: prefix and body of
//       every symbol, the prefix read from the LDS image; RX: the nsc used bins in output order).  A workgroup holds
//       max(N, 4096) points, i.e. 4096 / N symbols for small N, one butterfly's values per thread.  LDS layout: one double2
//       of padding after every 16, so that the strided stores of the early passes (stride R * 16 B) spread over the banks.
//       The twiddles of a butterfly: W^(step r) for the powers of two of r from the table, the others as their products.
//   ofdm_dft_kernel<TX>  every other accepted N (any size up to 65536): a direct DFT over the plan's twiddle table, one
//       workgroup per symbol, the input streamed through the LDS in chunks, each thread summing 4 output bins in index order.
//
// Twiddles: W[k] = e^{-2 pi i k / N}, computed once on the host in long double from angles reduced exactly to the nearest
// quarter turn (integer arithmetic), and kept by the plan.  The inverse transform uses their conjugates and scales by 1/N.
// Every symbol goes through the same operations wherever it sits in the batch: outputs are bit-identical across batch sizes,
// positions and streams.  Offsets are 64-bit.
#include "cpx_internal.h"
#include "cpx_wave.h"             // grid_of

#include <climits>
#include <cmath>

using namespace cpx;

#define CPX_OFDM_MAX_NFFT 65536

struct cpx_ofdm {
    __attribute__((visibility("hidden"))) ~cpx_ofdm() = default;
    int nfft, nsc, cp, P, h;
    int logn;              // log2(nfft) when the fast kernel serves this size, else -1 (direct DFT)
    int device;
    double2 *d_tw = nullptr;   // [nfft] e^{-2 pi i k / nfft}
};

namespace {

struct OfdmArgs {
    const double2 *in;     // TX: x [nsym][nsc]; RX: y [B][ny]
    double2 *out;          // TX: [nsym][P + N]; RX: [nsym][nsc]
    const double2 *tw;     // [N]
    int64_t nsym;          // symbols in the whole batch
    int64_t rows;          // RX: symbols per row of y (ny / S)
    int64_t ny;            // RX: samples per row of y
    int nsc, h, cp, P;
};

__device__ __forceinline__ double2 cmul(double2 a, double2 w) { return make_double2(a.x * w.x - a.y * w.y, a.x * w.y + a.y * w.x); }
__device__ __forceinline__ double2 cmul_conj(double2 a, double2 w) { return make_double2(a.x * w.x + a.y * w.y, a.y * w.x - a.x * w.y); }
__device__ __forceinline__ double2 cadd(double2 a, double2 b) { return make_double2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ double2 csub(double2 a, double2 b) { return make_double2(a.x - b.x, a.y - b.y); }

// e^{-2 pi i m / 16}, m = 0..7: the twiddles of the in-register butterflies
__device__ constexpr double W16_RE[8] = {1.0, 0.92387953251128674, 0.70710678118654757, 0.38268343236508978,
                                         0.0, -0.38268343236508978, -0.70710678118654757, -0.92387953251128674};
__device__ constexpr double W16_IM[8] = {-0.0, -0.38268343236508978, -0.70710678118654757, -0.92387953251128674,
                                         -1.0, -0.92387953251128674, -0.70710678118654757, -0.38268343236508978};

// v * e^{-+2 pi i m / 16} (INV: the conjugate), m known at compile time after unrolling
template <bool INV>
__device__ __forceinline__ double2 rot16(double2 v, int m) {
    if (m == 0) return v;
    if (m == 4) return INV ? make_double2(-v.y, v.x) : make_double2(v.y, -v.x);
    const double2 w = make_double2(W16_RE[m], INV ? -W16_IM[m] : W16_IM[m]);
    return cmul(v, w);
}

constexpr int bitrev(int i, int bits) {
    int r = 0;
    for (int b = 0; b < bits; b++) r |= ((i >> b) & 1) << (bits - 1 - b);
    return r;
}
constexpr int ilog2(int r) { return r <= 1 ? 0 : 1 + ilog2(r / 2); }

// R-point DFT of v in registers (R = 2..16): radix-2 decimation in frequency, then the bit-reversal permutation
template <int R, bool INV>
__device__ __forceinline__ void dft_regs(double2 (&v)[R]) {
#pragma unroll
    for (int half = R / 2; half >= 1; half /= 2) {
#pragma unroll
        for (int start = 0; start < R; start += 2 * half) {
#pragma unroll
            for (int k = 0; k < half; k++) {
                const double2 a = v[start + k], b = v[start + k + half];
                v[start + k] = cadd(a, b);
                v[start + k + half] = rot16<INV>(csub(a, b), k * (8 / half));
            }
        }
    }
    double2 t[R];
#pragma unroll
    for (int i = 0; i < R; i++) t[i] = v[bitrev(i, ilog2(R))];
#pragma unroll
    for (int i = 0; i < R; i++) v[i] = t[i];
}

// radix of the passes but the first = complex values per thread and pass: 8, and 16 at N = 8192, where a symbol fills the
// workgroup and 8 values per thread would take 1024 threads (128 VGPRs each, too few)
constexpr int of_logr(int logn) { return logn == 13 ? 4 : 3; }
constexpr int OF_TILE = 4096;     // points per workgroup at least (several symbols for N < 4096)
constexpr int of_block(int logn) { return ((1 << logn) > OF_TILE ? (1 << logn) : OF_TILE) >> of_logr(logn); }
constexpr int of_pad(int i) { return i + (i >> 4); }

template <int LOGN>
struct FastShape {
    static constexpr int N = 1 << LOGN;
    static constexpr int BLOCK = of_block(LOGN);
    static constexpr int LOGR = of_logr(LOGN), RMAX = 1 << LOGR, PTS = RMAX;
    static constexpr int SPW = BLOCK * PTS / N;                    // symbols per workgroup
    static constexpr int NPAD = of_pad(N);                         // LDS stride of a symbol
    static constexpr int R0 = (LOGN % LOGR) ? (1 << (LOGN % LOGR)) : RMAX;  // radix of the first pass
    static constexpr int LDS = SPW * NPAD;
};

// operand k (0 <= k < N) of symbol s for the first pass: TX the bin map over x, RX the samples past the prefix
template <int N, bool TX>
__device__ __forceinline__ double2 first_operand(const OfdmArgs &a, const double2 *src, int k) {
    if (TX) {
        if (k >= N - a.h) return src[k - (N - a.h)];
        if (k >= 1 && k <= a.h) return src[a.h + k - 1];
        return make_double2(0.0, 0.0);
    }
    return src[k];
}

template <int N, bool TX>
__device__ __forceinline__ const double2 *symbol_input(const OfdmArgs &a, int64_t s) {
    if (TX) return a.in + s * a.nsc;
    const int64_t b = s / a.rows, i = s - b * a.rows;
    return a.in + b * a.ny + i * (int64_t)(N + a.cp) + a.cp;
}

// sample / bin n of symbol s, written straight to HBM (direct DFT)
template <bool TX>
__device__ __forceinline__ void store_output(const OfdmArgs &a, int N, int64_t s, int n, double2 v) {
    if (TX) {
        double2 *o = a.out + s * (int64_t)(a.P + N);
        o[a.P + n] = v;
        if (n >= N - a.P) o[n - (N - a.P)] = v;
    } else {
        double2 *o = a.out + s * a.nsc;
        if (n >= N - a.h) o[n - (N - a.h)] = v;
        if (n >= 1 && n <= a.h) o[a.h + n - 1] = v;
    }
}

// one Stockham pass of radix R over the SPW symbols from sym0; NS = product of the earlier radices.  In place in the LDS: every
// thread reads all its operands, the workgroup synchronises, then writes.  Recurses into the next pass at compile time.
template <int LOGN, bool TX, int R, int NS>
__device__ __forceinline__ void fast_pass(const OfdmArgs &a, int64_t sym0, double2 *lds) {
    using S = FastShape<LOGN>;
    constexpr int N = S::N, NB = N / R, BPT = S::PTS / R;
    constexpr bool FIRST = NS == 1, LAST = NS * R == N;
    double2 v[BPT][R];
#pragma unroll
    for (int b = 0; b < BPT; b++) {
        const int g = threadIdx.x + b * S::BLOCK, sl = g / NB, j = g % NB;
        if constexpr (FIRST) {
            const int64_t s = sym0 + sl;
            const bool live = s < a.nsym;
            const double2 *src = live ? symbol_input<N, TX>(a, s) : nullptr;
#pragma unroll
            for (int r = 0; r < R; r++) v[b][r] = live ? first_operand<N, TX>(a, src, j + r * NB) : make_double2(0.0, 0.0);
        } else {
#pragma unroll
            for (int r = 0; r < R; r++) v[b][r] = lds[sl * S::NPAD + of_pad(j + r * NB)];
            // W^(step r): the powers of two of r from the table, the others as products of those (at most three multiplications)
            const int step = (j % NS) * (N / (NS * R));
            double2 w[R];
#pragma unroll
            for (int r = 1; r < R; r++) {
                const int hb = 1 << ilog2(r);
                w[r] = hb == r ? a.tw[step * r] : cmul(w[hb], w[r - hb]);
                v[b][r] = TX ? cmul_conj(v[b][r], w[r]) : cmul(v[b][r], w[r]);
            }
        }
    }
    if constexpr (!FIRST) __syncthreads();
#pragma unroll
    for (int b = 0; b < BPT; b++) {
        dft_regs<R, TX>(v[b]);
        const int g = threadIdx.x + b * S::BLOCK, sl = g / NB, j = g % NB;
        const int base = (j / NS) * NS * R + j % NS;
#pragma unroll
        for (int r = 0; r < R; r++) {
            const int n = base + r * NS;
            lds[sl * S::NPAD + of_pad(n)] = v[b][r];
        }
    }
    if constexpr (!LAST) {
        __syncthreads();
        fast_pass<LOGN, TX, S::RMAX, NS * R>(a, sym0, lds);
    }
}

// the workgroup's outputs as one contiguous run, read from the LDS image of its transformed symbols
template <int LOGN, bool TX>
__device__ __forceinline__ void staged_write(const OfdmArgs &a, int64_t sym0, const double2 *lds) {
    using S = FastShape<LOGN>;
    constexpr int N = S::N;
    constexpr double SCALE = TX ? 1.0 / N : 1.0;   // exact: N is a power of two
    const int per = TX ? a.P + N : a.nsc;                      // output elements per symbol
    const int64_t left = a.nsym - sym0;
    const int nsyms = left < S::SPW ? (int)left : S::SPW;
    const int total = nsyms * per;
    double2 *dst = a.out + sym0 * per;
    int sl = threadIdx.x / per, m = threadIdx.x % per;     // (symbol, element) of e, advanced incrementally
    for (int e = threadIdx.x; e < total; e += S::BLOCK) {
        int n;
        if (TX) n = m < a.P ? N - a.P + m : m - a.P;
        else n = m < a.h ? N - a.h + m : m - a.h + 1;
        const double2 v = lds[sl * S::NPAD + of_pad(n)];
        dst[e] = make_double2(v.x * SCALE, v.y * SCALE);
        m += S::BLOCK;
        while (m >= per) { m -= per; sl++; }
    }
}

template <int LOGN, bool TX>
__global__ __launch_bounds__(of_block(LOGN)) void ofdm_fast_kernel(OfdmArgs a) {
    using S = FastShape<LOGN>;
    __shared__ double2 lds[S::LDS];
    const int64_t ntiles = (a.nsym + S::SPW - 1) / S::SPW;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t sym0 = tile * S::SPW;
        fast_pass<LOGN, TX, S::R0, 1>(a, sym0, lds);
        __syncthreads();
        staged_write<LOGN, TX>(a, sym0, lds);
        __syncthreads();          // the next tile's first pass overwrites the image
    }
}

// ---- direct DFT for every other size ------------------------------------------------------------------------------------
constexpr int OD_BLOCK = 256;
constexpr int OD_KPT = 4;         // output bins per thread and sweep
constexpr int OD_CHUNK = 2048;    // input samples staged in the LDS at a time

template <bool TX>
__global__ __launch_bounds__(OD_BLOCK) void ofdm_dft_kernel(OfdmArgs a, int N) {
    __shared__ double2 xs[OD_CHUNK];
    const double scale = TX ? 1.0 / N : 1.0;
    for (int64_t s = blockIdx.x; s < a.nsym; s += gridDim.x) {
        const double2 *src;
        if (TX) src = a.in + s * a.nsc;
        else {
            const int64_t b = s / a.rows, i = s - b * a.rows;
            src = a.in + b * a.ny + i * (int64_t)(N + a.cp) + a.cp;
        }
        for (int k0 = 0; k0 < N; k0 += OD_BLOCK * OD_KPT) {
            double2 acc[OD_KPT];
            int kq[OD_KPT], idx[OD_KPT];
#pragma unroll
            for (int q = 0; q < OD_KPT; q++) {
                acc[q] = make_double2(0.0, 0.0);
                const int k = k0 + threadIdx.x + q * OD_BLOCK;
                kq[q] = k < N ? k : 0;          // bins past N: a harmless sweep over W[0], not stored
            }
            for (int n0 = 0; n0 < N; n0 += OD_CHUNK) {
                const int len = N - n0 < OD_CHUNK ? N - n0 : OD_CHUNK;
                __syncthreads();
                for (int t = threadIdx.x; t < len; t += OD_BLOCK) {
                    const int k = n0 + t;
                    double2 v;
                    if (TX) {
                        if (k >= N - a.h) v = src[k - (N - a.h)];
                        else if (k >= 1 && k <= a.h) v = src[a.h + k - 1];
                        else v = make_double2(0.0, 0.0);
                    } else {
                        v = src[k];
                    }
                    xs[t] = v;
                }
                __syncthreads();
#pragma unroll
                for (int q = 0; q < OD_KPT; q++) idx[q] = (int)(((int64_t)n0 * kq[q]) % N);
                for (int t = 0; t < len; t++) {
                    const double2 xv = xs[t];
#pragma unroll
                    for (int q = 0; q < OD_KPT; q++) {
                        const double2 w = a.tw[idx[q]];
                        acc[q] = cadd(acc[q], TX ? cmul_conj(xv, w) : cmul(xv, w));
                        idx[q] += kq[q];
                        if (idx[q] >= N) idx[q] -= N;
                    }
                }
            }
#pragma unroll
            for (int q = 0; q < OD_KPT; q++) {
                const int k = k0 + threadIdx.x + q * OD_BLOCK;
                if (k < N) store_output<TX>(a, N, s, k, make_double2(acc[q].x * scale, acc[q].y * scale));
            }
        }
    }
}

template <bool TX>
int launch_fast(int logn, const OfdmArgs &a, hipStream_t st) {
#define OF_CASE(L)                                                                                                   \
    case L: {                                                                                                        \
        using S = FastShape<L>;                                                                                      \
        hipLaunchKernelGGL((ofdm_fast_kernel<L, TX>), dim3(grid_of((a.nsym + S::SPW - 1) / S::SPW)), dim3(S::BLOCK), \
                           0, st, a);                                                                                \
        break;                                                                                                       \
    }
    switch (logn) {
        OF_CASE(1) OF_CASE(2) OF_CASE(3) OF_CASE(4) OF_CASE(5) OF_CASE(6) OF_CASE(7) OF_CASE(8) OF_CASE(9) OF_CASE(10)
        OF_CASE(11) OF_CASE(12) OF_CASE(13)
        default: CPX_REQUIRE(false, CPX_EINVAL, "ofdm: no fast kernel for log2(nfft) = %d", logn);
    }
#undef OF_CASE
    CPX_HIP(hipGetLastError());
    note_kernel("ofdm_fast_kernel<%d,%s>", 1 << logn, TX ? "tx" : "rx");
    return CPX_OK;
}

template <bool TX>
int launch(const cpx_ofdm *p, OfdmArgs a, hipStream_t st) {
    a.tw = p->d_tw;
    a.nsc = p->nsc;
    a.h = p->h;
    a.cp = p->cp;
    a.P = p->P;
    if (p->logn >= 0) return launch_fast<TX>(p->logn, a, st);
    hipLaunchKernelGGL((ofdm_dft_kernel<TX>), dim3(grid_of(a.nsym)), dim3(OD_BLOCK), 0, st, a, p->nfft);
    CPX_HIP(hipGetLastError());
    note_kernel("ofdm_dft_kernel<%d,%s>", p->nfft, TX ? "tx" : "rx");
    return CPX_OK;
}

// W[k] = e^{-2 pi i k / N}: 4k = q N + r with q the nearest quarter turn (integers, exact), so the angle 2 pi k / N =
// q pi / 2 + pi r / (2 N) leaves |pi r / (2 N)| <= pi / 4 to cosl / sinl; the quarter turns are exact swaps and signs
std::vector<double> twiddles(int N) {
    std::vector<double> tw(2 * (size_t)N);
    const long double pi = 3.141592653589793238462643383279502884L;
    for (int64_t k = 0; k < N; k++) {
        const int64_t q = (4 * k + N / 2) / N, r = 4 * k - q * N;
        const long double ang = pi * (long double)r / (2.0L * N);
        const long double c = cosl(ang), s = sinl(ang);
        long double re, im;
        switch (q & 3) {
            case 0: re = c; im = s; break;
            case 1: re = -s; im = c; break;
            case 2: re = -c; im = -s; break;
            default: re = s; im = -c; break;
        }
        tw[2 * k] = (double)re;
        tw[2 * k + 1] = -(double)im;
    }
    return tw;
}

}  // namespace

extern "C" {

int cpx_ofdm_create(int nfft, int nsc, int cp_length, cpx_ofdm **out) {
    CPX_TRACE("cpx_ofdm_create");
    CPX_REQUIRE(out, CPX_EINVAL, "ofdm: null pointer");
    *out = nullptr;
    CPX_REQUIRE(nfft >= 2, CPX_EINVAL, "ofdm: nfft = %d, need at least 2", nfft);
    CPX_REQUIRE(nfft <= CPX_OFDM_MAX_NFFT, CPX_ELIMIT, "ofdm: nfft = %d is above the engine's limit of %d", nfft, CPX_OFDM_MAX_NFFT);
    CPX_REQUIRE(nsc >= 2 && nsc % 2 == 0, CPX_EINVAL, "ofdm: nsc = %d, need an even number >= 2", nsc);
    CPX_REQUIRE(nsc / 2 <= nfft - 1, CPX_EINVAL, "ofdm: nsc / 2 = %d subcarriers per side do not fit nfft = %d (at most nfft - 1)",
                nsc / 2, nfft);
    CPX_REQUIRE(cp_length >= 0, CPX_EINVAL, "ofdm: cp_length = %d is negative", cp_length);
    int rc = ensure_device();
    if (rc) return rc;
    cpx_ofdm *p = new cpx_ofdm();
    p->nfft = nfft;
    p->nsc = nsc;
    p->cp = cp_length;
    p->P = (cp_length > 0 && cp_length < nfft) ? cp_length : nfft;   // len(t[-cp_length:]) in the reference
    p->h = nsc / 2;
    p->logn = -1;
    if ((nfft & (nfft - 1)) == 0 && nfft <= 8192) p->logn = ilog2(nfft);
    (void)hipGetDevice(&p->device);
    const std::vector<double> tw = twiddles(nfft);
    if ((rc = upload((void **)&p->d_tw, tw.data(), sizeof(double) * tw.size(), "ofdm"))) {
        cpx_ofdm_destroy(p);
        return rc;
    }
    *out = p;
    return CPX_OK;
}

int cpx_ofdm_destroy(cpx_ofdm *p) {
    if (!p) return CPX_OK;
    (void)hipFree(p->d_tw);
    delete p;
    return CPX_OK;
}

int cpx_ofdm_tx_dev(const cpx_ofdm *p, const double *d_x_re_im, int64_t B, int64_t nsym, double *d_out_re_im, void *stream) {
    CPX_TRACE("cpx_ofdm_tx_dev");
    CPX_REQUIRE(p, CPX_EINVAL, "ofdm_tx: null plan");
    if (int rcd = check_handle_device(p->device, "ofdm_tx")) return rcd;
    CPX_REQUIRE(B >= 0 && nsym >= 0, CPX_EINVAL, "ofdm_tx: negative size");
    CPX_REQUIRE(B == 0 || nsym <= INT64_MAX / 16 / (p->P + p->nfft) / B, CPX_EINVAL, "ofdm_tx: %lld x %lld symbols overflow",
                (long long)B, (long long)nsym);
    if (B * nsym == 0) return CPX_OK;
    CPX_REQUIRE(d_x_re_im && d_out_re_im, CPX_EINVAL, "ofdm_tx: null pointer");
    OfdmArgs a{};
    a.in = reinterpret_cast<const double2 *>(d_x_re_im);
    a.out = reinterpret_cast<double2 *>(d_out_re_im);
    a.nsym = B * nsym;
    return launch<true>(p, a, pick_stream(stream));
}

int cpx_ofdm_rx_dev(const cpx_ofdm *p, const double *d_y_re_im, int64_t B, int64_t ny, double *d_out_re_im, void *stream) {
    CPX_TRACE("cpx_ofdm_rx_dev");
    CPX_REQUIRE(p, CPX_EINVAL, "ofdm_rx: null plan");
    if (int rcd = check_handle_device(p->device, "ofdm_rx")) return rcd;
    CPX_REQUIRE(B >= 0 && ny >= 0, CPX_EINVAL, "ofdm_rx: negative size");
    CPX_REQUIRE(B == 0 || ny <= INT64_MAX / 16 / B, CPX_EINVAL, "ofdm_rx: %lld x %lld samples overflow", (long long)B, (long long)ny);
    const int64_t rows = ny / ((int64_t)p->nfft + p->cp);
    if (B * rows == 0) return CPX_OK;
    CPX_REQUIRE(d_y_re_im && d_out_re_im, CPX_EINVAL, "ofdm_rx: null pointer");
    OfdmArgs a{};
    a.in = reinterpret_cast<const double2 *>(d_y_re_im);
    a.out = reinterpret_cast<double2 *>(d_out_re_im);
    a.nsym = B * rows;
    a.rows = rows;
    a.ny = ny;
    return launch<false>(p, a, pick_stream(stream));
}

int cpx_ofdm_tx(const cpx_ofdm *p, const double *x_re_im, int64_t B, int64_t nsym, double *out_re_im) {
    CPX_TRACE("cpx_ofdm_tx");
    CPX_REQUIRE(p, CPX_EINVAL, "ofdm_tx: null plan");
    CPX_REQUIRE(B >= 0 && nsym >= 0, CPX_EINVAL, "ofdm_tx: negative size");
    CPX_REQUIRE(B == 0 || nsym <= INT64_MAX / 16 / (p->P + p->nfft) / B, CPX_EINVAL, "ofdm_tx: %lld x %lld symbols overflow",
                (long long)B, (long long)nsym);
    const size_t in_bytes = 16 * (size_t)(B * nsym) * p->nsc, out_bytes = 16 * (size_t)(B * nsym) * (p->P + p->nfft);
    CPX_REQUIRE((x_re_im || in_bytes == 0) && (out_re_im || out_bytes == 0), CPX_EINVAL, "ofdm_tx: null pointer");
    int rc = ensure_device();
    if (rc) return rc;
    if (out_bytes == 0) return CPX_OK;
    HostStage s;
    const double *din;
    double *dout;
    if ((rc = s.in(x_re_im, in_bytes, &din)) || (rc = s.out(out_bytes, &dout)) || (rc = cpx_ofdm_tx_dev(p, din, B, nsym, dout, s.st)))
        return rc;
    return s.get(out_re_im, dout, out_bytes);
}

int cpx_ofdm_rx(const cpx_ofdm *p, const double *y_re_im, int64_t B, int64_t ny, double *out_re_im) {
    CPX_TRACE("cpx_ofdm_rx");
    CPX_REQUIRE(p, CPX_EINVAL, "ofdm_rx: null plan");
    CPX_REQUIRE(B >= 0 && ny >= 0, CPX_EINVAL, "ofdm_rx: negative size");
    CPX_REQUIRE(B == 0 || ny <= INT64_MAX / 16 / B, CPX_EINVAL, "ofdm_rx: %lld x %lld samples overflow", (long long)B, (long long)ny);
    const int64_t rows = ny / ((int64_t)p->nfft + p->cp);
    const size_t in_bytes = 16 * (size_t)(B * ny), out_bytes = 16 * (size_t)(B * rows) * p->nsc;
    CPX_REQUIRE((y_re_im || in_bytes == 0) && (out_re_im || out_bytes == 0), CPX_EINVAL, "ofdm_rx: null pointer");
    int rc = ensure_device();
    if (rc) return rc;
    if (out_bytes == 0) return CPX_OK;
    HostStage s;
    const double *din;
    double *dout;
    if ((rc = s.in(y_re_im, in_bytes, &din)) || (rc = s.out(out_bytes, &dout)) || (rc = cpx_ofdm_rx_dev(p, din, B, ny, dout, s.st)))
        return rc;
    return s.get(out_re_im, dout, out_bytes);
}

}  // extern "C"
