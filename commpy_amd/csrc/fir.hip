// FIR filtering of sampled waveforms and a carrier frequency offset, batched, complex128 with float64 arithmetic only
// (cpx_set_precision does not apply).  What the reference does with numpy.convolve over a zero-stuffed stream:
//
//   interpolating FIR (pulse shaping)   out[b] = convolve(upsample(x[b], sps), h)          [B][n sps + ntaps - 1]
//   decimating FIR (matched filter)     out[b] = convolve(y[b], h)[offset::sps]            [B][ceil((n + ntaps - 1 - offset) / sps)]
//   frequency offset                    out[b][k] = x[b][k] (cos t + i sin t), t = step_b k rounded once to float64
//
// Every output sample is one chain of fused multiply-adds over its taps in ASCENDING TAP INDEX, started from +0 (complex taps:
// re += hr xr, re -= hi xi, im += hr xi, im += hi xr per tap).  Terms whose input lies outside the row are zeros and leave the
// chain's value unchanged, so it does not matter whether a kernel skips them: the result depends only on (ntaps, sps, offset,
// index in the row), never on B, the row, the tile, the kernel or the stream.  Taps are expected to be finite.
//
// Kernels, chosen per call from the plan and the shape (no process-wide switch); real and complex taps are two instantiations:
//   fir_interp_kernel<C>    sps <= 64.  A workgroup of 256 threads owns G R consecutive input positions q (G = 256 / sps, R = 4),
//       i.e. G R sps contiguous outputs.  Thread (p, g) = (t mod sps, t / sps) computes phase p of q = q0 + g R + r, r < R: per j
//       one tap h[p + j sps] from the LDS (consecutive lanes, consecutive taps) and ONE new input x[q - j] -- the R inputs of a
//       step slide through registers -- for 2 R (real) or 4 R (complex) FMAs.  Taps and the inputs under them are staged in the
//       LDS in chunks of 512 / sps values of j; the zeros of the upsampled stream are never formed.  For a fixed r the lanes of
//       a phase run store sps contiguous samples.  Input tile padded by one double2 per 4 (the lane stride is R = 4).
//   fir_decim_kernel<C, R>  a workgroup of 128 threads owns 128 R consecutive kept outputs (R = 4, 2 or 1, the largest whose
//       input window (128 R - 1) sps + min(ntaps, 512) fits the LDS and keeps at least half the lanes of a row's tiles busy).
//       Taps in chunks of 512: per tap one LDS broadcast read (the tap is uniform across the wave) shared by the R outputs of
//       the lane, and R input reads.  Lanes read inputs R sps apart; the tile is stored with one double2 of padding
//       per 2^a samples, 2^a the largest power of two dividing R sps, which makes the lane stride odd (conflict-free
//       ds_read_b128) while the padding of a lane's own offset stays uniform across the wave.
//   fir_interp_direct<C> / fir_decim_direct<C>  every other shape (sps above the tiled kernels' range, rows much shorter than
//       a tile): one output per thread over the flattened batch, operands from global memory (L1 / L2).
//   freq_offset_kernel      one sample per lane and step, sincos() of the float64 product (full-range argument reduction).
// Offsets are 64-bit throughout.
#include "cpx_internal.h"
#include "cpx_rotate.h"
#include "cpx_wave.h"

#include <climits>

using namespace cpx;

#define CPX_FIR_MAX_TAPS 8192

struct cpx_fir {
    __attribute__((visibility("hidden"))) ~cpx_fir() = default;
    int ntaps, cplx, device;
    double *d_taps = nullptr;   // [ntaps] or [ntaps][2]
};

namespace {

template <bool C> struct TapOf { using T = double; };
template <> struct TapOf<true> { using T = double2; };

__device__ __forceinline__ double tap_zero(double) { return 0.0; }
__device__ __forceinline__ double2 tap_zero(double2) { return make_double2(0.0, 0.0); }

// one tap of the chain: a real tap here, a complex one in cpx_wave.h (named so that both overloads are found from this namespace)
using cpx::mac;
__device__ __forceinline__ void mac(double2 &acc, double h, double2 x) {
    acc.x = fma(h, x.x, acc.x);
    acc.y = fma(h, x.y, acc.y);
}

struct FirArgs {
    const double2 *in;      // [B][n]
    double2 *out;           // [B][lout]
    const void *taps;       // [ntaps] double or double2
    int64_t n, lout;        // samples per input / output row
    int64_t tiles_per_row, ntiles;
    int64_t total;          // B * lout (direct kernels)
    int ntaps, sps;
    int64_t offset;         // decimator
    int pad_shift;          // decimator: a (31 = no padding)
};

unsigned fir_grid(int64_t items) { return grid_of(items, 1 << 20); }

// ---- interpolator ----------------------------------------------------------------------------------------------------------
constexpr int FI_BLOCK = 256, FI_R = 4, FI_KT = 512, FI_MAX_SPS = 64;
constexpr int FI_XS = 1920;                               // padded input tile: (1024 + 512 - 1) * 5 / 4 rounded up
__device__ __forceinline__ int fi_pad(int i) { return i + (i >> 2); }

template <bool C>
__global__ __launch_bounds__(FI_BLOCK) void fir_interp_kernel(FirArgs a) {
    using TapT = typename TapOf<C>::T;
    constexpr int R = FI_R;
    __shared__ TapT tl[FI_KT];
    __shared__ double2 xs[FI_XS];
    const TapT *h = static_cast<const TapT *>(a.taps);
    const int sps = a.sps, t = threadIdx.x;
    const int G = FI_BLOCK / sps, TQ = G * R;
    const int g = t / sps, p = t - g * sps;
    const bool live = g < G;
    const int T = (a.ntaps + sps - 1) / sps;               // taps per phase at most
    const int JC = FI_KT / sps;                             // values of j per chunk
    for (int64_t tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
        const int64_t b = tile / a.tiles_per_row;
        const int64_t q0 = (tile - b * a.tiles_per_row) * TQ;
        const double2 *x = a.in + b * a.n;
        double2 acc[R];
#pragma unroll
        for (int r = 0; r < R; r++) acc[r] = make_double2(0.0, 0.0);
        for (int jc = 0; jc < T; jc += JC) {
            const int JCn = T - jc < JC ? T - jc : JC;
            const int JCpad = (JCn + R - 1) / R * R;
            // LDS position w holds x[q0 - (jc + JCpad - 1) + w]
            const int64_t s0 = q0 - (jc + JCpad - 1);
            const int W = TQ + JCpad - 1;
            for (int i = t; i < JCn * sps; i += FI_BLOCK) {
                const int k = jc * sps + i;
                tl[i] = k < a.ntaps ? h[k] : tap_zero(TapT());
            }
            for (int w = t; w < W; w += FI_BLOCK) {
                const int64_t s = s0 + w;
                xs[fi_pad(w)] = (s >= 0 && s < a.n) ? x[s] : make_double2(0.0, 0.0);
            }
            __syncthreads();
            if (live) {
                const int base = g * R;
                double2 xr[R];                              // xr[(r + R - 1 - u) mod R] = the input of output r at step u
#pragma unroll
                for (int r = 0; r < R; r++) xr[(r + R - 1) % R] = xs[fi_pad(base + r + JCpad - 1)];
                for (int ua = 0; ua < JCpad; ua += R) {
#pragma unroll
                    for (int bb = 0; bb < R; bb++) {
                        const int u = ua + bb;
                        if (u < JCn) {
                            const int k = (jc + u) * sps + p;
                            if (k < a.ntaps) {              // no tap, no term: a non-finite input must not meet a padded zero
                                const TapT tap = tl[u * sps + p];
#pragma unroll
                                for (int r = 0; r < R; r++) mac(acc[r], tap, xr[(r + R - 1 - bb) % R]);
                            }
                        }
                        if (u + 1 < JCpad) xr[(2 * R - 2 - bb) % R] = xs[fi_pad(base + JCpad - 2 - u)];
                    }
                }
            }
            __syncthreads();
        }
        if (live) {
            double2 *o = a.out + b * a.lout;
#pragma unroll
            for (int r = 0; r < R; r++) {
                const int64_t m = (q0 + g * R + r) * sps + p;
                if (m < a.lout) o[m] = acc[r];
            }
        }
    }
}

template <bool C>
__global__ __launch_bounds__(256) void fir_interp_direct(FirArgs a) {
    using TapT = typename TapOf<C>::T;
    const TapT *h = static_cast<const TapT *>(a.taps);
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < a.total; idx += (int64_t)gridDim.x * blockDim.x) {
        const int64_t b = idx / a.lout, m = idx - b * a.lout;
        const int64_t q = m / a.sps;
        const int p = (int)(m - q * a.sps);
        const double2 *x = a.in + b * a.n;
        double2 acc = make_double2(0.0, 0.0);
        int64_t s = q;
        for (int64_t k = p; k < a.ntaps && s >= 0; k += a.sps, s--)      // 64-bit: p + sps may pass INT_MAX
            if (s < a.n) mac(acc, h[k], x[s]);
        a.out[idx] = acc;
    }
}

// ---- decimator -------------------------------------------------------------------------------------------------------------
constexpr int FD_BLOCK = 128, FD_KC = 512;
constexpr size_t FD_LDS_BYTES = 60 * 1024;

template <bool C, int R>
__global__ __launch_bounds__(FD_BLOCK) void fir_decim_kernel(FirArgs a) {
    using TapT = typename TapOf<C>::T;
    extern __shared__ double2 fd_lds[];
    TapT *tl = reinterpret_cast<TapT *>(fd_lds);                         // [FD_KC]
    double2 *xs = fd_lds + FD_KC * sizeof(TapT) / sizeof(double2);       // the padded input tile
    const TapT *h = static_cast<const TapT *>(a.taps);
    constexpr int TO = FD_BLOCK * R;
    const int sps = a.sps, t = threadIdx.x, sh = a.pad_shift;
    const int Sd = R * sps;
    const int lane_base = t * (Sd + (Sd >> sh));
    for (int64_t tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
        const int64_t b = tile / a.tiles_per_row;
        const int64_t i0 = (tile - b * a.tiles_per_row) * TO;
        const double2 *y = a.in + b * a.n;
        double2 acc[R];
#pragma unroll
        for (int r = 0; r < R; r++) acc[r] = make_double2(0.0, 0.0);
        for (int kc = 0; kc < a.ntaps; kc += FD_KC) {
            const int KCn = a.ntaps - kc < FD_KC ? a.ntaps - kc : FD_KC;
            // LDS position w holds y[offset + i0 sps - (kc + KCn - 1) + w]
            const int64_t s0 = a.offset + i0 * sps - (kc + KCn - 1);
            const int W = (TO - 1) * sps + KCn;
            for (int i = t; i < KCn; i += FD_BLOCK) tl[i] = h[kc + i];
            for (int w = t; w < W; w += FD_BLOCK) {
                const int64_t s = s0 + w;
                xs[w + (w >> sh)] = (s >= 0 && s < a.n) ? y[s] : make_double2(0.0, 0.0);
            }
            __syncthreads();
            for (int u = 0; u < KCn; u++) {
                const TapT tap = tl[u];                                  // uniform address: one broadcast read per wave
#pragma unroll
                for (int r = 0; r < R; r++) {
                    const int e = r * sps + KCn - 1 - u;                 // uniform across the wave, and so is its padding
                    mac(acc[r], tap, xs[lane_base + e + (e >> sh)]);
                }
            }
            __syncthreads();
        }
        double2 *o = a.out + b * a.lout;
#pragma unroll
        for (int r = 0; r < R; r++) {
            const int64_t i = i0 + (int64_t)t * R + r;
            if (i < a.lout) o[i] = acc[r];
        }
    }
}

template <bool C>
__global__ __launch_bounds__(256) void fir_decim_direct(FirArgs a) {
    using TapT = typename TapOf<C>::T;
    const TapT *h = static_cast<const TapT *>(a.taps);
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < a.total; idx += (int64_t)gridDim.x * blockDim.x) {
        const int64_t b = idx / a.lout, i = idx - b * a.lout;
        const int64_t m = a.offset + i * a.sps;                          // index in the full convolution
        const double2 *y = a.in + b * a.n;
        const int klo = m - (a.n - 1) > 0 ? (int)(m - (a.n - 1)) : 0;
        const int khi = m < a.ntaps - 1 ? (int)m : a.ntaps - 1;
        double2 acc = make_double2(0.0, 0.0);
        for (int k = klo; k <= khi; k++) mac(acc, h[k], y[m - k]);
        a.out[idx] = acc;
    }
}

// ---- frequency offset ------------------------------------------------------------------------------------------------------
constexpr int FO_BLOCK = 256, FO_CHUNK = 1024;

__global__ __launch_bounds__(FO_BLOCK) void freq_offset_kernel(const double2 *x, double2 *out, const double *step, int batched,
                                                               int64_t n, int64_t chunks_per_row, int64_t nchunks) {
    for (int64_t c = blockIdx.x; c < nchunks; c += gridDim.x) {
        const int64_t b = c / chunks_per_row;
        const int64_t k0 = (c - b * chunks_per_row) * FO_CHUNK;
        const double st = step[batched ? b : 0];
#pragma unroll
        for (int i = 0; i < FO_CHUNK / FO_BLOCK; i++) {
            const int64_t k = k0 + threadIdx.x + i * FO_BLOCK;
            if (k < n) out[b * n + k] = freq_rotate(x[b * n + k], st, k);
        }
    }
}

// ---- launches --------------------------------------------------------------------------------------------------------------
template <bool C>
int launch_interp(FirArgs a, int64_t B, hipStream_t st) {
    const int64_t nq = (a.lout + a.sps - 1) / a.sps;
    const int TQ = a.sps <= FI_MAX_SPS ? FI_BLOCK / a.sps * FI_R : 0;
    // the tiled kernel when its tiles are at least half full
    if (TQ && 2 * nq >= TQ) {
        a.tiles_per_row = (nq + TQ - 1) / TQ;
        a.ntiles = B * a.tiles_per_row;
        hipLaunchKernelGGL((fir_interp_kernel<C>), dim3(fir_grid(a.ntiles)), dim3(FI_BLOCK), 0, st, a);
        CPX_HIP(hipGetLastError());
        note_kernel("fir_interp_kernel<%s>", C ? "complex" : "real");
        return CPX_OK;
    }
    hipLaunchKernelGGL((fir_interp_direct<C>), dim3(fir_grid((a.total + 255) / 256)), dim3(256), 0, st, a);
    CPX_HIP(hipGetLastError());
    note_kernel("fir_interp_direct<%s>", C ? "complex" : "real");
    return CPX_OK;
}

template <bool C, int R>
bool try_decim(FirArgs a, int64_t B, hipStream_t st) {
    const int64_t Sd = (int64_t)R * a.sps;
    const int TO = FD_BLOCK * R;
    int sh = __builtin_ctzll((unsigned long long)Sd);
    if (sh == 0) sh = 31;
    const int64_t W = (int64_t)(TO - 1) * a.sps + (a.ntaps < FD_KC ? a.ntaps : FD_KC);
    const int64_t Wp = W + (W >> sh) + 1;
    const size_t tap_bytes = FD_KC * (C ? 16 : 8);
    if (Wp * 16 + tap_bytes > FD_LDS_BYTES) return false;
    const int64_t tiles = (a.lout + TO - 1) / TO;
    if (2 * a.lout < tiles * TO) return false;          // less than half of the lanes would have an output
    a.pad_shift = sh;
    a.tiles_per_row = tiles;
    a.ntiles = B * tiles;
    hipLaunchKernelGGL((fir_decim_kernel<C, R>), dim3(fir_grid(a.ntiles)), dim3(FD_BLOCK), (size_t)Wp * 16 + tap_bytes, st, a);
    note_kernel("fir_decim_kernel<%s,%d>", C ? "complex" : "real", R);
    return true;
}

template <bool C>
int launch_decim(const FirArgs &a, int64_t B, hipStream_t st) {
    if (!try_decim<C, 4>(a, B, st) && !try_decim<C, 2>(a, B, st) && !try_decim<C, 1>(a, B, st)) {
        hipLaunchKernelGGL((fir_decim_direct<C>), dim3(fir_grid((a.total + 255) / 256)), dim3(256), 0, st, a);
        note_kernel("fir_decim_direct<%s>", C ? "complex" : "real");
    }
    CPX_HIP(hipGetLastError());
    return CPX_OK;
}

// sizes of an interpolator / decimator call; CPX_OK and *lout = samples per output row
int interp_sizes(const cpx_fir *p, int64_t B, int64_t n, int sps, int64_t *lout) {
    CPX_REQUIRE(p, CPX_EINVAL, "fir_interp: null plan");
    CPX_REQUIRE(B >= 0 && n >= 0, CPX_EINVAL, "fir_interp: negative size");
    CPX_REQUIRE(sps >= 1, CPX_EINVAL, "fir_interp: sps = %d, need at least 1", sps);
    CPX_REQUIRE(B == 0 || n > 0, CPX_EINVAL, "fir_interp: n = 0 (an empty row cannot be convolved)");
    CPX_REQUIRE(B == 0 || n <= (INT64_MAX / 64 - p->ntaps) / sps / B, CPX_EINVAL, "fir_interp: %lld x %lld x %d samples overflow",
                (long long)B, (long long)n, sps);
    *lout = n * sps + p->ntaps - 1;
    return CPX_OK;
}

int decim_sizes(const cpx_fir *p, int64_t B, int64_t n, int sps, int64_t offset, int64_t *lout) {
    CPX_REQUIRE(p, CPX_EINVAL, "fir_decim: null plan");
    CPX_REQUIRE(B >= 0 && n >= 0, CPX_EINVAL, "fir_decim: negative size");
    CPX_REQUIRE(sps >= 1, CPX_EINVAL, "fir_decim: sps = %d, need at least 1", sps);
    CPX_REQUIRE(B == 0 || n > 0, CPX_EINVAL, "fir_decim: n = 0 (an empty row cannot be convolved)");
    CPX_REQUIRE(B == 0 || n <= (INT64_MAX / 64 - p->ntaps) / B, CPX_EINVAL, "fir_decim: %lld x %lld samples overflow", (long long)B,
                (long long)n);
    if (B == 0) { *lout = 0; return CPX_OK; }
    const int64_t full = n + p->ntaps - 1;
    CPX_REQUIRE(offset >= 0 && offset < full, CPX_EINVAL, "fir_decim: offset = %lld is outside the %lld samples of the full convolution",
                (long long)offset, (long long)full);
    *lout = (full - offset + sps - 1) / sps;
    return CPX_OK;
}

int freq_sizes(int64_t B, int64_t n, int step_batched) {
    CPX_REQUIRE(B >= 0 && n >= 0, CPX_EINVAL, "freq_offset: negative size");
    CPX_REQUIRE(step_batched == 0 || step_batched == 1, CPX_EINVAL, "freq_offset: step_batched = %d, need 0 or 1", step_batched);
    CPX_REQUIRE(B == 0 || n <= INT64_MAX / 64 / B, CPX_EINVAL, "freq_offset: %lld x %lld samples overflow", (long long)B, (long long)n);
    return CPX_OK;
}

}  // namespace

extern "C" {

int cpx_fir_create(const double *taps, int ntaps, int taps_complex, cpx_fir **out) {
    CPX_TRACE("cpx_fir_create");
    CPX_REQUIRE(out, CPX_EINVAL, "fir: null pointer");
    *out = nullptr;
    CPX_REQUIRE(taps, CPX_EINVAL, "fir: null pointer");
    CPX_REQUIRE(ntaps >= 1, CPX_EINVAL, "fir: ntaps = %d, need at least 1", ntaps);
    CPX_REQUIRE(ntaps <= CPX_FIR_MAX_TAPS, CPX_ELIMIT, "fir: ntaps = %d is above the engine's limit of %d", ntaps, CPX_FIR_MAX_TAPS);
    CPX_REQUIRE(taps_complex == 0 || taps_complex == 1, CPX_EINVAL, "fir: taps_complex = %d, need 0 or 1", taps_complex);
    int rc = ensure_device();
    if (rc) return rc;
    cpx_fir *p = new cpx_fir();
    p->ntaps = ntaps;
    p->cplx = taps_complex;
    (void)hipGetDevice(&p->device);
    if ((rc = upload((void **)&p->d_taps, taps, sizeof(double) * (size_t)ntaps * (taps_complex ? 2 : 1), "fir"))) {
        cpx_fir_destroy(p);
        return rc;
    }
    *out = p;
    return CPX_OK;
}

int cpx_fir_destroy(cpx_fir *p) {
    if (!p) return CPX_OK;
    (void)hipFree(p->d_taps);
    delete p;
    return CPX_OK;
}

int cpx_fir_interp_dev(const cpx_fir *p, const double *d_x_re_im, int64_t B, int64_t n, int sps, double *d_out_re_im, void *stream) {
    CPX_TRACE("cpx_fir_interp_dev");
    int64_t lout;
    if (int rc = interp_sizes(p, B, n, sps, &lout)) return rc;
    if (B == 0) return CPX_OK;
    if (int rcd = check_handle_device(p->device, "fir_interp")) return rcd;
    CPX_REQUIRE(d_x_re_im && d_out_re_im, CPX_EINVAL, "fir_interp: null pointer");
    FirArgs a{};
    a.in = reinterpret_cast<const double2 *>(d_x_re_im);
    a.out = reinterpret_cast<double2 *>(d_out_re_im);
    a.taps = p->d_taps;
    a.n = n;
    a.lout = lout;
    a.total = B * lout;
    a.ntaps = p->ntaps;
    a.sps = sps;
    return p->cplx ? launch_interp<true>(a, B, pick_stream(stream)) : launch_interp<false>(a, B, pick_stream(stream));
}

int cpx_fir_decim_dev(const cpx_fir *p, const double *d_y_re_im, int64_t B, int64_t n, int sps, int64_t offset, double *d_out_re_im,
                      void *stream) {
    CPX_TRACE("cpx_fir_decim_dev");
    int64_t lout;
    if (int rc = decim_sizes(p, B, n, sps, offset, &lout)) return rc;
    if (B == 0) return CPX_OK;
    if (int rcd = check_handle_device(p->device, "fir_decim")) return rcd;
    CPX_REQUIRE(d_y_re_im && d_out_re_im, CPX_EINVAL, "fir_decim: null pointer");
    FirArgs a{};
    a.in = reinterpret_cast<const double2 *>(d_y_re_im);
    a.out = reinterpret_cast<double2 *>(d_out_re_im);
    a.taps = p->d_taps;
    a.n = n;
    a.lout = lout;
    a.total = B * lout;
    a.ntaps = p->ntaps;
    a.sps = sps;
    a.offset = offset;
    return p->cplx ? launch_decim<true>(a, B, pick_stream(stream)) : launch_decim<false>(a, B, pick_stream(stream));
}

int cpx_freq_offset_dev(const double *d_x_re_im, int64_t B, int64_t n, const double *d_step, int step_batched, double *d_out_re_im,
                        void *stream) {
    CPX_TRACE("cpx_freq_offset_dev");
    if (int rc = freq_sizes(B, n, step_batched)) return rc;
    if (B * n == 0) return CPX_OK;
    CPX_REQUIRE(d_x_re_im && d_out_re_im && d_step, CPX_EINVAL, "freq_offset: null pointer");
    const int64_t cpr = (n + FO_CHUNK - 1) / FO_CHUNK, nchunks = B * cpr;
    hipLaunchKernelGGL(freq_offset_kernel, dim3(fir_grid(nchunks)), dim3(FO_BLOCK), 0, pick_stream(stream),
                       reinterpret_cast<const double2 *>(d_x_re_im), reinterpret_cast<double2 *>(d_out_re_im), d_step, step_batched, n,
                       cpr, nchunks);
    CPX_HIP(hipGetLastError());
    note_kernel("freq_offset_kernel");
    return CPX_OK;
}

int cpx_fir_interp(const cpx_fir *p, const double *x_re_im, int64_t B, int64_t n, int sps, double *out_re_im) {
    CPX_TRACE("cpx_fir_interp");
    int64_t lout;
    if (int rc = interp_sizes(p, B, n, sps, &lout)) return rc;
    if (B == 0) return CPX_OK;
    CPX_REQUIRE(x_re_im && out_re_im, CPX_EINVAL, "fir_interp: null pointer");
    int rc = ensure_device();
    if (rc) return rc;
    const size_t in_bytes = 16 * (size_t)(B * n), out_bytes = 16 * (size_t)(B * lout);
    HostStage s;
    const double *din;
    double *dout;
    if ((rc = s.in(x_re_im, in_bytes, &din)) || (rc = s.out(out_bytes, &dout)) || (rc = cpx_fir_interp_dev(p, din, B, n, sps, dout, s.st)))
        return rc;
    return s.get(out_re_im, dout, out_bytes);
}

int cpx_fir_decim(const cpx_fir *p, const double *y_re_im, int64_t B, int64_t n, int sps, int64_t offset, double *out_re_im) {
    CPX_TRACE("cpx_fir_decim");
    int64_t lout;
    if (int rc = decim_sizes(p, B, n, sps, offset, &lout)) return rc;
    if (B == 0) return CPX_OK;
    CPX_REQUIRE(y_re_im && out_re_im, CPX_EINVAL, "fir_decim: null pointer");
    int rc = ensure_device();
    if (rc) return rc;
    const size_t in_bytes = 16 * (size_t)(B * n), out_bytes = 16 * (size_t)(B * lout);
    HostStage s;
    const double *din;
    double *dout;
    if ((rc = s.in(y_re_im, in_bytes, &din)) || (rc = s.out(out_bytes, &dout)) ||
        (rc = cpx_fir_decim_dev(p, din, B, n, sps, offset, dout, s.st)))
        return rc;
    return s.get(out_re_im, dout, out_bytes);
}

int cpx_freq_offset(const double *x_re_im, int64_t B, int64_t n, const double *step, int step_batched, double *out_re_im) {
    CPX_TRACE("cpx_freq_offset");
    if (int rc = freq_sizes(B, n, step_batched)) return rc;
    if (B * n == 0) return CPX_OK;
    CPX_REQUIRE(x_re_im && out_re_im && step, CPX_EINVAL, "freq_offset: null pointer");
    int rc = ensure_device();
    if (rc) return rc;
    const size_t bytes = 16 * (size_t)(B * n);
    HostStage s;
    const double *din, *dstep;
    double *dout;
    if ((rc = s.in(x_re_im, bytes, &din)) || (rc = s.in(step, sizeof(double) * (size_t)(step_batched ? B : 1), &dstep)) ||
        (rc = s.out(bytes, &dout)) || (rc = cpx_freq_offset_dev(din, B, n, dstep, step_batched, dout, s.st)))
        return rc;
    return s.get(out_re_im, dout, bytes);
}

}  // extern "C"
