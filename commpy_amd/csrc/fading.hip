// Doppler-fading multipath channel: a tapped delay line whose tap gains follow Clarke's model (sum of sinusoids,
// Jakes Doppler spectrum), Rayleigh or Rician per tap, batched, complex128 with float64 arithmetic only (cpx_set_precision does not
// apply, no path switch).  Not in the reference; the yardstick is the NumPy model of tests/fading_model.py.  The definitions are
// written out in include/commpy_amd.h ("Doppler-fading multipath channel").
//
//   params     (nu, phi) of every sinusoid and of the line of sight                          -> [B][nr][nt][L][Ns + 1][2] float64
//   gains      G[b][j][r][t][l], block j at time tau = t0 + j hold                            -> [B][nblk][nr][nt][L]
//   convolve   y[b][r][m] = sum_t sum_l G[b][m div hold][r][t][l] x[b][t][m - l]    x [B][nt][n] -> y [B][nr][n + L - 1]
//   channel    gains, then convolve; without a caller's G the gains live in the scratch arena, at most CPX_FADING_SCRATCH_BYTES
//
// Every draw is a pure function of (seed, stream id, row, antenna pair, tap, sinusoid): fade_sinusoid() below is the ONLY place a
// (nu, phi) is formed, and fade_gain() the only place a gain is, so a value never depends on the kernel, on the batch, on how paths
// and blocks are spread over workgroups, or on where a call starts in time (no rotation recurrences).
//   fading_params_kernel   one sinusoid per thread over the flattened batch.
//   fading_gains_kernel    a workgroup owns (a group of PC consecutive paths of the call, a chunk of JC blocks); the paths are
//       numbered over rows (the counters are linear in that number), so a group may span rows where a row has few paths.  The
//       group's PC (Ns + 1) pairs (nu, phi) are drawn once (Philox + cospi) into the LDS, sinusoid-major so that the lanes of a wave
//       read consecutive entries; then one gain per thread and step, paths fastest, so that stores run along G's innermost axes.
//       PC (Ns + 1) <= 2048 entries (32 KB), PC <= 256; JC >= 16 (where there are as many blocks) keeps the draws below 1/16 of the
//       sincospi work.
//   fading_taps_kernel     the per-tap scales (a_l, c_l) reach the device as kernel arguments, 128 taps per launch: stream-ordered,
//       no host buffer has to outlive the call.
// Convolution: cpx_multipath's chain, one chain of fused multiply-adds from +0 over t ascending, then tap index ascending, per tap
// re += gr xr, re -= gi xi, im += gr xi, im += gi xr; only the tap SET changes with the output's block.  The shape picks the kernel:
//   fading_tiled_kernel<NRG>   rows of at least 512 outputs whose tiles meet tap sets that fit the LDS: with `sets` = the most blocks
//       that 1024 consecutive outputs can meet (capped by the blocks there are), sets nr nt L <= 2048 (32 KB).  multipath_kernel's
//       tile (256 threads x 4 consecutive outputs x NRG antennas, inputs sliding through registers, taps in chunks of 512); a thread
//       whose four outputs share a block reads each tap once (a broadcast across the wave where the wave shares the block), a thread
//       that straddles an edge reads one tap per output.
//   fading_direct_kernel       everything else (short rows, or many small blocks: with hold = 1 every output has its own nt L taps
//       and the taps are the dominant traffic): one output per thread, operands from global memory through L1 / L2.
// Terms under a row's edges are skipped (direct) or meet zero inputs (tiled): the value is the same for finite data, so both forms,
// and cpx_multipath where the gains do not change, agree bit for bit.  Offsets are 64-bit, grids are capped at 65 535 workgroups.
#include "cpx_internal.h"
#include "cpx_rng.h"
#include "cpx_wave.h"             // mac: the chain step shared with fir.hip and ofdm_chan.hip; grid_of

#include <climits>
#include <cmath>

using namespace cpx;

#define CPX_FD_MAX_L 1024
#define CPX_FD_MAX_TAPS 2048       // nr nt L of one tap set
#define CPX_FD_MAX_SIN 256

namespace {

constexpr int64_t FD_TWO52 = (int64_t)1 << 52;

// ---- the model -------------------------------------------------------------------------------------------------------------------
struct FdDraw {
    uint64_t seed, stream, path0;   // path0 = first_row nr nt L, modulo 2^64
    double fd, fd_los;
    int ns;
};

// (nu, phi) of sinusoid s < Ns of path p, or of its line of sight (s == Ns)
__device__ __forceinline__ double2 fade_sinusoid(const FdDraw &d, uint64_t path, int s) {
    const Philox r = philox4x32_10(path * (uint64_t)(d.ns + 1) + (uint64_t)s, d.stream, d.seed);
    const double phi = u01(r.c[2], r.c[3]);
    const double nu = s < d.ns ? d.fd * cospi(2.0 * u01(r.c[0], r.c[1])) : d.fd_los;
    return make_double2(nu, phi);
}

// (cos, sin) of 2 pi (nu tau + phi): the phase is reduced exactly before the only rounding trigonometry sees
__device__ __forceinline__ double2 fade_phasor(double2 np, double tau) {
    const double psi = fma(np.x, tau, np.y);
    const double rho = psi - rint(psi);
    double sn, cs;
    sincospi(2.0 * rho, &sn, &cs);
    return make_double2(cs, sn);
}

// the gain of one path at time tau from its Ns + 1 pairs sp[s * stride]; tap = (a_l, c_l), c_l < 0: no line of sight
__device__ __forceinline__ double2 fade_gain(const double2 *sp, int stride, int ns, double2 tap, double tau) {
    double2 S = make_double2(0.0, 0.0);
    for (int s = 0; s < ns; s++) {
        const double2 e = fade_phasor(sp[s * stride], tau);
        S.x += e.x;
        S.y += e.y;
    }
    double2 g = make_double2(tap.x * S.x, tap.x * S.y);
    if (tap.y >= 0.0) {
        const double2 e = fade_phasor(sp[ns * stride], tau);
        g.x = fma(tap.y, e.x, g.x);
        g.y = fma(tap.y, e.y, g.y);
    } else if (tap.x == 0.0) {
        g = make_double2(0.0, 0.0);                          // a tap without power: exact +0
    }
    return g;
}

__global__ __launch_bounds__(256) void fading_params_kernel(FdDraw d, int64_t total, double2 *out) {
    const int ns1 = d.ns + 1;
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
        const int64_t p = idx / ns1;
        out[idx] = fade_sinusoid(d, d.path0 + (uint64_t)p, (int)(idx - p * ns1));
    }
}

constexpr int FT_CHUNK = 128;
struct TapChunk { double2 v[FT_CHUNK]; };

__global__ __launch_bounds__(FT_CHUNK) void fading_taps_kernel(TapChunk c, int cnt, double2 *dst) {
    if ((int)threadIdx.x < cnt) dst[threadIdx.x] = c.v[threadIdx.x];
}

constexpr int FG_BLOCK = 256, FG_LDS = 2048, FG_MAX_PC = 256, FG_MIN_JC = 16, FG_ITEMS = 4096;

struct FgArgs {
    FdDraw d;
    double2 *G;                     // [B][nblk][P]
    const double2 *taps;            // [L] (a_l, c_l)
    int64_t nblk, hold, t0;
    int64_t paths;                  // B P: the paths of the call, numbered row-major (the counters are linear in this number)
    int64_t jchunks, ntiles;
    int P, L, PC, JC;
};

__global__ __launch_bounds__(FG_BLOCK) void fading_gains_kernel(FgArgs a) {
    __shared__ double2 sp[FG_LDS];                          // pair s of the group's path pp at [s * pcn + pp]
    const int ns1 = a.d.ns + 1;
    for (int64_t tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
        const int64_t pg = tile / a.jchunks, jc = tile - pg * a.jchunks;
        const int64_t g0 = pg * a.PC;                       // the group's first path
        const int pcn = a.paths - g0 < a.PC ? (int)(a.paths - g0) : a.PC;
        const int64_t j0 = jc * a.JC;
        const int jcn = a.nblk - j0 < a.JC ? (int)(a.nblk - j0) : a.JC;
        const uint64_t pbase = a.d.path0 + (uint64_t)g0;
        for (int e = threadIdx.x; e < pcn * ns1; e += FG_BLOCK) {
            const int s = e / pcn, pp = e - s * pcn;
            sp[e] = fade_sinusoid(a.d, pbase + (uint64_t)pp, s);
        }
        __syncthreads();
        for (int i = threadIdx.x; i < pcn * jcn; i += FG_BLOCK) {
            const int jj = i / pcn, pp = i - jj * pcn;
            const int64_t j = j0 + jj;
            const int64_t b = (g0 + pp) / a.P;
            const int path = (int)(g0 + pp - b * a.P);
            const double tau = (double)(a.t0 + j * a.hold);  // below 2^52: exact
            a.G[(b * a.nblk + j) * a.P + path] = fade_gain(sp + pp, pcn, a.d.ns, a.taps[path % a.L], tau);
        }
        __syncthreads();
    }
}

// ---- the time-varying convolution ------------------------------------------------------------------------------------------------
constexpr int FC_BLOCK = 256, FC_R = 4, FC_TQ = FC_BLOCK * FC_R, FC_KC = 512;
constexpr int FC_XS = 1920;                                 // padded input tile: (1024 + 512 - 1) * 5 / 4 rounded up
__device__ __forceinline__ int fc_pad(int i) { return i + (i >> 2); }

struct FcArgs {
    const double2 *x;       // [B][nt][n]
    const double2 *g;       // [B][gblk][nr][nt][L] or [gblk][nr][nt][L]: the tap sets of blocks jbase .. jbase + gblk - 1
    double2 *y;             // [B][nr][lout]
    int64_t n, lout, hold;
    int64_t m_lo, m_hi;     // the outputs computed: m_lo <= m < m_hi of every row
    int64_t jbase, gblk;
    int64_t tiles_per_row, ntiles;
    int64_t total;          // B nr (m_hi - m_lo) (direct kernel)
    int nt, nr, L, g_batched;
};

template <int NRG>
__global__ __launch_bounds__(FC_BLOCK) void fading_tiled_kernel(FcArgs a) {
    constexpr int R = FC_R;
    __shared__ double2 tl[CPX_FD_MAX_TAPS];
    __shared__ double2 xs[FC_XS];
    const int t = threadIdx.x;
    const int ntaps = a.nr * a.nt * a.L;
    bool staged = false;
    for (int64_t tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
        const int64_t b = tile / a.tiles_per_row;
        const int64_t q0 = a.m_lo + (tile - b * a.tiles_per_row) * FC_TQ;
        const int64_t mend = (q0 + FC_TQ < a.m_hi ? q0 + FC_TQ : a.m_hi) - 1;   // the tile's last output
        const int64_t j0 = q0 / a.hold;
        const int nsets = (int)(mend / a.hold - j0) + 1;    // the host made sure that nsets ntaps <= CPX_FD_MAX_TAPS
        if (a.g_batched || a.gblk > 1 || !staged) {         // uniform; readable after the first barrier below
            const double2 *g = a.g + ((a.g_batched ? b : 0) * a.gblk + (j0 - a.jbase)) * ntaps;
            for (int i = t; i < nsets * ntaps; i += FC_BLOCK) tl[i] = g[i];
            staged = true;
        }
        int soff[R];                                        // the tap set of each of this thread's outputs
#pragma unroll
        for (int r = 0; r < R; r++) {
            const int64_t m = q0 + t * R + r;
            soff[r] = (int)((m < mend ? m : mend) / a.hold - j0) * ntaps;
        }
        const bool same = soff[0] == soff[R - 1];
        for (int r0 = 0; r0 < a.nr; r0 += NRG) {
            double2 acc[NRG][R];
#pragma unroll
            for (int i = 0; i < NRG; i++)
#pragma unroll
                for (int r = 0; r < R; r++) acc[i][r] = make_double2(0.0, 0.0);
            for (int tx = 0; tx < a.nt; tx++) {
                const double2 *x = a.x + (b * a.nt + tx) * a.n;
                for (int jc = 0; jc < a.L; jc += FC_KC) {
                    const int JCn = a.L - jc < FC_KC ? a.L - jc : FC_KC;
                    const int JCpad = (JCn + R - 1) / R * R;
                    // LDS position w holds x[q0 - (jc + JCpad - 1) + w]
                    const int64_t s0 = q0 - (jc + JCpad - 1);
                    const int W = FC_TQ + JCpad - 1;
                    for (int w = t; w < W; w += FC_BLOCK) {
                        const int64_t s = s0 + w;
                        xs[fc_pad(w)] = (s >= 0 && s < a.n) ? x[s] : make_double2(0.0, 0.0);
                    }
                    __syncthreads();
                    const int base = t * R;
                    // an antenna past nr repeats the last one (its sums are not stored)
                    const int tap0 = tx * a.L + jc;
                    int toff[NRG];
#pragma unroll
                    for (int i = 0; i < NRG; i++) toff[i] = (r0 + i < a.nr ? r0 + i : a.nr - 1) * a.nt * a.L;
                    double2 xr[R];                          // xr[(r + R - 1 - u) mod R] = the input of output r at step u
#pragma unroll
                    for (int r = 0; r < R; r++) xr[(r + R - 1) % R] = xs[fc_pad(base + r + JCpad - 1)];
                    for (int ua = 0; ua < JCpad; ua += R) {
#pragma unroll
                        for (int bb = 0; bb < R; bb++) {
                            const int u = ua + bb;
                            if (u < JCn) {                  // no tap, no term
#pragma unroll
                                for (int i = 0; i < NRG; i++) {
                                    const int ti = tap0 + toff[i] + u;
                                    if (same) {
                                        const double2 tap = tl[soff[0] + ti];
#pragma unroll
                                        for (int r = 0; r < R; r++) mac(acc[i][r], tap, xr[(r + R - 1 - bb) % R]);
                                    } else {
#pragma unroll
                                        for (int r = 0; r < R; r++) mac(acc[i][r], tl[soff[r] + ti], xr[(r + R - 1 - bb) % R]);
                                    }
                                }
                            }
                            if (u + 1 < JCpad) xr[(2 * R - 2 - bb) % R] = xs[fc_pad(base + JCpad - 2 - u)];
                        }
                    }
                    __syncthreads();
                }
            }
#pragma unroll
            for (int i = 0; i < NRG; i++) {
                if (r0 + i < a.nr) {
                    double2 *o = a.y + (b * a.nr + r0 + i) * a.lout;
#pragma unroll
                    for (int r = 0; r < R; r++) {
                        const int64_t m = q0 + t * R + r;
                        if (m < a.m_hi) o[m] = acc[i][r];
                    }
                }
            }
        }
    }
}

__global__ __launch_bounds__(256) void fading_direct_kernel(FcArgs a) {
    const int64_t span = a.m_hi - a.m_lo;
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < a.total; idx += (int64_t)gridDim.x * blockDim.x) {
        const int64_t q = idx / span, m = a.m_lo + (idx - q * span);
        const int64_t b = q / a.nr;
        const int r = (int)(q - b * a.nr);
        const double2 *g = a.g + (((a.g_batched ? b : 0) * a.gblk + (m / a.hold - a.jbase)) * a.nr + r) * a.nt * a.L;
        const int klo = m - (a.n - 1) > 0 ? (int)(m - (a.n - 1)) : 0;
        const int khi = m < a.L - 1 ? (int)m : a.L - 1;
        double2 acc = make_double2(0.0, 0.0);
        for (int tx = 0; tx < a.nt; tx++) {
            const double2 *x = a.x + (b * a.nt + tx) * a.n;
            for (int k = klo; k <= khi; k++) mac(acc, g[tx * a.L + k], x[m - k]);
        }
        a.y[q * a.lout + m] = acc;
    }
}

// ---- checks (all before ensure_device) -------------------------------------------------------------------------------------------
int shape_check(const char *what, int64_t B, int nr, int nt, int L) {
    CPX_REQUIRE(B >= 0, CPX_EINVAL, "%s: negative batch size", what);
    CPX_REQUIRE(nt >= 1 && nr >= 1 && L >= 1, CPX_EINVAL, "%s: nt = %d, nr = %d, L = %d, need at least 1 of each", what, nt, nr, L);
    CPX_REQUIRE(L <= CPX_FD_MAX_L, CPX_ELIMIT, "%s: L = %d is above the engine's limit of %d", what, L, CPX_FD_MAX_L);
    CPX_REQUIRE((int64_t)nr * nt * L <= CPX_FD_MAX_TAPS, CPX_ELIMIT, "%s: nr nt L = %lld taps per block are above the engine's limit of %d",
                what, (long long)nr * nt * L, CPX_FD_MAX_TAPS);
    return CPX_OK;
}

int draw_check(const char *what, int64_t B, int nr, int nt, int L, int ns, double fd, double fd_los) {
    if (int rc = shape_check(what, B, nr, nt, L)) return rc;
    CPX_REQUIRE(ns >= 1, CPX_EINVAL, "%s: %d sinusoids per path, need at least 1", what, ns);
    CPX_REQUIRE(ns <= CPX_FD_MAX_SIN, CPX_ELIMIT, "%s: %d sinusoids per path are above the engine's limit of %d", what, ns, CPX_FD_MAX_SIN);
    CPX_REQUIRE(fd >= 0.0 && fd <= 0.5, CPX_EINVAL, "%s: fd = %g cycles per sample is outside [0, 0.5]", what, fd);
    CPX_REQUIRE(fd_los >= -0.5 && fd_los <= 0.5, CPX_EINVAL, "%s: fd_los = %g cycles per sample is outside [-0.5, 0.5]", what, fd_los);
    CPX_REQUIRE(B == 0 || B <= INT64_MAX / 64 / ((int64_t)nr * nt * L * (ns + 1)), CPX_EINVAL, "%s: %lld rows overflow", what, (long long)B);
    return CPX_OK;
}

int time_check(const char *what, int64_t B, int nr, int nt, int L, int64_t hold, int64_t t0, int64_t nblk) {
    CPX_REQUIRE(hold >= 1, CPX_EINVAL, "%s: hold = %lld samples per block, need at least 1", what, (long long)hold);
    CPX_REQUIRE(t0 >= 0, CPX_EINVAL, "%s: t0 = %lld is negative", what, (long long)t0);
    CPX_REQUIRE(nblk >= 1, CPX_EINVAL, "%s: %lld blocks, need at least 1", what, (long long)nblk);
    CPX_REQUIRE(t0 < FD_TWO52 && hold < FD_TWO52 && nblk <= (FD_TWO52 - 1 - t0) / hold, CPX_EINVAL,
                "%s: t0 + nblk hold reaches 2^52 (t0 = %lld, nblk = %lld, hold = %lld)", what, (long long)t0, (long long)nblk, (long long)hold);
    CPX_REQUIRE(B == 0 || nblk <= INT64_MAX / 64 / B / ((int64_t)nr * nt * L), CPX_EINVAL, "%s: %lld x %lld tap sets overflow", what,
                (long long)B, (long long)nblk);
    return CPX_OK;
}

int conv_check(const char *what, int g_batched, int64_t B, int nt, int nr, int64_t n, int L, int64_t hold) {
    if (int rc = shape_check(what, B, nr, nt, L)) return rc;
    CPX_REQUIRE(g_batched == 0 || g_batched == 1, CPX_EINVAL, "%s: g_batched = %d, need 0 or 1", what, g_batched);
    CPX_REQUIRE(B == 0 || n >= 1, CPX_EINVAL, "%s: n = %lld (an empty row cannot be convolved)", what, (long long)n);
    CPX_REQUIRE(hold >= 1, CPX_EINVAL, "%s: hold = %lld samples per block, need at least 1", what, (long long)hold);
    CPX_REQUIRE(B == 0 || n <= (INT64_MAX / 64 - L) / B / ((int64_t)nr * nt * L), CPX_EINVAL, "%s: %lld x %lld samples overflow", what,
                (long long)B, (long long)n);
    return CPX_OK;
}

// the per-tap scales (a_l, c_l) of the header, c_l = -1 where there is no line of sight (kf == 0, or a tap without power)
int tap_scales(const char *what, const double *pdp, const double *kf, int L, int ns, std::vector<double2> &out) {
    out.resize(L);
    for (int l = 0; l < L; l++) {
        const double p = pdp[l], k = kf ? kf[l] : 0.0;
        CPX_REQUIRE(std::isfinite(p) && p >= 0.0, CPX_EINVAL, "%s: pdp[%d] = %g is not a finite power >= 0", what, l, p);
        CPX_REQUIRE(std::isfinite(k) && k >= 0.0, CPX_EINVAL, "%s: kf[%d] = %g is not a finite K factor >= 0", what, l, k);
        const double a = std::sqrt(p / ((1.0 + k) * (double)ns));
        const double c = std::sqrt(p * k / (1.0 + k));
        CPX_REQUIRE(std::isfinite(a) && std::isfinite(c), CPX_EINVAL, "%s: pdp[%d] kf[%d] overflows", what, l, l);
        out[l] = make_double2(p == 0.0 ? 0.0 : a, (k > 0.0 && p > 0.0) ? c : -1.0);
    }
    return CPX_OK;
}

struct FdModel {
    int nr, nt, L, ns;
    double fd, fd_los;
    int64_t hold;
    uint64_t seed, stream, first_row;
    FdDraw draw() const {
        return FdDraw{seed, stream, first_row * (uint64_t)((int64_t)nr * nt * L), fd, fd_los, ns};
    }
};

// ---- launchers -------------------------------------------------------------------------------------------------------------------
int launch_taps(Scratch &sc, const std::vector<double2> &taps, hipStream_t st, const double2 **d_taps) {
    double2 *dst = nullptr;
    if (int rc = sc.get(st, Slot::fading_taps, 16 * (size_t)CPX_FD_MAX_L, &dst)) return rc;
    for (size_t off = 0; off < taps.size(); off += FT_CHUNK) {
        TapChunk c{};
        const int cnt = (int)(taps.size() - off < (size_t)FT_CHUNK ? taps.size() - off : (size_t)FT_CHUNK);
        for (int i = 0; i < cnt; i++) c.v[i] = taps[off + i];
        hipLaunchKernelGGL(fading_taps_kernel, dim3(1), dim3(FT_CHUNK), 0, st, c, cnt, dst + off);
    }
    CPX_HIP(hipGetLastError());
    *d_taps = dst;
    return CPX_OK;
}

// rows first_row + b0 .. + b0 + B - 1 of the model, blocks j0 .. j0 + nblk - 1 from t0 -> G [B][nblk][P]
int launch_gains(const FdModel &md, const double2 *d_taps, int64_t b0, int64_t B, int64_t t0, int64_t j0, int64_t nblk, double2 *G,
                 hipStream_t st) {
    FgArgs a{};
    a.P = md.nr * md.nt * md.L;
    a.L = md.L;
    a.d = md.draw();
    a.d.path0 += (uint64_t)b0 * (uint64_t)a.P;
    a.G = G;
    a.taps = d_taps;
    a.nblk = nblk;
    a.hold = md.hold;
    a.t0 = t0 + j0 * md.hold;
    a.paths = B * a.P;
    int64_t pc = FG_LDS / (md.ns + 1);
    if (pc > FG_MAX_PC) pc = FG_MAX_PC;
    if (pc > a.paths) pc = a.paths;
    a.PC = (int)pc;
    int64_t jc = (FG_ITEMS + pc - 1) / pc;
    if (jc < FG_MIN_JC) jc = FG_MIN_JC;
    if (jc > nblk) jc = nblk;
    a.JC = (int)jc;
    a.jchunks = (nblk + jc - 1) / jc;
    a.ntiles = ((a.paths + pc - 1) / pc) * a.jchunks;
    hipLaunchKernelGGL(fading_gains_kernel, dim3(grid_of(a.ntiles)), dim3(FG_BLOCK), 0, st, a);
    CPX_HIP(hipGetLastError());
    return CPX_OK;
}

// the most blocks that FC_TQ consecutive outputs can meet
int64_t sets_per_tile(int64_t hold) { return (FC_TQ - 2 + hold) / hold + 1; }

// outputs m_lo <= m < m_hi of B rows; g holds the tap sets of blocks jbase .. jbase + gblk - 1.  *name: the kernel launched
int launch_convolve(const double2 *x, const double2 *g, int g_batched, int64_t B, int nt, int nr, int64_t n, int L, int64_t hold,
                    double2 *y, int64_t m_lo, int64_t m_hi, int64_t jbase, int64_t gblk, hipStream_t st, char *name, size_t name_len) {
    FcArgs a{};
    a.x = x; a.g = g; a.y = y;
    a.n = n;
    a.lout = n + L - 1;
    a.hold = hold;
    a.m_lo = m_lo; a.m_hi = m_hi;
    a.jbase = jbase; a.gblk = gblk;
    a.nt = nt; a.nr = nr; a.L = L; a.g_batched = g_batched;
    const int64_t span = m_hi - m_lo;
    a.total = B * nr * span;
    const int64_t blocks = (m_hi - 1) / hold - m_lo / hold + 1;
    int64_t sets = sets_per_tile(hold);
    if (sets > blocks) sets = blocks;
    // the tiled kernel when a row's tiles are at least half full and the tap sets under a tile fit the LDS
    if (2 * span >= FC_TQ && sets * ((int64_t)nr * nt * L) <= CPX_FD_MAX_TAPS) {
        a.tiles_per_row = (span + FC_TQ - 1) / FC_TQ;
        a.ntiles = B * a.tiles_per_row;
        const dim3 grid(grid_of(a.ntiles)), block(FC_BLOCK);
        const int nrg = nr >= 3 ? 4 : nr;
        if (nrg == 4) hipLaunchKernelGGL(fading_tiled_kernel<4>, grid, block, 0, st, a);
        else if (nrg == 2) hipLaunchKernelGGL(fading_tiled_kernel<2>, grid, block, 0, st, a);
        else hipLaunchKernelGGL(fading_tiled_kernel<1>, grid, block, 0, st, a);
        CPX_HIP(hipGetLastError());
        snprintf(name, name_len, "fading_tiled_kernel<%d>", nrg);
        return CPX_OK;
    }
    hipLaunchKernelGGL(fading_direct_kernel, dim3(grid_of((a.total + 255) / 256)), dim3(256), 0, st, a);
    CPX_HIP(hipGetLastError());
    snprintf(name, name_len, "fading_direct_kernel");
    return CPX_OK;
}

}  // namespace

extern "C" {

int cpx_fading_params_dev(int64_t B, int nr, int nt, int L, int n_sin, double fd, double fd_los, uint64_t seed, uint64_t stream_id,
                          uint64_t first_row, double *d_params, void *stream) {
    CPX_TRACE("cpx_fading_params_dev");
    if (int rc = draw_check("fading_params", B, nr, nt, L, n_sin, fd, fd_los)) return rc;
    if (B == 0) return CPX_OK;
    CPX_REQUIRE(d_params, CPX_EINVAL, "fading_params: null pointer");
    const FdModel md{nr, nt, L, n_sin, fd, fd_los, 1, seed, stream_id, first_row};
    const int64_t total = B * nr * nt * L * (n_sin + 1);
    hipLaunchKernelGGL(fading_params_kernel, dim3(grid_of((total + 255) / 256)), dim3(256), 0, pick_stream(stream), md.draw(), total,
                       reinterpret_cast<double2 *>(d_params));
    CPX_HIP(hipGetLastError());
    note_kernel("fading_params_kernel");
    return CPX_OK;
}

int cpx_fading_params(int64_t B, int nr, int nt, int L, int n_sin, double fd, double fd_los, uint64_t seed, uint64_t stream_id,
                      uint64_t first_row, double *params) {
    CPX_TRACE("cpx_fading_params");
    if (int rc = draw_check("fading_params", B, nr, nt, L, n_sin, fd, fd_los)) return rc;
    if (B == 0) return CPX_OK;
    CPX_REQUIRE(params, CPX_EINVAL, "fading_params: null pointer");
    int rc = ensure_device();
    if (rc) return rc;
    const size_t bytes = 16 * (size_t)(B * nr * nt * L * (n_sin + 1));
    HostStage s;
    double *dp;
    if ((rc = s.out(bytes, &dp)) || (rc = cpx_fading_params_dev(B, nr, nt, L, n_sin, fd, fd_los, seed, stream_id, first_row, dp, s.st)))
        return rc;
    return s.get(params, dp, bytes);
}

int cpx_fading_gains_dev(int64_t B, int nr, int nt, int L, const double *pdp, const double *kf, int n_sin, double fd, double fd_los,
                         int64_t hold, int64_t t0, int64_t nblk, uint64_t seed, uint64_t stream_id, uint64_t first_row,
                         double *d_G_re_im, void *stream) {
    CPX_TRACE("cpx_fading_gains_dev");
    if (int rc = draw_check("fading_gains", B, nr, nt, L, n_sin, fd, fd_los)) return rc;
    if (int rc = time_check("fading_gains", B, nr, nt, L, hold, t0, nblk)) return rc;
    if (B == 0) return CPX_OK;
    CPX_REQUIRE(pdp && d_G_re_im, CPX_EINVAL, "fading_gains: null pointer");
    std::vector<double2> taps;
    if (int rc = tap_scales("fading_gains", pdp, kf, L, n_sin, taps)) return rc;
    const FdModel md{nr, nt, L, n_sin, fd, fd_los, hold, seed, stream_id, first_row};
    hipStream_t st = pick_stream(stream);
    Scratch sc;
    const double2 *d_taps;
    if (int rc = launch_taps(sc, taps, st, &d_taps)) return rc;
    if (int rc = launch_gains(md, d_taps, 0, B, t0, 0, nblk, reinterpret_cast<double2 *>(d_G_re_im), st)) return rc;
    note_kernel("fading_gains_kernel");
    return CPX_OK;
}

int cpx_fading_gains(int64_t B, int nr, int nt, int L, const double *pdp, const double *kf, int n_sin, double fd, double fd_los,
                     int64_t hold, int64_t t0, int64_t nblk, uint64_t seed, uint64_t stream_id, uint64_t first_row, double *G_re_im) {
    CPX_TRACE("cpx_fading_gains");
    if (int rc = draw_check("fading_gains", B, nr, nt, L, n_sin, fd, fd_los)) return rc;
    if (int rc = time_check("fading_gains", B, nr, nt, L, hold, t0, nblk)) return rc;
    if (B == 0) return CPX_OK;
    CPX_REQUIRE(pdp && G_re_im, CPX_EINVAL, "fading_gains: null pointer");
    std::vector<double2> taps;
    int rc = tap_scales("fading_gains", pdp, kf, L, n_sin, taps);
    if (rc || (rc = ensure_device())) return rc;
    const size_t bytes = 16 * (size_t)(B * nblk * nr * nt * L);
    HostStage s;
    double *dg;
    if ((rc = s.out(bytes, &dg)) ||
        (rc = cpx_fading_gains_dev(B, nr, nt, L, pdp, kf, n_sin, fd, fd_los, hold, t0, nblk, seed, stream_id, first_row, dg, s.st)))
        return rc;
    return s.get(G_re_im, dg, bytes);
}

int cpx_fading_convolve_dev(const double *d_x_re_im, const double *d_G_re_im, int g_batched, int64_t B, int nt, int nr, int64_t n, int L,
                            int64_t hold, double *d_y_re_im, void *stream) {
    CPX_TRACE("cpx_fading_convolve_dev");
    if (int rc = conv_check("fading_convolve", g_batched, B, nt, nr, n, L, hold)) return rc;
    if (B == 0) return CPX_OK;
    CPX_REQUIRE(d_x_re_im && d_G_re_im && d_y_re_im, CPX_EINVAL, "fading_convolve: null pointer");
    const int64_t lout = n + L - 1, nblk = (lout + hold - 1) / hold;
    char name[64];
    if (int rc = launch_convolve(reinterpret_cast<const double2 *>(d_x_re_im), reinterpret_cast<const double2 *>(d_G_re_im), g_batched, B, nt,
                                 nr, n, L, hold, reinterpret_cast<double2 *>(d_y_re_im), 0, lout, 0, nblk, pick_stream(stream), name,
                                 sizeof name))
        return rc;
    note_kernel("%s", name);
    return CPX_OK;
}

int cpx_fading_convolve(const double *x_re_im, const double *G_re_im, int g_batched, int64_t B, int nt, int nr, int64_t n, int L,
                        int64_t hold, double *y_re_im) {
    CPX_TRACE("cpx_fading_convolve");
    if (int rc = conv_check("fading_convolve", g_batched, B, nt, nr, n, L, hold)) return rc;
    if (B == 0) return CPX_OK;
    CPX_REQUIRE(x_re_im && G_re_im && y_re_im, CPX_EINVAL, "fading_convolve: null pointer");
    int rc = ensure_device();
    if (rc) return rc;
    const int64_t lout = n + L - 1, nblk = (lout + hold - 1) / hold;
    const size_t x_bytes = 16 * (size_t)(B * nt * n), g_bytes = 16 * (size_t)((g_batched ? B : 1) * nblk * nr * nt * L),
                 y_bytes = 16 * (size_t)(B * nr * lout);
    HostStage s;
    const double *dx, *dg;
    double *dy;
    if ((rc = s.in(x_re_im, x_bytes, &dx)) || (rc = s.in(G_re_im, g_bytes, &dg)) || (rc = s.out(y_bytes, &dy)) ||
        (rc = cpx_fading_convolve_dev(dx, dg, g_batched, B, nt, nr, n, L, hold, dy, s.st)))
        return rc;
    return s.get(y_re_im, dy, y_bytes);
}

// the checks shared by both forms of cpx_fading_channel; *nblk = the blocks of a row
static int channel_check(int64_t B, int nt, int nr, int64_t n, int L, int n_sin, double fd, double fd_los, int64_t hold, int64_t t0,
                         int64_t *nblk) {
    if (int rc = draw_check("fading_channel", B, nr, nt, L, n_sin, fd, fd_los)) return rc;
    if (int rc = conv_check("fading_channel", 1, B, nt, nr, n, L, hold)) return rc;
    *nblk = B == 0 ? 1 : (n + L - 1 + hold - 1) / hold;
    return time_check("fading_channel", B, nr, nt, L, hold, t0, *nblk);
}

int cpx_fading_channel_dev(const double *d_x_re_im, int64_t B, int nt, int nr, int64_t n, int L, const double *pdp, const double *kf,
                           int n_sin, double fd, double fd_los, int64_t hold, int64_t t0, uint64_t seed, uint64_t stream_id,
                           uint64_t first_row, double *d_y_re_im, double *d_G_re_im, void *stream) {
    CPX_TRACE("cpx_fading_channel_dev");
    int64_t nblk = 0;
    if (int rc = channel_check(B, nt, nr, n, L, n_sin, fd, fd_los, hold, t0, &nblk)) return rc;
    CPX_REQUIRE(d_y_re_im || d_G_re_im, CPX_EINVAL, "fading_channel: no output requested");
    if (B == 0) return CPX_OK;
    CPX_REQUIRE(pdp && (d_x_re_im || !d_y_re_im), CPX_EINVAL, "fading_channel: null pointer");
    std::vector<double2> taps;
    if (int rc = tap_scales("fading_channel", pdp, kf, L, n_sin, taps)) return rc;
    const FdModel md{nr, nt, L, n_sin, fd, fd_los, hold, seed, stream_id, first_row};
    hipStream_t st = pick_stream(stream);
    const double2 *x = reinterpret_cast<const double2 *>(d_x_re_im);
    double2 *y = reinterpret_cast<double2 *>(d_y_re_im);
    const int64_t lout = n + L - 1, ntaps = (int64_t)nr * nt * L;
    char name[64] = "";
    Scratch sc;
    const double2 *d_taps;
    if (int rc = launch_taps(sc, taps, st, &d_taps)) return rc;
    if (d_G_re_im) {
        double2 *G = reinterpret_cast<double2 *>(d_G_re_im);
        if (int rc = launch_gains(md, d_taps, 0, B, t0, 0, nblk, G, st)) return rc;
        if (!y) {
            note_kernel("fading_gains_kernel");
            return CPX_OK;
        }
        if (int rc = launch_convolve(x, G, 1, B, nt, nr, n, L, hold, y, 0, lout, 0, nblk, st, name, sizeof name)) return rc;
        note_kernel("fading_gains_kernel+%s", name);
        return CPX_OK;
    }
    // the gains in the scratch arena, at most CPX_FADING_SCRATCH_BYTES at a time: chunks of whole rows, or, where one row's gains are
    // above the budget, of whole blocks of one row.  Gains and sums are pure functions of their indices: the chunks change nothing.
    const int64_t budget = CPX_FADING_SCRATCH_BYTES / 16;                   // complex values
    const int64_t row = nblk * ntaps;
    double2 *G = nullptr;
    int64_t chunks = 0;
    if (row <= budget) {
        int64_t rows = budget / row;
        if (rows > B) rows = B;
        if (int rc = sc.get(st, Slot::fading_gains, 16 * (size_t)(rows * row), &G)) return rc;
        for (int64_t b0 = 0; b0 < B; b0 += rows, chunks++) {
            const int64_t bn = B - b0 < rows ? B - b0 : rows;
            if (int rc = launch_gains(md, d_taps, b0, bn, t0, 0, nblk, G, st)) return rc;
            if (int rc = launch_convolve(x + b0 * nt * n, G, 1, bn, nt, nr, n, L, hold, y + b0 * nr * lout, 0, lout, 0, nblk, st, name,
                                         sizeof name))
                return rc;
        }
    } else {
        const int64_t per = budget / ntaps;                                  // blocks per chunk, at least 2048
        if (int rc = sc.get(st, Slot::fading_gains, 16 * (size_t)(per * ntaps), &G)) return rc;
        for (int64_t b = 0; b < B; b++) {
            for (int64_t j0 = 0; j0 < nblk; j0 += per, chunks++) {
                const int64_t jn = nblk - j0 < per ? nblk - j0 : per;
                const int64_t m_hi = (j0 + jn) * hold < lout ? (j0 + jn) * hold : lout;
                if (int rc = launch_gains(md, d_taps, b, 1, t0, j0, jn, G, st)) return rc;
                if (int rc = launch_convolve(x + b * nt * n, G, 1, 1, nt, nr, n, L, hold, y + b * nr * lout, j0 * hold, m_hi, j0, jn, st,
                                             name, sizeof name))
                    return rc;
            }
        }
    }
    note_kernel("fading_gains_kernel+%s (%lld chunks)", name, (long long)chunks);
    return CPX_OK;
}

int cpx_fading_channel(const double *x_re_im, int64_t B, int nt, int nr, int64_t n, int L, const double *pdp, const double *kf, int n_sin,
                       double fd, double fd_los, int64_t hold, int64_t t0, uint64_t seed, uint64_t stream_id, uint64_t first_row,
                       double *y_re_im, double *G_re_im) {
    CPX_TRACE("cpx_fading_channel");
    int64_t nblk = 0;
    if (int rc = channel_check(B, nt, nr, n, L, n_sin, fd, fd_los, hold, t0, &nblk)) return rc;
    CPX_REQUIRE(y_re_im || G_re_im, CPX_EINVAL, "fading_channel: no output requested");
    if (B == 0) return CPX_OK;
    CPX_REQUIRE(pdp && (x_re_im || !y_re_im), CPX_EINVAL, "fading_channel: null pointer");
    std::vector<double2> taps;
    int rc = tap_scales("fading_channel", pdp, kf, L, n_sin, taps);
    if (rc || (rc = ensure_device())) return rc;
    const size_t x_bytes = 16 * (size_t)(B * nt * n), g_bytes = 16 * (size_t)(B * nblk * nr * nt * L), y_bytes = 16 * (size_t)(B * nr * (n + L - 1));
    HostStage s;
    const double *dx = nullptr;
    double *dy = nullptr, *dg = nullptr;
    if (y_re_im && ((rc = s.in(x_re_im, x_bytes, &dx)) || (rc = s.out(y_bytes, &dy)))) return rc;
    if (G_re_im && (rc = s.out(g_bytes, &dg))) return rc;
    if ((rc = cpx_fading_channel_dev(dx, B, nt, nr, n, L, pdp, kf, n_sin, fd, fd_los, hold, t0, seed, stream_id, first_row, dy, dg, s.st)))
        return rc;
    if (y_re_im && (rc = s.get(y_re_im, dy, y_bytes))) return rc;
    return G_re_im ? s.get(G_re_im, dg, g_bytes) : CPX_OK;
}

}  // extern "C"
