// The frequency-selective channel and pilot-aided OFDM channel estimation, batched, complex128 with float64
// arithmetic only (cpx_set_precision does not apply).  Not in the reference; the yardstick is the NumPy model of tests/ofdm_chan_model.py.
//
//   multipath   y[b][r] = sum_t convolve(x[b][t], g[b][r][t])                                   x [B][nt][n] -> y [B][nr][n + L - 1]
//   map         data [B][ndata][nt] + the plan's pilots -> grid [B][nt][nsym][nsc] (cpx_ofdm_tx's input for B nt rows)
//   estimate    Y [B][nr][nsym][nsc] (cpx_ofdm_rx's output) -> H^ per subcarrier, and (y, H^) per data element in the MIMO
//               detectors' layout: y_data [B][ndata][nr], h_data [B][ndata][nr][nt]
//
// Multipath: every output sample is ONE chain of fused multiply-adds from +0 over t ascending, then tap index ascending (per
// complex tap re += gr xr, re -= gi xi, im += gr xi, im += gi xr: cpx_wave.h's mac, fir.hip's too).  Terms under a row's edges are
// skipped (direct kernel) or meet zero inputs (tiled kernel), which leaves the chain's value unchanged for finite data: the result depends on
// (nt, L, n, index in the row) alone, never on B, the row's place, the stream or whether g is shared.  The row's shape picks the
// kernel (no process-wide switch):
//   multipath_kernel<NRG>   n + L - 1 >= 512.  A workgroup of 256 threads owns 1024 consecutive output positions of one b, for ALL
//       receive antennas: the taps g[b] (at most 2048, 32 KB) are staged in the LDS once, the window of x[b][t] under the tile once
//       per t (and per group of NRG = 1, 2 or 4 receive antennas; nr <= 4 is one group, so each window comes from HBM once).  A
//       thread owns 4 consecutive positions of NRG antennas: per tap NRG broadcast reads of the tap and ONE new input -- the four
//       inputs of a step slide through registers, as in fir_interp_kernel at sps = 1 -- for 16 NRG FMAs.  Taps in chunks of 512.
//       A group's antennas past nr repeat the last one and are not stored (nr = 3 does the arithmetic of 4).
//   multipath_direct        shorter rows: one output per thread over the flattened batch, operands from global memory (L1 / L2).
//
// Estimation, least squares at the pilots then a caller-supplied interpolation matrix per transmit antenna (the engine does not
// interpret W: linear, time-limited and Wiener interpolation are all "a matrix"):
//   ofdm_ls_kernel       LS[b][i][r] = (sum_s Y[b][r][s][k] c_s) / count over the pilots of item i = (antenna t, its j-th pilot
//                        subcarrier k) in ascending symbol order, c_s = conj(p_s) / |p_s|^2 formed on the host; one item per thread.
//   ofdm_interp_kernel   H^[b][k][r][t] = sum_j W_t[k][j] LS[b][t, j][r], an fma chain from +0 over ascending j.  A workgroup owns
//                        64 subcarriers x 32 columns (b, r) of one antenna: the W_t tile [16 j][64 k] is staged in the LDS once and
//                        shared by all 32 columns (a thread: one k, 8 columns of its wave, whose LS values are LDS broadcasts).
//   ofdm_hdemap_kernel   h_data[b][d] = H^[b][sc(d)], runs of nr nt contiguous complex values, read while H^ is still in the L2.
//   ofdm_ydemap_kernel   y_data[b][d][r] = Y[b][r][re(d)]: the transposition goes through the LDS (odd row stride), so that loads
//                        run along the subcarriers and stores are one contiguous run per workgroup.
//   ofdm_map_kernel      the inverse for the transmitter: a contiguous run of data vectors -> LDS -> one row of the grid per antenna.
// Time tracking (cpx_pilots_create_tv / cpx_pilots_estimate_tv): the estimator is separable, frequency first, then time.
// Antenna t's pilots form a rectangle, its pilot symbols s_0 < ... < s_{ns_t - 1} times its pilot subcarriers; a second caller-supplied
// matrix V_t [nsym][ns_t] spreads the estimates at the pilot symbols over all symbols (linear, hold, Wiener: all "a matrix").
//   ofdm_ls_kernel          on tables with ONE pilot per item (t, i, j): LSp = Y[s_i][k_j] c, one mac from +0 (its division by 1 is exact)
//   ofdm_interp_kernel<1>   Hp[b][i][k][r][t] = sum_j W_t[k][j] LSp[b][r][t][i][j]: the same tile and chain with columns (b, r, i)
//   ofdm_tv_kernel          H^[b][s][k][r][t] = sum_i V_t[s][i] Hp[b][i][k][r][t], a chain of mac from +0 over ascending i, fused with the
//                           demap.  A workgroup owns 256 consecutive values of one frame's [nsc][nr][nt] plane: a thread loads its
//                           element of Hp for the first 4 pilot symbols once into registers (further ones are read again per symbol,
//                           from the L1 / L2), then loops over the symbols; per symbol it stores the value to h_sym (if requested) and,
//                           where the resource element carries data, to h_data -- consecutive lanes, consecutive addresses, since the
//                           data elements of a symbol are numbered by ascending subcarrier.  H^ per symbol is never read back.  V
//                           (all antennas) is staged in the LDS once per workgroup where it fits 16 KB.
// On the host both estimators are sequences of the same steps (est_begin, est_ls_interp on the estimator's tables and Interp,
// est_ydemap_end); each adds only its own launch between them, ofdm_hdemap_kernel or ofdm_tv_kernel.
// Every output element goes through the same operations wherever its frame sits in the batch: bit-identical across batch sizes,
// positions, streams and whichever outputs are requested; a frame's samples meet no other frame's (NaN isolation).  Offsets 64-bit.
#include "cpx_internal.h"
#include "cpx_wave.h"             // mac: the chain step shared with fir.hip and fading.hip; grid_of

#include <algorithm>
#include <climits>
#include <cmath>

using namespace cpx;

#define CPX_MP_MAX_L 1024
#define CPX_MP_MAX_TAPS 2048       // nr nt L of one row: 32 KB of LDS
#define CPX_OC_MAX_ANT 1024        // nt of a plan, nr of an estimate: one resource element's antennas must fit an LDS tile

struct cpx_ofdm_pilots {
    __attribute__((visibility("hidden"))) ~cpx_ofdm_pilots() = default;
    int nsc, nsym, nt, device;
    int64_t npil, ndata, nls;       // nls = sum_t np_t, the least-squares items of a (b, r)
    int32_t *d_code = nullptr;      // [nsym nsc] data element d >= 0, or -1 - i for pilot i
    int32_t *d_dcount = nullptr;    // [nsym nsc + 1] data elements in front of each resource element
    int32_t *d_data_re = nullptr;   // [ndata] sym nsc + sc
    int32_t *d_data_sc = nullptr;   // [ndata]
    int32_t *d_pil_tx = nullptr;    // [npil]
    double2 *d_pil_val = nullptr;   // [npil]
    int32_t *d_ls_ptr = nullptr;    // [nls + 1] into the pilots sorted by (antenna, subcarrier, symbol)
    int32_t *d_ls_re = nullptr;     // [npil] resource element of each sorted pilot
    double2 *d_ls_coef = nullptr;   // [npil] conj(p) / |p|^2
    int64_t *d_ant = nullptr;       // [nt][3] np_t, first item, offset of W_t in d_w (complex values)
    double2 *d_w = nullptr;         // W_0 [nsc][np_0], W_1 ...
    // time tracking (cpx_pilots_create_tv), absent (ns_max = 0) in a plan of cpx_pilots_create
    int ns_max = 0;                 // the most pilot symbols of an antenna
    int64_t nlsp = 0, nv = 0;       // nlsp = sum_t ns_t np_t items (t, i, j) of a (b, r); nv = sum_t nsym ns_t entries of V
    int32_t *d_tv_ptr = nullptr;    // [nlsp + 1] 0, 1, 2 ...: ofdm_ls_kernel's tables with one pilot per item, ordered (t, i, j)
    int32_t *d_tv_re = nullptr;     // [nlsp] resource element s_i nsc + k_j
    double2 *d_tv_coef = nullptr;   // [nlsp] conj(p) / |p|^2
    int64_t *d_tv_ant = nullptr;    // [nt][3] ns_t, first item, offset of V_t in d_v (complex values)
    double2 *d_v = nullptr;         // V_0 [nsym][ns_0], V_1 ...
};

namespace {

// ---- multipath -------------------------------------------------------------------------------------------------------------
constexpr int MP_BLOCK = 256, MP_R = 4, MP_TQ = MP_BLOCK * MP_R, MP_KC = 512;
constexpr int MP_XS = 1920;                               // padded input tile: (1024 + 512 - 1) * 5 / 4 rounded up
__device__ __forceinline__ int mp_pad(int i) { return i + (i >> 2); }

struct MpArgs {
    const double2 *x;       // [B][nt][n]
    const double2 *g;       // [B][nr][nt][L] or [nr][nt][L]
    double2 *y;             // [B][nr][lout]
    int64_t n, lout;
    int64_t tiles_per_row, ntiles;
    int64_t total;          // B nr lout (direct kernel)
    int nt, nr, L, g_batched;
};

template <int NRG>
__global__ __launch_bounds__(MP_BLOCK) void multipath_kernel(MpArgs a) {
    constexpr int R = MP_R;
    __shared__ double2 tl[CPX_MP_MAX_TAPS];
    __shared__ double2 xs[MP_XS];
    const int t = threadIdx.x;
    const int ntaps = a.nr * a.nt * a.L;
    bool staged = false;
    for (int64_t tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
        const int64_t b = tile / a.tiles_per_row;
        const int64_t q0 = (tile - b * a.tiles_per_row) * MP_TQ;
        if (a.g_batched || !staged) {                       // uniform; readable after the first barrier below
            const double2 *g = a.g + (a.g_batched ? b : 0) * ntaps;
            for (int i = t; i < ntaps; i += MP_BLOCK) tl[i] = g[i];
            staged = true;
        }
        for (int r0 = 0; r0 < a.nr; r0 += NRG) {
            double2 acc[NRG][R];
#pragma unroll
            for (int i = 0; i < NRG; i++)
#pragma unroll
                for (int r = 0; r < R; r++) acc[i][r] = make_double2(0.0, 0.0);
            for (int tx = 0; tx < a.nt; tx++) {
                const double2 *x = a.x + (b * a.nt + tx) * a.n;
                for (int jc = 0; jc < a.L; jc += MP_KC) {
                    const int JCn = a.L - jc < MP_KC ? a.L - jc : MP_KC;
                    const int JCpad = (JCn + R - 1) / R * R;
                    // LDS position w holds x[q0 - (jc + JCpad - 1) + w]
                    const int64_t s0 = q0 - (jc + JCpad - 1);
                    const int W = MP_TQ + JCpad - 1;
                    for (int w = t; w < W; w += MP_BLOCK) {
                        const int64_t s = s0 + w;
                        xs[mp_pad(w)] = (s >= 0 && s < a.n) ? x[s] : make_double2(0.0, 0.0);
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
                    for (int r = 0; r < R; r++) xr[(r + R - 1) % R] = xs[mp_pad(base + r + JCpad - 1)];
                    for (int ua = 0; ua < JCpad; ua += R) {
#pragma unroll
                        for (int bb = 0; bb < R; bb++) {
                            const int u = ua + bb;
                            if (u < JCn) {                  // no tap, no term
#pragma unroll
                                for (int i = 0; i < NRG; i++) {
                                    const double2 tap = tl[tap0 + toff[i] + u];                 // uniform: a broadcast read
#pragma unroll
                                    for (int r = 0; r < R; r++) mac(acc[i][r], tap, xr[(r + R - 1 - bb) % R]);
                                }
                            }
                            if (u + 1 < JCpad) xr[(2 * R - 2 - bb) % R] = xs[mp_pad(base + JCpad - 2 - u)];
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
                        if (m < a.lout) o[m] = acc[i][r];
                    }
                }
            }
        }
    }
}

__global__ __launch_bounds__(256) void multipath_direct(MpArgs a) {
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < a.total; idx += (int64_t)gridDim.x * blockDim.x) {
        const int64_t q = idx / a.lout, m = idx - q * a.lout;
        const int64_t b = q / a.nr;
        const int r = (int)(q - b * a.nr);
        const double2 *g = a.g + ((a.g_batched ? b : 0) * a.nr + r) * a.nt * a.L;
        const int klo = m - (a.n - 1) > 0 ? (int)(m - (a.n - 1)) : 0;
        const int khi = m < a.L - 1 ? (int)m : a.L - 1;
        double2 acc = make_double2(0.0, 0.0);
        for (int tx = 0; tx < a.nt; tx++) {
            const double2 *x = a.x + (b * a.nt + tx) * a.n;
            for (int k = klo; k <= khi; k++) mac(acc, g[tx * a.L + k], x[m - k]);
        }
        a.y[idx] = acc;
    }
}

int multipath_sizes(int g_batched, int64_t B, int nt, int nr, int64_t n, int L) {
    CPX_REQUIRE(B >= 0, CPX_EINVAL, "multipath: negative batch size");
    CPX_REQUIRE(nt >= 1 && nr >= 1 && L >= 1, CPX_EINVAL, "multipath: nt = %d, nr = %d, L = %d, need at least 1 of each", nt, nr, L);
    CPX_REQUIRE(g_batched == 0 || g_batched == 1, CPX_EINVAL, "multipath: g_batched = %d, need 0 or 1", g_batched);
    CPX_REQUIRE(B == 0 || n >= 1, CPX_EINVAL, "multipath: n = %lld (an empty row cannot be convolved)", (long long)n);
    CPX_REQUIRE(L <= CPX_MP_MAX_L, CPX_ELIMIT, "multipath: L = %d is above the engine's limit of %d", L, CPX_MP_MAX_L);
    CPX_REQUIRE((int64_t)nr * nt * L <= CPX_MP_MAX_TAPS, CPX_ELIMIT, "multipath: nr nt L = %lld taps per row are above the engine's limit of %d",
                (long long)nr * nt * L, CPX_MP_MAX_TAPS);
    CPX_REQUIRE(B == 0 || n <= (INT64_MAX / 64 - L) / B / (nt > nr ? nt : nr), CPX_EINVAL, "multipath: %lld x %lld samples overflow",
                (long long)B, (long long)n);
    return CPX_OK;
}

// ---- pilot plan: map, least squares, interpolation, demap ----------------------------------------------------------------------
constexpr int OC_BLOCK = 256, OC_TILE = 2048;              // LDS tile of the transpositions, complex values
// resource / data elements per tile for rows of `width` antennas: the row stride width | 1 is odd (conflict-free both ways)
int oc_rows(int width) { const int v = OC_TILE / (width | 1); return v > 256 ? 256 : v; }

struct OcArgs {
    const int32_t *code, *dcount, *data_re, *data_sc, *pil_tx, *ls_ptr, *ls_re;
    const double2 *pil_val, *ls_coef, *w;
    const int64_t *ant, *tv_ant;
    int64_t B, F, ndata, nls;       // F = nsym nsc
    int nsc, nt, nr, rows;          // rows: oc_rows of the kernel's width
    int ns_max;                     // ofdm_interp_kernel<true>
};

__global__ __launch_bounds__(OC_BLOCK) void ofdm_map_kernel(OcArgs a, const double2 *data, double2 *grid) {
    __shared__ double2 lds[OC_TILE];
    const int rs = a.nt | 1;
    const int64_t rtiles = (a.F + a.rows - 1) / a.rows, ntiles = a.B * rtiles;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t b = tile / rtiles;
        const int64_t re0 = (tile - b * rtiles) * a.rows;
        const int ren = a.F - re0 < a.rows ? (int)(a.F - re0) : a.rows;
        const int dlo = a.dcount[re0], dn = a.dcount[re0 + ren] - dlo;
        const double2 *src = data + (b * a.ndata + dlo) * a.nt;
        for (int w = threadIdx.x; w < dn * a.nt; w += OC_BLOCK) {
            const int dl = w / a.nt, t = w - dl * a.nt;
            lds[dl * rs + t] = src[w];
        }
        __syncthreads();
        for (int w = threadIdx.x; w < a.nt * ren; w += OC_BLOCK) {
            const int t = w / ren, rl = w - t * ren;
            const int c = a.code[re0 + rl];
            double2 v = make_double2(0.0, 0.0);
            if (c >= 0) v = lds[(c - dlo) * rs + t];
            else if (a.pil_tx[-1 - c] == t) v = a.pil_val[-1 - c];
            grid[(b * a.nt + t) * a.F + re0 + rl] = v;
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(OC_BLOCK) void ofdm_ls_kernel(OcArgs a, const double2 *Y, double2 *ls) {
    const int64_t total = a.B * a.nls * a.nr;
    for (int64_t idx = (int64_t)blockIdx.x * OC_BLOCK + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * OC_BLOCK) {
        const int64_t q = idx / a.nr, b = q / a.nls;
        const int r = (int)(idx - q * a.nr), i = (int)(q - b * a.nls);
        const double2 *y = Y + (b * a.nr + r) * a.F;
        const int s0 = a.ls_ptr[i], s1 = a.ls_ptr[i + 1];
        double2 acc = make_double2(0.0, 0.0);
        for (int s = s0; s < s1; s++) mac(acc, a.ls_coef[s], y[a.ls_re[s]]);
        const double cnt = (double)(s1 - s0);
        ls[idx] = make_double2(acc.x / cnt, acc.y / cnt);
    }
}

constexpr int IK_KT = 64, IK_CT = 32, IK_JC = 16, IK_CPT = IK_CT / (OC_BLOCK / 64);

// TV: the columns are (b, r, i) with i < ns_max a pilot symbol (skipped where antenna t has fewer), ls holds one item per (t, i, j) and
// the output is Hp [B][ns_max][nsc][nr][nt]; tile, staging and chain are the same
template <bool TV>
__global__ __launch_bounds__(OC_BLOCK) void ofdm_interp_kernel(OcArgs a, const double2 *ls, double2 *hsc) {
    __shared__ double2 wt[IK_JC][IK_KT + 1];               // W_t tile, transposed; the odd stride spreads the staging stores
    __shared__ double2 lt[IK_JC][IK_CT];
    const int64_t C = TV ? a.B * a.nr * a.ns_max : a.B * a.nr;   // columns (b, r) or (b, r, i)
    const int64_t ktiles = (a.nsc + IK_KT - 1) / IK_KT, ctiles = (C + IK_CT - 1) / IK_CT;
    const int64_t ntiles = ctiles * a.nt * ktiles;
    const int kl = threadIdx.x & 63, cg = threadIdx.x >> 6;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t ct = tile / (a.nt * ktiles), rem = tile - ct * (a.nt * ktiles);
        const int t = (int)(rem / ktiles);
        const int k0 = (int)(rem - t * ktiles) * IK_KT;
        const int64_t c0 = ct * IK_CT;
        const int np = (int)a.ant[3 * t];
        const int64_t item0 = TV ? a.tv_ant[3 * t + 1] : a.ant[3 * t + 1];
        const int ns = TV ? (int)a.tv_ant[3 * t] : 1;
        const double2 *w = a.w + a.ant[3 * t + 2];
        double2 acc[IK_CPT];
#pragma unroll
        for (int i = 0; i < IK_CPT; i++) acc[i] = make_double2(0.0, 0.0);
        for (int j0 = 0; j0 < np; j0 += IK_JC) {
            const int JCn = np - j0 < IK_JC ? np - j0 : IK_JC;
            for (int e = threadIdx.x; e < IK_KT * IK_JC; e += OC_BLOCK) {
                const int kk = e / IK_JC, jj = e - kk * IK_JC;
                if (jj < JCn) wt[jj][kk] = k0 + kk < a.nsc ? w[(int64_t)(k0 + kk) * np + j0 + jj] : make_double2(0.0, 0.0);
            }
            for (int e = threadIdx.x; e < IK_JC * IK_CT; e += OC_BLOCK) {
                const int jj = e / IK_CT, cc = e - jj * IK_CT;
                if (jj < JCn) {
                    const int64_t c = c0 + cc;
                    if constexpr (TV) {
                        const int64_t q = c / a.ns_max, b = q / a.nr;
                        const int i = (int)(c - q * a.ns_max);
                        lt[jj][cc] = c < C && i < ns ? ls[(b * a.nls + item0 + (int64_t)i * np + j0 + jj) * a.nr + (q - b * a.nr)]
                                                     : make_double2(0.0, 0.0);
                    } else {
                        const int64_t b = c / a.nr;
                        lt[jj][cc] = c < C ? ls[(b * a.nls + item0 + j0 + jj) * a.nr + (c - b * a.nr)] : make_double2(0.0, 0.0);
                    }
                }
            }
            __syncthreads();
            for (int jj = 0; jj < JCn; jj++) {
                const double2 wv = wt[jj][kl];
#pragma unroll
                for (int i = 0; i < IK_CPT; i++) mac(acc[i], wv, lt[jj][cg * IK_CPT + i]);
            }
            __syncthreads();
        }
        if (k0 + kl < a.nsc) {
#pragma unroll
            for (int i = 0; i < IK_CPT; i++) {
                const int64_t c = c0 + cg * IK_CPT + i;
                if constexpr (TV) {
                    const int64_t q = c / a.ns_max, b = q / a.nr;
                    const int ip = (int)(c - q * a.ns_max);
                    if (c < C && ip < ns) hsc[(((b * a.ns_max + ip) * a.nsc + k0 + kl) * a.nr + (q - b * a.nr)) * a.nt + t] = acc[i];
                } else if (c < C) {
                    const int64_t b = c / a.nr;
                    hsc[((b * a.nsc + k0 + kl) * a.nr + (c - b * a.nr)) * a.nt + t] = acc[i];
                }
            }
        }
    }
}

constexpr int HD_ROWS = 256;                                // data elements per workgroup

__global__ __launch_bounds__(OC_BLOCK) void ofdm_hdemap_kernel(OcArgs a, const double2 *hsc, double2 *hdata) {
    const int E = a.nr * a.nt;
    const int64_t dtiles = (a.ndata + HD_ROWS - 1) / HD_ROWS, ntiles = a.B * dtiles;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t b = tile / dtiles;
        const int64_t d0 = (tile - b * dtiles) * HD_ROWS;
        const int dn = a.ndata - d0 < HD_ROWS ? (int)(a.ndata - d0) : HD_ROWS;
        const double2 *src = hsc + b * a.nsc * E;
        double2 *dst = hdata + (b * a.ndata + d0) * E;
        for (int w = threadIdx.x; w < dn * E; w += OC_BLOCK) {
            const int dl = w / E, e = w - dl * E;
            dst[w] = src[(int64_t)a.data_sc[d0 + dl] * E + e];
        }
    }
}

__global__ __launch_bounds__(OC_BLOCK) void ofdm_ydemap_kernel(OcArgs a, const double2 *Y, double2 *ydata) {
    __shared__ double2 lds[OC_TILE];
    const int rs = a.nr | 1;
    const int64_t dtiles = (a.ndata + a.rows - 1) / a.rows, ntiles = a.B * dtiles;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t b = tile / dtiles;
        const int64_t d0 = (tile - b * dtiles) * a.rows;
        const int dn = a.ndata - d0 < a.rows ? (int)(a.ndata - d0) : a.rows;
        for (int w = threadIdx.x; w < a.nr * dn; w += OC_BLOCK) {
            const int r = w / dn, dl = w - r * dn;
            lds[dl * rs + r] = Y[(b * a.nr + r) * a.F + a.data_re[d0 + dl]];
        }
        __syncthreads();
        double2 *dst = ydata + (b * a.ndata + d0) * a.nr;
        for (int w = threadIdx.x; w < dn * a.nr; w += OC_BLOCK) {
            const int dl = w / a.nr, r = w - dl * a.nr;
            dst[w] = lds[dl * rs + r];
        }
        __syncthreads();
    }
}

constexpr int TV_NS = 4;          // pilot symbols of an element kept in registers
constexpr int TV_VMAX = 1024;     // entries of V staged in the LDS (16 KB)

struct TvArgs {
    const int32_t *code;
    const int64_t *tv_ant;
    const double2 *v, *hp;          // hp [B][ns_max][nsc][nr][nt]
    double2 *hsym, *hdata;          // either may be null
    int64_t B, ndata, FE, nv;       // FE = nsc nr nt, one symbol's plane
    int nsc, nsym, nt, E, ns_max;   // E = nr nt
};

// time interpolation fused with the demap: one element (k, r, t) per thread, its pilot symbols loaded once, all symbols written
template <bool VLDS>
__global__ __launch_bounds__(OC_BLOCK) void ofdm_tv_kernel(TvArgs a) {
    __shared__ double2 vs[VLDS ? TV_VMAX : 1];
    if constexpr (VLDS) {
        for (int i = threadIdx.x; i < (int)a.nv; i += OC_BLOCK) vs[i] = a.v[i];
        __syncthreads();
    }
    auto v_at = [&](int64_t i) -> double2 {
        if constexpr (VLDS) return vs[i];
        else return a.v[i];
    };
    const int32_t *__restrict__ code = a.code;
    const int64_t ftiles = (a.FE + OC_BLOCK - 1) / OC_BLOCK, ntiles = a.B * ftiles;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t b = tile / ftiles;
        const int64_t f = (tile - b * ftiles) * OC_BLOCK + threadIdx.x;
        if (f >= a.FE) continue;
        const int64_t k = f / a.E;
        const int e = (int)(f - k * a.E), t = e % a.nt;
        const int ns = (int)a.tv_ant[3 * t];
        const int64_t voff = a.tv_ant[3 * t + 2];
        const double2 *h = a.hp + b * a.ns_max * a.FE + f;  // pilot symbol i at h[i FE]
        double2 hr[TV_NS];
#pragma unroll
        for (int i = 0; i < TV_NS; i++) hr[i] = i < ns ? h[i * a.FE] : make_double2(0.0, 0.0);
        for (int s = 0; s < a.nsym; s++) {
            const int64_t vrow = voff + (int64_t)s * ns;
            double2 acc = make_double2(0.0, 0.0);
#pragma unroll
            for (int i = 0; i < TV_NS; i++)
                if (i < ns) mac(acc, v_at(vrow + i), hr[i]);
            for (int i = TV_NS; i < ns; i++) mac(acc, v_at(vrow + i), h[i * a.FE]);
            if (a.hsym) a.hsym[(b * a.nsym + s) * a.FE + f] = acc;
            if (a.hdata) {
                const int d = code[(int64_t)s * a.nsc + k];
                if (d >= 0) a.hdata[(b * a.ndata + d) * a.E + e] = acc;
            }
        }
    }
}

// the tables ofdm_ls_kernel walks: a frame's (an item = the pilots of one (antenna, subcarrier)) or time tracking's (one pilot per item)
struct LsTables { const int32_t *ptr, *re; const double2 *coef; int64_t n; };
LsTables frame_tables(const cpx_ofdm_pilots *p) { return {p->d_ls_ptr, p->d_ls_re, p->d_ls_coef, p->nls}; }
LsTables tv_tables(const cpx_ofdm_pilots *p) { return {p->d_tv_ptr, p->d_tv_re, p->d_tv_coef, p->nlsp}; }

OcArgs plan_args(const cpx_ofdm_pilots *p, int64_t B, const LsTables &ls) {
    OcArgs a{};
    a.code = p->d_code; a.dcount = p->d_dcount; a.data_re = p->d_data_re; a.data_sc = p->d_data_sc; a.pil_tx = p->d_pil_tx;
    a.ls_ptr = ls.ptr; a.ls_re = ls.re; a.pil_val = p->d_pil_val; a.ls_coef = ls.coef; a.w = p->d_w; a.ant = p->d_ant;
    a.B = B; a.F = (int64_t)p->nsym * p->nsc; a.ndata = p->ndata; a.nls = ls.n;
    a.nsc = p->nsc; a.nt = p->nt;
    a.tv_ant = p->d_tv_ant; a.ns_max = p->ns_max;
    return a;
}

int map_sizes(const cpx_ofdm_pilots *p, int64_t B) {
    CPX_REQUIRE(p, CPX_EINVAL, "ofdm_map: null plan");
    CPX_REQUIRE(B >= 0, CPX_EINVAL, "ofdm_map: negative batch size");
    CPX_REQUIRE(B == 0 || B <= INT64_MAX / 64 / ((int64_t)p->nsym * p->nsc * p->nt), CPX_EINVAL, "ofdm_map: %lld frames overflow", (long long)B);
    return CPX_OK;
}

// nsym nsc nt nr values per frame: the size of Y times nt, and of cpx_pilots_estimate_tv's h_sym, its largest array
int estimate_sizes(const cpx_ofdm_pilots *p, int64_t B, int nr, const void *h_sc, const void *y_data, const void *h_data,
                   const char *what = "ofdm_estimate") {
    CPX_REQUIRE(p, CPX_EINVAL, "%s: null plan", what);
    CPX_REQUIRE(B >= 0, CPX_EINVAL, "%s: negative batch size", what);
    CPX_REQUIRE(nr >= 1, CPX_EINVAL, "%s: nr = %d, need at least 1", what, nr);
    CPX_REQUIRE(nr <= CPX_OC_MAX_ANT, CPX_ELIMIT, "%s: nr = %d is above the engine's limit of %d", what, nr, CPX_OC_MAX_ANT);
    CPX_REQUIRE(h_sc || y_data || h_data, CPX_EINVAL, "%s: no output requested", what);
    CPX_REQUIRE(B == 0 || B <= INT64_MAX / 64 / ((int64_t)p->nsym * p->nsc * p->nt * nr), CPX_EINVAL, "%s: %lld frames overflow", what,
                (long long)B);
    return CPX_OK;
}

int estimate_tv_sizes(const cpx_ofdm_pilots *p, int64_t B, int nr, const void *h_sym, const void *y_data, const void *h_data) {
    if (int rc = estimate_sizes(p, B, nr, h_sym, y_data, h_data, "ofdm_estimate_tv")) return rc;
    CPX_REQUIRE(p->ns_max > 0, CPX_EINVAL, "ofdm_estimate_tv: the plan has no time matrices (it was made by cpx_pilots_create, not cpx_pilots_create_tv)");
    return CPX_OK;
}

// ---- the steps of an estimate call, shared by cpx_pilots_estimate_dev and cpx_pilots_estimate_tv_dev -------------------------------
struct Est {
    hipStream_t st;
    OcArgs a;
    const double2 *Y;
    char names[160] = "";           // the launches so far, joined with '+': cpx_last_kernel's text
    void launched(const char *kernel) {
        if (names[0]) strcat(names, "+");
        strcat(names, kernel);
    }
};

// after the size checks of a call with B > 0: the plan's device, the input, the stream and the kernels' arguments
int est_begin(Est &e, const cpx_ofdm_pilots *p, const char *what, const LsTables &ls, const double *d_Y_re_im, int64_t B, int nr,
              void *stream) {
    if (int rcd = check_handle_device(p->device, what)) return rcd;
    CPX_REQUIRE(d_Y_re_im, CPX_EINVAL, "%s: null pointer", what);
    e.st = pick_stream(stream);
    e.a = plan_args(p, B, ls);
    e.a.nr = nr;
    e.Y = reinterpret_cast<const double2 *>(d_Y_re_im);
    return CPX_OK;
}

// the interpolation in frequency of one estimator: its kernel, and the arena slots of the least-squares values and of its output
struct Interp {
    void (*kernel)(OcArgs, const double2 *, double2 *);
    const char *name;
    Slot ls, out;
};

// least squares on the tables of e.a, then k over B nr per columns into *out [B][per][nsc][nr][nt] (null: taken from k's slot)
int est_ls_interp(Est &e, Scratch &sc, const Interp &k, int per, double2 **out) {
    const OcArgs &a = e.a;
    double2 *ls = nullptr;
    if (int rc = sc.get(e.st, k.ls, 16 * (size_t)(a.B * a.nls * a.nr), &ls)) return rc;
    if (!*out)
        if (int rc = sc.get(e.st, k.out, 16 * (size_t)(a.B * per * a.nsc * a.nr * a.nt), out)) return rc;
    hipLaunchKernelGGL(ofdm_ls_kernel, dim3(grid_of((a.B * a.nls * a.nr + OC_BLOCK - 1) / OC_BLOCK)), dim3(OC_BLOCK), 0, e.st, a, e.Y,
                       ls);
    const int64_t itiles = ((a.B * a.nr * per + IK_CT - 1) / IK_CT) * a.nt * ((a.nsc + IK_KT - 1) / IK_KT);
    hipLaunchKernelGGL(k.kernel, dim3(grid_of(itiles)), dim3(OC_BLOCK), 0, e.st, a, ls, *out);
    e.launched("ofdm_ls_kernel");
    e.launched(k.name);
    return CPX_OK;
}

// y_data where it is asked for and the frame has data elements, then the call's end
int est_ydemap_end(Est &e, double *d_y_data) {
    if (d_y_data && e.a.ndata) {
        e.a.rows = oc_rows(e.a.nr);
        hipLaunchKernelGGL(ofdm_ydemap_kernel, dim3(grid_of(e.a.B * ((e.a.ndata + e.a.rows - 1) / e.a.rows))), dim3(OC_BLOCK), 0, e.st,
                           e.a, e.Y, reinterpret_cast<double2 *>(d_y_data));
        e.launched("ofdm_ydemap_kernel");
    }
    CPX_HIP(hipGetLastError());
    note_kernel("%s", e.names);
    return CPX_OK;
}

// a host-buffer estimator: dev = the device one, first = the first output (h_sc or h_sym) of first_bytes bytes
using EstimateDev = int (*)(const cpx_ofdm_pilots *, const double *, int64_t, int, double *, double *, double *, void *);
int estimate_host(EstimateDev dev, const char *what, const cpx_ofdm_pilots *p, const double *Y_re_im, int64_t B, int nr, double *first,
                  size_t first_bytes, double *y_data, double *h_data) {
    CPX_REQUIRE(Y_re_im, CPX_EINVAL, "%s: null pointer", what);
    int rc = ensure_device();
    if (rc) return rc;
    const size_t in_bytes = 16 * (size_t)(B * nr * p->nsym * p->nsc);
    const size_t y_bytes = y_data ? 16 * (size_t)(B * p->ndata * nr) : 0, hd_bytes = h_data ? 16 * (size_t)(B * p->ndata * nr * p->nt) : 0;
    if (!first) first_bytes = 0;
    HostStage s;
    const double *din;
    double *dfirst = nullptr, *dy = nullptr, *dhd = nullptr;
    if ((rc = s.in(Y_re_im, in_bytes, &din))) return rc;
    if (first && (rc = s.out(first_bytes, &dfirst))) return rc;
    if (y_data && (rc = s.out(y_bytes, &dy))) return rc;
    if (h_data && (rc = s.out(hd_bytes, &dhd))) return rc;
    if ((rc = dev(p, din, B, nr, dfirst, dy, dhd, s.st))) return rc;
    if ((rc = s.get(first, dfirst, first_bytes)) || (rc = s.get(y_data, dy, y_bytes))) return rc;
    return s.get(h_data, dhd, hd_bytes);
}

}  // namespace

extern "C" {

int cpx_multipath_dev(const double *d_x_re_im, const double *d_g_re_im, int g_batched, int64_t B, int nt, int nr, int64_t n, int L,
                      double *d_y_re_im, void *stream) {
    CPX_TRACE("cpx_multipath_dev");
    if (int rc = multipath_sizes(g_batched, B, nt, nr, n, L)) return rc;
    if (B == 0) return CPX_OK;
    CPX_REQUIRE(d_x_re_im && d_g_re_im && d_y_re_im, CPX_EINVAL, "multipath: null pointer");
    MpArgs a{};
    a.x = reinterpret_cast<const double2 *>(d_x_re_im);
    a.g = reinterpret_cast<const double2 *>(d_g_re_im);
    a.y = reinterpret_cast<double2 *>(d_y_re_im);
    a.n = n;
    a.lout = n + L - 1;
    a.total = B * nr * a.lout;
    a.nt = nt; a.nr = nr; a.L = L; a.g_batched = g_batched;
    hipStream_t st = pick_stream(stream);
    // the tiled kernel when a row's tiles are at least half full
    if (2 * a.lout >= MP_TQ) {
        a.tiles_per_row = (a.lout + MP_TQ - 1) / MP_TQ;
        a.ntiles = B * a.tiles_per_row;
        const dim3 grid(grid_of(a.ntiles)), block(MP_BLOCK);
        const int nrg = nr >= 3 ? 4 : nr;
        if (nrg == 4) hipLaunchKernelGGL(multipath_kernel<4>, grid, block, 0, st, a);
        else if (nrg == 2) hipLaunchKernelGGL(multipath_kernel<2>, grid, block, 0, st, a);
        else hipLaunchKernelGGL(multipath_kernel<1>, grid, block, 0, st, a);
        CPX_HIP(hipGetLastError());
        note_kernel("multipath_kernel<%d>", nrg);
        return CPX_OK;
    }
    hipLaunchKernelGGL(multipath_direct, dim3(grid_of((a.total + 255) / 256)), dim3(256), 0, st, a);
    CPX_HIP(hipGetLastError());
    note_kernel("multipath_direct");
    return CPX_OK;
}

int cpx_multipath(const double *x_re_im, const double *g_re_im, int g_batched, int64_t B, int nt, int nr, int64_t n, int L,
                  double *y_re_im) {
    CPX_TRACE("cpx_multipath");
    if (int rc = multipath_sizes(g_batched, B, nt, nr, n, L)) return rc;
    if (B == 0) return CPX_OK;
    CPX_REQUIRE(x_re_im && g_re_im && y_re_im, CPX_EINVAL, "multipath: null pointer");
    int rc = ensure_device();
    if (rc) return rc;
    const size_t x_bytes = 16 * (size_t)(B * nt * n), g_bytes = 16 * (size_t)((g_batched ? B : 1) * nr * nt * L),
                 y_bytes = 16 * (size_t)(B * nr * (n + L - 1));
    HostStage s;
    const double *dx, *dg;
    double *dy;
    if ((rc = s.in(x_re_im, x_bytes, &dx)) || (rc = s.in(g_re_im, g_bytes, &dg)) || (rc = s.out(y_bytes, &dy)) ||
        (rc = cpx_multipath_dev(dx, dg, g_batched, B, nt, nr, n, L, dy, s.st)))
        return rc;
    return s.get(y_re_im, dy, y_bytes);
}

// both forms of the plan: tv = with the time matrices v_re_im
static int pilots_create(int nsc, int nsym, int nt, int64_t npil, const int32_t *pil_sym, const int32_t *pil_sc, const int32_t *pil_tx,
                         const double *pil_val_re_im, const double *w_re_im, bool tv, const double *v_re_im, cpx_ofdm_pilots **out) {
    CPX_REQUIRE(out, CPX_EINVAL, "ofdm_pilots: null pointer");
    *out = nullptr;
    CPX_REQUIRE(nsc >= 2 && nsc % 2 == 0, CPX_EINVAL, "ofdm_pilots: nsc = %d, need an even number >= 2", nsc);
    CPX_REQUIRE(nsym >= 1 && nt >= 1 && npil >= 1, CPX_EINVAL, "ofdm_pilots: nsym = %d, nt = %d, npil = %lld, need at least 1 of each", nsym, nt,
                (long long)npil);
    CPX_REQUIRE(pil_sym && pil_sc && pil_tx && pil_val_re_im && w_re_im, CPX_EINVAL, "ofdm_pilots: null pointer");
    CPX_REQUIRE(!tv || v_re_im, CPX_EINVAL, "ofdm_pilots: null time matrices (v_re_im)");
    CPX_REQUIRE(nt <= CPX_OC_MAX_ANT, CPX_ELIMIT, "ofdm_pilots: nt = %d is above the engine's limit of %d", nt, CPX_OC_MAX_ANT);
    const int64_t F = (int64_t)nsym * nsc;
    CPX_REQUIRE(F <= INT32_MAX / 2, CPX_ELIMIT, "ofdm_pilots: a frame of %lld resource elements is above the engine's limit", (long long)F);
    CPX_REQUIRE(npil <= F, CPX_EINVAL, "ofdm_pilots: %lld pilots on %lld resource elements (one appears twice)", (long long)npil, (long long)F);
    std::vector<int32_t> code(F, 0);
    std::vector<char> used(F, 0);
    struct Pil { int32_t tx, sc, sym, i; };
    std::vector<Pil> pil(npil);
    std::vector<int64_t> per_ant(nt, 0);
    for (int64_t i = 0; i < npil; i++) {
        const int32_t s = pil_sym[i], k = pil_sc[i], t = pil_tx[i];
        CPX_REQUIRE(s >= 0 && s < nsym && k >= 0 && k < nsc && t >= 0 && t < nt, CPX_EINVAL,
                    "ofdm_pilots: pilot %lld at (symbol %d, subcarrier %d, antenna %d) is out of range", (long long)i, s, k, t);
        const int64_t re = (int64_t)s * nsc + k;
        CPX_REQUIRE(!used[re], CPX_EINVAL, "ofdm_pilots: resource element (symbol %d, subcarrier %d) appears twice", s, k);
        const double vr = pil_val_re_im[2 * i], vi = pil_val_re_im[2 * i + 1];
        CPX_REQUIRE(std::isfinite(vr) && std::isfinite(vi) && (vr != 0.0 || vi != 0.0) && std::isfinite(vr * vr + vi * vi) &&
                        vr * vr + vi * vi > 0.0,
                    CPX_EINVAL, "ofdm_pilots: pilot %lld has a value that is zero or not finite", (long long)i);
        used[re] = 1;
        code[re] = (int32_t)(-1 - i);
        pil[i] = Pil{t, k, s, (int32_t)i};
        per_ant[t]++;
    }
    for (int t = 0; t < nt; t++) CPX_REQUIRE(per_ant[t] > 0, CPX_EINVAL, "ofdm_pilots: antenna %d has no pilot", t);
    std::sort(pil.begin(), pil.end(), [](const Pil &a, const Pil &b) {
        return a.tx != b.tx ? a.tx < b.tx : a.sc != b.sc ? a.sc < b.sc : a.sym < b.sym;
    });
    std::vector<int32_t> ls_ptr, ls_re(npil);
    std::vector<double> ls_coef(2 * (size_t)npil);
    std::vector<int64_t> ant(3 * (size_t)nt, 0);
    int64_t w_total = 0;
    for (int64_t s = 0; s < npil; s++) {
        const Pil &q = pil[s];
        if (s == 0 || q.tx != pil[s - 1].tx || q.sc != pil[s - 1].sc) {
            if (s == 0 || q.tx != pil[s - 1].tx) ant[3 * q.tx + 1] = (int64_t)ls_ptr.size();
            ls_ptr.push_back((int32_t)s);
            ant[3 * q.tx]++;
        }
        ls_re[s] = q.sym * nsc + q.sc;
        const double vr = pil_val_re_im[2 * q.i], vi = pil_val_re_im[2 * q.i + 1], m2 = vr * vr + vi * vi;
        ls_coef[2 * s] = vr / m2;
        ls_coef[2 * s + 1] = -vi / m2;
    }
    const int64_t nls = (int64_t)ls_ptr.size();
    ls_ptr.push_back((int32_t)npil);
    for (int t = 0; t < nt; t++) {
        ant[3 * t + 2] = w_total;
        w_total += (int64_t)nsc * ant[3 * t];
    }
    for (int64_t i = 0; i < 2 * w_total; i++)
        CPX_REQUIRE(std::isfinite(w_re_im[i]), CPX_EINVAL, "ofdm_pilots: the interpolation matrices hold a value that is not finite");
    // time tracking: per antenna the rectangle (pilot symbols) x (pilot subcarriers), one least-squares item per pilot in (t, i, j) order
    std::vector<int32_t> tv_ptr, tv_re;
    std::vector<double> tv_coef;
    std::vector<int64_t> tv_ant(3 * (size_t)nt, 0);
    int64_t nv = 0;
    int ns_max = 0;
    if (tv) {
        tv_re.reserve(npil);
        tv_coef.reserve(2 * (size_t)npil);
        std::vector<int32_t> syms, on_sym(nsym);
        for (int t = 0; t < nt; t++) {
            const int64_t i0 = ls_ptr[ant[3 * t + 1]], i1 = ls_ptr[ant[3 * t + 1] + ant[3 * t]];   // antenna t's sorted pilots
            std::fill(on_sym.begin(), on_sym.end(), 0);
            for (int64_t s = i0; s < i1; s++) on_sym[pil[s].sym]++;
            syms.clear();
            for (int s = 0; s < nsym; s++) {
                if (!on_sym[s]) continue;
                CPX_REQUIRE(on_sym[s] == ant[3 * t], CPX_EINVAL,
                            "ofdm_pilots: antenna %d has pilots on %d of its %lld pilot subcarriers in symbol %d (time tracking needs the "
                            "same subcarriers on every pilot symbol)", t, on_sym[s], (long long)ant[3 * t], s);
                syms.push_back(s);
            }
            const int ns = (int)syms.size();
            tv_ant[3 * t] = ns;
            tv_ant[3 * t + 1] = (int64_t)tv_re.size();
            tv_ant[3 * t + 2] = nv;
            nv += (int64_t)nsym * ns;
            CPX_REQUIRE(nv <= INT32_MAX / 2, CPX_ELIMIT, "ofdm_pilots: time matrices of %lld values are above the engine's limit", (long long)nv);
            ns_max = ns > ns_max ? ns : ns_max;
            for (int i = 0; i < ns; i++) {
                for (int64_t j = 0; j < ant[3 * t]; j++) {
                    // the pilots of subcarrier k_j are sorted by symbol, and every pilot symbol is among them: the i-th is s_i's
                    const int64_t s = ls_ptr[ant[3 * t + 1] + j] + i;
                    tv_re.push_back(ls_re[s]);
                    tv_coef.push_back(ls_coef[2 * s]);
                    tv_coef.push_back(ls_coef[2 * s + 1]);
                }
            }
        }
        for (int64_t i = 0; i < 2 * nv; i++)
            CPX_REQUIRE(std::isfinite(v_re_im[i]), CPX_EINVAL, "ofdm_pilots: the time matrices hold a value that is not finite");
        tv_ptr.resize(tv_re.size() + 1);
        for (size_t i = 0; i < tv_ptr.size(); i++) tv_ptr[i] = (int32_t)i;
    }
    std::vector<int32_t> dcount(F + 1), data_re, data_sc, ptx(npil);
    data_re.reserve(F - npil);
    data_sc.reserve(F - npil);
    for (int64_t re = 0; re < F; re++) {
        dcount[re] = (int32_t)data_re.size();
        if (!used[re]) {
            code[re] = (int32_t)data_re.size();
            data_re.push_back((int32_t)re);
            data_sc.push_back((int32_t)(re % nsc));
        }
    }
    dcount[F] = (int32_t)data_re.size();
    for (int64_t i = 0; i < npil; i++) ptx[i] = pil_tx[i];
    int rc = ensure_device();
    if (rc) return rc;
    cpx_ofdm_pilots *p = new cpx_ofdm_pilots();
    p->nsc = nsc; p->nsym = nsym; p->nt = nt;
    p->npil = npil; p->ndata = (int64_t)data_re.size(); p->nls = nls;
    (void)hipGetDevice(&p->device);
    const char *what = "ofdm_pilots";
    if ((rc = upload((void **)&p->d_code, code.data(), 4 * code.size(), what)) ||
        (rc = upload((void **)&p->d_dcount, dcount.data(), 4 * dcount.size(), what)) ||
        (p->ndata && ((rc = upload((void **)&p->d_data_re, data_re.data(), 4 * data_re.size(), what)) ||
                      (rc = upload((void **)&p->d_data_sc, data_sc.data(), 4 * data_sc.size(), what)))) ||
        (rc = upload((void **)&p->d_pil_tx, ptx.data(), 4 * ptx.size(), what)) ||
        (rc = upload((void **)&p->d_pil_val, pil_val_re_im, 16 * (size_t)npil, what)) ||
        (rc = upload((void **)&p->d_ls_ptr, ls_ptr.data(), 4 * ls_ptr.size(), what)) ||
        (rc = upload((void **)&p->d_ls_re, ls_re.data(), 4 * ls_re.size(), what)) ||
        (rc = upload((void **)&p->d_ls_coef, ls_coef.data(), 8 * ls_coef.size(), what)) ||
        (rc = upload((void **)&p->d_ant, ant.data(), 8 * ant.size(), what)) ||
        (rc = upload((void **)&p->d_w, w_re_im, 16 * (size_t)w_total, what)) ||
        (tv && ((rc = upload((void **)&p->d_tv_ptr, tv_ptr.data(), 4 * tv_ptr.size(), what)) ||
                (rc = upload((void **)&p->d_tv_re, tv_re.data(), 4 * tv_re.size(), what)) ||
                (rc = upload((void **)&p->d_tv_coef, tv_coef.data(), 8 * tv_coef.size(), what)) ||
                (rc = upload((void **)&p->d_tv_ant, tv_ant.data(), 8 * tv_ant.size(), what)) ||
                (rc = upload((void **)&p->d_v, v_re_im, 16 * (size_t)nv, what))))) {
        cpx_pilots_destroy(p);
        return rc;
    }
    if (tv) {
        p->ns_max = ns_max;
        p->nlsp = (int64_t)tv_re.size();
        p->nv = nv;
    }
    *out = p;
    return CPX_OK;
}

int cpx_pilots_create(int nsc, int nsym, int nt, int64_t npil, const int32_t *pil_sym, const int32_t *pil_sc, const int32_t *pil_tx,
                           const double *pil_val_re_im, const double *w_re_im, cpx_ofdm_pilots **out) {
    CPX_TRACE("cpx_pilots_create");
    return pilots_create(nsc, nsym, nt, npil, pil_sym, pil_sc, pil_tx, pil_val_re_im, w_re_im, false, nullptr, out);
}

int cpx_pilots_create_tv(int nsc, int nsym, int nt, int64_t npil, const int32_t *pil_sym, const int32_t *pil_sc, const int32_t *pil_tx,
                         const double *pil_val_re_im, const double *w_re_im, const double *v_re_im, cpx_ofdm_pilots **out) {
    CPX_TRACE("cpx_pilots_create_tv");
    return pilots_create(nsc, nsym, nt, npil, pil_sym, pil_sc, pil_tx, pil_val_re_im, w_re_im, true, v_re_im, out);
}

int cpx_pilots_destroy(cpx_ofdm_pilots *p) {
    if (!p) return CPX_OK;
    for (void *d : {(void *)p->d_code, (void *)p->d_dcount, (void *)p->d_data_re, (void *)p->d_data_sc, (void *)p->d_pil_tx,
                    (void *)p->d_pil_val, (void *)p->d_ls_ptr, (void *)p->d_ls_re, (void *)p->d_ls_coef, (void *)p->d_ant, (void *)p->d_w,
                    (void *)p->d_tv_ptr, (void *)p->d_tv_re, (void *)p->d_tv_coef, (void *)p->d_tv_ant, (void *)p->d_v})
        (void)hipFree(d);
    delete p;
    return CPX_OK;
}

int cpx_pilots_map_dev(const cpx_ofdm_pilots *p, const double *d_data_re_im, int64_t B, double *d_grid_re_im, void *stream) {
    CPX_TRACE("cpx_pilots_map_dev");
    if (int rc = map_sizes(p, B)) return rc;
    if (B == 0) return CPX_OK;
    if (int rcd = check_handle_device(p->device, "ofdm_map")) return rcd;
    CPX_REQUIRE((d_data_re_im || p->ndata == 0) && d_grid_re_im, CPX_EINVAL, "ofdm_map: null pointer");
    OcArgs a = plan_args(p, B, frame_tables(p));
    a.rows = oc_rows(p->nt);
    const int64_t ntiles = B * ((a.F + a.rows - 1) / a.rows);
    hipLaunchKernelGGL(ofdm_map_kernel, dim3(grid_of(ntiles)), dim3(OC_BLOCK), 0, pick_stream(stream), a,
                       reinterpret_cast<const double2 *>(d_data_re_im), reinterpret_cast<double2 *>(d_grid_re_im));
    CPX_HIP(hipGetLastError());
    note_kernel("ofdm_map_kernel");
    return CPX_OK;
}

int cpx_pilots_map(const cpx_ofdm_pilots *p, const double *data_re_im, int64_t B, double *grid_re_im) {
    CPX_TRACE("cpx_pilots_map");
    if (int rc = map_sizes(p, B)) return rc;
    if (B == 0) return CPX_OK;
    CPX_REQUIRE((data_re_im || p->ndata == 0) && grid_re_im, CPX_EINVAL, "ofdm_map: null pointer");
    int rc = ensure_device();
    if (rc) return rc;
    const size_t in_bytes = 16 * (size_t)(B * p->ndata * p->nt), out_bytes = 16 * (size_t)(B * p->nt * p->nsym * p->nsc);
    HostStage s;
    const double *din;
    double *dout;
    if ((rc = s.in(data_re_im, in_bytes, &din)) || (rc = s.out(out_bytes, &dout)) || (rc = cpx_pilots_map_dev(p, din, B, dout, s.st))) return rc;
    return s.get(grid_re_im, dout, out_bytes);
}

int cpx_pilots_estimate_dev(const cpx_ofdm_pilots *p, const double *d_Y_re_im, int64_t B, int nr, double *d_h_sc, double *d_y_data,
                          double *d_h_data, void *stream) {
    CPX_TRACE("cpx_pilots_estimate_dev");
    if (int rc = estimate_sizes(p, B, nr, d_h_sc, d_y_data, d_h_data)) return rc;
    if (B == 0) return CPX_OK;
    Est e;
    if (int rc = est_begin(e, p, "ofdm_estimate", frame_tables(p), d_Y_re_im, B, nr, stream)) return rc;
    Scratch sc;
    if (d_h_sc || (d_h_data && p->ndata)) {
        double2 *hsc = reinterpret_cast<double2 *>(d_h_sc);
        const Interp k = {ofdm_interp_kernel<false>, "ofdm_interp_kernel", Slot::ofdm_ls, Slot::ofdm_hsc};
        if (int rc = est_ls_interp(e, sc, k, 1, &hsc)) return rc;
        if (d_h_data && p->ndata) {
            hipLaunchKernelGGL(ofdm_hdemap_kernel, dim3(grid_of(B * ((p->ndata + HD_ROWS - 1) / HD_ROWS))), dim3(OC_BLOCK), 0, e.st, e.a,
                               hsc, reinterpret_cast<double2 *>(d_h_data));
            e.launched("ofdm_hdemap_kernel");
        }
    }
    return est_ydemap_end(e, d_y_data);
}

int cpx_pilots_estimate(const cpx_ofdm_pilots *p, const double *Y_re_im, int64_t B, int nr, double *h_sc, double *y_data, double *h_data) {
    CPX_TRACE("cpx_pilots_estimate");
    if (int rc = estimate_sizes(p, B, nr, h_sc, y_data, h_data)) return rc;
    if (B == 0) return CPX_OK;
    return estimate_host(cpx_pilots_estimate_dev, "ofdm_estimate", p, Y_re_im, B, nr, h_sc, 16 * (size_t)(B * p->nsc * nr * p->nt), y_data,
                         h_data);
}

int cpx_pilots_estimate_tv_dev(const cpx_ofdm_pilots *p, const double *d_Y_re_im, int64_t B, int nr, double *d_h_sym, double *d_y_data,
                               double *d_h_data, void *stream) {
    CPX_TRACE("cpx_pilots_estimate_tv_dev");
    if (int rc = estimate_tv_sizes(p, B, nr, d_h_sym, d_y_data, d_h_data)) return rc;
    if (B == 0) return CPX_OK;
    Est e;
    if (int rc = est_begin(e, p, "ofdm_estimate_tv", tv_tables(p), d_Y_re_im, B, nr, stream)) return rc;
    Scratch sc;
    if (d_h_sym || (d_h_data && p->ndata)) {
        double2 *hp = nullptr;
        const Interp k = {ofdm_interp_kernel<true>, "ofdm_interp_kernel<tv>", Slot::ofdm_lsp, Slot::ofdm_hp};
        if (int rc = est_ls_interp(e, sc, k, p->ns_max, &hp)) return rc;
        TvArgs v{};
        v.code = p->d_code; v.tv_ant = p->d_tv_ant; v.v = p->d_v; v.hp = hp;
        v.hsym = reinterpret_cast<double2 *>(d_h_sym);
        v.hdata = p->ndata ? reinterpret_cast<double2 *>(d_h_data) : nullptr;
        v.B = B; v.ndata = p->ndata; v.FE = (int64_t)p->nsc * nr * p->nt; v.nv = p->nv;
        v.nsc = p->nsc; v.nsym = p->nsym; v.nt = p->nt; v.E = nr * p->nt; v.ns_max = p->ns_max;
        const dim3 grid(grid_of(B * ((v.FE + OC_BLOCK - 1) / OC_BLOCK)));
        if (p->nv <= TV_VMAX) hipLaunchKernelGGL(ofdm_tv_kernel<true>, grid, dim3(OC_BLOCK), 0, e.st, v);
        else hipLaunchKernelGGL(ofdm_tv_kernel<false>, grid, dim3(OC_BLOCK), 0, e.st, v);
        e.launched(p->nv <= TV_VMAX ? "ofdm_tv_kernel<lds>" : "ofdm_tv_kernel<global>");
    }
    return est_ydemap_end(e, d_y_data);
}

int cpx_pilots_estimate_tv(const cpx_ofdm_pilots *p, const double *Y_re_im, int64_t B, int nr, double *h_sym, double *y_data,
                           double *h_data) {
    CPX_TRACE("cpx_pilots_estimate_tv");
    if (int rc = estimate_tv_sizes(p, B, nr, h_sym, y_data, h_data)) return rc;
    if (B == 0) return CPX_OK;
    return estimate_host(cpx_pilots_estimate_tv_dev, "ofdm_estimate_tv", p, Y_re_im, B, nr, h_sym,
                         16 * (size_t)(B * nr * p->nsym * p->nsc) * p->nt, y_data, h_data);
}

}  // extern "C"
