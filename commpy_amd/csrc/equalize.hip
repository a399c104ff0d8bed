// Finite-length MMSE equalisation of a known multipath channel: the linear equaliser (nb = 0) and the decision-feedback equaliser
// (nb >= 1 feedback taps), hard and soft output, for L, nf <= 64 taps, nb <= 64 and any constellation of 2 .. 256 points.
//
// y_t = sum_l h_l x_{t-l} + w_t, x_t = c[a_t] for 0 <= t < n and 0 elsewhere; Es the mean symbol energy, N0 = noise_var, d the delay.
// The rule (float64, real and imaginary parts separate doubles, every product rounded before it is added, every sum from 0.0 in
// ascending index order, -ffp-contract=off; a b = (ar br - ai bi, ar bi + ai br), a conj(b) = (ar br + ai bi, ai br - ar bi)):
//   design      H[i][k] = h_{k-i} for 0 <= k-i < L (i < nf); K = all columns but d+1 .. d+nb.  For j <= i:
//               S[i][j] = sum over k in K, i <= k < j+L, of h_{k-i} conj(h_{k-j}); R[i][j] = Es S[i][j], and + N0 on the diagonal, whose
//               imaginary part is never computed.  p_i = Es h_{d-i} (0 outside the taps).
//   L D L^H     column j: g_k = (D_k Lr[j][k], -(D_k Li[j][k])) for k < j; v_i = R[i][j] - sum_{k<j} L[i][k] g_k for i >= j;
//               D_j = Re v_j; L[i][j] = (vr / D_j, vi / D_j) for i > j.
//   solve       a_i = p_i - sum_{k<i} L[i][k] a_k; b_i = (ar / D_i, ai / D_i); u_i = b_i - sum_{k>i} u_k conj(L[k][i]), i descending,
//               every sum over k ascending.
//   taps        ff_i = conj(u_i); fb_j = sum_i ff_i h_{d+j-i} over the i with 0 <= d+j-i < L, j = 1 .. nb;
//               gain = sum_i (ffr hr - ffi hi) of h_{d-i} over the i with 0 <= d-i < L; nu = (Es (1 - gain)) / gain.
//   equalise    z_t = sum_{i<nf} ff_i y_{t+d-i} - sum_{j=1..nb, t-j>=0} fb_j c[a^_{t-j}], a sample outside the row read as 0.0 and
//               multiplied like any other; x^_t = (zr / gain, zi / gain); a^_t = the first minimum over a ascending of
//               e = x^_t - c[a], er er + ei ei, a later point winning only if strictly smaller.
//   soft        llr[t m + i] = (min over the a with bit i = 1 - min over the a with bit i = 0 of that distance) / nu, bits MSB first,
//               each minimum from +inf over a ascending, replaced only by a strictly smaller value.
//   rejection   a row whose y, h or noise_var holds a NaN or +-inf (or a noise_var <= 0), one of whose pivots D_j is not positive and
//               finite, or whose gain is not a finite number in (0, 1): zero indices and bits, NaN everything else.
//
// eq_design_kernel: one wave per row, lane i owns row i of the matrix.  The strict lower triangle of L is kept column by column in
//   LDS (nf (nf-1) / 2 complex), R is never stored: lane i forms R[i][j] from the taps when column j is due.  Every lane runs its
//   own sums serially in k, so the rule's order needs no cross-lane reduction; g_k is computed by lane k and read as a broadcast.
//   Forward substitution hands a_k on by a lane read; the backward sum of u_i starts at k = i+1, the last u to become known, so it
//   is a serial chain: the lanes k > i form their products at once, the chain of additions is walked by every lane over LDS.  With
//   shared taps, a scalar noise_var and no design output requested the design runs once (eq_scan_kernel then flags the rows whose y
//   is not finite); else per row, the scan included.
// eq_filter_kernel<LGM>: a workgroup of 256 lanes takes EQ_TILE = 256 steps of one row: taps, the window of y (zero outside the row)
//   and the points in LDS, lane = step.  nb = 0: the slicer follows at once.  nb > 0: the sums go to the arena, [row][t].
// eq_dfe_kernel<LGM>: the feedback recursion, a serial chain per row: one row per lane, 64 rows per wave; the row's feedback taps and
//   its last 64 decisions (one byte each) in LDS, lane-private columns, so the chain needs no barrier.
//   LGM = 0: hard output only; LGM = m: the per-bit minima as well.  The arena block of sums is as large as y.  All grids are
//   grid-stride loops under a cap, so a result depends on neither the batch nor the grid.
#include "cpx_internal.h"
#include "cpx_slice.h"
#include "cpx_wave.h"

using namespace cpx;

#define CPX_EQ_MAX_TAPS 64                 // L, nf and nb
#define CPX_EQ_MAX_M 256
#define CPX_EQ_MAX_N (1 << 30)
#define EQ_TILE 256

namespace {

struct EqDesign {
    const double *h;                       // [L][2] or [rows][L][2]
    const double *nv;                      // [1] or [rows]
    const double *y;                       // [rows][n_y][2] scanned for NaN / inf, or null
    int64_t rows, n_y;
    int L, nf, nb, d, h_batched, nv_batched;
    double es;
    double *ff, *fb, *gain, *nu;           // [rows][nf][2], [rows][nb][2], [rows], [rows]
    uint8_t *flag;                         // [rows]: 1 = rejected
};

struct EqRun {
    const double *y, *cst, *ff, *fb, *gain, *nu;
    const uint8_t *flag;                   // [B]
    int64_t rows;
    int64_t dstride;                       // 0: one design for every row, 1: per row
    int n, n_y, nf, nb, d, M, m;           // m = 0: M is no power of two
    int32_t *indices;
    uint8_t *bits;
    double *est, *llr;
    double *zbuf;                          // nb > 0: [rows][n][2], the feed-forward sums, and nothing else is written by the filter
};

// L[i][k], i > k, of the packed strict lower triangle: column k starts behind the nf-1 + .. + nf-k entries of the columns before it
#define EQ_L(i, k) ((k) * (2 * nf - (k) - 1) / 2 + ((i) - (k) - 1))

__global__ __launch_bounds__(64) void eq_design_kernel(EqDesign a) {
    extern __shared__ double eq_lmat[];                        // Lr, Li: the strict lower triangle, column by column (EQ_L)
    __shared__ double hr[64], hi[64], gr[64], gi[64], Dl[64], qr[64], qi[64];
    const int lane = threadIdx.x, nf = a.nf, L = a.L, d = a.d, nb = a.nb;
    double *Lr = eq_lmat, *Li = eq_lmat + nf * (nf - 1) / 2;
    const double es = a.es;
    for (int64_t row = blockIdx.x; row < a.rows; row += gridDim.x) {
        const double *hrow = a.h + (a.h_batched ? row * 2 * L : 0);
        __syncthreads();                                       // the previous row's tables have been read
        bool bad = false;
        if (lane < L) {
            const double r = hrow[2 * lane], i = hrow[2 * lane + 1];
            hr[lane] = r;
            hi[lane] = i;
            bad = not_finite(r) || not_finite(i);
        }
        const double n0 = a.nv[a.nv_batched ? row : 0];
        bad |= not_finite(n0) || !(n0 > 0.0);
        bad = __ballot(bad) != 0ull;
        if (a.y) bad |= scan_row(a.y + row * 2 * a.n_y, 2 * a.n_y, lane);
        __syncthreads();

        // ---- L D L^H, column by column
        for (int j = 0; j < nf; j++) {
            if (lane < j) {
                const double D = Dl[lane];
                gr[lane] = D * Lr[EQ_L(j, lane)];
                gi[lane] = -(D * Li[EQ_L(j, lane)]);
            }
            __syncthreads();
            double vr = 0.0, vi = 0.0;
            if (lane >= j && lane < nf) {
                double sr = 0.0, si = 0.0;
                for (int k = lane; k < j + L; k++) {
                    if (k >= d + 1 && k <= d + nb) continue;
                    const double ar = hr[k - lane], ai = hi[k - lane], br = hr[k - j], bi = hi[k - j];
                    sr = sr + (ar * br + ai * bi);
                    si = si + (ai * br - ar * bi);
                }
                double tr = 0.0, ti = 0.0;
                for (int k = 0; k < j; k++) {
                    const double lr = Lr[EQ_L(lane, k)], li = Li[EQ_L(lane, k)], xr = gr[k], xi = gi[k];
                    tr = tr + (lr * xr - li * xi);
                    ti = ti + (lr * xi + li * xr);
                }
                if (lane == j) {
                    vr = (es * sr + n0) - tr;
                    Dl[j] = vr;
                } else {
                    vr = es * sr - tr;
                    vi = es * si - ti;
                }
            }
            __syncthreads();
            const double Dj = Dl[j];
            bad |= !(Dj > 0.0) || not_finite(Dj);
            if (lane > j && lane < nf) {
                Lr[EQ_L(lane, j)] = vr / Dj;
                Li[EQ_L(lane, j)] = vi / Dj;
            }
            __syncthreads();
        }

        // ---- forward substitution: lane k's a_k is final at step k
        double pr = 0.0, pi = 0.0;
        if (lane < nf && d - lane >= 0 && d - lane < L) {
            pr = es * hr[d - lane];
            pi = es * hi[d - lane];
        }
        double sr = 0.0, si = 0.0;
        for (int k = 0; k < nf; k++) {
            const double akr = __shfl(pr - sr, k), aki = __shfl(pi - si, k);
            if (lane > k && lane < nf) {
                const double lr = Lr[EQ_L(lane, k)], li = Li[EQ_L(lane, k)];
                sr = sr + (lr * akr - li * aki);
                si = si + (lr * aki + li * akr);
            }
        }
        const double Di = lane < nf ? Dl[lane] : 1.0;
        const double br = (pr - sr) / Di, bi = (pi - si) / Di;

        // ---- backward substitution: the sum of u_i runs over k = i+1 .. nf-1 ascending
        double ur = 0.0, ui = 0.0;
        for (int i = nf - 1; i >= 0; i--) {
            if (lane > i && lane < nf) {
                const double lr = Lr[EQ_L(lane, i)], li = Li[EQ_L(lane, i)];
                qr[lane] = ur * lr + ui * li;
                qi[lane] = ui * lr - ur * li;
            }
            __syncthreads();
            double tr = 0.0, ti = 0.0;
            for (int k = i + 1; k < nf; k++) {
                tr = tr + qr[k];
                ti = ti + qi[k];
            }
            if (lane == i) {
                ur = br - tr;
                ui = bi - ti;
            }
            __syncthreads();
        }

        // ---- the taps
        const double fr = ur, fi = -ui;
        if (lane < nf) {
            gr[lane] = fr;
            gi[lane] = fi;
        }
        __syncthreads();
        double gain = 0.0;
        {
            const int lo = d - L + 1 > 0 ? d - L + 1 : 0, hi_ = d < nf - 1 ? d : nf - 1;
            for (int i = lo; i <= hi_; i++) gain = gain + (gr[i] * hr[d - i] - gi[i] * hi[d - i]);
        }
        const double nu = (es * (1.0 - gain)) / gain;
        bad |= not_finite(gain) || !(gain > 0.0) || !(gain < 1.0);
        const double nan = __builtin_nan("");
        if (lane < nb) {
            const int j = lane + 1;
            const int lo = d + j - L + 1 > 0 ? d + j - L + 1 : 0, hi_ = d + j < nf - 1 ? d + j : nf - 1;
            double tr = 0.0, ti = 0.0;
            for (int i = lo; i <= hi_; i++) {
                const double xr = hr[d + j - i], xi = hi[d + j - i];
                tr = tr + (gr[i] * xr - gi[i] * xi);
                ti = ti + (gr[i] * xi + gi[i] * xr);
            }
            a.fb[(row * nb + lane) * 2] = bad ? nan : tr;
            a.fb[(row * nb + lane) * 2 + 1] = bad ? nan : ti;
        }
        if (lane < nf) {
            a.ff[(row * nf + lane) * 2] = bad ? nan : fr;
            a.ff[(row * nf + lane) * 2 + 1] = bad ? nan : fi;
        }
        if (lane == 0) {
            a.gain[row] = bad ? nan : gain;
            a.nu[row] = bad ? nan : nu;
            a.flag[row] = bad ? 1 : 0;
        }
    }
}

// shared design: flag[row] = the design's flag, or a NaN / inf in the row's y; one wave per row
__global__ __launch_bounds__(256) void eq_scan_kernel(const double *y, int64_t B, int64_t n_y, const uint8_t *design_flag, uint8_t *flag) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint8_t df = design_flag[0];
    for (int64_t row = (int64_t)blockIdx.x * 4 + wave; row < B; row += (int64_t)gridDim.x * 4) {
        const bool bad = scan_row(y + row * 2 * n_y, 2 * n_y, lane);
        if (lane == 0) flag[row] = (bad || df) ? 1 : 0;
    }
}

template <int LGM>
__device__ __forceinline__ void store_symbol(const EqRun &a, int64_t row, int t, int sel, double xr, double xi, const double *m0,
                                             const double *m1, double nu, bool bad) {
    const int64_t at = row * a.n + t;
    const double nan = __builtin_nan("");
    const int sym = bad ? 0 : sel;
    if (a.indices) a.indices[at] = sym;
    if (a.bits)
        for (int i = 0; i < a.m; i++) a.bits[at * a.m + i] = (uint8_t)((sym >> (a.m - 1 - i)) & 1);
    if (a.est) {
        a.est[at * 2] = bad ? nan : xr;
        a.est[at * 2 + 1] = bad ? nan : xi;
    }
    if constexpr (LGM > 0) {
#pragma unroll
        for (int i = 0; i < LGM; i++) a.llr[at * LGM + i] = bad ? nan : (m1[i] - m0[i]) / nu;
    }
}

template <int LGM>
__global__ __launch_bounds__(EQ_TILE) void eq_filter_kernel(EqRun a) {
    __shared__ double fr[64], fi[64], yr[EQ_TILE + 63], yi[EQ_TILE + 63], cr[CPX_EQ_MAX_M], ci[CPX_EQ_MAX_M];
    const int tid = threadIdx.x, nf = a.nf, n = a.n, n_y = a.n_y;
    const int64_t tpr = (n + EQ_TILE - 1) / EQ_TILE, tiles = a.rows * tpr;
    for (int i = tid; i < a.M; i += EQ_TILE) {
        cr[i] = a.cst[2 * i];
        ci[i] = a.cst[2 * i + 1];
    }
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t row = tile / tpr, drow = row * a.dstride;
        const int t0 = (int)(tile % tpr) * EQ_TILE;
        __syncthreads();                                       // the previous tile's window has been read
        if (tid < nf) {
            fr[tid] = a.ff[(drow * nf + tid) * 2];
            fi[tid] = a.ff[(drow * nf + tid) * 2 + 1];
        }
        const int64_t first = (int64_t)t0 + a.d - (nf - 1);    // the window's first sample
        for (int w = tid; w < EQ_TILE + nf - 1; w += EQ_TILE) {
            const int64_t s = first + w;
            const bool in = s >= 0 && s < n_y;
            yr[w] = in ? a.y[(row * n_y + s) * 2] : 0.0;
            yi[w] = in ? a.y[(row * n_y + s) * 2 + 1] : 0.0;
        }
        __syncthreads();
        const int t = t0 + tid;
        double sr = 0.0, si = 0.0;
        for (int i = 0; i < nf; i++) {
            const double ar = fr[i], ai = fi[i], br = yr[tid + nf - 1 - i], bi = yi[tid + nf - 1 - i];
            sr = sr + (ar * br - ai * bi);
            si = si + (ar * bi + ai * br);
        }
        if (t >= n) continue;
        if (a.zbuf) {
            const int64_t at = row * n + t;
            a.zbuf[at * 2] = sr;
            a.zbuf[at * 2 + 1] = si;
            continue;
        }
        const double gain = a.gain[drow], nu = a.nu[drow];
        const bool bad = a.flag[row] != 0;
        const double xr = (sr - 0.0) / gain, xi = (si - 0.0) / gain;
        double m0[LGM > 0 ? LGM : 1], m1[LGM > 0 ? LGM : 1];
        const int sel = slice<LGM>(xr, xi, cr, ci, a.M, m0, m1);
        store_symbol<LGM>(a, row, t, sel, xr, xi, m0, m1, nu, bad);
    }
}

template <int LGM>
__global__ __launch_bounds__(64) void eq_dfe_kernel(EqRun a) {
    extern __shared__ double eq_fbtab[];                       // fbr[nb][64], fbi[nb][64]
    __shared__ double cr[CPX_EQ_MAX_M], ci[CPX_EQ_MAX_M];
    __shared__ uint8_t hist[64 * 64];                          // decision of step t of lane's row at (t & 63) 64 + lane
    const int lane = threadIdx.x, nb = a.nb, n = a.n;
    double *fbr = eq_fbtab, *fbi = eq_fbtab + nb * 64;
    for (int i = lane; i < a.M; i += 64) {
        cr[i] = a.cst[2 * i];
        ci[i] = a.cst[2 * i + 1];
    }
    const int64_t groups = (a.rows + 63) / 64;
    for (int64_t grp = blockIdx.x; grp < groups; grp += gridDim.x) {
        const int64_t local = grp * 64 + lane;
        const bool valid = local < a.rows;
        const int64_t row = valid ? local : 0, drow = row * a.dstride;      // a lane without a row works on the first
        __syncthreads();
        for (int j = 0; j < nb; j++) {
            fbr[j * 64 + lane] = a.fb[(drow * nb + j) * 2];
            fbi[j * 64 + lane] = a.fb[(drow * nb + j) * 2 + 1];
        }
        const double gain = a.gain[drow], nu = a.nu[drow];
        const bool bad = a.flag[row] != 0;
        __syncthreads();
        const double *z = a.zbuf + row * (int64_t)n * 2;
        double znr = z[0], zni = z[1];
        for (int t = 0; t < n; t++) {
            const double sr = znr, si = zni;
            const int tn = t + 1 < n ? t + 1 : t;              // the next step's sums are fetched during this one
            znr = z[2 * (int64_t)tn];
            zni = z[2 * (int64_t)tn + 1];
            double br = 0.0, bi = 0.0;
            const int jmax = nb < t ? nb : t;
            for (int j = 1; j <= jmax; j++) {
                const int p = hist[((t - j) & 63) * 64 + lane];
                const double ar = fbr[(j - 1) * 64 + lane], ai = fbi[(j - 1) * 64 + lane], xr = cr[p], xi = ci[p];
                br = br + (ar * xr - ai * xi);
                bi = bi + (ar * xi + ai * xr);
            }
            const double xr = (sr - br) / gain, xi = (si - bi) / gain;
            double m0[LGM > 0 ? LGM : 1], m1[LGM > 0 ? LGM : 1];
            const int sel = slice<LGM>(xr, xi, cr, ci, a.M, m0, m1);
            hist[(t & 63) * 64 + lane] = (uint8_t)sel;
            if (valid) store_symbol<LGM>(a, row, t, sel, xr, xi, m0, m1, nu, bad);
        }
    }
}

// the limits both entry points share
int check_eq(const cpx_modem *md, double es, int64_t B, int64_t n, int L, int nf, int nb, int delay, bool have_nv, bool soft, bool any_output) {
    CPX_REQUIRE(md, CPX_EINVAL, "mmse_equalize: null pointer");
    CPX_REQUIRE(B >= 0, CPX_EINVAL, "mmse_equalize: B = %lld", (long long)B);
    CPX_REQUIRE(L >= 1 && L <= CPX_EQ_MAX_TAPS, CPX_EINVAL, "mmse_equalize: L = %d taps, the limit is 1 <= L <= %d", L, CPX_EQ_MAX_TAPS);
    CPX_REQUIRE(nf >= 1 && nf <= CPX_EQ_MAX_TAPS, CPX_EINVAL, "mmse_equalize: nf = %d, the limit is 1 <= nf <= %d", nf, CPX_EQ_MAX_TAPS);
    CPX_REQUIRE(nb >= 0 && nb <= CPX_EQ_MAX_TAPS, CPX_EINVAL, "mmse_equalize: nb = %d, the limit is 0 <= nb <= %d", nb, CPX_EQ_MAX_TAPS);
    CPX_REQUIRE(delay >= 0, CPX_EINVAL, "mmse_equalize: delay = %d, the limit is 0 <= delay", delay);
    CPX_REQUIRE(delay + nb <= nf + L - 2, CPX_EINVAL, "mmse_equalize: delay = %d, nb = %d, the limit is delay + nb <= nf + L - 2 = %d", delay,
                nb, nf + L - 2);
    CPX_REQUIRE(md->M >= 2 && md->M <= CPX_EQ_MAX_M, CPX_EINVAL, "mmse_equalize: a constellation of %d points, the limit is 2 <= M <= %d",
                md->M, CPX_EQ_MAX_M);
    CPX_REQUIRE(!soft || (1 << md->nbits) == md->M, CPX_EINVAL,
                "mmse_equalize: a constellation of %d points, the limit for bits and LLRs is M a power of two", md->M);
    CPX_REQUIRE(n >= 1 && n <= CPX_EQ_MAX_N, CPX_EINVAL, "mmse_equalize: n = %lld symbols, the limit is 1 <= n <= 2^30", (long long)n);
    CPX_REQUIRE(have_nv, CPX_EINVAL, "mmse_equalize: noise_var is required");
    CPX_REQUIRE(es > 0.0 && es < __builtin_huge_val(), CPX_EINVAL, "mmse_equalize: Es must be positive and finite");
    CPX_REQUIRE(any_output, CPX_EINVAL, "mmse_equalize: no output requested");
    return CPX_OK;
}

template <int LGM>
void launch_filter(const EqRun &a, unsigned grid, hipStream_t st) {
    hipLaunchKernelGGL((eq_filter_kernel<LGM>), dim3(grid), dim3(EQ_TILE), 0, st, a);
}
template <int LGM>
void launch_dfe(const EqRun &a, unsigned grid, hipStream_t st) {
    const unsigned lds = (unsigned)(16 * 64 * a.nb);
    // above 48 feedback taps the table and the static arrays pass 64 KiB (an error shows at hipGetLastError behind the launch)
    if (lds > 49152u) (void)hipFuncSetAttribute((const void *)eq_dfe_kernel<LGM>, hipFuncAttributeMaxDynamicSharedMemorySize, 65536);
    hipLaunchKernelGGL((eq_dfe_kernel<LGM>), dim3(grid), dim3(64), lds, st, a);
}

void run_filter(int lgm, const EqRun &a, unsigned grid, hipStream_t st) {
    switch (lgm) {
    case 0: return launch_filter<0>(a, grid, st);
    case 1: return launch_filter<1>(a, grid, st);
    case 2: return launch_filter<2>(a, grid, st);
    case 3: return launch_filter<3>(a, grid, st);
    case 4: return launch_filter<4>(a, grid, st);
    case 5: return launch_filter<5>(a, grid, st);
    case 6: return launch_filter<6>(a, grid, st);
    case 7: return launch_filter<7>(a, grid, st);
    default: return launch_filter<8>(a, grid, st);
    }
}
void run_dfe(int lgm, const EqRun &a, unsigned grid, hipStream_t st) {
    switch (lgm) {
    case 0: return launch_dfe<0>(a, grid, st);
    case 1: return launch_dfe<1>(a, grid, st);
    case 2: return launch_dfe<2>(a, grid, st);
    case 3: return launch_dfe<3>(a, grid, st);
    case 4: return launch_dfe<4>(a, grid, st);
    case 5: return launch_dfe<5>(a, grid, st);
    case 6: return launch_dfe<6>(a, grid, st);
    case 7: return launch_dfe<7>(a, grid, st);
    default: return launch_dfe<8>(a, grid, st);
    }
}

size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }      // every part of the arena block starts on a 256-byte boundary

}  // namespace

extern "C" {

int cpx_mmse_equalize_dev(const cpx_modem *md, double es, const double *d_y, const double *d_h, int h_batched, int64_t B, int64_t n, int L,
                          int tail, const double *d_noise_var, int nv_batched, int nf, int nb, int delay, int32_t *d_indices,
                          uint8_t *d_bits, double *d_estimate, double *d_llr, double *d_noise, double *d_ff, double *d_fb, double *d_gain,
                          void *stream) {
    CPX_TRACE("cpx_mmse_equalize_dev");
    const bool symbols = d_indices || d_bits || d_estimate || d_llr;
    if (int rc = check_eq(md, es, B, n, L, nf, nb, delay, d_noise_var != nullptr, d_bits || d_llr,
                          symbols || d_noise || d_ff || d_fb || d_gain))
        return rc;
    if (B == 0) return CPX_OK;
    CPX_REQUIRE(d_y && d_h, CPX_EINVAL, "mmse_equalize: null pointer");
    if (int rcd = check_handle_device(md->device, "mmse_equalize")) return rcd;
    hipStream_t st = pick_stream(stream);
    const int64_t n_y = n + (tail ? L - 1 : 0);
    // one design serves every row when nothing of it differs from row to row and none of it is asked for
    const bool shared = !h_batched && !nv_batched && !d_noise && !d_ff && !d_fb && !d_gain;
    const int64_t D = shared ? 1 : B;
    const size_t b_flag = up256((size_t)B + 1), b_ff = d_ff ? 0 : up256(16 * (size_t)D * nf), b_fb = d_fb ? 0 : up256(16 * (size_t)D * nb),
                 b_gain = d_gain ? 0 : up256(8 * (size_t)D), b_nu = d_noise ? 0 : up256(8 * (size_t)D);
    Scratch sc;
    uint8_t *blk = nullptr;
    if (int rc = sc.get(st, Slot::eq_design, b_flag + b_ff + b_fb + b_gain + b_nu, &blk)) return rc;
    uint8_t *flag = blk;
    double *ff = d_ff ? d_ff : (double *)(blk + b_flag);
    double *fb = d_fb ? d_fb : (double *)(blk + b_flag + b_ff);
    double *gain = d_gain ? d_gain : (double *)(blk + b_flag + b_ff + b_fb);
    double *nu = d_noise ? d_noise : (double *)(blk + b_flag + b_ff + b_fb + b_gain);

    const int64_t cus = device_cus();
    EqDesign da{d_h, d_noise_var, shared ? nullptr : d_y, D, n_y, L, nf, nb, delay, h_batched ? 1 : 0, nv_batched ? 1 : 0, es,
                ff, fb, gain, nu, shared ? flag + B : flag};
    const int64_t design_cap = cus * 8;
    hipLaunchKernelGGL(eq_design_kernel, dim3(grid_of(D, design_cap)), dim3(64), (unsigned)(8 * nf * (nf - 1)), st, da);
    CPX_HIP(hipGetLastError());
    if (shared) {
        hipLaunchKernelGGL(eq_scan_kernel, dim3(grid_of((B + 3) / 4, cus * 8)), dim3(256), 0, st, d_y, B, n_y, flag + B, flag);
        CPX_HIP(hipGetLastError());
    }
    const int lgm = d_llr ? md->nbits : 0;
    const int64_t filter_cap = cus * 16, dfe_cap = cus * 16;
    if (symbols) {
        EqRun ra{d_y, md->d_const, ff, fb, gain, nu, flag, B, shared ? 0 : 1, (int)n, (int)n_y, nf, nb, delay, md->M,
                 (1 << md->nbits) == md->M ? md->nbits : 0, d_indices, d_bits, d_estimate, d_llr, nullptr};
        const int64_t tpr = (n + EQ_TILE - 1) / EQ_TILE;
        if (nb == 0) {
            run_filter(lgm, ra, grid_of(B * tpr, filter_cap), st);
            CPX_HIP(hipGetLastError());
        } else {
            if (int rc = sc.get(st, Slot::eq_sums, 16 * (size_t)B * (size_t)n, &ra.zbuf)) return rc;
            run_filter(0, ra, grid_of(B * tpr, filter_cap), st);   // with zbuf set the filter pass writes nothing but the sums
            CPX_HIP(hipGetLastError());
            run_dfe(lgm, ra, grid_of((B + 63) / 64, dfe_cap), st);
            CPX_HIP(hipGetLastError());
        }
    }
    note_kernel("%s<%d> nf=%d nb=%d designs=%lld design_cap=%lld filter_cap=%lld dfe_cap=%lld",
                !symbols ? "eq_design_kernel" : nb ? "eq_dfe_kernel" : "eq_filter_kernel", symbols ? lgm : 0, nf, nb, (long long)D,
                (long long)design_cap, (long long)filter_cap, (long long)dfe_cap);
    return CPX_OK;
}

int cpx_mmse_equalize(const cpx_modem *md, double es, const double *y, const double *h, int h_batched, int64_t B, int64_t n, int L, int tail,
                      const double *noise_var, int nv_batched, int nf, int nb, int delay, int32_t *indices, uint8_t *bits,
                      double *estimate, double *llr, double *noise, double *ff, double *fb, double *gain) {
    CPX_TRACE("cpx_mmse_equalize");
    if (int rc = check_eq(md, es, B, n, L, nf, nb, delay, noise_var != nullptr, bits || llr,
                          indices || bits || estimate || llr || noise || ff || fb || gain))
        return rc;
    if (B == 0) return CPX_OK;
    CPX_REQUIRE(y && h, CPX_EINVAL, "mmse_equalize: null pointer");
    int rc = ensure_device();
    if (rc) return rc;
    const size_t b = (size_t)B, nm = (size_t)n * (size_t)md->nbits, n_y = (size_t)n + (tail ? (size_t)L - 1 : 0);
    HostStage::Out outs[8] = {{indices, 4 * b * (size_t)n}, {bits, b * nm},  {estimate, 16 * b * (size_t)n}, {llr, 8 * b * nm},
                              {noise, 8 * b},               {ff, 16 * b * (size_t)nf}, {fb, 16 * b * (size_t)nb}, {gain, 8 * b}};
    HostStage s;
    const double *dy, *dh, *dnv;
    if ((rc = s.in(y, 16 * b * n_y, &dy)) || (rc = s.in(h, 16 * (size_t)L * (h_batched ? b : 1), &dh)) ||
        (rc = s.in(noise_var, 8 * (nv_batched ? b : 1), &dnv)) || (rc = s.out(outs)))
        return rc;
    if ((rc = cpx_mmse_equalize_dev(md, es, dy, dh, h_batched, B, n, L, tail, dnv, nv_batched, nf, nb, delay, outs[0].as<int32_t>(),
                                    outs[1].as<uint8_t>(), outs[2].as<double>(), outs[3].as<double>(), outs[4].as<double>(),
                                    outs[5].as<double>(), outs[6].as<double>(), outs[7].as<double>(), s.st)))
        return rc;
    return s.get(outs);
}

}  // extern "C"
