// Adaptive equalisation: a linear (nb = 0) or decision-feedback (nb >= 1) equaliser that learns its taps from a training prefix and
// then tracks on its own decisions, with the LMS, the normalised LMS or the RLS update; nf <= 64 feed-forward taps one sample apart
// (sps samples per symbol: T/sps spacing), nb <= 64 feedback taps one symbol apart, any constellation of 2 .. 256 points.
//
// The rule (float64, real and imaginary parts separate doubles, every product rounded before it is added, every sum from 0.0 in
// ascending index order, -ffp-contract=off; a b = (ar br - ai bi, ar bi + ai br), a conj(b) = (ar br + ai bi, ai br - ar bi)),
// with d = delay, N = nf + nb, c the constellation, theta = (ff, fb), for t = 0 .. n-1:
//   regressor   x[i] = y[t sps + d - i] for i < nf, a sample outside the row read as 0.0 and multiplied like any other;
//               x[nf + j - 1] = -r_{t-j} (each part negated) for j = 1 .. nb, and 0.0 where t - j < 0, multiplied like any other.
//   output      z_t = (sum_{k<nf} theta_k x_k) + (sum_{nf<=k<N} theta_k x_k), no conjugate, the two sums formed separately.
//   decision    a^_t = the first minimum over a ascending of e = z_t - c[a], er er + ei ei, a later point winning only if strictly
//               smaller (the slicer of equalize.hip).  It is the 'indices' output at every t, training included.
//   reference   r_t = c[training[t]] for t < nt, else c[a^_t]; e_t = r_t - z_t.
//   lms         w = (mu er, mu ei); theta_k <- theta_k + w conj(x_k), k ascending.
//   nlms        the same with mu_t = mu / (eps + sum_{k<N} (xr xr + xi xi)) in place of mu.
//   rls         P = I / delta = (1.0 / delta) on the diagonal before the first step.  g_i = sum_{j<N} P[i][j] conj(x_j);
//               den = lambda + sum_{k<N} (xr gr - xi gi); kappa_i = (gr_i / den, gi_i / den); theta_i <- theta_i + kappa_i e_t;
//               P[i][j] <- ((Pr - qr) / lambda, (Pi - qi) / lambda) with q = kappa_i conj(g_j).
//   rejection   a row whose y (all n_y samples), ff0, fb0, step, forgetting, delta or eps holds a NaN or +-inf or lies outside its
//               range (step > 0, 0 < forgetting <= 1, delta > 0, eps >= 0), one of whose training labels is negative or >= M, one of
//               whose z_t is not finite, or one of whose den is not positive and finite: zero indices and bits, NaN everything else.
//
// ad_lms_kernel (lms, nlms): the recursion is a serial chain per row, so one row per lane, R rows per wave, one wave per workgroup.  In
//   LDS, lane-private columns [k][R]: the N taps, a ring of the last W samples (W the power of two >= nf; sample s at s & (W-1)) and a
//   ring of the last 64 reference labels (one byte each), so the chain needs no barrier.  The next step's sps samples are fetched
//   during this step.  R = 64 where 16 R (N + W) bytes and the 8 KiB of static tables fit the 160 KiB of a compute unit (N + W <= 152),
//   else R = 32 and the upper half of the wave retires: at nf = nb = 64 that is 96 KiB where 64 rows would need 192 KiB.
// ad_rls_kernel: a row per lane cannot hold P, so two rows per wave (N <= 32): lane i of a half owns row i of P, column by column in LDS
//   ([j][32], 16 KiB a row of the batch), and tap i.  x and g are written once and read by every lane as a broadcast; each lane runs
//   the sums of z and den itself, serially in k, so the rule's order needs no cross-lane reduction.  Three barriers of a one-wave
//   workgroup per step.
// A rejected row is found during the recursion, after some of its results were stored: the kernel rewrites the row at its end.  Both
// grids are grid-stride loops under a cap, so a result depends on neither the batch nor the grid.
#include "cpx_internal.h"
#include "cpx_slice.h"
#include "cpx_wave.h"                      // grid_of

using namespace cpx;

#define CPX_AD_MAX_TAPS 64                 // nf and nb
#define CPX_AD_RLS_MAX_TAPS 32             // nf + nb with 'rls': P is 16 KiB per row
#define CPX_AD_MAX_M 256
#define CPX_AD_MAX_N (1 << 30)
#define CPX_AD_MAX_SPS 8
#define CPX_AD_LDS_MAX 163840u

namespace {

enum { AD_LMS = 0, AD_NLMS = 1, AD_RLS = 2 };

struct AdRun {
    const double *y, *cst;                 // [rows][n_y][2], [M][2]
    const int32_t *training;               // [nt] or [rows][nt]
    const double *p1, *p2;                 // lms, nlms: step, unused; rls: forgetting, delta; [1] or [rows]
    const double *ff0, *fb0;               // [nf][2] or [rows][nf][2], the same with nb; null = zeros
    double eps;
    int64_t rows, n_y, nt, d;
    int n, nf, nb, sps, M, m, alg;         // m = 0: M is no power of two
    int R, W;                              // ad_lms_kernel: rows per wave, ring length
    int tr_batched, p1_batched, p2_batched, ff0_batched, fb0_batched;
    int32_t *indices;
    uint8_t *bits;
    double *est, *err, *ff, *fb;
};

__device__ __forceinline__ void store_step(const AdRun &a, int64_t row, int t, int sel, double zr, double zi, double er, double ei) {
    const int64_t at = row * a.n + t;
    if (a.indices) a.indices[at] = sel;
    if (a.bits)
        for (int i = 0; i < a.m; i++) a.bits[at * a.m + i] = (uint8_t)((sel >> (a.m - 1 - i)) & 1);
    if (a.est) {
        a.est[at * 2] = zr;
        a.est[at * 2 + 1] = zi;
    }
    if (a.err) {
        a.err[at * 2] = er;
        a.err[at * 2 + 1] = ei;
    }
}

// a rejected row: steps t0, t0 + stride, .. and taps k0, k0 + stride, ..
__device__ __forceinline__ void store_rejected(const AdRun &a, int64_t row, int first, int stride) {
    const double nan = __builtin_nan("");
    for (int t = first; t < a.n; t += stride) store_step(a, row, t, 0, nan, nan, nan, nan);
    for (int k = first; k < a.nf; k += stride)
        if (a.ff) a.ff[(row * a.nf + k) * 2] = a.ff[(row * a.nf + k) * 2 + 1] = nan;
    for (int k = first; k < a.nb; k += stride)
        if (a.fb) a.fb[(row * a.nb + k) * 2] = a.fb[(row * a.nb + k) * 2 + 1] = nan;
}

__device__ __forceinline__ double sample(const double *yrow, int64_t s, int64_t n_y, int part) {
    return s >= 0 && s < n_y ? yrow[2 * s + part] : 0.0;
}

__global__ __launch_bounds__(64) void ad_lms_kernel(AdRun a) {
    extern __shared__ double ad_cols[];                        // thr[N][R], thi[N][R], wr[W][R], wi[W][R]
    __shared__ double cr[CPX_AD_MAX_M], ci[CPX_AD_MAX_M];
    __shared__ uint8_t hist[64 * 64];                          // reference label of step t of lane's row at (t & 63) 64 + lane
    const int lane = threadIdx.x, R = a.R, W = a.W, nf = a.nf, nb = a.nb, N = nf + nb, n = a.n, sps = a.sps, M = a.M;
    const int64_t n_y = a.n_y, d = a.d, nt = a.nt;
    double *thr = ad_cols, *thi = thr + N * R, *wr = thi + N * R, *wi = wr + W * R;
    for (int i = lane; i < M; i += 64) {
        cr[i] = a.cst[2 * i];
        ci[i] = a.cst[2 * i + 1];
    }
    __syncthreads();
    if (lane >= R) return;                                     // no barrier from here on: every column is the lane's own
    const bool nlms = a.alg == AD_NLMS;
    const int64_t groups = (a.rows + R - 1) / R;
    for (int64_t grp = blockIdx.x; grp < groups; grp += gridDim.x) {
        const int64_t local = grp * R + lane;
        const bool valid = local < a.rows;
        const int64_t row = valid ? local : 0;                 // a lane without a row works on the first
        const double *yrow = a.y + row * 2 * n_y;
        bool bad = false;
        for (int r = 0; r < R && grp * R + r < a.rows; r++) {  // the group's rows are scanned by all its lanes, a row at a time
            const bool any = scan_lanes(a.y + (grp * R + r) * 2 * n_y, 2 * n_y, lane, R) != 0ull;
            if (r == lane) bad = any;
        }
        const double mu = a.p1[a.p1_batched ? row : 0], eps = a.eps;
        bad |= not_finite(mu) || !(mu > 0.0) || not_finite(eps) || !(eps >= 0.0);
        for (int k = 0; k < N; k++) {
            const double *src = k < nf ? a.ff0 : a.fb0;
            double vr = 0.0, vi = 0.0;
            if (src) {
                const int64_t at = k < nf ? (a.ff0_batched ? row * nf : 0) + k : (a.fb0_batched ? row * nb : 0) + (k - nf);
                vr = src[2 * at];
                vi = src[2 * at + 1];
            }
            bad |= not_finite(vr) || not_finite(vi);
            thr[k * R + lane] = vr;
            thi[k * R + lane] = vi;
        }
        for (int w = 0; w < W; w++) {                          // the ring before step 0: samples d - W + 1 .. d
            const int64_t s = d - w;
            const int at = (int)(s & (W - 1)) * R + lane;
            wr[at] = sample(yrow, s, n_y, 0);
            wi[at] = sample(yrow, s, n_y, 1);
        }
        for (int k = 0; k < 64; k++) hist[k * 64 + lane] = 0;
        const int32_t *tr = a.training + (a.tr_batched ? row * nt : 0);

        for (int t = 0; t < n && !bad; t++) {
            const int64_t s0 = (int64_t)t * sps + d;           // x[0] is sample s0; the next step's are s0 + 1 .. s0 + sps
            double nr[CPX_AD_MAX_SPS], ni[CPX_AD_MAX_SPS];
#pragma unroll
            for (int q = 0; q < CPX_AD_MAX_SPS; q++)
                if (q < sps) {
                    nr[q] = sample(yrow, s0 + 1 + q, n_y, 0);
                    ni[q] = sample(yrow, s0 + 1 + q, n_y, 1);
                }
            double fr = 0.0, fi = 0.0, pw = 0.0;
            for (int i = 0; i < nf; i++) {
                const int at = (int)((s0 - i) & (W - 1)) * R + lane;
                const double ar = thr[i * R + lane], ai = thi[i * R + lane], xr = wr[at], xi = wi[at];
                fr = fr + (ar * xr - ai * xi);
                fi = fi + (ar * xi + ai * xr);
                if (nlms) pw = pw + (xr * xr + xi * xi);
            }
            double br = 0.0, bi = 0.0;
            for (int j = 1; j <= nb; j++) {
                const int p = hist[((t - j) & 63) * 64 + lane];
                const double xr = j <= t ? -cr[p] : 0.0, xi = j <= t ? -ci[p] : 0.0;
                const double ar = thr[(nf + j - 1) * R + lane], ai = thi[(nf + j - 1) * R + lane];
                br = br + (ar * xr - ai * xi);
                bi = bi + (ar * xi + ai * xr);
                if (nlms) pw = pw + (xr * xr + xi * xi);
            }
            const double zr = fr + br, zi = fi + bi;
            double m0[1], m1[1];
            const int sel = slice<0>(zr, zi, cr, ci, M, m0, m1);
            int lab = sel;
            if (t < nt) {
                lab = tr[t];
                if (lab < 0 || lab >= M) {
                    bad = true;
                    lab = 0;
                }
            }
            if (not_finite(zr) || not_finite(zi)) bad = true;
            if (bad) break;
            const double er = cr[lab] - zr, ei = ci[lab] - zi;
            const double mt = nlms ? mu / (eps + pw) : mu;
            const double ur = mt * er, ui = mt * ei;
            for (int i = 0; i < nf; i++) {
                const int at = (int)((s0 - i) & (W - 1)) * R + lane;
                const double xr = wr[at], xi = wi[at];
                thr[i * R + lane] = thr[i * R + lane] + (ur * xr + ui * xi);
                thi[i * R + lane] = thi[i * R + lane] + (ui * xr - ur * xi);
            }
            for (int j = 1; j <= nb; j++) {
                const int p = hist[((t - j) & 63) * 64 + lane];
                const double xr = j <= t ? -cr[p] : 0.0, xi = j <= t ? -ci[p] : 0.0;
                thr[(nf + j - 1) * R + lane] = thr[(nf + j - 1) * R + lane] + (ur * xr + ui * xi);
                thi[(nf + j - 1) * R + lane] = thi[(nf + j - 1) * R + lane] + (ui * xr - ur * xi);
            }
            hist[(t & 63) * 64 + lane] = (uint8_t)lab;         // after the update: with nb = 64 it takes the place of step t - 64
#pragma unroll
            for (int q = 0; q < CPX_AD_MAX_SPS; q++)
                if (q < sps) {
                    const int at = (int)((s0 + 1 + q) & (W - 1)) * R + lane;
                    wr[at] = nr[q];
                    wi[at] = ni[q];
                }
            if (valid) store_step(a, row, t, sel, zr, zi, er, ei);
        }
        if (!valid) continue;
        if (bad) {
            store_rejected(a, row, 0, 1);
            continue;
        }
        for (int k = 0; k < nf; k++)
            if (a.ff) {
                a.ff[(row * nf + k) * 2] = thr[k * R + lane];
                a.ff[(row * nf + k) * 2 + 1] = thi[k * R + lane];
            }
        for (int k = 0; k < nb; k++)
            if (a.fb) {
                a.fb[(row * nb + k) * 2] = thr[(nf + k) * R + lane];
                a.fb[(row * nb + k) * 2 + 1] = thi[(nf + k) * R + lane];
            }
    }
}

__global__ __launch_bounds__(64) void ad_rls_kernel(AdRun a) {
    __shared__ double Pr[2][32 * 32], Pi[2][32 * 32];          // P[i][j] of a half's row at [j 32 + i]
    __shared__ double xsr[2][32], xsi[2][32], gsr[2][32], gsi[2][32], tsr[2][32], tsi[2][32];
    __shared__ double cr[CPX_AD_MAX_M], ci[CPX_AD_MAX_M];
    __shared__ int hist[2][32];                                // reference label of step t at t & 31 (nb <= 31)
    const int lane = threadIdx.x, h = lane >> 5, i = lane & 31, nf = a.nf, nb = a.nb, N = nf + nb, n = a.n, sps = a.sps, M = a.M;
    const int64_t n_y = a.n_y, d = a.d, nt = a.nt;
    for (int k = lane; k < M; k += 64) {
        cr[k] = a.cst[2 * k];
        ci[k] = a.cst[2 * k + 1];
    }
    double *pr = Pr[h], *pi = Pi[h];
    const int64_t pairs = (a.rows + 1) / 2;
    for (int64_t pair = blockIdx.x; pair < pairs; pair += gridDim.x) {
        const int64_t local = pair * 2 + h;
        const bool valid = local < a.rows;
        const int64_t row = valid ? local : 0;                 // a half without a row works on the first
        const double *yrow = a.y + row * 2 * n_y;
        __syncthreads();                                       // the previous pair's tables have been read
        const unsigned long long in_y = scan_lanes(yrow, 2 * n_y, i, 32);  // each half scans its own row
        const double lam = a.p1[a.p1_batched ? row : 0], dl = a.p2[a.p2_batched ? row : 0];
        double vr = 0.0, vi = 0.0;
        if (i < N) {
            const double *src = i < nf ? a.ff0 : a.fb0;
            if (src) {
                const int64_t at = i < nf ? (a.ff0_batched ? row * nf : 0) + i : (a.fb0_batched ? row * nb : 0) + (i - nf);
                vr = src[2 * at];
                vi = src[2 * at + 1];
            }
            tsr[h][i] = vr;
            tsi[h][i] = vi;
            const double p0 = 1.0 / dl;
            for (int j = 0; j < N; j++) {
                pr[j * 32 + i] = j == i ? p0 : 0.0;
                pi[j * 32 + i] = 0.0;
            }
        }
        hist[h][i] = 0;
        const unsigned long long in_taps = __ballot(not_finite(vr) || not_finite(vi));
        bool bad = (((in_y | in_taps) >> (32 * h)) & 0xffffffffull) != 0ull;
        bad |= not_finite(lam) || !(lam > 0.0) || !(lam <= 1.0) || not_finite(dl) || !(dl > 0.0);
        const int32_t *tr = a.training + (a.tr_batched ? row * nt : 0);
        double thr = vr, thi = vi;                             // tap i
        double nyr = i < nf ? sample(yrow, d - i, n_y, 0) : 0.0, nyi = i < nf ? sample(yrow, d - i, n_y, 1) : 0.0;
        __syncthreads();

        for (int t = 0; t < n; t++) {
            double xr = nyr, xi = nyi;                         // the next step's sample is fetched during this one
            if (i < nf) {
                const int64_t s = (int64_t)(t + 1) * sps + d - i;
                nyr = sample(yrow, s, n_y, 0);
                nyi = sample(yrow, s, n_y, 1);
            } else if (i < N) {
                const int j = i - nf + 1, p = hist[h][(t - j) & 31];
                xr = j <= t ? -cr[p] : 0.0;
                xi = j <= t ? -ci[p] : 0.0;
            }
            if (i < N) {
                xsr[h][i] = xr;
                xsi[h][i] = xi;
            }
            __syncthreads();
            double fr = 0.0, fi = 0.0, br = 0.0, bi = 0.0;
            for (int k = 0; k < nf; k++) {
                const double ar = tsr[h][k], ai = tsi[h][k], ur = xsr[h][k], ui = xsi[h][k];
                fr = fr + (ar * ur - ai * ui);
                fi = fi + (ar * ui + ai * ur);
            }
            for (int k = nf; k < N; k++) {
                const double ar = tsr[h][k], ai = tsi[h][k], ur = xsr[h][k], ui = xsi[h][k];
                br = br + (ar * ur - ai * ui);
                bi = bi + (ar * ui + ai * ur);
            }
            const double zr = fr + br, zi = fi + bi;
            double gr = 0.0, gi = 0.0;
            if (i < N) {
                for (int j = 0; j < N; j++) {
                    const double ar = pr[j * 32 + i], ai = pi[j * 32 + i], ur = xsr[h][j], ui = xsi[h][j];
                    gr = gr + (ar * ur + ai * ui);
                    gi = gi + (ai * ur - ar * ui);
                }
                gsr[h][i] = gr;
                gsi[h][i] = gi;
            }
            __syncthreads();
            double sum = 0.0;
            for (int k = 0; k < N; k++) sum = sum + (xsr[h][k] * gsr[h][k] - xsi[h][k] * gsi[h][k]);
            const double den = lam + sum;
            double m0[1], m1[1];
            const int sel = slice<0>(zr, zi, cr, ci, M, m0, m1);
            int lab = sel;
            if (t < nt) {
                lab = tr[t];
                if (lab < 0 || lab >= M) {
                    bad = true;
                    lab = 0;
                }
            }
            bad |= not_finite(zr) || not_finite(zi) || not_finite(den) || !(den > 0.0);
            const double er = cr[lab] - zr, ei = ci[lab] - zi;
            if (i < N) {
                const double kr = gr / den, ki = gi / den;
                thr = thr + (kr * er - ki * ei);
                thi = thi + (kr * ei + ki * er);
                tsr[h][i] = thr;
                tsi[h][i] = thi;
                for (int j = 0; j < N; j++) {
                    const double ur = gsr[h][j], ui = gsi[h][j];
                    pr[j * 32 + i] = (pr[j * 32 + i] - (kr * ur + ki * ui)) / lam;
                    pi[j * 32 + i] = (pi[j * 32 + i] - (ki * ur - kr * ui)) / lam;
                }
            }
            if (i == 0) {
                hist[h][t & 31] = lab;
                if (valid) store_step(a, row, t, sel, zr, zi, er, ei);
            }
            __syncthreads();
        }
        if (!valid) continue;
        if (bad) {
            store_rejected(a, row, i, 32);
            continue;
        }
        if (i < nf && a.ff) {
            a.ff[(row * nf + i) * 2] = thr;
            a.ff[(row * nf + i) * 2 + 1] = thi;
        }
        if (i >= nf && i < N && a.fb) {
            a.fb[(row * nb + i - nf) * 2] = thr;
            a.fb[(row * nb + i - nf) * 2 + 1] = thi;
        }
    }
}

// a parameter's host values, where the caller has them: every one must satisfy lo < v (or lo <= v with `closed`) and v <= hi; a NaN
// passes, it rejects its row
bool in_range(const double *v, int64_t count, double lo, bool closed, double hi) {
    for (int64_t i = 0; v && i < count; i++)
        if (v[i] < lo || (!closed && v[i] == lo) || v[i] > hi) return false;
    return true;
}

// the limits both entry points share; step, forgetting and delta are host values or null (the device form cannot read them: the kernels
// reject the rows)
int check_adaptive(const cpx_modem *md, int64_t B, int64_t n_y, int64_t n, int sps, int64_t nt, int nf, int nb, int delay, int algorithm,
                   bool have_step, bool have_forgetting, bool have_delta, const double *step, int64_t n_step, const double *forgetting,
                   int64_t n_forgetting, const double *delta, int64_t n_delta, double eps, bool want_bits, bool any_output) {
    const double inf = __builtin_huge_val();
    CPX_REQUIRE(md, CPX_EINVAL, "adaptive_equalize: null pointer");
    CPX_REQUIRE(B >= 0, CPX_EINVAL, "adaptive_equalize: B = %lld", (long long)B);
    CPX_REQUIRE(algorithm == AD_LMS || algorithm == AD_NLMS || algorithm == AD_RLS, CPX_EINVAL,
                "adaptive_equalize: algorithm = %d, the limit is 0 ('lms'), 1 ('nlms') or 2 ('rls')", algorithm);
    CPX_REQUIRE(nf >= 1 && nf <= CPX_AD_MAX_TAPS, CPX_EINVAL, "adaptive_equalize: nf = %d, the limit is 1 <= nf <= %d", nf, CPX_AD_MAX_TAPS);
    CPX_REQUIRE(nb >= 0 && nb <= CPX_AD_MAX_TAPS, CPX_EINVAL, "adaptive_equalize: nb = %d, the limit is 0 <= nb <= %d", nb, CPX_AD_MAX_TAPS);
    CPX_REQUIRE(algorithm != AD_RLS || nf + nb <= CPX_AD_RLS_MAX_TAPS, CPX_EINVAL,
                "adaptive_equalize: nf + nb = %d with 'rls', the limit is nf + nb <= %d", nf + nb, CPX_AD_RLS_MAX_TAPS);
    CPX_REQUIRE(delay >= 0, CPX_EINVAL, "adaptive_equalize: delay = %d, the limit is 0 <= delay", delay);
    CPX_REQUIRE(sps >= 1 && sps <= CPX_AD_MAX_SPS, CPX_EINVAL, "adaptive_equalize: sps = %d, the limit is 1 <= sps <= %d", sps, CPX_AD_MAX_SPS);
    CPX_REQUIRE(md->M >= 2 && md->M <= CPX_AD_MAX_M, CPX_EINVAL, "adaptive_equalize: a constellation of %d points, the limit is 2 <= M <= %d",
                md->M, CPX_AD_MAX_M);
    CPX_REQUIRE(!want_bits || (1 << md->nbits) == md->M, CPX_EINVAL,
                "adaptive_equalize: a constellation of %d points, the limit for bits is M a power of two", md->M);
    CPX_REQUIRE(n >= 1 && n <= CPX_AD_MAX_N, CPX_EINVAL, "adaptive_equalize: n = %lld symbols, the limit is 1 <= n <= 2^30", (long long)n);
    CPX_REQUIRE(n_y >= 0 && n_y <= (int64_t)CPX_AD_MAX_N * CPX_AD_MAX_SPS, CPX_EINVAL,
                "adaptive_equalize: n_y = %lld samples, the limit is 0 <= n_y <= 2^33", (long long)n_y);
    CPX_REQUIRE(nt >= 0 && nt <= n, CPX_EINVAL, "adaptive_equalize: nt = %lld training symbols, the limit is 0 <= nt <= n = %lld",
                (long long)nt, (long long)n);
    if (algorithm == AD_RLS) {
        CPX_REQUIRE(!have_step, CPX_EINVAL, "adaptive_equalize: step is given with 'rls', which takes forgetting and delta");
        CPX_REQUIRE(have_forgetting && have_delta, CPX_EINVAL, "adaptive_equalize: forgetting and delta are required with 'rls'");
        CPX_REQUIRE(in_range(forgetting, n_forgetting, 0.0, false, 1.0), CPX_EINVAL,
                    "adaptive_equalize: forgetting, the limit is 0 < forgetting <= 1");
        CPX_REQUIRE(in_range(delta, n_delta, 0.0, false, inf), CPX_EINVAL, "adaptive_equalize: delta, the limit is delta > 0");
    } else {
        CPX_REQUIRE(have_step, CPX_EINVAL, "adaptive_equalize: step is required with 'lms' and 'nlms'");
        CPX_REQUIRE(in_range(step, n_step, 0.0, false, inf), CPX_EINVAL, "adaptive_equalize: step, the limit is step > 0");
        CPX_REQUIRE(!(eps < 0.0), CPX_EINVAL, "adaptive_equalize: eps = %g, the limit is eps >= 0", eps);
    }
    CPX_REQUIRE(any_output, CPX_EINVAL, "adaptive_equalize: no output requested");
    return CPX_OK;
}

int ring_length(int nf) {
    int w = 1;
    while (w < nf) w *= 2;
    return w;
}

}  // namespace

extern "C" {

int cpx_adaptive_equalize_dev(const cpx_modem *md, const double *d_y, int64_t B, int64_t n_y, int64_t n, int sps, const int32_t *d_training,
                              int tr_batched, int64_t nt, int nf, int nb, int delay, int algorithm, const double *d_step, int step_batched,
                              const double *d_forgetting, int fg_batched, const double *d_delta, int dl_batched, double eps,
                              const double *d_ff0, int ff0_batched, const double *d_fb0, int fb0_batched, int32_t *d_indices,
                              uint8_t *d_bits, double *d_estimate, double *d_error, double *d_ff, double *d_fb, void *stream) {
    CPX_TRACE("cpx_adaptive_equalize_dev");
    if (int rc = check_adaptive(md, B, n_y, n, sps, nt, nf, nb, delay, algorithm, d_step != nullptr, d_forgetting != nullptr,
                                d_delta != nullptr, nullptr, 0, nullptr, 0, nullptr, 0, eps, d_bits != nullptr,
                                d_indices || d_bits || d_estimate || d_error || d_ff || d_fb))
        return rc;
    if (B == 0) return CPX_OK;
    CPX_REQUIRE(d_y && (d_training || nt == 0), CPX_EINVAL, "adaptive_equalize: null pointer");
    if (int rcd = check_handle_device(md->device, "adaptive_equalize")) return rcd;
    hipStream_t st = pick_stream(stream);
    const bool rls = algorithm == AD_RLS;
    AdRun ra{d_y, md->d_const, d_training, rls ? d_forgetting : d_step, rls ? d_delta : nullptr, d_ff0, d_fb0, eps, B, n_y, nt, delay,
             (int)n, nf, nb, sps, md->M, (1 << md->nbits) == md->M ? md->nbits : 0, algorithm, 64, ring_length(nf), tr_batched ? 1 : 0,
             rls ? (fg_batched ? 1 : 0) : (step_batched ? 1 : 0), dl_batched ? 1 : 0, ff0_batched ? 1 : 0, fb0_batched ? 1 : 0,
             d_indices, d_bits, d_estimate, d_error, d_ff, d_fb};
    const int64_t cus = device_cus();
    if (rls) {
        const int64_t rls_cap = cus * 4;
        hipLaunchKernelGGL(ad_rls_kernel, dim3(grid_of((B + 1) / 2, rls_cap)), dim3(64), 0, st, ra);
        CPX_HIP(hipGetLastError());
        note_kernel("ad_rls_kernel nf=%d nb=%d rows_per_wave=2 rls_cap=%lld", nf, nb, (long long)rls_cap);
        return CPX_OK;
    }
    const unsigned stat = 16 * CPX_AD_MAX_M + 64 * 64;          // cr, ci, hist
    if (16u * 64u * (unsigned)(nf + nb + ra.W) + stat > CPX_AD_LDS_MAX) ra.R = 32;
    const unsigned lds = 16u * (unsigned)ra.R * (unsigned)(nf + nb + ra.W);
    // above 48 KiB the dynamic table needs the attribute (an error shows at hipGetLastError behind the launch)
    if (lds > 49152u) (void)hipFuncSetAttribute((const void *)ad_lms_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(CPX_AD_LDS_MAX - stat));
    const int64_t lms_cap = cus * 4;
    hipLaunchKernelGGL(ad_lms_kernel, dim3(grid_of((B + ra.R - 1) / ra.R, lms_cap)), dim3(64), lds, st, ra);
    CPX_HIP(hipGetLastError());
    note_kernel("ad_lms_kernel %s nf=%d nb=%d rows_per_wave=%d lds=%u lms_cap=%lld", algorithm == AD_NLMS ? "nlms" : "lms", nf, nb, ra.R,
                lds + stat, (long long)lms_cap);
    return CPX_OK;
}

int cpx_adaptive_equalize(const cpx_modem *md, const double *y, int64_t B, int64_t n_y, int64_t n, int sps, const int32_t *training,
                          int tr_batched, int64_t nt, int nf, int nb, int delay, int algorithm, const double *step, int step_batched,
                          const double *forgetting, int fg_batched, const double *delta, int dl_batched, double eps, const double *ff0,
                          int ff0_batched, const double *fb0, int fb0_batched, int32_t *indices, uint8_t *bits, double *estimate,
                          double *error, double *ff, double *fb) {
    CPX_TRACE("cpx_adaptive_equalize");
    if (int rc = check_adaptive(md, B, n_y, n, sps, nt, nf, nb, delay, algorithm, step != nullptr, forgetting != nullptr, delta != nullptr,
                                step, step_batched ? B : 1, forgetting, fg_batched ? B : 1, delta, dl_batched ? B : 1, eps,
                                bits != nullptr, indices || bits || estimate || error || ff || fb))
        return rc;
    if (B == 0) return CPX_OK;
    CPX_REQUIRE(y && (training || nt == 0), CPX_EINVAL, "adaptive_equalize: null pointer");
    int rc = ensure_device();
    if (rc) return rc;
    const size_t b = (size_t)B, nn = (size_t)n;
    HostStage::Out outs[6] = {{indices, 4 * b * nn},   {bits, b * nn * (size_t)md->nbits}, {estimate, 16 * b * nn},
                              {error, 16 * b * nn},    {ff, 16 * b * (size_t)nf},          {fb, 16 * b * (size_t)nb}};
    HostStage s;
    const double *dy, *dstep = nullptr, *dfg = nullptr, *ddl = nullptr, *dff0 = nullptr, *dfb0 = nullptr;
    const int32_t *dtr = nullptr;
    if ((rc = s.in(y, 16 * b * (size_t)n_y, &dy)) || (nt > 0 && (rc = s.in(training, 4 * (size_t)nt * (tr_batched ? b : 1), &dtr))) ||
        (step && (rc = s.in(step, 8 * (step_batched ? b : 1), &dstep))) ||
        (forgetting && (rc = s.in(forgetting, 8 * (fg_batched ? b : 1), &dfg))) ||
        (delta && (rc = s.in(delta, 8 * (dl_batched ? b : 1), &ddl))) ||
        (ff0 && (rc = s.in(ff0, 16 * (size_t)nf * (ff0_batched ? b : 1), &dff0))) ||
        (fb0 && (rc = s.in(fb0, 16 * (size_t)nb * (fb0_batched ? b : 1), &dfb0))) || (rc = s.out(outs)))
        return rc;
    if ((rc = cpx_adaptive_equalize_dev(md, dy, B, n_y, n, sps, dtr, tr_batched, nt, nf, nb, delay, algorithm, dstep, step_batched, dfg,
                                        fg_batched, ddl, dl_batched, eps, dff0, ff0_batched, dfb0, fb0_batched, outs[0].as<int32_t>(),
                                        outs[1].as<uint8_t>(), outs[2].as<double>(), outs[3].as<double>(), outs[4].as<double>(),
                                        outs[5].as<double>(), s.st)))
        return rc;
    return s.get(outs);
}

}  // extern "C"
