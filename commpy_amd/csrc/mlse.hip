// Trellis equalisation of a known multipath channel: maximum-likelihood sequence estimation (Viterbi) and its max-log-MAP soft output
// with a-priori LLRs, for M <= 16 points, L >= 2 taps and S = M^(L-1) <= 256 states, blocks of 1 .. 4096 symbols.
//
// A block of n symbols a_0 .. a_{n-1} with values c[a] is sent in silence: y_t = sum_l h_l c[a_{t-l}] + w_t, the terms with t - l < 0 or
// t - l >= n absent.  The rule (float64, real and imaginary parts separate doubles, every product rounded before it is added, sums in
// the order written, -ffp-contract=off):
//   state after step t  s' = a_t M^(L-2) + ... + a_{t-L+2}; candidates into s' in the order old = 0 .. M-1, pred = (s' mod M^(L-2)) M + old
//   branch metric       xh = sum_{l=0}^{L-1} h_l c[a_{t-l}], l ascending from 0.0, a product is (hr cr - hi ci, hr ci + hi cr), the terms
//                       with t - l < 0 skipped; e = y_t - xh; d = er er + ei ei
//   prior cost          P_t[a] = noise_var (sum of La over the bits 1 of a, MSB first, from 0.0); 0.0 without a prior
//   forward             alpha_0 = 0; alpha_{t+1}[s'] = (first minimum over old of alpha_t[pred] + d) + P_t[a_t]; a later candidate wins only
//                       if strictly smaller; the winning old is the decision
//   tail                beta_n[s] = sum_{j=0}^{L-2} |y_{n+j} - xh_j(s)|^2, j ascending from 0.0, xh_j(s) over l = j+1 .. L-1 (and
//                       n + j - l >= 0); beta_n = 0 without the tail
//   hard output         s* = first minimum of alpha_n + beta_n, that minimum is the metric; the indices from s* and the decisions
//   soft output         beta_t[s] = min over a of (d_t(s, a) + (P_t[a] + beta_{t+1}[s'])); Lambda_t[s'] = alpha_{t+1}[s'] + beta_{t+1}[s'];
//                       llr[t m + i] = (min over the s' whose a_t has bit i = 1 of Lambda_t - the same with bit i = 0) / noise_var
//   A row whose y, h, prior or noise_var holds a NaN or +-inf (or a noise_var <= 0) is rejected: zero indices and bits, NaN metric,
//   NaN LLRs.
//
// mlse_kernel<LGM, LGS>: one state per lane.  A workgroup is W = max(64, S) lanes and holds R = W / S rows: 64 / S rows share a wave
//   when S < 64, a row takes S / 64 waves when S > 64.  L = LGS / LGM + 1 is a compile-time constant.  Per row and once: z[s'], the
//   sum's prefix over l <= L-2 (a register, and in LDS for the backward pass), and w[old] = h_{L-1} c[old] (M register pairs), so that
//   xh = z + w is the rule's sum; the first L-1 steps take the masked prefix from the tap and point tables in LDS.  A step: the lane
//   hands on its metric through LDS (two buffers in turn: one barrier per step), reads the M metrics of its predecessors -- they are
//   neighbours -- in 16-byte pieces, and takes the first minimum of M candidates.  Decisions are one ballot word per wave and label bit,
//   in LDS where the block's words fit 48 KiB, else in the workgroup's slab of the scratch arena.  The traceback is walked by every
//   lane of a row; lane i keeps the symbol of step tb0 + i of a segment of S steps.
//   Soft output: the forward pass also stores alpha of every step in the workgroup's slab of the scratch arena ([n][W] doubles, every
//   lane reads back only what it wrote); the backward pass carries beta through LDS and reduces Lambda over the lanes per label bit
//   (over the state bits below the label in registers, DPP moves for the first four; the S >> CB values left per row go
//   through LDS with beta, and lane i of the row takes label bit i's two minima from them).
//   The grid is persistent: what the runtime's occupancy query says is resident, cut down so that the slabs stay within
//   MLSE_SCRATCH_CAP; a workgroup strides over the groups of R rows, so a result depends on neither the batch size nor the grid.
#include "cpx_internal.h"
#include "cpx_wave.h"

using namespace cpx;

#define CPX_MLSE_MAX_M 16
#define CPX_MLSE_MAX_STATES 256
#define CPX_MLSE_MAX_N 4096
#define MLSE_DEC_LDS_MAX 49152u            // a block's decision words stay in LDS up to this size
#define MLSE_SCRATCH_CAP (256ull << 20)    // of decision and alpha slabs together

namespace {

struct MlseArgs {
    const double *y;                       // [B][n_y][2]
    const double *h;                       // [L][2] or [B][L][2]
    const double *cst;                     // [M][2]
    const double *nv;                      // null, [1] or [B]
    const double *prior;                   // null or [B][n m]
    int64_t B;
    int n, n_y, h_batched, nv_batched, tail;
    int32_t *indices;                      // [B][n] or null
    uint8_t *bits;                         // [B][n m] or null
    double *metric;                        // [B] or null
    double *llr;                           // [B][n m] or null
    unsigned long long *dec_g;             // null: the decisions are in LDS; else [grid][n][LGM][waves]
    double *alpha_g;                       // soft output: [grid][n][W]
};

__device__ __forceinline__ bool not_finite(double v) { return !(__builtin_fabs(v) < __builtin_huge_val()); }

__device__ __forceinline__ double xmin(double v, int d) {
    const double o = __shfl_xor(v, d);
    return o < v ? o : v;
}

// one 32-bit half per DPP move; every lane is active where these are used
template <int CTRL>
__device__ __forceinline__ double dpp_mov(double v) {
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, 0xf, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, 0xf, 0xf, false);
    return __hiloint2double(hi, lo);
}

// min over the lane pairs of bit BIT, for BIT ascending from 0: the lanes that differ below BIT already hold one value, so the mirrors
// of eight and sixteen lanes (partner 7 - i, 15 - i) reach a lane of the other half just as xor would
template <int BIT>
__device__ __forceinline__ double pair_min(double v) {
    double o;
    if constexpr (BIT == 0) o = dpp_mov<0xB1>(v);              // quad_perm [1, 0, 3, 2]
    else if constexpr (BIT == 1) o = dpp_mov<0x4E>(v);         // quad_perm [2, 3, 0, 1]
    else if constexpr (BIT == 2) o = dpp_mov<0x141>(v);        // row_half_mirror
    else if constexpr (BIT == 3) o = dpp_mov<0x140>(v);        // row_mirror
    else o = __shfl_xor(v, 1 << BIT);
    return o < v ? o : v;
}

template <int LGM, int LGS>
__global__ __launch_bounds__((1 << LGS) < 64 ? 64 : (1 << LGS)) void mlse_kernel(MlseArgs a) {
    constexpr int M = 1 << LGM, S = 1 << LGS, W = S < 64 ? 64 : S, R = W / S, L = LGS / LGM + 1, NW = W / 64;
    constexpr int TOP = LGS - LGM;                             // the newest symbol is s >> TOP; S / M = 1 << TOP = M^(L-2)
    constexpr int LW = LGS < 6 ? LGS : 6;                      // state bits that are lane bits of a wave
    extern __shared__ unsigned long long ml_dec_lds[];
    __shared__ __attribute__((aligned(16))) double abuf[2][W]; // the metrics a step starts from (forward: alpha, backward: beta)
    __shared__ double ztr[W], zti[W];                          // z[s'] of every row
    __shared__ double htr[R][L], hti[R][L], ctr[M], cti[M];
    __shared__ double ptab[2][R][M];                           // P_t[a] of the backward step
    constexpr int CB = TOP < LW ? TOP : LW, NG = S >> CB;       // Lambda is reduced over CB lane bits in registers, NG values per row are left
    __shared__ double lamtab[2][R][NG];
    __shared__ double redv[NW];
    __shared__ int reds[NW], badf[R];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int g = tid >> LGS, s = tid & (S - 1), gsh = lane - (S < 64 ? s : lane);      // gsh: the row's first bit in a ballot word
    const int n = a.n, n_y = a.n_y;
    const int newest = s >> TOP;
    const int64_t groups = (a.B + R - 1) / R;
    // the decision words: the workgroup's slab of the arena, or LDS (two address spaces, so two accesses behind a uniform branch: one
    // flat pointer would make every LDS wait a wait for the global accesses in flight as well)
    unsigned long long *const dec_g = a.dec_g ? a.dec_g + (size_t)blockIdx.x * (size_t)n * (LGM * NW) : nullptr;
    double *aslab = a.alpha_g ? a.alpha_g + (size_t)blockIdx.x * (size_t)n * W : nullptr;

    // xh of the first L-1 steps: the prefix over l <= t (t <= L-2) of the branch into sp
    auto masked = [&](int t, int sp, double &xr, double &xi) {
        xr = 0.0;
        xi = 0.0;
#pragma unroll
        for (int l = 0; l < L - 1; l++)
            if (l <= t) {
                const int sym = (sp >> (LGS - LGM * (l + 1))) & (M - 1);
                const double hr = htr[g][l], hi = hti[g][l], cr = ctr[sym], ci = cti[sym];
                xr = xr + (hr * cr - hi * ci);
                xi = xi + (hr * ci + hi * cr);
            }
    };

    for (int64_t blk = blockIdx.x; blk < groups; blk += gridDim.x) {
        const int64_t row = blk * R + g;
        const bool valid = row < a.B;
        const int64_t rc = valid ? row : 0;                    // the lanes of a row that does not exist work on row 0 and write nothing
        const double *y = a.y + rc * 2 * n_y;
        const double *hrow = a.h + (a.h_batched ? rc * 2 * L : 0);
        const double *pri = a.prior ? a.prior + rc * n * LGM : nullptr;
        __syncthreads();                                       // the previous group's tables have been read
        if (s < L) {
            htr[g][s] = hrow[2 * s];
            hti[g][s] = hrow[2 * s + 1];
        }
        if (tid < M) {
            ctr[tid] = a.cst[2 * tid];
            cti[tid] = a.cst[2 * tid + 1];
        }
        if (s == 0) badf[g] = 0;
        __syncthreads();
        bool bad = false;
        for (int i = s; i < 2 * n_y; i += S) bad |= not_finite(y[i]);
        for (int i = s; i < 2 * L; i += S) bad |= not_finite(hrow[i]);
        if (pri)
            for (int i = s; i < n * LGM; i += S) bad |= not_finite(pri[i]);
        double nv = 1.0;
        if (a.nv) {
            nv = a.nv[a.nv_batched ? rc : 0];
            bad |= not_finite(nv) || !(nv > 0.0);
        }
        if (bad) badf[g] = 1;

        // ---- z[s'] and w[old]
        double zr, zi;
        masked(L - 2, s, zr, zi);
        ztr[tid] = zr;
        zti[tid] = zi;
        const double hlr = htr[g][L - 1], hli = hti[g][L - 1];
        double wr[M], wi[M];
#pragma unroll
        for (int o = 0; o < M; o++) {
            wr[o] = hlr * ctr[o] - hli * cti[o];
            wi[o] = hlr * cti[o] + hli * ctr[o];
        }
        __syncthreads();
        bad = badf[g] != 0;

        // ---- forward: add-compare-select
        double al = 0.0;
        const int pb = (g << LGS) + ((s & ((1 << TOP) - 1)) << LGM);
        // y and the prior of step t + 1 are fetched during step t, by every lane (no load behind a divergent branch)
        double yr = y[0], yi = y[1], pl[LGM];
#pragma unroll
        for (int i = 0; i < LGM; i++) pl[i] = pri ? pri[i] : 0.0;
        for (int t = 0; t < n; t++) {
            double *ab = abuf[t & 1];
            ab[tid] = al;
            const int tn = t + 1 < n_y ? t + 1 : t, tp = t + 1 < n ? t + 1 : t;
            const double ynr = y[2 * tn], yni = y[2 * tn + 1];
            double pacc = 0.0, pln[LGM];
#pragma unroll
            for (int i = 0; i < LGM; i++) {
                pln[i] = pri ? pri[tp * LGM + i] : 0.0;
                pacc = ((newest >> (LGM - 1 - i)) & 1) ? pacc + pl[i] : pacc;
            }
            const double P = nv * pacc;
            __syncthreads();
            double ap[M];
            const double2 *ap2 = reinterpret_cast<const double2 *>(ab + pb);
#pragma unroll
            for (int o = 0; o < M; o += 2) {
                const double2 v = ap2[o >> 1];
                ap[o] = v.x;
                ap[o + 1] = v.y;
            }
            double best = 0.0;
            int sel = 0;
            if (t >= L - 1) {
#pragma unroll
                for (int o = 0; o < M; o++) {
                    const double xr = zr + wr[o], xi = zi + wi[o];
                    const double er = yr - xr, ei = yi - xi;
                    const double d = er * er + ei * ei;
                    const double c = ap[o] + d;
                    if (o == 0 || c < best) {
                        best = c;
                        sel = o;
                    }
                }
            } else {
                double xr, xi;
                masked(t, s, xr, xi);
                const double er = yr - xr, ei = yi - xi;
                const double d = er * er + ei * ei;
#pragma unroll
                for (int o = 0; o < M; o++) {
                    const double c = ap[o] + d;
                    if (o == 0 || c < best) {
                        best = c;
                        sel = o;
                    }
                }
            }
            al = best + P;
#pragma unroll
            for (int p = 0; p < LGM; p++) {
                const unsigned long long wd = __ballot((sel >> p) & 1);
                if (lane == 0) {
                    if (dec_g) dec_g[(t * LGM + p) * NW + wave] = wd;
                    else ml_dec_lds[(t * LGM + p) * NW + wave] = wd;
                }
            }
            if (aslab) aslab[(size_t)t * W + tid] = al;
            yr = ynr;
            yi = yni;
#pragma unroll
            for (int i = 0; i < LGM; i++) pl[i] = pln[i];
        }

        // ---- the tail: beta_n
        double be = 0.0;
        if (a.tail) {
#pragma unroll
            for (int j = 0; j < L - 1; j++) {
                double xr = 0.0, xi = 0.0;
#pragma unroll
                for (int l = j + 1; l <= L - 1; l++)
                    if (l <= n + j) {
                        const int sym = (s >> (LGS - LGM * (l - j))) & (M - 1);
                        const double hr = htr[g][l], hi = hti[g][l], cr = ctr[sym], ci = cti[sym];
                        xr = xr + (hr * cr - hi * ci);
                        xi = xi + (hr * ci + hi * cr);
                    }
                const double er = y[2 * (n + j)] - xr, ei = y[2 * (n + j) + 1] - xi;
                be = be + (er * er + ei * ei);
            }
        }

        // ---- s*: the first minimum of alpha_n + beta_n
        const double tot = al + be;
        double mn = tot;
#pragma unroll
        for (int b = 0; b < LW; b++) mn = xmin(mn, 1 << b);
        unsigned long long eq = __ballot(tot == mn) >> gsh;
        if (S < 64) eq &= (1ull << (S & 63)) - 1ull;
        int sstar = eq ? __ffsll((long long)eq) - 1 : 0;
        if (NW > 1) {
            if (lane == 0) {
                redv[wave] = mn;
                reds[wave] = wave * 64 + sstar;
            }
            __syncthreads();
            mn = redv[0];
            sstar = reds[0];
#pragma unroll
            for (int w = 1; w < NW; w++)
                if (redv[w] < mn) {
                    mn = redv[w];
                    sstar = reds[w];
                }
        }
        if (valid && s == 0 && a.metric) a.metric[row] = bad ? __builtin_nan("") : mn;

        // ---- traceback: every lane of a row walks the same path, lane i keeps the symbol of step tb0 + i
        if (a.indices || a.bits) {
            __syncthreads();                                   // the decision words of every wave are in place
            int st = sstar;
            // the walk over one segment, once per address space of the words
            auto walk = [&](auto dec_load, int tb0, int hi) {
                int mysym = 0;
                if constexpr (NW == 1) {
                    constexpr int U = LGM <= 2 ? 8 : 4;        // steps whose words are in flight together: their addresses are known
                    for (int tt = hi - 1; tt >= tb0; tt -= U) {
                        unsigned long long wd[U][LGM];
#pragma unroll
                        for (int u = 0; u < U; u++) {
                            const int at = tt - u >= tb0 ? tt - u : tb0;
#pragma unroll
                            for (int p = 0; p < LGM; p++) wd[u][p] = dec_load(at * LGM + p);
                        }
#pragma unroll
                        for (int u = 0; u < U; u++)
                            if (tt - u >= tb0) {
                                mysym = (tt - u - tb0 == s) ? (st >> TOP) : mysym;
                                int old = 0;
#pragma unroll
                                for (int p = 0; p < LGM; p++) old |= (int)((wd[u][p] >> (gsh + st)) & 1ull) << p;
                                st = ((st & ((1 << TOP) - 1)) << LGM) | old;
                            }
                    }
                } else {
                    for (int tt = hi - 1; tt >= tb0; tt--) {
                        mysym = (tt - tb0 == s) ? (st >> TOP) : mysym;
                        int old = 0;
#pragma unroll
                        for (int p = 0; p < LGM; p++) old |= (int)((dec_load((tt * LGM + p) * NW + (st >> 6)) >> (st & 63)) & 1ull) << p;
                        st = ((st & ((1 << TOP) - 1)) << LGM) | old;
                    }
                }
                return mysym;
            };
            for (int tb0 = ((n - 1) / S) * S; tb0 >= 0; tb0 -= S) {
                const int hi = n < tb0 + S ? n : tb0 + S;
                int mysym;
                if (dec_g) mysym = walk([&](int idx) { return dec_g[idx]; }, tb0, hi);
                else mysym = walk([&](int idx) { return ml_dec_lds[idx]; }, tb0, hi);
                if (valid && tb0 + s < n) {
                    const int sym = bad ? 0 : mysym;
                    if (a.indices) a.indices[row * n + tb0 + s] = sym;
                    if (a.bits) {
#pragma unroll
                        for (int i = 0; i < LGM; i++) a.bits[(row * n + tb0 + s) * LGM + i] = (uint8_t)((sym >> (LGM - 1 - i)) & 1);
                    }
                }
            }
        }

        // ---- backward: beta and the LLRs
        if (a.llr) {
            __syncthreads();                                   // abuf is free
            double bt = be;                                    // beta_{t+1} of this lane's state
            double anext = aslab[(size_t)(n - 1) * W + tid];
            const int old = s & (M - 1);
            const double wor = hlr * ctr[old] - hli * cti[old], woi = hlr * cti[old] + hli * ctr[old];
            // what step t reads from memory is fetched during step t + 1: its y, and on the lanes s < M its prior
            double ycr = y[2 * (n - 1)], yci = y[2 * (n - 1) + 1];
            double pcur[LGM];
#pragma unroll
            for (int i = 0; i < LGM; i++) pcur[i] = (pri && s < M) ? pri[(n - 1) * LGM + i] : 0.0;
            for (int t = n - 1; t >= 0; t--) {
                const double lam = anext + bt;
                double ynr = 0.0, yni = 0.0, pnx[LGM];
#pragma unroll
                for (int i = 0; i < LGM; i++) pnx[i] = 0.0;
                if (t > 0) {
                    anext = aslab[(size_t)(t - 1) * W + tid];
                    ynr = y[2 * (t - 1)];
                    yni = y[2 * (t - 1) + 1];
                    if (pri && s < M) {
#pragma unroll
                        for (int i = 0; i < LGM; i++) pnx[i] = pri[(t - 1) * LGM + i];
                    }
                }
                // Lambda's minimum over the CB state bits below the label that are lane bits; one lane per value hands it on
                double c = lam;
                if constexpr (CB > 0) c = pair_min<0>(c);
                if constexpr (CB > 1) c = pair_min<1>(c);
                if constexpr (CB > 2) c = pair_min<2>(c);
                if constexpr (CB > 3) c = pair_min<3>(c);
                if constexpr (CB > 4) c = pair_min<4>(c);
                if constexpr (CB > 5) c = pair_min<5>(c);
                if ((s & ((1 << CB) - 1)) == 0) lamtab[t & 1][g][s >> CB] = c;
                double *bb = abuf[t & 1];
                if (t > 0) {
                    bb[tid] = bt;
                    if (s < M) {
                        double pacc = 0.0;
#pragma unroll
                        for (int i = 0; i < LGM; i++)
                            if ((s >> (LGM - 1 - i)) & 1) pacc = pacc + pcur[i];
                        ptab[t & 1][g][s] = nv * pacc;
                    }
                }
                __syncthreads();
                if (s < LGM) {                                 // lane i of a row: label bit i, MSB first
                    double m0 = __builtin_huge_val(), m1 = __builtin_huge_val();
#pragma unroll
                    for (int k = 0; k < NG; k++) {
                        const double v = lamtab[t & 1][g][k];
                        const bool one = ((k >> (TOP - CB)) >> (LGM - 1 - s)) & 1;
                        m1 = (one && v < m1) ? v : m1;
                        m0 = (!one && v < m0) ? v : m0;
                    }
                    if (valid) a.llr[(row * n + t) * LGM + s] = bad ? __builtin_nan("") : (m1 - m0) / nv;
                }
                if (t == 0) break;
                // beta_t from beta_{t+1}
                double nb = 0.0;
#pragma unroll
                for (int q = 0; q < M; q++) {
                    const int sp = (q << TOP) | (s >> LGM), idx = (g << LGS) + sp;
                    double xr, xi;
                    if (t >= L - 1) {
                        xr = ztr[idx] + wor;
                        xi = zti[idx] + woi;
                    } else {
                        masked(t, sp, xr, xi);
                    }
                    const double er = ycr - xr, ei = yci - xi;
                    const double d = er * er + ei * ei;
                    const double cand = d + (ptab[t & 1][g][q] + bb[idx]);
                    nb = (q == 0 || cand < nb) ? cand : nb;
                }
                bt = nb;
                ycr = ynr;
                yci = yni;
#pragma unroll
                for (int i = 0; i < LGM; i++) pcur[i] = pnx[i];
            }
        }
    }
}

// the limits both entry points share; *lgm, *lgs: the kernel's class
int check_mlse(const cpx_modem *md, int64_t B, int64_t n, int L, bool have_nv, bool need_nv, bool any_output, int *lgm, int *lgs) {
    CPX_REQUIRE(md, CPX_EINVAL, "mlse: null pointer");
    CPX_REQUIRE(B >= 0, CPX_EINVAL, "mlse: B = %lld", (long long)B);
    CPX_REQUIRE(md->M >= 2 && md->M <= CPX_MLSE_MAX_M && (1 << md->nbits) == md->M, CPX_EINVAL,
                "mlse: a constellation of %d points, the limit is a power of two from 2 to %d", md->M, CPX_MLSE_MAX_M);
    CPX_REQUIRE(L >= 2, CPX_EINVAL, "mlse: L = %d taps, the limit is L >= 2", L);
    CPX_REQUIRE(L <= 9 && md->nbits * (L - 1) <= 8, CPX_EINVAL, "mlse: M = %d, L = %d, the limit is M^(L-1) <= %d states", md->M, L,
                CPX_MLSE_MAX_STATES);
    CPX_REQUIRE(n >= 1 && n <= CPX_MLSE_MAX_N, CPX_EINVAL, "mlse: n = %lld symbols, the limit is 1 <= n <= %d", (long long)n, CPX_MLSE_MAX_N);
    CPX_REQUIRE(any_output, CPX_EINVAL, "mlse: no output requested");
    CPX_REQUIRE(have_nv || !need_nv, CPX_EINVAL, "mlse: noise_var is required for the LLRs and with a prior");
    *lgm = md->nbits;
    *lgs = md->nbits * (L - 1);
    return CPX_OK;
}

template <int LGM, int LGS>
int launch(MlseArgs a, Scratch &sc, hipStream_t st) {
    constexpr int S = 1 << LGS, W = S < 64 ? 64 : S, R = W / S, NW = W / 64;
    const size_t dec_bytes = 8ull * LGM * NW * (size_t)a.n, alpha_bytes = a.llr ? 8ull * W * (size_t)a.n : 0;
    const bool dec_lds = dec_bytes <= MLSE_DEC_LDS_MAX;
    const unsigned lds = dec_lds ? (unsigned)dec_bytes : 0u;
    // workgroups that registers, LDS and wave slots let share a compute unit, cut down to what the slabs allow
    int per_cu = 0;
    CPX_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void *)mlse_kernel<LGM, LGS>, W, lds));
    CPX_REQUIRE(per_cu >= 1, CPX_EHIP, "mlse: the runtime's occupancy query gives no resident workgroup for %u bytes of LDS", lds);
    int64_t cap = (int64_t)device_cus() * per_cu;
    const size_t slab = (dec_lds ? 0 : dec_bytes) + alpha_bytes;
    if (slab && cap > (int64_t)(MLSE_SCRATCH_CAP / slab)) cap = (int64_t)(MLSE_SCRATCH_CAP / slab);
    const int64_t groups = (a.B + R - 1) / R;
    const unsigned grid = grid_of(groups, cap);
    a.dec_g = nullptr;
    a.alpha_g = nullptr;
    if (!dec_lds)
        if (int rc = sc.get(st, Slot::mlse_dec, (size_t)grid * dec_bytes, &a.dec_g)) return rc;
    if (a.llr)
        if (int rc = sc.get(st, Slot::mlse_alpha, (size_t)grid * alpha_bytes, &a.alpha_g)) return rc;
    hipLaunchKernelGGL((mlse_kernel<LGM, LGS>), dim3(grid), dim3(W), lds, st, a);
    CPX_HIP(hipGetLastError());
    note_kernel("mlse_kernel<%d,%d> rows=%d cap=%lld dec=%s soft=%d", LGM, LGS, R, (long long)cap, dec_lds ? "lds" : "arena", a.llr ? 1 : 0);
    return CPX_OK;
}

int dispatch(int lgm, int lgs, const MlseArgs &a, Scratch &sc, hipStream_t st) {
#define MLSE_CASE(m, s) \
    if (lgm == m && lgs == s) return launch<m, s>(a, sc, st);
    MLSE_CASE(1, 1) MLSE_CASE(1, 2) MLSE_CASE(1, 3) MLSE_CASE(1, 4) MLSE_CASE(1, 5) MLSE_CASE(1, 6) MLSE_CASE(1, 7) MLSE_CASE(1, 8)
    MLSE_CASE(2, 2) MLSE_CASE(2, 4) MLSE_CASE(2, 6) MLSE_CASE(2, 8)
    MLSE_CASE(3, 3) MLSE_CASE(3, 6)
    MLSE_CASE(4, 4) MLSE_CASE(4, 8)
#undef MLSE_CASE
    set_error("mlse: no kernel for M = %d, S = %d", 1 << lgm, 1 << lgs);
    return CPX_EINVAL;
}

}  // namespace

extern "C" {

int cpx_mlse_dev(const cpx_modem *md, const double *d_y, const double *d_h, int h_batched, int64_t B, int64_t n, int L, int tail,
                 const double *d_noise_var, int nv_batched, const double *d_prior, int32_t *d_indices, uint8_t *d_bits, double *d_metric,
                 double *d_llr, void *stream) {
    CPX_TRACE("cpx_mlse_dev");
    int lgm, lgs;
    if (int rc = check_mlse(md, B, n, L, d_noise_var != nullptr, d_llr || d_prior, d_indices || d_bits || d_metric || d_llr, &lgm, &lgs))
        return rc;
    if (B == 0) return CPX_OK;
    CPX_REQUIRE(d_y && d_h, CPX_EINVAL, "mlse: null pointer");
    if (int rcd = check_handle_device(md->device, "mlse")) return rcd;
    MlseArgs a{d_y, d_h, md->d_const, d_noise_var, d_prior, B, (int)n, (int)n + (tail ? L - 1 : 0), h_batched ? 1 : 0, nv_batched ? 1 : 0,
               tail ? 1 : 0, d_indices, d_bits, d_metric, d_llr, nullptr, nullptr};
    Scratch sc;
    return dispatch(lgm, lgs, a, sc, pick_stream(stream));
}

int cpx_mlse(const cpx_modem *md, const double *y, const double *h, int h_batched, int64_t B, int64_t n, int L, int tail,
             const double *noise_var, int nv_batched, const double *prior, int32_t *indices, uint8_t *bits, double *metric, double *llr) {
    CPX_TRACE("cpx_mlse");
    int lgm, lgs;
    if (int rc = check_mlse(md, B, n, L, noise_var != nullptr, llr || prior, indices || bits || metric || llr, &lgm, &lgs)) return rc;
    if (B == 0) return CPX_OK;
    CPX_REQUIRE(y && h, CPX_EINVAL, "mlse: null pointer");
    int rc = ensure_device();
    if (rc) return rc;
    const size_t b = (size_t)B, nm = (size_t)n * (size_t)md->nbits, n_y = (size_t)n + (tail ? (size_t)L - 1 : 0);
    HostStage::Out outs[4] = {{indices, 4 * b * (size_t)n}, {bits, b * nm}, {metric, 8 * b}, {llr, 8 * b * nm}};
    HostStage s;
    const double *dy, *dh, *dnv = nullptr, *dpr = nullptr;
    if ((rc = s.in(y, 16 * b * n_y, &dy)) || (rc = s.in(h, 16 * (size_t)L * (h_batched ? b : 1), &dh))) return rc;
    if (noise_var && (rc = s.in(noise_var, 8 * (nv_batched ? b : 1), &dnv))) return rc;
    if (prior && (rc = s.in(prior, 8 * b * nm, &dpr))) return rc;
    if ((rc = s.out(outs))) return rc;
    if ((rc = cpx_mlse_dev(md, dy, dh, h_batched, B, n, L, tail, dnv, nv_batched, dpr, outs[0].as<int32_t>(), outs[1].as<uint8_t>(),
                           outs[2].as<double>(), outs[3].as<double>(), s.st)))
        return rc;
    return s.get(outs);
}

}  // extern "C"
