// Linear MIMO detection: zero-forcing and MMSE equalisation followed by per-stream slicing (hard) or per-stream max-log LLRs
// (soft).  Not in the reference; DESIGN.md 4.12.  float64 throughout, -ffp-contract=off, no precision mode, no path switch: nt picks
// the kernel.
//
// Per received vector, with the modem's m = 2^nb points, a regulariser reg >= 0 and an LLR scale noise_var:
//   A = H^H H + reg I  (Hermitian nt x nt, lower triangle only, real diagonal),  b = H^H y      summed over the rows of H, r ascending
//   A = L L^H (Cholesky),  M = L^-1,  z = M^H (M b) = A^-1 b,  a_i = (A^-1)_ii = sum_{j >= i} |M_ji|^2
//   g_i = 1 - reg a_i,  xhat_i = z_i / g_i (unbiased),  nu_i = noise_var a_i / g_i
//   reg = 0: zero forcing (xhat = H^+ y, nu_i = noise_var a_i);  reg = N0 / Es: unbiased MMSE.  One kernel, only reg differs.
//   hard  idx[i]        = first minimum of |xhat_i - s|^2 over the points in index order (strict <, from index 0: ties to the lowest
//                         index, a NaN estimate to index 0)
//   soft  llr[i nb + k] = (min_{s: bit k = 1} |xhat_i - s|^2 - min_{s: bit k = 0} |xhat_i - s|^2) / (2 nu_i), bit k of a point = bit
//                         k of its index, MSB first (the modem's labels); positive: bit 0; the factor 2 is cpx_kbest_soft's
// A vector fails when a Cholesky pivot is not a positive finite number (singular H under ZF, nt > nr with reg = 0, NaN / inf in H),
// when a component of b is not finite (NaN / inf in y) or when some g_i is not positive.  "Positive" is taken in float64's terms: the
// pivot of column j must exceed 4 (nr + nt) 2^-52 A_jj, because rounding leaves an exactly singular A a pivot of either sign of that
// order, and such a vector has to fail wherever and however it is summed.  Of a failed vector all its xhat, nu and LLRs are then NaN and
// its indices 0.  No vector reads another vector's data, and every vector goes through the same operations in the same order
// whatever the batch size, its position in the batch, the stream, and whether H is shared or one per vector: outputs are bit-identical
// across all of those.
//
// mimo_linear_kernel<NT>  (nt = 1..8)  ONE VECTOR PER LANE, 64 vectors per workgroup.  A (lower triangle), b and then L^-1 -- written
//   over L in place, the diagonal holding 1 / L_ii from the factorisation on -- are fully unrolled register arrays; nr is a run-time
//   loop.  The workgroup's tile of H and y is contiguous in memory (lane l's H starts nr nt 16 bytes after lane l - 1's): it is staged
//   through LDS by coalesced loads, R rows of every vector at a time (R chosen by the host so that the stage stays near 20 KB), each
//   vector's rows at an odd 16-byte stride so that the per-lane ds_read_b128 spread over the banks.  A shared H is staged once per
//   workgroup and read by every lane at the same address (broadcast).  Outputs go back the same way: per-lane values into LDS at an odd
//   stride, then one contiguous run per workgroup.
// mimo_linear_wave_kernel (nt >= 9)    one wave per vector, as the other MIMO kernels: H, y, A / L, M and the vectors in LDS, lanes
//   across the entries of A, the rows of a Cholesky column, the columns of M, the streams and the LLRs.  CPX_ELIMIT above 64 KB.
// Both walk the constellation from an LDS copy of md->d_const made once per workgroup, take 64-bit offsets and grid-stride over the
// batch.
#include "cpx_internal.h"

#include <cmath>

using namespace cpx;

namespace {

constexpr int WAVE = 64;
constexpr size_t LDS_MAX = 64 * 1024;      // dynamic LDS budget of one workgroup
constexpr int REG_MAX_NT = 8;              // streams the one-vector-per-lane kernel is instantiated for
constexpr int STAGE_ENTRIES = 20;          // R (nt + 1) complex entries of a vector staged at a time: 64 * 20 * 16 B = 20 KB
constexpr int REG_MAX_GRID = 2048;         // workgroups of a launch: 8 per CU, what the stage's LDS lets be resident
constexpr int WAVE_MAX_GRID = 4096;

__device__ __forceinline__ double abs2(double2 a) { return a.x * a.x + a.y * a.y; }
__device__ __forceinline__ bool is_fin(double v) { return fabs(v) < INFINITY; }   // false for NaN

// element e = lane, lane + 64, ... of `count` runs of `run` items: (v, k) = (e / run, e % run) kept by increments
struct RunWalk {
    int v, k, dv, dk, run;
    __device__ __forceinline__ RunWalk(int lane, int run_) : v(lane / run_), k(lane % run_), dv(WAVE / run_), dk(WAVE % run_), run(run_) {}
    __device__ __forceinline__ void next() {
        v += dv;
        k += dk;
        if (k >= run) { k -= run; v++; }
    }
};

// global -> LDS: `count` runs of `run` items, run v at src + v * src_stride and dst + v * dst_stride
template <class T>
__device__ __forceinline__ void stage_in(T *dst, int dst_stride, const T *__restrict__ src, int64_t src_stride, int run, int count,
                                         int lane) {
    RunWalk w(lane, run);
    for (int e = lane; e < count * run; e += WAVE, w.next()) dst[w.v * dst_stride + w.k] = src[w.v * src_stride + w.k];
}

// LDS -> global: the `count` runs of `run` items at src + v * src_stride become one contiguous run at dst
template <class T>
__device__ __forceinline__ void flush_out(T *__restrict__ dst, const T *src, int src_stride, int run, int count, int lane) {
    RunWalk w(lane, run);
    for (int e = lane; e < count * run; e += WAVE, w.next()) dst[e] = src[w.v * src_stride + w.k];
}

// first minimum of |x - s|^2 over the points, strict <
__device__ __forceinline__ int slice_hard(double xr, double xi, const double2 *sc, int m) {
    int bi = 0;
    double best = 0.0;
    for (int s = 0; s < m; s++) {
        const double2 p = sc[s];
        const double dx = xr - p.x, dy = xi - p.y, d = dx * dx + dy * dy;
        if (s == 0 || d < best) { best = d; bi = s; }
    }
    return bi;
}

// (min over the points with bit `sh` of the index set) - (min over the others), over 2 nu
__device__ __forceinline__ double slice_llr(double xr, double xi, double nu, const double2 *sc, int m, int sh) {
    double mn0 = INFINITY, mn1 = INFINITY;
    for (int s = 0; s < m; s++) {
        const double2 p = sc[s];
        const double dx = xr - p.x, dy = xi - p.y, d = dx * dx + dy * dy;
        if ((s >> sh) & 1) mn1 = d < mn1 ? d : mn1;
        else mn0 = d < mn0 ? d : mn0;
    }
    return (mn1 - mn0) / (2.0 * nu);
}

// LDS, in 16-byte units: sc [m] | stage: H (64 vectors at stride hstr, or one shared copy) then y (64 at stride ystr); the output
// runs reuse the stage
template <int NT>
__global__ __launch_bounds__(WAVE) void mimo_linear_kernel(const double2 *__restrict__ y, const double2 *__restrict__ H, int h_batched,
                                                           int64_t B, int nr, int R, const double2 *__restrict__ c, int m, int nbits,
                                                           double reg, double noise_var, double pivot_tol,
                                                           int32_t *__restrict__ out_idx, double *__restrict__ out_llr, double *__restrict__ out_xhat,
                                                           double *__restrict__ out_nu) {
    extern __shared__ double2 lds_lin[];
    const int lane = threadIdx.x;
    double2 *sc = lds_lin, *sH = sc + m;
    const int hstr = h_batched ? ((R * NT) | 1) : 0, ystr = R | 1;
    double2 *sy = sH + (h_batched ? WAVE * hstr : R * NT);
    double *so = reinterpret_cast<double *>(sH);
    int32_t *so32 = reinterpret_cast<int32_t *>(sH);
    for (int i = lane; i < m; i += WAVE) sc[i] = c[i];
    const int64_t hvec = int64_t(nr) * NT;
    for (int64_t t0 = int64_t(blockIdx.x) * WAVE; t0 < B; t0 += int64_t(gridDim.x) * WAVE) {
        const int nv = int(B - t0 < WAVE ? B - t0 : WAVE);
        double Ar[NT][NT], Ai[NT][NT];     // lower triangle; Ai's diagonal is not used
        double2 bv[NT];
#pragma unroll
        for (int i = 0; i < NT; i++) {
            bv[i] = make_double2(0.0, 0.0);
#pragma unroll
            for (int j = 0; j <= i; j++) Ar[i][j] = Ai[i][j] = 0.0;
        }
        for (int r0 = 0; r0 < nr; r0 += R) {
            const int rc = nr - r0 < R ? nr - r0 : R;
            __syncthreads();               // the previous readers of the stage are done
            if (h_batched) stage_in(sH, hstr, H + t0 * hvec + int64_t(r0) * NT, hvec, rc * NT, nv, lane);
            else stage_in(sH, 0, H + int64_t(r0) * NT, 0, rc * NT, 1, lane);
            stage_in(sy, ystr, y + t0 * nr + r0, int64_t(nr), rc, nv, lane);
            __syncthreads();
            const double2 *myH = sH + lane * hstr, *myy = sy + lane * ystr;
            for (int r = 0; r < rc; r++) {
                double2 h[NT];
#pragma unroll
                for (int i = 0; i < NT; i++) h[i] = myH[r * NT + i];
                const double2 yv = myy[r];
#pragma unroll
                for (int i = 0; i < NT; i++) {       // conj(h_i) y, conj(h_i) h_j
                    bv[i].x += h[i].x * yv.x + h[i].y * yv.y;
                    bv[i].y += h[i].x * yv.y - h[i].y * yv.x;
#pragma unroll
                    for (int j = 0; j < i; j++) {
                        Ar[i][j] += h[i].x * h[j].x + h[i].y * h[j].y;
                        Ai[i][j] += h[i].x * h[j].y - h[i].y * h[j].x;
                    }
                    Ar[i][i] += h[i].x * h[i].x + h[i].y * h[i].y;
                }
            }
        }
        bool bad = false;
#pragma unroll
        for (int i = 0; i < NT; i++) {
            Ar[i][i] += reg;
            bad |= !(is_fin(bv[i].x) && is_fin(bv[i].y));
        }
        // Cholesky in place: L below the diagonal, 1 / L_jj on it
#pragma unroll
        for (int j = 0; j < NT; j++) {
            const double ajj = Ar[j][j];
            double p = ajj;
#pragma unroll
            for (int k = 0; k < j; k++) p -= Ar[j][k] * Ar[j][k] + Ai[j][k] * Ai[j][k];
            bad |= !(p > pivot_tol * ajj && p < INFINITY);
            const double inv = 1.0 / sqrt(p);
            Ar[j][j] = inv;
#pragma unroll
            for (int i = j + 1; i < NT; i++) {
                double sr = Ar[i][j], si = Ai[i][j];
#pragma unroll
                for (int k = 0; k < j; k++) {        // L_ik conj(L_jk)
                    sr -= Ar[i][k] * Ar[j][k] + Ai[i][k] * Ai[j][k];
                    si -= Ai[i][k] * Ar[j][k] - Ar[i][k] * Ai[j][k];
                }
                Ar[i][j] = sr * inv;
                Ai[i][j] = si * inv;
            }
        }
        // M = L^-1 over L, column after column: column j reads L's columns j.. only, which are still L
#pragma unroll
        for (int j = 0; j < NT; j++) {
#pragma unroll
            for (int i = j + 1; i < NT; i++) {
                double sr = Ar[i][j] * Ar[j][j], si = Ai[i][j] * Ar[j][j];
#pragma unroll
                for (int k = j + 1; k < i; k++) {    // L_ik M_kj
                    sr += Ar[i][k] * Ar[k][j] - Ai[i][k] * Ai[k][j];
                    si += Ar[i][k] * Ai[k][j] + Ai[i][k] * Ar[k][j];
                }
                Ar[i][j] = -sr * Ar[i][i];
                Ai[i][j] = -si * Ar[i][i];
            }
        }
        double2 w[NT];
#pragma unroll
        for (int i = 0; i < NT; i++) {               // w = M b
            double sr = 0.0, si = 0.0;
#pragma unroll
            for (int j = 0; j < i; j++) {
                sr += Ar[i][j] * bv[j].x - Ai[i][j] * bv[j].y;
                si += Ar[i][j] * bv[j].y + Ai[i][j] * bv[j].x;
            }
            w[i] = make_double2(sr + Ar[i][i] * bv[i].x, si + Ar[i][i] * bv[i].y);
        }
        double xr[NT], xi[NT], nu[NT];
#pragma unroll
        for (int i = 0; i < NT; i++) {               // z = M^H w, a = the squared norm of M's column i
            double sr = Ar[i][i] * w[i].x, si = Ar[i][i] * w[i].y, a = Ar[i][i] * Ar[i][i];
#pragma unroll
            for (int j = i + 1; j < NT; j++) {       // conj(M_ji) w_j
                sr += Ar[j][i] * w[j].x + Ai[j][i] * w[j].y;
                si += Ar[j][i] * w[j].y - Ai[j][i] * w[j].x;
                a += Ar[j][i] * Ar[j][i] + Ai[j][i] * Ai[j][i];
            }
            const double g = 1.0 - reg * a;
            bad |= !(g > 0.0);
            xr[i] = sr / g;
            xi[i] = si / g;
            nu[i] = noise_var * a / g;
        }
        if (bad) {
#pragma unroll
            for (int i = 0; i < NT; i++) xr[i] = xi[i] = nu[i] = NAN;
        }
        if (out_xhat) {
            const int n = 2 * NT, str = n | 1;
            __syncthreads();
#pragma unroll
            for (int i = 0; i < NT; i++) { so[lane * str + 2 * i] = xr[i]; so[lane * str + 2 * i + 1] = xi[i]; }
            __syncthreads();
            flush_out(out_xhat + t0 * n, so, str, n, nv, lane);
        }
        if (out_nu) {
            const int str = NT | 1;
            __syncthreads();
#pragma unroll
            for (int i = 0; i < NT; i++) so[lane * str + i] = nu[i];
            __syncthreads();
            flush_out(out_nu + t0 * NT, so, str, NT, nv, lane);
        }
        if (out_idx) {
            const int str = NT | 1;
            __syncthreads();
#pragma unroll
            for (int i = 0; i < NT; i++) so32[lane * str + i] = bad ? 0 : slice_hard(xr[i], xi[i], sc, m);
            __syncthreads();
            flush_out(out_idx + t0 * NT, so32, str, NT, nv, lane);
        }
        if (out_llr) {
            const int n = NT * nbits, str = n | 1;
            __syncthreads();
#pragma unroll
            for (int i = 0; i < NT; i++)
                for (int k = 0; k < nbits; k++)
                    so[lane * str + i * nbits + k] = bad ? NAN : slice_llr(xr[i], xi[i], nu[i], sc, m, nbits - 1 - k);
            __syncthreads();
            flush_out(out_llr + t0 * n, so, str, n, nv, lane);
        }
    }
}

// a pivot at or below this share of its diagonal entry is rounding noise: 4 (nr + nt) 2^-52, four times the bound on what the sums of
// the Gram matrix and of the factorisation leave of an exactly singular matrix's pivot
double pivot_tolerance(int nr, int nt) { return 4.0 * (double(nr) + double(nt)) * 0x1p-52; }

// bytes of dynamic LDS of the one-vector-per-lane kernel: the constellation, then the larger of the stage and the widest output run
size_t reg_lds_bytes(int nt, int R, int m, int nbits, int h_batched) {
    const size_t stage = 16 * (h_batched ? size_t(WAVE) * ((R * nt) | 1) : size_t(R) * nt) + 16 * size_t(WAVE) * (R | 1);
    const size_t outs = 8 * size_t(WAVE) * size_t((nt * (nbits > 2 ? nbits : 2)) | 1);
    return 16 * size_t(m) + (stage > outs ? stage : outs);
}

struct WaveLayout {   // offsets in 16-byte units, then in 8-byte units from `dbl`
    int H, y, A, M, b, w, x, dbl, dinv, nu, units;
};

WaveLayout wave_layout(int nr, int nt, int m) {
    WaveLayout L;
    int64_t o = m;
    auto take = [&](int64_t n) { int64_t r = o; o += n; return int(r < INT32_MAX ? r : INT32_MAX); };
    L.H = take(int64_t(nr) * nt);
    L.y = take(nr);
    L.A = take(int64_t(nt) * nt);
    L.M = take(int64_t(nt) * nt);
    L.b = take(nt);
    L.w = take(nt);
    L.x = take(nt);
    L.dbl = take(nt);          // two arrays of nt doubles
    L.dinv = 0;
    L.nu = nt;
    L.units = int(o < INT32_MAX ? o : INT32_MAX);
    return L;
}

__global__ __launch_bounds__(WAVE) void mimo_linear_wave_kernel(const double2 *__restrict__ y, const double2 *__restrict__ H,
                                                                int64_t hstride, int64_t B, int nr, int nt, const double2 *__restrict__ c,
                                                                int m, int nbits, double reg, double noise_var, double pivot_tol,
                                                                WaveLayout L,
                                                                int32_t *__restrict__ out_idx, double *__restrict__ out_llr,
                                                                double2 *__restrict__ out_xhat, double *__restrict__ out_nu) {
    extern __shared__ double2 lds_lw[];
    const int lane = threadIdx.x;
    double2 *sc = lds_lw, *sH = lds_lw + L.H, *sy = lds_lw + L.y, *A = lds_lw + L.A, *M = lds_lw + L.M, *sb = lds_lw + L.b,
            *sw = lds_lw + L.w, *sx = lds_lw + L.x;
    double *dinv = reinterpret_cast<double *>(lds_lw + L.dbl) + L.dinv, *snu = reinterpret_cast<double *>(lds_lw + L.dbl) + L.nu;
    for (int i = lane; i < m; i += WAVE) sc[i] = c[i];
    for (int64_t b = blockIdx.x; b < B; b += gridDim.x) {
        const double2 *Hb = H + b * hstride, *yb = y + b * nr;
        __syncthreads();
        for (int i = lane; i < nr * nt; i += WAVE) sH[i] = Hb[i];
        for (int i = lane; i < nr; i += WAVE) sy[i] = yb[i];
        __syncthreads();
        for (int e = lane; e < nt * nt; e += WAVE) {             // the lower triangle of H^H H + reg I
            const int i = e / nt, j = e - i * nt;
            if (j > i) continue;
            double sr = 0.0, si = 0.0;
            for (int r = 0; r < nr; r++) {
                const double2 hi = sH[r * nt + i], hj = sH[r * nt + j];
                sr += hi.x * hj.x + hi.y * hj.y;
                si += hi.x * hj.y - hi.y * hj.x;
            }
            A[e] = make_double2(i == j ? sr + reg : sr, si);
        }
        bool lane_bad = false;
        for (int i = lane; i < nt; i += WAVE) {
            double sr = 0.0, si = 0.0;
            for (int r = 0; r < nr; r++) {
                const double2 hi = sH[r * nt + i], yv = sy[r];
                sr += hi.x * yv.x + hi.y * yv.y;
                si += hi.x * yv.y - hi.y * yv.x;
            }
            sb[i] = make_double2(sr, si);
            lane_bad |= !(is_fin(sr) && is_fin(si));
        }
        __syncthreads();
        bool ok = true;
        for (int j = 0; j < nt; j++) {                           // left-looking Cholesky, lanes over the rows of column j
            const double ajj = A[j * nt + j].x;
            double p = ajj;
            for (int k = 0; k < j; k++) p -= abs2(A[j * nt + k]);
            ok &= p > pivot_tol * ajj && p < INFINITY;
            const double inv = 1.0 / sqrt(p);
            for (int i = j + 1 + lane; i < nt; i += WAVE) {
                double2 s = A[i * nt + j];
                for (int k = 0; k < j; k++) {
                    const double2 lik = A[i * nt + k], ljk = A[j * nt + k];
                    s.x -= lik.x * ljk.x + lik.y * ljk.y;
                    s.y -= lik.y * ljk.x - lik.x * ljk.y;
                }
                A[i * nt + j] = make_double2(s.x * inv, s.y * inv);
            }
            if (lane == 0) dinv[j] = inv;
            __syncthreads();
        }
        for (int j = lane; j < nt; j += WAVE) {                  // M = L^-1, one column per lane
            M[j * nt + j] = make_double2(dinv[j], 0.0);
            for (int i = j + 1; i < nt; i++) {
                const double2 lij = A[i * nt + j];
                double sr = lij.x * dinv[j], si = lij.y * dinv[j];
                for (int k = j + 1; k < i; k++) {
                    const double2 lik = A[i * nt + k], mkj = M[k * nt + j];
                    sr += lik.x * mkj.x - lik.y * mkj.y;
                    si += lik.x * mkj.y + lik.y * mkj.x;
                }
                M[i * nt + j] = make_double2(-sr * dinv[i], -si * dinv[i]);
            }
        }
        __syncthreads();
        for (int i = lane; i < nt; i += WAVE) {                  // w = M b
            double sr = 0.0, si = 0.0;
            for (int j = 0; j <= i; j++) {
                const double2 mij = M[i * nt + j], bj = sb[j];
                sr += mij.x * bj.x - mij.y * bj.y;
                si += mij.x * bj.y + mij.y * bj.x;
            }
            sw[i] = make_double2(sr, si);
        }
        __syncthreads();
        for (int i = lane; i < nt; i += WAVE) {                  // z = M^H w, a, the unbiased estimate and its noise
            double sr = 0.0, si = 0.0, a = 0.0;
            for (int j = i; j < nt; j++) {
                const double2 mji = M[j * nt + i], wj = sw[j];
                sr += mji.x * wj.x + mji.y * wj.y;
                si += mji.x * wj.y - mji.y * wj.x;
                a += abs2(mji);
            }
            const double g = 1.0 - reg * a;
            lane_bad |= !(g > 0.0);
            sx[i] = make_double2(sr / g, si / g);
            snu[i] = noise_var * a / g;
        }
        const bool bad = !ok || __any(lane_bad);
        __syncthreads();
        for (int i = lane; i < nt; i += WAVE) {
            const double2 x = sx[i];
            if (out_xhat) out_xhat[b * nt + i] = bad ? make_double2(NAN, NAN) : x;
            if (out_nu) out_nu[b * nt + i] = bad ? NAN : snu[i];
            if (out_idx) out_idx[b * nt + i] = bad ? 0 : slice_hard(x.x, x.y, sc, m);
        }
        if (out_llr) {
            const int nbt = nt * nbits;
            for (int e = lane; e < nbt; e += WAVE) {
                const int i = e / nbits, k = e - i * nbits;
                out_llr[b * nbt + e] = bad ? NAN : slice_llr(sx[i].x, sx[i].y, snu[i], sc, m, nbits - 1 - k);
            }
        }
    }
}

template <int NT>
void launch_reg(int grid, size_t lds, hipStream_t st, const double2 *y, const double2 *H, int h_batched, int64_t B, int nr, int R,
                const double2 *c, int m, int nbits, double reg, double noise_var, double tol, int32_t *idx, double *llr, double *xhat,
                double *nu) {
    hipLaunchKernelGGL(mimo_linear_kernel<NT>, dim3(grid), dim3(WAVE), lds, st, y, H, h_batched, B, nr, R, c, m, nbits, reg, noise_var,
                       tol, idx, llr, xhat, nu);
}

}  // namespace

extern "C" {

int cpx_mimo_linear_dev(const cpx_modem *md, const double *d_y, const double *d_h, int h_batched, int64_t B, int nr, int nt, double reg,
                        double noise_var, int32_t *d_idx, double *d_llr, double *d_xhat, double *d_nu, void *stream) {
    CPX_TRACE("cpx_mimo_linear_dev");
    const char *what = "mimo_linear";
    CPX_REQUIRE(reg >= 0.0, CPX_EINVAL, "%s: reg must be zero or positive (got %g)", what, reg);          // NaN fails the comparison
    CPX_REQUIRE(noise_var == noise_var, CPX_EINVAL, "%s: noise_var is NaN", what);
    CPX_REQUIRE(d_idx || d_llr || d_xhat || d_nu, CPX_EINVAL, "%s: no output requested", what);
    if (int rc = mimo_check(md, B, nr, nt, what)) return rc;
    const int m = md->M, nbits = md->nbits;
    CPX_REQUIRE(m == 1 << nbits, CPX_EINVAL, "%s: the modem does not have 2^nbits points", what);
    if (B == 0) return CPX_OK;
    CPX_REQUIRE(d_y && d_h, CPX_EINVAL, "%s: null pointer", what);
    hipStream_t st = pick_stream(stream);
    const double2 *y = reinterpret_cast<const double2 *>(d_y), *H = reinterpret_cast<const double2 *>(d_h);
    const double2 *c = reinterpret_cast<const double2 *>(md->d_const);
    h_batched = h_batched != 0;
    const double tol = pivot_tolerance(nr, nt);
    if (nt <= REG_MAX_NT) {
        int R = STAGE_ENTRIES / (nt + 1);
        R = R < 1 ? 1 : (R > nr ? nr : R);
        const size_t lds = reg_lds_bytes(nt, R, m, nbits, h_batched);
        CPX_REQUIRE(lds <= LDS_MAX, CPX_ELIMIT, "%s: %d points of %d bits exceed the kernel's LDS (%zu of %zu bytes)", what, m, nbits, lds,
                    LDS_MAX);
        const int64_t tiles = (B + WAVE - 1) / WAVE;
        const int grid = int(tiles < REG_MAX_GRID ? tiles : REG_MAX_GRID);
        switch (nt) {
#define CPX_LIN_CASE(N) \
    case N: launch_reg<N>(grid, lds, st, y, H, h_batched, B, nr, R, c, m, nbits, reg, noise_var, tol, d_idx, d_llr, d_xhat, d_nu); break;
            CPX_LIN_CASE(1) CPX_LIN_CASE(2) CPX_LIN_CASE(3) CPX_LIN_CASE(4) CPX_LIN_CASE(5) CPX_LIN_CASE(6) CPX_LIN_CASE(7) CPX_LIN_CASE(8)
#undef CPX_LIN_CASE
        }
        CPX_HIP(hipGetLastError());
        note_kernel("mimo_linear_kernel<%d> (m %d, %dx%d, %s H, %d rows staged)", nt, m, nr, nt, h_batched ? "own" : "shared", R);
        return CPX_OK;
    }
    const WaveLayout L = wave_layout(nr, nt, m);
    const size_t lds = 16 * size_t(L.units);
    CPX_REQUIRE(lds <= LDS_MAX, CPX_ELIMIT, "%s: the state of one %dx%d vector exceeds the kernel's LDS (%zu of %zu bytes)", what, nr, nt,
                lds, LDS_MAX);
    hipLaunchKernelGGL(mimo_linear_wave_kernel, dim3(int(B < WAVE_MAX_GRID ? B : WAVE_MAX_GRID)), dim3(WAVE), lds, st, y, H,
                       h_batched ? int64_t(nr) * nt : int64_t(0), B, nr, nt, c, m, nbits, reg, noise_var, tol, L, d_idx, d_llr,
                       reinterpret_cast<double2 *>(d_xhat), d_nu);
    CPX_HIP(hipGetLastError());
    note_kernel("mimo_linear_wave_kernel (m %d, %dx%d, %zu B per vector)", m, nr, nt, lds);
    return CPX_OK;
}

int cpx_mimo_linear(const cpx_modem *md, const double *y, const double *h, int h_batched, int64_t B, int nr, int nt, double reg,
                    double noise_var, int32_t *idx, double *llr, double *xhat, double *nu) {
    CPX_TRACE("cpx_mimo_linear");
    const char *what = "mimo_linear";
    CPX_REQUIRE(reg >= 0.0, CPX_EINVAL, "%s: reg must be zero or positive (got %g)", what, reg);
    CPX_REQUIRE(noise_var == noise_var, CPX_EINVAL, "%s: noise_var is NaN", what);
    CPX_REQUIRE(idx || llr || xhat || nu, CPX_EINVAL, "%s: no output requested", what);
    const void *some = idx ? static_cast<const void *>(idx) : llr ? static_cast<const void *>(llr) : xhat ? static_cast<const void *>(xhat) : nu;
    if (int rc = mimo_host_check(y, h, B, nr, nt, some)) return rc;
    HostStage s;
    const double *dy, *dh;
    int32_t *d_idx = nullptr;
    double *d_llr = nullptr, *d_xhat = nullptr, *d_nu = nullptr;
    const size_t V = size_t(B) * nt, n_llr = 8 * V * (md ? size_t(md->nbits) : 0);
    int rc;
    if ((rc = mimo_in(s, y, h, h_batched, B, nr, nt, &dy, &dh)) || (idx && (rc = s.out(4 * V, &d_idx))) ||
        (llr && (rc = s.out(n_llr, &d_llr))) || (xhat && (rc = s.out(16 * V, &d_xhat))) || (nu && (rc = s.out(8 * V, &d_nu))) ||
        (rc = cpx_mimo_linear_dev(md, dy, dh, h_batched, B, nr, nt, reg, noise_var, d_idx, d_llr, d_xhat, d_nu, s.st)) ||
        (idx && (rc = s.get(idx, d_idx, 4 * V))) || (llr && (rc = s.get(llr, d_llr, n_llr))) ||
        (xhat && (rc = s.get(xhat, d_xhat, 16 * V))) || (nu && (rc = s.get(nu, d_nu, 8 * V))))
        return rc;
    return CPX_OK;
}

}  // extern "C"
