// Symbol-timing and carrier recovery of a matched-filtered single-carrier burst: the interpolator / timing-error detector / loop filter /
// controller loop, with an optional decision-directed carrier PLL on the strobes, fused in one kernel; one row = one independent loop.
// y holds nominally sps samples per symbol (2 <= sps <= 8); c is the constellation of a cpx_modem (label = position), optional.
//
// The rule (float64, real and imaginary parts separate doubles, every product rounded before it is added, -ffp-contract=off; a sample
// index outside [0, n_y) reads 0.0 and is used like any other sample).  Per-row state: the sampling position m (int64) and mu, from m0
// and mu0; the timing integrator v = 0.0; the period w = (double)sps; the carrier phase phi = phase0 and its integrator f = 0.0; the
// previous strobe and the previous reference.  For k = 0 .. n-1:
//   interpolate   z_k = I(m, mu), each part on its own.  'linear': x0 + mu (x1 - x0) with x0 = y[m], x1 = y[m+1].  'cubic' (4-sample
//                 Lagrange in Farrow form), with xm = y[m-1], x0 = y[m], x1 = y[m+1], x2 = y[m+2] and S = 0.16666666666666666 (the
//                 double nearest 1/6; the divisions are multiplications by S and by 0.5):
//                     v3 = ((x2 - xm) + 3.0 (x0 - x1)) S
//                     v2 = ((x1 + xm) 0.5) - x0
//                     v1 = ((6.0 x1 - x2) - (3.0 x0 + 2.0 xm)) S
//                     I  = ((v3 mu + v2) mu + v1) mu + x0
//   derotate      with a carrier loop (c, s) = unit_phasor(phi) (cpx_phasor.h) and z'_k = (zr c + zi s, zi c - zr s); without: z' = z.
//   decide        with a constellation, a^_k = the first minimum over a ascending of e = z'_k - c[a], er er + ei ei, a later point
//                 winning only if strictly smaller (cpx_slice.h).  Reference r_k = c[training[k]] for k < nt, else c[a^_k].
//   timing error  e_0 = 0.0 and no midpoint is read at k = 0.  'gardner': t = mu - 0.5 w, fl = floor(t), zm = I(m + fl, t - fl),
//                 e_k = (zr_{k-1} - zr_k) zmr + (zi_{k-1} - zi_k) zmi on the UNrotated strobes (the detector is blind to phase).
//                 'mm': e_k = (rr_{k-1} z'r_k + ri_{k-1} z'i_k) - (rr_k z'r_{k-1} + ri_k z'i_{k-1}).
//   carrier       ep = z'i_k rr_k - z'r_k ri_k; f <- f + kc2 ep; phi <- phi + (f + kc1 ep); phi <- phi - rint(phi).  The row is
//                 rejected unless |phi| <= 0.5 (a NaN fails).
//   loop filter   v <- v + k2 e_k; w = sps + (v + k1 e_k).  The row is rejected unless 0.5 sps < w < 1.5 sps.
//   controller    t = mu + w, fl = floor(t), m <- m + fl, mu <- t - fl.
//   outputs       symbols[k] = z'_k; indices[k] = a^_k; position[k] = (double)m + mu, before the controller; error[k] = e_k; phase[k] =
//                 phi after its update.  count = the strobes all of whose interpolator reads (the window of z_k and, for 'gardner' and
//                 k >= 1, that of zm) had their indices in [0, n_y).
//   rejection     a row whose y (all n_y samples), k1, k2, kc1, kc2, mu0 or phase0 holds a NaN or +-inf or lies outside its range
//                 (k1, k2, kc1, kc2 >= 0; 0 <= mu0 < 1; |phase0| <= 0.5; 0 <= m0 < n_y), one of whose training labels is negative or
//                 >= M, or one of whose w or phi fails its test: zero integers, NaN floats.
//
// tr_loop_kernel<ted, interp, carrier>: the recursion is a serial chain per row -- every position depends on the previous error, and with
//   'mm' on the previous decision -- so one row per lane, one wave per workgroup, as ad_lms_kernel.  The samples come from a lane-private
//   LDS ring filled ahead of the chain, not straight from global memory: the address of a strobe's window is known only when the previous
//   step's controller has run, so a direct read would put a whole memory latency into every link of the chain, and at the batch of the
//   benchmark there are fewer than two waves a compute unit to hide it.  The ring holds the last 64 samples of the lane's row, sample s at
//   slot s & 63, as columns [slot][lane] of doubles (lane l and slot q at dword 2 (64 q + l): the bank depends on the lane alone, so lanes
//   at different positions do not conflict).  A step reads no sample below m - 7 (the midpoint lies less than 0.75 sps = 6 samples back,
//   and the cubic reads one more) and none above m + 2, and m advances by at most 12.  With `hi` the first sample not yet in the ring, a
//   lane whose hi < m + 16 fetches the 16 samples hi .. hi + 15 at the start of the step and writes them at its end, behind the step's own
//   reads: hi >= m + 3 holds at every step (no fetch: hi >= m + 16 >= m' + 3; fetch: hi + 16 >= m + 19 >= m' + 3), and hi <= m + 57 (40
//   at the start, below 32 after a fetch), so the ring's oldest sample hi - 64 is never above m - 7.  (As compiled, the wait for the
//   sixteen loads sits at the end of the fetching branch, so a fetch's latency is spread over 16 / sps steps, not hidden: DESIGN 4.26.)
//   The constellation sits in LDS.
//   A rejected row is found during the recursion, after some of its results were stored: the kernel rewrites the row at its end.  The
//   grid is a grid-stride loop under a cap, so a result depends on neither the batch nor the grid.
#include "cpx_internal.h"
#include "cpx_phasor.h"
#include "cpx_slice.h"
#include "cpx_wave.h"                      // grid_of

using namespace cpx;

#define CPX_TR_MAX_M 256
#define CPX_TR_MAX_N (1 << 30)
#define CPX_TR_MIN_SPS 2
#define CPX_TR_MAX_SPS 8
#define CPX_TR_RING 64                     // samples of a row held in LDS
#define CPX_TR_CHUNK 16                    // samples fetched at once; at least the largest advance of m, 12

namespace {

enum { TR_GARDNER = 0, TR_MM = 1 };
enum { TR_LINEAR = 0, TR_CUBIC = 1 };

struct TrRun {
    const double *y, *cst;                 // [rows][n_y][2], [M][2] (null without a modem)
    const int32_t *training;               // [nt] or [rows][nt]
    const double *k1, *k2, *kc1, *kc2;     // [1] or [rows]; kc1, kc2 null without the carrier loop
    const int64_t *m0;
    const double *mu0, *phase0;
    int64_t rows, n_y, nt;
    int n, sps, M, m;                      // m = 0: no modem, or M is no power of two
    int tr_batched, k1_batched, k2_batched, kc1_batched, kc2_batched, m0_batched, mu0_batched, phase0_batched;
    double *symbols;
    int32_t *indices;
    uint8_t *bits;
    double *position, *error, *phase;
    int32_t *count;
};

__device__ __forceinline__ void store_strobe(const TrRun &a, int64_t row, int k, double zr, double zi, int sel, double pos, double e,
                                             double phi) {
    const int64_t at = row * a.n + k;
    if (a.symbols) {
        a.symbols[at * 2] = zr;
        a.symbols[at * 2 + 1] = zi;
    }
    if (a.indices) a.indices[at] = sel;
    if (a.bits)
        for (int i = 0; i < a.m; i++) a.bits[at * a.m + i] = (uint8_t)((sel >> (a.m - 1 - i)) & 1);
    if (a.position) a.position[at] = pos;
    if (a.error) a.error[at] = e;
    if (a.phase) a.phase[at] = phi;
}

__device__ __forceinline__ double sample(const double *yrow, int64_t s, int64_t n_y, int part) {
    return s >= 0 && s < n_y ? yrow[2 * s + part] : 0.0;
}

__device__ __forceinline__ double farrow(double xm, double x0, double x1, double x2, double mu) {
    const double v3 = ((x2 - xm) + 3.0 * (x0 - x1)) * 0.16666666666666666;
    const double v2 = ((x1 + xm) * 0.5) - x0;
    const double v1 = ((6.0 * x1 - x2) - (3.0 * x0 + 2.0 * xm)) * 0.16666666666666666;
    return ((v3 * mu + v2) * mu + v1) * mu + x0;
}

// I(m, mu) from the lane's column of the ring; true if every index read lay in [0, n_y)
template <int INTERP>
__device__ __forceinline__ bool interpolate(const double *rr, const double *ri, int lane, int64_t m, double mu, int64_t n_y, double &zr,
                                            double &zi) {
    const int s0 = (int)(m & (CPX_TR_RING - 1)) * 64 + lane, s1 = (int)((m + 1) & (CPX_TR_RING - 1)) * 64 + lane;
    if constexpr (INTERP == TR_LINEAR) {
        const double ar = rr[s0], ai = ri[s0];
        zr = ar + mu * (rr[s1] - ar);
        zi = ai + mu * (ri[s1] - ai);
        return m >= 0 && m + 1 < n_y;
    } else {
        const int sm = (int)((m - 1) & (CPX_TR_RING - 1)) * 64 + lane, s2 = (int)((m + 2) & (CPX_TR_RING - 1)) * 64 + lane;
        zr = farrow(rr[sm], rr[s0], rr[s1], rr[s2], mu);
        zi = farrow(ri[sm], ri[s0], ri[s1], ri[s2], mu);
        return m >= 1 && m + 2 < n_y;
    }
}

template <int TED, int INTERP, int PLL>
__global__ __launch_bounds__(64) void tr_loop_kernel(TrRun a) {
    extern __shared__ double tr_ring[];                        // rr[RING][64], ri[RING][64]
    __shared__ double cr[CPX_TR_MAX_M], ci[CPX_TR_MAX_M];
    const int lane = threadIdx.x, n = a.n, M = a.M;
    const int64_t n_y = a.n_y, nt = a.nt;
    const double fsps = (double)a.sps;
    double *rr = tr_ring, *ri = tr_ring + CPX_TR_RING * 64;
    for (int i = lane; i < M; i += 64) {
        cr[i] = a.cst[2 * i];
        ci[i] = a.cst[2 * i + 1];
    }
    __syncthreads();                                           // no barrier from here on: every column of the ring is the lane's own
    const int64_t groups = (a.rows + 63) / 64;
    for (int64_t grp = blockIdx.x; grp < groups; grp += gridDim.x) {
        const int64_t local = grp * 64 + lane;
        const bool valid = local < a.rows;
        const int64_t row = valid ? local : 0;                 // a lane without a row works on the first
        const double *yrow = a.y + row * 2 * n_y;
        bool bad = false;
        for (int r = 0; r < 64 && grp * 64 + r < a.rows; r++) {  // the group's rows are scanned by all its lanes, a row at a time
            const bool any = scan_lanes(a.y + (grp * 64 + r) * 2 * n_y, 2 * n_y, lane, 64) != 0ull;
            if (r == lane) bad = any;
        }
        const double k1 = a.k1[a.k1_batched ? row : 0], k2 = a.k2[a.k2_batched ? row : 0];
        double kc1 = 0.0, kc2 = 0.0;
        if constexpr (PLL) {
            kc1 = a.kc1[a.kc1_batched ? row : 0];
            kc2 = a.kc2[a.kc2_batched ? row : 0];
        }
        const int64_t m0 = a.m0[a.m0_batched ? row : 0];
        const double mu0 = a.mu0[a.mu0_batched ? row : 0], phase0 = a.phase0[a.phase0_batched ? row : 0];
        bad |= not_finite(k1) || !(k1 >= 0.0) || not_finite(k2) || !(k2 >= 0.0) || not_finite(kc1) || !(kc1 >= 0.0) || not_finite(kc2) ||
               !(kc2 >= 0.0);
        bad |= !(mu0 >= 0.0) || !(mu0 < 1.0) || !(__builtin_fabs(phase0) <= 0.5) || m0 < 0 || m0 >= n_y;
        int64_t m = bad ? 0 : m0;
        double mu = bad ? 0.0 : mu0, phi = bad ? 0.0 : phase0;
        double v = 0.0, w = fsps, f = 0.0, pzr = 0.0, pzi = 0.0, prr = 0.0, pri = 0.0;
        int32_t inside_count = 0;
        int64_t hi = m + 40;
        for (int64_t s = m - 8; s < hi; s++) {                 // the ring before the first strobe
            const int at = (int)(s & (CPX_TR_RING - 1)) * 64 + lane;
            rr[at] = sample(yrow, s, n_y, 0);
            ri[at] = sample(yrow, s, n_y, 1);
        }
        const int32_t *tr = a.training + (a.tr_batched ? row * nt : 0);

        for (int k = 0; k < n && !bad; k++) {
            const bool fetch = hi < m + CPX_TR_CHUNK;          // written at the end of the step
            double nr[CPX_TR_CHUNK], ni[CPX_TR_CHUNK];
            if (fetch) {
#pragma unroll
                for (int q = 0; q < CPX_TR_CHUNK; q++) {       // sixteen loads in flight: the address is clamped, not the load skipped
                    const int64_t s = hi + q;
                    const bool in_row = s >= 0 && s < n_y;
                    const double *at = yrow + 2 * (in_row ? s : 0);
                    const double vr = at[0], vi = at[1];
                    nr[q] = in_row ? vr : 0.0;
                    ni[q] = in_row ? vi : 0.0;
                }
            }
            double zr, zi;
            bool inside = interpolate<INTERP>(rr, ri, lane, m, mu, n_y, zr, zi);
            double dr = zr, di = zi;
            if constexpr (PLL) {
                double c, s;
                unit_phasor(phi, c, s);
                dr = zr * c + zi * s;
                di = zi * c - zr * s;
            }
            int sel = 0;
            double rfr = 0.0, rfi = 0.0;
            if (M > 0) {
                double d0[1], d1[1];
                sel = slice<0>(dr, di, cr, ci, M, d0, d1);
                int lab = sel;
                if (k < nt) {
                    lab = tr[k];
                    if (lab < 0 || lab >= M) {
                        bad = true;
                        lab = 0;
                    }
                }
                rfr = cr[lab];
                rfi = ci[lab];
            }
            double e = 0.0;
            if (k > 0) {
                if constexpr (TED == TR_GARDNER) {
                    const double t = mu - 0.5 * w, fl = __builtin_floor(t);
                    double mr, mi;
                    inside &= interpolate<INTERP>(rr, ri, lane, m + (int64_t)fl, t - fl, n_y, mr, mi);
                    e = (pzr - zr) * mr + (pzi - zi) * mi;
                } else {
                    e = (prr * dr + pri * di) - (rfr * pzr + rfi * pzi);
                }
            }
            const double pos = (double)m + mu;
            if constexpr (PLL) {
                const double ep = di * rfr - dr * rfi;
                f = f + kc2 * ep;
                phi = phi + (f + kc1 * ep);
                phi = phi - __builtin_rint(phi);
                if (!(__builtin_fabs(phi) <= 0.5)) bad = true;
            }
            v = v + k2 * e;
            w = fsps + (v + k1 * e);
            if (!(0.5 * fsps < w && w < 1.5 * fsps)) bad = true;
            if (bad) break;
            inside_count += inside ? 1 : 0;
            if (valid) store_strobe(a, row, k, dr, di, sel, pos, e, phi);
            const double t = mu + w, fl = __builtin_floor(t);
            m += (int64_t)fl;
            mu = t - fl;
            if constexpr (TED == TR_GARDNER) {
                pzr = zr;
                pzi = zi;
            } else {
                pzr = dr;
                pzi = di;
                prr = rfr;
                pri = rfi;
            }
            if (fetch) {
#pragma unroll
                for (int q = 0; q < CPX_TR_CHUNK; q++) {
                    const int at = (int)((hi + q) & (CPX_TR_RING - 1)) * 64 + lane;
                    rr[at] = nr[q];
                    ri[at] = ni[q];
                }
                hi += CPX_TR_CHUNK;
            }
        }
        if (!valid) continue;
        if (bad) {
            const double nan = __builtin_nan("");
            for (int k = 0; k < n; k++) store_strobe(a, row, k, nan, nan, 0, nan, nan, nan);
        }
        if (a.count) a.count[row] = bad ? 0 : inside_count;
    }
}

typedef void (*TrKernel)(TrRun);
const TrKernel tr_kernels[2][2][2] = {
    {{tr_loop_kernel<TR_GARDNER, TR_LINEAR, 0>, tr_loop_kernel<TR_GARDNER, TR_LINEAR, 1>},
     {tr_loop_kernel<TR_GARDNER, TR_CUBIC, 0>, tr_loop_kernel<TR_GARDNER, TR_CUBIC, 1>}},
    {{tr_loop_kernel<TR_MM, TR_LINEAR, 0>, tr_loop_kernel<TR_MM, TR_LINEAR, 1>},
     {tr_loop_kernel<TR_MM, TR_CUBIC, 0>, tr_loop_kernel<TR_MM, TR_CUBIC, 1>}}};

// a parameter's host values, where the caller has them: every one must satisfy lo <= v and v <= hi (v < hi with `open`); a NaN passes,
// it rejects its row
bool in_range(const double *v, int64_t count, double lo, double hi, bool open) {
    for (int64_t i = 0; v && i < count; i++)
        if (v[i] < lo || v[i] > hi || (open && v[i] == hi)) return false;
    return true;
}

struct HostValues {                        // null in the device form, which cannot read them: the kernel rejects the rows
    const double *k1 = nullptr, *k2 = nullptr, *kc1 = nullptr, *kc2 = nullptr, *mu0 = nullptr, *phase0 = nullptr;
    const int64_t *m0 = nullptr;
    int64_t n_k1 = 0, n_k2 = 0, n_kc1 = 0, n_kc2 = 0, n_mu0 = 0, n_phase0 = 0, n_m0 = 0;
};

// the limits both entry points share; of the handle only M and nbits are read
int check_recover(const cpx_modem *md, int64_t B, int64_t n_y, int64_t n, int sps, int ted, int interp, bool have_k, bool have_kc1,
                  bool have_kc2, bool have_start, int64_t nt, const HostValues &h, bool want_labels, bool want_bits, bool want_phase,
                  bool any_output) {
    const double inf = __builtin_huge_val();
    CPX_REQUIRE(B >= 0, CPX_EINVAL, "timing_recover: B = %lld", (long long)B);
    CPX_REQUIRE(ted == TR_GARDNER || ted == TR_MM, CPX_EINVAL, "timing_recover: ted = %d, the limit is 0 ('gardner') or 1 ('mm')", ted);
    CPX_REQUIRE(interp == TR_LINEAR || interp == TR_CUBIC, CPX_EINVAL, "timing_recover: interp = %d, the limit is 0 ('linear') or 1 ('cubic')",
                interp);
    CPX_REQUIRE(sps >= CPX_TR_MIN_SPS && sps <= CPX_TR_MAX_SPS, CPX_EINVAL, "timing_recover: sps = %d, the limit is %d <= sps <= %d", sps,
                CPX_TR_MIN_SPS, CPX_TR_MAX_SPS);
    CPX_REQUIRE(n >= 1 && n <= CPX_TR_MAX_N, CPX_EINVAL, "timing_recover: n = %lld strobes, the limit is 1 <= n <= 2^30", (long long)n);
    CPX_REQUIRE(n_y >= 1 && n_y <= (int64_t)CPX_TR_MAX_N * CPX_TR_MAX_SPS, CPX_EINVAL,
                "timing_recover: n_y = %lld samples, the limit is 1 <= n_y <= 2^33", (long long)n_y);
    CPX_REQUIRE(have_k, CPX_EINVAL, "timing_recover: k1 and k2 are required");
    CPX_REQUIRE(have_kc1 == have_kc2, CPX_EINVAL, "timing_recover: the carrier loop takes both kc1 and kc2");
    CPX_REQUIRE(have_start, CPX_EINVAL, "timing_recover: m0, mu0 and phase0 are required");
    CPX_REQUIRE(md || ted != TR_MM, CPX_EINVAL, "timing_recover: 'mm' needs a modem");
    CPX_REQUIRE(md || !have_kc1, CPX_EINVAL, "timing_recover: the carrier loop needs a modem");
    CPX_REQUIRE(md || nt == 0, CPX_EINVAL, "timing_recover: training needs a modem");
    CPX_REQUIRE(md || !want_labels, CPX_EINVAL, "timing_recover: indices and bits need a modem");
    CPX_REQUIRE(!md || (md->M >= 2 && md->M <= CPX_TR_MAX_M), CPX_EINVAL,
                "timing_recover: a constellation of %d points, the limit is 2 <= M <= %d", md ? md->M : 0, CPX_TR_MAX_M);
    CPX_REQUIRE(!want_bits || (1 << md->nbits) == md->M, CPX_EINVAL,
                "timing_recover: a constellation of %d points, the limit for bits is M a power of two", md->M);
    CPX_REQUIRE(!want_phase || have_kc1, CPX_EINVAL, "timing_recover: phase is asked for without the carrier loop");
    CPX_REQUIRE(nt >= 0 && nt <= n, CPX_EINVAL, "timing_recover: nt = %lld training symbols, the limit is 0 <= nt <= n = %lld", (long long)nt,
                (long long)n);
    CPX_REQUIRE(in_range(h.k1, h.n_k1, 0.0, inf, false) && in_range(h.k2, h.n_k2, 0.0, inf, false), CPX_EINVAL,
                "timing_recover: k1, k2, the limit is k1 >= 0 and k2 >= 0");
    CPX_REQUIRE(in_range(h.kc1, h.n_kc1, 0.0, inf, false) && in_range(h.kc2, h.n_kc2, 0.0, inf, false), CPX_EINVAL,
                "timing_recover: carrier, the limit is kc1 >= 0 and kc2 >= 0");
    CPX_REQUIRE(in_range(h.mu0, h.n_mu0, 0.0, 1.0, true), CPX_EINVAL, "timing_recover: mu0, the limit is 0 <= mu0 < 1");
    CPX_REQUIRE(in_range(h.phase0, h.n_phase0, -0.5, 0.5, false), CPX_EINVAL, "timing_recover: phase0, the limit is |phase0| <= 0.5");
    for (int64_t i = 0; h.m0 && i < h.n_m0; i++)
        CPX_REQUIRE(h.m0[i] >= 0 && h.m0[i] < n_y, CPX_EINVAL, "timing_recover: m0 = %lld, the limit is 0 <= m0 < n_y = %lld",
                    (long long)h.m0[i], (long long)n_y);
    CPX_REQUIRE(any_output, CPX_EINVAL, "timing_recover: no output requested");
    return CPX_OK;
}

}  // namespace

extern "C" {

int cpx_timing_recover_dev(const cpx_modem *md, const double *d_y, int64_t B, int64_t n_y, int64_t n, int sps, int ted, int interp,
                           const double *d_k1, int k1_batched, const double *d_k2, int k2_batched, const double *d_kc1, int kc1_batched,
                           const double *d_kc2, int kc2_batched, const int32_t *d_training, int tr_batched, int64_t nt, const int64_t *d_m0,
                           int m0_batched, const double *d_mu0, int mu0_batched, const double *d_phase0, int phase0_batched,
                           double *d_symbols, int32_t *d_indices, uint8_t *d_bits, double *d_position, double *d_error, double *d_phase,
                           int32_t *d_count, void *stream) {
    CPX_TRACE("cpx_timing_recover_dev");
    if (int rc = check_recover(md, B, n_y, n, sps, ted, interp, d_k1 && d_k2, d_kc1 != nullptr, d_kc2 != nullptr,
                               d_m0 && d_mu0 && d_phase0, nt, HostValues(), d_indices || d_bits, d_bits != nullptr, d_phase != nullptr,
                               d_symbols || d_indices || d_bits || d_position || d_error || d_phase || d_count))
        return rc;
    if (B == 0) return CPX_OK;
    CPX_REQUIRE(d_y && (d_training || nt == 0), CPX_EINVAL, "timing_recover: null pointer");
    if (md) {
        if (int rcd = check_handle_device(md->device, "timing_recover")) return rcd;
    } else if (int rcd = ensure_device()) {
        return rcd;
    }
    hipStream_t st = pick_stream(stream);
    const int pll = d_kc1 ? 1 : 0, M = md ? md->M : 0;
    TrRun ra{d_y, md ? md->d_const : nullptr, d_training, d_k1, d_k2, d_kc1, d_kc2, d_m0, d_mu0, d_phase0, B, n_y, nt, (int)n, sps, M,
             md && (1 << md->nbits) == md->M ? md->nbits : 0, tr_batched ? 1 : 0, k1_batched ? 1 : 0, k2_batched ? 1 : 0,
             kc1_batched ? 1 : 0, kc2_batched ? 1 : 0, m0_batched ? 1 : 0, mu0_batched ? 1 : 0, phase0_batched ? 1 : 0, d_symbols,
             d_indices, d_bits, d_position, d_error, d_phase, d_count};
    const TrKernel fn = tr_kernels[ted][interp][pll];
    const unsigned lds = 16u * CPX_TR_RING * 64u;              // 64 KiB: above 48 KiB the dynamic table needs the attribute
    CPX_HIP(hipFuncSetAttribute((const void *)fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    const int64_t tr_cap = (int64_t)device_cus() * 2;           // two workgroups' rings fit a compute unit's 160 KiB
    fn<<<dim3(grid_of((B + 63) / 64, tr_cap)), dim3(64), lds, st>>>(ra);
    CPX_HIP(hipGetLastError());
    note_kernel("tr_loop_kernel %s %s carrier=%d sps=%d M=%d tr_cap=%lld", ted == TR_MM ? "mm" : "gardner",
                interp == TR_CUBIC ? "cubic" : "linear", pll, sps, M, (long long)tr_cap);
    return CPX_OK;
}

int cpx_timing_recover(const cpx_modem *md, const double *y, int64_t B, int64_t n_y, int64_t n, int sps, int ted, int interp,
                       const double *k1, int k1_batched, const double *k2, int k2_batched, const double *kc1, int kc1_batched,
                       const double *kc2, int kc2_batched, const int32_t *training, int tr_batched, int64_t nt, const int64_t *m0,
                       int m0_batched, const double *mu0, int mu0_batched, const double *phase0, int phase0_batched, double *symbols,
                       int32_t *indices, uint8_t *bits, double *position, double *error, double *phase, int32_t *count) {
    CPX_TRACE("cpx_timing_recover");
    const size_t b = B > 0 ? (size_t)B : 0;
    const auto per = [&](int batched) { return (int64_t)(batched ? b : 1); };
    HostValues h;
    h.k1 = k1, h.k2 = k2, h.kc1 = kc1, h.kc2 = kc2, h.mu0 = mu0, h.phase0 = phase0, h.m0 = m0;
    h.n_k1 = per(k1_batched), h.n_k2 = per(k2_batched), h.n_kc1 = per(kc1_batched), h.n_kc2 = per(kc2_batched);
    h.n_mu0 = per(mu0_batched), h.n_phase0 = per(phase0_batched), h.n_m0 = per(m0_batched);
    if (B == 0) h = HostValues();                              // nothing to read of an empty batch
    if (int rc = check_recover(md, B, n_y, n, sps, ted, interp, k1 && k2, kc1 != nullptr, kc2 != nullptr, m0 && mu0 && phase0, nt, h,
                               indices || bits, bits != nullptr, phase != nullptr,
                               symbols || indices || bits || position || error || phase || count))
        return rc;
    if (B == 0) return CPX_OK;
    CPX_REQUIRE(y && (training || nt == 0), CPX_EINVAL, "timing_recover: null pointer");
    int rc = ensure_device();
    if (rc) return rc;
    const size_t nn = (size_t)n;
    HostStage::Out outs[7] = {{symbols, 16 * b * nn}, {indices, 4 * b * nn}, {bits, b * nn * (size_t)(md ? md->nbits : 0)},
                              {position, 8 * b * nn}, {error, 8 * b * nn},   {phase, 8 * b * nn},
                              {count, 4 * b}};
    HostStage s;
    const double *dy, *dk1, *dk2, *dkc1 = nullptr, *dkc2 = nullptr, *dmu0, *dphase0;
    const int64_t *dm0;
    const int32_t *dtr = nullptr;
    if ((rc = s.in(y, 16 * b * (size_t)n_y, &dy)) || (rc = s.in(k1, 8 * (size_t)per(k1_batched), &dk1)) ||
        (rc = s.in(k2, 8 * (size_t)per(k2_batched), &dk2)) || (kc1 && (rc = s.in(kc1, 8 * (size_t)per(kc1_batched), &dkc1))) ||
        (kc2 && (rc = s.in(kc2, 8 * (size_t)per(kc2_batched), &dkc2))) ||
        (nt > 0 && (rc = s.in(training, 4 * (size_t)nt * (tr_batched ? b : 1), &dtr))) ||
        (rc = s.in(m0, 8 * (size_t)per(m0_batched), &dm0)) || (rc = s.in(mu0, 8 * (size_t)per(mu0_batched), &dmu0)) ||
        (rc = s.in(phase0, 8 * (size_t)per(phase0_batched), &dphase0)) || (rc = s.out(outs)))
        return rc;
    if ((rc = cpx_timing_recover_dev(md, dy, B, n_y, n, sps, ted, interp, dk1, k1_batched, dk2, k2_batched, dkc1, kc1_batched, dkc2,
                                     kc2_batched, dtr, tr_batched, nt, dm0, m0_batched, dmu0, mu0_batched, dphase0, phase0_batched,
                                     outs[0].as<double>(), outs[1].as<int32_t>(), outs[2].as<uint8_t>(), outs[3].as<double>(),
                                     outs[4].as<double>(), outs[5].as<double>(), outs[6].as<int32_t>(), s.st)))
        return rc;
    return s.get(outs);
}

}  // extern "C"
