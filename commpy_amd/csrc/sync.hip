// OFDM timing and carrier-frequency-offset synchronisation, batched, complex128 with float64 arithmetic only
// (cpx_set_precision does not apply; no process-wide switch).  Not in the reference; the yardstick is tests/sync_model.py.
//
//   y [B][nr][n], lag D >= 1, window W >= 1, nq = n - D, nd = nq - W + 1
//   q[b][i] = sum_r conj(y[b][r][i]) y[b][r][i+D]                       e[b][i] = 1/2 sum_r (|y[b][r][i]|^2 + |y[b][r][i+D]|^2)
//   P[b][d] = sum_{i=d}^{d+W-1} q[b][i],  E[b][d] likewise from e        M[b][d] = |P|^2 / E^2  (+0 where E == 0, NaN where E is NaN)
//   metric     P, E, M [B][nd], whichever are requested
//   estimate   per row the first largest non-NaN M in a search range: d^, M[d^], step = -atan2(Im P, Re P) / D -- nothing [B][nd] is written
//   align      out[b][r][k] = y[b][r][start[b] + offset + k] (+0 outside the row) rotated by step[b] k as freq_offset_kernel rotates
//
// Running sums without a running error.  The q axis of a row is cut into tiles of T = 1024 anchored at multiples of T.  scan_tile()
// forms q and e of one tile (per element a chain of fused multiply-adds from +0 over r ascending) and their exclusive in-tile prefix
// C in the LDS: a thread sums its 4 consecutive elements, the 64 thread sums of a wave are scanned by shuffles (Hillis-Steele, the
// lower operand first), the 4 wave sums in ascending order.  C(j) is a fixed tree over the elements below j and nothing else.  With
// k = d / T, j = d mod T, k' = (d + W) / T, j' = (d + W) mod T a window is
//   k' == k:   P = C_k(j') - C_k(j)
//   k' >  k:   P = ((total_k - C_k(j)) + mid) + C_k'(j'),  mid = total_{k+1} + ... + total_{k'-1} from +0 in ascending order
// The outputs of one tile meet two values of k' (k + W / T and the next), so a workgroup scans at most three tiles -- its own, tile
// k + W / T, and the first W mod T elements of the one behind it -- and the cost per output does not grow with W; the totals come
// from a first launch (sync_totals_kernel, the same scan_tile), which is skipped where no window needs one (W < T, W == T).
// No rounding of an output involves a product further than T - 1 positions from its window, and every value depends on the row's
// samples and on (n, D, W, d) alone: batch size, the row's place, the stream, the form (host or device) and the outputs requested
// give the same bits.  A NaN or an infinity spoils the windows that share a tile sum with it: its own row only.
// tile_windows() is the ONE device function behind metric and estimate: their P, E and M agree bit for bit.
//
// The search is a two-stage reduction: each tile writes its first maximum (M, d, P) to the scratch arena, sync_finish_kernel takes
// the first maximum of a row's tiles.  `m > best` lets NaNs lose, the lower d wins a tie.  Offsets 64-bit; grids capped at 65 535
// workgroups that stride over their tiles.
#include "cpx_internal.h"
#include "cpx_rotate.h"
#include "cpx_wave.h"             // grid_of

#include <climits>
#include <cmath>

using namespace cpx;

#define CPX_SYNC_MAX_ANT 1024
#define CPX_SYNC_MAX_LAG (1 << 20)      // D and W: the totals between a window's ends are summed once per workgroup

namespace {

constexpr int SY_BLOCK = 256, SY_R = 4, SY_T = SY_BLOCK * SY_R, SY_WAVES = SY_BLOCK / 64;

struct Sum3 { double x, y, e; };     // (Re q, Im q, e)
__device__ __forceinline__ Sum3 zero3() { return Sum3{0.0, 0.0, 0.0}; }
__device__ __forceinline__ Sum3 add3(Sum3 a, Sum3 b) { return Sum3{a.x + b.x, a.y + b.y, a.e + b.e}; }
__device__ __forceinline__ Sum3 sub3(Sum3 a, Sum3 b) { return Sum3{a.x - b.x, a.y - b.y, a.e - b.e}; }
// c ? a : b by component (a select of whole structs is lowered through memory)
__device__ __forceinline__ Sum3 sel3(bool c, Sum3 a, Sum3 b) { return Sum3{c ? a.x : b.x, c ? a.y : b.y, c ? a.e : b.e}; }
__device__ __forceinline__ Sum3 shfl_up3(Sum3 a, int off) { return Sum3{__shfl_up(a.x, off), __shfl_up(a.y, off), __shfl_up(a.e, off)}; }

struct SyPart { double m; long long d; double pr, pi; };    // a tile's (a row's) first maximum; d = -1: none

struct SyArgs {
    const double2 *y;       // [B][nr][n]
    double *tot;            // [B][ntq][3] tile totals (null: no window needs one)
    int64_t n, nq;          // nq = n - D; nd = nq - W + 1
    int64_t ntq;            // tiles of q per row
    int64_t k0, nk;         // the tiles a launch covers per row: k0 .. k0 + nk - 1
    int64_t B;
    int nr, D, W;
};

// the launch's tiles (row b, tile kt < nk of it), strided over a grid of tiles-of-a-row x rows in ONE loop: no 64-bit division in
// the kernel, and one loop's worth of hoisted address terms
#define SY_FOR_TILES(a, b, kt)                                   \
    for (int64_t b = blockIdx.y, kt = blockIdx.x; b < (a).B; kt += gridDim.x, kt >= (a).nk ? (kt = blockIdx.x, b += gridDim.y) : 0)

// at most 65 535 workgroups in all
dim3 tile_grid(int64_t B, int64_t nk) {
    const unsigned gx = grid_of(nk);
    return dim3(gx, grid_of(B < 65535 / gx ? B : 65535 / gx));
}

struct SyLds {
    double2 q[SY_T];
    double e[SY_T];
    double w[SY_WAVES][3];
};

// element j of the tile in the LDS: (q, e) before the scan, their exclusive prefix after it
__device__ __forceinline__ Sum3 prefix_at(const SyLds &s, int j) {
    const double2 v = s.q[j];
    return Sum3{v.x, v.y, s.e[j]};
}

// q and e of the first `need` elements of tile k of row b (zeros behind them and behind the row's end), their exclusive in-tile
// prefix left in s.q / s.e when KEEP; returns the tile's total.  Collective; the LDS may be read after it returns.
template <bool KEEP>
__device__ __forceinline__ Sum3 scan_tile(const SyArgs &a, int64_t b, int64_t k, int need, SyLds &s) {
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int64_t i0 = k * SY_T;
    const double2 *yt = a.y + b * a.nr * a.n + i0;          // the tile's first element (the caller made sure it exists) on antenna 0
    const int left = a.nq - i0 < need ? (int)(a.nq - i0) : need;
    __syncthreads();                                        // the previous user of the LDS is done
    // element idx = t + c SY_BLOCK, c < 4: coalesced loads, all antennas of the four elements in one loop.  An element that is not
    // wanted reads the tile's first element and is zeroed after the loads: no divergent region around them.
    double qr[SY_R], qi[SY_R], e[SY_R];
    int at[SY_R];
    bool live[SY_R];
#pragma unroll
    for (int c = 0; c < SY_R; c++) {
        live[c] = t + c * SY_BLOCK < left;
        at[c] = live[c] ? t + c * SY_BLOCK : 0;
        qr[c] = qi[c] = e[c] = 0.0;
    }
    for (int r = 0; r < a.nr; r++, yt += a.n) {
#pragma unroll
        for (int c = 0; c < SY_R; c++) {
            const double2 u = yt[at[c]], v = yt[at[c] + a.D];
            qr[c] = fma(u.x, v.x, qr[c]);
            qr[c] = fma(u.y, v.y, qr[c]);
            qi[c] = fma(u.x, v.y, qi[c]);
            qi[c] = fma(-u.y, v.x, qi[c]);
            e[c] = fma(u.x, u.x, e[c]);
            e[c] = fma(u.y, u.y, e[c]);
            e[c] = fma(v.x, v.x, e[c]);
            e[c] = fma(v.y, v.y, e[c]);
        }
    }
#pragma unroll
    for (int c = 0; c < SY_R; c++) {
        s.q[t + c * SY_BLOCK] = live[c] ? make_double2(qr[c], qi[c]) : make_double2(0.0, 0.0);
        s.e[t + c * SY_BLOCK] = live[c] ? 0.5 * e[c] : 0.0;
    }
    __syncthreads();
    Sum3 inc = zero3();
#pragma unroll
    for (int c = 0; c < SY_R; c++) inc = add3(inc, prefix_at(s, t * SY_R + c));
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const Sum3 o = shfl_up3(inc, off);
        if (lane >= off) inc = add3(o, inc);
    }
    Sum3 exc = shfl_up3(inc, 1);
    if (lane == 0) exc = zero3();
    if (lane == 63) { s.w[wave][0] = inc.x; s.w[wave][1] = inc.y; s.w[wave][2] = inc.e; }
    __syncthreads();
    Sum3 base = zero3(), total = zero3();
#pragma unroll
    for (int w = 0; w < SY_WAVES; w++) {
        const Sum3 ws{s.w[w][0], s.w[w][1], s.w[w][2]};
        if (w < wave) base = add3(base, ws);
        total = add3(total, ws);
    }
    if (KEEP) {
        base = add3(base, exc);                             // the elements are read again rather than kept across the scan
#pragma unroll
        for (int c = 0; c < SY_R; c++) {
            const Sum3 el = prefix_at(s, t * SY_R + c);
            s.q[t * SY_R + c] = make_double2(base.x, base.y);
            s.e[t * SY_R + c] = base.e;
            base = add3(base, el);
        }
        __syncthreads();
    }
    return total;
}

// P, E and M of the outputs d = k T + threadIdx.x + c SY_BLOCK, c < 4, of row b (values past nd are meaningless and finite or not).
// Collective.
__device__ __forceinline__ void tile_windows(const SyArgs &a, int64_t b, int64_t k, SyLds &s, double2 (&P)[SY_R], double (&E)[SY_R],
                                             double (&M)[SY_R]) {
    const int t = threadIdx.x;
    const int wq = a.W / SY_T, wr = a.W % SY_T;
    Sum3 acc[SY_R];
    // pass 0: tile k itself; pass 1: tile k + wq, where the windows with jj < T end; pass 2: the first wr elements of the tile behind
    // it, where the others end.  One loop, so that scan_tile is instantiated once.
#pragma unroll 1
    for (int pass = 0; pass < 3; pass++) {
        if ((pass == 1 && wq == 0) || (pass == 2 && wr == 0)) continue;
        const int64_t kk = pass == 0 ? k : pass == 1 ? k + wq : k + wq + 1;
        const bool there = kk < a.ntq;                      // (a window may end exactly where the row's q ends)
        Sum3 tot = zero3();
        if (there) tot = scan_tile<true>(a, b, kk, pass == 2 ? wr : SY_T, s);
        // the whole tiles between the window's ends, from +0 in ascending order: k + 1 .. k + wq - 1 for the windows that end in tile
        // k + wq, one more for the others
        Sum3 mid = zero3();
        if (pass > 0) {
            const double *tb = a.tot + (b * a.ntq) * 3;
            const int64_t mlast = pass == 1 ? k + wq : k + wq + 1, mend = mlast < a.ntq ? mlast : a.ntq;
            for (int64_t m = k + 1; m < mend; m++) mid = add3(mid, Sum3{tb[3 * m], tb[3 * m + 1], tb[3 * m + 2]});
        }
        const int first = pass == 2 ? SY_T : 0;
#pragma unroll
        for (int c = 0; c < SY_R; c++) {
            const int j = t + c * SY_BLOCK, jj = j + wr;
            if (pass == 0) {
                const bool same = wq == 0 && jj < SY_T;     // the window ends in tile k too
                const Sum3 cj = prefix_at(s, j), ce = prefix_at(s, same ? jj : j);
                acc[c] = sub3(sel3(same, ce, tot), cj);
            } else {
                const bool mine = (jj < SY_T) == (pass == 1);
                const Sum3 ce = prefix_at(s, mine ? jj - first : 0);
                acc[c] = sel3(mine, add3(add3(acc[c], mid), sel3(there, ce, zero3())), acc[c]);
            }
        }
    }
#pragma unroll
    for (int c = 0; c < SY_R; c++) {
        P[c] = make_double2(acc[c].x, acc[c].y);
        E[c] = acc[c].e;
        double m = 0.0;
        if (!(acc[c].e == 0.0)) {                           // a NaN E gives a NaN M
            const double rr = acc[c].x / acc[c].e, ri = acc[c].y / acc[c].e;
            m = rr * rr + ri * ri;
        }
        M[c] = m;
    }
}

__global__ __launch_bounds__(SY_BLOCK) void sync_totals_kernel(SyArgs a) {
    __shared__ SyLds s;
    SY_FOR_TILES(a, b, kt) {
        const int64_t k = a.k0 + kt;
        const Sum3 tot = scan_tile<false>(a, b, k, SY_T, s);
        if (threadIdx.x == 0) {
            double *o = a.tot + (b * a.ntq + k) * 3;
            o[0] = tot.x; o[1] = tot.y; o[2] = tot.e;
        }
    }
}

__global__ __launch_bounds__(SY_BLOCK) void sync_metric_kernel(SyArgs a, double2 *Pout, double *Eout, double *Mout) {
    __shared__ SyLds s;
    SY_FOR_TILES(a, b, kt) {
        const int64_t k = a.k0 + kt;
        double2 P[SY_R];
        double E[SY_R], M[SY_R];
        tile_windows(a, b, k, s, P, E, M);
        const int64_t nd = a.nq - a.W + 1;
#pragma unroll
        for (int c = 0; c < SY_R; c++) {
            const int64_t d = k * SY_T + threadIdx.x + c * SY_BLOCK;
            if (d < nd) {
                if (Pout) Pout[b * nd + d] = P[c];
                if (Eout) Eout[b * nd + d] = E[c];
                if (Mout) Mout[b * nd + d] = M[c];
            }
        }
    }
}

// the better of two candidates: the larger M (a NaN never is), then the lower d; (-1, -1) = none
__device__ __forceinline__ bool beats(double m, long long d, double bm, long long bd) { return m > bm || (m == bm && d < bd); }

// the workgroup's first maximum from every thread's (bm, bd); collective, all threads return it
__device__ __forceinline__ void block_first_max(double &bm, long long &bd, double (&wm)[SY_WAVES], long long (&wd)[SY_WAVES]) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const double om = __shfl_xor(bm, off);
        const long long od = __shfl_xor(bd, off);
        if (beats(om, od, bm, bd)) { bm = om; bd = od; }
    }
    __syncthreads();                                        // wm / wd of the previous tile have been read
    if ((threadIdx.x & 63) == 0) { wm[threadIdx.x >> 6] = bm; wd[threadIdx.x >> 6] = bd; }
    __syncthreads();
    bm = wm[0]; bd = wd[0];
#pragma unroll
    for (int w = 1; w < SY_WAVES; w++)
        if (beats(wm[w], wd[w], bm, bd)) { bm = wm[w]; bd = wd[w]; }
}

__global__ __launch_bounds__(SY_BLOCK) void sync_search_kernel(SyArgs a, int64_t lo, int64_t hi, SyPart *part) {      // [lo, hi) within [0, nd)
    __shared__ SyLds s;
    __shared__ double wm[SY_WAVES];
    __shared__ long long wd[SY_WAVES];
    SY_FOR_TILES(a, b, kt) {
        const int64_t k = a.k0 + kt;
        double2 P[SY_R];
        double E[SY_R], M[SY_R];
        tile_windows(a, b, k, s, P, E, M);
        double bm = -1.0, pr = 0.0, pi = 0.0;
        long long bd = -1;
#pragma unroll
        for (int c = 0; c < SY_R; c++) {                    // ascending d
            const int64_t d = k * SY_T + threadIdx.x + c * SY_BLOCK;
            if (d >= lo && d < hi && M[c] > bm) { bm = M[c]; bd = d; pr = P[c].x; pi = P[c].y; }
        }
        const long long mine = bd;
        block_first_max(bm, bd, wm, wd);
        if (bd >= 0 ? mine == bd : threadIdx.x == 0) part[b * a.nk + kt] = SyPart{bm, bd, pr, pi};
    }
}

__global__ __launch_bounds__(SY_BLOCK) void sync_finish_kernel(const SyPart *part, int64_t B, int64_t nk, double D, long long *d_hat,
                                                               double *peak, double *step) {
    __shared__ double wm[SY_WAVES];
    __shared__ long long wd[SY_WAVES];
    for (int64_t b = blockIdx.x; b < B; b += gridDim.x) {
        double bm = -1.0, pr = 0.0, pi = 0.0;
        long long bd = -1;
        for (int64_t i = threadIdx.x; i < nk; i += SY_BLOCK) {      // ascending d
            const SyPart p = part[b * nk + i];
            if (p.m > bm) { bm = p.m; bd = p.d; pr = p.pr; pi = p.pi; }
        }
        const long long mine = bd;
        block_first_max(bm, bd, wm, wd);
        if (bd >= 0 ? mine == bd : threadIdx.x == 0) {
            const double nan = __builtin_nan("");
            d_hat[b] = bd;
            peak[b] = bd >= 0 ? bm : nan;
            step[b] = bd >= 0 ? -atan2(pi, pr) / D : nan;
        }
    }
}

constexpr int AL_CHUNK = 1024;

__global__ __launch_bounds__(SY_BLOCK) void sync_align_kernel(const double2 *y, double2 *out, const long long *start, const double *step,
                                                              long long offset, int nr, int64_t n, int64_t nout, int64_t chunks_per_row,
                                                              int64_t nchunks) {
    for (int64_t c = blockIdx.x; c < nchunks; c += gridDim.x) {
        const int64_t row = c / chunks_per_row, b = row / nr;
        const int64_t k0 = (c - row * chunks_per_row) * AL_CHUNK;
        long long s0;
        const bool lost = __builtin_add_overflow(start[b], offset, &s0);     // nothing of such a row is inside it
        const double st = step ? step[b] : 0.0;
#pragma unroll
        for (int i = 0; i < AL_CHUNK / SY_BLOCK; i++) {
            const int64_t k = k0 + threadIdx.x + i * SY_BLOCK;
            if (k < nout) {
                const bool inside = !lost && s0 >= -k && s0 < n - k;
                const double2 v = inside ? y[row * n + (s0 + k)] : make_double2(0.0, 0.0);
                out[row * nout + k] = step ? freq_rotate(v, st, k) : v;
            }
        }
    }
}

// the shape checks of metric and estimate
int sync_sizes(const char *what, int64_t B, int nr, int64_t n, int64_t D, int64_t W) {
    CPX_REQUIRE(B >= 0, CPX_EINVAL, "%s: negative batch size", what);
    CPX_REQUIRE(nr >= 1 && D >= 1 && W >= 1, CPX_EINVAL, "%s: nr = %d, D = %lld, W = %lld, need at least 1 of each", what, nr, (long long)D,
                (long long)W);
    CPX_REQUIRE(nr <= CPX_SYNC_MAX_ANT, CPX_ELIMIT, "%s: nr = %d is above the engine's limit of %d", what, nr, CPX_SYNC_MAX_ANT);
    CPX_REQUIRE(D <= CPX_SYNC_MAX_LAG && W <= CPX_SYNC_MAX_LAG, CPX_ELIMIT, "%s: D = %lld, W = %lld, the engine's limit is %d", what,
                (long long)D, (long long)W, CPX_SYNC_MAX_LAG);
    CPX_REQUIRE(B == 0 || n - D - W + 1 >= 1, CPX_EINVAL, "%s: n = %lld samples hold no window of D + W = %lld", what, (long long)n,
                (long long)(D + W));
    CPX_REQUIRE(B == 0 || n <= INT64_MAX / 64 / B / nr, CPX_EINVAL, "%s: %lld x %d x %lld samples overflow", what, (long long)B, nr, (long long)n);
    return CPX_OK;
}

int search_range(int64_t B, int64_t n, int64_t D, int64_t W, int64_t d_lo, int64_t d_hi, int64_t *lo, int64_t *hi) {
    CPX_REQUIRE(d_lo < d_hi, CPX_EINVAL, "sync_estimate: the search range [%lld, %lld) is empty", (long long)d_lo, (long long)d_hi);
    if (B == 0) return CPX_OK;
    const int64_t nd = n - D - W + 1;
    *lo = d_lo > 0 ? d_lo : 0;
    *hi = d_hi < nd ? d_hi : nd;
    CPX_REQUIRE(*lo < *hi, CPX_EINVAL, "sync_estimate: the search range [%lld, %lld) holds none of the row's %lld positions", (long long)d_lo,
                (long long)d_hi, (long long)nd);
    return CPX_OK;
}

int align_sizes(int64_t B, int nr, int64_t n, int64_t nout) {
    CPX_REQUIRE(B >= 0 && n >= 0, CPX_EINVAL, "sync_align: negative size");
    CPX_REQUIRE(nr >= 1 && nout >= 1, CPX_EINVAL, "sync_align: nr = %d, nout = %lld, need at least 1 of each", nr, (long long)nout);
    CPX_REQUIRE(nr <= CPX_SYNC_MAX_ANT, CPX_ELIMIT, "sync_align: nr = %d is above the engine's limit of %d", nr, CPX_SYNC_MAX_ANT);
    CPX_REQUIRE(B == 0 || (n <= INT64_MAX / 64 / B / nr && nout <= INT64_MAX / 64 / B / nr), CPX_EINVAL, "sync_align: %lld x %d rows overflow",
                (long long)B, nr);
    return CPX_OK;
}

// the launch geometry shared by metric and estimate; queues sync_totals_kernel where a window needs a total
int windows_setup(SyArgs &a, const double *d_y, int64_t B, int nr, int64_t n, int64_t D, int64_t W, int64_t lo, int64_t hi, Scratch &sc,
                  hipStream_t st, bool *totals) {
    a.y = reinterpret_cast<const double2 *>(d_y);
    a.B = B; a.n = n; a.D = (int)D; a.W = (int)W; a.nr = nr;
    a.nq = n - D;
    a.ntq = (a.nq + SY_T - 1) / SY_T;
    const int64_t wq = W / SY_T, wr = W - wq * SY_T;
    const int64_t k0 = lo / SY_T, k1 = (hi - 1) / SY_T;
    *totals = wq >= 2 || (wq >= 1 && wr > 0);
    a.tot = nullptr;
    if (*totals) {
        if (int rc = sc.get(st, Slot::sync_totals, 24 * (size_t)(B * a.ntq), &a.tot)) return rc;
        // the tiles between the ends of the windows of tiles k0 .. k1
        a.k0 = k0 + 1;
        const int64_t last = k1 + wq < a.ntq - 1 ? k1 + wq : a.ntq - 1;
        a.nk = last - a.k0 + 1;
        if (a.nk > 0) {
            hipLaunchKernelGGL(sync_totals_kernel, tile_grid(B, a.nk), dim3(SY_BLOCK), 0, st, a);
        }
    }
    a.k0 = k0;
    a.nk = k1 - k0 + 1;
    return CPX_OK;
}

}  // namespace

extern "C" {

int cpx_sync_metric_dev(const double *d_y_re_im, int64_t B, int nr, int64_t n, int64_t D, int64_t W, double *d_P_re_im, double *d_E,
                        double *d_M, void *stream) {
    CPX_TRACE("cpx_sync_metric_dev");
    if (int rc = sync_sizes("sync_metric", B, nr, n, D, W)) return rc;
    CPX_REQUIRE(d_P_re_im || d_E || d_M, CPX_EINVAL, "sync_metric: no output requested");
    if (B == 0) return CPX_OK;
    CPX_REQUIRE(d_y_re_im, CPX_EINVAL, "sync_metric: null pointer");
    hipStream_t st = pick_stream(stream);
    Scratch sc;
    SyArgs a{};
    bool totals;
    if (int rc = windows_setup(a, d_y_re_im, B, nr, n, D, W, 0, n - D - W + 1, sc, st, &totals)) return rc;
    hipLaunchKernelGGL(sync_metric_kernel, tile_grid(B, a.nk), dim3(SY_BLOCK), 0, st, a, reinterpret_cast<double2 *>(d_P_re_im), d_E, d_M);
    CPX_HIP(hipGetLastError());
    note_kernel(totals ? "sync_totals_kernel+sync_metric_kernel" : "sync_metric_kernel");
    return CPX_OK;
}

int cpx_sync_metric(const double *y_re_im, int64_t B, int nr, int64_t n, int64_t D, int64_t W, double *P_re_im, double *E, double *M) {
    CPX_TRACE("cpx_sync_metric");
    if (int rc = sync_sizes("sync_metric", B, nr, n, D, W)) return rc;
    CPX_REQUIRE(P_re_im || E || M, CPX_EINVAL, "sync_metric: no output requested");
    if (B == 0) return CPX_OK;
    CPX_REQUIRE(y_re_im, CPX_EINVAL, "sync_metric: null pointer");
    int rc = ensure_device();
    if (rc) return rc;
    const size_t in_bytes = 16 * (size_t)(B * nr * n), cells = (size_t)(B * (n - D - W + 1));
    HostStage s;
    const double *dy;
    double *dP = nullptr, *dE = nullptr, *dM = nullptr;
    if ((rc = s.in(y_re_im, in_bytes, &dy))) return rc;
    if (P_re_im && (rc = s.out(16 * cells, &dP))) return rc;
    if (E && (rc = s.out(8 * cells, &dE))) return rc;
    if (M && (rc = s.out(8 * cells, &dM))) return rc;
    if ((rc = cpx_sync_metric_dev(dy, B, nr, n, D, W, dP, dE, dM, s.st))) return rc;
    if ((rc = s.get(P_re_im, dP, P_re_im ? 16 * cells : 0)) || (rc = s.get(E, dE, E ? 8 * cells : 0))) return rc;
    return s.get(M, dM, M ? 8 * cells : 0);
}

int cpx_sync_estimate_dev(const double *d_y_re_im, int64_t B, int nr, int64_t n, int64_t D, int64_t W, int64_t d_lo, int64_t d_hi,
                          int64_t *d_d_hat, double *d_peak, double *d_step, void *stream) {
    CPX_TRACE("cpx_sync_estimate_dev");
    if (int rc = sync_sizes("sync_estimate", B, nr, n, D, W)) return rc;
    int64_t lo = 0, hi = 0;
    if (int rc = search_range(B, n, D, W, d_lo, d_hi, &lo, &hi)) return rc;
    if (B == 0) return CPX_OK;
    CPX_REQUIRE(d_y_re_im && d_d_hat && d_peak && d_step, CPX_EINVAL, "sync_estimate: null pointer");
    hipStream_t st = pick_stream(stream);
    Scratch sc;
    SyArgs a{};
    bool totals;
    if (int rc = windows_setup(a, d_y_re_im, B, nr, n, D, W, lo, hi, sc, st, &totals)) return rc;
    SyPart *part = nullptr;
    if (int rc = sc.get(st, Slot::sync_parts, sizeof(SyPart) * (size_t)(B * a.nk), &part)) return rc;
    hipLaunchKernelGGL(sync_search_kernel, tile_grid(B, a.nk), dim3(SY_BLOCK), 0, st, a, lo, hi, part);
    hipLaunchKernelGGL(sync_finish_kernel, dim3(grid_of(B)), dim3(SY_BLOCK), 0, st, part, B, a.nk, (double)D,
                       reinterpret_cast<long long *>(d_d_hat), d_peak, d_step);
    CPX_HIP(hipGetLastError());
    note_kernel(totals ? "sync_totals_kernel+sync_search_kernel+sync_finish_kernel" : "sync_search_kernel+sync_finish_kernel");
    return CPX_OK;
}

int cpx_sync_estimate(const double *y_re_im, int64_t B, int nr, int64_t n, int64_t D, int64_t W, int64_t d_lo, int64_t d_hi, int64_t *d_hat,
                      double *peak, double *step) {
    CPX_TRACE("cpx_sync_estimate");
    if (int rc = sync_sizes("sync_estimate", B, nr, n, D, W)) return rc;
    int64_t lo = 0, hi = 0;
    if (int rc = search_range(B, n, D, W, d_lo, d_hi, &lo, &hi)) return rc;
    if (B == 0) return CPX_OK;
    CPX_REQUIRE(y_re_im && d_hat && peak && step, CPX_EINVAL, "sync_estimate: null pointer");
    int rc = ensure_device();
    if (rc) return rc;
    HostStage s;
    const double *dy;
    int64_t *dd;
    double *dp, *ds;
    if ((rc = s.in(y_re_im, 16 * (size_t)(B * nr * n), &dy)) || (rc = s.out(8 * (size_t)B, &dd)) || (rc = s.out(8 * (size_t)B, &dp)) ||
        (rc = s.out(8 * (size_t)B, &ds)) || (rc = cpx_sync_estimate_dev(dy, B, nr, n, D, W, d_lo, d_hi, dd, dp, ds, s.st)))
        return rc;
    if ((rc = s.get(d_hat, dd, 8 * (size_t)B)) || (rc = s.get(peak, dp, 8 * (size_t)B))) return rc;
    return s.get(step, ds, 8 * (size_t)B);
}

int cpx_sync_align_dev(const double *d_y_re_im, int64_t B, int nr, int64_t n, const int64_t *d_start, const double *d_step, int64_t offset,
                       int64_t nout, double *d_out_re_im, void *stream) {
    CPX_TRACE("cpx_sync_align_dev");
    if (int rc = align_sizes(B, nr, n, nout)) return rc;
    if (B == 0) return CPX_OK;
    CPX_REQUIRE((d_y_re_im || n == 0) && d_start && d_out_re_im, CPX_EINVAL, "sync_align: null pointer");
    CPX_REQUIRE(d_out_re_im != d_y_re_im, CPX_EINVAL, "sync_align: out must not alias y");
    const int64_t chunks_per_row = (nout + AL_CHUNK - 1) / AL_CHUNK, nchunks = B * nr * chunks_per_row;
    hipLaunchKernelGGL(sync_align_kernel, dim3(grid_of(nchunks)), dim3(SY_BLOCK), 0, pick_stream(stream),
                       reinterpret_cast<const double2 *>(d_y_re_im), reinterpret_cast<double2 *>(d_out_re_im),
                       reinterpret_cast<const long long *>(d_start), d_step, (long long)offset, nr, n, nout, chunks_per_row, nchunks);
    CPX_HIP(hipGetLastError());
    note_kernel("sync_align_kernel");
    return CPX_OK;
}

int cpx_sync_align(const double *y_re_im, int64_t B, int nr, int64_t n, const int64_t *start, const double *step, int64_t offset, int64_t nout,
                   double *out_re_im) {
    CPX_TRACE("cpx_sync_align");
    if (int rc = align_sizes(B, nr, n, nout)) return rc;
    if (B == 0) return CPX_OK;
    CPX_REQUIRE((y_re_im || n == 0) && start && out_re_im, CPX_EINVAL, "sync_align: null pointer");
    CPX_REQUIRE(out_re_im != y_re_im, CPX_EINVAL, "sync_align: out must not alias y");
    int rc = ensure_device();
    if (rc) return rc;
    const size_t out_bytes = 16 * (size_t)(B * nr * nout);
    HostStage s;
    const double *dy, *dstep = nullptr;
    const int64_t *dstart;
    double *dout;
    if ((rc = s.in(y_re_im, 16 * (size_t)(B * nr * n), &dy)) || (rc = s.in(start, 8 * (size_t)B, &dstart))) return rc;
    if (step && (rc = s.in(step, 8 * (size_t)B, &dstep))) return rc;
    if ((rc = s.out(out_bytes, &dout)) || (rc = cpx_sync_align_dev(dy, B, nr, n, dstart, dstep, offset, nout, dout, s.st))) return rc;
    return s.get(out_re_im, dout, out_bytes);
}

}  // extern "C"
