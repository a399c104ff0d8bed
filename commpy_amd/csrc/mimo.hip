// MIMO detection (commpy/modulation.py:299-565, 568-646): exhaustive ML search, K-best Schnorr-Euchner search with hard,
// soft (max-log over the final candidate list) and candidate-list outputs, and the soft-output best-first stack search (see
// the section below and DESIGN.md 4.7).  float64 throughout, -ffp-contract=off.
//
// One wave (64 lanes, one workgroup) per received vector, grid-striding over the batch.
//   ML      the nt x m table of column-times-point products sits in LDS (when it fits); lanes stride over hypothesis PREFIXES
//           (antennas 0..nt-2) and each prefix's residual is reused for the m points of the last antenna, so a hypothesis
//           costs nr complex subtractions and squares.  A lexicographic (metric, index) argmin across the wave gives the first
//           minimum -- NumPy's argmin, NaN first.
//   K-best complex Householder QR of [H | y] in the workgroup's storage, then the breadth-first search of the reference: children
//           at position point * nb_can + parent, the min(nb_hyp, K) smallest accumulated distances kept IN ASCENDING ORDER, ties
//           (and NaN, which sorts last) broken by the lowest child position.  Selection is K rounds of a wave argmin: every lane
//           caches the minimum of the children it owns, one cross-lane reduction per round picks the winner, only the winner's
//           lane rescans.  That yields exactly the sorted prefix the reference's argsort takes, for K * (6 shuffles + N / 64)
//           steps instead of the N^2 / 64 of rank counting or N log^2 N / 64 of a bitonic sort.
// The state of a vector (QR workspace, two candidate buffers, the children) lives in LDS on the fast path and in a global
// workspace on the general path (same code, templated on the storage): arguments whose state exceeds LDS_MAX take the latter,
// cpx_kbest_set_path("general") forces it.
#include "cpx_internal.h"

#include <atomic>
#include <cmath>
#include <cstdlib>

using namespace cpx;

// shared with mimo_linear.hip (cpx_internal.h)
namespace cpx {

int mimo_check(const cpx_modem *md, int64_t B, int nr, int nt, const char *what) {
    CPX_REQUIRE(md, CPX_EINVAL, "%s: null modem", what);
    if (int rc = check_handle_device(md->device, what)) return rc;
    CPX_REQUIRE(B >= 0 && nr >= 1 && nt >= 1, CPX_EINVAL, "%s: need B >= 0, nr >= 1, nt >= 1", what);
    return CPX_OK;
}

// the host-buffer wrappers' checks, ensure_device() first
int mimo_host_check(const double *y, const double *h, int64_t B, int nr, int nt, const void *out) {
    if (int rc = ensure_device()) return rc;
    CPX_REQUIRE(B >= 0 && nr >= 1 && nt >= 1, CPX_EINVAL, "mimo: need B >= 0, nr >= 1, nt >= 1");
    CPX_REQUIRE((y && h && out) || B == 0, CPX_EINVAL, "mimo: null pointer");
    return CPX_OK;
}

// y and H staged; an empty batch stages neither (its device entry point gets null y and H, and its outputs are empty downloads)
int mimo_in(HostStage &s, const double *y, const double *h, int h_batched, int64_t B, int nr, int nt, const double **dy,
            const double **dh) {
    *dy = *dh = nullptr;
    if (B == 0) return CPX_OK;
    if (int rc = s.in(y, 16 * size_t(B) * nr, dy)) return rc;
    return s.in(h, 16 * size_t(nr) * nt * (h_batched ? size_t(B) : 1), dh);
}

}  // namespace cpx

namespace {

constexpr int WAVE = 64;
constexpr size_t LDS_MAX = 64 * 1024;   // dynamic LDS budget of one workgroup on the fast paths
constexpr int64_t MAX_HYP = int64_t(1) << 31;

__device__ __forceinline__ double2 cmul(double2 a, double2 b) { return make_double2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }
__device__ __forceinline__ double2 csub(double2 a, double2 b) { return make_double2(a.x - b.x, a.y - b.y); }
__device__ __forceinline__ double abs2(double2 a) { return a.x * a.x + a.y * a.y; }

// (metric, index) order: NaN before numbers (ML: argmin returns the first NaN) or after them (K-best: argsort puts NaN last),
// equal metrics by index
template <bool NAN_FIRST>
__device__ __forceinline__ bool key_less(double a, long long ia, double b, long long ib) {
    const bool an = a != a, bn = b != b;
    if (an || bn) return (an && bn) ? ia < ib : (NAN_FIRST ? an : bn);
    if (a != b) return a < b;
    return ia < ib;
}

template <bool NAN_FIRST>
__device__ __forceinline__ void wave_argmin(double &m, long long &i) {
#pragma unroll
    for (int off = WAVE / 2; off >= 1; off >>= 1) {
        const double om = __shfl_xor(m, off);
        const long long oi = __shfl_xor(i, off);
        if (key_less<NAN_FIRST>(om, oi, m, i)) { m = om; i = oi; }
    }
}

// ---- ML --------------------------------------------------------------------------------------------------------------------
// LDS: H [nr][nt], y [nr], per-lane residual [64][nr], TAB: products [nt][m][nr]
template <bool TAB>
__global__ __launch_bounds__(WAVE) void mimo_ml_kernel(const double2 *__restrict__ y, const double2 *__restrict__ H, int64_t hstride,
                                                       int64_t B, int nr, int nt, const double2 *__restrict__ c, int m, int lgm,
                                                       int32_t *__restrict__ out) {
    extern __shared__ double2 lds[];
    double2 *sH = lds, *sy = sH + nr * nt, *res = sy + nr, *T = res + WAVE * nr;
    const int lane = threadIdx.x;
    double2 *my = res + lane * nr;
    const long long P = 1ll << (lgm * (nt - 1));   // prefixes over antennas 0..nt-2
    for (int64_t b = blockIdx.x; b < B; b += gridDim.x) {
        const double2 *Hb = H + b * hstride, *yb = y + b * nr;
        for (int i = lane; i < nr * nt; i += WAVE) sH[i] = Hb[i];
        for (int i = lane; i < nr; i += WAVE) sy[i] = yb[i];
        __syncthreads();
        if (TAB) {
            for (int i = lane; i < nt * m * nr; i += WAVE) {
                const int r = i % nr, p = (i / nr) % m, t = i / (nr * m);
                T[i] = cmul(sH[r * nt + t], c[p]);
            }
            __syncthreads();
        }
        double best = INFINITY;
        long long bi = 0x7fffffffffffffffll;
        const int last = nt - 1;
        for (long long p = lane; p < P; p += WAVE) {
            for (int r = 0; r < nr; r++) my[r] = sy[r];
            for (int t = 0; t < last; t++) {
                const int d = int(p >> (lgm * (last - 1 - t))) & (m - 1);
                for (int r = 0; r < nr; r++) my[r] = csub(my[r], TAB ? T[(t * m + d) * nr + r] : cmul(sH[r * nt + t], c[d]));
            }
            for (int q = 0; q < m; q++) {
                double met = 0.0;
                for (int r = 0; r < nr; r++)
                    met += abs2(csub(my[r], TAB ? T[(last * m + q) * nr + r] : cmul(sH[r * nt + last], c[q])));
                const long long idx = (p << lgm) | q;
                if (key_less<true>(met, idx, best, bi)) { best = met; bi = idx; }
            }
        }
        wave_argmin<true>(best, bi);
        for (int t = lane; t < nt; t += WAVE) out[b * nt + t] = int32_t(bi >> (lgm * (nt - 1 - t))) & (m - 1);
        __syncthreads();
    }
}

// complex Householder QR of the row-major [nr][w] matrix A = [H | y] (w = nt + 1) by one wave, in place: after the first
// kend columns, the upper part of A[0..kend-1][0..w-2] holds R and A[0..kend-1][w-1] = Q^H y.  Below the diagonal: the
// reflectors (not read by the searches).
__device__ __forceinline__ void householder_qr(double2 *A, int nr, int w, int kend, int lane) {
    for (int k = 0; k < kend; k++) {
        double tail = 0.0;
        for (int i = k + 1; i < nr; i++) tail += abs2(A[i * w + k]);
        const double2 x0 = A[k * w + k];
        const double nx = sqrt(abs2(x0) + tail);
        const double ax0 = hypot(x0.x, x0.y);
        const double2 ph = ax0 > 0.0 ? make_double2(x0.x / ax0, x0.y / ax0) : make_double2(1.0, 0.0);
        const double2 alpha = make_double2(-ph.x * nx, -ph.y * nx);
        const double2 v0 = csub(x0, alpha);
        const double vn2 = abs2(v0) + tail;
        // a zero column is skipped; a NaN column reflects, so that the NaN reaches every later column and Q^H y as it does in
        // LAPACK's QR (skipping it would leave a finite R and y behind a NaN entry of H)
        const bool reflect = !(nx <= 0.0) && !(vn2 <= 0.0);
        if (reflect) {
            for (int j = k + 1 + lane; j < w; j += WAVE) {
                double2 s = make_double2(v0.x * A[k * w + j].x + v0.y * A[k * w + j].y, v0.x * A[k * w + j].y - v0.y * A[k * w + j].x);
                for (int i = k + 1; i < nr; i++) {
                    const double2 vi = A[i * w + k], a = A[i * w + j];
                    s.x += vi.x * a.x + vi.y * a.y;      // conj(v_i) a
                    s.y += vi.x * a.y - vi.y * a.x;
                }
                const double2 f = make_double2(2.0 * s.x / vn2, 2.0 * s.y / vn2);
                A[k * w + j] = csub(A[k * w + j], cmul(f, v0));
                for (int i = k + 1; i < nr; i++) A[i * w + j] = csub(A[i * w + j], cmul(f, A[i * w + k]));
            }
        }
        __syncthreads();
        if (lane == 0 && reflect) A[k * w + k] = alpha;
        __syncthreads();
    }
}

// ---- K-best -----------------------------------------------------------------------------------------------------------------
struct KbLayout {   // byte offsets into one vector's state
    size_t A, Pd0, Pd1, Pt0, Pt1, Pi0, Pi1, Ct, sel, Ck, bytes;
};

KbLayout kb_layout(int nr, int nt, int K, int m) {
    KbLayout L;
    size_t o = 0;
    auto take = [&](size_t n, size_t al) { o = (o + al - 1) / al * al; size_t r = o; o += n; return r; };
    const size_t N = size_t(K) * m;
    L.A = take(16 * size_t(nr) * (nt + 1), 16);
    L.Pd0 = take(16 * size_t(K) * nt, 16);
    L.Pd1 = take(16 * size_t(K) * nt, 16);
    L.Pt0 = take(8 * size_t(K), 8);
    L.Pt1 = take(8 * size_t(K), 8);
    L.Ct = take(8 * N, 8);
    L.Pi0 = take(4 * size_t(K) * nt, 4);
    L.Pi1 = take(4 * size_t(K) * nt, 4);
    L.sel = take(4 * size_t(K), 4);
    L.Ck = take(N, 1);
    L.bytes = (o + 15) / 16 * 16;
    return L;
}

enum { KB_HARD = 0, KB_SOFT = 1, KB_LIST = 2 };

template <bool GLOBAL>
__global__ __launch_bounds__(WAVE) void kbest_kernel(const double2 *__restrict__ y, const double2 *__restrict__ H, int64_t hstride,
                                                     int64_t B, int nr, int nt, const double2 *__restrict__ c, int m, int nbits, int K,
                                                     KbLayout L, char *ws, int mode, double noise_var, int32_t *__restrict__ out_idx,
                                                     double *__restrict__ out_llr, int32_t *__restrict__ out_count) {
    extern __shared__ double2 lds_d2[];
    char *base = GLOBAL ? ws + size_t(blockIdx.x) * L.bytes : reinterpret_cast<char *>(lds_d2);
    double2 *A = reinterpret_cast<double2 *>(base + L.A);
    double2 *Pd[2] = {reinterpret_cast<double2 *>(base + L.Pd0), reinterpret_cast<double2 *>(base + L.Pd1)};
    double *Pt[2] = {reinterpret_cast<double *>(base + L.Pt0), reinterpret_cast<double *>(base + L.Pt1)};
    int32_t *Pi[2] = {reinterpret_cast<int32_t *>(base + L.Pi0), reinterpret_cast<int32_t *>(base + L.Pi1)};
    double *Ct = reinterpret_cast<double *>(base + L.Ct);
    int32_t *sel = reinterpret_cast<int32_t *>(base + L.sel);
    uint8_t *Ck = reinterpret_cast<uint8_t *>(base + L.Ck);
    const int lane = threadIdx.x;
    const int w = nt + 1;   // row stride of [H | y]
    for (int64_t b = blockIdx.x; b < B; b += gridDim.x) {
        const double2 *Hb = H + b * hstride, *yb = y + b * nr;
        for (int i = lane; i < nr * w; i += WAVE) {
            const int r = i / w, j = i - r * w;
            A[i] = j < nt ? Hb[r * nt + j] : yb[r];
        }
        __syncthreads();
        householder_qr(A, nr, w, nt, lane);   // A[0..nt-1][0..nt-1] holds R (upper part), A[0..nt-1][nt] = Q^H y
        // the search, antenna nt-1 down to 0
        int cur = 0, nb = 1;
        for (int t = lane; t < nt; t += WAVE) { Pd[0][t] = A[t * w + nt]; Pi[0][t] = 0; }
        if (lane == 0) Pt[0][0] = 0.0;
        __syncthreads();
        for (int coor = nt - 1; coor >= 0; coor--) {
            const int N = nb * m;
            const double2 rcc = A[coor * w + coor];
            double lm = NAN;
            long long li = 0x7fffffffffffffffll;
            for (int j = lane; j < N; j += WAVE) {
                const int p = j / nb, q = j - p * nb;
                const double2 e = csub(Pd[cur][q * nt + coor], cmul(rcc, c[p]));
                const double tot = Pt[cur][q] + abs2(e);
                Ct[j] = tot;
                Ck[j] = 0;
                if (li == 0x7fffffffffffffffll || key_less<false>(tot, j, lm, li)) { lm = tot; li = j; }
            }
            const int nk = N < K ? N : K;
            for (int k = 0; k < nk; k++) {
                double bm = lm;
                long long bj = li;
                wave_argmin<false>(bm, bj);   // lanes without a child left carry index INT64_MAX: never chosen while one remains
                if (lane == 0) sel[k] = int32_t(bj);
                if (bj == li) {               // the owner lane: retire the child, rescan its own
                    Ck[bj] = 1;
                    lm = NAN;
                    li = 0x7fffffffffffffffll;
                    for (int j = lane; j < N; j += WAVE)
                        if (!Ck[j] && (li == 0x7fffffffffffffffll || key_less<false>(Ct[j], j, lm, li))) { lm = Ct[j]; li = j; }
                }
            }
            __syncthreads();
            const int nxt = cur ^ 1;
            for (int i = lane; i < nk * nt; i += WAVE) {
                const int k = i / nt, t = i - k * nt;
                const int j = sel[k], p = j / nb, q = j - p * nb;
                const double2 d = Pd[cur][q * nt + t];
                double2 nd = d;
                if (t < coor) nd = csub(d, cmul(A[t * w + coor], c[p]));
                else if (t == coor) nd = csub(d, cmul(rcc, c[p]));
                Pd[nxt][i] = nd;
                Pi[nxt][i] = t == coor ? p : Pi[cur][q * nt + t];
                if (t == 0) Pt[nxt][k] = Ct[j];
            }
            __syncthreads();
            cur = nxt;
            nb = nk;
        }
        if (mode == KB_HARD) {
            for (int t = lane; t < nt; t += WAVE) out_idx[b * nt + t] = Pi[cur][t];
        } else if (mode == KB_LIST) {
            for (int i = lane; i < K * nt; i += WAVE) out_idx[b * K * nt + i] = i < nb * nt ? Pi[cur][i] : -1;
            if (lane == 0) out_count[b] = nb;
        } else {
            // max-log LLRs on the ORIGINAL y and H: metric = norm(y - H x)**2 (sqrt, then squared, as the reference)
            for (int k = lane; k < nb; k += WAVE) {
                double s = 0.0;
                for (int r = 0; r < nr; r++) {
                    double2 hx = make_double2(0.0, 0.0);
                    for (int t = 0; t < nt; t++) {
                        const double2 pr = cmul(Hb[r * nt + t], c[Pi[cur][k * nt + t]]);
                        hx.x += pr.x;
                        hx.y += pr.y;
                    }
                    s += abs2(csub(yb[r], hx));
                }
                const double n = sqrt(s);
                Ct[k] = n * n;
            }
            __syncthreads();
            const int nbt = nt * nbits;
            for (int i = lane; i < nbt; i += WAVE) {
                const int t = i / nbits, sh = nbits - 1 - (i - t * nbits);
                double mn[2] = {INFINITY, INFINITY};
                for (int k = 0; k < nb; k++) {
                    const int bit = (Pi[cur][k * nt + t] >> sh) & 1;
                    const double v = Ct[k];
                    if (mn[bit] == mn[bit] && (v != v || v < mn[bit])) mn[bit] = v;   // NumPy's min: NaN propagates
                }
                out_llr[b * nbt + i] = -(mn[0] - mn[1]) / (2.0 * noise_var);
            }
        }
        __syncthreads();
    }
}

bool kbest_forced_general() { return mode_of(Switch::kbest_path) == 1; }   // cpx_kbest_set_path / CPX_KBEST_PATH

int grid_for(int64_t B) { return int(B < 1048576 ? B : 1048576); }

// K clipped to what the search can ever hold (m^nt survivors), saturating
int kbest_effective_K(int K, int m, int nt) {
    int64_t cap = 1;
    for (int t = 0; t < nt && cap < K; t++) cap *= m;
    return int(cap < K ? cap : K);
}

int kbest_run(const cpx_modem *md, const double *d_y, const double *d_h, int h_batched, int64_t B, int nr, int nt, int K, int mode,
              double noise_var, int32_t *d_idx, double *d_llr, int32_t *d_count, void *stream) {
    const char *what = "kbest";
    if (int rc = mimo_check(md, B, nr, nt, what)) return rc;
    CPX_REQUIRE(nt <= nr, CPX_EINVAL, "h has more columns than rows");
    CPX_REQUIRE(K >= 1, CPX_EINVAL, "kbest: K must be a positive integer");
    if (B == 0) return CPX_OK;
    const int m = md->M, Ke = kbest_effective_K(K, m, nt);
    CPX_REQUIRE(int64_t(Ke) * m < MAX_HYP, CPX_ELIMIT, "kbest: K * m above 2^31 children");
    hipStream_t st = pick_stream(stream);
    const KbLayout L = kb_layout(nr, nt, Ke, m);
    const double2 *y = reinterpret_cast<const double2 *>(d_y), *H = reinterpret_cast<const double2 *>(d_h);
    const double2 *c = reinterpret_cast<const double2 *>(md->d_const);
    const int64_t hs = h_batched ? int64_t(nr) * nt : 0;
    if (L.bytes <= LDS_MAX && !kbest_forced_general()) {
        hipLaunchKernelGGL(kbest_kernel<false>, dim3(grid_for(B)), dim3(WAVE), L.bytes, st, y, H, hs, B, nr, nt, c, m, md->nbits, Ke, L,
                           (char *)nullptr, mode, noise_var, d_idx, d_llr, d_count);
        CPX_HIP(hipGetLastError());
        note_kernel("kbest_kernel<lds> (K %d, m %d, %dx%d)", Ke, m, nr, nt);
        return CPX_OK;
    }
    Scratch sc;
    int64_t grid = B < 2048 ? B : 2048;
    const int64_t budget = (int64_t(1) << 31) / int64_t(L.bytes);   // at most 2 GB of workspace
    if (grid > budget) grid = budget > 0 ? budget : 1;
    char *ws = nullptr;
    if (int rc = sc.get(st, Slot::kbest_state, size_t(grid) * L.bytes, &ws)) return rc;
    hipLaunchKernelGGL(kbest_kernel<true>, dim3(int(grid)), dim3(WAVE), 0, st, y, H, hs, B, nr, nt, c, m, md->nbits, Ke, L,
                       ws, mode, noise_var, d_idx, d_llr, d_count);
    CPX_HIP(hipGetLastError());
    note_kernel("kbest_kernel<global> (K %d, m %d, %dx%d)", Ke, m, nr, nt);
    return CPX_OK;
}

// ---- best-first (soft output) -----------------------------------------------------------------------------------------------
// The stack search of commpy/modulation.py:422-565.  Stack i (0 <= i < nr) holds nodes of depth d = nr - i: the symbols of
// positions i..nr-1.  A stack is an array of records sorted by metric (insertion after equal metrics, bisect.insort); a
// record is 8-byte words {metric, parent metric, int32 rank among its siblings, int32 symbols[d]}, so that a node's next
// sibling is found again by re-evaluating its parent's m children (one per lane) and selecting rank + 1.  Stack i never
// holds more than cap[i] = min(stack_size[i-1] + 1, m^d) records (one pop and at most two pushes per iteration, each tree
// node pushed at most once); stack 0 holds at most the one leaf of an iteration.
constexpr int BF_MAXNR = 64;

struct BfLayout {
    int64_t off[BF_MAXNR];    // byte offset of stack i's records
    int32_t cap[BF_MAXNR];    // capacity of stack i (records)
    int32_t keep[BF_MAXNR];   // stack i is truncated to keep[i] records after each iteration (stack_size[i-1]; keep[0] = 0)
    size_t A, counter, cm, mapsym, cnt, cur, sel, bytes;
    int64_t max_iter;         // sum_{c=1..nr} m^c, saturated: the number of tree nodes, a hard cap on the iterations
};

__host__ __device__ inline int bf_words(int d) { return 2 + (d + 2) / 2; }   // record of a depth-d node, 8-byte words

// m^e saturated at `limit`
int64_t pow_sat(int64_t m, int e, int64_t limit) {
    int64_t r = 1;
    for (int i = 0; i < e; i++) {
        if (r > limit / m) return limit;
        r *= m;
    }
    return r < limit ? r : limit;
}

// false: the state of one vector exceeds what the engine can address (a stack of over 2^31 records or 2^40 bytes)
bool bf_layout(int nr, int nt, int m, int nbits, const int32_t *stack_size, BfLayout *L) {
    memset(L, 0, sizeof(*L));
    size_t o = 0;
    auto take = [&](size_t n, size_t al) { o = (o + al - 1) / al * al; size_t r = o; o += n; return r; };
    L->A = take(16 * size_t(nr) * (nt + 1), 16);
    L->counter = take(8 * size_t(nr) * nbits, 8);
    L->cm = take(8 * size_t(m), 8);
    L->cur = take(8 * size_t(bf_words(nr)), 8);
    L->sel = take(16, 8);
    L->mapsym = take(4 * size_t(nr), 4);
    L->cnt = take(4 * size_t(nr), 4);
    for (int i = 0; i < nr; i++) {
        const int64_t s = i == 0 ? 0 : stack_size[i - 1];
        const int64_t cap = i == 0 ? 1 : pow_sat(m, nr - i, s + 1);
        if (cap > INT32_MAX) return false;
        L->cap[i] = int32_t(cap);
        L->keep[i] = int32_t(s < cap ? s : cap);
        L->off[i] = int64_t(take(8 * size_t(cap) * bf_words(nr - i), 8));
        if (o > (size_t(1) << 40)) return false;
    }
    L->bytes = (o + 15) / 16 * 16;
    int64_t total = 0;
    for (int c = 1; c <= nr; c++) {
        const int64_t t = pow_sat(m, c, INT64_MAX);
        total = t > INT64_MAX - total ? INT64_MAX : total + t;
    }
    L->max_iter = total;
    return true;
}

// NumPy's maximum / minimum: a NaN operand propagates
__device__ __forceinline__ double np_max(double a, double b) { return a != a ? a : (b != b ? b : (b > a ? b : a)); }
__device__ __forceinline__ double np_min(double a, double b) { return a != a ? a : (b != b ? b : (b < a ? b : a)); }

__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
    for (int off = WAVE / 2; off >= 1; off >>= 1) v = np_max(v, __shfl_xor(v, off));
    return v;
}

__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
    for (int off = WAVE / 2; off >= 1; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

template <bool GLOBAL>
__global__ __launch_bounds__(WAVE) void best_first_kernel(const double2 *__restrict__ y, const double2 *__restrict__ H, int64_t hstride,
                                                          int64_t B, int nr, int nt, const double2 *__restrict__ c, int m, int nbits,
                                                          const uint8_t *__restrict__ labels, double llr_max, BfLayout L, char *ws,
                                                          double *__restrict__ out_llr, int32_t *__restrict__ out_iters) {
    extern __shared__ double2 lds_bf[];
    char *base = GLOBAL ? ws + size_t(blockIdx.x) * L.bytes : reinterpret_cast<char *>(lds_bf);
    double2 *A = reinterpret_cast<double2 *>(base + L.A);
    double *counter = reinterpret_cast<double *>(base + L.counter);
    double *cm = reinterpret_cast<double *>(base + L.cm);
    uint64_t *cur = reinterpret_cast<uint64_t *>(base + L.cur);
    double *sel_m = reinterpret_cast<double *>(base + L.sel);
    int32_t *sel_q = reinterpret_cast<int32_t *>(base + L.sel + 8);
    int32_t *mapsym = reinterpret_cast<int32_t *>(base + L.mapsym);
    int32_t *cnt = reinterpret_cast<int32_t *>(base + L.cnt);
    const int lane = threadIdx.x;
    const int w = nt + 1;
    const int nbt = nr * nbits;
    auto stack = [&](int i) { return reinterpret_cast<uint64_t *>(base + L.off[i]); };
    auto rec_metric = [](const uint64_t *r) { return __longlong_as_double((long long)r[0]); };
    auto rec_ints = [](uint64_t *r) { return reinterpret_cast<int32_t *>(r + 2); };   // [0] rank, [1..d] symbols
    auto label = [&](int sym, int b) -> int { return labels ? labels[sym * nbits + b] != 0 : (sym >> (nbits - 1 - b)) & 1; };

    // metrics of the m children of the depth-(cd-1) node {parent symbols `ps`, metric pm} into cm[], then the child of rank r
    // in (metric, index) order -- NaN last, equal metrics to the lowest index: -> (*q, *met), uniform
    auto select_child = [&](int cd, const int32_t *ps, double pm, int r, int *q_out, double *met_out) {
        const int row = nr - cd, col0 = nt - cd;
        const double2 *Ar = A + row * w;
        double lm = NAN;
        int li = INT32_MAX;
        for (int q = lane; q < m; q += WAVE) {
            double2 s = cmul(Ar[col0], c[q]);
            for (int k = 1; k < cd; k++) {
                const double2 p = cmul(Ar[col0 + k], c[ps[k - 1]]);
                s.x += p.x;
                s.y += p.y;
            }
            const double2 e = csub(Ar[nt], s);
            const double a = hypot(e.x, e.y);
            const double met = a * a + pm;
            cm[q] = met;
            if (li == INT32_MAX || key_less<false>(met, q, lm, li)) { lm = met; li = q; }
        }
        __syncthreads();
        if (r == 0) {
            long long li64 = li == INT32_MAX ? 0x7fffffffffffffffll : li;
            wave_argmin<false>(lm, li64);
            *q_out = int(li64);
            *met_out = lm;
            return;
        }
        for (int q = lane; q < m; q += WAVE) {
            const double mq = cm[q];
            int rank = 0;
            for (int o = 0; o < m; o++) rank += key_less<false>(cm[o], o, mq, q);
            if (rank == r) { *sel_q = q; *sel_m = mq; }
        }
        __syncthreads();
        *q_out = *sel_q;
        *met_out = *sel_m;
        __syncthreads();
    };

    // insert a depth-(nr-i) record {met, pm, rank, [q, ps[0..d-2]]} into stack i after the records of metric <= met.
    // false: the stack is full, which the capacity bound excludes (the vector is then reported, not written)
    auto insert = [&](int i, double met, double pm, int rank, int q, const int32_t *ps) -> bool {
        const int d = nr - i, W = bf_words(d), n = cnt[i];
        if (n >= L.cap[i]) return false;
        uint64_t *st = stack(i);
        int le = 0;
        for (int k = lane; k < n; k += WAVE) le += rec_metric(st + size_t(k) * W) <= met;
        const int pos = wave_sum(le);
        const int64_t lo = int64_t(pos) * W;
        for (int64_t hi = int64_t(n) * W; hi > lo; hi -= WAVE) {   // shift [pos, n) one record up, top chunk first
            const int64_t j = hi - WAVE + lane;
            const bool mv = j >= lo;
            const uint64_t v = mv ? st[j] : 0;
            __syncthreads();
            if (mv) st[j + W] = v;
            __syncthreads();
        }
        if (lane == 0) {
            uint64_t *r = st + size_t(pos) * W;
            r[0] = (uint64_t)__double_as_longlong(met);
            r[1] = (uint64_t)__double_as_longlong(pm);
            int32_t *ri = rec_ints(r);
            ri[0] = rank;
            ri[1] = q;
            for (int k = 0; k + 1 < d; k++) ri[2 + k] = ps[k];
            cnt[i] = n + 1;
        }
        __syncthreads();
        return true;
    };

    for (int64_t b = blockIdx.x; b < B; b += gridDim.x) {
        const double2 *Hb = H + b * hstride, *yb = y + b * nr;
        for (int i = lane; i < nr * w; i += WAVE) {
            const int r = i / w, j = i - r * w;
            A[i] = j < nt ? Hb[r * nt + j] : yb[r];
        }
        for (int e = lane; e < nbt; e += WAVE) counter[e] = INFINITY;
        for (int i = lane; i < nr; i += WAVE) cnt[i] = 0;
        __syncthreads();
        householder_qr(A, nr, w, nr, lane);   // nr <= nt: R is [nr][nt], upper trapezoidal
        bool have_map = false, bad = false;
        double map = INFINITY;
        // the best child of the root goes to the last stack unconditionally
        {
            int q;
            double met;
            select_child(1, nullptr, 0.0, 0, &q, &met);
            bad |= !insert(nr - 1, met, 0.0, 0, q, nullptr);
        }
        int64_t iter = 0;
        for (;;) {
            bool any = false;
            for (int i = 1; i < nr; i++) any |= cnt[i] > 0;
            if (!any || bad) break;
            if (++iter > L.max_iter) { bad = true; break; }
            for (int i = 1; i < nr; i++) {   // pop stack i, push its next sibling back and its best child into stack i - 1
                const int n = cnt[i];
                if (n == 0) continue;
                const int d = nr - i, W = bf_words(d);
                uint64_t *st = stack(i);
                for (int k = lane; k < W; k += WAVE) cur[k] = st[k];
                __syncthreads();
                for (int64_t lo = 0; lo < int64_t(n - 1) * W; lo += WAVE) {   // pop the front: shift [1, n) one record down
                    const int64_t j = lo + lane;
                    const bool mv = j < int64_t(n - 1) * W;
                    const uint64_t v = mv ? st[j + W] : 0;
                    __syncthreads();
                    if (mv) st[j] = v;
                    __syncthreads();
                }
                if (lane == 0) cnt[i] = n - 1;
                __syncthreads();
                const double node_met = rec_metric(cur), node_pm = __longlong_as_double((long long)cur[1]);
                const int32_t *ci = rec_ints(cur);
                const int rank = ci[0];
                const int32_t *syms = ci + 1;   // positions i..nr-1
                // search radius: inf before the first leaf, else max(max(counter[:i]), max(counter[i:] where the bits differ
                // from the MAP's)), an empty selection counting as +inf
                double radius = INFINITY;
                if (have_map) {
                    double lo_max = -INFINITY, a2 = -INFINITY;
                    bool differ = false;
                    for (int e = lane; e < nbt; e += WAVE) {
                        const int t = e / nbits, bb = e - t * nbits;
                        if (t < i) lo_max = np_max(lo_max, counter[e]);
                        else if (label(syms[t - i], bb) != label(mapsym[t], bb)) { a2 = np_max(a2, counter[e]); differ = true; }
                    }
                    lo_max = wave_max(lo_max);
                    a2 = __any(differ) ? wave_max(a2) : INFINITY;
                    radius = a2 > lo_max ? a2 : lo_max;   // Python's max(a, b)
                }
                if (rank + 1 < m) {
                    int q;
                    double met;
                    select_child(d, syms + 1, node_pm, rank + 1, &q, &met);
                    if (met <= radius) bad |= !insert(i, met, node_pm, rank + 1, q, syms + 1);
                }
                {
                    int q;
                    double met;
                    select_child(d + 1, syms, node_met, 0, &q, &met);
                    if (met <= radius) bad |= !insert(i - 1, met, node_met, 0, q, syms);
                }
            }
            if (cnt[0] > 0) {   // the leaf of this iteration
                const uint64_t *leaf = stack(0);
                const double lm = rec_metric(leaf);
                const int32_t *ls = reinterpret_cast<const int32_t *>(leaf + 2) + 1;
                const bool better = lm < map;
                const double with = better ? map : lm;
                if (better) {
                    map = lm;
                    have_map = true;
                    for (int t = lane; t < nr; t += WAVE) mapsym[t] = ls[t];
                }
                const double lo = map - llr_max, hi = map + llr_max;
                for (int e = lane; e < nbt; e += WAVE) counter[e] = np_min(np_max(np_min(counter[e], with), lo), hi);
                __syncthreads();
            }
            if (lane == 0)
                for (int i = 0; i < nr; i++) cnt[i] = cnt[i] < L.keep[i] ? cnt[i] : L.keep[i];
            __syncthreads();
        }
        for (int e = lane; e < nbt; e += WAVE) {
            double v = NAN;
            if (have_map && !bad) {
                const int t = e / nbits;
                v = (map - counter[e]) * (label(mapsym[t], e - t * nbits) ? 1.0 : -1.0);
            }
            out_llr[b * nbt + e] = v;
        }
        if (out_iters && lane == 0) out_iters[b] = bad ? -1 : int32_t(iter < INT32_MAX ? iter : INT32_MAX);
        __syncthreads();
    }
}

bool bf_forced_general() { return mode_of(Switch::best_first_path) == 1; }   // cpx_best_first_set_path / CPX_BEST_FIRST_PATH

int bf_run(const cpx_modem *md, const double *d_y, const double *d_h, int h_batched, int64_t B, int nr, int nt,
           const int32_t *stack_size, double llr_max, const uint8_t *d_labels, double *d_llr, int32_t *d_iters, void *stream) {
    const char *what = "best_first";
    if (int rc = mimo_check(md, B, nr, nt, what)) return rc;
    CPX_REQUIRE(nr >= 2, CPX_EINVAL, "best_first: need at least 2 receive antennas (h has %d rows)", nr);
    CPX_REQUIRE(nr <= nt, CPX_EINVAL, "best_first: h has more rows than columns (%d > %d): no leaf can be reached", nr, nt);
    CPX_REQUIRE(nr <= BF_MAXNR, CPX_ELIMIT, "best_first: %d receive antennas above the engine's %d", nr, BF_MAXNR);
    CPX_REQUIRE(stack_size, CPX_EINVAL, "best_first: null stack_size");
    for (int i = 0; i + 1 < nr; i++)
        CPX_REQUIRE(stack_size[i] >= 1, CPX_EINVAL, "best_first: stack_size[%d] = %d; every stack must hold a node", i, stack_size[i]);
    const int m = md->M;
    CPX_REQUIRE(m >= 2 && (m & (m - 1)) == 0, CPX_EINVAL, "best_first: the constellation length %d is not a power of two", m);
    BfLayout L;
    CPX_REQUIRE(bf_layout(nr, nt, m, md->nbits, stack_size, &L), CPX_ELIMIT, "best_first: the stacks of one vector exceed the engine's state limit");
    if (B == 0) return CPX_OK;
    hipStream_t st = pick_stream(stream);
    const double2 *y = reinterpret_cast<const double2 *>(d_y), *H = reinterpret_cast<const double2 *>(d_h);
    const double2 *c = reinterpret_cast<const double2 *>(md->d_const);
    const int64_t hs = h_batched ? int64_t(nr) * nt : 0;
    if (L.bytes <= LDS_MAX && !bf_forced_general()) {
        hipLaunchKernelGGL(best_first_kernel<false>, dim3(grid_for(B)), dim3(WAVE), L.bytes, st, y, H, hs, B, nr, nt, c, m, md->nbits,
                           d_labels, llr_max, L, (char *)nullptr, d_llr, d_iters);
        CPX_HIP(hipGetLastError());
        note_kernel("best_first_kernel<lds> (m %d, %dx%d, %zu B per vector)", m, nr, nt, L.bytes);
        return CPX_OK;
    }
    CPX_REQUIRE(L.bytes <= (size_t(1) << 31), CPX_ELIMIT, "best_first: %zu bytes of state per vector above the 2 GB workspace", L.bytes);
    Scratch sc;
    int64_t grid = B < 2048 ? B : 2048;
    const int64_t budget = (int64_t(1) << 31) / int64_t(L.bytes);   // at most 2 GB of workspace
    if (grid > budget) grid = budget > 0 ? budget : 1;
    char *ws = nullptr;
    if (int rc = sc.get(st, Slot::best_first_state, size_t(grid) * L.bytes, &ws)) return rc;
    hipLaunchKernelGGL(best_first_kernel<true>, dim3(int(grid)), dim3(WAVE), 0, st, y, H, hs, B, nr, nt, c, m, md->nbits, d_labels,
                       llr_max, L, ws, d_llr, d_iters);
    CPX_HIP(hipGetLastError());
    note_kernel("best_first_kernel<global> (m %d, %dx%d, %zu B per vector)", m, nr, nt, L.bytes);
    return CPX_OK;
}

}  // namespace

extern "C" {

int cpx_kbest_set_path(const char *mode) { return set_mode(Switch::kbest_path, mode); }

int cpx_mimo_ml_dev(const cpx_modem *md, const double *d_y, const double *d_h, int h_batched, int64_t B, int nr, int nt,
                    int32_t *d_idx, void *stream) {
    CPX_TRACE("cpx_mimo_ml_dev");
    if (int rc = mimo_check(md, B, nr, nt, "mimo_ml")) return rc;
    const int m = md->M, lgm = md->nbits;
    CPX_REQUIRE(int64_t(lgm) * nt <= 31, CPX_EINVAL, "mimo_ml: m^nt above 2^31 hypotheses per vector");
    if (B == 0) return CPX_OK;
    const size_t base = 16 * (size_t(nr) * nt + nr + size_t(WAVE) * nr), tab = 16 * size_t(nt) * m * nr;
    CPX_REQUIRE(base <= LDS_MAX, CPX_ELIMIT, "mimo_ml: %d receive antennas exceed the kernel's LDS", nr);
    hipStream_t st = pick_stream(stream);
    const double2 *y = reinterpret_cast<const double2 *>(d_y), *H = reinterpret_cast<const double2 *>(d_h);
    const double2 *c = reinterpret_cast<const double2 *>(md->d_const);
    const int64_t hs = h_batched ? int64_t(nr) * nt : 0;
    const bool use_tab = base + tab <= LDS_MAX;
    if (use_tab)
        hipLaunchKernelGGL(mimo_ml_kernel<true>, dim3(grid_for(B)), dim3(WAVE), base + tab, st, y, H, hs, B, nr, nt, c, m, lgm, d_idx);
    else
        hipLaunchKernelGGL(mimo_ml_kernel<false>, dim3(grid_for(B)), dim3(WAVE), base, st, y, H, hs, B, nr, nt, c, m, lgm, d_idx);
    CPX_HIP(hipGetLastError());
    note_kernel("mimo_ml_kernel<%s> (m %d, %dx%d)", use_tab ? "table" : "direct", m, nr, nt);
    return CPX_OK;
}

int cpx_mimo_ml(const cpx_modem *md, const double *y, const double *h, int h_batched, int64_t B, int nr, int nt, int32_t *idx) {
    CPX_TRACE("cpx_mimo_ml");
    if (int rc = mimo_host_check(y, h, B, nr, nt, idx)) return rc;
    HostStage s;
    const double *dy, *dh;
    int32_t *d_idx;
    const size_t n = 4 * size_t(B) * nt;
    int rc;
    if ((rc = mimo_in(s, y, h, h_batched, B, nr, nt, &dy, &dh)) || (rc = s.out(n, &d_idx)) ||
        (rc = cpx_mimo_ml_dev(md, dy, dh, h_batched, B, nr, nt, d_idx, s.st)))
        return rc;
    return s.get(idx, d_idx, n);
}

int cpx_kbest_hard_dev(const cpx_modem *md, const double *d_y, const double *d_h, int h_batched, int64_t B, int nr, int nt, int K,
                       int32_t *d_idx, void *stream) {
    CPX_TRACE("cpx_kbest_hard_dev");
    return kbest_run(md, d_y, d_h, h_batched, B, nr, nt, K, KB_HARD, 0.0, d_idx, nullptr, nullptr, stream);
}

int cpx_kbest_hard(const cpx_modem *md, const double *y, const double *h, int h_batched, int64_t B, int nr, int nt, int K, int32_t *idx) {
    CPX_TRACE("cpx_kbest_hard");
    if (int rc = mimo_host_check(y, h, B, nr, nt, idx)) return rc;
    HostStage s;
    const double *dy, *dh;
    int32_t *d_idx;
    const size_t n = 4 * size_t(B) * nt;
    int rc;
    if ((rc = mimo_in(s, y, h, h_batched, B, nr, nt, &dy, &dh)) || (rc = s.out(n, &d_idx)) ||
        (rc = cpx_kbest_hard_dev(md, dy, dh, h_batched, B, nr, nt, K, d_idx, s.st)))
        return rc;
    return s.get(idx, d_idx, n);
}

int cpx_kbest_soft_dev(const cpx_modem *md, const double *d_y, const double *d_h, int h_batched, int64_t B, int nr, int nt, int K,
                       double noise_var, double *d_llr, void *stream) {
    CPX_TRACE("cpx_kbest_soft_dev");
    return kbest_run(md, d_y, d_h, h_batched, B, nr, nt, K, KB_SOFT, noise_var, nullptr, d_llr, nullptr, stream);
}

int cpx_kbest_soft(const cpx_modem *md, const double *y, const double *h, int h_batched, int64_t B, int nr, int nt, int K,
                   double noise_var, double *llr) {
    CPX_TRACE("cpx_kbest_soft");
    if (int rc = mimo_host_check(y, h, B, nr, nt, llr)) return rc;
    HostStage s;
    const double *dy, *dh;
    double *d_llr;
    const size_t n = 8 * size_t(B) * nt * (md ? size_t(md->nbits) : 0);
    int rc;
    if ((rc = mimo_in(s, y, h, h_batched, B, nr, nt, &dy, &dh)) || (rc = s.out(n, &d_llr)) ||
        (rc = cpx_kbest_soft_dev(md, dy, dh, h_batched, B, nr, nt, K, noise_var, d_llr, s.st)))
        return rc;
    return s.get(llr, d_llr, n);
}

int cpx_kbest_list_dev(const cpx_modem *md, const double *d_y, const double *d_h, int h_batched, int64_t B, int nr, int nt, int K,
                       int32_t *d_cand, int32_t *d_count, void *stream) {
    CPX_TRACE("cpx_kbest_list_dev");
    return kbest_run(md, d_y, d_h, h_batched, B, nr, nt, K, KB_LIST, 0.0, d_cand, nullptr, d_count, stream);
}

int cpx_kbest_list(const cpx_modem *md, const double *y, const double *h, int h_batched, int64_t B, int nr, int nt, int K,
                   int32_t *cand, int32_t *count) {
    CPX_TRACE("cpx_kbest_list");
    CPX_REQUIRE(md && K >= 1 && nt >= 1, CPX_EINVAL, "kbest: null modem, K < 1 or nt < 1");
    const size_t n = 4 * size_t(B) * size_t(kbest_effective_K(K, md->M, nt)) * nt;
    if (int rc = mimo_host_check(y, h, B, nr, nt, cand)) return rc;
    HostStage s;
    const double *dy, *dh;
    int32_t *d_cand, *d_count;
    int rc;
    if ((rc = mimo_in(s, y, h, h_batched, B, nr, nt, &dy, &dh)) || (rc = s.out(n, &d_cand)) ||
        (rc = s.out(4 * size_t(B), &d_count)) ||
        (rc = cpx_kbest_list_dev(md, dy, dh, h_batched, B, nr, nt, K, d_cand, d_count, s.st)) || (rc = s.get(cand, d_cand, n)))
        return rc;
    return count ? s.get(count, d_count, 4 * size_t(B)) : CPX_OK;
}

}  // extern "C"

extern "C" {

int cpx_best_first_set_path(const char *mode) { return set_mode(Switch::best_first_path, mode); }

int cpx_best_first_dev(const cpx_modem *md, const double *d_y, const double *d_h, int h_batched, int64_t B, int nr, int nt,
                       const int32_t *stack_size, double llr_max, const uint8_t *d_labels, double *d_llr, int32_t *d_iters,
                       void *stream) {
    CPX_TRACE("cpx_best_first_dev");
    return bf_run(md, d_y, d_h, h_batched, B, nr, nt, stack_size, llr_max, d_labels, d_llr, d_iters, stream);
}

int cpx_best_first(const cpx_modem *md, const double *y, const double *h, int h_batched, int64_t B, int nr, int nt,
                   const int32_t *stack_size, double llr_max, const uint8_t *labels, double *llr) {
    CPX_TRACE("cpx_best_first");
    CPX_REQUIRE(md, CPX_EINVAL, "best_first: null modem");
    const int nbits = md->nbits;
    if (labels)
        for (int i = 0; i < md->M * nbits; i++)
            CPX_REQUIRE(labels[i] <= 1, CPX_EINVAL, "best_first: label table entry %d is %d, not 0 or 1", i, int(labels[i]));
    if (int rc = mimo_host_check(y, h, B, nr, nt, llr)) return rc;
    HostStage s;
    const double *dy, *dh;
    uint8_t *d_labels = nullptr;
    double *d_llr;
    int32_t *d_iters;
    std::vector<int32_t> iters(size_t(B > 0 ? B : 0));
    const size_t n = 8 * size_t(B) * nr * nbits;
    int rc;
    if ((rc = mimo_in(s, y, h, h_batched, B, nr, nt, &dy, &dh)) ||
        (labels && B > 0 && (rc = s.in(labels, size_t(md->M) * nbits, &d_labels))) || (rc = s.out(n, &d_llr)) ||
        (rc = s.out(4 * iters.size(), &d_iters)) ||
        (rc = cpx_best_first_dev(md, dy, dh, h_batched, B, nr, nt, stack_size, llr_max, d_labels, d_llr, d_iters, s.st)) ||
        (rc = s.get(llr, d_llr, n)) || (rc = s.get(iters.data(), d_iters, 4 * iters.size())))
        return rc;
    for (int64_t b = 0; b < B; b++)
        CPX_REQUIRE(iters[b] >= 0, CPX_EHIP, "best_first: vector %lld hit the search's iteration cap (an engine fault)", (long long)b);
    return CPX_OK;
}

}  // extern "C"
