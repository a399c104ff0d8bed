// Max-log list MIMO detection with a-priori LLRs, and the detector / decoder exchange of iterative detection and decoding
// (commpy/links.py:345-407 with a list detector as `detector`).  float64 throughout, -ffp-contract=off; the
// kernels have one form only (no precision mode, no path switch).
//
// The candidate list of a vector is searched ONCE on the channel metric (cpx_kbest_list, Hochwald / ten Brink list sphere
// detection); every later pass reweighs the same list with new priors.  Per vector:
//   list_dist_kernel   d_c = norm(y - H x_c)^2 of each candidate, one thread per candidate, in the order of kbest_kernel's soft
//                      output: per receive antenna r (ascending) hx = 0 + sum_t H[r][t] x_c[t] (t ascending, complex products written
//                      out), s = 0 + sum_r |y_r - hx|^2, d = sqrt(s) * sqrt(s).  A thread owns a candidate whatever the batch, the
//                      grid or the stream, so the order never changes.  Rows past count hold +inf.
//   list_detect        (device function, shared by the two kernels below)  with La_k the prior clipped to +-clip,
//                        S_c    = 0 + sum_k b_k(c) La_k          k ascending over the bits 1 of candidate c, once per vector
//                        cost_c = d_c + (2 noise_var) S_c        = 2 noise_var * (d_c / (2 noise_var) + S_c): the scaled form keeps a
//                        L_k    = -(min_{b_k = 0} cost - min_{b_k = 1} cost) / (2 noise_var)     zero prior bit-identical to
//                      cpx_kbest_soft; clipped to +-clip, an empty side counting as +inf.  A NaN among the vector's distances
//                      (i.e. in y or H) or priors makes all its LLRs NaN.
//   list_llr_kernel    prior (nullable) -> posterior
//   idd_exchange_kernel  ext = dec_out - dec_in, posterior with prior ext, dec_in <- posterior - ext (last: posterior)
// A group of G lanes serves one vector (G = the power of two holding max(nt nb, min(Ke, 64)), so 64 / G vectors per wave): lane g
// builds the cost of candidates g, g + G, ... into LDS, then lane k < nt nb takes the two minima of bit k over the list.
#include "cpx_internal.h"

#include <cmath>

using namespace cpx;

namespace {

constexpr int WAVE = 64;
constexpr int MAX_BITS = 64;               // bits per vector: one lane each, and one uint64_t of labels per candidate
constexpr size_t LDS_MAX = 64 * 1024;
constexpr int DIST_BLOCK = 256;
constexpr int MAX_GRID = 16384;            // workgroups of a grid-striding launch

__global__ __launch_bounds__(DIST_BLOCK) void list_dist_kernel(const double2 *__restrict__ y, const double2 *__restrict__ H,
                                                               int64_t hstride, int64_t B, int nr, int nt,
                                                               const double2 *__restrict__ c, int m, const int32_t *__restrict__ cand,
                                                               const int32_t *__restrict__ count, int Ke, double *__restrict__ dist) {
    const int64_t total = B * Ke;
    for (int64_t i = int64_t(blockIdx.x) * DIST_BLOCK + threadIdx.x; i < total; i += int64_t(gridDim.x) * DIST_BLOCK) {
        const int64_t b = i / Ke;
        const int k = int(i - b * Ke);
        double d = INFINITY;
        if (k < count[b]) {
            const double2 *Hb = H + b * hstride, *yb = y + b * nr;
            const int32_t *x = cand + i * nt;
            bool ok = true;
            for (int t = 0; t < nt; t++) ok &= x[t] >= 0 && x[t] < m;
            if (ok) {
                double s = 0.0;
                for (int r = 0; r < nr; r++) {
                    double hx = 0.0, hy = 0.0;
                    for (int t = 0; t < nt; t++) {
                        const double2 h = Hb[r * nt + t], p = c[x[t]];
                        hx += h.x * p.x - h.y * p.y;
                        hy += h.x * p.y + h.y * p.x;
                    }
                    const double ex = yb[r].x - hx, ey = yb[r].y - hy;
                    s += ex * ex + ey * ey;
                }
                const double n = sqrt(s);
                d = n * n;
            } else {
                d = NAN;                   // an index outside the constellation: the vector's LLRs come out NaN
            }
        }
        dist[i] = d;
    }
}

__device__ __forceinline__ double clamp_keep_nan(double v, double lim) { return v > lim ? lim : (v < -lim ? -lim : v); }

// The detector of one vector by the G lanes of its group (gl = lane in the group, grp = group in the wave); called by every
// lane of the wave (two barriers).  `prior` is lane gl's bit (ignored unless has_prior and gl < nbt), cnt = 0 for a group
// without a vector.  Returns the posterior of bit gl (gl < nbt).
__device__ __forceinline__ double list_detect(const int32_t *cand_v, int cnt, const double *dist_v, int gl, int G, int grp, int nt,
                                              int nbits, bool has_prior, double prior, double two_nv, double clip, double *s_la,
                                              double *s_cost, uint64_t *s_word) {
    const int nbt = nt * nbits;
    bool bad = false;
    if (has_prior && gl < nbt) {
        const double la = clamp_keep_nan(prior, clip);
        s_la[gl] = la;
        bad = la != la;
    }
    __syncthreads();
    for (int k = gl; k < cnt; k += G) {
        const double d = dist_v[k];
        uint64_t word = 0;
        double S = 0.0;
        for (int t = 0; t < nt; t++) {
            const int idx = cand_v[k * nt + t];
            for (int j = 0; j < nbits; j++) {
                if ((idx >> (nbits - 1 - j)) & 1) {
                    const int bit = t * nbits + j;
                    word |= uint64_t(1) << bit;
                    if (has_prior) S += s_la[bit];
                }
            }
        }
        bad |= d != d;
        s_cost[k] = has_prior ? d + two_nv * S : d;
        s_word[k] = word;
    }
    const uint64_t votes = __ballot(bad);
    const uint64_t mine = G == WAVE ? votes : (votes >> (grp * G)) & ((uint64_t(1) << G) - 1);
    __syncthreads();
    double mn[2] = {INFINITY, INFINITY};
    if (gl < nbt)
        for (int k = 0; k < cnt; k++) {
            const int bit = int(s_word[k] >> gl) & 1;
            const double v = s_cost[k];
            if (v < mn[bit]) mn[bit] = v;
        }
    const double L = clamp_keep_nan(-(mn[0] - mn[1]) / two_nv, clip);
    return mine ? NAN : L;
}

// EXCHANGE = false: io = prior (nullable) in, out = posterior.  EXCHANGE = true: io = the decoder's input (read, then rewritten),
// dec_out = the decoder's output.
template <bool EXCHANGE>
__global__ __launch_bounds__(WAVE) void list_llr_kernel(const int32_t *__restrict__ cand, const int32_t *__restrict__ count,
                                                        const double *__restrict__ dist, int64_t B, int nt, int nbits, int Ke, int G,
                                                        double *io, const double *__restrict__ dec_out, double two_nv, double clip,
                                                        int last, double *__restrict__ out) {
    extern __shared__ double lds_idd[];
    const int lane = threadIdx.x, vpw = WAVE / G, grp = lane / G, gl = lane - grp * G, nbt = nt * nbits;
    double *s_la = lds_idd + grp * MAX_BITS;
    double *s_cost = lds_idd + vpw * MAX_BITS + size_t(grp) * Ke;
    uint64_t *s_word = reinterpret_cast<uint64_t *>(lds_idd + vpw * MAX_BITS + size_t(vpw) * Ke) + size_t(grp) * Ke;
    for (int64_t base = int64_t(blockIdx.x) * vpw; base < B; base += int64_t(gridDim.x) * vpw) {
        const int64_t b = base + grp;
        const bool live = b < B, act = live && gl < nbt;
        int cnt = live ? count[b] : 0;
        cnt = cnt < 0 ? 0 : (cnt > Ke ? Ke : cnt);
        double prior = 0.0;
        if (EXCHANGE) {
            if (act) prior = dec_out[b * nbt + gl] - io[b * nbt + gl];
        } else if (act && io) {
            prior = io[b * nbt + gl];
        }
        const double L = list_detect(cand + (live ? b : 0) * Ke * nt, cnt, dist + (live ? b : 0) * Ke, gl, G, grp, nt, nbits,
                                     EXCHANGE || io != nullptr, prior, two_nv, clip, s_la, s_cost, s_word);
        if (act) {
            if (EXCHANGE) io[b * nbt + gl] = last ? L : L - prior;
            else out[b * nbt + gl] = L;
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(DIST_BLOCK) void llr_sign_kernel(const double *__restrict__ llr, int64_t n, int8_t *__restrict__ bits) {
    for (int64_t i = int64_t(blockIdx.x) * DIST_BLOCK + threadIdx.x; i < n; i += int64_t(gridDim.x) * DIST_BLOCK)
        bits[i] = int8_t(__double_as_longlong(llr[i]) < 0);      // np.signbit, as ldpc_bp_decode's dec_word
}

int pow2_at_least(int v) {
    int g = 1;
    while (g < v) g <<= 1;
    return g;
}

struct ListShape { int nbt, G; size_t lds; };

// the checks the three list entry points share; B == 0 is accepted with null data
int list_check(const cpx_modem *md, int64_t B, int nt, int Ke, const char *what, ListShape *s) {
    CPX_REQUIRE(md, CPX_EINVAL, "%s: null modem", what);
    if (int rc = check_handle_device(md->device, what)) return rc;
    CPX_REQUIRE(B >= 0 && nt >= 1, CPX_EINVAL, "%s: need B >= 0 and nt >= 1", what);
    CPX_REQUIRE(Ke >= 1, CPX_EINVAL, "%s: Ke must be at least 1 (got %d)", what, Ke);
    CPX_REQUIRE(md->M == 1 << md->nbits, CPX_EINVAL, "%s: the modem does not have 2^nbits points", what);
    CPX_REQUIRE(int64_t(nt) * md->nbits <= MAX_BITS, CPX_ELIMIT, "%s: %d x %d bits per vector above the kernel's %d", what, nt,
                md->nbits, MAX_BITS);
    s->nbt = nt * md->nbits;
    s->G = pow2_at_least(s->nbt > (Ke < WAVE ? Ke : WAVE) ? s->nbt : (Ke < WAVE ? Ke : WAVE));
    s->lds = 8 * size_t(WAVE / s->G) * (MAX_BITS + 2 * size_t(Ke));
    CPX_REQUIRE(s->lds <= LDS_MAX, CPX_ELIMIT, "%s: a list of %d candidates exceeds the kernel's LDS (%zu of %zu bytes)", what, Ke,
                s->lds, LDS_MAX);
    return CPX_OK;
}

int clip_check(double noise_var, double clip, const char *what) {
    CPX_REQUIRE(clip > 0.0, CPX_EINVAL, "%s: clip must be positive (got %g)", what, clip);   // NaN fails the comparison too
    CPX_REQUIRE(noise_var > 0.0 && noise_var < INFINITY, CPX_EINVAL, "%s: noise_var must be positive and finite (got %g)", what,
                noise_var);                                                                  // inf * a zero prior sum would be NaN
    return CPX_OK;
}

int grid_of(int64_t items, int per_block) {
    const int64_t g = (items + per_block - 1) / per_block;
    return int(g < MAX_GRID ? g : MAX_GRID);
}

template <bool EXCHANGE>
int list_launch(const cpx_modem *md, const int32_t *cand, const int32_t *count, const double *dist, int64_t B, int nt, int Ke,
                double *io, const double *dec_out, double noise_var, double clip, int last, double *out, void *stream,
                const char *what) {
    ListShape s;
    if (int rc = list_check(md, B, nt, Ke, what, &s)) return rc;
    if (int rc = clip_check(noise_var, clip, what)) return rc;
    if (B == 0) return CPX_OK;
    CPX_REQUIRE(cand && count && dist && (EXCHANGE ? io && dec_out : out != nullptr), CPX_EINVAL, "%s: null pointer", what);
    const int vpw = WAVE / s.G;
    hipLaunchKernelGGL(list_llr_kernel<EXCHANGE>, dim3(grid_of(B, vpw)), dim3(WAVE), s.lds, pick_stream(stream), cand, count, dist, B,
                       nt, md->nbits, Ke, s.G, io, dec_out, 2.0 * noise_var, clip, last, out);
    CPX_HIP(hipGetLastError());
    note_kernel("%s (%d bits, Ke %d, %d vectors per wave%s)", EXCHANGE ? "idd_exchange_kernel" : "list_llr_kernel", s.nbt, Ke, vpw,
                EXCHANGE ? (last ? ", last" : "") : (io ? ", prior" : ", no prior"));
    return CPX_OK;
}

}  // namespace

extern "C" {

int cpx_mimo_list_dist_dev(const cpx_modem *md, const double *d_y, const double *d_h, int h_batched, int64_t B, int nr, int nt,
                           const int32_t *d_cand, const int32_t *d_count, int Ke, double *d_dist, void *stream) {
    CPX_TRACE("cpx_mimo_list_dist_dev");
    const char *what = "mimo_list_dist";
    ListShape s;
    if (int rc = list_check(md, B, nt, Ke, what, &s)) return rc;
    CPX_REQUIRE(nr >= 1, CPX_EINVAL, "%s: nr must be at least 1", what);
    if (B == 0) return CPX_OK;
    CPX_REQUIRE(d_y && d_h && d_cand && d_count && d_dist, CPX_EINVAL, "%s: null pointer", what);
    hipLaunchKernelGGL(list_dist_kernel, dim3(grid_of(B * Ke, DIST_BLOCK)), dim3(DIST_BLOCK), 0, pick_stream(stream),
                       reinterpret_cast<const double2 *>(d_y), reinterpret_cast<const double2 *>(d_h),
                       h_batched ? int64_t(nr) * nt : int64_t(0), B, nr, nt, reinterpret_cast<const double2 *>(md->d_const), md->M,
                       d_cand, d_count, Ke, d_dist);
    CPX_HIP(hipGetLastError());
    note_kernel("list_dist_kernel (m %d, %dx%d, Ke %d)", md->M, nr, nt, Ke);
    return CPX_OK;
}

int cpx_mimo_list_dist(const cpx_modem *md, const double *y, const double *h, int h_batched, int64_t B, int nr, int nt,
                       const int32_t *cand, const int32_t *count, int Ke, double *dist) {
    CPX_TRACE("cpx_mimo_list_dist");
    CPX_REQUIRE(md && Ke >= 1 && nt >= 1 && nr >= 1 && B >= 0, CPX_EINVAL, "mimo_list_dist: null modem, Ke < 1, nt < 1, nr < 1 or B < 0");
    CPX_REQUIRE((y && h && cand && count && dist) || B == 0, CPX_EINVAL, "mimo_list_dist: null pointer");
    if (int rc = ensure_device()) return rc;
    if (B == 0) return cpx_mimo_list_dist_dev(md, nullptr, nullptr, h_batched, 0, nr, nt, nullptr, nullptr, Ke, nullptr, nullptr);
    HostStage s;
    const double *dy, *dh;
    const int32_t *d_cand, *d_count;
    double *d_dist;
    const size_t n = 8 * size_t(B) * Ke;
    int rc;
    if ((rc = s.in(y, 16 * size_t(B) * nr, &dy)) || (rc = s.in(h, 16 * size_t(nr) * nt * (h_batched ? size_t(B) : 1), &dh)) ||
        (rc = s.in(cand, 4 * size_t(B) * Ke * nt, &d_cand)) || (rc = s.in(count, 4 * size_t(B), &d_count)) ||
        (rc = s.out(n, &d_dist)) ||
        (rc = cpx_mimo_list_dist_dev(md, dy, dh, h_batched, B, nr, nt, d_cand, d_count, Ke, d_dist, s.st)))
        return rc;
    return s.get(dist, d_dist, n);
}

int cpx_mimo_list_llr_dev(const cpx_modem *md, const int32_t *d_cand, const int32_t *d_count, const double *d_dist, int64_t B, int nt,
                          int Ke, const double *d_prior_or_null, double noise_var, double clip, double *d_llr, void *stream) {
    CPX_TRACE("cpx_mimo_list_llr_dev");
    return list_launch<false>(md, d_cand, d_count, d_dist, B, nt, Ke, const_cast<double *>(d_prior_or_null), nullptr, noise_var, clip,
                              0, d_llr, stream, "mimo_list_llr");
}

int cpx_mimo_list_llr(const cpx_modem *md, const int32_t *cand, const int32_t *count, const double *dist, int64_t B, int nt, int Ke,
                      const double *prior_or_null, double noise_var, double clip, double *llr) {
    CPX_TRACE("cpx_mimo_list_llr");
    CPX_REQUIRE(md && Ke >= 1 && nt >= 1 && B >= 0, CPX_EINVAL, "mimo_list_llr: null modem, Ke < 1, nt < 1 or B < 0");
    CPX_REQUIRE((cand && count && dist && llr) || B == 0, CPX_EINVAL, "mimo_list_llr: null pointer");
    if (int rc = clip_check(noise_var, clip, "mimo_list_llr")) return rc;
    if (int rc = ensure_device()) return rc;
    if (B == 0) return cpx_mimo_list_llr_dev(md, nullptr, nullptr, nullptr, 0, nt, Ke, nullptr, noise_var, clip, nullptr, nullptr);
    HostStage s;
    const int32_t *d_cand, *d_count;
    const double *d_dist, *d_prior = nullptr;
    double *d_llr;
    const size_t n = 8 * size_t(B) * nt * size_t(md->nbits);
    int rc;
    if ((rc = s.in(cand, 4 * size_t(B) * Ke * nt, &d_cand)) || (rc = s.in(count, 4 * size_t(B), &d_count)) ||
        (rc = s.in(dist, 8 * size_t(B) * Ke, &d_dist)) || (prior_or_null && (rc = s.in(prior_or_null, n, &d_prior))) ||
        (rc = s.out(n, &d_llr)) ||
        (rc = cpx_mimo_list_llr_dev(md, d_cand, d_count, d_dist, B, nt, Ke, d_prior, noise_var, clip, d_llr, s.st)))
        return rc;
    return s.get(llr, d_llr, n);
}

int cpx_mimo_idd_exchange_dev(const cpx_modem *md, const int32_t *d_cand, const int32_t *d_count, const double *d_dist, int64_t B,
                              int nt, int Ke, double *d_dec_in_inout, const double *d_dec_out, double noise_var, double clip, int last,
                              void *stream) {
    CPX_TRACE("cpx_mimo_idd_exchange_dev");
    return list_launch<true>(md, d_cand, d_count, d_dist, B, nt, Ke, d_dec_in_inout, d_dec_out, noise_var, clip, last != 0, nullptr,
                             stream, "mimo_idd_exchange");
}

int cpx_mimo_llr_hard_dev(const double *d_llr, int64_t n, int8_t *d_bits, void *stream) {
    CPX_TRACE("cpx_mimo_llr_hard_dev");
    CPX_REQUIRE(n >= 0, CPX_EINVAL, "mimo_llr_hard: negative length");
    if (n == 0) return CPX_OK;
    CPX_REQUIRE(d_llr && d_bits, CPX_EINVAL, "mimo_llr_hard: null pointer");
    hipLaunchKernelGGL(llr_sign_kernel, dim3(grid_of(n, DIST_BLOCK)), dim3(DIST_BLOCK), 0, pick_stream(stream), d_llr, n, d_bits);
    CPX_HIP(hipGetLastError());
    note_kernel("llr_sign_kernel");
    return CPX_OK;
}

}  // extern "C"
