// MIMO flat-fading channel and hard-decision error count on the device: the two stages a MIMO link needs around the
// detectors so that a Monte-Carlo point never leaves HBM.
//   MIMOFlatChannel.propagate  commpy/channels.py:242-330 (Kronecker model H = sqrtm(Rr) G sqrtm(Rt)^T + mean, y = H x + noise), with
//                              Philox counter streams (cpx_rng.h) in place of NumPy's MT19937
//   mimo_receiver hard path    commpy_amd/links.py (bits of the detected constellation indices, MSB first) counted against the message
// float64, -ffp-contract=off (build.py), like mimo.hip: the channel's products are bit-exact against a host loop in the documented order.
//
// mimo_channel_kernel: one lane per received vector, grid-striding over the batch.  Per vector v (global index gv = first_vector + v):
//   x[a]     = constellation[label of bits[(v nt + a) nb ..][0..nb)], MSB first                     (modulate_kernel, linksim.hip)
//   G[r][a]  = sqrt(1/2) (n_re + j n_im), Box-Muller on philox(gv nr nt + r nt + a, stream_fading, seed)   (awgn_add, cpx_rng.h)
//   T[r][p]  = sum_q A[r][q] G[q][p]             q ascending   (skipped, T = G, when A is the identity)
//   H[r][a]  = sum_p T[r][p] Bt[p][a] + mean[r][a]  p ascending, mean last   (product skipped when Bt is the identity)
//   y[r]     = sum_a H[r][a] x[a]  a ascending, then + noise_scale (n_re + j n_im) from philox(gv nr + r, stream_noise, seed)
// Every sum starts from 0 + the first product; a complex product is (ar br - ai bi, ar bi + ai br).  The noise of y is exactly
// cpx_awgn_dev(H x, ..., stream_noise) over the flattened [V][nr] array, and G is cpx_awgn_dev of zeros with scale sqrt(1/2): element
// indices are global, so [0, V) in one launch or in several (first_vector) gives the same bytes.
// Per-lane scratch (x, one row of T, and the whole G when A is not the identity) is interleaved across the wave (element e of lane l
// at e * 64 + l: conflict-free LDS, coalesced global) and lives in LDS while a wave's share fits 64 KB, else in a global workspace.
#include "cpx_internal.h"
#include "cpx_rng.h"

using namespace cpx;

struct cpx_mimo_channel {
    __attribute__((visibility("hidden"))) ~cpx_mimo_channel() = default;
    int nr, nt;
    int device;
    bool a_identity, b_identity;
    double *d_mats = nullptr;   // A [nr][nr], Bt [nt][nt], mean [nr][nt], complex (re, im), one allocation
};

namespace {

constexpr int MC_WAVE = 64;
constexpr size_t MC_LDS_MAX = 64 * 1024;
constexpr int ME_BLOCK = 256;

__device__ __forceinline__ double2 mc_mul(double2 a, double2 b) { return make_double2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }
__device__ __forceinline__ double2 mc_add(double2 a, double2 b) { return make_double2(a.x + b.x, a.y + b.y); }

// scratch elements of one lane: x [nt], T row [nt], G [nr][nt] (only when A is not the identity)
inline int64_t mc_scratch_elems(int nr, int nt, bool a_identity) { return 2 * int64_t(nt) + (a_identity ? 0 : int64_t(nr) * nt); }

template <bool GLOBAL>
__global__ __launch_bounds__(MC_WAVE) void mimo_channel_kernel(const uint8_t *__restrict__ bits, int64_t V, uint64_t first, int nb,
                                                               const double2 *__restrict__ cst, const double2 *__restrict__ A,
                                                               const double2 *__restrict__ Bt, const double2 *__restrict__ mean, int nr,
                                                               int nt, int a_identity, int b_identity, double noise_scale, uint64_t seed,
                                                               uint64_t s_fade, uint64_t s_noise, double2 *__restrict__ y,
                                                               double2 *__restrict__ H, double2 *__restrict__ ws, int64_t per) {
    extern __shared__ double2 mc_lds[];
    const int lane = threadIdx.x;
    double2 *base = GLOBAL ? ws + int64_t(blockIdx.x) * per * MC_WAVE : mc_lds;
    double2 *sx = base + lane, *sT = sx + int64_t(nt) * MC_WAVE, *sG = sT + int64_t(nt) * MC_WAVE;   // element e at [e * MC_WAVE]
    const int64_t nh = int64_t(nr) * nt;
    for (int64_t v = int64_t(blockIdx.x) * MC_WAVE + lane; v < V; v += int64_t(gridDim.x) * MC_WAVE) {
        const uint64_t gv = first + uint64_t(v);
        const uint8_t *bv = bits + v * nt * nb;
        for (int a = 0; a < nt; a++) {
            int label = 0;
            for (int q = 0; q < nb; q++) label = (label << 1) | (bv[int64_t(a) * nb + q] & 1);
            sx[int64_t(a) * MC_WAVE] = cst[label];
        }
        const uint64_t g0 = gv * uint64_t(nh);
        if (!a_identity)
            for (int64_t e = 0; e < nh; e++)
                sG[e * MC_WAVE] = awgn_add(make_double2(0.0, 0.0), g0 + uint64_t(e), M_SQRT1_2, M_SQRT1_2, seed, s_fade);
        double2 *Hv = H + v * nh, *yv = y + v * nr;
        for (int r = 0; r < nr; r++) {
            for (int p = 0; p < nt; p++) {                                   // row r of T = A G
                double2 t;
                if (a_identity) {
                    t = awgn_add(make_double2(0.0, 0.0), g0 + uint64_t(r) * nt + p, M_SQRT1_2, M_SQRT1_2, seed, s_fade);
                } else {
                    t = make_double2(0.0, 0.0);
                    for (int q = 0; q < nr; q++) t = mc_add(t, mc_mul(A[int64_t(r) * nr + q], sG[(int64_t(q) * nt + p) * MC_WAVE]));
                }
                sT[int64_t(p) * MC_WAVE] = t;
            }
            double2 acc = make_double2(0.0, 0.0);
            for (int a = 0; a < nt; a++) {                                   // row r of H = T Bt + mean, and y[r] = H[r] . x
                double2 h;
                if (b_identity) {
                    h = sT[int64_t(a) * MC_WAVE];
                } else {
                    h = make_double2(0.0, 0.0);
                    for (int p = 0; p < nt; p++) h = mc_add(h, mc_mul(sT[int64_t(p) * MC_WAVE], Bt[int64_t(p) * nt + a]));
                }
                h = mc_add(h, mean[int64_t(r) * nt + a]);
                Hv[int64_t(r) * nt + a] = h;
                acc = mc_add(acc, mc_mul(h, sx[int64_t(a) * MC_WAVE]));
            }
            yv[r] = awgn_add(acc, gv * uint64_t(nr) + uint64_t(r), noise_scale, noise_scale, seed, s_noise);
        }
    }
}

// errs[t] = number of message bits of transmission t that differ from the MSB-first labels of its detected indices: symbol s of
// transmission t is idx[t * (bits_per_tx / nb) + s], its bits msg[t][s nb .. s nb + nb).  One wave per transmission, lanes over
// symbols, butterfly sum (count_errors_kernel's shape).
__global__ __launch_bounds__(ME_BLOCK) void mimo_hard_errors_kernel(const int32_t *__restrict__ idx, int nb, const uint8_t *__restrict__ msg,
                                                                    int64_t T, int64_t bits_per_tx, int32_t *__restrict__ errs) {
    const int lane = threadIdx.x & 63;
    const int64_t nsym = bits_per_tx / nb, nwaves = int64_t(gridDim.x) * (ME_BLOCK / 64);
    const uint32_t mask = (nb >= 32) ? 0xFFFFFFFFu : ((1u << nb) - 1u);
    for (int64_t t = int64_t(blockIdx.x) * (ME_BLOCK / 64) + (threadIdx.x >> 6); t < T; t += nwaves) {
        const int32_t *it = idx + t * nsym;
        const uint8_t *mt = msg + t * bits_per_tx;
        int32_t e = 0;
        for (int64_t s = lane; s < nsym; s += 64) {
            uint32_t word = 0;
            for (int q = 0; q < nb; q++) word = (word << 1) | (mt[s * nb + q] & 1u);
            e += __popc((uint32_t(it[s]) ^ word) & mask);
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) e += __shfl_xor(e, off);
        if (lane == 0) errs[t] = e;
    }
}

bool is_identity(const double *m, int n) {
    for (int i = 0; i < n; i++)
        for (int j = 0; j < n; j++) {
            const double re = m[2 * (i * n + j)], im = m[2 * (i * n + j) + 1];
            if (re != (i == j ? 1.0 : 0.0) || im != 0.0) return false;
        }
    return true;
}

}  // namespace

extern "C" {

int cpx_mimo_channel_create(int nr, int nt, const double *sqrt_rr, const double *sqrt_rt_T, const double *mean, cpx_mimo_channel **out) {
    CPX_TRACE("cpx_mimo_channel_create");
    CPX_REQUIRE(sqrt_rr && sqrt_rt_T && mean && out, CPX_EINVAL, "mimo_channel: null pointer");
    CPX_REQUIRE(nr >= 1 && nt >= 1, CPX_EINVAL, "mimo_channel: need nr >= 1 and nt >= 1 (got %d x %d)", nr, nt);
    for (size_t i = 0; i < 2 * (size_t(nr) * nr); i++)
        CPX_REQUIRE(std::isfinite(sqrt_rr[i]), CPX_EINVAL, "mimo_channel: sqrtm(Rr) holds a non-finite entry");
    for (size_t i = 0; i < 2 * (size_t(nt) * nt); i++)
        CPX_REQUIRE(std::isfinite(sqrt_rt_T[i]), CPX_EINVAL, "mimo_channel: sqrtm(Rt).T holds a non-finite entry");
    int rc = ensure_device();
    if (rc) return rc;
    const size_t na = size_t(nr) * nr, nbt = size_t(nt) * nt, nm = size_t(nr) * nt;
    std::vector<double> host(2 * (na + nbt + nm));
    std::memcpy(host.data(), sqrt_rr, 16 * na);
    std::memcpy(host.data() + 2 * na, sqrt_rt_T, 16 * nbt);
    std::memcpy(host.data() + 2 * (na + nbt), mean, 16 * nm);
    cpx_mimo_channel *ch = new cpx_mimo_channel();
    ch->nr = nr;
    ch->nt = nt;
    (void)hipGetDevice(&ch->device);
    ch->a_identity = is_identity(sqrt_rr, nr);
    ch->b_identity = is_identity(sqrt_rt_T, nt);
    if ((rc = upload((void **)&ch->d_mats, host.data(), 8 * host.size(), "mimo_channel"))) {
        cpx_mimo_channel_destroy(ch);
        return rc;
    }
    *out = ch;
    return CPX_OK;
}

int cpx_mimo_channel_destroy(cpx_mimo_channel *ch) {
    if (!ch) return CPX_OK;
    (void)hipFree(ch->d_mats);
    delete ch;
    return CPX_OK;
}

int cpx_mimo_channel_run_dev(const cpx_mimo_channel *ch, const cpx_modem *md, const uint8_t *d_bits, int64_t V, uint64_t first_vector,
                             double noise_scale, uint64_t seed, uint64_t stream_fading, uint64_t stream_noise, double *d_y_re_im,
                             double *d_h_re_im, void *stream) {
    CPX_TRACE("cpx_mimo_channel_run_dev");
    CPX_REQUIRE(ch && md, CPX_EINVAL, "mimo_channel: null handle");
    if (int rcd = check_handle_device(ch->device, "mimo_channel")) return rcd;
    if (int rcd = check_handle_device(md->device, "mimo_channel")) return rcd;
    CPX_REQUIRE(V >= 0, CPX_EINVAL, "mimo_channel: negative batch");
    CPX_REQUIRE(md->nbits >= 1 && md->nbits <= 30 && md->M == (1 << md->nbits), CPX_EINVAL,
                "mimo_channel: the modem's %d points are not 2^nb labels of nb bits", md->M);
    CPX_REQUIRE(std::isfinite(noise_scale) && noise_scale >= 0.0, CPX_EINVAL, "mimo_channel: noise_scale %g is not a finite value >= 0",
                noise_scale);
    if (V == 0) return CPX_OK;
    CPX_REQUIRE(d_bits && d_y_re_im && d_h_re_im, CPX_EINVAL, "mimo_channel: null pointer");
    const int nr = ch->nr, nt = ch->nt;
    const int64_t per = mc_scratch_elems(nr, nt, ch->a_identity);
    const size_t wave_bytes = size_t(per) * MC_WAVE * 16;
    hipStream_t st = pick_stream(stream);
    const double2 *mats = reinterpret_cast<const double2 *>(ch->d_mats);
    const double2 *A = mats, *Bt = A + size_t(nr) * nr, *mean = Bt + size_t(nt) * nt;
    const double2 *cst = reinterpret_cast<const double2 *>(md->d_const);
    double2 *y = reinterpret_cast<double2 *>(d_y_re_im), *H = reinterpret_cast<double2 *>(d_h_re_im);
    int64_t grid = (V + MC_WAVE - 1) / MC_WAVE;
    if (wave_bytes <= MC_LDS_MAX) {
        if (grid > 65536) grid = 65536;
        hipLaunchKernelGGL(mimo_channel_kernel<false>, dim3(unsigned(grid)), dim3(MC_WAVE), wave_bytes, st, d_bits, V, first_vector, md->nbits,
                           cst, A, Bt, mean, nr, nt, int(ch->a_identity), int(ch->b_identity), noise_scale, seed, stream_fading,
                           stream_noise, y, H, (double2 *)nullptr, per);
        CPX_HIP(hipGetLastError());
        note_kernel("mimo_channel_kernel<lds> (%dx%d%s%s)", nr, nt, ch->a_identity ? "" : ", A", ch->b_identity ? "" : ", Bt");
        return CPX_OK;
    }
    // a wave's scratch above 64 KB: the same kernel on a global workspace of at most 1 GB (at least one wave's share: no shape is refused,
    // a share the device cannot hold fails as CPX_ENOMEM)
    Scratch sc;
    const int64_t budget = (int64_t(1) << 30) / int64_t(wave_bytes);
    if (grid > budget) grid = budget > 0 ? budget : 1;
    if (grid > 8192) grid = 8192;
    double2 *ws = nullptr;
    if (int rc = sc.get(st, Slot::mimo_channel_state, size_t(grid) * wave_bytes, &ws)) return rc;
    hipLaunchKernelGGL(mimo_channel_kernel<true>, dim3(unsigned(grid)), dim3(MC_WAVE), 0, st, d_bits, V, first_vector, md->nbits, cst, A, Bt,
                       mean, nr, nt, int(ch->a_identity), int(ch->b_identity), noise_scale, seed, stream_fading, stream_noise, y, H,
                       ws, per);
    CPX_HIP(hipGetLastError());
    note_kernel("mimo_channel_kernel<global> (%dx%d%s%s)", nr, nt, ch->a_identity ? "" : ", A", ch->b_identity ? "" : ", Bt");
    return CPX_OK;
}

int cpx_mimo_hard_errors_dev(const int32_t *d_idx, int nb, const uint8_t *d_msg, int64_t T, int64_t bits_per_tx, int32_t *d_errs,
                             void *stream) {
    CPX_TRACE("cpx_mimo_hard_errors_dev");
    CPX_REQUIRE(nb >= 1 && nb <= 31, CPX_EINVAL, "mimo_hard_errors: %d bits per symbol outside 1..31", nb);
    CPX_REQUIRE(T >= 0 && bits_per_tx >= 0, CPX_EINVAL, "mimo_hard_errors: negative size");
    CPX_REQUIRE(bits_per_tx % nb == 0, CPX_EINVAL, "mimo_hard_errors: %lld bits per transmission are not whole symbols of %d bits",
                (long long)bits_per_tx, nb);
    if (T == 0) return CPX_OK;
    CPX_REQUIRE(d_idx && d_msg && d_errs, CPX_EINVAL, "mimo_hard_errors: null pointer");
    int64_t blocks = (T + ME_BLOCK / 64 - 1) / (ME_BLOCK / 64);
    if (blocks > 256 * 32) blocks = 256 * 32;
    hipLaunchKernelGGL(mimo_hard_errors_kernel, dim3(unsigned(blocks)), dim3(ME_BLOCK), 0, pick_stream(stream), d_idx, nb, d_msg, T, bits_per_tx,
                       d_errs);
    CPX_HIP(hipGetLastError());
    return CPX_OK;
}

}  // extern "C"
