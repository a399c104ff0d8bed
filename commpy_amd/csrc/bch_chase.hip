// Chase-II soft-decision decoding of binary BCH codes with Pyndiah's soft output; the component decoder of turbo product codes.
//
// The rule (tests/chase_model.py is its NumPy form, bit for bit).  Per word of n values x_i = llr_i, or fl(llr_i + fl(alpha prior_i)):
// hard decisions h_i = (x_i < 0), reliabilities r_i = |x_i|; the p least reliable positions by (r_i, i) ascending; every test pattern
// tau < 2^p flips the positions its bits name and is decoded by the rule of bch_decode_kernel (the syndromes of bch_dev.h, Berlekamp-
// Massey and the Chien search of cpx_gf.h: the functions that kernel calls); a success is a candidate c_tau with the metric M_tau = sum of r_i over c_tau != h, added serially in ascending position order.
// D is the candidate of least metric (ties: lowest tau).  extrinsic_i = s_i (M_C - M_D) - x_i with s_i = +1 for d_i = 0 and -1
// otherwise and M_C the least metric of the candidates that differ from D at i; s_i beta where there is none.  A word with a non-finite
// x_i is rejected on its own: candidates -1, metric +inf, the hard decisions, extrinsic 0.
//
// bch_chase_kernel: one word per wave, the field tables staged into LDS once per workgroup, no block barrier after that.  Per word:
//   1. x is read once into LDS (xs), its signs ballot into rw; a non-finite value ends the word at 7;
//   2. S_1 .. S_2t of h exactly as bch_decode_kernel computes them; lane j - 1 keeps S_j and, for each of the p least reliable positions
//      (p wave-wide argmin rounds over xs, each taking the least key above the one before), the contribution alpha^(j d) of its degree
//      d: the syndromes of a test pattern are p conditional XORs on a register and never touch the word again;
//   3. per tau: Berlekamp-Massey and the Chien search, whose roots arrive as a list of positions.  The candidate is kept as its sparse
//      difference from h -- the flipped test positions and the roots, less the positions that are both -- sorted by a rank count over
//      at most p + t lanes; lane e then fetches r of the e-th position and the metric is a serial sum of lane broadcasts;
//   4. D's positions are set in a bit mask of the word (dm); xs is refilled with +inf and becomes the competitor array;
//   5. one pass over the candidates min-updates it at the symmetric difference with D: a candidate's lanes update where the mask is
//      clear; D's lanes update unless the candidate holds their position (a broadcast loop over the candidate, entered only when one of
//      its positions is in D).  Positions of one set are distinct, so a step has no write conflict; the work grows with 2^p (p + t),
//      not with 2^p n;
//   6. x is read a second time (by the lane that then writes the position, so extrinsic may alias prior) and the outputs are written;
//   7. D's bits are cleared.
// Every address is b sb + j sj + i si in elements (word (b, j), element i): rows and columns of a block decode in place.
#include "bch_dev.h"

#include <cmath>

using namespace cpx;

#define CHASE_MAX_P 8

namespace {

struct ChaseArgs {
    const double *llr, *prior;             // prior may be null
    const uint16_t *tab;
    double alpha, beta;
    int64_t B, J, sb, sj, si;              // words (b, j), element strides of llr / prior / extrinsic / codeword
    int64_t kb, kj, ki;                    // the same for bits
    int m, N, n, k, t, nw, p;
    uint8_t *bits, *word;
    double *ext, *metric;
    int32_t *cands;
};

__host__ __device__ inline unsigned up8(unsigned v) { return (v + 7u) & ~7u; }

// bytes of LDS per wave, in the order of the kernel's pointers: xs [n] double; rw, dm [nw] 64-bit each; cmet [2^p] double; synd, clog,
// roots, lrp (64 uint16 each); clen [2^p] uint16; cpos [2^p][p + t] uint16
__host__ __device__ inline unsigned chase_wave_lds(int n, int nw, int t, int p) {
    const unsigned nc = 1u << p;
    return 8u * (unsigned)n + 16u * (unsigned)nw + 8u * nc + 4u * 128u + up8(2u * nc) + up8(2u * nc * (unsigned)(p + t));
}

__global__ __launch_bounds__(CPX_GF_MAX_WAVES * 64) void bch_chase_kernel(ChaseArgs a) {
    extern __shared__ double2 chase_lds_raw[];
    unsigned char *base = reinterpret_cast<unsigned char *>(chase_lds_raw);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
    const int n = a.n, k = a.k, t = a.t, N = a.N, nw = a.nw, p = a.p, dmax = p + t, ncand = 1 << p;
    const Gf gf = stage_tables(base, a.tab, a.m, N);
    unsigned char *mine = base + gf_tab_lds(a.m) + (unsigned)wave * chase_wave_lds(n, nw, t, p);
    double *xs = reinterpret_cast<double *>(mine);
    unsigned long long *rw = reinterpret_cast<unsigned long long *>(xs + n), *dm = rw + nw;
    double *cmet = reinterpret_cast<double *>(dm + nw);
    uint16_t *synd = reinterpret_cast<uint16_t *>(cmet + ncand), *clog = synd + 64, *roots = clog + 64, *lrp = roots + 64;
    uint16_t *clen = lrp + 64;
    uint16_t *cpos = reinterpret_cast<uint16_t *>(reinterpret_cast<unsigned char *>(clen) + up8(2u * (unsigned)ncand));
    const double inf = __builtin_huge_val();

    for (int c = lane; c < nw; c += 64) dm[c] = 0ull;
    const int64_t words = a.B * a.J;
    for (int64_t w = (int64_t)blockIdx.x * waves + wave; w < words; w += (int64_t)gridDim.x * waves) {
        const int64_t wb = w / a.J, wj = w - wb * a.J;
        const int64_t at = wb * a.sb + wj * a.sj, atk = wb * a.kb + wj * a.kj;
        wave_sync();                                              // the previous word's arrays have been read
        // 1. the word
        bool bad = false;
        for (int c0 = 0; c0 < nw; c0 += 4) {
            double x[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int i = (c0 + u) * 64 + lane;
                x[u] = 0.0;
                if (i < n) {
                    x[u] = a.llr[at + i * a.si];
                    if (a.prior) x[u] = x[u] + a.alpha * a.prior[at + i * a.si];
                }
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int i = (c0 + u) * 64 + lane;
                if (i < n) xs[i] = x[u];
                bad |= !(fabs(x[u]) < inf);
                const unsigned long long hw = __ballot(x[u] < 0.0);
                if (lane == 0 && c0 + u < nw) rw[c0 + u] = hw;
            }
        }
        const bool rejected = __ballot(bad) != 0ull;
        wave_sync();
        int count = 0, best = 0;
        double best_metric = inf;
        if (!rejected) {
            // 2. syndromes of h, the least reliable positions and their contributions
            syndromes(gf, rw, synd, n, nw, t, lane);
            const unsigned s0 = lane < 2 * t ? synd[lane] : 0u;
            unsigned cb[CHASE_MAX_P];
            double pr = -1.0;                                     // the key chosen last: (pr, pi), below every real key
            int pi = -1;
            int my_lrp = 0;
#pragma unroll
            for (int b = 0; b < CHASE_MAX_P; ++b) {
                cb[b] = 0u;
                if (b < p) {
                    double r = inf;
                    int ri = 0x7fffffff;
                    for (int i = lane; i < n; i += 64) {
                        const double v = fabs(xs[i]);
                        const bool above = v > pr || (v == pr && i > pi);
                        if (above && (v < r || (v == r && i < ri))) { r = v; ri = i; }
                    }
#pragma unroll
                    for (int d = 32; d >= 1; d >>= 1) {
                        const double orr = __shfl_xor(r, d);
                        const int oi = __shfl_xor(ri, d);
                        if (orr < r || (orr == r && oi < ri)) { r = orr; ri = oi; }
                    }
                    pr = r;
                    pi = ri;                                       // p <= n: there is always a position left
                    if (lane == b) my_lrp = ri;
                    if (lane < 2 * t) cb[b] = gf.ex[(unsigned)((lane + 1) * (n - 1 - ri)) % (unsigned)N];
                }
            }
            // the test positions in ascending order: lrp[rank] = position, lrp[8 + rank] = the bit of tau that flips it
            {
                int rank = 0;
                for (int e = 0; e < p; ++e) rank += __shfl(my_lrp, e) < my_lrp ? 1 : 0;
                if (lane < p) { lrp[rank] = (uint16_t)my_lrp; lrp[8 + rank] = (uint16_t)lane; }
            }
            wave_sync();
            // 3. the test patterns
            for (unsigned tau = 0; tau < (unsigned)ncand; ++tau) {
                unsigned s = s0;
#pragma unroll
                for (int b = 0; b < CHASE_MAX_P; ++b)
                    if ((tau >> b) & 1u) s ^= cb[b];
                wave_sync();                                      // the pattern before has read synd, roots and its cpos row
                if (lane < 2 * t) synd[lane] = (uint16_t)s;
                wave_sync();
                int L = 0;
                if (__ballot(s != 0u) != 0ull) {
                    unsigned C = lane == 0 ? 1u : 0u;
                    if (berlekamp_massey(gf, synd, 2 * t, 0, lane, C, L)) continue;
                    if (chien_search<false, true>(gf, C, L, clog, nullptr, roots, n, nw, lane) != L) continue;
                    wave_sync();
                }
                // the difference from h: lanes 0 .. p - 1 the flipped test positions, lanes 8 .. 8 + L - 1 the roots
                const bool is_root = lane >= 8 && lane < 8 + L;
                bool valid = is_root || (lane < p && ((tau >> lrp[8 + (lane & 7)]) & 1u));
                const int pos = is_root ? (int)roots[lane - 8] : (int)lrp[lane & 7];
                for (int j = 0; j < p; ++j) {
                    if (!((tau >> lrp[8 + j]) & 1u)) continue;
                    const bool same = is_root && pos == (int)lrp[j];
                    if (same) valid = false;
                    if (__ballot(same) != 0ull && lane == j) valid = false;
                }
                const int key = valid ? pos : 0x7fffffff;
                int rank = 0;
                for (int e = 0; e < 8 + L; ++e) rank += __shfl(key, e) < key ? 1 : 0;
                const int len = __popcll(__ballot(valid));
                uint16_t *row = cpos + count * dmax;
                if (valid) row[rank] = (uint16_t)pos;
                wave_sync();
                const double r = lane < len ? fabs(xs[row[lane]]) : 0.0;
                double metric = 0.0;
                for (int e = 0; e < len; ++e) metric = metric + __shfl(r, e);
                if (lane == 0) { cmet[count] = metric; clen[count] = (uint16_t)len; }
                if (metric < best_metric) { best_metric = metric; best = count; }
                ++count;
            }
            wave_sync();
        }
        // 4. D's bit mask; xs becomes the competitor array
        int dlen = 0, dpos = -1;
        if (count > 0) {
            dlen = clen[best];
            if (lane < dlen) {
                dpos = cpos[best * dmax + lane];
                atomicOr(&dm[dpos >> 6], 1ull << (dpos & 63));
            }
            for (int i = lane; i < n; i += 64) xs[i] = inf;
            wave_sync();
            // 5. competitors
            for (int c = 0; c < count; ++c) {
                const double mc = cmet[c];
                const int len = clen[c];
                const int q = lane < len ? (int)cpos[c * dmax + lane] : 0;     // an idle lane looks at position 0 and writes nothing
                const bool in_d = lane < len && ((dm[q >> 6] >> (q & 63)) & 1ull);
                if (lane < len && !in_d && mc < xs[q]) xs[q] = mc;
                bool held = false;                                // this lane's position of D is one of the candidate's
                if (__ballot(in_d) != 0ull)
                    for (int e = 0; e < len; ++e) held |= __shfl(q, e) == dpos;
                if (lane < dlen && !held) {
                    if (mc < xs[dpos]) xs[dpos] = mc;
                }
                wave_sync();
            }
        }
        // 6. outputs
        for (int c = 0; c < nw; ++c) {
            const int i = c * 64 + lane;
            if (i < n) {
                unsigned bit = (unsigned)((rw[c] >> lane) & 1ull);
                double e = 0.0;
                if (count > 0) {
                    double x = a.llr[at + i * a.si];
                    if (a.prior) x = x + a.alpha * a.prior[at + i * a.si];
                    bit ^= (unsigned)((dm[c] >> lane) & 1ull);
                    const double sgn = bit ? -1.0 : 1.0, mc = xs[i];
                    e = mc < inf ? sgn * (mc - best_metric) - x : sgn * a.beta;
                }
                if (a.ext) a.ext[at + i * a.si] = e;
                if (a.word) a.word[at + i * a.si] = (uint8_t)bit;
                if (a.bits && i < k) a.bits[atk + i * a.ki] = (uint8_t)bit;
            }
        }
        if (lane == 0) {
            if (a.metric) a.metric[w] = best_metric;
            if (a.cands) a.cands[w] = rejected ? -1 : count;
        }
        wave_sync();
        // 7. D's bits
        if (lane < dlen) dm[dpos >> 6] = 0ull;
    }
}

int chase_check(const cpx_bch *h, int p, int64_t B, int64_t J, int64_t sb, int64_t sj, int64_t si, double alpha, double beta, bool any_out,
                unsigned *lds_out, int *waves_out) {
    CPX_REQUIRE(h, CPX_EINVAL, "bch_chase: null handle");
    CPX_REQUIRE(B >= 0 && J >= 1, CPX_EINVAL, "bch_chase: B = %lld, J = %lld", (long long)B, (long long)J);
    CPX_REQUIRE(p >= 1 && p <= CHASE_MAX_P && p <= h->n, CPX_EINVAL, "bch_chase: p = %d is outside 1 .. min(%d, n = %d)", p, CHASE_MAX_P, h->n);
    CPX_REQUIRE(std::isfinite(alpha), CPX_EINVAL, "bch_chase: alpha is not finite");
    CPX_REQUIRE(std::isfinite(beta) && beta >= 0.0, CPX_EINVAL, "bch_chase: beta must be finite and >= 0");
    CPX_REQUIRE(any_out, CPX_EINVAL, "bch_chase: no output requested");
    const int64_t lim = (int64_t)1 << 40, n = h->n;
    CPX_REQUIRE(si >= 1 && si < lim && sj >= 0 && sj < lim && sb >= 0 && sb < lim && B < lim && J < lim, CPX_EINVAL,
                "bch_chase: strides (%lld, %lld, %lld) or sizes out of range", (long long)sb, (long long)sj, (long long)si);
    // words must not overlap: the code axis inside the word axis j or the other way round, both inside b
    const int64_t span_i = (n - 1) * si, span_j = (J - 1) * sj;
    CPX_REQUIRE(J == 1 || sj > span_i || (sj >= 1 && si > span_j), CPX_EINVAL, "bch_chase: the words of one block overlap (sj = %lld, si = %lld)",
                (long long)sj, (long long)si);
    CPX_REQUIRE(B <= 1 || sb > span_i + span_j, CPX_EINVAL, "bch_chase: the blocks overlap (sb = %lld)", (long long)sb);
    CPX_REQUIRE(B <= 1 || (B - 1) <= ((int64_t)1 << 60) / sb, CPX_EINVAL, "bch_chase: B sb does not fit");
    const int nw = (h->n + 63) / 64;
    const unsigned per = chase_wave_lds(h->n, nw, h->t, p), tab = gf_tab_lds(h->m);
    // waves per workgroup: the count that keeps most waves on a compute unit (each workgroup stages the tables again, a wave holds its word)
    int waves = 1, most = 0;
    for (int w = gf_waves(h->m); w >= 1; --w) {
        const uint64_t need = ((uint64_t)tab + (uint64_t)w * per + 15u) & ~(uint64_t)15u;
        if (need > CPX_GF_LDS_MAX) continue;
        const int per_cu = wgs_per_cu(need, w);
        if (w * per_cu > most) { most = w * per_cu; waves = w; }
    }
    const uint64_t lds = ((uint64_t)tab + (uint64_t)waves * per + 15u) & ~(uint64_t)15u;
    CPX_REQUIRE(lds <= CPX_GF_LDS_MAX, CPX_ELIMIT, "bch_chase: m = %d, n = %d, t = %d, p = %d needs %llu bytes of LDS, the limit is %d", h->m, h->n,
                h->t, p, (unsigned long long)lds, CPX_GF_LDS_MAX);
    *lds_out = (unsigned)lds;
    *waves_out = waves;
    return CPX_OK;
}

}  // namespace

extern "C" {

int cpx_chase_bch_dev(const cpx_bch *h, const double *d_llr, const double *d_prior, double alpha, double beta, int p, int64_t B, int64_t J,
                      int64_t sb, int64_t sj, int64_t si, uint8_t *d_bits, uint8_t *d_codeword, double *d_extrinsic, double *d_metric,
                      int32_t *d_candidates, void *stream) {
    CPX_TRACE("cpx_chase_bch_dev");
    unsigned lds;
    int waves;
    if (int rc = chase_check(h, p, B, J, sb, sj, si, alpha, beta, d_bits || d_codeword || d_extrinsic || d_metric || d_candidates, &lds, &waves))
        return rc;
    if (B == 0) return CPX_OK;
    CPX_REQUIRE(d_llr, CPX_EINVAL, "bch_chase: null pointer");
    if (int rcd = check_handle_device(h->device, "bch_chase")) return rcd;
    if (int rcl = raise_lds((const void *)bch_chase_kernel, CPX_GF_LDS_MAX, h->device, "bch_chase")) return rcl;
    ChaseArgs a;
    a.llr = d_llr;
    a.prior = d_prior;
    a.tab = h->d_tab;
    a.alpha = alpha;
    a.beta = beta;
    a.B = B;
    a.J = J;
    a.sb = sb;
    a.sj = J == 1 ? 0 : sj;
    a.si = si;
    // bits is dense, nested as the input is: [B][J][k] where the code axis is the inner one, [B][k][J] where the word axis is
    const bool code_inner = J == 1 || sj > (int64_t)(h->n - 1) * si;
    a.kb = J * h->k;
    a.kj = code_inner ? h->k : 1;
    a.ki = code_inner ? 1 : J;
    a.m = h->m;
    a.N = h->N;
    a.n = h->n;
    a.k = h->k;
    a.t = h->t;
    a.nw = (h->n + 63) / 64;
    a.p = p;
    a.bits = d_bits;
    a.word = d_codeword;
    a.ext = d_extrinsic;
    a.metric = d_metric;
    a.cands = d_candidates;
    const int64_t wgs = (B * J + waves - 1) / waves;
    hipLaunchKernelGGL(bch_chase_kernel, dim3(resident_grid(wgs, lds, waves)), dim3(waves * 64), lds, pick_stream(stream), a);
    CPX_HIP(hipGetLastError());
    note_kernel("bch_chase_kernel");
    return CPX_OK;
}

int cpx_chase_bch(const cpx_bch *h, const double *llr, const double *prior, double alpha, double beta, int p, int64_t B, uint8_t *bits,
                  uint8_t *codeword, double *extrinsic, double *metric, int32_t *candidates) {
    CPX_TRACE("cpx_chase_bch");
    unsigned lds;
    int waves;
    const int64_t n = h ? h->n : 1;
    if (int rc = chase_check(h, p, B, 1, n, 0, 1, alpha, beta, bits || codeword || extrinsic || metric || candidates, &lds, &waves)) return rc;
    if (B == 0) return CPX_OK;
    CPX_REQUIRE(llr, CPX_EINVAL, "bch_chase: null pointer");
    int rc = ensure_device();
    if (rc) return rc;
    const size_t b = (size_t)B;
    HostStage::Out outs[5] = {
        {bits, b * (size_t)h->k}, {codeword, b * (size_t)h->n}, {extrinsic, 8 * b * (size_t)h->n}, {metric, 8 * b}, {candidates, 4 * b}};
    HostStage s;
    const double *dl, *dp = nullptr;
    if ((rc = s.in(llr, 8 * b * (size_t)h->n, &dl))) return rc;
    if (prior && (rc = s.in(prior, 8 * b * (size_t)h->n, &dp))) return rc;
    if ((rc = s.out(outs))) return rc;
    if ((rc = cpx_chase_bch_dev(h, dl, dp, alpha, beta, p, B, 1, n, 0, 1, outs[0].as<uint8_t>(), outs[1].as<uint8_t>(), outs[2].as<double>(),
                                outs[3].as<double>(), outs[4].as<int32_t>(), s.st)))
        return rc;
    return s.get(outs);
}

}  // extern "C"
