// Tail-biting convolutional codes: encoder and wrap-around Viterbi decoder (WAVA) for trellises of 2 .. 64 states, k <= 2, n <= 6.
//
// A block is T trellis steps; the encoder starts in the state it ends in, so a code word is a closed path.  The decoder runs the trellis
// round the block up to max_wraps times, from all-zero state metrics, and after every trip looks for a survivor that ends in the
// state in which it began.  The rule (float64, sums in the order written, -ffp-contract=off):
//   bm_t[c] = sum over the n bits, MSB first and starting from 0.0, of viterbi_decode's per-bit metric of step t (bit_metrics below);
//   M[s] = 0 before the first trip.  On trip w = 1 .. max_wraps:
//   1. M_start = M;
//   2. steps t = 0 .. T - 1: cand_j = M[pred_j] + bm_t[code_j] in np.where order, the first minimum is kept (a later candidate
//      replaces it only if strictly smaller); metrics run on across trips without rescaling;
//   3. origin[s] = the state in which the survivor ending in s began this trip; net[s] = M[s] - M_start[origin[s]];
//   4. s* = first state of minimum M; origin[s*] == s*: return that path, wraps = w, tailbiting = 1, metric = net[s*];
//   5. else c = first state of minimum net among the states with origin[s] == s; c replaces the remembered candidate only if its net
//      is strictly smaller; a remembered candidate keeps its bits;
//   6. after the last trip: the remembered candidate with wraps = max_wraps, tailbiting = 1; none: the path of the last s* with
//      tailbiting = 0, metric = net[s*].
//   A row that holds a NaN, or +-inf under 'hard' / 'unquantized', is rejected: zero bits, wraps = 0, tailbiting = 0, metric = NaN.
//
// tbcc_decode_kernel<LGS, I_T, SR, N_T>: the state-per-lane layout of viterbi_wave_kernel (lane = codeword slot g * S + state s,
//   G = 64 / S code words per wave, the predecessors' metrics exchanged through LDS, one ballot word per step, two for k = 2), with
//   * the whole block's T decision words kept in LDS (no ring: the traceback needs all of them);
//   * no per-step first-argmin: s* is taken once per trip;
//   * the origin travelling forward with the survivor: a lane hands on its metric and, in a byte beside it, its survivor's origin, reads
//     those of its predecessors (a shift register's two are neighbours: one 16-byte and one 2-byte read) and keeps the origin of the one
//     it selects (no walk back over T steps per state and trip);
//   * code words of one wave finishing on different trips: `done` freezes a code word's results while its lanes run on.
//   The branch-metric table is built from the received values S steps at a time (lane (g, i) prepares step t_base + i of code word g,
//   the next chunk's values prefetched): exp + log per value are lane-parallel, a few instructions per step, and the LDS of a wave
//   stays 64 rows however long the block.  A block of one chunk (T <= S) keeps its table across the trips; a longer one rebuilds it
//   on every trip.  With n = 2 or 3 known at compile time (shift-register trellises) a row is 2^(n+1) - 2 additions and the step
//   loop's row offsets are constants.  A traceback (every lane of a code word walks the same path; lane i keeps the symbol of step
//   tb0 + i of a segment of S steps and writes it) runs when a code word finishes or remembers a better candidate.
//   The waves of a workgroup share nothing and never meet; a wave strides over the groups of G code words, and the grid is
//   TB_GRID_ROUNDS times what is resident, so that waves whose code words needed few trips pick up more of them.
// tbcc_encode_kernel: one code word per lane, two table walks (the first finds the end state, the second emits).
#include "cpx_internal.h"
#include "cpx_math.h"
#include "cpx_wave.h"

#include <mutex>

using namespace cpx;

#define CPX_TBCC_MAX_STATES 64
#define CPX_TBCC_MAX_K 2
#define CPX_TBCC_MAX_N 6
#define CPX_TBCC_MAX_BITS 8192             // T * k: the block's decision words stay in LDS (64 KiB per wave at the limit)
#define CPX_TBCC_MAX_WRAPS 32
#define CPX_TBCC_LDS_MAX (160 * 1024)
#define TB_MAX_WAVES 4
#define TB_GRID_ROUNDS 16
#define TB_ENC_THREADS 256

namespace {

// orders this wave's LDS writes before its later reads (the waves of a workgroup never meet).  LDS only: a fence would also wait for the
// global loads in flight, i.e. for the prefetched chunk
__device__ __forceinline__ void wave_sync() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
}

// Per-bit metrics of one received value, as viterbi_decode takes them (viterbi.hip bit_metrics): m0 = cost of code bit 0, m1 = of 1.
// 'soft': r is clipped to +-500 by the caller; exp_pm500 is the device library's exp on that interval, operation for operation.
__device__ __forceinline__ void bit_metrics(int type, double r, double &m0, double &m1) {
    if (type == CPX_VIT_HARD) {
        const long long ri = (long long)r;
        m0 = (double)(ri ^ 0ll);
        m1 = (double)(ri ^ 1ll);
    } else if (type == CPX_VIT_SOFT) {
        const double nll0 = fast_log<false>(exp_pm500(r) + 1.0);
        m0 = nll0;
        m1 = nll0 - r;
    } else {
        const double d0 = r - (-1.0), d1 = r - 1.0;
        m0 = d0 * d0;
        m1 = d1 * d1;
    }
}

struct TbArgs {
    const double *coded;                                   // [B][T n]
    const int32_t *pred_state, *pred_input, *pred_code;    // [S][I], np.where order
    int64_t B;
    int T, k, n, NC, type, max_wraps;
    unsigned wave_lds;                                     // bytes of LDS per wave
    uint8_t *bits;                                         // [B][T k] or null
    int32_t *wraps;                                        // [B] or null
    uint8_t *tailbiting;                                   // [B] or null
    double *metric;                                        // [B] or null
};

// bytes of LDS per wave: 64 metrics, 64 rows of NC branch metrics, T decision words per plane, the predecessor table, 64 origins;
// a multiple of 16: the metric pairs are read as 16 bytes
__host__ __device__ inline unsigned tb_wave_lds(int T, int NC, int PL, int S, int I) {
    return (64u * 8u + 64u * 8u * (unsigned)NC + 8u * (unsigned)PL * (unsigned)T + 2u * (unsigned)(S * I) + 64u + 15u) & ~15u;
}

// minimum over the 2^LGS lanes of a code word, on every one of them (no NaN among the operands)
template <int LGS>
__device__ __forceinline__ double group_min(double v) {
#pragma unroll
    for (int d = 1; d < (1 << LGS); d <<= 1) {
        const double o = __shfl_xor(v, d);
        v = o < v ? o : v;
    }
    return v;
}

// LGS: log2(states); I_T: branches per state (2 or 4); SR: shift-register trellis (k = 1, predecessor j of s is ((s << 1) & (S - 1)) | j,
// the input on every branch into s is s >> (LGS - 1)): the traceback needs no table; N_T: outputs per step when known at compile time
// (2, 3), 0 = run-time n <= 6
template <int LGS, int I_T, bool SR, int N_T>
__global__ __launch_bounds__(TB_MAX_WAVES * 64) void tbcc_decode_kernel(TbArgs a) {
    extern __shared__ double2 tb_lds_raw[];
    constexpr int PL = (I_T == 2) ? 1 : 2;
    constexpr int S = 1 << LGS, G = 64 >> LGS, CH = S;
    constexpr unsigned long long gmask = (S == 64) ? ~0ull : ((1ull << (S & 63)) - 1ull);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
    const int g = lane >> LGS, s = lane & (S - 1), gshift = g << LGS;
    constexpr int NMAX = N_T ? N_T : CPX_TBCC_MAX_N;
    const int T = a.T, n = N_T ? N_T : a.n, NC = N_T ? (1 << N_T) : a.NC, k = a.k;
    const bool rebuild = T > CH;                                  // one chunk: its branch metrics stay in LDS across the trips

    unsigned char *mine = reinterpret_cast<unsigned char *>(tb_lds_raw) + (size_t)wave * a.wave_lds;
    double *pmbuf = reinterpret_cast<double *>(mine);                                 // [64] the metrics a step starts from
    double *bm = pmbuf + 64;                                                          // [64][NC]
    unsigned long long *dec = reinterpret_cast<unsigned long long *>(bm + 64 * NC);   // [T][PL]
    unsigned short *ptab = reinterpret_cast<unsigned short *>(dec + (size_t)T * PL);  // [S * I]
    unsigned char *obuf = reinterpret_cast<unsigned char *>(ptab + S * I_T);          // [64] ... and their survivors' origins

    int pidx[I_T], pcode[I_T];
#pragma unroll
    for (int j = 0; j < I_T; j++) {
        pidx[j] = gshift + a.pred_state[s * I_T + j];
        pcode[j] = a.pred_code[s * I_T + j];
    }
    for (int idx = lane; idx < S * I_T; idx += 64) ptab[idx] = (unsigned short)(a.pred_state[idx] | (a.pred_input[idx] << 8));
    const double *rowbase = bm + gshift * NC;
    // shift register: the two predecessors 2 (s mod S/2), + 1 are neighbours: one 16-byte read for their metrics, one 2-byte read for
    // their origins
    const double2 *ppair = reinterpret_cast<const double2 *>(pmbuf + gshift + 2 * (s & (S / 2 - 1)));
    const unsigned short *opair = reinterpret_cast<const unsigned short *>(obuf + gshift + 2 * (s & (S / 2 - 1)));
    double *my_pm = pmbuf + lane;
    unsigned char *my_ob = obuf + lane;
    const double *row0 = rowbase + pcode[0], *row1 = rowbase + pcode[1];
    const int64_t Tk = (int64_t)T * k, Tn = (int64_t)T * n;
    const int64_t groups = (a.B + G - 1) / G;

    for (int64_t blk = (int64_t)blockIdx.x * waves + wave; blk < groups; blk += (int64_t)gridDim.x * waves) {
        const int64_t cw = blk * G + g;
        const bool valid_cw = cw < a.B;
        const double *x = a.coded + (valid_cw ? cw : 0) * Tn;
        // lane (g, s) prepares step t_base + s of code word g
        auto load_chunk = [&](int t_base, double *r) {
            const int t = t_base + s;
            const bool have = valid_cw && t < T;
#pragma unroll
            for (int j = 0; j < NMAX; j++) r[j] = (have && j < n) ? x[(int64_t)t * n + j] : 0.0;
        };
        double rcur[NMAX];
        load_chunk(0, rcur);

        double pm = 0.0;                                          // M[s] = 0 before the first trip
        bool done = !valid_cw, have_cand = false, bad = false;
        double cand_net = 0.0, r_metric = __builtin_nan("");
        int r_wraps = 0, r_tb = 0;

        for (int w = 1; w <= a.max_wraps; ++w) {
            const double mstart = pm;
            int org = s;
            for (int t_base = 0; t_base < T; t_base += CH) {
                // ---- branch metrics of this chunk
                wave_sync();                                      // the previous chunk's rows have been read
                if (w == 1 || rebuild) {
                    double m0[NMAX], m1[NMAX];
#pragma unroll
                    for (int j = 0; j < NMAX; j++) {
                        double r = rcur[j];
                        if (w == 1) bad |= (r != r) || (a.type != CPX_VIT_SOFT && __builtin_fabs(r) == __builtin_huge_val());
                        if (a.type == CPX_VIT_SOFT) r = fmin(fmax(r, -500.0), 500.0);
                        m0[j] = 0.0;
                        m1[j] = 0.0;
                        if (j < n) bit_metrics(a.type, r, m0[j], m1[j]);
                    }
                    double *row = bm + lane * NC;
                    if constexpr (N_T > 0) {
                        // the sums of the first j + 1 bits from those of the first j: ((0.0 + m[0]) + m[1]) + ..., MSB first, every sum once
                        double lev[1 << N_T];
                        lev[0] = 0.0;
#pragma unroll
                        for (int j = 0; j < N_T; j++)
#pragma unroll
                            for (int q = (1 << j) - 1; q >= 0; --q) {
                                const double v = lev[q];
                                lev[2 * q + 1] = v + m1[j];
                                lev[2 * q] = v + m0[j];
                            }
#pragma unroll
                        for (int c = 0; c < (1 << N_T); c++) row[c] = lev[c];
                    } else {
                        for (int c = 0; c < NC; c++) {
                            double acc = 0.0;
#pragma unroll
                            for (int j = 0; j < NMAX; j++)
                                if (j < n) acc += ((c >> (n - 1 - j)) & 1) ? m1[j] : m0[j];
                            row[c] = acc;
                        }
                    }
                    if (rebuild) load_chunk(t_base + CH < T ? t_base + CH : 0, rcur);   // lands during the steps below; after the last chunk: the next trip's first
                }
                wave_sync();

                // ---- add-compare-select
                const int nsteps = T - t_base < CH ? T - t_base : CH;
                unsigned long long mydec0 = 0, mydec1 = 0;                // decision word(s) of step t_base + s
                auto acs = [&](const int i) {
                    const double *row = rowbase + i * NC;
                    *my_pm = pm;
                    *my_ob = (unsigned char)org;
                    asm volatile("" ::: "memory");                        // LDS operations of one wave execute in order
                    unsigned long long w0, w1 = 0;
                    if (I_T == 2) {
                        double a0, a1;
                        int o0, o1;
                        if (SR) {
                            const double2 pp = *ppair;
                            const unsigned oo = *opair;
                            a0 = pp.x; a1 = pp.y;
                            o0 = (int)(oo & 0xffu); o1 = (int)(oo >> 8);
                        } else {
                            a0 = pmbuf[pidx[0]]; a1 = pmbuf[pidx[1]];
                            o0 = obuf[pidx[0]]; o1 = obuf[pidx[1]];
                        }
                        const double best = a0 + row0[i * NC];
                        const double c1 = a1 + row1[i * NC];
                        const bool d = c1 < best;                         // the first minimum is kept
                        pm = d ? c1 : best;
                        org = d ? o1 : o0;
                        w0 = __ballot(d);
                    } else {
                        double best = pmbuf[pidx[0]] + row[pcode[0]];
                        int jb = 0, ob = obuf[pidx[0]];
#pragma unroll
                        for (int j = 1; j < I_T; j++) {
                            const double c = pmbuf[pidx[j]] + row[pcode[j]];
                            const int oj = obuf[pidx[j]];
                            if (c < best) { best = c; jb = j; ob = oj; }
                        }
                        pm = best;
                        org = ob;
                        w0 = __ballot(jb & 1);
                        w1 = __ballot(jb & 2);
                    }
                    asm volatile("" ::: "memory");
                    const bool minestep = (s == i);                       // lane (g, i) keeps the word of step t_base + i
                    mydec0 = minestep ? w0 : mydec0;
                    if (PL == 2) mydec1 = minestep ? w1 : mydec1;
                };
                for (int i0 = 0; i0 < nsteps; i0 += 4) {                  // four steps per pass: the rows' offsets are constants
#pragma unroll
                    for (int u = 0; u < 4; u++)
                        if (i0 + u < nsteps) acs(i0 + u);
                }
                if (g == 0 && t_base + s < T) {                           // the G code word slots hold identical words
                    dec[(t_base + s) * PL] = mydec0;
                    if (PL == 2) dec[(t_base + s) * PL + 1] = mydec1;
                }
            }
            // ---- end of trip w: origins, net metrics, s* and the candidate
            pmbuf[lane] = mstart;
            wave_sync();
            const double net = pm - pmbuf[gshift + org];
            wave_sync();
            const double mn = group_min<LGS>(pm);
            const unsigned long long eq = (__ballot(pm == mn) >> gshift) & gmask;
            const int sstar = eq ? __ffsll((long long)eq) - 1 : 0;
            const int org_star = __shfl(org, gshift + sstar);
            const double net_star = __shfl(net, gshift + sstar);
            unsigned long long eg = 0;
            int c = 0;
            double net_c = 0.0;
            if (__ballot(!done && org_star != sstar)) {                   // some code word of the wave has not closed: the candidates
                const bool elig = org == s;
                eg = (__ballot(elig) >> gshift) & gmask;
                const double mn2 = group_min<LGS>(elig ? net : __builtin_huge_val());
                const unsigned long long eqc = (__ballot(elig && net == mn2) >> gshift) & gmask;
                c = eqc ? __ffsll((long long)eqc) - 1 : eg ? __ffsll((long long)eg) - 1 : 0;
                net_c = __shfl(net, gshift + c);
            }
            const unsigned long long badg = (__ballot(bad) >> gshift) & gmask;

            int wstart = -1;                                              // the state a traceback starts from this trip, if any
            bool wzero = false;                                           // ... or zero bits (a rejected row)
            if (!done) {
                if (w == 1 && badg) {
                    wzero = true;
                    done = true;                                          // wraps 0, tailbiting 0, metric NaN
                } else if (org_star == sstar) {
                    wstart = sstar;
                    r_wraps = w; r_tb = 1; r_metric = net_star;
                    done = true;
                } else {
                    if (eg && (!have_cand || net_c < cand_net)) {
                        have_cand = true;
                        cand_net = net_c;
                        wstart = c;
                    }
                    if (w == a.max_wraps) {
                        r_wraps = w;
                        if (have_cand) { r_tb = 1; r_metric = cand_net; }
                        else { r_tb = 0; r_metric = net_star; wstart = sstar; }
                        done = true;
                    }
                }
            }
            // ---- traceback: every lane of a code word walks the same path, lane i keeps the symbol of step tb0 + i
            const bool wr = (wstart >= 0 || wzero) && valid_cw;
            if (a.bits && __ballot(wr)) {
                int st = wstart < 0 ? 0 : wstart;
                for (int tb0 = ((T - 1) / S) * S; tb0 >= 0; tb0 -= S) {
                    const int hi = T < tb0 + S ? T : tb0 + S;
                    int mysym = 0;
                    if constexpr (SR) {
                        // the state after step t holds the inputs of steps t, t - 1 .. t - LGS + 1, the latest on top: every LGS steps the
                        // lanes that own one of these steps take their bit, in between only the state moves.  The LGS decision words of
                        // a block are in flight together (their addresses do not depend on the path); a block that reaches below the
                        // segment reads words it does not use, still inside this wave's LDS (the rows of bm lie in front of dec)
                        for (int tt = hi - 1; tt >= tb0; tt -= LGS) {
                            const unsigned back = (unsigned)(tt - tb0 - s);
                            mysym = back < (unsigned)LGS ? (st >> (LGS - 1 - (int)back)) & 1 : mysym;
                            unsigned long long d0[LGS];
#pragma unroll
                            for (int u = 0; u < LGS; u++) d0[u] = dec[tt - u];
#pragma unroll
                            for (int u = 0; u < LGS; u++)
                                if (tt - u >= tb0) st = ((st << 1) & (S - 1)) | (int)((d0[u] >> (gshift + st)) & 1ull);
                        }
                    } else {
                        for (int tt = hi - 1; tt >= tb0; tt -= 8) {       // eight decision words in flight
                            unsigned long long d0[8], d1[8];
#pragma unroll
                            for (int u = 0; u < 8; u++) {
                                const int at = tt - u >= tb0 ? tt - u : tb0;
                                d0[u] = dec[at * PL];
                                d1[u] = PL == 2 ? dec[at * PL + 1] : 0ull;
                            }
#pragma unroll
                            for (int u = 0; u < 8; u++) {
                                if (tt - u >= tb0) {
                                    int j = (int)((d0[u] >> (gshift + st)) & 1ull);
                                    if (PL == 2) j |= (int)((d1[u] >> (gshift + st)) & 1ull) << 1;
                                    const unsigned e = ptab[st * I_T + j];
                                    mysym = (tt - u - tb0 == s) ? (int)(e >> 8) : mysym;
                                    st = (int)(e & 0xffu);
                                }
                            }
                        }
                    }
                    if (wr && tb0 + s < T)
                        for (int b = 0; b < k; b++)
                            a.bits[cw * Tk + (int64_t)(tb0 + s) * k + b] = wzero ? (uint8_t)0 : (uint8_t)((mysym >> (k - 1 - b)) & 1);
                }
            }
            if (__ballot(!done) == 0ull) break;                           // every code word of the wave has finished
        }
        if (valid_cw && s == 0) {
            if (a.wraps) a.wraps[cw] = r_wraps;
            if (a.tailbiting) a.tailbiting[cw] = (uint8_t)r_tb;
            if (a.metric) a.metric[cw] = r_metric;
        }
    }
}

struct TbEncArgs {
    const uint8_t *msg;                    // [B][T k], bit 0 of a byte counts
    const int32_t *next, *out;             // [S][I]
    uint8_t *word;                         // [B][T n]
    uint8_t *closed;                       // [B] or null: 1 = the emitting walk ended in the state in which it began
    int64_t B;
    int T, k, n, S, I;
};

__global__ __launch_bounds__(TB_ENC_THREADS) void tbcc_encode_kernel(TbEncArgs a) {
    __shared__ unsigned short tab[CPX_TBCC_MAX_STATES * 4];               // next state | output << 8
    for (int idx = threadIdx.x; idx < a.S * a.I; idx += blockDim.x) tab[idx] = (unsigned short)(a.next[idx] | (a.out[idx] << 8));
    __syncthreads();
    const int T = a.T, k = a.k, n = a.n, I = a.I;
    for (int64_t cw = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; cw < a.B; cw += (int64_t)gridDim.x * blockDim.x) {
        const uint8_t *m = a.msg + cw * T * k;
        uint8_t *o = a.word + cw * T * n;
        auto symbol = [&](int t) {
            int in = 0;
            for (int b = 0; b < k; b++) in = (in << 1) | (m[(int64_t)t * k + b] & 1);
            return in;
        };
        int st = 0;
        for (int t = 0; t < T; t++) st = tab[st * I + symbol(t)] & 0xff;           // from state 0: where the message leaves the encoder
        const int s0 = st;
        for (int t = 0; t < T; t++) {                                              // from there: the code word
            const unsigned e = tab[st * I + symbol(t)];
            const int code = (int)(e >> 8);
            for (int j = 0; j < n; j++) o[(int64_t)t * n + j] = (uint8_t)((code >> (n - 1 - j)) & 1);
            st = (int)(e & 0xffu);
        }
        if (a.closed) a.closed[cw] = st == s0 ? 1 : 0;
    }
}

// the limits both entry points share
int check_code(const cpx_trellis *t, int64_t B, int64_t T, const char *what) {
    CPX_REQUIRE(t, CPX_EINVAL, "%s: null pointer", what);
    CPX_REQUIRE(B >= 0, CPX_EINVAL, "%s: B = %lld", what, (long long)B);
    CPX_REQUIRE(t->S >= 2 && t->S <= CPX_TBCC_MAX_STATES, CPX_ELIMIT, "%s: %d states, the limit is a power of two from 2 to %d", what, t->S,
                CPX_TBCC_MAX_STATES);
    CPX_REQUIRE(t->k <= CPX_TBCC_MAX_K && t->n <= CPX_TBCC_MAX_N, CPX_ELIMIT, "%s: k = %d, n = %d, the limits are k <= %d and n <= %d", what,
                t->k, t->n, CPX_TBCC_MAX_K, CPX_TBCC_MAX_N);
    CPX_REQUIRE(T >= 1 && T * t->k <= CPX_TBCC_MAX_BITS, CPX_ELIMIT, "%s: T = %lld steps, the limits are T >= 1 and T k <= %d", what,
                (long long)T, CPX_TBCC_MAX_BITS);
    return CPX_OK;
}

int check_decode(const cpx_trellis *t, int64_t B, int64_t T, int decoding_type, int max_wraps, bool any_output) {
    if (int rc = check_code(t, B, T, "tbcc_decode")) return rc;
    CPX_REQUIRE(decoding_type == CPX_VIT_HARD || decoding_type == CPX_VIT_SOFT || decoding_type == CPX_VIT_UNQUANTIZED, CPX_EINVAL,
                "tbcc_decode: decoding_type %d", decoding_type);
    CPX_REQUIRE(max_wraps >= 1 && max_wraps <= CPX_TBCC_MAX_WRAPS, CPX_ELIMIT, "tbcc_decode: max_wraps = %d, the limit is 1 .. %d", max_wraps,
                CPX_TBCC_MAX_WRAPS);
    CPX_REQUIRE(any_output, CPX_EINVAL, "tbcc_decode: no output requested");
    return CPX_OK;
}

// dynamic LDS above 64 KiB has to be allowed once per kernel and device
int raise_lds(const void *fn, int slot, int device) {
    static std::mutex mu;
    static bool raised[30][64] = {};
    CPX_REQUIRE(device >= 0 && device < 64, CPX_ELIMIT, "tbcc: device index %d is outside 0 .. 63", device);
    std::lock_guard<std::mutex> lk(mu);
    if (!raised[slot][device]) {
        CPX_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, CPX_TBCC_LDS_MAX));
        raised[slot][device] = true;
    }
    return CPX_OK;
}

template <int LGS, int I_T, bool SR, int N_T>
int launch_decode(TbArgs a, int device, hipStream_t st) {
    constexpr int S = 1 << LGS, G = 64 >> LGS, PL = (I_T == 2) ? 1 : 2;
    a.wave_lds = tb_wave_lds(a.T, a.NC, PL, S, I_T);
    // waves per workgroup: four where that stays within 64 KiB, so that several workgroups share a compute unit
    int waves = (int)(65536u / a.wave_lds);
    waves = waves < 1 ? 1 : waves > TB_MAX_WAVES ? TB_MAX_WAVES : waves;
    const unsigned lds = a.wave_lds * (unsigned)waves;
    CPX_REQUIRE(lds <= CPX_TBCC_LDS_MAX, CPX_ELIMIT, "tbcc_decode: T = %d, n = %d needs %u bytes of LDS", a.T, a.n, lds);
    const void *fn = (const void *)tbcc_decode_kernel<LGS, I_T, SR, N_T>;
    if (int rc = raise_lds(fn, (LGS - 1) * 5 + (I_T == 4 ? 4 : !SR ? 3 : N_T == 3 ? 2 : N_T == 2 ? 1 : 0), device)) return rc;
    // workgroups that LDS and 32 waves let share a compute unit; the grid is TB_GRID_ROUNDS times that: code words take one to max_wraps
    // trips, and the hardware hands a free slot the next workgroup, which evens out what a grid of exactly the resident size would
    // leave to its slowest wave (measured: the exact size is 15 - 40 % slower at 1 dB)
    int per_cu = (int)(CPX_TBCC_LDS_MAX / lds);
    if (per_cu > 32 / waves) per_cu = 32 / waves;
    const int64_t groups = (a.B + G - 1) / G, wgs = (groups + waves - 1) / waves;
    hipLaunchKernelGGL((tbcc_decode_kernel<LGS, I_T, SR, N_T>), dim3(grid_of(wgs, (int64_t)device_cus() * per_cu * TB_GRID_ROUNDS)), dim3(waves * 64), lds, st,
                       a);
    CPX_HIP(hipGetLastError());
    note_kernel("tbcc_decode_kernel<%d,%d,%d,%d> waves=%d lds=%u per_cu=%d", LGS, I_T, SR ? 1 : 0, N_T, waves, lds, per_cu);
    return CPX_OK;
}

template <int LGS>
int launch_decode_lg(const cpx_trellis *t, const TbArgs &a, hipStream_t st) {
    if (t->I == 4) return launch_decode<LGS, 4, false, 0>(a, t->device, st);
    if (!t->cls.shift_register) return launch_decode<LGS, 2, false, 0>(a, t->device, st);
    if (t->n == 2) return launch_decode<LGS, 2, true, 2>(a, t->device, st);      // the rates in use: the table's size and the rows' offsets
    if (t->n == 3) return launch_decode<LGS, 2, true, 3>(a, t->device, st);      // are compile-time constants
    return launch_decode<LGS, 2, true, 0>(a, t->device, st);
}

}  // namespace

extern "C" {

int cpx_tbcc_encode_dev(const cpx_trellis *t, const uint8_t *d_msg, int64_t B, int64_t T, uint8_t *d_word, uint8_t *d_closed, void *stream) {
    CPX_TRACE("cpx_tbcc_encode_dev");
    if (int rc = check_code(t, B, T, "tbcc_encode")) return rc;
    if (B == 0) return CPX_OK;
    CPX_REQUIRE(d_msg && d_word, CPX_EINVAL, "tbcc_encode: null pointer");
    if (int rcd = check_handle_device(t->device, "tbcc_encode")) return rcd;
    TbEncArgs a{d_msg, t->d_next, t->d_out, d_word, d_closed, B, (int)T, t->k, t->n, t->S, t->I};
    const int64_t wgs = (B + TB_ENC_THREADS - 1) / TB_ENC_THREADS;
    hipLaunchKernelGGL(tbcc_encode_kernel, dim3(grid_of(wgs, (int64_t)device_cus() * 8)), dim3(TB_ENC_THREADS), 0, pick_stream(stream), a);
    CPX_HIP(hipGetLastError());
    note_kernel("tbcc_encode_kernel");
    return CPX_OK;
}

int cpx_tbcc_encode(const cpx_trellis *t, const uint8_t *msg, int64_t B, int64_t T, uint8_t *word, uint8_t *closed) {
    CPX_TRACE("cpx_tbcc_encode");
    if (int rc = check_code(t, B, T, "tbcc_encode")) return rc;
    if (B == 0) return CPX_OK;
    CPX_REQUIRE(msg && word, CPX_EINVAL, "tbcc_encode: null pointer");
    int rc = ensure_device();
    if (rc) return rc;
    const size_t in_bytes = (size_t)B * (size_t)T * (size_t)t->k, out_bytes = (size_t)B * (size_t)T * (size_t)t->n;
    HostStage::Out outs[2] = {{word, out_bytes}, {closed, (size_t)B}};
    HostStage s;
    const uint8_t *din;
    if ((rc = s.in(msg, in_bytes, &din)) || (rc = s.out(outs))) return rc;
    if ((rc = cpx_tbcc_encode_dev(t, din, B, T, outs[0].as<uint8_t>(), outs[1].as<uint8_t>(), s.st))) return rc;
    return s.get(outs);
}

int cpx_tbcc_decode_dev(const cpx_trellis *t, const double *d_coded, int64_t B, int64_t T, int decoding_type, int max_wraps, uint8_t *d_bits,
                        int32_t *d_wraps, uint8_t *d_tailbiting, double *d_metric, void *stream) {
    CPX_TRACE("cpx_tbcc_decode_dev");
    if (int rc = check_decode(t, B, T, decoding_type, max_wraps, d_bits || d_wraps || d_tailbiting || d_metric)) return rc;
    if (B == 0) return CPX_OK;
    CPX_REQUIRE(d_coded, CPX_EINVAL, "tbcc_decode: null pointer");
    if (int rcd = check_handle_device(t->device, "tbcc_decode")) return rcd;
    TbArgs a{d_coded, t->d_pred_state, t->d_pred_input, t->d_pred_code, B, (int)T, t->k, t->n, 1 << t->n, decoding_type, max_wraps, 0u,
             d_bits, d_wraps, d_tailbiting, d_metric};
    hipStream_t st = pick_stream(stream);
    switch (t->cls.lgS) {
    case 1: return launch_decode_lg<1>(t, a, st);
    case 2: return launch_decode_lg<2>(t, a, st);
    case 3: return launch_decode_lg<3>(t, a, st);
    case 4: return launch_decode_lg<4>(t, a, st);
    case 5: return launch_decode_lg<5>(t, a, st);
    default: return launch_decode_lg<6>(t, a, st);
    }
}

int cpx_tbcc_decode(const cpx_trellis *t, const double *coded, int64_t B, int64_t T, int decoding_type, int max_wraps, uint8_t *bits,
                    int32_t *wraps, uint8_t *tailbiting, double *metric) {
    CPX_TRACE("cpx_tbcc_decode");
    if (int rc = check_decode(t, B, T, decoding_type, max_wraps, bits || wraps || tailbiting || metric)) return rc;
    if (B == 0) return CPX_OK;
    CPX_REQUIRE(coded, CPX_EINVAL, "tbcc_decode: null pointer");
    int rc = ensure_device();
    if (rc) return rc;
    const size_t b = (size_t)B;
    HostStage::Out outs[4] = {{bits, b * (size_t)T * (size_t)t->k}, {wraps, 4 * b}, {tailbiting, b}, {metric, 8 * b}};
    HostStage s;
    const double *din;
    if ((rc = s.in(coded, 8 * b * (size_t)T * (size_t)t->n, &din)) || (rc = s.out(outs))) return rc;
    if ((rc = cpx_tbcc_decode_dev(t, din, B, T, decoding_type, max_wraps, outs[0].as<uint8_t>(), outs[1].as<int32_t>(), outs[2].as<uint8_t>(),
                                  outs[3].as<double>(), s.st)))
        return rc;
    return s.get(outs);
}

}  // extern "C"
