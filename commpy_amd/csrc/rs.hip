// Reed-Solomon codes over GF(2^m), 3 <= m <= 14: systematic encoder and bounded-distance errors-and-erasures decoder (syndromes, erasure
// locator, Berlekamp-Massey, Chien search, Forney's values).
//
// A word is n symbols of 16 bits, of which the low m count; symbol i is the coefficient of x^(n-1-i): the k message symbols first, then
// the r = n - k symbols of x^r m(x) mod g(x), g(x) = prod_{j<r} (x - alpha^(fcr+j)).  A code shortened from N = 2^m - 1 to n drops the
// highest degrees.  The handle holds exp[e] = alpha^e and log[v] as uint16 tables of 2^m entries each and the logarithms of g.
//
// rs_decode_kernel<R>, R = 8, 16, 32 or 64 >= r: one received word per wave, up to 16 waves per workgroup, workgroups stride over the
//   batch.  The two tables are staged into LDS once per workgroup; after that barrier the waves never meet again.  Per word:
//   1. symbols and flags are read once, 64 positions per load and four loads of each in flight; every symbol is masked to m bits as it
//      arrives.  The flags are kept as ballot words in LDS (er); the symbols are not kept: the output pass reads them again;
//   2. syndromes, lanes over positions: a lane with symbol v at degree d adds v alpha^((fcr+j) d) to its accumulator j, j = 0 .. R-1
//      (one table read for log v, then the exponent moves by d from j to j + 1: an add, a wrap and one gather per term); R wave XORs
//      at the end leave S_j on lane j and in LDS.  f > r: failure.  All S_j zero: accepted, go to 8;
//   3. Gamma, lane q holding the coefficient of x^q: one shift-multiply-XOR step per flagged position, read from the ballots;
//   4. Berlekamp-Massey (cpx_gf.h, the function bch_decode_kernel calls with f = 0) from rho = f with C = B = Gamma, lane q holding C_q
//      and B_q, the discrepancy an XOR across the wave; it stops as a failure at the first length with 2 L - f > r;
//   5. Chien search (cpx_gf.h, likewise), four chunks at a time: the lane of degree d evaluates Lambda(alpha^-d); the ballot of the roots
//      is kept per chunk (fm), its popcount adds to the root count, and root number j leaves its position in rpos[j].  Corrected iff
//      Lambda_L != 0 and the count equals L;
//   6. Omega_i = sum_q Lambda_q S_(i-q) on lane i, i < r (lane-local sums over LDS reads);
//   7. Forney, lanes over roots (L <= 63 of them): lane j evaluates Omega and the odd part of Lambda at the alpha^-d of root j and
//      keeps Y = alpha^(-d fcr) Omega / Lambda_odd (Lambda_odd(x) = x Lambda'(x)) in LDS: one pass however long the word;
//   8. symbols out, read again chunk by chunk and masked; a root lane XORs the Y of its root number into its symbol.
// rs_encode_kernel<R>: one word per lane, 64 words per wave, the remainder in R registers per lane (g is taken as x^(R-r) g(x), so
//   that the register indices are static).  The wave reads 64 message symbols of each of its words at a time (coalesced row segments,
//   masked, copied to the output on the way) into a padded LDS tile, every lane then runs 64 division steps along its own row:
//   log of the feedback symbol, then one gather per remainder symbol with the generator's logarithms as kernel-argument data.  The
//   parity symbols leave through the same tile, so that the global writes are row segments as well.
#include "cpx_gf.h"

using namespace cpx;

#define CPX_RS_MAX_R 63                    // a polynomial of degree r has a coefficient per lane
#define RS_ENC_WAVES 4
#define RS_TILE_PITCH 66                   // uint16 per tile row: 33 dwords, so that the lanes' rows start on distinct banks

struct cpx_rs {
    __attribute__((visibility("hidden"))) ~cpx_rs() = default;
    int m, N, n, k, r, fcr, device;
    uint16_t glog[64];                     // log of g's coefficient of x^i, i < r; CPX_GF_NONE for zero
    uint16_t *d_tab = nullptr;             // [2][2^m]: exp then log
};

namespace {

struct RsDecArgs {
    const uint16_t *in;                    // [B][n]
    const uint8_t *erased;                 // [B][n] or null
    const uint16_t *tab;
    int64_t B;
    int m, N, n, k, r, fcr, nw;            // nw = ceil(n / 64)
    uint16_t *symbols, *word;              // [B][k], [B][n]
    int32_t *errors;                       // [B]
};

// bytes of LDS per wave: er and fm (nw 64-bit words each), then S (later Y), log Lambda, log Omega and the roots' positions (64 uint16 each)
__host__ __device__ inline unsigned rs_wave_lds(int nw) { return 16u * (unsigned)nw + 4u * 2u * 64u; }

template <int R>
__global__ __launch_bounds__(CPX_GF_MAX_WAVES * 64) void rs_decode_kernel(RsDecArgs a) {
    extern __shared__ double2 rs_lds_raw[];
    unsigned char *base = reinterpret_cast<unsigned char *>(rs_lds_raw);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, waves = blockDim.x >> 6;
    const int n = a.n, k = a.k, r = a.r, N = a.N, nw = a.nw, fcr = a.fcr;
    const unsigned mask = (1u << a.m) - 1u;
    const Gf gf = stage_tables(base, a.tab, a.m, N);
    unsigned char *mine = base + gf_tab_lds(a.m) + (unsigned)wave * rs_wave_lds(nw);
    unsigned long long *er = reinterpret_cast<unsigned long long *>(mine), *fm = er + nw;
    uint16_t *synd = reinterpret_cast<uint16_t *>(fm + nw), *clog = synd + 64, *olog = clog + 64, *rpos = olog + 64, *yv = synd;
    const int fstep = (int)((64u * (unsigned)fcr) % (unsigned)N);  // fcr d mod N moves by this from one chunk to the next

    for (int64_t cw = (int64_t)blockIdx.x * waves + wave; cw < a.B; cw += (int64_t)gridDim.x * waves) {
        wave_sync();                                              // the previous word's arrays have been read
        const uint16_t *in = a.in + cw * n;
        const uint8_t *flag = a.erased ? a.erased + cw * n : nullptr;
        const int d0 = n - 1 - lane;                              // the degree of this lane's position in chunk 0; negative: no position
        // ---- 1, 2: symbols, flags, syndromes
        unsigned acc[R];
#pragma unroll
        for (int u = 0; u < R; ++u) acc[u] = 0u;
        int f = 0;
        int fd = d0 > 0 ? (int)(((unsigned)fcr * (unsigned)d0) % (unsigned)N) : 0;       // fcr d0 < 2^28
        for (int c0 = 0; c0 < nw; c0 += 4) {
            unsigned sym[4];
            uint8_t fl[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int i = (c0 + u) * 64 + lane;
                sym[u] = i < n ? (unsigned)in[i] & mask : 0u;     // only the low m bits of a symbol count
                fl[u] = flag && i < n ? flag[i] : (uint8_t)0;
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const unsigned long long w = __ballot(fl[u] != 0);
                if (c0 + u < nw) {
                    if (lane == 0) { er[c0 + u] = w; fm[c0 + u] = 0ull; }
                    f += __popcll(w);
                }
            }
#pragma nounroll
            for (int u = 0; u < 4; ++u) {                         // one copy of the R gathers: u is uniform, the selects are cheap
                const unsigned v = u == 0 ? sym[0] : u == 1 ? sym[1] : u == 2 ? sym[2] : sym[3];
                int d = d0 - (c0 + u) * 64;
                if (d < 0) d = 0;                                 // past the word's end: v is 0
                const unsigned take = v ? 0xFFFFu : 0u;
                int e = (int)gf.lg[v] + fd;
                if (e >= N) e -= N;
#pragma unroll
                for (int j = 0; j < R; ++j) {
                    acc[j] ^= gf.ex[e] & take;                    // e stays in 0 .. N - 1 on every lane
                    e += d;
                    if (e >= N) e -= N;
                }
                fd -= fstep;
                if (fd < 0) fd += N;
            }
        }
        unsigned S = 0u;
#pragma unroll
        for (int j = 0; j < R; ++j) {
            const unsigned s = wave_xor(acc[j]);
            if (lane == j) S = s;
        }
        if (lane >= r) S = 0u;
        synd[lane] = (uint16_t)S;
        wave_sync();
        int errors = 0, L = 0;
        bool fail = f > r;
        const bool dirty = __ballot(S != 0u) != 0ull;
        if (!fail && dirty) {
            // ---- 3: the erasure locator, coefficient q on lane q
            unsigned C = lane == 0 ? 1u : 0u;
            for (int c = 0; c < nw && f > 0; ++c) {
                unsigned long long w = er[c];
                while (w) {
                    const int b = __ffsll((long long)w) - 1;
                    w &= w - 1ull;
                    const int d = n - 1 - (c * 64 + b);           // 0 .. N - 1: the logarithm of the locator alpha^d
                    const unsigned below = (unsigned)__shfl((int)C, lane > 0 ? lane - 1 : 0);
                    unsigned term = 0u;
                    if (lane > 0 && below) {
                        int e = (int)gf.lg[below] + d;
                        if (e >= N) e -= N;
                        term = gf.ex[e];
                    }
                    C ^= term;
                }
            }
            // ---- 4, 5: Berlekamp-Massey from rho = f and Gamma, then the Chien search: the roots' ballots to fm, their positions to rpos
            fail = berlekamp_massey(gf, synd, r, f, lane, C, L);
            if (!fail && chien_search<true, true>(gf, C, L, clog, fm, rpos, n, nw, lane) != L) fail = true;
            if (!fail) {
                // ---- 6: Omega = S Lambda mod x^r, coefficient i on lane i
                unsigned om = 0u;
                for (int q = 0; q <= L; ++q) {
                    const int cl = clog[q];
                    if (cl == (int)CPX_GF_NONE) continue;
                    const unsigned s = lane >= q && lane < r ? (unsigned)synd[lane - q] : 0u;
                    int e = cl + (int)gf.lg[s];
                    if (e >= N) e -= N;
                    om ^= s ? (unsigned)gf.ex[e] : 0u;
                }
                olog[lane] = om ? gf.lg[om] : (uint16_t)CPX_GF_NONE;
                wave_sync();
                // ---- 7: Forney, root number `lane` on lane `lane`: Omega and the odd part of Lambda at alpha^-d
                const int d = lane < L ? n - 1 - (int)rpos[lane] : 0;
                const int kk = d > 0 ? N - d : 0;
                int qk = 0;
                unsigned ov = olog[0] != CPX_GF_NONE ? (unsigned)gf.ex[olog[0]] : 0u, odd = 0u;
                for (int q = 1; q <= r; ++q) {                    // L <= r
                    qk += kk;
                    if (qk >= N) qk -= N;
                    const int ol = q < r ? (int)olog[q] : (int)CPX_GF_NONE, cl = (q & 1) && q <= L ? (int)clog[q] : (int)CPX_GF_NONE;
                    if (ol != (int)CPX_GF_NONE) {
                        int e = ol + qk;
                        if (e >= N) e -= N;
                        ov ^= gf.ex[e];
                    }
                    if (cl != (int)CPX_GF_NONE) {
                        int e = cl + qk;
                        if (e >= N) e -= N;
                        odd ^= gf.ex[e];
                    }
                }
                unsigned Y = 0u;
                if (ov) {                                         // at a root odd = alpha^-d Lambda'(alpha^-d) is not zero: L simple roots
                    const int back = (int)(((unsigned)fcr * (unsigned)d) % (unsigned)N);
                    int e = (int)gf.lg[ov] - (int)gf.lg[odd] - back;
                    if (e < 0) e += N;
                    if (e < 0) e += N;
                    Y = gf.ex[e];
                }
                yv[lane] = (uint16_t)Y;                           // over the syndromes: Omega has been formed
            }
            errors = fail ? -1 : L - f;
            wave_sync();
        } else if (fail) {
            errors = -1;
        }
        // ---- 8: symbols out, read again; root number j of the word takes yv[j]
        const bool fix = !fail && dirty;
        int seen = 0;
        for (int c = 0; c < nw; ++c) {
            const int i = c * 64 + lane;
            unsigned sym = i < n ? (unsigned)in[i] & mask : 0u;
            const unsigned long long roots = fix ? fm[c] : 0ull;
            if ((roots >> lane) & 1ull) sym ^= yv[(seen + __popcll(roots & ((1ull << lane) - 1ull))) & 63];
            seen += __popcll(roots);
            if (a.word && i < n) a.word[cw * n + i] = (uint16_t)sym;
            if (a.symbols && i < k) a.symbols[cw * k + i] = (uint16_t)sym;
        }
        if (a.errors && lane == 0) a.errors[cw] = errors;
    }
}

struct RsEncArgs {
    const uint16_t *msg;                   // [B][k]
    const uint16_t *tab;
    uint16_t *out;                         // [B][n]
    int64_t B;
    int m, N, n, k, r;
    uint16_t glog[64];                     // of x^(R-r) g(x) without its leading term: entry R - r + i = log g_i, CPX_GF_NONE below
};

template <int R>
__global__ __launch_bounds__(RS_ENC_WAVES * 64) void rs_encode_kernel(RsEncArgs a) {
    extern __shared__ double2 rs_lds_raw[];
    unsigned char *base = reinterpret_cast<unsigned char *>(rs_lds_raw);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n = a.n, k = a.k, r = a.r, N = a.N;
    const unsigned mask = (1u << a.m) - 1u;
    const Gf gf = stage_tables(base, a.tab, a.m, N);
    uint16_t *tile = reinterpret_cast<uint16_t *>(base + gf_tab_lds(a.m)) + (size_t)wave * 64 * RS_TILE_PITCH;
    const int64_t groups = (a.B + 63) / 64;
    for (int64_t g = (int64_t)blockIdx.x * RS_ENC_WAVES + wave; g < groups; g += (int64_t)gridDim.x * RS_ENC_WAVES) {
        const int64_t w0 = g * 64;
        const int rows = a.B - w0 < 64 ? (int)(a.B - w0) : 64;
        unsigned Rm[R];
#pragma unroll
        for (int q = 0; q < R; ++q) Rm[q] = 0u;
        for (int c0 = 0; c0 < k; c0 += 64) {
            const int i = c0 + lane;
            wave_sync();                                          // the tile's previous content has been read
            for (int r0 = 0; r0 < rows; r0 += 8) {                // eight loads in flight
                unsigned v[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) v[u] = i < k && r0 + u < rows ? (unsigned)a.msg[(w0 + r0 + u) * k + i] & mask : 0u;
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    if (r0 + u < rows) {
                        if (i < k) a.out[(w0 + r0 + u) * n + i] = (uint16_t)v[u];
                        tile[(r0 + u) * RS_TILE_PITCH + lane] = (uint16_t)v[u];
                    }
                }
            }
            wave_sync();
            const int steps = k - c0 < 64 ? k - c0 : 64;
            for (int s = 0; s < steps; ++s) {
                const unsigned in = lane < rows ? (unsigned)tile[lane * RS_TILE_PITCH + s] : 0u;
                const unsigned fb = Rm[R - 1] ^ in;               // below 2^m: both were masked or came out of the table
                const unsigned take = fb ? 0xFFFFu : 0u;
                const int lf = gf.lg[fb];
#pragma unroll
                for (int q = R - 1; q >= 1; --q) {
                    unsigned term = 0u;
                    if (a.glog[q] != CPX_GF_NONE) {               // uniform: kernel-argument data
                        int e = lf + (int)a.glog[q];
                        if (e >= N) e -= N;
                        term = gf.ex[e] & take;
                    }
                    Rm[q] = Rm[q - 1] ^ term;
                }
                {
                    unsigned term = 0u;
                    if (a.glog[0] != CPX_GF_NONE) {
                        int e = lf + (int)a.glog[0];
                        if (e >= N) e -= N;
                        term = gf.ex[e] & take;
                    }
                    Rm[0] = term;
                }
            }
        }
        // parity symbol p (0 .. r - 1) of a word is the coefficient of x^(r - 1 - p): register R - 1 - p
        wave_sync();
#pragma unroll
        for (int p = 0; p < R; ++p)
            if (p < r) tile[lane * RS_TILE_PITCH + p] = (uint16_t)Rm[R - 1 - p];
        wave_sync();
        if (lane < r)
            for (int row = 0; row < rows; ++row) a.out[(w0 + row) * n + k + lane] = tile[row * RS_TILE_PITCH + lane];
    }
}

inline int rs_regs(int r) { return r <= 8 ? 8 : r <= 16 ? 16 : r <= 32 ? 32 : 64; }
inline unsigned rs_enc_lds(int m) { return (gf_tab_lds(m) + RS_ENC_WAVES * 64u * RS_TILE_PITCH * 2u + 15u) & ~15u; }

template <int R>
int launch_decode(const RsDecArgs &a, int device, int waves, unsigned lds, hipStream_t st) {
    if (int rc = raise_lds((const void *)rs_decode_kernel<R>, CPX_GF_LDS_MAX, device, "rs")) return rc;
    const int64_t wgs = (a.B + waves - 1) / waves;
    hipLaunchKernelGGL(rs_decode_kernel<R>, dim3(resident_grid(wgs, lds, waves)), dim3(waves * 64), lds, st, a);
    return CPX_OK;
}

template <int R>
int launch_encode(const RsEncArgs &a, int device, hipStream_t st) {
    if (int rc = raise_lds((const void *)rs_encode_kernel<R>, CPX_GF_LDS_MAX, device, "rs")) return rc;
    const unsigned lds = rs_enc_lds(a.m);
    const int64_t groups = (a.B + 63) / 64, wgs = (groups + RS_ENC_WAVES - 1) / RS_ENC_WAVES;
    hipLaunchKernelGGL(rs_encode_kernel<R>, dim3(resident_grid(wgs, lds, RS_ENC_WAVES)), dim3(RS_ENC_WAVES * 64), lds, st, a);
    return CPX_OK;
}

}  // namespace

extern "C" {

int cpx_rs_create(int m, uint32_t prim_poly, int n, int k, int fcr, const uint16_t *genpoly, cpx_rs **out) {
    CPX_TRACE("cpx_rs_create");
    CPX_REQUIRE(out, CPX_EINVAL, "rs: null pointer");
    *out = nullptr;
    CPX_REQUIRE(genpoly, CPX_EINVAL, "rs: null pointer");
    std::vector<uint16_t> tab;
    if (int rct = gf_field("rs", m, prim_poly, n, tab)) return rct;
    const int N = (1 << m) - 1;
    CPX_REQUIRE(k >= 1 && k < n, CPX_EINVAL, "rs: k = %d is outside 1 .. n - 1 = %d", k, n - 1);
    const int r = n - k;
    CPX_REQUIRE(r <= CPX_RS_MAX_R, CPX_ELIMIT, "rs: n - k = %d is above the engine's limit of %d", r, CPX_RS_MAX_R);
    CPX_REQUIRE(fcr >= 0 && fcr < N, CPX_EINVAL, "rs: fcr = %d is outside 0 .. 2^m - 2 = %d", fcr, N - 1);
    const uint16_t *lg = tab.data() + ((size_t)1 << m);
    for (int i = 0; i <= r; ++i)
        CPX_REQUIRE(genpoly[i] <= N, CPX_EINVAL, "rs: genpoly[%d] = %d is no element of GF(2^%d)", i, (int)genpoly[i], m);
    CPX_REQUIRE(genpoly[r] == 1, CPX_EINVAL, "rs: the generator's coefficient of x^%d is %d, need 1 (monic of degree n - k)", r, (int)genpoly[r]);
    for (int j = 0; j < r; ++j)
        CPX_REQUIRE(gf_eval(tab, m, genpoly, r, (fcr + j) % N) == 0, CPX_EINVAL, "rs: the generator does not vanish at alpha^%d", fcr + j);
    int rc = ensure_device();
    if (rc) return rc;
    cpx_rs *p = new cpx_rs();
    p->m = m;
    p->N = N;
    p->n = n;
    p->k = k;
    p->r = r;
    p->fcr = fcr;
    for (int i = 0; i < 64; ++i) p->glog[i] = i < r && genpoly[i] ? lg[genpoly[i]] : (uint16_t)CPX_GF_NONE;
    (void)hipGetDevice(&p->device);
    if ((rc = upload((void **)&p->d_tab, tab.data(), sizeof(uint16_t) * tab.size(), "rs"))) {
        cpx_rs_destroy(p);
        return rc;
    }
    *out = p;
    return CPX_OK;
}

int cpx_rs_destroy(cpx_rs *p) {
    if (!p) return CPX_OK;
    (void)hipFree(p->d_tab);
    delete p;
    return CPX_OK;
}

int cpx_rs_encode_dev(const cpx_rs *p, const uint16_t *d_msg, int64_t B, uint16_t *d_word, void *stream) {
    CPX_TRACE("cpx_rs_encode_dev");
    if (int rc = check_batch(p, B, "rs_encode")) return rc;
    if (B == 0) return CPX_OK;
    CPX_REQUIRE(d_msg && d_word, CPX_EINVAL, "rs_encode: null pointer");
    if (int rcd = check_handle_device(p->device, "rs_encode")) return rcd;
    const int R = rs_regs(p->r);
    RsEncArgs a;
    a.msg = d_msg;
    a.tab = p->d_tab;
    a.out = d_word;
    a.B = B;
    a.m = p->m;
    a.N = p->N;
    a.n = p->n;
    a.k = p->k;
    a.r = p->r;
    for (int q = 0; q < 64; ++q) a.glog[q] = q >= R - p->r && q < R ? p->glog[q - (R - p->r)] : (uint16_t)CPX_GF_NONE;
    hipStream_t st = pick_stream(stream);
    int rc;
    switch (R) {
    case 8: rc = launch_encode<8>(a, p->device, st); break;
    case 16: rc = launch_encode<16>(a, p->device, st); break;
    case 32: rc = launch_encode<32>(a, p->device, st); break;
    default: rc = launch_encode<64>(a, p->device, st); break;
    }
    if (rc) return rc;
    CPX_HIP(hipGetLastError());
    note_kernel("rs_encode_kernel<%d>", R);
    return CPX_OK;
}

int cpx_rs_encode(const cpx_rs *p, const uint16_t *msg, int64_t B, uint16_t *word) {
    CPX_TRACE("cpx_rs_encode");
    if (int rc = check_batch(p, B, "rs_encode")) return rc;
    if (B == 0) return CPX_OK;
    CPX_REQUIRE(msg && word, CPX_EINVAL, "rs_encode: null pointer");
    int rc = ensure_device();
    if (rc) return rc;
    const size_t in_bytes = 2 * (size_t)B * (size_t)p->k, out_bytes = 2 * (size_t)B * (size_t)p->n;
    HostStage s;
    const uint16_t *din;
    uint16_t *dout;
    if ((rc = s.in(msg, in_bytes, &din)) || (rc = s.out(out_bytes, &dout)) || (rc = cpx_rs_encode_dev(p, din, B, dout, s.st))) return rc;
    return s.get(word, dout, out_bytes);
}

int cpx_rs_decode_dev(const cpx_rs *p, const uint16_t *d_in, const uint8_t *d_erased, int64_t B, uint16_t *d_symbols, uint16_t *d_word,
                      int32_t *d_errors, void *stream) {
    CPX_TRACE("cpx_rs_decode_dev");
    if (int rc = check_batch(p, B, "rs_decode")) return rc;
    CPX_REQUIRE(d_symbols || d_word || d_errors, CPX_EINVAL, "rs_decode: no output requested");
    if (B == 0) return CPX_OK;
    CPX_REQUIRE(d_in, CPX_EINVAL, "rs_decode: null pointer");
    if (int rcd = check_handle_device(p->device, "rs_decode")) return rcd;
    const int nw = (p->n + 63) / 64, waves = gf_waves(p->m), R = rs_regs(p->r);
    const unsigned lds = (gf_tab_lds(p->m) + (unsigned)waves * rs_wave_lds(nw) + 15u) & ~15u;
    CPX_REQUIRE(lds <= CPX_GF_LDS_MAX, CPX_ELIMIT, "rs_decode: m = %d, n = %d needs %u bytes of LDS", p->m, p->n, lds);
    RsDecArgs a{d_in, d_erased, p->d_tab, B, p->m, p->N, p->n, p->k, p->r, p->fcr, nw, d_symbols, d_word, d_errors};
    hipStream_t st = pick_stream(stream);
    int rc;
    switch (R) {
    case 8: rc = launch_decode<8>(a, p->device, waves, lds, st); break;
    case 16: rc = launch_decode<16>(a, p->device, waves, lds, st); break;
    case 32: rc = launch_decode<32>(a, p->device, waves, lds, st); break;
    default: rc = launch_decode<64>(a, p->device, waves, lds, st); break;
    }
    if (rc) return rc;
    CPX_HIP(hipGetLastError());
    note_kernel("rs_decode_kernel<%d>", R);
    return CPX_OK;
}

int cpx_rs_decode(const cpx_rs *p, const uint16_t *in, const uint8_t *erased, int64_t B, uint16_t *symbols, uint16_t *word, int32_t *errors) {
    CPX_TRACE("cpx_rs_decode");
    if (int rc = check_batch(p, B, "rs_decode")) return rc;
    CPX_REQUIRE(symbols || word || errors, CPX_EINVAL, "rs_decode: no output requested");
    if (B == 0) return CPX_OK;
    CPX_REQUIRE(in, CPX_EINVAL, "rs_decode: null pointer");
    int rc = ensure_device();
    if (rc) return rc;
    const size_t b = (size_t)B;
    HostStage::Out outs[3] = {{symbols, 2 * b * (size_t)p->k}, {word, 2 * b * (size_t)p->n}, {errors, 4 * b}};
    HostStage s;
    const uint16_t *din;
    const uint8_t *der = nullptr;
    if ((rc = s.in(in, 2 * b * (size_t)p->n, &din))) return rc;
    if (erased && (rc = s.in(erased, b * (size_t)p->n, &der))) return rc;
    if ((rc = s.out(outs))) return rc;
    if ((rc = cpx_rs_decode_dev(p, din, der, B, outs[0].as<uint16_t>(), outs[1].as<uint16_t>(), outs[2].as<int32_t>(), s.st))) return rc;
    return s.get(outs);
}

}  // extern "C"
