// Binary BCH codes: systematic encoder and bounded-distance decoder (syndromes, Berlekamp-Massey, Chien search) over GF(2^m), 3 <= m <= 14.
//
// A word is n bits, bit i the coefficient of x^(n-1-i): the k message bits first, then the n - k bits of x^(n-k) m(x) mod g(x).  A code
// shortened from 2^m - 1 to n drops the highest degrees.  Field elements are integers (bit j = coefficient of alpha^j); the handle holds
// exp[e] = alpha^e and log[v] as uint16 tables of 2^m entries each.
//
// The decoder's stages are shared code: field arithmetic, Berlekamp-Massey and the Chien search live in cpx_gf.h (bch_chase.hip and
// rs.hip run the same functions), the syndromes of a binary word in bch_dev.h (with bch_chase.hip).
// bch_decode_kernel: one received word per wave, up to 16 waves per workgroup, workgroups stride over the batch.  The two tables are staged
//   into LDS once per workgroup (2^(m+2) bytes: 64 KiB at m = 14); after that barrier the waves never meet again.  Per word:
//   1. the bytes are read once, 64 positions per load and eight loads in flight, and kept as ballot words in LDS (rw);
//   2. S_j for odd j, four indices at a time: a lane whose bit is set adds alpha^(j d) of its degree d (the exponent moves by -64 j mod N
//      from one 64-position chunk to the next); XOR across the wave; S_2j = S_j^2 by repeated squaring on the lane of the odd j.  All
//      zero: no error, skip to 5;
//   3. Berlekamp-Massey over the 2t syndromes, lane i holding the coefficients C_i and B_i (degrees stay <= t <= 32: the first length
//      above t is a failure at once), the discrepancy an XOR across the wave;
//   4. Chien search, four chunks at a time: the lane of degree d evaluates sigma(alpha^-d); the ballot of the roots is the chunk's flip
//      mask (fm), its popcount adds to the root count.  The word is corrected iff sigma's leading coefficient is non-zero and the count
//      equals its degree;
//   5. bytes out: (rw ^ fm) bit by bit, fm taken as zero after a failure.
//   The table gathers are 2-byte reads at data-dependent addresses, two entries per bank word: they conflict at random (not measured).
// bch_encode_kernel: one word per lane, 64 words per wave.  The wave reads 64 message bytes of each of its words at a time (a coalesced
//   row segment, copied to the output on the way) and ballots them into one 64-bit word per lane; every lane then runs 64 steps of the long
//   division on its own remainder of RW 64-bit words, the generator being kernel-argument data.  Nothing in it is specific to BCH codes.
#include "bch_dev.h"

using namespace cpx;

#define BCH_ENC_THREADS 256

namespace {

struct BchDecArgs {
    const uint8_t *in;                     // [B][n], non-zero = 1
    const uint16_t *tab;
    int64_t B;
    int m, N, n, k, t, nw;                 // nw = ceil(n / 64)
    uint8_t *bits, *word;                  // [B][k], [B][n]
    int32_t *errors;                       // [B]
};

// bytes of LDS per wave: rw and fm (nw 64-bit words each), then the 2t syndromes and the logarithms of sigma's coefficients
__host__ __device__ inline unsigned bch_wave_lds(int nw) { return 16u * (unsigned)nw + 2u * 64u + 2u * 64u; }

__global__ __launch_bounds__(CPX_GF_MAX_WAVES * 64) void bch_decode_kernel(BchDecArgs a) {
    extern __shared__ double2 bch_lds_raw[];
    unsigned char *base = reinterpret_cast<unsigned char *>(bch_lds_raw);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, waves = blockDim.x >> 6;
    const int n = a.n, k = a.k, t = a.t, N = a.N, nw = a.nw;
    const Gf gf = stage_tables(base, a.tab, a.m, N);
    unsigned char *mine = base + gf_tab_lds(a.m) + (unsigned)wave * bch_wave_lds(nw);
    unsigned long long *rw = reinterpret_cast<unsigned long long *>(mine), *fm = rw + nw;
    uint16_t *synd = reinterpret_cast<uint16_t *>(fm + nw), *clog = synd + 64;

    for (int64_t cw = (int64_t)blockIdx.x * waves + wave; cw < a.B; cw += (int64_t)gridDim.x * waves) {
        wave_sync();                                              // the previous word's arrays have been read
        const uint8_t *in = a.in + cw * n;
        for (int c0 = 0; c0 < nw; c0 += 8) {                      // eight loads in flight: the chain of global latencies is what costs
            uint8_t byte[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int i = (c0 + u) * 64 + lane;
                byte[u] = i < n ? in[i] : (uint8_t)0;
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const unsigned long long w = __ballot(byte[u] != 0);
                if (lane == 0 && c0 + u < nw) { rw[c0 + u] = w; fm[c0 + u] = 0ull; }
            }
        }
        wave_sync();
        syndromes(gf, rw, synd, n, nw, t, lane);
        int errors = 0;
        const bool dirty = __ballot(lane < 2 * t && synd[lane] != 0) != 0ull;
        if (dirty) {
            unsigned C = lane == 0 ? 1u : 0u;
            int L;
            bool fail = berlekamp_massey(gf, synd, 2 * t, 0, lane, C, L);
            if (!fail && chien_search<true, false>(gf, C, L, clog, fm, nullptr, n, nw, lane) != L) fail = true;
            errors = fail ? -1 : L;
            wave_sync();
        }
        const bool flip = errors > 0;
        for (int c = 0; c < nw; ++c) {
            const int i = c * 64 + lane;
            const unsigned long long w = flip ? rw[c] ^ fm[c] : rw[c];
            const uint8_t bit = (uint8_t)((w >> lane) & 1ull);
            if (a.word && i < n) a.word[cw * n + i] = bit;
            if (a.bits && i < k) a.bits[cw * k + i] = bit;
        }
        if (a.errors && lane == 0) a.errors[cw] = errors;
    }
}

struct BchEncArgs {
    const uint8_t *msg;                    // [B][k], bit 0 of every byte
    uint8_t *out;                          // [B][n]
    int64_t B;
    int n, k, deg;
    uint64_t gen[CPX_BCH_MAX_GEN_WORDS];
};

template <int RW>
__global__ __launch_bounds__(BCH_ENC_THREADS) void bch_encode_kernel(BchEncArgs a) {
    const int lane = threadIdx.x & 63, waves = BCH_ENC_THREADS / 64;
    const int n = a.n, k = a.k, deg = a.deg;
    const int top_bit = (deg - 1) & 63;                           // of word RW - 1 = (deg - 1) / 64
    const unsigned long long top_mask = top_bit == 63 ? ~0ull : ((1ull << (top_bit + 1)) - 1ull);
    const int64_t groups = (a.B + 63) / 64;
    for (int64_t g = (int64_t)blockIdx.x * waves + (threadIdx.x >> 6); g < groups; g += (int64_t)gridDim.x * waves) {
        const int64_t w0 = g * 64;
        const int rows = a.B - w0 < 64 ? (int)(a.B - w0) : 64;
        unsigned long long R[RW];
#pragma unroll
        for (int q = 0; q < RW; ++q) R[q] = 0ull;
        for (int c0 = 0; c0 < k; c0 += 64) {
            const int i = c0 + lane;
            unsigned long long bits = 0ull;
            for (int r = 0; r < rows; ++r) {
                int bit = 0;
                if (i < k) {
                    bit = a.msg[(w0 + r) * k + i] & 1;
                    a.out[(w0 + r) * n + i] = (uint8_t)bit;
                }
                const unsigned long long w = __ballot(bit);
                if (lane == r) bits = w;
            }
            const int steps = k - c0 < 64 ? k - c0 : 64;
            for (int s = 0; s < steps; ++s) {
                const unsigned long long fb = ((R[RW - 1] >> top_bit) ^ (bits >> s)) & 1ull;
                const unsigned long long take = 0ull - fb;
#pragma unroll
                for (int q = RW - 1; q >= 1; --q) R[q] = ((R[q] << 1) | (R[q - 1] >> 63)) ^ (a.gen[q] & take);
                R[0] = (R[0] << 1) ^ (a.gen[0] & take);
            }
        }
        R[RW - 1] &= top_mask;
        // parity bit p (0 .. deg - 1) of a word is the coefficient of x^(deg - 1 - p)
        for (int p0 = 0; p0 < deg; p0 += 64) {
            const int p = p0 + lane, x = deg - 1 - p;
            for (int r = 0; r < rows; ++r) {
                unsigned long long v = 0ull;
#pragma unroll
                for (int q = 0; q < RW; ++q) {
                    const unsigned long long wq = __shfl(R[q], r);
                    if (p < deg && (x >> 6) == q) v = wq;
                }
                if (p < deg) a.out[(w0 + r) * n + k + p] = (uint8_t)((v >> (x & 63)) & 1ull);
            }
        }
    }
}

template <int RW>
void launch_encode(const BchEncArgs &a, hipStream_t st) {
    const int64_t groups = (a.B + 63) / 64, wgs = (groups + BCH_ENC_THREADS / 64 - 1) / (BCH_ENC_THREADS / 64);
    hipLaunchKernelGGL(bch_encode_kernel<RW>, dim3(grid_of(wgs, (int64_t)device_cus() * 8)), dim3(BCH_ENC_THREADS), 0, st, a);
}

}  // namespace

extern "C" {

int cpx_bch_create(int m, uint32_t prim_poly, int n, int t, const uint8_t *genpoly_bits, int genpoly_degree, cpx_bch **out) {
    CPX_TRACE("cpx_bch_create");
    CPX_REQUIRE(out, CPX_EINVAL, "bch: null pointer");
    *out = nullptr;
    CPX_REQUIRE(genpoly_bits, CPX_EINVAL, "bch: null pointer");
    std::vector<uint16_t> tab;
    if (int rct = gf_field("bch", m, prim_poly, n, tab)) return rct;
    const int N = (1 << m) - 1;
    CPX_REQUIRE(t >= 1 && t <= CPX_BCH_MAX_T, CPX_ELIMIT, "bch: t = %d is outside the engine's range 1 .. %d", t, CPX_BCH_MAX_T);
    CPX_REQUIRE(2 * t < N, CPX_ELIMIT, "bch: t = %d, need 2 t < 2^m - 1 = %d", t, N);
    const int deg = genpoly_degree;
    CPX_REQUIRE(deg >= 1 && deg < n, CPX_EINVAL, "bch: the generator's degree %d is outside 1 .. n - 1 = %d", deg, n - 1);
    CPX_REQUIRE(deg <= 64 * CPX_BCH_MAX_GEN_WORDS, CPX_ELIMIT, "bch: the generator's degree %d is above the engine's limit of %d", deg,
                64 * CPX_BCH_MAX_GEN_WORDS);
    for (int i = 0; i <= deg; ++i)
        CPX_REQUIRE(genpoly_bits[i] <= 1, CPX_EINVAL, "bch: genpoly_bits[%d] = %d, need 0 or 1", i, (int)genpoly_bits[i]);
    CPX_REQUIRE(genpoly_bits[deg] == 1, CPX_EINVAL, "bch: the generator's coefficient of x^%d is zero", deg);
    CPX_REQUIRE(genpoly_bits[0] == 1, CPX_EINVAL, "bch: the generator has no constant term");
    for (int j = 1; j <= 2 * t; ++j)
        CPX_REQUIRE(gf_eval(tab, m, genpoly_bits, deg, j) == 0, CPX_EINVAL, "bch: the generator does not vanish at alpha^%d", j);
    int rc = ensure_device();
    if (rc) return rc;
    cpx_bch *p = new cpx_bch();
    p->m = m;
    p->N = N;
    p->n = n;
    p->t = t;
    p->deg = deg;
    p->k = n - deg;
    for (uint64_t &w : p->gen) w = 0;
    for (int i = 0; i < deg; ++i)
        if (genpoly_bits[i]) p->gen[i >> 6] |= 1ull << (i & 63);
    (void)hipGetDevice(&p->device);
    if ((rc = upload((void **)&p->d_tab, tab.data(), sizeof(uint16_t) * tab.size(), "bch"))) {
        cpx_bch_destroy(p);
        return rc;
    }
    *out = p;
    return CPX_OK;
}

int cpx_bch_destroy(cpx_bch *p) {
    if (!p) return CPX_OK;
    (void)hipFree(p->d_tab);
    delete p;
    return CPX_OK;
}

int cpx_bch_encode_dev(const cpx_bch *p, const uint8_t *d_msg, int64_t B, uint8_t *d_word, void *stream) {
    CPX_TRACE("cpx_bch_encode_dev");
    if (int rc = check_batch(p, B, "bch_encode")) return rc;
    if (B == 0) return CPX_OK;
    CPX_REQUIRE(d_msg && d_word, CPX_EINVAL, "bch_encode: null pointer");
    if (int rcd = check_handle_device(p->device, "bch_encode")) return rcd;
    BchEncArgs a;
    a.msg = d_msg;
    a.out = d_word;
    a.B = B;
    a.n = p->n;
    a.k = p->k;
    a.deg = p->deg;
    for (int q = 0; q < CPX_BCH_MAX_GEN_WORDS; ++q) a.gen[q] = p->gen[q];
    hipStream_t st = pick_stream(stream);
    switch ((p->deg + 63) / 64) {
    case 1: launch_encode<1>(a, st); break;
    case 2: launch_encode<2>(a, st); break;
    case 3: launch_encode<3>(a, st); break;
    case 4: launch_encode<4>(a, st); break;
    case 5: launch_encode<5>(a, st); break;
    case 6: launch_encode<6>(a, st); break;
    default: launch_encode<7>(a, st); break;
    }
    CPX_HIP(hipGetLastError());
    note_kernel("bch_encode_kernel<%d>", (p->deg + 63) / 64);
    return CPX_OK;
}

int cpx_bch_encode(const cpx_bch *p, const uint8_t *msg, int64_t B, uint8_t *word) {
    CPX_TRACE("cpx_bch_encode");
    if (int rc = check_batch(p, B, "bch_encode")) return rc;
    if (B == 0) return CPX_OK;
    CPX_REQUIRE(msg && word, CPX_EINVAL, "bch_encode: null pointer");
    int rc = ensure_device();
    if (rc) return rc;
    const size_t in_bytes = (size_t)B * (size_t)p->k, out_bytes = (size_t)B * (size_t)p->n;
    HostStage s;
    const uint8_t *din;
    uint8_t *dout;
    if ((rc = s.in(msg, in_bytes, &din)) || (rc = s.out(out_bytes, &dout)) || (rc = cpx_bch_encode_dev(p, din, B, dout, s.st))) return rc;
    return s.get(word, dout, out_bytes);
}

int cpx_bch_decode_dev(const cpx_bch *p, const uint8_t *d_in, int64_t B, uint8_t *d_bits, uint8_t *d_word, int32_t *d_errors, void *stream) {
    CPX_TRACE("cpx_bch_decode_dev");
    if (int rc = check_batch(p, B, "bch_decode")) return rc;
    CPX_REQUIRE(d_bits || d_word || d_errors, CPX_EINVAL, "bch_decode: no output requested");
    if (B == 0) return CPX_OK;
    CPX_REQUIRE(d_in, CPX_EINVAL, "bch_decode: null pointer");
    if (int rcd = check_handle_device(p->device, "bch_decode")) return rcd;
    const int nw = (p->n + 63) / 64, waves = gf_waves(p->m);
    const unsigned lds = (gf_tab_lds(p->m) + (unsigned)waves * bch_wave_lds(nw) + 15u) & ~15u;
    CPX_REQUIRE(lds <= CPX_GF_LDS_MAX, CPX_ELIMIT, "bch_decode: m = %d, n = %d needs %u bytes of LDS", p->m, p->n, lds);
    if (int rcl = raise_lds((const void *)bch_decode_kernel, CPX_GF_LDS_MAX, p->device, "bch_decode")) return rcl;
    BchDecArgs a{d_in, p->d_tab, B, p->m, p->N, p->n, p->k, p->t, nw, d_bits, d_word, d_errors};
    const int64_t wgs = (B + waves - 1) / waves;
    hipLaunchKernelGGL(bch_decode_kernel, dim3(resident_grid(wgs, lds, waves)), dim3(waves * 64), lds, pick_stream(stream), a);
    CPX_HIP(hipGetLastError());
    note_kernel("bch_decode_kernel");
    return CPX_OK;
}

int cpx_bch_decode(const cpx_bch *p, const uint8_t *in, int64_t B, uint8_t *bits, uint8_t *word, int32_t *errors) {
    CPX_TRACE("cpx_bch_decode");
    if (int rc = check_batch(p, B, "bch_decode")) return rc;
    CPX_REQUIRE(bits || word || errors, CPX_EINVAL, "bch_decode: no output requested");
    if (B == 0) return CPX_OK;
    CPX_REQUIRE(in, CPX_EINVAL, "bch_decode: null pointer");
    int rc = ensure_device();
    if (rc) return rc;
    const size_t b = (size_t)B;
    HostStage::Out outs[3] = {{bits, b * (size_t)p->k}, {word, b * (size_t)p->n}, {errors, 4 * b}};
    HostStage s;
    const uint8_t *din;
    if ((rc = s.in(in, b * (size_t)p->n, &din)) || (rc = s.out(outs))) return rc;
    if ((rc = cpx_bch_decode_dev(p, din, B, outs[0].as<uint8_t>(), outs[1].as<uint8_t>(), outs[2].as<int32_t>(), s.st))) return rc;
    return s.get(outs);
}

}  // extern "C"
