// Viterbi decoder, "codeword per lane" path for large batches of the standard rate-1/2 feed-forward codes.
// Same contract and decision rule as viterbi.hip (/root/reference/commpy/channelcoding/convcode.py:661-749,
// :590-657, :575-587) and the same float64 operations in the same order: bit-identical output.
//
// viterbi.hip maps one trellis STATE to a lane: every step pays a cross-lane exchange of the path metrics, an
// all-lane float64 minimum (first-argmin rule) and a ballot -- 26 VALU instructions per trellis step per codeword,
// VALU-issue bound.  When the batch gives every SIMD of the chip a wavefront of 64 codewords, a lane can own a
// whole CODEWORD instead:
//   * the S path metrics live in the lane's registers and are updated IN PLACE.  The radix-2 butterfly of a
//     shift-register trellis reads states (2j, 2j+1) and writes (j, j+S/2); leaving the results where the inputs
//     were rotates the logical->physical register map by one bit per step, so log2(S) unrolled steps return to the
//     identity: 2S VGPRs hold the metrics and the add-compare-select of all states is straight-line code with NO
//     cross-lane traffic (2 v_add_f64, v_cmp_lt_f64, v_min_f64 or 2 v_cndmask, v_addc per state);
//   * WHICH of the four branch metrics a branch uses depends on the generator polynomials; they are template
//     parameters (the branch code is a constexpr function), instantiated for the standard codes below and checked
//     against the trellis tables the caller built -- any other trellis takes the state-per-lane kernels;
//   * the first-argmin state of a step is an in-lane v_min_f64 tree + an in-lane first-equal scan;
//   * traceback, two forms:
//       - fused (viterbi_cw_fused_kernel, default traceback depth 5 m): the decision words stay in an LDS ring per
//         wave, the walk of step t-1 is pipelined through the arithmetic of step t, decoded bits leave through an
//         LDS tile -- one kernel, HBM traffic = LLRs in + bits out;
//       - two kernels (any depth <= 48): decision words and first-argmin states go to a workspace in HBM,
//         [group of 64 codewords][step][lane] so that every store is one coalesced line per wave (9 B per
//         codeword-step), and viterbi_cw_tb_kernel runs the sliding traceback: one workgroup per group stages a
//         window of 64 + tb - 2 steps in LDS (row stride 65 words: the lanes of a wave walk consecutive rows of one
//         column without bank conflicts) and every wave traces two codewords at a time, lane = output step.
// Measured on MI355X for BASELINE config 2 (B = 65536, K = 7, soft): see DESIGN.md 4.1.
#include "cpx_internal.h"
#include "cpx_math.h"
#include "viterbi_cw_asm.h"
#ifndef CPX_GEN_GB
#define CPX_GEN_GB 2      // (rounds 3 / 4: butterflies per LDS fetch group of the table-driven kernel; unused since the index-mode selection of round 5)
#endif

#include <atomic>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <type_traits>

using namespace cpx;

namespace {

template <int LGS, unsigned G0, unsigned G1>
struct SrCode {
    static constexpr int S = 1 << LGS;
    static constexpr int parity(unsigned v) { return __builtin_popcount(v) & 1; }
    // 2-bit output (MSB = first generator) of the branch into state s from its j-th predecessor:
    // register = [input bit | predecessor state], convcode.py:166-175 (generator MSB taps the input)
    static constexpr int code(int s, int j) {
        const unsigned p = (unsigned)(((s << 1) & (S - 1)) | j), b = (unsigned)(s >> (LGS - 1));
        const unsigned reg = (b << LGS) | p;
        return (parity(reg & G0) << 1) | parity(reg & G1);
    }
};

template <int LGS>
constexpr int rotl(int s, int r) {
    r %= LGS;
    return r == 0 ? s : (((s << r) | (s >> (LGS - r))) & ((1 << LGS) - 1));
}

__device__ __forceinline__ double vmin(double a, double b) {      // one v_min_f64 (fmin adds canonicalising v_max)
    double r;
    asm("v_min_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}

// One add-compare-select decision: d = (y < x); result = d ? y : x (first minimum wins, convcode.py:633-642);
// acc = 2*acc + d shifts the decision bit in.  Two forms:
//  * acs_min: v_cmp + v_addc + v_min_f64 -- equal to the select whenever neither operand is NaN, which holds for
//    'hard' (integer metrics) and 'soft' (the clip maps a NaN input to -500, metrics are >= 0 or +inf, only added);
//  * acs_select: v_cmp + 2 v_cndmask + v_addc, the select of viterbi.hip itself -- used for 'unquantized', where a NaN
//    input reaches the metrics and v_min_f64's NaN rule (return the other operand) would differ.
__device__ __forceinline__ double acs_min(unsigned &acc, double x, double y) {
    double r;
    asm("v_cmp_lt_f64 vcc, %3, %2\n\tv_addc_co_u32 %1, vcc, %1, %1, vcc\n\tv_min_f64 %0, %2, %3"
        : "=&v"(r), "+v"(acc) : "v"(x), "v"(y) : "vcc");
    return r;
}
// the first decision of a word: acc = d, written outright (v_cndmask_b32 0, 1, vcc) -- no accumulator to clear every step
__device__ __forceinline__ double acs_min_first(unsigned &acc, double x, double y) {
    double r;
    asm("v_cmp_lt_f64 vcc, %3, %2\n\tv_cndmask_b32 %1, 0, 1, vcc\n\tv_min_f64 %0, %2, %3"
        : "=&v"(r), "=&v"(acc) : "v"(x), "v"(y) : "vcc");
    return r;
}

// The two selects of one butterfly as ONE statement (x0 = min(x0, y0) with its decision into acc0, then the same for x1 / y1 / acc1):
// the compiler pads the boundary between two asm statements with an s_nop wherever they end up next to each other.
__device__ __forceinline__ void acs_min_pair(unsigned &acc0, unsigned &acc1, double &x0, double y0, double &x1, double y1) {
    asm("v_cmp_lt_f64 vcc, %4, %0\n\tv_addc_co_u32 %2, vcc, %2, %2, vcc\n\tv_min_f64 %0, %0, %4\n\t"
        "v_cmp_lt_f64 vcc, %5, %1\n\tv_addc_co_u32 %3, vcc, %3, %3, vcc\n\tv_min_f64 %1, %1, %5"
        : "+&v"(x0), "+&v"(x1), "+&v"(acc0), "+&v"(acc1) : "v"(y0), "v"(y1) : "vcc");   // early clobber: y1 is read after x0 and acc0 are written
}

__device__ __forceinline__ double acs_select(unsigned &acc, double x, double y) {
    int rlo, rhi;
    asm("v_cmp_lt_f64 vcc, %4, %3\n\tv_cndmask_b32 %0, %5, %7, vcc\n\tv_cndmask_b32 %1, %6, %8, vcc\n\t"
        "v_addc_co_u32 %2, vcc, %2, %2, vcc"
        : "=&v"(rlo), "=&v"(rhi), "+v"(acc)
        : "v"(x), "v"(y), "v"(__double2loint(x)), "v"(__double2hiint(x)), "v"(__double2loint(y)), "v"(__double2hiint(y))
        : "vcc");
    return __hiloint2double(rhi, rlo);
}

struct CwParams {
    const double *coded;          // [B][len]
    unsigned long long *dec;      // [groups][T][64]  decision word of step t of the lane's codeword
    unsigned char *best;          // [groups][T][64]  first-argmin state
    uint8_t *bits;                // [B][L]
    uint8_t *nanflags;            // 'soft': one byte per item of the redo launch (64 / S consecutive codewords; one codeword for 64 states),
                                  // 1 = an item's codeword received a NaN (viterbi.hip decodes the item again, NaN-exact)
    int64_t B, len, L, T, Lk, Tp;   // Tp: T rounded up to whole groups of log2(S) steps (row count of dec/best)
    int type, tb;
    unsigned goff[4];             // table-driven kernel (G0 = G1 = 0): per butterfly j the REGISTER OFFSET 2 c_j of the branch metric of its code
                                  // c_j (the 2-bit code of the branch 2j -> j, input 0), packed eight 4-bit fields per word (round 5: four scalar
                                  // registers; thirty-two separate ones spilled to VGPR lanes)
};

// 'soft': the reference's clip lets a NaN through and the codeword's metrics are NaN from that step on (convcode.py:719,
// :633-645).  The kernels here only DETECT that -- one unordered compare of the step's two received values, OR-ed into a
// lane mask on the scalar unit -- and go on with the NaN clipped to -500; flagged codewords are decoded again by the
// NaN-exact state-per-lane kernel (viterbi.hip, "NaN among 'soft' inputs").
__device__ __forceinline__ void nan_or(unsigned long long &mask, double r0, double r1) {
#ifdef CPX_AB_NO_NAN_DETECT                                         // A/B builds only (experiments/README.md): what the detection costs
    (void)mask; (void)r0; (void)r1;
    return;
#endif
    asm("v_cmp_u_f64 vcc, %1, %2\n\ts_or_b64 %0, %0, vcc" : "+s"(mask) : "v"(r0), "v"(r1) : "vcc", "scc");
}
// The pinned form (cw_step, FILLERS): the compare writes a scalar pair of its own and the caller ORs that into the mask later; the mask is
// only read at the end of the kernel.  Timed, taking the two scalar readers of a step (this OR, the tie test) away from the vector
// compares that feed them is worth 1.7 % with no instruction removed (profiles/viterbi_leftovers_ab.txt); the supposed reason is that a
// scalar instruction reading what a vector compare has just written holds the wave until the vector pipeline has delivered it.
// CPX_AB_SCALAR_BEHIND_COMPARE (A/B builds only) puts both readers back where the parent had them.
__device__ __forceinline__ unsigned long long nan_lanes(double r0, double r1) {
#ifdef CPX_AB_NO_NAN_DETECT
    return 0;
#else
    return __builtin_amdgcn_ballot_w64(__builtin_isunordered(r0, r1));   // one v_cmp_u_f64 into a scalar pair (every lane of the wave is active)
#endif
}

// Per-bit metrics of one received value (convcode.py:575-587) -- identical to viterbi.hip
__device__ __forceinline__ void bit_metrics_cw(int type, double r, double &m0, double &m1) {
    if (type == CPX_VIT_HARD) {
        long long ri = (long long)r;
        m0 = (double)(ri ^ 0ll);
        m1 = (double)(ri ^ 1ll);
    } else if (type == CPX_VIT_SOFT) {
        double nll0 = fast_log<false>(exp(r) + 1.0);   // r is clipped to +-500: the argument is finite and >= 1
        m0 = nll0;
        m1 = nll0 - r;
    } else {
        double d0 = r - (-1.0), d1 = r - 1.0;
        m0 = d0 * d0;
        m1 = d1 * d1;
    }
}

// The fused kernel's form of the 'soft' clip and metrics (cw_step<..., LEAN = true>): the same values with fewer instructions.
//  * clip: fmin(fmax(r, -500), 500) compiles to three instructions -- the kernels run in IEEE mode (the code object's kernel descriptor
//    has ieee_mode = 1, dx10_clamp = 1), where v_max_f64 / v_min_f64 turn a SIGNALLING NaN operand into a quiet NaN instead of returning
//    the other operand, so the compiler quiets r first (v_max_f64 r, r).  For every number and for a quiet NaN -- what NumPy, torch and
//    the engine's own generators produce -- the two instructions below return the same value: r clipped, NaN -> -500 (v_max_f64 returns
//    the non-NaN operand).  A signalling NaN comes out as +500 instead of -500; that value is never seen: nan_or flags the codeword
//    (v_cmp_u_f64 is true for either kind of NaN) and the NaN-exact redo launch decodes it again and overwrites all of its bits; the clip
//    only has to keep the arithmetic of the discarded pass finite.  The constants sit in scalar registers, as the compiler keeps them.
//  * exp_pm500 / fast_log<false, false, true>: cpx_math.h, bit-identical on the clipped range.
__device__ __forceinline__ double clip500(double r) {
    double c;
    asm("v_max_f64 %0, %1, %2\n\tv_min_f64 %0, %0, %3" : "=&v"(c) : "v"(r), "s"(-500.0), "s"(500.0));
    return c;
}
__device__ __forceinline__ void soft_metrics_lean(double r, double &m0, double &m1) {
    const double nll0 = fast_log<false, false, true>(exp_pm500(r) + 1.0);   // |r| <= 500: the argument is finite and >= 1
    m0 = nll0;
    m1 = nll0 - r;
}

// One traceback hop: the decision bit of state st is bit 63 - st of the step's word, i.e. the top bit of (w << st)
// (v_lshlrev_b64 uses the low 6 bits of st only); st' = (st << 1) | bit in one v_alignbit_b32.  The high bits of st are
// never masked on the way -- only st mod S is meaningful (for S < 64 the shift amount is masked explicitly).
template <int LGS>
__device__ __forceinline__ unsigned tb_hop(unsigned long long w, unsigned st) {
    const unsigned hi = (unsigned)((w << (st & ((1u << LGS) - 1u))) >> 32);       // LGS = 6: the mask is the hardware's own
    return __builtin_amdgcn_alignbit(st, hi, 31);
}

// One trellis step with the logical->physical map rotated by R: physical register rotl(s, R) holds state s before the
// step and rotl(s, R + 1) after it.
// The hot loop is kept free of branches (decoding type as a template parameter, unconditional loads and stores): with
// control flow between the prefetch and its use the compiler waits for vmcnt(0) right after issuing the loads and the
// memory latency of every group is exposed (measured: 3.26 ms instead of 1.75 ms for BASELINE config 2).
struct NoHook {
    template <int P> __device__ __forceinline__ void at() const {}
};
// FILLERS.  `fill(integral_constant<P>, word)`, P = 0 .. 3, is the caller's own per-step work that does not depend on the first-argmin
// (the fused kernel: ring-slot address, NaN test, ring write of the step's decision word, OR into the NaN mask), cut into four pieces.  Where the step
// has the 32-bit first-argmin, its asm statements form a chain in which each reads registers the one before wrote, and the compiler
// pads every such boundary with an s_nop (it cannot see into the statements); one piece is pinned into each of the four boundaries
// instead, in the order 0 .. 3, so the wait state is spent on an instruction the step needs anyway.  A step that is given fillers also
// takes the two selects of a butterfly as one statement (acs_min_pair) and the tie mask ahead of the index (CPX_ROW_BLOCK_LAST).  Only
// the fused kernel's compile-time-hop 'soft' flavours pass them (PIN there); every other caller passes NoFill and gets the step it had:
// the run-time-hop kernels sit at their scalar-register ceiling and the flavours without the 32-bit first-argmin have no chain to fill --
// both were measured slower with the new form (experiments/README.md).
struct NoFill {};
template <int P, class Fill>
__device__ __forceinline__ void pinned_fill(const Fill &fill, unsigned long long word) {
    __builtin_amdgcn_sched_barrier(0);
    fill(std::integral_constant<int, P>{}, word);
    __builtin_amdgcn_sched_barrier(0);
}

// `hook.at<P>()` is called at four fixed points of the step (after the branch metrics, after each half of the butterflies,
// after the minimum tree): the fused kernel issues the traceback reads of the previous step there.
// G0 = G1 = 0: TABLE-DRIVEN codes -- any shift-register code whose two generators both tap the input bit and the oldest register bit
// (every rate-1/2 code of full constraint length).  The four branches of butterfly j then carry the codes c_j, c_j ^ 3, c_j ^ 3, c_j,
// so one 2-bit number per butterfly describes the code; it arrives packed in scalar registers (goff) and selects the branch metric by
// VGPR index mode (round 5, see the GEN branch below; rounds 3 / 4: an LDS table [4][64 lanes] of pairs (metric of c, metric of c ^ 3) and
// every butterfly reads its pair from there: 32 16-byte LDS reads + 32 address adds per step more than the compiled-in codes.
// LEAN (the fused kernel): clip500 / soft_metrics_lean above, and the branch metrics without the leading "0.0 +" of NumPy's add.reduce.
// Adding +0.0 changes exactly one value, -0.0 (to +0.0; a NaN stays the NaN it was: the per-bit metrics are results of arithmetic,
// already quiet), and no per-bit metric is ever -0.0: 'hard' converts an integer (never -0.0), 'unquantized' takes a square (sign +),
// 'soft' m0 = log(x), x >= 1, ends in a subtraction a - b that is -0.0 only for a = -0.0, b = +0.0 -- a = dk ln2_hi is +0.0 or >= 0.69 --
// and m1 = m0 - r is -0.0 only for m0 = -0.0 (x - x is +0.0 in round-to-nearest).  The other kernels keep the literal form.
template <int LGS, unsigned G0, unsigned G1, int TYPE, int R, bool LEAN = false, class Hook = NoHook, class Fill = NoFill>
__device__ __forceinline__ void cw_step(double (&pm)[1 << LGS], double r0, double r1, unsigned long long &word, int &best,
                                        const Hook &hook = Hook(), unsigned char *bml = nullptr, const unsigned *gidx = nullptr,
                                        const Fill &fill = Fill()) {
    constexpr int type = TYPE;
    using C = SrCode<LGS, G0, G1>;
    constexpr bool GEN = G0 == 0 && G1 == 0;
    constexpr bool FILLED = !std::is_same<Fill, NoFill>::value;   // (FILLERS above)
    constexpr int S = 1 << LGS, H = S / 2;
    double m00, m01, m10, m11;
    if constexpr (LEAN && TYPE == CPX_VIT_SOFT) {                  // coded_bits.clip(-500, 500) (:719)
        r0 = clip500(r0);
        r1 = clip500(r1);
        soft_metrics_lean(r0, m00, m01);
        soft_metrics_lean(r1, m10, m11);
    } else {
        if (type == CPX_VIT_SOFT) {
            r0 = fmin(fmax(r0, -500.0), 500.0);
            r1 = fmin(fmax(r1, -500.0), 500.0);
        }
        bit_metrics_cw(type, r0, m00, m01);
        bit_metrics_cw(type, r1, m10, m11);
    }
    double bmv[4];                                                 // NumPy add.reduce, n < 8: sequential from 0
    if constexpr (LEAN) {
        bmv[0] = m00 + m10; bmv[1] = m00 + m11;
        bmv[2] = m01 + m10; bmv[3] = m01 + m11;
    } else {
        bmv[0] = (0.0 + m00) + m10; bmv[1] = (0.0 + m00) + m11;
        bmv[2] = (0.0 + m01) + m10; bmv[3] = (0.0 + m01) + m11;
    }
    unsigned da = 0, db = 0;                                       // decisions of states 0..H-1 / H..S-1
    hook.template at<0>();
    auto butterfly = [&](int j, double m_a0, double m_a1, double m_b0, double m_b1) {
        const int x = rotl<LGS>(2 * j, R), y = rotl<LGS>(2 * j + 1, R);
        const double a = pm[x], b = pm[y];                         // metrics of the predecessors 2j, 2j+1
        const double a0 = a + m_a0, a1 = b + m_a1;                 // into state j      (:629)
        const double b0 = a + m_b0, b1 = b + m_b1;                 // into state j + S/2
        if (TYPE == CPX_VIT_UNQUANTIZED) {
            pm[x] = acs_select(da, a0, a1);                        // state j     now lives in register rotl(j, R+1) = x
            pm[y] = acs_select(db, b0, b1);                        // state j+S/2 now lives in register y
        } else if (j == 0) {                                       // (j is a constant once the loop is unrolled)
            pm[x] = acs_min_first(da, a0, a1);
            pm[y] = acs_min_first(db, b0, b1);
        } else if constexpr (FILLED) {
            double ra = a0, rb = b0;
            acs_min_pair(da, db, ra, a1, rb, b1);
            pm[x] = ra;
            pm[y] = rb;
        } else {
            pm[x] = acs_min(da, a0, a1);
            pm[y] = acs_min(db, b0, b1);
        }
    };
    if constexpr (GEN) {
        // Round 5: the metric of "code c_j of butterfly j" is selected by VGPR INDEX MODE (s_set_gpr_idx_on, GFX9): the step's four
        // branch metrics sit in eight consecutive registers, the wave-uniform code arrives in a scalar register, and the four additions of
        // a butterfly read `v[base + 2 c]` / `v[base + 2 (c ^ 3)]` as their first operand -- the scalar unit, idle in this kernel, does the
        // selecting and the vector unit executes exactly the instructions of a compiled-in code.  (Rounds 3 / 4 parked the metrics as
        // (c, c ^ 3) pairs in an LDS table and read 16 bytes per butterfly: 32 LDS reads, their address adds and waits per step and
        // 64 - 98 values spilled to AGPRs: 1.94 ms on the config-2 geometry against 1.55 ms for compiled-in generators.)  The table is
        // pinned to v[248:255] because an index-mode operand must be named in the asm text; the mode is on for the four additions only
        // (it would redirect the first operand of EVERY vector instruction), and scripts/micro/gpr_idx_check.hip checks the addressing.
        typedef double cpx_d4 __attribute__((ext_vector_type(4)));
        // two tables: the metrics in code order and in REVERSED order -- code c ^ 3 = 3 - c sits at offset 2 c of the reversed one, so ONE
        // index serves all four additions of a butterfly.  With one wave per SIMD every instruction, scalar or not, costs an issue slot:
        // the first version (one table; s_bfe_u32 + on + s_xor_b32 + idx + off + three s_nop per butterfly) took 2.21 ms where the LDS
        // table took 1.94.  Now the mode is switched on once per step with index 0 -- harmless for every other vector instruction --
        // and a butterfly costs two scalar instructions: its index in, index 0 back.
        const cpx_d4 tab = {bmv[0], bmv[1], bmv[2], bmv[3]}, rtab = {bmv[3], bmv[2], bmv[1], bmv[0]};
        // (every statement that sets the index names m0 as clobbered -- s_set_gpr_idx_on / _idx write M0[7:0] -- and
        //  tests/test_isa_guards.py scans the built code object: between `on` and `off` nothing else may write or consume M0.)
        asm volatile("s_set_gpr_idx_on 0, 1" ::: "memory", "m0");
        auto acs_pair = [&](int j, double a0, double a1, double b0, double b1) {
            const int x = rotl<LGS>(2 * j, R), y = rotl<LGS>(2 * j + 1, R);
            if (TYPE == CPX_VIT_UNQUANTIZED) {
                pm[x] = acs_select(da, a0, a1);                    // state j     now lives in register rotl(j, R+1) = x
                pm[y] = acs_select(db, b0, b1);                    // state j+S/2 now lives in register y
            } else {
                pm[x] = acs_min(da, a0, a1);
                pm[y] = acs_min(db, b0, b1);
            }
        };
        if constexpr (H >= 4 && TYPE != CPX_VIT_UNQUANTIZED) {
            // two butterflies per statement, additions AND add-compare-selects (acs_min's three instructions, four times): three scalar
            // instructions per pair.  (Separate statements cost a wait state each: the compiler pads every boundary between two inline-asm
            // blocks with an s_nop -- 2.2 per butterfly when the selects were statements of their own.)
#pragma unroll
            for (int j = 0; j < H; j += 2) {
                if (j == H / 2) hook.template at<1>();          // (index 0 while it runs)
                const int x0 = rotl<LGS>(2 * j, R), y0 = rotl<LGS>(2 * j + 1, R), x1 = rotl<LGS>(2 * j + 2, R), y1 = rotl<LGS>(2 * j + 3, R);
                const double a = pm[x0], b = pm[y0], c = pm[x1], d = pm[y1];      // predecessors 2j, 2j+1 | 2j+2, 2j+3
                double a0, a1, b0, b1, c0, c1, d0, d1;             // (the four minima overwrite a0, b0, c0, d0)
                asm volatile("s_set_gpr_idx_idx %[i0]\n\t"
                             "v_add_f64 %[a0], v[248:249], %[a]\n\t"   // into state j:       predecessor 2j   + code c      (:629)
                             "v_add_f64 %[b1], v[248:249], %[b]\n\t"   // into state j + S/2: predecessor 2j+1 + code c
                             "v_add_f64 %[a1], v[240:241], %[b]\n\t"   // into state j:       predecessor 2j+1 + code c ^ 3
                             "v_add_f64 %[b0], v[240:241], %[a]\n\t"   // into state j + S/2: predecessor 2j   + code c ^ 3
                             "s_set_gpr_idx_idx %[i1]\n\t"
                             "v_add_f64 %[c0], v[248:249], %[c]\n\t"
                             "v_add_f64 %[d1], v[248:249], %[d]\n\t"
                             "v_add_f64 %[c1], v[240:241], %[d]\n\t"
                             "v_add_f64 %[d0], v[240:241], %[c]\n\t"
                             "s_set_gpr_idx_idx 0\n\t"
                             "v_cmp_lt_f64 vcc, %[a1], %[a0]\n\tv_addc_co_u32 %[da], vcc, %[da], %[da], vcc\n\tv_min_f64 %[a0], %[a0], %[a1]\n\t"
                             "v_cmp_lt_f64 vcc, %[b1], %[b0]\n\tv_addc_co_u32 %[db], vcc, %[db], %[db], vcc\n\tv_min_f64 %[b0], %[b0], %[b1]\n\t"
                             "v_cmp_lt_f64 vcc, %[c1], %[c0]\n\tv_addc_co_u32 %[da], vcc, %[da], %[da], vcc\n\tv_min_f64 %[c0], %[c0], %[c1]\n\t"
                             "v_cmp_lt_f64 vcc, %[d1], %[d0]\n\tv_addc_co_u32 %[db], vcc, %[db], %[db], vcc\n\tv_min_f64 %[d0], %[d0], %[d1]"
                             : [a0] "=&v"(a0), [a1] "=&v"(a1), [b0] "=&v"(b0), [b1] "=&v"(b1), [c0] "=&v"(c0), [c1] "=&v"(c1),
                               [d0] "=&v"(d0), [d1] "=&v"(d1), [da] "+v"(da), [db] "+v"(db)
                             : [i0] "s"(gidx[j]), [i1] "s"(gidx[j + 1]), [a] "v"(a), [b] "v"(b), [c] "v"(c), [d] "v"(d),
                               "{v[248:255]}"(tab), "{v[240:247]}"(rtab)
                             : "vcc", "m0");
                pm[x0] = a0; pm[y0] = b0;                          // state j now lives in register rotl(j, R+1) = x0, state j+S/2 in y0
                pm[x1] = c0; pm[y1] = d0;
            }
        } else {
#pragma unroll
            for (int j = 0; j < H; j++) {
                if (j == H / 2) hook.template at<1>();
                const double a = pm[rotl<LGS>(2 * j, R)], b = pm[rotl<LGS>(2 * j + 1, R)];
                double a0, a1, b0, b1;
                asm volatile("s_set_gpr_idx_idx %[ic]\n\t"
                             "v_add_f64 %[a0], v[248:249], %[a]\n\t"
                             "v_add_f64 %[b1], v[248:249], %[b]\n\t"
                             "v_add_f64 %[a1], v[240:241], %[b]\n\t"
                             "v_add_f64 %[b0], v[240:241], %[a]\n\t"
                             "s_set_gpr_idx_idx 0"
                             : [a0] "=&v"(a0), [a1] "=&v"(a1), [b0] "=&v"(b0), [b1] "=&v"(b1)
                             : [ic] "s"(gidx[j]), [a] "v"(a), [b] "v"(b), "{v[248:255]}"(tab), "{v[240:247]}"(rtab)
                             : "m0");
                acs_pair(j, a0, a1, b0, b1);
            }
        }
        asm volatile("s_set_gpr_idx_off" ::: "memory", "m0");
    } else {
#pragma unroll
        for (int j = 0; j < H; j++) {
            if (j == H / 2) hook.template at<1>();
            butterfly(j, bmv[C::code(j, 0)], bmv[C::code(j, 1)], bmv[C::code(j + H, 0)], bmv[C::code(j + H, 1)]);
        }
    }
    hook.template at<2>();
    int bst = 0;
    // 'soft', 64 states: FIRST-ARGMIN ON THE HIGH DWORDS.  The step needs the first-argmin state only, not the minimum, and every 'soft'
    // path metric is +0.0, a positive number or +inf -- never NaN, never negative, never -0.0 (the clip maps a NaN input to -500, the
    // per-bit metrics are >= +0.0 and never -0.0, see LEAN above, and metrics are only added and selected, see acs_min).  For such
    // doubles the numeric order IS the unsigned order of the 64-bit patterns, equal values have equal patterns, and +inf (0x7ff00000
    // 00000000) is simply the largest pattern in the domain.  Hence the minimum's high dword is the unsigned minimum of the 64 high dwords,
    // and the first-argmin state is one of the states whose high dword equals it (the "hits"): with exactly one hit that state IS the
    // first-argmin, whatever the low dwords hold.  The step needs that state's index and whether a lane has more than one hit, not a hit
    // bit per state, so it reads both off an 8 x 8 GRID of the high dwords, logical state s = 8 j + i in row j and column i: the eight row
    // minima, the eight column minima, m = the minimum of the column minima, and one 16-bit word of "row / column minimum == m" bits
    // (v_cmp_eq_u32 -> v_addc_co_u32, as the decision words are shifted in; columns in bits 15:8, rows in bits 7:0).  Every lane has at
    // least one hit row and one hit column.  Two different hit states differ in row or in column, so two row bits or two column bits are
    // set; and two set row (column) bits come from two different hit states: exactly two bits set <=> exactly one hit, the state
    // 8 j* + i* (tests/test_viterbi_argmin_rowcol_gpu.py asserts the identity on its metrics).  106 instructions (16 x 4 minima, 4 for m,
    // 16 x 2 hit bits, 6 for index and tie mask) where a hit bit per state took 166.  Column part first, then hook 3, then the rows three
    // at a time, each compared as soon as it exists: ten temporaries at most.
    // With two or more hits in any lane (an exact tie, or metrics that differ only in the low
    // dword) the whole wave runs the float64 tree and first-equal scan below and takes their result -- on the benchmark's input 0.54 % of
    // the wave-steps, 0.48 % of them the five all-tie steps of the zero tail (profiles/viterbi_argmin32_tie_rate.txt).  The branch is
    // wave-uniform (an SGPR pair written by one compare) and marked unlikely: the float64 block sits out of line, the step's hot path has
    // no taken branch, and the hook calls stay unconditional and in order.  (Measured issue costs: profiles/viterbi_argmin32_issue_cost.txt.)
    constexpr bool ARGMIN32 = LEAN && S == 64 && TYPE == CPX_VIT_SOFT && !GEN;   // the fused kernel, compiled-in generators
    unsigned long long tie = ~0ull;                                // lanes with more than one hit (hit word: not exactly two bits)
    // shifting the decisions in in increasing state order leaves state j of a half at bit H-1-j of its word; placing the
    // lower half on top puts state s at bit 63 - s of the 64-bit word: the traceback reads it as the top bit of (w << s)
    if constexpr (FILLED) word = ((unsigned long long)da << (64 - H)) | ((unsigned long long)db << (64 - S));   // (the ring write is a filler)
    static_assert(!FILLED || ARGMIN32, "fillers go between the statements of the 32-bit first-argmin");
    if constexpr (ARGMIN32) {
        // (state s sits in register rotl(s, R + 1): only a question of which operand is named)
#define CPX_HI(s) "v"(__double2hiint(pm[rotl<LGS>((s), R + 1)]))
#define CPX_COL(i) CPX_HI(i), CPX_HI((i) + 8), CPX_HI((i) + 16), CPX_HI((i) + 24), CPX_HI((i) + 32), CPX_HI((i) + 40), CPX_HI((i) + 48), CPX_HI((i) + 56)
#define CPX_ROW(j) CPX_HI(8 * (j)), CPX_HI(8 * (j) + 1), CPX_HI(8 * (j) + 2), CPX_HI(8 * (j) + 3), CPX_HI(8 * (j) + 4), CPX_HI(8 * (j) + 5), CPX_HI(8 * (j) + 6), CPX_HI(8 * (j) + 7)
        unsigned q0, q1, q2, q3, q4, q5, q6, q7, m, w;                 // column minima, the minimum, the hit word
        asm(CPX_COL_BLOCK3 : "=&v"(q0), "=&v"(q1), "=&v"(q2) : CPX_COL(0), CPX_COL(1), CPX_COL(2));
        asm(CPX_COL_BLOCK3 : "=&v"(q3), "=&v"(q4), "=&v"(q5) : CPX_COL(3), CPX_COL(4), CPX_COL(5));
        if constexpr (FILLED) pinned_fill<0>(fill, word);
        asm(CPX_COL_BLOCK_LAST : "=&v"(q6), "=&v"(q7), "=&v"(m), "=&v"(w) : "v"(q0), "v"(q1), "v"(q2), "v"(q3), "v"(q4), "v"(q5), CPX_COL(6), CPX_COL(7)
            : "vcc");
        hook.template at<3>();
        if constexpr (FILLED) pinned_fill<1>(fill, word);
        unsigned r0_, r1_, r2_;                                        // row minima: dead once compared
        asm(CPX_ROW_BLOCK3 : "+v"(w), "=&v"(r0_), "=&v"(r1_), "=&v"(r2_) : "v"(m), CPX_ROW(7), CPX_ROW(6), CPX_ROW(5) : "vcc");
        if constexpr (FILLED) pinned_fill<2>(fill, word);
        asm(CPX_ROW_BLOCK3 : "+v"(w), "=&v"(r0_), "=&v"(r1_), "=&v"(r2_) : "v"(m), CPX_ROW(4), CPX_ROW(3), CPX_ROW(2) : "vcc");
        if constexpr (FILLED) pinned_fill<3>(fill, word);
#ifdef CPX_AB_SCALAR_BEHIND_COMPARE
        constexpr bool TIE_FIRST = false;
#else
        constexpr bool TIE_FIRST = FILLED;
#endif
        if constexpr (TIE_FIRST)
            asm(CPX_ROW_BLOCK_LAST : "+v"(w), "=&v"(r0_), "=&v"(r1_), "=&v"(bst), "=&s"(tie) : "v"(m), CPX_ROW(1), CPX_ROW(0) : "vcc");
        else
            asm(CPX_ROW_BLOCK_LAST_INDEX_FIRST : "+v"(w), "=&v"(r0_), "=&v"(r1_), "=&v"(bst), "=&s"(tie) : "v"(m), CPX_ROW(1), CPX_ROW(0) : "vcc");
#undef CPX_ROW
#undef CPX_COL
#undef CPX_HI
    }
    if (__builtin_expect(tie != 0, !ARGMIN32)) {
        // first-argmin state (:645): the minimum (v_min_f64 tree, as viterbi.hip's cross-lane tree) and the first state equal to it
        double m0 = pm[0], m1 = pm[1 % S], m2 = pm[2 % S], m3 = pm[3 % S];
        if constexpr (S == 64) {
            // 60 v_min_f64 as three statements of four interleaved chains (viterbi_cw_asm.h: one statement per instruction cost an
            // s_nop per dependent pair and serialised the chains)
#define CPX_V4(a) "v"(pm[a]), "v"(pm[(a) + 1]), "v"(pm[(a) + 2]), "v"(pm[(a) + 3])
            asm(CPX_MIN_BLOCK24 : "+v"(m0), "+v"(m1), "+v"(m2), "+v"(m3)
                : CPX_V4(4), CPX_V4(8), CPX_V4(12), CPX_V4(16), CPX_V4(20), CPX_V4(24));
            asm(CPX_MIN_BLOCK24 : "+v"(m0), "+v"(m1), "+v"(m2), "+v"(m3)
                : CPX_V4(28), CPX_V4(32), CPX_V4(36), CPX_V4(40), CPX_V4(44), CPX_V4(48));
            asm(CPX_MIN_BLOCK12 : "+v"(m0), "+v"(m1), "+v"(m2), "+v"(m3) : CPX_V4(52), CPX_V4(56), CPX_V4(60));
#undef CPX_V4
        } else {
#pragma unroll
            for (int s = 4; s < S; s += 4) {
                m0 = vmin(m0, pm[s]); m1 = vmin(m1, pm[s + 1]); m2 = vmin(m2, pm[s + 2]); m3 = vmin(m3, pm[s + 3]);
            }
        }
        const double mn = vmin(vmin(m0, m1), vmin(m2, m3));
        if constexpr (!ARGMIN32) hook.template at<3>();
        if constexpr (S == 64) {
            // first state equal to the minimum, scanned downwards (a later, lower state overwrites): per four states four compares
            // into four SGPR pairs, then the four selects with inline-constant state numbers -- three instructions always sit
            // between a float64 compare and the select that reads its mask (back to back the pair needs two wait states).  Three
            // statements of 24 / 24 / 16 states (30 operands is the limit of one).
            unsigned long long k0, k1, k2, k3;
#define CPX_S4(a) "v"(pm[rotl<LGS>((a), R + 1)]), "v"(pm[rotl<LGS>((a) - 1, R + 1)]), "v"(pm[rotl<LGS>((a) - 2, R + 1)]), "v"(pm[rotl<LGS>((a) - 3, R + 1)])
            asm(CPX_SCAN_BLOCK0 : "+v"(bst), "=&s"(k0), "=&s"(k1), "=&s"(k2), "=&s"(k3)
                : "v"(mn), CPX_S4(63), CPX_S4(59), CPX_S4(55), CPX_S4(51), CPX_S4(47), CPX_S4(43));
            asm(CPX_SCAN_BLOCK1 : "+v"(bst), "=&s"(k0), "=&s"(k1), "=&s"(k2), "=&s"(k3)
                : "v"(mn), CPX_S4(39), CPX_S4(35), CPX_S4(31), CPX_S4(27), CPX_S4(23), CPX_S4(19));
            asm(CPX_SCAN_BLOCK2 : "+v"(bst), "=&s"(k0), "=&s"(k1), "=&s"(k2), "=&s"(k3)
                : "v"(mn), CPX_S4(15), CPX_S4(11), CPX_S4(7), CPX_S4(3));
#undef CPX_S4
        } else if constexpr (S % 4 == 0) {
#pragma unroll
            for (int s = S - 4; s >= 0; s -= 4) {
                unsigned long long k0, k1, k2, k3;
                asm("v_cmp_eq_f64 %1, %5, %9\n\tv_cmp_eq_f64 %2, %6, %9\n\tv_cmp_eq_f64 %3, %7, %9\n\tv_cmp_eq_f64 %4, %8, %9\n\t"
                    "v_cndmask_b32 %0, %0, %10, %1\n\tv_cndmask_b32 %0, %0, %11, %2\n\tv_cndmask_b32 %0, %0, %12, %3\n\t"
                    "v_cndmask_b32 %0, %0, %13, %4"
                    : "+v"(bst), "=&s"(k0), "=&s"(k1), "=&s"(k2), "=&s"(k3)
                    : "v"(pm[rotl<LGS>(s + 3, R + 1)]), "v"(pm[rotl<LGS>(s + 2, R + 1)]), "v"(pm[rotl<LGS>(s + 1, R + 1)]),
                      "v"(pm[rotl<LGS>(s, R + 1)]), "v"(mn), "n"(s + 3), "n"(s + 2), "n"(s + 1), "n"(s));   // inline constants
            }
        } else {
#pragma unroll
            for (int s = S - 1; s >= 0; s--) bst = (pm[rotl<LGS>(s, R + 1)] == mn) ? s : bst;
        }
    }
    if constexpr (!FILLED) word = ((unsigned long long)da << (64 - H)) | ((unsigned long long)db << (64 - S));
    best = bst;
}

// ---- float32 path metrics: the "fp32-fast" mode (cpx_set_precision) -- NOT the parity mode ------------------
// 'soft' and 'unquantized' metrics in float32; the soft branch metric is the correlation form (the term common to all
// branches of a step is dropped: no exp, no log), and near-ties between path metrics may resolve differently (measured
// mismatch rate: DESIGN.md 4.1).  'hard' metrics of 0/1 inputs are Hamming distances <= 2 T, exact in float32
// for T < 2^22: identical bits.
// Same structure as cw_step: in-place butterflies, decision words, first-argmin state; the minimum tree uses v_min3_f32.
__device__ __forceinline__ float acs_min_f32(unsigned &acc, float x, float y) {
    float r;
    asm("v_cmp_lt_f32 vcc, %3, %2\n\tv_addc_co_u32 %1, vcc, %1, %1, vcc\n\tv_min_f32 %0, %2, %3"
        : "=&v"(r), "+v"(acc) : "v"(x), "v"(y) : "vcc");
    return r;
}
__device__ __forceinline__ float vmin3_f32(float a, float b, float c) {
    float r;
    asm("v_min3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}
__device__ __forceinline__ void bit_metrics_f32(int type, double r, float &m0, float &m1) {
    if (type == CPX_VIT_HARD) {
        const long long ri = (long long)r;
        m0 = (float)(ri ^ 0ll);
        m1 = (float)(ri ^ 1ll);
    } else if (type == CPX_VIT_SOFT) {
        // the reference's metrics are m0 = log(e^r + 1), m1 = m0 - r: every branch of a step carries the same
        // m0(r0) + m0(r1), which cannot change a comparison between paths of equal length -- the fast mode drops it
        // (correlation metric, SURVEY Appendix C: 0 flipped bits of 263 680 against the reference) and with it the exp and
        // the log of every received value
        m0 = 0.0f;
        m1 = -(float)r;
    } else {
        const float x = (float)r, d0 = x + 1.0f, d1 = x - 1.0f;
        m0 = d0 * d0;
        m1 = d1 * d1;
    }
}

template <int LGS, unsigned G0, unsigned G1, int TYPE, int R, bool LEAN = false, class Hook = NoHook>   // (LEAN: float64 only, ignored here)
__device__ __forceinline__ void cw_step(float (&pm)[1 << LGS], double r0, double r1, unsigned long long &word, int &best,
                                        const Hook &hook = Hook(), unsigned char * = nullptr, const unsigned * = nullptr) {
    using C = SrCode<LGS, G0, G1>;
    constexpr int S = 1 << LGS, H = S / 2;
    if (TYPE == CPX_VIT_SOFT) {                                    // coded_bits.clip(-500, 500) (:719)
        r0 = fmin(fmax(r0, -500.0), 500.0);
        r1 = fmin(fmax(r1, -500.0), 500.0);
    }
    float m00, m01, m10, m11;
    bit_metrics_f32(TYPE, r0, m00, m01);
    bit_metrics_f32(TYPE, r1, m10, m11);
    float bmv[4];
    bmv[0] = (0.0f + m00) + m10; bmv[1] = (0.0f + m00) + m11;
    bmv[2] = (0.0f + m01) + m10; bmv[3] = (0.0f + m01) + m11;
    unsigned da = 0, db = 0;
    hook.template at<0>();
#pragma unroll
    for (int j = 0; j < H; j++) {
        if (j == H / 2) hook.template at<1>();
        const int x = rotl<LGS>(2 * j, R), y = rotl<LGS>(2 * j + 1, R);
        const float a = pm[x], b = pm[y];
        const float a0 = a + bmv[C::code(j, 0)], a1 = b + bmv[C::code(j, 1)];
        const float b0 = a + bmv[C::code(j + H, 0)], b1 = b + bmv[C::code(j + H, 1)];
        pm[x] = acs_min_f32(da, a0, a1);
        pm[y] = acs_min_f32(db, b0, b1);
    }
    hook.template at<2>();
    float mn;
    if constexpr (S >= 8 && S % 8 == 0) {
        float m0 = pm[0], m1 = pm[1], m2 = pm[2], m3 = pm[3];
#pragma unroll
        for (int s = 4; s + 8 <= S; s += 8) {
            m0 = vmin3_f32(m0, pm[s], pm[s + 1]); m1 = vmin3_f32(m1, pm[s + 2], pm[s + 3]);
            m2 = vmin3_f32(m2, pm[s + 4], pm[s + 5]); m3 = vmin3_f32(m3, pm[s + 6], pm[s + 7]);
        }
        m0 = vmin3_f32(m0, pm[S - 4], pm[S - 3]);
        m1 = vmin3_f32(m1, pm[S - 2], pm[S - 1]);
        mn = fminf(vmin3_f32(m0, m1, m2), m3);
    } else {
        mn = pm[0];
#pragma unroll
        for (int s = 1; s < S; s++) mn = fminf(mn, pm[s]);
    }
    hook.template at<3>();
    int bst = 0;
    if constexpr (S % 4 == 0) {
#pragma unroll
        for (int s = S - 4; s >= 0; s -= 4) {
            unsigned long long k0, k1, k2, k3;
            asm("v_cmp_eq_f32 %1, %5, %9\n\tv_cmp_eq_f32 %2, %6, %9\n\tv_cmp_eq_f32 %3, %7, %9\n\tv_cmp_eq_f32 %4, %8, %9\n\t"
                "v_cndmask_b32 %0, %0, %10, %1\n\tv_cndmask_b32 %0, %0, %11, %2\n\tv_cndmask_b32 %0, %0, %12, %3\n\t"
                "v_cndmask_b32 %0, %0, %13, %4"
                : "+v"(bst), "=&s"(k0), "=&s"(k1), "=&s"(k2), "=&s"(k3)
                : "v"(pm[rotl<LGS>(s + 3, R + 1)]), "v"(pm[rotl<LGS>(s + 2, R + 1)]), "v"(pm[rotl<LGS>(s + 1, R + 1)]),
                  "v"(pm[rotl<LGS>(s, R + 1)]), "v"(mn), "n"(s + 3), "n"(s + 2), "n"(s + 1), "n"(s));
        }
    } else {
#pragma unroll
        for (int s = S - 1; s >= 0; s--) bst = (pm[rotl<LGS>(s, R + 1)] == mn) ? s : bst;
    }
    word = ((unsigned long long)da << (64 - H)) | ((unsigned long long)db << (64 - S));
    best = bst;
}

// Workgroups of four wavefronts (one group of 64 codewords each): the four waves of a workgroup land on the four SIMDs
// of one CU, so 256 workgroups put exactly one wave on every SIMD of the chip.  (With single-wave workgroups the
// dispatcher packed two waves per SIMD on half of the CUs for B = 65536: 2.98 ms instead of 1.75 ms.)
constexpr int ACS_WAVES = 4;

template <int LGS, unsigned G0, unsigned G1, int TYPE>
__global__ __launch_bounds__(64 * ACS_WAVES) void viterbi_cw_acs_kernel(CwParams p) {
    constexpr int S = 1 << LGS;
    const int lane = threadIdx.x & 63;
    const int64_t grp = (int64_t)blockIdx.x * ACS_WAVES + (threadIdx.x >> 6);
    const int64_t cw = grp * 64 + lane;
    if (grp * 64 >= p.B) return;                                                   // whole wave beyond the batch
    const bool valid = cw < p.B;
    const double *x = p.coded + (valid ? cw : 0) * p.len;
    unsigned long long *dec = p.dec + grp * p.Tp * 64 + lane;                      // rows of steps T+1..Tp: never read
    unsigned char *best = p.best + grp * p.Tp * 64 + lane;

    double pm[S];
#pragma unroll
    for (int s = 0; s < S; s++) pm[s] = (s == 0) ? 0.0 : __builtin_huge_val();   // path_metrics[:,0] = inf, [0][0] = 0 (:705-706)

    const double pad = (TYPE == CPX_VIT_UNQUANTIZED) ? -1.0 : 0.0;                // t > L//k -> padding (:722-734)
    // step indices are 32-bit (the dispatcher guarantees T < 2^31): the scalar unit has no signed 64-bit compare, and
    // 64-bit step arithmetic put ~20 VALU instructions per step of purely wave-uniform work into the hot loop
    const int T = (int)p.T, tmax = (int)((p.Lk < p.T) ? p.Lk : p.T);              // tmax: last step with received values (>= 1)
    auto load = [&](int t) {                                                      // always a valid address; padded below
        const int tc = (t < tmax) ? t : tmax;
        return *reinterpret_cast<const double2 *>(x + (int64_t)(tc - 1) * 2);
    };
    double2 cur[LGS], nxt[LGS];
#pragma unroll
    for (int u = 0; u < LGS; u++) cur[u] = load(1 + u);
    unsigned long long nanmask = 0;                                               // 'soft': lanes that received a NaN
    // groups of LGS steps; a partial last group simply runs on (steps > T see padding, their rows are never read)
    for (int t = 1; t <= T; t += LGS) {
#pragma unroll
        for (int u = 0; u < LGS; u++) nxt[u] = load(t + LGS + u);                // prefetch: lands during this group
#pragma unroll
        for (int u = 0; u < LGS; u++) {
            const bool have = t + u <= tmax;
            cur[u].x = have ? cur[u].x : pad;
            cur[u].y = have ? cur[u].y : pad;
        }
        unsigned long long *d = dec + (int64_t)(t - 1) * 64;
        unsigned char *b = best + (int64_t)(t - 1) * 64;
        auto one = [&](auto rtag, const double2 &v) {
            constexpr int R = decltype(rtag)::value;
            unsigned long long word;
            int bst;
            if constexpr (TYPE == CPX_VIT_SOFT) nan_or(nanmask, v.x, v.y);
            cw_step<LGS, G0, G1, TYPE, R>(pm, v.x, v.y, word, bst);
            d[R * 64] = word;
            b[R * 64] = (unsigned char)bst;
        };
        if constexpr (LGS >= 1) one(std::integral_constant<int, 0>{}, cur[0]);
        if constexpr (LGS >= 2) one(std::integral_constant<int, 1>{}, cur[1 % LGS]);
        if constexpr (LGS >= 3) one(std::integral_constant<int, 2>{}, cur[2 % LGS]);
        if constexpr (LGS >= 4) one(std::integral_constant<int, 3>{}, cur[3 % LGS]);
        if constexpr (LGS >= 5) one(std::integral_constant<int, 4>{}, cur[4 % LGS]);
        if constexpr (LGS >= 6) one(std::integral_constant<int, 5>{}, cur[5 % LGS]);
#pragma unroll
        for (int u = 0; u < LGS; u++) cur[u] = nxt[u];
    }
    // One flag per ITEM of the redo kernel = 64 / S consecutive codewords (viterbi_dispatch reads them that way); the two-kernel form
    // is only instantiated for 64 states, where an item is one codeword and this per-codeword store IS the per-item one.
    static_assert(LGS == 6, "viterbi_cw_acs_kernel writes per-codeword NaN flags: valid for 64-state trellises only (items of one codeword)");
    if constexpr (TYPE == CPX_VIT_SOFT)
        if (valid) p.nanflags[cw] = (uint8_t)((nanmask >> lane) & 1ull);
}

// ---- fused variant: add-compare-select AND sliding traceback in one kernel, no workspace in HBM -------------------------
// For the default traceback depth of the K = 7 code (tb_depth = 5 m = 30, H = tb - 2 = 28 hops) the decision words never
// leave the CU: every wave keeps the last 32 words of its 64 codewords in an LDS ring [slot][lane] (conflict-free, each
// lane reads only its own column) and, right after the add-compare-select of step t, walks the H hops back from the
// step's first-argmin state -- 2 VALU instructions per hop (tb_hop), LDS addresses that do not depend on the states, the
// whole walk straight-line code whose LDS reads are spread over the next step's arithmetic (WalkHook).  The ring is stored
// twice, 32 slots apart, so that the H + 1 words of a walk sit at constant offsets below one base address.  The decoded
// bit of step t - H goes to a staging tile in LDS and the tile is written out every 96 steps, one coalesced 64-byte
// store per codeword and half-tile.  HBM traffic is the algorithmic one again (the two-kernel path moves 9 B per
// codeword-step through a workspace and back).
constexpr int FR_RING = 32, FR_CHUNK = 96, FR_OBPAD = 100;     // ring slots (mirrored), steps per flush (a multiple of LGS), tile row bytes
// Traceback depths above the default (tb_depth 31 .. 48 for K = 7) run the same kernel on a ring of FR_RING_DEEP slots that is
// NOT mirrored -- the same LDS per wave (64 slots once instead of 32 twice) --: a walk's words then wrap around the ring and
// every hop forms its own LDS address, ((q - h) mod 64) * 512 + lane * 8: one more vector add per hop (+6 % per step with 46
// hops).  Round 2 sent these depths to the two-kernel form (1.66 x the time: decision words through HBM and back).
constexpr int FR_RING_DEEP = 64;

// slots of one wave: the ring (twice if mirrored) + one dummy slot per copy for steps > T
template <int RING, bool MIR> constexpr int fused_slots() { return MIR ? 2 * RING + 2 : RING + 1; }
template <int RING, bool MIR, bool GEN = false>
constexpr size_t fused_wave_lds() {
    // ring + dummy slot(s), staging tile
    return (size_t)fused_slots<RING, MIR>() * 64 * 8 + (size_t)64 * FR_OBPAD;   // (GEN: rounds 3 / 4 kept an LDS table of 4 KB here)
}

// The traceback walk of one step.  Its LDS reads are cut into four batches that cw_step's hook ISSUES between the phases of the NEXT
// step, so their latency hides behind the add-compare-select arithmetic (left to itself the compiler emits the walk as 14 read ->
// wait -> 2-hop rounds at the end of the step: +0.5 ms); sched_barrier pins the batches where they are put.  In the LATE form (below) the
// hops all run in finish(), behind ONE wait for the LDS counter: the youngest read was issued before the row part of the first-argmin, the
// others hundreds of instructions earlier, and with one wave per SIMD every counted wait in front of a pair of hops is an issue slot of
// its own even when it never waits (the compiler counted the reads down one by one: 13 waits per step).  The wait is the builtin, not an
// asm statement, so that the compiler's own wait insertion knows the counter is zero behind it and adds nothing; it names the LDS
// counter only (vmcnt and expcnt at their maxima): the next group's LLR prefetch stays in flight.
//
// WHICH HOPS A WALK NEEDS.  The state of a walk is never masked (tb_hop): after n hops its bit k is the bit shifted in at hop n - k
// (k < n) or bit k - n of the start state.  The output of a walk of H hops, bit LGS - 1 of its final state, is therefore bit sh of the
// state after he hops, he = max(H - (LGS - 1), 0), sh = LGS - 1 - min(H, LGS - 1) (tests/test_viterbi_walk_stop.py): the last LGS - 1
// hops and the ring words they read cannot change it.
//  * compile-time hop count (!RT): all H hops stand in the source and the compiler's dead-code elimination removes the last LGS - 1
//    and their reads by itself (23 of the 28 hops of the K = 7 default depth are in the code object) -- nothing to "add back".
//  * RT: the number of hops is a run-time value (traceback depths below the flavour's own), every compiled hop slot runs and slots
//    h >= he leave the state alone (one v_cndmask each; their LDS reads still go to valid, older ring slots).  The select hides the
//    identity from the compiler, so it is spelled out: only NH = H - (LGS - 1) slots are compiled and loaded, he and sh come from the
//    caller as wave-uniform values.
constexpr int WAIT_LGKM0 = 0xC07F;          // s_waitcnt simm16 (gfx9): vmcnt 63 (bits 15:14, 3:0), expcnt 7 (6:4), lgkmcnt 0 (11:8)
//
// LATE selects the single-wait form.  It is on exactly where the step has the tie branch of the 32-bit first-argmin ('soft', 64 states,
// float64, compiled-in generators): there the compiler sinks the hops behind the branch's join whatever the source says, so all NH words
// are live until finish() anyway and the single wait costs no register.  Every other flavour has no such branch; its hops really run
// between the phases, batch P - 1 at hook P and the last batch in finish(), with PER words live at a time -- holding all NH words to the
// end of the step there cost up to 32 AGPRs and the first VGPR spills (experiments/README.md), so those flavours keep the batched hops.
template <int LGS, int H, bool RT = false, int RING = FR_RING, bool MIR = true, bool LATE = false>
struct WalkHook {
    static constexpr int NH = RT ? (H > LGS - 1 ? H - (LGS - 1) : 0) : H;   // compiled hop slots
    static constexpr int NB = 4, PER = (NH + NB - 1) / NB;
    // MIR: ring pointer of the walked step t': word of step t' - h at pw[(RING - h) * 64].  Not mirrored: pw = this lane's
    // column, q = ring slot of step t' (wave-uniform), word of step t' - h at pw[((q - h) mod RING) * 64].
    const unsigned long long *pw;
    int q;
    mutable unsigned st;                    // state of the walk
    int he, sh;                             // RT: hops to execute, bit of the state to take after them (!RT: H, LGS - 1)
    mutable unsigned long long buf[LATE ? (NH > 0 ? NH : 1) : (PER > 0 ? PER : 1)];   // LATE: word h in buf[h]; else batch B, word i in buf[i]
    __device__ __forceinline__ unsigned long long word(int h) const {
        return MIR ? pw[(RING - h) * 64] : pw[((q - h) & (RING - 1)) * 64];
    }
    template <int B> __device__ __forceinline__ void issue() const {       // the reads of batch B
#pragma unroll
        for (int i = 0; i < PER; i++)
            if (B * PER + i < NH) buf[LATE ? B * PER + i : i] = word(B * PER + i);
    }
    template <int B> __device__ __forceinline__ void hops() const {        // the hops of batch B
#pragma unroll
        for (int i = 0; i < PER; i++)
            if (B * PER + i < NH) {
                const unsigned nx = tb_hop<LGS>(buf[LATE ? B * PER + i : i], st);
                st = (!RT || B * PER + i < he) ? nx : st;
            }
    }
    template <int P> __device__ __forceinline__ void at() const {
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (!LATE && P > 0) hops<P - 1>();
        issue<P>();
        __builtin_amdgcn_sched_barrier(0);
    }
    __device__ __forceinline__ void finish() const {
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (LATE) {
            if constexpr (NH > 0) {
                __builtin_amdgcn_s_waitcnt(WAIT_LGKM0);
                asm volatile("" : "+v"(st));    // every hop reads st: none of them is moved above the wait (the hops are pure arithmetic)
            }
            hops<0>(); hops<1>(); hops<2>(); hops<3>();
        } else {
            hops<NB - 1>();
        }
        __builtin_amdgcn_sched_barrier(0);
    }
    __device__ __forceinline__ unsigned bit() const { return (st >> (RT ? sh : LGS - 1)) & 1u; }   // the walk's output
};

// THE BURST FORM: the LGS walks of a group in one go (LATE flavours with a compile-time hop count on the mirrored ring).  The walk of
// step s reads the words of steps s .. s - NHE + 1, the walk of step s + 1 all but one of them again: walked one per step, every ring word
// is fetched NHE times.  Here steps R = 0 .. LGS - 2 of a group starting at step t run with no walk at all (NoHook: no ring read, no wait,
// no hop, no tile byte) and step R = LGS - 1 carries the walks of steps t - 1 .. t + LGS - 2 -- the walk left pending by the previous
// group and this group's first LGS - 1; the walk of step t + LGS - 1 stays pending, as one walk is pending in the other form.  Together
// they name NW = NHE + LGS - 1 distinct words (28 for the K = 7 default depth, not 6 x 23), the word of step t + LGS - 2 - d at
// pb[(RING - d) * 64], pb = the ring slot of step t + LGS - 2: adjacent slots, fetched in pairs, each word once per group, issued in four
// batches at the hook points of that one step (newest words first: the hops need them first) and used by up to LGS walks from registers.
// All hops run in finish() behind one wait, the LGS chains interleaved (they are independent).
// Only the hops the output can see are written (NHE = H - (LGS - 1), output = bit 0 of the state: see above).
// RING SAFETY.  When the burst reads, the newest slot written is that of step t + LGS - 2 (every LDS access of a wave is executed in
// order) and the oldest word it needs is d = NW - 1, hop NHE - 1 of the pending walk.  The ring holds d = 0 .. RING - 1; the write of step
// t + LGS - 1 comes after finish() and replaces d = RING - 1.  Hence NHE + LGS <= RING (asserted in the kernel; one slot to spare).
// tests/test_viterbi_walk_burst.py models the schedule slot by slot, across the ring wrap and the chunk boundary.
// RT (a traceback depth below the flavour's own): all NHE hop slots run and slots h >= he leave the state alone, as in WalkHook; their
// reads go to the same NW slots.
template <int LGS, int NHE, int RING, bool RT>
struct WalkBurst {
    static constexpr int NW = NHE + LGS - 1;                      // distinct words of the LGS walks
    static constexpr int NB = 4, PER = 2 * ((NW + 2 * NB - 1) / (2 * NB));   // words per batch: even, so that a batch is whole pairs of slots
    const unsigned long long *pb;           // ring slot (lower copy) of step t + LGS - 2
    int he, sh;                             // RT: hops to execute, bit of the state to take after them (!RT: NHE, 0)
    mutable unsigned st[LGS];               // st[k]: state of the walk of step t - 1 + k (before finish(): the step's first-argmin state)
    mutable unsigned long long w[NW];       // w[d]: word of step t + LGS - 2 - d
    template <int P> __device__ __forceinline__ void at() const {
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int i = 0; i < PER; i++)
            if (P * PER + i < NW) w[P * PER + i] = pb[(RING - (P * PER + i)) * 64];
        __builtin_amdgcn_sched_barrier(0);
    }
    __device__ __forceinline__ void finish() const {
        static_assert(LGS == 6, "the walk states are named one by one below");
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_waitcnt(WAIT_LGKM0);
        asm volatile("" : "+v"(st[0]), "+v"(st[1]), "+v"(st[2]), "+v"(st[3]), "+v"(st[4]), "+v"(st[5]));   // no hop moves above the wait (WalkHook)
#pragma unroll
        for (int h = 0; h < NHE; h++) {
#pragma unroll
            for (int k = 0; k < LGS; k++) {
                const unsigned nx = tb_hop<LGS>(w[LGS - 1 - k + h], st[k]);
                st[k] = (!RT || h < he) ? nx : st[k];
            }
        }
        __builtin_amdgcn_sched_barrier(0);
    }
    __device__ __forceinline__ unsigned bit(int k) const { return (st[k] >> (RT ? sh : 0)) & 1u; }   // the output of walk k (!RT: sh = 0 after NHE hops)
};

template <int LGS, unsigned G0, unsigned G1, int TYPE, int HT, bool RT = false, class F = double, int RING = FR_RING, bool MIR = true>
__global__ __launch_bounds__(64 * ACS_WAVES) void viterbi_cw_fused_kernel(CwParams p) {
    constexpr int S = 1 << LGS, FR_GROUPS = FR_CHUNK / LGS, CHUNK = FR_GROUPS * LGS;
    static_assert(HT >= 0 && HT + 1 <= RING && (RING & (RING - 1)) == 0 && CHUNK + 1 <= FR_OBPAD, "ring / tile too small");
    const int H = RT ? p.tb - 2 : HT;                                              // hops of a walk = tb_depth - 2
    constexpr bool GEN = G0 == 0 && G1 == 0;                                        // table-driven code (cw_step)
#ifdef CPX_VIT_SPEC_LG
    // per-pair code object (see the end of the file): launched through hipModuleLaunchKernel, whose functions have no
    // "dynamic LDS above 64 KiB" attribute to raise -- the ring and the tiles are a static array of the same size instead
    __shared__ __attribute__((aligned(16))) unsigned char smem[ACS_WAVES * fused_wave_lds<RING, MIR, GEN>()];
#else
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
#endif
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t grp = (int64_t)blockIdx.x * ACS_WAVES + wv;
    const int64_t cw = grp * 64 + lane;
    if (grp * 64 >= p.B) return;                                                   // whole wave beyond the batch
    if constexpr (LGS == 6 && !MIR && !GEN && RING == FR_RING) __builtin_amdgcn_s_setprio(3);   // the Lean32 flavour: another kernel's waves share the SIMD
    const bool valid = cw < p.B;
    const double *x = p.coded + (valid ? cw : 0) * p.len;
    static_assert(!GEN || (!MIR && std::is_same<F, double>::value), "table-driven codes: unmirrored ring, float64");
    unsigned long long *ring = reinterpret_cast<unsigned long long *>(smem + (size_t)wv * fused_wave_lds<RING, MIR, GEN>());
    unsigned char *obuf = reinterpret_cast<unsigned char *>(ring + fused_slots<RING, MIR>() * 64);
    unsigned long long *mycol = ring + lane;                                       // slot s of this lane's codeword: mycol[s * 64]
    unsigned char *myrow = obuf + lane * FR_OBPAD;

    F pm[S];
#pragma unroll
    for (int s = 0; s < S; s++) pm[s] = (s == 0) ? (F)0.0 : (F)__builtin_huge_val();   // path_metrics[:,0] = inf, [0][0] = 0 (:705-706)
    // table-driven codes: the register offset 2 c_j of every butterfly, unpacked once into scalar registers (cw_step, GEN)
    unsigned gidx[GEN ? S / 2 : 1];
#pragma unroll
    for (int j = 0; j < (GEN ? S / 2 : 1); j++) gidx[j] = GEN ? __builtin_amdgcn_ubfe(p.goff[j >> 3], 4 * (j & 7), 4) : 0u;

    const double pad = (TYPE == CPX_VIT_UNQUANTIZED) ? -1.0 : 0.0;                // t > L//k -> padding (:722-734)
    const int T = (int)p.T, tmax = (int)((p.Lk < p.T) ? p.Lk : p.T);              // 32-bit step indices, see the ACS kernel
    auto load = [&](int t) {                                                      // always a valid address; padded at use
        const int tc = (t < tmax) ? t : tmax;
        return *reinterpret_cast<const double2 *>(x + (int64_t)(tc - 1) * 2);
    };
    double2 cur[LGS];
#pragma unroll
    for (int u = 0; u < LGS; u++) cur[u] = load(1 + u);
    int best_T = 0;                                                               // first-argmin state of step T
    unsigned long long nanmask = 0;                                               // 'soft': lanes that received a NaN
    constexpr bool LATE = LGS == 6 && TYPE == CPX_VIT_SOFT && !GEN && std::is_same<F, double>::value;   // cw_step's ARGMIN32 (WalkHook)
    WalkHook<LGS, HT, RT, RING, MIR, LATE> walk;                                             // walk of the previous step (step 0: a dummy)
    walk.pw = mycol;
    walk.q = 0;
    walk.st = 0;
    walk.he = H > LGS - 1 ? H - (LGS - 1) : 0;                                     // (WalkHook: the hops the output bit can see)
    walk.sh = H > LGS - 1 ? 0 : LGS - 1 - H;
    // the burst form (WalkBurst): `walk` then only carries the pending walk (pw, st) to the end of the last chunk.  Deep64 and Lean32
    // (rings stored once) and every flavour that is not LATE keep the walk per step.
    constexpr bool BURST = LATE && MIR && HT > LGS - 1;
    // the step with its own work pinned between the first-argmin statements (cw_step, FILLERS): Mirrored32 at the default depth and Lean32.
    // Not the run-time-hop kernels (every depth below the default, Deep64): at their scalar-register ceiling the six pairs of the NaN
    // tests are spilled inside the loop, measured +1.8 % and +1.0 %.
    constexpr bool PIN = LATE && !RT;
    constexpr int NHE = BURST ? HT - (LGS - 1) : 1;                                 // hop slots: the hops the output can see
    static_assert(!BURST || NHE + LGS <= RING, "ring too small for the words of LGS walks at once");
    WalkBurst<LGS, NHE, RING, RT> burst;
    burst.pb = mycol;
    burst.he = walk.he;
    burst.sh = walk.sh;
#pragma unroll
    for (int k = 0; k < LGS; k++) burst.st[k] = 0;                                 // st[0]: the pending walk (step 0: a dummy)

    // writes the decoded bits staged in tile entries 0 .. n-1: entry li holds the result of the walk of step tc0 + li - 1,
    // i.e. output step so = tc0 + li - 1 - H, and is written when 1 <= so <= min(T - H, L).  Those bounds are wave-uniform, so the
    // entries to write are one range [lo, hi) per flush, worked out on the scalar unit; a lane's two entries (lane, lane + 64) get one
    // predicate each per flush instead of five terms per store, and a store's address is a scalar row pointer (advanced by L per
    // codeword) plus a 32-bit lane offset.  (Before: 64-bit vector index arithmetic and the whole predicate in front of each of the 128
    // byte stores, ~220 instructions per round of eight codewords.)
    const int so_max = (int)((p.L < (int64_t)(T - H)) ? p.L : (int64_t)(T - H));   // last output step the flushes write (may be < 1)
    auto flush = [&](int tc0, int n) {
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                         // the tile rows are complete (same wave wrote them)
        const int64_t cwb = grp * 64;
        const int ncw = (int)((p.B - cwb < 64) ? (p.B - cwb) : 64);
        const int so0 = tc0 - 1 - H;                                               // output step of entry 0
        const int lo = so0 >= 1 ? 0 : 1 - so0;
        const int hi = (so_max - so0 + 1 < n) ? so_max - so0 + 1 : n;
        if (lo < hi) {
            const bool w0 = lane >= lo && lane < hi, w1 = lane + 64 >= lo && lane + 64 < hi;
            const unsigned o0 = (unsigned)(lane - lo), o1 = o0 + 64u;              // byte offsets from entry lo (used where w0 / w1 hold)
            const int l1 = (lane + 64 < FR_OBPAD) ? lane + 64 : FR_OBPAD - 1;      // entries >= n are never written: read inside the row
            unsigned char *row = p.bits + cwb * p.L + (so0 + lo - 1);              // entry lo of the group's first codeword
            // eight codewords per round: their LDS reads are all in flight before the first store waits for one (one codeword
            // per round put an LDS round trip in front of every store: ~19 k cycles per 96 steps, 5 % of the kernel)
            for (int c0 = 0; c0 < ncw; c0 += 8) {
                unsigned char v[8][2];
#pragma unroll
                for (int u = 0; u < 8; u++) {
                    v[u][0] = obuf[(c0 + u) * FR_OBPAD + lane];
                    v[u][1] = obuf[(c0 + u) * FR_OBPAD + l1];
                }
                if (c0 + 8 <= ncw) {                                               // (always, but for the batch's last group)
                    if (w0) {
#pragma unroll
                        for (int u = 0; u < 8; u++) row[(int64_t)u * p.L + o0] = v[u][0];
                    }
                    if (w1) {
#pragma unroll
                        for (int u = 0; u < 8; u++) row[(int64_t)u * p.L + o1] = v[u][1];
                    }
                } else {
#pragma unroll
                    for (int u = 0; u < 8; u++)
                        if (c0 + u < ncw) {
                            if (w0) row[(int64_t)u * p.L + o0] = v[u][0];
                            if (w1) row[(int64_t)u * p.L + o1] = v[u][1];
                        }
                }
                row += 8 * p.L;
            }
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                         // tile read before the next chunk overwrites it
    };

    // One group of LGS steps starting at step t; `tile` = the lane's tile entry of step t.  Two bodies:
    //  * FAST: every step of the group AND every step of the prefetch it issues for the next group carries received values and lies
    //    inside [1, T] (t + 2 LGS - 1 <= tmax <= T).  Then `have` and `live` below hold for all LGS steps, the prefetch clamp is the
    //    identity and step T is not among them: the pad selects, the clamp, the dummy-slot selects of the ring write(s) and the best_T
    //    select are not compiled in.  With the selects gone the two stores of the mirrored ring sit a constant RING slots apart.
    //  * general: any group (the body of every group before the split) -- the last groups of a codeword, all of them for T < 2 LGS.
    // The values are the same either way: the fast body drops selects whose condition is known, never an operation on a metric.
    auto group = [&](auto ftag, const int t, unsigned char *tile) __attribute__((always_inline)) {
        constexpr bool FAST = decltype(ftag)::value;
        // prefetch of the NEXT group, all of it at the top of this one: a whole group (~4700 instructions) lies between
        // a load and the vmcnt(0) the compiler puts at the loop head.  (Reloading cur[R] inside step R saved 12
        // registers but left the youngest load only one step of lead: rocprofv3 showed 14.5 % of the wave cycles
        // parked in s_waitcnt.)
        double2 nxt[LGS];
        const double2 *xt = reinterpret_cast<const double2 *>(x) + (t - 1);   // FAST: one address per group, the steps are immediate offsets
#pragma unroll
        for (int u = 0; u < LGS; u++) nxt[u] = FAST ? xt[LGS + u] : load(t + LGS + u);
        auto one = [&](auto rtag) {
            constexpr int R = decltype(rtag)::value;
            const int tt = t + R;
            const bool have = FAST || tt <= tmax;
            const double r0 = have ? cur[R].x : pad, r1 = have ? cur[R].y : pad;
            unsigned long long word;
            int bst;
            // What the step does besides its arithmetic, in four pieces: the address of the ring slot of step tt, the NaN test of the step's
            // two values, the write of the decision word to the slot and (mirrored ring) its copy RING slots above, the OR into the NaN
            // mask.  The (at most LGS - 1) steps > T of the last group write to two dummy slots instead: the ring must keep the words of
            // steps T-H+1 .. T for the final walk.  PIN: cw_step places the pieces between its first-argmin statements (FILLERS); otherwise
            // the NaN test stands in front of the step and the ring write behind the walk, as they always did.
            unsigned long long nank = 0;                                      // lanes whose step received a NaN
            int q = 0;
            unsigned long long *wb = nullptr;
            auto fill = [&](auto ptag, unsigned long long wd) __attribute__((always_inline)) {
                constexpr int P = decltype(ptag)::value;
                if constexpr (P == 0) {
                    q = tt & (RING - 1);
                    wb = mycol + q * 64;
                }
#ifdef CPX_AB_SCALAR_BEHIND_COMPARE
                if constexpr (P == 1 && TYPE == CPX_VIT_SOFT) nan_or(nanmask, cur[R].x, cur[R].y);
#else
                if constexpr (P == 1 && TYPE == CPX_VIT_SOFT) nank = nan_lanes(cur[R].x, cur[R].y);   // (steps > tmax re-read step tmax)
                if constexpr (P == 3 && TYPE == CPX_VIT_SOFT) nanmask |= nank;  // (a dozen vector instructions behind the compare)
#endif
                if constexpr (P == 2) {
                    const bool live = FAST || tt <= T;
                    if constexpr (MIR) {
                        unsigned long long *w0 = live ? wb : mycol + (2 * RING) * 64;
                        unsigned long long *w1 = live ? wb + RING * 64 : mycol + (2 * RING + 1) * 64;
                        *w0 = wd;
                        *w1 = wd;
                    } else {
                        unsigned long long *w0 = live ? wb : mycol + RING * 64;
                        *w0 = wd;
                    }
                }
            };
            auto step = [&](const auto &hook) __attribute__((always_inline)) {
                if constexpr (PIN) cw_step<LGS, G0, G1, TYPE, R, true>(pm, r0, r1, word, bst, hook, nullptr, gidx, fill);
                else cw_step<LGS, G0, G1, TYPE, R, true>(pm, r0, r1, word, bst, hook, nullptr, gidx);
            };
            if constexpr (!PIN && TYPE == CPX_VIT_SOFT) nan_or(nanmask, cur[R].x, cur[R].y);   // (steps > tmax re-read step tmax)
            if constexpr (BURST && R == LGS - 1) {
                burst.pb = mycol + ((tt - 1) & (RING - 1)) * 64;              // the slot of step t + LGS - 2, written by the step before
                step(burst);                                                  // + the read batches of the group's walks
                burst.finish();                                               // one wait, then the hops of the walks of steps t - 1 .. t + LGS - 2
#pragma unroll
                for (int k = 0; k < LGS; k++) tile[k] = (unsigned char)burst.bit(k);   // entry k: the walk of step t - 1 + k
            } else if constexpr (BURST) {
                step(NoHook());                                               // no walk in this step
            } else {
            step(walk);                                                       // + the four read batches of the walk of step tt - 1
            walk.finish();                                                    // one wait, then all of its hops
            tile[R] = (unsigned char)walk.bit();                              // input bit of the branch into the state at step tt - 1 - H
            }
            if constexpr (!PIN) {                                             // the ring write, behind the walk
                const bool live = FAST || tt <= T;
                q = tt & (RING - 1);
                wb = mycol + q * 64;
                if constexpr (MIR) {
                    unsigned long long *w0 = live ? wb : mycol + (2 * RING) * 64;
                    unsigned long long *w1 = live ? wb + RING * 64 : mycol + (2 * RING + 1) * 64;
                    *w0 = word;
                    *w1 = word;
                } else {
                    unsigned long long *w0 = live ? wb : mycol + RING * 64;
                    *w0 = word;
                }
            }
            if constexpr (MIR) walk.pw = wb;                                  // next: the walk of this step
            else walk.q = q;
            if constexpr (!FAST) best_T = (tt == T) ? bst : best_T;
            walk.st = (unsigned)bst;
            if constexpr (BURST) burst.st[(R + 1) % LGS] = (unsigned)bst;     // start state of this step's walk (R = LGS - 1: the pending one)
        };
        if constexpr (LGS >= 1) one(std::integral_constant<int, 0>{});
        if constexpr (LGS >= 2) one(std::integral_constant<int, 1 % LGS>{});
        if constexpr (LGS >= 3) one(std::integral_constant<int, 2 % LGS>{});
        if constexpr (LGS >= 4) one(std::integral_constant<int, 3 % LGS>{});
        if constexpr (LGS >= 5) one(std::integral_constant<int, 4 % LGS>{});
        if constexpr (LGS >= 6) one(std::integral_constant<int, 5 % LGS>{});
#pragma unroll
        for (int u = 0; u < LGS; u++) cur[u] = nxt[u];
    };

    for (int tc0 = 1; tc0 <= T; tc0 += CHUNK) {
        const int left = (T - tc0) / LGS + 1;                                      // groups that start at a step <= T
        const int ngroups = left < FR_GROUPS ? left : FR_GROUPS;
        // the chunk's fast groups are its first nfast ones (the condition only gets harder as t grows): wave-uniform, scalar unit
        const int room = tmax - tc0 - (2 * LGS - 1);                               // >= 0: the chunk's first group is fast
        const int nfast = room < 0 ? 0 : (room / LGS + 1 < ngroups ? room / LGS + 1 : ngroups);
        int t = tc0;
        unsigned char *tile = myrow;                                               // advanced by LGS entries per group: the step's offset R is an immediate
        for (int g = 0; g < nfast; g++, t += LGS, tile += LGS) group(std::true_type{}, t, tile);
        for (int g = nfast; g < ngroups; g++, t += LGS, tile += LGS) group(std::false_type{}, t, tile);
        int n = ngroups * LGS;
        if (tc0 + CHUNK > T) {                                                     // last chunk: finish the pending walk (of its last step)
            unsigned st = walk.st;
            for (int h = 0; h < H; h++) st = tb_hop<LGS>(walk.word(h), st);
            myrow[n] = (unsigned char)((st >> (LGS - 1)) & 1u);
            n++;
        }
        flush(tc0, n);
    }
    if constexpr (TYPE == CPX_VIT_SOFT)
    {   // one flag per ITEM of the state-per-lane redo kernel (viterbi.hip): 64 / S consecutive codewords (one codeword for S = 64)
            constexpr int CPI = 64 / S;
            const int64_t item = grp * (64 / CPI) + lane;
            if (lane < 64 / CPI && item * CPI < p.B)
                p.nanflags[item] = (uint8_t)(((nanmask >> (lane * CPI)) & (CPI == 64 ? ~0ull : ((1ull << CPI) - 1ull))) != 0);
        }
    // the last H output steps: one walk from best[T]; the state before hop h is the state of step T - h
    if (valid) {
        const int qT = T & (RING - 1);
        unsigned st = (unsigned)best_T;
        for (int h = 0; h < H; h++) {
            const int so = T - h;
            if (so < 1) break;
            if (so - 1 < p.L) p.bits[cw * p.L + so - 1] = (uint8_t)((st >> (LGS - 1)) & 1u);
            st = tb_hop<LGS>(mycol[((qT - h) & (RING - 1)) * 64], st);
        }
    }
}

// Sliding traceback: bit of output step s = input bit of the state at step s on the path traced back from
// best[min(s + tb - 2, T)] (the rule of viterbi.hip).  One workgroup per group of 64 codewords; per pass of 64 output
// steps the rows of steps base .. base + 63 + tb - 2 are staged in LDS; wave w traces codewords w, w+8, ... two at a
// time (two independent dependent-load chains), lane i = output step base + i.
constexpr int TB_THREADS = 512, TB_WAVES = TB_THREADS / 64, TB_STRIDE = 65;

template <int LGS>
__global__ __launch_bounds__(TB_THREADS) void viterbi_cw_tb_kernel(CwParams p) {
    (void)LGS;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int H = p.tb - 2, rows = 64 + H;
    unsigned long long *win = reinterpret_cast<unsigned long long *>(smem);        // [rows][65]
    unsigned char *bwin = reinterpret_cast<unsigned char *>(win + (size_t)rows * TB_STRIDE);   // [rows][64]
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t grp = blockIdx.x;
    const unsigned long long *dec = p.dec + grp * p.Tp * 64;
    const unsigned char *best = p.best + grp * p.Tp * 64;
    for (int64_t base = 1; base <= p.T; base += 64) {
        int64_t need = base + 63 + H;
        if (need > p.T) need = p.T;
        __syncthreads();                                                          // readers of the previous window are done
        for (int64_t tt = base + w; tt <= need; tt += TB_WAVES) {                 // row of step tt -> window row tt - base
            win[(tt - base) * TB_STRIDE + lane] = dec[(tt - 1) * 64 + lane];
            bwin[(tt - base) * 64 + lane] = best[(tt - 1) * 64 + lane];
        }
        __syncthreads();
        const int64_t so = base + lane;                                           // output step of this lane
        const bool full = base + 63 + H <= p.T;                                   // every lane of the pass walks all H hops
        int64_t t0 = so + H;
        if (t0 > p.T) t0 = p.T;
        for (int c0 = w; c0 < 64; c0 += 2 * TB_WAVES) {
            const int c1 = c0 + TB_WAVES;
            unsigned st0 = 0, st1 = 0;
            if (so <= p.T) {
                st0 = bwin[(t0 - base) * 64 + c0];
                st1 = bwin[(t0 - base) * 64 + c1];
            }
            // hop h uses the decision word of step so + H - h (clipped lanes wait until that step is <= T)
            int idx = (lane + H) * TB_STRIDE;                                     // window row of step so + H
            if (full) {
                // the addresses do not depend on the states: unrolled, the reads of four hops are in flight together
#pragma unroll 4
                for (int h = 0; h < H; h++) {
                    st0 = tb_hop<LGS>(win[idx + c0], st0);
                    st1 = tb_hop<LGS>(win[idx + c1], st1);
                    idx -= TB_STRIDE;
                }
            } else {
                for (int h = 0; h < H; h++) {
                    const bool go = so + H - h <= p.T;                            // rows past `need` hold stale words: skipped
                    const unsigned n0 = tb_hop<LGS>(win[idx + c0], st0), n1 = tb_hop<LGS>(win[idx + c1], st1);
                    st0 = go ? n0 : st0;
                    st1 = go ? n1 : st1;
                    idx -= TB_STRIDE;
                }
            }
            const int64_t pos = so - 1;
            if (so <= p.T && pos < p.L) {
                const int64_t cwa = grp * 64 + c0, cwb = grp * 64 + c1;
                if (cwa < p.B) p.bits[cwa * p.L + pos] = (uint8_t)((st0 >> (LGS - 1)) & 1u);   // input bit of the branch into st
                if (cwb < p.B) p.bits[cwb * p.L + pos] = (uint8_t)((st1 >> (LGS - 1)) & 1u);
            }
        }
    }
}

// ---- host side: one launcher for every flavour of the fused kernel ---------------------------------------------------------------
// A flavour = ring slots, mirrored or stored once, and the hop count the walk is compiled for (tb_depth - 2 of the deepest window it
// serves; shallower windows run the same flavour with a run-time hop count, RT).
template <int RING_, bool MIR_, int HOPS_>
struct Flavour {
    static constexpr int RING = RING_, HOPS = HOPS_;
    static constexpr bool MIR = MIR_;
};
// the reference's default traceback depth, tb_depth = 5 * total_memory (convcode.py:701) ...
template <int LGS> constexpr int fused_tb() { return 5 * LGS; }
// ... and the deepest window of the deep ring (run-time hop count, float64 metrics only)
template <int LGS> constexpr int fused_tb_deep() { return 8 * LGS; }
// 64 states up to the default depth: 157 KB of LDS per workgroup
template <int LGS> using Mirrored32 = Flavour<FR_RING, true, fused_tb<LGS>() - 2>;
// 64 states, tb_depth 31 .. 48 (see FR_RING_DEEP)
template <int LGS> using Deep64 = Flavour<FR_RING_DEEP, false, fused_tb_deep<LGS>() - 2>;
// 64 states on the 32-slot ring stored ONCE ('soft', default depth, float64): 93 KB of LDS per workgroup instead of 157, one more
// instruction per traceback hop.  Used for the round(s) of a batch that ALSO has a remainder on the state-per-lane kernels
// (viterbi_dispatch, round 6): with the mirrored ring a round's workgroup holds the CU's whole LDS and the remainder's workgroups are
// not placed until it retires (profiles/r06_viterbi_remainder_overlap_ab.txt); with this one they run beside it.
template <int LGS> using Lean32 = Flavour<FR_RING, false, fused_tb<LGS>() - 2>;
// Small trellises (4 .. 32 states) and every table-driven code, up to the default depth: a 16- or 32-slot unmirrored ring cut to the
// depth -- 14.6 / 22.8 KB of LDS per wave instead of 39, so that two workgroups fit a CU (the one-wave-per-SIMD structure of the
// 64-state kernel leaves a 4-state step, ~60 instructions, waiting for its own latencies: 0.77 ms on BASELINE config 1 where the
// state-per-lane kernel takes 0.56; with the small ring 0.42 ms).
template <int LGS> using Small = Flavour<(fused_tb<LGS>() - 1 <= 16 ? 16 : 32), false, fused_tb<LGS>() - 2>;

// Launches ONE instantiation; false (nothing launched) on a device that cannot give it its LDS: the caller tries the next form.
template <class FL, int LGS, unsigned G0, unsigned G1, int TYPE, bool RT, class F>
bool launch_fused_kernel(const CwParams &p, hipStream_t st) {
    auto *fn = viterbi_cw_fused_kernel<LGS, G0, G1, TYPE, FL::HOPS, RT, F, FL::RING, FL::MIR>;
    constexpr size_t lds = ACS_WAVES * fused_wave_lds<FL::RING, FL::MIR, G0 == 0 && G1 == 0>();
    if (lds > 64 * 1024) {                                       // > 64 KiB of dynamic LDS is opt-in, once per kernel and device
        static bool raised[64] = {};
        static std::mutex raised_mu;                             // host threads may launch concurrently (ctypes drops the GIL)
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return false;
        std::lock_guard<std::mutex> lk(raised_mu);
        if (!raised[dev]) {
            if (hipFuncSetAttribute((const void *)fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) {
                (void)hipGetLastError();                         // a device with less LDS
                return false;
            }
            raised[dev] = true;
        }
    }
    const unsigned groups = (unsigned)((p.B + 63) / 64), blocks = (groups + ACS_WAVES - 1) / ACS_WAVES;
    hipLaunchKernelGGL(fn, dim3(blocks), dim3(64 * ACS_WAVES), lds, st, p);
    return true;
}

// decoding type -> template argument; RT: the walk takes its hop count from p.tb
template <class FL, int LGS, unsigned G0, unsigned G1, class F, bool RT>
bool launch_fused_rt(const CwParams &p, hipStream_t st) {
    if (p.type == CPX_VIT_HARD) return launch_fused_kernel<FL, LGS, G0, G1, CPX_VIT_HARD, RT, F>(p, st);
    if (p.type == CPX_VIT_SOFT) return launch_fused_kernel<FL, LGS, G0, G1, CPX_VIT_SOFT, RT, F>(p, st);
    return launch_fused_kernel<FL, LGS, G0, G1, CPX_VIT_UNQUANTIZED, RT, F>(p, st);
}
// the default depth runs the compile-time walk; smaller depths the same kernel with a run-time hop count (round 4)
template <class FL, int LGS, unsigned G0, unsigned G1, class F = double>
bool launch_fused(const CwParams &p, hipStream_t st) {
    return p.tb != FL::HOPS + 2 ? launch_fused_rt<FL, LGS, G0, G1, F, true>(p, st) : launch_fused_rt<FL, LGS, G0, G1, F, false>(p, st);
}

// the two-kernel form: decision words through HBM (p.dec, p.best)
template <int LGS, unsigned G0, unsigned G1>
void launch_two_kernels(const CwParams &p, size_t tb_lds, hipStream_t st) {
    const unsigned groups = (unsigned)((p.B + 63) / 64), ablocks = (groups + ACS_WAVES - 1) / ACS_WAVES;
    const dim3 ab(64 * ACS_WAVES);
    if (p.type == CPX_VIT_HARD) hipLaunchKernelGGL((viterbi_cw_acs_kernel<LGS, G0, G1, CPX_VIT_HARD>), dim3(ablocks), ab, 0, st, p);
    else if (p.type == CPX_VIT_SOFT) hipLaunchKernelGGL((viterbi_cw_acs_kernel<LGS, G0, G1, CPX_VIT_SOFT>), dim3(ablocks), ab, 0, st, p);
    else hipLaunchKernelGGL((viterbi_cw_acs_kernel<LGS, G0, G1, CPX_VIT_UNQUANTIZED>), dim3(ablocks), ab, 0, st, p);
    hipLaunchKernelGGL((viterbi_cw_tb_kernel<LGS>), dim3(groups), dim3(TB_THREADS), tb_lds, st, p);
}

}  // namespace

#ifdef CPX_VIT_SPEC_LG
// ---- a code object for ONE generator pair (round 6) ------------------------------------------------------------------------------
// Any rate-1/2 code of full constraint length runs the table-driven flavour above (branch metric selected by VGPR index mode: 1.78 ms
// on the config-2 geometry where a compiled-in pair takes 1.55).  Compiled with
//     hipcc --offload-arch=gfx950 --cuda-device-only -DCPX_VIT_SPEC_LG=6 -DCPX_VIT_SPEC_G0=<g0> -DCPX_VIT_SPEC_G1=<g1> -c viterbi_cw.hip
// this file yields a code object that holds nothing but the six fused kernels of THAT pair (three decoding types x {default depth,
// run-time hop count}), generators as template arguments like the built-in pairs; commpy_amd/jit.py builds and caches it,
// cpx_trellis_attach_viterbi_code loads it (hipModuleLoadData) and viterbi_codeword_path launches it in place of the table-driven
// kernel.  Generators in the template's convention ("MSB taps the input", see BUILTIN_PAIRS below).  64 states: the Mirrored32
// flavour; fewer: Small.
namespace {
constexpr int SPEC_LG = CPX_VIT_SPEC_LG;
constexpr int SPEC_RING = SPEC_LG == 6 ? FR_RING : (5 * SPEC_LG - 1 <= 16 ? 16 : 32);
constexpr bool SPEC_MIR = SPEC_LG == 6;
#define CPX_SPEC(TYPE, RT)                                                                                                  \
    template __global__ void viterbi_cw_fused_kernel<SPEC_LG, CPX_VIT_SPEC_G0, CPX_VIT_SPEC_G1, TYPE, 5 * SPEC_LG - 2, RT, double, \
                                                     SPEC_RING, SPEC_MIR>(CwParams);
CPX_SPEC(CPX_VIT_HARD, false) CPX_SPEC(CPX_VIT_HARD, true) CPX_SPEC(CPX_VIT_SOFT, false) CPX_SPEC(CPX_VIT_SOFT, true)
CPX_SPEC(CPX_VIT_UNQUANTIZED, false) CPX_SPEC(CPX_VIT_UNQUANTIZED, true)
#undef CPX_SPEC
}  // namespace
#else

namespace {

// The generator pairs with kernels of their own, in the template's convention: bit lg taps the input.  commpy's default
// polynomial_format='MSB' makes the LEAST significant bit of the octal number the D^0 tap (convcode.py:211-222), i.e. the bit-reversed
// number here: (133,171) -> (155,117).
struct Pair { int lg; unsigned g0, g1; };
constexpr Pair BUILTIN_PAIRS[] = {
    {6, 0155u, 0117u},     // K = 7 (133,171), commpy default format: 802.11 / BASELINE configs 2 and 5
    {6, 0117u, 0155u},     // K = 7 (171,133)
    {6, 0133u, 0171u},     // K = 7 (133,171) written with polynomial_format='LSB' (convcode.py:216-222)
    {6, 0171u, 0133u},     // K = 7 (171,133), 'LSB'
    // Wifi80211 as shipped: its generators are written in DECIMAL, (133, 171), and dec2bitarray wraps them to (5, 43)
    // (wifi80211.py:49, utilities.py:81-85) -- 0000101 / 0101011, bit-reversed 0120 / 0152.  The reference's
    // own link simulation (BASELINE config 5 with default arguments) decodes this 64-state code.
    {6, 0120u, 0152u},
    {2, 05u, 07u},         // K = 3 (5,7) -- BASELINE config 1
    {4, 031u, 027u},       // K = 5 (23,35)
};
constexpr int N_BUILTIN = sizeof(BUILTIN_PAIRS) / sizeof(BUILTIN_PAIRS[0]);

int builtin_index(const TrellisClass &c) {
    if (c.linear_half)
        for (int i = 0; i < N_BUILTIN; i++)
            if (BUILTIN_PAIRS[i].lg == c.lgS && BUILTIN_PAIRS[i].g0 == c.g0 && BUILTIN_PAIRS[i].g1 == c.g1) return i;
    return -1;
}

const char *type_name(int type) { return type == CPX_VIT_HARD ? "hard" : type == CPX_VIT_SOFT ? "soft" : "unquantized"; }

// what one call of viterbi_codeword_path works with
struct CwCall {
    CwParams p;
    Scratch *sc;
    hipStream_t st;
    size_t tb_lds;           // traceback window of the two-kernel form
    int64_t groups;
    bool lean_ring, two_kernels, f32;
};

CwResult done(CwFlavour f, const char *form) {
    if (hipGetLastError() == hipSuccess) return {true, CPX_OK, f};
    set_error("viterbi (%scodeword path): launch failed", form);
    return {true, CPX_EHIP, f};
}

// A built-in pair.  64 states: always handled here -- the fused kernel up to tb_depth 48, else (or on request) two kernels.
// Fewer states: the small ring up to the default depth; not handled otherwise.
template <int LG, unsigned GA, unsigned GB>
CwResult run_builtin(CwCall &c) {
    CwParams &p = c.p;
    const int tb = p.tb, type = p.type;
    if constexpr (LG == 6) {
        if (c.lean_ring && type == CPX_VIT_SOFT && tb == fused_tb<LG>() && !c.two_kernels && !c.f32 &&
            launch_fused_kernel<Lean32<LG>, LG, GA, GB, CPX_VIT_SOFT, false, double>(p, c.st)) {
            const CwResult r = done(CwFlavour::lean, "fused ");
            note_kernel("viterbi_cw_fused_kernel<%d,0%o,0%o,%s,%d,ring stored once>", LG, GA, GB, type_name(type), fused_tb<LG>() - 2);
            return r;
        }
        const bool deep = tb > fused_tb<LG>();
        if (tb >= 2 && tb <= fused_tb_deep<LG>() && !c.two_kernels &&
            (deep ? launch_fused_rt<Deep64<LG>, LG, GA, GB, double, true>(p, c.st)
                  : c.f32 ? launch_fused<Mirrored32<LG>, LG, GA, GB, float>(p, c.st) : launch_fused<Mirrored32<LG>, LG, GA, GB, double>(p, c.st))) {
            const CwResult r = done(deep ? CwFlavour::deep : CwFlavour::mirrored, "fused ");
            note_kernel("viterbi_cw_fused_kernel<%d,0%o,0%o,%s,%d%s%s>", LG, GA, GB, type_name(type),
                        (deep ? fused_tb_deep<LG>() : fused_tb<LG>()) - 2,
                        deep ? ",runtime hops,64-slot ring" : tb == fused_tb<LG>() ? "" : ",runtime hops", (c.f32 && !deep) ? ",f32" : "");
            return r;
        }
        p.Tp = (p.T + LG - 1) / LG * LG;
        if (int rc = c.sc->get(c.st, Slot::state, sizeof(unsigned long long) * (size_t)(c.groups * p.Tp * 64), &p.dec)) return {true, rc, CwFlavour::two_kernels};
        if (int rc = c.sc->get(c.st, Slot::state2, (size_t)(c.groups * p.Tp * 64), &p.best)) return {true, rc, CwFlavour::two_kernels};
        launch_two_kernels<LG, GA, GB>(p, c.tb_lds, c.st);
        const CwResult r = done(CwFlavour::two_kernels, "");
        note_kernel("viterbi_cw_acs_kernel<%d,0%o,0%o,%s> + viterbi_cw_tb_kernel<%d>", LG, GA, GB, type_name(type), LG);
        return r;
    } else {
        if (tb >= 2 && tb <= fused_tb<LG>() && !c.two_kernels && !c.f32 && launch_fused<Small<LG>, LG, GA, GB>(p, c.st)) {
            const CwResult r = done(CwFlavour::small, "small fused ");
            note_kernel("viterbi_cw_fused_kernel<%d,0%o,0%o,%s,%d,small ring%s>", LG, GA, GB, type_name(type), fused_tb<LG>() - 2,
                        tb == fused_tb<LG>() ? "" : ",runtime hops");
            return r;
        }
        return {};
    }
}
template <int I = 0>
CwResult run_builtin_at(int i, CwCall &c) {
    if constexpr (I < N_BUILTIN) {
        constexpr Pair P = BUILTIN_PAIRS[I];
        return i == I ? run_builtin<P.lg, P.g0, P.g1>(c) : run_builtin_at<I + 1>(i, c);
    } else {
        return {};
    }
}

// any other end-tap code (4 .. 64 states), up to its default depth: the table-driven kernel, G0 = G1 = 0 (cw_step reads p.goff)
template <int LG = 6>
CwResult run_table(int lg, CwCall &c) {
    if constexpr (LG >= 2) {
        if (lg != LG) return run_table<LG - 1>(lg, c);
        if (!launch_fused<Small<LG>, LG, 0u, 0u>(c.p, c.st)) return {};
        const CwResult r = done(CwFlavour::table, "table-driven ");
        note_kernel("viterbi_cw_fused_kernel<%d,table-driven,%s,%d%s>", LG, type_name(c.p.type), fused_tb<LG>() - 2,
                    c.p.tb == fused_tb<LG>() ? "" : ",runtime hops");
        return r;
    } else {
        return {};
    }
}

}  // namespace

namespace cpx {

CwResult viterbi_codeword_path(const cpx_trellis *t, const double *d_coded, int64_t B, int64_t len, int64_t L, int64_t T,
                               int tb, int type, uint8_t *d_bits, uint8_t *nanflags, Scratch &sc, hipStream_t st, bool any_batch_size,
                               bool lean_ring) {
    // path override (cpx_viterbi_set_path / CPX_VITERBI_PATH): "wave" = state-per-lane kernels; "cw" = this path whatever
    // the batch size; "cw!" = fail instead of falling back; "cw2", "cw2!" = the two-kernel form even where the fused
    // kernel applies
    const int pf = viterbi_path_flags();
    if (pf & 1) return {};
    const bool forced = (pf & 2) || any_batch_size, strict = pf & 4;
    auto reject = [&](const char *why) -> CwResult {
        if (!strict) return {};
        set_error("viterbi (codeword path): %s", why);
        return {true, CPX_ELIMIT, CwFlavour::none};
    };
    if (!forced && !viterbi_round_pays(B, viterbi_round())) return {};
    const TrellisClass &k = t->cls;
    if (t->I != 2 || t->k != 1 || t->n != 2 || T < 1) return reject("needs a rate-1/2, k = 1 trellis");
    if ((len & 1) || ((uintptr_t)d_coded & 15)) return reject("rows must be 16-byte aligned");
    CwCall c;
    c.sc = &sc;
    c.st = st;
    c.tb_lds = (size_t)(64 + tb - 2) * (TB_STRIDE * 8 + 64);
    if (c.tb_lds > 64 * 1024) return reject("traceback window exceeds 64 KiB of LDS");
    c.groups = (B + 63) / 64;
    if (c.groups >= (1ll << 31) || T >= (1ll << 31) - 64) return reject("batch too large / block too long");
    CwParams &p = c.p;
    p.coded = d_coded; p.bits = d_bits; p.B = B; p.len = len; p.L = L; p.T = T; p.Lk = L;   // k = 1
    p.type = type; p.tb = tb; p.nanflags = nanflags;
    if (type == CPX_VIT_SOFT && !nanflags) return reject("'soft' needs the NaN flag array");
    c.lean_ring = lean_ring;
    c.two_kernels = pf & 8;
    // float32 path metrics when the caller selected "fp32-fast" (cpx_set_precision) -- fused kernel of the built-in 64-state pairs only.
    // ('hard' metrics of 0/1 inputs are Hamming distances <= 2 T, exact in float32: there the fast mode returns identical bits.)
    c.f32 = precision_fast() && T < (1ll << 22);
    if (const CwResult r = run_builtin_at(builtin_index(k), c); r.handled) return r;
    // every other flavour: up to the default depth, fused, float64 (deeper windows, and the fp32-fast mode, go to the state-per-lane kernels)
    const bool plain = tb >= 2 && !c.two_kernels && !c.f32;
    // a code object compiled for this code's generators (cpx_trellis_attach_viterbi_code): the built-in pairs' kernel, from a module
    if (t->spec_mod && plain && tb <= 5 * t->spec_lg) {
        const bool rt = tb != 5 * t->spec_lg;
        hipFunction_t fn = t->spec_fn[type][rt ? 1 : 0];
        const unsigned groups32 = (unsigned)c.groups, blocks = (groups32 + ACS_WAVES - 1) / ACS_WAVES;
        void *args[] = {(void *)&p};
        if (hipModuleLaunchKernel(fn, blocks, 1, 1, 64 * ACS_WAVES, 1, 1, 0, st, args, nullptr) != hipSuccess) {
            (void)hipGetLastError();
            set_error("viterbi (per-pair code object): launch failed");
            return {true, CPX_EHIP, CwFlavour::code_object};
        }
        note_kernel("viterbi_cw_fused_kernel<%d,0%o,0%o,%s,%d%s> (code object of this pair)", t->spec_lg, t->spec_g0, t->spec_g1,
                    type_name(type), 5 * t->spec_lg - 2, rt ? ",runtime hops" : "");
        return {true, CPX_OK, CwFlavour::code_object};
    }
    if (k.end_tap && plain && tb <= 5 * k.lgS) {
        memcpy(p.goff, k.goff, sizeof(p.goff));
        if (const CwResult r = run_table(k.lgS, c); r.handled) return r;
    }
    return reject("no instantiation for this trellis");
}

}  // namespace cpx

extern "C" int cpx_viterbi_set_path(const char *mode) { return cpx::set_mode(cpx::Switch::viterbi_path, mode); }

// ---- per-pair code objects (round 6): query and attach -------------------------------------------------------------------------
extern "C" int cpx_trellis_viterbi_spec_query(const cpx_trellis *t, int *lg, unsigned *g0, unsigned *g1) {
    CPX_REQUIRE(t && lg && g0 && g1, CPX_EINVAL, "cpx_trellis_viterbi_spec_query: null pointer");
    *lg = 0; *g0 = 0; *g1 = 0;
    const cpx::TrellisClass &k = t->cls;
    // what the table-driven kernel serves today and a compiled pair would serve faster: full-constraint-length codes that are not built in
    if (!k.end_tap || !k.linear_half || builtin_index(k) >= 0 || t->spec_mod) return CPX_OK;
    *lg = k.lgS; *g0 = k.g0; *g1 = k.g1;
    return CPX_OK;
}

extern "C" int cpx_trellis_attach_viterbi_code(cpx_trellis *t, const void *image, size_t bytes) {
    CPX_REQUIRE(t && image && bytes >= 64, CPX_EINVAL, "cpx_trellis_attach_viterbi_code: null / empty image");
    if (int rcd = cpx::check_handle_device(t->device, "attach_viterbi_code")) return rcd;
    CPX_REQUIRE(!t->spec_mod, CPX_EINVAL, "cpx_trellis_attach_viterbi_code: the trellis already has a code object");
    CPX_REQUIRE(t->cls.linear_half, CPX_EINVAL,
                "cpx_trellis_attach_viterbi_code: not a rate-1/2 shift-register code of 4 .. 64 states");
    const int lg = t->cls.lgS;
    const unsigned g0 = t->cls.g0, g1 = t->cls.g1;
    hipModule_t mod = nullptr;
    if (hipModuleLoadData(&mod, image) != hipSuccess) {
        (void)hipGetLastError();
        cpx::set_error("cpx_trellis_attach_viterbi_code: hipModuleLoadData refused the image");
        return CPX_EHIP;
    }
    // the kernels are looked up BY THE GENERATORS OF THIS TRELLIS: an image compiled for another pair has no such symbols and is refused
    const int ring = lg == 6 ? FR_RING : (5 * lg - 1 <= 16 ? 16 : 32);
    hipFunction_t fn[3][2];
    for (int type = 0; type < 3; type++)
        for (int rt = 0; rt < 2; rt++) {
            char name[200];
            snprintf(name, sizeof(name), "_ZN12_GLOBAL__N_123viterbi_cw_fused_kernelILi%dELj%uELj%uELi%dELi%dELb%dEdLi%dELb%dEEEvNS_8CwParamsE",
                     lg, g0, g1, type, 5 * lg - 2, rt, ring, lg == 6 ? 1 : 0);
            if (hipModuleGetFunction(&fn[type][rt], mod, name) != hipSuccess) {
                (void)hipGetLastError();
                (void)hipModuleUnload(mod);
                cpx::set_error("cpx_trellis_attach_viterbi_code: the image has no kernel %s (compiled for other generators, or from other sources)", name);
                return CPX_EINVAL;
            }
        }
    memcpy(t->spec_fn, fn, sizeof(fn));
    t->spec_lg = lg; t->spec_g0 = g0; t->spec_g1 = g1;
    t->spec_mod = mod;                                            // last: the dispatcher tests this field (attach while another thread
    return CPX_OK;                                                //  decodes with the same handle is still the caller's to serialise)
}

extern "C" int cpx_trellis_has_viterbi_code(const cpx_trellis *t) { return (t && t->spec_mod) ? 1 : 0; }

extern "C" int cpx_trellis_detach_viterbi_code(cpx_trellis *t) {
    CPX_REQUIRE(t, CPX_EINVAL, "cpx_trellis_detach_viterbi_code: null trellis");
    if (t->spec_mod) {
        (void)hipDeviceSynchronize();                             // nothing may still run from the module
        (void)hipModuleUnload(t->spec_mod);
        t->spec_mod = nullptr;
        t->spec_lg = 0;
    }
    return CPX_OK;
}
#endif  // CPX_VIT_SPEC_LG
