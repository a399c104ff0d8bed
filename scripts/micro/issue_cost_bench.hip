// Micro-benchmark: issue cost per instruction of ONE wave per SIMD on gfx950, for the opcodes of the fused Viterbi kernel's
// first-argmin block (csrc/viterbi_cw.hip, cw_step): the float64 minimum tree and first-equal scan against a 32-bit tree
// (v_min3_u32) and hit words (v_cmp_eq_u32 + v_addc_co_u32).  Independent streams, and the real compare -> consumer pairs.
// The kernel runs exactly one wave per SIMD, so what an instruction costs is what it holds the issue port for, plus
// whatever the next instruction waits for; sibling of chain_bench.hip (which measured the dependent float64 chain).
//
//     hipcc --offload-arch=gfx950 -O3 scripts/micro/issue_cost_bench.hip -o issue_cost_bench && ./issue_cost_bench
#include <hip/hip_runtime.h>
#include <cstdio>
#define CHECK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("HIP error %s line %d\n", hipGetErrorString(e), __LINE__); return 1; } } while (0)
#define REP8(x) x x x x x x x x
// every body is 16 instructions; da .. dd: doubles, ua .. ud: 32-bit words, k0 .. k3: SGPR pairs
#define KERNEL(NAME, BODY)                                                                                      \
    __global__ __launch_bounds__(256) void NAME(double *out, int iters) {                                      \
        double da = threadIdx.x * 1e-3 + 0.5, db = da + 0.1, dc = da + 0.2, dd = da + 0.3, dm = 0.25;              \
        unsigned ua = threadIdx.x, ub = ua + 1, uc = ua + 2, ud = ua + 3, um = 7;                                 \
        unsigned long long k0, k1, k2, k3;                                                                       \
        for (int i = 0; i < iters; i++) { REP8(BODY) }                                                           \
        out[blockIdx.x * blockDim.x + threadIdx.x] = da + db + dc + dd + (double)(ua + ub + uc + ud);           \
    }
#define X4(s) s "\n" s "\n" s "\n" s "\n"
#define DOPS : "+v"(da), "+v"(db), "+v"(dc), "+v"(dd), "+v"(ua), "+v"(ub), "+v"(uc), "+v"(ud), "=&s"(k0), "=&s"(k1), "=&s"(k2), "=&s"(k3) \
             : "v"(dm), "v"(um) : "vcc", "scc"
// operands: %0-%3 doubles, %4-%7 words, %8-%11 SGPR pairs, %12 a double, %13 a word
KERNEL(k_add_f64,    asm volatile(X4("v_add_f64 %0, %0, %12\n v_add_f64 %1, %1, %12\n v_add_f64 %2, %2, %12\n v_add_f64 %3, %3, %12") DOPS);)
KERNEL(k_min_f64,    asm volatile(X4("v_min_f64 %0, %0, %12\n v_min_f64 %1, %1, %12\n v_min_f64 %2, %2, %12\n v_min_f64 %3, %3, %12") DOPS);)
KERNEL(k_cmp_eq_f64, asm volatile(X4("v_cmp_eq_f64 %8, %0, %12\n v_cmp_eq_f64 %9, %1, %12\n v_cmp_eq_f64 %10, %2, %12\n v_cmp_eq_f64 %11, %3, %12") DOPS);)
KERNEL(k_min3_u32,   asm volatile(X4("v_min3_u32 %4, %4, %13, %5\n v_min3_u32 %5, %5, %13, %6\n v_min3_u32 %6, %6, %13, %7\n v_min3_u32 %7, %7, %13, %4") DOPS);)
KERNEL(k_cmp_eq_u32, asm volatile(X4("v_cmp_eq_u32 vcc, %4, %13\n v_cmp_eq_u32 vcc, %5, %13\n v_cmp_eq_u32 vcc, %6, %13\n v_cmp_eq_u32 vcc, %7, %13") DOPS);)
KERNEL(k_cmp_eq_u32_sgpr, asm volatile(X4("v_cmp_eq_u32 %8, %4, %13\n v_cmp_eq_u32 %9, %5, %13\n v_cmp_eq_u32 %10, %6, %13\n v_cmp_eq_u32 %11, %7, %13") DOPS);)
KERNEL(k_cndmask,    asm volatile("s_mov_b64 %8, 5\n s_mov_b64 %9, 6\n s_mov_b64 %10, 7\n s_mov_b64 %11, 9\n"
                                  "v_cndmask_b32 %4, %4, 3, %8\n v_cndmask_b32 %5, %5, 3, %9\n v_cndmask_b32 %6, %6, 3, %10\n v_cndmask_b32 %7, %7, 3, %11\n"
                                  "v_cndmask_b32 %4, %4, 3, %8\n v_cndmask_b32 %5, %5, 3, %9\n v_cndmask_b32 %6, %6, 3, %10\n v_cndmask_b32 %7, %7, 3, %11\n"
                                  "v_cndmask_b32 %4, %4, 3, %8\n v_cndmask_b32 %5, %5, 3, %9\n v_cndmask_b32 %6, %6, 3, %10\n v_cndmask_b32 %7, %7, 3, %11" DOPS);)
KERNEL(k_addc,       asm volatile(X4("v_addc_co_u32 %4, vcc, %4, %4, vcc\n v_addc_co_u32 %5, vcc, %5, %5, vcc\n v_addc_co_u32 %6, vcc, %6, %6, vcc\n v_addc_co_u32 %7, vcc, %7, %7, vcc") DOPS);)
// the pairs as the kernel issues them
// today's scan: four float64 compares into four SGPR pairs, then the four selects (one chain)
KERNEL(k_pair_scan_f64_q, asm volatile(X4("v_cmp_eq_f64 %8, %0, %12\n v_cmp_eq_f64 %9, %1, %12\n v_cmp_eq_f64 %10, %2, %12\n v_cmp_eq_f64 %11, %3, %12\n"
                                          "v_cndmask_b32 %4, %4, 3, %8\n v_cndmask_b32 %4, %4, 4, %9\n v_cndmask_b32 %4, %4, 5, %10\n v_cndmask_b32 %4, %4, 6, %11") DOPS);)
// hit words through vcc, back to back, two words alternating (acs_min's compare -> v_addc distance)
KERNEL(k_pair_hit_vcc, asm volatile(X4("v_cmp_eq_u32 vcc, %13, %6\n v_addc_co_u32 %4, vcc, %4, %4, vcc\n v_cmp_eq_u32 vcc, %13, %7\n v_addc_co_u32 %5, vcc, %5, %5, vcc") DOPS);)
// hit words through four SGPR pairs: four compares, then four v_addc (VOP3), two words alternating -- the scan's distance
KERNEL(k_pair_hit_sgpr, asm volatile(X4("v_cmp_eq_u32 %8, %13, %6\n v_cmp_eq_u32 %9, %13, %7\n v_cmp_eq_u32 %10, %13, %6\n v_cmp_eq_u32 %11, %13, %7\n"
                                        "v_addc_co_u32 %4, %8, %4, %4, %8\n v_addc_co_u32 %5, %9, %5, %5, %9\n v_addc_co_u32 %4, %10, %4, %4, %10\n v_addc_co_u32 %5, %11, %5, %5, %11") DOPS);)
// one add-compare-select as the kernel has it (the 32-bit block's neighbour in the step): 2 v_add_f64, v_cmp_lt_f64, v_addc, v_min_f64
KERNEL(k_acs, asm volatile(X4("v_cmp_lt_f64 vcc, %1, %0\n v_addc_co_u32 %4, vcc, %4, %4, vcc\n v_min_f64 %2, %0, %1\n v_add_f64 %3, %3, %12") DOPS);)
// (the groups write SCC: DOPS names it as clobbered, or the compiler keeps its own loop compare in SCC across the statement)
// what a wave-uniform skip INSIDE an asm statement would cost: a group of s_cmp + forward s_cbranch over one instruction + two VALU
// instructions, with the branch taken (the flag is 0: the instruction is skipped) and not taken (the flag is 1: it runs)
#define SKIP_GROUP "s_cmp_eq_u64 %8, 0\n s_cbranch_scc1 1f\n v_min_f64 %0, %0, %12\n1:\n v_min3_u32 %4, %4, %13, %5\n v_min3_u32 %5, %5, %13, %4\n"
KERNEL(k_skip_taken,    asm volatile("s_mov_b64 %8, 0\n" SKIP_GROUP SKIP_GROUP SKIP_GROUP SKIP_GROUP DOPS);)
KERNEL(k_skip_untaken,  asm volatile("s_mov_b64 %8, 1\n" SKIP_GROUP SKIP_GROUP SKIP_GROUP SKIP_GROUP DOPS);)

int main() {
    double *d_out;
    CHECK(hipMalloc(&d_out, sizeof(double) * 256 * 256));
    const int iters = 20000;
    struct { const char *name; void (*k)(double *, int); double per_iter; } ks[] = {
        {"v_add_f64, 4 independent chains", k_add_f64, 128}, {"v_min_f64, 4 independent chains", k_min_f64, 128},
        {"v_cmp_eq_f64 -> 4 SGPR pairs", k_cmp_eq_f64, 128}, {"v_min3_u32, 4 chains", k_min3_u32, 128},
        {"v_cmp_eq_u32 -> vcc", k_cmp_eq_u32, 128}, {"v_cmp_eq_u32 -> 4 SGPR pairs (VOP3)", k_cmp_eq_u32_sgpr, 128},
        {"v_cndmask_b32 (SGPR-pair mask), 4 chains", k_cndmask, 128}, {"v_addc_co_u32 through vcc, 4 words", k_addc, 128},
        {"pair: 4 v_cmp_eq_f64 + 4 v_cndmask_b32 (the scan)", k_pair_scan_f64_q, 256},
        {"pair: v_cmp_eq_u32 vcc + v_addc, back to back, 2 words", k_pair_hit_vcc, 128},
        {"pair: 4 v_cmp_eq_u32 (SGPR) + 4 v_addc (VOP3), 2 words", k_pair_hit_sgpr, 256},
        {"mix: v_cmp_lt_f64 + v_addc + v_min_f64 + v_add_f64", k_acs, 128},
        // per GROUP (32 groups per iteration), not per instruction: minus the two v_min3_u32 (4.1 ns) it is the cost of the skip itself
        {"GROUP: s_cmp + s_cbranch TAKEN over 1 + 2 v_min3_u32", k_skip_taken, 32},
        {"GROUP: s_cmp + s_cbranch not taken + v_min_f64 + 2 v_min3", k_skip_untaken, 32},
    };
    for (auto &e : ks) {
        float best = 1e30f;
        for (int rep = 0; rep < 3; rep++) {
            hipEvent_t a, b;
            CHECK(hipEventCreate(&a)); CHECK(hipEventCreate(&b));
            hipLaunchKernelGGL(e.k, dim3(256), dim3(256), 0, 0, d_out, 10);      // one workgroup of four waves per CU: one wave per SIMD
            CHECK(hipEventRecord(a));
            hipLaunchKernelGGL(e.k, dim3(256), dim3(256), 0, 0, d_out, iters);
            CHECK(hipEventRecord(b));
            CHECK(hipEventSynchronize(b));
            float ms; CHECK(hipEventElapsedTime(&ms, a, b));
            best = ms < best ? ms : best;
        }
        printf("%-58s %8.3f ms -> %.3f ns per %s\n", e.name, best, best * 1e6 / (iters * e.per_iter), e.per_iter == 32 ? "group" : "instruction");
        fflush(stdout);
    }
    return 0;
}
