// Bit-equality of the fused Viterbi kernel's lean branch-metric arithmetic (csrc/cpx_math.h: exp_pm500, div_unscaled,
// fast_log<false, false, true>) with the forms it replaces (the device library's exp, the IEEE division sequence), on gfx950:
//   hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -I commpy_amd/csrc -I include scripts/micro/bm_exact_check.hip -o scripts/micro/bm_exact_check
//   scripts/micro/bm_exact_check
// Prints the number of differing bit patterns per function; exit status 1 if any differs.  Arguments: r over [-500, 500] (uniform,
// dense around 0, around the multiples of ln 2 / 2 and of ln 2, at the clip), and for the logarithm every exponent 0 .. 1023 with random
// mantissas plus the mantissas next to 1 and to sqrt(1/2) / sqrt(2), where the argument reduction changes branch and f = m - 1 is 0
// or a few ulp.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <cstdint>
#include "cpx_math.h"

__device__ __forceinline__ uint64_t rng(uint64_t &s) { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return s; }
__device__ __forceinline__ double unit(uint64_t &s) { return (double)(rng(s) >> 11) * 0x1p-53; }
__device__ __forceinline__ bool same(double a, double b) { return __double_as_longlong(a) == __double_as_longlong(b); }

__global__ void check(int n, unsigned long long *bad) {
    uint64_t s = 0x9E3779B97F4A7C15ull * (blockIdx.x * blockDim.x + threadIdx.x + 1);
    unsigned long long be = 0, bl = 0, bm = 0, bq = 0;
    for (int i = 0; i < n; i++) {
        double r;
        const int kind = i & 7;
        const long long k = (long long)(rng(s) % 2887) - 1443;                 // |k ln 2 / 2| <= 500.1
        const long long ulps = (long long)(rng(s) % 9) - 4;
        if (kind == 0) r = (unit(s) * 2 - 1) * 500.0;
        else if (kind == 1) r = (unit(s) * 2 - 1) * 45.0;
        else if (kind == 2) r = (double)k * 0.34657359027997264;               // ln 2 / 2: the exp's rounding boundaries (odd k) ...
        else if (kind == 3) r = (double)k * 0.34657359027997264 * (1.0 + (unit(s) - 0.5) * 0x1p-40);
        else if (kind == 4) r = log(ldexp(1.4142135623730951, (int)(rng(s) % 700)) * (1.0 + (unit(s) - 0.5) * 0x1p-44) - 1.0);   // log's sqrt(2) boundary
        else if (kind == 5) r = (unit(s) * 2 - 1) * ldexp(1.0, -(int)(rng(s) % 1074));
        else if (kind == 6) r = (rng(s) & 1 ? 1.0 : -1.0) * (30.0 + unit(s) * 10.0);   // exp(r) + 1 stops changing
        else r = (rng(s) & 1 ? 1.0 : -1.0) * (500.0 - unit(s) * 0x1p-30);
        r = __longlong_as_double(__double_as_longlong(r) + ((kind == 2 || kind == 7) ? ulps : 0));
        r = fmin(fmax(r, -500.0), 500.0);
        const double e0 = exp(r), e1 = cpx::exp_pm500(r);
        be += !same(e0, e1);
        const double l0 = cpx::fast_log<false>(e0 + 1.0), l1 = cpx::fast_log<false, false, true>(e1 + 1.0);
        bm += !same(l0, l1) || !same(l0 - r, l1 - r);
        // the logarithm alone, any finite argument >= 1
        const int ex = (int)(rng(s) % 1024);
        uint64_t man = rng(s) & 0x000fffffffffffffull;
        if ((i & 3) == 1) man = (rng(s) % 17);                                                 // 1 + a few ulp: f = 0 ... 16 ulp
        if ((i & 3) == 2) man = 0x000fffffffffffffull - (rng(s) % 17);                         // 2 - a few ulp: f = -(a few ulp)
        if ((i & 3) == 3) man = 0x6a09e667f3bcdull + (rng(s) % 33) - 16;                       // sqrt(2): the reduction's branch
        const double x = __longlong_as_double((long long)(((uint64_t)(1023 + ex) << 52) | man));
        bl += !same(cpx::fast_log<false>(x), cpx::fast_log<false, false, true>(x));
        // the quotient alone, on the reduction's operand ranges
        const double f = (i & 1) ? (unit(s) * 0.7072 - 0.2929) : ldexp(unit(s) * 2 - 1, -(int)(rng(s) % 53));
        bq += !same(f / (2.0 + f), cpx::div_unscaled(f, 2.0 + f));
    }
    atomicAdd(&bad[0], be); atomicAdd(&bad[1], bm); atomicAdd(&bad[2], bl); atomicAdd(&bad[3], bq);
}

int main() {
    unsigned long long *d_b, b[4];
    if (hipMalloc(&d_b, 32) != hipSuccess || hipMemset(d_b, 0, 32) != hipSuccess) { printf("no device\n"); return 2; }
    const int n = 4000, blocks = 1024, threads = 256;
    check<<<blocks, threads>>>(n, d_b);
    if (hipMemcpy(b, d_b, 32, hipMemcpyDeviceToHost) != hipSuccess) { printf("kernel failed: %s\n", hipGetErrorString(hipGetLastError())); return 2; }
    const double tot = (double)n * blocks * threads;
    printf("arguments per function: %.0f\n", tot);
    printf("exp_pm500(r) != exp(r), |r| <= 500                         : %llu\n", b[0]);
    printf("branch metrics m0 = log(exp(r) + 1), m1 = m0 - r differ     : %llu\n", b[1]);
    printf("fast_log<false,false,true>(x) != fast_log<false>(x), x >= 1 : %llu\n", b[2]);
    printf("div_unscaled(f, 2 + f) != f / (2 + f)                       : %llu\n", b[3]);
    return (b[0] | b[1] | b[2] | b[3]) ? 1 : 0;
}
