// The sample rotation shared by freq_offset_kernel (fir.hip) and sync_align_kernel (sync.hip), which must agree bit for bit.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace cpx {

// v (cos t + i sin t) with t = step k rounded once to float64: sincos() of the float64 product (full-range argument reduction),
// then four products and two sums, unfused (the library is compiled with -ffp-contract=off).
__device__ __forceinline__ double2 freq_rotate(double2 v, double step, int64_t k) {
    const double theta = step * (double)k;
    double sn, cs;
    sincos(theta, &sn, &cs);
    return make_double2(v.x * cs - v.y * sn, v.x * sn + v.y * cs);
}

}  // namespace cpx
