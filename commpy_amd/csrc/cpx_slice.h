// What the equalisers share on the device (equalize.hip, adaptive.hip): the test for a NaN or an infinity, the scan of a row's samples
// (by a wave or by part of one) and the slicer.
#pragma once
#include "cpx_internal.h"

namespace cpx {

__device__ __forceinline__ bool not_finite(double v) { return !(__builtin_fabs(v) < __builtin_huge_val()); }

// samples first, first + stride, .. of a row: the wave's ballot of the lanes that met a NaN or an infinity (a row may be shared out
// over part of a wave: the caller keeps the bits of the lanes that scanned it)
__device__ __forceinline__ unsigned long long scan_lanes(const double *y, int64_t doubles, int first, int stride) {
    bool bad = false;
    for (int64_t i = first; i < doubles; i += stride) bad |= not_finite(y[i]);
    return __ballot(bad);
}

// one row's samples over the whole wave: true on every lane if any is a NaN or an infinity
__device__ __forceinline__ bool scan_row(const double *y, int64_t doubles, int lane) { return scan_lanes(y, doubles, lane, 64) != 0ull; }

// the slicer: first minimum over the points in ascending order and, with LGM > 0, the two minima of every label bit
template <int LGM>
__device__ __forceinline__ int slice(double xr, double xi, const double *cr, const double *ci, int M, double *m0, double *m1) {
    constexpr int NB = LGM > 0 ? LGM : 1;
#pragma unroll
    for (int i = 0; i < NB; i++) {
        m0[i] = __builtin_huge_val();
        m1[i] = __builtin_huge_val();
    }
    double best = 0.0;
    int sel = 0;
#pragma unroll 4
    for (int p = 0; p < M; p++) {
        const double er = xr - cr[p], ei = xi - ci[p];
        const double dd = er * er + ei * ei;
        if (p == 0 || dd < best) {
            best = dd;
            sel = p;
        }
        if constexpr (LGM > 0) {
#pragma unroll
            for (int i = 0; i < LGM; i++) {
                const bool one = (p >> (LGM - 1 - i)) & 1;
                m1[i] = (one && dd < m1[i]) ? dd : m1[i];
                m0[i] = (!one && dd < m0[i]) ? dd : m0[i];
            }
        }
    }
    return sel;
}

}  // namespace cpx
