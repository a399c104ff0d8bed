// What the waveform stages share: the chain step that fir.hip, ofdm_chan.hip and fading.hip must agree on bit for bit, and the grid cap
// of their launchers (ofdm.hip and sync.hip as well).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace cpx {

// one complex tap of the chain: re += hr xr, re -= hi xi, im += hr xi, im += hi xr, four fused multiply-adds in this order
__device__ __forceinline__ void mac(double2 &acc, double2 h, double2 x) {
    acc.x = fma(h.x, x.x, acc.x);
    acc.x = fma(-h.y, x.y, acc.x);
    acc.y = fma(h.x, x.y, acc.y);
    acc.y = fma(h.y, x.x, acc.y);
}

// workgroups of a grid-stride launch over `items` tiles: at least 1, at most `cap`
inline unsigned grid_of(int64_t items, int64_t cap = 65535) {
    return (unsigned)(items < 1 ? 1 : items > cap ? cap : items);
}

}  // namespace cpx
