// What the algebraic codecs (bch.hip, rs.hip) share on the host: the exp / log tables of GF(2^m) as a handle builds them.
#pragma once
#include "cpx_internal.h"

#include <vector>

namespace cpx {

// tab = [2][2^m] uint16: exp[e] = alpha^e (e = 0 .. N, N = 2^m - 1, alpha = x), then log[v] (log[0] = 0).  CPX_EINVAL with "<who>: ..."
// unless x generates the multiplicative group under prim_poly (whose degree the caller has checked).
inline int gf_tables(const char *who, int m, uint32_t prim_poly, std::vector<uint16_t> &tab) {
    const int N = (1 << m) - 1;
    tab.assign((size_t)2 << m, 0);
    uint16_t *ex = tab.data(), *lg = ex + ((size_t)1 << m);
    unsigned v = 1;
    for (int e = 0; e < N; ++e) {
        CPX_REQUIRE(e == 0 || v != 1u, CPX_EINVAL, "%s: prim_poly = %u is not primitive (x has order %d, not %d)", who, prim_poly, e, N);
        ex[e] = (uint16_t)v;
        lg[v] = (uint16_t)e;
        v <<= 1;
        if (v >> m) v ^= prim_poly;
    }
    CPX_REQUIRE(v == 1u, CPX_EINVAL, "%s: prim_poly = %u is not primitive (x does not return to 1 after %d steps)", who, prim_poly, N);
    ex[N] = 1;
    return CPX_OK;
}

}  // namespace cpx
