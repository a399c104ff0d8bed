// unit_phasor(u) = (cos 2 pi u, sin 2 pi u) for |u| <= 0.5 as a fixed sequence of float64 operations, so that a host model repeats it
// bit for bit (sincos / sincospi differ in their last bits between libraries, which a feedback loop with decisions turns into
// different results).  With -ffp-contract=off, every operation rounded on its own:
//   q = rint(4 u) (ties to even; -2 .. 2),  r = u - 0.25 q (exact, |r| <= 0.125),  x = r * 6.283185307179586 (|x| <= pi / 4),
//   x2 = x x,  p = S8, p = p x2 + S_k for k = 7 .. 0, sin = x p;  c = C8, c = c x2 + C_k for k = 7 .. 0, cos = c,
//   with S_k = (-1)^k / (2k + 1)! and C_k = (-1)^k / (2k)! as the nearest doubles (Taylor through x^17 and x^16);
//   quadrant by exact swaps and negations: q = 0: (cos, sin); 1: (-sin, cos); 2 and -2: (-cos, -sin); -1: (sin, -cos).
// Each part is within 2^-51 of the true value (DESIGN 4.26 has the derivation; tests/test_recovery_host.py measures it).
#pragma once

namespace cpx {

__device__ __forceinline__ void unit_phasor(double u, double &c, double &s) {
    const double qd = __builtin_rint(4.0 * u);
    const double r = u - 0.25 * qd;
    const double x = r * 6.283185307179586;
    const double x2 = x * x;
    double p = 2.8114572543455206e-15;
    p = p * x2 + -7.647163731819816e-13;
    p = p * x2 + 1.6059043836821613e-10;
    p = p * x2 + -2.505210838544172e-08;
    p = p * x2 + 2.7557319223985893e-06;
    p = p * x2 + -0.0001984126984126984;
    p = p * x2 + 0.008333333333333333;
    p = p * x2 + -0.16666666666666666;
    p = p * x2 + 1.0;
    const double sn = x * p;
    double g = 4.779477332387385e-14;
    g = g * x2 + -1.1470745597729725e-11;
    g = g * x2 + 2.08767569878681e-09;
    g = g * x2 + -2.755731922398589e-07;
    g = g * x2 + 2.48015873015873e-05;
    g = g * x2 + -0.001388888888888889;
    g = g * x2 + 0.041666666666666664;
    g = g * x2 + -0.5;
    g = g * x2 + 1.0;
    const int q = (int)qd;
    c = q == 0 ? g : q == 1 ? -sn : q == -1 ? sn : -g;
    s = q == 0 ? sn : q == 1 ? g : q == -1 ? -g : -sn;
}

}  // namespace cpx
