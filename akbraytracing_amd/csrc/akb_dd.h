// Double-double (double-word) arithmetic and the two primitives of the reference's option_mpmath
// branch, for the device kernels and for a host build of the same code (its CPU test).
//
// With option_mpmath set, the reference evaluates mirr_ray_intersection and reflect_ray column by
// column in mpmath at mp.dps = 20 (AKB_raytrace_20250312.py:399-443, :474-500, :510-552) and rounds
// the result to float64; every input and output is float64. Here the arithmetic in between runs on
// unevaluated sums hi + lo of two float64s (|lo| <= ulp(hi) / 2, ~106 bits), which is wider than
// mp.dps = 20 (~70 bits) and maps onto v_fma_f64 / v_add_f64.
//
// The library is built with -ffp-contract=off: every error-free product is an explicit
// __builtin_fma and nothing relies on contraction. Division and square root of one double are the
// IEEE correctly rounded operations on the host and on gfx950, so both builds give the same bits.
//
// Relative error bounds, u = 2^-53 (all at most 2^-100):
//   dd_add          3 u^2 + 13 u^3   AccurateDWPlusDW, Joldes, Muller, Popescu, "Tight and rigorous
//                                    error bounds for basic building blocks of double-word
//                                    arithmetic", ACM TOMS 44(2), 2017, Algorithm 6 / Theorem 3.1
//   dd_add_d        2 u^2            DWPlusFP, ibid. Algorithm 4 / Theorem 2.2
//   dd_mul_d        2 u^2            DWTimesFP3, ibid. Algorithm 9 / Theorem 4.3
//   dd_mul_dd       5 u^2            DWTimesDW3, ibid. Algorithm 12 / Theorem 5.3 (4 u^2 there; 5 u^2
//                                    in the formal proof of Muller and Rideau, "Formalization of
//                                    double-word arithmetic, and comments on [the above]", ACM TOMS
//                                    48(1), 2022)
//   dd_div          15 u^2 + 56 u^3  DWDivDW2, JMP 2017 Algorithm 17 / Theorem 6.2   (< 2^-102)
//   dd_sqrt         25/8 u^2         SQRTDWtoDW, Lefevre, Louvet, Muller, Picot, Rideau, "Accurate
//                                    calculation of Euclidean norms using double-word arithmetic",
//                                    ACM TOMS 49(1), 2023, Algorithm 8 / Theorem 4.2
//   two_prod        exact (no underflow), the first-level products of two float64s
// dd_to_double(x) is x.hi: every operation returns a normalised pair, hi = RN(hi + lo).
#pragma once

#include <math.h>

#include "akb_sincos.h"

#define AKB_DD_FN AKB_SC_FN

namespace akb_dd {

using akb_sc::DD;
using akb_sc::dd_add;
using akb_sc::fast_two_sum;
using akb_sc::two_prod;
using akb_sc::two_sum;

AKB_DD_FN DD dd_neg(DD a) { return DD{-a.hi, -a.lo}; }
AKB_DD_FN DD dd_sub(DD a, DD b) { return dd_add(a, dd_neg(b)); }
// multiplication by a power of two is exact on both words
AKB_DD_FN DD dd_scale2(DD a, double pow2) { return DD{a.hi * pow2, a.lo * pow2}; }

AKB_DD_FN DD dd_add_d(DD a, double b) {
    const DD s = two_sum(a.hi, b);
    return fast_two_sum(s.hi, a.lo + s.lo);
}

AKB_DD_FN DD dd_mul_d(DD a, double b) {
    const DD c = two_prod(a.hi, b);
    return fast_two_sum(c.hi, __builtin_fma(a.lo, b, c.lo));
}

AKB_DD_FN DD dd_mul_dd(DD a, DD b) {
    const DD c = two_prod(a.hi, b.hi);
    const double t0 = a.lo * b.lo;
    const double t1 = __builtin_fma(a.hi, b.lo, t0);
    const double c2 = __builtin_fma(a.lo, b.hi, t1);
    return fast_two_sum(c.hi, c.lo + c2);
}

AKB_DD_FN DD dd_div(DD x, DD y) {
    const double th = x.hi / y.hi;
    const DD r = dd_mul_d(y, th);
    const double ph = x.hi - r.hi;  // exact
    const double dl = x.lo - r.lo;
    const double tl = (ph + dl) / y.hi;
    return fast_two_sum(th, tl);
}

// x >= 0; +0 for x == 0 (the algorithm's quotient would be 0 / 0)
AKB_DD_FN DD dd_sqrt(DD x) {
    if (x.hi == 0.0) return DD{0.0, 0.0};
    const double sh = sqrt(x.hi);
    const double r1 = __builtin_fma(-sh, sh, x.hi);
    const double r2 = x.lo + r1;
    return fast_two_sum(sh, r2 / (2.0 * sh));
}

AKB_DD_FN double dd_to_double(DD a) { return a.hi; }

// coefficient * (exact product of two ray components)
AKB_DD_FN DD term(double c, double x, double y) { return dd_mul_d(two_prod(x, y), c); }

// mirr_ray_intersection's mpmath branch for one column (AKB_raytrace_20250312.py:415-440): A, B, C,
// D = B^2 - 4AC, t = (-B +- sqrt D) / (2A), point = t * ray + source, in double-double from float64
// inputs, the point rounded once to float64. Returns false, with a NaN point, where D < 0 (the
// branch's per-column rule; D == 0 is a hit). Q: the ten coefficients a..j.
AKB_DD_FN bool quadric_hit_dd(const double (&Q)[10], double l, double m, double n, double p, double q, double r,
                              bool negative, double& x, double& y, double& z) {
    const double a = Q[0], b = Q[1], c = Q[2], d = Q[3], e = Q[4], f = Q[5], g = Q[6], h = Q[7], i = Q[8], j = Q[9];
    DD A = term(a, l, l);
    A = dd_add(A, term(b, m, m));
    A = dd_add(A, term(c, n, n));
    A = dd_add(A, term(d, m, l));
    A = dd_add(A, term(e, n, l));
    A = dd_add(A, term(f, m, n));

    DD B = dd_scale2(term(a, p, l), 2.0);
    B = dd_add(B, dd_scale2(term(b, q, m), 2.0));
    B = dd_add(B, dd_scale2(term(c, r, n), 2.0));
    B = dd_add(B, dd_mul_d(dd_add(two_prod(p, m), two_prod(q, l)), d));
    B = dd_add(B, dd_mul_d(dd_add(two_prod(p, n), two_prod(r, l)), e));
    B = dd_add(B, dd_mul_d(dd_add(two_prod(r, m), two_prod(q, n)), f));
    B = dd_add(B, two_prod(g, l));
    B = dd_add(B, two_prod(h, m));
    B = dd_add(B, two_prod(i, n));

    DD C = term(a, p, p);
    C = dd_add(C, term(b, q, q));
    C = dd_add(C, term(c, r, r));
    C = dd_add(C, term(d, p, q));
    C = dd_add(C, term(e, p, r));
    C = dd_add(C, term(f, q, r));
    C = dd_add(C, two_prod(g, p));
    C = dd_add(C, two_prod(h, q));
    C = dd_add(C, two_prod(i, r));
    C = dd_add_d(C, j);

    const DD D = dd_sub(dd_mul_dd(B, B), dd_scale2(dd_mul_dd(A, C), 4.0));
    if (D.hi < 0.0 || (D.hi == 0.0 && D.lo < 0.0)) {
        x = y = z = __builtin_nan("");
        return false;
    }
    const DD s = dd_sqrt(D);
    const DD num = negative ? dd_sub(dd_neg(B), s) : dd_add(dd_neg(B), s);
    const DD t = dd_div(num, dd_scale2(A, 2.0));
    x = dd_to_double(dd_add_d(dd_mul_d(t, l), p));
    y = dd_to_double(dd_add_d(dd_mul_d(t, m), q));
    z = dd_to_double(dd_add_d(dd_mul_d(t, n), r));
    return true;
}

// reflect_ray's mpmath branch for one column (:481-498, :510-552): A = ray . N, phi = ray - 2 A N,
// then phi / ||phi||, rounded once to float64. A column of zero norm is left unnormalised (returns
// false). The three quotients share one double-double reciprocal of the norm (dd_div of 1, then
// dd_mul_dd: (15 + 5) u^2 + O(u^3) on top of the norm's own error, still below 2^-100).
AKB_DD_FN bool reflect_dd(double l, double m, double n, double nx, double ny, double nz, double& rx, double& ry,
                          double& rz) {
    DD A = two_prod(l, nx);
    A = dd_add(A, two_prod(m, ny));
    A = dd_add(A, two_prod(n, nz));
    const DD A2 = dd_scale2(A, -2.0);
    const DD fx = dd_add_d(dd_mul_d(A2, nx), l);
    const DD fy = dd_add_d(dd_mul_d(A2, ny), m);
    const DD fz = dd_add_d(dd_mul_d(A2, nz), n);
    const DD s2 = dd_add(dd_add(dd_mul_dd(fx, fx), dd_mul_dd(fy, fy)), dd_mul_dd(fz, fz));
    if (s2.hi == 0.0) {
        rx = fx.hi;
        ry = fy.hi;
        rz = fz.hi;
        return false;
    }
    const DD inv = dd_div(DD{1.0, 0.0}, dd_sqrt(s2));
    rx = dd_to_double(dd_mul_dd(fx, inv));
    ry = dd_to_double(dd_mul_dd(fy, inv));
    rz = dd_to_double(dd_mul_dd(fz, inv));
    return true;
}

}  // namespace akb_dd
