// Mirror figure error as a thin screen on the optical path, for the device kernels and for a host
// build of the same code (its CPU test).
//
// A mirror's measured figure is a height map h(u, w) in the mirror's own frame: an origin and two
// unit, orthogonal axes e_u, e_w in lab coordinates, and a row-major (nw, nu) float64 table of
// heights in metres sampled at u0 + i du, w0 + j dw. A ray that hits the mirror at P with the unit
// incoming direction d and the unit surface normal n gains the optical path
//     delta = -2 h(u(P), w(P)) |d . n|
// (|d . n| = sin of the grazing angle): the thin-screen model, first-order exact for the wavefront
// by Fermat's principle. Positive h is a bump towards the incoming beam whatever sign the quadric's
// gradient has, hence the absolute value.
//
// Every operation is spelled out once, here; the library is built with -ffp-contract=off and the
// host build of the tests likewise, so the stage kernel, the fused chain kernels and g++ give the
// same bits. Evaluation at P = (x, y, z):
//   u = ((x - ox) eux + (y - oy) euy) + (z - oz) euz,  w likewise with e_w
//   per axis (n samples): s = (u - u0) / du; outside when s < 0 or s > n - 1 (never for NaN);
//     sc = s clamped to [0, n - 1] in floating point (NaN -> 0), i = (int) floor(sc), t = sc - floor(sc)
//     (t = NaN for a NaN s); an axis with one sample is constant along it: i = 0, t = 0, never outside
//   Keys cubic convolution with a = -1/2 (Catmull-Rom) over i - 1 .. i + 2, the four indices clamped
//     to [0, n - 1] (edge replicate); weights in Horner form (weights() below)
//   separable: r_j = ((cu0 h[j][i0] + cu1 h[j][i1]) + cu2 h[j][i2]) + cu3 h[j][i3] for the four rows,
//     h = ((cw0 r_0 + cw1 r_1) + cw2 r_2) + cw3 r_3
//   a hit outside on either axis contributes h = +0 and reports it (the caller raises the mirror's
//     AKB_FLAG_FIG_OUTSIDE bit)
//   delta = (-2 h) * |(l nx + m ny) + n nz|
// Index safety: the float-to-int conversion only ever sees a value already clamped to [0, n - 1], and
// the four indices are clamped as integers, so no load leaves the table for any coordinate - NaN,
// +-inf and huge values included. A NaN coordinate (a missed ray) selects index 0 with NaN weights:
// the term is NaN like the rest of the ray's row, and no flag is raised for it.
//
// Slope error (the ray-spot modes): the same sixteen samples and two fractions also give
// the map's gradient, and the gradient turns the normal the reflection uses - no further load.
//   derivative weights in Horner form (dweights() below; they sum to zero)
//   hu = (((cw0 ru'_0 + cw1 ru'_1) + cw2 ru'_2) + cw3 ru'_3) / du with ru'_j row j combined with the
//     derivative weights in u, in combine's association; hw likewise with the plain weights in u and
//     the derivative weights in w, divided by dw; an axis with one sample has derivative +0 along it;
//     a hit outside the map has hu = hw = +0; a NaN fraction gives NaN
//   sigma = (d . N > 0) ? -1 : 1 (sigma N is the normal turned towards the incoming beam; positive h
//     is a bump towards it), g = hu e_u + hw e_w component by component (gx = hu eux + hw ewx),
//     N' = (N - sigma g) / sqrt((x^2 + y^2) + z^2) of the numerator - always normalised for a hit
//     inside the map, N itself for a hit outside it. g is not projected onto the local tangent plane:
//     e_u, e_w are the frame's, and across a footprint the quadric's normal turns by milliradians.
//   N' replaces N in the reflection only (reflect_ray's order, A = (l nx + m ny) + n nz, all three
//     components whatever the mirror's kind); the path term keeps the quadric's own N.
//
// Displaced points (the wave chain): the Huygens sum samples each mirror at the traced hit
// points, so a map moves every sample along the surface normal by its height there - no wavelength
// enters, and no load beyond locate()'s sixteen.
//   dn = (l nx + m ny) + n nz (dot_dn) with N the quadric's unit normal at the hit and d = (l, m, n) the
//     incoming direction; only the sign of dn is read, so d need not be unit
//   sigma = (dn > 0) ? -1 : 1 (deflect's rule: sigma N points towards the incoming beam)
//   h = combine() of the sixteen samples, as in eval
//   s = sigma * h
//   x' = x + s * nx, y' = y + s * ny, z' = z + s * nz
//   a hit outside the map returns (x, y, z) themselves (a select, not P + 0 N) and reports it; a NaN
//     hit gives NaN and no report
// Positive h is a bump towards the incoming beam, as above.
#pragma once

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define AKB_FIG_FN __host__ __device__ __forceinline__
#else
#define AKB_FIG_FN static inline
#endif

namespace akb_fig {

// one mirror's map (akb_figure_map of include/akb_raytrace.h, field for field)
struct Map {
    const double* h;  // (nw, nu) row-major heights in metres; NULL: no map on this mirror
    double o[3], eu[3], ew[3];
    double u0, du, w0, dw;
    int32_t nu, nw;
};

// the Catmull-Rom weights of samples i - 1, i, i + 1, i + 2 at fraction t (they sum to one)
AKB_FIG_FN void weights(double t, double (&c)[4]) {
    c[0] = ((-0.5 * t + 1.0) * t - 0.5) * t;
    c[1] = ((1.5 * t - 2.5) * t) * t + 1.0;
    c[2] = ((-1.5 * t + 2.0) * t + 0.5) * t;
    c[3] = ((0.5 * t - 0.5) * t) * t;
}

// d/dt of weights(): the derivative weights of the same four samples (they sum to zero)
AKB_FIG_FN void dweights(double t, double (&c)[4]) {
    c[0] = (-1.5 * t + 2.0) * t - 0.5;
    c[1] = (4.5 * t - 5.0) * t;
    c[2] = (-4.5 * t + 4.0) * t + 0.5;
    c[3] = (1.5 * t - 1.0) * t;
}

// one axis: the four clamped sample indices and the fraction t; returns true for a coordinate
// outside the map
AKB_FIG_FN bool axis(double u, double u0, double du, int32_t n, int32_t (&idx)[4], double& t_out) {
    double sc = 0.0, t = 0.0;
    bool outside = false;
    if (n > 1) {
        const double s = (u - u0) / du;
        const double top = (double)(n - 1);
        outside = s < 0.0 || s > top;
        sc = s >= 0.0 ? s : 0.0;  // NaN -> 0
        sc = sc <= top ? sc : top;
        t = s != s ? s : sc - floor(sc);
    }
    const int32_t i = (int32_t)floor(sc);  // sc in [0, n - 1]
    const int32_t hi = n - 1;
    idx[0] = i - 1 < 0 ? 0 : i - 1;
    idx[1] = i;
    idx[2] = i + 1 > hi ? hi : i + 1;
    idx[3] = i + 2 > hi ? hi : i + 2;
    t_out = t;
    return outside;
}

// the sixteen table offsets (row-major, 32-bit: the host checks nu * nw < 2^28) and the two fractions
// of the hit (x, y, z); returns true for a hit outside the map. The weights are formed from the
// fractions where the samples are combined, so only two values wait beside the sixteen loads.
AKB_FIG_FN bool locate(const Map& M, double x, double y, double z, int32_t (&off)[16], double& tu, double& tw) {
    const double dx = x - M.o[0], dy = y - M.o[1], dz = z - M.o[2];
    const double u = (dx * M.eu[0] + dy * M.eu[1]) + dz * M.eu[2];
    const double w = (dx * M.ew[0] + dy * M.ew[1]) + dz * M.ew[2];
    int32_t iu[4], iw[4];
    const bool ou = axis(u, M.u0, M.du, M.nu, iu, tu);
    const bool ow = axis(w, M.w0, M.dw, M.nw, iw, tw);
    for (int j = 0; j < 4; ++j)
        for (int i = 0; i < 4; ++i) off[4 * j + i] = iw[j] * M.nu + iu[i];
    return ou || ow;
}

// the height from the sixteen loaded samples v[4 j + i] = h[off[4 j + i]]
AKB_FIG_FN double combine(const double (&v)[16], double tu, double tw, bool outside) {
    double cu[4], cw[4], r[4];
    weights(tu, cu);
    weights(tw, cw);
    for (int j = 0; j < 4; ++j)
        r[j] = ((cu[0] * v[4 * j] + cu[1] * v[4 * j + 1]) + cu[2] * v[4 * j + 2]) + cu[3] * v[4 * j + 3];
    const double h = ((cw[0] * r[0] + cw[1] * r[1]) + cw[2] * r[2]) + cw[3] * r[3];
    return outside ? 0.0 : h;
}

// the map's gradient (dh/du, dh/dw) from the same sixteen samples and two fractions
AKB_FIG_FN void gradient(const double (&v)[16], double tu, double tw, const Map& M, bool outside, double& hu,
                         double& hw) {
    double cu[4], cw[4], du[4], dw[4], r[4], rd[4];
    weights(tu, cu);
    weights(tw, cw);
    dweights(tu, du);
    dweights(tw, dw);
    for (int j = 0; j < 4; ++j) {
        r[j] = ((cu[0] * v[4 * j] + cu[1] * v[4 * j + 1]) + cu[2] * v[4 * j + 2]) + cu[3] * v[4 * j + 3];
        rd[j] = ((du[0] * v[4 * j] + du[1] * v[4 * j + 1]) + du[2] * v[4 * j + 2]) + du[3] * v[4 * j + 3];
    }
    const double gu = (((cw[0] * rd[0] + cw[1] * rd[1]) + cw[2] * rd[2]) + cw[3] * rd[3]) / M.du;
    const double gw = (((dw[0] * r[0] + dw[1] * r[1]) + dw[2] * r[2]) + dw[3] * r[3]) / M.dw;
    hu = (outside || M.nu == 1) ? 0.0 : gu;
    hw = (outside || M.nw == 1) ? 0.0 : gw;
}

// the deflected unit normal N' in place of the unit normal (nx, ny, nz); dn = d . N
AKB_FIG_FN void deflect(double& nx, double& ny, double& nz, double dn, const Map& M, double hu, double hw,
                        bool outside) {
    const double sigma = dn > 0.0 ? -1.0 : 1.0;
    const double gx = hu * M.eu[0] + hw * M.ew[0];
    const double gy = hu * M.eu[1] + hw * M.ew[1];
    const double gz = hu * M.eu[2] + hw * M.ew[2];
    const double x = nx - sigma * gx, y = ny - sigma * gy, z = nz - sigma * gz;
    const double s = sqrt((x * x + y * y) + z * z);
    nx = outside ? nx : x / s;
    ny = outside ? ny : y / s;
    nz = outside ? nz : z / s;
}

// the displaced point P' = P + (sigma h) N in place of the hit (x, y, z); (nx, ny, nz) the unit normal,
// dn = d . N
AKB_FIG_FN void displace(double& x, double& y, double& z, double nx, double ny, double nz, double dn, double h,
                         bool outside) {
    const double sigma = dn > 0.0 ? -1.0 : 1.0;
    const double s = sigma * h;
    const double px = x + s * nx, py = y + s * ny, pz = z + s * nz;
    x = outside ? x : px;
    y = outside ? y : py;
    z = outside ? z : pz;
}

// the path term from the height and d . n
AKB_FIG_FN double path_term(double h, double dn) { return (-2.0 * h) * fabs(dn); }

// d . n in the association order the chain's reflection uses
AKB_FIG_FN double dot_dn(double l, double m, double n, double nx, double ny, double nz) {
    return (l * nx + m * ny) + n * nz;
}

// the whole evaluation for one hit: height in *h (when given), the sixteen offsets in off (when
// given), outside reported in *outside; returns delta
AKB_FIG_FN double eval(const Map& M, double x, double y, double z, double dn, bool* outside, double* h_out,
                       int32_t* off_out) {
    int32_t off[16];
    double tu, tw, v[16];
    const bool o = locate(M, x, y, z, off, tu, tw);
    for (int k = 0; k < 16; ++k) v[k] = M.h[off[k]];
    const double h = combine(v, tu, tw, o);
    if (outside) *outside = o;
    if (h_out) *h_out = h;
    if (off_out)
        for (int k = 0; k < 16; ++k) off_out[k] = off[k];
    return path_term(h, dn);
}

// the deflected normal for one hit with the unit normal (nx, ny, nz) and the unit incoming direction
// (l, m, n): N' in place; returns true for a hit outside the map (N untouched)
AKB_FIG_FN bool eval_normal(const Map& M, double x, double y, double z, double l, double m, double n, double& nx,
                            double& ny, double& nz) {
    int32_t off[16];
    double tu, tw, v[16], hu, hw;
    const bool o = locate(M, x, y, z, off, tu, tw);
    for (int k = 0; k < 16; ++k) v[k] = M.h[off[k]];
    gradient(v, tu, tw, M, o, hu, hw);
    deflect(nx, ny, nz, dot_dn(l, m, n, nx, ny, nz), M, hu, hw, o);
    return o;
}

// the displaced point for one hit with the unit normal (nx, ny, nz) and the incoming direction
// (l, m, n): P' in place, the interpolated height in h (+0 outside); returns true for a hit outside
// the map (P untouched)
AKB_FIG_FN bool eval_displace(const Map& M, double& x, double& y, double& z, double l, double m, double n, double nx,
                              double ny, double nz, double& h) {
    int32_t off[16];
    double tu, tw, v[16];
    const bool o = locate(M, x, y, z, off, tu, tw);
    for (int k = 0; k < 16; ++k) v[k] = M.h[off[k]];
    h = combine(v, tu, tw, o);
    displace(x, y, z, nx, ny, nz, dot_dn(l, m, n, nx, ny, nz), h, o);
    return o;
}

}  // namespace akb_fig
