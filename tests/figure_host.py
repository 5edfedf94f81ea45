"""Shared by test_figure_cpu.py and test_figure_gpu.py: a host (g++) build of csrc/akb_figure.h behind
a small extern "C" shim, and an independent restatement of the evaluation in exact rational
arithmetic (fractions.Fraction) that does not call the header."""
import atexit
import ctypes
import functools
import os
import shutil
import subprocess
import tempfile
from fractions import Fraction

import numpy as np

from conftest import ROOT

CSRC = os.path.join(ROOT, "akbraytracing_amd", "csrc")

SRC = r'''
#include "akb_figure.h"
using akb_fig::Map;
static Map make(const double* tab, const double* frame, const double* grid, int nu, int nw) {
    Map M;
    M.h = tab;
    for (int k = 0; k < 3; ++k) {
        M.o[k] = frame[k];
        M.eu[k] = frame[3 + k];
        M.ew[k] = frame[6 + k];
    }
    M.u0 = grid[0];
    M.du = grid[1];
    M.w0 = grid[2];
    M.dw = grid[3];
    M.nu = nu;
    M.nw = nw;
    return M;
}
// the header's evaluation at n points (pts (3, n)) with given d . n: delta, height, the sixteen
// table offsets and the outside report of each
extern "C" void fig_eval(const double* tab, const double* frame, const double* grid, int nu, int nw,
                         const double* pts, const double* dn, long n, double* delta, double* h, int* off,
                         int* outside) {
    const Map M = make(tab, frame, grid, nu, nw);
    for (long i = 0; i < n; ++i) {
        bool o;
        delta[i] = akb_fig::eval(M, pts[i], pts[n + i], pts[2 * n + i], dn[i], &o, h + i, off + 16 * i);
        outside[i] = o;
    }
}
// the stage kernel's loop on the host: unit normal by norm_vector's expressions, then the term;
// flag word bits 0x8 (outside) and 0x2 (zero normal)
extern "C" void fig_stage(const double* tab, const double* frame, const double* grid, int nu, int nw,
                          const double* c, const double* hit, const double* dir, long n, double* out,
                          int accumulate, int* flags) {
    const Map M = make(tab, frame, grid, nu, nw);
    for (long i = 0; i < n; ++i) {
        const double x = hit[i], y = hit[n + i], z = hit[2 * n + i];
        double nx = 2.0 * c[0] * x + c[3] * y + c[4] * z + c[6];
        double ny = 2.0 * c[1] * y + c[3] * x + c[5] * z + c[7];
        double nz = 2.0 * c[2] * z + c[4] * x + c[5] * y + c[8];
        const double s = sqrt(nx * nx + ny * ny + nz * nz);
        if (s == 0.0) *flags |= 2;
        const double dn = akb_fig::dot_dn(dir[i], dir[n + i], dir[2 * n + i], nx / s, ny / s, nz / s);
        bool o;
        const double d = akb_fig::eval(M, x, y, z, dn, &o, nullptr, nullptr);
        if (o) *flags |= 8;
        out[i] = (accumulate ? out[i] : 0.0) + d;
    }
}
'''


@functools.lru_cache(maxsize=None)
def host_lib():
    d = tempfile.mkdtemp(prefix="akb_fig_host_")
    atexit.register(shutil.rmtree, d, ignore_errors=True)
    cpp = os.path.join(d, "fig.cpp")
    with open(cpp, "w") as f:
        f.write(SRC)
    so = os.path.join(d, "libfig.so")
    subprocess.run(["g++", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-I", CSRC, cpp, "-o", so], check=True)
    L = ctypes.CDLL(so)
    vp, cl, ci = ctypes.c_void_p, ctypes.c_long, ctypes.c_int
    L.fig_eval.argtypes = [vp, vp, vp, ci, ci, vp, vp, cl, vp, vp, vp, vp]
    L.fig_stage.argtypes = [vp, vp, vp, ci, ci, vp, vp, vp, cl, vp, ci, vp]
    return L


def _pack(fm):
    tab = np.ascontiguousarray(fm.height, dtype=np.float64)
    frame = np.ascontiguousarray(np.concatenate([fm.origin, fm.e_u, fm.e_w]), dtype=np.float64)
    grid = np.array([fm.u0, fm.du, fm.w0, fm.dw], dtype=np.float64)
    return tab, frame, grid


def host_eval(fm, pts, dn):
    """the header at pts (3, n) with d . n = dn (n): (delta, h, offsets (n, 16), outside (n) bool)"""
    tab, frame, grid = _pack(fm)
    pts = np.ascontiguousarray(pts, dtype=np.float64)
    n = pts.shape[1]
    dn = np.ascontiguousarray(np.broadcast_to(np.asarray(dn, dtype=np.float64), (n,)))
    delta, h = np.empty(n), np.empty(n)
    off = np.empty((n, 16), dtype=np.int32)
    out = np.empty(n, dtype=np.int32)
    host_lib().fig_eval(tab.ctypes.data, frame.ctypes.data, grid.ctypes.data, fm.nu, fm.nw, pts.ctypes.data,
                        dn.ctypes.data, n, delta.ctypes.data, h.ctypes.data, off.ctypes.data, out.ctypes.data)
    return delta, h, off, out.astype(bool)


def host_stage(fm, coeffs, hit, dirs, out=None):
    """the stage kernel's loop on the host; out given: accumulate into it. Returns (out, flags)."""
    tab, frame, grid = _pack(fm)
    c = np.ascontiguousarray(coeffs, dtype=np.float64)
    hit = np.ascontiguousarray(hit, dtype=np.float64)
    dirs = np.ascontiguousarray(dirs, dtype=np.float64)
    n = hit.shape[1]
    acc = out is not None
    out = np.empty(n) if out is None else np.ascontiguousarray(out, dtype=np.float64).copy()
    fl = np.zeros(1, dtype=np.int32)
    host_lib().fig_stage(tab.ctypes.data, frame.ctypes.data, grid.ctypes.data, fm.nu, fm.nw, c.ctypes.data,
                         hit.ctypes.data, dirs.ctypes.data, n, out.ctypes.data, int(acc), fl.ctypes.data)
    return out, int(fl[0])


# ---- the exact evaluation (rational arithmetic; written from the model, not from the header) ----

def _F(x):
    return Fraction(float(x))


def _cr_weights(t):
    """Keys' cubic convolution kernel with a = -1/2 at distances 1 + t, t, 1 - t, 2 - t"""
    a = Fraction(-1, 2)

    def k(x):
        x = abs(x)
        if x <= 1:
            return (a + 2) * x**3 - (a + 3) * x**2 + 1
        if x < 2:
            return a * x**3 - 5 * a * x**2 + 8 * a * x - 4 * a
        return Fraction(0)
    return [k(1 + t), k(t), k(1 - t), k(2 - t)]


def _exact_axis(u, u0, du, n):
    """(indices, weights, outside) of one axis for the exact coordinate u"""
    if n == 1:
        return [0, 0, 0, 0], [Fraction(0), Fraction(1), Fraction(0), Fraction(0)], False
    s = (u - u0) / du
    outside = s < 0 or s > n - 1
    sc = min(max(s, Fraction(0)), Fraction(n - 1))
    i = sc.numerator // sc.denominator
    t = sc - i
    idx = [min(max(i + d, 0), n - 1) for d in (-1, 0, 1, 2)]
    return idx, _cr_weights(t), outside


def exact_eval(fm, pts, dn):
    """delta, h (as floats rounded once from the exact value), outside, and S = sum |w_i w_j h_ij|
    (float, rounded up a little) per point, for finite points"""
    pts = np.asarray(pts, dtype=np.float64)
    n = pts.shape[1]
    dn = np.broadcast_to(np.asarray(dn, dtype=np.float64), (n,))
    o = [_F(v) for v in fm.origin]
    eu = [_F(v) for v in fm.e_u]
    ew = [_F(v) for v in fm.e_w]
    delta, h, outside, S = np.empty(n), np.empty(n), np.zeros(n, dtype=bool), np.empty(n)
    for c in range(n):
        d = [_F(pts[k, c]) - o[k] for k in range(3)]
        u = sum(d[k] * eu[k] for k in range(3))
        w = sum(d[k] * ew[k] for k in range(3))
        iu, cu, ou = _exact_axis(u, _F(fm.u0), _F(fm.du), fm.nu)
        iw, cw, ow = _exact_axis(w, _F(fm.w0), _F(fm.dw), fm.nw)
        val = Fraction(0)
        sabs = Fraction(0)
        for j in range(4):
            for i in range(4):
                term = cw[j] * cu[i] * _F(fm.height[iw[j], iu[i]])
                val += term
                sabs += abs(term)
        outside[c] = ou or ow
        if outside[c]:
            val = Fraction(0)
        h[c] = float(val)
        delta[c] = float(-2 * val * abs(_F(dn[c])))
        S[c] = float(sabs) * (1 + 2.0**-50)
    return delta, h, outside, S


EPS = 2.0**-53


def error_bound(fm, pts, dn, S):
    """A bound on |header - exact| of delta at finite points inside the map (or exactly classified),
    derived from the header's operation count (u = 2^-53 per rounding, first order, with a factor 2
    of slack for the second-order terms):

    coordinates  u_fl: per axis three differences, three products, two sums - each term of the dot
                 product passes at most 4 roundings: |u_fl - u| <= 4 u sum_k |d_k e_k|; s = (u - u0) / du
                 adds the difference's and the quotient's rounding: ds <= (|u_fl - u| + u |u - u0|) / du + u |s|.
                 t = sc - floor(sc) is exact. The interpolant is C1 and piecewise cubic; its
                 derivative in s is at most sum_i |w_i'(t)| Hmax <= 3 Hmax per axis (the maximum of
                 the four |w_i'| sums over [0, 1], at t = 1/2), times the other axis's sum of |w_j| <= 5/4
                 (at t = 1/2): a coordinate error moves h by at most 3.75 Hmax ds.
    weights      each Horner form is at most 6 roundings of partial results bounded by 5 (the sum of
                 |coefficients| at |t| <= 1): |dc| <= 30 u, on 8 weights, each multiplying at most
                 5/4 Hmax of the other axis's weighted samples: <= 8 * 30 u * 1.25 Hmax = 300 u Hmax.
    combination  every product w_j (w_i h_ij) passes at most 8 roundings (its two products and at most
                 three additions in each of the two left-to-right sums): <= 8 u S with
                 S = sum |w_i w_j h_ij|.
    path term    -2 h is exact; the product with |d . n| rounds once: u |delta|.
    """
    pts = np.asarray(pts, dtype=np.float64)
    n = pts.shape[1]
    dn = np.abs(np.broadcast_to(np.asarray(dn, dtype=np.float64), (n,)))
    Hmax = float(np.max(np.abs(fm.height)))
    d = np.abs(pts - fm.origin.reshape(3, 1))
    ds = np.zeros(n)
    for e, x0, dx, m in ((fm.e_u, fm.u0, fm.du, fm.nu), (fm.e_w, fm.w0, fm.dw, fm.nw)):
        if m == 1:
            continue
        mag = (d * np.abs(e).reshape(3, 1)).sum(axis=0)
        ds += (4 * EPS * mag + EPS * (mag + abs(x0))) / dx + EPS * (mag + abs(x0)) / dx
    eh = 3.75 * Hmax * ds + 300 * EPS * Hmax + 8 * EPS * S
    return 2.0 * (2.0 * dn * eh + EPS * 2.0 * dn * Hmax * 1.25 * 1.25)
