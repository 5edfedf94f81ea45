"""Shared by test_dd_cpu.py and test_dd_gpu.py: a host (g++) build of csrc/akb_dd.h behind a small
extern "C" shim, the recorded option_mpmath calls of tests/golden/akb_mpmath_17.npz, and a 250-bit
mpmath evaluation of the two primitives written out here (rounded once to float64)."""
import atexit
import ctypes
import functools
import os
import shutil
import subprocess
import tempfile

import numpy as np

from conftest import ROOT, golden

SRC = r'''
#include "akb_dd.h"
using akb_dd::DD;
// op: 0 add, 1 mul, 2 div, 3 sqrt (of a), 4 dd * double (b_hi), 5 dd + double (b_hi), 6 sub
extern "C" void dd_arith(int op, const double* a, const double* b, long n, double* out) {
    for (long i = 0; i < n; ++i) {
        const DD x{a[2 * i], a[2 * i + 1]}, y{b[2 * i], b[2 * i + 1]};
        DD r{0.0, 0.0};
        switch (op) {
            case 0: r = akb_dd::dd_add(x, y); break;
            case 1: r = akb_dd::dd_mul_dd(x, y); break;
            case 2: r = akb_dd::dd_div(x, y); break;
            case 3: r = akb_dd::dd_sqrt(x); break;
            case 4: r = akb_dd::dd_mul_d(x, y.hi); break;
            case 5: r = akb_dd::dd_add_d(x, y.hi); break;
            case 6: r = akb_dd::dd_sub(x, y); break;
        }
        out[2 * i] = r.hi;
        out[2 * i + 1] = r.lo;
    }
}
// the stage kernels' loops on the host: (ptr, ld, inc) views, OR-ed flag word (1: miss, 4: zero reflect)
extern "C" void isect_batch(const double* c, const double* d, long dld, long dinc, const double* o, long old_,
                            long oinc, int negative, long n, double* out, long out_ld, int* flags) {
    double Q[10];
    for (int k = 0; k < 10; ++k) Q[k] = c[k];
    for (long i = 0; i < n; ++i) {
        double x, y, z;
        if (!akb_dd::quadric_hit_dd(Q, d[i * dinc], d[dld + i * dinc], d[2 * dld + i * dinc], o[i * oinc],
                                    o[old_ + i * oinc], o[2 * old_ + i * oinc], negative != 0, x, y, z))
            *flags |= 1;
        out[i] = x;
        out[out_ld + i] = y;
        out[2 * out_ld + i] = z;
    }
}
extern "C" void reflect_batch(const double* d, long dld, long dinc, const double* v, long vld, long vinc, long n,
                              double* out, long out_ld, int* flags) {
    for (long i = 0; i < n; ++i) {
        double x, y, z;
        if (!akb_dd::reflect_dd(d[i * dinc], d[dld + i * dinc], d[2 * dld + i * dinc], v[i * vinc],
                                v[vld + i * vinc], v[2 * vld + i * vinc], x, y, z))
            *flags |= 4;
        out[i] = x;
        out[out_ld + i] = y;
        out[2 * out_ld + i] = z;
    }
}
'''


@functools.lru_cache(maxsize=None)
def host_lib():
    d = tempfile.mkdtemp(prefix="akb_dd_host_")
    atexit.register(shutil.rmtree, d, ignore_errors=True)
    cpp = os.path.join(d, "dd.cpp")
    with open(cpp, "w") as f:
        f.write(SRC)
    so = os.path.join(d, "libdd.so")
    inc = os.path.join(ROOT, "akbraytracing_amd", "csrc")
    subprocess.run(["g++", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-I", inc, cpp, "-o", so], check=True)
    L = ctypes.CDLL(so)
    vp, cl, ci = ctypes.c_void_p, ctypes.c_long, ctypes.c_int
    L.dd_arith.argtypes = [ci, vp, vp, cl, vp]
    L.isect_batch.argtypes = [vp, vp, cl, cl, vp, cl, cl, ci, cl, vp, cl, vp]
    L.reflect_batch.argtypes = [vp, cl, cl, vp, cl, cl, cl, vp, cl, vp]
    return L


def _view(a):
    """(array, ld, inc) of a (3, n) / (3, 1) / (3,) float64 array: one column broadcasts"""
    a = np.ascontiguousarray(a, dtype=np.float64)
    if a.ndim == 1:
        return a, 1, 0
    return a, a.shape[1], (1 if a.shape[1] > 1 else 0)


def host_arith(op, a, b):
    """a, b: (n, 2) arrays of (hi, lo); returns (n, 2)"""
    a = np.ascontiguousarray(a, dtype=np.float64)
    b = np.ascontiguousarray(b, dtype=np.float64)
    out = np.empty_like(a)
    host_lib().dd_arith(op, a.ctypes.data, b.ctypes.data, a.shape[0], out.ctypes.data)
    return out


def host_isect(coeffs, ray, source, negative=False, n=None):
    c = np.ascontiguousarray(coeffs, dtype=np.float64)
    d, dld, dinc = _view(ray)
    o, old_, oinc = _view(source)
    n = max(d.shape[-1] if d.ndim == 2 else 1, o.shape[-1] if o.ndim == 2 else 1) if n is None else n
    out = np.empty((3, n))
    fl = np.zeros(1, dtype=np.int32)
    host_lib().isect_batch(c.ctypes.data, d.ctypes.data, dld, dinc, o.ctypes.data, old_, oinc, int(bool(negative)), n,
                           out.ctypes.data, n, fl.ctypes.data)
    return out, int(fl[0])


def host_reflect(ray, nrm, n=None):
    d, dld, dinc = _view(ray)
    v, vld, vinc = _view(nrm)
    n = max(d.shape[-1] if d.ndim == 2 else 1, v.shape[-1] if v.ndim == 2 else 1) if n is None else n
    out = np.empty((3, n))
    fl = np.zeros(1, dtype=np.int32)
    host_lib().reflect_batch(d.ctypes.data, dld, dinc, v.ctypes.data, vld, vinc, n, out.ctypes.data, n,
                             fl.ctypes.data)
    return out, int(fl[0])


# ---- the recorded calls -----------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def fixture():
    return golden("akb_mpmath_17.npz")


@functools.lru_cache(maxsize=None)
def calls():
    """[(key, name, inputs, negative, reference output, reference deviation in ulp)] in call order"""
    f = fixture()
    out = []
    for k in sorted(x[:-4] for x in f.files if x.startswith("c") and x.endswith("_out")):
        name = k.split("_", 1)[1]
        ins = [f[f"{k}_in{j}"] for j in range(3 if name == "mirr_ray_intersection" else 2)]
        out.append((k, name, ins, bool(f[f"{k}_neg"]), f[f"{k}_out"], float(f[f"{k}_refdev"])))
    return out


# ---- the exact evaluation (mpmath, 250 bits, rounded once) ------------------------------------

PREC = 250


def mp_isect(coeffs, ray, source, negative=False):
    import mpmath
    ray = np.asarray(ray, dtype=np.float64).reshape(3, -1)
    source = np.asarray(source, dtype=np.float64).reshape(3, -1)
    out = np.empty((3, ray.shape[1]))
    with mpmath.workprec(PREC):
        mpf = mpmath.mpf
        a, b, c, d, e, f, g, h, i, j = (mpf(float(x)) for x in coeffs)
        for col in range(ray.shape[1]):
            l, m, n = (mpf(float(v)) for v in ray[:, col])
            p, q, r = (mpf(float(v)) for v in source[:, col])
            A = a * l * l + b * m * m + c * n * n + d * m * l + e * n * l + f * m * n
            B = (2 * a * p * l + 2 * b * q * m + 2 * c * r * n + d * (p * m + q * l) + e * (p * n + r * l)
                 + f * (r * m + q * n) + g * l + h * m + i * n)
            C = a * p * p + b * q * q + c * r * r + d * p * q + e * p * r + f * q * r + g * p + h * q + i * r + j
            D = B * B - 4 * A * C
            if D < 0:
                out[:, col] = np.nan
                continue
            s = mpmath.sqrt(D)
            t = (-B - s) / (2 * A) if negative else (-B + s) / (2 * A)
            out[:, col] = [float(t * l + p), float(t * m + q), float(t * n + r)]
    return out


def mp_reflect(ray, nrm):
    import mpmath
    ray = np.asarray(ray, dtype=np.float64).reshape(3, -1)
    nrm = np.asarray(nrm, dtype=np.float64).reshape(3, -1)
    out = np.empty((3, ray.shape[1]))
    with mpmath.workprec(PREC):
        mpf = mpmath.mpf
        for col in range(ray.shape[1]):
            l, m, n = (mpf(float(v)) for v in ray[:, col])
            nx, ny, nz = (mpf(float(v)) for v in nrm[:, col])
            A = l * nx + m * ny + n * nz
            phi = [l - 2 * A * nx, m - 2 * A * ny, n - 2 * A * nz]
            s = mpmath.sqrt(phi[0] * phi[0] + phi[1] * phi[1] + phi[2] * phi[2])
            if s != 0:
                phi = [v / s for v in phi]
            out[:, col] = [float(v) for v in phi]
    return out


@functools.lru_cache(maxsize=None)
def exact_outputs():
    """the 250-bit evaluation of every recorded call, computed once and shared (read-only)"""
    res = {}
    for key, name, ins, neg, _, _ in calls():
        r = mp_isect(ins[0], ins[1], ins[2], neg) if name == "mirr_ray_intersection" else mp_reflect(ins[0], ins[1])
        r.setflags(write=False)
        res[key] = r
    return res


def ulp_dev(got, want):
    """|got - want| per column in ulp of the expected column's largest component,
    np.spacing(max(|x|, |y|, |z|)); a NaN matches a NaN"""
    got = np.asarray(got, dtype=np.float64).reshape(3, -1)
    want = np.asarray(want, dtype=np.float64).reshape(3, -1)
    both_nan = np.isnan(got) & np.isnan(want)
    scale = np.spacing(np.max(np.abs(want), axis=0))
    return np.max(np.where(both_nan, 0.0, np.abs(got - want) / scale), axis=0)
