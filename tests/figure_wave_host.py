"""Shared by test_figure_wave_cpu.py and test_figure_wave_gpu.py: a host (g++) build of the displacement
part of csrc/akb_figure.h (displace, eval_displace) behind a small extern "C" shim that runs the stage
kernel's loop, beside figure_host.py's and figure_slope_host.py's builds of the other parts."""
import atexit
import ctypes
import functools
import os
import shutil
import subprocess
import tempfile

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
// the stage kernel's loop on the host: unit normal by norm_vector's expressions, then the displaced
// point (the hit itself where the normal has zero norm); flag word bits 0x8 (outside) and 0x2 (zero
// normal). unit (3, n), when given, receives the unit normals; outside (n) the per-sample report
extern "C" void fw_stage(const double* tab, const double* frame, const double* grid, int nu, int nw,
                         const double* c, const double* hit, const double* dir, long n, double* out, double* h_out,
                         double* unit, int* outside, int* flags) {
    const Map M = make(tab, frame, grid, nu, nw);
    for (long i = 0; i < n; ++i) {
        const double x = hit[i], y = hit[n + i], z = hit[2 * n + i];
        double nx = 2.0 * c[0] * x + c[3] * y + c[4] * z + c[6];
        double ny = 2.0 * c[1] * y + c[3] * x + c[5] * z + c[7];
        double nz = 2.0 * c[2] * z + c[4] * x + c[5] * y + c[8];
        const double s = sqrt(nx * nx + ny * ny + nz * nz);
        const bool zero = s == 0.0;
        if (zero) *flags |= 2;
        nx = nx / s;
        ny = ny / s;
        nz = nz / s;
        double px = x, py = y, pz = z, h;
        const bool o = akb_fig::eval_displace(M, px, py, pz, dir[i], dir[n + i], dir[2 * n + i], nx, ny, nz, h);
        if (o) *flags |= 8;
        out[i] = zero ? x : px;
        out[n + i] = zero ? y : py;
        out[2 * n + i] = zero ? z : pz;
        if (h_out) h_out[i] = h;
        if (unit) {
            unit[i] = nx;
            unit[n + i] = ny;
            unit[2 * n + i] = nz;
        }
        if (outside) outside[i] = o;
    }
}
// displace() alone on given unit normals, d . N and heights
extern "C" void fw_displace(const double* p, const double* nrm, const double* dn, const double* h, const int* outside,
                            long n, double* out) {
    for (long i = 0; i < n; ++i) {
        double x = p[i], y = p[n + i], z = p[2 * n + i];
        akb_fig::displace(x, y, z, nrm[i], nrm[n + i], nrm[2 * n + i], dn[i], h[i], outside[i] != 0);
        out[i] = x;
        out[n + i] = y;
        out[2 * n + i] = z;
    }
}
'''


@functools.lru_cache(maxsize=None)
def host_lib():
    d = tempfile.mkdtemp(prefix="akb_fig_wave_host_")
    atexit.register(shutil.rmtree, d, ignore_errors=True)
    cpp = os.path.join(d, "figw.cpp")
    with open(cpp, "w") as f:
        f.write(SRC)
    so = os.path.join(d, "libfigw.so")
    subprocess.run(["g++", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-I", CSRC, cpp, "-o", so], check=True)
    L = ctypes.CDLL(so)
    vp, cl, ci = ctypes.c_void_p, ctypes.c_long, ctypes.c_int
    L.fw_stage.argtypes = [vp, vp, vp, ci, ci, vp, vp, vp, cl, vp, vp, vp, vp, vp]
    L.fw_displace.argtypes = [vp, vp, vp, vp, vp, cl, vp]
    return L


def _pack(fm):
    tab = np.ascontiguousarray(fm.height, dtype=np.float64)
    frame = np.ascontiguousarray(np.concatenate([fm.origin, fm.e_u, fm.e_w]), dtype=np.float64)
    grid = np.array([fm.u0, fm.du, fm.w0, fm.dw], dtype=np.float64)
    return tab, frame, grid


def host_stage(fm, coeffs, hit, dirs):
    """the stage kernel's loop on the host: a dict with points (3, n), h (n), unit (3, n) the quadric's
    unit normals, outside (n) bool and the flag word"""
    tab, frame, grid = _pack(fm)
    c = np.ascontiguousarray(coeffs, dtype=np.float64)
    hit = np.ascontiguousarray(hit, dtype=np.float64)
    dirs = np.ascontiguousarray(dirs, dtype=np.float64)
    n = hit.shape[1]
    assert dirs.shape == hit.shape
    out, h, unit = np.empty((3, n)), np.empty(n), np.empty((3, n))
    o = np.zeros(n, dtype=np.int32)
    fl = np.zeros(1, dtype=np.int32)
    host_lib().fw_stage(tab.ctypes.data, frame.ctypes.data, grid.ctypes.data, fm.nu, fm.nw, c.ctypes.data,
                        hit.ctypes.data, dirs.ctypes.data, n, out.ctypes.data, h.ctypes.data, unit.ctypes.data,
                        o.ctypes.data, fl.ctypes.data)
    return dict(points=out, h=h, unit=unit, outside=o.astype(bool), flags=int(fl[0]))


def host_displace(p, nrm, dn, h, outside=None):
    """displace() of the header on points p (3, n), unit normals nrm (3, n), dn (n), h (n)"""
    p = np.ascontiguousarray(p, dtype=np.float64)
    nrm = np.ascontiguousarray(nrm, dtype=np.float64)
    n = p.shape[1]
    dn = np.ascontiguousarray(np.broadcast_to(np.asarray(dn, dtype=np.float64), (n,)))
    h = np.ascontiguousarray(np.broadcast_to(np.asarray(h, dtype=np.float64), (n,)))
    o = np.zeros(n, dtype=np.int32) if outside is None else np.ascontiguousarray(outside, dtype=np.int32)
    out = np.empty((3, n))
    host_lib().fw_displace(p.ctypes.data, nrm.ctypes.data, dn.ctypes.data, h.ctypes.data, o.ctypes.data, n,
                           out.ctypes.data)
    return out
