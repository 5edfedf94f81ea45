"""The slope part of csrc/akb_figure.h without a GPU (a g++ build, figure_slope_host.py): the derivative
weights, the gradient of the interpolant, and the deflected normal against closed forms."""
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import figure_slope_host as FS
from conftest import ROOT, golden_json

from akbraytracing_amd.figure import FigureMap, _centre_ray, mirror_frames

U = 2.0**-53  # one rounding


def _geom():
    from akbraytracing_amd.wavefront import SystemGeometry
    return SystemGeometry.from_dict(golden_json("akb_geometry.json"))


def _exact_dweights(t):
    """d/dt of Keys' cubic convolution kernel (a = -1/2) at distances 1 + t, t, 1 - t, 2 - t, written
    from the kernel's definition, not from the header's Horner forms"""
    a = Fraction(-1, 2)

    def dk(x):  # x >= 0
        if x <= 1:
            return 3 * (a + 2) * x * x - 2 * (a + 3) * x
        return 3 * a * x * x - 10 * a * x + 8 * a
    return [dk(1 + t), dk(t), -dk(1 - t), -dk(2 - t)]


def test_dweights_sum_derivative_and_exact_ends():
    """each Horner form is at most 4 operations on partial results bounded by 5 for t in [0, 1]
    (|4.5 t - 5| <= 5 is the largest): |error| <= 4 * 5 u = 20 u per weight; their sum adds three
    roundings of values below 2: |sum| <= 4 * 20 u + 3 * 2 u"""
    rng = np.random.default_rng(1)
    t = np.concatenate([rng.uniform(0, 1, 500), [0.0, 1.0, 0.5, 2.0**-30, 1 - 2.0**-30]])
    _, dc = FS.host_weights(t)
    for i, ti in enumerate(t):
        want = _exact_dweights(Fraction(float(ti)))
        assert sum(want) == 0
        err = max(abs(Fraction(float(dc[i, k])) - want[k]) for k in range(4))
        assert err <= 20 * U, (ti, float(err))
    assert np.all(np.abs(((dc[:, 0] + dc[:, 1]) + dc[:, 2]) + dc[:, 3]) <= 86 * U)
    _, ends = FS.host_weights([0.0, 1.0])
    assert np.array_equal(ends[0], [-0.5, 0.0, 0.5, 0.0]) and np.array_equal(ends[1], [0.0, -0.5, 0.0, 0.5])


def test_gradient_is_continuous_across_cells():
    """C1: at t = 1 of cell i and at t = 0 of cell i + 1 the same samples meet the same weights (the
    derivative weights there are exactly (0, -1/2, 0, 1/2) and (-1/2, 0, 1/2, 0), the plain ones (0, 0, 1,
    0) and (0, 1, 0, 0)); the zero products add +-0, so only the association could differ. Bound: 4 ulp of
    the largest term max|h| / pitch; measured on the host build: 0 (printed)."""
    rng = np.random.default_rng(2)
    nw, nu, du, dw = 9, 11, 0.0125, 0.004
    worst = 0.0
    for _ in range(50):
        tab = 1e-9 * rng.standard_normal((nw, nu))
        i, j = int(rng.integers(1, nu - 3)), int(rng.integers(1, nw - 3))
        tw = float(rng.uniform(0, 1))
        tu = float(rng.uniform(0, 1))
        rows, cols = np.arange(j - 1, j + 3), np.arange(i - 1, i + 3)
        # along u: cell i at t = 1 against cell i + 1 at t = 0, the same rows and fraction in w
        a = FS.host_gradient(tab[np.ix_(rows, cols)].reshape(1, 16), 1.0, tw, du, dw)
        b = FS.host_gradient(tab[np.ix_(rows, cols + 1)].reshape(1, 16), 0.0, tw, du, dw)
        # along w likewise
        c = FS.host_gradient(tab[np.ix_(rows, cols)].reshape(1, 16), tu, 1.0, du, dw)
        d = FS.host_gradient(tab[np.ix_(rows + 1, cols)].reshape(1, 16), tu, 0.0, du, dw)
        hmax = np.abs(tab).max()
        for (p, q) in ((a, b), (c, d)):
            for k, pitch in ((0, du), (1, dw)):
                diff = abs(p[k][0] - q[k][0])
                worst = max(worst, diff / np.spacing(hmax / pitch))
                assert diff <= 4 * np.spacing(hmax / pitch)
    print(f"gradient across a cell border: worst difference {worst:.3f} ulp of max|h| / pitch")


def _horner(t):
    """the header's weights and derivative weights at t with a first-order bound on each one's rounding
    error in units of u, propagated along its own Horner form: every rounded operation adds u |result|,
    a product with t scales the error carried so far by t; 0.5 t is exact. Returns (c, ec, d, ed)."""
    def mul_t(v, e, exact=False):
        return v * t, e * t + (0.0 if exact else abs(v * t))

    def add(v, e, k):
        return v + k, e + abs(v + k)

    def run(k0, steps):
        v, e = mul_t(k0, 0.0, exact=abs(k0) == 0.5)
        for st in steps:
            v, e = mul_t(v, e) if st is None else add(v, e, st)
        return v, e
    c = [run(-0.5, [1.0, None, -0.5, None]), run(1.5, [-2.5, None, None, 1.0]), run(-1.5, [2.0, None, 0.5, None]),
         run(0.5, [-0.5, None, None])]
    d = [run(-1.5, [2.0, None, -0.5]), run(4.5, [-5.0, None]), run(-4.5, [4.0, None, 0.5]), run(1.5, [-1.0, None])]
    return (np.array([v for v, _ in c]), np.array([e for _, e in c]), np.array([v for v, _ in d]),
            np.array([e for _, e in d]))


def _path_bound(a, ea, b, eb, H, eH, pitch):
    """first-order rounding bound (units of u) of (((b0 R0 + b1 R1) + b2 R2) + b3 R3) / pitch with
    R_j = ((a0 H_j0 + a1 H_j1) + a2 H_j2) + a3 H_j3 along the header's own sum path: the weights' errors
    ea, eb and the samples' eH enter through the products, every product and every partial sum adds
    u |its value|, the division u |the result|"""
    rows, erows = np.empty(4), np.empty(4)
    for j in range(4):
        p = a * H[j]
        e = ea * np.abs(H[j]) + np.abs(a) * eH[j] + np.abs(p)
        s1 = p[0] + p[1]
        s2 = s1 + p[2]
        s3 = s2 + p[3]
        rows[j], erows[j] = s3, e.sum() + abs(s1) + abs(s2) + abs(s3)
    p = b * rows
    e = eb * np.abs(rows) + np.abs(b) * erows + np.abs(p)
    s1 = p[0] + p[1]
    s2 = s1 + p[2]
    s3 = s2 + p[3]
    return (e.sum() + abs(s1) + abs(s2) + abs(s3)) / pitch + abs(s3 / pitch)


@pytest.mark.parametrize("nw,nu", [(7, 5), (4, 4), (6, 9)])
def test_linear_ramp_gradient(nw, nu):
    """h = s u + r w sampled on the grid: Catmull-Rom reproduces it, so at interior points (one cell
    from every edge, where no index is clamped) hu = s and hw = r whatever the fractions - the
    coordinates' rounding does not enter. What remains is rounding along the sixteen-term sum, bounded
    point by point (_path_bound) from each weight's own Horner form at that point's fractions (_horner)
    and the table's own rounding (U_i = u0 + i du, s U_i, r W_j and their sum: at most
    4 u (|s U_i| + |r W_j|) per sample), times 1.01 for the second-order terms. The weights' errors act
    on samples of size Hmax without cancelling, so the bound is 10 to 40 u Hmax / pitch (printed beside
    what the host build gives); test_dyadic_ramp_is_exact below is the sharp check of the low bits."""
    rng = np.random.default_rng(10 * nw + nu)
    q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    s, r = 3e-7, -2e-7
    u0, du, w0, dw = -0.03, 0.0125, 0.002, 0.004
    Ug, Wg = u0 + du * np.arange(nu), w0 + dw * np.arange(nw)
    fm = FigureMap(s * Ug[None, :] + r * Wg[:, None], u0, du, w0, dw, (0.5, -0.25, 146.0), q[:, 0], q[:, 1])
    eH = 4.0 * (np.abs(s * Ug)[None, :] + np.abs(r * Wg)[:, None])
    m = 200
    # fractions away from the cell borders, so that the header's cell is the one the bound is formed for
    su = rng.integers(1, nu - 2, m) + rng.uniform(0.01, 0.99, m)
    sw = rng.integers(1, nw - 2, m) + rng.uniform(0.01, 0.99, m)
    pts = (fm.origin.reshape(3, 1) + np.outer(fm.e_u, u0 + du * su) + np.outer(fm.e_w, w0 + dw * sw)
           + 1e-4 * np.cross(fm.e_u, fm.e_w).reshape(3, 1))
    hu, hw, out = FS.host_grad_at(fm, pts)
    hmax = np.abs(fm.height).max()
    assert not out.any()
    worst = [0.0, 0.0, 0.0, 0.0]
    for k in range(m):
        i, j = int(np.floor(su[k])), int(np.floor(sw[k]))
        cu, ecu, dcu, edu = _horner(su[k] - i)
        cw, ecw, dcw, edw = _horner(sw[k] - j)
        H, e = fm.height[j - 1:j + 3, i - 1:i + 3], eH[j - 1:j + 3, i - 1:i + 3]
        bu = 1.01 * U * _path_bound(dcu, edu, cw, ecw, H, e, du)
        # hw: the rows combined with the plain weights in u, then the derivative weights in w
        bw = 1.01 * U * _path_bound(cu, ecu, dcw, edw, H, e, dw)
        assert abs(hu[k] - s) <= bu and abs(hw[k] - r) <= bw, (k, abs(hu[k] - s) / bu, abs(hw[k] - r) / bw)
        worst = [max(worst[0], abs(hu[k] - s) / (U * hmax / du)), max(worst[1], bu / (U * hmax / du)),
                 max(worst[2], abs(hw[k] - r) / (U * hmax / dw)), max(worst[3], bw / (U * hmax / dw))]
    print(f"ramp, in u Hmax / pitch: |hu - s| {worst[0]:.1f} (largest bound {worst[1]:.1f}), "
          f"|hw - r| {worst[2]:.1f} (largest bound {worst[3]:.1f})")


def test_dyadic_ramp_is_exact():
    """a ramp whose every operation is exact: axes along x and y, a power-of-two grid, heights that are
    small integers times 2^-23 and fractions k / 8. The weights' Horner forms, the sixteen products, their
    sums and the division by the pitch then round nowhere, so hu == s and hw == r to the last bit - one
    wrong low bit in a derivative weight would show."""
    nw, nu = 7, 9
    s, r = 2.0**-20, -3 * 2.0**-22
    u0, du, w0, dw = -1.0, 0.5, 2.0, 0.25
    Ug, Wg = u0 + du * np.arange(nu), w0 + dw * np.arange(nw)
    fm = FigureMap(s * Ug[None, :] + r * Wg[:, None], u0, du, w0, dw, (0, 0, 0), (1, 0, 0), (0, 1, 0))
    fu, fw = np.meshgrid(np.arange(8 * 1, 8 * (nu - 2) + 1) / 8.0, np.arange(8 * 1, 8 * (nw - 2) + 1) / 8.0)
    pts = np.array([u0 + du * fu.ravel(), w0 + dw * fw.ravel(), np.zeros(fu.size)])
    hu, hw, out = FS.host_grad_at(fm, pts)
    assert not out.any()
    assert np.all(hu == s) and np.all(hw == r)


def test_degenerate_tables_outside_and_nan():
    rng = np.random.default_rng(3)
    g = _geom()
    c = g.mirrors[0].coeffs
    for nw, nu in ((1, 9), (9, 1)):
        fm = FigureMap(1e-9 * rng.standard_normal((nw, nu)), -0.04, 0.01, -0.04, 0.01, (0, 0, 0), (1, 0, 0), (0, 1, 0))
        pts = np.array([rng.uniform(-0.03, 0.03, 20), rng.uniform(-0.03, 0.03, 20), np.zeros(20)])
        hu, hw, out = FS.host_grad_at(fm, pts)
        flat = hw if nw == 1 else hu
        other = hu if nw == 1 else hw
        assert not out.any()
        assert np.all(flat == 0.0) and not np.signbit(flat).any()  # exactly +0 along the one-sample axis
        assert np.abs(other).max() > 0
    fm = FigureMap(1e-9 * rng.standard_normal((7, 5)), -0.02, 0.01, -0.03, 0.01, (0, 0, 0), (1, 0, 0), (0, 1, 0))
    outside = np.array([[-0.03, 0.0, 0.0], [0.021, 0.0, 0.0], [0.0, -0.031, 0.0], [0.0, 0.0301, 0.0]]).T
    hu, hw, out = FS.host_grad_at(fm, outside)
    assert out.all()
    for a in (hu, hw):
        assert np.all(a == 0.0) and not np.signbit(a).any()
    # through the stage loop: an outside hit keeps the quadric's unit normal and sets the flag ...
    fr = mirror_frames(g)[0]
    hit, d, N = _centre_ray(g)[0]
    ramp = FigureMap(1e-6 * (-0.02 + 0.01 * np.arange(5))[None, :] * np.ones((5, 1)), -0.02, 0.01, -0.02, 0.01,
                     fr["origin"], fr["e_u"], fr["e_w"])
    far = (hit + 0.05 * fr["e_u"]).reshape(3, 1)
    nrm, fl = FS.host_stage(ramp, c, far, d.reshape(3, 1))
    grad = np.array([2 * c[0] * far[0] + c[3] * far[1] + c[4] * far[2] + c[6],
                     2 * c[1] * far[1] + c[3] * far[0] + c[5] * far[2] + c[7],
                     2 * c[2] * far[2] + c[4] * far[0] + c[5] * far[1] + c[8]])
    assert fl == 8 and np.array_equal(nrm, grad / np.sqrt(grad[0]**2 + grad[1]**2 + grad[2]**2))
    # ... and a NaN hit gives a NaN normal and no flag
    nrm, fl = FS.host_stage(ramp, c, np.full((3, 1), np.nan), d.reshape(3, 1))
    assert fl == 0 and np.isnan(nrm).all()
    # inside, with a zero map: still normalised, a unit vector equal to N to an ulp
    zero = FigureMap(np.zeros((5, 5)), -0.02, 0.01, -0.02, 0.01, fr["origin"], fr["e_u"], fr["e_w"])
    nrm, fl = FS.host_stage(zero, c, hit.reshape(3, 1), d.reshape(3, 1))
    assert fl == 0 and np.abs(nrm[:, 0] - N).max() <= 2 * np.spacing(1.0)


def _last_mirror_case(s, axis, negate):
    """the centre ray at the last mirror of the AKB fixture with the ramp h = s u (axis 'u') or h = s w
    on it: (exit direction without map, exit direction with it, the frame, d, N)"""
    g = _geom()
    k = len(g.mirrors) - 1
    fr = mirror_frames(g)[k]
    hit, d, N = _centre_ray(g)[k]
    x = -0.02 + 0.01 * np.arange(5)
    tab = s * (x[None, :] * np.ones((5, 1)) if axis == "u" else x[:, None] * np.ones((1, 5)))
    fm = FigureMap(tab, -0.02, 0.01, -0.02, 0.01, fr["origin"], fr["e_u"], fr["e_w"])
    c = np.array(g.mirrors[k].coeffs) * (-1.0 if negate else 1.0)
    n1, fl = FS.host_stage(fm, c, hit.reshape(3, 1), d.reshape(3, 1))
    assert fl == 0
    n1 = n1[:, 0]

    def reflect(n):
        A = (d[0] * n[0] + d[1] * n[1]) + d[2] * n[2]
        r = d - (2.0 * A) * n
        return r / np.sqrt((r[0] * r[0] + r[1] * r[1]) + r[2] * r[2])
    n0 = -N if negate else N
    return reflect(n0), reflect(n1), fr, d, N


@pytest.mark.parametrize("negate", [False, True])
def test_in_plane_ramp_turns_the_exit_ray_by_twice_the_slope_angle(negate):
    """h = s u with e_u in the plane of incidence turns the beam-facing normal by atan(s) in that plane
    (n' ~ n - s e_u), the exit ray by 2 atan(s). Margin: relative 1e-6 = 2e-12 rad for s = 1e-6 (the
    direction components round at about 1e-15; e_u . N is zero only to the last bit)."""
    s = 1e-6
    r0, r1, fr, d, N = _last_mirror_case(s, "u", negate)
    ang = np.arctan2(np.linalg.norm(np.cross(r0, r1)), r0 @ r1)
    print(f"in-plane ramp: angle {ang:.15e}, 2 atan(s) {2 * np.arctan(s):.15e}")
    assert abs(ang - 2 * np.arctan(s)) <= 1e-6 * 2 * np.arctan(s)
    # the rotation stays in the plane of incidence
    assert abs((r1 - r0) @ fr["e_w"]) <= 1e-6 * 2 * s
    # sign: the surface rises along +e_u (downstream), its beam-facing normal tips back towards -e_u,
    # the local grazing angle grows and the exit ray leaves more steeply: it gains along the normal
    assert (r1 - r0) @ fr["normal"] > 0


@pytest.mark.parametrize("negate", [False, True])
def test_sideways_ramp_chord(negate):
    """h = s w: with d . e_w = 0, N' = (n - s e_w) / sqrt(1 + s^2) and ||r' - r|| = 2 |d . N| s / sqrt(1 + s^2)"""
    s = 1e-6
    r0, r1, fr, d, N = _last_mirror_case(s, "w", negate)
    chord = np.linalg.norm(r1 - r0)
    want = 2 * abs(d @ N) * s / np.sqrt(1 + s * s)
    print(f"sideways ramp: chord {chord:.15e}, closed form {want:.15e}")
    assert abs(chord - want) <= 1e-6 * want
    # the surface rises along +e_w: the beam-facing normal tips to -e_w, and so does the exit ray
    assert (r1 - r0) @ fr["e_w"] < 0


@pytest.mark.parametrize("axis", ["u", "w"])
def test_gradient_sign_of_the_quadric_does_not_matter(axis):
    """the ten coefficients negated: N and sigma both flip, N' flips exactly, and the reflection is even
    in the normal - the exit directions are the same to the last bit"""
    a = _last_mirror_case(1e-6, axis, False)
    b = _last_mirror_case(1e-6, axis, True)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_stand_alone_program_runs_clean(tmp_path):
    """tests/figure_slope_main.cpp as a plain host program (its header says how to build it under
    AddressSanitizer and UBSan, which is how it is meant to be run by hand)"""
    exe = str(tmp_path / "figure_slope")
    subprocess.run(["g++", "-O1", "-ffp-contract=off", "-I", os.path.join(ROOT, "akbraytracing_amd", "csrc"),
                    os.path.join(ROOT, "tests", "figure_slope_main.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 failures" in r.stdout


def test_abi_and_descriptor_field():
    import ctypes
    import re
    from akbraytracing_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "akb_raytrace.h")).read()
    # the number stays where tests/test_figure_cpu.py pins it; the layout is guarded by akb_chain_desc_size
    assert int(re.search(r"#define AKB_ABI_VERSION (\d+)", hdr).group(1)) == _lib.ABI_VERSION
    assert "akb_figure_normal_f64" in _lib.EXPORTS and "akb_figure_normal_f64" in hdr
    # appended: every earlier field keeps its offset
    assert _lib.ChainDesc._fields_[-1][0] == "fig_slope"
    assert _lib.ChainDesc.fig_slope.offset == _lib.ChainDesc.fig_out.offset + ctypes.sizeof(ctypes.c_void_p)
