"""csrc/akb_figure.h and akbraytracing_amd/figure.py without a GPU: a g++ build of the header
against an exact rational restatement of the model, the exact cases, the index contract,
FigureMap's validation and readers, mirror_frames, and the ABI."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import figure_host as FH
from conftest import GOLDEN, ROOT, golden_json

from akbraytracing_amd.figure import FigureMap, check_figure, mirror_frames, outside_error

SHAPES = [(4, 4), (7, 5), (1, 9), (9, 1)]  # (nw, nu)


def _rot(rng):
    """a random orthonormal pair (e_u, e_w), unit and orthogonal to a few ulp"""
    q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    return q[:, 0], q[:, 1]


def _map(rng, nw, nu, axes=None, origin=None, height=None):
    eu, ew = axes if axes is not None else _rot(rng)
    h = 1e-9 * rng.standard_normal((nw, nu)) if height is None else height
    origin = rng.uniform(-2.0, 150.0, 3) if origin is None else origin
    return FigureMap(h, -0.03, 0.0125, 0.002, 0.004, origin, eu, ew)


def _points(fm, su, sw, off_plane=0.0):
    """lab points at grid coordinates (su, sw) (in pitches from u0 / w0)"""
    u = fm.u0 + fm.du * np.asarray(su)
    w = fm.w0 + fm.dw * np.asarray(sw)
    n = np.cross(fm.e_u, fm.e_w)
    return fm.origin.reshape(3, 1) + np.outer(fm.e_u, u) + np.outer(fm.e_w, w) + off_plane * n.reshape(3, 1)


@pytest.mark.parametrize("nw,nu", SHAPES)
def test_host_build_matches_exact_restatement(nw, nu):
    """random interior points in a random frame: |header - exact| within figure_host.error_bound
    (derived there from the operation count and sum |w_i w_j h_ij|, no fitted number)"""
    rng = np.random.default_rng(100 * nw + nu)
    fm = _map(rng, nw, nu)
    m = 200
    su = rng.uniform(0.02, max(nu - 1, 1) - 0.02, m) if nu > 1 else rng.uniform(-5, 5, m)
    sw = rng.uniform(0.02, max(nw - 1, 1) - 0.02, m) if nw > 1 else rng.uniform(-5, 5, m)
    pts = _points(fm, su, sw, off_plane=1e-4)
    dn = rng.uniform(-0.2, 0.2, m)
    got, h, off, out = FH.host_eval(fm, pts, dn)
    want, hx, outx, S = FH.exact_eval(fm, pts, dn)
    assert not out.any() and not outx.any()
    assert off.min() >= 0 and off.max() < nw * nu
    err = np.abs(got - want)
    bound = FH.error_bound(fm, pts, dn, S)
    assert np.all(err <= bound), (err.max(), bound[np.argmax(err / bound)])
    # the bound is a rounding bound, not a loose one: far below the heights themselves
    assert bound.max() < 1e-6 * np.abs(fm.height).max()


@pytest.mark.parametrize("nw,nu", SHAPES)
def test_host_build_edges_exact_frame(nw, nu):
    """edge and near-edge points in a frame whose coordinates are exact (axes along x and y, power-of-two
    grid): both evaluations classify every point alike, including the points on the map's border"""
    rng = np.random.default_rng(7 * nw + nu)
    fm = FigureMap(1e-9 * rng.standard_normal((nw, nu)), -1.0, 0.5, 2.0, 0.25, (0, 0, 0), (1, 0, 0), (0, 1, 0))
    eu = [0.0, 2.0**-20, 0.5, nu - 1 - 2.0**-20, float(nu - 1)] if nu > 1 else [0.0, 3.0]
    ew = [0.0, 2.0**-20, 0.5, nw - 1 - 2.0**-20, float(nw - 1)] if nw > 1 else [0.0, -2.0]
    su, sw = [a.ravel() for a in np.meshgrid(eu, ew)]
    pts = _points(fm, su, sw)
    dn = np.full(su.size, 0.16)
    got, h, off, out = FH.host_eval(fm, pts, dn)
    want, hx, outx, S = FH.exact_eval(fm, pts, dn)
    assert not out.any() and not outx.any()
    assert off.min() >= 0 and off.max() < nw * nu
    assert np.all(np.abs(got - want) <= FH.error_bound(fm, pts, dn, S))
    # at a sample the interpolant returns the sample (weights 0, 1, 0, 0)
    if nu > 1 and nw > 1:
        k = (su == 0.0) & (sw == 0.0)
        assert h[k][0] == fm.height[0, 0]


def test_constant_map_is_constant_times_path_factor():
    """the weights sum to one: a constant map returns c * (-2 |d . n|) to the same bound"""
    rng = np.random.default_rng(5)
    c = 3.25e-9
    fm = _map(rng, 6, 8, height=np.full((6, 8), c))
    m = 300
    pts = _points(fm, rng.uniform(0, 7, m), rng.uniform(0, 5, m))
    dn = rng.uniform(-0.2, 0.2, m)
    got, h, off, out = FH.host_eval(fm, pts, dn)
    want = -2.0 * c * np.abs(dn)
    S = np.full(m, 1.25 * 1.25 * c)  # sum |w_i w_j| <= (5/4)^2
    assert not out.any()
    assert np.all(np.abs(got - want) <= FH.error_bound(fm, pts, dn, S))


def test_quadratic_map_reproduced_where_no_clamping():
    """Catmull-Rom reproduces quadratics: a map sampled from a + b u + c w + e u^2 + f u w + g w^2
    is returned at points whose 4 x 4 support lies inside the table"""
    rng = np.random.default_rng(11)
    nw, nu = 9, 10
    a, b, c, e, f, g = 1e-9 * rng.standard_normal(6)
    eu, ew = _rot(rng)
    proto = FigureMap(np.zeros((nw, nu)), -0.03, 0.0125, 0.002, 0.004, (0.5, -0.25, 146.0), eu, ew)
    U = proto.u0 + proto.du * np.arange(nu)
    W = proto.w0 + proto.dw * np.arange(nw)

    def q(u, w):
        return a + b * u + c * w + e * u * u + f * u * w + g * w * w
    fm = FigureMap(q(U[None, :], W[:, None]), proto.u0, proto.du, proto.w0, proto.dw, proto.origin, eu, ew)
    m = 300
    su, sw = rng.uniform(1.0, nu - 2.0, m), rng.uniform(1.0, nw - 2.0, m)
    pts = _points(fm, su, sw)
    dn = np.full(m, 0.17)
    got, h, off, out = FH.host_eval(fm, pts, dn)
    want_h = q(fm.u0 + fm.du * su, fm.w0 + fm.dw * sw)
    want, hx, outx, S = FH.exact_eval(fm, pts, dn)
    assert not out.any()
    # the exact interpolant equals the quadratic up to the table's own rounding (one ulp per sample,
    # weighted by sum |w_i w_j| <= 25/16) and the rounding of want_h's own evaluation (a few ulp of
    # its largest term), and the points themselves are origin + e_u u + e_w w rounded three times per
    # component (at most 3 u max|P| each, under 6 u max|P| along a unit axis; 8 taken), which moves
    # the quadratic by at most its gradient times that
    Um, Wm = np.abs(U).max(), np.abs(W).max()
    scale = np.abs([a, b * Um, c * Wm, e * Um**2, f * Um * Wm, g * Wm**2]).max()
    grad = abs(b) + 2 * abs(e) * Um + abs(f) * Wm + abs(c) + 2 * abs(g) * Wm + abs(f) * Um
    pos = 8 * FH.EPS * np.abs(pts).max()
    assert np.all(np.abs(hx - want_h) <= 64 * FH.EPS * scale + 1.6 * FH.EPS * np.abs(fm.height).max() + grad * pos)
    assert np.all(np.abs(got - want) <= FH.error_bound(fm, pts, dn, S))


@pytest.mark.parametrize("nw,nu", SHAPES)
def test_index_contract(nw, nu):
    """NaN, +-inf, +-1e300 and one pitch outside each edge: flag, zero or NaN as specified, and
    every reported table offset inside the table"""
    tab = 1e-9 * (np.arange(nw * nu, dtype=np.float64) + 1).reshape(nw, nu)
    fm = FigureMap(tab, -1.0, 0.5, 2.0, 0.25, (0, 0, 0), (1, 0, 0), (0, 1, 0))
    u_in, w_in = fm.u0 + 0.5 * fm.du * (nu - 1), fm.w0 + 0.5 * fm.dw * (nw - 1)
    us = [np.nan, np.inf, -np.inf, 1e300, -1e300, fm.u0 - fm.du, fm.u0 + fm.du * nu, fm.u0, fm.u0 + fm.du * (nu - 1), u_in]
    ws = [np.nan, np.inf, -np.inf, 1e300, -1e300, fm.w0 - fm.dw, fm.w0 + fm.dw * nw, fm.w0, fm.w0 + fm.dw * (nw - 1), w_in]
    u, w = [a.ravel() for a in np.meshgrid(us, ws)]
    pts = np.stack([u, w, np.zeros_like(u)])
    with np.errstate(invalid="ignore"):
        d, h, off, out = FH.host_eval(fm, pts, 0.25)
        # the map coordinates are the frame's dot products: an infinite or NaN lab coordinate reaches
        # both (inf * 0 is NaN), so the expectation is formed from them, not from the lab point
        u, w = (u * 1.0 + w * 0.0) + 0.0 * 0.0, (u * 0.0 + w * 1.0) + 0.0 * 0.0
        out_u = (nu > 1) & ((u < fm.u0) | (u > fm.u0 + fm.du * (nu - 1)))
        out_w = (nw > 1) & ((w < fm.w0) | (w > fm.w0 + fm.dw * (nw - 1)))
    assert off.min() >= 0 and off.max() < nw * nu
    outside = out_u | out_w
    assert np.array_equal(out, outside)
    assert np.all(h[outside] == 0.0) and np.all(d[outside] == 0.0)
    nan_in = ~outside & (((nu > 1) & np.isnan(u)) | ((nw > 1) & np.isnan(w)))
    assert np.all(np.isnan(h[nan_in])) and np.all(np.isnan(d[nan_in]))
    # a NaN coordinate selects index 0 on its axis (offsets 4 j + i: the base sample is i = 1, j = 1)
    if nu > 1:
        assert np.all(off[np.isnan(u), 5] % nu == 0)
    if nw > 1:
        assert np.all(off[np.isnan(w), 5] // nu == 0)
    ok = ~outside & ~nan_in
    assert ok.any() and np.all(h[ok] > 0.0) and np.all(d[ok] < 0.0)


def test_index_contract_standalone_program(tmp_path):
    """the same case as a stand-alone C++ program (tests/figure_index_main.cpp; its header says how to
    build it with the host sanitizers): built plainly here, it checks itself"""
    exe = tmp_path / "figure_index"
    subprocess.run(["g++", "-O1", "-ffp-contract=off", "-I", FH.CSRC, os.path.join(ROOT, "tests", "figure_index_main.cpp"),
                    "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "400 evaluations, 0 failures" in r.stdout


def test_accumulate_order_on_host():
    """the stage loop: the first term is 0 + delta, later terms add to the row"""
    rng = np.random.default_rng(3)
    fm = FigureMap(1e-9 * rng.standard_normal((5, 6)), -1.0, 0.5, 2.0, 0.25, (0, 0, 0), (1, 0, 0), (0, 1, 0))
    coeffs = [0, 0, 0, 0, 0, 0, 0, 0, 1.0, 0]  # the plane z = 0, normal (0, 0, 1)
    hit = np.stack([rng.uniform(-1, 1.5, 50), rng.uniform(2, 3, 50), np.zeros(50)])
    dirs = np.stack([np.full(50, np.cos(0.16)), np.zeros(50), np.full(50, -np.sin(0.16))])
    one, fl = FH.host_stage(fm, coeffs, hit, dirs)
    d, h, _, _ = FH.host_eval(fm, hit, np.sin(0.16))
    assert fl == 0 and np.array_equal(one, 0.0 + d)
    two, _ = FH.host_stage(fm, coeffs, hit, dirs, out=one)
    assert np.array_equal(two, one + d)
    # positive h is a bump towards the beam whatever the gradient's sign: the flipped plane gives the same
    flipped, _ = FH.host_stage(fm, [-c for c in coeffs], hit, dirs)
    assert np.array_equal(flipped, one)
    hit[0, 0] = 10.0
    _, fl = FH.host_stage(fm, coeffs, hit, dirs)
    assert fl == 8


# ---- FigureMap --------------------------------------------------------------------------------

def test_figuremap_validation():
    ok = dict(u0=0.0, du=1.0, w0=0.0, dw=1.0, origin=(0, 0, 0), e_u=(1, 0, 0), e_w=(0, 1, 0))
    FigureMap(np.zeros((3, 4)), **ok)
    assert FigureMap(np.zeros(5), **ok).height.shape == (1, 5)
    for bad in (np.nan, np.inf):
        h = np.zeros((3, 4))
        h[1, 2] = bad
        with pytest.raises(ValueError, match="finite"):
            FigureMap(h, **ok)
    with pytest.raises(ValueError, match="unit"):
        FigureMap(np.zeros((3, 4)), **dict(ok, e_u=(1.0 + 1e-9, 0, 0)))
    with pytest.raises(ValueError, match="orthogonal"):
        FigureMap(np.zeros((3, 4)), **dict(ok, e_w=(1e-9, np.sqrt(1 - 1e-18), 0)))
    for k in ("du", "dw"):
        for v in (0.0, -1.0, np.nan):
            with pytest.raises(ValueError, match="pitch"):
                FigureMap(np.zeros((3, 4)), **dict(ok, **{k: v}))
    with pytest.raises(ValueError):
        FigureMap(np.zeros((2, 3, 4)), **ok)
    assert check_figure(None, 4) is None and check_figure([None] * 4, 4) is None
    with pytest.raises(ValueError, match="per mirror"):
        check_figure([None] * 3, 4)
    with pytest.raises(ValueError):
        check_figure([1.0, None], 2)
    assert outside_error(0x7) is None
    assert "mirror 2" in outside_error(0x8 << 8) and "mirror 0, 3" in outside_error(0x8008)


def test_from_profile_and_csv():
    frame = dict(origin=(0.0, 0.0, 0.0), e_u=(0, 1, 0), e_w=(0, 0, 1))
    fm = FigureMap.from_csv(os.path.join(GOLDEN, "figure_profile.csv"), frame)
    raw = np.loadtxt(os.path.join(GOLDEN, "figure_profile.csv"), delimiter=",", skiprows=1)
    assert (fm.nw, fm.nu) == (1, 21)
    assert fm.u0 == raw[0, 0] * 1e-3 and fm.du == pytest.approx(5e-3, rel=1e-15)
    assert np.array_equal(fm.height[0], raw[:, 1] * 1e-3)
    # constant along e_w, the profile along e_u: the samples come back at the sample points
    # (at the CSV's own abscissae; s = (u - u0) / du is an integer to a few ulp of 20, and the
    # interpolant's slope is at most 3 Hmax per pitch: 1e-12 Hmax leaves two decades)
    pts = np.stack([np.zeros(21), raw[:, 0] * 1e-3, np.linspace(-40, 40, 21)])
    d, h, off, out = FH.host_eval(fm, pts, 1.0)
    assert not out.any() and h[0] == fm.height[0, 0]
    assert np.max(np.abs(h - fm.height[0])) <= 1e-12 * np.abs(fm.height).max()
    with pytest.raises(ValueError, match="equally spaced"):
        FigureMap.from_profile([0.0, 1.0, 3.0], [0, 0, 0], frame)
    with pytest.raises(ValueError, match="equally spaced"):
        FigureMap.from_profile([2.0, 1.0, 0.0], [0, 0, 0], frame)


@pytest.mark.parametrize("name,K", [("akb_geometry.json", 4), ("kb_geometry.json", 2)])
def test_mirror_frames(name, K):
    from akbraytracing_amd.wavefront import SystemGeometry
    g = SystemGeometry.from_dict(golden_json(name))
    frames = mirror_frames(g)
    assert len(frames) == K
    for fr, m in zip(frames, g.mirrors):
        eu, ew, n = fr["e_u"], fr["e_w"], fr["normal"]
        for v in (eu, ew, n):
            assert abs(v @ v - 1.0) <= 1e-15
        assert abs(eu @ ew) <= 1e-15 and abs(eu @ n) <= 1e-15 and abs(ew @ n) <= 1e-15
        assert np.max(np.abs(np.cross(n, eu) - ew)) <= 1e-15
        x, y, z = fr["origin"]
        a, b, c, d, e, f, gg, h, i, j = m.coeffs
        terms = [a * x * x, b * y * y, c * z * z, d * x * y, e * x * z, f * y * z, gg * x, h * y, i * z, j]
        # on the quadric to the rounding of its own ten terms
        assert abs(sum(terms)) <= 64 * FH.EPS * max(abs(t) for t in terms)
        assert 0.0 < fr["grazing"] < 0.5
        FigureMap(np.zeros((2, 2)), 0, 1, 0, 1, fr["origin"], eu, ew)  # passes the axis validation
    # e_u follows the beam: the next mirror lies downstream along it
    assert (frames[1]["origin"] - frames[0]["origin"]) @ frames[0]["e_u"] > 0


def test_abi_layout():
    from akbraytracing_amd import _lib
    L = _lib.lib()
    assert L.akb_abi_version() == _lib.ABI_VERSION == 19
    assert L.akb_chain_desc_size() == ctypes.sizeof(_lib.ChainDesc)
    assert ctypes.sizeof(_lib.FigureMapDesc) == 8 + 9 * 8 + 4 * 8 + 8
    assert _lib.ChainDesc.fig.size == 7 * ctypes.sizeof(_lib.FigureMapDesc)
    assert hasattr(L, "akb_figure_opl_f64")
