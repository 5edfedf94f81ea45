"""Figure maps in the wave chain without a GPU: csrc/akb_figure.h's displace in a g++ build
(figure_wave_host.py) against a step-by-step rational evaluation, its value rules, its consistency with
the thin screen's path term on the recorded 'wave' file sets, the stand-alone program, and
figure.sampling with the warning saveWaveData draws from it."""
import os
import subprocess
import warnings
from fractions import Fraction

import numpy as np
import pytest

import figure_host as FH
import figure_wave_host as FW
from conftest import ROOT, golden, golden_json
from figure_maps import AMP, make_maps

from akbraytracing_amd.figure import FigureMap, _centre_ray, mirror_frames, sampling

SHAPES = [(4, 4), (7, 5), (1, 9), (9, 1)]  # (nw, nu)


def _geom():
    from akbraytracing_amd.wavefront import SystemGeometry
    return SystemGeometry.from_dict(golden_json("akb_geometry.json"))


def _F(x):
    return Fraction(float(x))


def _rn(q):
    """one rounding to float64 (Fraction -> float is correctly rounded), back as an exact rational"""
    return Fraction(float(q))


def _exact_displace(p, nrm, d, h):
    """the header's spelled-out expression, every operation exact in rationals and then rounded once:
    dn = (l nx + m ny) + n nz; sigma = dn > 0 ? -1 : 1; s = sigma h; x' = x + s nx (y, z likewise)"""
    out = np.empty_like(p)
    for i in range(p.shape[1]):
        N = [_F(v) for v in nrm[:, i]]
        l, m, n = (_F(v) for v in d[:, i])
        dn = _rn(_rn(_rn(l * N[0]) + _rn(m * N[1])) + _rn(n * N[2]))
        sigma = Fraction(-1) if dn > 0 else Fraction(1)
        s = _rn(sigma * _F(h[i]))
        for k in range(3):
            out[k, i] = float(_rn(_F(p[k, i]) + _rn(s * N[k])))
    return out


def _cloud(fm, fr, rng, n=60):
    """points over the map's interior, a little off the tangent plane"""
    lu, lw = fm.du * max(fm.nu - 1, 1), fm.dw * max(fm.nw - 1, 1)
    a = fm.u0 + lu * rng.uniform(0.02, 0.98, n)
    b = fm.w0 + lw * rng.uniform(0.02, 0.98, n)
    return (fr["origin"].reshape(3, 1) + np.outer(fr["e_u"], a) + np.outer(fr["e_w"], b)
            + np.outer(fr["normal"], 1e-5 * rng.standard_normal(n)))


def _map_on(fr, shape, rng, amp=1e-8, half=(0.04, 0.004)):
    nw, nu = shape
    du, dw = 2 * half[0] / max(nu - 1, 1), 2 * half[1] / max(nw - 1, 1)
    return FigureMap(amp * rng.standard_normal((nw, nu)), -half[0], du, -half[1], dw, fr["origin"], fr["e_u"], fr["e_w"])


@pytest.mark.parametrize("shape", SHAPES)
def test_displace_is_the_spelled_out_expression(shape):
    """the stage loop's points equal the rational evaluation rounded step by step, bit for bit, from the
    loop's own unit normals and heights (the height's own order is tests/test_figure_cpu.py's); h_out is
    the height eval() gives; and with the ten coefficients negated sigma and N both flip: the same points
    to the last bit"""
    rng = np.random.default_rng(100 * shape[0] + shape[1])
    g = _geom()
    frames = mirror_frames(g)
    moved = False
    for k, m in enumerate(g.mirrors):
        fr = frames[k]
        fm = _map_on(fr, shape, rng)
        pts = _cloud(fm, fr, rng)
        _, d, _ = _centre_ray(g)[k]
        # unnormalised directions of either sense and a spread of sizes: only the sign of d . N is read
        dirs = np.outer(d, rng.uniform(0.1, 30.0, pts.shape[1]) * rng.choice([-1.0, 1.0], pts.shape[1]))
        dirs += 1e-3 * rng.standard_normal(dirs.shape)
        c = np.array(m.coeffs)
        r = FW.host_stage(fm, c, pts, dirs)
        assert r["flags"] == 0 and not r["outside"].any()
        want = _exact_displace(pts, r["unit"], dirs, r["h"])
        assert np.array_equal(r["points"], want), k
        dn = (dirs[0] * r["unit"][0] + dirs[1] * r["unit"][1]) + dirs[2] * r["unit"][2]
        assert np.array_equal(FW.host_displace(pts, r["unit"], dn, r["h"]), want)
        _, h, _, _ = FH.host_eval(fm, pts, dn)
        assert np.array_equal(r["h"], h)
        moved = moved or np.any(r["points"] != pts)
        neg = FW.host_stage(fm, -c, pts, dirs)
        assert np.array_equal(neg["unit"], -r["unit"])
        assert np.array_equal(neg["points"], r["points"]) and np.array_equal(neg["h"], r["h"])
    assert moved


def test_value_rules():
    rng = np.random.default_rng(5)
    g = _geom()
    fr = mirror_frames(g)[0]
    hit, d, N = _centre_ray(g)[0]
    c = np.array(g.mirrors[0].coeffs)
    fm = _map_on(fr, (7, 5), rng)
    # outside: P bit for bit, h = +0, the flag; one pitch beyond each edge, -0.0 coordinates kept
    far = np.stack([hit + a * fr["e_u"] + b * fr["e_w"] for a, b in
                    ((-0.04 - fm.du, 0.0), (0.04 + fm.du, 0.0), (0.0, -0.004 - fm.dw), (0.0, 0.004 + fm.dw))], axis=1)
    r = FW.host_stage(fm, c, far, np.outer(d, np.ones(4)))
    assert r["flags"] == 8 and r["outside"].all()
    assert far.tobytes() == r["points"].tobytes()
    assert np.all(r["h"] == 0.0) and not np.signbit(r["h"]).any()
    z = np.array([[-0.0], [0.0], [-0.0]])
    out = FW.host_displace(z, np.array([[np.inf], [np.nan], [1.0]]), 1.0, 0.0, outside=[1])
    assert out.tobytes() == z.tobytes()  # a select, not P + 0 N
    # NaN: NaN, no flag
    r = FW.host_stage(fm, c, np.full((3, 2), np.nan), np.outer(d, np.ones(2)))
    assert r["flags"] == 0 and np.isnan(r["points"]).all() and np.isnan(r["h"]).all() and not r["outside"].any()
    # zero gradient: P, the flag
    flat = np.zeros(10)
    flat[9] = 1.0
    pts = _cloud(fm, fr, rng, 5)
    r = FW.host_stage(fm, flat, pts, np.outer(d, np.ones(5)))
    assert r["flags"] == 2 and pts.tobytes() == r["points"].tobytes()
    # a constant map: the step along the beam-facing normal is h0 to 4 ulp of the largest coordinate
    # (x' = RN(x + RN(s nx)): half an ulp of the coordinate per component, projected onto a unit vector
    # at most sqrt(3) / 2 ulp, plus the products' roundings at 1e-16 of h0 and ||N|| - 1 at 2e-16)
    for h0 in (1e-9, -3e-8, 1e-7):
        const = FigureMap(np.full((4, 4), h0), -0.04, 0.08 / 3, -0.004, 0.008 / 3, fr["origin"], fr["e_u"], fr["e_w"])
        pts = _cloud(const, fr, rng)
        for sense in (1.0, -1.0):
            r = FW.host_stage(const, c, pts, np.outer(sense * d, np.ones(pts.shape[1])))
            sigma = np.where((sense * d) @ r["unit"] > 0, -1.0, 1.0)
            step = ((r["points"] - pts) * (sigma * r["unit"])).sum(0)
            assert np.abs(r["h"] - h0).max() <= 8 * np.spacing(abs(h0))  # the weights sum to one to rounding
            assert np.abs(step - h0).max() <= 4 * np.spacing(np.abs(pts).max())
            # towards the incoming beam: against d for positive h
            assert np.all(np.sign(((r["points"] - pts) * (sense * d).reshape(3, 1)).sum(0)) == -np.sign(h0))


def _unit(v):
    return v / np.sqrt((v * v).sum(0))


def _len(v):
    v = v.astype(np.longdouble)
    return np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])


def _chains():
    """(name, [A, P, B, N or None]) per mirror of the two recorded 'wave' file sets, in the order the beam
    meets the mirrors. The KB set carries the reference's own normals and detector hits; the AKB set
    records neither, so there B of the last mirror is the image grid's centre and N the bisector of the
    two segments (what the reference forms for its *_norm arrays) - the identity below is geometry about
    any A, P, B whose normal bisects them."""
    kb = golden("kb_savewave_33.npz")
    src = kb["w_source"]
    out = [("kb M1", src, kb["w_vmirr_hyp"], kb["w_hmirr_hyp"], kb["w_vmirr_norm"]),
           ("kb M2", kb["w_vmirr_hyp"], kb["w_hmirr_hyp"], kb["w_detcenter"], kb["w_hmirr_norm"])]
    f = golden("savewave_33.npz")
    m = {k: f[f"plain_points_M{k}"][:3] for k in (1, 2, 3, 4)}
    focus = f["plain_points_gridImage"].mean(axis=1).reshape(3, 1)
    seq = [f["plain_points_source"].reshape(3, 1), m[1], m[3], m[4], m[2], focus]  # vhyp, vell, hell, hhyp
    for k in range(1, 5):
        out.append((f"akb trace {k - 1}", seq[k - 1], seq[k], seq[k + 1], None))
    return out


def _fixture_frame(P, d, N):
    """a mirror frame from the recorded samples, as figure.mirror_frames forms it from the centre ray"""
    c = P.shape[1] // 2
    n = -N[:, c] if d[:, c] @ N[:, c] > 0 else N[:, c]
    eu = d[:, c] - (d[:, c] @ n) * n
    eu = eu / np.linalg.norm(eu)
    ew = np.cross(n, eu)
    ew = ew / np.linalg.norm(ew)
    return dict(origin=P[:, c].copy(), e_u=eu, e_w=ew, normal=n)


def test_displaced_points_agree_with_the_thin_screen():
    """The test that pins the sign. A sample P between its previous point A and its next point B, moved to
    P' = P + sigma h N, changes the path A -> P -> B by the thin screen's term:

        (|P' - A| + |B - P'|) - (|P - A| + |B - P|) = -2 h |d . N| +- tol,  d = (P - A) / |P - A|.

    First order: the step s N (s = sigma h) changes the path by s N . (d - d') with d' the outgoing unit
    vector; N bisects, d . N = -d' . N, so the change is 2 s (d . N) = 2 sigma h (d . N) = -2 h |d . N| by
    sigma's rule. Second order: the step's component across each segment, at most |h|, lengthens that
    segment by at most h^2 / (2 length) - bounded with the factor 2 dropped, which also covers the third
    order: h_max^2 (1 / |P - A| + 1 / |B - P|). Rounding, with C = 146 m the largest coordinate: P' is
    rounded to half an ulp(C) per component, an error e that enters the two displaced lengths as
    e . d - e . d', at most sqrt(3) ulp(C). The lengths themselves are formed in np.longdouble, so
    on a platform with a wider long double that is all; where long double is double, each of the four
    lengths adds its coordinate differences (Sterbenz-exact between neighbouring mirrors, half an ulp(C)
    per component against the source: sqrt(3) / 2 for two of them), its sum of squares and root (at
    most 1.5 * 2^-53 relative: 0.9 ulp(C) at 146 m for the two source segments, nothing at a metre) and
    the two sums and the difference half an ulp each: sqrt(3) + sqrt(3) + 1.8 + 1.5 = 6.8. Both inside
    8 ulp(C). The term itself is 3e-10 to 4e-8 m.
    The worst case is printed: 7.4e-13 m against 1.7e-12 m, on the AKB set's short last segment at
    h = 1e-7 m, where the second-order term is the larger one."""
    worst = (0.0, 0.0, "")
    for name, A, P, B, N in _chains():
        d = _unit(P - A)
        if N is None:
            N = _unit((d - _unit(B - P)) / 2)
        dn = (d[0] * N[0] + d[1] * N[1]) + d[2] * N[2]
        n = P.shape[1]
        fr = _fixture_frame(P, d, N)
        maps = make_maps([fr] * 4, [P] * 4, SHAPES)
        heights = [(f"const {h0:g}", np.full(n, h0)) for h0 in (1e-9, 1e-8, 1e-7)]
        for fm in maps:
            _, h, _, outside = FH.host_eval(fm, P, dn)
            assert not outside.any() and np.abs(h).max() > 0.05 * AMP
            heights.append((f"map {fm.nw}x{fm.nu}", h))
        C = max(np.abs(A).max(), np.abs(P).max(), np.abs(B).max())
        L = np.longdouble
        a, b = _len(P.astype(L) - A), _len(B.astype(L) - P)
        for label, h in heights:
            Pd = FW.host_displace(P, N, dn, h)
            lhs = ((_len(Pd.astype(L) - A) + _len(B.astype(L) - Pd)) - (a + b)).astype(np.float64)
            rhs = -2.0 * h * np.abs(dn)
            tol = 8 * np.spacing(C) + np.abs(h).max()**2 * (1 / a + 1 / b).astype(np.float64)
            res = np.abs(lhs - rhs)
            i = int(np.argmax(res / tol))
            if res[i] / tol[i] > worst[0]:
                worst = (res[i] / tol[i], res[i], f"{name}, {label}: residual {res[i]:.2e} m, tol {tol[i]:.2e} m, "
                                                  f"term {abs(rhs[i]):.2e} m")
            assert np.all(res <= tol), (name, label, res[i], tol[i])
            assert np.abs(rhs).max() > 100 * tol.max()  # the term is resolved
    print("thin screen against displaced points, worst case:", worst[2])


def test_stand_alone_program_runs_clean(tmp_path):
    """tests/figure_displace_main.cpp as a plain host program (its header says how to build it under
    AddressSanitizer and UBSan, which is how it is meant to be run by hand)"""
    exe = str(tmp_path / "figure_displace")
    subprocess.run(["g++", "-O1", "-ffp-contract=off", "-I", os.path.join(ROOT, "akbraytracing_amd", "csrc"),
                    os.path.join(ROOT, "tests", "figure_displace_main.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 failures" in r.stdout


def _lattice(n_v, n_h, row, col, fm):
    """a sheared lattice in the map's plane: sample (j, i) at i row + j col, row and col given as (u, w)"""
    j, i = np.meshgrid(np.arange(n_v), np.arange(n_h), indexing="ij")
    u = (i * row[0] + j * col[0]).ravel()
    w = (i * row[1] + j * col[1]).ravel()
    return fm.origin.reshape(3, 1) + np.outer(fm.e_u, u) + np.outer(fm.e_w, w)


def test_sampling_and_the_aliasing_warning():
    """a sheared lattice with row step (3 mm, 0.1 mm) and column step (-1 mm, 0.4 mm) in (u, w): the
    largest neighbour spacing is 3 mm along e_u and 0.4 mm along e_w (to rounding at the lattice's
    size); saveWaveData's warning fires just above the pitch and stays silent just below it, and never
    for an axis with one map sample"""
    from akbraytracing_amd import wavedata as W
    rng = np.random.default_rng(9)
    q, _ = np.linalg.qr(rng.standard_normal((3, 3)))

    def fm_with(du, dw, shape=(5, 6)):
        return FigureMap(np.zeros(shape), -1.0, du, -1.0, dw, (0.5, -0.25, 146.0), q[:, 0], q[:, 1])

    fm = fm_with(1e-3, 1e-3)
    grid = _lattice(7, 9, (3e-3, 1e-4), (-1e-3, 4e-4), fm)
    s = sampling(fm, grid, 7, 9)
    assert abs(s["su"] - 3e-3) <= 1e-12 and abs(s["sw"] - 4e-4) <= 1e-12
    assert s["du"] == 1e-3 and s["dw"] == 1e-3
    # a (4, n) array as saved (the dS row is not read), and a single row
    assert sampling(fm, np.vstack([grid, np.ones((1, 63))]), 7, 9) == s
    one = sampling(fm, grid[:, :9], 1, 9)
    assert abs(one["su"] - 3e-3) <= 1e-12 and abs(one["sw"] - 1e-4) <= 1e-12
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        W._warn_sampling(2, 4, fm_with(3.001e-3, 4.001e-4), (grid, 7, 9))  # both pitches above the spacing
        W._warn_sampling(2, 4, fm_with(1e-6, 4.001e-4, shape=(5, 1)), (grid, 7, 9))  # one sample along u
    with pytest.warns(UserWarning, match=r"mirror 2 \(points_M4\.npy\).*3\.000e-03 m along e_u.*2\.999e-03") as rec:
        W._warn_sampling(2, 4, fm_with(2.999e-3, 4.001e-4), (grid, 7, 9))
    assert len(rec) == 1 and "e_w" not in str(rec[0].message)
    with pytest.warns(UserWarning, match=r"e_u.*and.*4\.000e-04 m along e_w.*3\.999e-04") as rec:
        W._warn_sampling(0, 1, fm_with(2.999e-3, 3.999e-4), (grid, 7, 9))
    assert len(rec) == 1  # one warning per mirror, both axes in it


def test_abi_and_entry_point():
    import re
    from akbraytracing_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "akb_raytrace.h")).read()
    assert int(re.search(r"#define AKB_ABI_VERSION (\d+)", hdr).group(1)) == _lib.ABI_VERSION == 19
    assert "akb_figure_displace_f64" in _lib.EXPORTS and hdr.count("akb_figure_displace_f64") >= 2
    import inspect
    from akbraytracing_amd import wavedata as W
    for f in (W.saveWaveData, W.plot_result_wave, W.kb_wave):
        assert inspect.signature(f).parameters["figure"].default is None
