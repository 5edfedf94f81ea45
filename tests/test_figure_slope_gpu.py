"""Figure maps that deflect the rays (slope error) on the device: the stage kernel
akb_figure_normal_f64 against the host build of csrc/akb_figure.h (bit for bit), the fused chain and
batch kernels with fig_slope against the staged composition intersection -> deflected normal ->
reflect_ray (bit for bit), the refusals of the wavefront entry points, and the spot modes with figure=.

All grids are 33 x 33 = 1089 rays: four full 256-ray segments plus a tail."""
import ctypes

import numpy as np
import pytest
import torch

import figure_slope_host as FS
from conftest import golden, golden_json
from figure_maps import make_maps as _make_maps

pytestmark = pytest.mark.gpu

N = 33
SHAPES = [(7, 5), (4, 4), (1, 9), (9, 1)]  # (nw, nu) of the four maps


def _geom(name):
    from akbraytracing_amd.wavefront import SystemGeometry
    return SystemGeometry.from_dict(golden_json(name))


def _tables(g, gpu):
    return (torch.from_numpy(np.tan(g.angle_h.table(N))).to(gpu), torch.from_numpy(np.tan(g.angle_v.table(N))).to(gpu))


_CACHE = {}


def _setup(name, gpu):
    """geometry, tables, the map-free trace (the shared reference footprint) and the maps"""
    if name in _CACHE:
        return _CACHE[name]
    from akbraytracing_amd.figure import mirror_frames
    from akbraytracing_amd.trace import grid_dirs, trace_chain
    g = _geom(name)
    th, tv = _tables(g, gpu)
    free = trace_chain(g.mirrors, tan_h=th, tan_v=tv, src=g.source, want=("hits", "last_hit", "dir_out", "opl"))
    hits = free.hits.cpu().numpy()
    K = len(g.mirrors)
    frames = mirror_frames(g)
    maps = _make_maps(frames, hits, SHAPES[:K] if K == 4 else [(7, 5), (1, 9)])
    some = _make_maps(frames, hits, [None, (4, 4), None, (9, 1)][:K] if K == 4 else [None, (9, 1)])
    shrunk = _make_maps(frames, hits, [(7, 5)] + [None] * (K - 1), margin=-0.2)
    dirs0 = grid_dirs(th, tv)
    src = torch.tensor(g.source, dtype=torch.float64, device=gpu).reshape(3, 1).expand(3, N * N).contiguous()
    _CACHE[name] = dict(g=g, th=th, tv=tv, free=free, maps=maps, some=some, shrunk=shrunk, dirs0=dirs0, src=src, frames=frames)
    return _CACHE[name]


def _device_normal(fm, coeffs, hit, ray):
    from akbraytracing_amd.figure import figure_normal
    return figure_normal(fm, coeffs, hit, ray)


def test_stage_kernel_equals_host_build(gpu):
    """akb_figure_normal_f64 == the g++ build of the header on the chain's hits, every mirror and map
    shape; with a NaN column (a ray aimed away from the first mirror) and with a map shrunk inside the
    footprint; the outside flag exactly where the host reports it"""
    from akbraytracing_amd.trace import trace_chain
    S = _setup("akb_geometry.json", gpu)
    g = S["g"]
    bad = S["dirs0"].clone()
    bad[:, 700] = torch.tensor([0.0, 1.0, 0.0], dtype=torch.float64)
    r = trace_chain(g.mirrors, dirs=bad, src=g.source, want=("hits",))
    assert bool(torch.isnan(r.hits[:, :, 700]).all()) and int(torch.isnan(r.hits).sum()) == 3 * len(g.mirrors)
    from akbraytracing_amd import primitives as P
    ray = bad
    for k, m in enumerate(g.mirrors):
        hit = r.hits[k].contiguous()
        for fm, want_flag in ((S["maps"][k], 0), (S["shrunk"][0] if k == 0 else None, 8)):
            if fm is None:
                continue
            got, fl = _device_normal(fm, m.coeffs, hit, ray)
            want, hfl = FS.host_stage(fm, m.coeffs, hit.cpu().numpy(), ray.cpu().numpy())
            assert fl == hfl == want_flag, (k, fl, hfl)
            assert np.array_equal(got.cpu().numpy(), want, equal_nan=True), k
            assert np.isnan(want[:, 700]).all() and np.isfinite(np.delete(want, 700, axis=1)).all()
            plain = P.norm_vector(m.coeffs, hit).cpu().numpy()
            moved = np.any(got.cpu().numpy() != plain, axis=0)
            moved[700] = False
            if want_flag:  # outside hits keep the quadric's unit normal, to the bit
                _, _, outside = FS.host_grad_at(fm, hit.cpu().numpy())
                assert outside.any() and not outside.all()
                assert not moved[outside].any() and moved[~outside & np.isfinite(want[0])].any()
            else:
                assert moved.mean() > 0.9  # the maps do something
        # the next mirror's incoming directions, per ray (the primitives' all-NaN rule is per call)
        nrm = torch.from_numpy(FS.host_stage(S["maps"][k], m.coeffs, hit.cpu().numpy(), ray.cpu().numpy())[0]).to(gpu)
        rr = ray - 2.0 * (ray * nrm).sum(0) * nrm
        ray = (rr / rr.norm(dim=0)).contiguous()


def _staged(S, maps):
    """the staged composition on the full grid: hits, exit directions, opl = sum of segments in order
    plus the path terms' sum, fig_opl"""
    from akbraytracing_amd.figure import stage_normals
    hits, ray, segs, word, terms = stage_normals(S["g"].mirrors, maps, S["dirs0"], S["src"], with_segments=True,
                                                 with_terms=True)
    assert word == 0
    opl = segs[0]
    for s in segs[1:]:
        opl = opl + s
    return torch.stack(hits), ray, opl + terms, terms


@pytest.mark.parametrize("name", ["akb_geometry.json", "kb_geometry.json"])
@pytest.mark.parametrize("which", ["maps", "some"])
def test_fused_chain_with_slope_equals_staged_composition(gpu, name, which):
    """trace_chain(figure=..., figure_slope=True): last hit, exit direction, hits, opl and fig_opl equal
    intersection -> akb_figure_normal_f64 -> reflect_ray (+ akb_figure_opl_f64 on the deflected path) bit
    for bit: grid and explicit directions, hits on and off, a ray0 / n_rays window, maps that only
    deflect (no opl), and the sink kernels"""
    from akbraytracing_amd.reduce import LeafSink
    from akbraytracing_amd.trace import trace_chain
    S = _setup(name, gpu)
    g, maps = S["g"], S[which]
    hits, ray, opl, terms = _staged(S, maps)
    assert not torch.equal(ray, S["free"].dir_out)  # the maps deflect
    # and the hits move behind the first mapped mirror only
    upstream = any(m is not None for m in maps[:-1])
    assert torch.equal(hits[0], S["free"].hits[0]) and torch.equal(hits[-1], S["free"].hits[-1]) != upstream
    for kw in (dict(tan_h=S["th"], tan_v=S["tv"]), dict(dirs=S["dirs0"])):
        for want in (("hits", "last_hit", "dir_out", "opl", "fig_opl"), ("last_hit", "dir_out", "opl", "fig_opl")):
            r = trace_chain(g.mirrors, src=g.source, want=want, figure=maps, figure_slope=True, **kw)
            assert int(r.flags.item()) == 0
            if "hits" in want:
                assert torch.equal(r.hits, hits)
            assert torch.equal(r.last_hit, hits[-1]) and torch.equal(r.dir_out, ray)
            assert torch.equal(r.fig_opl, terms) and torch.equal(r.opl, opl)
        # maps that only deflect: no opl row, no path term
        for want in (("hits", "last_hit", "dir_out"), ("last_hit", "dir_out")):
            r = trace_chain(g.mirrors, src=g.source, want=want, figure=maps, figure_slope=True, **kw)
            assert torch.equal(r.last_hit, hits[-1]) and torch.equal(r.dir_out, ray) and r.opl is None
            if "hits" in want:
                assert torch.equal(r.hits, hits)
    # a window of the grid: rays 300 .. 799 (a partial first segment, a full one, a tail)
    r = trace_chain(g.mirrors, tan_h=S["th"], tan_v=S["tv"], src=g.source, want=("hits", "last_hit", "dir_out", "opl", "fig_opl"),
                    figure=maps, figure_slope=True, ray0=300, n_rays=500)
    assert torch.equal(r.hits, hits[:, :, 300:800]) and torch.equal(r.dir_out, ray[:, 300:800])
    assert torch.equal(r.opl, opl[300:800]) and torch.equal(r.fig_opl, terms[300:800])
    # the sink kernels (pass 2's fixed output set, and the full one with the detector rows)
    for want in (("last_hit", "dir_out", "opl"), ("last_hit", "dir_out", "opl", "det", "fig_opl")):
        sink = LeafSink(5, N * N, 0b00011, gpu)
        r = trace_chain(g.mirrors, tan_h=S["th"], tan_v=S["tv"], src=g.source, det_ghij=g.det1, want=want, sink=sink,
                        figure=maps, figure_slope=True)
        assert torch.equal(r.last_hit, hits[-1]) and torch.equal(r.dir_out, ray) and torch.equal(r.opl, opl)
        q = trace_chain(g.mirrors, tan_h=S["th"], tan_v=S["tv"], src=g.source, det_ghij=g.det1, want=("det", "atan", "opl"),
                        figure=maps, figure_slope=True)
        sums, counts = sink.finish()
        assert int(counts[2].item()) == N * N
        assert abs(float(sums[2]) - float(q.det[0].sum())) <= 1e-9 * abs(float(q.det[0].sum()))


def test_outside_hit_with_slope_reflects_about_the_quadric_normal(gpu):
    """a map narrower than the footprint: the flag is raised, and the fused chain still equals the staged
    composition (outside hits reflect about N itself)"""
    from akbraytracing_amd.figure import stage_normals
    from akbraytracing_amd.trace import trace_chain
    S = _setup("akb_geometry.json", gpu)
    g = S["g"]
    hits, ray, _, word = stage_normals(g.mirrors, S["shrunk"], S["dirs0"], S["src"])
    r = trace_chain(g.mirrors, tan_h=S["th"], tan_v=S["tv"], src=g.source, want=("hits", "dir_out"), figure=S["shrunk"],
                    figure_slope=True)
    assert word == 0x8 and int(r.flags.item()) == 0x8
    assert torch.equal(r.hits, torch.stack(hits)) and torch.equal(r.dir_out, ray)


def test_slope_off_is_byte_identical_to_the_unset_field(gpu):
    from akbraytracing_amd.trace import trace_chain
    S = _setup("akb_geometry.json", gpu)
    g = S["g"]
    want = ("hits", "last_hit", "dir_out", "opl", "fig_opl")
    for kw in (dict(tan_h=S["th"], tan_v=S["tv"]), dict(dirs=S["dirs0"])):
        a = trace_chain(g.mirrors, src=g.source, want=want, figure=S["maps"], **kw)
        b = trace_chain(g.mirrors, src=g.source, want=want, figure=S["maps"], figure_slope=False, **kw)
        for f in want:
            assert torch.equal(getattr(a, f), getattr(b, f)), f
        # the thin screen leaves the path alone
        plain = trace_chain(g.mirrors, src=g.source, want=want[:4], **kw)
        assert torch.equal(a.dir_out, plain.dir_out) and torch.equal(a.hits, plain.hits)
        # and without maps figure_slope changes nothing
        c = trace_chain(g.mirrors, src=g.source, want=want[:4], figure_slope=True, **kw)
        assert torch.equal(c.dir_out, plain.dir_out) and torch.equal(c.opl, plain.opl)


def _af_builds():
    from akbraytracing_amd.geometry import build_akb
    f = golden("akb_autofocus.npz")
    cases = [dict(params=f[f"g{k}_params"], source_shift=f[f"g{k}_source_shift"]) for k in (0, 2)]
    assert not np.array_equal(cases[0]["params"], cases[1]["params"])
    return [build_akb(c["params"], source_shift=c["source_shift"]) for c in (cases[0], cases[1], cases[0])]


def test_batch_equals_single_launches(gpu):
    """TracedSystems over three systems (two distinct params vectors of the autofocus fixture, and the
    first again without maps, through a callable figure) equals three trace_chain(figure_slope=True)
    launches bit for bit; evaluate() on two planes gives finite sizes; a descriptor with a map and
    fig_slope = 0 is refused"""
    from akbraytracing_amd import _lib
    from akbraytracing_amd.autofocus import TracedSystems, _tables
    from akbraytracing_amd.figure import mirror_frames
    from akbraytracing_amd.geometry import mirrors_of
    from akbraytracing_amd.trace import ChainLaunch, trace_chain
    bs = _af_builds()
    free = TracedSystems(bs, ray_num=N, want_hits=True, tilt=False)
    fh = free.hits.cpu().numpy()
    figs = {id(b): _make_maps(mirror_frames(b), fh[s], SHAPES) for s, b in enumerate(bs[:2])}
    figs[id(bs[2])] = None
    ts = TracedSystems(bs, ray_num=N, want_hits=True, figure=lambda b: figs[id(b)])
    for s, b in enumerate(bs):
        th, tv = (torch.from_numpy(x).to(gpu) for x in _tables(b, N))
        r = trace_chain(mirrors_of(b), tan_h=th, tan_v=tv, src=b["source"], want=("hits", "last_hit", "dir_out"),
                        figure=figs[id(b)], figure_slope=True)
        assert torch.equal(r.hits, ts.hits[s]) and torch.equal(r.dir_out, ts.dir[s]) and torch.equal(r.last_hit, ts.pt[s])
    assert not torch.equal(ts.dir[0], free.dir[0]) and torch.equal(ts.dir[2], free.dir[2])
    sv, sh = ts.evaluate(np.array([0.0, 1e-4]))
    assert sv.shape == (3, 2) and np.isfinite(sv).all() and np.isfinite(sh).all()
    # without the hits rows too (the other kernel instantiation)
    t2 = TracedSystems(bs, ray_num=N, tilt=False, figure=lambda b: figs[id(b)])
    assert torch.equal(t2.dir, ts.dir) and torch.equal(t2.pt, ts.pt)
    # a map that would not deflect is refused
    b = bs[0]
    th, tv = (torch.from_numpy(x).to(gpu) for x in _tables(b, N))
    c = ChainLaunch(mirrors_of(b), tan_h=th, tan_v=tv, src=b["source"], want=("last_hit", "dir_out", "opl"), figure=figs[id(b)])
    L = _lib.lib()
    assert L.akb_trace_chain_batch_f64(c.desc, 1, None) == -1 and b"fig_slope" in L.akb_last_error()
    # a map that covers too little raises
    small = _make_maps(mirror_frames(b), fh[0], [None, None, (4, 4), None], margin=-0.2)
    with pytest.raises(_lib.AKBError, match="figure map of mirror 2"):
        TracedSystems([b], ray_num=N, figure=small)


def test_wavefront_entry_points_refuse_fig_slope(gpu):
    from akbraytracing_amd import _lib
    from akbraytracing_amd.trace import ChainLaunch
    from akbraytracing_amd.wavefront import RayWave
    S = _setup("akb_geometry.json", gpu)
    g = S["g"]
    L = _lib.lib()
    c = ChainLaunch(g.mirrors, tan_h=S["th"], tan_v=S["tv"], src=g.source, want=("last_hit", "dir_out"), figure_slope=True)
    c.res.last_hit.fill_(7.0)
    d = c.desc
    assert d.fig_slope == 1
    z = ctypes.c_void_p(0)
    sink = _lib.LeafSink()
    calls = [lambda: L.akb_trace_chain_dd_f64(d, None), lambda: L.akb_trace_chain_samples_f64(d, None),
             lambda: L.akb_chain_tilt_f64(d, ctypes.c_void_p(8), z, z, z, z, z, N * N, N * N, z, z, z, z, z, z,
                                          ctypes.byref(sink), None)]
    for f in calls:
        assert f() == -1
        assert b"fig_slope" in L.akb_last_error()
    torch.cuda.synchronize()
    assert bool((c.res.last_hit == 7.0).all()) and int(c.res.flags.item()) == 0
    with pytest.raises(ValueError, match="thin screen"):
        ChainLaunch(g.mirrors, tan_h=S["th"], tan_v=S["tv"], src=g.source, want=("last_hit",), figure_slope=True,
                    precision="dd")
    with pytest.raises(TypeError):
        RayWave(g, N, figure=S["maps"], figure_slope=True)


def test_plot_result_test_ramp_moves_the_centroid(gpu):
    """A ramp h = s u (s = 1e-6) on the last mirror of the trace, untilted 'test' mode. The hits on the
    mirrors do not move; every exit ray turns by delta = 2 atan(s) in its plane of incidence towards the
    beam-facing normal (the CPU analytic test), so detector hit i moves by delta L_i w_i with L_i its
    last-hit-to-detector distance and w_i the in-plane unit vector across the ray, stretched onto the
    plane x = const by at most 1 / r_x^2.

    Sign: the centroid moves along the centre ray's beam-facing normal.
    Magnitude against delta L_c (L_c: the centre ray's distance), from the map-free trace alone:
      | ||mean_i(delta L_i w_i)|| - delta L_c | <= delta (max_i |L_i - L_c| (1 + e) + L_c e),
      e = phi^2 / 2 + max_i (1 / r_x,i^2 - 1) + phi
    phi: the largest angle between the rays' w_i (the normals at the footprint's hits against the centre
    ray's, plus the exit directions' spread): parallel vectors within phi average to at least cos phi;
    the last phi covers the ramp's gradient s e_u taken in the frame's axes instead of each hit's own
    tangent plane (the slope seen there is s cos of an angle below phi - second order - and its
    direction turns with the normal, first order). The interpolant of a ramp is the ramp at interior
    points (one cell from every edge; the map is built so), to rounding."""
    from akbraytracing_amd.autofocus import plot_result_test
    from akbraytracing_amd.figure import FigureMap, mirror_frames
    from akbraytracing_amd.geometry import build_akb
    from akbraytracing_amd import primitives as P
    f = golden("akb_autofocus.npz")
    params = f["g0_params"]
    b = build_akb(params)
    K = len(b["mirrors"])
    free = plot_result_test(params, option_tilt=False, ray_num=N)
    last, det0, ang0 = free[1], free[4], free[5]  # the last mirror of the trace is the second returned
    fr = mirror_frames(b)[K - 1]
    u = fr["e_u"] @ (last - fr["origin"].reshape(3, 1))
    w = fr["e_w"] @ (last - fr["origin"].reshape(3, 1))
    du, dw = np.ptp(u) / 3, np.ptp(w) / 3
    u0, w0 = u.min() - 2 * du, w.min() - 2 * dw  # footprint inside cells 2 .. 5 of 8 samples
    s = 1e-6
    tab = s * (u0 + du * np.arange(8))[None, :] * np.ones((8, 1))
    fig = [None] * (K - 1) + [FigureMap(tab, u0, du, w0, dw, fr["origin"], fr["e_u"], fr["e_w"])]
    got = plot_result_test(params, option_tilt=False, ray_num=N, figure=fig)
    for k in range(4):
        assert np.array_equal(got[k], free[k])
    shift = got[4].mean(axis=1) - det0.mean(axis=1)
    delta = 2 * np.arctan(s)
    L = np.linalg.norm(det0 - last, axis=0)
    c = (N * N) // 2
    coeffs = b["mirrors"][K - 1]["coeffs"]
    nrm = P.norm_vector(coeffs, torch.from_numpy(np.ascontiguousarray(last)).to(gpu)).cpu().numpy()
    nrm = nrm * np.sign(nrm.T @ fr["normal"])  # beam-facing
    wv = nrm - (nrm * ang0).sum(0) * ang0
    wv = wv / np.linalg.norm(wv, axis=0)
    phi = np.arccos(np.clip(wv.T @ wv[:, c], -1, 1)).max()
    e = phi**2 / 2 + (1 / ang0[0]**2 - 1).max() + phi
    margin = delta * (np.abs(L - L[c]).max() * (1 + e) + L[c] * e)
    print(f"centroid shift {shift}, |shift| {np.linalg.norm(shift):.6e}, delta L_c {delta * L[c]:.6e}, margin {margin:.3e} "
          f"(phi {phi:.2e}, spread of L {np.abs(L - L[c]).max():.3e} of {L[c]:.3f} m)")
    assert shift @ fr["normal"] > 0
    assert abs(np.linalg.norm(shift) - delta * L[c]) <= margin
    # The footprint is long against the working distance, so the bound above is wide. The same model ray
    # by ray, shift = delta mean_i(L_i (w_i - r_i w_x,i / r_x,i)), leaves only what it neglects: the
    # gradient s e_u taken in the frame's axes instead of hit i's tangent plane turns the deflection by at
    # most the angle phi_n between that hit's normal and the centre ray's (first order), and second-order
    # terms in delta (1e-6 relative).
    proj = wv - ang0 * (wv[0] / ang0[0])
    model = delta * (L * proj).mean(axis=1)
    phi_n = np.arccos(np.clip(nrm.T @ nrm[:, c], -1, 1)).max()
    print(f"ray-by-ray model {model}, |shift - model| {np.linalg.norm(shift - model):.3e}, phi_n {phi_n:.3e}")
    assert np.linalg.norm(shift - model) <= (phi_n + 1e-6) * np.linalg.norm(model)


def test_calc_FoC_and_auto_focus_NA_take_figure(gpu):
    """one source position of calc_FoC (the FoC-mode auto_focus_NA inside it) with a callable figure that
    follows the mirrors: a sinusoidal profile of 0.5 microrad RMS slope on the last mirror widens the spot
    in that mirror's focusing direction (h) by more than it does across it; the cache keeps systems
    with different figures apart"""
    from akbraytracing_amd import autofocus as AFm
    from akbraytracing_amd.figure import FigureMap, mirror_frames
    f = golden("akb_autofocus.npz")
    p0 = f["af0_start"].copy()
    uu = np.linspace(-0.05, 0.05, 2001)
    amp, lam = 3.2e-10, 2.83e-3  # slope RMS amp 2 pi / lam / sqrt(2) = 0.5e-6

    def figure(b):
        fr = mirror_frames(b)[len(b["mirrors"]) - 1]
        return [None] * (len(b["mirrors"]) - 1) + [FigureMap.from_profile(uu, amp * np.sin(2 * np.pi * uu / lam), fr)]

    plain = AFm.calc_FoC(p0.copy(), range_h=[0.0, 0.0, 1], range_v=[0.0, 0.0, 1])
    fig = AFm.calc_FoC(p0.copy(), range_h=[0.0, 0.0, 1], range_v=[0.0, 0.0, 1], figure=figure)
    for k in ("focuspointX", "focuspointY", "focuspointZ", "focussizeH", "focussizeV"):
        assert fig[k].shape == (1, 1) and np.isfinite(fig[k]).all()
    dh = fig["focussizeH"][0, 0] - plain["focussizeH"][0, 0]
    dv = fig["focussizeV"][0, 0] - plain["focussizeV"][0, 0]
    print(f"calc_FoC extent H {plain['focussizeH'][0, 0]:.3e} -> {fig['focussizeH'][0, 0]:.3e}, "
          f"V {plain['focussizeV'][0, 0]:.3e} -> {fig['focussizeV'][0, 0]:.3e}")
    # the peak deflection 2 * sqrt(2) * 0.5e-6 over at least 1 cm to the focus, both ways: the extent
    # grows by more than 1e-8 m in h
    assert dh > 1e-8 and dh > abs(dv)
    cache = AFm._SystemCache(True, 53, figure=figure)
    with pytest.raises(ValueError, match="another figure"):
        AFm.auto_focus_NA(100, p0.copy(), 1, 1, False, None, verbose=False, cache=cache)


def test_missed_ray_with_maps_takes_the_staged_composition(gpu):
    """the source moved by a metre, so that every ray misses the second mirror, with maps set: the
    flagged system goes through figure.stage_normals, whose primitives apply the reference's all-NaN
    rule - the same rows as the map-free flagged system, and no outside error (the maps are 1-D profiles
    two hundred kilometres long: no finite hit is outside, and a NaN hit raises no flag)"""
    from akbraytracing_amd import _lib
    from akbraytracing_amd.autofocus import TracedSystems
    from akbraytracing_amd.figure import FigureMap, mirror_frames
    good = _af_builds()[0]
    b = dict(good)
    b["source"] = [float(good["source"][0]), float(good["source"][1]), float(good["source"][2]) + 1.0]
    figs = [FigureMap.from_profile([-1e5, 1e5], [1e-3, -1e-3], fr) for fr in mirror_frames(good)]
    free = TracedSystems([b], ray_num=N, want_hits=True, tilt=False)
    ts = TracedSystems([b], ray_num=N, want_hits=True, tilt=False, figure=figs)
    for t in (free, ts):
        fl = int(t.flags[0].item())
        assert fl & 0x1111111 and not fl & 0x8888888, hex(fl)  # a miss on some mirror, nothing outside
        assert bool(torch.isnan(t.dir).all()) and bool(torch.isnan(t.pt).all())
        assert bool(torch.isnan(t.hits[0, 1:]).all())
    # the first mirror is hit before anything deflects: the same finite hits
    assert bool(torch.isfinite(ts.hits[0, 0]).all()) and torch.equal(ts.hits[0, 0], free.hits[0, 0])
    # the same maps on the unmoved system do deflect
    ok = TracedSystems([good], ray_num=N, tilt=False, figure=figs)
    assert int(ok.flags[0].item()) == 0 and bool(torch.isfinite(ok.dir).all())
    assert not torch.equal(ok.dir, TracedSystems([good], ray_num=N, tilt=False).dir)
