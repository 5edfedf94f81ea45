"""Figure maps on the device: the stage kernel against the host build of csrc/akb_figure.h (bit for
bit), the fused chain kernels against the stage kernels' sum in mirror order (bit for bit), and
RayWave / the drivers with figure= (run, pipeline, shards, staged and double-double paths)."""
import ctypes
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import figure_host as FH
from conftest import GOLDEN, golden_json

pytestmark = pytest.mark.gpu

AMP = 1e-9  # 1 nm of figure


def _geom(name="akb_geometry.json"):
    from akbraytracing_amd.wavefront import SystemGeometry
    return SystemGeometry.from_dict(golden_json(name))


def _tables(g, n, gpu):
    return (torch.from_numpy(np.tan(g.angle_h.table(n))).to(gpu), torch.from_numpy(np.tan(g.angle_v.table(n))).to(gpu))


_MAPS = {}


def _maps(name="akb_geometry.json", which=None, zero=False, margin=0.25, nu=24, nw=6):
    """One smooth 2-D map per mirror (which: the mirrors that get one) in mirror_frames' frames,
    covering the 33 x 33 grid's footprint plus a margin (the launch range is the same for every grid
    size and for the resampled pass 2). Returns (maps, slopes): slopes[k] bounds |grad h| of map k."""
    key = (name, which, zero, margin, nu, nw)
    if key in _MAPS:
        return _MAPS[key]
    from akbraytracing_amd.figure import FigureMap, mirror_frames
    from akbraytracing_amd.trace import trace_chain
    g = _geom(name)
    dev = torch.device("cuda", 0)
    th, tv = _tables(g, 33, dev)
    hits = trace_chain(g.mirrors, tan_h=th, tan_v=tv, src=g.source, want=("hits",)).hits.cpu().numpy()
    maps, slopes = [], []
    for k, fr in enumerate(mirror_frames(g)):
        if which is not None and k not in which:
            maps.append(None)
            slopes.append(0.0)
            continue
        d = hits[k] - fr["origin"].reshape(3, 1)
        u, w = fr["e_u"] @ d, fr["e_w"] @ d
        lu, lw = np.ptp(u), np.ptp(w)
        u0, w0 = u.min() - margin * lu, w.min() - margin * lw
        du, dw = (1 + 2 * margin) * lu / (nu - 1), (1 + 2 * margin) * lw / (nw - 1)
        U, W = u0 + du * np.arange(nu), w0 + dw * np.arange(nw)
        ku, kw = 2 * np.pi * (1.5 + 0.5 * k) / (nu * du), 2 * np.pi / (nw * dw)
        h = AMP * np.sin(ku * U[None, :] + 0.3 * k) * np.cos(kw * W[:, None])
        maps.append(FigureMap(np.zeros_like(h) if zero else h, u0, du, w0, dw, fr["origin"], fr["e_u"], fr["e_w"]))
        # Catmull-Rom's derivative is at most 3 Hmax per pitch on each axis (figure_host.error_bound)
        slopes.append(3 * AMP / du + 3 * AMP / dw)
    _MAPS[key] = (maps, slopes)
    return _MAPS[key]


def _incoming(g, hits, dirs0):
    """the unit directions entering each mirror, rebuilt as the staged chain does"""
    from akbraytracing_amd import primitives as P
    out, ray = [], dirs0
    for k, m in enumerate(g.mirrors):
        out.append(ray)
        if k + 1 < len(g.mirrors):
            ray = P.reflect_ray(ray, P.norm_vector(m.coeffs, hits[k].contiguous()))
    return out


def _stage(fm, coeffs, hit, ray, out=None):
    from akbraytracing_amd import _lib, device as D
    n = hit.shape[1]
    acc = out is not None
    out = torch.empty(n, dtype=torch.float64, device=hit.device) if out is None else out
    fl = torch.zeros(1, dtype=torch.int32, device=hit.device)
    hit, ray = hit.contiguous(), ray.contiguous()
    _lib.check(_lib.lib().akb_figure_opl_f64(fm.desc(hit.device), D.host_f64(coeffs), D.ptr(hit), n, 1, D.ptr(ray), n, 1,
                                             n, D.ptr(out), int(acc), D.ptr(fl), D.stream_handle()))
    return out, int(fl.item())


@pytest.mark.parametrize("name", ["akb_geometry.json", "kb_geometry.json"])
@pytest.mark.parametrize("n", [17, 33, 97])
def test_stage_kernel_equals_host_build_and_fused_equals_stage_sum(gpu, name, n):
    """on the chain's own hits: stage kernel == g++ build of the header, bit for bit, mirror by mirror
    (written and accumulated); the fused k_chain's fig_opl == the stage kernels' sum in mirror order,
    with grid rays and with explicit dirs; opl within one rounding; everything else identical"""
    from akbraytracing_amd.figure import stage_terms
    from akbraytracing_amd.trace import grid_dirs, trace_chain
    g = _geom(name)
    maps, _ = _maps(name)
    th, tv = _tables(g, n, gpu)
    want = ("hits", "last_hit", "dir_out", "det", "atan", "opl")
    base = trace_chain(g.mirrors, tan_h=th, tan_v=tv, src=g.source, det_ghij=g.det1, want=want)
    dirs0 = grid_dirs(th, tv)
    inc = _incoming(g, base.hits, dirs0)
    acc_dev, acc_host = None, None
    for k, m in enumerate(g.mirrors):
        one, fl = _stage(maps[k], m.coeffs, base.hits[k], inc[k])
        hone, hfl = FH.host_stage(maps[k], m.coeffs, base.hits[k].cpu().numpy(), inc[k].cpu().numpy())
        assert fl == 0 and hfl == 0
        assert np.array_equal(one.cpu().numpy(), hone), k
        assert float(one.abs().max()) > 0.01 * AMP  # the maps do something
        acc_dev, _ = _stage(maps[k], m.coeffs, base.hits[k], inc[k], out=acc_dev) if acc_dev is not None else (one, 0)
        acc_host = hone if acc_host is None else FH.host_stage(maps[k], m.coeffs, base.hits[k].cpu().numpy(),
                                                               inc[k].cpu().numpy(), out=acc_host)[0]
    assert np.array_equal(acc_dev.cpu().numpy(), acc_host)
    total, word = stage_terms(g.mirrors, maps, [base.hits[k] for k in range(len(maps))], dirs0)
    assert word == 0 and torch.equal(total, acc_dev)
    for kw in (dict(tan_h=th, tan_v=tv), dict(dirs=dirs0)):
        plain = base if "tan_h" in kw else trace_chain(g.mirrors, src=g.source, det_ghij=g.det1, want=want, **kw)
        fig = trace_chain(g.mirrors, src=g.source, det_ghij=g.det1, want=want + ("fig_opl",), figure=maps, **kw)
        assert torch.equal(fig.fig_opl, total)
        # opl_fig = RN(opl_0 + fig_opl): one rounding of a sum of metres
        o0 = plain.opl.cpu().numpy()
        err = np.abs(fig.opl.cpu().numpy() - (o0 + total.cpu().numpy()))
        assert np.all(err <= np.spacing(o0))
        for f in ("hits", "last_hit", "dir_out", "det", "atan"):
            assert torch.equal(getattr(fig, f), getattr(plain, f)), f
        assert int(fig.flags.item()) == int(plain.flags.item()) == 0
        # None on every mirror, and all-zero maps: today's bits
        none = trace_chain(g.mirrors, src=g.source, det_ghij=g.det1, want=want, figure=[None] * len(maps), **kw)
        zero = trace_chain(g.mirrors, src=g.source, det_ghij=g.det1, want=want + ("fig_opl",),
                           figure=_maps(name, zero=True)[0], **kw)
        for f in want:
            assert torch.equal(getattr(none, f), getattr(plain, f)) and torch.equal(getattr(zero, f), getattr(plain, f)), f
        assert not zero.fig_opl.any()


def test_map_on_one_mirror_only(gpu):
    from akbraytracing_amd.trace import grid_dirs, trace_chain
    g = _geom()
    maps, _ = _maps(which=(2,))
    assert [m is None for m in maps] == [True, True, False, True]
    th, tv = _tables(g, 33, gpu)
    r = trace_chain(g.mirrors, tan_h=th, tan_v=tv, src=g.source, want=("hits", "opl", "fig_opl"), figure=maps)
    inc = _incoming(g, r.hits, grid_dirs(th, tv))
    one, _ = _stage(maps[2], g.mirrors[2].coeffs, r.hits[2], inc[2])
    assert torch.equal(r.fig_opl, one)


@pytest.mark.parametrize("name,n", [("akb_geometry.json", 17), ("akb_geometry.json", 33), ("akb_geometry.json", 97),
                                    ("kb_geometry.json", 33)])
def test_raywave_sink_path(gpu, name, n):
    """RayWave.run(): pass 2 is the sink kernel's figure instantiation; fig_opl == the stage sum on
    pass 2's own hits; every other pass-2 row as without maps; zero maps and None: today's bits"""
    from akbraytracing_amd.figure import stage_terms
    from akbraytracing_amd.trace import grid_dirs, trace_chain
    from akbraytracing_amd.wavefront import RayWave
    g = _geom(name)
    maps, _ = _maps(name)
    rs = name.startswith("akb")
    plain = {k: (v.clone() if isinstance(v, torch.Tensor) else v)
             for k, v in RayWave(g, n, resample_pass=rs).run(full=False).items()}
    out = RayWave(g, n, resample_pass=rs, figure=maps).run()
    h = trace_chain(g.mirrors, tan_h=out["tan_h2"], tan_v=out["tan_v2"], src=g.source, want=("hits",)).hits
    total, word = stage_terms(g.mirrors, maps, [h[k] for k in range(len(maps))], grid_dirs(out["tan_h2"], out["tan_v2"]))
    assert word == 0 and torch.equal(out["fig_opl"], total)
    o0 = plain["opl"].cpu().numpy()
    assert np.all(np.abs(out["opl"].cpu().numpy() - (o0 + total.cpu().numpy())) <= np.spacing(o0))
    for k in ("last_hit", "dir_out", "detcenter2", "tan_h2"):
        if plain.get(k) is not None:
            assert torch.equal(out[k], plain[k]), k
    assert out["flags"] == plain["flags"] == (0, 0)
    assert not torch.equal(out["dist_err2"], plain["dist_err2"])
    for fig in (_maps(name, zero=True)[0], [None] * len(maps)):
        z = RayWave(g, n, resample_pass=rs, figure=fig).run()
        for k in ("opl", "last_hit", "dir_out", "dist_err2", "wave2", "detcenter2", "total2"):
            if plain.get(k) is not None:
                assert torch.equal(z[k], plain[k]), k


def test_full_rows_variant_and_perturbation_order(gpu):
    """run(full=True) takes the sink kernel's other figure instantiation; perturbation and figure add
    in the stated order, opl = (opl + d_pert) + d_fig"""
    from akbraytracing_amd.legendre import LegendrePerturbation, orders
    from akbraytracing_amd.wavefront import RayWave
    g = _geom()
    maps, _ = _maps()
    n = 33
    fixed = RayWave(g, n, figure=maps).run()
    fixed = {k: fixed[k].clone() for k in ("opl", "fig_opl", "wave2")}
    full = RayWave(g, n, figure=maps).run(full=True)
    for k, v in fixed.items():
        assert torch.equal(full[k], v), k
    c = np.zeros(len(orders(5)))
    c[3], c[7] = 2e-9, -1e-9
    pert = LegendrePerturbation(c)
    p_only = RayWave(g, n, perturbation=pert).run()["opl"].clone()
    both = RayWave(g, n, perturbation=pert, figure=maps).run()
    assert torch.equal(both["fig_opl"], fixed["fig_opl"])
    assert torch.equal(both["opl"], p_only + both["fig_opl"])


def test_pipelined_three_systems_equal_sequential_runs(gpu):
    """launch_front / launch_back with the fused tilt and OPD (bench.py's --fuse 2 schedule) over
    consecutive systems with figure maps: the bits of sequential run()s"""
    from test_gpu_parity import _fused_pipeline, _variants
    from akbraytracing_amd.wavefront import RayWave
    n, lag = 65, 2
    systems = _variants(3)
    maps, _ = _maps()
    rw = RayWave(_geom(), n, figure=maps)
    wants = []
    for s in systems:
        o = rw.run(geometry=s)
        wants.append({k: o[k].clone() for k in ("wave2", "dist_err2", "detcenter2", "total2")})
    assert not torch.equal(wants[0]["wave2"], wants[1]["wave2"])
    bs = torch.cuda.Stream()
    outs, kinds = [], []

    def back(front):
        kinds.append((front.tilt is not None, front.opd is not None))
        with torch.cuda.stream(bs):
            o = rw.launch_back(front, stream=bs)
            outs.append({k: o[k].clone() for k in wants[0]})

    seq = [systems[i % 3] for i in range(lag + 4)]
    kws = [dict(geometry=s, next_geometry=seq[i + 1] if i + 1 < len(seq) else None) for i, s in enumerate(seq)]
    want_kinds = _fused_pipeline(rw, back, lag, kws)
    torch.cuda.synchronize()
    assert kinds == want_kinds and (True, True) in kinds
    for i, o in enumerate(outs):
        for k, v in wants[i % 3].items():
            assert torch.equal(o[k], v), (i, k)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _shard_worker(rank, world, port, n, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank), AKB_DIST_BACKEND="gloo")
    import torch.distributed as dist
    from akbraytracing_amd import dist as AD
    from akbraytracing_amd.wavefront import RayWave, Shard
    AD.init_from_env()
    try:
        dev = torch.device("cuda", torch.cuda.current_device())
        maps, _ = _maps()
        rw = RayWave(_geom(), n, shard=Shard.split(n, world, rank), comm=AD.TorchComm(dev), figure=maps)
        o = rw.run()
        torch.cuda.synchronize()
        np.savez(os.path.join(out_dir, f"r{rank}.npz"), **{k: o[k].cpu().numpy() for k in ("fig_opl", "opl", "wave2", "dist_err2")})
    finally:
        dist.destroy_process_group()


def test_two_ray_shards_equal_the_unsharded_run(gpu, tmp_path):
    from akbraytracing_amd.wavefront import RayWave
    n = 129
    one = RayWave(_geom(), n, figure=_maps()[0]).run()
    want = {k: one[k].cpu().numpy() for k in ("fig_opl", "opl", "wave2", "dist_err2")}
    del one
    torch.cuda.synchronize()
    mp.start_processes(_shard_worker, args=(2, _free_port(), n, str(tmp_path)), nprocs=2, join=True, start_method="spawn")
    parts = [np.load(os.path.join(tmp_path, f"r{r}.npz")) for r in range(2)]
    for k, v in want.items():
        assert np.array_equal(np.concatenate([p[k] for p in parts]), v), k


def test_double_double_run_with_figure(gpu):
    """RayWave(precision="dd", figure=...): fig_opl equals the float64 run's to a bound derived from
    the hits' distance and the map's slope; DistError2 equals the figure-free double-double run plus
    the centred fig_opl within 1 ulp of the OPL in nm (the run adds the terms to the OPD maps centred,
    RayWave._add_figure_centred: added to the 146 m path rows ahead of the means they measured 1.104
    ulp, from the terms' quantisation to the rows' ulp and the float64 means' own rounding)."""
    from akbraytracing_amd.wavefront import RayWave
    g = _geom()
    maps, slopes = _maps()
    n = 33
    f64 = RayWave(g, n, figure=maps).run()["fig_opl"].cpu().numpy()
    free = RayWave(g, n, precision="dd").run()
    free = {k: free[k].cpu().numpy() for k in ("dist_err2", "opl")}
    dd = RayWave(g, n, precision="dd", figure=maps).run()
    fig = dd["fig_opl"].cpu().numpy()
    # the float64 and double-double hits differ by at most 5e-10 m (DESIGN's double-double section), so
    # each mirror's height differs by at most slope_k * 5e-10 * sqrt(2) (both map axes), and its term
    # by twice that times |d . n| <= 1 (taken as 1); the directions' difference (1e-12 at most) moves
    # |d . n| by as much: 2 Hmax 1e-12 per mirror
    bound = sum(2 * s * 5e-10 * np.sqrt(2) + 2 * AMP * 1e-12 for s in slopes)
    d = np.max(np.abs(fig - f64))
    print(f"dd vs f64 fig_opl: max |diff| {d:.3e} m, bound {bound:.3e} m")
    assert d <= bound
    ulp_nm = np.spacing(free["opl"].max()) * 1e9
    want = free["dist_err2"] + (fig - fig.mean()) * 1e9
    e = np.abs(dd["dist_err2"].cpu().numpy() - want)
    print(f"dd DistError2 vs figure-free + centred fig_opl: max {e.max() / ulp_nm:.3f} ulp(OPL) in nm, "
          f"{np.mean(e > ulp_nm):.4f} of the rays above 1")
    assert np.all(e <= ulp_nm)
    # the reported path row carries the rounded terms
    assert np.all(np.abs(dd["opl"].cpu().numpy() - (free["opl"] + fig)) <= np.spacing(free["opl"]))


def test_map_narrower_than_the_footprint_raises(gpu):
    from akbraytracing_amd._lib import AKBError
    from akbraytracing_amd.wavefront import RayWave
    g = _geom()
    narrow = list(_maps()[0])
    narrow[1] = _maps(margin=-0.2)[0][1]
    with pytest.raises(AKBError, match="figure map of mirror 1"):
        RayWave(g, 33, figure=narrow).run()
    with pytest.raises(AKBError, match="figure map of mirror 1"):
        RayWave(g, 17, figure=narrow, precision="dd").run()


def test_missing_ray_among_finite_ones(gpu):
    """one explicitly aimed missing ray: NaN fig_opl, no outside flag, the others unchanged"""
    from akbraytracing_amd.trace import grid_dirs, trace_chain
    g = _geom()
    maps, _ = _maps()
    th, tv = _tables(g, 17, gpu)
    dirs = grid_dirs(th, tv)
    want = trace_chain(g.mirrors, dirs=dirs, src=g.source, want=("opl", "fig_opl"), figure=maps)
    bad = dirs.clone()
    bad[:, 100] = torch.tensor([0.0, 1.0, 0.0], dtype=torch.float64)  # away from the first mirror
    r = trace_chain(g.mirrors, dirs=bad, src=g.source, want=("opl", "fig_opl"), figure=maps)
    fl = int(r.flags.item())
    assert fl & 0x1 and not fl & 0x8888888
    keep = torch.ones(17 * 17, dtype=torch.bool, device=gpu)
    keep[100] = False
    assert bool(torch.isnan(r.fig_opl[100])) and bool(torch.isnan(r.opl[100]))
    assert torch.equal(r.fig_opl[keep], want.fig_opl[keep]) and torch.equal(r.opl[keep], want.opl[keep])


def test_refused_entry_points(gpu):
    """the four entry points with no figure plumbing return AKB_E_ARG and launch nothing"""
    from akbraytracing_amd import _lib
    from akbraytracing_amd.trace import ChainLaunch
    g = _geom()
    maps, _ = _maps()
    th, tv = _tables(g, 17, gpu)
    L = _lib.lib()
    c = ChainLaunch(g.mirrors, tan_h=th, tan_v=tv, src=g.source, want=("opl", "fig_opl"), figure=maps)
    c.res.opl.fill_(7.0)
    c.res.fig_opl.fill_(7.0)
    d = c.desc
    z = ctypes.c_void_p(0)
    calls = [lambda: L.akb_trace_chain_dd_f64(d, None), lambda: L.akb_trace_chain_batch_f64(d, 1, None),
             lambda: L.akb_trace_chain_samples_f64(d, None),
             lambda: L.akb_chain_tilt_f64(d, z, z, z, z, z, z, 289, 289, z, z, z, z, z, z, None, None)]
    sink = _lib.LeafSink()
    calls[3] = lambda: L.akb_chain_tilt_f64(d, ctypes.c_void_p(8), z, z, z, z, z, 289, 289, z, z, z, z, z, z,
                                            ctypes.byref(sink), None)
    for f in calls:
        assert f() == -1
        assert b"figure maps" in L.akb_last_error()
    # fig_out alone is refused too
    d2 = ChainLaunch(g.mirrors, tan_h=th, tan_v=tv, src=g.source, want=("opl", "fig_opl")).desc
    assert L.akb_trace_chain_dd_f64(d2, None) == -1
    torch.cuda.synchronize()
    assert bool((c.res.opl == 7.0).all()) and bool((c.res.fig_opl == 7.0).all()) and int(c.res.flags.item()) == 0
    # and the Python layer refuses the double-double chain with maps before any call
    with pytest.raises(ValueError, match="double-double"):
        ChainLaunch(g.mirrors, tan_h=th, tan_v=tv, src=g.source, want=("opl",), figure=maps, precision="dd")


def test_plot_result_ray_wave_with_figure(gpu, tmp_path):
    """the driver at 33 x 33: finite results, a 1-D sinusoid on one mirror moves the Legendre terms,
    and without figure the files are byte-identical to a run that never heard of it"""
    from akbraytracing_amd import geometry as G
    from akbraytracing_amd.driver import plot_result_ray_wave, ray_wave_conditions
    from akbraytracing_amd.figure import FigureMap, mirror_frames
    from akbraytracing_amd.wavefront import SystemGeometry
    from test_driver import _best_params
    params = _best_params()
    b = G.build_akb(params)
    det2 = np.zeros(10)
    det2[6] = 1
    det2[9] = -(np.float64(b["s2f_middle"]) + np.float64(b["defocus"]) + ray_wave_conditions()[0])
    fr = mirror_frames(SystemGeometry.from_dict(dict(b, det2=[float(x) for x in det2])))[0]
    u = np.linspace(-0.5, 0.5, 401)  # a metre-long 1-D profile: covers any footprint on the mirror
    fig = [FigureMap.from_profile(u, 2e-9 * np.sin(2 * np.pi * u / 0.05), fr), None, None, None]
    dirs = [tmp_path / s for s in ("a", "b", "c")]
    for d in dirs:
        d.mkdir()
    plain = plot_result_ray_wave(params, 33, directory=str(dirs[0]), workdir=str(dirs[0]), verbose=False)
    again = plot_result_ray_wave(params, 33, directory=str(dirs[1]), workdir=str(dirs[1]), verbose=False, figure=None)
    got = plot_result_ray_wave(params, 33, directory=str(dirs[2]), workdir=str(dirs[2]), verbose=False, figure=fig)
    for a in got:
        assert np.all(np.isfinite(a))
    assert np.array_equal(got[1], plain[1]) and not np.array_equal(got[0], plain[0])
    names = sorted(os.listdir(dirs[0]))
    assert names == sorted(os.listdir(dirs[1])) and names
    for f in names:
        assert (dirs[0] / f).read_bytes() == (dirs[1] / f).read_bytes(), f
