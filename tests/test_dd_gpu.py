"""The double-double (option_mpmath) path on the device: the two stage kernels against the host
build of the same header (bit for bit), the fused chain against the staged composition (bit for
bit), and RayWave / the driver / install() against the reference's recorded mpmath run and the
exact run of tests/golden/akb_mpmath_17.npz (make_golden_mpmath.py)."""
import os
import types

import numpy as np
import pytest
import torch

import dd_host as H
from conftest import golden_json

pytestmark = pytest.mark.gpu

NM_BAR = 1e-4  # nm: the project's bar on DistError2 / Wave2 against the reference


def _same(a, b):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    b = b.cpu().numpy() if isinstance(b, torch.Tensor) else np.asarray(b)
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def _view(a):
    a = np.ascontiguousarray(a, dtype=np.float64)
    if a.ndim == 1:
        return a, 1, 0
    return a, a.shape[1], (1 if a.shape[1] > 1 else 0)


def _dev_isect(coeffs, ray, source, negative, n):
    """akb_isect_dd_f64 through ctypes with explicit (ptr, ld, inc) views"""
    from akbraytracing_amd import _lib, device as D
    d, dld, dinc = _view(ray)
    o, old_, oinc = _view(source)
    td, to = D.to_dev(d), D.to_dev(o)
    out, fl = D.empty((3, n)), D.flags_tensor()
    _lib.check(_lib.lib().akb_isect_dd_f64(D.host_f64(coeffs), D.ptr(td), dld, dinc, D.ptr(to), old_, oinc,
                                           int(bool(negative)), n, D.ptr(out), n, D.ptr(fl), D.stream_handle()))
    return out.cpu().numpy(), int(fl.item())


def _dev_reflect(ray, nrm, n):
    from akbraytracing_amd import _lib, device as D
    d, dld, dinc = _view(ray)
    v, vld, vinc = _view(nrm)
    td, tv = D.to_dev(d), D.to_dev(v)
    out, fl = D.empty((3, n)), D.flags_tensor()
    _lib.check(_lib.lib().akb_reflect_dd_f64(D.ptr(td), dld, dinc, D.ptr(tv), vld, vinc, n, D.ptr(out), n, D.ptr(fl),
                                             D.stream_handle()))
    return out.cpu().numpy(), int(fl.item())


# ---------------------------------------------------------------------------- stage kernels

def test_stage_kernels_match_the_host_build_on_the_fixture(gpu):
    """n = 289 (and the run's 3- and 4-column calls) through the Python layer, n = 1 from a column"""
    from akbraytracing_amd import extended as X
    for key, name, ins, neg, ref, _ in H.calls():
        if name == "mirr_ray_intersection":
            got = X.mirr_ray_intersection(ins[0], ins[1], ins[2], negative=neg)
            want, _ = H.host_isect(ins[0], ins[1], ins[2], neg)
            one = X.mirr_ray_intersection(ins[0], ins[1][:, 0], ins[2][:, 0], negative=neg)
        else:
            got = X.reflect_ray(ins[0], ins[1])
            want, _ = H.host_reflect(ins[0], ins[1])
            one = X.reflect_ray(ins[0][:, 0], ins[1][:, 0])
        assert isinstance(got, np.ndarray) and _same(got, want), key
        assert one.shape == (3, 1) and _same(one[:, 0], want[:, 0]), key  # (3,) in, (3, 1) out
    # torch in, torch out
    key, name, ins, neg, _, _ = next(c for c in H.calls() if c[4].shape[1] == 289)
    t = X.mirr_ray_intersection(ins[0], torch.from_numpy(ins[1]).to(gpu), torch.from_numpy(ins[2]).to(gpu), neg)
    assert isinstance(t, torch.Tensor) and t.is_cuda and _same(t, H.host_isect(ins[0], ins[1], ins[2], neg)[0])


def test_stage_kernels_second_grid_stride_iteration(gpu):
    """The launch caps its grid at 2048 workgroups of 256 threads: n = 2048 * 256 + 777 is not a
    multiple of 256 and sends the first 777 threads through a second iteration."""
    n = 2048 * 256 + 777
    key, name, ins, neg, _, _ = next(c for c in H.calls() if c[1] == "mirr_ray_intersection" and c[3]
                                     and c[4].shape[1] == 289)
    rng = np.random.default_rng(5)
    ray = np.resize(ins[1], (3, n)) * (1.0 + 1e-7 * rng.standard_normal((3, n)))
    src = np.resize(ins[2], (3, n)) + 1e-6 * rng.standard_normal((3, n))
    got, fl = _dev_isect(ins[0], ray, src, neg, n)
    want, hfl = H.host_isect(ins[0], ray, src, neg)
    assert fl == hfl and _same(got, want)
    assert not np.isnan(got[:, -1]).any()  # the tail was written
    nrm = rng.standard_normal((3, n))
    nrm /= np.linalg.norm(nrm, axis=0)
    got, fl = _dev_reflect(ray, nrm, n)
    want, hfl = H.host_reflect(ray, nrm)
    assert fl == hfl == 0 and _same(got, want)


def test_stage_kernels_broadcast_views(gpu):
    """inc = 0 for the direction and for the origin (one vector for every column)"""
    key, name, ins, neg, _, _ = next(c for c in H.calls() if c[1] == "mirr_ray_intersection" and c[4].shape[1] == 289)
    n = 289
    d0, s0 = ins[1][:, 144].copy(), ins[2][:, 144].copy()
    got, _ = _dev_isect(ins[0], d0, ins[2], neg, n)
    assert _same(got, H.host_isect(ins[0], d0, ins[2], neg, n)[0])
    assert _same(got, H.host_isect(ins[0], np.repeat(d0[:, None], n, axis=1), ins[2], neg)[0])
    got, _ = _dev_isect(ins[0], ins[1], s0, neg, n)
    assert _same(got, H.host_isect(ins[0], ins[1], s0, neg, n)[0])
    assert _same(got, H.host_isect(ins[0], ins[1], np.repeat(s0[:, None], n, axis=1), neg)[0])
    key, name, rins, _, _, _ = next(c for c in H.calls() if c[1] == "reflect_ray" and c[4].shape[1] == 289)
    got, _ = _dev_reflect(rins[0][:, 7].copy(), rins[1], n)
    assert _same(got, H.host_reflect(np.repeat(rins[0][:, 7:8], n, axis=1), rins[1])[0])
    got, _ = _dev_reflect(rins[0], rins[1][:, 7].copy(), n)
    assert _same(got, H.host_reflect(rins[0], np.repeat(rins[1][:, 7:8], n, axis=1))[0])


def test_stage_kernels_value_rules_per_column(gpu):
    """two missing columns and one zero-norm column: flags set, the neighbours untouched"""
    from akbraytracing_amd import _lib
    n = 300
    rng = np.random.default_rng(9)
    sphere = [1, 1, 1, 0, 0, 0, 0, 0, 0, -1]
    ray = np.zeros((3, n))
    ray[0] = 1.0
    src = np.stack([np.full(n, -5.0), rng.uniform(-0.9, 0.9, n), rng.uniform(-0.3, 0.3, n)])
    src[1, 17] = 1.5     # misses
    src[1, 256] = -2.25  # misses (second workgroup)
    src[1:, 100] = [1.0, 0.0]  # tangent: D == 0 hits
    got, fl = _dev_isect(sphere, ray, src, False, n)
    want, hfl = H.host_isect(sphere, ray, src)
    assert fl == hfl == _lib.FLAG_MISS and _same(got, want)
    miss = np.isnan(got).any(axis=0)
    assert list(np.flatnonzero(miss)) == [17, 256] and np.all(np.isnan(got[:, miss]))
    assert np.array_equal(got[:, 100], [0.0, 1.0, 0.0])
    clean = src.copy()
    clean[1, [17, 256]] = 0.25
    ref, fl0 = _dev_isect(sphere, ray, clean, False, n)
    assert fl0 == 0 and np.array_equal(ref[:, ~miss], got[:, ~miss])
    d = rng.standard_normal((3, n))
    nrm = rng.standard_normal((3, n))
    nrm /= np.linalg.norm(nrm, axis=0)
    d[:, 41] = 0.0
    got, fl = _dev_reflect(d, nrm, n)
    want, hfl = H.host_reflect(d, nrm)
    assert fl == hfl == _lib.FLAG_ZERO_REFLECT and _same(got, want)
    assert np.array_equal(got[:, 41], [0.0, 0.0, 0.0])
    assert np.allclose(np.linalg.norm(np.delete(got, 41, axis=1), axis=0), 1.0, rtol=0, atol=1e-15)


# ---------------------------------------------------------------------------- fused chain

def _system(name, n=33):
    from akbraytracing_amd.wavefront import SystemGeometry
    g = SystemGeometry.from_dict(golden_json(name))
    tan_h = torch.from_numpy(np.tan(g.angle_h.table(n))).cuda()
    tan_v = torch.from_numpy(np.tan(g.angle_v.table(n))).cuda()
    return g, tan_h, tan_v


def _atan_slope(x):
    """the trace's arctan of a slope row (akb_selftest_arith_f64's column 9)"""
    from akbraytracing_amd import _lib, device as D
    x = x.contiguous()
    out = torch.empty((x.shape[0], 13), dtype=torch.float64, device=x.device)
    _lib.check(_lib.lib().akb_selftest_arith_f64(D.ptr(x), D.ptr(x), x.shape[0], D.ptr(out), D.stream_handle()))
    return out[:, 9].contiguous()


def _staged(g, dirs, org):
    """the staged composition: double-double intersection and reflection (extended.prims), the
    existing float64 stage kernels for everything else"""
    from akbraytracing_amd import extended as X, primitives as P
    from akbraytracing_amd.trace import staged_chain
    hits, ray, segs = staged_chain(g.mirrors, dirs, org, with_segments=True, prims=X.prims)
    opl = segs[0]
    for s in segs[1:]:
        opl = opl + s
    det = P.plane_ray_intersection([0] * 6 + list(g.det1), ray, hits[-1])
    return dict(hits=torch.stack(hits), last_hit=hits[-1], dir_out=ray, opl=opl, det=det,
                atan=torch.stack([_atan_slope(ray[1] / ray[0]), _atan_slope(ray[2] / ray[0])]),
                slope_h=ray[1] / ray[0], slope_v=ray[2] / ray[0])


WANT = ("hits", "last_hit", "dir_out", "det", "opl", "atan")


def _check_chain(r, want, sl=slice(None)):
    assert int(r.flags.item()) == 0
    assert _same(r.hits, want["hits"][:, :, sl])
    for k in ("last_hit", "dir_out", "det", "atan"):
        assert _same(getattr(r, k), want[k][:, sl]), k
    assert _same(r.opl, want["opl"][sl])


@pytest.fixture(scope="module")
def akb33(gpu):
    """the AKB's four mirrors (minus root on the last) on a 33 x 33 grid: geometry, tables, explicit
    directions, constant origin block and the staged composition's outputs (computed once, read-only)"""
    from akbraytracing_amd.trace import grid_dirs
    g, tan_h, tan_v = _system("akb_geometry.json")
    assert len(g.mirrors) == 4 and g.mirrors[-1].negative
    dirs = grid_dirs(tan_h, tan_v)
    org = torch.tensor(g.source, dtype=torch.float64, device=gpu).reshape(3, 1).expand(3, 33 * 33).contiguous()
    return g, tan_h, tan_v, dirs, org, _staged(g, dirs, org)


def test_chain_matches_the_staged_composition_akb(akb33):
    from akbraytracing_amd.trace import trace_chain
    from akbraytracing_amd.wavefront import sample_plan
    g, tan_h, tan_v, dirs, org, want = akb33
    hb, he, col = sample_plan(33)
    r = trace_chain(g.mirrors, tan_h=tan_h, tan_v=tan_v, src=g.source, det_ghij=g.det1, want=WANT,
                    samples=(hb, he, col), precision="dd")
    _check_chain(r, want)
    assert _same(r.samp_h, want["slope_h"][hb:he])
    assert _same(r.samp_v, want["slope_v"][col::33])
    # explicit directions give the same bits
    e = trace_chain(g.mirrors, dirs=dirs, src=g.source, det_ghij=g.det1, want=WANT, precision="dd")
    _check_chain(e, want)
    # and the double-double chain is not the float64 chain
    f = trace_chain(g.mirrors, tan_h=tan_h, tan_v=tan_v, src=g.source, want=("last_hit",))
    assert not _same(f.last_hit, r.last_hit)


def test_chain_window_starting_mid_row(akb33):
    from akbraytracing_amd.trace import trace_chain
    g, tan_h, tan_v, dirs, org, want = akb33
    ray0, cnt = 5 * 33 + 7, 300
    hb, he, col = 160, 200, 16  # the pick range starts before the window
    r = trace_chain(g.mirrors, tan_h=tan_h, tan_v=tan_v, ray0=ray0, n_rays=cnt, src=g.source, det_ghij=g.det1,
                    want=WANT, samples=(hb, he, col), precision="dd")
    _check_chain(r, want, slice(ray0, ray0 + cnt))
    lo, hi = max(hb, ray0), min(he, ray0 + cnt)
    assert _same(r.samp_h[lo - hb:hi - hb], want["slope_h"][lo:hi])
    assert torch.isnan(r.samp_h[:lo - hb]).all()
    rows = [iv for iv in range(33) if ray0 <= iv * 33 + col < ray0 + cnt]
    assert _same(r.samp_v[rows], want["slope_v"][col::33][rows])
    other = [iv for iv in range(33) if iv not in rows]
    assert torch.isnan(r.samp_v[other]).all()  # rays outside the window are not traced


def test_chain_per_ray_origins(akb33, gpu):
    from akbraytracing_amd.trace import trace_chain
    g, tan_h, tan_v, dirs, org, _ = akb33
    gen = torch.Generator(device="cpu").manual_seed(3)
    org2 = (org.cpu() + 1e-7 * torch.randn(org.shape, generator=gen, dtype=torch.float64)).to(gpu)
    want = _staged(g, dirs, org2)
    r = trace_chain(g.mirrors, tan_h=tan_h, tan_v=tan_v, src=org2, det_ghij=g.det1, want=WANT, precision="dd")
    _check_chain(r, want)
    e = trace_chain(g.mirrors, dirs=dirs, src=org2, det_ghij=g.det1, want=WANT, precision="dd")
    _check_chain(e, want)


def test_chain_matches_the_staged_composition_kb(gpu):
    from akbraytracing_amd.trace import grid_dirs, trace_chain
    g, tan_h, tan_v = _system("kb_geometry.json")
    assert len(g.mirrors) == 2
    dirs = grid_dirs(tan_h, tan_v)
    org = torch.tensor(g.source, dtype=torch.float64, device=gpu).reshape(3, 1).expand(3, 33 * 33).contiguous()
    want = _staged(g, dirs, org)
    r = trace_chain(g.mirrors, tan_h=tan_h, tan_v=tan_v, src=g.source, det_ghij=g.det1, want=WANT, precision="dd")
    _check_chain(r, want)
    e = trace_chain(g.mirrors, dirs=dirs, src=g.source, det_ghij=g.det1, want=WANT, precision="dd")
    _check_chain(e, want)


def test_chain_refuses_descriptor_fields_it_does_not_implement(akb33, gpu):
    from akbraytracing_amd import _lib, device as D
    from akbraytracing_amd.reduce import LeafSink
    from akbraytracing_amd.trace import ChainLaunch
    g, tan_h, tan_v, dirs, org, _ = akb33
    L = _lib.lib()
    n = 33 * 33
    buf = torch.zeros(64, dtype=torch.float64, device=gpu)
    pert = torch.zeros((1, 33), dtype=torch.float64, device=gpu)
    sink = LeafSink(5, n, 0b00011, gpu)

    def launch():
        return ChainLaunch(g.mirrors, tan_h=tan_h, tan_v=tan_v, src=g.source, det_ghij=g.det1,
                           want=("last_hit", "opl"), precision="dd")
    for what in ("copy", "pert", "sink"):
        c = launch()
        c.res.last_hit.fill_(7.0)
        if what == "copy":
            c.desc.copy_src, c.desc.copy_dst, c.desc.copy_n = D.ptr(buf), D.ptr(buf[32:]), 8
        elif what == "pert":
            c.desc.pert_h, c.desc.pert_v, c.desc.pert_terms = D.ptr(pert), D.ptr(pert), 1
        else:
            c.desc.sink = sink.desc
        st = L.akb_trace_chain_dd_f64(c.desc, D.stream_handle())
        assert st == -1, what  # AKB_E_ARG
        assert b"not implemented" in L.akb_last_error(), what
        torch.cuda.synchronize()
        assert bool((c.res.last_hit == 7.0).all()), what  # nothing was launched
        assert L.akb_trace_chain_f64(c.desc, D.stream_handle()) == 0, what  # the float64 chain takes the field
    with pytest.raises(ValueError):
        ChainLaunch(g.mirrors, tan_h=tan_h, tan_v=tan_v, src=g.source, det_ghij=g.det1, want=("opl",), sink=sink,
                    precision="dd")


# ---------------------------------------------------------------------------- RayWave, driver, install

def _best_params():
    p = np.zeros(26)  # AKB_raytrace_20250312.py:14586-14592, the fixtures' params
    p[0], p[1], p[8], p[9], p[13] = -5.73452570e-03, -2.87624337e-03, 1.05000000e-02, -3.59399021e-05, 2.39536993e-06
    p[20], p[21], p[25] = 1.05000000e-02, -3.59399021e-05, 2.39536993e-06
    return p


def test_raywave_dd_resolves_the_aligned_wavefront(gpu):
    """DistError2 / Wave2 at 17 x 17 against the fixture's exact run (300-bit primitives) and the
    reference's own mpmath run; the float64 RayWave must miss the same bar.
    Measured on MI355X: double-double against the exact run 0.0 nm (both maps bit-equal), against the
    reference's mpmath run 5.7e-5 nm (that run's own distance from the exact one); float64 against the
    exact run 0.060 nm on a 0.083 nm wavefront."""
    from akbraytracing_amd import extended as X, geometry as G
    from akbraytracing_amd.driver import ray_wave_conditions
    from akbraytracing_amd.wavefront import RayWave, SystemGeometry
    f = H.fixture()
    b = G.build_akb(_best_params(), option_set=True, prims=X.prims)
    det2 = np.zeros(10)
    det2[6] = 1
    det2[9] = -(np.float64(b["s2f_middle"]) + np.float64(b["defocus"]) + ray_wave_conditions(True)[0])
    sysg = SystemGeometry.from_dict(dict(b, det2=[float(x) for x in det2]))
    run = RayWave(sysg, 17, precision="dd").run()
    de2, w2 = run["dist_err2"].cpu().numpy(), run["wave2"].cpu().numpy()
    gap = f["exact_minus_ref_nm"]
    err = dict(de2_exact=np.max(np.abs(de2 - f["exact_dist_err2"])), w2_exact=np.max(np.abs(w2 - f["exact_wave2"])),
               de2_ref=np.max(np.abs(de2 - f["ref_dist_err2"])), w2_ref=np.max(np.abs(w2 - f["ref_wave2"])))
    fp = RayWave(sysg, 17).run()
    fp_err = np.max(np.abs(fp["wave2"].cpu().numpy() - f["exact_wave2"]))
    print("dd RayWave vs the fixture (nm):", {k: float(v) for k, v in err.items()},
          "exact - reference run:", gap.tolist(), "Wave2 range:", float(np.ptp(f["exact_wave2"])),
          "float64 RayWave vs exact:", float(fp_err))
    assert err["de2_exact"] <= NM_BAR and err["w2_exact"] <= NM_BAR
    assert err["de2_ref"] <= NM_BAR + gap[0] and err["w2_ref"] <= NM_BAR + gap[1]
    assert fp_err > NM_BAR  # plain float64 cannot resolve it: the mode does something
    with pytest.raises(ValueError):
        RayWave(sysg, 17, comm=object(), precision="dd")
    from akbraytracing_amd.wavefront import Shard
    with pytest.raises(ValueError):
        RayWave(sysg, 17, shard=Shard(0, 289), precision="dd")


def _mode_run(n, flag, wd):
    """one plot_result_ray_wave call: (its result or the exception it raised, the files it wrote)"""
    from akbraytracing_amd.driver import plot_result_ray_wave
    wd.mkdir()
    try:
        res = plot_result_ray_wave(_best_params(), n, directory=str(wd / "out"), workdir=str(wd), verbose=False,
                                   option_mpmath=flag)
    except ValueError as e:
        res = e
    return res, sorted(os.path.relpath(os.path.join(r, x), wd) for r, _, fs in os.walk(wd) for x in fs)


def test_plot_result_ray_wave_option_mpmath(gpu, tmp_path):
    """The mode with option_mpmath=True returns finite (inner_products, orders, pvs) and writes the
    float64 call's files.

    At 17 x 17 the mode cannot return for either precision: extract_affine_square_region raises the
    reference's own ValueError (:1047-1119, "矩形が4点で検出できませんでした": the 17 x 17 pupil
    map's outline does not reduce to four corners; measured on MI355X, 16 points for the float64
    call and for the option_mpmath call alike). So at 17 x 17 this checks what can hold - both calls
    end the same way, having written the same files up to that step - and the finite return value
    is checked at 25 x 25, where the float64 call completes (so do 33 and 65)."""
    r64, f64 = _mode_run(17, False, tmp_path / "a17")
    rdd, fdd = _mode_run(17, True, tmp_path / "b17")
    assert fdd == f64 and len(fdd) >= 3
    if isinstance(r64, ValueError):
        assert isinstance(rdd, ValueError) and str(rdd) == str(r64)
    else:
        assert all(np.all(np.isfinite(np.asarray(x, dtype=float))) for x in rdd)
    r64, f64 = _mode_run(25, False, tmp_path / "a25")
    rdd, fdd = _mode_run(25, True, tmp_path / "b25")
    assert not isinstance(r64, ValueError) and not isinstance(rdd, ValueError)
    ip, orders, pvs = rdd
    assert len(ip) == len(orders) == len(pvs) - 1 > 0
    assert all(np.all(np.isfinite(np.asarray(x, dtype=float))) for x in (ip, orders, pvs))
    assert fdd == f64 and len(fdd) >= 7


def test_install_device_mpmath_routes_the_primitives(gpu):
    import akbraytracing_amd
    mod = types.ModuleType("fake_driver")
    mod.option_mpmath = True
    calls = []
    mod.mirr_ray_intersection = lambda *a, **k: calls.append("isect") or "orig"
    mod.reflect_ray = lambda *a, **k: calls.append("reflect") or "orig"
    akbraytracing_amd.install(mod, mpmath="device")
    exact = H.exact_outputs()
    for name in ("mirr_ray_intersection", "reflect_ray"):
        key, _, ins, neg, ref, refdev = next(c for c in H.calls() if c[1] == name)
        got = mod.mirr_ray_intersection(ins[0], ins[1], ins[2], negative=neg) if name == "mirr_ray_intersection" \
            else mod.reflect_ray(ins[0], ins[1])
        assert isinstance(got, np.ndarray) and got.shape == ref.shape
        assert np.all(H.ulp_dev(got, exact[key]) <= 1.0)
        assert np.all(H.ulp_dev(got, ref) <= refdev + 1.0)
        assert np.all(np.abs(got - exact[key]) <= np.abs(ref - exact[key]))
    assert not calls
    mod.option_mpmath = False  # the float64 kernels again
    akbraytracing_amd.uninstall(mod)
    assert mod.reflect_ray(1, 2) == "orig"
