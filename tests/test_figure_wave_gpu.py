"""Figure maps in the wave chain on the device: the stage kernel akb_figure_displace_f64
against the host build of csrc/akb_figure.h (bit for bit), plot_result_wave / kb_wave / saveWaveData with
figure= against the composition by hand and against the figure-free run, and run_wave_chain on a file
set written with maps.

All grids are 33 x 33 = 1089 samples (four full 256-lane workgroups plus a tail); maps are at most 64 x 8."""
import ctypes
import os
import warnings

import numpy as np
import pytest
import torch

import figure_wave_host as FW
import oracle as O
from conftest import golden
from figure_maps import make_maps

pytestmark = pytest.mark.gpu

N = 33
SHAPES = [(4, 4), (7, 5), (1, 9), (9, 1), (8, 64)]  # (nw, nu); the last is the 64 x 8 map
STAMP = "20250101_000000"

_CACHE = {}


def _setup(kind, gpu):
    """the built system, pass 2's hits of the 33 x 33 'wave' trace (the shared footprint), each mirror's
    incoming directions by displace_hits' rule, the frames and the maps"""
    if kind in _CACHE:
        return _CACHE[kind]
    from akbraytracing_amd import geometry as G
    from akbraytracing_amd.figure import mirror_frames
    from akbraytracing_amd.wavedata import two_pass_trace
    if kind == "akb":
        params = golden("akb_autofocus.npz")["g0_params"]
        b = G.build_akb(params)
    else:
        params = golden("kb_savewave_33.npz")["params"]
        b = G.build_kb(params)
    mir = G.mirrors_of(b)
    K = len(mir)
    hits, refl, det = two_pass_trace(b, N, "wave")
    src = torch.tensor([float(x) for x in b["source"]], dtype=torch.float64, device=gpu).reshape(3, 1)
    dirs = [(hits[k] - (src if k == 0 else hits[k - 1])).contiguous() for k in range(K)]
    frames = mirror_frames(b)
    hn = hits.cpu().numpy()
    full = make_maps(frames, hn, SHAPES[:K] if K == 4 else [(7, 5), (1, 9)])
    some = make_maps(frames, hn, [None, (4, 4), None, (9, 1)] if K == 4 else [None, (7, 5)])
    S = dict(params=params, b=b, mir=mir, K=K, hits=hits, refl=refl, det=det, dirs=dirs, frames=frames, hn=hn, full=full,
             some=some, src=src)
    _CACHE[kind] = S
    return S


def _one_map(fr, hn, shp, margin=0.25):
    """make_maps for one mirror, in its second slot: the first slot's phase is zero, and with it a map of
    one sample along u"""
    return make_maps([fr, fr], [hn, hn], [None, shp], margin=margin)[1]


def _device(fm, coeffs, hit, dirs):
    from akbraytracing_amd.figure import displace
    p, fl, h = displace(fm, coeffs, hit, dirs, want_height=True)
    q, fl2 = displace(fm, coeffs, hit, dirs)  # the h_out = NULL path
    assert fl2 == fl and np.array_equal(p.cpu().numpy(), q.cpu().numpy(), equal_nan=True)
    return p.cpu().numpy(), h.cpu().numpy(), fl


@pytest.mark.parametrize("kind", ["akb", "kb"])
def test_stage_kernel_equals_host_build(gpu, kind):
    """akb_figure_displace_f64 == the g++ build of the header, points and h_out bit for bit, on every
    mirror's pass-2 hits with every map shape; with a map covering half the footprint (the flag, the
    outside samples untouched bit for bit) and with a NaN column (NaN out, no flag)"""
    S = _setup(kind, gpu)
    for k, m in enumerate(S["mir"]):
        hit, dirs = S["hits"][k].contiguous(), S["dirs"][k]
        hn, dn = hit.cpu().numpy(), dirs.cpu().numpy()
        for shp in SHAPES:
            fm = _one_map(S["frames"][k], hn, shp)
            got, h, fl = _device(fm, m.coeffs, hit, dirs)
            want = FW.host_stage(fm, m.coeffs, hn, dn)
            assert fl == want["flags"] == 0, (k, shp, fl)
            assert got.tobytes() == want["points"].tobytes() and h.tobytes() == want["h"].tobytes(), (k, shp)
            assert np.any(got != hn, axis=0).mean() > 0.9  # the maps do something
        # half the footprint
        half = _one_map(S["frames"][k], hn, (7, 5), margin=-0.25)
        got, h, fl = _device(half, m.coeffs, hit, dirs)
        want = FW.host_stage(half, m.coeffs, hn, dn)
        o = want["outside"]
        assert fl == want["flags"] == 8 and 0.2 < o.mean() < 0.95
        assert got.tobytes() == want["points"].tobytes() and h.tobytes() == want["h"].tobytes()
        assert got[:, o].tobytes() == hn[:, o].tobytes() and np.all(h[o] == 0.0) and not np.signbit(h[o]).any()
        assert np.any(got[:, ~o] != hn[:, ~o], axis=0).mean() > 0.9
        # a NaN column
        bad = hit.clone()
        bad[:, 700] = float("nan")
        got, h, fl = _device(S["full"][k], m.coeffs, bad, dirs)
        want = FW.host_stage(S["full"][k], m.coeffs, bad.cpu().numpy(), dn)
        assert fl == want["flags"] == 0
        assert np.array_equal(got, want["points"], equal_nan=True) and np.array_equal(h, want["h"], equal_nan=True)
        assert np.isnan(got[:, 700]).all() and np.isnan(h[700]) and np.isfinite(np.delete(got, 700, axis=1)).all()


def test_refusals(gpu):
    """out overlapping hit or dir, a map without a table, a frame that is not orthonormal and a
    non-positive pitch are refused before anything is launched"""
    from akbraytracing_amd import _lib, device as D
    S = _setup("kb", gpu)
    L = _lib.lib()
    fm, m = S["full"][0], S["mir"][0]
    n = N * N
    buf = torch.zeros(3 * n + 7, dtype=torch.float64, device=gpu)
    hit, dirs = S["hits"][0].contiguous(), S["dirs"][0]
    out = torch.full((3, n), 7.0, dtype=torch.float64, device=gpu)
    fl = torch.zeros(1, dtype=torch.int32, device=gpu)
    c = D.host_f64(m.coeffs)
    esz = 8

    def call(desc, hp, dp, op):
        return L.akb_figure_displace_f64(desc, c, hp, n, dp, n, n, op, n, None, D.ptr(fl), D.stream_handle())

    desc = fm.desc(gpu)
    buf[:3 * n] = hit.reshape(-1)
    shifted = ctypes.c_void_p(buf.data_ptr() + 7 * esz)  # seven elements into the same block
    for hp, dp, op in ((D.ptr(hit), D.ptr(dirs), D.ptr(hit)), (D.ptr(hit), D.ptr(dirs), D.ptr(dirs)),
                       (D.ptr(buf), D.ptr(dirs), shifted), (shifted, D.ptr(dirs), D.ptr(buf)),
                       (D.ptr(hit), D.ptr(buf), shifted)):
        assert call(desc, hp, dp, op) == -1 and b"overlap" in L.akb_last_error()
    assert call(desc, D.ptr(hit), D.ptr(dirs), D.ptr(out)) == 0
    torch.cuda.synchronize()
    assert bool((out != 7.0).all())
    out.fill_(7.0)
    bad = fm.desc(gpu)
    bad.table = None
    assert call(bad, D.ptr(hit), D.ptr(dirs), D.ptr(out)) == -1 and b"table" in L.akb_last_error()
    bad = fm.desc(gpu)
    bad.e_u[0] = bad.e_u[0] + 1e-6
    assert call(bad, D.ptr(hit), D.ptr(dirs), D.ptr(out)) == -1 and b"axes" in L.akb_last_error()
    bad = fm.desc(gpu)
    bad.du = 0.0
    assert call(bad, D.ptr(hit), D.ptr(dirs), D.ptr(out)) == -1 and b"pitch" in L.akb_last_error()
    assert L.akb_figure_displace_f64(desc, c, D.ptr(hit), n - 1, D.ptr(dirs), n, n, D.ptr(out), n, None, D.ptr(fl),
                                     D.stream_handle()) == -1
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and int(fl.item()) == 0


def _wave(kind, S, **kw):
    from akbraytracing_amd import wavedata as W
    if kind == "akb":
        return W.plot_result_wave(S["params"], N, **kw)
    return W.kb_wave(S["params"], N, **kw)


# where each mirror (trace order) stands in the returned tuple
SLOTS = dict(akb=(1, 3, 4, 2), kb=(1, 2))


def _same(a, b):
    if isinstance(a, np.ndarray):
        return isinstance(b, np.ndarray) and a.shape == b.shape and a.tobytes() == b.tobytes()
    return a == b


@pytest.mark.parametrize("kind", ["akb", "kb"])
def test_wave_mode_with_figure(gpu, kind):
    """the mirror grids equal rotate_points(displace(...)) composed by hand from the two-pass trace, bit
    for bit; every other entry of the tuple is the figure=None call's; figure=[None] * K is the
    no-argument call; a callable gives its list's result; a map that does not cover the footprint raises
    AKBError naming the mirror"""
    from akbraytracing_amd import _lib, primitives as P
    from akbraytracing_amd.figure import displace, displace_hits
    from akbraytracing_amd.reduce import means_to_host, np_sum
    S = _setup(kind, gpu)
    K = S["K"]
    free = _wave(kind, S)
    none = _wave(kind, S, figure=[None] * K)
    assert len(free) == len(none) and all(_same(a, b) for a, b in zip(free, none))
    ang = S["refl"].cpu().numpy()
    theta_y = -np.mean(np.arctan(ang[2, :] / ang[0, :]))
    theta_z = np.mean(np.arctan(ang[1, :] / ang[0, :]))
    (focus,) = means_to_host([np_sum(S["det"])])
    for maps in (S["full"], S["some"]):
        got = _wave(kind, S, figure=maps)
        assert len(got) == len(free)
        moved, word = displace_hits(S["mir"], maps, [S["hits"][k] for k in range(K)], S["b"]["source"])
        assert word == 0
        for k in range(K):
            slot = SLOTS[kind][k]
            if maps[k] is None:
                assert moved[k] is S["hits"][k] or torch.equal(moved[k], S["hits"][k])
                assert _same(got[slot], free[slot]), k
                continue
            p, fl = displace(maps[k], S["mir"][k].coeffs, S["hits"][k], S["dirs"][k])
            assert fl == 0 and torch.equal(p, moved[k])
            want = P.rotate_points(p, focus, -theta_y, -theta_z).cpu().numpy()
            assert _same(got[slot], want), k
            assert not _same(got[slot], free[slot])
        for i in range(len(free)):
            if i not in SLOTS[kind]:
                assert _same(got[i], free[i]), i
        if maps is S["full"]:
            calls = []

            def figure(b, maps=maps):
                calls.append(b)
                return maps
            via = _wave(kind, S, figure=figure)
            assert len(calls) == 1 and isinstance(calls[0], dict) and all(_same(a, b) for a, b in zip(via, got))
    short = make_maps(S["frames"], S["hn"], [None] * (K - 1) + [(7, 5)], margin=-0.25)
    with pytest.raises(_lib.AKBError, match=f"figure map of mirror {K - 1}"):
        _wave(kind, S, figure=short)
    with pytest.raises(ValueError, match="one entry"):
        _wave(kind, S, figure=S["full"][:1])


@pytest.mark.parametrize("kind", ["akb", "kb"])
@pytest.mark.parametrize("run", ["plain", "thin"])
def test_save_wave_data_with_figure(gpu, tmp_path, kind, run):
    """saveWaveData(figure=maps) beside the figure-free set written with the same timestamp, plain and with
    the fixtures' downsample factors: the source, both grids, the conditions text and the unmapped
    mirrors' files byte for byte; a mapped mirror's rows 0-2 the (downsampled) displaced grid, row 3
    calc_dS of those rows, bit for bit"""
    from akbraytracing_amd import wavedata as W
    S = _setup(kind, gpu)
    f = golden("savewave_33.npz" if kind == "akb" else "kb_savewave_33.npz")
    down = tuple(int(x) for x in f[f"{run}_downsample"])
    kw = dict(ray_num_H=N, defocus_for_wave=float(f["defocusForWave"]), downsample=down, timestamp=STAMP,
              option_AKB=kind == "akb")
    maps = S["some"]
    with warnings.catch_warnings():
        warnings.filterwarnings("error", message=".*aliased")  # maps this coarse are sampled finely
        a = W.saveWaveData(S["params"], directory=str(tmp_path / "free"), **kw)
        b = W.saveWaveData(S["params"], directory=str(tmp_path / "fig"), figure=maps, **kw)
    assert sorted(os.listdir(a)) == sorted(os.listdir(b))

    def raw(folder, name):
        with open(os.path.join(folder, name), "rb") as fh:
            return fh.read()
    for name in ("points_source.npy", "points_gridImage.npy", "points_gridDefocus.npy", "calculation_conditions.txt"):
        assert raw(a, name) == raw(b, name), name
    tup = _wave(kind, S, figure=maps, defocus_for_wave=kw["defocus_for_wave"])
    h1, v1, h2, v2 = down[:4]
    # file number, tuple slot and downsample factors per mirror in trace order
    files = ((1, 1, h1, v1), (3, 3, h1, v1), (4, 4, h2, v2), (2, 2, h2, v2)) if kind == "akb" else ((1, 1, h1, v1), (2, 2, h2, v2))
    for k, (m, slot, dh, dv) in enumerate(files):
        name = f"points_M{m}.npy"
        if maps[k] is None:
            assert raw(a, name) == raw(b, name), name
            continue
        got = np.load(os.path.join(b, name))
        grid, nv, nh = W.downsample_array_3_n(tup[slot], N, N, dh, dv)
        assert got.shape == (4, nv * nh) and got[:3].tobytes() == grid.tobytes(), name
        ds = W.calc_dS(np.ascontiguousarray(got[:3]), nv, nh)
        assert got[3].tobytes() == ds.ravel().tobytes(), name
        assert raw(a, name) != raw(b, name)
        assert not np.array_equal(got[3], np.load(os.path.join(a, name))[3])  # dS follows the displaced grid


def test_save_wave_data_warns_when_the_grid_aliases_the_map(gpu, tmp_path):
    """a 64 x 8 map over a 33 x 33 footprint has a pitch below the sample spacing along e_u: one warning
    naming the mirror, and the same files as without the warning filter"""
    from akbraytracing_amd import wavedata as W
    S = _setup("kb", gpu)
    fine = make_maps(S["frames"], S["hn"], [None, (8, 64)])
    f = golden("kb_savewave_33.npz")
    with pytest.warns(UserWarning, match=r"mirror 1 \(points_M2\.npy\).*along e_u.*aliased") as rec:
        W.saveWaveData(S["params"], directory=str(tmp_path / "w"), ray_num_H=N, defocus_for_wave=float(f["defocusForWave"]),
                       timestamp=STAMP, option_AKB=False, figure=fine)
    assert len([r for r in rec if "aliased" in str(r.message)]) == 1


def test_wave_chain_on_a_figure_set(gpu, tmp_path):
    """run_wave_chain on the KB pair's file set written with maps on both mirrors runs to the end with
    finite fields; its M1 field is the point source's exp(-ikr) / r at the saved displaced points (the
    oracle's sum, to the 1e-9 of max |u| of tests/test_wavecalc_gpu.py's M1 stage); the image differs
    from the figure-free run's"""
    from akbraytracing_amd import wavedata as W
    S = _setup("kb", gpu)
    f = golden("kb_savewave_33.npz")
    kw = dict(ray_num_H=N, defocus_for_wave=float(f["defocusForWave"]), timestamp=STAMP, option_AKB=False)
    a = W.saveWaveData(S["params"], directory=str(tmp_path / "free"), **kw)
    b = W.saveWaveData(S["params"], directory=str(tmp_path / "fig"), figure=S["full"], **kw)
    free = W.run_wave_chain(a, None, resume_dir=None)
    fig = W.run_wave_chain(b, None, resume_dir=None)
    assert sorted(fig) == ["Image", "Image2", "M1", "M2"]
    for name, u in fig.items():
        assert np.isfinite(u).all() and np.abs(u).max() > 0, name
    m1 = np.load(os.path.join(b, "points_M1.npy"))
    assert not np.array_equal(m1[:3], np.load(os.path.join(a, "points_M1.npy"))[:3])
    src = np.load(os.path.join(b, "points_source.npy")).reshape(3, 1)
    k = 2 * np.pi / 13.5e-9
    want = O.huygens_c(m1[0], m1[1], m1[2], src[0], src[1], src[2], np.ones(1, complex), k)
    assert np.max(np.abs(fig["M1"] - want)) <= 1e-9 * np.max(np.abs(want))
    assert not np.array_equal(fig["Image"], free["Image"])
    assert not np.array_equal(fig["M1"], free["M1"])
