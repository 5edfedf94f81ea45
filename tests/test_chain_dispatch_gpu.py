"""Every kernel that akb_trace_chain_f64 and akb_trace_chain_batch_f64 can launch (the table of
DESIGN 4.3; the fused pass 1 has tests of its own): the tables below mirror the dispatch, one case a
kernel instantiation and system.

The grid is n_h = 19 by n_v = 17, 323 rays: two 256-ray segments, the second partial, and unequal
sides so that a swapped row and column shows. Grid launches also run on the window ray0 = 5,
n_rays = 300, which starts inside a grid row. Explicit directions are the same 323 rays, per-ray
origins the constant source in every column. The references are the staged compositions
(trace.staged_chain, figure.stage_terms, figure.stage_normals), formed once per system; everything
is compared bit for bit but the arctan rows against np.arctan (2 ulp, test_gpu_parity's bar)."""
import numpy as np
import pytest
import torch

from conftest import golden, golden_json
from figure_maps import make_maps

pytestmark = pytest.mark.gpu

N_H, N_V = 19, 17
N = N_H * N_V
WINDOW = (5, 300)  # ray0, n_rays
SYSTEMS = ["akb_geometry.json", "kb_geometry.json"]
SHAPES = [(7, 5), (4, 4), (1, 9), (9, 1)]  # (nw, nu) of the maps
MAPS = ["none", "path", "deflect"]

_CACHE = {}


def _ulp_diff(a, b):
    return np.max(np.abs(a - b) / np.spacing(np.maximum(np.abs(a), np.abs(b))))


def _rows(hits, ray, opl, fig_opl, det1):
    from akbraytracing_amd import primitives as P
    hits = torch.stack(hits)
    det = P.plane_ray_intersection([0] * 6 + list(det1), ray, hits[-1])
    return dict(hits=hits, last_hit=hits[-1], dir_out=ray, opl=opl, fig_opl=fig_opl, det=det)


def _setup(name, gpu):
    """geometry, tables, and per kind of maps the staged rows of the full grid"""
    if name in _CACHE:
        return _CACHE[name]
    from akbraytracing_amd.figure import mirror_frames, stage_normals, stage_terms
    from akbraytracing_amd.trace import grid_dirs, staged_chain
    from akbraytracing_amd.wavefront import SystemGeometry
    g = SystemGeometry.from_dict(golden_json(name))
    th = torch.from_numpy(np.tan(g.angle_h.table(N_H))).to(gpu)
    tv = torch.from_numpy(np.tan(g.angle_v.table(N_V))).to(gpu)
    dirs0 = grid_dirs(th, tv)
    src = torch.tensor(g.source, dtype=torch.float64, device=gpu).reshape(3, 1).expand(3, N).contiguous()

    def total(segs):
        opl = segs[0]
        for s in segs[1:]:
            opl = opl + s
        return opl

    hits, ray, segs = staged_chain(g.mirrors, dirs0, src, with_segments=True)
    maps = make_maps(mirror_frames(g), torch.stack(hits).cpu().numpy(), SHAPES[:len(g.mirrors)])
    ref = {"none": _rows(hits, ray, total(segs), None, g.det1)}
    terms, word = stage_terms(g.mirrors, maps, hits, dirs0)
    assert word == 0
    ref["path"] = _rows(hits, ray, total(segs) + terms, terms, g.det1)
    dh, dray, dsegs, word, dterms = stage_normals(g.mirrors, maps, dirs0, src, with_segments=True, with_terms=True)
    assert word == 0 and not torch.equal(dray, ray)
    ref["deflect"] = _rows(dh, dray, total(dsegs) + dterms, dterms, g.det1)
    _CACHE[name] = dict(g=g, th=th, tv=tv, dirs0=dirs0, src=src, maps=maps, ref=ref, atan={})
    return _CACHE[name]


def _launch(S, maps, rays, source, want, window=None, sink=None):
    from akbraytracing_amd.trace import trace_chain
    g = S["g"]
    sl = slice(None) if window is None else slice(window[0], window[0] + window[1])
    if rays == "grid":
        kw = dict(tan_h=S["th"], tan_v=S["tv"])
        if window is not None:
            kw.update(ray0=window[0], n_rays=window[1])
    else:
        kw = dict(dirs=S["dirs0"][:, sl].contiguous())
    src = g.source if source == "point" else S["src"][:, sl].contiguous()
    return trace_chain(g.mirrors, src=src, det_ghij=g.det1, want=want, sink=sink,
                       figure=None if maps == "none" else S["maps"], figure_slope=maps == "deflect", **kw)


def _check(S, maps, r, want, window=None):
    """every requested row of r against the staged rows; the flag word"""
    sl = slice(None) if window is None else slice(window[0], window[0] + window[1])
    ref = S["ref"][maps]
    assert int(r.flags.item()) == 0
    for f in want:
        if f == "atan":
            continue
        got = getattr(r, f)
        assert got is not None and torch.equal(got, ref[f][..., sl]), f
    if "atan" in want:
        at = r.atan.cpu().numpy()
        first = S["atan"].setdefault(maps, np.full((2, N), np.nan))
        fresh = np.isnan(first[:, sl])
        first[:, sl] = np.where(fresh, at, first[:, sl])
        assert np.array_equal(at, first[:, sl])  # the same bits from every kernel
        d = ref["dir_out"][:, sl].cpu().numpy()
        assert _ulp_diff(at[0], np.arctan(d[1] / d[0])) <= 2 and _ulp_diff(at[1], np.arctan(d[2] / d[0])) <= 2


def _windows(rays):
    return (None, WINDOW) if rays == "grid" else (None,)


def _id(v):
    if isinstance(v, bool):
        return "y" if v else "n"
    return str(v).replace("_geometry.json", "")


# rows, no maps (k_chain): (rays, opl, hits, source)
ROWS = [(rays, opl, hits, "point") for rays in ("grid", "explicit") for opl in (True, False) for hits in (True, False)]
ROWS += [("grid", opl, False, "per-ray") for opl in (True, False)]


@pytest.mark.parametrize("name", SYSTEMS, ids=_id)
@pytest.mark.parametrize("rays,opl,hits,source", ROWS, ids=_id)
def test_rows(gpu, name, rays, opl, hits, source):
    S = _setup(name, gpu)
    want = ("last_hit", "dir_out", "det", "atan") + (("opl",) if opl else ()) + (("hits",) if hits else ())
    for w in _windows(rays):
        r = _launch(S, "none", rays, source, want, window=w)
        assert (r.opl is None) == (not opl) and (r.hits is None) == (not hits)
        _check(S, "none", r, want, window=w)


# rows, maps (k_chain_fig): (rays, hits, maps, opl); the path term alone always comes with opl
ROWS_FIG = [(rays, hits, maps, opl) for rays in ("grid", "explicit") for hits in (True, False)
            for maps, opl in (("path", True), ("deflect", True), ("deflect", False))]


@pytest.mark.parametrize("name", SYSTEMS, ids=_id)
@pytest.mark.parametrize("rays,hits,maps,opl", ROWS_FIG, ids=_id)
def test_rows_with_maps(gpu, name, rays, hits, maps, opl):
    S = _setup(name, gpu)
    want = ("last_hit", "dir_out", "det", "atan") + (("opl", "fig_opl") if opl else ()) + (("hits",) if hits else ())
    for w in _windows(rays):
        r = _launch(S, maps, rays, "point", want, window=w)
        assert (r.opl is None) == (not opl)
        _check(S, maps, r, want, window=w)


def _check_sink(S, maps, rays, source, want, window):
    """the rows the sink launch writes, and its five sums and counts against numpy's on the arctan and
    detector rows that the matching row-writing launch produces"""
    from akbraytracing_amd.reduce import LeafSink
    n = N if window is None else window[1]
    sink = LeafSink(5, n, 0b00011, S["th"].device)
    r = _launch(S, maps, rays, source, want, window=window, sink=sink)
    _check(S, maps, r, want, window=window)
    rows = ("det", "atan") + (("opl",) if maps == "path" else ())
    q = _launch(S, maps, rays, source, rows, window=window)
    _check(S, maps, q, rows, window=window)
    sums, counts = sink.finish()
    sums, counts = sums.cpu().numpy(), counts.cpu().numpy()
    at, det = q.atan.cpu().numpy(), q.det.cpu().numpy()
    assert np.isfinite(at).all() and np.isfinite(det).all()
    want_sums = [np.nansum(at[0]), np.nansum(at[1]), np.sum(det[0]), np.sum(det[1]), np.sum(det[2])]
    assert np.array_equal(sums, np.array(want_sums)) and np.array_equal(counts, np.full(5, n))


# sink, no maps (k_chain_sink): (rays, opl, source, fixed); fixed is RayWave's pass 2 - grid rays
# from the point source writing exactly last_hit, dir_out and opl
SINK = [("grid", opl, source, False) for opl in (True, False) for source in ("point", "per-ray")]
SINK += [("grid", True, "point", True)]
SINK += [("explicit", opl, "point", False) for opl in (True, False)]


@pytest.mark.parametrize("name", SYSTEMS, ids=_id)
@pytest.mark.parametrize("rays,opl,source,fixed", SINK, ids=_id)
def test_sink(gpu, name, rays, opl, source, fixed):
    S = _setup(name, gpu)
    want = ("last_hit", "dir_out") + (("opl",) if opl else ()) + (() if fixed else ("det",))
    for w in _windows(rays):
        _check_sink(S, "none", rays, source, want, w)


# sink, maps (k_chain_sink_fig): (launch, maps)
SINK_FIG = [(launch, maps) for launch in ("grid-fixed", "grid", "explicit") for maps in ("path", "deflect")]


@pytest.mark.parametrize("name", SYSTEMS, ids=_id)
@pytest.mark.parametrize("launch,maps", SINK_FIG, ids=_id)
def test_sink_with_maps(gpu, name, launch, maps):
    S = _setup(name, gpu)
    rays = "explicit" if launch == "explicit" else "grid"
    want = ("last_hit", "dir_out", "opl") + (() if launch == "grid-fixed" else ("det", "fig_opl"))
    for w in _windows(rays):
        _check_sink(S, maps, rays, "point", want, w)


def _batch_systems(gpu):
    """three AKB systems (two parameter vectors of the autofocus fixture, the first twice) with their
    19 x 17 tables, and maps for the first two"""
    if "batch" in _CACHE:
        return _CACHE["batch"]
    from akbraytracing_amd.figure import mirror_frames
    from akbraytracing_amd.geometry import build_akb, mirrors_of
    from akbraytracing_amd.trace import trace_chain
    from akbraytracing_amd.wavefront import AngleRange
    f = golden("akb_autofocus.npz")
    builts = [build_akb(f[f"g{k}_params"], source_shift=f[f"g{k}_source_shift"]) for k in (0, 2, 0)]
    out = []
    for s, b in enumerate(builts):
        th = torch.from_numpy(np.tan(AngleRange(**b["angle_h"]).table(N_H))).to(gpu)
        tv = torch.from_numpy(np.tan(AngleRange(**b["angle_v"]).table(N_V))).to(gpu)
        mir = mirrors_of(b)
        figure = None
        if s < 2:
            free = trace_chain(mir, tan_h=th, tan_v=tv, src=b["source"], want=("hits",))
            figure = make_maps(mirror_frames(b), free.hits.cpu().numpy(), SHAPES)
        out.append(dict(mirrors=mir, th=th, tv=tv, src=b["source"], figure=figure))
    _CACHE["batch"] = out
    return out


@pytest.mark.parametrize("maps", [False, True], ids=["plain", "deflect"])
@pytest.mark.parametrize("opl", [True, False], ids=_id)
@pytest.mark.parametrize("hits", [True, False], ids=_id)
def test_batch_equals_single_launches(gpu, maps, opl, hits):
    """k_chain_batch / k_chain_batch_fig: three systems in one launch against three single launches
    (with maps: the third system has none and runs the same kernel)"""
    from akbraytracing_amd import _lib
    from akbraytracing_amd import device as D
    from akbraytracing_amd.trace import ChainLaunch
    want = ("last_hit", "dir_out") + (("opl",) if opl else ()) + (("hits",) if hits else ())
    systems = _batch_systems(gpu)
    launches = [ChainLaunch(s["mirrors"], tan_h=s["th"], tan_v=s["tv"], src=s["src"], want=want,
                            figure=s["figure"] if maps else None, figure_slope=maps) for s in systems]
    singles = []
    for c in launches:
        r = c.launch()
        assert int(r.flags.item()) == 0
        singles.append({f: getattr(r, f).clone() for f in want})
        for f in want:
            getattr(r, f).fill_(float("nan"))
    descs = (_lib.ChainDesc * len(launches))()
    for k, c in enumerate(launches):
        descs[k] = c.desc
    _lib.check(_lib.lib().akb_trace_chain_batch_f64(descs, len(launches), D.stream_handle()))
    for c, one in zip(launches, singles):
        assert int(c.res.flags.item()) == 0
        for f in want:
            assert torch.equal(getattr(c.res, f), one[f]), f
    if maps:  # the maps deflect where there are some
        assert not torch.equal(singles[0]["dir_out"], singles[2]["dir_out"])


@pytest.mark.parametrize("entry", ["akb_trace_chain_f64", "akb_trace_chain_batch_f64"])
@pytest.mark.parametrize("row", ["hits", "last_hit", "dir_out", "det_out"])
def test_short_row_is_refused(gpu, entry, row):
    """a requested row with a leading dimension below n_rays: AKB_E_ARG, nothing launched"""
    from akbraytracing_amd import _lib
    from akbraytracing_amd.trace import ChainLaunch
    S = _setup(SYSTEMS[0], gpu)
    g = S["g"]
    c = ChainLaunch(g.mirrors, tan_h=S["th"], tan_v=S["tv"], src=g.source, det_ghij=g.det1,
                    want=("hits", "last_hit", "dir_out", "det"))
    outs = (c.res.hits, c.res.last_hit, c.res.dir_out, c.res.det)
    for t in outs:
        t.fill_(7.0)
    setattr(c.desc, row + "_ld", N - 1)
    L = _lib.lib()
    st = L.akb_trace_chain_f64(c.desc, None) if entry == "akb_trace_chain_f64" else L.akb_trace_chain_batch_f64(c.desc, 1, None)
    assert st == -1 and (row + "_ld < n_rays").encode() in L.akb_last_error()
    torch.cuda.synchronize()
    assert all(bool((t == 7.0).all()) for t in outs) and int(c.res.flags.item()) == 0
