"""Figure maps that deflect the rays (slope error), measured:

    python scripts/bench_figure_slope.py [--n 3163] [--reps 20] [--systems 100] [--out bench_out/bench_figure_slope.json]

* the pass-2-shaped fused sink kernel (k_chain_sink_fig: grid rays from the point source, last hit,
  exit direction and OPL rows, the five-quantity sink) on an n x n grid with four 1024 x 32 maps,
  figure_slope off and on, and the same launch without maps;
* akb_trace_chain_batch_f64 over `systems` 53 x 53 systems with four maps each (k_chain_batch_fig) and
  without (k_chain_batch);
  both by device events around the launch, the median of `reps` after a warm-up;
* a physical cross-check: a sinusoidal 1-D profile of known RMS slope sigma on the last mirror,
  auto_focus_NA's best spot sizes at 53 x 53 with and without it, beside 2 sigma L (L: the rays'
  distances from that mirror to the focus, centre and RMS over the footprint) added in quadrature in
  the mirror's focusing direction. Reported, not asserted.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from bench_figure import footprint_maps, geom  # noqa: E402


def events_ms(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return dict(ms_median=float(np.median(ms)), ms_min=float(min(ms)), ms_max=float(max(ms)))


def pass2_shaped(g, n, figure, slope, reps):
    from akbraytracing_amd.reduce import LeafSink
    from akbraytracing_amd.trace import ChainLaunch
    dev = torch.device("cuda", 0)
    th = torch.from_numpy(np.tan(g.angle_h.table(n))).to(dev)
    tv = torch.from_numpy(np.tan(g.angle_v.table(n))).to(dev)
    sink = LeafSink(5, n * n, 0b00011, dev)
    c = ChainLaunch(g.mirrors, tan_h=th, tan_v=tv, src=g.source, det_ghij=g.det1, want=("last_hit", "dir_out", "opl"),
                    sink=sink, figure=figure, figure_slope=slope)
    r = events_ms(c.launch, reps)
    r["flags"] = int(c.res.flags.item())
    return r


def af_params():
    f = np.load(os.path.join(ROOT, "tests", "golden", "akb_autofocus.npz"))
    return np.array(f["g0_params"], dtype=np.float64)


def built_maps(b, nu=1024, nw=32, amp=1e-9, ray_num=33, hits=None):
    """four maps over the footprint of a geometry.build_akb system (traced at ray_num x ray_num)"""
    from akbraytracing_amd.autofocus import TracedSystems
    from akbraytracing_amd.figure import FigureMap, mirror_frames
    if hits is None:
        hits = TracedSystems([b], ray_num=ray_num, want_hits=True, tilt=False).hits[0].cpu().numpy()
    maps = []
    for k, fr in enumerate(mirror_frames(b)):
        d = hits[k] - fr["origin"].reshape(3, 1)
        u, w = fr["e_u"] @ d, fr["e_w"] @ d
        lu, lw = np.ptp(u), np.ptp(w)
        u0, w0 = u.min() - 0.25 * lu, w.min() - 0.25 * lw
        du, dw = 1.5 * lu / (nu - 1), 1.5 * lw / (nw - 1)
        U, W = u0 + du * np.arange(nu), w0 + dw * np.arange(nw)
        h = amp * np.sin(2 * np.pi * 7 * (U[None, :] - u0) / (nu * du)) * np.cos(2 * np.pi * (W[:, None] - w0) / (nw * dw))
        maps.append(FigureMap(h, u0, du, w0, dw, fr["origin"], fr["e_u"], fr["e_w"]))
    return maps


def batch(systems, reps, with_maps):
    from akbraytracing_amd import _lib, device as D
    from akbraytracing_amd.autofocus import TracedSystems
    from akbraytracing_amd.geometry import build_akb
    b = build_akb(af_params())
    maps = built_maps(b) if with_maps else None
    ts = TracedSystems([b] * systems, ray_num=53, tilt=False, figure=maps)
    L = _lib.lib()
    r = events_ms(lambda: _lib.check(L.akb_trace_chain_batch_f64(ts.descs, ts.S, D.stream_handle())), reps)
    r["flags"] = int(ts.flags.max().item())
    return r


def cross_check(sigma=0.5e-6, periods=5):
    """auto_focus_NA's best spot sizes with a sinusoidal profile of RMS slope sigma on the last mirror"""
    from akbraytracing_amd.autofocus import TracedSystems, auto_focus_NA
    from akbraytracing_amd.figure import FigureMap, mirror_frames
    from akbraytracing_amd.geometry import build_akb
    p0 = af_params()
    b0 = build_akb(p0)
    K = len(b0["mirrors"])
    ts0 = TracedSystems([b0], ray_num=53, want_hits=True, tilt=False)
    hits, dirs = ts0.hits[0].cpu().numpy(), ts0.dir[0].cpu().numpy()
    fr0 = mirror_frames(b0)[K - 1]
    u = fr0["e_u"] @ (hits[K - 1] - fr0["origin"].reshape(3, 1))
    lam = np.ptp(u) / periods
    amp = sigma * np.sqrt(2.0) * lam / (2 * np.pi)
    uu = np.linspace(-2 * np.ptp(u), 2 * np.ptp(u), 4001)  # the search moves the mirrors: a generous profile

    def figure(b):
        fr = mirror_frames(b)[K - 1]
        return [None] * (K - 1) + [FigureMap.from_profile(uu, amp * np.sin(2 * np.pi * uu / lam), fr)]

    out = {}
    for name, fig in (("plain", None), ("figure", figure)):
        p = p0.copy()
        sv, sh, p = auto_focus_NA(100, p, 1, 1, False, None, verbose=False, figure=fig)
        out[name] = dict(size_v=float(sv), size_h=float(sh), params0=float(p[0]), params1=float(p[1]))
    # each ray's distance along itself from its hit on that mirror to the focal plane x = const the plain
    # search found (the exit beam is inclined to x, and the sweep's tilt turns it onto x about the
    # focus). The footprint is long against the working distance, so the RMS over the rays is what
    # 2 sigma L means here.
    Lr = (float(b0["s2f_middle"]) + out["plain"]["params0"] - hits[K - 1][0]) / dirs[0]
    Lc, Lrms = float(Lr[Lr.size // 2]), float(np.sqrt(np.mean(Lr * Lr)))
    out["exit_dir_x_mean"] = float(dirs[0].mean())
    nrm = fr0["normal"]
    axis = "h" if abs(nrm[1]) > abs(nrm[2]) else "v"
    s0 = out["plain"]["size_" + axis]
    out.update(sigma_slope_rad=sigma, period_m=float(lam), amplitude_m=float(amp), mirror=K - 1, focusing_axis=axis,
               distance_centre_m=Lc, distance_min_m=float(Lr.min()), distance_max_m=float(Lr.max()), distance_rms_m=Lrms,
               two_sigma_L_centre_m=2 * sigma * Lc, two_sigma_L_rms_m=2 * sigma * Lrms,
               predicted_size_m=float(np.hypot(s0, 2 * sigma * Lrms)), measured_size_m=out["figure"]["size_" + axis])
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--n", type=int, default=3163)
    p.add_argument("--reps", type=int, default=20)
    p.add_argument("--systems", type=int, default=100)
    p.add_argument("--out", default=os.path.join("bench_out", "bench_figure_slope.json"))
    a = p.parse_args()
    g = geom()
    maps = footprint_maps(g)
    res = dict(n=a.n, reps=a.reps, systems=a.systems)
    res["sink_plain"] = pass2_shaped(g, a.n, None, False, a.reps)
    res["sink_fig_slope_off"] = pass2_shaped(g, a.n, maps, False, a.reps)
    res["sink_fig_slope_on"] = pass2_shaped(g, a.n, maps, True, a.reps)
    res["slope_on_over_off"] = res["sink_fig_slope_on"]["ms_median"] / res["sink_fig_slope_off"]["ms_median"]
    res["batch_plain"] = batch(a.systems, a.reps, False)
    res["batch_fig"] = batch(a.systems, a.reps, True)
    res["cross_check"] = cross_check()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
