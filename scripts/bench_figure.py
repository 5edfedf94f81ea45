"""Figure maps in the trace, measured:

    python scripts/bench_figure.py [--n 3163] [--reps 20] [--check-n 257] [--out bench_out/bench_figure.json]

* pass-2 time (the fused sink kernel, RayWave's own launch) on an n x n grid with four 1024 x 32
  maps against the same launch without maps: device events, the median of `reps` after a warm-up;
* a physical cross-check of the thin-screen model: a constant map delta = 100 nm on one mirror
  against the same mirror rigidly shifted by delta along its centre normal (geometry's coefficient
  shifts). Both changes of Wave2 have best-fit piston, tilt and defocus removed (least squares over
  the ray grid's indices); the RMS of their difference is reported beside the RMS of each change.
  Reported, not asserted.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def geom():
    from akbraytracing_amd.wavefront import SystemGeometry
    return SystemGeometry.load(os.path.join(ROOT, "tests", "golden", "akb_geometry.json"))


def footprint_maps(g, nu=1024, nw=32, amp=1e-9, const=None, which=None, margin=0.25):
    """one map per mirror over the beam's footprint (traced at 33 x 33) plus a margin"""
    from akbraytracing_amd.figure import FigureMap, mirror_frames
    from akbraytracing_amd.trace import trace_chain
    dev = torch.device("cuda", 0)
    th = torch.from_numpy(np.tan(g.angle_h.table(33))).to(dev)
    tv = torch.from_numpy(np.tan(g.angle_v.table(33))).to(dev)
    hits = trace_chain(g.mirrors, tan_h=th, tan_v=tv, src=g.source, want=("hits",)).hits.cpu().numpy()
    maps = []
    for k, fr in enumerate(mirror_frames(g)):
        if which is not None and k not in which:
            maps.append(None)
            continue
        d = hits[k] - fr["origin"].reshape(3, 1)
        u, w = fr["e_u"] @ d, fr["e_w"] @ d
        lu, lw = np.ptp(u), np.ptp(w)
        u0, w0 = u.min() - margin * lu, w.min() - margin * lw
        du, dw = (1 + 2 * margin) * lu / (nu - 1), (1 + 2 * margin) * lw / (nw - 1)
        if const is not None:
            h = np.full((nw, nu), const)
        else:
            U, W = u0 + du * np.arange(nu), w0 + dw * np.arange(nw)
            h = amp * np.sin(2 * np.pi * 7 * (U[None, :] - u0) / (nu * du)) * np.cos(2 * np.pi * (W[:, None] - w0) / (nw * dw))
        maps.append(FigureMap(h, u0, du, w0, dw, fr["origin"], fr["e_u"], fr["e_w"]))
    return maps


def pass2_ms(g, n, figure, reps):
    from akbraytracing_amd.wavefront import RayWave
    rw = RayWave(g, n, figure=figure)
    for _ in range(3):
        rw.run()
    torch.cuda.synchronize()
    rw.kernel_events = []
    for _ in range(reps):
        rw.run()
    torch.cuda.synchronize()
    ms = [a.elapsed_time(b) for a, b in rw.kernel_events]
    return dict(ms_median=float(np.median(ms)), ms_min=float(min(ms)), ms_max=float(max(ms)))


def detrend(w, n):
    """w (n * n, ray order) minus its least-squares piston, tilt and defocus over the grid indices"""
    y, x = np.meshgrid(np.linspace(-1, 1, n), np.linspace(-1, 1, n), indexing="ij")
    A = np.stack([np.ones(n * n), x.ravel(), y.ravel(), (x * x).ravel(), (y * y).ravel()], axis=1)
    ok = np.isfinite(w)
    c, *_ = np.linalg.lstsq(A[ok], w[ok], rcond=None)
    return w - A @ c


def cross_check(g, n, k=1, delta=100e-9):
    import copy

    from akbraytracing_amd import geometry as G
    from akbraytracing_amd.figure import mirror_frames
    from akbraytracing_amd.wavefront import RayWave
    base = RayWave(g, n).run()["wave2"].cpu().numpy()
    fig = RayWave(g, n, figure=footprint_maps(g, nu=8, nw=4, const=delta, which=(k,))).run()["wave2"].cpu().numpy()
    nrm = mirror_frames(g)[k]["normal"]  # turned towards the incoming beam: +delta is a bump
    g2 = copy.deepcopy(g)
    c = g2.mirrors[k].coeffs
    c = G.shift_z(G.shift_y(G.shift_x(c, delta * nrm[0]), delta * nrm[1]), delta * nrm[2])
    g2.mirrors[k].coeffs = [float(v) for v in c]
    moved = RayWave(g2, n).run()["wave2"].cpu().numpy()
    a, b = detrend(fig - base, n), detrend(moved - base, n)
    rms = lambda v: float(np.sqrt(np.nanmean(v * v)))
    return dict(mirror=k, delta_nm=delta * 1e9, n=n, rms_change_map_nm=rms(a), rms_change_shift_nm=rms(b),
                rms_difference_nm=rms(a - b), raw_rms_map_nm=rms(fig - base), raw_rms_shift_nm=rms(moved - base))


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--n", type=int, default=3163)
    p.add_argument("--reps", type=int, default=20)
    p.add_argument("--check-n", type=int, default=257)
    p.add_argument("--out", default=os.path.join("bench_out", "bench_figure.json"))
    a = p.parse_args()
    g = geom()
    res = dict(n=a.n, reps=a.reps)
    res["pass2_plain"] = pass2_ms(g, a.n, None, a.reps)
    res["pass2_figure"] = pass2_ms(g, a.n, footprint_maps(g), a.reps)
    res["pass2_ratio"] = res["pass2_figure"]["ms_median"] / res["pass2_plain"]["ms_median"]
    res["cross_check"] = cross_check(g, a.check_n)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
