"""Figure maps in the wave chain (displaced mirror points), measured:

    python scripts/bench_figure_wave.py [--n 3163] [--reps 20] [--grid 257] [--skip-twice] [--out bench_out/bench_figure_wave.json]

* akb_figure_displace_f64 on the last mirror's hits of an n x n trace of the AKB system with a 1024 x 32
  map, with and without the height row, next to akb_figure_normal_f64 on the same inputs: device events
  around the launch, the median of `reps` after a warm-up;
* a physical cross-check: the KB pair with a sinusoidal 1-D profile (amplitude a, period p) on its last
  mirror, saveWaveData(figure=...) and run_wave_chain at grid x grid and at twice that, the focal-plane
  intensity along that mirror's focusing direction beside the figure-free run. First-order satellites
  are expected at +-lambda L / (p sin theta) from the peak with (J1(phi) / J0(phi))^2 of its intensity,
  phi = 2 k a sin theta, L and theta the centre ray's distance to the focal plane and grazing angle.
  Reported, not asserted. The figure-free image is only a focus once the Huygens sums between the
  mirrors are sampled finely enough (the chain is normally run at 3163 x 3163, about 200 s for the
  M1 -> M2 stage alone); the plain run's peak column and peak value at both grids show whether it is.
"""
import argparse
import json
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from bench_figure import footprint_maps, geom  # noqa: E402
from bench_figure_slope import events_ms  # noqa: E402

LAMBDA = 13.5e-9  # the Wavecalc driver's wavelength with option_HighNA


def kernel_times(n, reps):
    from akbraytracing_amd import _lib, device as D
    from akbraytracing_amd.trace import trace_chain
    dev = torch.device("cuda", 0)
    g = geom()
    K = len(g.mirrors)
    fm = footprint_maps(g, which=(K - 1,))[K - 1]
    th = torch.from_numpy(np.tan(g.angle_h.table(n))).to(dev)
    tv = torch.from_numpy(np.tan(g.angle_v.table(n))).to(dev)
    hits = trace_chain(g.mirrors, tan_h=th, tan_v=tv, src=g.source, want=("hits",)).hits
    hit = hits[K - 1].contiguous()
    ray = hits[K - 1] - hits[K - 2]
    ray = (ray / ray.norm(dim=0)).contiguous()
    del hits
    N = n * n
    out = torch.empty((3, N), dtype=torch.float64, device=dev)
    h = torch.empty(N, dtype=torch.float64, device=dev)
    fl = torch.zeros(1, dtype=torch.int32, device=dev)
    L = _lib.lib()
    desc, c, s = fm.desc(dev), D.host_f64(g.mirrors[K - 1].coeffs), D.stream_handle()

    def displace(hp):
        return lambda: _lib.check(L.akb_figure_displace_f64(desc, c, D.ptr(hit), N, D.ptr(ray), N, N, D.ptr(out), N, hp,
                                                            D.ptr(fl), s))

    res = dict(n=n, reps=reps, map="1024x32")
    res["displace"] = events_ms(displace(None), reps)
    res["displace_with_height"] = events_ms(displace(D.ptr(h)), reps)
    res["normal"] = events_ms(lambda: _lib.check(L.akb_figure_normal_f64(desc, c, D.ptr(hit), N, D.ptr(ray), N, N, D.ptr(out),
                                                                         N, D.ptr(fl), s)), reps)
    res["flags"] = int(fl.item())
    # bytes moved: hit and dir in, out (and the heights) written; the table stays in L2
    for name, rows in (("displace", 9), ("displace_with_height", 10), ("normal", 9)):
        res[name]["GBps"] = rows * 8 * N / (res[name]["ms_median"] * 1e-3) / 1e9
    return res


def _bessel(phi):
    """J0 and J1 by their power series (phi of order one)"""
    j0 = j1 = 0.0
    term0, term1 = 1.0, phi / 2
    for m in range(30):
        j0 += term0
        j1 += term1
        term0 *= -(phi / 2)**2 / ((m + 1)**2)
        term1 *= -(phi / 2)**2 / ((m + 1) * (m + 2))
    return j0, j1


def _line(field, n):
    """|u|^2 along y (the columns of the (z, y) image grid) through the peak, and the peak's column"""
    inten = np.abs(field.reshape(n, n))**2
    iz, iy = np.unravel_index(np.argmax(inten), inten.shape)
    return inten[iz], int(iy)


def _satellites(line, iy, pitch, lo, hi):
    """per side: the highest sample between lo and hi (metres) from the peak - its offset and its
    intensity over the peak's - and the summed intensity of that window over the summed main lobe
    (|offset| < lo)"""
    y = (np.arange(line.size) - iy) * pitch
    main = line[np.abs(y) < lo].sum()
    out = {}
    for side, sel in (("minus", (y <= -lo) & (y >= -hi)), ("plus", (y >= lo) & (y <= hi))):
        if not sel.any():
            out[side] = None
            continue
        j = np.flatnonzero(sel)[np.argmax(line[sel])]
        out[side] = dict(offset_m=float(y[j]), peak_ratio=float(line[j] / line[iy]), sum_ratio=float(line[sel].sum() / main))
    return out


def cross_check(n, phi=0.5, offset=0.8e-6, ysize=1e-6):
    """the KB pair (params = 0), a sine on the last mirror of the trace; grid n x n. p is picked so that
    the centre ray's first orders fall `offset` from the peak, inside the +-2 ysize the image stage covers;
    a from phi."""
    from akbraytracing_amd import geometry as G
    from akbraytracing_amd import wavedata as W
    from akbraytracing_amd.figure import FigureMap, mirror_frames
    params = np.zeros(26)
    b = G.build_kb(params)
    fr = mirror_frames(b)[-1]
    sin_t = float(fr["grazing"])
    # the centre ray's distance from the mirror to the focal plane x = s2f_middle + defocus, along itself
    r0 = W.kb_wave(params, 33, defocus_for_wave=0.0)
    hm, det = r0[2], r0[3]
    c = hm.shape[1] // 2
    L = float(np.linalg.norm(det[:, c] - hm[:, c]))
    Ls = np.linalg.norm(det - hm, axis=0)
    p = LAMBDA * L / (offset * sin_t)
    k = 2 * np.pi / LAMBDA
    a = phi / (2 * k * sin_t)
    uu = (p / 16) * np.arange(-int(1.6 / p), int(1.6 / p) + 1)  # sixteen samples a period over +-0.1 m
    fm = FigureMap.from_profile(uu, a * np.sin(2 * np.pi * uu / p), fr)
    j0, j1 = _bessel(phi)
    out = dict(grid=n, wavelength_m=LAMBDA, grazing_sin=sin_t, distance_centre_m=L, distance_min_m=float(Ls.min()),
               distance_max_m=float(Ls.max()), period_m=p, amplitude_m=a, phi=phi, expected_offset_m=offset,
               expected_ratio=(j1 / j0)**2, image_half_width_m=2 * ysize)
    lines = {}
    with tempfile.TemporaryDirectory() as tmp:
        for name, fig in (("plain", None), ("figure", [None, fm])):
            folder = W.saveWaveData(params, ysize, ysize, ray_num_H=n, directory=os.path.join(tmp, name), option_AKB=False,
                                    defocus_for_wave=0.0, timestamp="bench", figure=fig)
            cond = W.read_conditions(folder)
            fields = W.run_wave_chain(folder, None, resume_dir=None)
            line, iy = _line(fields["Image"], cond["pix_y"])
            lines[name] = (line, iy)
            grid = np.load(os.path.join(folder, "points_gridImage.npy"))
            pitch = 2 * float(np.ptp(grid[1])) / (cond["pix_y"] - 1)  # the image stage scales the grid by 2
            out[name] = dict(peak=float(line[iy]), peak_column=iy, pitch_m=pitch,
                             satellites=_satellites(line, iy, pitch, 0.4 * offset, 2.0 * offset))
    out["peak_ratio_figure_over_plain"] = out["figure"]["peak"] / out["plain"]["peak"]
    out["expected_peak_ratio_J0_squared"] = j0**2
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--n", type=int, default=3163)
    p.add_argument("--reps", type=int, default=20)
    p.add_argument("--grid", type=int, default=257)
    p.add_argument("--skip-twice", action="store_true", help="leave out the run at twice the grid")
    p.add_argument("--out", default=os.path.join("bench_out", "bench_figure_wave.json"))
    a = p.parse_args()
    res = dict(kernel=kernel_times(a.n, a.reps))
    res["cross_check"] = cross_check(a.grid)
    if not a.skip_twice:
        res["cross_check_twice_the_grid"] = cross_check(2 * a.grid - 1)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
