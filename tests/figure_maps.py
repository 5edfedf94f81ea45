"""Smooth figure maps over a traced footprint, shared by the GPU tests that trace with maps."""
import numpy as np

AMP = 1e-8


def make_maps(frames, hits, shapes, margin=0.25):
    """one smooth map per mirror (None where shapes[k] is None) covering the footprint hits[k] (3, n)
    of a map-free trace plus a margin on each side, in the given frames"""
    from akbraytracing_amd.figure import FigureMap
    maps = []
    for k, (fr, shp) in enumerate(zip(frames, shapes)):
        if shp is None:
            maps.append(None)
            continue
        nw, nu = shp
        d = hits[k] - fr["origin"].reshape(3, 1)
        u, w = fr["e_u"] @ d, fr["e_w"] @ d
        lu, lw = np.ptp(u), np.ptp(w)
        u0, w0 = u.min() - margin * lu, w.min() - margin * lw
        du = (1 + 2 * margin) * lu / max(nu - 1, 1)
        dw = (1 + 2 * margin) * lw / max(nw - 1, 1)
        Ug, Wg = u0 + du * np.arange(nu), w0 + dw * np.arange(nw)
        h = AMP * np.sin(2 * np.pi * (Ug[None, :] - u0) / (1.7 * lu) + 0.3 * k) * np.cos(2 * np.pi * (Wg[:, None] - w0) / (2.3 * lw))
        maps.append(FigureMap(h, u0, du, w0, dw, fr["origin"], fr["e_u"], fr["e_w"]))
    return maps
