"""Mirror figure error in the trace: per-mirror height maps on the optical path.

The reference's users rotate the traced mirror hits into the mirror's own frame, subtract the traced
profile from the fabricator's "process data" CSV and plot the residual (compareCSV.py,
AKB_calc_rotate.py, surfacedetailAKB.py): the measured figure error. A FigureMap feeds that residual
back into the trace. The ray path stays as it is; each ray's optical path gains, per mirror,

    delta = -2 h(u, w) |d . N|

with h the map's height at the ray's hit point (in the mirror's frame), d the unit incoming
direction and N the unit normal there - |d . N| is the sine of the grazing angle. This is the
thin-screen model, first-order exact for the wavefront by Fermat's principle; positive h is a bump
towards the incoming beam. csrc/akb_figure.h holds every operation's order (Catmull-Rom cubic
convolution, edge replicate); the fused chain, the stage kernel akb_figure_opl_f64 and a host build
give the same bits.

A hit outside the map contributes 0 and raises the mirror's AKB_FLAG_FIG_OUTSIDE bit; RayWave turns
that into an AKBError naming the mirror.

The ray-spot modes (the batched 'test' trace, auto_focus_NA, calc_FoC; trace_chain(figure_slope=True))
also let the map deflect the ray: the reflection takes N' = (N - sigma g) / ||N - sigma g|| with
g = dh/du e_u + dh/dw e_w the map's gradient and sigma N the normal turned towards the incoming beam
(DESIGN 7.5). stage_normals is that trace stage by stage. The wavefront modes keep the thin screen.

The wave chain (wavedata.saveWaveData / plot_result_wave / kb_wave with figure=, then run_wave_chain)
samples each mirror at the traced hit points, so there the map moves every sample along the normal:
P' = P + sigma h N (displace, displace_hits; akb_figure_displace_f64). sampling compares a
grid's sample spacing with the map's pitch.
"""
import numpy as np

from . import _lib

AXIS_TOL = 1e-12  # |e.e - 1| and |e_u.e_w| (the library checks the same bound)


class FigureMap:
    """A height map (metres) on one mirror: height[(j, i)] at u = u0 + i du, w = w0 + j dw in the frame
    (origin, e_u, e_w) given in lab coordinates. height is (nw, nu); a 1-D array is one row (nw = 1).
    An axis with one sample is constant along it (a 1-D profile such as the fabrication CSVs)."""

    def __init__(self, height, u0, du, w0, dw, origin, e_u, e_w):
        h = np.array(height, dtype=np.float64)
        if h.ndim == 1:
            h = h.reshape(1, -1)
        if h.ndim != 2 or h.size == 0:
            raise ValueError("a figure map needs a 1-D or 2-D height table")
        if h.size >= 1 << 28:
            raise ValueError("figure map beyond 2^28 samples")
        if not np.all(np.isfinite(h)):
            raise ValueError("figure map heights must be finite (unmeasured cells are not supported)")
        self.height = np.ascontiguousarray(h)
        self.u0, self.du, self.w0, self.dw = float(u0), float(du), float(w0), float(dw)
        if not (self.du > 0.0 and self.dw > 0.0 and np.isfinite([self.u0, self.du, self.w0, self.dw]).all()):
            raise ValueError("figure map pitches must be positive and its grid finite")
        self.origin = np.array(origin, dtype=np.float64).reshape(3)
        self.e_u = np.array(e_u, dtype=np.float64).reshape(3)
        self.e_w = np.array(e_w, dtype=np.float64).reshape(3)
        if not np.all(np.isfinite(self.origin)):
            raise ValueError("figure map origin must be finite")
        uu, ww, uw = self.e_u @ self.e_u, self.e_w @ self.e_w, self.e_u @ self.e_w
        if not (abs(uu - 1.0) <= AXIS_TOL and abs(ww - 1.0) <= AXIS_TOL):
            raise ValueError("figure map axes must be unit vectors")
        if not abs(uw) <= AXIS_TOL:
            raise ValueError("figure map axes must be orthogonal")
        self._dev = {}

    nu = property(lambda self: self.height.shape[1])
    nw = property(lambda self: self.height.shape[0])

    def device(self, dev=None):
        """The height table on the device (cached per device)."""
        import torch

        from . import device as D
        dev = dev if dev is not None else D.device()
        key = str(dev)
        if key not in self._dev:
            self._dev[key] = torch.from_numpy(self.height).to(dev)
        return self._dev[key]

    def fill(self, m, dev=None):
        """Write this map into an akb_figure_map (_lib.FigureMapDesc); returns the device table to
        keep alive."""
        from . import device as D
        t = self.device(dev)
        m.table = D.ptr(t)
        for k in range(3):
            m.origin[k], m.e_u[k], m.e_w[k] = self.origin[k], self.e_u[k], self.e_w[k]
        m.u0, m.du, m.w0, m.dw = self.u0, self.du, self.w0, self.dw
        m.nu, m.nw = self.nu, self.nw
        return t

    def desc(self, dev=None):
        m = _lib.FigureMapDesc()
        self._keep = self.fill(m, dev)
        return m

    @staticmethod
    def from_profile(u, h, frame):
        """A 1-D profile h(u) along the frame's e_u (constant along e_w): u equally spaced and
        increasing (checked to 1e-6 of the pitch). frame: a dict with origin, e_u, e_w (mirror_frames)."""
        u = np.asarray(u, dtype=np.float64).ravel()
        h = np.asarray(h, dtype=np.float64).ravel()
        if u.shape != h.shape or u.size < 2:
            raise ValueError("a profile needs two equally long arrays of at least two samples")
        du = (u[-1] - u[0]) / (u.size - 1)
        if not du > 0.0 or np.max(np.abs(np.diff(u) - du)) > 1e-6 * du:
            raise ValueError("a profile's abscissa must be equally spaced and increasing")
        return FigureMap(h.reshape(1, -1), u[0], du, 0.0, 1.0, frame["origin"], frame["e_u"], frame["e_w"])

    @staticmethod
    def from_csv(path, frame, scale_u=1e-3, scale_h=1e-3, skiprows=1):
        """The two-column "x,y" CSV the reference's compareCSV.py reads (np.loadtxt, delimiter ',', one
        header row; millimetres there, hence the default scales to metres)."""
        d = np.loadtxt(path, delimiter=',', skiprows=skiprows)
        return FigureMap.from_profile(d[:, 0] * scale_u, d[:, 1] * scale_h, frame)


def _centre_ray(geometry):
    """The launch grid's centre ray traced on the host (float64, the reference's expressions):
    per mirror the hit, the unit incoming direction and the unit gradient normal."""
    ah, av = geometry.angle_h, geometry.angle_v
    th = np.tan(0.5 * (ah.start + ah.stop) - np.float64(ah.offset))
    tv = np.tan(0.5 * (av.start + av.stop) - np.float64(av.offset))
    d = np.array([1.0, th, tv])
    d = d / np.linalg.norm(d)
    p = np.array(geometry.source, dtype=np.float64)
    out = []
    for m in geometry.mirrors:
        a, b, c, dd, e, f, g, h, i, j = m.coeffs
        l, mm, n = d
        x, y, z = p
        A = a * l * l + b * mm * mm + c * n * n + dd * mm * l + e * n * l + f * mm * n
        B = (2 * a * x * l + 2 * b * y * mm + 2 * c * z * n + dd * (x * mm + y * l) + e * (x * n + z * l)
             + f * (z * mm + y * n) + g * l + h * mm + i * n)
        C = a * x * x + b * y * y + c * z * z + dd * x * y + e * x * z + f * y * z + g * x + h * y + i * z + j
        D = B * B - 4 * A * C
        if not D > 0:
            raise _lib.AKBError("the centre ray misses a mirror: no frame")
        t = (-B - np.sqrt(D)) / (2 * A) if m.negative else (-B + np.sqrt(D)) / (2 * A)
        hit = p + t * d
        N = np.array([2 * a * hit[0] + dd * hit[1] + e * hit[2] + g, 2 * b * hit[1] + dd * hit[0] + f * hit[2] + h,
                      2 * c * hit[2] + e * hit[0] + f * hit[1] + i])
        N = N / np.linalg.norm(N)
        out.append((hit, d.copy(), N))
        r = d - 2 * (d @ N) * N
        d = r / np.linalg.norm(r)
        p = hit
    return out


class _GeometryView:
    """mirrors, source and the two angle ranges of what geometry.build_akb / build_kb return"""

    def __init__(self, built):
        from . import geometry as G
        from .wavefront import AngleRange
        self.mirrors = G.mirrors_of(built)
        self.source = [float(x) for x in built["source"]]
        self.angle_h = AngleRange(**built["angle_h"])
        self.angle_v = AngleRange(**built["angle_v"])


def mirror_frames(geometry):
    """One frame per mirror from the launch grid's centre ray: origin = its hit, e_u = the incoming
    direction projected onto the tangent plane and normalised, e_w = n x e_u with n the unit normal
    turned towards the incoming beam - the frame in which a fabricator's length profile is
    measured. geometry: a SystemGeometry, or the dict geometry.build_akb / build_kb return (only the
    mirrors, the source and the two angle ranges are read). Returns a list of dicts (origin, e_u, e_w,
    normal, grazing = the centre ray's |d . n|)."""
    if isinstance(geometry, dict):
        geometry = _GeometryView(geometry)
    frames = []
    for hit, d, N in _centre_ray(geometry):
        n = -N if d @ N > 0 else N
        eu = d - (d @ n) * n
        eu = eu / np.linalg.norm(eu)
        eu = eu - (eu @ n) * n  # one re-orthogonalisation: e_u . n to the last bit
        eu = eu / np.linalg.norm(eu)
        ew = np.cross(n, eu)
        ew = ew / np.linalg.norm(ew)
        frames.append(dict(origin=hit, e_u=eu, e_w=ew, normal=n, grazing=abs(d @ n)))
    return frames


def check_figure(figure, n_mirrors):
    """Validate a `figure=` argument: None, or one FigureMap / None per mirror."""
    if figure is None:
        return None
    figure = list(figure)
    if len(figure) != n_mirrors:
        raise ValueError(f"figure needs one entry (FigureMap or None) per mirror: {n_mirrors}")
    for f in figure:
        if f is not None and not isinstance(f, FigureMap):
            raise ValueError("figure entries must be FigureMap or None")
    if all(f is None for f in figure):
        return None
    return figure


def outside_error(flags):
    """The AKBError message for the figure bits of a chain's flag word, or None."""
    ks = [k for k in range(_lib.MAX_MIRRORS) if flags & (_lib.FLAG_FIG_OUTSIDE << (4 * k))]
    if not ks:
        return None
    return ("a ray hit outside the figure map of mirror " + ", ".join(str(k) for k in ks)
            + f" (trace flags {flags:#x}): the map must cover the beam's footprint on the mirror")


def stage_terms(mirrors, figure, hits, dirs0, prims=None, flags_out=None):
    """The figure terms from materialised hits, mirror by mirror with the stage kernel
    (akb_figure_opl_f64), summed in mirror order: what the fused chain adds, bit for bit. hits: K
    tensors (3, n); dirs0: the (3, n) unit directions entering mirror 0. The incoming directions of
    the later mirrors are rebuilt as the staged chain does (reflect_ray of norm_vector; prims:
    primitives, or extended.prims for the double-double reflection). Returns (fig_opl (n), flag word
    with mirror k's AKB_FLAG_FIG_OUTSIDE at 4k)."""
    import torch

    from . import device as D
    from . import primitives as P
    prims = prims if prims is not None else P
    L = _lib.lib()
    n = hits[0].shape[1]
    dev = hits[0].device
    out = torch.zeros(n, dtype=D.F64, device=dev)
    word = 0
    ray = dirs0
    started = False
    for k, m in enumerate(mirrors):
        p = hits[k].contiguous()
        f = figure[k]
        if f is not None:
            fl = torch.zeros(1, dtype=torch.int32, device=dev)
            ray_c = ray.contiguous()
            _lib.check(L.akb_figure_opl_f64(f.desc(dev), D.host_f64(m.coeffs), D.ptr(p), n, 1, D.ptr(ray_c), n, 1, n,
                                            D.ptr(out), int(started), D.ptr(fl), D.stream_handle()))
            started = True
            if int(fl.item()) & _lib.FLAG_FIG_OUTSIDE:
                word |= _lib.FLAG_FIG_OUTSIDE << (4 * k)
        if k + 1 < len(mirrors):
            ray = prims.reflect_ray(ray, prims.norm_vector(m.coeffs, p))
    return out, word


def figure_normal(fm, coeffs, hit, ray):
    """One mirror's deflected unit normals (akb_figure_normal_f64) from hits and unit incoming
    directions, (3, n) device tensors: ((3, n) normals, the kernel's flag word)."""
    import torch

    from . import device as D
    n = hit.shape[1]
    hit, ray = hit.contiguous(), ray.contiguous()
    out = torch.empty((3, n), dtype=D.F64, device=hit.device)
    fl = torch.zeros(1, dtype=torch.int32, device=hit.device)
    _lib.check(_lib.lib().akb_figure_normal_f64(fm.desc(hit.device), D.host_f64(coeffs), D.ptr(hit), n, D.ptr(ray), n, n,
                                                D.ptr(out), n, D.ptr(fl), D.stream_handle()))
    return out, int(fl.item())


def displace(fm, coeffs, hit, dirs, want_height=False):
    """One mirror's displaced sample points (akb_figure_displace_f64) from hits and incoming directions
    (only the sign of d . N is read: they need not be unit), (3, n) device tensors: P' = P + sigma h N,
    P itself outside the map. Returns ((3, n) points, the kernel's flag word[, the heights (n)])."""
    import torch

    from . import device as D
    n = hit.shape[1]
    hit, dirs = hit.contiguous(), dirs.contiguous()
    out = torch.empty((3, n), dtype=D.F64, device=hit.device)
    h = torch.empty(n, dtype=D.F64, device=hit.device) if want_height else None
    fl = torch.zeros(1, dtype=torch.int32, device=hit.device)
    _lib.check(_lib.lib().akb_figure_displace_f64(fm.desc(hit.device), D.host_f64(coeffs), D.ptr(hit), n, D.ptr(dirs), n, n,
                                                  D.ptr(out), n, D.ptr(h) if want_height else None, D.ptr(fl),
                                                  D.stream_handle()))
    if want_height:
        return out, int(fl.item()), h
    return out, int(fl.item())


def displace_hits(mirrors, figure, hits, src):
    """The wave chain's mirror grids with the maps on them: mirror k's materialised hits
    (3, n) moved by displace() with the incoming direction hits[k] - hits[k - 1] (hits[0] - src for the
    first mirror; unnormalised, only its sign is used). figure: one FigureMap or None per mirror; src:
    the source point (3 values, or a (3, 1) / (3, n) tensor). Returns (the list of grids - an unmapped
    mirror's tensor unchanged -, the flag word with mirror k's bits at 4k)."""
    import torch

    from . import device as D
    out, word = [], 0
    prev = None
    for k, m in enumerate(mirrors):
        p = hits[k]
        f = figure[k]
        if f is None:
            out.append(p)
        else:
            if prev is None:
                prev = src if isinstance(src, torch.Tensor) else torch.tensor([float(x) for x in src], dtype=D.F64)
                prev = prev.to(device=p.device, dtype=D.F64).reshape(3, -1)
            q, fl = displace(f, m.coeffs, p, p - prev)
            word |= (fl & (_lib.FLAG_FIG_OUTSIDE | _lib.FLAG_ZERO_NORMAL)) << (4 * k)
            out.append(q)
        prev = p
    return out, word


def sampling(fm, grid, n_v, n_h):
    """How finely a (3, n_v * n_h) grid of sample points (row-major, n_h fastest) samples the map fm: the
    largest distance between neighbouring samples - along the rows and along the columns - measured
    along e_u and along e_w, next to the map's pitches. Returns a dict (su, sw, du, dw). Host numpy."""
    g = np.asarray(grid, dtype=np.float64)[:3].reshape(3, int(n_v), int(n_h))
    d = g - fm.origin.reshape(3, 1, 1)
    out = {}
    for name, e in (("su", fm.e_u), ("sw", fm.e_w)):
        c = np.tensordot(e, d, axes=(0, 0))
        steps = [np.abs(np.diff(c, axis=a)) for a in (0, 1) if c.shape[a] > 1]
        out[name] = float(max((s.max() for s in steps), default=0.0))
    out["du"], out["dw"] = fm.du, fm.dw
    return out


def stage_normals(mirrors, figure, dirs, src, with_segments=False, prims=None, with_terms=False):
    """trace.staged_chain with the mapped mirrors deflecting: per mirror the intersection, then the
    deflected normal (akb_figure_normal_f64; norm_vector for a mirror without a map), then reflect_ray -
    what the fused chain with figure_slope gives, bit for bit, and the path a flagged trace takes (the
    primitives apply the reference's all-NaN / passthrough rules). dirs, src: (3, n) device tensors;
    prims as in stage_terms. Returns (hits, exit directions, segments, flag word with mirror k's
    AKB_FLAG_FIG_OUTSIDE at 4k); with_terms appends the path terms' sum in mirror order (stage_terms'
    value on the deflected path: akb_figure_opl_f64 with each mirror's actual incoming directions)."""
    import torch

    from . import device as D
    from . import primitives as P
    prims = prims if prims is not None else P
    hits, segs = [], []
    ray, org = dirs, src
    word = 0
    terms, started = None, False
    if with_terms:
        terms = torch.zeros(dirs.shape[1], dtype=D.F64, device=dirs.device)
    for k, m in enumerate(mirrors):
        p = prims.mirr_ray_intersection(m.coeffs, ray, org, negative=m.negative)
        if with_segments:
            segs.append(prims.segment_length(org, p))
        f = figure[k] if figure is not None else None
        nrm = None
        if f is not None and with_terms:
            n = p.shape[1]
            pc, rc = p.contiguous(), ray.contiguous()
            tfl = torch.zeros(1, dtype=torch.int32, device=p.device)
            _lib.check(_lib.lib().akb_figure_opl_f64(f.desc(p.device), D.host_f64(m.coeffs), D.ptr(pc), n, 1, D.ptr(rc),
                                                     n, 1, n, D.ptr(terms), int(started), D.ptr(tfl), D.stream_handle()))
            started = True
        if f is not None:
            nrm, fl = figure_normal(f, m.coeffs, p, ray)
            if fl & _lib.FLAG_FIG_OUTSIDE:
                word |= _lib.FLAG_FIG_OUTSIDE << (4 * k)
            if fl & _lib.FLAG_ZERO_NORMAL:  # the reference's passthrough rule, undeflected
                nrm = None
        if nrm is None:
            nrm = prims.norm_vector(m.coeffs, p)
        ray = prims.reflect_ray(ray, nrm)
        org = p
        hits.append(p)
    if with_terms:
        return hits, ray, segs, word, terms
    return hits, ray, segs, word
