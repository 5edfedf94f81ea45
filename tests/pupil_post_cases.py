"""Shared by test_pupil_post_cpu.py and test_pupil_post_gpu.py: the input maps that take
akb_pupil_post_f64 through every branch its entry point admits, and the references they are held
to - the float64 oracle chain (oracle.pupilmap, oracle.psfcalc) and the same fit and prefilter in
np.longdouble, which bound the oracle's own error.

Every map is formed once per process and handed out read-only; the oracle's results on it likewise.
"""
import functools

import numpy as np

import oracle.psfcalc as OPC
import oracle.pupilmap as OPM

LD = np.longdouble

# (ny, nx) of the aperture family and the branch of csrc/akb_psfcalc.hip each one reaches
SHAPES = [
    (3, 3), (5, 7),              # spline_line_reg on lines shorter than its 8 lanes; nanmean leaves of 9 and 35 points
    (9, 17), (17, 9),            # segments of 2 and 3 with empty top lanes
    (64, 100), (100, 100),       # in LDS; 10000 = a full 8192 buffer + 1808
    (127, 129), (129, 127),      # in LDS (16383), k_spline_block on one axis, then on the other
    (128, 129),                  # 16512: the first size read from global memory, basis tables on
    (160, 160),                  # a plausible FaithfulPupil(size=)
    (256, 256),                  # kPostMax, 8 buffers, k_spline_block's longest line
    (257, 255),                  # tables off; k_spline_lines on axis 0, k_spline_block on axis 1
    (40, 1500), (1500, 40),      # nx > 1024 in PostIdx (di = 0); lines of 1500
]
SEEDS = {}  # (ny, nx) -> seed where ny * 1000 + nx breaks a condition of test_pupil_post_cpu.py (none does)

EDGE_SHAPES = [(128, 128), (160, 160)]
EDGE_SEED = 5


def edge_drs(nx):
    """The row differences of the edge family: angles 0, small of both signs, exactly -+45 degrees,
    beyond 45 degrees of both signs (cosdg / sindg's second octant), and two middling ones."""
    h = 3 * nx // 4 - nx // 4
    return [0, 1, -1, h, -h, 100, -100, 17, -40]


def _read_only(a):
    a.setflags(write=False)
    return a


def _poly(ny, nx, rng, cross):
    y, x = np.mgrid[0:ny, 0:nx].astype(np.float64)
    u = (2 * x - (nx - 1)) / max(nx - 1, 1)
    v = (2 * y - (ny - 1)) / max(ny - 1, 1)
    m = 7.0 + 0.3 * u - 0.2 * v + 0.15 * u * u + 0.05 * v * v
    if cross:
        m = m + 0.04 * u * v * v
    return y, u, v, m + 0.01 * rng.standard_normal((ny, nx))


@functools.lru_cache(maxsize=None)
def make(ny, nx, seed=None):
    """The aperture family: a quadratic + cubic surface with noise; for sides of at least 9, NaN
    outside a tilted ellipse and max(3, finite // 200) finite points moved by +-0.5 (the outliers the
    3-sigma filter must drop)."""
    if seed is None:
        seed = SEEDS.get((ny, nx), ny * 1000 + nx)
    rng = np.random.default_rng(seed)
    _, u, v, m = _poly(ny, nx, rng, True)
    if min(ny, nx) >= 9:
        c, s = np.cos(0.35), np.sin(0.35)
        p, q = c * u + s * v, -s * u + c * v
        m[(p / 0.95) ** 2 + (q / 0.7) ** 2 > 1.0] = np.nan
        fin = np.flatnonzero(np.isfinite(m))
        idx = rng.choice(fin, size=max(3, fin.size // 200), replace=False)
        m.flat[idx] += 0.5 * rng.choice([-1, 1], size=idx.size)
    return _read_only(m)


@functools.lru_cache(maxsize=None)
def make_edge(ny, nx, dr, seed=EDGE_SEED):
    """The edge family: the same surface without the outliers, NaN above a straight top edge whose
    first valid rows at columns nx // 4 and 3 nx // 4 differ by exactly dr, and NaN where
    u^2 + v^2 > 1.1."""
    rng = np.random.default_rng(seed)
    y, u, v, m = _poly(ny, nx, rng, False)
    c1, c3 = nx // 4, nx * 3 // 4
    s = -dr / (c3 - c1)  # first row at c1 minus first row at c3 = dr
    top = np.rint(ny * 0.45 + s * (np.arange(nx) - (c1 + c3) / 2) * 0.9999 + 0.25)
    m[y < top[None, :]] = np.nan
    m[(u * u + v * v) > 1.1] = np.nan
    return _read_only(m)


def first_fit(z, sigma=3):
    """The oracle's first (five-term) fit of z = m - nanmean: (residuals over the finite points, the
    3-sigma threshold), as oracle.pupilmap forms them."""
    x, y = np.meshgrid(np.arange(z.shape[1]), np.arange(z.shape[0]))
    mask = ~np.isnan(z)
    xf, yf, zf = x[mask].astype(np.float64), y[mask].astype(np.float64), z[mask]
    A1 = np.stack([xf, yf, np.ones_like(xf), xf ** 2, yf ** 2], axis=1)
    res = zf - A1 @ np.linalg.lstsq(A1, zf, rcond=None)[0]
    return res, sigma * np.std(res)


def oracle_chain(m):
    """The oracle's chain on a map: dict(mean, z, corrected, rng, res, thr, rot, deg, mask_rot, rotated)."""
    m = np.asarray(m)
    mean = np.nanmean(m)
    z = m - mean
    corrected = OPM.plane_correction_with_nan_and_outlier_filter(z)
    res, thr = first_fit(z)
    with np.errstate(invalid="ignore"):
        rot = OPC.rotation_estimate(corrected)
        deg = np.degrees(rot)
        mask_rot = OPC.rotate((~np.isnan(corrected)).astype(float), deg)
        rotated = OPC.rotate_with_nan(corrected, deg)
    out = dict(mean=mean, z=z, corrected=corrected, rng=float(np.nanmax(corrected) - np.nanmin(corrected)),
               res=res, thr=thr, rot=rot, deg=deg, mask_rot=mask_rot, rotated=rotated)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def aperture_case(ny, nx):
    m = make(ny, nx)
    return m, oracle_chain(m)


@functools.lru_cache(maxsize=None)
def edge_case(ny, nx, dr):
    m = make_edge(ny, nx, dr)
    return m, oracle_chain(m)


# ---- the same operations in np.longdouble (64-bit significand on x86): the oracle's own error ----

def _solve_ld(A, b):
    """A x = b by Gaussian elimination with partial pivoting in np.longdouble."""
    A, b = A.astype(LD).copy(), b.astype(LD).copy()
    n = len(b)
    for k in range(n):
        p = k + int(np.argmax(np.abs(A[k:, k])))
        A[[k, p]] = A[[p, k]]
        b[[k, p]] = b[[p, k]]
        for i in range(k + 1, n):
            l = A[i, k] / A[k, k]
            A[i] -= l * A[k]
            b[i] -= l * b[k]
    x = np.zeros(n, LD)
    for k in range(n - 1, -1, -1):
        x[k] = (b[k] - A[k, k + 1:] @ x[k + 1:]) / A[k, k]
    return x


def plane_correction_ld(z, sigma=3):
    """plane_correction_with_nan_and_outlier_filter of z in np.longdouble: the two least-squares fits
    as normal equations in the basis 1, X, Y, X^2, Y^2 with X, Y the indices scaled to [-1, 1] (the
    same planes and quadratics as the index basis spans). Returns (corrected, points dropped)."""
    ny, nx = z.shape
    yy, xx = np.mgrid[0:ny, 0:nx]
    X = (2 * xx - (nx - 1)) / LD(nx - 1)
    Y = (2 * yy - (ny - 1)) / LD(ny - 1)
    m = ~np.isnan(z)
    zf = z[m].astype(LD)
    B = np.stack([np.ones_like(X[m]), X[m], Y[m], X[m] ** 2, Y[m] ** 2], axis=1)
    c = _solve_ld(B.T @ B, B.T @ zf)
    res = zf - B @ c
    keep = np.abs(res) < sigma * np.sqrt(np.mean((res - res.mean()) ** 2))
    B3 = B[keep][:, :3]
    p = _solve_ld(B3.T @ B3, B3.T @ zf[keep])
    return z.astype(LD) - (p[0] + p[1] * X + p[2] * Y), int((~keep).sum())


def _spline_filter1d_ld(x):
    z = np.sqrt(LD(3)) - 2
    c = x.astype(LD) * ((1 - z) * (1 - 1 / z))
    n = len(c)
    if n == 1:
        return c
    zn1 = z ** (n - 1)
    c0 = c[0] + zn1 * c[n - 1]
    zi = z
    for i in range(1, n - 1):
        c0 += zi * (c[i] + zn1 * c[n - 1 - i])
        zi *= z
    c[0] = c0 / (1 - zn1 * zn1)
    for i in range(1, n):
        c[i] += z * c[i - 1]
    c[n - 1] = (z * c[n - 2] + c[n - 1]) * z / (z * z - 1)
    for i in range(n - 2, -1, -1):
        c[i] = z * (c[i + 1] - c[i])
    return c


def spline_filter_ld(img):
    """oracle.psfcalc.spline_filter's recursion in np.longdouble."""
    out = np.apply_along_axis(_spline_filter1d_ld, 0, np.asarray(img).astype(LD))
    return np.apply_along_axis(_spline_filter1d_ld, 1, out)


# ---- the maps the post and the host chain must refuse alike ----

def refusal_maps():
    """name -> (map, exception type name): 'TypeError' (too few points for a fit) or 'LinAlgError'
    (Y^2 = 1 on a two-row map: the five-term system is exactly singular)."""
    rng = np.random.default_rng(11)
    few = np.full((8, 8), np.nan)
    few[2, 3], few[4, 1], few[5, 6] = 1.0, 2.5, -0.5
    return {
        "2x2": (7.0 + rng.standard_normal((2, 2)), "TypeError"),
        "8x8 with 3 points": (few, "TypeError"),
        "8x8 all NaN": (np.full((8, 8), np.nan), "TypeError"),
        "2x5": (7.0 + rng.standard_normal((2, 5)), "LinAlgError"),
        "2x3": (7.0 + rng.standard_normal((2, 3)), "LinAlgError"),
    }


def nan_column_map(ny=64, nx=100):
    """An aperture map whose column nx // 4 is all NaN: the rotation estimate is NaN."""
    m = make(ny, nx).copy()
    m[:, nx // 4] = np.nan
    return m
