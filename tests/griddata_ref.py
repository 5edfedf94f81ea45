"""References and lattices shared by the griddata tests (test_gpu_parity.py, test_host.py,
test_griddata_small_cpu.py, test_griddata_small_gpu.py, test_cone_parts_gpu.py): the deformed test
lattices, the structured triangulation and scipy's gradient problem restated in numpy, a converged
scipy Clough-Tocher interpolant, and the cone solve's plan arithmetic restated on arrays."""
import ctypes

import numpy as np
import torch


def _scale_tol(ref):
    """1e-6 of the map's range, or 64 ulp of its largest magnitude (the 65x65 Wave2 carries a
    ~1e7 nm offset, so rounding alone is ~1e-8 there)."""
    return max(1e-6 * (np.nanmax(ref) - np.nanmin(ref)), 64 * np.spacing(np.nanmax(np.abs(ref))))


def _lattice(nv, nh, seed):
    u, v = np.meshgrid(np.linspace(-1, 1, nh), np.linspace(-1, 1, nv))
    X = u * 1e-4 + 3e-6 * v ** 2 - 2e-6 * u * v + 1e-6 * v ** 3
    Y = v * 1.3e-4 + 4e-6 * u ** 2 + 1e-6 * u ** 3
    rng = np.random.default_rng(seed)
    F = 0.3 * u ** 2 - 0.2 * u * v + 0.1 * np.sin(3 * v) + 1e-3 * rng.standard_normal(u.shape)
    return X, Y, F


# The small and thin lattices: below every kernel's tile or strip constant (62-cell strips with
# segments of 8 rows, 60 / 62 owned columns and 24 rows a sweep wave, 8 x 8 claim blocks, 16 x 32 band
# tiles) and around the cone solve's interior threshold 2K + 6 (34 at K = 14).
SMALL = [(2, 2), (2, 3), (3, 2), (2, 9), (9, 2), (3, 3), (3, 17), (5, 5), (7, 64), (64, 7), (9, 9), (16, 17),
         (31, 31), (33, 34), (34, 34), (35, 40), (63, 65)]
SMALL_TARGETS = [(23, 29), (71, 77)]  # (mx, my): coarser than some cells / finer than every cell


def small_lattice(nv, nh):
    """_lattice(nv, nh) with square-ish cells: X, Y, F (nv, nh)."""
    X, Y, F = _lattice(nv, nh, seed=100 * nv + nh)
    return X * (nh / nv), Y, F


def small_targets(X, Y, mx, my):
    """The product's own axis form (linspaces over the extent), with some targets outside the hull."""
    return np.linspace(X.min(), X.max(), mx), np.linspace(Y.min() - 1e-6, Y.max(), my)


def small_values(F, nvals):
    """One to three value sets on a lattice (the cone tests' three)."""
    f = F.ravel()
    return np.stack([f, np.cos(3 * f), f ** 2])[:nvals]


def converged_scipy(X, Y, F, tol=1e-12, maxiter=4000):
    """scipy's own Clough-Tocher interpolant on qhull's triangulation with its gradient iteration
    run to tol: an independent, converged reference for the gradients (.grad) and the values."""
    from scipy.interpolate import CloughTocher2DInterpolator
    from scipy.spatial import Delaunay
    P = np.stack([np.ravel(X), np.ravel(Y)], 1)
    return CloughTocher2DInterpolator(Delaunay(P), np.ravel(F), tol=tol, maxiter=maxiter)


def hull_distance(points, targets):
    """Each target's distance to the nearest edge (segment) of the points' convex hull: (len(targets),).
    Plain numpy: Andrew's monotone chain, then point-to-segment distances."""
    P = np.unique(np.asarray(points, np.float64).reshape(-1, 2), axis=0)  # sorted by x, then y

    def chain(pts):
        h = []
        for p in pts:
            while len(h) >= 2 and ((h[-1][0] - h[-2][0]) * (p[1] - h[-2][1])
                                   - (h[-1][1] - h[-2][1]) * (p[0] - h[-2][0])) <= 0:
                h.pop()
            h.append(p)
        return h

    lower, upper = chain(P), chain(P[::-1])
    H = np.array(lower[:-1] + upper[:-1])
    A, B = H, np.roll(H, -1, axis=0)
    T = np.asarray(targets, np.float64).reshape(-1, 2)
    d = np.full(len(T), np.inf)
    for a, b in zip(A, B):
        e = b - a
        s = np.clip(((T - a) @ e) / (e @ e), 0.0, 1.0)
        d = np.minimum(d, np.hypot(*(T - (a + s[:, None] * e)).T))
    return d


def near_hull(X, Y, gx, gy, rel=1e-9):
    """(my, mx) mask of the targets within rel of the points' extent of a hull edge: where the inside
    test is decided by rounding, on either side."""
    GH, GV = np.meshgrid(gx, gy)
    P = np.stack([np.ravel(X), np.ravel(Y)], 1)
    ext = max(np.ptp(P[:, 0]), np.ptp(P[:, 1]))
    return (hull_distance(P, np.stack([GH.ravel(), GV.ravel()], 1)) <= rel * ext).reshape(GH.shape)


def interior_mask(owner, nv, nh, K):
    """cone_interior() (akb_griddata.hip) on an owner array: True where the target's triangle lies in a
    cell whose (2K + 4)^2 box is clear of the ring by one vertex (a patch forms it), and the cells'
    (iv, ih) arrays (meaningless where the owner is unclaimed or a pocket)."""
    o = np.asarray(owner).astype(np.int64)
    cell_tri = o < 2 * (nv - 1) * (nh - 1)
    c = np.where(cell_tri, o >> 1, 0)
    iv, ih = c // (nh - 1), c % (nh - 1)
    m = cell_tri & (iv - K - 1 >= 1) & (iv + K + 2 <= nv - 2) & (ih - K - 1 >= 1) & (ih + K + 2 <= nh - 2)
    return m, iv, ih


def interior_cells(owner, nv, nh, K):
    """The distinct interior target cells of an owner array, sorted: [(iv, ih), ...]."""
    m, iv, ih = interior_mask(owner, nv, nh, K)
    return sorted(set(zip(iv[m].tolist(), ih[m].tolist())))


# ----------------------------------------------------------------------------- the triangulation (host)

def _cell_diag_np(X, Y):
    """Cell split by the in-circle test (the rule the device cell pass applies): (nv - 1, nh - 1) bool,
    True = p01-p10."""
    x0, y0 = X[:-1, :-1], Y[:-1, :-1]
    bx, by = X[:-1, 1:] - x0, Y[:-1, 1:] - y0
    cx, cy = X[1:, 1:] - x0, Y[1:, 1:] - y0
    dx, dy = X[1:, :-1] - x0, Y[1:, :-1] - y0
    adx, ady, bdx, bdy, cdx, cdy = -dx, -dy, bx - dx, by - dy, cx - dx, cy - dy
    A, B, C = adx * adx + ady * ady, bdx * bdx + bdy * bdy, cdx * cdx + cdy * cdy
    det = adx * (bdy * C - B * cdy) - ady * (bdx * C - B * cdx) + A * (bdx * cdy - bdy * cdx)
    o = bx * cy - by * cx
    return np.where(o > 0, det, -det) > 0


def _cell_tris_np(X, Y):
    """Cell split by the in-circle test (the rule the device cell pass applies), as vertex triples."""
    nv, nh = X.shape
    diag = _cell_diag_np(X, Y)
    iv, ih = np.meshgrid(np.arange(nv - 1), np.arange(nh - 1), indexing="ij")
    p00 = iv * nh + ih
    p01, p10, p11 = p00 + 1, p00 + nh, p00 + nh + 1
    t0 = np.where(diag[..., None], np.stack([p00, p01, p10], -1), np.stack([p00, p01, p11], -1))
    t1 = np.where(diag[..., None], np.stack([p01, p11, p10], -1), np.stack([p00, p11, p10], -1))
    return np.concatenate([t0.reshape(-1, 3), t1.reshape(-1, 3)])


def _ring_np(nv, nh):
    return np.array([ih for ih in range(nh - 1)] + [iv * nh + nh - 1 for iv in range(nv - 1)] +
                    [(nv - 1) * nh + ih for ih in range(nh - 1, 0, -1)] + [iv * nh for iv in range(nv - 1, 0, -1)])


def _pockets(X, Y):
    from akbraytracing_amd import _lib
    L = _lib.lib()
    nv, nh = X.shape
    r = _ring_np(nv, nh)
    rx, ry = np.ascontiguousarray(X.ravel()[r]), np.ascontiguousarray(Y.ravel()[r])
    cap = len(r)
    tri, nbr = np.zeros((cap, 3), np.int32), np.zeros((cap, 3), np.int32)
    edge, xptr, xidx, n = np.zeros(cap, np.int32), np.zeros(cap + 1, np.int32), np.zeros(6 * cap, np.int32), np.zeros(1, np.int32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    _lib.check(L.akb_gd_pockets(p(rx), p(ry), nv, nh, cap, p(n), p(tri), p(nbr), p(edge), p(xptr), p(xidx)))
    return tri[:n[0]], nbr[:n[0]], edge, xptr, xidx[:xptr[-1]]


# ----------------------------------------------------------------------------- the gradients

def _interp_k_sweeps(cg, vals, gx, gy, K):
    """akb_gd_eval_f64 on the global Chebyshev iteration's gradients after exactly K sweeps."""
    from akbraytracing_amd import _lib
    from akbraytracing_amd import device as D
    f = vals if isinstance(vals, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(vals))
    f = f.to(cg.dev).reshape(-1, cg.nv * cg.nh).contiguous()
    grad = cg.gradients(f, maxiter=K, check_every=K, adaptive=False, tol=0.0)
    gxt, gyt = torch.from_numpy(gx).to(cg.dev), torch.from_numpy(gy).to(cg.dev)
    mx, my, nv = gx.size, gy.size, int(f.shape[0])
    owner = torch.empty(mx * my, dtype=torch.int32, device=cg.dev)
    out = torch.empty((nv, my, mx), dtype=torch.float64, device=cg.dev)
    _lib.check(_lib.lib().akb_gd_eval_f64(*cg._tri_args(), D.ptr(gxt), mx, D.ptr(gyt), my, D.ptr(f), D.ptr(grad), nv,
                                          D.ptr(owner), D.ptr(out), D.stream_handle()))
    return out.cpu().numpy()


def _gradient_system(cg, f):
    """scipy's gradient problem on cg's triangulation in numpy: per vertex the local solve's
    Q = 4 sum r^-3 e e^T and s = sum (6 (f_i - f_j) + 2 e.g_j) r^-3 e over its edges (lattice edges by
    the cell diagonals, a ring vertex's pocket chords from xptr / xidx) as the sparse fixed-point
    problem g = c + J g (_interpnd.pyx's estimate_gradients_2d_global). Returns (J, c)."""
    import scipy.sparse as sp
    nv, nh = cg.nv, cg.nh
    x, y = cg.x.cpu().numpy(), cg.y.cpu().numpy()
    d = cg.diag.cpu().numpy().reshape(nv - 1, nh - 1).astype(bool)
    idx = np.arange(nv * nh).reshape(nv, nh)
    E = [(idx[:, :-1].ravel(), idx[:, 1:].ravel()), (idx[:-1, :].ravel(), idx[1:, :].ravel()),
         (idx[:-1, :-1][~d], idx[1:, 1:][~d]), (idx[:-1, 1:][d], idx[1:, :-1][d])]
    I = np.concatenate([e[0] for e in E])
    J = np.concatenate([e[1] for e in E])
    I, J = np.concatenate([I, J]), np.concatenate([J, I])
    xptr, xidx = cg.xptr.cpu().numpy(), cg.xidx.cpu().numpy()
    ring = np.concatenate([idx[0, :-1], idx[:-1, -1], idx[-1, :0:-1], idx[:0:-1, 0]])
    ci = np.repeat(ring, np.diff(xptr))
    I, J = np.concatenate([I, ci]), np.concatenate([J, xidx[:xptr[-1]]])
    ex, ey = x[J] - x[I], y[J] - y[I]
    r3 = (ex * ex + ey * ey) ** -1.5
    n = nv * nh
    q = [4 * np.bincount(I, w, n) for w in (ex * ex * r3, ex * ey * r3, ey * ey * r3)]
    Qi = np.linalg.inv(np.stack([np.stack([q[0], q[1]], -1), np.stack([q[1], q[2]], -1)], -2))
    w6 = 6 * (f[I] - f[J])
    s0 = np.stack([np.bincount(I, w6 * ex * r3, n), np.bincount(I, w6 * ey * r3, n)], 1)
    c = -np.einsum("nij,nj->ni", Qi, s0).ravel()
    rows, cols, vals = [], [], []
    for (a_, b_, w) in ((0, 0, ex * ex), (0, 1, ex * ey), (1, 0, ex * ey), (1, 1, ey * ey)):
        rows.append(2 * I + a_)
        cols.append(2 * J + b_)
        vals.append(2 * w * r3)
    A = sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(2 * n, 2 * n))
    return -(sp.block_diag(list(Qi), format="csr") @ A), c
