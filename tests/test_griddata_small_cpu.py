"""What the small-lattice GPU tests (test_griddata_small_gpu.py) assume of their reference, checked on
the host, so that a failure there is about the kernels: the structured triangulation is qhull's on
every SMALL shape (scipy is a valid reference, no ambiguity mask), the converged scipy interpolant's
own noise floor, how many targets sit on a hull edge, and the cone solve's interior arithmetic."""
import numpy as np
import pytest

from griddata_ref import (SMALL, SMALL_TARGETS, _cell_tris_np, _pockets, converged_scipy, hull_distance, interior_cells,
                          interior_mask, near_hull, small_lattice, small_targets)

NEAR_HULL_CAP = 0.03  # the largest share of targets the GPU tests may leave out of the NaN-mask comparison


@pytest.mark.parametrize("nv,nh", SMALL)
def test_small_structured_triangulation_equals_qhull(nv, nh):
    """In-circle cell splits + akb_gd_pockets (host) = scipy's Delaunay, triangle for triangle
    (test_host.py::test_structured_triangulation_equals_qhull's check, on the SMALL lattices)."""
    from akbraytracing_amd import build
    from scipy.spatial import Delaunay
    build.build(verbose=False)
    X, Y, _ = small_lattice(nv, nh)
    tri, nbr, edge, xptr, xidx = _pockets(X, Y)
    ours = np.concatenate([_cell_tris_np(X, Y), tri])
    q = Delaunay(np.stack([X.ravel(), Y.ravel()], 1)).simplices
    print(f"({nv},{nh}): {len(tri)} pockets")
    assert len(ours) == len(q)
    assert set(map(tuple, np.sort(ours, 1))) == set(map(tuple, np.sort(q, 1)))
    assert xptr[-1] == len(xidx) and len(xidx) % 2 == 0
    assert np.count_nonzero(edge >= 0) == np.count_nonzero(nbr <= -2)


@pytest.mark.parametrize("nv,nh", SMALL)
def test_converged_scipy_noise_floor(nv, nh):
    """converged_scipy (tol 1e-12) against a tol 1e-15 solve: values to 1e-12 of the range, gradients
    to 1e-11 of their scale - the reference's own noise, three orders under the GPU tests' 1e-9 bars."""
    X, Y, F = small_lattice(nv, nh)
    a, b = converged_scipy(X, Y, F), converged_scipy(X, Y, F, tol=1e-15, maxiter=40000)
    ga, gb = a.grad.reshape(-1, 2), b.grad.reshape(-1, 2)
    dg = np.max(np.abs(ga - gb)) / np.max(np.abs(gb))
    gx, gy = small_targets(X, Y, *SMALL_TARGETS[1])
    GH, GV = np.meshgrid(gx, gy)
    va, vb = a(GH, GV), b(GH, GV)
    assert np.array_equal(np.isnan(va), np.isnan(vb))
    dv = np.nanmax(np.abs(va - vb)) / (np.nanmax(vb) - np.nanmin(vb))
    print(f"({nv},{nh}): values {dv:.1e} of the range, gradients {dg:.1e} of their scale")
    assert dv <= 1e-12 and dg <= 1e-11


def test_hull_distance_on_a_square():
    P = np.array([[0, 0], [2, 0], [2, 2], [0, 2], [1, 1], [1, 0]], float)  # an interior and a collinear point
    T = np.array([[1, 1], [1, 0.25], [3, 1], [3, 3], [0, 0], [-1, 2]], float)
    assert np.allclose(hull_distance(P, T), [1, 0.25, 1, np.sqrt(2), 0, 1], rtol=0, atol=1e-15)


@pytest.mark.parametrize("nv,nh", SMALL)
def test_targets_on_a_hull_edge_are_few(nv, nh):
    """Targets within 1e-9 of the extent of a hull edge (where the NaN mask is rounding's to decide):
    none, except on the nv == 3 lattices, whose left column has two vertices at x == X.min() so that
    the first target column lies on a hull edge; at most 3 % there."""
    X, Y, _ = small_lattice(nv, nh)
    for mx, my in SMALL_TARGETS:
        near = near_hull(X, Y, *small_targets(X, Y, mx, my))
        print(f"({nv},{nh}) {mx} x {my}: {near.sum()} of {near.size} targets on a hull edge")
        assert near.mean() <= NEAR_HULL_CAP
        if nv != 3:
            assert near.sum() == 0
        else:
            assert near[:, 1:].sum() == 0  # the first column only


def _owners(nv, nh):
    """A synthetic owner array: both triangles of every cell, a pocket id and an unclaimed target."""
    nc = (nv - 1) * (nh - 1)
    return np.concatenate([np.arange(2 * nc), [2 * nc, 2 * nc + 5, np.iinfo(np.int32).max]]).astype(np.int32)


def test_interior_plan_arithmetic():
    """interior_mask restates cone_interior(): nv, nh >= 2K + 6 for an interior cell - none at (33, 34)
    for K = 14, the one cell (16, 16) at (34, 34), cells K + 2 .. n - K - 4 = 3 .. 4 at (9, 9) for K = 1,
    two rows at (35, 40); pockets and unclaimed targets are never interior."""
    assert interior_cells(_owners(33, 34), 33, 34, 14) == []
    assert interior_cells(_owners(34, 34), 34, 34, 14) == [(16, 16)]
    assert interior_cells(_owners(9, 9), 9, 9, 1) == [(iv, ih) for iv in (3, 4) for ih in (3, 4)]
    assert interior_cells(_owners(35, 40), 35, 40, 14) == [(iv, ih) for iv in (16, 17) for ih in range(16, 23)]
    m, _, _ = interior_mask(_owners(34, 34), 34, 34, 14)
    assert m.sum() == 2 and not m[-3:].any()  # the cell's two triangles
    for nv, nh in SMALL:
        for K in (1, 2, 3, 7, 12, 14):
            cells = interior_cells(_owners(nv, nh), nv, nh, K)
            assert (len(cells) > 0) == (min(nv, nh) >= 2 * K + 6)
            assert len(cells) == max(nv - 2 * K - 5, 0) * max(nh - 2 * K - 5, 0)
