"""griddata on small and thin lattices (griddata_ref.SMALL: 2 x 2 up to 63 x 65), where every kernel's
tile or strip is larger than the lattice, band_tiles() clips its regions, and the cone solve has no,
one or one row of interior target cells: the cell pass, the four claim routes, the gradients and
values against a converged scipy Clough-Tocher interpolant (tests/test_griddata_small_cpu.py pins
that reference's own preconditions), and the cone solve against the global K-sweep iteration."""
import functools

import numpy as np
import pytest
import torch

from griddata_ref import (SMALL, SMALL_TARGETS, _cell_diag_np, _gradient_system, _interp_k_sweeps, _scale_tol,
                          converged_scipy, interior_cells, interior_mask, near_hull, small_lattice, small_targets,
                          small_values)

pytestmark = pytest.mark.gpu

NEAR_HULL_CAP = 0.03  # test_griddata_small_cpu.py::test_targets_on_a_hull_edge_are_few
UNCLAIMED = np.iinfo(np.int32).max
CONE_K = (1, 2, 3, 7, 12, 14)


@functools.lru_cache(maxsize=None)
def _reference(nv, nh, k):
    """The converged scipy interpolant of value set k on the (nv, nh) lattice: built once, never changed."""
    X, Y, F = small_lattice(nv, nh)
    return converged_scipy(X, Y, small_values(F, 3)[k])


def _grid(nv, nh):
    from akbraytracing_amd.griddata import CubicGrid
    X, Y, F = small_lattice(nv, nh)
    return X, Y, F, CubicGrid(X.ravel(), Y.ravel(), nv, nh)


def _claims(cg, gx, gy, work):
    """akb_gd_claims_f64 over every row: the owners (host)."""
    from akbraytracing_amd import _lib
    from akbraytracing_amd import device as D
    tgx, tgy = torch.tensor(gx, device=cg.dev), torch.tensor(gy, device=cg.dev)
    owner = torch.empty(gx.size * gy.size, dtype=torch.int32, device=cg.dev)
    _lib.check(_lib.lib().akb_gd_claims_f64(D.ptr(cg.x), D.ptr(cg.y), cg.nv, cg.nh, D.ptr(cg.diag), cg.npock,
                                            D.ptr(cg.ptri), D.ptr(cg.pnbr), D.ptr(cg.edge_tri), 0, -1, 1, D.ptr(tgx),
                                            gx.size, D.ptr(tgy), gy.size, D.ptr(owner),
                                            None if work is None else D.ptr(work), None))
    torch.cuda.synchronize()
    return owner.cpu().numpy()


def _cone_work(cg, mx, my, nvals=1):
    from akbraytracing_amd import _lib
    from akbraytracing_amd import device as D
    need = int(_lib.lib().akb_gd_cone_work_bytes(cg.nv, cg.nh, mx, my, nvals))
    return torch.empty(need // 8 + 1, dtype=D.F64, device=cg.dev)


def _eval_owners(cg, gx, gy):
    """akb_gd_eval_f64's owners (its claim kernel: per-cell blocks, or per-triangle under AKB_GD_CLAIM_TRI)."""
    from akbraytracing_amd import _lib
    from akbraytracing_amd import device as D
    n = cg.nv * cg.nh
    f = torch.zeros(n, dtype=torch.float64, device=cg.dev)
    grad = torch.zeros(2 * n, dtype=torch.float64, device=cg.dev)
    tgx, tgy = torch.tensor(gx, device=cg.dev), torch.tensor(gy, device=cg.dev)
    owner = torch.empty(gx.size * gy.size, dtype=torch.int32, device=cg.dev)
    out = torch.empty(gx.size * gy.size, dtype=torch.float64, device=cg.dev)
    _lib.check(_lib.lib().akb_gd_eval_f64(*cg._tri_args(), D.ptr(tgx), gx.size, D.ptr(tgy), gy.size, D.ptr(f),
                                          D.ptr(grad), 1, D.ptr(owner), D.ptr(out), None))
    torch.cuda.synchronize()
    return owner.cpu().numpy()


@pytest.mark.parametrize("nv,nh", SMALL)
def test_small_cell_pass(gpu, nv, nh):
    """The cell pass on a lattice below its 62-cell strips and 8-row segments: the in-circle splits,
    no error flag (bits 0, 1, 2, 5 clear and one orientation: the word is 8 or 16, the orientation
    bits being set on every lattice), a clean pocket status, and the pass with the claims fused in
    (then the pockets' claims) giving the two-pass owners and diagonals bit for bit."""
    from akbraytracing_amd import _lib
    from akbraytracing_amd import device as D
    L = _lib.lib()
    X, Y, F, cg = _grid(nv, nh)
    assert np.array_equal(cg.diag.cpu().numpy().reshape(nv - 1, nh - 1).astype(bool), _cell_diag_np(X, Y))
    dev = cg.dev
    diag2 = torch.full_like(cg.diag, 7)
    flags2 = torch.zeros(1, dtype=torch.int32, device=dev)
    ring = torch.empty(2 * cg.L, dtype=torch.float64, device=dev)
    _lib.check(L.akb_gd_cells_f64(D.ptr(cg.x), D.ptr(cg.y), nv, nh, D.ptr(diag2), 1e-10, D.ptr(flags2),
                                  D.ptr(ring[:cg.L]), D.ptr(ring[cg.L:]), None))
    torch.cuda.synchronize()
    assert int(flags2.item()) in (8, 16)
    assert torch.equal(diag2, cg.diag)
    assert int(cg._status.item()) == 0
    for mx, my in SMALL_TARGETS:
        gx, gy = small_targets(X, Y, mx, my)
        want = _claims(cg, gx, gy, None)
        tgx, tgy = torch.tensor(gx, device=dev), torch.tensor(gy, device=dev)
        got = torch.empty(mx * my, dtype=torch.int32, device=dev)
        diag = torch.full_like(cg.diag, 7)
        flags = torch.zeros(1, dtype=torch.int32, device=dev)
        _lib.check(L.akb_gd_cells_claims_f64(D.ptr(cg.x), D.ptr(cg.y), nv, nh, D.ptr(diag), 1e-10, D.ptr(flags),
                                             D.ptr(tgx), mx, D.ptr(tgy), my, D.ptr(got), None))
        _lib.check(L.akb_gd_claim_pockets_f64(D.ptr(cg.x), D.ptr(cg.y), nv, nh, D.ptr(diag), cg.npock, D.ptr(cg.ptri),
                                              D.ptr(tgx), mx, D.ptr(tgy), my, D.ptr(got), None))
        torch.cuda.synchronize()
        assert torch.equal(diag, cg.diag)
        assert int(flags.item()) == int(flags2.item())
        assert np.array_equal(got.cpu().numpy(), want)


@pytest.mark.parametrize("nv,nh", SMALL)
def test_small_claim_routes_agree(gpu, monkeypatch, nv, nh):
    """The four claim routes - per-cell blocks, per-triangle, akb_gd_claims_f64 without a work buffer
    (blocks) and with it (scan + hit) - give the same owners on lattices below their 8 x 8 blocks, on
    targets coarser and finer than the cells; the claimed targets are scipy's inside ones."""
    X, Y, F, cg = _grid(nv, nh)
    for mx, my in SMALL_TARGETS:
        gx, gy = small_targets(X, Y, mx, my)
        blocks = _eval_owners(cg, gx, gy)
        monkeypatch.setenv("AKB_GD_CLAIM_TRI", "1")
        tri = _eval_owners(cg, gx, gy)
        monkeypatch.delenv("AKB_GD_CLAIM_TRI")
        plain = _claims(cg, gx, gy, None)
        scan = _claims(cg, gx, gy, _cone_work(cg, mx, my))
        assert np.array_equal(blocks, tri)
        assert np.array_equal(plain, tri)
        assert np.array_equal(scan, tri)
        ntri = 2 * (nv - 1) * (nh - 1) + cg.npock
        claimed = tri != UNCLAIMED
        assert tri[claimed].min() >= 0 and tri[claimed].max() < ntri
        GH, GV = np.meshgrid(gx, gy)
        inside = _reference(nv, nh, 0).tri.find_simplex(np.stack([GH.ravel(), GV.ravel()], 1)) >= 0
        near = near_hull(X, Y, gx, gy).ravel()
        assert near.mean() <= NEAR_HULL_CAP
        assert np.array_equal(claimed[~near], inside[~near])
        assert 0.3 < claimed.mean() < 1.0  # targets inside and outside the hull


@pytest.mark.parametrize("nv,nh", SMALL)
def test_small_gradients(gpu, nv, nh):
    """The register sweeps (k_gd_sweeps<2, ..> on a pair of value sets, <1, ..> on a single one) and the
    ring kernels on lattices below a wave's 60 / 62 owned columns and 24 rows: converged (tol 1e-12)
    against scipy's own converged gradients to 1e-9 of max|grad| (test_gradient_iteration_vs_numpy_system's
    bar against its direct solve); five sweeps from zero against the numpy restatement of the same
    iteration to 1e-12 of the scale; two batchings of the launches and one, two or three value sets
    at a time give the same bits."""
    from akbraytracing_amd.griddata import chebyshev_weights
    X, Y, F, cg = _grid(nv, nh)
    n = nv * nh
    vals = small_values(F, 3)
    gc = cg.gradients(vals, tol=1e-12).cpu().numpy()
    assert cg.sweeps < 400 and cg.history[-1] < 1e-12
    for k in range(3):
        ref = _reference(nv, nh, k).grad.reshape(n, 2)
        scale = np.max(np.abs(ref))
        d = np.max(np.abs(gc[k] - ref)) / scale
        print(f"({nv},{nh}) set {k}: gradients {d:.2e} of max|grad| from converged scipy ({cg.sweeps} sweeps)")
        assert d <= 1e-9
    om = chebyshev_weights(8)
    g5 = cg.gradients(vals, maxiter=5, check_every=5, tol=0.0).cpu().numpy()
    for k in range(3):
        Jm, c = _gradient_system(cg, vals[k])
        xp, xc = np.zeros_like(c), c.copy()  # x_0 = 0, x_1 = the plain sweep
        for j in range(1, 5):
            xp, xc = xc, om[j] * (Jm @ xc + c - xp) + xp
        assert np.max(np.abs(g5[k].ravel() - xc)) <= 1e-12 * np.max(np.abs(xc)), k
    assert np.array_equal(g5, cg.gradients(vals, maxiter=5, check_every=3, adaptive=False, tol=0.0).cpu().numpy())
    for nvals in (1, 2):  # the single set through <1, ..>, the pair through <2, ..>
        part = cg.gradients(vals[:nvals], maxiter=5, check_every=5, tol=0.0).cpu().numpy()
        assert np.array_equal(part, g5[:nvals]), nvals
        assert np.array_equal(part, cg.gradients(vals[:nvals], maxiter=5, check_every=2, adaptive=False, tol=0.0).cpu().numpy())


@pytest.mark.parametrize("nv,nh", SMALL)
def test_small_values(gpu, nv, nh):
    """interp (tol 1e-12) against the converged scipy interpolant at max(1e-9 of the range, 64 ulp): a
    Clough-Tocher value is linear in the gradients (held to 1e-9 of their scale above) and on these
    coarse lattices gradient scale x edge length is about the range; four orders over the reference's
    measured noise. The same NaN mask, the targets within 1e-9 of the extent of a hull edge left out
    of the mask comparison only (at most 3 %). The drop-in griddata at its default tolerance stays
    within 1e-6 of the range of scipy.interpolate.griddata."""
    from scipy.interpolate import griddata as sp_griddata
    from akbraytracing_amd.griddata import griddata
    X, Y, F, cg = _grid(nv, nh)
    vals = small_values(F, 3)
    for mx, my in SMALL_TARGETS:
        gx, gy = small_targets(X, Y, mx, my)
        GH, GV = np.meshgrid(gx, gy)
        near = near_hull(X, Y, gx, gy)
        assert near.mean() <= NEAR_HULL_CAP
        for nvals in (1, 3):
            got = cg.interp(vals[:nvals], gx, gy, tol=1e-12).cpu().numpy()
            for k in range(nvals):
                ref = _reference(nv, nh, k)(GH, GV)
                assert np.array_equal(np.isnan(got[k])[~near], np.isnan(ref)[~near])
                both = np.isfinite(got[k]) & np.isfinite(ref)
                assert both.mean() > 0.3
                rng_ = np.nanmax(ref) - np.nanmin(ref)
                d = np.max(np.abs(got[k] - ref)[both])
                print(f"({nv},{nh}) {mx} x {my} set {k} of {nvals}: values {d / rng_:.2e} of the range from converged "
                      f"scipy, {near.sum()} of {near.size} targets on a hull edge")
                assert d <= max(1e-9 * rng_, 64 * np.spacing(np.nanmax(np.abs(ref))))
        want = sp_griddata((X.ravel(), Y.ravel()), F.ravel(), (GH, GV), method="cubic")
        drop = griddata((X.ravel(), Y.ravel()), F.ravel(), (GH, GV), method="cubic", grid_shape=(nv, nh))
        assert np.array_equal(np.isnan(drop)[~near], np.isnan(want)[~near])
        both = np.isfinite(drop) & np.isfinite(want)
        d = np.max(np.abs(drop - want)[both])
        print(f"({nv},{nh}) {mx} x {my}: drop-in griddata {d / (np.nanmax(want) - np.nanmin(want)):.2e} of the range "
              f"from scipy.interpolate.griddata")
        assert d <= _scale_tol(want)


@pytest.mark.parametrize("nv,nh", SMALL)
def test_small_cone_equals_global_sweeps(gpu, nv, nh):
    """The cone solve where a lattice is thinner than the band (every band_tiles region clipped, no
    interior target at all for min(nv, nh) < 2K + 6), with exactly one interior cell ((34, 34) at
    K = 14) and with two rows of them ((35, 40) at K = 14), K = 1 and 2 included (the patches' Q == 0
    steps): the global iteration's K-sweep values bit for bit, NaN mask included, for one to three
    value sets; both change words finite and non-negative. The 71 x 77 targets are finer than every
    cell."""
    X, Y, F, cg = _grid(nv, nh)
    mx, my = SMALL_TARGETS[1]
    gx, gy = small_targets(X, Y, mx, my)
    owner = _claims(cg, gx, gy, _cone_work(cg, mx, my))
    counts = []
    for i, K in enumerate(CONE_K):
        nvals = 1 + (i + nv + nh) % 3
        cells = interior_cells(owner, nv, nh, K)
        counts.append(len(cells))
        if min(nv, nh) < 2 * K + 6:
            assert cells == []  # everything through k_gd_cone_band
            assert not interior_mask(owner, nv, nh, K)[0].any()
        else:
            assert len(cells) > 0
        if (nv, nh, K) == (34, 34, 14):
            assert cells == [(16, 16)]
        if (nv, nh, K) == (35, 40, 14):
            assert cells == [(iv, ih) for iv in (16, 17) for ih in range(16, 23)]
        vals = small_values(F, nvals)
        got = cg.interp_cone(vals, gx, gy, sweeps=K).cpu().numpy()
        change = cg.cone_change.cpu().numpy().view(np.float64)
        want = _interp_k_sweeps(cg, vals, gx, gy, K)
        assert np.array_equal(got, want, equal_nan=True), K
        assert np.array_equal(np.isnan(got[0]).ravel(), owner == UNCLAIMED), K
        assert np.all(np.isfinite(change)) and np.all(change >= 0), (K, change)
    print(f"({nv},{nh}): interior target cells for K in {CONE_K}: {counts}")
    assert 0.3 < np.isfinite(got).mean() < 1.0
