"""The conditions test_pupil_post_gpu.py's inputs must meet, asserted with the oracle alone (no GPU):
no discrete decision of the chain (a point kept or dropped by the 3-sigma filter, a rotated pixel
inside or outside the mask) sits where rounding could flip it, so a mask or kept-set mismatch on the
device is always a real failure; and the float64 oracle is itself within a tenth of the bars the
device is held to, measured against the same operations in np.longdouble.

A case that breaks a condition gets another seed (pupil_post_cases.SEEDS); the conditions stay.
"""
import numpy as np
import pytest

import oracle.psfcalc as OPC
import pupil_post_cases as C

EDGE_CASES = [(ny, nx, dr) for ny, nx in C.EDGE_SHAPES for dr in C.edge_drs(nx)]


def _threshold_margin(o):
    return float(np.min(np.abs(np.abs(o["res"]) - o["thr"])) / o["thr"])


@pytest.mark.parametrize("ny,nx", C.SHAPES)
def test_aperture_case_conditions(ny, nx):
    """Conditions 1 and 2 on an aperture-family map, and the generator's own promises (all finite
    below a side of 9; NaNs and at least 3 dropped outliers from there on)."""
    m, o = C.aperture_case(ny, nx)
    assert m.shape == (ny, nx)
    marg = _threshold_margin(o)
    dropped = int((np.abs(o["res"]) >= o["thr"]).sum())
    mm = float(np.min(np.abs(o["mask_rot"] - 0.5)))
    print(f"{ny}x{nx}: finite {np.isfinite(m).mean():.2f}, dropped {dropped}, nearest residual {marg:.2e} thr "
          f"from the threshold, rotation {o['deg']:.3f} deg, nearest rotated mask value {mm:.2e} from 0.5")
    assert marg > 1e-6
    assert mm > 1e-9
    if min(ny, nx) >= 9:
        assert np.isnan(m).any() and dropped >= 3
    else:
        assert np.isfinite(m).all()
    assert np.isfinite(o["rot"]) and np.isfinite(o["rotated"]).any()


@pytest.mark.parametrize("ny,nx,dr", EDGE_CASES)
def test_edge_case_conditions(ny, nx, dr):
    """Conditions 1 and 2 on an edge-family map, and that its rotation estimate is atan(dr / h)
    exactly: the first valid rows at columns nx // 4 and 3 nx // 4 differ by dr."""
    m, o = C.edge_case(ny, nx, dr)
    c1, c3 = nx // 4, nx * 3 // 4
    first = [int(np.flatnonzero(np.isfinite(m[:, c]))[0]) for c in (c1, c3)]
    assert first[0] - first[1] == dr
    assert o["rot"] == np.arctan(dr / (c1 - c3))
    marg = _threshold_margin(o)
    mm = float(np.min(np.abs(o["mask_rot"] - 0.5)))
    print(f"{ny}x{nx} dr={dr}: rotation {o['deg']:.4f} deg, nearest residual {marg:.2e} thr from the threshold, "
          f"nearest rotated mask value {mm:.2e} from 0.5, rotated finite {np.isfinite(o['rotated']).mean():.2f}")
    assert marg > 1e-6
    assert mm > 1e-9
    assert np.isfinite(o["rotated"]).any()


def test_edge_family_angles_cover_the_octants():
    """The edge family's angles: exact 0, both signs, exactly -+45 degrees, and |angle| > 45 of both
    signs (cosdg / sindg's second octant)."""
    for ny, nx in C.EDGE_SHAPES:
        deg = np.array([C.edge_case(ny, nx, dr)[1]["deg"] for dr in C.edge_drs(nx)])
        assert deg[0] == 0.0
        assert 45.0 in deg and -45.0 in deg
        assert (deg > 45.0).any() and (deg < -45.0).any()
        assert ((deg > 0) & (deg < 45)).any() and ((deg < 0) & (deg > -45)).any()


@pytest.mark.parametrize("ny,nx", C.SHAPES)
def test_oracle_fit_against_long_double(ny, nx):
    """Condition 3, the fit: oracle.pupilmap (float64 lstsq on the index basis) within 1e-13 of the
    range of the same two fits solved in np.longdouble - a tenth of the device's 1e-12 bar."""
    _, o = C.aperture_case(ny, nx)
    ref, dropped = C.plane_correction_ld(o["z"])
    assert dropped == int((np.abs(o["res"]) >= o["thr"]).sum())
    assert np.array_equal(np.isnan(ref), np.isnan(o["corrected"]))
    d = float(np.nanmax(np.abs(o["corrected"] - ref))) / o["rng"]
    print(f"{ny}x{nx}: float64 oracle fit vs long double {d:.2e} of the range")
    assert d <= 1e-13


@pytest.mark.parametrize("ny,nx", [(3, 3), (9, 17), (100, 100), (129, 127), (256, 256), (40, 1500)])
def test_oracle_prefilter_against_long_double(ny, nx):
    """Condition 3, the prefilter: oracle.psfcalc.spline_filter within 1e-14 of max|coef| of the same
    recursion in np.longdouble - a tenth of the device's 1e-13 bar - on the map and on its mask."""
    _, o = C.aperture_case(ny, nx)
    c = o["corrected"]
    for name, a in (("map", np.nan_to_num(c)), ("mask", (~np.isnan(c)).astype(float))):
        r = C.spline_filter_ld(a)
        d = float(np.max(np.abs(OPC.spline_filter(a) - r)) / np.max(np.abs(r)))
        print(f"{ny}x{nx} {name}: float64 oracle prefilter vs long double {d:.2e} of max|coef|")
        assert d <= 1e-14


def test_refusal_maps_are_what_they_claim():
    """The refused maps' point counts, and that a two-row map's scaled Y^2 is identically 1."""
    r = C.refusal_maps()
    assert np.isfinite(r["2x2"][0]).sum() == 4
    assert np.isfinite(r["8x8 with 3 points"][0]).sum() == 3
    assert np.isfinite(r["8x8 all NaN"][0]).sum() == 0
    for k in ("2x5", "2x3"):
        assert r[k][0].shape[0] == 2 and np.isfinite(r[k][0]).all() and r[k][0].size >= 5
    Y = (2.0 * np.arange(2) - 1) / 1.0
    assert np.array_equal(Y * Y, np.ones(2))
    m = C.nan_column_map()
    assert np.isnan(m[:, m.shape[1] // 4]).all() and np.isfinite(m).sum() > 100
    o = C.oracle_chain(m)
    assert np.isnan(o["rot"]) and np.isnan(o["rotated"]).all()
