"""akb_pupil_post_f64 on every map shape its entry point admits (MI355X): each stage against the
float64 oracle (oracle.pupilmap, oracle.psfcalc - themselves held to a tenth of these bars against
np.longdouble by test_pupil_post_cpu.py), against numpy / scipy.special bit for bit where the kernel
promises their bits, and against the host-driven chain. pupil_post_cases.py lists the shapes and
the branch of csrc/akb_psfcalc.hip each one reaches; test_pupil_post_cpu.py shows that no kept-or-
dropped or inside-or-outside decision on these inputs is within rounding of flipping, so every mask
is compared for equality.

Bars (the project's own): maps 1e-12 of the corrected map's range (test_pupil_post_equals_host_chain),
the threshold 1e-12 relative, the angle 2 ulp, the prefilter 1e-13 of max|coef| (the coefficients
enter a rotated pixel with non-negative weights summing to one: a tenth of the rotated map's bar).
"""
import warnings

import numpy as np
import pytest
import torch
from scipy.special import cosdg, sindg

import oracle.psfcalc as OPC
import pupil_post_cases as C

pytestmark = pytest.mark.gpu

EDGE_CASES = [(ny, nx, dr) for ny, nx in C.EDGE_SHAPES for dr in C.edge_drs(nx)]
HEAD = 16  # the post's work buffer: 16 clock words, then the (2, ny, nx) prefilter coefficients


def _bits(a):
    return np.asarray(a, dtype=np.float64).view(np.uint64)


def _same_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _close(got, want, bar, what):
    """Equal NaN masks and values within bar; returns the largest distance."""
    assert np.array_equal(np.isnan(got), np.isnan(want)), f"{what}: NaN masks differ"
    d = float(np.nanmax(np.abs(got - want))) if np.isfinite(want).any() else 0.0
    assert d <= bar, f"{what}: {d:.3e} > {bar:.3e}"
    return d


def _lines_prefilter(corrected_dev):
    """The coefficients akb_rotate_with_nan_f64 leaves in its work buffer for a device map: the NaN
    split and spline_line on a thread per line (k_spline_lines), both axes."""
    from akbraytracing_amd import _lib
    from akbraytracing_amd import device as D
    L = _lib.lib()
    ny, nx = (int(v) for v in corrected_dev.shape)
    work = torch.empty(int(L.akb_rotate_work_bytes(ny, nx)) // 8, dtype=torch.float64, device=corrected_dev.device)
    out, opd = torch.empty_like(corrected_dev), torch.empty_like(corrected_dev)
    rot, off = np.array([1.0, 0.0, 0.0, 1.0]), np.zeros(2)
    _lib.check(L.akb_rotate_with_nan_f64(D.ptr(corrected_dev), ny, nx, D.host_f64(rot), D.host_f64(off), D.ptr(out),
                                         D.ptr(opd), D.ptr(work), D.stream_handle()))
    return work.cpu().numpy().reshape(2, ny, nx)


def _check_post(m, o, label):
    """Every device check of one case: m the input map, o its oracle_chain."""
    from akbraytracing_amd import pupilmap as PM
    ny, nx = m.shape
    md = torch.tensor(m, device="cuda")  # (a copy: the shared map is read-only)
    r = PM.pupil_post(md)
    PM.pupil_post_check(r["params"])
    p = r["params"].cpu().numpy()
    rng_ = o["rng"]
    # nanmean, count, range
    assert _same_bits(p[0], o["mean"]), f"nanmean {p[0]!r} != numpy's {o['mean']!r}"
    assert p[1] == np.isfinite(m).sum()
    assert p[18] == np.nanmin(m) and p[19] == np.nanmax(m)
    assert p[17] == 0.0
    # the corrected map: against the oracle and against the host chain
    got_c = r["corrected"].cpu().numpy()
    d_c = _close(got_c, o["corrected"], 1e-12 * rng_, "corrected vs oracle")
    host_c = PM.plane_correction_with_nan_and_outlier_filter(md - float(o["mean"])).cpu().numpy()
    d_h = _close(got_c, host_c, 1e-12 * rng_, "corrected vs host chain")
    d_thr = abs(p[10] - o["thr"]) / o["thr"]
    assert d_thr <= 1e-12, f"3-sigma threshold {p[10]!r} vs {o['thr']!r}"
    # the angle and scipy.ndimage.rotate's matrix and offsets
    assert abs(p[11] - o["rot"]) <= 2 * np.spacing(abs(o["rot"])), f"rot {p[11]!r} vs {o['rot']!r}"
    assert _same_bits(p[12], np.degrees(p[11]))
    assert _same_bits(p[13], cosdg(p[12])), f"cos_deg({p[12]!r}) = {p[13]!r}, cosdg {cosdg(p[12])!r}"
    assert _same_bits(p[14], sindg(p[12])), f"sin_deg({p[12]!r}) = {p[14]!r}, sindg {sindg(p[12])!r}"
    cs, sn = np.float64(p[13]), np.float64(p[14])
    cy, cx = np.float64((ny - 1) / 2.0), np.float64((nx - 1) / 2.0)
    t0, t1 = cs * cy, sn * cx
    assert _same_bits(p[15], cy - (t0 + t1))
    t0, t1 = (-sn) * cy, cs * cx
    assert _same_bits(p[16], cx - (t0 + t1))
    # the prefilter
    coef = r["work"][HEAD:HEAD + 2 * ny * nx].cpu().numpy().reshape(2, ny, nx)
    if max(ny, nx) > 128:  # k_spline_block / k_spline_lines: spline_line's operations in its order
        assert _same_bits(coef, _lines_prefilter(r["corrected"])), "prefilter differs from k_spline_lines' bits"
    d_pf = []
    for k, a in enumerate((np.nan_to_num(got_c), (~np.isnan(got_c)).astype(float))):
        want = OPC.spline_filter(a)
        scale = float(np.max(np.abs(want)))
        d_pf.append(float(np.max(np.abs(coef[k] - want))) / scale)
        assert d_pf[-1] <= 1e-13, f"prefilter of the {('map', 'mask')[k]}: {d_pf[-1]:.3e} of max|coef|"
    # the rotated map: from the device's own corrected map and angle, then end to end
    got_r = r["rotated"].cpu().numpy()
    d_rs = _close(got_r, OPC.rotate_with_nan(got_c, p[12]), 1e-12 * rng_, "rotated vs oracle (stage)")
    assert _same_bits(r["opd"].cpu().numpy(), got_r * 1e-9)
    d_re = _close(got_r, o["rotated"], 1e-12 * rng_, "rotated vs oracle (end to end)")
    assert np.isfinite(got_r).any()
    print(f"{label}: corrected {d_c / rng_:.2e} (oracle) {d_h / rng_:.2e} (host chain) of the range, threshold "
          f"{d_thr:.2e}, prefilter {d_pf[0]:.2e} (map) {d_pf[1]:.2e} (mask) of max|coef|, rotated {d_rs / rng_:.2e} "
          f"(stage) {d_re / rng_:.2e} (end to end) of the range, angle {p[12]:.4f} deg")


@pytest.mark.parametrize("ny,nx", C.SHAPES)
def test_pupil_post_aperture_shapes(gpu, ny, nx):
    """Every branch a shape selects: the nanmean's buffers and leaves, the map in LDS or in global
    memory, the basis tables on or off, PostIdx with nx > 1024, k_spline_post's short and ragged
    lines, k_spline_block and k_spline_lines - with outliers the 3-sigma filter must drop."""
    m, o = C.aperture_case(ny, nx)
    _check_post(m, o, f"{ny}x{nx}")


@pytest.mark.parametrize("ny,nx,dr", EDGE_CASES)
def test_pupil_post_edge_angles(gpu, ny, nx, dr):
    """cos_deg / sin_deg at an exact 0, both signs, exactly -+45 degrees and beyond (cephes' second
    octant), bit for bit scipy.special's cosdg / sindg, and the rotation at those angles."""
    m, o = C.edge_case(ny, nx, dr)
    _check_post(m, o, f"{ny}x{nx} dr={dr}")


def _raised(fn):
    try:
        fn()
    except Exception as e:  # noqa: BLE001 - the type is what is compared
        return type(e)
    return None


@pytest.mark.parametrize("name", list(C.refusal_maps()))
def test_pupil_post_refuses_as_the_host_chain(gpu, name):
    """The post's flags (params[17], raised by pupil_post_check) against the host chain's exceptions:
    too few points for a fit is curve_fit's TypeError; a two-row map's Y^2 = 1 makes the five-term
    normal system exactly singular, numpy's LinAlgError - and the nanmean is numpy's nevertheless."""
    from akbraytracing_amd import pupilmap as PM
    m, kind = C.refusal_maps()[name]
    want = {"TypeError": TypeError, "LinAlgError": np.linalg.LinAlgError}[kind]
    md = torch.from_numpy(m).cuda()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)  # the all-NaN map's empty mean
        mean = float(np.nanmean(m))
    host = _raised(lambda: PM.plane_correction_with_nan_and_outlier_filter(md - mean))
    r = PM.pupil_post(md)
    p = r["params"].cpu().numpy()
    post = _raised(lambda: PM.pupil_post_check(p))
    print(f"{name}: host chain {host}, post {post} (flags {p[17]:.0f})")
    assert host is want
    assert post is want
    assert p[1] == np.isfinite(m).sum()
    if kind == "LinAlgError":
        assert _same_bits(p[0], mean)
        assert int(p[17]) & 2


def test_pupil_post_nan_rotation_estimate(gpu):
    """A map whose column nx // 4 has no finite point: the rotation estimate is NaN and the rotated
    map all NaN, as the oracle's; no flag is raised (the reference goes on with NaNs too)."""
    from akbraytracing_amd import pupilmap as PM
    m = C.nan_column_map()
    o = C.oracle_chain(m)
    assert np.isnan(o["rot"]) and np.isnan(o["rotated"]).all()
    r = PM.pupil_post(torch.from_numpy(m).cuda())
    PM.pupil_post_check(r["params"])
    p = r["params"].cpu().numpy()
    assert p[17] == 0.0
    assert np.isnan(p[11])
    assert _same_bits(p[0], o["mean"])
    _close(r["corrected"].cpu().numpy(), o["corrected"], 1e-12 * o["rng"], "corrected vs oracle")
    assert np.isnan(r["rotated"].cpu().numpy()).all() and np.isnan(r["opd"].cpu().numpy()).all()


def test_pupil_post_refuses_more_than_65536_points(gpu):
    from akbraytracing_amd import _lib
    from akbraytracing_amd import pupilmap as PM
    with pytest.raises(_lib.AKBError, match="65536"):
        PM.pupil_post(torch.zeros((256, 257), dtype=torch.float64).cuda())
