"""Host-side logic and the C ABI boundary, without a GPU (no compute calls)."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT, golden_json
from griddata_ref import _cell_tris_np, _pockets, _ring_np  # noqa: F401


def test_library_exports_every_header_symbol():
    from akbraytracing_amd import _lib, build
    build.build(verbose=False)
    L = _lib.lib()
    with open(os.path.join(ROOT, "include", "akb_raytrace.h")) as f:
        hdr = f.read()
    declared = set(re.findall(r"^\s*(?:const char\*|int64_t|int|void)\s+(akb_\w+)\s*\(", hdr, re.M))
    assert declared == set(_lib.EXPORTS)
    for sym in declared:
        assert hasattr(L, sym), sym
    raw = ctypes.CDLL(build.SO)
    for sym in declared:
        getattr(raw, sym)


def test_abi_version_and_struct_layout():
    from akbraytracing_amd import _lib
    L = _lib.lib()
    assert L.akb_abi_version() == _lib.ABI_VERSION
    assert L.akb_chain_desc_size() == ctypes.sizeof(_lib.ChainDesc)
    # no GPU in this container: device count is 0 and calls report errors instead of crashing
    assert L.akb_device_count() >= 0


def test_library_carries_the_tree_sources_hash(tmp_path):
    """Provenance: the loaded library's akb_sources_hash() is the tree's, and a source edit changes
    the tree's hash (so _lib.lib() would refuse the stale library)."""
    import shutil
    from akbraytracing_amd import _lib, build
    assert _lib.sources_hash() == build.sources_hash()
    csrc = tmp_path / "pkg" / "csrc"  # the header sits at csrc/../../include, as in the tree
    shutil.copytree(build.CSRC, csrc)
    os.makedirs(tmp_path / "include")
    shutil.copy(os.path.join(ROOT, "include", "akb_raytrace.h"), tmp_path / "include")
    assert build.sources_hash(str(csrc)) == build.sources_hash()
    with open(csrc / "akb_trace.hip", "a") as f:
        f.write("\n// edit\n")
    assert build.sources_hash(str(csrc)) != build.sources_hash()


def test_invalid_arguments_are_reported_not_crashed():
    from akbraytracing_amd import _lib
    L = _lib.lib()
    st = L.akb_isect_f64(None, None, 0, 0, None, 0, 0, 0, 10, None, 0, None, None)
    assert st == -1
    assert b"null pointer" in L.akb_last_error()
    with pytest.raises(_lib.AKBError):
        _lib.check(st)
    desc = _lib.ChainDesc()
    desc.n_mirrors = 9
    assert L.akb_trace_chain_f64(ctypes.byref(desc), None) == -1
    assert L.akb_pairwise_work_bytes(3, 10_000_000) == 3 * 1221 * 16


@pytest.mark.parametrize("reserve", [0, 8, 40, 64, 128])
def test_reserved_cu_mask_is_even_over_xcds_under_either_bit_mapping(reserve):
    from akbraytracing_amd import _lib
    L = _lib.lib()
    m = np.zeros(8, dtype=np.uint32)
    assert L.akb_reserved_cu_mask(reserve, 256, m.ctypes.data) == 0
    off = [b for b in range(256) if not (int(m[b // 32]) >> (b % 32)) & 1]
    assert len(off) == reserve
    per = reserve // 8
    # blocks of 32 bits per XCD, or bit % 8 round-robin: the same count on each of the eight
    assert all(sum(1 for b in off if b // 32 == x) == per for x in range(8))
    assert all(sum(1 for b in off if b % 8 == x) == per for x in range(8))
    assert L.akb_reserved_cu_mask(12, 256, m.ctypes.data) == -1


def test_header_comments_cite_reference_lines():
    with open(os.path.join(ROOT, "include", "akb_raytrace.h")) as f:
        hdr = f.read()
    for ref in ("EllipseRaytrace3D.py:18-45", "psf_fft.py:29-125", "Wavecalc_raytrace_fromData_CPU0402.py:71-124"):
        assert ref in hdr


def test_geometry_and_sample_plan():
    from akbraytracing_amd.wavefront import SystemGeometry, sample_plan, Shard
    import oracle.pipeline as OPL
    g = SystemGeometry.from_dict(golden_json("akb_geometry.json"))
    assert len(g.mirrors) == 4 and [m.negative for m in g.mirrors] == [False, False, False, True]
    assert len(g.det1) == 4 and g.det1[0] == 1.0
    for n in (65, 64, 3163, 3164, 10000):
        hb, he, col = sample_plan(n)
        c2, v_idx, s2, e2, h_idx = OPL.sample_indices(n, n)
        assert (hb, he, col) == (s2, e2, c2)
        assert he - hb == n
    # flat shards cut at numpy's 8192-element sum buffers (the last one takes the short buffer)
    for n, w in ((3163, 8), (129, 2), (10000, 8), (8945, 8), (3163, 1), (65, 1)):
        shards = [Shard.split(n, w, r) for r in range(w)]
        assert shards[0].start == 0 and sum(s.count for s in shards) == n * n
        for a, b in zip(shards, shards[1:]):
            assert a.start + a.count == b.start and a.count % 8192 == 0
        counts = [s.full_buffers() for s in shards]
        assert max(counts) - min(counts) <= 1 and sum(counts) == n * n // 8192
    assert [s.count for s in (Shard.split(10000, 8, r) for r in range(8))][:2] == [1526 * 8192, 1526 * 8192]
    with pytest.raises(ValueError):
        Shard.split(65, 2, 0)  # 4225 rays: no full buffer to give each rank


def test_angle_tables_match_reference_fixture():
    from akbraytracing_amd.wavefront import SystemGeometry
    from conftest import golden
    g = SystemGeometry.from_dict(golden_json("akb_geometry.json"))
    f = golden("akb_raywave_65.npz")
    assert np.array_equal(g.angle_h.table(65), f["rand_h"])
    assert np.array_equal(g.angle_v.table(65), f["rand_v"])
    assert np.array_equal(np.tan(g.angle_h.table(65)), f["tan_h"])


def test_resample_matches_oracle():
    from akbraytracing_amd.wavefront import resample
    import oracle.pipeline as OPL
    rng = np.random.default_rng(1)
    ah = np.sort(rng.random(33))
    av = np.sort(rng.random(33))
    rh, rv = np.linspace(0, 1, 33), np.linspace(-1, 0, 33)
    a = resample(ah, av, rh, rv)
    b = OPL.resample_from_angles(ah, av, rh, rv)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_resample_restatement_matches_scipy_interp1d():
    """akb_resample_f64 (numpy linspace + scipy interp1d(kind='linear') restated in C) against
    scipy itself: sorted, reversed, tied, unsorted and near-monotone angle samples, and the
    out-of-range ValueError."""
    import scipy.interpolate as si
    from akbraytracing_amd.wavefront import resample_axis
    rng = np.random.default_rng(5)
    for t in range(1000):
        n = int(rng.integers(1, 300))
        kind = t % 5
        x = np.sort(rng.standard_normal(n))
        if kind == 1:
            x = x[::-1].copy()
        elif kind == 2:
            x = np.round(x, 1)
        elif kind == 3:
            x = rng.standard_normal(n)
        elif kind == 4:
            x = np.tan(np.linspace(-0.01, 0.02, n)) * (1 + 1e-9 * rng.standard_normal(n))
        y = rng.standard_normal(n)
        try:
            ref = si.interp1d(x, y, kind="linear")(np.linspace(x[0], x[-1], n))
        except ValueError:
            with pytest.raises(ValueError):
                resample_axis(x, y)
            continue
        assert np.array_equal(resample_axis(x, y), ref, equal_nan=True), (t, n, kind)


def test_psf_host_helpers_match_reference_formulas():
    from akbraytracing_amd import psf as G
    import oracle.psf as OP
    a = np.arange(12.0).reshape(3, 4)
    padded, crop = G.ensure_even_size(a)
    assert padded.shape == (4, 4) and crop == (slice(0, 3), slice(0, 4)) and padded[3].sum() == 0
    same, none = G.ensure_even_size(np.ones((4, 6)))
    assert none is None and same.shape == (4, 6)
    for dt in (np.int32, np.bool_, np.float32, np.complex128):  # np.pad keeps the dtype (psf_fft.py:15)
        src = np.ones((3, 5), dtype=dt)
        p, _ = G.ensure_even_size(src)
        ref = np.pad(src, ((0, 1), (0, 1)), mode="constant", constant_values=0)
        assert p.dtype == ref.dtype and np.array_equal(p, ref)
    wy, wx, m = G.hann_axes(9, 10)
    w = np.outer(wy, wx)
    assert m == w.max()
    x, y = G.image_axes(64, 48, 5e-6, 4e-6, 13.5e-9, 1e-2)
    _, xr, yr = OP.psf(np.zeros((24, 32)), np.ones((24, 32)), 13.5e-9, 5e-6, 1e-2, 2, dy=4e-6)
    assert np.array_equal(x, xr) and np.array_equal(y, yr)
    db = G.psf_to_db(np.array([1.0, 1e-3, 0.0]))
    assert np.allclose(db, [0.0, -30.0, -60.0])


def test_psf_argument_errors_before_any_device_work():
    from akbraytracing_amd import psf as G
    with pytest.raises(ValueError):
        G._check_args((4, 4), (4, 5), 2, None)
    with pytest.raises(ValueError):
        G._check_args((4, 4), (4, 4), 0, None)
    with pytest.raises(ValueError):
        G._check_args((4, 4), (4, 4), 2.5, None)
    with pytest.raises(ValueError):
        G._check_args((4, 4), (4, 4), 2, "blackman")
    G._check_args((4, 4), (4, 4), 3, "HANN")


def test_install_rebinds_and_respects_option_mpmath():
    import types
    import akbraytracing_amd
    from akbraytracing_amd import primitives as P
    mod = types.ModuleType("driver")
    mod.option_mpmath = True
    orig = lambda *a, **k: "reference"  # noqa: E731
    mod.mirr_ray_intersection = orig
    mod.compute_psf_fft = orig
    mod.unrelated = orig
    names = akbraytracing_amd.install(mod)
    assert set(names) == {"mirr_ray_intersection", "compute_psf_fft"}
    assert mod.mirr_ray_intersection.__wrapped__ is orig
    assert mod.unrelated is orig
    # option_mpmath routes the mpmath-aware primitives to the reference's own branch
    assert mod.mirr_ray_intersection(1, 2, 3) == "reference"
    assert akbraytracing_amd.install(mod) == names  # idempotent
    akbraytracing_amd.uninstall(mod)
    assert mod.mirr_ray_intersection is orig and mod.compute_psf_fft is orig


def test_install_covers_the_post_trace_steps():
    import types
    import akbraytracing_amd
    mod = types.ModuleType("driver")
    orig = lambda *a, **k: "reference"  # noqa: E731
    post = ["griddata", "plane_correction_with_nan_and_outlier_filter", "psf_calc", "find_defocus", "calc_dS"]
    for name in post:
        setattr(mod, name, orig)
    assert set(akbraytracing_amd.install(mod)) == set(post)
    assert all(getattr(mod, n).__wrapped__ is orig for n in post)
    akbraytracing_amd.uninstall(mod)
    assert all(getattr(mod, n) is orig for n in post)


def test_product_path_fails_loudly_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from akbraytracing_amd import primitives as P, _lib
    with pytest.raises(_lib.AKBError):
        P.normalize_vector(np.ones((3, 4)))


def test_product_package_never_imports_the_oracle():
    pkg = os.path.join(ROOT, "akbraytracing_amd")
    for dirpath, _, files in os.walk(pkg):
        for fn in files:
            if fn.endswith(".py"):
                with open(os.path.join(dirpath, fn)) as f:
                    src = f.read()
                assert not re.search(r"^\s*(import|from)\s+oracle", src, re.M), fn


def test_dropin_psf_module_exports():
    import importlib
    import sys
    import akbraytracing_amd
    sys.path.insert(0, akbraytracing_amd.DROPIN_DIR)
    try:
        sys.modules.pop("psf_fft", None)
        m = importlib.import_module("psf_fft")
        assert m.compute_psf_fft.__module__ == "akbraytracing_amd.psf"
        assert set(m.__all__) == {"compute_psf_fft", "psf_to_db", "ensure_even_size"}
    finally:
        sys.path.remove(akbraytracing_amd.DROPIN_DIR)
        sys.modules.pop("psf_fft", None)


# ----------------------------------------------------------------------------- griddata triangulation

def _grids():
    from conftest import golden
    f = golden("akb_raywave_65.npz")
    yield "ray_wave_65", f["detcenter2"][1].reshape(65, 65), f["detcenter2"][2].reshape(65, 65)
    u, v = np.meshgrid(np.linspace(-1, 1, 300), np.linspace(-1, 1, 280))
    yield "akb_like", u * 1e-4 + 3e-6 * v ** 2 - 2e-6 * u * v + 1e-6 * v ** 3, v * 1.3e-4 + 4e-6 * u ** 2 + 1e-6 * u ** 3
    yield "skewed", u + 0.05 * v + 0.03 * (u + 0.3) ** 2, 0.8 * v - 0.04 * (v - 0.2) * u + 0.02 * u ** 3


@pytest.mark.parametrize("case", ["ray_wave_65", "akb_like", "skewed"])
def test_structured_triangulation_equals_qhull(case):
    """Cells split by the in-circle test + akb_gd_pockets (host) = scipy's Delaunay (qhull),
    triangle for triangle, on the reference's 65x65 detector hits and deformed lattices."""
    from akbraytracing_amd import build
    from scipy.spatial import Delaunay
    build.build(verbose=False)
    name, X, Y = next(g for g in _grids() if g[0] == case)
    tri, nbr, edge, xptr, xidx = _pockets(X, Y)
    ours = np.concatenate([_cell_tris_np(X, Y), tri])
    P = np.stack([X.ravel(), Y.ravel()], 1)
    q = Delaunay(P).simplices
    assert len(ours) == len(q)
    assert set(map(tuple, np.sort(ours, 1))) == set(map(tuple, np.sort(q, 1)))
    # every pocket chord is listed from both ends, and every pocket edge on the ring is mapped
    assert xptr[-1] == len(xidx) and len(xidx) % 2 == 0
    assert np.count_nonzero(edge >= 0) == np.count_nonzero(nbr <= -2)


def test_pockets_refuse_a_cut_corner():
    from akbraytracing_amd import _lib
    u, v = np.meshgrid(np.linspace(-1, 1, 20), np.linspace(-1, 1, 20))
    X, Y = u.copy(), v.copy()
    X[0, 0], Y[0, 0] = -0.5, -0.5   # the corner pulled inside the hull
    with pytest.raises(_lib.AKBError):
        _pockets(X, Y)


def test_bench_picks_the_newest_profile_that_matches_the_sources(tmp_path, monkeypatch):
    """bench.py's profile lookup: tags order r05y < r05aa < r05an < r06a, and the newest file whose
    sources hash matches wins over a newer stale one (else the newest, flagged as not matching)."""
    import json
    import sys
    sys.path.insert(0, ROOT)
    import bench
    monkeypatch.setattr(bench, "ROOT", str(tmp_path))
    files = []
    for tag, sha in (("r04n", "a"), ("r05y", "b"), ("r05aa", "a"), ("r05an", "a"), ("r06a", "c")):
        f = tmp_path / f"{tag}_roofline.json"
        f.write_text(json.dumps({"tag": tag, "sources_sha256": sha}))
        files.append(str(f))
    assert sorted(reversed(files), key=bench._tag_key) == files
    d, name, ok = bench._pick_profile(files, "a")
    assert (d["tag"], name, ok) == ("r05an", "r05an_roofline.json", True)
    d, name, ok = bench._pick_profile(files, "zzz")
    assert (d["tag"], ok) == ("r06a", False)
    assert bench._pick_profile([], "a") == ({}, None, False)


def test_bench_dump_outputs_samples_and_masks(tmp_path):
    """bench.py --dump-outputs' writer on host tensors: rows per ray on the fixed seeded sample
    (the same indices on every call, written as ray_index), small arrays whole, an array over the
    PSF budget as a seeded sample with its indices, NaNs as zeros beside their mask, integer words
    and non-tensors left out, everything float64 / float32 and under 64 MB."""
    import sys
    import torch
    sys.path.insert(0, ROOT)
    import bench
    n = bench.DUMP_RAYS + 1000
    rays = dict(opl=torch.arange(n, dtype=torch.float64), last_hit=torch.arange(3 * n, dtype=torch.float64).reshape(3, n),
                wave2=torch.arange(n, dtype=torch.float64) * 0.5, dist_err2=None, flags=torch.zeros(1, dtype=torch.int32),
                slot=0)
    m = torch.arange(128 * 128, dtype=torch.float64).reshape(128, 128)
    m[0, :5] = float("nan")
    big = torch.arange(bench.DUMP_PSF_BYTES // 8 + 8, dtype=torch.float64)
    res = dict(psf=big, map=m, change=torch.zeros(2, dtype=torch.int64), converged=True)
    info = bench.dump_outputs(str(tmp_path / "a"), rays, res)
    again = bench.dump_outputs(str(tmp_path / "b"), rays, res)
    assert info["arrays"] == again["arrays"] == ["last_hit", "map", "map_nan", "opl", "psf", "psf_index", "ray_index",
                                                 "wave2"]
    A = {k: np.load(tmp_path / "a" / (k + ".npy")) for k in info["arrays"]}
    for k in info["arrays"]:
        assert np.array_equal(A[k], np.load(tmp_path / "b" / (k + ".npy"))), k
        assert A[k].dtype in (np.float64, np.float32), k
    assert info["bytes"] == sum(a.nbytes for a in A.values()) <= 64_000_000
    idx = A["ray_index"].astype(np.int64)
    assert idx.shape == (bench.DUMP_RAYS,) and np.all(np.diff(idx) > 0) and 0 <= idx[0] and idx[-1] < n
    assert np.array_equal(A["opl"], idx) and np.array_equal(A["wave2"], idx * 0.5)
    assert np.array_equal(A["last_hit"], np.stack([idx, idx + n, idx + 2 * n]))
    pick = A["psf_index"].astype(np.int64)
    assert pick.size == bench.DUMP_PSF_BYTES // 16 and np.all(np.diff(pick) > 0) and np.array_equal(A["psf"], pick)
    assert A["map_nan"].sum() == 5 and (A["map_nan"][0, :5] == 1).all() and (A["map"][0, :5] == 0).all()
    assert np.array_equal(A["map"][1:], m.numpy()[1:])


def _ring_order(W, d):
    """ring d of a W x W box clockwise from its top-left vertex (the plain depth order's ring)"""
    s1 = W - 2 * d - 1
    out = []
    for i in range(4 * s1):
        q, e = divmod(i, s1)
        out.append([(d, d + e), (d + e, d + s1), (d + s1, d + s1 - e), (d + s1 - e, d)][q])
    return out


def _sweep_read_cycles(K, S, verts):
    """LDS-array cycles of one step's sweep reads (both set parities), MI355X_MICROARCH.md §LDS:
    ds_read_b128 serves a wave in four 16-lane groups, bank = (byte address / 4) mod 64, and each
    extra distinct address on a busy bank costs a cycle. verts[t] = (r, c) or None. Returns
    (cycles, conflict-free cycles)."""
    W, P = 2 * K + 4, 33
    N1, N2 = (W - 2) ** 2, (W - 2 * S - 2) ** 2
    groups = [[0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27],
              [4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31]]
    groups += [[x + 32 for x in g] for g in groups]
    offs = [P, P + 2, 1, 2 * P + 1, 0, 2, 2 * P, 2 * P + 2]
    Q = max(S - 1, K - S - 1)
    tot = ideal = 0
    for par in (0, 1):
        for q in range(1, Q + 1):
            for w in range((N1 + N2 + 63) // 64):
                lanes = []
                for lane in range(64):
                    t = w * 64 + lane
                    if t >= N1 + N2 or verts[t] is None:
                        lanes.append(None)
                        continue
                    r, c = verts[t]
                    dep = min(r, c, W - 1 - r, W - 1 - c)
                    role = 0 if t < N2 else 1 if t < 2 * N2 else 2
                    fresh = role == 2 or role == par
                    j = q + 1 if fresh else S + 1 + q
                    ok = dep >= j and j <= (S if fresh else K)
                    lanes.append((r * P + c - P - 1, 0 if fresh else 1) if ok else None)
                if all(x is None for x in lanes):
                    continue
                for o in offs:
                    ideal += 4
                    for g in groups:
                        banks = {}
                        for lane in g:
                            if lanes[lane] is None:
                                continue
                            a = (lanes[lane][1] * 2 * P * 32 + lanes[lane][0] + o) * 16
                            for k in range(4):
                                banks.setdefault((a // 4 + k) % 64, set()).add(a)
                        tot += max((len(v) for v in banks.values()), default=0)
    return tot, ideal


def test_patch_vertex_order_is_a_bank_conflict_lean_permutation():
    """k_gd_cone_patch's thread -> vertex table (akb_gd_patch_order, host only): every thread set
    holds exactly its vertices (inner A / B: depth >= S + 1, outer: depth 1 .. S), the corners
    (depth K + 1) first in each inner set, idle threads past N1 + N2; at the bench's K = 12 the
    sweeps' simulated LDS read cycles are within 1.15x of conflict-free, where the plain depth
    order takes 1.8x."""
    from akbraytracing_amd import _lib
    L = _lib.lib()
    for K in range(1, 15):
        tab = np.zeros(1024, np.uint16)
        S = L.akb_gd_patch_order(K, tab.ctypes.data_as(ctypes.c_void_p))
        assert S >= (K + 1) // 2
        W = 2 * K + 4
        N1, N2 = (W - 2) ** 2, (W - 2 * S - 2) ** 2
        assert N1 + N2 + 4 <= 1024
        rc = [(int(v) & 0xFF, int(v) >> 8) for v in tab]
        dep = lambda v: min(v[0], v[1], W - 1 - v[0], W - 1 - v[1])  # noqa: E731
        inner = sorted((r, c) for r in range(W) for c in range(W) if dep((r, c)) >= S + 1)
        outer = sorted((r, c) for r in range(W) for c in range(W) if 1 <= dep((r, c)) <= S)
        assert sorted(rc[:N2]) == inner and sorted(rc[N2:2 * N2]) == inner
        assert sorted(rc[2 * N2:N1 + N2]) == outer
        assert all(v == 0xFFFF for v in tab[N1 + N2:])
        assert all(dep(rc[q]) == K + 1 and dep(rc[N2 + q]) == K + 1 for q in range(4))
        if K == 12:
            got, ideal = _sweep_read_cycles(K, S, rc[:N1 + N2])
            plain = []
            for lo, hi in ((S + 1, K + 1), (S + 1, K + 1), (1, S)):
                for d in range(hi, lo - 1, -1):
                    plain += _ring_order(W, d)
            base, ideal2 = _sweep_read_cycles(K, S, plain)
            # (the permuted order keeps a few more waves active a sweep: its own conflict-free count)
            assert got <= 1.15 * ideal and base >= 1.7 * ideal2 and got <= 0.65 * base, (got, ideal, base, ideal2)
    assert L.akb_gd_patch_order(0, tab.ctypes.data_as(ctypes.c_void_p)) < 0
