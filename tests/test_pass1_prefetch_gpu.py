"""The fused pass 1 (k_chain_tilt) where its workgroups walk more than one segment: the software
pipeline - the next segment's table entries and tilt rows loaded during this segment's stores, the
OPD rows consumed behind the leaf sums - against sequential RayWave.run() calls, bit for bit.

The fast fused-pipeline tests of test_gpu_parity.py stop at n = 1001 (3,915 segments), below the
fused launch's grid, where every workgroup walks one segment and nothing is prefetched."""
import copy

import numpy as np
import pytest
import torch

from conftest import golden_json

pytestmark = pytest.mark.gpu

ROWS = ("last_hit", "dir_out", "opl", "detcenter2", "total2", "dist_err2", "wave2")
SEG = 256  # rays per segment (kLeafSeg)


def _systems(k):
    """bench.py's cycled systems (bench.system_variants) of the C3 geometry."""
    import bench
    from akbraytracing_amd.wavefront import SystemGeometry
    return bench.system_variants(SystemGeometry.from_dict(golden_json("akb_geometry.json")), k)


def _pass1_grid():
    """Workgroups of the fused pass-1 launch: four rounds of the three workgroups a CU holds
    (chain_tilt in akb_trace.hip), capped at 8192."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    return min(4 * 3 * cus, 8192)


def _n_past_grid():
    """The smallest n whose n^2 rays fill more segments than the fused launch has workgroups, so
    that the first workgroups walk a second segment and the rest do not (a square rarely lands on
    exactly one segment more: at 3072 workgroups n = 887 gives 3074 segments)."""
    g = _pass1_grid()
    n = int(np.sqrt(g * SEG))
    while (n * n + SEG - 1) // SEG <= g:
        n += 1
    return n


def _fused_pipeline(rw, back, kws):
    """Fronts pipelined exactly as bench.py --fuse 2 issues them: run k's pass-1 kernel tilts run
    k-2 and forms run k-3's OPD; the runs left in flight drain through launch_back."""
    fr = []
    for kw in kws:
        if len(fr) == 3:
            old = fr.pop(0)
            fr.append(rw.launch_front(overlap=lambda p=old: back(p), fuse=fr[0], fuse_opd=old, **kw))
        elif len(fr) == 2:
            fr.append(rw.launch_front(fuse=fr[0], **kw))
        else:
            fr.append(rw.launch_front(**kw))
    for f in fr:
        back(f)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


@pytest.mark.parametrize("n", [1461, 2049, "past-grid"])
def test_pipelined_segments_equal_sequential_runs(gpu, n):
    """Eight distinct systems through the --fuse 2 pipeline, five of them tilted and OPD-formed
    inside later pass-1 kernels: every row a caller receives, the tilt parameter block, the extent
    keys and both flag words equal a sequential run() of the same system.
    n = 1461: 8,338 segments, the last one partial (249 rays: some lanes' prefetch is masked);
    n = 2049: 16,401 segments, five or six a workgroup, the last partial;
    past-grid: the smallest n with more segments than workgroups (_n_past_grid)."""
    from akbraytracing_amd.wavefront import RayWave
    if n == "past-grid":
        n = _n_past_grid()
        assert (n * n + SEG - 1) // SEG > _pass1_grid() >= ((n - 1) ** 2 + SEG - 1) // SEG
    systems = _systems(8)
    rw = RayWave(systems[0], n)
    want = []
    for g in systems:
        seq = rw.run(geometry=g)
        want.append(({k: seq[k].clone() for k in ROWS}, rw._ext[seq["slot"]].clone(), rw.pupil(32)[1].clone(),
                     seq.tilt_params().copy(), tuple(seq["flags"])))
    assert not torch.equal(want[0][0]["wave2"], want[1][0]["wave2"])  # the systems really differ
    bs = torch.cuda.Stream()
    got, kinds = [], []

    def back(front):
        kinds.append((front.tilt is not None, front.opd is not None))
        with torch.cuda.stream(bs):
            o = rw.launch_back(front, stream=bs)
            keys = rw._ext[o["slot"]].clone()
            got.append(({k: o[k].clone() for k in ROWS}, keys, rw.pupil(32)[1].clone(), o))

    kws = [dict(geometry=g, next_geometry=systems[i + 1] if i + 1 < len(systems) else None)
           for i, g in enumerate(systems)]
    _fused_pipeline(rw, back, kws)
    torch.cuda.synchronize()
    assert kinds == [(True, True)] * 5 + [(True, False)] + [(False, False)] * 2
    for i, ((rows, keys, pitch, o), (wrows, wkeys, wpitch, wparams, wflags)) in enumerate(zip(got, want)):
        for k in ROWS:
            assert torch.equal(rows[k], wrows[k]), (i, k)
        assert torch.equal(keys, wkeys), i
        assert torch.equal(pitch, wpitch), i
        assert np.array_equal(_bits(o.tilt_params()), _bits(wparams)), i
        assert tuple(o["flags"]) == wflags == (0, 0), i


# The C3 geometry with the last mirror's linear and constant terms replaced so that, of the
# 1461^2 grid rays, exactly the far corner misses it: 150 rays in grid rows 1443-1460 and columns
# 1445-1460, the first of them flat ray 2,109,683 (segment 8,240); the middle row and column (the
# resample's pick rays) hit with a discriminant above 2e7. Found on the host: the discriminant
# of every ray at that mirror, from the oracle's chain through the first three mirrors, fitted
# linearly in the four terms to fall off along the grid's diagonal, then the constant term bisected
# to 150 misses.
MISS_TERMS = [-4596435.945137726, 55421.89498538428, 1194495.865399548, 333410849.12432027]


def test_pipelined_pass1_raises_for_a_miss_in_a_later_segment(gpu):
    """Rays that miss only in segments past every workgroup's first (segment 8,240 on, of 8,338):
    the fused, software-pipelined pass 1 raises the flag as the sequential run does, when that
    run's back half is taken - not earlier (the pick rays all hit) and with the same flag word."""
    from akbraytracing_amd import _lib
    from akbraytracing_amd.wavefront import RayWave, SystemGeometry
    n = 1461
    assert 8240 >= _pass1_grid()
    good = _systems(5)
    d = copy.deepcopy(golden_json("akb_geometry.json"))
    d["mirrors"][-1]["coeffs"][6:10] = MISS_TERMS
    bad = SystemGeometry.from_dict(d)
    with pytest.raises(_lib.AKBError, match="pass 1") as seq:
        RayWave(good[0], n).run(geometry=bad)
    systems = good[:3] + [bad] + good[4:]
    rw = RayWave(systems[0], n)
    bs = torch.cuda.Stream()
    taken = []

    def back(front):
        with torch.cuda.stream(bs):
            rw.launch_back(front, stream=bs)
        taken.append(front)

    kws = [dict(geometry=g, next_geometry=systems[i + 1] if i + 1 < len(systems) else None)
           for i, g in enumerate(systems)]
    with pytest.raises(_lib.AKBError, match="pass 1") as pip:
        _fused_pipeline(rw, back, kws)
    torch.cuda.synchronize()
    assert len(taken) == 3  # runs 0-2 came back; run 3, the system with the misses, raised
    assert str(pip.value) == str(seq.value)
