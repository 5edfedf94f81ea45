"""The sharded cone solve's entry points - akb_gd_cells_window_f64, akb_gd_claims_f64 with a row window,
akb_gd_cone_part_f64 (own0, own1, band_on, cnt), akb_gd_part_finish_f64 - emulated rank by rank in one
process, as faithful_dist.ShardedFaithfulPupil drives them, against the one-call solve on the whole
lattice. No torch.distributed and no subprocesses: the collectives are an elementwise minimum and a sum.

The plan pieces are built directly from hand-made Shard lists (ShardPlan._window, vertex_band_segments,
cell_band_segments), so the cuts fall in the middle of a row, one rank holds less than a row, and the
band owner is any rank. Every rank sees full-size buffers that hold the truth only where its plan says
the data is backed - its window's rows, on the band owner also every rank's band - and a finite poison
everywhere else (x, y scaled by 1 + 2^-10, f + 1, the diagonals flipped, the work buffer filled): a
read the plan does not back changes bits instead of passing on a previous run's identical values."""
import numpy as np
import pytest
import torch

from griddata_ref import _lattice, small_values

pytestmark = pytest.mark.gpu

UNCLAIMED = np.iinfo(np.int32).max
MX, MY = 40, 45


def _shards(n, cuts):
    from akbraytracing_amd.wavefront import Shard
    cuts = [0] + list(cuts) + [n * n]
    return [Shard(a, b - a) for a, b in zip(cuts, cuts[1:])]


# n, K, the cuts (flat ray indices, mid-row; one rank under a row), the band owner, the value sets
CASES = [
    (41, 1, (23,), 0, 1),
    (41, 1, (8 * 41 + 13, 17 * 41 + 23, 17 * 41 + 30, 30 * 41 + 5), 4, 2),
    (41, 3, (40 * 41 + 23,), 1, 2),  # the band owner holds 18 rays of the last row: no cell row of its own
    (41, 3, (8 * 41 + 13, 17 * 41 + 23, 17 * 41 + 30, 30 * 41 + 5), 2, 1),
    (67, 12, (22 * 67 + 40, 44 * 67 + 9, 44 * 67 + 39), 0, 2),  # windows of ~22 rows, a halo of 15: each reaches
    (67, 12, (22 * 67 + 40, 44 * 67 + 9, 44 * 67 + 39), 2, 1),  # past its neighbours; rank 2 holds 30 rays
    (131, 7, (60 * 131 + 77, 60 * 131 + 127), 0, 1),
    (131, 7, (60 * 131 + 77, 60 * 131 + 127), 1, 2),
]


def _fill(dst, src, runs):
    for a, b in runs:
        dst[..., a:b] = src[..., a:b]


@pytest.mark.parametrize("n,K,cuts,root,nvals", CASES)
def test_cone_parts_equal_the_one_call_solve(gpu, n, K, cuts, root, nvals):
    from akbraytracing_amd import _lib
    from akbraytracing_amd import device as D
    from akbraytracing_amd.faithful_dist import ShardPlan, band_depth, cell_band_segments, vertex_band_segments
    from akbraytracing_amd.griddata import CubicGrid, chebyshev_weights
    L = _lib.lib()
    X, Y, F = _lattice(n, n, seed=7 * n + K)
    vals = small_values(F, nvals)
    gx = np.linspace(X.min(), X.max(), MX)
    gy = np.linspace(Y.min() - 1e-6, Y.max(), MY)  # some targets outside the hull
    m = MX * MY
    shards = _shards(n, cuts)
    world = len(shards)
    assert sum(s.count for s in shards) == n * n and any(s.count < n for s in shards)
    assert all(s.start % n for s in shards[1:])  # every cut in the middle of a row

    # the truth and the whole-lattice result: one CubicGrid, one akb_gd_cone_eval_f64
    cg = CubicGrid(X.ravel(), Y.ravel(), n, n)
    dev = cg.dev
    want = cg.interp_cone(vals, gx, gy, sweeps=K)
    want_change = cg.cone_change.cpu().numpy().copy()
    tgx, tgy = torch.tensor(gx, device=dev), torch.tensor(gy, device=dev)
    need = int(L.akb_gd_cone_work_bytes(n, n, MX, MY, nvals))
    work = torch.empty(need // 8 + 1, dtype=D.F64, device=dev)
    tri = (D.ptr(cg.ptri), D.ptr(cg.pnbr), D.ptr(cg.edge_tri))
    want_owner = torch.empty(m, dtype=torch.int32, device=dev)
    _lib.check(L.akb_gd_claims_f64(D.ptr(cg.x), D.ptr(cg.y), n, n, D.ptr(cg.diag), cg.npock, *tri, 0, -1, 1,
                                   D.ptr(tgx), MX, D.ptr(tgy), MY, D.ptr(want_owner), D.ptr(work), None))
    torch.cuda.synchronize()
    claimed = want_owner != UNCLAIMED
    assert 0.3 < claimed.float().mean().item() < 1.0
    assert torch.equal(torch.isnan(want[0]).reshape(-1), ~claimed)

    xyf = torch.cat([cg.x[None], cg.y[None], torch.as_tensor(vals, device=dev)])  # (2 + nvals, n * n)
    poison = xyf.clone()
    poison[:2] *= 1 + 2.0 ** -10
    poison[2:] += 1.0
    truth_diag = cg.diag
    d = band_depth(K) + 1
    wins = [ShardPlan._window(n, K, s) for s in shards]
    omegas = D.host_f64(chebyshev_weights(max(K, 1)))

    # stage 1 per rank: the window buffers, the cell pass over the window, the band to its owner
    bufs = []
    for r, s in enumerate(shards):
        (claim0, claim1), (R0, R1), (cells0, cells1) = wins[r]
        assert R0 <= claim0 <= claim1 <= n - 1 and cells0 <= claim0 and claim1 <= cells1
        buf = poison.clone()
        _fill(buf, xyf, [(R0 * n, R1 * n)])
        if r == root:
            for q in shards:
                _fill(buf, xyf, vertex_band_segments(q.start, q.start + q.count, n, d))
        diag = 1 - truth_diag  # every split flipped: a cell the pass does not form stays wrong
        flags = torch.zeros(1, dtype=torch.int32, device=dev)
        _lib.check(L.akb_gd_cells_window_f64(D.ptr(buf[0]), D.ptr(buf[1]), n, n, cells0, cells1, D.ptr(diag), 1e-10,
                                             D.ptr(flags), None))
        torch.cuda.synchronize()
        c0, c1 = cells0 * (n - 1), cells1 * (n - 1)
        assert torch.equal(diag[c0:c1], truth_diag[c0:c1]), r
        assert torch.equal(diag[:c0], 1 - truth_diag[:c0]) and torch.equal(diag[c1:], 1 - truth_diag[c1:]), r
        # no error bit (1, 2, 4, 32) and one orientation (bit 3 or 4, set by every cell)
        assert int(flags.item()) in ((8, 16) if c1 > c0 else (0,)), (r, int(flags.item()))
        bufs.append((buf, diag))
    rdiag = bufs[root][1]
    for q in shards:  # BandGather: the other ranks' band cells into the band owner's diagonals
        _fill(rdiag, truth_diag, cell_band_segments(q.start, q.start + q.count, n, d))

    # stage 2: every rank's claims over its own cell rows, MIN-reduced
    owner = torch.full((m,), UNCLAIMED, dtype=torch.int32, device=dev)
    for r, s in enumerate(shards):
        buf, diag = bufs[r]
        is_root = r == root
        pock = (cg.npock, *tri) if is_root else (0, None, None, None)
        mine = torch.empty(m, dtype=torch.int32, device=dev)
        work.fill_(1e3)
        _lib.check(L.akb_gd_claims_f64(D.ptr(buf[0]), D.ptr(buf[1]), n, n, D.ptr(diag), *pock, wins[r][0][0],
                                       wins[r][0][1], int(is_root), D.ptr(tgx), MX, D.ptr(tgy), MY, D.ptr(mine),
                                       D.ptr(work), None))
        owner = torch.minimum(owner, mine)
    torch.cuda.synchronize()
    assert torch.equal(owner, want_owner)

    # stage 3: every rank's part on the reduced owners, SUM-reduced, then the finish
    out = torch.zeros((nvals, m), dtype=D.F64, device=dev)
    cnt = torch.zeros(m, dtype=D.F64, device=dev)
    change = np.zeros(2, np.int64)
    formed = []
    for r, s in enumerate(shards):
        buf, diag = bufs[r]
        is_root = r == root
        pock = (cg.npock, *tri) if is_root else (0, None, None, None)
        chords = (D.ptr(cg.xptr), D.ptr(cg.xidx)) if is_root else (None, None)
        part = torch.full((nvals, m), 1e3, dtype=D.F64, device=dev)
        pcnt = torch.full((m,), 1e3, dtype=D.F64, device=dev)
        pchg = torch.zeros(2, dtype=torch.int64, device=dev)
        work.fill_(1e3)
        _lib.check(L.akb_gd_cone_part_f64(D.ptr(buf[0]), D.ptr(buf[1]), n, n, D.ptr(diag), *pock, *chords, s.start,
                                          s.start + s.count, int(is_root), D.ptr(tgx), MX, D.ptr(tgy), MY,
                                          D.ptr(buf[2:]), nvals, K, omegas, D.ptr(work), D.ptr(owner), D.ptr(part),
                                          D.ptr(pcnt), D.ptr(pchg), None))
        torch.cuda.synchronize()
        assert torch.all((pcnt == 0) | (pcnt == 1)), r
        assert torch.all(part[:, pcnt == 0] == 0), r
        formed.append(int(pcnt.sum().item()))
        out += part
        cnt += pcnt
        change = np.maximum(change, pchg.cpu().numpy())  # ordered double bits: non-negative int64
    assert torch.equal(cnt, claimed.to(D.F64))  # every claimed target formed once, by one rank
    _lib.check(L.akb_gd_part_finish_f64(D.ptr(out), D.ptr(cnt), m, nvals, None))
    torch.cuda.synchronize()
    got, ref = out.cpu().numpy(), want.reshape(nvals, m).cpu().numpy()
    assert np.array_equal(got, ref, equal_nan=True)
    assert np.array_equal(change, want_change), (change.view(np.float64), want_change.view(np.float64))
    print(f"n={n} K={K} world={world} root={root} nvals={nvals}: targets formed per rank {formed}")
    assert sum(1 for f in formed if f > 0) >= 2  # the solve really was split
