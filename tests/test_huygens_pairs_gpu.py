"""The Huygens kernel (csrc/akb_huygens.hip) pair by pair, on the MI355X: the hand-written sqrt, the
1 / (2 r) amplitude, the Cody-Waite phase reduction and its quadrants, the library fix-up loop, both
target slots of a lane, explicit source splits and the work buffer, the value rules and scale_field,
each against the high-precision reference of tests/huygens_ref.py at the bounds derived there.
Every test prints the figures it asserts (pytest -s)."""
import numpy as np
import pytest
import torch

import huygens_ref as R

pytestmark = pytest.mark.gpu

U53 = 2.0 ** -53


def _dev(a, dev):
    return torch.from_numpy(np.array(a)).to(dev)  # (a copy: the shared cases are read-only)


def _run(dev, t, s, w, k, splits=0, work=None):
    from akbraytracing_amd.wavecalc import propagate
    args = [_dev(a, dev) for a in t] + [_dev(a, dev) for a in s]
    return propagate(*args, _dev(np.asarray(w, dtype=np.complex128), dev), k, splits=splits, work=work).cpu().numpy()


def _nan_work(dev, n, m, splits, extra=0):
    """The work buffer of a call, NaN-filled: a partial row the kernels leave unwritten shows."""
    from akbraytracing_amd import _lib
    need = int(_lib.lib().akb_huygens_work_bytes(n, m, splits))
    assert need % 8 == 0
    return torch.full((need // 8 + extra,), float("nan"), dtype=torch.float64, device=dev), need // 8


def _one_pair(dev, t, s, k):
    """m = 1, u = 1: out = (2 RN(amp cos), 2 RN(amp sin)) per target. Asserts on every target the
    direction bound (DIR_SLOW where the phase may leave the fast range), the amplitude bound and
    the vector bound (their sum: it is what sees a half-turn, out -> -out)."""
    r, ph = R.pair_geometry(t, s, k)
    out = _run(dev, t, s, np.ones(1, dtype=np.complex128), k)
    assert np.all(np.isfinite(out.real) & np.isfinite(out.imag))
    d, e, v = R.pair_errors(out, r, ph)
    slow = R.may_be_slow(ph).ravel()
    bound = np.where(slow, R.DIR_SLOW, R.DIR_FAST)
    i, j = int(np.argmax(d / bound)), int(np.argmax(e))
    print(f"direction max {np.max(d[~slow], initial=0) / U53:.3f} x 2^-53 (fast), "
          f"{np.max(d[slow], initial=0) / U53:.3f} x 2^-53 (fix-up, {int(np.sum(slow))} targets); "
          f"amplitude max {e[j]:.3e}; vector max {np.max(v):.3e}; worst at ph = {ph.ravel()[i]!r}, r = {r.ravel()[j]!r}")
    assert np.all(d <= bound), (i, d[i], ph.ravel()[i])
    assert np.all(e <= R.AMP_BOUND), (j, e[j], r.ravel()[j])
    assert np.all(v <= R.AMP_BOUND + bound), (int(np.argmax(v)), np.max(v), ph.ravel()[int(np.argmax(v))])


# ----------------------------------------------------------------------------- 1. one pair per target

@pytest.mark.parametrize("sign", [1, -1])
@pytest.mark.parametrize("kmag", R.PAIR_KS)
def test_one_pair_per_target_every_phase_decade(gpu, kmag, sign):
    pytest.importorskip("mpmath")
    _one_pair(gpu, R.pair_targets(20000, 1), R.PAIR_SOURCE, sign * kmag)


@pytest.mark.parametrize("n", [1, 256, 257, 512, 513])
def test_one_pair_per_target_lane_slot_edges(gpu, n):
    pytest.importorskip("mpmath")
    _one_pair(gpu, R.pair_targets(n, n), R.PAIR_SOURCE, R.K_TOP if n % 2 else -R.K_TOP)


# ----------------------------------------------------------------------------- 2. quadrant boundaries

@pytest.mark.parametrize("k", [1.0, -1.0])
def test_quadrant_boundaries_and_the_fast_threshold(gpu, k):
    pytest.importorskip("mpmath")
    r, q = R.quadrant_radii()
    assert {int(v) % 4 for v in q if v == int(v)} == {0, 1, 2, 3}
    t = np.vstack([np.zeros_like(r), np.zeros_like(r), r])
    rr, ph = R.pair_geometry(t, np.zeros((3, 1)), k)
    assert np.array_equal(rr.ravel(), r) and np.array_equal(ph.ravel(), -k * r)
    # 2^-49 only from q = 2^40 - 1 up (where the rounded quotient may reach 2^40), 2^-50 below
    slow = R.may_be_slow(ph).ravel()
    assert np.all(q[slow] >= 2.0 ** 40 - 1) and np.all(slow[q >= 2.0 ** 40 - 0.5]) and np.sum(~slow) > 100
    _one_pair(gpu, t, np.zeros((3, 1)), k)


# ----------------------------------------------------------------------------- 3. the sqrt

def test_sqrt_every_distance_correctly_rounded_at_1e11_rad(gpu):
    """One ulp of r moves these phases by ~1e-5 rad, 1e10 times the direction bound: a misrounded
    sqrt or a contracted sum of squares fails it on the pairs it touches."""
    pytest.importorskip("mpmath")
    t = R.sqrt_targets(200_000, 4)
    _, ph = R.pair_geometry(t, R.PAIR_SOURCE, R.SQRT_K)
    assert np.min(np.abs(ph)) > 3e10 and np.max(np.abs(ph)) < 2e11
    _one_pair(gpu, t, R.PAIR_SOURCE, R.SQRT_K)


@pytest.mark.parametrize("exp", [-380, 499])
def test_sqrt_at_the_ends_of_its_stated_range(gpu, exp):
    """r = np.sqrt(x) at |d| = 2^-380 and 2^499, as far as propagate's output can show it: through
    the phase (-k) * r at ~1e11 rad, where one ulp of r is 0.5 to 1 ulp of the phase. A slip of r
    that rounds to the same phase is the same output and is not seen (up to half of one-ulp slips,
    tests/test_huygens_ref_cpu.py); every other one breaks the direction bound by ~1e10."""
    pytest.importorskip("mpmath")
    t, s, k = R.sqrt_range_case(exp, 4000, 5)
    _one_pair(gpu, t, s, k)


# ----------------------------------------------------------------------------- sums

def _check_sum(name, got, rows=None):
    """got (over the case's host rows) against the sum reference at the sum bound; returns the worst
    ratio to the bound."""
    c = R.sum_case(name)
    m = c["s"].shape[1]
    ratio = np.abs(got - c["ref"]) / c["scale"]
    if rows is not None:
        ratio = ratio[rows]
    assert np.all(np.isfinite(ratio)), name
    worst = float(np.max(ratio)) / R.sum_bound(m)
    assert worst <= 1.0, (name, worst, int(np.argmax(ratio)))
    return worst


# ----------------------------------------------------------------------------- 4. the fix-up loop

@pytest.mark.parametrize("splits", [1, 3])
@pytest.mark.parametrize("name", ["fixup:all", "fixup:source", "fixup:targets", "fixup:targets@257"])
def test_fixup_loop(gpu, name, splits):
    c = R.sum_case(name)
    n, m = c["t"].shape[1], c["s"].shape[1]
    work, _ = _nan_work(gpu, n, m, splits)
    got = _run(gpu, c["t"], c["s"], c["w"], c["k"], splits=splits, work=work)
    far = np.zeros(n, dtype=bool)
    far[c["far"]] = True
    worst_far = _check_sum(name, got, far)
    worst_near = _check_sum(name, got, ~far) if not np.all(far) else 0.0
    print(f"{name} splits {splits}: far targets {worst_far:.4f}, near targets {worst_near:.4f} of the sum bound")
    if not np.all(far):
        # the near targets' sums do not know about the far ones (nor about the slots past the end)
        work.fill_(float("nan"))
        alone = _run(gpu, c["t"][:, ~far], c["s"], c["w"], c["k"], splits=splits, work=work)
        assert np.array_equal(got[~far].view(np.uint64), alone.view(np.uint64))


# ----------------------------------------------------------------------------- 5. shapes and splits

def _shape_run(dev, name, splits):
    c = R.sum_case(name)
    n, m = c["t"].shape[1], c["s"].shape[1]
    work, _ = _nan_work(dev, n, m, splits)
    got = _run(dev, c["t"], c["s"], c["w"], c["k"], splits=splits, work=work)
    assert got.shape == (n,)
    assert np.all(np.isfinite(got.real) & np.isfinite(got.imag))  # (the unchecked targets too)
    worst = _check_sum(name, got[c["rows"]])
    print(f"{name} splits {splits}: {worst:.4f} of the sum bound")


@pytest.mark.parametrize("n,m", R.SHAPE_NM[:14])
@pytest.mark.parametrize("splits", [0, 1, 2])
def test_shapes_against_the_sum_reference(gpu, n, m, splits):
    _shape_run(gpu, f"shape:{n}x{m}", splits)


@pytest.mark.parametrize("splits", [1, 2, 3, 7, 127, 128, 129, 257, 300, 301])
def test_splits_against_the_sum_reference(gpu, splits):
    _shape_run(gpu, "shape:513x300", splits)


def test_empty_trailing_splits(gpu):
    _shape_run(gpu, "shape:513x10", 7)  # 2 sources per split: splits 5 and 6 are empty


def test_most_splits(gpu):
    _shape_run(gpu, "shape:3x300", 65535)


# ----------------------------------------------------------------------------- 6. splits, bit for bit

@pytest.fixture(scope="module")
def split_inputs(gpu):
    c = R.sum_case("shape:513x300")
    t = [_dev(a, gpu) for a in c["t"]]
    s = [_dev(a, gpu) for a in c["s"]]
    return t, s, _dev(c["w"], gpu), c["k"], {}


@pytest.mark.parametrize("splits", [2, 127, 128, 129, 257, 301])
def test_splits_are_the_documented_composition(gpu, split_inputs, splits):
    """propagate(splits=s) is: the partial of split i = propagate(sources [jb, je), splits=1), zeros
    for an empty split; partials added in float64 in chunks of 128 consecutive splits, then the
    chunks in order."""
    from akbraytracing_amd.wavecalc import propagate
    t, s, w, k, partials = split_inputs
    n, m = t[0].shape[0], s[0].shape[0]
    per = -(-m // splits)
    rows = []
    for i in range(splits):
        jb, je = min(i * per, m), min(i * per + per, m)
        if (jb, je) not in partials:
            partials[jb, je] = (np.zeros(n, dtype=np.complex128) if jb == je else
                                propagate(*t, *(a[jb:je] for a in s), w[jb:je], k, splits=1).cpu().numpy())
        rows.append(partials[jb, je])
    chunks = []
    for c0 in range(0, splits, 128):
        acc = rows[c0].copy()
        for p in rows[c0 + 1:c0 + 128]:
            acc = acc + p
        chunks.append(acc)
    want = chunks[0]
    for p in chunks[1:]:
        want = want + p
    work, _ = _nan_work(gpu, n, m, splits)
    got = propagate(*t, *s, w, k, splits=splits, work=work).cpu().numpy()
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))


@pytest.mark.parametrize("splits", [1, 3, 129])
def test_a_target_slice_is_the_slice_of_the_whole_call(gpu, splits):
    c = R.sum_case("shape:1030x40")
    whole = _run(gpu, c["t"], c["s"], c["w"], c["k"], splits=splits)
    part = _run(gpu, c["t"][:, 250:520], c["s"], c["w"], c["k"], splits=splits)
    assert np.array_equal(part.view(np.uint64), whole[250:520].view(np.uint64))


# ----------------------------------------------------------------------------- 7. work size

@pytest.mark.parametrize("splits", [2, 129])
def test_work_bytes_is_what_the_kernels_write(gpu, splits):
    """work = a view of exactly akb_huygens_work_bytes inside a sentinel-filled tensor: every double
    of the view is written, none before or after it."""
    from akbraytracing_amd import _lib
    c = R.sum_case("shape:513x300")
    n, m = c["t"].shape[1], c["s"].shape[1]
    need = int(_lib.lib().akb_huygens_work_bytes(n, m, splits)) // 8
    chunks = -(-splits // 128)
    assert need == (splits + (chunks if chunks > 1 else 0)) * 2 * n
    sentinel, guard = -1.2345e300, 4096
    big = torch.full((guard + need + guard,), sentinel, dtype=torch.float64, device=gpu)
    got = _run(gpu, c["t"], c["s"], c["w"], c["k"], splits=splits, work=big[guard:guard + need])
    _check_sum("shape:513x300", got[c["rows"]])
    host = big.cpu().numpy()
    assert np.all(host[:guard] == sentinel) and np.all(host[guard + need:] == sentinel)
    assert not np.any(host[guard:guard + need] == sentinel)


def test_split_count_and_empty_sizes(gpu):
    from akbraytracing_amd._lib import AKBError
    c = R.sum_case("shape:3x300")
    with pytest.raises(AKBError):
        _run(gpu, c["t"], c["s"], c["w"], c["k"], splits=65536)
    none = np.zeros((3, 0))
    for splits in (0, 1, 3):
        out = _run(gpu, c["t"], none, np.zeros(0, dtype=np.complex128), c["k"], splits=splits)
        assert out.shape == (3,) and np.array_equal(out.view(np.uint64), np.zeros(6, dtype=np.uint64))
        out = _run(gpu, none, c["s"], c["w"], c["k"], splits=splits)
        assert out.shape == (0,) and out.dtype == np.complex128


# ----------------------------------------------------------------------------- 8. value rules

def _all_nan(z):
    return bool(np.all(np.isnan(z.real) & np.isnan(z.imag)))


@pytest.mark.parametrize("splits", [1, 3])
def test_target_on_a_source_is_nan_and_its_neighbours_are_not(gpu, splits):
    c = R.sum_case("value")
    on = np.zeros(c["t"].shape[1], dtype=bool)
    on[c["far"]] = True
    assert _all_nan(c["ref"][on])  # numpy's rule
    got = _run(gpu, c["t"], c["s"], c["w"], c["k"], splits=splits)
    assert _all_nan(got[on])
    print(f"value splits {splits}: {_check_sum('value', got, ~on):.4f} of the sum bound")


@pytest.mark.parametrize("splits", [1, 3])
def test_inf_coordinate_is_nan(gpu, splits):
    c = R.sum_case("shape:257x40")
    clean = _run(gpu, c["t"], c["s"], c["w"], c["k"], splits=splits)
    t = c["t"].copy()
    t[0, 3], t[1, 256], t[2, 100] = np.inf, -np.inf, np.inf
    hit = np.zeros(257, dtype=bool)
    hit[[3, 256, 100]] = True
    with np.errstate(invalid="ignore"):
        assert _all_nan(R.sum_reference(t[:, hit], c["s"], c["w"], c["k"])[0])  # numpy's rule
    got = _run(gpu, t, c["s"], c["w"], c["k"], splits=splits)
    assert _all_nan(got[hit]) and np.array_equal(got[~hit].view(np.uint64), clean[~hit].view(np.uint64))
    s = c["s"].copy()
    s[2, 17] = np.inf  # an inf source coordinate: every target
    assert _all_nan(_run(gpu, c["t"], s, c["w"], c["k"], splits=splits))


# ----------------------------------------------------------------------------- 9. scale_field

@pytest.mark.parametrize("m", [1, 255, 256, 257, 70001])
def test_scale_field_is_numpys_complex_times_real(gpu, m):
    """Bit for bit numpy's u * ds (complex128 * float64: the real promoted to d + 0i, the full
    complex product), signed zeros included; a NaN where numpy has a NaN (re = inf with d finite
    gives a NaN imaginary part: inf * 0)."""
    from akbraytracing_amd.wavecalc import scale_field
    rng = np.random.default_rng(m)
    special = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1.0, -2.5, 1e-320, 1e308])
    u = rng.standard_normal(m) + 1j * rng.standard_normal(m)
    ds = rng.standard_normal(m)
    # the special (re, im, d) triples from the front, shuffled so that a small m sees every kind
    # (all 729 once m allows), ordinary values behind
    g = np.array(np.meshgrid(special, special, special, indexing="ij")).reshape(3, -1)
    g = g[:, rng.permutation(g.shape[1])][:, :m]
    u.real[:g.shape[1]], u.imag[:g.shape[1]] = g[0], g[1]
    ds[:g.shape[1]] = g[2]
    if m > 1000:
        u[-1], ds[-1] = complex(np.inf, 1.0), 2.0
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        want = u * ds
    if m > 1000:
        assert want[-1].real == np.inf and np.isnan(want[-1].imag)
    got = scale_field(_dev(u, gpu), _dev(ds, gpu)).cpu().numpy()
    for a, b in ((got.real, want.real), (got.imag, want.imag)):
        nan = np.isnan(b)
        assert np.array_equal(np.isnan(a), nan)
        assert np.array_equal(a[~nan].view(np.uint64), b[~nan].view(np.uint64))
