"""The Huygens reference helper (tests/huygens_ref.py) against itself, on the CPU: the sum reference
against a 200-bit sum, numpy's restatement (oracle/huygens.py) inside the sum bound on every input
the GPU tests use (the reference must pass its own bar), the pair errors on correctly rounded
values and on a one-ulp slip of r, the phase decades the pair inputs cover, and numpy's r = 0."""
import numpy as np
import pytest

import huygens_ref as R
from oracle import huygens as OH


def test_sum_reference_against_200_bit_sum():
    pytest.importorskip("mpmath")
    t, s, w, k = R.shape_case(9, 300, seed=3)
    ref, scale = R.sum_reference(t, s, w, k)
    err = np.abs(ref - R.mp_sum(t, s, w, k)) / scale
    print(f"sum reference vs 200-bit sum: {np.max(err) / 2.0 ** -53:.3f} x 2^-53 x scale")
    assert np.max(err) <= 2.0 ** -52


@pytest.mark.parametrize("name", R.SUM_CASES)
def test_numpy_restatement_is_inside_the_sum_bound(name):
    c = R.sum_case(name)
    rows, m = c["rows"], c["s"].shape[1]
    with np.errstate(divide="ignore", invalid="ignore"):
        got = OH.propagate(*c["t"][:, rows], *c["s"], c["w"], c["k"], np.ones(m))
    on_source = np.isin(rows, c["far"]) if name == "value" else np.zeros(rows.shape[0], dtype=bool)
    assert np.all(np.isnan(got[on_source].real) & np.isnan(got[on_source].imag))
    assert np.all(np.isnan(c["ref"][on_source].real) & np.isnan(c["ref"][on_source].imag))
    ratio = np.abs(got - c["ref"])[~on_source] / c["scale"][~on_source]
    print(f"{name}: numpy restatement {np.max(ratio) / 2.0 ** -53:.3f} x 2^-53 x scale")
    assert np.all(np.isfinite(c["scale"][~on_source])) and np.max(ratio) <= R.sum_bound(m)


def test_fixup_cases_leave_the_fast_range_where_they_say():
    """The fix-up inputs put exactly the pairs they name beyond 2^40 pi/2, with room to spare on
    either side, and no other sum case has a phase near the edge."""
    edge = R.FAST_Q * np.pi / 2
    for name in R.SUM_CASES:
        c = R.sum_case(name)
        _, ph = R.pair_geometry(c["t"], c["s"], c["k"])
        slow = np.abs(ph) >= edge
        assert not np.any((np.abs(ph) > 0.8 * edge) & (np.abs(ph) < 1.2 * edge)), name
        want = np.zeros_like(slow)
        if name == "fixup:all":
            want[:] = True
        elif name == "fixup:source":
            want[:, 137] = True
        elif name.startswith("fixup:targets"):
            want[c["far"], :] = True
            # a lane slot past the last target sits at the origin: beyond the range too
            _, ph0 = R.pair_geometry(np.zeros((3, 1)), c["s"], c["k"])
            assert np.all(np.abs(ph0) > 1.2 * edge)
        assert np.array_equal(slow, want), name


def test_pair_inputs_cover_every_phase_decade():
    decades = set()
    for k in R.PAIR_KS:
        _, ph = R.pair_geometry(R.pair_targets(20000, 1), R.PAIR_SOURCE, k)
        assert not np.any(R.may_be_slow(ph))
        decades |= set(np.floor(np.log10(np.abs(ph))).astype(int).ravel())
    assert decades >= set(range(-3, 13))
    _, ph = R.pair_geometry(R.pair_targets(20000, 1), R.PAIR_SOURCE, R.K_TOP)
    assert np.max(np.abs(ph)) > 0.99 * R.K_TOP  # just under 2^40 pi/2
    for exp in (-380, 499):
        t, s, k = R.sqrt_range_case(exp, 4000, 5)
        r, ph = R.pair_geometry(t, s, k)
        assert np.all(r * r >= 2.0 ** -767) and np.all(r * r <= 2.0 ** 1000) and not np.any(R.may_be_slow(ph))
        assert r[0, 0] == 2.0 ** exp and np.min(np.abs(ph)) > 1e10


def test_pair_errors_on_rounded_values_and_on_a_one_ulp_slip():
    """Correctly rounded cos / r and sin / r sit well inside the bounds; the same outputs for an r
    one ulp off at k r ~ 1e11 break the direction bound by orders of magnitude."""
    pytest.importorskip("mpmath")
    t = R.sqrt_targets(500, 2)
    r, ph = R.pair_geometry(t, R.PAIR_SOURCE, R.SQRT_K)
    (c, _), (s, _) = R.mp_cos_sin(ph)
    d, e, v = R.pair_errors((c + 1j * s) / r, r, ph)
    assert np.max(d) <= 2.0 ** -52 and np.max(e) <= 2.0 ** -51 and np.max(v) <= 2.0 ** -51
    # a half-turn (the quadrant off by two) leaves direction and amplitude alone: the vector error sees it
    d, e, v = R.pair_errors(-(c + 1j * s) / r, r, ph)
    assert np.max(d) <= 2.0 ** -52 and np.max(e) <= 2.0 ** -51 and np.min(v) > 1.99
    # a quarter-turn shows in the direction
    assert np.min(R.pair_errors((-s + 1j * c) / r, r, ph)[0]) > 0.99
    r1 = np.nextafter(r, np.inf)
    (c, _), (s, _) = R.mp_cos_sin(-R.SQRT_K * r1)
    d = R.pair_errors((c + 1j * s) / r1, r, ph)[0]
    # (k ulp(r) is 0.5 to 1 ulp of the phase here: a slip that rounds to the same (-k) * r is the
    # same pair, the others are off by a whole ulp of the phase)
    moved = -R.SQRT_K * r1 != ph
    assert np.mean(moved) > 0.5 and np.min(d[moved.ravel()]) > 1e4 * R.DIR_FAST


def test_numpy_formula_at_zero_distance():
    p = np.array([1.0, 2.0, 3.0])
    with np.errstate(divide="ignore", invalid="ignore"):
        got = OH.propagate(*p[:, None], *p[:, None], np.array([1 + 0j]), R.EUV_K, np.ones(1))
        ref, _ = R.sum_reference(p[:, None], p[:, None], np.array([1 + 0j]), R.EUV_K)
    assert np.isnan(got[0].real) and np.isnan(got[0].imag)
    assert np.isnan(ref[0].real) and np.isnan(ref[0].imag)
