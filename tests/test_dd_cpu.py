"""The double-double arithmetic and the two option_mpmath primitives of csrc/akb_dd.h, built for the
host with g++ (-O2 -ffp-contract=off) and checked against mpmath: the header is shared code, so this
pins the arithmetic the GPU runs (test_dd_gpu.py compares the kernels with this build bit for bit).

Bounds. Arithmetic: the published relative bounds of the algorithms are all below 2^-100 (akb_dd.h).
Primitives: a float64 evaluation of the worst recorded call (the 4th mirror) is off by ~5e-10 m on
points of ~1e2 m, ~2^14 ulp, so cancellation amplifies a working precision's unit roundoff by ~2^15;
a few tens of double-double operations at 2^-100 each then leave the result within ~2^-80 relative,
~2^-27 ulp, of the exact value. Rounding that once gives the correctly rounded float64 unless the
exact value lies within 2^-27 ulp of a rounding boundary: every value within 1 ulp, and far fewer than
1 value in 1000 different at all (measured on this fixture: none).
"""
import types

import numpy as np
import pytest

import dd_host as H

mpmath = pytest.importorskip("mpmath")

BOUND = 2.0 ** -100


def _dd(rng, n, lo_exp=-30, hi_exp=30):
    """n normalised double-double numbers (hi, lo) of mixed signs and magnitudes"""
    hi = rng.uniform(1.0, 2.0, n) * 2.0 ** rng.integers(lo_exp, hi_exp, n) * rng.choice([-1.0, 1.0], n)
    lo = rng.uniform(-0.5, 0.5, n) * np.spacing(np.abs(hi))
    s = hi + lo
    return np.stack([s, lo - (s - hi)], axis=1)


def _edge(x, sign):
    """x.hi with lo at the edge of hi's ulp: +-(ulp / 2) (1 - 2^-52)"""
    half = 0.5 * np.spacing(np.abs(x[:, 0]))
    return np.stack([x[:, 0], sign * np.nextafter(half, 0.0)], axis=1)


def _operands(seed):
    rng = np.random.default_rng(seed)
    a, b = _dd(rng, 1500), _dd(rng, 1500)
    c = _dd(rng, 300, -3, 3)
    pairs = [
        (a, b),
        (c, np.stack([c[:, 0], -c[:, 1]], axis=1)),                 # equal hi
        (c, np.stack([-c[:, 0], rng.uniform(-0.49, 0.49, 300) * np.spacing(np.abs(c[:, 0]))], axis=1)),  # hi cancels
        (_edge(c, 1.0), _edge(_dd(rng, 300, -3, 3), -1.0)),         # lo at the edge of hi's ulp
        (_edge(c, -1.0), np.stack([-c[:, 0], np.zeros(300)], axis=1)),
        (_edge(c, 1.0), _edge(c, 1.0)),
    ]
    return np.concatenate([p[0] for p in pairs]), np.concatenate([p[1] for p in pairs])


def _check(op, a, b, exact):
    got = H.host_arith(op, a, b)
    worst = 0.0
    with mpmath.workprec(300):
        for k in range(a.shape[0]):
            x = mpmath.mpf(float(a[k, 0])) + mpmath.mpf(float(a[k, 1]))
            y = mpmath.mpf(float(b[k, 0])) + mpmath.mpf(float(b[k, 1]))
            want = exact(x, y)
            r = mpmath.mpf(float(got[k, 0])) + mpmath.mpf(float(got[k, 1]))
            if want == 0:
                assert r == 0, (op, k)
                continue
            worst = max(worst, float(abs((r - want) / want)))
    print(f"op {op}: worst relative error 2^{np.log2(worst) if worst else -np.inf:.2f}")
    assert worst <= BOUND, (op, worst)


def test_add_sub_within_2pow_minus_100():
    a, b = _operands(1)
    _check(0, a, b, lambda x, y: x + y)
    _check(6, a, b, lambda x, y: x - y)
    _check(5, a, b, lambda x, y: x + mpmath.mpf(_hi(y)))


def _hi(y):
    """the float64 nearest to y (dd + double uses b's high word only)"""
    return float(y)


def test_mul_within_2pow_minus_100():
    a, b = _operands(2)
    _check(1, a, b, lambda x, y: x * y)
    _check(4, a, b, lambda x, y: x * mpmath.mpf(_hi(y)))


def test_div_within_2pow_minus_100():
    a, b = _operands(3)
    _check(2, a, b, lambda x, y: x / y)


def test_sqrt_within_2pow_minus_100():
    a, b = _operands(4)
    a = np.where(a[:, :1] < 0, -a, a)
    _check(3, a, b, lambda x, y: mpmath.sqrt(x))
    z = H.host_arith(3, np.zeros((1, 2)), np.zeros((1, 2)))
    assert z[0, 0] == 0.0 and z[0, 1] == 0.0


def _host(name, ins, neg):
    if name == "mirr_ray_intersection":
        return H.host_isect(ins[0], ins[1], ins[2], neg)[0]
    return H.host_reflect(ins[0], ins[1])[0]


def test_primitives_on_the_fixture_match_the_exact_evaluation():
    exact = H.exact_outputs()
    total = differ = 0
    for key, name, ins, neg, ref, refdev in H.calls():
        got = _host(name, ins, neg)
        want = exact[key]
        assert got.shape == want.shape == ref.shape
        dev = H.ulp_dev(got, want)
        assert np.all(dev <= 1.0), (key, float(dev.max()))
        total += got.size
        differ += int(np.sum(got != want))
    print(f"{differ} of {total} values differ from the exact evaluation")
    assert differ * 1000 <= total


def test_primitives_against_the_reference_outputs():
    exact = H.exact_outputs()
    for key, name, ins, neg, ref, refdev in H.calls():
        got = _host(name, ins, neg)
        # the stored deviation is the reference's own (mp.dps = 20) from the exact evaluation
        assert float(H.ulp_dev(ref, exact[key]).max()) == refdev
        assert np.all(H.ulp_dev(got, ref) <= refdev + 1.0), key
        assert np.all(np.abs(got - exact[key]) <= np.abs(ref - exact[key])), key


def test_value_rules():
    sphere = [1, 1, 1, 0, 0, 0, 0, 0, 0, -1]
    ray = np.array([[1.0, 1.0, 1.0], [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]])
    src = np.array([[-5.0, -5.0, -5.0], [0.5, 1.5, 1.0], [0.0, 0.0, 0.0]])  # hit, miss, tangent (D == 0)
    out, fl = H.host_isect(sphere, ray, src)
    assert fl == 1
    assert np.all(np.isnan(out[:, 1])) and not np.isnan(out[:, [0, 2]]).any()
    assert np.array_equal(out[:, 2], [0.0, 1.0, 0.0])
    assert np.array_equal(out[:, [0, 2]], H.mp_isect(sphere, ray, src)[:, [0, 2]])
    out_n, _ = H.host_isect(sphere, ray, src, negative=True)
    assert np.array_equal(out_n[:, 0], H.mp_isect(sphere, ray, src, True)[:, 0]) and np.all(np.isnan(out_n[:, 1]))
    # a zero-norm reflection is left as it is, its neighbours are normalised
    d = np.array([[0.6, 0.0, 3.0], [0.8, 0.0, 0.0], [0.0, 0.0, 4.0]])
    nrm = np.array([[0.0, 1.0, 0.0], [1.0, 0.0, 1.0], [0.0, 0.0, 0.0]])
    r, fl = H.host_reflect(d, nrm)
    assert fl == 4
    assert np.array_equal(r[:, 1], [0.0, 0.0, 0.0])
    assert np.array_equal(r, H.mp_reflect(d, nrm))
    assert np.array_equal(r[:, 2], [0.6, 0.0, 0.8])
    # (3,) inputs
    o1, _ = H.host_isect(sphere, np.array([1.0, 0.0, 0.0]), np.array([-5.0, 0.5, 0.0]))
    assert o1.shape == (3, 1) and np.array_equal(o1[:, 0], out[:, 0])
    r1, _ = H.host_reflect(np.array([0.6, 0.8, 0.0]), np.array([0.0, 1.0, 0.0]))
    assert r1.shape == (3, 1) and np.array_equal(r1[:, 0], r[:, 0])


def test_install_routing_without_a_gpu():
    import akbraytracing_amd
    mod = types.ModuleType("driver")
    mod.option_mpmath = True
    orig = lambda *a, **k: "reference"  # noqa: E731
    mod.mirr_ray_intersection = orig
    mod.reflect_ray = orig
    mod.plot_result_debug = orig
    akbraytracing_amd.install(mod)
    assert mod.mirr_ray_intersection(1, 2, 3) == "reference" and mod.reflect_ray(1, 2) == "reference"
    assert mod.mirr_ray_intersection.__akb_mpmath__ == "reference"
    akbraytracing_amd.install(mod, mpmath="device")  # rebinds: nothing is launched here
    for name in ("mirr_ray_intersection", "reflect_ray", "plot_result_debug"):
        w = getattr(mod, name)
        assert w.__akb_mpmath__ == "device" and w.__wrapped__ is orig, name
    mod.option_mpmath = False  # other modes of plot_result_debug still reach the reference's function
    assert mod.plot_result_debug(np.zeros(26), "no_such_mode") == "reference"
    with pytest.raises(ValueError):
        akbraytracing_amd.install(mod, mpmath="host")
    akbraytracing_amd.uninstall(mod)
    assert mod.mirr_ray_intersection is orig and mod.plot_result_debug is orig


def test_dd_is_not_an_alias_of_fp64():
    import oracle as O
    key, name, ins, neg, ref, _ = next(c for c in H.calls() if c[1] == "mirr_ray_intersection" and c[3]
                                       and c[4].shape[1] == 289)
    fp64 = O.mirr_ray_intersection(ins[0], ins[1], ins[2], negative=True)
    got = _host(name, ins, neg)
    assert np.all(H.ulp_dev(got, H.exact_outputs()[key]) <= 1.0)
    worst = float(np.max(np.abs(fp64 - got)))
    print(f"float64 restatement - double-double on the 4th mirror: {worst:.3e} m")
    assert worst > 1e-11
