"""Reference for the Huygens kernel's per-pair arithmetic (csrc/akb_huygens.hip), the bounds its
source comments promise, and the inputs the CPU and GPU tests share. TEST INFRASTRUCTURE ONLY.

The kernel shares four roundings with numpy, and the reference repeats exactly those in float64:

    dx, dy, dz = t - s;  x = (dx*dx + dy*dy) + dz*dz;  r = np.sqrt(x);  ph = (-k) * r

Everything after them is taken in high precision:

* pair reference: cos / sin of the double ph from mpmath at 200 bits (kept as hi + lo doubles);
  the direction and amplitude errors of an output are then formed in np.longdouble (64-bit
  significand: 2^-11 of the bounds), or in mpmath where longdouble is no wider than double;
* sum reference: per term (1/r) (cos ph + i sin ph) w_j in float64 and math.fsum over the terms
  (0.07 * 2^-53 * scale away from the 200-bit sum, see tests/test_huygens_ref_cpu.py).

Bounds, each from what the kernel's source promises (none measured from the kernel):

* direction |a S - b C| / hypot(a, b) <= 2^-50 for out = (a, b) from one source with u = 1: sin and
  cos < 1 ulp each (<= 2^-52 absolute, sqrt(2) 2^-52 as an angle) plus 2^-53 relative from each of
  the products amp*cs and amp*sn = 4.7e-16 < 2^-50; 2^-49 where the fix-up loop may run (the
  library's sincos at the OpenCL double bound of 4 ulp);
* amplitude |hypot(a, b) r - 1| <= 2e-13 (the comment's "~1e-13", doubled for the tilde);
* vector |(a, b) r - (C, S)| <= 2e-13 + the direction bound: the two above are blind to out -> -out
  (a half-turn: the quadrant off by two, both sign flips wrong); a length within 2e-13 of 1 at an
  angle within the direction bound of the true one lies this close to (C, S), and -out lies 2 away;
* sums over m sources |got - ref| <= (2e-13 + 2^-49 + m 2^-52) * sum_j |w_j| / r_j: amplitude,
  direction and the two FMAs per pair of the accumulation.
"""
import functools
import math

import numpy as np

EUV_K = 2.0 * np.pi / 13.5e-9
FAST_Q = 2.0 ** 40             # |rint(ph 2/pi)| below this: the kernel's Cody-Waite path
DIR_FAST = 2.0 ** -50
DIR_SLOW = 2.0 ** -49
AMP_BOUND = 2e-13
HOST_PAIRS = 200_000           # most pairs a case takes through the host reference

_WIDE = np.finfo(np.longdouble).nmant >= 63


def sum_bound(m):
    return 2e-13 + 2.0 ** -49 + m * 2.0 ** -52


def may_be_slow(ph):
    """True where a phase may leave the fast range (the kernel compares the rounded quotient
    rint(ph 2/pi), so a phase within one quadrant of the edge counts)."""
    return np.abs(ph) >= (FAST_Q - 1.0) * (np.pi / 2)


def pair_geometry(t, s, k):
    """t (3, n), s (3, m) -> r, ph of shape (n, m), in the kernel's and numpy's float64 order."""
    t, s = np.asarray(t, dtype=np.float64), np.asarray(s, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        dx = t[0][:, None] - s[0][None, :]
        dy = t[1][:, None] - s[1][None, :]
        dz = t[2][:, None] - s[2][None, :]
        x = (dx * dx + dy * dy) + dz * dz
        r = np.sqrt(x)
        ph = (-np.float64(k)) * r
    return r, ph


def mp_cos_sin(ph):
    """cos and sin of the doubles ph at 200 bits, each as a (hi, lo) pair of float64 arrays."""
    from mpmath import libmp  # (mpmath's kernel functions: 2e5 phases in a few seconds)
    out = np.empty((4,) + ph.shape)
    flat = out.reshape(4, -1)
    for i, v in enumerate(ph.ravel()):
        c, s = libmp.mpf_cos_sin(libmp.from_float(float(v)), 200, "n")
        flat[0, i] = fc = libmp.to_float(c)
        flat[1, i] = libmp.to_float(libmp.mpf_sub(c, libmp.from_float(fc), 200, "n"))
        flat[2, i] = fs = libmp.to_float(s)
        flat[3, i] = libmp.to_float(libmp.mpf_sub(s, libmp.from_float(fs), 200, "n"))
    return (out[0], out[1]), (out[2], out[3])


def pair_errors(out, r, ph):
    """Direction error |a S - b C| / hypot(a, b), amplitude error |hypot(a, b) r - 1| and vector
    error |(a, b) r - (C, S)| of the one-source outputs out = a + i b (u = 1) against the pair
    reference, as float64 arrays."""
    out, r, ph = np.asarray(out).ravel(), np.asarray(r).ravel(), np.asarray(ph).ravel()
    (c_hi, c_lo), (s_hi, s_lo) = mp_cos_sin(ph)
    if _WIDE:
        L = np.longdouble
        a, b = out.real.astype(L), out.imag.astype(L)
        C, S = c_hi.astype(L) + c_lo.astype(L), s_hi.astype(L) + s_lo.astype(L)
        h = np.hypot(a, b)
        rl = r.astype(L)
        return ((np.abs(a * S - b * C) / h).astype(np.float64), np.abs(h * rl - 1).astype(np.float64),
                np.hypot(a * rl - C, b * rl - S).astype(np.float64))
    import mpmath
    d, e, v = np.empty(out.shape), np.empty(out.shape), np.empty(out.shape)
    with mpmath.workprec(200):
        for i in range(out.shape[0]):
            a, b = mpmath.mpf(float(out[i].real)), mpmath.mpf(float(out[i].imag))
            C = mpmath.mpf(float(c_hi[i])) + mpmath.mpf(float(c_lo[i]))
            S = mpmath.mpf(float(s_hi[i])) + mpmath.mpf(float(s_lo[i]))
            h = mpmath.hypot(a, b)
            d[i] = float(abs(a * S - b * C) / h)
            rr = mpmath.mpf(float(r[i]))
            e[i] = float(abs(h * rr - 1))
            v[i] = float(mpmath.hypot(a * rr - C, b * rr - S))
    return d, e, v


def _fsum(v):
    return math.fsum(v) if np.all(np.isfinite(v)) else float(np.sum(v))


def sum_reference(t, s, w, k):
    """The sum reference and its scale: (ref (n,) complex128, sum_j |w_j| / r_j (n,))."""
    r, ph = pair_geometry(t, s, k)
    w = np.asarray(w, dtype=np.complex128)
    with np.errstate(divide="ignore", invalid="ignore"):
        term = (1.0 / r) * (np.cos(ph) + 1j * np.sin(ph)) * w[None, :]
        scale = np.array([_fsum(row) for row in np.abs(w)[None, :] / r])
    ref = np.array([complex(_fsum(row.real), _fsum(row.imag)) for row in term]).reshape(-1)
    return ref.astype(np.complex128), scale


def mp_sum(t, s, w, k):
    """The same sum with every term and the accumulation at 200 bits (from the doubles r, ph, w)."""
    import mpmath
    r, ph = pair_geometry(t, s, k)
    out = np.empty(r.shape[0], dtype=np.complex128)
    with mpmath.workprec(200):
        for i in range(r.shape[0]):
            acc = mpmath.mpc(0)
            for j in range(r.shape[1]):
                c, sn = mpmath.cos_sin(mpmath.mpf(float(ph[i, j])))
                acc += mpmath.mpc(c, sn) / mpmath.mpf(float(r[i, j])) * mpmath.mpc(complex(w[j]))
            out[i] = complex(acc)
    return out


def host_rows(n, m):
    """The targets a case checks on the host: all of them within HOST_PAIRS pairs, else the lane
    slot and block edges plus an even spread."""
    if n * m <= HOST_PAIRS:
        return np.arange(n)
    edge = [i for i in (0, 255, 256, 257, 511, 512, n - 1) if i < n]
    rest = np.linspace(0, n - 1, HOST_PAIRS // m - len(edge)).astype(np.int64)
    return np.unique(np.concatenate([np.array(edge, dtype=np.int64), rest]))


# ----------------------------------------------------------------------------- pair inputs

PAIR_SOURCE = np.array([[0.3], [-0.2], [0.1]])
K_TOP = 0.998 * (FAST_Q - 1.0) * (np.pi / 2)  # with offsets <= 1 m every phase stays on the fast path
PAIR_KS = (1e3, 1e6, K_TOP)  # |ph| over 1e-3..1e3, 1..1e6 and 1.7e6..1.7e12 with offsets 1e-6..1 m


def pair_targets(n, seed):
    """n targets at random 3-D offsets of 1e-6 to 1 m from PAIR_SOURCE (log-uniform length, one in
    sixteen within a tenth of the top), so one k spans six decades of phase."""
    rng = np.random.default_rng(seed)
    d = rng.standard_normal((3, n))
    d /= np.sqrt(np.sum(d * d, axis=0))
    length = 10.0 ** rng.uniform(-6.0, 0.0, n)
    top = rng.random(n) < 1.0 / 16
    length[top] = rng.uniform(0.9, 1.0, int(np.sum(top)))
    return PAIR_SOURCE + d * length


def quadrant_radii():
    """Distances r (targets on the z axis, source at the origin, |k| = 1) at the doubles nearest
    q pi/2 and (q + 1/2) pi/2 and their two neighbours on either side, for q in 0..8, 2^20 +- 1,
    2^35 +- 3 and 2^40 - 2 .. 2^40 + 2: every residue of q mod 4, the worst cancellation of the
    reduction, the edge of the kernel polynomials' interval and the fast / fix-up threshold.
    r = 0 (q = 0) is a target on a source, so its place is taken by small distances of the sqrt's
    stated range. Returns (r, q)."""
    import mpmath
    qs = list(range(9)) + [2 ** 20 - 1, 2 ** 20 + 1, 2 ** 35 - 3, 2 ** 35 + 3] + [2 ** 40 + d for d in range(-2, 3)]
    assert {q % 4 for q in qs} == {0, 1, 2, 3}
    r, qq = [2.0 ** -380, 1e-100, 1e-8], [0.0, 0.0, 0.0]
    with mpmath.workprec(200):
        for q in qs:
            for h in (0.0, 0.5):
                if q + h == 0:
                    continue
                c = float(mpmath.pi * (q + h) / 2)
                for v in (np.nextafter(np.nextafter(c, 0.0), 0.0), np.nextafter(c, 0.0), c,
                          np.nextafter(c, np.inf), np.nextafter(np.nextafter(c, np.inf), np.inf)):
                    r.append(float(v))
                    qq.append(q + h)
    r, qq = np.array(r), np.array(qq)
    return r, qq


SQRT_K = 4e11


def sqrt_targets(n, seed):
    """Offsets of 5 to 25 cm per axis from PAIR_SOURCE: k r ~ 1e11 at SQRT_K, where one ulp of r
    moves the phase by ~1e-5 rad."""
    rng = np.random.default_rng(seed)
    return PAIR_SOURCE + rng.uniform(0.05, 0.25, (3, n)) * rng.choice([-1.0, 1.0], (3, n))


def sqrt_range_case(exp, n, seed):
    """Offsets from a source at the origin with |d| in [2^(exp-1), 2^exp] per axis (the first
    targets on one axis at exactly 2^exp), and the k that puts the phases at ~1e11 rad:
    x = r^2 then sits at the end of the sqrt's stated range for exp = -380 and 499."""
    rng = np.random.default_rng(seed)
    t = np.ldexp(rng.uniform(0.5, 1.0, (3, n)), exp) * rng.choice([-1.0, 1.0], (3, n))
    t[:, :3] = np.diag([math.ldexp(1.0, exp)] * 3)
    return t, np.zeros((3, 1)), math.ldexp(1e11, -exp)


# ----------------------------------------------------------------------------- sum inputs

def _box(rng, n, centre, half=5e-4):
    return np.asarray(centre, dtype=np.float64)[:, None] + rng.uniform(-half, half, (3, n))


def _field(rng, m):
    return rng.standard_normal(m) + 1j * rng.standard_normal(m)


def shape_case(n, m, seed=21):
    """m sources in a 1 mm box at the origin, n targets in a 1 mm box 5 cm downstream, EUV k."""
    rng = np.random.default_rng(seed)
    return _box(rng, n, [0, 0, 0.05]), _box(rng, m, [0, 0, 0]), _field(rng, m), EUV_K


FAR = np.array([3000.0, 4000.0, 0.0])  # 5 km


def fixup_case(kind, n=513, m=300, seed=22):
    """Inputs whose phases leave the fast range (|k r| >= 2^40 pi/2 = 1.7e12 rad):
    all:     every pair (k = 1e6 x EUV);
    source:  one source 5 km away, its weight raised 1e5 times so that its term is the size of a
             near one (a dropped or doubled term shows); every target takes the fix-up loop, in the
             far source's split only;
    targets: the sources and the near targets 5 km from the origin, two far targets (index 5, and
             the last index of slot 1: 300 for n = 513, 256 for n = 257) near the origin - where the
             lane slots past the end sit too.
    Returns (t, s, w, k, far) with far the indices of the far targets (all of them or none for the
    first two kinds)."""
    rng = np.random.default_rng(seed)
    if kind == "all":
        t, s, w, _ = shape_case(n, m, seed)
        return t, s, w, EUV_K * 1e6, np.arange(n)
    if kind == "source":
        t, s, w, k = shape_case(n, m, seed)
        s[:, 137] += FAR
        w[137] *= 1e5
        return t, s, w, k, np.arange(n)
    assert kind == "targets"
    t, s, w = _box(rng, n, FAR + [0, 0, 0.05]), _box(rng, m, FAR), _field(rng, m)
    far = np.array([5, 300 if n > 300 else n - 1])
    t[:, far] = np.array([[10.0, -7.0], [-20.0, 3.0], [5.0, 1.0]])
    return t, s, w, EUV_K, far


def value_case(n=257, m=40, seed=23):
    """Targets 7 and 256 (slot 1) lie on sources 3 and 20; every other pair is ordinary."""
    t, s, w, k = shape_case(n, m, seed)
    t[:, 7], t[:, 256] = s[:, 3], s[:, 20]
    return t, s, w, k, np.array([7, 256])


SHAPE_NM = ([(n, 40) for n in (1, 255, 256, 257, 511, 512, 513, 1030)]
            + [(513, m) for m in (1, 255, 256, 257, 512, 513)] + [(513, 300), (513, 10), (3, 300)])


@functools.lru_cache(maxsize=None)
def sum_case(name):
    """A named sum case with its reference, computed once per process and shared (read-only):
    dict(t, s, w, k, rows, ref, scale, far), ref and scale over the targets rows."""
    kind, _, arg = name.partition(":")
    far = np.array([], dtype=np.int64)
    if kind == "shape":
        n, m = (int(v) for v in arg.split("x"))
        t, s, w, k = shape_case(n, m)
    elif kind == "fixup":
        what, _, n = arg.partition("@")
        t, s, w, k, far = fixup_case(what, int(n or 513))
    else:
        assert name == "value"
        t, s, w, k, far = value_case()
    rows = host_rows(t.shape[1], s.shape[1])
    ref, scale = sum_reference(t[:, rows], s, w, k)
    case = dict(t=t, s=s, w=w, k=k, rows=rows, ref=ref, scale=scale, far=far)
    for v in case.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return case


SUM_CASES = ([f"shape:{n}x{m}" for n, m in SHAPE_NM]
             + ["fixup:all", "fixup:source", "fixup:targets", "fixup:targets@257", "value"])
