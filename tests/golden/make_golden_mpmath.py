"""Record tests/golden/akb_mpmath_17.npz from the REFERENCE's option_mpmath branch.

Run where the reference is present (make_golden.REF; it is only read and never travels):

    python tests/golden/make_golden_mpmath.py

With option_mpmath set, mirr_ray_intersection and reflect_ray of AKB_raytrace_20250312.py run a
per-column mpmath loop at mp.dps = 20 (:399-443, :474-500). Two 17 x 17 'ray_wave' runs of
plot_result_debug at make_golden.best_params() with option_set = True are recorded:

  the reference run   option_mpmath = True, the reference's own two functions;
  the exact run       the same driver with the two functions replaced by 300-bit mpmath evaluations
                      of the same expressions, rounded once to float64 (the value rules unchanged:
                      NaN per column where D < 0, a zero-norm reflection left unnormalised).

Recorded:
  c{k}_{name}_in{j}, _neg, _out   every mirr_ray_intersection / reflect_ray call of the reference
                                  run, the 289-column ones and the N <= 4 ones, in call order
  c{k}_{name}_refdev              that call's largest deviation of the reference's output from the
                                  300-bit evaluation of the same inputs, in ulp of the expected
                                  column's largest component (np.spacing(max(|x|, |y|, |z|)))
  ref_* / exact_*                 the griddata inputs of each run (:3689): det2_y, det2_z,
                                  dist_err2, wave2
  exact_minus_ref_nm              max |DistError2 difference|, max |Wave2 difference| of the two runs
"""
import os
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import OUT, REF, _stub_modules, best_params  # noqa: E402

N = 17
NAMES = ("mirr_ray_intersection", "reflect_ray")
PREC = 300


def exact_isect(coeffs, ray, source, negative=False):
    import mpmath
    with mpmath.workprec(PREC):
        mpf = mpmath.mpf
        a, b, c, d, e, f_, g, h, i, j = [mpf(float(x)) for x in coeffs]
        ray = np.asarray(ray, dtype=np.float64).reshape(3, -1)
        source = np.asarray(source, dtype=np.float64).reshape(3, -1)
        out = np.empty((3, ray.shape[1]))
        for col in range(ray.shape[1]):
            l, m, n = (mpf(float(v)) for v in ray[:, col])
            p, q, r = (mpf(float(v)) for v in source[:, col])
            A = a*l**2 + b*m**2 + c*n**2 + d*m*l + e*n*l + f_*m*n
            B = (2*a*p*l + 2*b*q*m + 2*c*r*n + d*(p*m + q*l) + e*(p*n + r*l) + f_*(r*m + q*n)
                 + g*l + h*m + i*n)
            C = a*p**2 + b*q**2 + c*r**2 + d*p*q + e*p*r + f_*q*r + g*p + h*q + i*r + j
            D = B**2 - 4*A*C
            if D < 0:
                out[:, col] = np.nan
                continue
            s = mpmath.sqrt(D)
            t = (-B - s) / (2*A) if negative else (-B + s) / (2*A)
            out[:, col] = [float(t*l + p), float(t*m + q), float(t*n + r)]
    return out


def exact_reflect(ray, N_):
    import mpmath
    with mpmath.workprec(PREC):
        mpf = mpmath.mpf
        ray = np.asarray(ray, dtype=np.float64).reshape(3, -1)
        nrm = np.asarray(N_, dtype=np.float64).reshape(3, -1)
        out = np.empty((3, ray.shape[1]))
        for col in range(ray.shape[1]):
            l, m, n = (mpf(float(v)) for v in ray[:, col])
            nx, ny, nz = (mpf(float(v)) for v in nrm[:, col])
            A = l*nx + m*ny + n*nz
            phi = [l - 2*A*nx, m - 2*A*ny, n - 2*A*nz]
            s = mpmath.sqrt(phi[0]**2 + phi[1]**2 + phi[2]**2)
            if s != 0:
                phi = [v / s for v in phi]
            out[:, col] = [float(v) for v in phi]
    return out


def ulp_dev(got, want):
    """largest |got - want| in ulp of the expected column's largest component (NaN == NaN)"""
    got = np.asarray(got, dtype=np.float64).reshape(3, -1)
    want = np.asarray(want, dtype=np.float64).reshape(3, -1)
    both_nan = np.isnan(got) & np.isnan(want)
    scale = np.spacing(np.nanmax(np.abs(want), axis=0))
    dev = np.where(both_nan, 0.0, np.abs(got - want) / scale)
    return float(np.max(dev))


def run(A, funcs):
    """one 'ray_wave' run with the two primitives bound to `funcs`; returns (calls, griddata inputs)"""
    calls, grid_calls = [], []
    orig = {n: getattr(A, n) for n in NAMES}
    orig_grid = A.griddata

    def wrap(name, f):
        def g(*a, **k):
            r = f(*a, **k)
            calls.append((name, [np.array(x, dtype=np.float64) for x in a if not isinstance(x, bool)],
                          bool(k.get("negative", a[3] if len(a) > 3 else False)), np.array(r)))
            return r
        return g

    def griddata(points, values, xi, method="linear", **kw):
        grid_calls.append((np.array(points[0]), np.array(points[1]), np.array(values)))
        return orig_grid(points, values, xi, method=method, **kw)

    for n in NAMES:
        setattr(A, n, wrap(n, funcs.get(n, orig[n])))
    A.griddata = griddata
    try:
        A.plot_result_debug(best_params(), "ray_wave", option_save=False)
    except Exception as e:  # the cv2 stand-in is reached after the recorded quantities
        print("ray_wave stopped at:", repr(e))
    finally:
        A.griddata = orig_grid
        for n in NAMES:
            setattr(A, n, orig[n])
    return calls, grid_calls


def main():
    _stub_modules()
    sys.path.insert(0, REF)
    os.chdir(tempfile.mkdtemp(prefix="akb_golden_mp_"))
    import AKB_raytrace_20250312 as A
    import matplotlib.pyplot as plt

    A.wave_num_H = A.wave_num_V = N
    A.option_set = True
    A.option_mpmath = True
    calls, grid_ref = run(A, {})
    plt.close("all")
    A.option_mpmath = False  # the replacements below carry the whole evaluation
    _, grid_exact = run(A, {"mirr_ray_intersection": exact_isect, "reflect_ray": exact_reflect})
    plt.close("all")

    out = {}
    for k, (name, args, neg, res) in enumerate(calls):
        key = f"c{k:02d}_{name}"
        for j, a in enumerate(args):
            out[f"{key}_in{j}"] = a
        out[f"{key}_neg"] = np.array(neg)
        out[f"{key}_out"] = res
        want = (exact_isect(args[0], args[1], args[2], neg) if name == "mirr_ray_intersection"
                else exact_reflect(args[0], args[1]))
        out[f"{key}_refdev"] = np.array(ulp_dev(res, want))
        print(key, res.shape, "reference deviation", float(out[f"{key}_refdev"]), "ulp")
    for tag, g in (("ref", grid_ref), ("exact", grid_exact)):
        (y, z, de2), (_, _, w2) = g[0], g[1]
        out[f"{tag}_det2_y"], out[f"{tag}_det2_z"], out[f"{tag}_dist_err2"], out[f"{tag}_wave2"] = y, z, de2, w2
    diff = [float(np.max(np.abs(out["exact_dist_err2"] - out["ref_dist_err2"]))),
            float(np.max(np.abs(out["exact_wave2"] - out["ref_wave2"])))]
    out["exact_minus_ref_nm"] = np.array(diff)
    print("exact run - reference run, max |DistError2|, |Wave2| (nm):", diff)
    print("Wave2 range of the exact run (nm):", float(np.ptp(out["exact_wave2"])))
    np.savez_compressed(os.path.join(OUT, "akb_mpmath_17.npz"), **out)
    print("written", os.path.join(OUT, "akb_mpmath_17.npz"), len(calls), "calls")


if __name__ == "__main__":
    main()
