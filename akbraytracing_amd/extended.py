"""The reference's option_mpmath branch on the device: double-double intersection and reflection.

With `option_mpmath = True` (AKB_raytrace_20250312.py:92) the reference's mirr_ray_intersection
(:399-443) and reflect_ray (:474-500, :510-552) run a per-column Python loop of mpmath scalars at
mp.dps = 20 and round the result to float64; Legendrealignment and Finetuning (:13853-14043) set the
flag around every 'ray_wave' evaluation because plain float64 cannot resolve the wavefront of the
aligned system ("Double-double trace"). The two functions here take and return float64
like that branch and carry out the arithmetic in between in double-double (csrc/akb_dd.h, ~106
bits, wider than mp.dps = 20), one HIP kernel each, with the branch's value rules - which differ
from the numpy branch's (primitives.py):

  mirr_ray_intersection  NaN in the columns whose D < 0 only (D == 0 is a hit); no all-NaN rule
  reflect_ray            a zero-norm column is left unnormalised, the others are normalised
  shapes                 the result is 2-D, (3, ray columns): mpmath_matrix_to_numpy (:1305-1323)
                         always returns a matrix, so a (3,) input comes back as (3, 1); the loop
                         runs over the ray's columns and indexes the other argument with them

numpy in, numpy out; torch in, torch (device) out. `prims` carries these two and every other
primitive of primitives.py, for geometry.build_akb(prims=...) and trace.staged_chain(prims=...).
There is no CPU fallback: without a GPU these raise.
"""
from . import _lib
from . import device as D
from . import primitives as P


def _cols(t, what):
    if t.dim() == 1:
        if t.shape[0] != 3:
            raise ValueError(f"{what}: expected 3 components")
        return t.reshape(3, 1)
    if t.dim() != 2 or t.shape[0] != 3:
        raise ValueError(f"{what}: expected a (3, N) array")
    return t


def _pair(a, b, names):
    """Both arguments as (3, n) device blocks, n the first one's column count (the branch's loop
    bound); the second must have at least as many columns (IndexError as mpmath's matrix raises)."""
    x, y = _cols(D.to_dev(a), names[0]), _cols(D.to_dev(b), names[1])
    n = x.shape[1]
    if y.shape[1] < n:
        raise IndexError(f"{names[1]} has {y.shape[1]} columns, {names[0]} has {n}")
    if y.shape[1] > n:
        y = y[:, :n]
    return x.contiguous(), y.contiguous(), n


def mirr_ray_intersection(coeffs, ray, source, negative=False):
    as_torch = P._is_torch(ray, source)
    d, s, n = _pair(ray, source, ("ray", "source"))
    out = D.empty((3, n))
    fl = D.flags_tensor()
    _lib.check(_lib.lib().akb_isect_dd_f64(P._coeffs(coeffs), D.ptr(d), n, 1, D.ptr(s), n, 1, int(bool(negative)), n,
                                           D.ptr(out), n, D.ptr(fl), D.stream_handle()))
    return out if as_torch else out.cpu().numpy()


def reflect_ray(ray, N):
    as_torch = P._is_torch(ray, N)
    d, v, n = _pair(ray, N, ("ray", "N"))
    out = D.empty((3, n))
    fl = D.flags_tensor()
    _lib.check(_lib.lib().akb_reflect_dd_f64(D.ptr(d), n, 1, D.ptr(v), n, 1, n, D.ptr(out), n, D.ptr(fl),
                                             D.stream_handle()))
    return out if as_torch else out.cpu().numpy()


class _Prims:
    """primitives.py's namespace with the two double-double functions in place of the float64 ones."""
    mirr_ray_intersection = staticmethod(mirr_ray_intersection)
    reflect_ray = staticmethod(reflect_ray)

    def __getattr__(self, name):
        return getattr(P, name)


prims = _Prims()
