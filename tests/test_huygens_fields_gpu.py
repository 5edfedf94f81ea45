"""Several fields per pass of the Huygens kernel (akb_huygens_fields_f64, csrc/akb_huygens.hip) on
the MI355X. The contract needs no tolerance: row f of the result is, bit for bit, what the
single-field call (akb_huygens_f64, wavecalc.propagate) returns for u[f] alone with the same split
count - for every n, m, nf and splits, NaN and inf results, the fix-up loop and targets on a source
included. Every comparison here is of the uint64 views, so NaNs count. Inputs are those of
tests/huygens_ref.py."""
import functools

import numpy as np
import pytest
import torch

import huygens_ref as R

pytestmark = pytest.mark.gpu

NF_MAX = 17


def _dev(a, dev):
    return torch.from_numpy(np.array(a)).to(dev)  # (a copy: the shared cases are read-only)


@functools.lru_cache(maxsize=None)
def _fields_of(name):
    """NF_MAX fields over the sources of a huygens_ref sum case: its own first, random ones behind."""
    c = R.sum_case(name)
    m = c["s"].shape[1]
    rng = np.random.default_rng(1000 + m)
    W = rng.standard_normal((NF_MAX, m)) + 1j * rng.standard_normal((NF_MAX, m))
    W[0] = c["w"]
    W.setflags(write=False)
    return W


def _single(dev, t, s, w, k, splits):
    from akbraytracing_amd.wavecalc import propagate
    args = [_dev(a, dev) for a in t] + [_dev(a, dev) for a in s]
    return propagate(*args, _dev(np.asarray(w, dtype=np.complex128), dev), k, splits=splits).cpu().numpy()


def _fields(dev, t, s, W, k, splits, work=None):
    from akbraytracing_amd.wavecalc import propagate_fields
    args = [_dev(a, dev) for a in t] + [_dev(a, dev) for a in s]
    return propagate_fields(*args, _dev(np.asarray(W, dtype=np.complex128), dev), k, splits=splits,
                            work=work).cpu().numpy()


_SINGLES = {}


def _case_single(dev, name, f, splits):
    """The single-field call for field f of a named case, computed once per (case, field, splits)."""
    key = (name, f, splits)
    if key not in _SINGLES:
        c = R.sum_case(name)
        _SINGLES[key] = _single(dev, c["t"], c["s"], _fields_of(name)[f], c["k"], splits)
    return _SINGLES[key]


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint64),
                                                 np.ascontiguousarray(b).view(np.uint64))


def _check_case(dev, name, nf, splits, work=None):
    c = R.sum_case(name)
    got = _fields(dev, c["t"], c["s"], _fields_of(name)[:nf], c["k"], splits, work=work)
    assert got.shape == (nf, c["t"].shape[1]) and got.dtype == np.complex128
    for f in range(nf):
        assert _same_bits(got[f], _case_single(dev, name, f, splits)), (name, nf, splits, f)
    return got


def _group(gpu):
    from akbraytracing_amd.wavecalc import fields_per_pass
    g = fields_per_pass()
    assert g in (4, 8)
    return g


# ----------------------------------------------------------------------------- 1. shapes

@pytest.mark.parametrize("splits", [0, 1, 3])
@pytest.mark.parametrize("nf", [1, 2, 3, 4, 5, 6, 7, 8, 9, 17])
def test_every_group_size_and_remainder(gpu, nf, splits):
    """Every instantiation (2..G fields), the single-field kernel for a group of one, every remainder
    and more than two groups."""
    _check_case(gpu, "shape:513x300", nf, splits)


@pytest.mark.parametrize("splits", [0, 2])
@pytest.mark.parametrize("over", [False, True])
@pytest.mark.parametrize("n,m", [(1, 40), (256, 40), (257, 40), (512, 40), (513, 40), (513, 1), (513, 255),
                                 (513, 256), (513, 257), (513, 513), (3, 300)])
def test_lane_slot_and_tile_edges(gpu, n, m, over, splits):
    _check_case(gpu, f"shape:{n}x{m}", _group(gpu) + 1 if over else 3, splits)


@pytest.mark.parametrize("splits", [2, 127, 128, 129, 257, 301])
def test_reduce_levels(gpu, splits):
    _check_case(gpu, "shape:513x300", 3, splits)


@pytest.mark.parametrize("over", [False, True])
def test_empty_trailing_splits(gpu, over):
    _check_case(gpu, "shape:513x10", _group(gpu) + 1 if over else 3, 7)  # 2 sources per split: splits 5 and 6 are empty


# ----------------------------------------------------------------------------- 2. fix-up, special values

@pytest.mark.parametrize("splits", [1, 3])
@pytest.mark.parametrize("name", ["fixup:all", "fixup:source", "fixup:targets", "fixup:targets@257"])
def test_fixup_redoes_every_field_of_the_group(gpu, name, splits):
    c = R.sum_case(name)
    n = c["t"].shape[1]
    far = np.zeros(n, dtype=bool)
    far[c["far"]] = True
    got = _fields(gpu, c["t"], c["s"], _fields_of(name)[:3], c["k"], splits)
    for f in range(3):
        one = _case_single(gpu, name, f, splits)
        assert np.all(np.isfinite(one.real) & np.isfinite(one.imag))
        assert _same_bits(got[f][far], one[far]), (name, splits, f, "far")
        assert _same_bits(got[f][~far], one[~far]), (name, splits, f, "near")


@pytest.mark.parametrize("splits", [1, 3])
def test_target_on_a_source_is_nan_in_every_field(gpu, splits):
    c = R.sum_case("value")
    on = np.zeros(c["t"].shape[1], dtype=bool)
    on[c["far"]] = True
    got = _check_case(gpu, "value", 3, splits)
    for f in range(3):
        assert np.all(np.isnan(got[f][on].real) & np.isnan(got[f][on].imag))
        assert np.all(np.isfinite(got[f][~on].real) & np.isfinite(got[f][~on].imag))


# ----------------------------------------------------------------------------- 3. fields do not leak

@pytest.mark.parametrize("splits", [1, 3])
def test_fields_do_not_leak_into_each_other(gpu, splits):
    """A row of zeros, a row with a NaN and an inf entry, a row that is another row times 1j: each
    row is its own single call's, whatever its neighbours in the group hold."""
    c = R.sum_case("shape:513x300")
    W = np.array(_fields_of("shape:513x300")[:5])
    W[1] = 0.0
    W[2, 17], W[2, 200] = complex(np.nan, 1.0), complex(np.inf, -2.0)
    W[3] = W[0] * 1j
    got = _fields(gpu, c["t"], c["s"], W, c["k"], splits)
    for f in range(5):
        assert _same_bits(got[f], _single(gpu, c["t"], c["s"], W[f], c["k"], splits)), f
    assert _same_bits(got[0], _case_single(gpu, "shape:513x300", 0, splits))
    assert _same_bits(got[4], _case_single(gpu, "shape:513x300", 4, splits))
    assert np.all(got[1] == 0)
    assert np.all(np.isnan(got[2].real) | np.isnan(got[2].imag))
    # i (a + b i) = -b + a i, exact in every product and sum of the two FMA chains
    assert _same_bits(got[3].real, -got[0].imag) and _same_bits(got[3].imag, got[0].real)


# ----------------------------------------------------------------------------- 4. target slices

@pytest.mark.parametrize("splits", [1, 3, 129])
def test_a_target_slice_is_the_slice_of_the_whole_call(gpu, splits):
    c = R.sum_case("shape:1030x40")
    W = _fields_of("shape:1030x40")[:3]
    whole = _fields(gpu, c["t"], c["s"], W, c["k"], splits)
    part = _fields(gpu, c["t"][:, 250:520], c["s"], W, c["k"], splits)
    assert _same_bits(part, whole[:, 250:520])


# ----------------------------------------------------------------------------- 5. work buffer, empty sizes

@pytest.mark.parametrize("splits", [2, 129])
@pytest.mark.parametrize("nf", [3, 8, 17])
def test_work_bytes_bounds_what_the_kernels_write(gpu, nf, splits):
    """work = a view of exactly akb_huygens_fields_work_bytes inside a NaN-filled tensor: the result
    is the single calls' (no unwritten partial was read), and the guards before and behind the view
    are untouched."""
    from akbraytracing_amd import _lib
    L = _lib.lib()
    c = R.sum_case("shape:513x300")
    n, m = c["t"].shape[1], c["s"].shape[1]
    need = int(L.akb_huygens_fields_work_bytes(n, m, splits, nf))
    assert need == min(nf, _group(gpu)) * int(L.akb_huygens_work_bytes(n, m, splits)) and need % 8 == 0
    need //= 8
    guard = 4096
    big = torch.full((guard + need + guard,), float("nan"), dtype=torch.float64, device=gpu)
    _check_case(gpu, "shape:513x300", nf, splits, work=big[guard:guard + need])
    host = big.cpu().numpy()
    assert np.all(np.isnan(host[:guard])) and np.all(np.isnan(host[guard + need:]))
    assert not np.any(np.isnan(host[guard:guard + min(nf, _group(gpu)) * splits * 2 * n]))


def test_work_bytes_and_empty_sizes(gpu):
    from akbraytracing_amd import _lib
    L = _lib.lib()
    assert L.akb_huygens_fields_work_bytes(513, 300, 1, 5) == 0
    assert L.akb_huygens_fields_work_bytes(513, 300, 0, 5) == (min(5, _group(gpu))
                                                                * L.akb_huygens_work_bytes(513, 300, 0))
    c = R.sum_case("shape:3x300")
    W = _fields_of("shape:3x300")
    none = np.zeros((3, 0))
    for splits in (0, 1, 3):
        for nf in (1, 3, 9):
            out = _fields(gpu, c["t"], none, np.zeros((nf, 0), dtype=np.complex128), c["k"], splits)
            assert out.shape == (nf, 3) and _same_bits(out, np.zeros((nf, 3), dtype=np.complex128))
            out = _fields(gpu, none, c["s"], W[:nf], c["k"], splits)
            assert out.shape == (nf, 0) and out.dtype == np.complex128


def test_too_many_splits_is_refused(gpu):
    from akbraytracing_amd._lib import AKBError
    c = R.sum_case("shape:3x300")
    with pytest.raises(AKBError, match="65535"):
        _fields(gpu, c["t"], c["s"], _fields_of("shape:3x300")[:3], c["k"], 65536)
