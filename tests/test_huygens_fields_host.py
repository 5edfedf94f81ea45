"""The refusals of akb_huygens_fields_f64 and wavecalc.propagate_fields that happen before any
launch, without a GPU (the pointers handed in are never dereferenced)."""
import ctypes

import numpy as np
import pytest
import torch


def _call(L, n=4, m=4, nf=2, splits=1, null=(), work=None):
    buf = np.zeros(64)
    p = {name: (None if name in null else ctypes.c_void_p(buf.ctypes.data))
         for name in ("tx", "ty", "tz", "sx", "sy", "sz", "u", "out")}
    return L.akb_huygens_fields_f64(p["tx"], p["ty"], p["tz"], n, p["sx"], p["sy"], p["sz"], p["u"], m, nf, 1.0,
                                    p["out"], splits, work, None)


@pytest.mark.parametrize("kwargs,message", [
    (dict(nf=0), b"at least one field"),
    (dict(nf=-3), b"at least one field"),
    (dict(n=-1), b"negative size"),
    (dict(m=-1), b"negative size"),
    (dict(null=("tx",)), b"null target pointer"),
    (dict(null=("out",)), b"null target pointer"),
    (dict(null=("sy",)), b"null source pointer"),
    (dict(null=("u",)), b"null source pointer"),
    (dict(splits=65536), b"at most 65535 source splits"),
    (dict(splits=2), b"work buffer required"),
])
def test_refusals_carry_a_message(kwargs, message):
    from akbraytracing_amd import _lib
    L = _lib.lib()
    st = _call(L, **kwargs)
    assert st == -1 and message in L.akb_last_error()
    with pytest.raises(_lib.AKBError):
        _lib.check(st)


def test_no_targets_is_a_no_op_whatever_the_pointers():
    from akbraytracing_amd import _lib
    L = _lib.lib()
    assert _call(L, n=0, null=("tx", "ty", "tz", "sx", "sy", "sz", "u", "out")) == 0


def test_work_bytes_without_a_launch():
    from akbraytracing_amd import _lib, wavecalc
    L = _lib.lib()
    g = wavecalc.fields_per_pass()
    assert g in (4, 8)
    one = L.akb_huygens_work_bytes(513, 300, 129)
    assert one == (129 + 2) * 2 * 513 * 8
    for nf in (1, 2, g - 1, g, g + 1, 100):
        assert L.akb_huygens_fields_work_bytes(513, 300, 129, nf) == min(nf, g) * one
        assert L.akb_huygens_fields_work_bytes(513, 300, 1, nf) == 0
    assert L.akb_huygens_fields_work_bytes(513, 300, 129, 0) == 0
    assert L.akb_huygens_fields_work_bytes(0, 300, 129, 3) == 0 and L.akb_huygens_fields_work_bytes(513, 0, 129, 3) == 0


def test_propagate_fields_refuses_a_single_field_and_a_wrong_length():
    from akbraytracing_amd.wavecalc import propagate_fields
    t = [torch.zeros(5, dtype=torch.float64)] * 3
    s = [torch.zeros(7, dtype=torch.float64)] * 3
    with pytest.raises(ValueError, match="propagate takes a single field"):
        propagate_fields(*t, *s, torch.zeros(7, dtype=torch.complex128), 1.0)
    with pytest.raises(ValueError):
        propagate_fields(*t, *s, torch.zeros((2, 6), dtype=torch.complex128), 1.0)
    with pytest.raises(ValueError):
        propagate_fields(*t, *s, torch.zeros((0, 7), dtype=torch.complex128), 1.0)
    with pytest.raises(ValueError):
        propagate_fields(*t, *s, torch.zeros((2, 7), dtype=torch.complex64), 1.0)
