"""Host side of the tuning field sweep_one (the four-symbol sweep kernel's one-iteration
path): gs_set_tuning takes -1 (automatic, the default), 0 (never) and 1 (required) and
rejects everything else.  No device is touched: gs_set_tuning validates through the
library's table of tuning fields (gs_api.cpp kTuningFields: name, setter, getter), whose
sweep_one entry is called here on a zeroed stand-in for the tuning block."""
import ctypes as C

import pytest

from gibbssampling_amd import _native


class Field(C.Structure):
    _fields_ = [("name", C.c_char_p),
                ("set", C.CFUNCTYPE(C.c_bool, C.c_void_p, C.c_double)),
                ("get", C.CFUNCTYPE(C.c_double, C.c_void_p))]


@pytest.fixture(scope="module")
def field():
    lib = _native.load_library()
    n = C.c_int.in_dll(lib, "kTuningFieldCount").value
    table = (Field * n).in_dll(lib, "kTuningFields")
    found = [f for f in table if f.name == b"sweep_one"]
    assert len(found) == 1
    return found[0]


def test_sweep_one_takes_minus_one_zero_and_one(field):
    block = C.create_string_buffer(4096)  # (far larger than the tuning block)
    for v in (-1.0, 0.0, 1.0, -1.0):
        assert field.set(C.addressof(block), v)
        assert field.get(C.addressof(block)) == v


@pytest.mark.parametrize("v", [-2.0, 2.0, 0.5, -0.5, 1e9, float("nan"), float("inf")])
def test_sweep_one_rejects_other_values(field, v):
    block = C.create_string_buffer(4096)
    assert field.set(C.addressof(block), 1.0)
    assert not field.set(C.addressof(block), v)
    assert field.get(C.addressof(block)) == 1.0  # a rejected value changes nothing


def test_sweep_one_has_an_alias_for_ab_specs():
    assert _native.tuning_spec("GS_SWEEP_ONE=0") == {"sweep_one": 0.0}
