"""The update_values entry points of include/spmv_mi355x.h (CPU tier: no device is touched): they are declared, bound and exported,
refuse a NULL handle with a message that names them, and did not grow spmv_mi355x_opts."""
import ctypes

import pytest

NAMES = ("spmv_mi355x_update_values_prepare", "spmv_mi355x_update_values", "spmv_mi355x_update_values_device",
         "spmv_mi355x_update_values_state")


@pytest.fixture(scope="module")
def E():
    import spmv_mi355x as E
    return E


def test_symbols_are_bound_and_exported(E):
    lib = E.lib()
    for n in NAMES:
        assert n in E.SYMBOLS, n
        assert hasattr(lib, n), f"{n} is not exported by {E.LIB_PATH}"


@pytest.mark.parametrize("name", NAMES[:3])
def test_null_handle_is_refused_with_a_message(E, name):
    lib = E.lib()
    fn = getattr(lib, name)
    buf = (ctypes.c_double * 4)()
    args = {"spmv_mi355x_update_values_prepare": (None, (ctypes.c_int32 * 2)(0, 0)),
            "spmv_mi355x_update_values": (None, buf),
            "spmv_mi355x_update_values_device": (None, buf, None)}[name]
    assert fn(*args) == 1
    assert b"update_values" in lib.spmv_mi355x_last_error()


def test_state_of_a_null_handle_is_zero(E):
    assert E.lib().spmv_mi355x_update_values_state(None) == 0


def test_opts_did_not_grow(E):
    assert E.Opts._fields_[-1][0] == "value_storage"
