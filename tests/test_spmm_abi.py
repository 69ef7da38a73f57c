"""CPU tier of the multi-vector entry points (include/spmv_mi355x.h: spmv_mi355x_spmm_device_async, spmv_mi355x_time_spmm_device,
spmv_mi355x_spmm): exported, bound in python, and their argument errors come back as rc 1 with the entry point's name in the message
before any device is touched."""
import ctypes

import numpy as np
import pytest

NEW = ("spmv_mi355x_spmm_device_async", "spmv_mi355x_time_spmm_device", "spmv_mi355x_spmm")


def test_the_spmm_symbols_are_exported_and_bound():
    import spmv_mi355x as E
    lib = E.lib()
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in E.SYMBOLS, name
    for meth in ("spmm", "spmm_device", "time_spmm_device"):
        assert callable(getattr(E.Matrix, meth)), meth


@pytest.mark.parametrize("k,ldx,ldy", [(0, 4, 4), (-3, 4, 4), (4, 3, 4), (4, 4, 3), (4, 4, 4), (1, 1, 1)])
def test_bad_arguments_and_null_handle_without_a_device(k, ldx, ldy):
    import spmv_mi355x as E
    lib = E.lib()
    X = np.ones(64)
    Y = np.full(64, -7.25)
    xp, yp = X.ctypes.data_as(ctypes.c_void_p), Y.ctypes.data_as(ctypes.c_void_p)
    assert lib.spmv_mi355x_spmm_device_async(None, ctypes.c_int(k), xp, ctypes.c_long(ldx), yp, ctypes.c_long(ldy), ctypes.c_int(0), None) == 1
    msg = lib.spmv_mi355x_last_error()
    assert b"spmm_device_async" in msg
    assert (b"NULL handle" in msg) == (k >= 1 and ldx >= k and ldy >= k)
    ms = ctypes.c_double(-1.0)
    assert lib.spmv_mi355x_time_spmm_device(None, ctypes.c_int(k), xp, ctypes.c_long(ldx), yp, ctypes.c_long(ldy), ctypes.c_int(3), None,
                                            ctypes.byref(ms)) == 1
    assert b"time_spmm_device" in lib.spmv_mi355x_last_error() and ms.value == -1.0
    assert lib.spmv_mi355x_spmm(None, ctypes.c_int(k), xp, yp) == 1
    assert b"spmm" in lib.spmv_mi355x_last_error()
    assert np.all(Y == -7.25) and np.all(X == 1.0)
