"""CPU tier of the multi-RHS solvers (include/spmv_mi355x.h: spmv_mi355x_pcg_multi, spmv_mi355x_pbicgstab_multi): exported, bound
in python, and their argument errors come back as rc 1 with the entry point's name in the message before any device is touched,
leaving the caller's buffers alone."""
import ctypes

import numpy as np
import pytest

NEW = ("spmv_mi355x_pcg_multi", "spmv_mi355x_pbicgstab_multi")


def test_the_multi_solver_symbols_are_exported_and_bound():
    import spmv_mi355x as E
    lib = E.lib()
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in E.SYMBOLS, name
    for meth in ("pcg_multi", "pbicgstab_multi"):
        assert callable(getattr(E.Matrix, meth)), meth


def _call(fn, k, row_ptr, B, X, hist, info):
    p = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
    col = np.zeros(4, np.int32)
    val = np.ones(4)
    return fn(None, ctypes.c_int(k), p(row_ptr), p(col), p(val), p(B), p(X), ctypes.c_long(10), p(hist),
              None if info is None else ctypes.byref(info))


@pytest.mark.parametrize("name", NEW)
@pytest.mark.parametrize("case,k,expect", [
    ("null_handle", 2, b"NULL argument"),
    ("k0", 0, b"k must be >= 1"),
    ("k_negative", -4, b"k must be >= 1"),
    ("null_B", 2, b"NULL argument"),
    ("null_X", 2, b"NULL argument"),
    ("struct_size_unset", 2, b"struct_size not set"),
])
def test_argument_errors_without_a_device(name, case, k, expect):
    import spmv_mi355x as E
    lib = E.lib()
    fn = getattr(lib, name)
    row_ptr = np.arange(5, dtype=np.int32)
    B = np.full((4, 2), 3.5)
    X = np.full((4, 2), -7.25)
    hist = np.full(2 * 10 * 3, 9.0)
    info = (E.SolverInfo * 2)()
    info[0].struct_size = 0 if case == "struct_size_unset" else ctypes.sizeof(E.SolverInfo)
    info[0].iterations = info[1].iterations = -5
    rc = _call(fn, k, row_ptr, None if case == "null_B" else B, None if case == "null_X" else X, hist, info)
    assert rc == 1
    msg = lib.spmv_mi355x_last_error()
    assert name.removeprefix("spmv_mi355x_").encode() in msg, msg
    assert expect in msg, msg
    assert np.all(B == 3.5) and np.all(X == -7.25) and np.all(hist == 9.0)
    assert info[0].iterations == -5 and info[1].iterations == -5
