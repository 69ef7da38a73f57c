"""CPU tier of spmv_mi355x_spmm_plan (include/spmv_mi355x.h): exported, bound in python, and its argument errors come back as rc 1 with
the entry point's name in the message. The query is host-only: nothing here needs a device."""
import ctypes


def test_the_plan_symbol_is_exported_and_bound():
    import spmv_mi355x as E
    assert hasattr(E.lib(), "spmv_mi355x_spmm_plan")
    assert "spmv_mi355x_spmm_plan" in E.SYMBOLS
    assert callable(E.Matrix.spmm_plan)


def test_bad_arguments_without_a_device():
    import spmv_mi355x as E
    lib = E.lib()
    passes, cols = ctypes.c_int(-5), ctypes.c_int(-6)
    # a handle is only dereferenced after every argument check: a non-NULL token stands in for one where another argument is bad
    buf = ctypes.create_string_buffer(64)
    token = ctypes.c_void_p(ctypes.addressof(buf))
    bad = [(None, 4, ctypes.byref(passes), ctypes.byref(cols), b"NULL handle"),
           (token, 0, ctypes.byref(passes), ctypes.byref(cols), b"k must be >= 1"),
           (token, -2, ctypes.byref(passes), ctypes.byref(cols), b"k must be >= 1"),
           (token, 4, None, ctypes.byref(cols), b"NULL out pointer"),
           (token, 4, ctypes.byref(passes), None, b"NULL out pointer"),
           (None, 0, None, None, b"spmm_plan")]
    for h, k, po, co, text in bad:
        assert lib.spmv_mi355x_spmm_plan(h, ctypes.c_int(k), po, co) == 1, (k, text)
        msg = lib.spmv_mi355x_last_error()
        assert b"spmm_plan" in msg and text in msg, msg
    assert passes.value == -5 and cols.value == -6
