"""CPU tier of the least-squares solver (include/spmv_mi355x.h: spmv_mi355x_cgls): exported, bound in python, the info struct
mirrored field for field, and every argument error that needs no handle comes back as rc 1 with `cgls` in the message before any
device is touched, leaving the caller's buffers alone."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

NAN, INF = float("nan"), float("inf")


def test_the_symbol_is_exported_and_bound():
    import spmv_mi355x as E
    lib = E.lib()
    assert hasattr(lib, "spmv_mi355x_cgls")
    assert "spmv_mi355x_cgls" in E.SYMBOLS
    assert callable(E.Matrix.cgls)
    assert issubclass(E.LsqInfo, ctypes.Structure)


def test_lsq_info_layout_matches_the_header(tmp_path):
    import spmv_mi355x as E
    lines = ['printf("size %zu\\n", sizeof(spmv_mi355x_lsq_info));']
    lines += [f'printf("{f} %zu\\n", offsetof(spmv_mi355x_lsq_info, {f}));' for f, _ in E.LsqInfo._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "spmv_mi355x.h"\nint main(void) {\n' + "\n".join(lines) + "\nreturn 0; }\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(l.split() for l in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    assert int(got["size"]) == ctypes.sizeof(E.LsqInfo)
    for f, _ in E.LsqInfo._fields_:
        assert int(got[f]) == getattr(E.LsqInfo, f).offset, f


# (case, damp, tol, max_iterations, phrase). The handles are NULL in every case: the scalar and struct_size checks come before the
# NULL check, so each is met on its own; the NULL cases pass legal scalars.
CASES = [
    ("null_handles", 0.0, 1e-12, 10, b"NULL argument"),
    ("null_b", 0.0, 1e-12, 10, b"NULL argument"),
    ("null_x_out", 0.0, 1e-12, 10, b"NULL argument"),
    ("struct_size_unset", 0.0, 1e-12, 10, b"struct_size not set"),
    ("damp_negative", -1.0, 1e-12, 10, b"damp must be finite and >= 0"),
    ("damp_nan", NAN, 1e-12, 10, b"damp must be finite and >= 0"),
    ("damp_inf", INF, 1e-12, 10, b"damp must be finite and >= 0"),
    ("tol_negative", 0.0, -1.0, 10, b"tol must be finite and >= 0"),
    ("tol_nan", 0.0, NAN, 10, b"tol must be finite and >= 0"),
    ("max_iterations_negative", 0.0, 1e-12, -1, b"max_iterations < 0"),
]


@pytest.mark.parametrize("case,damp,tol,max_iterations,phrase", CASES, ids=[c[0] for c in CASES])
def test_argument_errors_without_a_device(case, damp, tol, max_iterations, phrase):
    import spmv_mi355x as E
    lib = E.lib()
    p = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
    b = np.full(4, 3.5)
    x = np.full(3, -7.25)
    hist = np.full(2 * 10, 9.0)
    info = E.LsqInfo()
    info.struct_size = 0 if case == "struct_size_unset" else ctypes.sizeof(E.LsqInfo)
    info.iterations, info.stop, info.rnorm, info.spmv_calls = -5, -6, -7.5, -8
    before = bytes(info)
    rc = lib.spmv_mi355x_cgls(None, None, None if case == "null_b" else p(b), None if case == "null_x_out" else p(x), damp, tol,
                              max_iterations, p(hist), ctypes.byref(info))
    assert rc == 1
    msg = lib.spmv_mi355x_last_error()
    assert b"cgls" in msg and phrase in msg, msg
    if case == "null_b":
        assert b" b " in msg, msg
    if case == "null_x_out":
        assert b" x_out " in msg, msg
    assert np.all(b == 3.5) and np.all(x == -7.25) and np.all(hist == 9.0)
    assert bytes(info) == before


def test_a_b_of_the_wrong_length_is_refused_before_the_call():
    import spmv_mi355x as E

    class Handle:                                       # Matrix.cgls reads m, n, dtype and h of both sides, nothing else
        m, n, dtype, h = 4, 3, np.dtype(np.float64), None

    with pytest.raises(ValueError, match="b must have 4 values"):
        E.Matrix.cgls(Handle(), Handle(), np.ones(3))
    with pytest.raises(ValueError, match="b must have 4 values"):
        E.Matrix.cgls(Handle(), Handle(), np.ones((4, 2)))
