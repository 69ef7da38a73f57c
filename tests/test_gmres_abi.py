"""CPU tier of the restarted GMRES solver (include/spmv_mi355x.h: spmv_mi355x_gmres): exported, bound in python, the info struct
mirrored field for field, and every argument error that needs no handle comes back as rc 1 with `gmres` in the message before any
device is touched, leaving the caller's buffers and info alone."""
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
    assert hasattr(lib, "spmv_mi355x_gmres")
    assert "spmv_mi355x_gmres" in E.SYMBOLS
    assert callable(E.Matrix.gmres)
    assert issubclass(E.GmresInfo, ctypes.Structure)


def test_gmres_info_layout_matches_the_header(tmp_path):
    import spmv_mi355x as E
    lines = ['printf("size %zu\\n", sizeof(spmv_mi355x_gmres_info));']
    lines += [f'printf("{f} %zu\\n", offsetof(spmv_mi355x_gmres_info, {f}));' for f, _ in E.GmresInfo._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "spmv_mi355x.h"\nint main(void) {\n' + "\n".join(lines) + "\nreturn 0; }\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(l.split() for l in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    assert int(got["size"]) == ctypes.sizeof(E.GmresInfo)
    assert [f for f, _ in E.GmresInfo._fields_] == ["struct_size", "iterations", "stop", "restarts", "rnorm", "rnorm0", "prnorm",
                                                    "xnorm", "spmv_calls", "seconds"]
    for f, _ in E.GmresInfo._fields_:
        assert int(got[f]) == getattr(E.GmresInfo, f).offset, f


# (case, restart, tol, max_iterations, phrase). The handle is NULL in every case: the scalar and struct_size checks come before the
# NULL check, so each is met on its own (and the scalar cases would meet the NULL check if theirs were missing); the NULL cases pass
# legal scalars.
CASES = [
    ("null_handle", 30, 1e-12, 10, b"NULL argument"),
    ("null_b", 30, 1e-12, 10, b"NULL argument"),
    ("null_x_out", 30, 1e-12, 10, b"NULL argument"),
    ("struct_size_unset", 30, 1e-12, 10, b"struct_size not set"),
    ("restart_zero", 0, 1e-12, 10, b"restart must be 1 .. 128"),
    ("restart_negative", -1, 1e-12, 10, b"restart must be 1 .. 128"),
    ("restart_129", 129, 1e-12, 10, b"restart must be 1 .. 128"),
    ("tol_negative", 30, -1.0, 10, b"tol must be finite and >= 0"),
    ("tol_nan", 30, NAN, 10, b"tol must be finite and >= 0"),
    ("tol_inf", 30, INF, 10, b"tol must be finite and >= 0"),
    ("max_iterations_negative", 30, 1e-12, -1, b"max_iterations < 0"),
]


@pytest.mark.parametrize("with_minv", (False, True), ids=("no_minv", "minv"))
@pytest.mark.parametrize("case,restart,tol,max_iterations,phrase", CASES, ids=[c[0] for c in CASES])
def test_argument_errors_without_a_device(case, restart, tol, max_iterations, phrase, with_minv):
    import spmv_mi355x as E
    lib = E.lib()
    p = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
    b = np.full(4, 3.5)
    x = np.full(4, -7.25)
    minv = np.full(4, 0.5) if with_minv else None
    hist = np.full(10, 9.0)
    info = E.GmresInfo()
    info.struct_size = 0 if case == "struct_size_unset" else ctypes.sizeof(E.GmresInfo)
    info.iterations, info.stop, info.restarts, info.rnorm, info.prnorm, info.spmv_calls = -5, -6, -4, -7.5, -8.5, -9
    before = bytes(info)
    rc = lib.spmv_mi355x_gmres(None, None if case == "null_b" else p(b), None if case == "null_x_out" else p(x), restart, p(minv),
                               tol, max_iterations, p(hist), ctypes.byref(info))
    assert rc == 1
    msg = lib.spmv_mi355x_last_error()
    assert b"gmres" in msg and phrase in msg, msg
    if case.startswith("null"):
        assert b" A " in msg, msg
    if case == "null_b":
        assert b" b " in msg, msg
    if case == "null_x_out":
        assert b" x_out " in msg, msg
    assert np.all(b == 3.5) and np.all(x == -7.25) and np.all(hist == 9.0)
    assert minv is None or np.all(minv == 0.5)
    assert bytes(info) == before


def test_vectors_of_the_wrong_length_are_refused_before_the_call():
    import spmv_mi355x as E

    class Handle:                                       # Matrix.gmres reads m, dtype and h, nothing else
        m, n, dtype, h = 4, 4, np.dtype(np.float64), None

    with pytest.raises(ValueError, match="b must have 4 values"):
        E.Matrix.gmres(Handle(), np.ones(3))
    with pytest.raises(ValueError, match="b must have 4 values"):
        E.Matrix.gmres(Handle(), np.ones((4, 2)))
    with pytest.raises(ValueError, match="minv must have 4 values"):
        E.Matrix.gmres(Handle(), np.ones(4), minv=np.ones(5))
