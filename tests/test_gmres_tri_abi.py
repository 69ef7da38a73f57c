"""CPU tier of GMRES with a triangular preconditioner (include/spmv_mi355x.h: spmv_mi355x_gmres_tri): exported, bound in python, the
spmv_mi355x_tri_precond struct mirrored field for field, and the refusals in their order: spmv_mi355x_gmres's own checks come first
and come back as rc 1 with `gmres_tri` in the message before any device is touched, whatever M holds (NULL, an unset struct_size,
three NULL parts: errors of LATER steps), leaving the caller's buffers, M and info alone. The checks of M itself lie behind the NULL
check of A and need a handle: test_gpu_gmres_tri.py has them."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

NAN, INF = float("nan"), float("inf")


def test_the_symbol_is_exported_and_bound():
    import spmv_mi355x as E
    assert hasattr(E.lib(), "spmv_mi355x_gmres_tri") and "spmv_mi355x_gmres_tri" in E.SYMBOLS
    assert issubclass(E.TriPrecond, ctypes.Structure)
    import inspect
    assert "precond" in inspect.signature(E.Matrix.gmres).parameters


def test_tri_precond_layout_matches_the_header(tmp_path):
    import spmv_mi355x as E
    lines = ['printf("size %zu\\n", sizeof(spmv_mi355x_tri_precond));']
    lines += [f'printf("{f} %zu\\n", offsetof(spmv_mi355x_tri_precond, {f}));' for f, _ in E.TriPrecond._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "spmv_mi355x.h"\nint main(void) {\n' + "\n".join(lines) + "\nreturn 0; }\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(l.split() for l in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    assert int(got["size"]) == ctypes.sizeof(E.TriPrecond)
    assert [f for f, _ in E.TriPrecond._fields_] == ["struct_size", "first", "scale_host", "second"]
    for f, _ in E.TriPrecond._fields_:
        assert int(got[f]) == getattr(E.TriPrecond, f).offset, f


# test_gmres_abi.py's table: the handle is NULL in every case, the scalar and struct_size checks come before the NULL check
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
# what M holds: each an error of a later step (or none), which must not be the one reported
PRECONDS = ("null", "size_unset", "all_null", "bad_scale", "scale")


@pytest.mark.parametrize("precond", PRECONDS)
@pytest.mark.parametrize("case,restart,tol,max_iterations,phrase", CASES, ids=[c[0] for c in CASES])
def test_the_checks_of_gmres_come_first(case, restart, tol, max_iterations, phrase, precond):
    import spmv_mi355x as E
    lib = E.lib()
    p = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
    b = np.full(4, 3.5)
    x = np.full(4, -7.25)
    scale = np.array([0.5, 0.0, NAN, 2.0]) if precond == "bad_scale" else np.full(4, 0.5)
    keep = scale.copy()
    hist = np.full(10, 9.0)
    M = E.TriPrecond(0 if precond == "size_unset" else ctypes.sizeof(E.TriPrecond), None,
                     p(scale) if precond in ("bad_scale", "scale") else None, None)
    m_before = bytes(M)
    info = E.GmresInfo()
    info.struct_size = 0 if case == "struct_size_unset" else ctypes.sizeof(E.GmresInfo)
    info.iterations, info.stop, info.restarts, info.rnorm, info.prnorm, info.spmv_calls = -5, -6, -4, -7.5, -8.5, -9
    before = bytes(info)
    rc = lib.spmv_mi355x_gmres_tri(None, None if case == "null_b" else p(b), None if case == "null_x_out" else p(x), restart,
                                   None if precond == "null" else ctypes.byref(M), tol, max_iterations, p(hist), ctypes.byref(info))
    assert rc == 1
    msg = lib.spmv_mi355x_last_error()
    assert msg.startswith(b"gmres_tri: ") and phrase in msg, msg
    if case.startswith("null"):
        assert b" A " in msg, msg
    if case == "null_b":
        assert b" b " in msg, msg
    if case == "null_x_out":
        assert b" x_out " in msg, msg
    assert np.all(b == 3.5) and np.all(x == -7.25) and np.all(hist == 9.0)
    assert scale.tobytes() == keep.tobytes() and bytes(M) == m_before
    assert bytes(info) == before


def test_what_python_refuses_before_the_call():
    import spmv_mi355x as E

    class Handle:                                       # Matrix.gmres reads m, dtype and h, nothing else
        m, n, dtype, h = 4, 4, np.dtype(np.float64), None

    with pytest.raises(ValueError, match="minv and precond"):
        E.Matrix.gmres(Handle(), np.ones(4), minv=np.ones(4), precond=(None, np.ones(4), None))
    with pytest.raises(ValueError, match="TriangularSolve"):
        E.Matrix.gmres(Handle(), np.ones(4), precond=("lower", None, None))
    with pytest.raises(ValueError, match="TriangularSolve"):
        E.Matrix.gmres(Handle(), np.ones(4), precond=(None, None, np.ones(4)))
    with pytest.raises(ValueError, match="scale of precond must have 4 values"):
        E.Matrix.gmres(Handle(), np.ones(4), precond=(None, np.ones(5), None))
    with pytest.raises(ValueError, match="b must have 4 values"):
        E.Matrix.gmres(Handle(), np.ones(3), precond=(None, np.ones(4), None))
    # the library's own refusals arrive as SpmvError: here the NULL handle, whatever the preconditioner
    with pytest.raises(E.SpmvError, match="gmres_tri: NULL argument"):
        E.Matrix.gmres(Handle(), np.ones(4), precond=(None, None, None))
