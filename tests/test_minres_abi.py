"""CPU tier of the symmetric indefinite solver (include/spmv_mi355x.h: spmv_mi355x_minres): exported, bound in python, the info
struct mirrored field for field, and every argument error that needs no handle comes back as rc 1 with `minres` in the message
before any device is touched, leaving the caller's buffers and info alone."""
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
    assert hasattr(lib, "spmv_mi355x_minres")
    assert "spmv_mi355x_minres" in E.SYMBOLS
    assert callable(E.Matrix.minres)
    assert issubclass(E.MinresInfo, ctypes.Structure)


def test_minres_info_layout_matches_the_header(tmp_path):
    import spmv_mi355x as E
    lines = ['printf("size %zu\\n", sizeof(spmv_mi355x_minres_info));']
    lines += [f'printf("{f} %zu\\n", offsetof(spmv_mi355x_minres_info, {f}));' for f, _ in E.MinresInfo._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "spmv_mi355x.h"\nint main(void) {\n' + "\n".join(lines) + "\nreturn 0; }\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(l.split() for l in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    assert int(got["size"]) == ctypes.sizeof(E.MinresInfo)
    assert [f for f, _ in E.MinresInfo._fields_] == ["struct_size", "iterations", "stop", "rnorm", "rnorm0", "prnorm", "prnorm0",
                                                     "xnorm", "spmv_calls", "seconds"]
    for f, _ in E.MinresInfo._fields_:
        assert int(got[f]) == getattr(E.MinresInfo, f).offset, f


# (case, shift, tol, max_iterations, phrase). The handle is NULL in every case: the scalar and struct_size checks come before the
# NULL check, so each is met on its own (and the scalar cases would meet the NULL check if theirs were missing); the NULL cases pass
# legal scalars.
CASES = [
    ("null_handle", 0.0, 1e-12, 10, b"NULL argument"),
    ("null_b", 0.0, 1e-12, 10, b"NULL argument"),
    ("null_x_out", 0.0, 1e-12, 10, b"NULL argument"),
    ("struct_size_unset", 0.0, 1e-12, 10, b"struct_size not set"),
    ("shift_nan", NAN, 1e-12, 10, b"shift must be finite"),
    ("shift_inf", INF, 1e-12, 10, b"shift must be finite"),
    ("shift_minus_inf", -INF, 1e-12, 10, b"shift must be finite"),
    ("tol_negative", 0.0, -1.0, 10, b"tol must be finite and >= 0"),
    ("tol_nan", 0.0, NAN, 10, b"tol must be finite and >= 0"),
    ("tol_inf", 0.0, INF, 10, b"tol must be finite and >= 0"),
    ("max_iterations_negative", 0.0, 1e-12, -1, b"max_iterations < 0"),
]


@pytest.mark.parametrize("with_minv", (False, True), ids=("no_minv", "minv"))
@pytest.mark.parametrize("case,shift,tol,max_iterations,phrase", CASES, ids=[c[0] for c in CASES])
def test_argument_errors_without_a_device(case, shift, tol, max_iterations, phrase, with_minv):
    import spmv_mi355x as E
    lib = E.lib()
    p = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
    b = np.full(4, 3.5)
    x = np.full(4, -7.25)
    minv = np.full(4, 0.5) if with_minv else None
    hist = np.full(10, 9.0)
    info = E.MinresInfo()
    info.struct_size = 0 if case == "struct_size_unset" else ctypes.sizeof(E.MinresInfo)
    info.iterations, info.stop, info.rnorm, info.prnorm, info.spmv_calls = -5, -6, -7.5, -8.5, -9
    before = bytes(info)
    rc = lib.spmv_mi355x_minres(None, None if case == "null_b" else p(b), None if case == "null_x_out" else p(x), shift, p(minv),
                                tol, max_iterations, p(hist), ctypes.byref(info))
    assert rc == 1
    msg = lib.spmv_mi355x_last_error()
    assert b"minres" in msg and phrase in msg, msg
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

    class Handle:                                       # Matrix.minres reads m, dtype and h, nothing else
        m, n, dtype, h = 4, 4, np.dtype(np.float64), None

    with pytest.raises(ValueError, match="b must have 4 values"):
        E.Matrix.minres(Handle(), np.ones(3))
    with pytest.raises(ValueError, match="b must have 4 values"):
        E.Matrix.minres(Handle(), np.ones((4, 2)))
    with pytest.raises(ValueError, match="minv must have 4 values"):
        E.Matrix.minres(Handle(), np.ones(4), minv=np.ones(5))
