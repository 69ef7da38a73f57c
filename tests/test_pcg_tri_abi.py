"""CPU tier of the CG preconditioned by triangular solves (include/spmv_mi355x.h: spmv_mi355x_pcg_tri): exported, declared and bound
in python, spmv_mi355x_pcg_tri_info mirrored field for field, the wrapper's own argument errors, and the refusals that need no handle
in their order: info->struct_size, tol, max_iterations come back as rc 1 with `pcg_tri` in the message before the NULL checks and
before any device is touched, whatever M holds (NULL, an unset struct_size, a bad scale: errors of LATER steps), leaving the caller's
buffers, M and info alone. The checks of M itself lie behind the NULL check of A and need a handle: test_gpu_pcg_tri.py has them.

The cases the GPU tier runs are checked here as well (pcg_tri_cases.py): the matrix is symmetric to the bit with cond_2 <= KAPPA,
the restatement of the header's recurrences converges to the dense solve within the GPU tier's bounds, and its iteration counts are
the table of pcg_tri_cases.COUNTS, so that a change of the cases shows here and not on the GPU."""
import ctypes
import inspect
import os
import subprocess

import numpy as np
import pytest

import pcg_tri_cases as pc
from conftest import ROOT

NAN, INF = float("nan"), float("inf")


def test_the_symbol_is_exported_declared_and_bound():
    import spmv_mi355x as E
    assert hasattr(E.lib(), "spmv_mi355x_pcg_tri") and "spmv_mi355x_pcg_tri" in E.SYMBOLS
    header = open(os.path.join(ROOT, "include", "spmv_mi355x.h")).read()
    assert "int  spmv_mi355x_pcg_tri(spmv_mi355x_matrix * A, const void * b_host, void * x_out_host," in header
    assert "} spmv_mi355x_pcg_tri_info;" in header
    assert issubclass(E.PcgTriInfo, ctypes.Structure)
    assert list(inspect.signature(E.Matrix.pcg_tri).parameters) == ["self", "b", "precond", "tol", "max_iterations", "history"]
    assert list(inspect.signature(E.sgs_precond).parameters)[:6] == ["row_ptr", "col_idx", "values", "n", "dtype", "block_rows"]


def test_the_info_layout_matches_the_header(tmp_path):
    import spmv_mi355x as E
    lines = ['printf("size %zu\\n", sizeof(spmv_mi355x_pcg_tri_info));']
    lines += [f'printf("{f} %zu\\n", offsetof(spmv_mi355x_pcg_tri_info, {f}));' for f, _ in E.PcgTriInfo._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "spmv_mi355x.h"\nint main(void) {\n' + "\n".join(lines) + "\nreturn 0; }\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(l.split() for l in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    assert int(got["size"]) == ctypes.sizeof(E.PcgTriInfo)
    assert [f for f, _ in E.PcgTriInfo._fields_] == ["struct_size", "iterations", "stop", "rnorm", "rnorm0", "prnorm", "xnorm",
                                                     "spmv_calls", "seconds"]
    for f, _ in E.PcgTriInfo._fields_:
        assert int(got[f]) == getattr(E.PcgTriInfo, f).offset, f


def test_the_header_no_longer_lists_cg_as_not_built():
    header = open(os.path.join(ROOT, "include", "spmv_mi355x.h")).read()
    assert "pcg / pbicgstab / minres" not in header
    assert header.count("pbicgstab / minres") >= 2


# the handle is NULL in every case: the scalar and struct_size checks come before the NULL check
CASES = [
    ("null_handle", 1e-12, 10, b"NULL argument"),
    ("null_b", 1e-12, 10, b"NULL argument"),
    ("null_x_out", 1e-12, 10, b"NULL argument"),
    ("struct_size_unset", 1e-12, 10, b"struct_size not set"),
    ("struct_size_unset_and_tol", -1.0, -1, b"struct_size not set"),
    ("tol_negative", -1.0, 10, b"tol must be finite and >= 0"),
    ("tol_nan", NAN, 10, b"tol must be finite and >= 0"),
    ("tol_inf", INF, 10, b"tol must be finite and >= 0"),
    ("tol_before_max_iterations", -1.0, -1, b"tol must be finite and >= 0"),
    ("max_iterations_negative", 1e-12, -1, b"max_iterations < 0"),
]
# what M holds: each an error of a later step (or none), which must not be the one reported
PRECONDS = ("null", "size_unset", "all_null", "bad_scale", "scale")


@pytest.mark.parametrize("precond", PRECONDS)
@pytest.mark.parametrize("case,tol,max_iterations,phrase", CASES, ids=[c[0] for c in CASES])
def test_the_checks_that_need_no_handle_in_their_order(case, tol, max_iterations, phrase, precond):
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
    info = E.PcgTriInfo()
    info.struct_size = 0 if case.startswith("struct_size_unset") else ctypes.sizeof(E.PcgTriInfo)
    info.iterations, info.stop, info.rnorm, info.rnorm0, info.prnorm, info.xnorm, info.spmv_calls = -5, -6, -7.5, -4.5, -8.5, -3.5, -9
    before = bytes(info)
    rc = lib.spmv_mi355x_pcg_tri(None, None if case == "null_b" else p(b), None if case == "null_x_out" else p(x),
                                 None if precond == "null" else ctypes.byref(M), tol, max_iterations, p(hist), ctypes.byref(info))
    assert rc == 1
    msg = lib.spmv_mi355x_last_error()
    assert msg.startswith(b"pcg_tri: ") and phrase in msg, msg
    if case.startswith("null"):
        assert b" A " in msg, msg
    if case == "null_b":
        assert b" b " in msg, msg
    if case == "null_x_out":
        assert b" x_out " in msg, msg
    assert np.all(b == 3.5) and np.all(x == -7.25) and np.all(hist == 9.0)
    assert scale.tobytes() == keep.tobytes() and bytes(M) == m_before
    assert bytes(info) == before


def test_a_null_info_is_legal_and_the_next_check_fires():
    import spmv_mi355x as E
    rc = E.lib().spmv_mi355x_pcg_tri(None, None, None, None, -1.0, 10, None, None)
    assert rc == 1 and b"pcg_tri: tol must be finite" in E.lib().spmv_mi355x_last_error()


def test_what_python_refuses_before_the_call():
    import spmv_mi355x as E

    class Handle:                                       # Matrix.pcg_tri reads m, dtype and h, nothing else
        m, n, dtype, h = 4, 4, np.dtype(np.float64), None

    with pytest.raises(ValueError, match="TriangularSolve"):
        E.Matrix.pcg_tri(Handle(), np.ones(4), precond=("lower", None, None))
    with pytest.raises(ValueError, match="TriangularSolve"):
        E.Matrix.pcg_tri(Handle(), np.ones(4), precond=(None, None, np.ones(4)))
    with pytest.raises(ValueError, match="scale of precond must have 4 values"):
        E.Matrix.pcg_tri(Handle(), np.ones(4), precond=(None, np.ones(5), None))
    with pytest.raises(ValueError, match="b must have 4 values"):
        E.Matrix.pcg_tri(Handle(), np.ones(3), precond=(None, np.ones(4), None))
    with pytest.raises(ValueError):
        E.Matrix.pcg_tri(Handle(), np.ones(4), precond=(None, None))            # not a triple
    # the library's own refusals arrive as SpmvError: here the NULL handle, with and without a preconditioner
    for precond in (None, (None, None, None), (None, np.ones(4), None)):
        with pytest.raises(E.SpmvError, match="pcg_tri: NULL argument"):
            E.Matrix.pcg_tri(Handle(), np.ones(4), precond=precond)
    with pytest.raises(E.SpmvError, match="pcg_tri: tol must be finite"):
        E.Matrix.pcg_tri(Handle(), np.ones(4), tol=-1.0)
    # sgs_precond finds a missing diagonal before it asks for a device
    with pytest.raises(ValueError, match="no diagonal"):
        E.sgs_precond(np.array([0, 1, 2], np.int32), np.array([1, 1], np.int32), np.ones(2), 2)


# ---- the cases of the GPU tier -------------------------------------------------------------------------------------------------------

def test_the_matrix_is_what_the_gpu_tier_assumes():
    P = pc.problem()
    rp, ci, va = P.csr
    assert P.n == 2025 and rp[-1] == 5 * P.n - 4 * 45 and P.k_row == 5
    assert np.array_equal(P.D, P.D.T)
    assert 90 < P.cond() <= pc.KAPPA
    L, lo, up = P.ic0()
    assert np.array_equal((L != 0), np.tril(P.D != 0)) and 1.4 < np.diag(L).min() < 1.6
    on = np.tril(P.D != 0)
    assert np.abs((L @ L.T - P.D)[on]).max() <= 1e-14 * np.abs(P.D).max()       # IC(0): exact on the pattern


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_the_restatement_converges_and_its_counts_are_the_table(dtype):
    P = pc.problem()
    tol = pc.PREC[dtype]["tol"]
    want, bn = P.solve(), np.linalg.norm(P.b)
    counts = {}
    for kind in pc.KINDS + ("mixed",):
        x, hist, stop = P.restatement(dtype, kind, tol)
        assert stop == 1 and x.dtype == dtype, kind
        counts[kind] = hist.size
        rn = np.linalg.norm(P.b - P.D @ x.astype(np.float64))
        ex = np.linalg.norm(x.astype(np.float64) - want) / np.linalg.norm(want)
        assert rn <= 0.1 * 10 * tol * bn and ex <= 0.03 * pc.KAPPA * 10 * tol, (kind, rn, ex)   # what the GPU tier's docstring quotes
    assert counts.pop("mixed") == counts["sgs"]                                  # B >= n drops nothing
    assert counts == pc.COUNTS[dtype], counts
    # properties of the input that the GPU tier relies on
    assert all(counts[B] < counts["jacobi"] for B in pc.BLOCKS)
    if dtype == np.float64:
        assert all(counts[k] > 2 * pc.POLL for k in ("none", "jacobi", 64))


def test_the_restatement_stops_as_the_header_says():
    P = pc.problem()
    A, b = P.dense(np.float64), P.b
    x, hist, stop = pc.restate(A, b, None, 0.0, 10, np.float64)
    assert stop == 2 and hist.size == 10
    x, hist, stop = pc.restate(A, b, None, 1e-12, 0, np.float64)
    assert stop == 2 and hist.size == 0 and not x.any()
    x, hist, stop = pc.restate(A, np.zeros(P.n), None, 1e-12, 10, np.float64)
    assert stop == 3 and hist.size == 0 and not x.any()
    x, hist, stop = pc.restate(P.dense(np.float64, True), b, None, 1e-12, 10, np.float64)
    assert stop == 4 and hist.size == 0 and not x.any()
    x, hist, stop = pc.restate(A, b, lambda v: -v / P.diag, 1e-12, 10, np.float64)
    assert stop == 4 and hist.size == 0 and not x.any()
