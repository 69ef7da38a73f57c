"""The k-column triangular solve and pcg_trsm_multi without a kernel launch (include/spmv_mi355x.h "K COLUMNS", "pcg_trsm_multi"):
the five symbols are exported, declared and bound; the refusals come back as rc 1 with their prefix, on the host; and
spmv_mi355x_trsv_solve_multi_plan gives exactly what a numpy restatement of the chunk rule gives.

The solve entries check the handle FIRST, so without a device (no handle can be created there) only the NULL-handle refusal can be
reached; it is shown to come before every other bad argument. The refusals behind it (k, the leading dimensions, in place with two
leading dimensions, a NULL block) and the plan need a handle: those tests are marked gpu, but launch nothing. They pass pointers that
are never dereferenced. pcg_trsm_multi checks what needs no handle first, as pcg_tri_multi does: its table runs on the CPU."""
import ctypes
import inspect
import os

import numpy as np
import pytest

import pcg_tri_multi_cases as mc
import trsv_blocked_cases as bc
import trsv_cases as tc
from conftest import ROOT
from trsv_cases import LOWER, UPPER

NAN, INF = float("nan"), float("inf")
TRSV = ("spmv_mi355x_trsv_solve_multi_device_async", "spmv_mi355x_trsv_solve_multi", "spmv_mi355x_trsv_solve_multi_plan",
        "spmv_mi355x_time_trsv_multi_device")
NEW = TRSV + ("spmv_mi355x_pcg_trsm_multi",)
LDS_BYTES = 160 * 1024
P = lambda a: a.ctypes.data_as(ctypes.c_void_p)


def test_the_symbols_are_exported_declared_and_bound():
    import spmv_mi355x as E
    header = open(os.path.join(ROOT, "include", "spmv_mi355x.h")).read()
    for sym in NEW:
        assert hasattr(E.lib(), sym) and sym in E.SYMBOLS, sym
        assert f"int  {sym}(" in header, sym
    assert ("int  spmv_mi355x_trsv_solve_multi_device_async(spmv_mi355x_trsv * T, int k, const void * b_dev, long ldb, void * x_dev, "
            "long ldx,\n\t\tvoid * hip_stream);") in header
    assert "int  spmv_mi355x_trsv_solve_multi(spmv_mi355x_trsv * T, int k, const void * B_host, void * X_host);" in header
    assert ("int  spmv_mi355x_trsv_solve_multi_plan(const spmv_mi355x_trsv * T, int k, long * matrix_passes_out, long * launches_out,\n"
            "\t\tint * max_chunk_out);") in header
    assert "int  spmv_mi355x_pcg_trsm_multi(spmv_mi355x_matrix * A, int k, const void * B_host, void * X_out_host," in header
    sig = lambda f: list(inspect.signature(f).parameters)
    assert sig(E.TriangularSolve.solve_multi) == ["self", "B"]
    assert sig(E.TriangularSolve.solve_multi_device) == ["self", "k", "b_ptr", "ldb", "x_ptr", "ldx", "stream"]
    assert sig(E.TriangularSolve.solve_multi_plan) == ["self", "k"]
    assert sig(E.TriangularSolve.time_multi_device) == ["self", "k", "b_ptr", "ldb", "x_ptr", "ldx", "iters", "stream"]
    assert sig(E.Matrix.pcg_trsm_multi) == ["self", "B", "precond", "tol", "max_iterations", "history"]
    assert sig(E.Matrix.pcg_tri_multi) == ["self", "B", "precond", "tol", "max_iterations", "history"]


def test_the_header_no_longer_lists_the_k_column_solve_as_not_built():
    header = open(os.path.join(ROOT, "include", "spmv_mi355x.h")).read()
    assert "NOT BUILT: a k-column triangular solve" not in header and "multi-RHS; update_values for a trsv handle" not in header
    assert "a non-zero x0, a k-column triangular solve" not in header
    source = open(os.path.join(ROOT, "spmv-research_amd", "csrc", "solver_pcg_tri.hip")).read()
    assert "ONE BODY, SEVEN ENTRIES" in source and "TriApplyMulti" in source


# ---- the solve entries: the handle comes first ---------------------------------------------------------------------------------------

def test_a_null_handle_is_refused_before_everything_else():
    """every other argument is bad as well (k = 0, ld < k, b == x with two leading dimensions, NULL blocks): the handle is named"""
    import spmv_mi355x as E
    lib = E.lib()
    v = np.full((4, 3), 2.5)
    for args in ((3, P(v), 3, P(v), 3), (0, P(v), 3, P(v), 3), (3, P(v), 2, P(v), 3), (3, P(v), 3, P(v), 4), (3, None, 3, None, 3),
                 (-1, None, 0, None, 1)):
        assert lib.spmv_mi355x_trsv_solve_multi_device_async(None, *args, None) == 1
        assert lib.spmv_mi355x_last_error().startswith(b"trsv_solve_multi: NULL argument ( T )"), lib.spmv_mi355x_last_error()
    for k in (2, 0):
        assert lib.spmv_mi355x_trsv_solve_multi(None, k, P(v), P(v)) == 1
        assert lib.spmv_mi355x_last_error().startswith(b"trsv_solve_multi: NULL argument ( T )")
    passes, launches, widest = ctypes.c_long(-3), ctypes.c_long(-4), ctypes.c_int(-5)
    for k in (2, 0):
        assert lib.spmv_mi355x_trsv_solve_multi_plan(None, k, ctypes.byref(passes), ctypes.byref(launches), ctypes.byref(widest)) == 1
        assert lib.spmv_mi355x_last_error().startswith(b"trsv_solve_multi_plan: NULL argument ( T )")
    assert (passes.value, launches.value, widest.value) == (-3, -4, -5)
    ms = ctypes.c_double(-1.0)
    assert lib.spmv_mi355x_time_trsv_multi_device(None, 2, P(v), 3, P(v), 3, 1, None, ctypes.byref(ms)) == 1
    assert b"trsv" in lib.spmv_mi355x_last_error() and ms.value == -1.0
    assert np.all(v == 2.5)


def test_what_python_refuses_before_the_call():
    import spmv_mi355x as E

    class Solve:                                        # TriangularSolve.solve_multi reads n, dtype and h
        n, dtype, h = 4, np.dtype(np.float64), None

    for bad in (np.ones(4), np.ones((3, 2)), np.ones((4, 0))):
        with pytest.raises(ValueError, match=r"B must have shape \(4, k\)"):
            E.TriangularSolve.solve_multi(Solve(), bad)
    with pytest.raises(E.SpmvError, match=r"trsv_solve_multi: NULL argument \( T \)"):
        E.TriangularSolve.solve_multi(Solve(), np.ones((4, 2)))

    class Handle:                                       # Matrix.pcg_trsm_multi reads m, dtype and h
        m, n, dtype, h = 4, 4, np.dtype(np.float64), None

    for bad in (np.ones(4), np.ones((3, 2))):
        with pytest.raises(ValueError, match=r"B must have shape \(4, k\)"):
            E.Matrix.pcg_trsm_multi(Handle(), bad)
    with pytest.raises(ValueError, match="TriangularSolve"):
        E.Matrix.pcg_trsm_multi(Handle(), np.ones((4, 2)), precond=("lower", None, None))
    for precond in (None, (None, np.ones(4), None)):
        with pytest.raises(E.SpmvError, match="pcg_trsm_multi: NULL argument"):
            E.Matrix.pcg_trsm_multi(Handle(), np.ones((4, 2)), precond=precond)


@pytest.mark.gpu
def test_the_refusals_behind_the_handle_in_their_order():
    """2. k < 1; 3. ldb < k or ldx < k; 4. b == x with ldb != ldx; 5. a NULL block: each with every LATER error in the same call. The
    pointers are host addresses: a refused call touches no device and dereferences nothing."""
    import spmv_mi355x as E
    lib = E.lib()
    rp, ci, va, n = tc.matrix("dag", LOWER)
    v, w = np.full((4, 4), 2.5), np.full((4, 4), -1.5)
    for T in (E.TriangularSolve(rp, ci, va, n), E.TriangularSolve(rp, ci, va, n, block_rows=100)):
        call = lambda k, b, ldb, x, ldx: lib.spmv_mi355x_trsv_solve_multi_device_async(T.h, k, b, ldb, x, ldx, None)
        ordered = [
            ((0, None, 0, None, 1), b"k = 0"),                       # behind it: ld < k is impossible at k = 0; in place; NULL
            ((-2, P(v), 1, P(v), 2), b"k = -2"),
            ((3, P(v), 2, P(v), 3), b"ldb = 2, ldx = 3"),            # behind it: in place with two leading dimensions
            ((3, None, 3, None, 2), b"ldb = 3, ldx = 2"),            # behind it: in place, NULL
            ((3, P(v), 3, P(v), 4), b"b == x (in place) needs ldb == ldx (got 3 and 4)"),
            ((3, None, 3, None, 4), b"b == x (in place) needs ldb == ldx"),          # behind it: NULL
            ((3, None, 3, P(w), 3), b"NULL argument ( b )"),
            ((3, P(v), 3, None, 3), b"NULL argument ( x )"),
            ((3, None, 3, None, 3), b"NULL argument ( b x )"),
        ]
        for args, phrase in ordered:
            assert call(*args) == 1, args
            msg = lib.spmv_mi355x_last_error()
            assert msg.startswith(b"trsv_solve_multi: ") and phrase in msg, (args, msg)
        assert lib.spmv_mi355x_trsv_solve_multi(T.h, 0, P(v), P(w)) == 1 and b"trsv_solve_multi: k = 0" in lib.spmv_mi355x_last_error()
        assert lib.spmv_mi355x_trsv_solve_multi(T.h, 2, None, P(w)) == 1
        assert b"trsv_solve_multi: NULL argument ( b )" in lib.spmv_mi355x_last_error()
        ms = ctypes.c_double(-1.0)
        assert lib.spmv_mi355x_time_trsv_multi_device(T.h, 3, P(v), 2, P(w), 3, 1, None, ctypes.byref(ms)) == 1
        assert b"trsv_solve_multi: ldb = 2, ldx = 3" in lib.spmv_mi355x_last_error() and ms.value == -1.0
        with pytest.raises(E.SpmvError, match="trsv_solve_multi_plan: k = 0"):
            T.solve_multi_plan(0)
        T.close()
    assert np.all(v == 2.5) and np.all(w == -1.5)


# ---- the plan against the restated chunk rule ----------------------------------------------------------------------------------------

def kmax_of(B, n, itemsize):
    """the largest KC in (8, 4, 2, 1) whose min(B, n) * KC values fit in 160 KiB of LDS; a global handle (B = None) has 8"""
    if B is None:
        return 8
    return next(kc for kc in (8, 4, 2, 1) if min(B, n) * kc * itemsize <= LDS_BYTES or kc == 1)


def passes_of(k, kmax):
    """chunks of kmax, then the binary remainder below it"""
    return k // kmax + bin(k % kmax).count("1")


def test_the_restated_chunk_rule_is_column_chunks_at_8():
    for k in range(1, 40):
        assert passes_of(k, 8) == len(mc.chunks(k))
    assert [passes_of(11, m) for m in (8, 4, 2, 1)] == [3, 4, 6, 11]
    assert [kmax_of(B, 20000, 8) for B in (2560, 2561, 5120, 5121, 10240, 10241, 16384)] == [8, 4, 4, 2, 2, 1, 1]
    assert [kmax_of(B, 20000, 4) for B in (5120, 5121, 10240, 10241, 16384)] == [8, 4, 4, 2, 2]
    assert kmax_of(16384, 3000, 8) == 4 and kmax_of(16384, 1, 8) == 8 and 2560 * 8 * 8 == LDS_BYTES


GLOBAL = [("prescribed", 64), ("prescribed", 256), ("bidiagonal", 0), ("dag", 0), ("padding", 0), ("one", 0)]


@pytest.mark.gpu
@pytest.mark.parametrize("uplo,side", ((LOWER, "lower"), (UPPER, "upper")), ids=("lower", "upper"))
@pytest.mark.parametrize("name,chain_rows", GLOBAL, ids=[f"{a}-{c}" for a, c in GLOBAL])
def test_the_plan_of_a_global_handle(name, chain_rows, uplo, side):
    import spmv_mi355x as E
    rp, ci, va, n = tc.matrix(name, uplo)
    T = E.TriangularSolve(rp, ci, va, n, uplo=side, chain_rows=chain_rows)
    launches = tc.plan_of(tc.levels_of(rp, ci, n, uplo), T.info["chain_rows"])[1]
    assert launches == T.info["launches"] > 0
    for k in (1, 3, 8, 9, 17):
        chunks = len(mc.chunks(k))
        assert T.solve_multi_plan(k) == dict(matrix_passes=chunks, launches=chunks * launches, max_chunk=8), k
    T.close()


EDGES = [(np.float64, 2560, 8), (np.float64, 2561, 4), (np.float64, 16384, 1), (np.float32, 16384, 2), (np.float32, 5120, 8),
         (np.float64, 1, 8)]


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,B,kmax", EDGES, ids=[f"{np.dtype(d).name}-{b}" for d, b, _ in EDGES])
def test_the_plan_of_a_blocked_handle_at_the_lds_edges(dtype, B, kmax):
    import spmv_mi355x as E
    rp, ci, va, n = bc.matrix("big_dag", LOWER)
    assert kmax_of(B, n, np.dtype(dtype).itemsize) == kmax
    T = E.TriangularSolve(rp, ci, va, n, dtype=dtype, block_rows=B)
    for k in (1, 2, 3, 8, 9, 17):
        passes = passes_of(k, kmax)
        assert T.solve_multi_plan(k) == dict(matrix_passes=passes, launches=passes, max_chunk=kmax), k
    T.close()


@pytest.mark.gpu
def test_the_plan_of_short_and_empty_handles():
    import spmv_mi355x as E
    # min(block_rows, n) counts: 3000 rows at B = 16384 are 24000 bytes per fp64 column, so 4 columns fit and 8 do not; 9 = 4 + 4 + 1
    rp, ci, va, n = tc.matrix("dag", LOWER)
    assert n == 3000 and kmax_of(16384, n, 8) == 4 and kmax_of(16384, n, 4) == 8
    T = E.TriangularSolve(rp, ci, va, n, block_rows=16384)
    assert T.solve_multi_plan(9) == dict(matrix_passes=3, launches=3, max_chunk=4)
    T.close()
    T = E.TriangularSolve(rp, ci, va, n, block_rows=16384, dtype=np.float32)
    assert T.solve_multi_plan(9) == dict(matrix_passes=2, launches=2, max_chunk=8)
    T.close()
    for B in (None, 64):
        T = E.TriangularSolve(np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros(0), 0, block_rows=B)
        assert T.solve_multi_plan(5) == dict(matrix_passes=0, launches=0, max_chunk=0)
        assert E.lib().spmv_mi355x_trsv_solve_multi_device_async(T.h, 5, None, 5, None, 5, None) == 0          # nothing to solve
        assert T.solve_multi(np.zeros((0, 5))).shape == (0, 5)
        T.close()


# ---- pcg_trsm_multi: the checks that need no handle, in pcg_tri_multi's order ------------------------------------------------------------

CASES = [
    ("null_handle", 3, None, 1e-12, 10, b"NULL argument"),
    ("null_B", 3, None, 1e-12, 10, b"NULL argument"),
    ("null_X_out", 3, None, 1e-12, 10, b"NULL argument"),
    ("k_zero", 0, None, 1e-12, 10, b"k = 0"),
    ("k_negative_before_everything", -2, 0, -1.0, -1, b"k = -2"),
    ("struct_size_unset_first", 3, 0, 1e-12, 10, b"infos[0].struct_size not set"),
    ("struct_size_unset_last", 3, 2, 1e-12, 10, b"infos[2].struct_size not set"),
    ("struct_size_before_tol", 3, 1, -1.0, -1, b"infos[1].struct_size not set"),
    ("tol_negative", 3, None, -1.0, 10, b"tol must be finite and >= 0"),
    ("tol_nan", 3, None, NAN, 10, b"tol must be finite and >= 0"),
    ("tol_inf", 3, None, INF, 10, b"tol must be finite and >= 0"),
    ("tol_before_max_iterations", 3, None, -1.0, -1, b"tol must be finite and >= 0"),
    ("max_iterations_negative", 3, None, 1e-12, -1, b"max_iterations < 0"),
]


def _infos(E, k, unset):
    infos = (E.PcgTriInfo * max(k, 1))()
    for j in range(max(k, 1)):
        infos[j].struct_size = 0 if j == unset else ctypes.sizeof(E.PcgTriInfo)
        infos[j].iterations, infos[j].stop, infos[j].rnorm, infos[j].spmv_calls = -5, -6, -7.5, -9
    return infos


@pytest.mark.parametrize("case,k,unset,tol,max_iterations,phrase", CASES, ids=[c[0] for c in CASES])
def test_pcg_trsm_multi_makes_the_checks_of_pcg_tri_multi_in_its_order(case, k, unset, tol, max_iterations, phrase):
    """the same call to both entries: the same refusal under either name, the caller's buffers and infos untouched"""
    import spmv_mi355x as E
    lib = E.lib()
    B, X, hist = np.full((4, 3), 3.5), np.full((4, 3), -7.25), np.full(30, 9.0)
    said = {}
    for entry in ("pcg_trsm_multi", "pcg_tri_multi"):
        infos = _infos(E, k, unset)
        before = bytes(infos)
        rc = getattr(lib, "spmv_mi355x_" + entry)(None, k, None if case == "null_B" else P(B), None if case == "null_X_out" else P(X), None,
                                                   tol, max_iterations, P(hist), infos)
        msg = lib.spmv_mi355x_last_error()
        assert rc == 1 and msg.startswith(entry.encode() + b": ") and phrase in msg, msg
        assert np.all(B == 3.5) and np.all(X == -7.25) and np.all(hist == 9.0) and bytes(infos) == before
        said[entry] = msg[len(entry):]
    assert said["pcg_trsm_multi"] == said["pcg_tri_multi"]


@pytest.mark.parametrize("part", ["first", "second", "both"])
def test_a_triangular_part_is_not_refused(part):
    """where pcg_tri_multi refuses the triangular part, pcg_trsm_multi goes on to the NULL check: first / second are not looked at
    before A is known"""
    import spmv_mi355x as E
    lib = E.lib()
    fake = np.zeros(8)                                   # any non-NULL address: it is never dereferenced
    scale = np.full(4, 0.5)
    M = E.TriPrecond(ctypes.sizeof(E.TriPrecond), P(fake) if part != "second" else None, P(scale), P(fake) if part != "first" else None)
    B, X = np.full((4, 2), 3.5), np.full((4, 2), -7.25)
    infos = _infos(E, 2, None)
    before = bytes(infos)
    assert lib.spmv_mi355x_pcg_tri_multi(None, 2, P(B), P(X), ctypes.byref(M), 1e-12, 10, None, infos) == 1
    assert b"no k-column triangular solve" in lib.spmv_mi355x_last_error()            # unchanged
    assert lib.spmv_mi355x_pcg_trsm_multi(None, 2, P(B), P(X), ctypes.byref(M), 1e-12, 10, None, infos) == 1
    assert lib.spmv_mi355x_last_error().startswith(b"pcg_trsm_multi: NULL argument ( A )"), lib.spmv_mi355x_last_error()
    assert lib.spmv_mi355x_pcg_trsm_multi(None, 2, P(B), P(X), ctypes.byref(M), -1.0, 10, None, infos) == 1
    assert b"pcg_trsm_multi: tol must be finite" in lib.spmv_mi355x_last_error()
    assert lib.spmv_mi355x_pcg_trsm_multi(None, 2, P(B), P(X), ctypes.byref(M), 1e-12, 10, None, None) == 1            # NULL infos are legal
    assert lib.spmv_mi355x_last_error().startswith(b"pcg_trsm_multi: NULL argument ( A )")
    assert np.all(B == 3.5) and np.all(X == -7.25) and bytes(infos) == before
