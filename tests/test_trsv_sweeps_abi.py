"""The Jacobi-sweep triangular solve without a kernel launch (include/spmv_mi355x.h "JACOBI SWEEPS"): the six symbols are exported,
declared and bound; the sequential restatement of tests/trsv_sweeps_reference.c returns the bits of tests/trsv_reference.c from
`levels` sweeps on; pcg_tri_cases.restate under the swept SGS / IC(0) gives the pinned iteration counts; and the refusals come back
as rc 1 with their prefix, on the host.

The entries check the handle FIRST, so without a device (no handle can be created there) only the NULL-handle refusal can be reached;
it is shown to come before every other bad argument. The refusals behind it and trsv_sweeps_info need a handle: those tests are marked
gpu, but launch nothing. They pass pointers that are never dereferenced."""
import ctypes
import inspect
import os

import numpy as np
import pytest

import pcg_tri_cases as pc
import trsv_cases as tc
import trsv_sweeps_cases as sc
from conftest import ROOT
from trsv_cases import LOWER, UPPER

NEW = ("spmv_mi355x_trsv_solve_sweeps_device_async", "spmv_mi355x_trsv_solve_sweeps", "spmv_mi355x_trsv_solve_sweeps_multi_device_async",
       "spmv_mi355x_trsv_solve_sweeps_multi", "spmv_mi355x_trsv_set_sweeps", "spmv_mi355x_trsv_sweeps_info")
P = lambda a: a.ctypes.data_as(ctypes.c_void_p)
FORMS = [(uplo, unit, dtype) for uplo in (LOWER, UPPER) for unit in (False, True) for dtype in (np.float64, np.float32)]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def test_the_symbols_are_exported_declared_and_bound():
    import spmv_mi355x as E
    header = open(os.path.join(ROOT, "include", "spmv_mi355x.h")).read()
    for sym in NEW:
        assert hasattr(E.lib(), sym) and sym in E.SYMBOLS, sym
        assert f"int  {sym}(" in header, sym
    assert ("int  spmv_mi355x_trsv_solve_sweeps_device_async(spmv_mi355x_trsv * T, int sweeps, const void * b_dev, void * x_dev, "
            "void * hip_stream);") in header
    assert "int  spmv_mi355x_trsv_solve_sweeps(spmv_mi355x_trsv * T, int sweeps, const void * b_host, void * x_host);" in header
    assert "int  spmv_mi355x_trsv_set_sweeps(spmv_mi355x_trsv * T, int sweeps /* 0 = exact (the default) */);" in header
    sig = lambda f: list(inspect.signature(f).parameters)
    assert sig(E.TriangularSolve.__init__)[-1] == "sweeps" and inspect.signature(E.TriangularSolve.__init__).parameters["sweeps"].default == 0
    assert sig(E.TriangularSolve.set_sweeps) == ["self", "sweeps"]
    assert isinstance(E.TriangularSolve.sweeps, property)
    assert sig(E.TriangularSolve.solve_sweeps) == ["self", "b", "sweeps"]
    assert sig(E.TriangularSolve.solve_sweeps_device) == ["self", "b_ptr", "x_ptr", "sweeps", "stream"]
    assert sig(E.TriangularSolve.solve_sweeps_multi) == ["self", "B", "sweeps"]
    assert sig(E.TriangularSolve.solve_sweeps_multi_device) == ["self", "k", "b_ptr", "ldb", "x_ptr", "ldx", "sweeps", "stream"]
    assert sig(E.TriangularSolve.sweeps_info) == ["self", "k"]
    source = open(os.path.join(ROOT, "spmv-research_amd", "csrc", "trsv.hpp")).read()
    assert "TRSV_SWEEPS_MAX = 1 << 20" in source and sc.SWEEPS_MAX == 1 << 20 >= 65536


# ---- the reference against the exact loop ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sc.MATRICES)
def test_levels_sweeps_return_the_bits_of_the_exact_solve(name):
    """fp64 and fp32, LOWER and UPPER, STORED and UNIT: sweeps = levels (from trsv_cases.levels_of) and levels + 3 are the sequential
    loop of trsv_reference.c to the bit. On prescribed (12 levels) and padding (2) one sweep less is NOT: the boundary is sharp."""
    differ = 0
    for uplo, unit, dtype in FORMS:
        A = tc.matrix(name, uplo)
        n = A[3]
        levels = sc.depth(name, uplo)
        assert levels == int(tc.levels_of(A[0], A[1], n, uplo).max()) + 1
        b = sc.rhs(n, dtype)
        before = b.tobytes()
        want = tc.reference(*A, uplo, unit, b, dtype)
        assert np.all(np.isfinite(want))
        for sweeps in (levels, levels + 3):
            got = sc.reference(*A, uplo, unit, b, dtype, sweeps)
            assert same_bits(got, want), f"{name} uplo {uplo} unit {unit} {np.dtype(dtype).name}: {sweeps} sweeps, {levels} levels: " \
                f"{int(np.sum(got != want))} of {n} rows differ"
        assert b.tobytes() == before
        if levels > 1:
            differ += not same_bits(sc.reference(*A, uplo, unit, b, dtype, levels - 1), want)
    assert {"one": 1, "diagonal": 1, "prescribed": 12, "padding": 2, "dag": 708, "stencil": 70}[name] == sc.depth(name, LOWER)
    if name in ("prescribed", "padding"):
        assert differ >= len(FORMS) - 1, f"{name}: levels - 1 sweeps differ from the exact solve in {differ} of {len(FORMS)} forms only"


def test_the_first_sweep_reads_no_entry():
    """x(1) = b / d: an Inf and a NaN among the off-diagonal entries do not reach it; the second sweep sees them"""
    rp, ci, va, n = tc.matrix("dag", LOWER)
    rows = np.repeat(np.arange(n), np.diff(rp))
    off = np.nonzero(ci != rows)[0]
    bad = va.copy()
    bad[off[0]], bad[off[-1]] = np.inf, np.nan
    for dtype in (np.float64, np.float32):
        b = sc.rhs(n, dtype)
        d = va[ci == rows].astype(dtype)
        assert same_bits(sc.reference(rp, ci, bad, n, LOWER, False, b, dtype, 1), (b / d).astype(dtype))
        assert same_bits(sc.reference(rp, ci, bad, n, LOWER, True, b, dtype, 1), b)
        assert not np.all(np.isfinite(sc.reference(rp, ci, bad, n, LOWER, False, b, dtype, 2)))


# ---- CG under the swept preconditioners -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ("sgs", "ic0"))
@pytest.mark.parametrize("dtype", (np.float64, np.float32), ids=("f64", "f32"))
def test_the_cg_counts_under_swept_preconditioners(dtype, kind):
    """one sweep is exactly the Jacobi count, 89 sweeps (the depth of spd_grid(45)'s triangles) the exact preconditioner's count"""
    Pr = pc.problem()
    rp, ci, _ = Pr.csr
    assert int(tc.levels_of(rp, ci, Pr.n, LOWER).max()) + 1 == 89 == int(tc.levels_of(rp, ci, Pr.n, UPPER).max()) + 1
    counts = {}
    for sweeps in sc.CG_SWEEPS:
        _, hist, stop = sc.cg_restatement(dtype, kind, sweeps)
        assert stop == 1, (kind, sweeps, stop)
        counts[sweeps] = hist.size
    print(f"[trsv_sweeps] CG on spd_grid(45), {np.dtype(dtype).name}, swept {kind}: iterations by sweeps {counts}")
    assert counts == sc.COUNTS[dtype][kind]
    assert counts[1] == pc.COUNTS[dtype]["jacobi"] and counts[89] == pc.COUNTS[dtype][kind]
    assert counts[1] > counts[2] > counts[4] >= counts[89]
    # at the depth the swept operator IS the exact one: the same history to the bit
    _, exact, _ = Pr.restatement(dtype, kind, pc.PREC[dtype]["tol"])
    assert same_bits(sc.cg_restatement(dtype, kind, 89)[1], exact)


# ---- the refusals ---------------------------------------------------------------------------------------------------------------------------

def test_a_null_handle_is_refused_before_everything_else():
    """every other argument is bad as well (sweeps out of range, k = 0, ld < k, NULL vectors): the handle is named"""
    import spmv_mi355x as E
    lib = E.lib()
    v = np.full((4, 3), 2.5)
    for sweeps in (2, 0, -1, sc.SWEEPS_MAX + 1):
        for args in ((3, P(v), 3, P(v), 3), (0, P(v), 3, P(v), 3), (3, P(v), 2, P(v), 3), (3, P(v), 3, P(v), 4), (3, None, 3, None, 3)):
            assert lib.spmv_mi355x_trsv_solve_sweeps_multi_device_async(None, sweeps, *args, None) == 1
            assert lib.spmv_mi355x_last_error().startswith(b"trsv_solve_sweeps: NULL argument ( T )"), lib.spmv_mi355x_last_error()
        for b, x in ((P(v), P(v)), (None, None)):
            assert lib.spmv_mi355x_trsv_solve_sweeps_device_async(None, sweeps, b, x, None) == 1
            assert lib.spmv_mi355x_last_error().startswith(b"trsv_solve_sweeps: NULL argument ( T )")
            assert lib.spmv_mi355x_trsv_solve_sweeps(None, sweeps, b, x) == 1
            assert lib.spmv_mi355x_last_error().startswith(b"trsv_solve_sweeps: NULL argument ( T )")
            assert lib.spmv_mi355x_trsv_solve_sweeps_multi(None, sweeps, 0, b, x) == 1
            assert lib.spmv_mi355x_last_error().startswith(b"trsv_solve_sweeps: NULL argument ( T )")
        assert lib.spmv_mi355x_trsv_set_sweeps(None, sweeps) == 1
        assert lib.spmv_mi355x_last_error().startswith(b"trsv_set_sweeps: NULL argument ( T )")
    setting, effective, launches, nbytes = ctypes.c_int(-3), ctypes.c_long(-4), ctypes.c_long(-5), ctypes.c_double(-6.0)
    for k in (1, 0):
        assert lib.spmv_mi355x_trsv_sweeps_info(None, k, ctypes.byref(setting), ctypes.byref(effective), ctypes.byref(launches),
                                                ctypes.byref(nbytes)) == 1
        assert lib.spmv_mi355x_last_error().startswith(b"trsv_sweeps_info: NULL argument ( T )")
    assert (setting.value, effective.value, launches.value, nbytes.value) == (-3, -4, -5, -6.0)
    assert np.all(v == 2.5)


def test_what_python_refuses_before_the_call():
    import spmv_mi355x as E

    class Solve:                                        # the solve_sweeps methods read n, dtype and h
        n, dtype, h = 4, np.dtype(np.float64), None

    with pytest.raises(ValueError, match="b must have 4 values"):
        E.TriangularSolve.solve_sweeps(Solve(), np.ones(3), 2)
    for bad in (np.ones(4), np.ones((3, 2)), np.ones((4, 0))):
        with pytest.raises(ValueError, match=r"B must have shape \(4, k\)"):
            E.TriangularSolve.solve_sweeps_multi(Solve(), bad, 2)
    with pytest.raises(E.SpmvError, match=r"trsv_solve_sweeps: NULL argument \( T \)"):
        E.TriangularSolve.solve_sweeps(Solve(), np.ones(4), 2)
    with pytest.raises(E.SpmvError, match=r"trsv_set_sweeps: NULL argument \( T \)"):
        E.TriangularSolve.set_sweeps(Solve(), 2)


@pytest.mark.gpu
def test_the_refusals_behind_the_handle_in_their_order():
    """2. sweeps out of range; then solve_multi's: 3. k < 1; 4. ldb < k or ldx < k; 5. b == x with ldb != ldx; 6. a NULL vector: each
    with every LATER error in the same call. The pointers are host addresses: a refused call touches no device, dereferences nothing
    and allocates nothing (sweeps_info stays at 0 bytes)."""
    import spmv_mi355x as E
    lib = E.lib()
    rp, ci, va, n = tc.matrix("dag", LOWER)
    v, w = np.full((4, 4), 2.5), np.full((4, 4), -1.5)
    top = sc.SWEEPS_MAX
    for T in (E.TriangularSolve(rp, ci, va, n), E.TriangularSolve(rp, ci, va, n, block_rows=100)):
        call = lambda s, k, b, ldb, x, ldx: lib.spmv_mi355x_trsv_solve_sweeps_multi_device_async(T.h, s, k, b, ldb, x, ldx, None)
        ordered = [
            ((0, 0, None, 0, None, 1), b"sweeps = 0: must be in 1 .. 1048576"),          # behind it: k, in place, NULL
            ((-3, 3, P(v), 2, P(v), 3), b"sweeps = -3"),
            ((top + 1, 3, None, 3, None, 3), b"sweeps = 1048577"),
            ((2, 0, None, 0, None, 1), b"k = 0"),
            ((top, -2, P(v), 1, P(v), 2), b"k = -2"),
            ((2, 3, P(v), 2, P(v), 3), b"ldb = 2, ldx = 3"),
            ((2, 3, None, 3, None, 2), b"ldb = 3, ldx = 2"),
            ((2, 3, P(v), 3, P(v), 4), b"b == x (in place) needs ldb == ldx (got 3 and 4)"),
            ((2, 3, None, 3, None, 4), b"b == x (in place) needs ldb == ldx"),
            ((2, 3, None, 3, P(w), 3), b"NULL argument ( b )"),
            ((2, 3, P(v), 3, None, 3), b"NULL argument ( x )"),
            ((1, 3, None, 3, None, 3), b"NULL argument ( b x )"),
        ]
        for args, phrase in ordered:
            assert call(*args) == 1, args
            msg = lib.spmv_mi355x_last_error()
            assert msg.startswith(b"trsv_solve_sweeps: ") and phrase in msg, (args, msg)
        for s, b, x, phrase in ((0, None, None, b"sweeps = 0"), (top + 1, P(v), P(w), b"sweeps = 1048577"), (2, None, P(w), b"NULL argument ( b )"),
                                (2, P(v), None, b"NULL argument ( x )")):
            for rc in (lib.spmv_mi355x_trsv_solve_sweeps_device_async(T.h, s, b, x, None), lib.spmv_mi355x_trsv_solve_sweeps(T.h, s, b, x),
                       lib.spmv_mi355x_trsv_solve_sweeps_multi(T.h, s, 2, b, x)):
                msg = lib.spmv_mi355x_last_error()
                assert rc == 1 and msg.startswith(b"trsv_solve_sweeps: ") and phrase in msg, (s, msg)
        assert lib.spmv_mi355x_trsv_solve_sweeps_multi(T.h, 2, 0, P(v), P(w)) == 1
        assert b"trsv_solve_sweeps: k = 0" in lib.spmv_mi355x_last_error()
        for s in (-1, top + 1):
            with pytest.raises(E.SpmvError, match=rf"trsv_set_sweeps: sweeps = {s}: must be in 0 \.\. 1048576"):
                T.set_sweeps(s)
        with pytest.raises(E.SpmvError, match="trsv_sweeps_info: k = 0"):
            T.sweeps_info(0)
        assert T.sweeps == 0 and T.sweeps_info()["bytes"] == 0
        T.close()
    assert np.all(v == 2.5) and np.all(w == -1.5)


@pytest.mark.gpu
def test_sweeps_info_before_any_solve():
    """the setting, min(setting, levels), effective * chunks, and no byte allocated: host only"""
    import spmv_mi355x as E
    for name, B in (("dag", None), ("dag", 100), ("prescribed", None), ("empty", None), ("empty", 64)):
        rp, ci, va, n = tc.matrix(name, UPPER)
        levels = sc.depth(name, UPPER, B)
        T = E.TriangularSolve(rp, ci, va, n, uplo="upper", block_rows=B)
        info, footprint = T.info, T.mem_footprint
        assert info["levels"] == levels
        assert T.sweeps_info() == dict(sweeps=0, effective=0, launches=0, bytes=0.0)
        for s in (1, 4, levels, levels + 5, sc.SWEEPS_MAX):
            if s < 1:
                continue
            T.set_sweeps(s)
            e = min(s, levels)
            assert T.sweeps == s
            for k, chunks in ((1, 1), (3, 2), (8, 1), (11, 3), (17, 3)):
                assert T.sweeps_info(k) == dict(sweeps=s, effective=e, launches=e * chunks, bytes=0.0), (name, B, s, k)
            assert T.info == info and E.lib().spmv_mi355x_trsv_mem_footprint(T.h) == footprint
        T.set_sweeps(0)
        assert T.sweeps_info(5) == dict(sweeps=0, effective=0, launches=0, bytes=0.0)
        T.close()
        T = E.TriangularSolve(rp, ci, va, n, uplo="upper", block_rows=B, sweeps=3)
        assert T.sweeps == 3 and T.sweeps_info()["effective"] == min(3, levels)
        T.close()
