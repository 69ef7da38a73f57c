"""Matrix.pcg_trsm_multi / spmv_mi355x_pcg_trsm_multi on the GPU (include/spmv_mi355x.h "pcg_trsm_multi"): k right-hand sides through
one tol-based CG whose preconditioner has triangular parts, SGS of A or the caller's IC(0), applied by the k-column triangular solve.

The contract is exact: on a handle whose SpMV is deterministic (asserted first in every test), column j returns the bits of
Matrix.pcg_tri on column j with the same preconditioner handles: every field of INFO_FIELDS, x and the history, compared as bytes.
No tolerance appears in this file. The single solves are held to the dense solve and to the restatement by test_gpu_pcg_tri.py; the
iteration counts of pcg_tri_cases.COUNTS are asserted for the first column as a cross-check that both sides ran the real thing.

The problem is pcg_tri_cases.problem() (n = 2025) and the blocks are those of pcg_tri_multi_cases.py. k in (1, 3, 4, 9) gives the
chunks 1 / 2+1 / 4 / 8+1 of the vector kernels and of a global triangular solve; a blocked handle of 64 or 256 rows keeps 8 columns
of its block in LDS."""
import ctypes

import numpy as np
import pytest

import pcg_tri_cases as pc
import pcg_tri_multi_cases as mc
from pcg_tri_cases import MAX_ITERATIONS, MIXED_B, POLL, PREC

pytestmark = pytest.mark.gpu

LAYOUTS = ("sell_c_sigma", "csr_vector")
INFO_FIELDS = ("iterations", "stop", "rnorm", "rnorm0", "prnorm", "xnorm")
DTYPES = [np.float64, np.float32]
KINDS = (64, 256, "sgs", "ic0", "mixed")
KS = (1, 3, 4, 9)


@pytest.fixture(scope="module")
def eng():
    import spmv_mi355x as eng
    assert eng.device_count() >= 1, "no GPU visible: the -m gpu tests need an MI355X"
    assert hasattr(eng.lib(), "spmv_mi355x_pcg_trsm_multi")
    return eng


def handle(eng, fmt, dtype):
    P = pc.problem()
    rp, ci, va = P.csr
    return eng.Matrix(rp, ci, va, P.n, P.n, fmt, dtype)


def precond(eng, kind, dtype):
    """(first, scale, second): blocked SGS of 64 or 256 rows, the global SGS, the IC(0) factors of pcg_tri_cases, or "mixed": a
    blocked first part (of MIXED_B >= n rows, so M stays symmetric), the scale, a global second part"""
    P = pc.problem()
    rp, ci, va = P.csr
    T = eng.TriangularSolve
    if kind == "ic0":
        _, lo, up = P.ic0()
        return T(*lo, P.n, uplo="lower", dtype=dtype), None, T(*up, P.n, uplo="upper", dtype=dtype)
    if kind == "mixed":
        return (T(rp, ci, va, P.n, uplo="lower", dtype=dtype, block_rows=MIXED_B), P.diag.astype(dtype),
                T(rp, ci, va, P.n, uplo="upper", dtype=dtype))
    return eng.sgs_precond(rp, ci, va, P.n, dtype=dtype, block_rows=None if kind == "sgs" else kind)


def close(M):
    for h in M or ():
        if h is not None and not isinstance(h, np.ndarray):
            h.close()


def deterministic(A):
    x = np.random.default_rng(5).uniform(-1, 1, A.n)
    return np.array_equal(A.spmv(x), A.spmv(x))


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True) and a.tobytes() == b.tobytes()


def assert_same_solve(got, want, what):
    for f in INFO_FIELDS:                                    # a NaN (the norms of a column with a NaN in b) equals a NaN
        assert got[f] == want[f] or (got[f] != got[f] and want[f] != want[f]), f"{what}: {f}: {got[f]!r} and {want[f]!r}"
    assert same_bits(got["x"], want["x"]), f"{what}: x"
    assert same_bits(got["history"], want["history"]), f"{what}: history"


# ---- 1. column against single ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("fmt", LAYOUTS)
@pytest.mark.parametrize("kind", KINDS, ids=str)
def test_the_solve_of_a_block_is_the_solve_of_each_column(eng, kind, fmt, dtype):
    A = handle(eng, fmt, dtype)
    assert deterministic(A)
    M = precond(eng, kind, dtype)
    if kind == "mixed":
        assert M[0].block_info()["block_rows"] == MIXED_B and M[0].block_info()["nnz_dropped"] == 0 and M[2].block_info()["block_rows"] == 0
    tol = PREC[dtype]["tol"]
    B = mc.solve_block().astype(dtype)
    what = f"{kind} {fmt} {np.dtype(dtype).name}"
    want = [A.pcg_tri(np.ascontiguousarray(B[:, j]), M, tol, MAX_ITERATIONS) for j in range(max(KS))]
    count = pc.COUNTS[dtype]["sgs" if kind == "mixed" else kind]
    print(f"[pcg_trsm_multi] {what}: single iterations {[w['iterations'] for w in want]}, the table has {count}")
    assert all(w["stop"] == 1 for w in want)
    assert want[0]["iterations"] == count, f"{what}: the single solve of b"
    for k in KS:
        got = A.pcg_trsm_multi(np.ascontiguousarray(B[:, :k]), M, tol, MAX_ITERATIONS)
        assert len(got) == k
        for j in range(k):
            assert_same_solve(got[j], want[j], f"{what}: column {j} of k = {k}")
        assert len({g["spmv_calls"] for g in got}) == 1 and len({g["seconds"] for g in got}) == 1
        latest = max(w["iterations"] for w in want[:k])
        assert latest <= got[0]["spmv_calls"] <= latest + 3 * POLL + 1, f"{what}: k = {k}: {got[0]['spmv_calls']} SpMMs, latest {latest}"
    assert got[0]["iterations"] == count
    close(M)
    A.close()


def test_partial_preconditioners(eng):
    """a first part alone, and a scale with a second part: every mix of parts is served"""
    P = pc.problem()
    A = handle(eng, "sell_c_sigma", np.float64)
    assert deterministic(A)
    sgs = precond(eng, 64, np.float64)
    B = np.ascontiguousarray(mc.solve_block()[:, :3])
    for M in ((sgs[0], None, None), (None, sgs[1], sgs[2]), (None, None, sgs[2])):
        # not symmetric, so CG may break down: whatever the single solve does, the column does; the cap keeps it short
        want = [A.pcg_tri(np.ascontiguousarray(B[:, j]), M, 1e-12, 20) for j in range(3)]
        got = A.pcg_trsm_multi(B, M, 1e-12, 20)
        for j in range(3):
            assert_same_solve(got[j], want[j], f"parts {[m is not None for m in M]}: column {j}")
    close(sgs)
    A.close()


# ---- 2. the freeze per column ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", (64, "sgs"), ids=str)
def test_a_stopped_column_is_frozen_while_its_neighbours_run(eng, kind):
    A = handle(eng, "sell_c_sigma", np.float64)
    assert deterministic(A)
    M = precond(eng, kind, np.float64)
    B = mc.freeze_columns()
    want = [A.pcg_tri(np.ascontiguousarray(B[:, j]), M, 1e-12, MAX_ITERATIONS) for j in range(5)]
    got = A.pcg_trsm_multi(B, M, 1e-12, MAX_ITERATIONS)
    print(f"[pcg_trsm_multi] freeze, {kind}: iterations {[g['iterations'] for g in got]}, stops {[g['stop'] for g in got]}, "
          f"{got[0]['spmv_calls']} SpMMs")
    assert tuple(g["stop"] for g in got) == mc.FREEZE_STOPS
    assert got[0]["iterations"] == pc.COUNTS[np.float64][kind]
    assert len({got[j]["iterations"] for j in (0, 1, 4)}) > 1, "the running columns stop at different iterations"
    for j in range(5):
        assert_same_solve(got[j], want[j], f"freeze, {kind}: column {j}")
    for j in (2, 3):
        assert got[j]["iterations"] == 0 and not got[j]["x"].any() and got[j]["history"].size == 0
    assert got[2]["rnorm0"] == 0 and got[2]["rnorm"] == 0
    close(M)
    A.close()


# ---- 3. without a triangular part: the bytes of pcg_tri_multi ---------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("kind", ("none", "jacobi"))
def test_without_a_triangular_part_it_is_pcg_tri_multi(eng, kind, dtype):
    P = pc.problem()
    A = handle(eng, "sell_c_sigma", dtype)
    assert deterministic(A)
    M = None if kind == "none" else (None, (1.0 / P.diag).astype(dtype), None)
    B = mc.solve_block().astype(dtype)
    tol = PREC[dtype]["tol"]
    want = A.pcg_tri_multi(B, M, tol, MAX_ITERATIONS)
    got = A.pcg_trsm_multi(B, M, tol, MAX_ITERATIONS)
    assert want[0]["iterations"] == pc.COUNTS[dtype][kind]
    for j in range(B.shape[1]):
        assert_same_solve(got[j], want[j], f"{kind} {np.dtype(dtype).name}: column {j}")
    assert got[0]["spmv_calls"] == want[0]["spmv_calls"]
    A.close()


# ---- 4. max_iterations -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", (256, "ic0"), ids=str)
def test_the_cap_stops_every_column_with_2(eng, kind):
    A = handle(eng, "sell_c_sigma", np.float64)
    assert deterministic(A)
    M = precond(eng, kind, np.float64)
    B = np.ascontiguousarray(mc.solve_block()[:, :3])
    want = [A.pcg_tri(np.ascontiguousarray(B[:, j]), M, 1e-12, 7) for j in range(3)]
    got = A.pcg_trsm_multi(B, M, 1e-12, 7)
    for j in range(3):
        assert got[j]["stop"] == 2 and got[j]["iterations"] == 7 and got[j]["history"].shape == (7,)
        assert_same_solve(got[j], want[j], f"cap 7: column {j}")
    want = [A.pcg_tri(np.ascontiguousarray(B[:, j]), M, 1e-12, 0) for j in range(3)]
    got = A.pcg_trsm_multi(B, M, 1e-12, 0)
    for j in range(3):
        assert got[j]["stop"] == 2 and got[j]["iterations"] == 0 and not got[j]["x"].any() and got[j]["history"].size == 0
        assert got[j]["rnorm"] == got[j]["rnorm0"]
        assert_same_solve(got[j], want[j], f"cap 0: column {j}")
    close(M)
    A.close()


# ---- 5. repeatability and the refusals that need a handle --------------------------------------------------------------------------------

def test_twice_the_same_bits(eng):
    A = handle(eng, "sell_c_sigma", np.float32)
    assert deterministic(A)
    M = precond(eng, 64, np.float32)
    B = mc.solve_block().astype(np.float32)
    a = A.pcg_trsm_multi(B, M, 1e-5, MAX_ITERATIONS)
    b = A.pcg_trsm_multi(B, M, 1e-5, MAX_ITERATIONS)
    for j in range(B.shape[1]):
        assert_same_solve(a[j], b[j], f"column {j}")
    close(M)
    A.close()


def test_the_parts_of_m_are_checked_as_pcg_tri_checks_them(eng):
    P = pc.problem()
    rp, ci, va = P.csr
    A = handle(eng, "sell_c_sigma", np.float64)
    sgs = precond(eng, 64, np.float64)
    B = np.ascontiguousarray(mc.solve_block()[:, :2])
    X = np.full((P.n, 2), -7.25)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    small = eng.TriPrecond(4, sgs[0].h, None, sgs[2].h)
    assert eng.lib().spmv_mi355x_pcg_trsm_multi(A.h, 2, p(B), p(X), ctypes.byref(small), 1e-12, 10, None, None) == 1
    assert eng.lib().spmv_mi355x_last_error().startswith(b"pcg_trsm_multi: M->struct_size = 4 is smaller")
    f32 = eng.TriangularSolve(rp, ci, va, P.n, uplo="upper", dtype=np.float32, block_rows=64)
    with pytest.raises(eng.SpmvError, match="pcg_trsm_multi: M->second has precision 1, the matrix 0"):
        A.pcg_trsm_multi(B, (sgs[0], sgs[1], f32))
    bad = np.array(sgs[1])
    bad[5] = 0.0
    with pytest.raises(eng.SpmvError, match=r"pcg_trsm_multi: scale\[5\] = 0"):
        A.pcg_trsm_multi(B, (sgs[0], bad, sgs[2]))
    assert np.all(X == -7.25)
    f32.close()
    close(sgs)
    A.close()
