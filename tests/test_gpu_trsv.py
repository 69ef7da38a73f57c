"""spmv_mi355x_trsv_* / TriangularSolve (include/spmv_mi355x.h "sparse triangular solve") on the GPU: every comparison is np.array_equal
against the sequential C loop of tests/trsv_reference.c. The solve is pinned to the bit, so no tolerance appears in this file.

How a wrong schedule is caught: before every out-of-place solve x is filled with NaN, so a row that reads a dependency before it was
written cannot come out equal; x and b sit between guard values that must survive. The matrices (trsv_cases.py) are the smallest at
which each path can still go wrong:
  bidiagonal 4097      4097 levels of one row: one chain launch that crosses the 64- and 1024-row marks
  prescribed, 64       level widths 1,1,1,2000,1,70,64,65,3,3000,1,1 at chain_rows = 64: chain -> level -> chain -> level ..., 64 and 65 on
                       either side of the threshold, 3000 rows over several workgroups with a partial last slice
  dag, 1 / 64 / 65536  a random DAG (levels not monotone in the row, duplicate entries) under an all-level, a mixed and an all-chain plan
  stencil 24^3         the triangle of a 7-point stencil: 70 levels of up to 432 rows under the default threshold and at chain_rows = 64
  padding              one row of 700 entries among one-entry rows of its level, in the chain kernel (1024) and in the level kernel (64)
  diagonal 1500        one level and no dependency: the level kernel over several workgroups
  one, empty           n = 1 and n = 0
each as LOWER and mirrored UPPER, STORED and UNIT, fp64 and fp32. References are computed once per (matrix, side, mode, precision)
and shared by the plans, which must therefore agree with each other too."""
import ctypes
import functools

import numpy as np
import pytest

import trsv_cases as tc
from trsv_cases import LOWER, UPPER

pytestmark = pytest.mark.gpu

GUARD = 4                 # elements on either side of a device vector
SENTINEL = 777.0
PLANS = [("bidiagonal", 0), ("prescribed", 64), ("dag", 1), ("dag", 64), ("dag", 65536), ("stencil", 0), ("stencil", 64), ("padding", 1024),
         ("padding", 64), ("diagonal", 0), ("one", 0), ("empty", 0)]
SIDES = ((LOWER, "lower"), (UPPER, "upper"))
DTYPES = (np.float64, np.float32)


@pytest.fixture(scope="module")
def eng():
    import spmv_mi355x as eng
    assert eng.device_count() >= 1, "no GPU visible: the -m gpu tests need an MI355X"
    return eng


def rhs(n, seed=11):
    return np.random.default_rng(seed).uniform(-1, 1, n)


@functools.lru_cache(maxsize=None)
def expected(name, uplo, unit, dtype, variant="", seed=11):
    """(matrix, b, reference x), read-only. variant: "" | "zero" (stored zero diagonal) | "none" (no diagonal stored) | "full" (the
    stencil with both triangles; the reference runs on the extracted triangle)"""
    A = tc.stencil_full() if variant == "full" else tc.matrix(name, uplo)
    if variant == "zero":
        A = tc.with_zero_diagonal(*A)
    if variant == "none":
        A = tc.without_diagonal(*A)
    R = tc.triangle(*A, uplo) if variant == "full" else A
    b = rhs(A[3], seed).astype(dtype)
    x = tc.reference(*R, uplo, unit, b, dtype)
    assert np.all(np.isfinite(x)), "the reference overflowed: two non-finite results must not pass as equal"
    for a in (b, x):
        a.setflags(write=False)
    return A, b, x


def device_solve(T, b, dtype, in_place=False, shift=0):
    """x of T.solve_device with b and x inside guarded device buffers, `shift` elements past the guard; x pre-filled with NaN"""
    import torch
    dt = torch.float64 if np.dtype(dtype) == np.float64 else torch.float32
    n, lo = len(b), GUARD + shift
    size = np.dtype(dtype).itemsize
    bb = torch.full((n + 2 * GUARD + shift,), SENTINEL, dtype=dt, device="cuda")
    bb[lo:lo + n] = torch.from_numpy(np.array(b)).cuda()
    if in_place:
        xb = bb
    else:
        xb = torch.full((n + 2 * GUARD + shift,), SENTINEL, dtype=dt, device="cuda")
        xb[lo:lo + n] = float("nan")
    T.solve_device(bb.data_ptr() + lo * size, xb.data_ptr() + lo * size)
    torch.cuda.synchronize()
    got = xb.cpu().numpy()
    assert np.all(got[:lo] == SENTINEL) and np.all(got[lo + n:] == SENTINEL), "a guard value around x was overwritten"
    if not in_place:
        kept = bb.cpu().numpy()
        assert np.array_equal(kept[lo:lo + n], b) and np.all(kept[:lo] == SENTINEL) and np.all(kept[lo + n:] == SENTINEL), "b was modified"
    return got[lo:lo + n]


def handle(eng, A, side, unit, dtype, chain_rows=0):
    return eng.TriangularSolve(*A, uplo=side, diag="unit" if unit else "stored", dtype=dtype, chain_rows=chain_rows)


@pytest.mark.parametrize("dtype", DTYPES, ids=("f64", "f32"))
@pytest.mark.parametrize("unit", (False, True), ids=("stored", "unit"))
@pytest.mark.parametrize("uplo,side", SIDES, ids=("lower", "upper"))
@pytest.mark.parametrize("name,chain_rows", PLANS, ids=[f"{a}-{c}" for a, c in PLANS])
def test_every_plan_gives_the_bits_of_the_sequential_loop(eng, name, chain_rows, uplo, side, unit, dtype):
    A, b, want = expected(name, uplo, unit, dtype)
    T = handle(eng, A, side, unit, dtype, chain_rows)
    got = device_solve(T, b, dtype)
    info = T.info
    T.close()
    assert np.array_equal(got, want), f"{int(np.sum(got != want))} of {len(want)} rows differ; plan {info}"
    # the plan that ran is the one the case is about
    level = tc.levels_of(A[0], A[1], A[3], uplo)
    assert (info["levels"], info["launches"], info["max_level_rows"]) == tc.plan_of(level, info["chain_rows"])


@pytest.mark.parametrize("dtype", DTYPES, ids=("f64", "f32"))
@pytest.mark.parametrize("uplo,side", SIDES, ids=("lower", "upper"))
@pytest.mark.parametrize("variant", ("zero", "none"))
def test_unit_ignores_a_stored_zero_and_a_missing_diagonal(eng, variant, uplo, side, dtype):
    A, b, want = expected("dag", uplo, True, dtype, variant)
    assert np.array_equal(want, expected("dag", uplo, True, dtype)[2])          # the reference ignores the diagonal too
    T = handle(eng, A, side, True, dtype, 64)
    got = device_solve(T, b, dtype)
    T.close()
    assert np.array_equal(got, want)


@pytest.mark.parametrize("dtype", DTYPES, ids=("f64", "f32"))
@pytest.mark.parametrize("unit", (False, True), ids=("stored", "unit"))
@pytest.mark.parametrize("uplo,side", SIDES, ids=("lower", "upper"))
def test_a_full_matrix_serves_both_triangles(eng, uplo, side, unit, dtype):
    A, b, want = expected("stencil", uplo, unit, dtype, "full")
    assert np.array_equal(want, expected("stencil", uplo, unit, dtype)[2])
    T = handle(eng, A, side, unit, dtype, 64)
    got = device_solve(T, b, dtype)
    kept = T.info["nnz_kept"]
    T.close()
    assert np.array_equal(got, want)
    tri = tc.triangle(*A, uplo)
    assert kept == len(tri[1]) - (A[3] if unit else 0)          # the triangle's entries; under UNIT without its diagonal


@pytest.mark.parametrize("dtype", DTYPES, ids=("f64", "f32"))
@pytest.mark.parametrize("uplo,side", SIDES, ids=("lower", "upper"))
@pytest.mark.parametrize("name,chain_rows", [("prescribed", 64), ("dag", 65536), ("dag", 1)], ids=("mixed", "chain", "levels"))
def test_in_place_and_at_an_odd_offset(eng, name, chain_rows, uplo, side, dtype):
    A, b, want = expected(name, uplo, False, dtype)
    T = handle(eng, A, side, False, dtype, chain_rows)
    assert np.array_equal(device_solve(T, b, dtype, in_place=True), want), "b is x"
    assert np.array_equal(device_solve(T, b, dtype, shift=1), want), "vectors at an odd element offset"
    assert np.array_equal(device_solve(T, b, dtype, in_place=True, shift=3), want), "b is x at an odd element offset"
    T.close()


@pytest.mark.parametrize("dtype", DTYPES, ids=("f64", "f32"))
@pytest.mark.parametrize("uplo,side", SIDES, ids=("lower", "upper"))
def test_one_handle_serves_several_solves_and_the_host_form_equals_the_device_form(eng, uplo, side, dtype):
    A, b1, want1 = expected("prescribed", uplo, False, dtype)
    _, b2, want2 = expected("prescribed", uplo, False, dtype, "", 12)
    assert not np.array_equal(want1, want2)
    T = handle(eng, A, side, False, dtype, 64)
    assert np.array_equal(device_solve(T, b1, dtype), want1)
    assert np.array_equal(device_solve(T, b2, dtype), want2)
    assert np.array_equal(T.solve(b2), want2) and np.array_equal(T.solve(b1), want1), "solve() with host buffers"
    x = np.array(b1)                                           # the host form in place
    p = x.ctypes.data_as(ctypes.c_void_p)
    assert eng.lib().spmv_mi355x_trsv_solve(T.h, p, p) == 0
    assert np.array_equal(x, want1)
    T.close()


@pytest.mark.parametrize("uplo,side", SIDES, ids=("lower", "upper"))
@pytest.mark.parametrize("name,chain_rows", PLANS, ids=[f"{a}-{c}" for a, c in PLANS])
def test_info_equals_analyze(eng, name, chain_rows, uplo, side):
    A = tc.matrix(name, uplo)
    rp, ci, va, n = A
    T = handle(eng, A, side, False, np.float64, chain_rows)
    info, footprint = T.info, T.mem_footprint
    T.close()
    an = eng.trsv_analyze(rp, ci, n, side, chain_rows)
    assert {k: info[k] for k in ("levels", "launches", "max_level_rows", "chain_rows")} == \
        {k: an[k] for k in ("levels", "launches", "max_level_rows", "chain_rows")}
    assert info["n"] == n and info["nnz_kept"] == len(ci)                      # the case matrices hold one triangle and its diagonal
    # at least the kept entries (12 bytes each off the diagonal, 8 on it) and the permutation; padding and the plan's arrays on top
    assert footprint >= 12 * (len(ci) - n) + 8 * n + 4 * n


def test_n_zero_solves_nothing(eng):
    import torch
    T = eng.TriangularSolve(np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros(0), 0)
    assert T.info == dict(n=0, nnz_kept=0, levels=0, launches=0, max_level_rows=0, chain_rows=T.info["chain_rows"])
    x = torch.full((8,), SENTINEL, dtype=torch.float64, device="cuda")
    T.solve_device(x.data_ptr(), x.data_ptr())
    T.solve_device(0, 0)                                       # no vector is needed for no rows
    torch.cuda.synchronize()
    assert bool(torch.all(x == SENTINEL))
    assert T.solve(np.zeros(0)).shape == (0,)
    T.close()
