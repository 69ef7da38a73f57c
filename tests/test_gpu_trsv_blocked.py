"""spmv_mi355x_trsv_create_blocked / TriangularSolve(block_rows=...) on the GPU: every comparison is np.array_equal against the
sequential C loop of tests/trsv_reference.c on the CSR with the dropped entries removed (trsv_blocked_cases.filtered). The solve is
pinned to the bit, so no tolerance appears in this file.

As in test_gpu_trsv.py x is filled with NaN before every out-of-place solve, so a row that reads a dependency before it was written
cannot come out equal, and x and b sit between guard values that must survive. The matrices are those of trsv_cases.py and one
20000-row DAG; with B in {1, 64, 100, 1024, 16384} they are the smallest at which the one kernel can still go wrong:
  a last block that is short                 every matrix whose n is no multiple of B; bidiagonal 4097 at B = 64 ends in a block of one row
  a block of one row                         B = 1, and `one`
  a level wider than the workgroup           prescribed at B = 16384: levels of 2000 and 3000 rows in a workgroup of 1024 threads
  a level narrower than a wave               bidiagonal: levels of one row; dag: mostly a few rows
  blocks with different level counts         dag at B = 100 and 1024: every block has its own depth, in one launch
  more workgroups than can be resident       bidiagonal at B = 1: 4097 workgroups
  LDS above 64 KiB                           big_dag (n = 20000) at B = 16384: 128 KiB in fp64, a full block followed by a short one
each as LOWER and mirrored UPPER, STORED and UNIT, fp64 and fp32. References are computed once per (matrix, B, side, mode, precision)."""
import ctypes
import functools

import numpy as np
import pytest

import trsv_blocked_cases as bc
import trsv_cases as tc
from trsv_cases import LOWER, UPPER

pytestmark = pytest.mark.gpu

GUARD = 4                 # elements on either side of a device vector
SENTINEL = 777.0
BLOCK_ROWS = (1, 64, 100, 1024, 16384)
NAMES = ("bidiagonal", "prescribed", "dag", "stencil", "padding", "diagonal", "one", "empty")
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
def expected(name, B, uplo, unit, dtype, seed=11):
    """(matrix, b, reference x of the filtered matrix), read-only"""
    A = bc.matrix(name, uplo)
    b = rhs(A[3], seed).astype(dtype)
    x = tc.reference(*bc.filtered(*A, B), uplo, unit, b, dtype)
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


def handle(eng, A, side, unit, dtype, B):
    return eng.TriangularSolve(*A, uplo=side, diag="unit" if unit else "stored", dtype=dtype, block_rows=B)


@pytest.mark.parametrize("dtype", DTYPES, ids=("f64", "f32"))
@pytest.mark.parametrize("unit", (False, True), ids=("stored", "unit"))
@pytest.mark.parametrize("uplo,side", SIDES, ids=("lower", "upper"))
@pytest.mark.parametrize("name", NAMES)
def test_every_block_size_gives_the_bits_of_the_sequential_loop_on_the_filtered_matrix(eng, name, uplo, side, unit, dtype):
    for B in BLOCK_ROWS:
        A, b, want = expected(name, B, uplo, unit, dtype)
        T = handle(eng, A, side, unit, dtype, B)
        got = device_solve(T, b, dtype)
        T.close()
        assert np.array_equal(got, want), f"B = {B}: {int(np.sum(got != want))} of {len(want)} rows differ"


@pytest.mark.parametrize("dtype", DTYPES, ids=("f64", "f32"))
@pytest.mark.parametrize("unit", (False, True), ids=("stored", "unit"))
@pytest.mark.parametrize("uplo,side", SIDES, ids=("lower", "upper"))
def test_a_block_of_128_kib_of_lds_followed_by_a_short_one(eng, uplo, side, unit, dtype):
    A, b, want = expected("big_dag", 16384, uplo, unit, dtype)
    T = handle(eng, A, side, unit, dtype, 16384)
    got = device_solve(T, b, dtype)
    info = T.block_info()
    T.close()
    assert (info["block_rows"], info["blocks"]) == (16384, 2)
    assert info["nnz_dropped"] == bc.dropped_of(A[0], A[1], A[3], uplo, 16384) > 0
    assert np.array_equal(got, want), f"{int(np.sum(got != want))} of {len(want)} rows differ"


@pytest.mark.parametrize("dtype", DTYPES, ids=("f64", "f32"))
@pytest.mark.parametrize("uplo,side", SIDES, ids=("lower", "upper"))
@pytest.mark.parametrize("name", ("prescribed", "dag", "stencil", "padding", "one"))
def test_one_block_gives_the_bits_of_the_global_handle(eng, name, uplo, side, dtype):
    """B >= n: nothing is dropped"""
    A = tc.matrix(name, uplo)
    b = rhs(A[3]).astype(dtype)
    G = eng.TriangularSolve(*A, uplo=side, dtype=dtype)
    T = handle(eng, A, side, False, dtype, 16384)
    assert T.block_info() == dict(block_rows=16384, blocks=1, max_block_levels=G.info["levels"], nnz_dropped=0)
    assert G.block_info() == dict(block_rows=0, blocks=0, max_block_levels=0, nnz_dropped=0)
    assert T.info["nnz_kept"] == G.info["nnz_kept"]
    want = device_solve(G, b, dtype)
    got = device_solve(T, b, dtype)
    G.close()
    T.close()
    assert np.array_equal(got, want) and np.array_equal(got, tc.reference(*A, uplo, False, b, dtype))


def test_the_blocked_result_differs_from_the_unblocked_one(eng):
    """what shows that the comparisons above can tell the two apart: on bidiagonal at B = 64 row 64 loses its one dependency"""
    A, b, want = expected("bidiagonal", 64, LOWER, False, np.float64)
    whole = tc.reference(*A, LOWER, False, b, np.float64)
    assert np.array_equal(want[:64], whole[:64]) and np.any(want[64:] != whole[64:])
    T = handle(eng, A, "lower", False, np.float64, 64)
    got = device_solve(T, b, np.float64)
    T.close()
    assert np.array_equal(got, want) and np.any(got[64:] != whole[64:])


@pytest.mark.parametrize("dtype", DTYPES, ids=("f64", "f32"))
@pytest.mark.parametrize("uplo,side", SIDES, ids=("lower", "upper"))
@pytest.mark.parametrize("name,B", [("prescribed", 16384), ("dag", 100), ("bidiagonal", 1)], ids=("wide", "many", "rows"))
def test_in_place_and_at_an_odd_offset(eng, name, B, uplo, side, dtype):
    A, b, want = expected(name, B, uplo, False, dtype)
    T = handle(eng, A, side, False, dtype, B)
    assert np.array_equal(device_solve(T, b, dtype, in_place=True), want), "b is x"
    assert np.array_equal(device_solve(T, b, dtype, shift=1), want), "vectors at an odd element offset"
    assert np.array_equal(device_solve(T, b, dtype, in_place=True, shift=3), want), "b is x at an odd element offset"
    T.close()


@pytest.mark.parametrize("dtype", DTYPES, ids=("f64", "f32"))
@pytest.mark.parametrize("uplo,side", SIDES, ids=("lower", "upper"))
def test_one_handle_serves_several_solves_and_the_host_form_equals_the_device_form(eng, uplo, side, dtype):
    A, b1, want1 = expected("dag", 100, uplo, False, dtype)
    _, b2, want2 = expected("dag", 100, uplo, False, dtype, 12)
    assert not np.array_equal(want1, want2)
    T = handle(eng, A, side, False, dtype, 100)
    assert np.array_equal(device_solve(T, b1, dtype), want1)
    assert np.array_equal(device_solve(T, b2, dtype), want2)
    assert np.array_equal(T.solve(b2), want2) and np.array_equal(T.solve(b1), want1), "solve() with host buffers"
    x = np.array(b1)                                           # the host form in place
    p = x.ctypes.data_as(ctypes.c_void_p)
    assert eng.lib().spmv_mi355x_trsv_solve(T.h, p, p) == 0
    assert np.array_equal(x, want1)
    T.close()


@pytest.mark.parametrize("uplo,side", SIDES, ids=("lower", "upper"))
@pytest.mark.parametrize("name", NAMES)
def test_info_and_block_info_equal_the_analysis(eng, name, uplo, side):
    A = tc.matrix(name, uplo)
    rp, ci, va, n = A
    for B in BLOCK_ROWS + (0,):
        T = handle(eng, A, side, False, np.float64, B)
        info, blk, footprint = T.info, T.block_info(), T.mem_footprint
        T.close()
        an = eng.trsv_analyze_blocked(rp, ci, n, side, B)
        assert blk == {k: an[k] for k in ("block_rows", "blocks", "max_block_levels", "nnz_dropped")}
        want = bc.analysis_of(rp, ci, n, uplo, an["block_rows"])
        assert {k: an[k] for k in ("blocks", "max_block_levels", "max_level_rows", "nnz_dropped")} == \
            {k: want[k] for k in ("blocks", "max_block_levels", "max_level_rows", "nnz_dropped")}
        # the case matrices hold one triangle and its diagonal
        assert info == dict(n=n, nnz_kept=len(ci) - an["nnz_dropped"], levels=an["max_block_levels"], launches=1 if n else 0,
                            max_level_rows=an["max_level_rows"], chain_rows=0)
        # at least the kept entries (12 bytes each off the diagonal, 8 on it) and the permutation
        assert footprint >= 12 * (len(ci) - n - an["nnz_dropped"]) + 8 * n + 4 * n


def test_n_zero_solves_nothing(eng):
    import torch
    T = eng.TriangularSolve(np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros(0), 0, block_rows=64)
    assert T.info == dict(n=0, nnz_kept=0, levels=0, launches=0, max_level_rows=0, chain_rows=0)
    assert T.block_info() == dict(block_rows=64, blocks=0, max_block_levels=0, nnz_dropped=0)
    x = torch.full((8,), SENTINEL, dtype=torch.float64, device="cuda")
    T.solve_device(x.data_ptr(), x.data_ptr())
    T.solve_device(0, 0)                                       # no vector is needed for no rows
    torch.cuda.synchronize()
    assert bool(torch.all(x == SENTINEL))
    assert T.solve(np.zeros(0)).shape == (0,)
    T.close()
