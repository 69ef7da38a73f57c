"""spmv_mi355x_trsv_solve_multi* / TriangularSolve.solve_multi* on the GPU (include/spmv_mi355x.h "K COLUMNS"): T X = B for k columns
of a row-major block over the handles of the single solve, global and blocked.

The contract is exact, so every comparison is np.array_equal plus equality of tobytes() and no tolerance appears in this file. Every
column is held to TWO references: the sequential C loop of tests/trsv_reference.c on that column (trsv_cases.reference; on the CSR
filtered by trsv_blocked_cases.filtered for a blocked handle), which is first asserted to be finite, and the single solve_device of
the SAME handle on that column. X is pre-filled with NaN, so a row that gathers a dependency before it was written cannot come out
equal. B and X sit in guarded buffers: the guards, the ld - k padding columns (a sentinel in X, a NaN with a payload in B) and B
itself must survive, compared as bytes.

The matrices are those of trsv_cases.py and trsv_blocked_cases.py, already the smallest that break the single kernels (levels of 2000
and 3000 rows over several workgroups, 64 / 65-row slice edges, a chain of 4097 levels of one row across the 1024-row mark, a
700-entry row for the unroll tail, 4097 workgroups, a level wider than the workgroup, LDS above 64 KiB). New ground here:
  the column counts       k in (1, 2, 3, 5, 8, 9, 11) = chunks 1 / 2 / 2+1 / 4+1 / 8 / 8+1 / 8+2+1: every KC runs, a column sits behind a
                          full chunk
  the leading dimension   ld = k on a base aligned to 64 bytes (vector rows where the chunk allows), ld = k + 3 with the block one
                          element off alignment (scalar rows), and the columns 3 .. 3 + k of a 16-wide block: ld is a multiple of
                          every KC but no chunk starts at a multiple of its KC
  in place                b == x, ldb == ldx
  the LDS edges           big_dag (n = 20000): fp64 B = 2560 at k = 8 is one pass at exactly 160 KiB, B = 2561 two passes of 4,
                          B = 16384 at k = 2 two passes of 1 in fp64 and one pass of 2 (128 KiB) in fp32
A handle is created once per test and serves every k, ld and placement of that test."""
import functools

import numpy as np
import pytest

import trsv_blocked_cases as bc
import trsv_cases as tc
from trsv_cases import LOWER, UPPER

pytestmark = pytest.mark.gpu

GUARD = 8                 # elements on either side of a block: 64 bytes in fp64, so the block behind it is aligned for every KC
SENTINEL = 777.0
KS = (1, 2, 3, 5, 8, 9, 11)
KMAX = max(KS)
SIDES = ((LOWER, "lower"), (UPPER, "upper"))
DTYPES = (np.float64, np.float32)


@pytest.fixture(scope="module")
def eng():
    import spmv_mi355x as eng
    assert eng.device_count() >= 1, "no GPU visible: the -m gpu tests need an MI355X"
    assert hasattr(eng.lib(), "spmv_mi355x_trsv_solve_multi_device_async")
    return eng


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True) and a.tobytes() == b.tobytes()


def nan_of(dtype, payload):
    """a quiet NaN with `payload` in its low mantissa bits"""
    if np.dtype(dtype) == np.float64:
        return np.array([0x7ff8000000000000 | payload], np.uint64).view(np.float64)[0]
    return np.array([0x7fc00000 | payload], np.uint32).view(np.float32)[0]


@functools.lru_cache(maxsize=None)
def block(n, dtype, seed=11):
    """n x KMAX right-hand sides of differing scale, read-only"""
    rng = np.random.default_rng(seed)
    B = np.ascontiguousarray(np.stack([(10.0 ** (j % 3 - 1)) * rng.uniform(-1, 1, n) for j in range(KMAX)], axis=1).astype(dtype))
    B.setflags(write=False)
    return B


@functools.lru_cache(maxsize=None)
def expected(name, B, uplo, unit, dtype, k=KMAX):
    """(matrix, the n x k block, the reference X column by column); B = None: a global handle, else the filtered matrix"""
    A = bc.matrix(name, uplo)
    rhs = np.ascontiguousarray(block(A[3], dtype)[:, :k])
    M = A if B is None else bc.filtered(*A, B)
    X = np.stack([tc.reference(*M, uplo, unit, np.ascontiguousarray(rhs[:, j]), dtype) for j in range(k)], axis=1) if A[3] else \
        np.zeros((0, k), dtype)
    assert np.all(np.isfinite(X)), "the reference overflowed: two non-finite results must not pass as equal"
    X.setflags(write=False)
    rhs.setflags(write=False)
    return A, rhs, X


def solve_multi(T, Bh, ld=None, shift=0, col0=0, in_place=False):
    """X of T.solve_multi_device for the n x k block Bh placed at the columns col0 .. col0 + k of an ld-wide block that starts
    `shift` elements behind the guard. Checks the guards, the padding columns and B."""
    import torch
    n, k = Bh.shape
    dtype = Bh.dtype
    ld = k if ld is None else ld
    assert ld >= col0 + k
    word = np.uint64 if dtype == np.float64 else np.uint32
    lo = GUARD + shift
    total = lo + n * ld + GUARD
    hb = np.full(total, SENTINEL, dtype)
    hb[lo:lo + n * ld] = nan_of(dtype, 0x51)
    hb[lo:lo + n * ld].reshape(n, ld)[:, col0:col0 + k] = Bh
    hx = np.full(total, SENTINEL, dtype)
    hx[lo:lo + n * ld].reshape(n, ld)[:, col0:col0 + k] = np.nan
    written = np.zeros(total, bool)
    written[lo:lo + n * ld].reshape(n, ld)[:, col0:col0 + k] = True
    tb = torch.from_numpy(hb.copy()).to("cuda")
    tx = tb if in_place else torch.from_numpy(hx.copy()).to("cuda")
    size = tb.element_size()
    off = (lo + col0) * size
    if shift == 0 and col0 == 0:
        assert (tb.data_ptr() + off) % (8 * size) == 0 and (tx.data_ptr() + off) % (8 * size) == 0          # a row of 8 values
    T.solve_multi_device(k, tb.data_ptr() + off, ld, tx.data_ptr() + off, ld)
    torch.cuda.synchronize()
    got = tx.cpu().numpy()
    before = hb if in_place else hx
    assert got[~written].view(word).tobytes() == before[~written].view(word).tobytes(), "a guard or a padding column of X was overwritten"
    if not in_place:
        assert tb.cpu().numpy().view(word).tobytes() == hb.view(word).tobytes(), "B, its padding or its guards were modified"
    return np.ascontiguousarray(got[lo:lo + n * ld].reshape(n, ld)[:, col0:col0 + k])


def solve_single(T, b):
    import torch
    tb = torch.from_numpy(np.array(b)).to("cuda")
    tx = torch.full_like(tb, float("nan"))
    T.solve_device(tb.data_ptr(), tx.data_ptr())
    torch.cuda.synchronize()
    return tx.cpu().numpy()


def assert_columns(got, want, singles, what):
    assert got.shape == want.shape and got.dtype == want.dtype
    for j in range(got.shape[1]):
        assert same_bits(got[:, j], want[:, j]), f"{what}: column {j} against the sequential loop: " \
            f"{int(np.sum(got[:, j] != want[:, j]))} of {len(want)} rows differ"
        assert same_bits(got[:, j], singles[j]), f"{what}: column {j} against the single solve"


def check_handle(T, rhs, want, what, ks=KS, strided=(1, 3, 9, 11), window=(2, 8), in_place=(5, 11)):
    """every k at ld = k on an aligned base; some at ld = k + 3 one element off alignment, some as the columns 3 .. 3 + k of a
    16-wide block, some in place (aligned, and off alignment with padding). k = 1 at ld = 1 is handed to the single solve, so k = 1
    is also run at ld = 4, where the chunk of one column is on its own."""
    singles = [solve_single(T, np.ascontiguousarray(rhs[:, j])) for j in range(max(ks))]
    for k in ks:
        assert_columns(solve_multi(T, rhs[:, :k]), want[:, :k], singles, f"{what}: k = {k}")
    for k in strided:
        assert_columns(solve_multi(T, rhs[:, :k], ld=k + 3, shift=1), want[:, :k], singles, f"{what}: k = {k}, ld = k + 3, off alignment")
    for k in window:
        assert_columns(solve_multi(T, rhs[:, :k], ld=16, col0=3), want[:, :k], singles, f"{what}: k = {k}, columns 3.. of 16")
    for k in in_place:
        assert_columns(solve_multi(T, rhs[:, :k], in_place=True), want[:, :k], singles, f"{what}: k = {k}, in place")
        assert_columns(solve_multi(T, rhs[:, :k], ld=k + 3, shift=1, in_place=True), want[:, :k], singles,
                       f"{what}: k = {k}, in place, ld = k + 3, off alignment")


# ---- the global plan -------------------------------------------------------------------------------------------------------------------

GLOBAL = [("prescribed", 64), ("prescribed", 256), ("bidiagonal", 0), ("padding", 0), ("dag", 0), ("one", 0)]


@pytest.mark.parametrize("dtype", DTYPES, ids=("f64", "f32"))
@pytest.mark.parametrize("unit", (False, True), ids=("stored", "unit"))
@pytest.mark.parametrize("uplo,side", SIDES, ids=("lower", "upper"))
@pytest.mark.parametrize("name,chain_rows", GLOBAL, ids=[f"{a}-{c}" for a, c in GLOBAL])
def test_every_column_of_a_global_solve_has_the_bits_of_the_sequential_loop_and_of_the_single_solve(eng, name, chain_rows, uplo, side,
                                                                                                     unit, dtype):
    A, rhs, want = expected(name, None, uplo, unit, dtype)
    T = eng.TriangularSolve(*A, uplo=side, diag="unit" if unit else "stored", dtype=dtype, chain_rows=chain_rows)
    if name == "prescribed":
        # levels of 2000 and 3000 rows are launches of their own at both sizes; those of 70 and 65 rows are chained only at 256
        assert T.info["launches"] == (9 if chain_rows == 64 else 5) and T.info["max_level_rows"] == 3000
    if name == "bidiagonal":
        assert T.info["launches"] == 1 and T.info["levels"] == 4097
    check_handle(T, rhs, want, f"{name} chain_rows {chain_rows}")
    T.close()


# ---- blocked handles -------------------------------------------------------------------------------------------------------------------

BLOCKED = [("dag", (1, 64, 100, 1024)), ("bidiagonal", (1, 64, 100, 1024)), ("prescribed", (1, 64, 100, 1024, 16384)),
           ("one", (1, 64, 100, 1024))]


@pytest.mark.parametrize("dtype", DTYPES, ids=("f64", "f32"))
@pytest.mark.parametrize("unit", (False, True), ids=("stored", "unit"))
@pytest.mark.parametrize("uplo,side", SIDES, ids=("lower", "upper"))
@pytest.mark.parametrize("name,sizes", BLOCKED, ids=[b[0] for b in BLOCKED])
def test_every_column_of_a_blocked_solve_has_the_bits_of_the_loop_on_the_filtered_matrix(eng, name, sizes, uplo, side, unit, dtype):
    """B = 1 on bidiagonal: 4097 workgroups; prescribed at B = 16384: levels of 2000 and 3000 rows in a workgroup of 1024 threads,
    and 5208 rows of LDS per column, so Kmax is 2 in fp64 and 4 in fp32"""
    for B in sizes:
        A, rhs, want = expected(name, B, uplo, unit, dtype)
        T = eng.TriangularSolve(*A, uplo=side, diag="unit" if unit else "stored", dtype=dtype, block_rows=B)
        if B == 16384:
            assert A[3] == 5208 and T.solve_multi_plan(8)["max_chunk"] == (2 if dtype == np.float64 else 4)
            assert T.info["max_level_rows"] == 3000
        if (name, B) == ("bidiagonal", 1):
            assert T.block_info()["blocks"] == 4097
        # the whole ladder of k at the two sizes where blocks differ most, a shorter one elsewhere
        full = B in (100, 16384)
        check_handle(T, rhs, want, f"{name} B = {B}", ks=KS if full else (1, 3, 8, 11), strided=(1, 3, 11) if full else (1, 11),
                     window=(2, 8) if full else (8,), in_place=(5, 11) if full else (5,))
        T.close()


EDGES = [(np.float64, 2560, 8, 1, 8), (np.float64, 2561, 8, 2, 4), (np.float64, 16384, 2, 2, 1), (np.float32, 16384, 2, 1, 2)]


@pytest.mark.parametrize("uplo,side", SIDES, ids=("lower", "upper"))
@pytest.mark.parametrize("dtype,B,k,passes,kmax", EDGES, ids=[f"{np.dtype(e[0]).name}-{e[1]}-k{e[2]}" for e in EDGES])
def test_the_lds_edges(eng, dtype, B, k, passes, kmax, uplo, side):
    """2560 rows of 8 fp64 values are exactly 160 KiB; one row more halves the chunk"""
    A, rhs, want = expected("big_dag", B, uplo, False, dtype, k)
    T = eng.TriangularSolve(*A, uplo=side, dtype=dtype, block_rows=B)
    assert T.solve_multi_plan(k) == dict(matrix_passes=passes, launches=passes, max_chunk=kmax)
    singles = [solve_single(T, np.ascontiguousarray(rhs[:, j])) for j in range(k)]
    assert_columns(solve_multi(T, rhs), want, singles, f"big_dag B = {B}, k = {k}")
    assert_columns(solve_multi(T, rhs, ld=k + 3, shift=1, in_place=True), want, singles, f"big_dag B = {B}, k = {k}, in place, strided")
    T.close()


# ---- independence, repeatability, the host form, no rows -------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=("f64", "f32"))
@pytest.mark.parametrize("B", (None, 100), ids=("global", "blocked"))
def test_a_nan_in_one_column_stays_in_that_column(eng, B, dtype):
    A, rhs, want = expected("dag", B, LOWER, False, dtype)
    T = eng.TriangularSolve(*A, dtype=dtype, block_rows=B)
    for j in (3, 9, 10):                                   # inside the chunk of 8, inside the chunk of 2, the chunk of 1
        bad = np.array(rhs)
        bad[17, j] = np.nan
        single = solve_single(T, np.ascontiguousarray(bad[:, j]))
        assert np.isnan(single[17]) and np.isnan(single).sum() < len(single), "the NaN reaches some rows, not all"
        got = solve_multi(T, bad)
        for c in range(KMAX):
            if c == j:
                assert same_bits(got[:, c], single), f"column {j} against the single solve of the same column"
            else:
                assert same_bits(got[:, c], want[:, c]), f"a NaN in column {j} moved column {c}"
    T.close()


@pytest.mark.parametrize("B", (None, 64), ids=("global", "blocked"))
def test_twice_the_same_bytes(eng, B):
    A, rhs, want = expected("prescribed", B, UPPER, False, np.float64)
    T = eng.TriangularSolve(*A, uplo="upper", block_rows=B)
    a, b = solve_multi(T, rhs), solve_multi(T, rhs)
    assert same_bits(a, b) and same_bits(a, want)
    T.close()


@pytest.mark.parametrize("dtype", DTYPES, ids=("f64", "f32"))
@pytest.mark.parametrize("B", (None, 100), ids=("global", "blocked"))
def test_the_host_form_after_k_grows_from_2_to_9(eng, B, dtype):
    A, rhs, want = expected("dag", B, LOWER, False, dtype)
    T = eng.TriangularSolve(*A, dtype=dtype, block_rows=B)
    for k in (2, 9, 3, 11):
        got = T.solve_multi(rhs[:, :k])
        assert got.shape == (A[3], k) and same_bits(got, want[:, :k]), f"solve_multi at k = {k}"
    x = np.array(rhs[:, :5])                              # the host form in place
    p = x.ctypes.data_as(__import__("ctypes").c_void_p)
    assert eng.lib().spmv_mi355x_trsv_solve_multi(T.h, 5, p, p) == 0
    assert same_bits(x, want[:, :5])
    assert same_bits(T.solve(np.ascontiguousarray(rhs[:, 0])), want[:, 0]), "the single host form beside it"
    T.close()


@pytest.mark.parametrize("B", (None, 64), ids=("global", "blocked"))
def test_no_rows_launch_nothing(eng, B):
    import torch
    A, rhs, want = expected("empty", B, LOWER, False, np.float64)
    T = eng.TriangularSolve(*A, block_rows=B)
    assert T.solve_multi_plan(11) == dict(matrix_passes=0, launches=0, max_chunk=0)
    x = torch.full((32,), SENTINEL, dtype=torch.float64, device="cuda")
    T.solve_multi_device(3, x.data_ptr(), 3, x.data_ptr(), 3)
    T.solve_multi_device(3, 0, 3, 0, 3)                   # no block is needed for no rows
    torch.cuda.synchronize()
    assert bool(torch.all(x == SENTINEL))
    assert T.solve_multi(np.zeros((0, 3))).shape == (0, 3)
    T.close()


def test_timing_runs_the_same_solve(eng):
    import torch
    A, rhs, want = expected("dag", None, LOWER, False, np.float64)
    T = eng.TriangularSolve(*A)
    tb = torch.from_numpy(np.array(rhs[:, :3])).to("cuda")
    tx = torch.full_like(tb, float("nan"))
    ms = T.time_multi_device(3, tb.data_ptr(), 3, tx.data_ptr(), 3, 2)
    assert ms > 0 and same_bits(tx.cpu().numpy(), want[:, :3])
    T.close()
