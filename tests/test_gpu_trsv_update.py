"""update_values for triangular solve handles (include/spmv_mi355x.h "UPDATE_VALUES") on the GPU. There is no tolerance anywhere: a
handle created on V1 and updated to V2 must hold, byte for byte, what a handle freshly created on V2 holds (stored_values(): every
slot, padding included, and the diagonal), must solve bit for bit like it and like the sequential C loop of tests/trsv_reference.c,
and an update back to V1 must restore create(V1). A refused update must leave every byte and every solve as they were.

V2 from V1 on the same pattern: off-diagonal entries times u (+-1) with u in [0.5, 1], diagonal entries times u (+-1) with u in
[1, 1.5]. That keeps trsv_cases' bound (row sums of |a_ij| <= 0.9, |d| >= 1), so nothing overflows even on the 4097-level chain."""
import ctypes
import functools

import numpy as np
import pytest

import ilu0_cases as ic
import pcg_tri_cases as pc
import trsv_blocked_cases as bc
import trsv_cases as tc
from trsv_cases import LOWER, UPPER

pytestmark = pytest.mark.gpu

UPLO = {LOWER: "lower", UPPER: "upper"}
DTYPES = (np.float64, np.float32)


@pytest.fixture(scope="module")
def eng():
    import spmv_mi355x as eng
    assert eng.device_count() >= 1, "no GPU visible: the -m gpu tests need an MI355X"
    return eng


def new_values(rp, ci, va, n, seed=2):
    rng = np.random.default_rng(seed)
    rows = np.repeat(np.arange(n), np.diff(rp))
    u = np.where(rows == ci, rng.uniform(1, 1.5, len(va)), rng.uniform(0.5, 1, len(va))) * rng.choice((-1.0, 1.0), len(va))
    out = np.asarray(va) * u
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def case(name, uplo):
    """(rp, ci, V1, n, V2)"""
    A = bc.convdiff()[:4] if name == "convdiff" else tc.matrix(name, uplo)
    return (*A, new_values(*A))


def same_bytes(a, b):
    """two stored_values() results, compared on the raw bytes"""
    for x, y in zip(a, b):
        if (x is None) != (y is None):
            return False
        if x is not None and not (x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x.view(np.uint8), y.view(np.uint8))):
            return False
    return True


def device_array(a):
    import torch
    t = torch.from_numpy(np.array(a, np.float64)).cuda()
    torch.cuda.synchronize()
    return t


def reference(rp, ci, va, n, uplo, unit, b, dtype, B):
    A = (rp, ci, va, n) if B is None else bc.filtered(rp, ci, np.asarray(va), n, B)
    return tc.reference(*A, uplo, unit, b, dtype)


def rhs(n, k=None):
    rng = np.random.default_rng(n + 7)
    return rng.uniform(-1, 1, n if k is None else (n, k))


# ---- 1. byte identity ------------------------------------------------------------------------------------------------------------------

BYTE_CASES = [(name, None) for name in ("prescribed", "padding", "dag", "stencil", "convdiff", "bidiagonal", "empty", "one")] + \
             [(name, 100) for name in ("prescribed", "padding", "dag", "bidiagonal", "empty", "one")] + \
             [(name, B) for name in ("stencil", "convdiff") for B in (64, 100, 256)]


@pytest.mark.parametrize("name,B", BYTE_CASES, ids=[f"{n}-{b}" for n, b in BYTE_CASES])
def test_an_updated_handle_is_a_fresh_handle(eng, name, B):
    for uplo in (LOWER, UPPER):
        rp, ci, v1, n, v2 = case(name, uplo)
        v2_dev = device_array(v2)
        b, Bk = rhs(n), rhs(n, 3)
        for diag in ("stored", "unit"):
            for dtype in DTYPES:
                what = f"{name} B={B} {UPLO[uplo]} {diag} {np.dtype(dtype).name}"
                make = lambda v: eng.TriangularSolve(rp, ci, v, n, UPLO[uplo], diag, dtype, block_rows=B)
                T, fresh = make(v1), make(v2)
                created, want = T.stored_values(), fresh.stored_values()
                x1, footprint = T.solve(b), T.mem_footprint
                assert T.update_values_state == 1 and T.update_values_bytes == 0
                T.update_values_prepare(rp, ci)
                assert T.update_values_state == 2
                assert T.update_values_bytes == 4 * len(want[0]) + (4 * n if diag == "stored" else 0) + 16
                assert eng.lib().spmv_mi355x_trsv_mem_footprint(T.h) == footprint == T.mem_footprint
                assert same_bytes(T.stored_values(), created), f"{what}: prepare changed the handle"
                T.update_values_prepare(rp, ci)                               # a second prepare does nothing
                # the host form
                T.update_values(v2)
                assert T.update_values_state == 2 and T.update_values_result() == -1
                assert same_bytes(T.stored_values(), want), f"{what}: the updated handle differs from create(V2)"
                x2 = T.solve(b)
                ref = reference(rp, ci, v2, n, uplo, diag == "unit", b, dtype, B)
                assert np.array_equal(x2, fresh.solve(b)) and np.array_equal(x2, ref), what
                if n:
                    X = T.solve_multi(Bk)
                    for j in range(3):
                        assert np.array_equal(X[:, j], reference(rp, ci, v2, n, uplo, diag == "unit", Bk[:, j], dtype, B)), (what, j)
                    assert np.array_equal(X, fresh.solve_multi(Bk))
                if not same_bytes(created, want):                             # UNIT without a kept entry stores no number at all
                    assert not np.array_equal(x1, x2), f"{what}: nothing was written"
                # back to V1: create(V1) again
                T.update_values(v1)
                assert same_bytes(T.stored_values(), created) and np.array_equal(T.solve(b), x1), what
                # the device form leaves the same bytes
                T.update_values_device(v2_dev.data_ptr())
                assert T.update_values_state == 2
                assert same_bytes(T.stored_values(), want) and np.array_equal(T.solve(b), x2), what
                T.close()
                fresh.close()


@functools.lru_cache(maxsize=None)
def long_pairs():
    """two levels of 550 000 rows, row 2m + 1 storing (2m, 2m + 1) and row 2m its diagonal: 550 000 slots and 1 100 000 positions,
    both more than one grid of the update kernels holds (2048 workgroups of 256 threads): the grid-stride loops"""
    n = 1100000
    rng = np.random.default_rng(n)
    odd = np.arange(n) % 2 == 1
    rp = np.concatenate([[0], np.cumsum(np.where(odd, 2, 1))])
    ci, va = np.empty(rp[-1], np.int64), np.empty(rp[-1])
    dia = rp[1:] - 1
    ci[dia] = np.arange(n)
    va[dia] = rng.uniform(1, 2, n)
    ci[dia[odd] - 1] = np.arange(n)[odd] - 1
    va[dia[odd] - 1] = rng.uniform(-0.9, 0.9, n // 2)
    A = (rp.astype(np.int32), ci.astype(np.int32), va, n)
    return (*A, new_values(*A))


def test_more_slots_than_one_grid(eng):
    rp, ci, v1, n, v2 = long_pairs()
    b = rhs(n)
    for dtype in DTYPES:
        T = eng.TriangularSolve(rp, ci, v1, n, "lower", "stored", dtype)
        fresh = eng.TriangularSolve(rp, ci, v2, n, "lower", "stored", dtype)
        want = fresh.stored_values()
        assert len(want[0]) == n // 2 > 2048 * 256
        x1 = T.solve(b)
        T.update_values_prepare(rp, ci).update_values(v2)
        assert same_bytes(T.stored_values(), want)
        x2 = T.solve(b)
        assert np.array_equal(x2, fresh.solve(b)) and np.array_equal(x2, tc.reference(rp, ci, v2, n, LOWER, False, b, dtype))
        assert not np.array_equal(x1, x2)
        T.close()
        fresh.close()


# ---- 2. refusals on the device ---------------------------------------------------------------------------------------------------------

def diagonal_entry(rp, ci, row):
    return rp[row] + np.flatnonzero(ci[rp[row]:rp[row + 1]] == row)[0]


@pytest.mark.parametrize("B", (None, 100), ids=str)
def test_a_bad_diagonal_is_refused_and_nothing_is_written(eng, B):
    rp, ci, v1, n, v2 = case("dag", LOWER)
    v2_good = device_array(v2)
    b = rhs(n)
    for dtype in DTYPES:
        T = eng.TriangularSolve(rp, ci, v1, n, "lower", "stored", dtype, block_rows=B)
        T.update_values_prepare(rp, ci)
        created, x1 = T.stored_values(), T.solve(b)
        for value, shown in ((0.0, "0"), (np.nan, "nan"), (np.inf, "inf"), (-np.inf, "-inf")):
            for rows in ((1234,), (2000, 77, 1500)):
                bad = np.array(v2)
                for r in rows:
                    bad[diagonal_entry(rp, ci, r)] = value
                msg = rf"^trsv_update_values: the diagonal of row {min(rows)} is {shown} in the handle's precision \(from {shown}\): " \
                      "it must be finite and non-zero$"
                with pytest.raises(eng.SpmvError, match=msg):
                    T.update_values(bad)
                assert T.update_values_state == 3 and T.update_values_result() == min(rows)
                assert same_bytes(T.stored_values(), created) and np.array_equal(T.solve(b), x1)
                # the async device form: the refusal is the device's, the result names the row
                dev = device_array(bad)
                T.update_values_device(dev.data_ptr(), wait=False)
                assert T.update_values_result() == min(rows) and T.update_values_state == 3
                with pytest.raises(eng.SpmvError, match=msg):
                    T.update_values_device(dev.data_ptr())
                assert same_bytes(T.stored_values(), created) and np.array_equal(T.solve(b), x1)
        # a good update afterwards: state 2 and the fresh handle's bytes
        fresh = eng.TriangularSolve(rp, ci, v2, n, "lower", "stored", dtype, block_rows=B)
        T.update_values_device(v2_good.data_ptr())
        assert T.update_values_state == 2 and T.update_values_result() == -1
        assert same_bytes(T.stored_values(), fresh.stored_values()) and np.array_equal(T.solve(b), fresh.solve(b))
        T.close()
        fresh.close()


def test_a_diagonal_that_narrows_to_zero_is_refused_in_fp32_only(eng):
    rp, ci, v1, n, v2 = case("dag", LOWER)
    tiny = np.array(v2)
    tiny[diagonal_entry(rp, ci, 9)] = 1e-60
    T32 = eng.TriangularSolve(rp, ci, v1, n, "lower", "stored", np.float32).update_values_prepare(rp, ci)
    created = T32.stored_values()
    with pytest.raises(eng.SpmvError, match=r"^trsv_update_values: the diagonal of row 9 is 0 in the handle's precision \(from 1e-60\)"):
        T32.update_values(tiny)
    assert T32.update_values_state == 3 and same_bytes(T32.stored_values(), created)
    with pytest.raises(eng.SpmvError, match=r"^trsv_create: the diagonal of row 9 is 0 in the handle's precision \(from 1e-60\)"):
        eng.TriangularSolve(rp, ci, tiny, n, "lower", "stored", np.float32)
    T32.close()
    T64 = eng.TriangularSolve(rp, ci, v1, n, "lower", "stored", np.float64).update_values_prepare(rp, ci)
    fresh = eng.TriangularSolve(rp, ci, tiny, n, "lower", "stored", np.float64)
    T64.update_values(tiny)
    assert T64.update_values_state == 2 and same_bytes(T64.stored_values(), fresh.stored_values())
    T64.close()
    fresh.close()


def test_a_unit_handle_takes_any_stored_diagonal(eng):
    rp, ci, v1, n, v2 = case("dag", LOWER)
    rows = np.repeat(np.arange(n), np.diff(rp))
    b = rhs(n)
    for value in (0.0, np.nan):
        v = np.array(v2)
        v[rows == ci] = value
        for dtype in DTYPES:
            T = eng.TriangularSolve(rp, ci, v1, n, "lower", "unit", dtype).update_values_prepare(rp, ci)
            fresh = eng.TriangularSolve(rp, ci, v, n, "lower", "unit", dtype)
            T.update_values(v)
            assert T.update_values_state == 2 and T.update_values_result() == -1
            assert same_bytes(T.stored_values(), fresh.stored_values())
            assert np.array_equal(T.solve(b), tc.reference(rp, ci, v2, n, LOWER, True, b, dtype))
            T.close()
            fresh.close()


# ---- 3. prepare: the pattern must be the handle's -----------------------------------------------------------------------------------------

def test_update_before_prepare_and_null_values(eng):
    rp, ci, v1, n, v2 = case("prescribed", LOWER)
    T = eng.TriangularSolve(rp, ci, v1, n, "lower")
    created, footprint = T.stored_values(), T.mem_footprint
    L, err = eng.lib(), lambda: eng.lib().spmv_mi355x_last_error().decode()
    # 2. the NULL array comes before 3. the missing prepare
    assert L.spmv_mi355x_trsv_update_values(T.h, None) == 1 and err() == "trsv_update_values: NULL argument ( values )"
    assert L.spmv_mi355x_trsv_update_values_device_async(T.h, None, None) == 1 and err() == "trsv_update_values: NULL argument ( values )"
    with pytest.raises(eng.SpmvError, match="^trsv_update_values: spmv_mi355x_trsv_update_values_prepare has not been called"):
        T.update_values(v2)
    with pytest.raises(eng.SpmvError, match="^trsv_update_values: spmv_mi355x_trsv_update_values_prepare has not been called"):
        T.update_values_result()
    assert T.update_values_state == 1 and T.update_values_bytes == 0 and L.spmv_mi355x_trsv_mem_footprint(T.h) == footprint
    assert same_bytes(T.stored_values(), created)
    T.update_values_prepare(rp, ci)
    assert L.spmv_mi355x_trsv_update_values(T.h, None) == 1 and err() == "trsv_update_values: NULL argument ( values )"
    assert T.update_values_state == 2 and same_bytes(T.stored_values(), created)
    T.close()


def test_prepare_refuses_another_pattern(eng):
    P = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    L, err = eng.lib(), lambda: eng.lib().spmv_mi355x_last_error().decode()
    # rows 2 and 3 depend on row 0; moving row 3's entry to column 1 changes no level, no place and no length: only its column
    rp = np.array([0, 1, 2, 4, 6], np.int32)
    ci = np.array([0, 1, 0, 2, 0, 3], np.int32)
    va = np.array([2.0, 3.0, 0.5, 4.0, 0.25, 5.0])
    b = np.arange(1.0, 5.0)
    moved = ci.copy()
    moved[4] = 1
    for B in (None, 4):
        T = eng.TriangularSolve(rp, ci, va, 4, "lower", block_rows=B)
        created, x = T.stored_values(), T.solve(b)
        with pytest.raises(eng.SpmvError, match="^trsv_update_values_prepare: the pattern is not the one the handle was created with: "
                                                "row 3 keeps other columns"):
            T.update_values_prepare(rp, moved)
        # a different n (and the rows to go with it)
        rp5 = np.append(rp, 7).astype(np.int32)
        ci5 = np.append(ci, 4).astype(np.int32)
        assert L.spmv_mi355x_trsv_update_values_prepare(T.h, 5, P(rp5), P(ci5)) == 1
        assert err() == "trsv_update_values_prepare: the pattern is not the one the handle was created with: n = 5, the handle has 4 rows"
        # a row that lost an entry: another length
        with pytest.raises(eng.SpmvError, match="^trsv_update_values_prepare: the pattern is not .* row 2 has another place"):
            T.update_values_prepare(np.array([0, 1, 2, 3, 5], np.int32), np.array([0, 1, 2, 0, 3], np.int32))
        # the checks of create come first: a missing diagonal
        with pytest.raises(eng.SpmvError, match="^trsv_update_values_prepare: row 1 has no diagonal entry"):
            T.update_values_prepare(np.array([0, 1, 1, 3, 5], np.int32), np.array([0, 0, 2, 0, 3], np.int32))
        assert T.update_values_state == 1 and T.update_values_bytes == 0
        assert same_bytes(T.stored_values(), created) and np.array_equal(T.solve(b), x)
        T.update_values_prepare(rp, ci)                                       # and the right one is still taken
        assert T.update_values_state == 2
        T.close()
    # the pattern of the other block size: the stencil without the couplings of B = 100, offered to a handle of B = 64
    rp, ci, v1, n, v2 = case("stencil", LOWER)
    other = bc.filtered(rp, ci, np.asarray(v1), n, 100)
    b = rhs(n)
    T = eng.TriangularSolve(rp, ci, v1, n, "lower", block_rows=64)
    created, x = T.stored_values(), T.solve(b)
    with pytest.raises(eng.SpmvError, match=r"^trsv_update_values_prepare: the pattern is not the one the handle was created with: row \d+ "):
        T.update_values_prepare(other[0], other[1])
    assert T.update_values_state == 1 and same_bytes(T.stored_values(), created) and np.array_equal(T.solve(b), x)
    # a pattern with MORE entries that the handle drops anyway is the handle's pattern in another entry order: accepted
    G = eng.TriangularSolve(other[0], other[1], other[2], n, "lower", block_rows=100)
    want = eng.TriangularSolve(rp, ci, v2, n, "lower", block_rows=100)
    G.update_values_prepare(rp, ci).update_values(v2)
    assert same_bytes(G.stored_values(), want.stored_values())
    for h in (T, G, want):
        h.close()


# ---- 4. streams --------------------------------------------------------------------------------------------------------------------------

def test_an_async_update_and_a_solve_on_one_stream(eng):
    import torch
    for name, B in (("dag", None), ("stencil", 100), ("bidiagonal", None)):
        rp, ci, v1, n, v2 = case(name, LOWER)
        b = rhs(n)
        for dtype in DTYPES:
            T = eng.TriangularSolve(rp, ci, v1, n, "lower", "stored", dtype, block_rows=B).update_values_prepare(rp, ci)
            fresh = eng.TriangularSolve(rp, ci, v2, n, "lower", "stored", dtype, block_rows=B)
            v = device_array(v2)
            bd = torch.from_numpy(b.astype(dtype)).cuda()
            xd = torch.zeros_like(bd)
            torch.cuda.synchronize()
            s = torch.cuda.Stream()
            T.update_values_device(v.data_ptr(), s.cuda_stream, wait=False)
            T.solve_device(bd.data_ptr(), xd.data_ptr(), s.cuda_stream)
            s.synchronize()
            assert np.array_equal(xd.cpu().numpy(), fresh.solve(b)), (name, B, dtype)
            assert T.update_values_result() == -1 and T.update_values_state == 2
            assert np.array_equal(v.cpu().numpy(), v2)                        # the caller's values are read, never written
            assert same_bytes(T.stored_values(), fresh.stored_values())
            T.close()
            fresh.close()


# ---- 5. ILU(0): the refreshed triple is the rebuilt one -------------------------------------------------------------------------------------

def close(M):
    for h in M or ():
        if h is not None and not isinstance(h, np.ndarray):
            h.close()


def ilu_values(name):
    """(rp, ci, V1, n, V2) for a refactorization: V2 stays diagonally dominant"""
    rp, ci, va, n = ic.matrix(name)
    rows = np.repeat(np.arange(n), np.diff(rp))
    if name == "spd_grid":                                                   # symmetric still: a heavier diagonal
        v2 = np.where(rows == ci, 1.3 * va, 0.9 * va)
    else:
        v2 = va * (1 + 0.1 * np.random.default_rng(5).uniform(-1, 1, len(va)))
        v2[rows == ci] = va[rows == ci] * 1.5
    return rp, ci, va, n, v2


@pytest.mark.parametrize("B", (None, 100), ids=str)
def test_update_precond_is_a_rebuilt_precond(eng, B):
    for name in ("spd_grid", "convdiff"):
        rp, ci, v1, n, v2 = ilu_values(name)
        v2_dev = device_array(v2)
        for dtype in DTYPES:
            F = eng.Ilu0(rp, ci, n, block_rows=B)
            M = F.factor(v1).precond(dtype)
            old = [M[0].stored_values(), M[2].stored_values()]
            F.factor_device(v2_dev.data_ptr())
            assert F.update_precond(M) is M
            G = eng.Ilu0(rp, ci, n, block_rows=B)
            W = G.factor(v2).precond(dtype)
            for k in (0, 2):
                assert same_bytes(M[k].stored_values(), W[k].stored_values()), (name, B, dtype, k)
                assert M[k].update_values_state == 2
            assert not same_bytes(M[0].stored_values(), old[0]) and not same_bytes(M[2].stored_values(), old[1])
            # the async form on another stream, back to V1
            import torch
            s = torch.cuda.Stream()
            F.factor_device(device_array(v1).data_ptr(), s.cuda_stream)
            F.update_precond(M, s.cuda_stream, wait=False)
            assert M[2].update_values_result() == -1 and M[0].update_values_result() == -1
            assert same_bytes(M[0].stored_values(), old[0]) and same_bytes(M[2].stored_values(), old[1])
            close(M)
            close(W)
            F.close()
            G.close()


def test_the_solvers_under_the_refreshed_triple(eng):
    P = pc.problem()
    rp, ci, v1, n, v2 = ilu_values("spd_grid")
    for dtype, lim in pc.PREC.items():
        for B in (None, 100):
            F = eng.Ilu0(rp, ci, n, block_rows=B)
            M = F.factor(v1).precond(dtype)
            F.factor(v2)
            F.update_precond(M)
            W = eng.ilu0_precond(rp, ci, v2, n, dtype, block_rows=B)
            A = eng.Matrix(rp, ci, v2, n, n, "sell_c_sigma", dtype)
            got = A.pcg_tri(P.b.astype(dtype), precond=M, tol=lim["tol"], max_iterations=pc.MAX_ITERATIONS)
            want = A.pcg_tri(P.b.astype(dtype), precond=W, tol=lim["tol"], max_iterations=pc.MAX_ITERATIONS)
            assert want["stop"] == 1 and got["stop"] == 1 and got["iterations"] == want["iterations"], (dtype, B)
            assert np.array_equal(got["x"], want["x"]) and np.array_equal(got["history"], want["history"]), (dtype, B)
            for h in (A, F):
                h.close()
            close(M)
            close(W)
    rp, ci, v1, n, v2 = ilu_values("convdiff")
    b = rhs(n)
    F = eng.Ilu0(rp, ci, n, block_rows=100)
    M = F.factor(v1).precond()
    F.factor(v2)
    F.update_precond(M)
    W = eng.ilu0_precond(rp, ci, v2, n, block_rows=100)
    A = eng.Matrix(rp, ci, v2, n, n, "sell_c_sigma", np.float64)
    got = A.gmres(b, restart=20, precond=M, tol=1e-12, max_iterations=400)
    want = A.gmres(b, restart=20, precond=W, tol=1e-12, max_iterations=400)
    assert want["stop"] == 1 and got["iterations"] == want["iterations"] and np.array_equal(got["x"], want["x"])
    for h in (A, F):
        h.close()
    close(M)
    close(W)


def test_a_breakdown_is_the_upper_handles_refusal(eng):
    rp, ci, bad, n = ic.singular()
    good = np.array([2.0, 1.0, 1.0, 2.0])
    b = np.array([1.0, -3.0])
    for dtype in DTYPES:
        F = eng.Ilu0(rp, ci, n)
        M = F.factor(good).precond(dtype)
        old = [M[0].stored_values(), M[2].stored_values()]
        x = [M[0].solve(b), M[2].solve(b)]
        F.factor(bad)
        assert F.info["breakdown_row"] == 1
        with pytest.raises(eng.SpmvError, match=r"^trsv_update_values: the diagonal of row 1 is 0 in the handle's precision \(from 0\)"):
            F.update_precond(M)
        assert M[2].update_values_state == 3 and M[0].update_values_state == 2      # the lower handle was never asked
        for k, h in enumerate((M[0], M[2])):
            assert same_bytes(h.stored_values(), old[k]) and np.array_equal(h.solve(b), x[k])
        # healthy numbers again
        F.factor(good * 2)
        F.update_precond(M)
        W = eng.Ilu0(rp, ci, n).factor(good * 2).precond(dtype)
        assert M[2].update_values_state == 2 and same_bytes(M[0].stored_values(), W[0].stored_values()) \
            and same_bytes(M[2].stored_values(), W[2].stored_values())
        close(M)
        close(W)
        F.close()


# ---- 6. SGS ---------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B", (None, 100), ids=str)
def test_sgs_precond_update_is_sgs_precond(eng, B):
    P = pc.problem()
    rp, ci, v1, n, v2 = ilu_values("spd_grid")
    for dtype, lim in pc.PREC.items():
        M = eng.sgs_precond(rp, ci, v1, n, dtype, block_rows=B)
        scale, before = M[1], M[1].copy()
        out = eng.sgs_precond_update(M, rp, ci, v2)
        W = eng.sgs_precond(rp, ci, v2, n, dtype, block_rows=B)
        assert out[0] is M[0] and out[1] is scale and out[2] is M[2]
        assert scale.dtype == W[1].dtype and np.array_equal(scale, W[1]) and not np.array_equal(scale, before)
        for k in (0, 2):
            assert same_bytes(M[k].stored_values(), W[k].stored_values()), (dtype, B, k)
        A = eng.Matrix(rp, ci, v2, n, n, "sell_c_sigma", dtype)
        got = A.pcg_tri(P.b.astype(dtype), precond=out, tol=lim["tol"], max_iterations=pc.MAX_ITERATIONS)
        want = A.pcg_tri(P.b.astype(dtype), precond=W, tol=lim["tol"], max_iterations=pc.MAX_ITERATIONS)
        assert want["stop"] == 1 and got["iterations"] == want["iterations"] and np.array_equal(got["x"], want["x"])
        A.close()
        close(M)
        close(W)
