"""SpGEMM on the GPU (include/spmv_mi355x.h "SpGEMM"): spmv_mi355x_spgemm_* / SpGemm / spgemm.

In every case pattern() equals the arrays of tests/spgemm_reference.c (the header's loop run sequentially, gcc -ffp-contract=off;
itself checked against scipy in test_spgemm_abi.py) exactly, and multiply() equals its values BIT FOR BIT. The cases of
spgemm_cases.py: spd_grid(45) squared and its lower triangle squared (whose pattern is fsai_pattern(power = 2)); a random rectangular
pair with empty and unsorted rows and a column twice in rows of A; rows at both sides of every bin boundary of csrc/spgemm.hpp for
both binnings; a row of 12 000 products and one that fills all n columns (tables in global memory); a row whose columns all hash
to one slot; cancellation to stored zeros; 32 * 2048 + 37 narrow rows (the grid-stride loop's second trip); the empty shapes.
Then determinism and reuse of a plan, the chain into update_values_device of a handle of C, A A^t through the CSR that a transposed
handle holds, and the refusal of nnz(C) >= 2^31."""
import ctypes

import numpy as np
import pytest

import pcg_tri_cases as pc
import spgemm_cases as sc

pytestmark = pytest.mark.gpu

DELTA = dict(sell_c=64, sell_delta=1, sell_sigma=64, sell_window=2)


@pytest.fixture(scope="module")
def eng():
    import spmv_mi355x as eng
    assert eng.device_count() >= 1, "no GPU visible: the -m gpu tests need an MI355X"
    return eng


def plan(eng, name):
    A, B = sc.case(name)
    return eng.SpGemm(A[0], A[1], A[3], A[4], B[0], B[1], B[4])


def differing(got, want):
    """the count of values that differ in their bits (0.0 and -0.0 differ, equal NaNs do not)"""
    return int(np.count_nonzero(got.view(np.uint64) != want.view(np.uint64)))


@pytest.mark.parametrize("name", sc.GPU_CASES)
def test_pattern_and_values_are_the_references(eng, name):
    A, B = sc.case(name)
    c_rp, c_ci, c_va = sc.reference_of(name)
    P = plan(eng, name)
    info = P.info()
    assert P.shape == (A[3], B[4]) and P.nnz == len(c_ci) == info["nnz_c"]
    assert P.row_ptr.dtype == np.int32 and P.col_idx.dtype == np.int32
    assert np.array_equal(P.row_ptr, c_rp) and np.array_equal(P.col_idx, c_ci), name
    got = P.multiply(A[2], B[2])
    assert got.dtype == np.float64 and got.shape == c_va.shape
    diff = differing(got, c_va)
    info = P.info()
    print(f"[spgemm] {name}: {diff} of {len(c_va)} values differ from the C reference; products {info['products']}, rows per bin "
          f"{info['symbolic_bin_rows']} symbolic, {info['numeric_bin_rows']} numeric, {info['symbolic_probes']} probes; symbolic "
          f"{info['symbolic_seconds']:.3g} s, numeric {info['multiply_seconds']:.3g} s, {info['device_bytes']:.3g} bytes held")
    assert diff == 0
    b_len = np.diff(B[0])
    products = np.array([b_len[A[1][A[0][i]:A[0][i + 1]]].sum() for i in range(A[3])], np.int64)
    assert info["products"] == products.sum() and info["max_row_products"] == (products.max() if len(products) else 0)
    assert info["max_row_c"] == (np.diff(c_rp).max() if A[3] else 0)
    assert (info["m"], info["k"], info["n"], info["nnz_a"], info["nnz_b"]) == (A[3], A[4], B[4], len(A[1]), len(B[1]))
    assert info["symbolic_bin_rows"] == np.bincount([sc.bin_of(min(p, B[4])) for p in products], minlength=sc.BINS).tolist()
    assert info["numeric_bin_rows"] == np.bincount([sc.bin_of(w) for w in np.diff(c_rp)], minlength=sc.BINS).tolist()
    assert info["device_bytes"] >= 4 * (len(A[0]) + len(A[1]) + len(B[0]) + len(B[1]) + len(c_rp) + len(c_ci))
    P.close()
    P.close()                                                          # closing twice is harmless


def test_every_instantiation_runs(eng):
    """bins: every bin of both binnings holds rows (the cases' own widths are pinned in test_spgemm_abi.py)"""
    P = plan(eng, "bins")
    info = P.info()
    assert all(c > 0 for c in info["symbolic_bin_rows"]) and all(c > 0 for c in info["numeric_bin_rows"]), info
    assert info["symbolic_bin_rows"] != info["numeric_bin_rows"]
    P.close()


def test_the_grid_pattern_is_fsai_pattern(eng):
    rp, ci, va, n, _ = pc.spd_grid(45)
    P = plan(eng, "grid_tril")
    prp, pci = eng.fsai_pattern(rp, ci, n, power=2)
    assert np.array_equal(P.row_ptr, prp) and np.array_equal(P.col_idx, pci)
    assert P.info()["max_row_products"] <= 25 and plan(eng, "grid").info()["max_row_products"] == 25
    P.close()


def test_colliding_columns_probe(eng):
    """every column of the row hashes to one slot: insertion t ends t slots on, whatever order the lanes arrive in"""
    P = plan(eng, "collide")
    w = sc.COLLIDE_WIDTH
    info = P.info()
    print(f"[spgemm] collide: {info['symbolic_probes']} probes beyond the first over 3 rows of {w} columns")
    # the row that names B's row twice has 2 w products: it is counted in a table of 8192 slots in global memory, under another hash
    assert info["symbolic_bin_rows"] == [0, 0, 0, 0, 0, 2, 1] and info["numeric_bin_rows"] == [0, 0, 0, 0, 0, 3, 0]
    assert info["symbolic_probes"] >= 2 * (w * (w - 1) // 2)
    P.close()


def test_cancellation_stores_zeros(eng):
    A, B = sc.case("cancel")
    rp, ci, va = eng.spgemm(A, B)
    assert rp.tolist() == [0, 5, 10] and ci.tolist() == [0, 2, 4, 7, 9] * 2
    assert np.all(va == 0) and differing(va, sc.reference_of("cancel")[2]) == 0 and not np.any(np.signbit(va))


def test_empty_plans_touch_nothing(eng):
    import torch
    for name in ("empty_m", "empty_k", "empty_n", "empty_a"):
        A, B = sc.case(name)
        P = plan(eng, name)
        assert P.nnz == 0 and np.array_equal(P.row_ptr, np.zeros(A[3] + 1, np.int32)) and P.col_idx.shape == (0,)
        assert P.multiply(A[2], B[2]).shape == (0,)
        x = torch.full((8,), -7.25, dtype=torch.float64, device="cuda")
        P.multiply_device(x.data_ptr(), x.data_ptr(), x.data_ptr())
        P.multiply_device(0, 0, 0)
        torch.cuda.synchronize()
        assert bool(torch.all(x == -7.25))
        P.close()


def test_null_values_and_struct_size(eng):
    P = plan(eng, "rect")
    with pytest.raises(eng.SpmvError, match=r"spgemm_multiply: NULL argument \( a_values b_values c_values \)"):
        P.multiply_device(0, 0, 0)
    st = eng.SpgemmStats()
    st.struct_size = 4
    assert eng.lib().spmv_mi355x_spgemm_info(P.h, ctypes.byref(st)) == 1
    assert eng.lib().spmv_mi355x_last_error().decode() == "spgemm_info: info->struct_size not set"
    # a shorter struct of an older caller: only its bytes are written
    st.struct_size = eng.SpgemmStats.nnz_c.offset + 8
    st.products = -5
    assert eng.lib().spmv_mi355x_spgemm_info(P.h, ctypes.byref(st)) == 0
    assert (st.struct_size, st.m, st.nnz_c, st.products) == (eng.SpgemmStats.nnz_c.offset + 8, 300, P.nnz, -5)
    P.close()


# ---- determinism and reuse ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ("rect", "bins"))
def test_a_plan_holds_no_values(eng, name):
    A, B = sc.case(name)
    rng = np.random.default_rng(11)
    a2, b2 = rng.uniform(-1, 1, len(A[2])), rng.uniform(-1, 1, len(B[2]))
    P = plan(eng, name)
    first = P.multiply(A[2], B[2])
    assert differing(P.multiply(A[2], B[2]), first) == 0                                 # twice: the same bits
    second = P.multiply(a2, b2)
    fresh = plan(eng, name)
    assert differing(second, fresh.multiply(a2, b2)) == 0                              # new values on the old plan: a fresh plan's
    assert differing(second, sc.reference(A, B, a2, b2)[2]) == 0
    assert differing(P.multiply(A[2], B[2]), first) == 0 and differing(first, second) > 0   # A1, A2, A1: the first result again
    P.close()
    fresh.close()


@pytest.mark.parametrize("fmt,opts", [("sell_c_sigma", DELTA), ("csr_vector", {})])
def test_the_chain_into_update_values_device(eng, fmt, opts):
    """multiply_device writes C's values in C's entry order: what update_values_device of a handle of C takes"""
    import torch
    A, B = sc.case("grid")
    n = B[4]
    P = plan(eng, "grid")
    c1 = P.multiply(A[2], B[2])
    M = eng.Matrix(P.row_ptr, P.col_idx, c1, A[3], n, fmt, np.float64, **opts)
    M.update_values_prepare(P.row_ptr)
    a2 = A[2] * np.random.default_rng(4).uniform(0.5, 1.5, len(A[2]))
    ta, tb = torch.from_numpy(a2).cuda(), torch.from_numpy(np.array(B[2])).cuda()
    tc = torch.full((P.nnz + 8,), -7.25, dtype=torch.float64, device="cuda")
    P.multiply_device(ta.data_ptr(), tb.data_ptr(), tc.data_ptr())
    M.update_values_device(tc.data_ptr())
    torch.cuda.synchronize()
    c2 = tc.cpu().numpy()
    assert np.all(c2[P.nnz:] == -7.25) and differing(c2[:P.nnz], sc.reference(A, B, a2)[2]) == 0
    F = eng.Matrix(P.row_ptr, P.col_idx, c2[:P.nnz], A[3], n, fmt, np.float64, **opts)
    x = np.random.default_rng(5).uniform(-1, 1, n)
    assert differing(M.spmv(x), F.spmv(x)) == 0 and differing(c1, c2[:P.nnz]) > 0
    for h in (M, F, P):
        h.close()


# ---- A A^t through a transposed handle -----------------------------------------------------------------------------------------------------

def test_a_at_through_the_transposed_handle(eng):
    """The CSR of A^t as transpose_csr built it on the device for a transpose = 1 handle, read back from the handle's plain SELL
    layout. A A^t is symmetric in its pattern, and its values lie within the bound of scipy's."""
    A, _ = sc.case("rect")
    rp, ci, va, m, k = A
    T = eng.Matrix(rp, ci, va, m, k, "sell_c_sigma", np.float64, transpose=1, sell_c=64, sell_delta=0)
    assert (T.m, T.n, T.transposed) == (k, m, 1)
    lay = T.sell_layout()
    assert lay["C"] == 64
    t_rp = np.concatenate([[0], np.cumsum(np.bincount(ci, minlength=k))]).astype(np.int32)
    t_ci, t_va = np.zeros(len(ci), np.int32), np.zeros(len(ci))
    for i, o in enumerate(lay["row_of_sorted"]):
        at = lay["slice_ptr"][i // 64] + np.arange(t_rp[o + 1] - t_rp[o]) * 64 + i % 64
        t_ci[t_rp[o]:t_rp[o + 1]], t_va[t_rp[o]:t_rp[o + 1]] = lay["col"][at], lay["val"][at]
    T.close()
    At = (t_rp, t_ci, t_va, k, m)
    assert np.array_equal(sc.scipy_of(At).toarray(), sc.scipy_of(A).toarray().T)
    # rect's A holds a column twice in some rows, so A^t does too, and as B it is refused; the product runs on both with the two
    # occurrences merged
    S = sc.scipy_of(A)
    S.sum_duplicates()
    S.sort_indices()
    A1 = (S.indptr.astype(np.int32), S.indices.astype(np.int32), S.data.copy(), m, k)
    with pytest.raises(eng.SpmvError, match=r"spgemm_create: row \d+ of B stores column \d+ twice"):
        eng.spgemm(A, At)
    c_rp, c_ci, c_va = eng.spgemm(A1, _merged(At))
    ref = sc.reference(A1, _merged(At))
    assert np.array_equal(c_rp, ref[0]) and np.array_equal(c_ci, ref[1]) and differing(c_va, ref[2]) == 0
    D = np.zeros((m, m), bool)
    D[np.repeat(np.arange(m), np.diff(c_rp)), c_ci] = True
    assert np.array_equal(D, D.T) and len(c_ci) > m
    share = sc.shares_of_the_bound(A1, _merged(At), c_rp, c_ci, c_va)
    print(f"[spgemm] A A^t of rect: nnz(C) = {len(c_ci)}, within {share.max():.3g} of its bound of scipy")
    assert np.all(share <= 1)


def _merged(M):
    """the same matrix with the two occurrences of a column summed (in the order scipy keeps: the row's entries stay in place)"""
    S = sc.scipy_of(M)
    S.sum_duplicates()
    return S.indptr.astype(np.int32), S.indices.astype(np.int32), S.data.copy(), M[3], M[4]


# ---- nnz(C) >= 2^31 ----------------------------------------------------------------------------------------------------------------------------

def test_a_product_beyond_int32_is_refused(eng):
    """a column of 46 341 ones times a row of 46 341 ones: 46 341^2 = 2 147 488 281 entries, refused at the symbolic step"""
    s = 46341
    ones_col = (np.arange(s + 1, dtype=np.int32), np.zeros(s, np.int32))
    ones_row = (np.array([0, s], np.int32), np.arange(s, dtype=np.int32))
    with pytest.raises(eng.SpmvError, match=r"spgemm_create: symbolic: C has 2147488281 entries"):
        eng.SpGemm(*ones_col, s, 1, *ones_row, s)
