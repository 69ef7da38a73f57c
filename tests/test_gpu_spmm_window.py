"""Y = A X on the LDS-window SELL layout (kernels_sell_window_spmm.hip) and spmv_mi355x_spmm_plan.

Every column of an spmm is bit-identical to the handle's own single-vector product of that column (beta 0 and 1), for both
precisions, every number of waves per slice, both builders and k from 1 to 16; strided X and Y touch nothing outside the k columns;
the plan query reports the passes the LDS rule gives (include/spmv_mi355x.h: need(K) <= 163 840 bytes) in three regimes; the
multi-RHS solvers on a default (window) handle reproduce the single solves bit for bit. The single-vector references are held to the
oracle by test_gpu_spmm.Columns."""
import os
import sys

import numpy as np
import pytest

import spmv_host as H
from conftest import ROOT, load_case
from test_gpu_spmm import KS, SENTINEL, Columns, _assert_exact, _make_columns  # noqa: F401
from test_gpu_solver_multi import _assert_same

sys.path.insert(0, os.path.join(ROOT, "tools"))
from solver_bench import stencil27  # noqa: E402

pytestmark = pytest.mark.gpu

LDS_MAX = 163840
# waves per slice, slices per group: 64 * split * group <= 1024 threads
SHAPES = [(1, 8), (2, 4), (4, 4), (8, 2)]


@pytest.fixture(scope="module")
def eng():
    import spmv_mi355x as eng
    assert eng.device_count() >= 1, "no GPU visible: the -m gpu tests need an MI355X"
    return eng


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def _spmm(torch, M, cols, k, beta):
    """test_gpu_spmm._spmm with a Y of its own: there Y0[:, :k].contiguous() is a VIEW of Y0 when the matrix has one row (a one-row
    slice is already contiguous), and a beta = 1 product would then accumulate into the reference's Y0 from call to call"""
    X = cols.X[:, :k].contiguous()
    Y = cols.Y0[:, :k].clone(memory_format=torch.contiguous_format) if beta else torch.full((M.m, k), SENTINEL, dtype=cols.X.dtype, device="cuda")
    assert Y.is_contiguous() and Y.data_ptr() != cols.Y0.data_ptr()
    M.spmm_device(k, X.data_ptr(), k, Y.data_ptr(), k, beta)
    torch.cuda.synchronize()
    return Y


def _window(eng, rp, ci, va, m, n, dtype, split, group, **opts):
    M = eng.Matrix(rp, ci, va, m, n, "sell_c_sigma", dtype, sell_window=1, sell_split=split, sell_group=group, **opts)
    assert "SELLW" in M.format_name, M.format_name
    return M


def _expected_kmax(M, split, group):
    """the rule of include/spmv_mi355x.h from the handle's stored group descriptors"""
    wmax = int(M.stored_array("groups", np.int32).reshape(-1, 4)[:, 1].max())
    vb = M.dtype.itemsize
    threads = 64 * split * group

    def need(K):
        return ((wmax + 1) * K * vb + 15) // 16 * 16 + (threads * K * vb if split > 1 else 0)
    assert need(1) <= LDS_MAX
    return max(K for K in (8, 4, 2, 1) if need(K) <= LDS_MAX), wmax


def _expected_plan(kmax, k):
    passes, widest = 0, 0
    while k > 0:
        K = max(c for c in (8, 4, 2, 1) if c <= min(kmax, k))
        passes, widest, k = passes + 1, max(widest, K), k - K
    return passes, widest


def _check_bit_identity(torch, M, seed, what, csr, split, group, ks=KS):
    cols = _make_columns(torch, M, seed, csr)
    assert cols.det, what
    kmax, _ = _expected_kmax(M, split, group)
    for k in ks:
        assert M.spmm_plan(k) == _expected_plan(kmax, k), f"{what} k={k}"
        for beta in (0, 1):
            Y = _spmm(torch, M, cols, k, beta)
            _assert_exact(torch, Y, (cols.ref1 if beta else cols.ref0)[:, :k], f"{what} k={k} beta={beta}")


def _band(n, half, inner=3):
    """a banded pattern: the diagonal, `inner` near neighbours on each side and the two far diagonals at +-half"""
    offs = sorted(set([-half, half] + list(range(-inner, inner + 1))))
    rows = np.arange(n)
    cols = rows[:, None] + np.array(offs)[None, :]
    ok = (cols >= 0) & (cols < n)
    rp = np.concatenate([[0], np.cumsum(ok.sum(axis=1))]).astype(np.int32)
    ci = cols[ok].astype(np.int32)
    va = np.random.default_rng(half).uniform(-1, 1, ci.size)
    return rp, ci, va


@pytest.mark.parametrize("dtype", (np.float64, np.float32), ids=("f64", "f32"))
@pytest.mark.parametrize("split,group", SHAPES, ids=[f"w{s}x{g}" for s, g in SHAPES])
@pytest.mark.parametrize("conv", (1, 2), ids=("gpu_builder", "host_builder"))
def test_cant_twin_bit_identical_per_column(eng, torch, dtype, split, group, conv):
    for scale in (0.1, 0.25):
        A = H.gen_named("cant", scale)
        rp, ci, va, m, n = A["row_ptr"], A["col_idx"], A["values"], A["m"], A["n"]
        M = _window(eng, rp, ci, va, m, n, dtype, split, group, convert_on=conv)
        _check_bit_identity(torch, M, 31, f"cant {scale} {np.dtype(dtype).name} {split}x{group} convert_on={conv}", (rp, ci, va), split, group)
        M.close()


@pytest.mark.parametrize("dtype", (np.float64, np.float32), ids=("f64", "f32"))
@pytest.mark.parametrize("split,group", SHAPES, ids=[f"w{s}x{g}" for s, g in SHAPES])
def test_stencil27_bit_identical_per_column(eng, torch, dtype, split, group):
    rp, ci, va, m = stencil27(24)
    rp = rp.astype(np.int32)
    for conv in (1, 2):
        M = _window(eng, rp, ci, va, m, m, dtype, split, group, convert_on=conv)
        _check_bit_identity(torch, M, 27, f"stencil27 24^3 {np.dtype(dtype).name} {split}x{group} convert_on={conv}", (rp, ci, va), split, group)
        M.close()


@pytest.mark.parametrize("case", ["empty_rows_formats", "empty_tail", "general_real", "rectangular", "tiny"])
@pytest.mark.parametrize("split,group", SHAPES, ids=[f"w{s}x{g}" for s, g in SHAPES])
def test_golden_cases_bit_identical_per_column(eng, torch, case, split, group):
    """empty rows (padding that points at the spare LDS slot), m % 64 != 0, m != n"""
    info, g = load_case(case)
    rp, ci, a = g["row_ptr"], g["col_idx"], g["values"]
    m, n = info["m"], info["n"]
    for dtype in (np.float64, np.float32):
        for conv in (1, 2):
            M = _window(eng, rp, ci, a, m, n, dtype, split, group, convert_on=conv)
            _check_bit_identity(torch, M, 7, f"{case} {np.dtype(dtype).name} {split}x{group} convert_on={conv}", (rp, ci, a), split, group,
                                ks=(1, 2, 3, 5, 8, 16))
            M.close()


@pytest.mark.parametrize("dtype", (np.float64, np.float32), ids=("f64", "f32"))
@pytest.mark.parametrize("split,group", [(1, 8), (4, 4)], ids=("w1x8", "w4x4"))
def test_strides_and_sentinels(eng, torch, dtype, split, group):
    """X at the start of a wider tensor or one element into it, odd and even ldx, Y with ldy > k: the gap columns of Y and the rows
    after rows() keep their sentinels bit for bit"""
    A = H.gen_named("cant", 0.1)
    rp, ci, va, m, n = A["row_ptr"], A["col_idx"], A["values"], A["m"], A["n"]
    M = _window(eng, rp, ci, va, m, n, dtype, split, group)
    cols = _make_columns(torch, M, 5, (rp, ci, va))
    assert cols.det
    dt = cols.X.dtype
    sent = torch.full((1,), SENTINEL, dtype=dt, device="cuda")
    for k in (1, 2, 3, 4, 8, 9):
        for ldx in (k, k + 1, 2 * k + 3):
            for x0 in (0, 1):
                for ldy in (k, k + 3):
                    for beta in (0, 1):
                        Xw = torch.full((n * ldx + x0 + 1,), SENTINEL, dtype=dt, device="cuda")
                        Xv = Xw[x0:x0 + n * ldx].view(n, ldx)
                        Xv[:, :k] = cols.X[:, :k]
                        Yw = torch.full((m + 3, ldy), SENTINEL, dtype=dt, device="cuda")
                        if beta:
                            Yw[:m, :k] = cols.Y0[:, :k]
                        M.spmm_device(k, Xv.data_ptr(), ldx, Yw.data_ptr(), ldy, beta)
                        torch.cuda.synchronize()
                        what = f"{M.format_name} k={k} ldx={ldx} x0={x0} ldy={ldy} beta={beta}"
                        _assert_exact(torch, Yw[:m, :k], (cols.ref1 if beta else cols.ref0)[:, :k], what)
                        assert bool((Yw[:m, k:] == sent).all()) and bool((Yw[m:] == sent).all()), f"{what}: a sentinel of Y changed"
    M.close()


def test_plan_narrow_window(eng):
    """regime 1: every K up to 8 fits LDS"""
    A = H.gen_named("cant", 0.1)
    rp, ci, va, m, n = A["row_ptr"], A["col_idx"], A["values"], A["m"], A["n"]
    for dtype in (np.float64, np.float32):
        M = _window(eng, rp, ci, va, m, n, dtype, 4, 4)
        kmax, wmax = _expected_kmax(M, 4, 4)
        assert kmax == 8, f"cant 0.1: window of {wmax} columns gives Kmax {kmax}, the case no longer tests the 8-column regime"
        assert M.spmm_plan(8) == (1, 8)
        assert M.spmm_plan(7) == (3, 4)
        assert M.spmm_plan(16) == (2, 8)
        assert M.spmm_plan(1) == (1, 1)
        M.close()


@pytest.mark.parametrize("dtype,kmax_want,plan5", [(np.float64, 1, (5, 1)), (np.float32, 2, (3, 2))], ids=("f64", "f32"))
def test_plan_and_products_wide_window(eng, torch, dtype, kmax_want, plan5):
    """regimes 2 and 3: one band pattern (1024-row groups, far diagonals at +-5000: windows of 11 024 columns) on which fp64 serves one
    column per pass, through the strided kernel, and fp32 two"""
    n = 24000
    rp, ci, va = _band(n, 5000)
    M = _window(eng, rp, ci, va, n, n, dtype, 1, 16)
    kmax, wmax = _expected_kmax(M, 1, 16)
    assert kmax == kmax_want, f"window of {wmax} columns gives Kmax {kmax}, not the regime this case is for"
    assert M.spmm_plan(5) == plan5
    assert M.spmm_plan(1) == (1, 1) and M.spmm_plan(2) == _expected_plan(kmax, 2)
    cols = _make_columns(torch, M, 50, (rp, ci, va))
    assert cols.det
    for k in (5, 2, 3):
        for beta in (0, 1):
            Y = _spmm(torch, M, cols, k, beta)
            _assert_exact(torch, Y, (cols.ref1 if beta else cols.ref0)[:, :k], f"{M.format_name} k={k} beta={beta}")
    M.close()


def test_plan_of_the_other_layouts(eng):
    A = H.gen_named("cant", 0.1)
    rp, ci, va, m, n = A["row_ptr"], A["col_idx"], A["values"], A["m"], A["n"]
    D = eng.Matrix(rp, ci, va, m, n, "sell_c_sigma", np.float64, sell_window=2)
    assert "SELLD" in D.format_name, D.format_name
    assert D.spmm_plan(7) == (3, 4) and D.spmm_plan(16) == (2, 8) and D.spmm_plan(1) == (1, 1)
    D.close()
    for fmt, opts in (("csr_vector", {}), ("csr_scalar", {}), ("sell_c_sigma", {"sell_c": 256})):
        V = eng.Matrix(rp, ci, va, m, n, fmt, np.float64, **opts)
        for k in (1, 5, 16):
            assert V.spmm_plan(k) == (k, 1), (fmt, k)
        V.close()
    # a handle without entries streams nothing
    rp0 = np.array([0, 2, 3, 5], np.int32)
    ci0 = np.array([0, 1, 1, 0, 1], np.int32)
    E0 = eng.Matrix(rp0, ci0, np.ones(5), 3, 4, "sell_c_sigma", np.float64, col_begin=2, col_end=4, col_filter_mode=1)
    assert E0.nnz == 0
    assert E0.spmm_plan(1) == (0, 0) and E0.spmm_plan(8) == (0, 0)
    E0.close()
    with pytest.raises(eng.SpmvError, match="spmm_plan"):
        D2 = eng.Matrix(rp, ci, va, m, n, "csr_scalar", np.float64)
        try:
            D2.spmm_plan(0)
        finally:
            D2.close()


def test_multi_rhs_solvers_on_the_default_handle(eng):
    """the 40^3 stencil with no layout options is a window handle: pcg_multi and pbicgstab_multi at k = 4 run one pass per SpMM and
    return the single solves bit for bit"""
    rp, ci, va, m = stencil27(40)
    rp = rp.astype(np.int32)
    M = eng.Matrix(rp, ci, va, m, m, "sell_c_sigma")
    assert "SELLW" in M.format_name, M.format_name
    assert M.spmm_plan(4) == (1, 4)
    B = np.ascontiguousarray(np.random.default_rng(40).uniform(0.5, 1.5, (m, 4)))
    for method, iters in (("pcg", 400), ("pbicgstab", 120)):
        single = getattr(M, method)
        want = [single(rp, ci, va, B[:, j].copy(), iters) for j in range(4)]
        assert all(w["iterations"] > 0 for w in want)
        got = getattr(M, method + "_multi")(rp, ci, va, B, iters)
        for j in range(4):
            _assert_same(got[j], want[j], f"{M.format_name} {method} column {j}")
    M.close()


@pytest.mark.parametrize("dtype", (np.float64, np.float32), ids=("f64", "f32"))
def test_host_path_and_second_stream(eng, torch, dtype):
    """spmv_mi355x_spmm on numpy arrays = the device path; a second stream gives the same bits"""
    A = H.gen_named("cant", 0.1)
    rp, ci, va, m, n = A["row_ptr"], A["col_idx"], A["values"], A["m"], A["n"]
    M = _window(eng, rp, ci, va, m, n, dtype, 2, 4)
    X = np.random.default_rng(8).uniform(-1, 1, (n, 6)).astype(dtype)
    Yh = M.spmm(X)
    Xt = torch.from_numpy(X).cuda()
    Yt = torch.empty((m, 6), dtype=Xt.dtype, device="cuda")
    s = torch.cuda.current_stream()
    M.spmm_device(6, Xt.data_ptr(), 6, Yt.data_ptr(), 6, 0, s.cuda_stream)
    s.synchronize()
    np.testing.assert_array_equal(Yt.cpu().numpy(), Yh)
    for j in range(6):
        np.testing.assert_array_equal(Yh[:, j], M.spmv(X[:, j]), err_msg=f"column {j}")
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        Y2 = torch.zeros((m, 6), dtype=Xt.dtype, device="cuda")
        M.spmm_device(6, Xt.data_ptr(), 6, Y2.data_ptr(), 6, 0, side.cuda_stream)
    side.synchronize()
    assert torch.equal(Y2, Yt)
    M.close()
