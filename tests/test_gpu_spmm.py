"""Y = A X for k vectors at once (spmv_mi355x_spmm_device_async, spmv_mi355x_spmm; kernels_sell_spmm.hip): on the SELL delta layout
every column of Y is bit-identical to the single-vector product of that column, for every value store, index mode, slice width,
waves per slice, builder, k and beta; strided X and Y touch nothing outside the k columns; every other layout runs per column and
matches the single-vector product; the host-buffer and torch paths agree; empty handles and bad arguments behave."""
import ctypes

import numpy as np
import pytest

import oracle
import spmv_host as H
from conftest import load_case
from test_gpu_parity import SENTINEL, compare_device_result

pytestmark = pytest.mark.gpu

KS = (1, 2, 3, 4, 5, 7, 8, 9, 16)
KMAX = max(KS)


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


@pytest.fixture
def modes_off():
    """Sets SPMV_MI355X_SELL_MODES_OFF for the handles created inside (read at every create())."""
    import os
    old = os.environ.get("SPMV_MI355X_SELL_MODES_OFF")

    def set_(v):
        os.environ["SPMV_MI355X_SELL_MODES_OFF"] = str(v)
    yield set_
    if old is None:
        os.environ.pop("SPMV_MI355X_SELL_MODES_OFF", None)
    else:
        os.environ["SPMV_MI355X_SELL_MODES_OFF"] = old


def _tdtype(torch, dtype):
    return torch.float64 if np.dtype(dtype) == np.float64 else torch.float32


def _six_slices(rng, w, n, m_cut=5):
    """One slice per index mode (affine, lane offsets, lane offsets with exceptions, 8-bit, 16-bit and 32-bit deltas) when every
    index-free mode is allowed, rows of w entries; the last `m_cut` rows are dropped (m not a multiple of 64)."""
    cols = []
    first = np.arange(64) + 7
    cols.append(first[:, None] + np.sort(rng.choice(4000, w, replace=False))[None, :])
    first = rng.permutation(64) * 3 + 20011
    steps = np.sort(rng.choice(4000, w, replace=False)) * 200
    cols.append(first[:, None] + steps[None, :])
    c = first[:, None] + steps[None, :] + 900000
    if w > 1:
        c[5, 1:] += np.arange(1, w) % 3 + 1
    cols.append(c)
    for span in (250, 60000, n - 10):
        base = rng.integers(0, n - span - 1)
        cols.append(np.sort(np.stack([rng.choice(span, w, replace=False) for _ in range(64)]), axis=1) + base)
    cols = np.sort(np.concatenate(cols), axis=1)
    m = cols.shape[0] - m_cut
    rp = (np.arange(m + 1) * w).astype(np.int32)
    return rp, cols[:m].reshape(-1).astype(np.int32), m


def _values(rng, m, w):
    """the nlpkkt twin's kind of values (exponents 1021 .. 1025: every full group qualifies for 7-byte storage)"""
    a = rng.uniform(0.25, 1.0, (m, w)) * rng.choice([-1.0, 1.0], (m, w))
    a[rng.uniform(size=(m, w)) < 0.1] = 4.0
    return a.reshape(-1)


class Columns:
    """X (n x KMAX) and Y0 (m x KMAX) on the device, and the single-vector products of every column: ref0[:, j] = A x_j,
    ref1[:, j] = y0_j + A x_j as spmv_device(beta = 1) computes it. The bit-identity contract of spmm is stated against these, so they
    come from the handle under test — and are themselves held to the oracle's product of `csr` = (row_ptr, col_idx, values), with
    the bound of test_gpu_parity.compare_device_result, before anything is compared with them."""

    def __init__(self, torch, M, X, Y0, csr):
        self.X, self.Y0 = X, Y0
        self.ref0 = torch.empty_like(Y0)
        self.ref1 = torch.empty_like(Y0)
        self.det = True
        rp, ci, a = csr
        dtype = M.dtype.type
        for j in range(X.shape[1]):
            x = X[:, j].contiguous()
            y = torch.full((M.m + 64,), SENTINEL, dtype=X.dtype, device="cuda")
            M.spmv_device(x.data_ptr(), y.data_ptr(), 0)
            y2 = torch.empty_like(y)
            M.spmv_device(x.data_ptr(), y2.data_ptr(), 0)
            torch.cuda.synchronize()
            self.det = self.det and bool(torch.equal(y[:M.m], y2[:M.m]))
            self.ref0[:, j] = y[:M.m]
            y1 = torch.full_like(y, SENTINEL)
            y1[:M.m] = Y0[:, j]
            M.spmv_device(x.data_ptr(), y1.data_ptr(), 1)
            torch.cuda.synchronize()
            self.ref1[:, j] = y1[:M.m]
            xj = x.cpu().numpy()
            y_ref = oracle.csr_spmv(rp, ci, a, xj, dtype)
            absrow = oracle.csr_spmv(rp, ci, np.abs(a), np.abs(xj).astype(np.float64))
            what = f"{M.format_name} single-vector product of column {j}"
            compare_device_result(y.cpu().numpy(), None, y_ref, absrow, 0, M.m, dtype, False, what + ", beta = 0")
            compare_device_result(y1.cpu().numpy(), Y0[:, j].cpu().numpy(), y_ref, absrow, 0, M.m, dtype, False, what + ", beta = 1")


def _make_columns(torch, M, seed, csr):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    dt = _tdtype(torch, M.dtype)
    X = (torch.rand((M.n, KMAX), generator=g, device="cuda", dtype=torch.float64) * 2 - 1).to(dt)
    Y0 = (torch.rand((M.m, KMAX), generator=g, device="cuda", dtype=torch.float64) * 2 - 1).to(dt)
    return Columns(torch, M, X, Y0, csr)


def _spmm(torch, M, cols, k, beta):
    X = cols.X[:, :k].contiguous()
    Y = cols.Y0[:, :k].contiguous() if beta else torch.full((M.m, k), SENTINEL, dtype=cols.X.dtype, device="cuda")
    M.spmm_device(k, X.data_ptr(), k, Y.data_ptr(), k, beta)
    torch.cuda.synchronize()
    return Y


def _assert_exact(torch, got, want, what):
    if not torch.equal(got, want):
        d = (got.double() - want.double()).abs()
        raise AssertionError(f"{what}: not bit-identical, {int((got != want).sum())} entries differ, max |d| {float(d.max())}")


def _check_delta_handle(torch, M, seed, what, csr, ks=KS):
    cols = _make_columns(torch, M, seed, csr)
    assert cols.det, what
    for k in ks:
        for beta in (0, 1):
            Y = _spmm(torch, M, cols, k, beta)
            _assert_exact(torch, Y, (cols.ref1 if beta else cols.ref0)[:, :k], f"{what} k={k} beta={beta}")


VALUE_STORES = [("f64", np.float64, 2), ("f64_v7", np.float64, 1), ("f32", np.float32, 0)]


@pytest.mark.parametrize("store", VALUE_STORES, ids=[s[0] for s in VALUE_STORES])
@pytest.mark.parametrize("split", (1, 2, 4))
def test_sell_delta_bit_identical_per_column(eng, torch, modes_off, store, split):
    """every index mode (with and without the index-free modes), slice widths 1..9 (tail groups of 1..3 steps), m % 64 != 0, n != m,
    host and GPU builder, k from 1 to 16, beta 0 and 1"""
    name, dtype, sell_values = store
    rng = np.random.default_rng(17 + split)
    n = 2_000_000
    for w in range(1, 10):
        rp, ci, m = _six_slices(rng, w, n)
        a = _values(rng, m, w)
        for off in (0, 7):
            modes_off(off)
            for conv in (1, 2):
                M = eng.Matrix(rp, ci, a, m, n, "sell_c_sigma", dtype, sell_c=64, sell_delta=1, sell_sigma=64, sell_split=split,
                               sell_window=2, sell_values=sell_values, convert_on=conv)
                if name == "f64_v7" and w >= 4:
                    assert M.format_name.endswith("_v7"), M.format_name
                _check_delta_handle(torch, M, w * 10 + off, f"{name} split={split} w={w} modes_off={off} convert_on={conv}", (rp, ci, a))
                M.close()


def test_sell_delta_from_stream(eng, torch):
    """a handle made by create_from_stream (the CSR assembled in device memory in pieces)"""
    A = H.gen_named("cant", 0.25)
    rp, ci, va, m, n = A["row_ptr"], A["col_idx"], A["values"], A["m"], A["n"]
    for dtype in (np.float64, np.float32):
        st = eng.CsrStream(m, n, int(rp[m]))
        for r0, r1 in ((0, m // 3), (m // 3, m // 3 + 1), (m // 3 + 1, m)):
            st.append(rp[r0:r1 + 1] - rp[r0], ci[rp[r0]:rp[r1]], va[rp[r0]:rp[r1]])
        S = st.finish("sell_c_sigma", dtype)
        _check_delta_handle(torch, S, 3, f"create_from_stream {np.dtype(dtype).name}", (rp, ci, va), ks=(1, 2, 4, 7, 8, 16))
        S.close()


@pytest.mark.parametrize("dtype", (np.float64, np.float32))
@pytest.mark.parametrize("fmt,opts,beta1_exact", [("sell_c_sigma", {"sell_c": 64, "sell_split": 1}, True), ("sell_c_sigma", {"sell_split": 2}, True),
                                                  ("csr_scalar", {}, True), ("csr_merge", {}, False)])
def test_strides_and_sentinels(eng, torch, dtype, fmt, opts, beta1_exact):
    """X at the start of a wider tensor or one element into it, with odd and even ldx, Y with ldy > k: the gap columns and the rows
    after rows() keep their sentinels bit for bit"""
    A = H.gen_named("cant", 0.1)
    rp, ci, va, m, n = A["row_ptr"], A["col_idx"], A["values"], A["m"], A["n"]
    M = eng.Matrix(rp, ci, va, m, n, fmt, dtype, **opts)
    cols = _make_columns(torch, M, 5, (rp, ci, va))
    dt = cols.X.dtype
    tol = 1e-10 if dt == torch.float64 else 1e-4
    sent = torch.full((1,), SENTINEL, dtype=dt, device="cuda")
    for k in (1, 2, 3, 4, 8, 9):
        for ldx in (k, k + 1, 2 * k + 3, k + 2):
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
                        what = f"{fmt}{opts} k={k} ldx={ldx} x0={x0} ldy={ldy} beta={beta}"
                        want = (cols.ref1 if beta else cols.ref0)[:, :k]
                        if cols.det and (beta == 0 or beta1_exact):
                            _assert_exact(torch, Yw[:m, :k], want, what)
                        else:
                            assert torch.allclose(Yw[:m, :k], want, rtol=tol, atol=tol), what
                        assert bool((Yw[:m, k:] == sent).all()) and bool((Yw[m:] == sent).all()), f"{what}: a sentinel of Y changed"
    M.close()


# every layout that spmm serves column by column, and whether spmv(beta = 1) is y + (A x) computed as spmm's column path computes it
OTHER_LAYOUTS = [
    ("csr_scalar", {}, True),
    ("csr_scalar", {"kahan": 1}, False),
    ("csr_vector", {}, True),
    ("csr_vector", {"lanes_per_row": 16, "rows_per_group": 4}, True),
    ("csr_stream", {}, False),
    ("csr_stream", {"stream_mode": 1, "lanes_per_row": 16}, False),
    ("csr_stream", {"stream_mode": 2, "lanes_per_row": 64}, False),
    ("csr_stream", {"stream_mode": 3}, False),
    ("csr_stream", {"stream_mode": 4}, False),
    ("csr_merge", {}, False),
    ("coo", {}, False),
    ("coo", {"col_blocks": -1}, False),
    ("csr_merge", {"col_blocks": -1}, False),
    ("sell_c_sigma", {"sell_c": 16, "sell_sigma": 16384}, True),
    ("sell_c_sigma", {"sell_c": 32, "sell_sigma": 256}, True),
    ("sell_c_sigma", {"sell_c": 256}, True),
    ("sell_c_sigma", {"sell_c": 64, "sell_delta": 2}, True),
    ("sell_c_sigma", {"sell_window": 1, "sell_split": 1}, False),
    ("sell_c_sigma", {"sell_window": 1, "sell_split": 2}, False),
]


@pytest.mark.parametrize("dtype", (np.float64, np.float32))
@pytest.mark.parametrize("fmt,opts,beta1_exact", OTHER_LAYOUTS, ids=[f + "".join(f":{k}={v}" for k, v in o.items()) for f, o, _ in OTHER_LAYOUTS])
def test_every_other_layout_per_column(eng, torch, dtype, fmt, opts, beta1_exact):
    A = H.gen_named("cant", 0.1)
    rp, ci, va, m, n = A["row_ptr"], A["col_idx"], A["values"], A["m"], A["n"]
    M = eng.Matrix(rp, ci, va, m, n, fmt, dtype, **opts)
    cols = _make_columns(torch, M, 9, (rp, ci, va))
    tol = 1e-10 if np.dtype(dtype) == np.float64 else 1e-4
    for k in (1, 3, 8):
        for beta in (0, 1):
            Y = _spmm(torch, M, cols, k, beta)
            want = (cols.ref1 if beta else cols.ref0)[:, :k]
            what = f"{M.format_name} {fmt}{opts} k={k} beta={beta}"
            if cols.det and (beta == 0 or beta1_exact):
                _assert_exact(torch, Y, want, what)
            else:
                assert torch.allclose(Y, want, rtol=tol, atol=tol), what
    M.close()


def test_symmetric_window_layout_per_column(eng, torch):
    """one triangle of a symmetric matrix in the LDS-window layout (mirrored entries through LDS atomics): to tolerance"""
    A = H.gen_named("cant", 0.25)
    rp, ci, va, m = A["row_ptr"], A["col_idx"], A["values"], A["m"]
    keep = np.concatenate([ci[rp[i]:rp[i + 1]] <= i for i in range(m)])
    lens = np.array([np.count_nonzero(ci[rp[i]:rp[i + 1]] <= i) for i in range(m)])
    trp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    M = eng.Matrix(trp, ci[keep], va[keep], m, m, "sell_c_sigma", np.float64, symmetric_input=1, sell_window=1)
    # what the handle multiplies by: the expansion T + T^t - diag T of the stored triangle
    import scipy.sparse as sp
    T = sp.csr_matrix((va[keep], ci[keep], trp), shape=(m, m))
    E = (T + sp.tril(T, -1).T).tocsr()
    E.sort_indices()
    cols = _make_columns(torch, M, 2, (E.indptr.astype(np.int32), E.indices.astype(np.int32), E.data.astype(np.float64)))
    for k in (1, 4, 5):
        for beta in (0, 1):
            Y = _spmm(torch, M, cols, k, beta)
            assert torch.allclose(Y, (cols.ref1 if beta else cols.ref0)[:, :k], rtol=1e-10, atol=1e-10), (M.format_name, k, beta)
    M.close()


@pytest.mark.parametrize("case", ["general_real", "rectangular", "empty_rows_formats", "huge_row", "tiny"])
@pytest.mark.parametrize("fmt,opts,exact", [("sell_c_sigma", {"sell_c": 64, "sell_split": 1}, True), ("sell_c_sigma", {"sell_split": 4}, False),
                                            ("csr_scalar", {}, True), ("csr_vector", {}, False), ("coo", {}, False)])
def test_golden_cases_against_the_csr_product(eng, case, fmt, opts, exact):
    info, g = load_case(case)
    rp, ci, a = g["row_ptr"], g["col_idx"], g["values"]
    m, n = info["m"], info["n"]
    X = np.random.default_rng(4).uniform(-1, 1, (n, 5))
    for dtype, tol in ((np.float64, 1e-12), (np.float32, 1e-5)):
        M = eng.Matrix(rp, ci, a, m, n, fmt, dtype, **opts)
        Y = M.spmm(X)
        assert Y.shape == (m, 5)
        for j in range(5):
            xj = np.ascontiguousarray(X[:, j])
            want = oracle.csr_spmv(rp, ci, a, xj, dtype, num_threads=1)
            absrow = oracle.csr_spmv(rp, ci, np.abs(a), np.abs(xj))
            if exact:
                np.testing.assert_array_equal(Y[:, j], want, err_msg=f"{case} {fmt}{opts} column {j}")
            err = np.abs(Y[:, j].astype(np.float64) - want.astype(np.float64))
            assert np.all(err <= tol * absrow + 1e-300), f"{case} {fmt}{opts} column {j}"
        M.close()


@pytest.mark.parametrize("fmt,opts", [("sell_c_sigma", {}), ("sell_c_sigma", {"sell_values": 1}), ("csr_vector", {})])
def test_host_and_torch_paths(eng, torch, fmt, opts):
    """spmv_mi355x_spmm on numpy arrays = the device path; (n, k) tensors on torch.cuda.current_stream() give the same"""
    A = H.gen_named("cant", 0.1)
    rp, ci, va, m, n = A["row_ptr"], A["col_idx"], A["values"], A["m"], A["n"]
    for dtype in (np.float64, np.float32):
        if opts.get("sell_values") and dtype == np.float32:
            continue
        M = eng.Matrix(rp, ci, va, m, n, fmt, dtype, **opts)
        X = np.random.default_rng(8).uniform(-1, 1, (n, 6)).astype(dtype)
        Yh = M.spmm(X)
        Xt = torch.from_numpy(X).cuda()
        Yt = torch.empty((m, 6), dtype=Xt.dtype, device="cuda")
        s = torch.cuda.current_stream()
        M.spmm_device(6, Xt.data_ptr(), 6, Yt.data_ptr(), 6, 0, s.cuda_stream)
        s.synchronize()
        np.testing.assert_array_equal(Yt.cpu().numpy(), Yh, err_msg=f"{fmt}{opts} {np.dtype(dtype).name}")
        for j in range(6):
            np.testing.assert_array_equal(Yh[:, j], M.spmv(X[:, j]), err_msg=f"{fmt}{opts} column {j}")
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            Y2 = torch.zeros((m, 6), dtype=Xt.dtype, device="cuda")
            M.spmm_device(6, Xt.data_ptr(), 6, Y2.data_ptr(), 6, 0, side.cuda_stream)
        side.synchronize()
        assert torch.equal(Y2, Yt)
        ms = M.time_spmm_device(6, Xt.data_ptr(), 6, Y2.data_ptr(), 6, 3, s.cuda_stream)
        assert ms > 0
        torch.cuda.synchronize()
        assert torch.equal(Y2, Yt)
        M.close()


def test_empty_handle(eng, torch):
    """nnz == 0 (a column filter that keeps no entry): beta 0 zeroes the k columns and nothing else, beta 1 leaves Y alone"""
    rp = np.array([0, 2, 3, 5], np.int32)
    ci = np.array([0, 1, 1, 0, 1], np.int32)
    M = eng.Matrix(rp, ci, np.ones(5), 3, 4, "sell_c_sigma", np.float64, col_begin=2, col_end=4, col_filter_mode=1)
    assert M.nnz == 0 and M.m == 3
    X = torch.ones((4, 3), dtype=torch.float64, device="cuda")
    Y = torch.full((4, 5), SENTINEL, dtype=torch.float64, device="cuda")
    M.spmm_device(3, X.data_ptr(), 3, Y.data_ptr(), 5, 1)
    torch.cuda.synchronize()
    assert bool((Y == SENTINEL).all())
    M.spmm_device(3, X.data_ptr(), 3, Y.data_ptr(), 5, 0)
    torch.cuda.synchronize()
    assert bool((Y[:3, :3] == 0).all()) and bool((Y[:3, 3:] == SENTINEL).all()) and bool((Y[3:] == SENTINEL).all())
    np.testing.assert_array_equal(M.spmm(np.ones((M.n, 2))), np.zeros((3, 2)))


def test_argument_errors_leave_y_untouched(eng, torch):
    A = H.gen_named("cant", 0.05)
    M = eng.Matrix(A["row_ptr"], A["col_idx"], A["values"], A["m"], A["n"], "sell_c_sigma", np.float64)
    L = eng.lib()
    X = torch.ones((M.n, 4), dtype=torch.float64, device="cuda")
    Y = torch.full((M.m, 4), SENTINEL, dtype=torch.float64, device="cuda")
    xp, yp = ctypes.c_void_p(X.data_ptr()), ctypes.c_void_p(Y.data_ptr())
    cl, ci_ = ctypes.c_long, ctypes.c_int
    bad = [(M.h, 0, xp, 4, yp, 4), (M.h, -1, xp, 4, yp, 4), (M.h, 4, xp, 3, yp, 4), (M.h, 4, xp, 4, yp, 2), (None, 4, xp, 4, yp, 4),
           (M.h, 4, None, 4, yp, 4), (M.h, 4, xp, 4, None, 4)]
    for h, k, x, ldx, y, ldy in bad:
        assert L.spmv_mi355x_spmm_device_async(h, ci_(k), x, cl(ldx), y, cl(ldy), ci_(0), None) == 1
        assert b"spmm_device_async" in L.spmv_mi355x_last_error(), (k, ldx, ldy)
        ms = ctypes.c_double()
        assert L.spmv_mi355x_time_spmm_device(h, ci_(k), x, cl(ldx), y, cl(ldy), ci_(2), None, ctypes.byref(ms)) == 1
        assert b"time_spmm_device" in L.spmv_mi355x_last_error()
    torch.cuda.synchronize()
    assert bool((Y == SENTINEL).all())
    Yh = np.full((M.m, 2), SENTINEL)
    for h, k, x in ((M.h, 0, np.ones((M.n, 2))), (None, 2, np.ones((M.n, 2))), (M.h, 2, None)):
        assert L.spmv_mi355x_spmm(h, ci_(k), None if x is None else x.ctypes.data_as(ctypes.c_void_p), Yh.ctypes.data_as(ctypes.c_void_p)) == 1
        assert b"spmm" in L.spmv_mi355x_last_error()
    assert np.all(Yh == SENTINEL)
    with pytest.raises(ValueError):
        M.spmm(np.ones(M.n))
    M.close()


def test_full_size_nlpkkt240_k4(eng, torch):
    """the headline handle (bench.py's defaults for the nlpkkt240 twin, 7-byte values under auto) with k = 4: every column of one spmm
    is bit-identical to a single SpMV of that column"""
    import bench
    A, _ = bench.load_workload(H, "nlpkkt240", 1.0)
    rp, ci, va, m, n = A["row_ptr"], A["col_idx"], A["values"], A["m"], A["n"]
    M = eng.Matrix(rp, ci, va, m, n, bench.DEFAULT_FORMAT["nlpkkt240"], np.float64, **bench.DEFAULT_OPTS.get("nlpkkt240", {}))
    del A, rp, ci, va
    assert M.format_name.endswith("_v7"), M.format_name
    g = torch.Generator(device="cuda")
    g.manual_seed(240)
    X = torch.rand((n, 4), generator=g, device="cuda", dtype=torch.float64) * 2 - 1
    Y = torch.empty((m, 4), dtype=torch.float64, device="cuda")
    M.spmm_device(4, X.data_ptr(), 4, Y.data_ptr(), 4, 0)
    y = torch.empty(m + 64, dtype=torch.float64, device="cuda")
    for j in range(4):
        x = X[:, j].contiguous()
        M.spmv_device(x.data_ptr(), y.data_ptr(), 0)
        torch.cuda.synchronize()
        _assert_exact(torch, Y[:, j], y[:m], f"nlpkkt240 column {j}")
    M.close()
