"""opts.value_storage = 1 (include/spmv_mi355x.h "mixed precision"): fp32-stored values under fp64 vectors on the SELL delta layout.

The contract: on every variant of the layout (waves per slice, index modes, builder, beta, spmm of any k) the product of a mixed
handle is BIT-IDENTICAL to that of an fp64 handle (sell_values = 2) built from values.astype(float32).astype(float64); its stored
arrays are byte for byte those of the F32 handle. The fp64 handle of the rounded values is itself held to the oracle first, so the
chain mixed == rounded fp64 ~ oracle has no link that compares the engine only with itself.

Tolerances. |y_mixed - oracle(unrounded)| per row: every stored value is off by at most half an fp32 ulp, |a~ - a| <= 2^-24 |a|, so the
exact product of the rounded matrix is within 2^-24 * sum|a_ij||x_j| of the exact product of the unrounded one; on top of it comes
the fp64 evaluation error of both sides, for which compare_device_result's bound is used as it stands: TOL[float64] * sum|a x|
(beta = 1: * (sum|a x| + |y0|))."""
import functools

import numpy as np
import pytest

import oracle
from test_gpu_parity import SENTINEL, TOL, compare_device_result
from test_gpu_spmm import _six_slices, _values

pytestmark = pytest.mark.gpu

N = 2_000_000
WIDTHS = (1, 2, 3, 4, 5, 7, 8, 17)               # every tail length, odd and even pair counts, at least four full groups
DELTA = dict(sell_c=64, sell_delta=1, sell_sigma=64, sell_window=2)
U24 = 2.0 ** -24


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


def _round32(a):
    return a.astype(np.float32).astype(np.float64)


class Problem:
    """A matrix, x, y0 and the oracle's products, computed once: of the rounded values (what the fp64 reference handle is held to) and
    of the unrounded ones (what the mixed result is bounded against)."""

    def __init__(self, rp, ci, a, m, n, seed):
        self.rp, self.ci, self.a, self.m, self.n = rp, ci, a, m, n
        self.ar = _round32(a)
        assert np.count_nonzero(self.ar != a) > 0.8 * a.size, "the values must not be representable in fp32"
        rng = np.random.default_rng(seed)
        self.x = rng.uniform(-1, 1, n)
        self.y0 = rng.uniform(-1, 1, m) * 8
        self.ref_rounded = oracle.csr_spmv(rp, ci, self.ar, self.x, np.float64)
        self.abs_rounded = oracle.csr_spmv(rp, ci, np.abs(self.ar), np.abs(self.x))
        self.ref_full = oracle.csr_spmv(rp, ci, a, self.x, np.float64)
        self.abs_full = oracle.csr_spmv(rp, ci, np.abs(a), np.abs(self.x))
        for v in (self.ar, self.x, self.y0, self.ref_rounded, self.abs_rounded, self.ref_full, self.abs_full):
            v.setflags(write=False)


@functools.lru_cache(maxsize=None)
def six_slice_problem(w):
    rng = np.random.default_rng(100 + w)
    rp, ci, m = _six_slices(rng, w, N)
    assert m % 64 != 0
    return Problem(rp, ci, _values(rng, m, w), m, N, 200 + w)


class Device:
    """x one element into its buffer, y three elements into a buffer of sentinels (odd element offsets)."""
    OX, G0, G1 = 1, 3, 2

    def __init__(self, torch, P):
        self.torch, self.P = torch, P
        self.xbuf = torch.full((self.OX + P.n,), SENTINEL, dtype=torch.float64, device="cuda")
        self.xbuf[self.OX:] = torch.from_numpy(P.x.copy()).cuda()

    def run(self, M, beta):
        """the y buffer [G0 guards | m values | G1 guards] after y = A x / y0 += A x, as a host array"""
        t, P = self.torch, self.P
        ybuf = t.full((self.G0 + P.m + self.G1,), SENTINEL, dtype=t.float64, device="cuda")
        if beta:
            ybuf[self.G0:self.G0 + P.m] = t.from_numpy(P.y0.copy()).cuda()
        t.cuda.synchronize()
        M.spmv_device(self.xbuf.data_ptr() + 8 * self.OX, ybuf.data_ptr() + 8 * self.G0, beta)
        t.cuda.synchronize()
        return ybuf.cpu().numpy()


def check_parity(eng, D, opts, what, unrounded_too=True):
    """mixed == fp64 handle of the rounded values (itself held to the oracle), != fp64 handle of the unrounded values, and within the
    derived bound of the oracle's product of the unrounded values"""
    P = D.P
    Mx = eng.Matrix(P.rp, P.ci, P.a, P.m, P.n, "sell_c_sigma", np.float64, value_storage=1, **opts)
    Mr = eng.Matrix(P.rp, P.ci, P.ar, P.m, P.n, "sell_c_sigma", np.float64, sell_values=2, **opts)
    Mu = eng.Matrix(P.rp, P.ci, P.a, P.m, P.n, "sell_c_sigma", np.float64, sell_values=2, **opts) if unrounded_too else None
    assert Mx.format_name == Mr.format_name + "_v4", (Mx.format_name, Mr.format_name)
    assert Mx.value_dtype == np.float32 and Mx.dtype == np.float64 and Mr.value_dtype == np.float64
    assert "mixed" in Mx.kernel_info()["name"] and "mixed" not in Mr.kernel_info()["name"]
    g0 = D.G0
    for beta in (0, 1):
        tag = f"{what} beta={beta}"
        y0 = P.y0 if beta else None
        yr = D.run(Mr, beta)
        compare_device_result(yr, y0, P.ref_rounded, P.abs_rounded, g0, P.m, np.float64, False, tag + " fp64 handle of the rounded values")
        yx = D.run(Mx, beta)
        bad = np.nonzero(yx.view(np.uint64) != yr.view(np.uint64))[0]
        assert bad.size == 0, f"{tag}: mixed handle differs from the fp64 handle of the rounded values at {bad.size} places, first {bad[:5] - g0}"
        y = yx[g0:g0 + P.m]
        want = P.ref_full if y0 is None else y0 + P.ref_full
        bound = U24 * P.abs_full + TOL[np.float64] * (P.abs_full + (0 if y0 is None else np.abs(y0)))
        err = np.abs(y - want)
        print(f"{tag}: max |y - unrounded reference| / bound = {float((err / np.maximum(bound, 1e-300)).max()):.3f}")
        worst = np.nonzero(err > bound)[0]
        assert worst.size == 0, f"{tag}: {worst.size} rows beyond 2^-24 sum|a x| + the fp64 bound; row {worst[:5]} err {err[worst[:5]]} bound {bound[worst[:5]]}"
        if Mu is not None:
            yu = D.run(Mu, beta)
            assert np.count_nonzero(yu[g0:g0 + P.m] != y) > 0, f"{tag}: the mixed product equals that of the unrounded values: nothing was narrowed"
    for M in (Mx, Mr, Mu):
        if M is not None:
            M.close()


# ---- 1. parity -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("split", (1, 2, 4))
def test_parity_on_every_variant(eng, torch, modes_off, split):
    for w in WIDTHS:
        D = Device(torch, six_slice_problem(w))
        for off in (0, 7):
            modes_off(off)
            for conv in (1, 2):
                check_parity(eng, D, dict(DELTA, sell_split=split, convert_on=conv), f"w={w} split={split} modes_off={off} convert_on={conv}",
                             unrounded_too=(conv == 1))


# ---- 2. layout -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("conv", (1, 2))
def test_stored_arrays_are_the_f32_handles(eng, modes_off, conv):
    for w, off in ((5, 0), (8, 0), (17, 7)):
        modes_off(off)
        P = six_slice_problem(w)
        opts = dict(DELTA, sell_split=1, convert_on=conv)
        Mx = eng.Matrix(P.rp, P.ci, P.a, P.m, P.n, "sell_c_sigma", np.float64, value_storage=1, **opts)
        Mf = eng.Matrix(P.rp, P.ci, P.a, P.m, P.n, "sell_c_sigma", np.float32, **opts)
        Md = eng.Matrix(P.rp, P.ci, P.a, P.m, P.n, "sell_c_sigma", np.float64, sell_values=2, **opts)
        assert eng.lib().spmv_mi355x_value_storage(Mx.h) == eng.F32 and eng.lib().spmv_mi355x_precision(Mx.h) == eng.F64
        assert eng.lib().spmv_mi355x_value_storage(Mf.h) == eng.F32 and eng.lib().spmv_mi355x_value_storage(Md.h) == eng.F64
        lx, lf = Mx.sell_layout(), Mf.sell_layout()
        for key in ("C", "sigma", "num_slices", "nnz_ext"):
            assert lx[key] == lf[key], key
        for key in ("slice_ptr", "col", "row_of_sorted", "val"):
            np.testing.assert_array_equal(lx[key], lf[key], err_msg=f"w={w} convert_on={conv}: {key}")
        assert np.array_equal(lx["val"], _round32(lx["val"])) and np.count_nonzero(lx["val"]) == P.a.size
        for name in ("val", "idx", "desc", "row_of_sorted"):
            np.testing.assert_array_equal(Mx.stored_array(name), Mf.stored_array(name), err_msg=f"w={w} convert_on={conv}: stored {name}")
        assert Mx.mem_footprint == Mf.mem_footprint < Md.mem_footprint
        assert Mx.csr_mem_footprint == Md.csr_mem_footprint > Mf.csr_mem_footprint
        for M in (Mx, Mf, Md):
            M.close()


# ---- 3. SpMM ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("split", (1, 2, 4))
def test_spmm_columns_are_the_single_vector_products(eng, torch, split):
    P = six_slice_problem(7)
    opts = dict(DELTA, sell_split=split)
    Mx = eng.Matrix(P.rp, P.ci, P.a, P.m, P.n, "sell_c_sigma", np.float64, value_storage=1, **opts)
    Md = eng.Matrix(P.rp, P.ci, P.ar, P.m, P.n, "sell_c_sigma", np.float64, sell_values=2, **opts)
    KMAX = 9
    g = torch.Generator(device="cuda")
    g.manual_seed(5)
    X = torch.rand((P.n, KMAX), generator=g, device="cuda", dtype=torch.float64) * 2 - 1
    Y0 = torch.rand((P.m, KMAX), generator=g, device="cuda", dtype=torch.float64) * 2 - 1
    ref = [torch.empty_like(Y0), torch.empty_like(Y0)]
    for j in range(KMAX):
        x = X[:, j].contiguous()
        for beta in (0, 1):
            for M in (Mx, Md):
                y = torch.full((P.m + 2,), SENTINEL, dtype=torch.float64, device="cuda")
                if beta:
                    y[:P.m] = Y0[:, j]
                M.spmv_device(x.data_ptr(), y.data_ptr(), beta)
                torch.cuda.synchronize()
                if M is Mx:
                    ref[beta][:, j] = y[:P.m]
                else:                                     # the single-vector reference itself: the fp64 handle of the rounded values
                    assert torch.equal(y[:P.m], ref[beta][:, j]), f"column {j} beta={beta}"
        if j == 0:
            xj = x.cpu().numpy()
            compare_device_result(np.append(ref[0][:, 0].cpu().numpy(), SENTINEL), None, oracle.csr_spmv(P.rp, P.ci, P.ar, xj, np.float64),
                                  oracle.csr_spmv(P.rp, P.ci, np.abs(P.ar), np.abs(xj)), 0, P.m, np.float64, False, "single-vector product of column 0")
    sent = torch.full((1,), SENTINEL, dtype=torch.float64, device="cuda")
    for k in (1, 2, 3, 4, 5, 8, 9):
        assert Mx.spmm_plan(k) == Md.spmm_plan(k), k
        for ldx, x0, ldy in ((k + 1, 1, k + 3), (k + 2, 0, k + 1)):
            for beta in (0, 1):
                Xw = torch.full((P.n * ldx + x0 + 1,), SENTINEL, dtype=torch.float64, device="cuda")
                Xv = Xw[x0:x0 + P.n * ldx].view(P.n, ldx)
                Xv[:, :k] = X[:, :k]
                Yw = torch.full((P.m + 3, ldy), SENTINEL, dtype=torch.float64, device="cuda")
                if beta:
                    Yw[:P.m, :k] = Y0[:, :k]
                Mx.spmm_device(k, Xv.data_ptr(), ldx, Yw.data_ptr(), ldy, beta)
                torch.cuda.synchronize()
                what = f"split={split} k={k} ldx={ldx} x0={x0} ldy={ldy} beta={beta}"
                assert torch.equal(Yw[:P.m, :k], ref[beta][:, :k]), f"{what}: a column is not the single-vector product"
                assert bool((Yw[:P.m, k:] == sent).all()) and bool((Yw[P.m:] == sent).all()), f"{what}: a guard of Y changed"
    # the host-buffer forms
    Xh = X[:, :5].cpu().numpy()
    np.testing.assert_array_equal(Mx.spmm(Xh), ref[0][:, :5].cpu().numpy())
    np.testing.assert_array_equal(Mx.spmv(np.ascontiguousarray(Xh[:, 2])), ref[0][:, 2].cpu().numpy())
    Mx.close()
    Md.close()


# ---- 4. stream -------------------------------------------------------------------------------------------------------------------

def test_from_stream(eng, torch):
    P = six_slice_problem(5)
    m, rp, ci = P.m, P.rp, P.ci
    st = eng.CsrStream(m, P.n, int(rp[m]))
    for r0, r1 in ((0, m // 3), (m // 3, m // 3 + 1), (m // 3 + 1, m)):
        st.append(rp[r0:r1 + 1] - rp[r0], ci[rp[r0]:rp[r1]], P.a[rp[r0]:rp[r1]])
    S = st.finish("sell_c_sigma", np.float64, value_storage=1, sell_sigma=64, sell_split=2)
    M = eng.Matrix(rp, ci, P.a, m, P.n, "sell_c_sigma", np.float64, value_storage=1, sell_sigma=64, sell_split=2, sell_window=2)
    assert S.format_name == M.format_name and S.format_name.endswith("_v4")
    assert S.value_dtype == np.float32 and S.dtype == np.float64 and S.mem_footprint == M.mem_footprint
    ls, lm = S.sell_layout(), M.sell_layout()
    for key in ("slice_ptr", "col", "row_of_sorted", "val"):
        np.testing.assert_array_equal(ls[key], lm[key], err_msg=key)
    D = Device(torch, P)
    for beta in (0, 1):
        ys, ym = D.run(S, beta), D.run(M, beta)
        compare_device_result(ys, P.y0 if beta else None, P.ref_rounded, P.abs_rounded, D.G0, m, np.float64, False, f"from stream beta={beta}")
        np.testing.assert_array_equal(ys.view(np.uint64), ym.view(np.uint64))
    S.close()
    M.close()


# ---- 5. the automatic layout choice --------------------------------------------------------------------------------------------------

def test_automatic_layout_goes_to_the_delta_layout(eng, torch):
    m, w = 65536, 17
    rng = np.random.default_rng(9)
    start = np.clip(np.arange(m) - 150, 0, m - 301)
    ci = np.sort(np.stack([rng.choice(300, w, replace=False) for _ in range(64)]), axis=1)[np.arange(m) % 64] + start[:, None]
    rp = (np.arange(m + 1) * w).astype(np.int32)
    ci = ci.reshape(-1).astype(np.int32)
    P = Problem(rp, ci, _values(rng, m, w), m, m, 10)
    default = eng.Matrix(rp, ci, P.a, m, m, "sell_c_sigma", np.float64)
    assert default.format_name.startswith("MI355X_SELLW_"), f"{default.format_name}: the default must be the LDS-window layout for this case to mean anything"
    default.close()
    Mx = eng.Matrix(rp, ci, P.a, m, m, "sell_c_sigma", np.float64, value_storage=1)
    assert Mx.format_name.startswith("MI355X_SELLD_64_") and Mx.format_name.endswith("_d_v4"), Mx.format_name
    Mx.close()
    check_parity(eng, Device(torch, P), dict(sell_window=2), "banded, automatic options")


# ---- 6. solvers ------------------------------------------------------------------------------------------------------------------

def test_solvers_run_unchanged(eng):
    import scipy.sparse as sp
    k = 12
    rng = np.random.default_rng(4)
    T1 = sp.diags([-np.ones(k - 1), np.zeros(k), -np.ones(k - 1)], [-1, 0, 1])
    I = sp.eye(k)
    L = (sp.kron(sp.kron(T1, I), I) + sp.kron(sp.kron(I, T1), I) + sp.kron(sp.kron(I, I), T1)).tocoo()
    keep = L.row < L.col
    U = sp.coo_matrix((L.data[keep] * rng.uniform(0.5, 1.0, int(keep.sum())), (L.row[keep], L.col[keep])), shape=L.shape)
    A = (U + U.T).tocsr()                                                    # symmetric, perturbed off-diagonal entries
    A = (A + sp.diags(np.asarray(abs(A).sum(axis=1)).ravel() * rng.uniform(1.1, 1.3, k ** 3))).tocsr()   # diagonally dominant: SPD
    A.sort_indices()
    m = k ** 3
    rp, ci, a = A.indptr.astype(np.int32), A.indices.astype(np.int32), A.data.astype(np.float64)
    ar = _round32(a)
    assert np.count_nonzero(ar != a) > 0.9 * a.size
    B = rng.uniform(0.5, 1.5, (m, 3))
    Mx = eng.Matrix(rp, ci, a, m, m, "sell_c_sigma", np.float64, value_storage=1, sell_window=2)
    Mr = eng.Matrix(rp, ci, ar, m, m, "sell_c_sigma", np.float64, sell_values=2, sell_window=2)
    Mu = eng.Matrix(rp, ci, a, m, m, "sell_c_sigma", np.float64, sell_values=2, sell_window=2)

    def same(got, want, what):
        for key in want:
            if key == "seconds":                                     # wall time of the solve: the one field that is no result
                continue
            if key in ("x", "history"):
                np.testing.assert_array_equal(got[key].view(np.uint64), want[key].view(np.uint64), err_msg=f"{what}: {key}")
            else:
                assert got[key] == want[key], f"{what}: {key} {got[key]!r} != {want[key]!r}"

    for name in ("pcg", "pbicgstab"):
        got, want = getattr(Mx, name)(rp, ci, ar, B[:, 0].copy(), 300), getattr(Mr, name)(rp, ci, ar, B[:, 0].copy(), 300)
        assert 0 < want["iterations"] <= 300 and want["history"].shape[0] == want["iterations"], name   # (the solvers may use every iteration)
        same(got, want, name)
        other = getattr(Mu, name)(rp, ci, ar, B[:, 0].copy(), 300)
        assert not np.array_equal(other["x"], got["x"]), f"{name}: the mixed handle multiplies with the unrounded values"
    got, want = Mx.pcg_multi(rp, ci, ar, B, 300), Mr.pcg_multi(rp, ci, ar, B, 300)
    for j in range(3):
        assert 0 < want[j]["iterations"] <= 300
        same(got[j], want[j], f"pcg_multi column {j}")
    for M in (Mx, Mr, Mu):
        M.close()


# ---- 7. fp32 vectors: the field is accepted and changes nothing ----------------------------------------------------------------------

def test_f32_precision_accepts_the_field(eng):
    P = six_slice_problem(5)
    x = P.x.astype(np.float32)
    for fmt, opts in (("sell_c_sigma", dict(DELTA, sell_split=2)), ("sell_c_sigma", dict(sell_c=32)), ("csr_vector", {})):
        Mv = eng.Matrix(P.rp, P.ci, P.a, P.m, P.n, fmt, np.float32, value_storage=1, **opts)
        Mf = eng.Matrix(P.rp, P.ci, P.a, P.m, P.n, fmt, np.float32, **opts)
        assert Mv.format_name == Mf.format_name and Mv.mem_footprint == Mf.mem_footprint
        assert Mv.value_dtype == np.float32 and Mv.dtype == np.float32
        y = Mv.spmv(x)
        np.testing.assert_array_equal(y, Mf.spmv(x), err_msg=fmt)
        absrow = P.abs_full
        assert np.all(np.abs(y - oracle.csr_spmv(P.rp, P.ci, P.a, x, np.float32)) <= TOL[np.float32] * absrow), fmt
        Mv.close()
        Mf.close()
