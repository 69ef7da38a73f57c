"""spmv_mi355x_update_values (include/spmv_mi355x.h "new values for an existing handle"): same pattern, new numbers.

The contract: a handle created from (pattern, V1, opts) and updated with V2 is indistinguishable from a handle freshly created from
(pattern, V2, opts) — every array spmv_mi355x_stored_array exposes is byte-identical, format_name / mem_footprint / sell_layout /
kernel_info / spmm_plan answer the same, and the products are bit-identical on every deterministic layout. The FRESH handle is itself
held to the oracle (compare_device_result) before anything is compared with it, so no link of the chain compares the engine only
with itself. The only tolerance used is test_gpu_parity.TOL through compare_device_result, on the fresh handles."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import oracle
from test_gpu_parity import ATOMIC_LAYOUTS, SENTINEL, TOL, compare_device_result
from test_gpu_spmm import _six_slices, _values
from test_gpu_value_storage import Device, _round32

pytestmark = pytest.mark.gpu

N = 2_000_000
WIDTHS = (1, 2, 3, 4, 5, 7, 8, 17)
DELTA = dict(sell_c=64, sell_delta=1, sell_sigma=64, sell_window=2)
STORED = {"delta": ("val", "idx", "desc", "row_of_sorted"), "window": ("val", "idx", "desc", "groups", "row_of_sorted"),
          "plain": ("val", "col", "slice_ptr", "row_of_sorted"), None: ()}


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


# ---- problems: one pattern, two value sets, x, y0, and the oracle's products (computed once, read-only) ------------------------------

class Case:
    def __init__(self, rp, ci, m, n, V1, V2, seed):
        self.rp, self.ci, self.m, self.n = rp, ci, m, n
        self.V = {1: V1, 2: V2}
        rng = np.random.default_rng(seed)
        self.x = rng.uniform(-1, 1, n)
        self.x[self.x == 0] = 0.5
        self.y0 = rng.uniform(-1, 1, m) * 8
        for v in (V1, V2, self.x, self.y0):
            v.setflags(write=False)
        self._refs = {}

    def stored(self, which, store):
        """the values a handle of value store `store` multiplies with, as fp64"""
        return _round32(self.V[which]) if store in ("f32", "mixed") else self.V[which]

    def refs(self, which, store):
        """(y_ref in the vectors' precision, sum |a x|) of the oracle for value set `which` as `store` keeps it"""
        key = (which, store)
        if key not in self._refs:
            dtype = np.float32 if store == "f32" else np.float64
            a = self.stored(which, store) if store == "mixed" else self.V[which]
            x = self.x.astype(dtype)
            self._refs[key] = (oracle.csr_spmv(self.rp, self.ci, a, x, dtype),
                               oracle.csr_spmv(self.rp, self.ci, np.abs(a), np.abs(x).astype(np.float64)))
        return self._refs[key]


class Dev:
    """test_gpu_value_storage.Device for either precision: x one element into its buffer, y three elements into a buffer of sentinels"""
    OX, G0, G1 = Device.OX, Device.G0, Device.G1

    def __init__(self, torch, case, dtype=np.float64):
        self.torch, self.c, self.dtype = torch, case, np.dtype(dtype).type
        self.tdt = torch.float64 if self.dtype == np.float64 else torch.float32
        self.item = np.dtype(dtype).itemsize
        self.xbuf = torch.full((self.OX + case.n,), SENTINEL, dtype=self.tdt, device="cuda")
        self.xbuf[self.OX:] = torch.from_numpy(case.x.astype(self.dtype)).cuda()
        self.y0 = case.y0.astype(self.dtype)

    def run(self, M, beta):
        t, c = self.torch, self.c
        ybuf = t.full((self.G0 + c.m + self.G1,), SENTINEL, dtype=self.tdt, device="cuda")
        if beta:
            ybuf[self.G0:self.G0 + c.m] = t.from_numpy(self.y0.copy()).cuda()
        t.cuda.synchronize()
        M.spmv_device(self.xbuf.data_ptr() + self.item * self.OX, ybuf.data_ptr() + self.item * self.G0, beta)
        t.cuda.synchronize()
        return ybuf.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _kind(M):
    n = M.format_name
    return "window" if "_SELLW_" in n else "delta" if "_SELLD_" in n else "plain" if "_SELL_" in n else None


def assert_same_handle(Mu, Mf, what):
    """everything a caller can ask a handle, of the updated handle against the fresh one"""
    assert Mu.format_name == Mf.format_name, f"{what}: format_name {Mu.format_name} != {Mf.format_name}"
    assert Mu.mem_footprint == Mf.mem_footprint, f"{what}: mem_footprint {Mu.mem_footprint} != {Mf.mem_footprint}"
    assert lib_name(Mu) == lib_name(Mf), what
    ku, kf = Mu.kernel_info(), Mf.kernel_info()
    assert (ku["name"], ku["block"]) == (kf["name"], kf["block"]), what
    for k in (1, 5, 9):
        assert Mu.spmm_plan(k) == Mf.spmm_plan(k), f"{what}: spmm_plan({k})"
    kind = _kind(Mf)
    for name in STORED[kind]:
        a, b = Mu.stored_array(name), Mf.stored_array(name)
        assert a.shape == b.shape, f"{what}: stored {name} has {a.size} bytes, the fresh handle's {b.size}"
        bad = np.nonzero(a != b)[0]
        assert bad.size == 0, f"{what}: stored {name} differs at {bad.size} bytes, first {bad[:5]}"
    if kind in ("delta", "plain"):
        lu, lf = Mu.sell_layout(), Mf.sell_layout()
        for key in ("C", "sigma", "num_slices", "nnz_ext"):
            assert lu[key] == lf[key], f"{what}: sell_layout {key}"
        for key in ("slice_ptr", "col", "row_of_sorted", "val"):
            assert _bits(lu[key]).tobytes() == _bits(lf[key]).tobytes(), f"{what}: sell_layout {key}"


def lib_name(M):
    import spmv_mi355x as E
    return E.lib().spmv_mi355x_format_name(M.h)            # the handle's own answer, not the binding's cached copy


def check_update(D, Mu, Mf, which, store, what):
    """the fresh handle Mf of value set `which` against the oracle; the updated handle Mu against Mf, bit for bit"""
    c = D.c
    y_ref, absrow = c.refs(which, store)
    assert_same_handle(Mu, Mf, what)
    for beta in (0, 1):
        tag = f"{what} beta={beta}"
        yf = D.run(Mf, beta)
        compare_device_result(yf, D.y0 if beta else None, y_ref, absrow, D.G0, c.m, D.dtype, False, tag + " fresh handle")
        yu = D.run(Mu, beta)
        bad = np.nonzero(_bits(yu).reshape(-1, D.item) != _bits(yf).reshape(-1, D.item))[0]
        assert bad.size == 0, f"{tag}: the updated handle's product differs from the fresh handle's, first at element {bad[:5] // 1 - D.G0}"


def create(eng, c, which, store, fmt, opts):
    dtype = np.float32 if store == "f32" else np.float64
    extra = {"value_storage": 1} if store == "mixed" else {}
    return eng.Matrix(c.rp, c.ci, c.V[which], c.m, c.n, fmt, dtype, **dict(opts, **extra))


# ---- 1. the delta layout -----------------------------------------------------------------------------------------------------------

def _v7_expected(lay):
    """the slices SellV7Range accepts, from the decoded plain layout: the values of the full groups of 4 steps (padding included) are
    exponent-0 or finite normals within 7 binades"""
    sp_, val = lay["slice_ptr"], lay["val"]
    out = []
    for s in range(lay["num_slices"]):
        width = (sp_[s + 1] - sp_[s]) // 64
        full = width // 4
        e = (val[sp_[s]:sp_[s] + 4 * full * 64].view(np.uint64) >> np.uint64(52)) & np.uint64(2047)
        normal = e[e > 0]
        out.append(bool(full > 0 and not (e == 2047).any() and (normal.size == 0 or int(normal.max()) - int(normal.min()) <= 6)))
    return np.array(out)


def _v7_stored(M):
    return (M.stored_array("desc", np.int64)[1:-2:2] & 8) != 0


@functools.lru_cache(maxsize=None)
def six_slice_case(w):
    rng = np.random.default_rng(300 + w)
    rp, ci, m = _six_slices(rng, w, N)
    assert m % 64 != 0
    V1 = _values(rng, m, w)
    V2 = _values(rng, m, w).reshape(m, w)
    full = 4 * (w // 4)
    if full:
        for s in (1, 4):                                    # wide range inside a full group: back to plain records
            V2[64 * s + 3, 0] *= 2.0 ** 20
            V2[64 * s + 40, full - 1] *= 2.0 ** -20
        V2[64 * 2 + 5, 1] = 0.0                             # exponent field 0 always fits: still 7 bytes
        V2[64 * 2 + 6, 2] = -0.0
        V2[64 * 2 + 7, 0] = 5e-324
    if w > full:                                            # wide range in the tail group only: still 7 bytes
        V2[64 * 3 + 9, full] *= 2.0 ** 20
        V2[64 * 3 + 10, w - 1] *= 2.0 ** -20
    return Case(rp, ci, m, N, V1, V2.reshape(-1).copy(), 400 + w)


DELTA_STORES = [("f64_v7", 1), ("f64", 2), ("f32", 0), ("mixed", 0)]


@pytest.mark.parametrize("store,sell_values", DELTA_STORES, ids=[s[0] for s in DELTA_STORES])
@pytest.mark.parametrize("split", (1, 2, 4))
def test_delta_layout(eng, torch, modes_off, split, store, sell_values):
    for w in WIDTHS:
        c = six_slice_case(w)
        D = Dev(torch, c, np.float32 if store == "f32" else np.float64)
        for off in (0, 7):
            modes_off(off)
            for conv in (1, 2):
                opts = dict(DELTA, sell_split=split, convert_on=conv, sell_values=sell_values)
                what = f"{store} w={w} split={split} modes_off={off} convert_on={conv}"
                fresh = {k: create(eng, c, k, store, "sell_c_sigma", opts) for k in (1, 2)}
                Mu = create(eng, c, 1, store, "sell_c_sigma", opts)
                assert Mu.update_values_state() == 1
                Mu.update_values_prepare(c.rp)
                assert Mu.update_values_state() == 2
                counts = [int(_v7_stored(Mu).sum())]
                for which in (2, 1):                         # the value array shrinks and grows once each
                    Mu.update_values(c.V[which])
                    check_update(D, Mu, fresh[which], which, store, f"{what} -> V{which}")
                    counts.append(int(_v7_stored(Mu).sum()))
                    if store == "f64_v7":
                        want = _v7_expected(fresh[which].sell_layout())
                        np.testing.assert_array_equal(_v7_stored(Mu), want, err_msg=f"{what} -> V{which}: 7-byte slices")
                if store == "f64_v7" and w >= 4:
                    assert 0 < counts[1] < counts[0] == counts[2], f"{what}: 7-byte slices after V1, V2, V1: {counts}"
                    assert Mu.format_name.endswith("_v7")
                elif store != "f64_v7":
                    assert counts == [0, 0, 0], what
                if store == "mixed" and conv == 1 and off == 0:
                    # the update narrowed V2: not the product of the unrounded values
                    Mu.update_values(c.V[2])
                    Md = create(eng, c, 2, "f64", "sell_c_sigma", dict(opts, sell_values=2))
                    assert not np.array_equal(D.run(Mu, 0), D.run(Md, 0)), f"{what}: nothing was narrowed"
                    Md.close()
                for M in (Mu, fresh[1], fresh[2]):
                    M.close()


def test_host_and_device_entry_give_the_same_bytes(eng, torch):
    c = six_slice_case(7)
    opts = dict(DELTA, sell_split=2, sell_values=1)
    Mh, Md = (create(eng, c, 1, "f64", "sell_c_sigma", opts) for _ in range(2))
    for M in (Mh, Md):
        M.update_values_prepare(c.rp)
    Mh.update_values(c.V[2])
    buf = torch.full((c.V[2].size + 1,), SENTINEL, dtype=torch.float64, device="cuda")
    buf[1:] = torch.from_numpy(c.V[2].copy()).cuda()          # one element in: 8-byte aligned only
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    Md.update_values_device(buf.data_ptr() + 8, side.cuda_stream)
    assert_same_handle(Md, Mh, "update_values_device against update_values")
    D = Dev(torch, c)
    np.testing.assert_array_equal(D.run(Md, 0), D.run(Mh, 0))
    Mh.close()
    Md.close()


# ---- 2. the LDS-window layout ------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def banded_case():
    rng = np.random.default_rng(21)
    m = 1003
    lens = rng.integers(1, 12, m)
    lens[17] = 0                                            # an empty row
    lens[500] = 23                                          # longer than its neighbours by more than 4
    lens[64 * 7:64 * 8] = 6                                 # a slice of equal rows: one contiguous stretch of the CSR array
    rows, cols = [], []
    for i in range(m):
        lo = max(0, min(i - 40, m - 81))
        cols.append(np.sort(rng.choice(80, lens[i], replace=False)) + lo)
        rows.append(np.full(lens[i], i))
    ci = np.concatenate(cols).astype(np.int32)
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    V1, V2 = rng.uniform(-2, 2, ci.size), rng.uniform(-2, 2, ci.size)
    return Case(rp, ci, m, m, V1, V2, 22)


@pytest.mark.parametrize("store", ("f64", "f32"))
@pytest.mark.parametrize("group", (1, 4))
def test_window_layout(eng, torch, store, group):
    c = banded_case()
    D = Dev(torch, c, np.float32 if store == "f32" else np.float64)
    for conv in (1, 2):
        opts = dict(sell_window=1, sell_group=group, sell_split=2, convert_on=conv)
        Mf = create(eng, c, 2, store, "sell_c_sigma", opts)
        Mu = create(eng, c, 1, store, "sell_c_sigma", opts)
        assert "_SELLW_" in Mu.format_name, Mu.format_name
        Mu.update_values_prepare(c.rp)
        Mu.update_values(c.V[2])
        check_update(D, Mu, Mf, 2, store, f"window {store} group={group} convert_on={conv}")
        Mu.close()
        Mf.close()


# ---- 3. plain SELL and the CSR-ordered layouts on one small irregular matrix -----------------------------------------------------------

@functools.lru_cache(maxsize=None)
def irregular_case():
    rng = np.random.default_rng(31)
    m, n = 333, 400
    lens = rng.integers(0, 13, m)
    lens[[0, 5, 64, 332]] = 0                               # empty rows, the first and the last among them
    lens[100] = 40
    ci = np.concatenate([np.sort(rng.choice(n, l, replace=False)) for l in lens]).astype(np.int32)
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    V1, V2 = rng.uniform(-2, 2, ci.size), rng.uniform(-2, 2, ci.size)
    return Case(rp, ci, m, n, V1, V2, 32)


@pytest.mark.parametrize("C", (16, 32, 64, 256))
def test_plain_sell(eng, torch, C):
    c = irregular_case()
    for store in ("f64", "f32"):
        D = Dev(torch, c, np.float32 if store == "f32" else np.float64)
        for sigma in (C, 0):
            for conv in (1, 2):
                opts = dict(sell_c=C, sell_delta=2, sell_sigma=sigma, sell_window=2, convert_on=conv)
                Mf = create(eng, c, 2, store, "sell_c_sigma", opts)
                Mu = create(eng, c, 1, store, "sell_c_sigma", opts)
                assert _kind(Mu) == "plain", Mu.format_name
                Mu.update_values_prepare(c.rp)
                Mu.update_values(c.V[2])
                check_update(D, Mu, Mf, 2, store, f"plain SELL C={C} sigma={sigma} {store} convert_on={conv}")
                Mu.close()
                Mf.close()


CSR_LAYOUTS = [("csr_scalar", {}), ("csr_scalar", {"kahan": 1}), ("csr_vector", {}), ("csr_stream", {"stream_mode": 1}),
               ("csr_stream", {"stream_mode": 2}), ("csr_stream", {"stream_mode": 3}), ("csr_stream", {"stream_mode": 4}),
               ("csr_merge", {}), ("coo", {})]


@pytest.mark.parametrize("fmt,opts", CSR_LAYOUTS, ids=[f + "".join(f"-{k}{v}" for k, v in o.items()) for f, o in CSR_LAYOUTS])
def test_csr_ordered_layouts(eng, torch, fmt, opts):
    c = irregular_case()
    for store in ("f64", "f32"):
        D = Dev(torch, c, np.float32 if store == "f32" else np.float64)
        Mf = create(eng, c, 2, store, fmt, opts)
        Mu = create(eng, c, 1, store, fmt, opts)
        Mu.update_values_prepare(c.rp)
        Mu.update_values(c.V[2])
        check_update(D, Mu, Mf, 2, store, f"{fmt} {opts} {store}")
        # the device entry with values that are 8-byte aligned only (the kernel's scalar-load form)
        Mu.update_values(c.V[1])
        buf = torch.full((c.V[2].size + 1,), SENTINEL, dtype=torch.float64, device="cuda")
        buf[1:] = torch.from_numpy(c.V[2].copy()).cuda()
        torch.cuda.synchronize()
        Mu.update_values_device(buf.data_ptr() + 8)
        check_update(D, Mu, Mf, 2, store, f"{fmt} {opts} {store}, unaligned device values")
        Mu.close()
        Mf.close()


def test_nan_and_inf_come_through(eng, torch):
    c = irregular_case()
    V = c.V[2].copy()
    r_nan, r_inf = 10, 200
    assert c.rp[r_nan + 1] > c.rp[r_nan] and c.rp[r_inf + 1] > c.rp[r_inf]
    V[c.rp[r_nan]] = np.nan
    V[c.rp[r_inf]] = np.inf
    for fmt, opts in (("csr_scalar", {}), ("sell_c_sigma", dict(DELTA, sell_values=1))):
        Mf = eng.Matrix(c.rp, c.ci, V, c.m, c.n, fmt, np.float64, **opts)
        Mu = eng.Matrix(c.rp, c.ci, c.V[1], c.m, c.n, fmt, np.float64, **opts)
        Mu.update_values_prepare(c.rp)
        Mu.update_values(V)
        assert_same_handle(Mu, Mf, f"{fmt} NaN / Inf")
        yu, yf = Mu.spmv(c.x), Mf.spmv(c.x)
        assert np.isnan(yu[r_nan]) and not np.isfinite(yu[r_inf]), (yu[r_nan], yu[r_inf])
        clean = np.ones(c.m, bool)
        clean[[r_nan, r_inf]] = False
        assert _bits(yu[clean]).tobytes() == _bits(yf[clean]).tobytes()
        y_ref, absrow = c.refs(2, "f64")
        assert np.all(np.abs(yf[clean] - y_ref[clean]) <= 1e-12 * np.maximum(absrow[clean], np.finfo(np.float64).tiny)), fmt
        Mu.close()
        Mf.close()


def test_merge_handle_updated_with_uniform_values_becomes_the_unit_handle(eng, torch):
    """the merge path's one choice from the values is made again: the updated handle is the _unit handle create() builds, and like it
    takes no further update"""
    c = irregular_case()
    ones = np.full(c.V[1].size, 1.0)
    Mf = eng.Matrix(c.rp, c.ci, ones, c.m, c.n, "csr_merge")
    Mu = eng.Matrix(c.rp, c.ci, c.V[1], c.m, c.n, "csr_merge")
    assert "_unit" in Mf.format_name and "_unit" not in Mu.format_name
    Mu.update_values_prepare(c.rp)
    Mu.update_values(ones)
    assert Mu.format_name == Mf.format_name and Mu.mem_footprint == Mf.mem_footprint
    y_ref = oracle.csr_spmv(c.rp, c.ci, ones, c.x, np.float64)
    absrow = oracle.csr_spmv(c.rp, c.ci, ones, np.abs(c.x))
    yf = Mf.spmv(c.x)
    assert np.all(np.abs(yf - y_ref) <= 1e-12 * np.maximum(absrow, np.finfo(np.float64).tiny))
    np.testing.assert_array_equal(Mu.spmv(c.x), yf)
    assert Mu.update_values_state() == 0
    with pytest.raises(eng.SpmvError, match="update_values"):
        Mu.update_values(c.V[2])
    Mu.close()
    Mf.close()


# ---- 4. a row block ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt,opts", [("sell_c_sigma", dict(DELTA, sell_values=1)), ("csr_vector", {})], ids=("delta", "csr_vector"))
def test_row_block(eng, torch, fmt, opts):
    c = irregular_case()
    r0, r1 = 70, 301
    e0, e1 = int(c.rp[r0]), int(c.rp[r1])
    blk = dict(opts, row_begin=r0, row_end=r1)
    Mf = eng.Matrix(c.rp, c.ci, c.V[2], c.m, c.n, fmt, np.float64, **blk)
    Mu = eng.Matrix(c.rp, c.ci, c.V[1], c.m, c.n, fmt, np.float64, **blk)
    assert Mu.m == r1 - r0 and Mu.nnz == e1 - e0
    Mu.update_values_prepare(c.rp[r0:r1 + 1] - c.rp[r0])
    Mu.update_values(c.V[2][e0:e1])
    assert_same_handle(Mu, Mf, f"row block {fmt}")
    y_ref, absrow = c.refs(2, "f64")
    yf = Mf.spmv(c.x)
    assert np.all(np.abs(yf - y_ref[r0:r1]) <= 1e-12 * np.maximum(absrow[r0:r1], np.finfo(np.float64).tiny))
    np.testing.assert_array_equal(Mu.spmv(c.x), yf)
    Mu.close()
    Mf.close()


# ---- 5. around the kernel ------------------------------------------------------------------------------------------------------------

def test_state_around_an_update(eng):
    """spmm scratch, solver and the host-buffer path before and after an update: the same bits as a fresh handle of the new values"""
    k = 12
    T = sp.diags([-np.ones(k - 1), 4 * np.ones(k), -np.ones(k - 1)], [-1, 0, 1])
    S = sp.diags([-np.ones(k - 1), -np.ones(k - 1)], [-1, 1])
    L = (sp.kron(sp.eye(k), T) + sp.kron(S, sp.eye(k))).tocsr()
    L.sort_indices()
    m = k * k
    rp, ci, V1 = L.indptr.astype(np.int32), L.indices.astype(np.int32), L.data.astype(np.float64)
    rng = np.random.default_rng(41)
    U = sp.triu(sp.csr_matrix((rng.uniform(0.5, 1.0, V1.size) * V1, ci, rp), shape=(m, m)), 1)
    A2 = (U + U.T + sp.diags(np.full(m, 4.5))).tocsr()      # symmetric, diagonally dominant: SPD, same pattern
    A2.sort_indices()
    assert np.array_equal(A2.indptr, rp) and np.array_equal(A2.indices, ci)
    V2 = A2.data.astype(np.float64)
    X = rng.uniform(-1, 1, (m, 5))
    B = rng.uniform(0.5, 1.5, (m, 2))
    x = rng.uniform(-1, 1, m)
    want_pcg = oracle.pcg(rp, ci, V2, B[:, 0].copy(), 40)
    y_ref, absrow = oracle.csr_spmv(rp, ci, V2, x, np.float64), oracle.csr_spmv(rp, ci, np.abs(V2), np.abs(x))
    for fmt, opts in (("sell_c_sigma", dict(sell_window=2, sell_values=1)), ("csr_vector", {}), ("sell_c_sigma", dict(sell_window=1))):
        Mf = eng.Matrix(rp, ci, V2, m, m, fmt, np.float64, **opts)
        Mu = eng.Matrix(rp, ci, V1, m, m, fmt, np.float64, **opts)
        assert np.all(np.abs(Mf.spmv(x) - y_ref) <= 1e-12 * absrow), f"{fmt}: the fresh handle against the oracle"
        Mu.update_values_prepare(rp)
        y1 = Mu.spmv(x, always_copy=False)
        Mu.spmm(X)
        Mu.pcg_multi(rp, ci, V1, B, 40)
        Mu.update_values(V2)
        # the host-buffer path with the reference's caching: the same x pointer again must still download the NEW product
        xs = np.ascontiguousarray(x)
        ya, yb = np.ones(m + 64), np.ones(m + 64)
        Mu.set_always_copy(False)
        Mu.spmv_raw(xs, ya)
        Mu.update_values(V1)
        Mu.spmv_raw(xs, yb)
        np.testing.assert_array_equal(yb[:m], y1, err_msg=f"{fmt}: host-buffer spmv after an update returned a stale y")
        assert not np.array_equal(ya[:m], yb[:m])
        Mu.update_values(V2)
        np.testing.assert_array_equal(Mu.spmm(X), Mf.spmm(X), err_msg=f"{fmt}: spmm k=5 after the update")
        got, want = Mu.pcg_multi(rp, ci, V2, B, 40), Mf.pcg_multi(rp, ci, V2, B, 40)
        for j in range(2):
            assert got[j]["iterations"] == want[j]["iterations"] > 0
            assert got[j]["x"].tobytes() == want[j]["x"].tobytes(), f"{fmt}: pcg_multi column {j}"
            assert got[j]["history"].tobytes() == want[j]["history"].tobytes(), f"{fmt}: pcg_multi history {j}"
        # the fresh handle's solve against the oracle's
        assert abs(want[0]["iterations"] - want_pcg["iterations"]) <= 2
        if want_pcg["iterations"] < 40:
            assert np.linalg.norm(want[0]["x"] - want_pcg["x"]) <= 1e-9 * np.linalg.norm(want_pcg["x"])
        Mu.close()
        Mf.close()


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------------------

def _refused(eng, M, x, call, pattern="update_values", absrow=None):
    """rc 1 with the message, and the product as before: the same bits, or — on the layouts whose LDS atomics add a row's products in
    an order that changes from launch to launch — two results that each lie within TOL * sum|a x| of the exact product"""
    before = M.spmv(x)
    with pytest.raises(eng.SpmvError, match=pattern):
        call()
    after = M.spmv(x)
    if any(t in M.format_name for t in ATOMIC_LAYOUTS):
        assert np.all(np.abs(after - before) <= 2 * TOL[np.float64] * absrow), f"{M.format_name}: a refused call changed the product"
    else:
        np.testing.assert_array_equal(after, before, err_msg=f"{M.format_name}: a refused call changed the product")


def test_refusals(eng):
    L = eng.lib()
    c = six_slice_case(5)
    M = create(eng, c, 1, "f64", "sell_c_sigma", dict(DELTA, sell_values=1))
    assert M.update_values_state() == 1
    _refused(eng, M, c.x, lambda: M.update_values(c.V[2]), "update_values.*prepare")
    rp_bad = c.rp.copy()
    rp_bad[1] -= 1                                          # row 0 one shorter, row 1 one longer: same nnz, another pattern
    _refused(eng, M, c.x, lambda: M.update_values_prepare(rp_bad), "row_ptr does not match the pattern this handle was built from")
    assert M.update_values_state() == 1
    for bad in (c.rp + 1, c.rp[::-1].copy(), np.minimum(c.rp, c.rp[-1] - 1)):
        _refused(eng, M, c.x, lambda bad=bad: M.update_values_prepare(bad), "update_values_prepare")
    M.update_values_prepare(c.rp)
    assert M.update_values_state() == 2
    M.update_values_prepare(c.rp)                           # twice is allowed
    M.update_values(c.V[2])
    M.close()

    ir = irregular_case()
    sym = sp.csr_matrix((ir.V[1], ir.ci, ir.rp), shape=(ir.m, ir.n))[:, :ir.m]
    tri = sp.triu(sym + sym.T).tocsr()
    tri.sort_indices()
    trp, tci, tva = tri.indptr.astype(np.int32), tri.indices.astype(np.int32), tri.data.astype(np.float64)
    cases = [("column filter", (ir.rp, ir.ci, ir.V[1], ir.m, ir.n, "csr_vector"), dict(col_begin=50, col_end=300, col_filter_mode=1)),
             ("symmetric input", (trp, tci, tva, ir.m, ir.m, "sell_c_sigma"), dict(symmetric_input=1)),
             ("symmetric input, window", (trp, tci, tva, ir.m, ir.m, "sell_c_sigma"), dict(symmetric_input=1, sell_window=1)),
             ("column-blocked", (ir.rp, ir.ci, ir.V[1], ir.m, ir.n, "coo"), dict(col_blocks=-1)),
             ("uniform merge", (ir.rp, ir.ci, np.ones(ir.V[1].size), ir.m, ir.n, "csr_merge"), {})]
    # a banded upper triangle large enough for create() to keep it as a triangle in the LDS-window layout
    bm, bw = 8192, 9
    bc = np.arange(bm)[:, None] + np.arange(bw)[None, :]
    keep = bc < bm
    brp = np.concatenate([[0], np.cumsum(keep.sum(axis=1))]).astype(np.int32)
    bva = np.where(bc == np.arange(bm)[:, None], 20.0, -1.0)[keep]
    cases.append(("symmetric input kept as a triangle", (brp, bc[keep].astype(np.int32), bva, bm, bm, "sell_c_sigma"),
                  dict(symmetric_input=1, sell_window=1)))
    for what, args, opts in cases:
        M = eng.Matrix(*args, np.float64, **opts)
        if "triangle" in what:
            assert "_SELLWS_" in M.format_name, M.format_name
        x = np.random.default_rng(7).uniform(-1, 1, M.n)
        assert M.update_values_state() == 0, what
        assert b"update_values" in L.spmv_mi355x_last_error(), what
        lrp = np.zeros(M.m + 1, np.int32)
        lrp[-1] = M.nnz
        S = abs(sp.csr_matrix((args[2], args[1], args[0]), shape=(args[3], args[4])))
        if opts.get("symmetric_input"):
            S = S + S.T - sp.diags(S.diagonal())
        absrow = np.asarray(S @ np.abs(x)).ravel()
        _refused(eng, M, x, lambda: M.update_values_prepare(lrp), absrow=absrow)
        _refused(eng, M, x, lambda: M.update_values(np.ones(M.nnz)), absrow=absrow)
        M.close()
