"""opts.transpose (include/spmv_mi355x.h "transposed handles"): a handle of A^t built on the GPU from the CSR of A.

The contract: a handle built from (A, opts with transpose = 1) is indistinguishable from the handle create() builds from the CSR of A^t
(rows in order, entries of a row in ascending row of A, duplicates in input order) with transpose = 0 and otherwise equal opts.
The reference CSR of A^t is made here in numpy with a stable argsort by column. Every comparison starts by holding the FRESH handle,
built from that reference, to oracle.csr_spmv on the same arrays (test_gpu_parity.compare_device_result and TOL, the only tolerance
used), so no link of the chain compares the engine with itself alone; the transposed handle is then compared with the fresh one: the
bytes of the stored arrays, the metadata answers, the bits of y = A^t x and y += A^t x through the device entry point (sentinels
around y, x at an odd element offset) and spmm at k = 3. The adjoint identity v.(A u) = u.(A^t v) is a second, independent check."""
import functools
import os

import numpy as np
import pytest
import scipy.sparse as sp

import oracle
from conftest import GOLDEN
from test_gpu_parity import ATOMIC_LAYOUTS, TOL, check, compare_device_result
from test_gpu_update_values import DELTA, Dev, _bits, assert_same_handle

pytestmark = pytest.mark.gpu


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


# ---- the reference transposition and the problems (computed once, read-only) ------------------------------------------------------------

def np_transpose(rp, ci, va, m, n):
    """CSR of A^t: a stable counting sort of the entries by column"""
    rows = np.repeat(np.arange(m, dtype=np.int32), np.diff(rp))
    order = np.argsort(ci, kind="stable")
    rp_t = np.concatenate([[0], np.cumsum(np.bincount(ci, minlength=n))]).astype(np.int32)
    return rp_t, rows[order].astype(np.int32), np.ascontiguousarray(va[order], np.float64)


class Case:
    """A (m x n) as given to create(..., transpose=1), and A^t = (rp, ci, va) of shape (self.m, self.n) = (n, m) of A: the attributes
    without prefix are those of the HANDLE (what test_gpu_update_values.Dev reads)"""

    def __init__(self, a_rp, a_ci, a_va, a_m, a_n, seed):
        self.a = (np.ascontiguousarray(a_rp, np.int32), np.ascontiguousarray(a_ci, np.int32), np.ascontiguousarray(a_va, np.float64))
        self.a_m, self.a_n = a_m, a_n
        assert self.a[0].shape == (a_m + 1,) and self.a[0][-1] == self.a[1].size == self.a[2].size
        self.rp, self.ci, self.va = np_transpose(*self.a, a_m, a_n)
        self.m, self.n = a_n, a_m
        rng = np.random.default_rng(seed)
        self.x = rng.uniform(-1, 1, self.n)
        self.x[self.x == 0] = 0.5
        self.y0 = rng.uniform(-1, 1, self.m) * 8
        self.X = rng.uniform(-1, 1, (self.n, 3))
        for v in self.a + (self.rp, self.ci, self.va, self.x, self.y0, self.X):
            v.setflags(write=False)
        self._refs = {}

    def refs(self, dtype, mixed=False):
        """(y_ref in the vectors' precision, sum |a x|, the same for the 3 columns of X) of the oracle on the reference CSR of A^t"""
        key = (np.dtype(dtype).name, mixed)
        if key not in self._refs:
            a = self.va.astype(np.float32).astype(np.float64) if mixed else self.va
            one = lambda x: (oracle.csr_spmv(self.rp, self.ci, a, np.ascontiguousarray(x, dtype), dtype),
                             oracle.csr_spmv(self.rp, self.ci, np.abs(a), np.abs(np.ascontiguousarray(x, np.float64))))
            self._refs[key] = one(self.x) + (tuple(one(self.X[:, j]) for j in range(3)),)
        return self._refs[key]

    def fresh(self, eng, fmt, dtype=np.float64, **opts):
        return eng.Matrix(self.rp, self.ci, self.va, self.m, self.n, fmt, dtype, **opts)

    def transposed(self, eng, fmt, dtype=np.float64, **opts):
        return eng.Matrix(*self.a, self.a_m, self.a_n, fmt, dtype, transpose=1, **opts)


def _random(rng, m, n, per_row, empty_rows=(), empty_cols=None):
    lens = rng.integers(0, 2 * per_row + 1, m)
    lens[list(empty_rows)] = 0
    lens = np.minimum(lens, n)
    cols = [np.sort(rng.choice(n, l, replace=False)) for l in lens]
    if empty_cols is not None:
        cols = [c[(c < empty_cols[0]) | (c >= empty_cols[1])] for c in cols]
    ci = np.concatenate(cols).astype(np.int32) if m else np.zeros(0, np.int32)
    rp = np.concatenate([[0], np.cumsum([c.size for c in cols])]).astype(np.int32)
    return rp, ci, rng.uniform(-2, 2, ci.size), m, n


@functools.lru_cache(maxsize=None)
def case(name):
    seed = 50 + sum(map(ord, name))
    rng = np.random.default_rng(seed + 1000)
    if name == "tall":
        return Case(*_random(rng, 1537, 1000, 6), seed)           # A^t is 1000 x 1537
    if name == "wide":
        return Case(*_random(rng, 1000, 1537, 6), seed)           # A^t is 1537 x 1000: n of A is no multiple of 64
    if name in ("n1024", "n1025"):
        return Case(*_random(rng, 900, int(name[1:]), 5), seed)    # the sort's key-bit boundary: 10 and 11 bits
    if name == "n1":
        rp, ci, va, m, n = _random(rng, 700, 1, 1)
        assert 0 < ci.size < 700
        return Case(rp, ci, va, m, n, seed)
    if name == "nnz0":
        return Case(np.zeros(301, np.int32), np.zeros(0, np.int32), np.zeros(0), 300, 200, seed)
    if name == "holes":
        c = Case(*_random(rng, 1200, 1100, 5, empty_rows=range(100), empty_cols=(200, 264)), seed)
        assert c.a[0][100] == 0 and np.all(np.diff(c.rp)[200:264] == 0) and c.rp[-1] > 3000
        return c
    if name == "hub_column":
        m, n = 70000, 300                                          # every row owns an entry in column 5, plus a sparse random rest
        rest = np.unique(rng.integers(0, m * n, 60000))
        rest = rest[rest % n != 5]
        rows, ci = np.concatenate([rest // n, np.arange(m)]), np.concatenate([rest % n, np.full(m, 5)])
        va = rng.uniform(-2, 2, rows.size)
        order = np.lexsort((ci, rows))
        rp = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=m))]).astype(np.int32)
        c = Case(rp, ci[order].astype(np.int32), va[order], m, n, seed)
        assert c.rp[6] - c.rp[5] == 70000
        return c
    if name == "duplicates":
        rp, ci, va, m, n = _random(rng, 400, 500, 6)
        ci, va = ci.copy(), va.copy()
        dup_rows = np.nonzero(np.diff(rp) >= 3)[0][::40][:5]       # an exact (row, column) duplicate with another value in five rows
        assert dup_rows.size == 5
        for r in dup_rows:
            s = rp[r]
            ci[s + 2] = ci[s]                                      # not adjacent in the input: columns c, c', c
            va[s + 2] = va[s] + 1.0
        c = Case(rp, ci, va, m, n, seed)
        c.dup_rows = dup_rows
        return c
    if name == "banded":
        m, hw = 8192, 40
        cols = []
        for i in range(m):
            lo, hi = max(0, i - hw), min(m, i + hw + 1)
            cols.append(np.arange(lo, hi)[rng.random(hi - lo) < 0.6])
        ci = np.concatenate(cols).astype(np.int32)
        rp = np.concatenate([[0], np.cumsum([c.size for c in cols])]).astype(np.int32)
        return Case(rp, ci, rng.uniform(-2, 2, ci.size), m, m, seed)
    if name in ("rectangular", "huge_row"):
        import spmv_host as H
        info, rp, ci, va = H.mtx_to_csr(os.path.join(GOLDEN, name + ".mtx"))       # the host reader
        return Case(rp, ci, va, info["m"], info["n"], seed)
    raise KeyError(name)


def compare(eng, torch, c, fmt, dtype=np.float64, what="", **opts):
    """the fresh handle of the numpy transpose against the oracle, the transposed handle against the fresh one. Returns both (open)."""
    dtype = np.dtype(dtype).type
    mixed = opts.get("value_storage") == 1 and dtype == np.float64
    y_ref, absrow, cols = c.refs(dtype, mixed)
    what = f"{what or fmt} {opts} {np.dtype(dtype).name}"
    Mf = c.fresh(eng, fmt, dtype, **opts)
    Mt = c.transposed(eng, fmt, dtype, **opts)
    assert (Mt.transposed, Mf.transposed) == (1, 0), what
    assert (Mt.m, Mt.n, Mt.nnz) == (Mf.m, Mf.n, Mf.nnz) == (c.m, c.n, c.va.size), f"{what}: rows / cols / nnz {(Mt.m, Mt.n, Mt.nnz)}"
    assert Mt.csr_mem_footprint == Mf.csr_mem_footprint, what
    assert_same_handle(Mt, Mf, what)
    atomic = any(t in Mf.format_name for t in ATOMIC_LAYOUTS)
    D = Dev(torch, c, dtype)
    for beta in (0, 1):
        tag = f"{what} beta={beta}"
        yf = D.run(Mf, beta)
        compare_device_result(yf, D.y0 if beta else None, y_ref, absrow, D.G0, c.m, dtype, False, tag + " fresh handle")
        yt = D.run(Mt, beta)
        if atomic:
            compare_device_result(yt, D.y0 if beta else None, y_ref, absrow, D.G0, c.m, dtype, False, tag + " transposed handle")
        else:
            bad = np.nonzero(_bits(yt).reshape(-1, D.item) != _bits(yf).reshape(-1, D.item))[0]
            assert bad.size == 0, f"{tag}: the transposed handle's product differs from the fresh handle's, first at element {bad[:5] - D.G0}"
    Yf, Yt = Mf.spmm(c.X.astype(dtype)), Mt.spmm(c.X.astype(dtype))
    for j in range(3):
        for Y, who in ((Yf, "fresh"),) + (((Yt, "transposed"),) if atomic else ()):
            check(np.ascontiguousarray(Y[:, j]), cols[j][0], cols[j][1], dtype, False, f"{what}: spmm column {j} of the {who} handle")
    if not atomic:
        assert _bits(Yt).tobytes() == _bits(Yf).tobytes(), f"{what}: spmm k=3"
    return Mt, Mf


def compare_and_close(*a, **kw):
    for M in compare(*a, **kw):
        M.close()


# ---- 1. every input through three layouts ------------------------------------------------------------------------------------------

INPUTS = ("tall", "wide", "n1024", "n1025", "n1", "nnz0", "holes", "hub_column", "duplicates", "rectangular", "huge_row")


@pytest.mark.parametrize("name", INPUTS)
def test_inputs(eng, torch, name):
    c = case(name)
    for fmt, opts in (("csr_vector", {}), ("sell_c_sigma", {}), ("sell_c_sigma", DELTA), ("coo", {})):
        compare_and_close(eng, torch, c, fmt, what=name, **opts)


def test_duplicates_keep_their_input_order(eng):
    """the stable order, seen from outside: the plain SELL layout of A^t lists a row's entries in the CSR's order"""
    c = case("duplicates")
    opts = dict(sell_c=64, sell_delta=2, sell_sigma=64, sell_window=2)
    Mt, Mf = c.transposed(eng, "sell_c_sigma", **opts), c.fresh(eng, "sell_c_sigma", **opts)
    lt, lf = Mt.sell_layout(), Mf.sell_layout()
    assert _bits(lt["val"]).tobytes() == _bits(lf["val"]).tobytes() and np.array_equal(lt["col"], lf["col"])
    # and the reference itself holds both values of a duplicate, first input first
    a_rp, a_ci, a_va = c.a
    for row in c.dup_rows:
        s = a_rp[row]
        col = a_ci[s]
        mine = np.nonzero(c.ci[c.rp[col]:c.rp[col + 1]] == row)[0] + c.rp[col]
        assert mine.size == 2 and c.va[mine[0]] == a_va[s] and c.va[mine[1]] == a_va[s + 2]
    Mt.close()
    Mf.close()


def test_banded_window_layout(eng, torch):
    c = case("banded")
    for dtype in (np.float64, np.float32):
        Mt, Mf = compare(eng, torch, c, "sell_c_sigma", dtype, sell_window=1)
        assert "_SELLW_" in Mt.format_name and "_SELLW_" in Mf.format_name, (Mt.format_name, Mf.format_name)
        Mt.close()
        Mf.close()


# ---- 2. formats and options --------------------------------------------------------------------------------------------------------

PLAIN = dict(sell_c=64, sell_delta=2, sell_sigma=64, sell_window=2)
LAYOUTS = [("csr_scalar", {}), ("csr_vector", {}), ("csr_merge", {}), ("sell_c_sigma", {}), ("coo", {}), ("csr_stream", {}),
           ("sell_c_sigma", PLAIN), ("sell_c_sigma", dict(PLAIN, sell_c=16, sell_sigma=32)), ("sell_c_sigma", DELTA),
           ("sell_c_sigma", dict(DELTA, sell_values=1)), ("sell_c_sigma", dict(DELTA, value_storage=1))]


@pytest.mark.parametrize("fmt,opts", LAYOUTS, ids=[f + "".join(f"-{k}{v}" for k, v in o.items()) for f, o in LAYOUTS])
def test_formats_and_options(eng, torch, fmt, opts):
    c = case("wide")
    Mt, Mf = compare(eng, torch, c, fmt, **opts)
    if opts.get("value_storage") == 1:
        assert Mt.format_name.endswith("_v4") and Mt.value_dtype == np.float32, Mt.format_name
    if opts == DELTA:
        assert "_SELLD_" in Mt.format_name
    if opts == PLAIN:
        assert "_SELL_64_" in Mt.format_name
    Mt.close()
    Mf.close()
    if opts.get("value_storage") != 1 and not opts.get("sell_values"):
        compare_and_close(eng, torch, c, fmt, np.float32, **opts)


def test_host_and_gpu_transposition_give_the_same_bytes(eng, torch):
    """convert_on = 2 transposes on the host (and builds there), convert_on = 1 on the GPU"""
    for name in ("wide", "duplicates", "holes"):
        c = case(name)
        for fmt, opts in (("sell_c_sigma", DELTA), ("sell_c_sigma", PLAIN), ("csr_vector", {})):
            Mh, Mfh = compare(eng, torch, c, fmt, what=name, **dict(opts, convert_on=2))
            Mg, Mfg = compare(eng, torch, c, fmt, what=name, **dict(opts, convert_on=1))
            assert_same_handle(Mh, Mg, f"{name} {fmt}: host against GPU transposition")
            x = c.x.astype(np.float64)
            assert _bits(Mh.spmv(x)).tobytes() == _bits(Mg.spmv(x)).tobytes()
            for M in (Mh, Mfh, Mg, Mfg):
                M.close()
    c = case("banded")
    Mh, Mfh = compare(eng, torch, c, "sell_c_sigma", sell_window=1, convert_on=2)
    Mg, Mfg = compare(eng, torch, c, "sell_c_sigma", sell_window=1, convert_on=1)
    assert_same_handle(Mh, Mg, "banded window: host against GPU transposition")
    for M in (Mh, Mfh, Mg, Mfg):
        M.close()


@pytest.mark.parametrize("fmt", ("coo", "csr_merge"))
def test_column_blocked_layout(eng, torch, fmt):
    c = case("wide")
    Mt, Mf = compare(eng, torch, c, fmt, col_blocks=-1)
    assert any(t in Mt.format_name for t in ATOMIC_LAYOUTS), Mt.format_name
    Mt.close()
    Mf.close()


ROW_COL = [dict(row_begin=300, row_end=900), dict(col_begin=100, col_end=640, col_filter_mode=1), dict(col_begin=100, col_end=640, col_filter_mode=2),
           dict(row_begin=300, row_end=900, col_begin=100, col_end=640, col_filter_mode=1)]


@pytest.mark.parametrize("sub", ROW_COL, ids=["rows", "cols_inside", "cols_outside", "rows_and_cols"])
def test_row_block_and_column_filter_are_in_the_coordinates_of_the_transpose(eng, torch, sub):
    c = case("wide")                                            # A^t is 1537 x 1000
    r0, r1 = sub.get("row_begin", 0), sub.get("row_end", c.m)
    T = sp.csr_matrix((c.va, c.ci, c.rp), shape=(c.m, c.n))
    mask = np.ones(c.n, bool)
    if sub.get("col_filter_mode"):
        inside = (np.arange(c.n) >= sub["col_begin"]) & (np.arange(c.n) < sub["col_end"])
        mask = inside if sub["col_filter_mode"] == 1 else ~inside
    xm = np.where(mask, c.x, 0.0)
    y_ref = oracle.csr_spmv(c.rp, c.ci, c.va, xm, np.float64)[r0:r1]
    absrow = oracle.csr_spmv(c.rp, c.ci, np.abs(c.va), np.abs(xm))[r0:r1]
    want_nnz = int((T[r0:r1] @ sp.diags(mask.astype(float))).count_nonzero())
    for fmt, opts in (("sell_c_sigma", DELTA), ("csr_vector", {})):
        Mf, Mt = c.fresh(eng, fmt, **dict(opts, **sub)), c.transposed(eng, fmt, **dict(opts, **sub))
        assert (Mt.m, Mt.n, Mt.nnz) == (Mf.m, Mf.n, Mf.nnz) == (r1 - r0, c.n, want_nnz), (sub, Mt.m, Mt.n, Mt.nnz)
        assert_same_handle(Mt, Mf, f"{fmt} {sub}")
        yf = Mf.spmv(c.x)
        check(yf, y_ref, absrow, np.float64, False, f"{fmt} {sub}: fresh handle")
        assert _bits(Mt.spmv(c.x)).tobytes() == _bits(yf).tobytes(), f"{fmt} {sub}"
        Mt.close()
        Mf.close()


# ---- 3. create_from_stream ---------------------------------------------------------------------------------------------------------

def _stream(eng, c, pieces, capacity, rows=None):
    a_rp, a_ci, a_va = c.a
    st = eng.CsrStream(c.a_m, c.a_n, capacity)
    for r0, r1 in pieces:
        st.append(a_rp[r0:r1 + 1] - a_rp[r0], a_ci[a_rp[r0]:a_rp[r1]], a_va[a_rp[r0]:a_rp[r1]])
    return st


@pytest.mark.parametrize("store", ("f64", "f64_v7", "f32", "mixed"))
def test_create_from_stream(eng, torch, store):
    c = case("wide")
    dtype = np.float32 if store == "f32" else np.float64
    opts = dict(DELTA, sell_values=1 if store == "f64_v7" else 2 if store == "f64" else 0, **({"value_storage": 1} if store == "mixed" else {}))
    st = _stream(eng, c, ((0, 17), (17, 640), (640, c.a_m)), c.a[1].size + 1000)
    S = st.finish("sell_c_sigma", dtype, transpose=1, **opts)
    Mf = c.fresh(eng, "sell_c_sigma", dtype, **dict(opts, convert_on=1))
    assert S.transposed == 1 and (S.m, S.n, S.nnz) == (c.m, c.n, c.va.size)
    assert_same_handle(S, Mf, f"from stream {store}")
    y_ref, absrow, _ = c.refs(dtype, store == "mixed")
    D = Dev(torch, c, dtype)
    for beta in (0, 1):
        yf = D.run(Mf, beta)
        compare_device_result(yf, D.y0 if beta else None, y_ref, absrow, D.G0, c.m, np.dtype(dtype).type, False, f"from stream {store} beta={beta}: fresh handle")
        assert _bits(D.run(S, beta)).tobytes() == _bits(yf).tobytes(), f"from stream {store} beta={beta}"
    # the untransposed stream of the same pieces is untouched by the feature
    S0 = _stream(eng, c, ((0, 17), (17, 640), (640, c.a_m)), c.a[1].size + 1000).finish("sell_c_sigma", dtype, **opts)
    assert S0.transposed == 0 and (S0.m, S0.n) == (c.a_m, c.a_n)
    for M in (S, S0, Mf):
        M.close()


def test_create_from_stream_edge_cases_and_an_unfinished_stream(eng, torch):
    for name in ("nnz0", "n1", "hub_column"):
        c = case(name)
        S = _stream(eng, c, ((0, c.a_m // 3), (c.a_m // 3, c.a_m)), c.a[1].size + 5).finish("sell_c_sigma", np.float64, transpose=1, **DELTA)
        Mf = c.fresh(eng, "sell_c_sigma", **DELTA)
        assert_same_handle(S, Mf, f"from stream {name}")
        y_ref, absrow, _ = c.refs(np.float64)
        yf = Mf.spmv(c.x)
        check(yf, y_ref, absrow, np.float64, False, f"from stream {name}: fresh handle")
        assert _bits(S.spmv(c.x)).tobytes() == _bits(yf).tobytes(), name
        S.close()
        Mf.close()
    c = case("wide")
    st = _stream(eng, c, ((0, 17), (17, 640)), c.a[1].size)
    with pytest.raises(eng.SpmvError, match=f"640 of {c.a_m} rows were appended"):
        st.finish("sell_c_sigma", np.float64, transpose=1)
    assert st.s is None                                         # consumed
    st = _stream(eng, c, ((0, c.a_m),), c.a[1].size)
    with pytest.raises(eng.SpmvError, match="transpose"):
        st.finish("sell_c_sigma", np.float64, transpose=3)


# ---- 4. the adjoint identity: v . (A u) = u . (A^t v) ---------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ("wide", "tall", "duplicates", "hub_column"))
def test_adjoint_identity(eng, name):
    c = case(name)
    a_rp, a_ci, a_va = c.a
    rng = np.random.default_rng(9)
    u, v = rng.uniform(-1, 1, c.a_n), rng.uniform(-1, 1, c.a_m)
    bound = TOL[np.float64] * float(np.abs(v) @ oracle.csr_spmv(a_rp, a_ci, np.abs(a_va), np.abs(u)))
    for fmt, opts in (("sell_c_sigma", DELTA), ("csr_vector", {}), ("csr_merge", {})):
        MA = eng.Matrix(a_rp, a_ci, a_va, c.a_m, c.a_n, fmt, np.float64, **opts)
        MT = c.transposed(eng, fmt, **opts)
        assert (MA.transposed, MT.transposed) == (0, 1)
        lhs, rhs = float(v @ MA.spmv(u)), float(u @ MT.spmv(v))
        assert abs(lhs - rhs) <= bound, f"{name} {fmt}: v.(A u) = {lhs!r}, u.(A^t v) = {rhs!r}, bound {bound!r}"
        MA.close()
        MT.close()


# ---- 5. solvers, refusals -----------------------------------------------------------------------------------------------------------

def test_pcg_on_a_transposed_handle_with_the_original_csr_for_the_diagonal(eng):
    k = 12
    I = sp.eye(k)
    T = sp.diags([-np.ones(k - 1), 2 * np.ones(k), -np.ones(k - 1)], [-1, 0, 1])
    L = (sp.kron(sp.kron(T, I), I) + sp.kron(sp.kron(I, T), I) + sp.kron(sp.kron(I, I), T) + 0.1 * sp.eye(k ** 3)).tocsr()
    L.sort_indices()
    m = k ** 3
    c = Case(L.indptr, L.indices, L.data, m, m, 5)
    b = np.random.default_rng(6).uniform(0.5, 1.5, m)
    want = oracle.pcg(c.rp, c.ci, c.va, b, 300)
    for fmt, opts in (("sell_c_sigma", {}), ("csr_vector", {})):
        Mt, Mf = c.transposed(eng, fmt, **opts), c.fresh(eng, fmt, **opts)
        got_t = Mt.pcg(*c.a, b, 300)                            # the CSR create() was given: the diagonal of A^t is that of A
        got_f = Mf.pcg(c.rp, c.ci, c.va, b, 300)
        assert got_t["iterations"] == got_f["iterations"] > 0
        assert got_t["x"].tobytes() == got_f["x"].tobytes() and got_t["history"].tobytes() == got_f["history"].tobytes(), fmt
        assert abs(got_f["iterations"] - want["iterations"]) <= 2
        assert np.linalg.norm(got_f["x"] - want["x"]) <= 1e-9 * np.linalg.norm(want["x"])
        Mt.close()
        Mf.close()


def test_update_values_is_refused_on_a_transposed_handle(eng):
    c = case("wide")
    L = eng.lib()
    for fmt, opts in (("sell_c_sigma", DELTA), ("csr_vector", {})):
        Mt, Mf = c.transposed(eng, fmt, **opts), c.fresh(eng, fmt, **opts)
        assert Mf.transposed == 0 and Mf.update_values_state() == 1
        assert Mt.transposed == 1 and Mt.update_values_state() == 0
        assert b"transpose" in L.spmv_mi355x_last_error()
        before = Mt.spmv(c.x)
        for call in (lambda: Mt.update_values_prepare(c.rp), lambda: Mt.update_values(np.ones(Mt.nnz))):
            with pytest.raises(eng.SpmvError, match="update_values.*transpose"):
                call()
        np.testing.assert_array_equal(Mt.spmv(c.x), before)
        Mt.close()
        Mf.close()


def test_bad_input_keeps_its_messages_with_transpose(eng):
    c = case("wide")
    a_rp, a_ci, a_va = c.a
    bad_ci = a_ci.copy()
    bad_ci[11] = c.a_n
    with pytest.raises(eng.SpmvError, match=rf"column index {c.a_n} out of range \[0,{c.a_n}\) at entry 11"):
        eng.Matrix(a_rp, bad_ci, a_va, c.a_m, c.a_n, "csr_vector", transpose=1)
    bad_rp = a_rp.copy()
    r = 1 + int(np.nonzero(np.diff(a_rp)[1:] > 0)[0][0])        # a row that owns entries: its two pointers swapped
    bad_rp[r], bad_rp[r + 1] = a_rp[r + 1], a_rp[r]
    with pytest.raises(eng.SpmvError, match=f"row_ptr is not monotone at row {r}$"):
        eng.Matrix(bad_rp, a_ci, a_va, c.a_m, c.a_n, "csr_vector", transpose=1)
    with pytest.raises(eng.SpmvError, match="bad row block"):   # rows of A^t: 1537, not the 1000 of A ... and 1538 is past both
        eng.Matrix(a_rp, a_ci, a_va, c.a_m, c.a_n, "csr_vector", transpose=1, row_begin=0, row_end=c.m + 1)
    M = eng.Matrix(a_rp, a_ci, a_va, c.a_m, c.a_n, "csr_vector", transpose=1, row_begin=c.a_m, row_end=c.m)   # past the rows of A
    assert M.m == c.m - c.a_m
    M.close()
