"""spmv_mi355x_update_values_prepare_transposed (include/spmv_mi355x.h "new values for an existing handle", TRANSPOSED HANDLES): a
handle built with transpose = 1 takes new values in the entry order of A, the only order its caller has.

The contract: a handle created from (pattern of A, V1, opts with transpose = 1), prepared with the pattern of A and updated with V2
(update_values_count() = nnz(A) values, V2[e] belonging to entry e of the CSR of A) is indistinguishable from the handle create()
builds from (pattern of A, V2, the same opts): assert_same_handle (stored bytes, names, footprint, plans), then y = A^t x,
y += A^t x (device entry, sentinels around y) and a 3-column spmm, bit for bit. The FRESH handle is first held to oracle.csr_spmv on
the numpy transpose of (A, V2) — V2 gathered through a stable argsort of the columns — with test_gpu_parity's check and TOL, the only tolerance
used, so no link of the chain compares the engine with itself alone. The map itself is read back exactly: with V2[e] = e + 1 every
stored value names the entry of A it came from."""
import functools

import numpy as np
import pytest

import oracle
from test_gpu_parity import SENTINEL, check, compare_device_result
from test_gpu_transpose import case
from test_gpu_update_values import DELTA, Dev, _bits, assert_same_handle

pytestmark = pytest.mark.gpu

PLAIN = dict(sell_c=64, sell_delta=2, sell_sigma=64, sell_window=2)


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


# ---- second value sets and their references (computed once, read-only) ----------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def order_of(name):
    """src of the reference: entry e of the CSR of A^t is entry order[e] of the CSR of A (numpy's stable argsort of the columns)"""
    o = np.argsort(case(name).a[1], kind="stable")
    o.setflags(write=False)
    return o


@functools.lru_cache(maxsize=None)
def second(name):
    """V2 in A's entry order, and the same values in the order of A^t"""
    c = case(name)
    V2 = np.random.default_rng(77 + c.a[1].size).uniform(-2, 2, c.a[1].size)
    V2[V2 == 0] = 0.5
    t = np.ascontiguousarray(V2[order_of(name)])
    V2.setflags(write=False)
    t.setflags(write=False)
    return V2, t


@functools.lru_cache(maxsize=None)
def refs(name, dtype_name, mixed):
    """(y_ref, sum |a x|, the same per column of X) of the oracle on the numpy transpose of (A, V2)"""
    c, dtype = case(name), np.dtype(dtype_name).type
    a = second(name)[1]
    if mixed:
        a = a.astype(np.float32).astype(np.float64)
    one = lambda x: (oracle.csr_spmv(c.rp, c.ci, a, np.ascontiguousarray(x, dtype), dtype),
                     oracle.csr_spmv(c.rp, c.ci, np.abs(a), np.abs(np.ascontiguousarray(x, np.float64))))
    return one(c.x) + (tuple(one(c.X[:, j]) for j in range(3)),)


def create_t(eng, c, values, fmt, dtype=np.float64, **opts):
    return eng.Matrix(c.a[0], c.a[1], values, c.a_m, c.a_n, fmt, dtype, transpose=1, **opts)


def prepare(Mt, c):
    Mt.update_values_prepare_transposed(c.a[0], c.a[1], c.a_m, c.a_n)


def same_products(torch, c, Mu, Mf, dtype, what):
    """assert_same_handle, then spmv with beta 0 and 1 and a 3-column spmm, bit for bit. Returns the fresh handle's device results."""
    assert_same_handle(Mu, Mf, what)
    D = Dev(torch, c, dtype)
    out = []
    for beta in (0, 1):
        yf, yu = D.run(Mf, beta), D.run(Mu, beta)
        bad = np.nonzero(_bits(yu).reshape(-1, D.item) != _bits(yf).reshape(-1, D.item))[0]
        assert bad.size == 0, f"{what} beta={beta}: the updated handle's product differs from the fresh handle's, first at element {bad[:5] - D.G0}"
        out.append(yf)
    X = c.X.astype(dtype)
    Yf, Yu = Mf.spmm(X), Mu.spmm(X)
    assert _bits(Yu).tobytes() == _bits(Yf).tobytes(), f"{what}: spmm k=3"
    return D, out, Yf


def check_updated(eng, torch, name, fmt, dtype=np.float64, what="", expect=None, **opts):
    """Mt created with the case's values, prepared, updated with V2, against the handle freshly created from V2 (itself against the
    oracle). Returns both, open."""
    c, dtype = case(name), np.dtype(dtype).type
    V2, _ = second(name)
    what = f"{what or name} {fmt} {opts} {np.dtype(dtype).name}"
    Mf = create_t(eng, c, V2, fmt, dtype, **opts)
    Mt = create_t(eng, c, c.a[2], fmt, dtype, **opts)
    if expect:
        assert expect in Mt.format_name and expect in Mf.format_name, (what, Mt.format_name, Mf.format_name)
    assert Mt.update_values_state() == 0 and Mt.update_values_count() == Mt.nnz, what
    prepare(Mt, c)
    assert Mt.update_values_state() == 2 and Mt.update_values_count() == c.a[1].size, what
    Mt.update_values(V2)
    D, ys, Yf = same_products(torch, c, Mt, Mf, dtype, what)
    y_ref, absrow, cols = refs(name, np.dtype(dtype).name, opts.get("value_storage") == 1 and dtype == np.float64)
    for beta in (0, 1):
        compare_device_result(ys[beta], D.y0 if beta else None, y_ref, absrow, D.G0, c.m, dtype, False, f"{what} beta={beta} fresh handle")
    for j in range(3):
        check(np.ascontiguousarray(Yf[:, j]), cols[j][0], cols[j][1], dtype, False, f"{what}: spmm column {j} of the fresh handle")
    return Mt, Mf


def close(*handles):
    for M in handles:
        M.close()


# ---- 1. layouts ---------------------------------------------------------------------------------------------------------------------

SELL_LAYOUTS = [("f64", np.float64, dict(DELTA, sell_values=2), "_SELLD_"), ("f64_v7", np.float64, dict(DELTA, sell_values=1), "_SELLD_"),
                ("f32", np.float32, dict(DELTA), "_SELLD_"), ("mixed", np.float64, dict(DELTA, value_storage=1), "_v4"),
                ("plain16", np.float64, dict(PLAIN, sell_c=16, sell_sigma=16), "_SELL_16_"),
                ("plain256", np.float64, dict(PLAIN, sell_c=256, sell_sigma=256), "_SELL_256_")]


@pytest.mark.parametrize("name", ("wide", "tall"))
@pytest.mark.parametrize("store,dtype,opts,expect", SELL_LAYOUTS, ids=[s[0] for s in SELL_LAYOUTS])
def test_sell_layouts(eng, torch, name, store, dtype, opts, expect):
    for split in ((1, 4) if "sell_delta" in opts and opts["sell_delta"] == 1 else (None,)):
        more = {} if split is None else {"sell_split": split}
        close(*check_updated(eng, torch, name, "sell_c_sigma", dtype, expect=expect, **dict(opts, **more)))


CSR_LAYOUTS = ("csr_scalar", "csr_vector", "csr_stream", "csr_merge", "coo")


@pytest.mark.parametrize("name", ("wide", "tall"))
@pytest.mark.parametrize("fmt", CSR_LAYOUTS)
def test_csr_ordered_layouts(eng, torch, name, fmt):
    close(*check_updated(eng, torch, name, fmt))
    close(*check_updated(eng, torch, name, fmt, np.float32))


def test_window_layout(eng, torch):
    close(*check_updated(eng, torch, "banded", "sell_c_sigma", expect="_SELLW_", sell_window=1))
    close(*check_updated(eng, torch, "banded", "sell_c_sigma", np.float32, expect="_SELLW_", sell_window=1))


# ---- 2. what create() chooses from the values is chosen again ------------------------------------------------------------------------

def _v7_stored(M):
    return (M.stored_array("desc", np.int64)[1:-2:2] & 8) != 0


def test_seven_byte_slices_are_selected_again(eng, torch):
    """V1 in [1, 2): every slice with a full group of 4 steps stores 7-byte values. V2 = V1 with one 2^-20 in the first step of three
    slices of A^t: those leave the 7-byte store, the value array grows past its allocation. Then back to V1."""
    c = case("tall")                                            # A^t is 1000 x 1537, about 9 entries per row
    o = order_of("tall")
    V1 = np.random.default_rng(3).uniform(1.0, 1.999, c.a[1].size)
    V2 = V1.copy()
    for s in (1, 4, 7):
        row = 64 * s
        assert c.rp[row + 1] > c.rp[row]
        V2[o[c.rp[row]]] = 2.0 ** -20                           # entry 0 of a row of A^t: step 0 of its slice, inside a full group
    opts = dict(DELTA, sell_values=1, sell_split=2)
    fresh = {1: create_t(eng, c, V1, "sell_c_sigma", **opts), 2: create_t(eng, c, V2, "sell_c_sigma", **opts)}
    Mt = create_t(eng, c, V1, "sell_c_sigma", **opts)
    prepare(Mt, c)
    counts, sizes = [int(_v7_stored(Mt).sum())], [Mt.stored_array("val").size]
    for which in (2, 1):
        Mt.update_values({1: V1, 2: V2}[which])
        same_products(torch, c, Mt, fresh[which], np.float64, f"7-byte slices -> V{which}")
        np.testing.assert_array_equal(_v7_stored(Mt), _v7_stored(fresh[which]))
        counts.append(int(_v7_stored(Mt).sum()))
        sizes.append(Mt.stored_array("val").size)
    assert counts[1] == counts[0] - 3 and counts[2] == counts[0] > 3, counts
    assert sizes[1] > sizes[0] == sizes[2], sizes
    assert Mt.format_name.endswith("_v7")
    # the fresh handle of V2 against the oracle
    t_va = V2[o]
    y_ref, absrow = oracle.csr_spmv(c.rp, c.ci, t_va, c.x, np.float64), oracle.csr_spmv(c.rp, c.ci, np.abs(t_va), np.abs(c.x))
    check(fresh[2].spmv(c.x), y_ref, absrow, np.float64, False, "7-byte slices: fresh handle of V2")
    close(Mt, fresh[1], fresh[2])


def test_merge_handle_updated_with_uniform_values_becomes_the_unit_handle(eng):
    c = case("wide")
    ones = np.ones(c.a[1].size)
    Mf = create_t(eng, c, ones, "csr_merge")
    Mt = create_t(eng, c, c.a[2], "csr_merge")
    assert "_unit" in Mf.format_name and "_unit" not in Mt.format_name
    prepare(Mt, c)
    Mt.update_values(ones)
    assert Mt.format_name == Mf.format_name and Mt.mem_footprint == Mf.mem_footprint
    y_ref, absrow = oracle.csr_spmv(c.rp, c.ci, ones, c.x, np.float64), oracle.csr_spmv(c.rp, c.ci, ones, np.abs(c.x))
    yf = Mf.spmv(c.x)
    check(yf, y_ref, absrow, np.float64, False, "unit merge: fresh handle")
    np.testing.assert_array_equal(Mt.spmv(c.x), yf)
    assert Mt.update_values_state() == 0
    with pytest.raises(eng.SpmvError, match="update_values"):
        Mt.update_values(second("wide")[0])
    with pytest.raises(eng.SpmvError, match="update_values_prepare_transposed"):
        prepare(Mt, c)
    close(Mt, Mf)


# ---- 3. the map itself ---------------------------------------------------------------------------------------------------------------

def _values_by_row(M, rp_t):
    """the stored values of a SELL handle with 64-row slices in the order of the local CSR, from the decoded layout"""
    lay = M.sell_layout()
    assert lay["C"] == 64
    out = np.zeros(rp_t[-1])
    for i, o in enumerate(lay["row_of_sorted"]):
        n = rp_t[o + 1] - rp_t[o]
        out[rp_t[o]:rp_t[o + 1]] = lay["val"][lay["slice_ptr"][i // 64] + np.arange(n) * 64 + i % 64]
    return out


@pytest.mark.parametrize("name", ("duplicates", "holes", "n1", "n1024", "n1025", "hub_column"))
def test_every_entry_receives_the_value_of_its_source(eng, torch, name):
    """V2[e] = e + 1: entry e of A^t must hold order[e] + 1, through the map derived on the GPU and through the one derived on the
    host (convert_on = 2) alike — their bytes are equal"""
    c, o = case(name), order_of(name)
    nnz = c.a[1].size
    V2 = np.arange(1, nnz + 1, dtype=np.float64)
    want = (o + 1).astype(np.float64)
    for opts in (PLAIN, DELTA):
        for conv in (1, 2):
            Mt = create_t(eng, c, c.a[2], "sell_c_sigma", **dict(opts, convert_on=conv))
            prepare(Mt, c)
            Mt.update_values(V2)
            got = _values_by_row(Mt, c.rp)
            bad = np.nonzero(got != want)[0]
            assert bad.size == 0, f"{name} {opts} convert_on={conv}: {bad.size} entries of A^t hold another entry's value, first {bad[:5]}: {got[bad[:5]]} for {want[bad[:5]]}"
            y = Mt.spmv(np.ones(c.n))                           # sums of integers below 2^53: exact in any order
            np.testing.assert_array_equal(y, np.add.reduceat(np.append(want, 0.0), c.rp[:-1]) * (np.diff(c.rp) > 0))
            Mt.close()
    if name == "duplicates":                                    # equal (row, column) entries keep their input order
        a_rp, a_ci, _ = c.a
        for row in c.dup_rows:
            s, col = a_rp[row], a_ci[a_rp[row]]
            mine = np.nonzero(c.ci[c.rp[col]:c.rp[col + 1]] == row)[0] + c.rp[col]
            assert mine.size == 2 and (o[mine[0]], o[mine[1]]) == (s, s + 2)
    # a CSR-ordered layout through the product alone
    Mt = create_t(eng, c, c.a[2], "csr_vector")
    prepare(Mt, c)
    Mt.update_values(V2)
    np.testing.assert_array_equal(Mt.spmv(np.ones(c.n)), np.add.reduceat(np.append(want, 0.0), c.rp[:-1]) * (np.diff(c.rp) > 0))
    Mt.close()


def test_nnz0(eng):
    c = case("nnz0")
    for fmt, opts in (("sell_c_sigma", DELTA), ("csr_vector", {})):
        Mt = create_t(eng, c, c.a[2], fmt, **opts)
        assert Mt.update_values_state() == 0
        prepare(Mt, c)
        assert Mt.update_values_state() == 2 and Mt.update_values_count() == 0 == Mt.nnz
        Mt.update_values(np.zeros(0))
        Mt.update_values_device(0)
        np.testing.assert_array_equal(Mt.spmv(c.x), np.zeros(c.m))
        Mt.close()


# ---- 4. a row block of A^t -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt,opts", [("sell_c_sigma", dict(DELTA, sell_values=1)), ("csr_vector", {})], ids=("delta", "csr_vector"))
def test_row_block(eng, torch, fmt, opts):
    c = case("wide")                                            # A^t is 1537 x 1000
    V2, t_va = second("wide")
    r0, r1 = 70, 1301
    blk = dict(opts, row_begin=r0, row_end=r1)
    Mf = create_t(eng, c, V2, fmt, **blk)
    Mt = create_t(eng, c, c.a[2], fmt, **blk)
    lnnz = int(c.rp[r1] - c.rp[r0])
    assert Mt.m == r1 - r0 and Mt.nnz == lnnz < c.a[1].size
    prepare(Mt, c)
    assert Mt.update_values_count() == c.a[1].size and Mt.nnz == lnnz
    with pytest.raises(ValueError):
        Mt.update_values(V2[:lnnz])
    Mt.update_values(V2)                                        # ALL of A's values
    assert_same_handle(Mt, Mf, f"row block {fmt}")
    y_ref, absrow, _ = refs("wide", "float64", False)
    yf = Mf.spmv(c.x)
    check(yf, y_ref[r0:r1], absrow[r0:r1], np.float64, False, f"row block {fmt}: fresh handle")
    np.testing.assert_array_equal(Mt.spmv(c.x), yf)
    X = c.X.copy()
    assert _bits(Mt.spmm(X)).tobytes() == _bits(Mf.spmm(X)).tobytes()
    close(Mt, Mf)


# ---- 5. the handle of a stream, host entry and device entry ------------------------------------------------------------------------------

def test_create_from_stream_handle(eng, torch):
    c = case("wide")
    V2, _ = second("wide")
    a_rp, a_ci, a_va = c.a
    opts = dict(DELTA, sell_values=1)
    st = eng.CsrStream(c.a_m, c.a_n, a_ci.size + 100)
    for q0, q1 in ((0, 17), (17, 640), (640, c.a_m)):
        st.append(a_rp[q0:q1 + 1] - a_rp[q0], a_ci[a_rp[q0]:a_rp[q1]], a_va[a_rp[q0]:a_rp[q1]])
    S = st.finish("sell_c_sigma", np.float64, transpose=1, **opts)
    assert S.transposed == 1 and S.update_values_state() == 0
    prepare(S, c)
    assert S.update_values_state() == 2
    S.update_values(V2)
    Mt, Mf = check_updated(eng, torch, "wide", "sell_c_sigma", **dict(opts, convert_on=1))
    same_products(torch, c, S, Mf, np.float64, "from stream against the fresh handle")
    same_products(torch, c, S, Mt, np.float64, "from stream against the updated create() handle")
    close(S, Mt, Mf)


@pytest.mark.parametrize("fmt,opts", [("sell_c_sigma", dict(DELTA, sell_values=1, sell_split=2)), ("csr_vector", {})], ids=("delta", "csr_vector"))
def test_host_and_device_entry_give_the_same_bytes(eng, torch, fmt, opts):
    c = case("tall")
    V2, _ = second("tall")
    Mh, Mf = check_updated(eng, torch, "tall", fmt, **opts)    # the host entry
    Md = create_t(eng, c, c.a[2], fmt, **opts)
    prepare(Md, c)
    buf = torch.full((V2.size + 1,), SENTINEL, dtype=torch.float64, device="cuda")
    buf[1:] = torch.from_numpy(V2.copy()).cuda()                # one element in: 8-byte aligned only
    assert (buf.data_ptr() + 8) % 16 == 8
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    Md.update_values_device(buf.data_ptr() + 8, side.cuda_stream)
    same_products(torch, c, Md, Mh, np.float64, f"{fmt}: update_values_device against update_values")
    same_products(torch, c, Md, Mf, np.float64, f"{fmt}: update_values_device against the fresh handle")
    close(Mh, Md, Mf)


# ---- 6. protocol and refusals ---------------------------------------------------------------------------------------------------------

def test_protocol_and_refusals(eng):
    L = eng.lib()
    c = case("wide")
    a_rp, a_ci, a_va = c.a
    V2, _ = second("wide")
    nnz = a_ci.size

    def refused(M, x, call, pattern):
        before = M.spmv(x)
        with pytest.raises(eng.SpmvError, match=pattern):
            call()
        np.testing.assert_array_equal(M.spmv(x), before, err_msg=f"{M.format_name}: a refused call changed the product")

    for fmt, opts in (("sell_c_sigma", dict(DELTA, sell_values=1)), ("csr_vector", {})):
        Mt = create_t(eng, c, a_va, fmt, **opts)
        assert Mt.update_values_state() == 0
        assert b"transpose" in L.spmv_mi355x_last_error()
        refused(Mt, c.x, lambda: Mt.update_values(np.ones(Mt.nnz)), "update_values.*transpose")
        refused(Mt, c.x, lambda: Mt.update_values_prepare(c.rp), "update_values_prepare.*transpose")
        assert Mt.update_values_state() == 0
        # shapes, nnz, columns: all before the handle is touched
        P = "update_values_prepare_transposed"
        refused(Mt, c.x, lambda: Mt.update_values_prepare_transposed(a_rp[:-1], a_ci[:a_rp[-2]], c.a_m - 1, c.a_n), f"{P}.*{c.a_m - 1} x {c.a_n}.*{c.a_m} x {c.a_n}")
        refused(Mt, c.x, lambda: Mt.update_values_prepare_transposed(a_rp, a_ci, c.a_m, c.a_n + 1), f"{P}.*{c.a_m} x {c.a_n + 1}.*{c.a_m} x {c.a_n}")
        rp_short = np.minimum(a_rp, nnz - 1).astype(np.int32)
        refused(Mt, c.x, lambda: Mt.update_values_prepare_transposed(rp_short, a_ci[:nnz - 1], c.a_m, c.a_n), f"{P}.*{nnz - 1}.*{nnz}")
        bad_ci = a_ci.copy()
        bad_ci[11] = c.a_n
        refused(Mt, c.x, lambda: Mt.update_values_prepare_transposed(a_rp, bad_ci, c.a_m, c.a_n), rf"{P}.*column index {c.a_n} out of range \[0,{c.a_n}\) at entry 11")
        bad_rp = a_rp.copy()
        r = 1 + int(np.nonzero(np.diff(a_rp)[1:] > 0)[0][0])
        bad_rp[r], bad_rp[r + 1] = a_rp[r + 1], a_rp[r]
        refused(Mt, c.x, lambda: Mt.update_values_prepare_transposed(bad_rp, a_ci, c.a_m, c.a_n), f"{P}.*row_ptr is not monotone at row {r}$")
        assert Mt.update_values_state() == 0
        if fmt == "sell_c_sigma":
            # equal nnz, other column counts: a column of A that alone is the longest row of its 64-row slice of A^t loses an entry
            # to a column of another slice, so that slice's width no longer matches
            counts = np.bincount(a_ci, minlength=c.a_n)
            alone = [s for s in range(c.a_n // 64) if (counts[64 * s:64 * s + 64] == counts[64 * s:64 * s + 64].max()).sum() == 1]
            assert alone, "no slice with a single longest row"
            hi = 64 * alone[0] + int(np.argmax(counts[64 * alone[0]:64 * alone[0] + 64]))
            other = a_ci.copy()
            e = int(np.nonzero(a_ci == hi)[0][0])
            other[e] = hi + 64 if hi + 64 < c.a_n else hi - 64
            refused(Mt, c.x, lambda: Mt.update_values_prepare_transposed(a_rp, other, c.a_m, c.a_n), f"{P}.*does not match the pattern")
            assert Mt.update_values_state() == 0
        prepare(Mt, c)
        assert Mt.update_values_state() == 2
        refused(Mt, c.x, lambda: Mt.update_values_prepare(c.rp), "update_values_prepare.*transpose")
        assert Mt.update_values_state() == 2                    # a prepared handle stays prepared
        prepare(Mt, c)                                          # twice is allowed
        Mt.update_values(V2)
        Mf = create_t(eng, c, V2, fmt, **opts)
        assert_same_handle(Mt, Mf, f"{fmt} after the refusals")
        np.testing.assert_array_equal(Mt.spmv(c.x), Mf.spmv(c.x))
        close(Mt, Mf)

    # handles the entry does not serve
    M0 = eng.Matrix(a_rp, a_ci, a_va, c.a_m, c.a_n, "csr_vector")
    xa = np.random.default_rng(8).uniform(-1, 1, c.a_n)
    refused(M0, xa, lambda: M0.update_values_prepare_transposed(a_rp, a_ci, c.a_m, c.a_n), "update_values_prepare_transposed.*transpose = 1")
    assert M0.update_values_state() == 1 and M0.update_values_count() == M0.nnz
    M0.close()
    Mc = create_t(eng, c, a_va, "csr_vector", col_begin=100, col_end=640, col_filter_mode=1)
    refused(Mc, c.x, lambda: Mc.update_values_prepare_transposed(a_rp, a_ci, c.a_m, c.a_n), "update_values_prepare_transposed.*column filter")
    assert Mc.update_values_state() == 0
    Mc.close()


# ---- 7. the pair: one array of new values refreshes A and A^t --------------------------------------------------------------------------

def test_cgls_pair_updated_from_one_array(eng):
    """the well-conditioned tall problem of the CGLS tests (singular values within a factor 1.7, asserted there and again here for
    V2), delta layout. x of the fresh pair against numpy.linalg.lstsq on the stacked system to kappa^2 * tol = 3e-12 (test_gpu_cgls's
    bound); the updated pair against the fresh pair bit for bit."""
    from test_gpu_cgls import _same, problem
    P = problem(3000, 1100)
    rp, ci, V1 = P.csr
    V2 = V1 * np.random.default_rng(12).uniform(1.0, 1.05, V1.size)
    D2 = np.zeros((P.m, P.n))
    D2[np.repeat(np.arange(P.m), np.diff(rp)), ci] = V2
    sv = np.linalg.svd(D2, compute_uv=False)
    assert sv[0] / sv[-1] <= 1.7
    damp = 0.25
    want = np.linalg.lstsq(np.vstack([D2, np.sqrt(damp) * np.eye(P.n)]), np.concatenate([P.b, np.zeros(P.n)]), rcond=None)[0]
    Af, Atf = P.handles(eng, "sell_c_sigma", np.float64, values=V2, **DELTA)
    A, At = P.handles(eng, "sell_c_sigma", np.float64, **DELTA)
    A.update_values_prepare(rp)
    At.update_values_prepare_transposed(rp, ci, P.m, P.n)
    A.update_values(V2)
    At.update_values(V2)
    fresh = Af.cgls(Atf, P.b, damp=damp)
    assert fresh["stop"] == 1 and fresh["iterations"] > 0
    assert np.linalg.norm(fresh["x"] - want) <= 3e-12 * np.linalg.norm(want)
    _same(A.cgls(At, P.b, damp=damp), fresh, "updated pair against the fresh pair")
    close(A, At, Af, Atf)
