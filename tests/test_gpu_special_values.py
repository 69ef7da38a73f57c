"""NaN, Inf and subnormals through every SpMV variant (-m gpu). The contract (include/spmv_mi355x.h, "special values"):

  1. confinement: y[i] of y = A x / y += A x is non-finite exactly for the rows i that store an entry in a column j with non-finite
     x[j]; every other row is finite and meets the bar it meets on finite input (bit-equal to the oracle for the row-sequential
     variants, TOL * sum|a x| otherwise). Whether a reached row holds Inf or NaN is not pinned: the count of rows that differ in kind
     from the oracle is printed;
  2. overwriting: beta = 0 overwrites y whatever it held, NaN included;
  3. subnormal products are not flushed.

The matrices (special_values_cases.py) hold empty and non-empty rows of many lengths in every 64-row slice, so that every padded
layout pads, in the 8-bit, 16-bit and int32 index modes of the delta layout. Beside the eight poison vectors of a case every layout
that sell_layout() decodes is poisoned where it hurts: at columns it holds at a zero-valued padding position of a row that does not
store them. Before any launch on poisoned data the decoded columns are checked to lie in [0, n).

Triangular solves: one Inf in b reaches exactly the rows that depend on its row."""
import numpy as np
import pytest
import scipy.sparse as sp

import special_values_cases as sv
import trsv_blocked_cases as bc
import trsv_cases as tc
from test_gpu_parity import ATOMIC_LAYOUTS, IDS, SENTINEL, TOL, VARIANTS, check, compare_device_result
from trsv_cases import LOWER, UPPER

pytestmark = pytest.mark.gpu

DTYPES = (np.float64, np.float32)
OX, G0, G1 = 1, 3, 2                               # x starts OX elements into its buffer; guards in front of and behind y


@pytest.fixture(scope="module")
def eng():
    import spmv_mi355x as eng
    assert eng.device_count() >= 1, "no GPU visible: the -m gpu tests need an MI355X"
    return eng


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def _tdt(torch, dtype):
    return torch.float64 if np.dtype(dtype) == np.float64 else torch.float32


def _build(eng, case, fmt, dtype, opts):
    """the handle, or None where a FORCED LDS-window layout refuses a shape whose slice groups span more than 65 536 columns or 128 KiB
    of x (the refusal test_synthetic_all_formats accepts)"""
    try:
        return eng.Matrix(case["rp"], case["ci"], case["va"], case["m"], case["n"], fmt, dtype, **opts)
    except eng.SpmvError as e:
        assert opts.get("sell_window") == 1 and "sell_window" in str(e) and case["n"] * np.dtype(dtype).itemsize > 128 * 1024, str(e)
        return None


class Device:
    """x and a guarded y on the device for one handle: launch() runs spmv_device and returns the whole y buffer"""

    def __init__(self, torch, A, dtype):
        self.torch, self.A, self.dtype = torch, A, dtype
        self.tdt = _tdt(torch, dtype)
        self.item = np.dtype(dtype).itemsize
        self.xbuf = torch.full((OX + A.n,), SENTINEL, dtype=self.tdt, device="cuda")

    def set_x(self, x):
        self.xbuf[OX:] = self.torch.from_numpy(np.array(x, dtype=self.dtype)).cuda()          # (a copy: the cases' arrays are read-only)

    def launch(self, beta, y_init=None, fill=SENTINEL):
        torch, m = self.torch, self.A.m
        ybuf = torch.full((G0 + m + G1,), SENTINEL, dtype=self.tdt, device="cuda")
        if y_init is not None:
            ybuf[G0:G0 + m] = torch.from_numpy(y_init).cuda()
        elif fill != SENTINEL:
            ybuf[G0:G0 + m] = fill
        torch.cuda.synchronize()
        self.A.spmv_device(self.xbuf.data_ptr() + OX * self.item, ybuf.data_ptr() + G0 * self.item, beta, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return ybuf.cpu().numpy()


def _confined(ybuf, g0, g1, expect, dtype, exact, what, y0=None):
    """ybuf = [g0 guards | m values | g1 guards]: the finite rows are the oracle's finite rows, they meet compare_device_result's bars (the
    guards with them), and the number of reached rows whose kind (Inf / NaN) differs from the oracle's is returned."""
    y_ref, finite, absrow = expect
    m = len(y_ref)
    y = ybuf[g0:g0 + m]
    got = np.isfinite(y)
    bad = np.nonzero(got != finite)[0]
    assert bad.size == 0, (f"{what}: {bad.size} rows differ from the oracle in being finite; rows {bad[:8]}: y {y[bad[:8]]!r}, "
                           f"oracle {y_ref[bad[:8]]!r}")
    packed = np.concatenate([ybuf[:g0], y[finite], ybuf[g0 + m:]])
    compare_device_result(packed, None if y0 is None else y0[finite], y_ref[finite], absrow[finite], g0, int(finite.sum()), dtype, exact, what)
    return int(np.sum(np.isnan(y[~finite]) != np.isnan(y_ref[~finite])))


def _padding_columns(A, case):
    """From sell_layout(): every decoded column lies in [0, n) — asserted here, on the host, before anything is launched on poisoned
    data — and the columns the layout holds at a zero-valued position of a row that does not store them (rows past the last one
    count: their lanes gather too). None when the handle's layout is not one sell_layout() decodes."""
    import spmv_mi355x as eng
    try:
        lay = A.sell_layout()
    except eng.SpmvError:
        return None
    C, sp_, col, val, ros = lay["C"], lay["slice_ptr"], lay["col"], lay["val"], lay["row_of_sorted"]
    assert col.size == val.size == sp_[-1]
    bad = np.nonzero((col < 0) | (col >= case["n"]))[0]
    assert bad.size == 0, f"{A.format_name}: {bad.size} stored positions hold a column outside [0, {case['n']}): position {bad[:5]} column {col[bad[:5]]}"
    pos = np.arange(col.size)
    sl = np.searchsorted(sp_, pos, side="right") - 1
    sorted_row = sl * C + (pos - sp_[sl]) % C
    row = np.where(sorted_row < case["m"], ros[np.minimum(sorted_row, case["m"] - 1)], -1)
    stored = set(zip(np.repeat(np.arange(case["m"]), case["lens"]).tolist(), case["ci"].tolist()))
    pad = np.nonzero(val == 0)[0]                   # no stored value of these cases is 0
    foreign = sorted({int(col[p]) for p in pad if (int(row[p]), int(col[p])) not in stored})
    return foreign


def _pick(cols, count=4):
    if len(cols) <= count:
        return list(cols)
    return [cols[i] for i in np.linspace(0, len(cols) - 1, count).round().astype(int)]


PARAMS = [(ci_, vi) for ci_ in range(len(sv.SHAPES)) for vi in range(len(VARIANTS))
          if sv.NAMES[ci_] != sv.INT32_ONLY or VARIANTS[vi][0] == "sell_c_sigma"]


@pytest.mark.parametrize("ci_,vi", PARAMS, ids=[f"{sv.NAMES[c]}-{IDS[v]}" for c, v in PARAMS])
def test_spmv_confines_overwrites_and_keeps_subnormals(eng, torch, oracle, ci_, vi):
    case = sv.ragged(*sv.SHAPES[ci_])
    fmt, opts, exact = VARIANTS[vi]
    columns, vectors = sv.poison_vectors(case)
    m = case["m"]
    for dtype in DTYPES:
        A = _build(eng, case, fmt, dtype, opts)
        if A is None:
            print(f"{case['name']} {IDS[vi]} {np.dtype(dtype).name}: the forced window layout refuses this shape")
            continue
        what = f"{case['name']}/{A.format_name}/{IDS[vi]}"
        atomic = any(t in A.format_name for t in ATOMIC_LAYOUTS)
        dev = Device(torch, A, dtype)
        y0 = (np.random.default_rng(77 + vi).uniform(-1, 1, m) * 8).astype(dtype)
        guards = np.full(G0, SENTINEL, dtype), np.full(G1, SENTINEL, dtype)
        # ---- the layout's own columns, checked on the host before the first poisoned launch
        foreign = _padding_columns(A, case)
        # ---- confinement: the eight vectors, host path and device call, beta 0 and beta 1
        kinds = 0
        for k, x in enumerate(vectors):
            expect = sv.expectation(case, k, dtype)
            tag = f"{what} x[{columns[k]}] = {sv.POISON[k % 3]}"
            y_host = A.spmv(x)
            kinds += _confined(np.concatenate([guards[0], y_host, guards[1]]), G0, G1, expect, dtype, exact, tag + " host path")
            dev.set_x(x)
            yb = dev.launch(0)
            kinds += _confined(yb, G0, G1, expect, dtype, exact, tag + " device beta=0")
            if not atomic:
                np.testing.assert_array_equal(yb[G0:G0 + m][expect[1]], y_host[expect[1]], err_msg=tag + ": device path vs host path")
            kinds += _confined(dev.launch(1, y0), G0, G1, expect, dtype, exact, tag + " device beta=1", y0=y0)
        # ---- adversarial columns: what the decoded layout holds at padding positions of rows that do not store it
        if foreign is None:
            print(f"{what}: no decodable SELL layout, the eight vectors only")
        elif not foreign:
            print(f"{what}: the layout holds no padding column that the padded row does not store")
        else:
            print(f"{what}: {len(foreign)} columns sit at padding positions of rows that do not store them; poisoning {_pick(foreign)}")
            for k, c in enumerate(_pick(foreign)):
                expect = sv.expectation_at(case, c, k, dtype)
                dev.set_x(sv.poisoned(case, c, k))
                kinds += _confined(dev.launch(0), G0, G1, expect, dtype, exact, f"{what} padding column x[{c}] = {sv.POISON[k % 3]} ({len(foreign)} such columns)")
        print(f"{what}: {kinds} reached rows differ in kind (Inf / NaN) from the oracle")
        # ---- overwriting: beta = 0 into a y of NaN (x[0] = Inf: no row stores column 0, every y is finite)
        expect = sv.expectation(case, 0, dtype)
        dev.set_x(vectors[0])
        plain = dev.launch(0)
        over = dev.launch(0, fill=float("nan"))
        _confined(over, G0, G1, expect, dtype, exact, what + " beta=0 into NaN")
        assert np.all(np.isfinite(over[G0:G0 + m])), what + ": beta=0 left a NaN of the old y"
        if not atomic:
            np.testing.assert_array_equal(over, plain, err_msg=what + ": beta=0 into NaN vs into the sentinel")
        # ---- subnormals: every product subnormal
        x, y_ref, absrow = sv.subnormal(case, dtype)
        dev.set_x(x)
        yb = dev.launch(0)
        y = yb[G0:G0 + m]
        assert np.all(yb[:G0] == dtype(SENTINEL)) and np.all(yb[G0 + m:] == dtype(SENTINEL)), what + ": guards (subnormal x)"
        bound = sv.subnormal_bound(case, absrow, dtype, TOL[dtype])
        err = np.abs(y.astype(np.float64) - y_ref.astype(np.float64))
        unit = sv.SUBNORMAL_UNIT[dtype]
        print(f"{what}: subnormal x: max |y - y_ref| = {err.max() / unit:.1f} units, y non-zero in {np.count_nonzero(y)} rows (oracle {np.count_nonzero(y_ref)})")
        if exact:
            np.testing.assert_array_equal(y, y_ref, err_msg=what + ": subnormal products")
        else:
            bad = np.nonzero(err > bound)[0]
            assert bad.size == 0, f"{what}: subnormal products: {bad.size} rows beyond the bound; rows {bad[:5]} err/unit {err[bad[:5]] / unit} y {y[bad[:5]]!r} y_ref {y_ref[bad[:5]]!r}"
        A.close()


# ---- SpMM: X holds the eight poison vectors, one per column ---------------------------------------------------------------------------

SPMM_VARIANTS = [
    ("sell_c_sigma", {"sell_c": 64, "sell_split": 1}, True, True),           # (format, options, exact, runs the int32 shape)
    ("sell_c_sigma", {"sell_c": 64, "sell_split": 1, "sell_sigma": 64}, True, True),
    ("sell_c_sigma", {"sell_split": 2}, False, True),
    ("sell_c_sigma", {"sell_split": 4, "sell_sigma": 128}, False, True),
    ("sell_c_sigma", {"sell_c": 64, "sell_split": 1, "sell_values": 1, "sell_sigma": 64}, True, True),
    ("sell_c_sigma", {"sell_window": 1, "sell_split": 1}, True, False),
    ("sell_c_sigma", {"sell_window": 1, "sell_split": 2, "sell_group": 4}, False, False),
    ("sell_c_sigma", {"sell_window": 1, "sell_split": 4, "sell_group": 1}, False, False),
    ("sell_c_sigma", {"sell_c": 32, "sell_sigma": 256}, False, False),
    ("sell_c_sigma", {"sell_c": 256}, True, False),
    ("csr_scalar", {}, True, False),
    ("csr_vector", {}, False, False),
    ("csr_stream", {}, False, False),
    ("csr_merge", {}, False, False),
    ("coo", {}, False, False),
    ("coo", {"col_blocks": -1}, False, False),
]
SPMM_PARAMS = [(c, v) for c in range(len(sv.SHAPES)) for v in range(len(SPMM_VARIANTS)) if sv.NAMES[c] != sv.INT32_ONLY or SPMM_VARIANTS[v][3]]


def _spmm_id(c, v):
    f, o, _, _ = SPMM_VARIANTS[v]
    return f"{sv.NAMES[c]}-{f}-{'-'.join(f'{k}{x}' for k, x in o.items()) or 'default'}"


@pytest.mark.parametrize("ci_,vi", SPMM_PARAMS, ids=[_spmm_id(c, v) for c, v in SPMM_PARAMS])
def test_spmm_confines_per_column(eng, torch, oracle, ci_, vi):
    case = sv.ragged(*sv.SHAPES[ci_])
    fmt, opts, exact, _ = SPMM_VARIANTS[vi]
    columns, vectors = sv.poison_vectors(case)
    m, n, k = case["m"], case["n"], len(vectors)
    X = np.stack(vectors, axis=1)
    for dtype in DTYPES:
        A = _build(eng, case, fmt, dtype, opts)
        if A is None:
            print(f"{_spmm_id(ci_, vi)} {np.dtype(dtype).name}: the forced window layout refuses this shape")
            continue
        what = f"{case['name']}/{A.format_name} spmm"
        tdt = _tdt(torch, dtype)
        Xd = torch.from_numpy(np.ascontiguousarray(X, dtype)).cuda()
        y0 = (np.random.default_rng(5).uniform(-1, 1, (m, k)) * 8).astype(dtype)
        results = [("host", A.spmm(X), None)]
        for beta in (0, 1):
            Yd = torch.full((G0 + m + G1, k), SENTINEL, dtype=tdt, device="cuda")
            if beta:
                Yd[G0:G0 + m] = torch.from_numpy(y0).cuda()
            torch.cuda.synchronize()
            A.spmm_device(k, Xd.data_ptr(), k, Yd.data_ptr() + G0 * k * np.dtype(dtype).itemsize, k, beta, torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            results.append((f"device beta={beta}", Yd.cpu().numpy(), y0 if beta else None))
        kinds = 0
        for tag, Y, init in results:
            for j in range(k):
                ybuf = Y[:, j] if Y.shape[0] > m else np.concatenate([np.full(G0, SENTINEL, dtype), Y[:, j], np.full(G1, SENTINEL, dtype)])
                kinds += _confined(np.ascontiguousarray(ybuf), G0, G1, sv.expectation(case, j, dtype), dtype, exact,
                                   f"{what} {tag} column {j}: x[{columns[j]}] = {sv.POISON[j % 3]}", y0=None if init is None else np.ascontiguousarray(init[:, j]))
        print(f"{what}: {kinds} reached entries differ in kind (Inf / NaN) from the oracle")
        A.close()


# ---- other handle kinds: fp32-stored values under fp64 vectors, transposed handles ----------------------------------------------------

@pytest.mark.parametrize("split", (1, 2, 4))
@pytest.mark.parametrize("ci_", range(len(sv.SHAPES)), ids=sv.NAMES)
def test_fp32_stored_values_confine(eng, torch, oracle, ci_, split):
    """value_storage = 1: fp64 vectors over values stored as fp32. The eight vectors, against the oracle on the values rounded to fp32; and
    a Matrix value of 1e300, which narrows to Inf: exactly the rows that hold it are non-finite."""
    case = sv.ragged(*sv.SHAPES[ci_])
    rp, ci, m, n = case["rp"], case["ci"], case["m"], case["n"]
    columns, vectors = sv.poison_vectors(case)
    exact = split == 1
    va32 = case["va"].astype(np.float32).astype(np.float64)
    for sigma in (64, 16384):
        A = eng.Matrix(rp, ci, case["va"], m, n, "sell_c_sigma", np.float64, value_storage=1, sell_split=split, sell_sigma=sigma)
        assert A.value_dtype == np.float32 and A.dtype == np.float64 and "_v4" in A.format_name, A.format_name
        what = f"{case['name']}/{A.format_name}"
        dev = Device(torch, A, np.float64)
        _padding_columns(A, case)
        kinds = 0
        for k, x in enumerate(vectors):
            y_ref = oracle.csr_spmv(rp, ci, va32, x)
            _, finite, absrow = sv.expectation(case, k, np.float64)
            expect = (y_ref, finite, absrow)
            kinds += _confined(np.concatenate([np.full(G0, SENTINEL), A.spmv(x), np.full(G1, SENTINEL)]), G0, G1, expect, np.float64, exact,
                               f"{what} x[{columns[k]}] host path")
            dev.set_x(x)
            kinds += _confined(dev.launch(0), G0, G1, expect, np.float64, exact, f"{what} x[{columns[k]}] device beta=0")
        print(f"{what}: {kinds} reached rows differ in kind (Inf / NaN) from the oracle")
        A.close()
        # a value that narrows to Inf, finite x
        va = case["va"].copy()
        hit = np.array([7, 2500, sv.NNZ - 1])
        va[hit] = (1e300, -1e300, 1e300)
        holds = np.zeros(m, bool)
        holds[np.searchsorted(rp, hit, side="right") - 1] = True
        x = sv.poisoned(case, 0, 0)
        x[0] = 0.25
        B = eng.Matrix(rp, ci, va, m, n, "sell_c_sigma", np.float64, value_storage=1, sell_split=split, sell_sigma=sigma)
        with np.errstate(over="ignore"):
            y_ref = oracle.csr_spmv(rp, ci, va.astype(np.float32).astype(np.float64), x)
        np.testing.assert_array_equal(np.isfinite(y_ref), ~holds)
        absrow = oracle.csr_spmv(rp, ci, np.abs(np.where(np.abs(va) > 1, 0.0, va)), np.abs(x))
        _confined(np.concatenate([np.full(G0, SENTINEL), B.spmv(x), np.full(G1, SENTINEL)]), G0, G1, (y_ref, ~holds, absrow), np.float64, exact,
                  f"{what}: 1e300 stored as fp32")
        B.close()


@pytest.mark.parametrize("dtype", DTYPES, ids=("f64", "f32"))
@pytest.mark.parametrize("ci_", range(len(sv.SHAPES)), ids=sv.NAMES)
def test_transposed_handles_confine(eng, torch, oracle, ci_, dtype):
    """transpose = 1: the handle of A^t, against the oracle on the scipy transpose. x has one entry per ROW of A; poisoning row i's
    reaches exactly the columns row i stores. Rows 100 (40 entries), 0, a row of one entry, an empty row, the last row."""
    case = sv.ragged(*sv.SHAPES[ci_])
    m, n = case["m"], case["n"]
    At = sp.csr_matrix((case["va"], case["ci"], case["rp"]), shape=(m, n)).T.tocsr()
    At.sort_indices()
    trp, tci, tva = At.indptr.astype(np.int32), At.indices.astype(np.int32), At.data
    base = np.random.default_rng(9).uniform(-1, 1, m)
    one = int(np.nonzero(case["lens"] == 1)[0][0])
    for split, exact in ((1, True), (4, False)):
        A = eng.Matrix(case["rp"], case["ci"], case["va"], m, n, "sell_c_sigma", dtype, transpose=1, sell_split=split)
        assert A.transposed == 1 and (A.m, A.n) == (n, m)
        what = f"{case['name']}/{A.format_name} transposed"
        dev = Device(torch, A, dtype)
        kinds = 0
        for k, i in enumerate((100, 0, one, 3, m - 1)):
            x = base.copy()
            x[i] = sv.POISON[k % 3]
            y_ref = oracle.csr_spmv(trp, tci, tva, x, dtype)
            reached = np.zeros(n, bool)
            reached[case["ci"][case["rp"][i]:case["rp"][i + 1]]] = True
            np.testing.assert_array_equal(np.isfinite(y_ref), ~reached)
            x[i] = 0.0
            absrow = oracle.csr_spmv(trp, tci, np.abs(tva), np.abs(x))
            x[i] = sv.POISON[k % 3]
            dev.set_x(x)
            kinds += _confined(dev.launch(0), G0, G1, (y_ref, ~reached, absrow), dtype, exact, f"{what} x[{i}] = {sv.POISON[k % 3]}")
        print(f"{what}: {kinds} reached rows differ in kind (Inf / NaN) from the oracle")
        A.close()


# ---- triangular solves: one Inf in b ------------------------------------------------------------------------------------------------------

def _reach(rp, ci, n, uplo, start):
    """the rows whose x depends on x[start]: start itself and, in solve order, every row that stores a reached column off its diagonal"""
    hit = np.zeros(n, bool)
    hit[start] = True
    for i in (range(n) if uplo == LOWER else range(n - 1, -1, -1)):
        c = ci[rp[i]:rp[i + 1]]
        c = c[c < i] if uplo == LOWER else c[c > i]
        if len(c) and hit[c].any():
            hit[i] = True
    return hit


def _inf_row(rp, ci, n, uplo):
    """a row with dependents: of seven rows spread over those that some other row stores off its diagonal, the one that reaches the
    most rows without reaching all of them"""
    rows = np.repeat(np.arange(n), np.diff(rp))
    used = np.unique(ci[ci < rows] if uplo == LOWER else ci[ci > rows])
    assert used.size > 0
    best, most = int(used[used.size // 2]), 0
    for c in used[np.linspace(0, used.size - 1, 7).round().astype(int)]:
        reach = int(_reach(rp, ci, n, uplo, int(c)).sum())
        if most < reach < n:
            best, most = int(c), reach
    return best


TRSV_HANDLES = [("plain", dict(chain_rows=0)), ("plain-chain64", dict(chain_rows=64)), ("plain-chain65536", dict(chain_rows=65536)),
                ("blocked64", dict(block_rows=64)), ("blocked1024", dict(block_rows=1024))]


@pytest.mark.parametrize("dtype", DTYPES, ids=("f64", "f32"))
@pytest.mark.parametrize("uplo,side", ((LOWER, "lower"), (UPPER, "upper")), ids=("lower", "upper"))
@pytest.mark.parametrize("name", ("dag", "prescribed", "padding"))
def test_an_inf_in_b_reaches_its_dependents_only(eng, torch, name, uplo, side, dtype):
    from test_gpu_trsv import device_solve
    for tag, opts in TRSV_HANDLES:
        A = bc.matrix(name, uplo) if "block_rows" in opts else tc.matrix(name, uplo)
        R = bc.filtered(*A, opts["block_rows"]) if "block_rows" in opts else A
        rp, ci, va, n = R
        start = _inf_row(rp, ci, n, uplo)
        b = np.random.default_rng(11).uniform(-1, 1, n).astype(dtype)
        b[start] = np.inf
        with np.errstate(invalid="ignore", over="ignore"):
            want = tc.reference(rp, ci, va, n, uplo, False, b, dtype)
        reached = _reach(rp, ci, n, uplo, start)
        np.testing.assert_array_equal(np.isfinite(want), ~reached, err_msg=f"{name} {tag}: the reference's finite rows are not the unreached ones")
        assert 1 < reached.sum() < n, f"{name} {tag}: row {start} reaches {reached.sum()} of {n} rows"
        T = eng.TriangularSolve(*A, uplo=side, diag="stored", dtype=dtype, **opts)
        got = device_solve(T, b, dtype)
        T.close()
        what = f"{name}/{tag}/{side}/{np.dtype(dtype).name}: b[{start}] = Inf reaches {int(reached.sum())} of {n} rows"
        bad = np.nonzero(np.isfinite(got) != ~reached)[0]
        assert bad.size == 0, f"{what}: {bad.size} rows differ from the reference in being finite; rows {bad[:8]}: x {got[bad[:8]]!r}"
        np.testing.assert_array_equal(got[~reached], want[~reached], err_msg=what)
        print(f"{what}; {int(np.sum(np.isnan(got[reached]) != np.isnan(want[reached])))} reached rows differ in kind")
