"""The paths of sell_delta_kernel with 7-byte values (kernels_sell.hip) behind its own workgroup size and the tile map it derives from
the handle's (sell_delta_tile_map): fp64 sell_c_sigma handles with sell_values = 1, which forces 7-byte values on small matrices. y is
compared BIT FOR BIT with the same matrix under SPMV_MI355X_SELL_VALUES=2 (the 8-byte path) and with the sequential CSR loop of the
oracle, for y = A x and for y += A x (a slice dealt twice, or not at all, shows in the second).

Shapes: slice widths of 1, 3, 4, 5, 8, 14 and 41 steps (below one group; 1 - 3 tail steps; whole groups only; the 4 + 3 + 2 + 1 group
trips of the slice loop) times m = 64, 65, 127 and 64 * 9 + 1 rows (one full slice; a last slice of one row; two slices; ten slices,
no multiple of the four slices per tile the handle's map counts in, so the derived map ends inside a tile of the handle's). Row
lengths: all equal (the sorted order is the identity: every slice holds 64 consecutive rows), every second row short (no slice
does), ragged with empty rows (padding). Columns: affine as a stencil's (the index-free modes) and random (8-, 16-, 32-bit deltas).
Values: with and without explicit 0.0 / -0.0, and one case with denormals."""
import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu

WIDTHS = (1, 3, 4, 5, 8, 14, 41)
ROWS = (64, 65, 127, 64 * 9 + 1)
COMMON = dict(sell_c=64, sell_delta=1, sell_split=1, sell_window=2)


@pytest.fixture(scope="module")
def eng():
    import spmv_mi355x as eng
    assert eng.device_count() >= 1, "no GPU visible: the -m gpu tests need an MI355X"
    return eng


def _matrix(rng, m, w, lengths, columns, zeros):
    """CSR of m rows of at most w entries. lengths: 'full' | 'alt' | 'ragged'; columns: 'affine' | 'random'."""
    if lengths == "full":
        ln = np.full(m, w)
    elif lengths == "alt":
        ln = np.where(np.arange(m) % 2 == 0, w, max(1, w // 2))
    else:
        ln = rng.integers(0, w + 1, m)
        ln[rng.integers(0, m)] = w
    if columns == "affine":
        n = m + 7 * w
        steps = np.arange(w) * 7
        cols = [i + steps[:ln[i]] for i in range(m)]
    else:
        n = (250, 60000, 200000)[int(rng.integers(0, 3))]                     # 8-, 16- or 32-bit deltas
        cols = [np.sort(rng.choice(n, ln[i], replace=False)) for i in range(m)]
    rp = np.concatenate([[0], np.cumsum(ln)]).astype(np.int32)
    ci = (np.concatenate(cols) if rp[-1] else np.zeros(0)).astype(np.int32)
    nnz = int(rp[-1])
    va = rng.uniform(0.25, 1.0, nnz) * rng.choice([-1.0, 1.0], nnz)          # exponents 1021 .. 1022: every full group qualifies
    va[rng.uniform(size=nnz) < 0.1] = 4.0
    if zeros:
        va[rng.uniform(size=nnz) < 0.1] = 0.0
        va[rng.uniform(size=nnz) < 0.02] = -0.0
    return rp, ci, va, n


def _consecutive_slices(ros, m):
    """per FULL slice: do its 64 sorted rows run r0 .. r0 + 63"""
    full = m // 64
    r = ros[:full * 64].reshape(full, 64).astype(np.int64)
    return np.all(r == r[:, :1] + np.arange(64)[None, :], axis=1)


def _both_products(M, x, y0):
    """y = A x through the host entry, and y0 + A x through the device entry with beta = 1"""
    y = M.spmv(x)
    M.upload_x(x)
    M.upload_y(y0)
    M.spmv_device(M.x_device(), M.y_device(), beta=1)
    return y, M.download_y()


def _check(eng, monkeypatch, rp, ci, va, m, n, rng, what, sigma, conv):
    x = rng.uniform(-1, 1, n)
    y0 = rng.uniform(-1, 1, m)
    y_seq = oracle.csr_spmv(rp, ci, va, x, np.float64, num_threads=1)
    opts = dict(COMMON, sell_sigma=sigma, convert_on=conv)
    monkeypatch.setenv("SPMV_MI355X_SELL_VALUES", "2")
    P = eng.Matrix(rp, ci, va, m, n, "sell_c_sigma", np.float64, sell_values=1, **opts)
    monkeypatch.delenv("SPMV_MI355X_SELL_VALUES")
    V = eng.Matrix(rp, ci, va, m, n, "sell_c_sigma", np.float64, sell_values=1, **opts)
    assert "_v7" not in P.format_name, what
    y8, y8b = _both_products(P, x, y0)
    y7, y7b = _both_products(V, x, y0)
    np.testing.assert_array_equal(y7, y8, err_msg=what + ": 7-byte against 8-byte values")
    np.testing.assert_array_equal(y7, y_seq, err_msg=what + ": against the CSR oracle")
    np.testing.assert_array_equal(y7b, y8b, err_msg=what + ": y += A x, 7-byte against 8-byte values")
    np.testing.assert_array_equal(y7b, y0 + y_seq, err_msg=what + ": y += A x against the CSR oracle")
    ros = V.stored_array("row_of_sorted", np.int32)
    name = V.format_name
    P.close()
    V.close()
    return name, ros


@pytest.mark.parametrize("w", WIDTHS)
def test_widths_rows_orders(eng, monkeypatch, w):
    rng = np.random.default_rng(1300 + w)
    case = 0
    for m in ROWS:
        for lengths in ("full", "alt", "ragged"):
            for columns in ("affine", "random"):
                case += 1
                zeros = case % 2 == 0
                rp, ci, va, n = _matrix(rng, m, w, lengths, columns, zeros)
                what = f"w={w} m={m} {lengths} {columns} zeros={zeros}"
                name, ros = _check(eng, monkeypatch, rp, ci, va, m, n, rng, what, sigma=64 if case % 3 else 4096, conv=1 + case % 2)
                if lengths == "full":
                    # equal lengths, stable sort: the identity, every slice consecutive — and with w >= 4 every slice in 7 bytes
                    np.testing.assert_array_equal(ros, np.arange(m), err_msg=what)
                    assert _consecutive_slices(ros, m).all(), what
                    assert name.endswith("_v7") == (w >= 4), (what, name)
                if lengths == "alt" and w >= 2:
                    assert not _consecutive_slices(ros, m).any(), what


def test_denormals(eng, monkeypatch):
    """exponent code 0 in full groups of compressed slices: denormals beside normal values, in consecutive and other slices"""
    rng = np.random.default_rng(77)
    for lengths in ("full", "alt"):
        m, w = 64 * 3 + 5, 9
        rp, ci, va, n = _matrix(rng, m, w, lengths, "affine", True)
        va[rp[3] + 1] = 5e-310
        va[rp[70] + 2] = -(2.0 ** -1074)
        va[rp[140]] = 2.0 ** -1030
        name, _ = _check(eng, monkeypatch, rp, ci, va, m, n, rng, f"denormals {lengths}", sigma=64, conv=1)
        assert name.endswith("_v7"), name
