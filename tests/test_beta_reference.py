"""CPU tier of the y += A x checks of tests/test_gpu_parity.py (check_device_call): the reference side alone, no GPU.

  * The bound the GPU tests hold a kernel to, |y - (y0 + y_ref)| <= tol * (sum|a x| + |y0|), is met by correct arithmetic in another
    summation order: the oracle's sequential product + y0 rounded in the handle's precision, against the oracle's threaded product
    and its merge-path product (rows cut between threads, partial sums recombined) + y0 in fp64 — on the SYNTH inputs, fp64 and fp32.
    Rows without entries come back as y0 exactly.
  * The comparison has teeth: compare_device_result accepts the correct buffer and rejects, naming the row, a y0 added twice, a y0
    dropped, an empty row off by one ulp, and a changed guard value — the failures a wrong `beta ? *yp + s : s` store, a carry
    fix-up, a superfluous clear or a store past rows() would produce."""
import numpy as np
import pytest

from conftest import MANIFEST
from test_gpu_parity import OFFSETS, SENTINEL, SYNTH, compare_device_result, device_layout, synth


def _inputs(kind, m, n):
    rng = np.random.default_rng(MANIFEST["seed"])
    rp, ci, a = synth(rng, m, n, kind)
    x = rng.uniform(-1, 1, n)
    return rp, ci, a, x


def _buffer(y, g0, g1, dtype):
    return np.concatenate([np.full(g0, SENTINEL, dtype), y.astype(dtype), np.full(g1, SENTINEL, dtype)])


def test_device_layout_covers_every_offset_pair():
    seen = {device_layout(i)[:2] for i in range(9)}
    assert seen == {(ox, g0) for ox in OFFSETS for g0 in OFFSETS}
    for i in range(60):
        ox, g0, g1, side_beta = device_layout(i)
        assert ox in OFFSETS and g0 in OFFSETS and g1 >= 1 and side_beta in (0, 1)
    assert {device_layout(i)[3] for i in range(4)} == {0, 1}


@pytest.mark.parametrize("kind,m,n", SYNTH, ids=[f"{k}-{m}x{n}" for k, m, n in SYNTH])
def test_reference_meets_its_own_bound(oracle, kind, m, n):
    rp, ci, a, x = _inputs(kind, m, n)
    absrow = oracle.csr_spmv(rp, ci, np.abs(a), np.abs(x))
    empty = np.diff(rp) == 0
    assert np.all(absrow[empty] == 0)
    for i, dtype in enumerate((np.float64, np.float32)):
        _, g0, g1, _ = device_layout(SYNTH.index((kind, m, n)) * 3 + 4 * i)
        y0 = (np.random.default_rng(1000 + i).uniform(-1, 1, m) * 8).astype(dtype)
        y_seq = oracle.csr_spmv(rp, ci, a, x, dtype)
        y_par = oracle.csr_spmv(rp, ci, a, x, dtype, num_threads=4)
        y_cut = oracle.merge_spmv(rp, ci, a, x, 61, dtype)
        what = f"{kind} {np.dtype(dtype).name}"
        plus = _buffer(y0 + y_seq, g0, g1, dtype)                   # y0 + s, rounded once in the handle's precision
        compare_device_result(plus, y0, y_seq, absrow, g0, m, dtype, True, what + " sequential, bit for bit")
        compare_device_result(plus, y0, y_par, absrow, g0, m, dtype, False, what + " against 4 threads")
        compare_device_result(plus, y0, y_cut, absrow, g0, m, dtype, False, what + " against the merge path")
        cut = _buffer((y0.astype(np.float64) + y_cut.astype(np.float64)).astype(dtype), g0, g1, dtype)
        compare_device_result(cut, y0, y_seq, absrow, g0, m, dtype, False, what + " merge path against sequential")
        assert np.array_equal(plus[g0:g0 + m][empty], y0[empty]) and np.array_equal(cut[g0:g0 + m][empty], y0[empty])
        # beta = 0 and y0 = 0 through the same function
        compare_device_result(_buffer(y_seq, g0, g1, dtype), None, y_par, absrow, g0, m, dtype, True, what + " beta 0")
        compare_device_result(_buffer(y_cut, g0, g1, dtype), np.zeros(m, dtype), y_seq, absrow, g0, m, dtype, False, what + " y0 = 0")


@pytest.mark.parametrize("exact", [False, True], ids=["bound", "exact"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_comparison_rejects_corrupted_results(oracle, dtype, exact):
    kind, m, n = SYNTH[1]                                            # `short`: a fifth of the rows are empty
    rp, ci, a, x = _inputs(kind, m, n)
    absrow = oracle.csr_spmv(rp, ci, np.abs(a), np.abs(x))
    y_ref = oracle.csr_spmv(rp, ci, a, x, dtype)
    y0 = (np.random.default_rng(7).uniform(-1, 1, m) * 8).astype(dtype)
    g0, g1 = 3, 2
    good = _buffer(y0 + y_ref, g0, g1, dtype)
    compare_device_result(good, y0, y_ref, absrow, g0, m, dtype, exact, "correct")
    lens = np.diff(rp)
    full = int(np.nonzero((lens > 0) & (np.abs(y0) > 1))[0][17])
    empty = int(np.nonzero(lens == 0)[0][5])

    def rejected(buf, row, what):
        with pytest.raises(AssertionError, match=rf"row \[?{row}\b") as e:
            compare_device_result(buf, y0, y_ref, absrow, g0, m, dtype, exact, what)
        assert what in str(e.value)

    twice = good.copy()
    twice[g0 + full] += y0[full]
    rejected(twice, full, "y0 added twice")
    dropped = good.copy()
    dropped[g0 + full] = y_ref[full]
    rejected(dropped, full, "y0 dropped")
    ulp = good.copy()
    ulp[g0 + empty] = np.nextafter(ulp[g0 + empty], dtype(np.inf))
    rejected(ulp, empty, "empty row off by one ulp")
    cleared = good.copy()
    cleared[g0 + empty] = 0                                          # the beta = 0 clear run under beta = 1
    rejected(cleared, empty, "empty row cleared")
    for pos, row in ((g0 + m, m), (g0 + m + g1 - 1, m + g1 - 1), (0, -g0), (g0 - 1, -1)):
        guard = good.copy()
        guard[pos] = np.nextafter(guard[pos], dtype(0))
        with pytest.raises(AssertionError, match=rf"guard .* at row {row} ") as e:
            compare_device_result(guard, y0, y_ref, absrow, g0, m, dtype, exact, "guard changed")
        assert "guard changed" in str(e.value)
    # the same guards under beta = 0
    guard = _buffer(y_ref, g0, g1, dtype)
    compare_device_result(guard, None, y_ref, absrow, g0, m, dtype, exact, "beta 0")
    guard[g0 + m] = 0
    with pytest.raises(AssertionError, match=rf"guard behind y overwritten at row {m} "):
        compare_device_result(guard, None, y_ref, absrow, g0, m, dtype, exact, "beta 0")
