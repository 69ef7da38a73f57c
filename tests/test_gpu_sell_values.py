"""7-byte fp64 values of the SELL delta layout (opts.sell_values; csrc/launch.hpp, kernels_sell.hip: SellVals): every index mode at
every slice width with and without the index-free modes, one to four waves per slice, host and GPU builder -> the same stored bytes,
the same plain layout as 8-byte values, bit-identical y; slices whose values do not qualify keep 8 bytes; the handle from a CSR
streamed in pieces equals the whole one; auto leaves small matrices alone and compresses large ones."""
import os

import numpy as np
import pytest

import oracle
import spmv_host as H

pytestmark = pytest.mark.gpu

V7_FLAG = 8


@pytest.fixture(scope="module")
def eng():
    import spmv_mi355x as eng
    assert eng.device_count() >= 1, "no GPU visible: the -m gpu tests need an MI355X"
    return eng


@pytest.fixture
def modes_off():
    """Sets SPMV_MI355X_SELL_MODES_OFF for the handles created inside (read at every create())."""
    old = os.environ.get("SPMV_MI355X_SELL_MODES_OFF")

    def set_(v):
        os.environ["SPMV_MI355X_SELL_MODES_OFF"] = str(v)
    yield set_
    if old is None:
        os.environ.pop("SPMV_MI355X_SELL_MODES_OFF", None)
    else:
        os.environ["SPMV_MI355X_SELL_MODES_OFF"] = old


def _kkt_like_values(rng, m, w):
    """Values as the nlpkkt twin's: off-diagonals in [0.25, 1) with both signs, a 4.0 on some steps (exponents 1021 .. 1025)."""
    a = rng.uniform(0.25, 1.0, (m, w)) * rng.choice([-1.0, 1.0], (m, w))
    a[rng.uniform(size=(m, w)) < 0.1] = 4.0
    return a


def _six_slices(rng, w, n):
    """384 rows of w entries each: one slice per index mode (affine, lane offsets, lane offsets with exceptions, 8-bit, 16-bit and
    32-bit deltas) when every index-free mode is allowed."""
    cols = []
    first = np.arange(64) + 7
    cols.append(first[:, None] + np.sort(rng.choice(4000, w, replace=False))[None, :])                      # affine
    first = rng.permutation(64) * 3 + 20011
    steps = np.sort(rng.choice(4000, w, replace=False)) * 200
    cols.append(first[:, None] + steps[None, :])                                                            # lane offsets
    c = first[:, None] + steps[None, :] + 900000
    if w > 1:
        c[5, 1:] += np.arange(1, w) % 3 + 1                                                                 # one row out of line
    cols.append(c)
    for span in (250, 60000, n - 10):                                                                       # 8 / 16 / 32-bit deltas
        base = rng.integers(0, n - span - 1)
        cols.append(np.sort(np.stack([rng.choice(span, w, replace=False) for _ in range(64)]), axis=1) + base)
    cols = np.sort(np.concatenate(cols), axis=1)
    m = cols.shape[0]
    rp = (np.arange(m + 1) * w).astype(np.int32)
    return rp, cols.reshape(-1).astype(np.int32), m


def _v7_flags(M):
    desc = M.stored_array("desc", np.int64)
    return desc[1:-2:2] & V7_FLAG                        # desc[2s + 1] of every slice (the last pair is the terminator)


def test_every_mode_width_split_and_builder(eng, modes_off):
    rng = np.random.default_rng(31)
    n = 2_000_000
    x = rng.uniform(-1, 1, n)
    for w in range(1, 20):
        rp, ci, m = _six_slices(rng, w, n)
        a = _kkt_like_values(rng, m, w).reshape(-1)
        y_seq = oracle.csr_spmv(rp, ci, a, x, np.float64, num_threads=1)
        for off in range(8):
            modes_off(off)
            for split in (1, 2, 4):
                common = dict(sell_c=64, sell_delta=1, sell_sigma=64, sell_split=split, sell_window=2)
                P = eng.Matrix(rp, ci, a, m, n, "sell_c_sigma", np.float64, sell_values=2, convert_on=1, **common)
                y_plain, l_plain = P.spmv(x), P.sell_layout()
                hv = {}
                for conv in (1, 2):
                    V = eng.Matrix(rp, ci, a, m, n, "sell_c_sigma", np.float64, sell_values=1, convert_on=conv, **common)
                    what = f"w={w} modes_off={off} split={split} convert_on={conv}"
                    if w >= 4:                                    # every slice has a full group: all six compress
                        assert V.format_name == P.format_name + "_v7", (what, V.format_name)
                        assert np.all(_v7_flags(V)), what
                        assert V.mem_footprint < P.mem_footprint, what
                    else:                                         # no full group of 4 steps: nothing to compress, the plain bytes
                        assert V.format_name == P.format_name and V.mem_footprint == P.mem_footprint, what
                    lv = V.sell_layout()
                    for k in ("slice_ptr", "col", "val", "row_of_sorted"):
                        np.testing.assert_array_equal(lv[k], l_plain[k], err_msg=f"{what} {k}")
                    assert lv["nnz_ext"] == l_plain["nnz_ext"]
                    y = V.spmv(x)
                    np.testing.assert_array_equal(y, y_plain, err_msg=what)
                    if split == 1:
                        np.testing.assert_array_equal(y, y_seq, err_msg=what)
                    hv[conv] = {k: V.stored_array(k) for k in ("val", "idx", "desc", "row_of_sorted")}
                    V.close()
                for k in hv[1]:
                    np.testing.assert_array_equal(hv[1][k], hv[2][k], err_msg=f"w={w} modes_off={off} split={split} host != GPU builder: {k}")
                P.close()


def test_fallback_only_where_it_must(eng):
    """Slices with a value 2^20 times its neighbours, an Inf or a NaN in a full group keep 8-byte values; a denormal, a -0.0 or an
    outlier in the tail group (stored as 8-byte pairs anyway) do not stop a slice; y is the same either way."""
    rng = np.random.default_rng(5)
    m, w, n = 64 * 8, 9, 5000                          # 9 steps: two full groups + a one-step tail
    rp = (np.arange(m + 1) * w).astype(np.int32)
    ci = np.sort(np.stack([rng.choice(n, w, replace=False) for _ in range(m)]), axis=1).reshape(-1).astype(np.int32)
    a = _kkt_like_values(rng, m, w)
    want = np.ones(8, bool)
    a[0 * 64 + 3, 2] *= 2.0 ** 20; want[0] = False     # 21 binades apart
    a[1 * 64 + 7, 5] = 5e-310                          # denormal: exponent code 0
    a[2 * 64 + 9, 0] = -0.0
    a[3 * 64 + 1, 6] = np.inf; want[3] = False
    a[4 * 64 + 60, 1] = np.nan; want[4] = False
    a[5 * 64 + 2, 8] = 2.0 ** 40                       # tail step: not part of any compressed group
    a[6 * 64 + 0, 3] = 2.0 ** -1074                    # smallest denormal beside a 4.0: still one slice
    a = a.reshape(-1)
    x = rng.uniform(-1, 1, n)
    for conv in (1, 2):
        P = eng.Matrix(rp, ci, a, m, n, "sell_c_sigma", np.float64, sell_c=64, sell_delta=1, sell_sigma=64, sell_split=1, sell_window=2,
                       sell_values=2, convert_on=conv)
        V = eng.Matrix(rp, ci, a, m, n, "sell_c_sigma", np.float64, sell_c=64, sell_delta=1, sell_sigma=64, sell_split=1, sell_window=2,
                       sell_values=1, convert_on=conv)
        np.testing.assert_array_equal(_v7_flags(V) != 0, want)
        np.testing.assert_array_equal(V.sell_layout()["val"], P.sell_layout()["val"])
        np.testing.assert_array_equal(V.spmv(x), P.spmv(x))           # NaN rows compare equal to NaN rows
        words = 2 * 224 + 64                               # a compressed slice of two full groups + one tail step
        assert V.stored_array("val").size == 8 * (want.sum() * words + (~want).sum() * 64 * w)
        P.close()
        V.close()


def test_pieces_equal_whole(eng):
    """The handle converted from a CSR streamed into device memory in pieces (convert_sell.hip: sell_delta_convert_resident) holds the
    same bytes as the one converted from the whole CSR, with 7-byte values."""
    A = H.gen_kkt(12)
    rp, ci, va, m, n = A["row_ptr"], A["col_idx"], A["values"], A["m"], A["n"]
    x = np.random.default_rng(2).uniform(-1, 1, n)
    W = eng.Matrix(rp, ci, va, m, n, "sell_c_sigma", np.float64, sell_values=1, sell_window=2, convert_on=1)
    st = eng.CsrStream(m, n, int(rp[m]))
    for r0, r1 in ((0, m // 3), (m // 3, m // 3 + 1), (m // 3 + 1, m)):
        st.append(rp[r0:r1 + 1] - rp[r0], ci[rp[r0]:rp[r1]], va[rp[r0]:rp[r1]])
    S = st.finish("sell_c_sigma", np.float64, sell_values=1)
    assert S.format_name == W.format_name and "_v7" in W.format_name and S.mem_footprint == W.mem_footprint
    for k in ("val", "idx", "desc", "row_of_sorted"):
        np.testing.assert_array_equal(S.stored_array(k), W.stored_array(k), err_msg=k)
    np.testing.assert_array_equal(S.spmv(x), W.spmv(x))
    S.close()
    W.close()


def test_auto_small_untouched_large_compressed(eng):
    for N, large in ((20, False), (100, True)):
        A = H.gen_kkt(N)
        rp, ci, va, m, n = A["row_ptr"], A["col_idx"], A["values"], A["m"], A["n"]
        nnz = int(rp[m])
        x = np.random.default_rng(N).uniform(-1, 1, n)
        Auto = eng.Matrix(rp, ci, va, m, n, "sell_c_sigma", np.float64)
        Off = eng.Matrix(rp, ci, va, m, n, "sell_c_sigma", np.float64, sell_values=2)
        if not large:
            assert Auto.format_name == Off.format_name and Auto.mem_footprint == Off.mem_footprint
        else:
            assert nnz > 50_000_000
            assert Auto.format_name == Off.format_name + "_v7"
            # one byte saved per stored slot of the (almost all) qualifying slices: 8.5 -> 7.5 B per non-zero at this size
            assert Off.mem_footprint - Auto.mem_footprint >= 0.9 * nnz, (Off.mem_footprint / nnz, Auto.mem_footprint / nnz)
            assert Auto.mem_footprint / nnz <= 7.6, Auto.mem_footprint / nnz
        np.testing.assert_array_equal(Auto.spmv(x), Off.spmv(x))
        Auto.close()
        Off.close()
