"""SpGEMM without a GPU (include/spmv_mi355x.h "SpGEMM"): the sequential reference of tests/spgemm_reference.c against scipy, every
refusal of spgemm_create that comes before the device is touched, and the struct_size handling of spmv_mi355x_spgemm_stats.

1. The reference's pattern is the pattern of scipy multiplying the two patterns with all-ones data (positive data cannot cancel, so
   that is the structural product whatever scipy does with zeros), and its values lie within 2 L u (|A| |B|)(i, j) of scipy's, L the
   products of the entry and u = 2^-53: both sums carry the standard L u bound.
2. The refusals, in the header's order, each with the prefix spgemm_create and nothing written to *out.
3. sizeof(spmv_mi355x_spgemm_stats) and its field offsets against the C compiler's; a struct_size below 8 is refused."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import spgemm_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def eng():
    import spmv_mi355x as eng
    return eng


# ---- 1. the reference ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sc.SMALL_CASES)
def test_the_reference_against_scipy(name):
    A, B = sc.case(name)
    c_rp, c_ci, c_va = sc.reference_of(name)
    s_rp, s_ci, _ = sc.scipy_pattern(A, B)
    assert np.array_equal(c_rp, s_rp) and np.array_equal(c_ci, s_ci), name
    assert c_rp[0] == 0 and all(np.all(np.diff(c_ci[c_rp[i]:c_rp[i + 1]]) > 0) for i in range(A[3]))
    share = sc.shares_of_the_bound(A, B, c_rp, c_ci, c_va)
    print(f"[spgemm] {name}: nnz(C) = {len(c_ci)}, the reference is within {share.max() if len(share) else 0:.3g} of its bound of scipy")
    assert np.all(share <= 1)


def test_the_cases_are_what_they_claim():
    A, B = sc.case("rect")
    rows = [A[1][A[0][i]:A[0][i + 1]] for i in range(A[3])]
    assert any(len(r) == 0 for r in rows) and any(len(set(r)) < len(r) for r in rows) and any(np.any(np.diff(r) < 0) for r in rows)
    b_len = np.diff(B[0])
    assert np.any(b_len == 0) and np.any(b_len[A[1]] == 0) and max(len(r) for r in rows) <= 13 and b_len.max() <= 12
    assert all(len(set(B[1][B[0][i]:B[0][i + 1]])) == b_len[i] for i in range(B[3]))
    # bins: both binnings see the first and the last width of every bin, and rows whose two bins differ
    A, B = sc.case("bins")
    c_rp, _, _ = sc.reference_of("bins")
    products = np.array([np.diff(B[0])[A[1][A[0][i]:A[0][i + 1]]].sum() for i in range(A[3])])
    for widths in (np.minimum(products, B[4]), np.diff(c_rp)):
        for w in [1] + [s + d for s in sc.BIN_WMAX for d in (0, 1)]:
            assert w in widths, w
    assert any(sc.bin_of(p) != sc.bin_of(w) for p, w in zip(products, np.diff(c_rp)))
    # global_table, dense_row, collide, cancel
    A, B = sc.case("global_table")
    assert np.diff(A[0])[0] == 300 and np.diff(B[0]).min() == 40 and B[4] == 20000
    c_rp, _, _ = sc.reference_of("dense_row")
    assert c_rp[1] == 3000 and sc.case("dense_row")[1][4] == 3000
    A, B = sc.case("collide")
    assert np.all(sc.hash_of(B[1], 4096) == 0) and len(B[1]) == sc.COLLIDE_WIDTH and sc.bin_of(len(B[1])) == sc.BINS - 2
    c_rp, c_ci, c_va = sc.reference_of("cancel")
    assert len(c_va) == 10 and np.all(c_va == 0) and not np.any(np.signbit(c_va))
    assert sc.case("wrap")[0][3] == 32 * 2048 + 37


def test_a_column_twice_in_a_row_of_a_is_two_steps():
    A = (np.array([0, 3], np.int32), np.array([1, 0, 1], np.int32), np.array([0.1, 0.7, 0.2]), 1, 2)
    B = (np.array([0, 1, 2], np.int32), np.array([0, 0], np.int32), np.array([0.3, 0.9]), 2, 1)
    _, c_ci, c_va = sc.reference(A, B)
    libm = ctypes.CDLL("libm.so.6")
    libm.fma.restype = ctypes.c_double
    libm.fma.argtypes = [ctypes.c_double] * 3
    assert c_ci.tolist() == [0] and c_va[0] == libm.fma(0.2, 0.9, libm.fma(0.7, 0.3, libm.fma(0.1, 0.9, 0.0)))


# ---- 2. the refusals ---------------------------------------------------------------------------------------------------------------------

def _create(eng, m, k, n, a_rp, a_ci, b_rp, b_ci, out=True):
    h = ctypes.c_void_p(0x5a5a)
    p = lambda a: None if a is None else np.ascontiguousarray(a, np.int32).ctypes.data_as(ctypes.c_void_p)
    keep = [None if a is None else np.ascontiguousarray(a, np.int32) for a in (a_rp, a_ci, b_rp, b_ci)]
    rc = eng.lib().spmv_mi355x_spgemm_create(ctypes.byref(h) if out else None, ctypes.c_int(-1), ctypes.c_long(m), ctypes.c_long(k),
                                             ctypes.c_long(n), *[p(a) for a in keep])
    msg = eng.lib().spmv_mi355x_last_error().decode()
    assert rc == 1 and msg.startswith("spgemm_create: "), (rc, msg)
    assert not out or not h.value, "*out must be NULL after a refusal"
    return msg


GOOD = dict(m=2, k=3, n=4, a_rp=[0, 2, 3], a_ci=[0, 2, 1], b_rp=[0, 1, 3, 4], b_ci=[3, 0, 2, 1])


def _with(**changes):
    return dict(GOOD, **changes)


def test_refusals_before_any_device(eng):
    big = 2 ** 31 - 1
    for dim in "mkn":
        for v in (-1, big, big + 5):
            assert f"{dim} = {v} out of range" in _create(eng, **_with(**{dim: v}))
    # the sizes come before the pointers
    assert "m = -1" in _create(eng, **_with(m=-1, a_rp=None))
    assert " out" in _create(eng, **GOOD, out=False)
    assert " a_row_ptr" in _create(eng, **_with(a_rp=None))
    assert " b_row_ptr" in _create(eng, **_with(b_rp=None))
    assert "a_col_idx" in _create(eng, **_with(a_ci=None))
    assert "b_col_idx" in _create(eng, **_with(b_ci=None))
    assert "a_row_ptr must start at 0" in _create(eng, **_with(a_rp=[1, 2, 3]))
    assert "a_row_ptr is not monotone at row 1" in _create(eng, **_with(a_rp=[0, 3, 2]))
    assert "b_row_ptr is not monotone at row 0" in _create(eng, **_with(b_rp=[0, -1, 3, 4]))
    msg = _create(eng, **_with(a_ci=[0, 3, 1]))
    assert "column index 3 of a out of range [0,3)" in msg
    assert "column index -1 of a" in _create(eng, **_with(a_ci=[0, -1, 1]))
    assert "column index 4 of b out of range [0,4) at entry 2" in _create(eng, **_with(b_ci=[3, 0, 4, 1]))
    # A is checked before B, the patterns before B's duplicates
    assert " of a " in _create(eng, **_with(a_ci=[0, 3, 1], b_ci=[3, 2, 2, 1]))
    msg = _create(eng, **_with(b_ci=[3, 2, 2, 1]))
    assert "row 1 of B stores column 2 twice" in msg
    # a column twice in a row of A is legal: with good arrays the only thing left to refuse is the device
    import torch
    if not torch.cuda.is_available():
        assert "no HIP device" in _create(eng, **_with(a_rp=[0, 3, 3], a_ci=[1, 2, 1]))


def test_the_other_entry_points_refuse_null(eng):
    L = eng.lib()
    st = eng.SpgemmStats()
    st.struct_size = ctypes.sizeof(eng.SpgemmStats)
    for call, prefix in ((lambda: L.spmv_mi355x_spgemm_pattern(None, None, None), "spgemm_pattern: NULL"),
                         (lambda: L.spmv_mi355x_spgemm_multiply(None, None, None, None), "spgemm_multiply: NULL"),
                         (lambda: L.spmv_mi355x_spgemm_multiply_device_async(None, None, None, None, None), "spgemm_multiply: NULL"),
                         (lambda: L.spmv_mi355x_spgemm_info(None, ctypes.byref(st)), "spgemm_info: NULL")):
        assert call() == 1 and L.spmv_mi355x_last_error().decode().startswith(prefix)
    assert L.spmv_mi355x_spgemm_destroy(None) == 0


# ---- 3. the info struct --------------------------------------------------------------------------------------------------------------------

def test_stats_layout_matches_the_header(eng, tmp_path):
    lines = ['printf("sizeof %zu\\n", sizeof(spmv_mi355x_spgemm_stats));', 'printf("bins %d\\n", SPMV_MI355X_SPGEMM_BINS);']
    for fname, _ in eng.SpgemmStats._fields_:
        lines.append(f'printf("{fname} %zu\\n", offsetof(spmv_mi355x_spgemm_stats, {fname}));')
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "spmv_mi355x.h"\nint main(void) {\n' + "\n".join(lines) + "\nreturn 0; }\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(l.split() for l in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    assert int(got["sizeof"]) == ctypes.sizeof(eng.SpgemmStats) and int(got["bins"]) == sc.BINS == len(eng.SpgemmStats().symbolic_bin_rows)
    for fname, _ in eng.SpgemmStats._fields_:
        assert int(got[fname]) == getattr(eng.SpgemmStats, fname).offset, fname
