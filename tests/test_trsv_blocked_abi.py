"""CPU tier of the blocked triangular solve (include/spmv_mi355x.h "THE BLOCKED FORM"): the symbols are exported and bound, every
argument error comes back as rc 1 in trsv_create's order and wording with block_rows in the place of chain_rows (scalars, NULL pointers,
the pattern, the stored diagonal; the device last), and spmv_mi355x_trsv_analyze_blocked gives exactly what a numpy restatement of the
blocked rule gives (trsv_blocked_cases.analysis_of): the level of every row within its block, blocks = ceil(n / B), nnz_dropped,
max_block_levels and max_level_rows."""
import ctypes

import numpy as np
import pytest

import trsv_blocked_cases as bc
import trsv_cases as tc
from conftest import has_gpu
from trsv_cases import LOWER, UPPER

F64, F32, STORED, UNIT = 0, 1, 0, 1
P = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def test_the_symbols_are_exported_and_bound():
    import spmv_mi355x as E
    for name in ("spmv_mi355x_trsv_analyze_blocked", "spmv_mi355x_trsv_create_blocked", "spmv_mi355x_trsv_block_info"):
        assert hasattr(E.lib(), name) and name in E.SYMBOLS, name
    assert callable(E.trsv_analyze_blocked) and hasattr(E.TriangularSolve, "block_info")


def test_chain_rows_and_block_rows_exclude_each_other():
    import spmv_mi355x as E
    rp, ci, va = good()
    with pytest.raises(ValueError, match="chain_rows"):
        E.TriangularSolve(rp, ci, va, 3, chain_rows=64, block_rows=0)
    with pytest.raises(ValueError, match="chain_rows"):
        E.TriangularSolve(rp, ci, va, 3, chain_rows=64, block_rows=2)


# ---- errors, in their order ---------------------------------------------------------------------------------------------------------

def good():
    """a valid 3 x 3 matrix with both triangles and a stored diagonal"""
    rp = np.array([0, 2, 5, 7], np.int32)
    ci = np.array([0, 1, 0, 1, 2, 1, 2], np.int32)
    va = np.array([2.0, 0.5, 0.25, -1.5, 0.125, 0.5, 1.0])
    return rp, ci, va


def create(uplo=LOWER, diag=STORED, precision=F64, n=3, rp="good", ci="good", va="good", block_rows=0, out="good"):
    import spmv_mi355x as E
    g = good()
    rp, ci, va = (g[k] if isinstance(a, str) else a for k, a in enumerate((rp, ci, va)))
    h = ctypes.c_void_p()
    rc = E.lib().spmv_mi355x_trsv_create_blocked(ctypes.byref(h) if out is not None else None, uplo, diag, precision, ctypes.c_long(n),
                                                 P(rp), P(ci), P(va), ctypes.c_long(block_rows), -1)
    msg = E.lib().spmv_mi355x_last_error().decode()
    if rc == 0:
        E.lib().spmv_mi355x_trsv_destroy(h)
    return rc, msg


BAD_RP, BAD_CI = np.array([0, 2, 1, 7], np.int32), np.array([0, 1, 0, 3, 2, 1, 2], np.int32)
ZERO_DIAG = np.array([2.0, 0.5, 0.25, 0.0, 0.125, 0.5, 1.0])
NO_DIAG = (np.array([0, 2, 3, 5], np.int32), np.array([0, 1, 0, 1, 2], np.int32), np.array([2.0, 0.5, 0.25, 0.5, 1.0]))
# (step, case, arguments, phrase): test_trsv_abi.py's table with block_rows for chain_rows. `behind` adds an error of a LATER step to the
# call where the case leaves room for one: the earlier error must be the one reported. The device lies behind every case.
ERRORS = [
    (1, "uplo", dict(uplo=2), "uplo must be SPMV_MI355X_LOWER (0) or SPMV_MI355X_UPPER (1) (got 2)"),
    (1, "uplo_negative", dict(uplo=-1), "uplo must be"),
    (1, "diag", dict(diag=2), "diag must be SPMV_MI355X_DIAG_STORED (0) or SPMV_MI355X_DIAG_UNIT (1) (got 2)"),
    (1, "precision", dict(precision=2), "unknown precision 2"),
    (1, "n_negative", dict(n=-1), "n = -1 out of range"),
    (1, "block_rows_negative", dict(block_rows=-1), "block_rows must be 0 (the default) or 1 .. 16384 (got -1)"),
    (1, "block_rows_large", dict(block_rows=16385), "block_rows must be 0 (the default) or 1 .. 16384 (got 16385)"),
    (2, "null_out", dict(out=None), "NULL argument ( out"),
    (2, "null_row_ptr", dict(rp=None), "NULL argument ( row_ptr"),
    (2, "null_col_idx", dict(ci=None), "NULL argument ( col_idx"),
    (2, "null_values", dict(va=None), "NULL argument ( values"),
    (3, "row_ptr_not_from_0", dict(rp=np.array([1, 2, 5, 7], np.int32)), "row_ptr must start at 0"),
    (3, "row_ptr_not_monotone", dict(rp=BAD_RP), "row_ptr is not monotone at row 1"),
    (3, "column_out_of_range", dict(ci=BAD_CI), "column index 3 out of range [0,3) at entry 3"),
    (3, "column_negative", dict(ci=np.array([0, 1, 0, 1, 2, -1, 2], np.int32)), "column index -1 out of range [0,3) at entry 5"),
    (4, "diagonal_missing", dict(rp=NO_DIAG[0], ci=NO_DIAG[1], va=NO_DIAG[2]), "row 1 has no diagonal entry"),
    (4, "diagonal_zero", dict(va=ZERO_DIAG), "the diagonal of row 1 is 0"),
    (4, "diagonal_nan", dict(va=np.array([2.0, 0.5, 0.25, 1.0, 0.125, 0.5, np.nan])), "the diagonal of row 2 is nan"),
    (4, "diagonal_inf", dict(va=np.array([np.inf, 0.5, 0.25, 1.0, 0.125, 0.5, 1.0])), "the diagonal of row 0 is inf"),
    (4, "diagonal_twice", dict(ci=np.array([0, 1, 0, 1, 1, 1, 2], np.int32)), "row 1 stores 2 entries with column 1"),
    (4, "first_bad_row_is_named", dict(va=np.array([2.0, 0.5, 0.25, 0.0, 0.125, 0.5, 0.0])), "the diagonal of row 1 is 0"),
]
BEHIND = {1: (dict(out=None), dict(rp=BAD_RP), dict(va=ZERO_DIAG)), 2: (dict(rp=BAD_RP), dict(ci=BAD_CI), dict(va=ZERO_DIAG)),
          3: (dict(va=ZERO_DIAG),), 4: ()}


@pytest.mark.parametrize("step,case,args,phrase", ERRORS, ids=[e[1] for e in ERRORS])
def test_create_errors_in_their_documented_order(step, case, args, phrase):
    rc, msg = create(**args)
    assert rc == 1
    assert msg.startswith("trsv_create_blocked: ") and phrase in msg, msg
    for behind in BEHIND[step]:
        if not set(behind) & set(args):
            rc, msg = create(**args, **behind)
            assert rc == 1 and msg.startswith("trsv_create_blocked: ") and phrase in msg, (behind, msg)


def test_the_diagonal_is_checked_whatever_the_block_size():
    """the diagonal is never dropped: a zero on it is refused at B = 1 too, and a diagonal that vanishes only in fp32 only there"""
    for B in (1, 2, 16384):
        rc, msg = create(va=ZERO_DIAG, block_rows=B)
        assert rc == 1 and "the diagonal of row 1 is 0" in msg, msg
    tiny = np.array([2.0, 0.5, 0.25, 1e-60, 0.125, 0.5, 1.0])
    rc, msg = create(precision=F32, va=tiny, block_rows=2)
    assert rc == 1 and msg.startswith("trsv_create_blocked: ") and "the diagonal of row 1 is 0" in msg, msg
    if not has_gpu():
        rc, msg = create(precision=F64, va=tiny, block_rows=2)
        assert rc == 1 and "no HIP device available" in msg, msg


@pytest.mark.parametrize("precision", (F64, F32))
@pytest.mark.parametrize("diag", (STORED, UNIT))
@pytest.mark.parametrize("uplo", (LOWER, UPPER))
def test_the_device_comes_last(uplo, diag, precision):
    """a valid matrix, at both ends of block_rows and at the default: without a GPU the library's no-device message, named as
    trsv_create_blocked's; with one a handle"""
    for args in (dict(), dict(block_rows=1), dict(block_rows=16384), dict(n=0, rp=np.zeros(1, np.int32), ci=None, va=None)):
        rc, msg = create(uplo=uplo, diag=diag, precision=precision, **args)
        if has_gpu():
            assert rc == 0, msg
        else:
            assert rc == 1
            assert msg.startswith("trsv_create_blocked: no HIP device available: this engine has no CPU fallback"), msg


def test_block_info_refuses_a_null_handle():
    import spmv_mi355x as E
    rows = ctypes.c_long(-3)
    assert E.lib().spmv_mi355x_trsv_block_info(None, ctypes.byref(rows), None, None, None) == 1
    assert b"trsv" in E.lib().spmv_mi355x_last_error() and rows.value == -3


ANALYZE_ERRORS = [
    ("uplo", dict(uplo=3), "uplo must be"),
    ("n_negative", dict(n=-2), "out of range"),
    ("block_rows", dict(block_rows=16385), "block_rows must be 0 (the default) or 1 .. 16384 (got 16385)"),
    ("block_rows_negative", dict(block_rows=-4), "block_rows must be 0 (the default) or 1 .. 16384 (got -4)"),
    ("null_row_ptr", dict(rp=None), "NULL argument ( row_ptr"),
    ("null_col_idx", dict(ci=None), "NULL argument ( col_idx"),
    ("row_ptr_not_from_0", dict(rp=np.array([2, 2, 5, 7], np.int32)), "row_ptr must start at 0"),
    ("row_ptr_not_monotone", dict(rp=BAD_RP), "row_ptr is not monotone at row 1"),
    ("column_out_of_range", dict(ci=BAD_CI), "column index 3 out of range [0,3) at entry 3"),
]


@pytest.mark.parametrize("case,args,phrase", ANALYZE_ERRORS, ids=[e[0] for e in ANALYZE_ERRORS])
def test_analyze_errors(case, args, phrase):
    import spmv_mi355x as E
    a = dict(uplo=LOWER, n=3, rp=good()[0], ci=good()[1], block_rows=0)
    a.update(args)
    lv = ctypes.POINTER(ctypes.c_int32)()
    blocks = ctypes.c_long(-9)
    rc = E.lib().spmv_mi355x_trsv_analyze_blocked(a["uplo"], ctypes.c_long(a["n"]), P(a["rp"]), P(a["ci"]), ctypes.c_long(a["block_rows"]),
                                                  ctypes.byref(lv), ctypes.byref(blocks), None, None, None, None)
    msg = E.lib().spmv_mi355x_last_error().decode()
    assert rc == 1 and msg.startswith("trsv_analyze_blocked: ") and phrase in msg, msg
    assert not lv and blocks.value == -9


# ---- the analysis against the restated rule -----------------------------------------------------------------------------------------

ANALYSIS = [("empty", 64), ("one", 64), ("one", 1), ("diagonal", 64), ("diagonal", 0), ("bidiagonal", 64), ("bidiagonal", 1), ("dag", 100),
            ("dag", 1024), ("dag", 16384), ("prescribed", 16384), ("padding", 64), ("padding", 1024), ("stencil", 576), ("stencil", 1000)]
KEYS = ("blocks", "max_block_levels", "max_level_rows", "nnz_dropped")


@pytest.mark.parametrize("uplo", (LOWER, UPPER), ids=("lower", "upper"))
@pytest.mark.parametrize("name,B", ANALYSIS, ids=[f"{a}-{c}" for a, c in ANALYSIS])
def test_analyze_matches_the_restated_rule(name, B, uplo):
    import spmv_mi355x as E
    rp, ci, va, n = tc.matrix(name, uplo)
    got = E.trsv_analyze_blocked(rp, ci, n, "lower" if uplo == LOWER else "upper", B)
    assert got["block_rows"] == (B if B else got["block_rows"]) and 1 <= got["block_rows"] <= 16384
    want = bc.analysis_of(rp, ci, n, uplo, got["block_rows"])
    assert got["level_of_row"].dtype == np.int32 and np.array_equal(got["level_of_row"], want["level_of_row"])
    assert {k: got[k] for k in KEYS} == {k: want[k] for k in KEYS}


def test_the_named_shapes_are_what_their_names_say():
    """the restated rule itself, on the cases whose answer is known in closed form"""
    import spmv_mi355x as E
    for uplo in (LOWER, UPPER):
        side = "lower" if uplo == LOWER else "upper"
        a = E.trsv_analyze_blocked(*tc.matrix("empty", uplo)[:2], 0, side, 64)
        assert [a[k] for k in KEYS] == [0, 0, 0, 0] and len(a["level_of_row"]) == 0
        # 4097 rows in blocks of 64: 65 blocks, the last of one row; the 64 entries that enter a block's first row are dropped
        rp, ci, va, n = tc.matrix("bidiagonal", uplo)
        a = E.trsv_analyze_blocked(rp, ci, n, side, 64)
        assert [a[k] for k in KEYS] == [65, 64, 1, 64]
        # LOWER: row i depends on i - 1, level i % 64. UPPER (mirrored): row i depends on i + 1; the level counts from the block's
        # last row, which is 63 + 64 b, or 4096 in the last block of one row
        i = np.arange(n)
        want = i % 64 if uplo == LOWER else np.minimum(i // 64 * 64 + 63, n - 1) - i
        assert np.array_equal(a["level_of_row"], want)
        a = E.trsv_analyze_blocked(rp, ci, n, side, 1)
        assert [a[k] for k in KEYS] == [4097, 1, 1, 4096] and not a["level_of_row"].any()          # everything dropped
        # one block: nothing dropped, the levels of the global analysis
        rp, ci, va, n = tc.matrix("prescribed", uplo)
        a = E.trsv_analyze_blocked(rp, ci, n, side, 16384)
        assert [a[k] for k in KEYS] == [1, 12, 3000, 0]
        assert np.array_equal(a["level_of_row"], E.trsv_analyze(rp, ci, n, side)["level_of_row"])
        # the 24^3 stencil in blocks of one grid plane: exactly the couplings between planes are dropped, 24^2 for each of the 23
        # pairs of neighbouring planes; within a plane the hyperplanes i + j of a 24^2 grid
        rp, ci, va, n = tc.matrix("stencil", uplo)
        a = E.trsv_analyze_blocked(rp, ci, n, side, 576)
        assert [a[k] for k in KEYS] == [24, 2 * 23 + 1, 24, 23 * 576]
        rows = np.repeat(np.arange(n), np.diff(rp))
        off = ci != rows
        assert a["nnz_dropped"] == int(np.sum(off & (np.abs(ci - rows) == 576)))


def test_a_full_matrix_is_analyzed_as_its_kept_triangle():
    import spmv_mi355x as E
    full = tc.stencil_full()
    for uplo, side in ((LOWER, "lower"), (UPPER, "upper")):
        a = E.trsv_analyze_blocked(full[0], full[1], full[3], side, 1000)
        t = tc.triangle(*full, uplo)
        want = bc.analysis_of(t[0], t[1], t[3], uplo, 1000)
        assert np.array_equal(a["level_of_row"], want["level_of_row"])
        assert {k: a[k] for k in KEYS} == {k: want[k] for k in KEYS}
        assert a["nnz_dropped"] == bc.dropped_of(full[0], full[1], full[3], uplo, 1000)          # the other triangle is not counted


def test_the_filtered_reference_solves_the_block_diagonal_system():
    """the yardstick of the GPU tier: the C reference on the filtered CSR against a dense numpy solve of the block-diagonal part"""
    rp, ci, va, n = tc.matrix("dag", LOWER)
    B = 100
    f = bc.filtered(rp, ci, va, n, B)
    D = np.zeros((n, n))
    np.add.at(D, (np.repeat(np.arange(n), np.diff(f[0])), f[1]), f[2])
    blk = np.arange(n) // B
    assert not D[blk[:, None] != blk[None, :]].any() and len(f[1]) == len(ci) - bc.dropped_of(rp, ci, n, LOWER, B)
    b = np.random.default_rng(5).uniform(-1, 1, n)
    x = tc.reference(*f, LOWER, False, b, np.float64)
    # test_trsv_abi.py's bound: fewer than 500 roundings of a quantity of modulus <= 1
    assert np.all(np.isfinite(x)) and np.abs(D @ x - b).max() <= 500 * 2.0 ** -53
    assert not np.array_equal(x, tc.reference(rp, ci, va, n, LOWER, False, b, np.float64))
