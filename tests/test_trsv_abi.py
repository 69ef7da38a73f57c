"""CPU tier of the sparse triangular solve (include/spmv_mi355x.h "sparse triangular solve"): the symbols are exported and bound, every
argument error comes back as rc 1 with `trsv` in the message in the documented order (scalars, NULL pointers, the pattern, the stored
diagonal) before any device is touched, a valid matrix reaches the library's no-device message on a machine without a GPU, and
spmv_mi355x_trsv_analyze gives exactly the levels and the launch plan of a numpy restatement of the two rules (trsv_cases.py)."""
import ctypes

import numpy as np
import pytest

import trsv_cases as tc
from conftest import has_gpu
from trsv_cases import LOWER, UPPER

F64, F32, STORED, UNIT = 0, 1, 0, 1
P = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def test_the_symbols_are_exported_and_bound():
    import spmv_mi355x as E
    names = ["spmv_mi355x_trsv_analyze", "spmv_mi355x_trsv_create", "spmv_mi355x_trsv_destroy", "spmv_mi355x_trsv_solve_device_async",
             "spmv_mi355x_trsv_solve", "spmv_mi355x_trsv_info", "spmv_mi355x_trsv_mem_footprint", "spmv_mi355x_time_trsv_device"]
    for name in names:
        assert hasattr(E.lib(), name) and name in E.SYMBOLS, name
    assert callable(E.trsv_analyze)
    for attr in ("solve", "solve_device", "info", "time_device", "close"):            # mem_footprint is set per instance
        assert hasattr(E.TriangularSolve, attr), attr
    assert (E.LOWER, E.UPPER, E.DIAG_STORED, E.DIAG_UNIT) == (0, 1, 0, 1)


# ---- errors, in their order ---------------------------------------------------------------------------------------------------------

def good():
    """a valid 3 x 3 matrix with both triangles and a stored diagonal"""
    rp = np.array([0, 2, 5, 7], np.int32)
    ci = np.array([0, 1, 0, 1, 2, 1, 2], np.int32)
    va = np.array([2.0, 0.5, 0.25, -1.5, 0.125, 0.5, 1.0])
    return rp, ci, va


def create(uplo=LOWER, diag=STORED, precision=F64, n=3, rp="good", ci="good", va="good", chain_rows=0, out="good"):
    import spmv_mi355x as E
    g = good()
    rp, ci, va = (g[k] if isinstance(a, str) else a for k, a in enumerate((rp, ci, va)))
    h = ctypes.c_void_p()
    rc = E.lib().spmv_mi355x_trsv_create(ctypes.byref(h) if out is not None else None, uplo, diag, precision, ctypes.c_long(n), P(rp), P(ci),
                                         P(va), chain_rows, -1)
    msg = E.lib().spmv_mi355x_last_error().decode()
    if rc == 0:
        E.lib().spmv_mi355x_trsv_destroy(h)
    return rc, msg


BAD_RP, BAD_CI = np.array([0, 2, 1, 7], np.int32), np.array([0, 1, 0, 3, 2, 1, 2], np.int32)
ZERO_DIAG = np.array([2.0, 0.5, 0.25, 0.0, 0.125, 0.5, 1.0])
NO_DIAG = (np.array([0, 2, 3, 5], np.int32), np.array([0, 1, 0, 1, 2], np.int32), np.array([2.0, 0.5, 0.25, 0.5, 1.0]))
# (step, case, arguments, phrase). `behind` adds an error of a LATER step to the call where the case leaves room for one: the earlier
# error must be the one reported. The last step, the device, lies behind every case.
ERRORS = [
    (1, "uplo", dict(uplo=2), "uplo must be"),
    (1, "uplo_negative", dict(uplo=-1), "uplo must be"),
    (1, "diag", dict(diag=2), "diag must be"),
    (1, "precision", dict(precision=2), "unknown precision"),
    (1, "n_negative", dict(n=-1), "n = -1 out of range"),
    (1, "chain_rows_negative", dict(chain_rows=-1), "chain_rows must be"),
    (1, "chain_rows_large", dict(chain_rows=65537), "chain_rows must be"),
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
    assert "trsv" in msg and phrase in msg, msg
    for behind in BEHIND[step]:
        if not set(behind) & set(args):
            rc, msg = create(**args, **behind)
            assert rc == 1 and "trsv" in msg and phrase in msg, (behind, msg)


def test_scalars_come_before_null_pointers_and_the_pattern_before_the_diagonal():
    rc, msg = create(uplo=7, rp=None, ci=None, va=None, out=None)
    assert rc == 1 and "uplo must be" in msg, msg
    rc, msg = create(rp=None, ci=BAD_CI)
    assert rc == 1 and "NULL argument" in msg, msg
    zero_diag = ZERO_DIAG
    rc, msg = create(rp=BAD_RP, va=zero_diag)
    assert rc == 1 and "not monotone" in msg, msg
    rc, msg = create(ci=BAD_CI, va=zero_diag)
    assert rc == 1 and "out of range" in msg, msg


def test_a_diagonal_that_vanishes_only_in_fp32_is_refused_only_there():
    tiny = np.array([2.0, 0.5, 0.25, 1e-60, 0.125, 0.5, 1.0])          # non-zero in fp64, 0 after narrowing to fp32
    rc, msg = create(precision=F32, va=tiny)
    assert rc == 1 and "trsv" in msg and "the diagonal of row 1 is 0" in msg, msg
    huge = np.array([2.0, 0.5, 0.25, 1e60, 0.125, 0.5, 1.0])           # finite in fp64, inf after narrowing
    rc, msg = create(precision=F32, va=huge)
    assert rc == 1 and "the diagonal of row 1 is inf" in msg, msg
    if not has_gpu():
        for va in (tiny, huge):
            rc, msg = create(precision=F64, va=va)
            assert rc == 1 and "no HIP device available" in msg, msg


def test_unit_ignores_the_stored_diagonal_whatever_it_holds():
    """zero, NaN, doubled or missing diagonals pass the host checks under DIAG_UNIT: what is left is the device"""
    cases = [dict(va=np.array([2.0, 0.5, 0.25, 0.0, 0.125, 0.5, np.nan])), dict(ci=np.array([0, 1, 0, 1, 1, 1, 2], np.int32)),
             dict(rp=NO_DIAG[0], ci=NO_DIAG[1], va=NO_DIAG[2])]
    for args in cases:
        rc, msg = create(diag=UNIT, **args)
        if has_gpu():
            assert rc == 0, msg
        else:
            assert rc == 1 and "trsv" in msg and "no HIP device available" in msg, msg


@pytest.mark.parametrize("precision", (F64, F32))
@pytest.mark.parametrize("diag", (STORED, UNIT))
@pytest.mark.parametrize("uplo", (LOWER, UPPER))
def test_a_valid_matrix_reaches_the_device_step(uplo, diag, precision):
    """without a GPU: the library's no-device message, named as trsv's; with one: a handle"""
    for args in (dict(), dict(n=0, rp=np.zeros(1, np.int32), ci=None, va=None)):
        rc, msg = create(uplo=uplo, diag=diag, precision=precision, **args)
        if has_gpu():
            assert rc == 0, msg
        else:
            assert rc == 1
            assert "trsv" in msg and "no HIP device available: this engine has no CPU fallback" in msg, msg


def test_the_other_entries_refuse_a_null_handle():
    import spmv_mi355x as E
    L = E.lib()
    b = np.ones(3)
    assert L.spmv_mi355x_trsv_solve(None, P(b), P(b)) == 1 and b"trsv" in L.spmv_mi355x_last_error()
    assert L.spmv_mi355x_trsv_solve_device_async(None, None, None, None) == 1 and b"trsv" in L.spmv_mi355x_last_error()
    assert L.spmv_mi355x_trsv_info(None, None, None, None, None, None, None) == 1 and b"trsv" in L.spmv_mi355x_last_error()
    ms = ctypes.c_double(-1.0)
    assert L.spmv_mi355x_time_trsv_device(None, None, None, 1, None, ctypes.byref(ms)) == 1 and b"trsv" in L.spmv_mi355x_last_error()
    assert L.spmv_mi355x_trsv_mem_footprint(None) == 0.0
    assert L.spmv_mi355x_trsv_destroy(None) == 0
    assert np.all(b == 1.0) and ms.value == -1.0


ANALYZE_ERRORS = [
    ("uplo", dict(uplo=3), "uplo must be"),
    ("n_negative", dict(n=-2), "out of range"),
    ("chain_rows", dict(chain_rows=70000), "chain_rows must be"),
    ("null_row_ptr", dict(rp=None), "NULL argument ( row_ptr"),
    ("null_col_idx", dict(ci=None), "NULL argument ( col_idx"),
    ("row_ptr_not_from_0", dict(rp=np.array([2, 2, 5, 7], np.int32)), "row_ptr must start at 0"),
    ("row_ptr_not_monotone", dict(rp=BAD_RP), "row_ptr is not monotone at row 1"),
    ("column_out_of_range", dict(ci=BAD_CI), "column index 3 out of range [0,3) at entry 3"),
]


@pytest.mark.parametrize("case,args,phrase", ANALYZE_ERRORS, ids=[e[0] for e in ANALYZE_ERRORS])
def test_analyze_errors(case, args, phrase):
    import spmv_mi355x as E
    a = dict(uplo=LOWER, n=3, rp=good()[0], ci=good()[1], chain_rows=0)
    a.update(args)
    lv = ctypes.POINTER(ctypes.c_int32)()
    levels = ctypes.c_long(-9)
    rc = E.lib().spmv_mi355x_trsv_analyze(a["uplo"], ctypes.c_long(a["n"]), P(a["rp"]), P(a["ci"]), a["chain_rows"], ctypes.byref(lv),
                                          ctypes.byref(levels), None, None, None)
    msg = E.lib().spmv_mi355x_last_error().decode()
    assert rc == 1 and "trsv" in msg and phrase in msg, msg
    assert not lv and levels.value == -9


# ---- the analysis against the restated rules ----------------------------------------------------------------------------------------

ANALYSIS = [("empty", 0), ("one", 0), ("diagonal", 0), ("diagonal", 1), ("bidiagonal", 0), ("bidiagonal", 1), ("prescribed", 64),
            ("prescribed", 0), ("prescribed", 65536), ("dag", 0), ("dag", 1), ("dag", 8), ("dag", 64), ("stencil", 0), ("stencil", 300),
            ("padding", 0), ("padding", 299)]


@pytest.mark.parametrize("uplo", (LOWER, UPPER), ids=("lower", "upper"))
@pytest.mark.parametrize("name,chain_rows", ANALYSIS, ids=[f"{a}-{c}" for a, c in ANALYSIS])
def test_analyze_matches_the_restated_rules(name, chain_rows, uplo):
    import spmv_mi355x as E
    rp, ci, va, n = tc.matrix(name, uplo)
    got = E.trsv_analyze(rp, ci, n, "lower" if uplo == LOWER else "upper", chain_rows)
    assert got["chain_rows"] == (chain_rows if chain_rows else got["chain_rows"]) and 1 <= got["chain_rows"] <= 65536
    level = tc.levels_of(rp, ci, n, uplo)
    levels, launches, widest = tc.plan_of(level, got["chain_rows"])     # the launch count from the threshold the library used
    assert got["level_of_row"].dtype == np.int32 and np.array_equal(got["level_of_row"], level)
    assert (got["levels"], got["launches"], got["max_level_rows"]) == (levels, launches, widest)


def test_the_named_shapes_are_what_their_names_say():
    """the restated rules themselves, on the cases whose answer is known in closed form"""
    import spmv_mi355x as E
    for uplo in (LOWER, UPPER):
        side = "lower" if uplo == LOWER else "upper"
        a = E.trsv_analyze(*tc.matrix("empty", uplo)[:2], 0, side)
        assert (a["levels"], a["launches"], a["max_level_rows"], len(a["level_of_row"])) == (0, 0, 0, 0)
        a = E.trsv_analyze(*tc.matrix("one", uplo)[:2], 1, side)
        assert (a["levels"], a["launches"], a["max_level_rows"]) == (1, 1, 1)
        a = E.trsv_analyze(*tc.matrix("diagonal", uplo)[:2], 1500, side)
        assert (a["levels"], a["launches"], a["max_level_rows"]) == (1, 1, 1500)
        a = E.trsv_analyze(*tc.matrix("bidiagonal", uplo)[:2], 4097, side)
        assert (a["levels"], a["launches"], a["max_level_rows"]) == (4097, 1, 1)
        want = np.arange(4097) if uplo == LOWER else np.arange(4096, -1, -1)
        assert np.array_equal(a["level_of_row"], want)
        rp, ci, va, n = tc.matrix("prescribed", uplo)
        a = E.trsv_analyze(rp, ci, n, side, 64)
        assert np.array_equal(np.bincount(a["level_of_row"]), tc.PRESCRIBED_WIDTHS)
        # thin runs [1,1,1] [1] [64] [3] [1,1] and the levels of 2000, 70, 65 and 3000 rows
        assert (a["levels"], a["launches"], a["max_level_rows"], a["chain_rows"]) == (12, 9, 3000, 64)
        a = E.trsv_analyze(*tc.matrix("dag", uplo)[:2], 3000, side)
        lv = a["level_of_row"] if uplo == LOWER else a["level_of_row"][::-1]
        assert np.any(np.diff(lv.astype(np.int64)) < 0), "the random DAG's levels must not be monotone in the row index"


def test_a_full_matrix_is_analyzed_as_its_kept_triangle():
    import spmv_mi355x as E
    full = tc.stencil_full()
    for uplo, side in ((LOWER, "lower"), (UPPER, "upper")):
        a = E.trsv_analyze(full[0], full[1], full[3], side)
        t = tc.triangle(*full, uplo)
        assert np.array_equal(a["level_of_row"], tc.levels_of(t[0], t[1], t[3], uplo))
        assert a["levels"] == 3 * 23 + 1                   # the hyperplanes i + j + k of a 24^3 grid
        assert (a["levels"], a["launches"], a["max_level_rows"]) == tc.plan_of(a["level_of_row"], a["chain_rows"])


def test_the_reference_solves_the_system():
    """the C reference against a dense numpy solve: the yardstick of the GPU tier is a triangular solve"""
    rp, ci, va, n = tc.matrix("dag", LOWER)
    D = np.zeros((n, n))
    np.add.at(D, (np.repeat(np.arange(n), np.diff(rp)), ci), va)
    b = np.random.default_rng(5).uniform(-1, 1, n)
    x = tc.reference(rp, ci, va, n, LOWER, False, b, np.float64)
    assert np.all(np.isfinite(x))
    # per row at most 8 fmas and a division on partial sums of modulus <= 1 + 0.9 * 10, then numpy's own 9 products of modulus <= 20
    # and their sum: fewer than 500 roundings of a quantity of modulus <= 1
    assert np.abs(D @ x - b).max() <= 500 * 2.0 ** -53
