"""CPU tier of the device ILU(0) (include/spmv_mi355x.h "ILU(0)"): the symbols are exported and bound; every argument error comes
back as rc 1 in the documented order and wording (scalars, NULL pointers, the pattern, unsorted rows, the missing diagonal; the device
last); and the yardstick of the GPU tier is itself checked: the C reference of tests/ilu0_reference.c against a dense numpy
restatement, the iteration counts of the restated CG and GMRES under the reference factor, and the levels, launches and dropped
entries a handle must report against the restated analysis of trsv_cases.py / trsv_blocked_cases.py.

The bound between the reference and the restatement, which differ in fma against multiply-then-subtract: an entry receives at most
n - 1 = 69 updates (the dense case; at most 2 on the grids), each of them a product of modulus <= 60 rounded once more, so two correct
evaluations lie within 69 * 60 * 2^-53 < 5e-13 of each other to first order: 1e-12 is asserted, absolute."""
import ctypes

import numpy as np
import pytest

import ilu0_cases as ic
import pcg_tri_cases as pc
import trsv_blocked_cases as bc
import trsv_cases as tc
from conftest import has_gpu
from trsv_cases import LOWER, UPPER

P = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
NAMES = ("spmv_mi355x_ilu0_create", "spmv_mi355x_ilu0_factor", "spmv_mi355x_ilu0_factor_device_async", "spmv_mi355x_ilu0_values",
         "spmv_mi355x_ilu0_values_device", "spmv_mi355x_ilu0_get_info", "spmv_mi355x_ilu0_mem_footprint", "spmv_mi355x_ilu0_destroy")


def test_the_symbols_are_exported_and_bound():
    import spmv_mi355x as E
    for name in NAMES:
        assert hasattr(E.lib(), name) and name in E.SYMBOLS, name
    assert callable(E.ilu0_precond) and all(hasattr(E.Ilu0, a) for a in ("factor", "factor_device", "values", "values_device", "info",
                                                                         "precond", "close"))
    assert ctypes.sizeof(E.Ilu0Info) == ctypes.sizeof(ctypes.c_size_t) + 10 * ctypes.sizeof(ctypes.c_long)


# ---- the reference against the dense restatement -----------------------------------------------------------------------------------

@pytest.mark.parametrize("B", (None, 64, 100, 256), ids=str)
@pytest.mark.parametrize("name", ("spd_grid", "convdiff", "dense70"))
def test_the_reference_is_the_dense_restatement(name, B):
    rp, ci, va, n = ic.matrix(name)
    f, bad = ic.factor(name, B)
    assert bad == -1 and np.all(np.isfinite(f))
    D = ic.dense_of(rp, ci, va, n)
    F = ic.restatement(D, B)
    d = np.abs(ic.dense_of(rp, ci, f, n) - F).max()
    print(f"[ilu0] {name} B={B}: the reference and the restatement differ by {d:.3g}")
    assert d <= 1e-12
    keep = ic.kept(rp, ci, n, B)
    assert np.array_equal(f[~keep], va[~keep])                                # dropped entries keep A's value
    if B is not None and name != "dense70":
        assert (~keep).any()
    # the blocked form is the global loop on the filtered CSR
    if B is not None:
        g = bc.filtered(rp, ci, va, n, B)
        assert np.array_equal(ic.reference(*g)[0], f[keep])


def test_ilu0_of_a_full_pattern_is_lu():
    """the pattern of the dense case is full, so L U = A up to rounding: about 3e-14 here, 1e-12 asserted"""
    rp, ci, va, n = ic.matrix("dense70")
    F = ic.dense_of(rp, ci, ic.factor("dense70")[0], n)
    L, U = np.tril(F, -1) + np.eye(n), np.triu(F)
    d = np.abs(L @ U - ic.dense_of(rp, ci, va, n)).max()
    print(f"[ilu0] dense70: |L U - A| = {d:.3g}")
    assert d <= 1e-12


def test_ilu0_of_an_spd_matrix_is_ic0():
    """U = D L^t for a symmetric matrix, so M = L U is the M of pcg_tri_cases.ic0: (L D^1/2) is its Cholesky-like factor"""
    rp, ci, va, n = ic.matrix("spd_grid")
    F = ic.dense_of(rp, ci, ic.factor("spd_grid")[0], n)
    L, d = np.tril(F, -1) + np.eye(n), np.diag(F)
    assert np.all(d > 0)
    C = pc.problem().ic0()[0]
    assert np.abs(L * np.sqrt(d)[None, :] - C).max() <= 1e-12
    assert np.abs(np.triu(F) - (L * d[None, :]).T).max() <= 1e-12


def test_the_breakdown_row_of_the_reference():
    f, bad = ic.reference(*ic.singular())
    assert bad == 1 and f.tolist() == [1.0, 1.0, 1.0, 0.0]
    rp, ci, va, n = ic.matrix("random")
    assert ic.factor("random")[1] == -1
    rows = np.repeat(np.arange(n), np.diff(rp))
    for value in (0.0, np.nan, np.inf):
        v = va.copy()
        v[(rows == ci) & np.isin(rows, (3, 10))] = value                      # rows 3 and 10 hold only their diagonal
        assert ic.reference(rp, ci, v, n)[1] == 3


# ---- the counts ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", (np.float64, np.float32), ids=("fp64", "fp32"))
def test_the_iteration_counts_under_the_reference_factor(dtype):
    """the table of the header's claim: the global ILU(0) takes IC(0)'s counts, and every blocked ILU(0) beats the SGS of its block size"""
    tol = pc.PREC[dtype]["tol"]
    Pr = pc.problem()
    for B in (None,) + ic.BLOCKS:
        _, hist, stop = ic.pcg_restatement(dtype, B, tol)
        assert stop == 1 and hist.size == ic.COUNTS[dtype][B], (B, hist.size)
    assert ic.COUNTS[dtype][None] == pc.COUNTS[dtype]["ic0"] == Pr.restatement(dtype, "ic0", tol)[1].size
    if dtype == np.float64:
        for B, kind in ((None, "sgs"),) + tuple((b, b) for b in ic.BLOCKS):
            sgs = Pr.restatement(dtype, kind, tol)[1].size
            assert sgs == pc.COUNTS[dtype][kind] and ic.COUNTS[dtype][B] < sgs, (B, sgs)


def test_gmres_under_the_reference_factor_beats_the_blocked_sgs():
    """convdiff(45), restart 20, B = 100: the restatement of test_gpu_gmres_tri.py with the reference ILU(0) against its blocked SGS"""
    import test_gpu_gmres_tri as gt
    Pg = gt.problem()
    rp, ci, va, n = ic.matrix("convdiff")
    M = ic.apply(rp, ci, ic.factor("convdiff", 100)[0], n, 100, np.float64)
    _, hist, stop, _ = gt.restate(Pg.dense(np.float64), Pg.b, 20, M, 1e-12, gt.MAX_ITERATIONS, np.float64)
    sgs = Pg.restatement(np.float64, 20, 100, 1e-12)[1].size
    print(f"[ilu0] gmres(20) on convdiff(45), B = 100: ILU(0) {hist.size}, SGS {sgs}")
    assert stop == 1 and sgs == 80 and hist.size < sgs


# ---- errors, in their order ---------------------------------------------------------------------------------------------------------

def good():
    """a valid 3 x 3 pattern with both triangles, sorted, a stored diagonal"""
    return np.array([0, 2, 5, 7], np.int32), np.array([0, 1, 0, 1, 2, 1, 2], np.int32)


def create(n=3, rp="good", ci="good", block_rows=-1, out="good", device=-1):
    import spmv_mi355x as E
    g = good()
    rp, ci = (g[k] if isinstance(a, str) else a for k, a in enumerate((rp, ci)))
    h = ctypes.c_void_p()
    rc = E.lib().spmv_mi355x_ilu0_create(ctypes.byref(h) if out is not None else None, ctypes.c_long(n), P(rp), P(ci),
                                         ctypes.c_long(block_rows), device)
    msg = E.lib().spmv_mi355x_last_error().decode()
    if rc == 0:
        E.lib().spmv_mi355x_ilu0_destroy(h)
    return rc, msg


BAD_RP, BAD_CI = np.array([0, 2, 1, 7], np.int32), np.array([0, 1, 0, 3, 2, 1, 2], np.int32)
UNSORTED = np.array([0, 1, 1, 0, 2, 1, 2], np.int32)                  # row 1: columns 1, 0, 2
TWICE = np.array([0, 1, 0, 1, 1, 1, 2], np.int32)                     # row 1: columns 0, 1, 1
NO_DIAG = (np.array([0, 2, 3, 5], np.int32), np.array([0, 1, 0, 1, 2], np.int32))
UNSORTED_NO_DIAG = (np.array([0, 2, 3, 5], np.int32), np.array([0, 1, 0, 2, 1], np.int32))         # row 1 no diagonal, row 2 unsorted
ERRORS = [
    (1, "n_negative", dict(n=-1), "n = -1 out of range"),
    (1, "block_rows_negative", dict(block_rows=-2), "block_rows must be -1 (global), 0 (the default) or 1 .. 16384 (got -2)"),
    (1, "block_rows_large", dict(block_rows=16385), "block_rows must be -1 (global), 0 (the default) or 1 .. 16384 (got 16385)"),
    (2, "null_out", dict(out=None), "NULL argument ( out"),
    (2, "null_row_ptr", dict(rp=None), "NULL argument ( row_ptr"),
    (2, "null_col_idx", dict(ci=None), "NULL argument ( col_idx"),
    (3, "row_ptr_not_from_0", dict(rp=np.array([1, 2, 5, 7], np.int32)), "row_ptr must start at 0"),
    (3, "row_ptr_not_monotone", dict(rp=BAD_RP), "row_ptr is not monotone at row 1"),
    (3, "column_out_of_range", dict(ci=BAD_CI), "column index 3 out of range [0,3) at entry 3"),
    (3, "column_negative", dict(ci=np.array([0, 1, 0, 1, 2, -1, 2], np.int32)), "column index -1 out of range [0,3) at entry 5"),
    (4, "unsorted", dict(ci=UNSORTED), "row 1: column 0 follows column 1"),
    (4, "column_twice", dict(ci=TWICE), "row 1: column 1 follows column 1"),
    (4, "unsorted_before_a_missing_diagonal", dict(rp=UNSORTED_NO_DIAG[0], ci=UNSORTED_NO_DIAG[1]), "row 2: column 1 follows column 2"),
    (5, "diagonal_missing", dict(rp=NO_DIAG[0], ci=NO_DIAG[1]), "row 1 has no diagonal entry"),
]
BEHIND = {1: (dict(out=None), dict(rp=BAD_RP), dict(ci=UNSORTED)), 2: (dict(rp=BAD_RP), dict(ci=BAD_CI), dict(ci=UNSORTED)),
          3: (dict(device=99),), 4: (dict(device=99),), 5: (dict(device=99),)}


@pytest.mark.parametrize("step,case,args,phrase", ERRORS, ids=[e[1] for e in ERRORS])
def test_create_errors_in_their_documented_order(step, case, args, phrase):
    rc, msg = create(**args)
    assert rc == 1
    assert msg.startswith("ilu0_create: ") and phrase in msg, msg
    for behind in BEHIND[step]:
        if not set(behind) & set(args):
            rc, msg = create(**args, **behind)
            assert rc == 1 and msg.startswith("ilu0_create: ") and phrase in msg, (behind, msg)


def test_the_device_comes_last():
    """a valid pattern, global, at both ends of block_rows and at the default, and n = 0: without a GPU the library's no-device
    message, named as ilu0_create's; with one a handle"""
    for args in (dict(), dict(block_rows=0), dict(block_rows=1), dict(block_rows=16384), dict(n=0, rp=np.zeros(1, np.int32), ci=None)):
        rc, msg = create(**args)
        if has_gpu():
            assert rc == 0, msg
        else:
            assert rc == 1
            assert msg.startswith("ilu0_create: no HIP device available: this engine has no CPU fallback"), msg


def test_the_entries_that_take_a_handle_refuse_null():
    import spmv_mi355x as E
    L = E.lib()
    values, ptr = np.ones(7), ctypes.c_void_p(5)
    info = E.Ilu0Info()
    info.struct_size = ctypes.sizeof(E.Ilu0Info)
    info.levels = -7
    for call, prefix in ((lambda: L.spmv_mi355x_ilu0_factor(None, P(values)), b"ilu0_factor: "),
                         (lambda: L.spmv_mi355x_ilu0_factor_device_async(None, P(values), None), b"ilu0_factor: "),
                         (lambda: L.spmv_mi355x_ilu0_values(None, P(values)), b"ilu0_values: "),
                         (lambda: L.spmv_mi355x_ilu0_values_device(None, ctypes.byref(ptr)), b"ilu0_values: "),
                         (lambda: L.spmv_mi355x_ilu0_get_info(None, ctypes.byref(info)), b"ilu0_get_info: ")):
        assert call() == 1
        msg = L.spmv_mi355x_last_error()
        assert msg.startswith(prefix) and b"NULL argument ( F" in msg, msg
    assert np.all(values == 1) and ptr.value == 5 and info.levels == -7
    assert L.spmv_mi355x_ilu0_destroy(None) == 0
    assert L.spmv_mi355x_ilu0_mem_footprint(None) == 0.0


# ---- what a handle must report, restated -------------------------------------------------------------------------------------------

def expected_info(name, B):
    """dict(levels, launches, max_level_rows, nnz_dropped, blocks) of the rule: the levels of trsv_cases.levels_of(LOWER) on A's
    pattern, within the blocks for the blocked form (trsv_blocked_cases.analysis_of); one launch per level behind level 0;
    max_level_rows = the most rows of one launch; dropped = the entries of both triangles outside their row's block"""
    rp, ci, va, n = ic.matrix(name)
    if B is None:
        level = tc.levels_of(rp, ci, n, LOWER)
        dropped, blocks = 0, 0
    else:
        a = bc.analysis_of(rp, ci, n, LOWER, B)
        level, blocks = a["level_of_row"], a["blocks"]
        dropped = bc.dropped_of(rp, ci, n, LOWER, B) + bc.dropped_of(rp, ci, n, UPPER, B)
        assert dropped == len(ci) - len(bc.filtered(rp, ci, va, n, B)[1])
    levels = int(level.max()) + 1 if n else 0
    return dict(n=n, nnz=len(ci), levels=levels, launches=max(levels - 1, 0), max_level_rows=int(np.bincount(level).max()) if n else 0,
                nnz_dropped=dropped, block_rows=B or 0, blocks=blocks)


def test_the_expected_info_of_the_named_shapes():
    """the restated rule on the cases whose answer is known in closed form (the GPU tier compares a handle's info with it)"""
    assert expected_info("empty", None) == dict(n=0, nnz=0, levels=0, launches=0, max_level_rows=0, nnz_dropped=0, block_rows=0, blocks=0)
    assert expected_info("one", None)["launches"] == 0 and expected_info("one", None)["levels"] == 1
    a = expected_info("arrow", None)
    assert (a["levels"], a["launches"], a["max_level_rows"], a["nnz"]) == (2, 1, 599, 2 * 599 + 600)
    a = expected_info("pairs", None)
    assert (a["levels"], a["launches"], a["max_level_rows"]) == (2, 1, 35000)
    a = expected_info("dense70", None)
    assert (a["levels"], a["launches"], a["max_level_rows"]) == (70, 69, 1)
    # the 45 x 45 grid: the hyperplanes i + j; in blocks of 100 rows (two grid lines and a bit) far fewer
    a = expected_info("spd_grid", None)
    assert (a["levels"], a["max_level_rows"]) == (89, 45)
    b = expected_info("spd_grid", 100)
    assert b["blocks"] == 21 and b["levels"] < a["levels"] and b["nnz_dropped"] > 0 and b["max_level_rows"] > a["max_level_rows"]
