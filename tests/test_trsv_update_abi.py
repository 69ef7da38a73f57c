"""CPU tier of update_values for triangular solve handles (include/spmv_mi355x.h "UPDATE_VALUES"): the symbols are exported and
bound, spmv_mi355x_trsv_update_map gives exactly what a numpy restatement of the stored layout gives, the map has the properties the
header states, and every refusal that needs no device comes back as rc 1 in the stated order.

The restatement (layout_of) is written from the header's words, not from the library's walk: positions ordered by (block, level
within the block, row), every (block, level) group cut into slices of up to 64 positions, entry k of lane r of a slice at
slice start + k * lanes + r, a row's kept entries in stored order, padding = -1. The levels come from trsv_cases.levels_of, on the
CSR without the entries that leave the row's block for the blocked form (trsv_blocked_cases.filtered)."""
import ctypes
import functools

import numpy as np
import pytest

import trsv_blocked_cases as bc
import trsv_cases as tc
from trsv_cases import LOWER, UPPER

STORED, UNIT = 0, 1
P = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
UPLO = {LOWER: "lower", UPPER: "upper"}
DIAG = {STORED: "stored", UNIT: "unit"}


def test_the_symbols_are_exported_and_bound():
    import spmv_mi355x as E
    for name in ("spmv_mi355x_trsv_update_map", "spmv_mi355x_trsv_update_values_prepare", "spmv_mi355x_trsv_update_values_bytes",
                 "spmv_mi355x_trsv_update_values_state", "spmv_mi355x_trsv_update_values_device_async",
                 "spmv_mi355x_trsv_update_values_result", "spmv_mi355x_trsv_update_values_device", "spmv_mi355x_trsv_update_values",
                 "spmv_mi355x_trsv_update_values_staged", "spmv_mi355x_trsv_stored_values"):
        assert hasattr(E.lib(), name) and name in E.SYMBOLS, name
    for name in ("update_values_prepare", "update_values", "update_values_device", "update_values_result", "update_values_state",
                 "update_values_bytes", "stored_values"):
        assert hasattr(E.TriangularSolve, name), name
    assert callable(E.trsv_update_map) and callable(E.sgs_precond_update) and hasattr(E.Ilu0, "update_precond")


# ---- the layout, restated -----------------------------------------------------------------------------------------------------------

def kept_of_row(rp, ci, i, uplo, B):
    """the entries of row i a solve reads beside the diagonal, in stored order"""
    js = np.arange(rp[i], rp[i + 1])
    c = ci[js].astype(np.int64)
    keep = c < i if uplo == LOWER else c > i
    if B:
        keep &= c // B == i // B
    return js[keep]


def layout_of(rp, ci, n, uplo, stored, B=None):
    """(slot_src, diag_src or None, perm) of the header's layout; B = None is the global form"""
    rp = np.asarray(rp, np.int64)
    if B:
        f = bc.filtered(rp, ci, np.zeros(len(ci)), n, B)
        level = tc.levels_of(f[0], f[1], n, uplo)
    else:
        level = tc.levels_of(rp, ci, n, uplo)
    block = np.arange(n) // B if B else np.zeros(n, np.int64)
    perm = np.lexsort((np.arange(n), level, block))                  # (block, level, row)
    key = block[perm] * (int(level.max()) + 1 if n else 1) + level[perm]
    starts = np.concatenate([[0], np.flatnonzero(np.diff(key)) + 1, [n]]) if n else np.zeros(1, np.int64)
    out = []
    for g in range(len(starts) - 1):
        for s0 in range(starts[g], starts[g + 1], 64):
            lanes = min(64, starts[g + 1] - s0)
            ent = [kept_of_row(rp, ci, perm[s0 + r], uplo, B) for r in range(lanes)]
            tile = np.full((max(len(e) for e in ent), lanes), -1, np.int64)
            for r, e in enumerate(ent):
                tile[:len(e), r] = e
            out.append(tile.ravel())
    slot_src = np.concatenate(out).astype(np.int32) if out else np.zeros(0, np.int32)
    diag_src = None
    if stored:
        diag_src = np.array([rp[i] + np.flatnonzero(ci[rp[i]:rp[i + 1]] == i)[0] for i in perm], np.int32).reshape(n)
    return slot_src, diag_src, perm


@functools.lru_cache(maxsize=None)
def case_matrix(name, uplo):
    if name == "convdiff":                                           # both triangles are stored: the other one must never appear
        return bc.convdiff()[:4]
    if name == "stencil_full":
        return tc.stencil_full()
    return tc.matrix(name, uplo)


MAP_CASES = [(name, None) for name in ("prescribed", "padding", "dag", "stencil", "stencil_full", "empty", "one")] + \
            [(name, B) for name in ("stencil", "convdiff") for B in (64, 100, 256)] + [("empty", 64), ("one", 64)]


@pytest.mark.parametrize("diag", (STORED, UNIT), ids=("stored", "unit"))
@pytest.mark.parametrize("uplo", (LOWER, UPPER), ids=("lower", "upper"))
@pytest.mark.parametrize("name,B", MAP_CASES, ids=[f"{n}-{b}" for n, b in MAP_CASES])
def test_the_map_is_the_restated_layout(name, B, uplo, diag):
    import spmv_mi355x as E
    rp, ci, va, n = case_matrix(name, uplo)
    got = E.trsv_update_map(rp, ci, n, UPLO[uplo], DIAG[diag], block_rows=B)
    slot_src, diag_src, perm = layout_of(rp, ci, n, uplo, diag == STORED, B)
    assert got["slots"] == len(slot_src) == len(got["slot_src"])
    assert got["slot_src"].dtype == np.int32 and np.array_equal(got["slot_src"], slot_src)
    if diag == STORED:
        assert np.array_equal(got["diag_src"], diag_src)
    else:
        assert got["diag_src"] is None
    # the properties, stated without the layout: every kept entry once and in stored order, nothing else, padding = the rest
    rows = np.repeat(np.arange(n), np.diff(rp))
    kept = ci < rows if uplo == LOWER else ci > rows
    if B:
        kept &= ci // B == rows // B
    src = got["slot_src"][got["slot_src"] >= 0]
    assert np.array_equal(np.sort(src), np.flatnonzero(kept))
    assert np.sum(got["slot_src"] == -1) == got["slots"] - kept.sum() and got["slot_src"].min(initial=-1) >= -1
    by_row = src[np.argsort(rows[src], kind="stable")]                # a row's entries in the order of their slots
    assert np.all((np.diff(by_row) > 0) | (np.diff(rows[by_row]) != 0))
    if diag == STORED and n:
        d = got["diag_src"]
        assert np.array_equal(ci[d], rows[d]) and np.array_equal(np.sort(rows[d]), np.arange(n)) and np.array_equal(rows[d], perm)
        first = np.array([rp[i] + np.flatnonzero(ci[rp[i]:rp[i + 1]] == i)[0] for i in range(n)])
        assert np.array_equal(d, first[perm])


def test_chain_rows_does_not_change_the_map():
    import spmv_mi355x as E
    rp, ci, va, n = tc.matrix("prescribed", LOWER)
    a = E.trsv_update_map(rp, ci, n, "lower", chain_rows=0)
    b = E.trsv_update_map(rp, ci, n, "lower", chain_rows=1)
    assert np.array_equal(a["slot_src"], b["slot_src"]) and np.array_equal(a["diag_src"], b["diag_src"])


def test_duplicates_are_separate_entries_and_the_first_diagonal_counts():
    import spmv_mi355x as E
    # row 1 stores column 0 twice; under UNIT row 1 may store its diagonal twice, which nobody reads
    rp = np.array([0, 1, 5], np.int32)
    ci = np.array([0, 0, 1, 0, 1], np.int32)
    got = E.trsv_update_map(rp, ci, 2, "lower", "unit")
    assert got["slot_src"].tolist() == [1, 3] and got["diag_src"] is None
    with pytest.raises(E.SpmvError, match="trsv_update_map: row 1 stores 2 entries with column 1"):
        E.trsv_update_map(rp, ci, 2, "lower", "stored")


# ---- refusals on the host, in their order --------------------------------------------------------------------------------------------

def good():
    rp = np.array([0, 2, 5, 7], np.int32)
    ci = np.array([0, 1, 0, 1, 2, 1, 2], np.int32)
    return rp, ci


def update_map(uplo=LOWER, diag=STORED, n=3, rp="good", ci="good", chain_rows=0, block_rows=-1):
    import spmv_mi355x as E
    g = good()
    rp, ci = (g[k] if isinstance(a, str) else a for k, a in enumerate((rp, ci)))
    ss, ds, slots = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_long(-7)
    rc = E.lib().spmv_mi355x_trsv_update_map(uplo, diag, n, P(rp), P(ci), chain_rows, block_rows, ctypes.byref(ss), ctypes.byref(slots),
                                             ctypes.byref(ds))
    msg = E.lib().spmv_mi355x_last_error().decode()
    if rc == 0:
        E.lib().spmv_mi355x_free(ss)
        E.lib().spmv_mi355x_free(ds)
    else:
        assert ss.value is None and ds.value is None
    return rc, msg


BAD_RP, BAD_CI = np.array([0, 2, 1, 7], np.int32), np.array([0, 1, 0, 3, 2, 1, 2], np.int32)
NO_DIAG = (np.array([0, 2, 3, 5], np.int32), np.array([0, 1, 0, 1, 2], np.int32))
TWO_DIAG = (np.array([0, 2, 5, 7], np.int32), np.array([0, 1, 1, 1, 2, 1, 2], np.int32))
# (step, case, arguments, phrase, an error of a LATER step added to the same call: the earlier one must be reported)
ERRORS = [
    (1, "uplo", dict(uplo=2), "uplo must be SPMV_MI355X_LOWER (0) or SPMV_MI355X_UPPER (1) (got 2)", dict(rp=None)),
    (1, "diag", dict(diag=2), "diag must be SPMV_MI355X_DIAG_STORED (0) or SPMV_MI355X_DIAG_UNIT (1) (got 2)", dict(rp=None)),
    (1, "n_negative", dict(n=-1), "n = -1 out of range", dict(rp=None)),
    (1, "chain_rows", dict(chain_rows=65537), "chain_rows must be 0 (the default) or 1 .. 65536 (got 65537)", dict(ci=None)),
    (1, "block_rows_large", dict(block_rows=16385), "block_rows must be 0 (the default) or 1 .. 16384 (got 16385)", dict(ci=None)),
    (1, "block_rows_below", dict(block_rows=-2), "block_rows must be -1 (the global form), 0 (the default) or 1 .. 16384 (got -2)",
     dict(uplo=2)),
    (2, "null_row_ptr", dict(rp=None), "NULL argument ( row_ptr", dict(ci=BAD_CI)),
    (2, "null_col_idx", dict(ci=None), "NULL argument ( col_idx", dict(rp=BAD_RP)),
    (3, "row_ptr_not_from_0", dict(rp=np.array([1, 2, 5, 7], np.int32)), "row_ptr must start at 0", dict(ci=TWO_DIAG[1])),
    (3, "row_ptr_not_monotone", dict(rp=BAD_RP), "row_ptr is not monotone at row 1", dict(ci=TWO_DIAG[1])),
    (3, "column_out_of_range", dict(ci=BAD_CI), "column index 3 out of range [0,3) at entry 3", {}),
    (4, "diagonal_missing", dict(rp=NO_DIAG[0], ci=NO_DIAG[1]), "row 1 has no diagonal entry", {}),
    (4, "diagonal_twice", dict(rp=TWO_DIAG[0], ci=TWO_DIAG[1]), "row 1 stores 2 entries with column 1", {}),
]


@pytest.mark.parametrize("step,case,args,phrase,behind", ERRORS, ids=[e[1] for e in ERRORS])
def test_update_map_refusals_in_order(step, case, args, phrase, behind):
    for extra in ({}, behind):
        rc, msg = update_map(**{**extra, **args})
        assert rc == 1 and msg.startswith("trsv_update_map: ") and phrase in msg, (case, msg)
    assert update_map()[0] == 0


def test_unit_needs_no_diagonal():
    assert update_map(diag=UNIT, rp=NO_DIAG[0], ci=NO_DIAG[1])[0] == 0
    assert update_map(diag=UNIT, rp=TWO_DIAG[0], ci=TWO_DIAG[1])[0] == 0


def test_null_handles():
    """the NULL handle is the first check of every entry: a NULL array behind it is not what is reported"""
    import spmv_mi355x as E
    L = E.lib()
    rp, ci = good()
    err = lambda: L.spmv_mi355x_last_error().decode()
    assert L.spmv_mi355x_trsv_update_values_state(None) == 0
    assert L.spmv_mi355x_trsv_update_values_bytes(None) == 0.0
    assert L.spmv_mi355x_trsv_update_values_prepare(None, 3, None, None) == 1 and err() == "trsv_update_values_prepare: NULL handle"
    assert L.spmv_mi355x_trsv_update_values_prepare(None, 3, P(rp), P(ci)) == 1 and err() == "trsv_update_values_prepare: NULL handle"
    for fn in (L.spmv_mi355x_trsv_update_values_device_async, L.spmv_mi355x_trsv_update_values_device):
        assert fn(None, None, None) == 1 and err() == "trsv_update_values: NULL handle"
    assert L.spmv_mi355x_trsv_update_values(None, None) == 1 and err() == "trsv_update_values: NULL handle"
    bad = ctypes.c_long(5)
    assert L.spmv_mi355x_trsv_update_values_result(None, ctypes.byref(bad)) == 1 and err() == "trsv_update_values: NULL handle"
    assert bad.value == -1
    assert L.spmv_mi355x_trsv_update_values_result(None, None) == 1
    slots = ctypes.c_long(5)
    assert L.spmv_mi355x_trsv_stored_values(None, None, ctypes.byref(slots), None) == 1 and err() == "trsv_stored_values: NULL handle"
    out = ctypes.c_void_p(1)
    assert L.spmv_mi355x_trsv_update_values_staged(None, ctypes.byref(out)) == 1 and err().startswith("trsv_update_values_staged: NULL")
    assert out.value is None
