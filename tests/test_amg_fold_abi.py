"""CPU tier of "AMG: the small levels as one launch" (include/spmv_mi355x.h): the symbols are exported, declared and bound, the stats
struct has the header's size, the refusals that need no handle come back, and the reference the GPU tier compares against
(tests/amg_fold_reference.c) is itself checked here, in float and double, against amg_cases.cycle_of restricted to the tail within
amg_cases.CYCLE_BOUND, with the lanes per row of the header's rule."""
import ctypes
import os
import re

import numpy as np
import pytest

import amg_cases as ac
import amg_fold_cases as fo
from conftest import ROOT

FOLD_SYMBOLS = ["spmv_mi355x_amg_set_fold", "spmv_mi355x_amg_fold_info", "spmv_mi355x_amg_apply_level_device_async"]


def test_the_symbols_are_exported_declared_and_bound():
    import spmv_mi355x as E
    header = open(os.path.join(ROOT, "include", "spmv_mi355x.h")).read()
    for sym in FOLD_SYMBOLS:
        assert hasattr(E.lib(), sym) and sym in E.SYMBOLS and sym + "(" in header, sym
    for name in ("set_fold", "fold_info", "apply_level", "apply_level_device"):
        assert callable(getattr(E.Amg, name))
    assert isinstance(E.Amg.fold_rows, property)
    # what is built left the list of what is not; what is still missing is listed
    assert "form, folding the small levels into one launch" not in header
    for phrase in ("NOT BUILT: update_values for a hierarchy", "NOT BUILT: a multi-workgroup tail", "folding by entries instead of rows",
                   "a fold for FSAI", "W-cycles inside the tail", "tests/amg_fold_reference.c"):
        assert phrase in header, phrase


def test_the_stats_struct():
    import spmv_mi355x as E
    S = E.AmgFoldStats
    # unsigned + 3 ints, 4 longs, 16 ints, a double
    assert ctypes.sizeof(S) == 16 + 4 * 8 + 16 * 4 + 8 == 120
    assert (S.fold_rows.offset, S.first_level.offset, S.folded_levels.offset, S.launches_per_apply.offset) == (4, 8, 12, 16)
    assert (S.spmvs_per_apply.offset, S.tail_products.offset, S.tail_entries.offset, S.lanes_per_row.offset, S.bytes.offset) == (24, 32, 40, 48, 112)
    header = open(os.path.join(ROOT, "include", "spmv_mi355x.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} spmv_mi355x_amg_fold_stats;", header).group(1)
    names = re.findall(r"(\w+)(?:\[\w+\])?[,;]", body)
    assert names == [k for k, _ in S._fields_], names


def test_refusals_that_need_no_handle():
    import spmv_mi355x as E
    L = E.lib()
    info = E.AmgFoldStats()
    info.struct_size = ctypes.sizeof(E.AmgFoldStats)
    v = np.ones(4)
    p = v.ctypes.data_as(ctypes.c_void_p)
    for call, prefix in ((lambda: L.spmv_mi355x_amg_set_fold(None, 0), b"amg_set_fold: NULL handle"),
                         (lambda: L.spmv_mi355x_amg_set_fold(None, -1), b"amg_set_fold: NULL handle"),
                         (lambda: L.spmv_mi355x_amg_fold_info(None, ctypes.byref(info)), b"amg_fold_info: NULL handle"),
                         (lambda: L.spmv_mi355x_amg_apply_level_device_async(None, 0, p, p, None), b"amg_apply_level: NULL handle"),
                         (lambda: L.spmv_mi355x_amg_apply_level_device_async(None, -1, None, None, None), b"amg_apply_level: NULL handle")):
        assert call() == 1
        assert L.spmv_mi355x_last_error().startswith(prefix), L.spmv_mi355x_last_error()
    assert np.all(v == 1)


# ---- the reference ---------------------------------------------------------------------------------------------------------------------

def test_the_rule_of_the_lanes_per_row():
    """the header's rule restated in Python, the reference's and the one the header and the reference file write down"""
    lib = fo.reference_lib(np.float64)
    for n, nnz in [(1, 1), (2, 4), (43, 43 * 20), (129, 129 * 7 - 12), (272, 814), (301, 301 * 301), (382, 3500), (511, 511 * 300), (512, 5000),
                   (513, 5000), (1024, 9000), (1025, 10 ** 6), (3450, 10348), (4697, 42000), (16, 16 * 16), (7, 7 * 7), (8, 8 * 200), (65536, 10 ** 7)]:
        want = max([g for g in (1, 2, 4, 8, 16, 32, 64) if g <= min(64, nnz // n, 1024 // n)], default=1)
        assert fo.lanes(n, nnz) == lib.amg_fold_reference_lanes(n, nnz) == want, (n, nnz)
    assert fo.lanes(301, 301 * 301) == 2 and fo.lanes(8, 1600) == 64 and fo.lanes(2025, 9945) == 1
    rule = "power of two <= min(64, nnz / n, 1024 / n) in integer division"
    assert rule in open(os.path.join(ROOT, "tests", "amg_fold_reference.c")).read()
    header = " ".join(open(os.path.join(ROOT, "include", "spmv_mi355x.h")).read().replace(" * ", " ").split())
    assert "power of two that is <= min(64, nnz(A_l) / n_l, 1024 / n_l) in integer division" in header


def test_stable_transposition():
    rng = np.random.default_rng(5)
    import scipy.sparse as sp
    P = sp.random(37, 11, 0.3, random_state=3, format="csr")
    P.sort_indices()
    rp, ci, va = fo.stable_transpose(P.indptr.astype(np.int32), P.indices.astype(np.int32), P.data, 37, 11)
    T = P.T.tocsr()
    T.sort_indices()
    assert np.array_equal(rp, T.indptr) and np.array_equal(ci, T.indices) and np.array_equal(va, T.data)
    # unsorted rows with no column twice: inside a column the rows still ascend
    perm = np.concatenate([rng.permutation(np.arange(a, b)) for a, b in zip(P.indptr[:-1], P.indptr[1:])]).astype(int)
    rp2, ci2, va2 = fo.stable_transpose(P.indptr.astype(np.int32), P.indices[perm].astype(np.int32), P.data[perm], 37, 11)
    assert np.array_equal(rp2, rp) and np.array_equal(ci2, ci) and np.array_equal(va2, va)


def _sub(ref, first):
    return dict(levels=ref["levels"] - first, stalled=ref["stalled"], lev=ref["lev"][first:])


@pytest.mark.parametrize("name,spec", [f for f in fo.FOLDS if f[1] != 1])
def test_the_reference_against_the_restated_cycle(name, spec):
    """cycle(f, v) of the sequential loops lies within CYCLE_BOUND of amg_cases.cycle_of over the levels f.., with G from the rule"""
    ref = ac.reference_of(name)
    rows = [L["n"] for L in ref["lev"]]
    f = fo.first_level(rows, fo.fold_rows_of(name, spec))
    assert f < len(rows)
    for dtype in (np.float64, np.float32):
        tail = fo.tail_of(name, dtype, f)
        assert tail.lanes == [fo.lanes(L["n"], len(L["A"][1])) for L in ref["lev"]]
        want_of = ac.cycle_of(_sub(ref, f), dtype, **ac.options(name))
        worst = 0.0
        for v in ac.vectors(rows[f]):
            v = v.astype(dtype)
            got = tail.apply(v)
            assert got.dtype == dtype and np.all(np.isfinite(got))
            assert np.array_equal(got, tail.apply(v)), "twice"
            want = want_of(v).astype(np.float64)
            worst = max(worst, float(np.abs(got.astype(np.float64) - want).max() / np.abs(want).max()))
        print(f"[amg fold] reference {name} f = {f} {np.dtype(dtype).name}: lanes {tail.lanes[f:]}, dense {tail.dense}, {worst:.3g} from the "
              f"restatement, {worst / ac.CYCLE_BOUND[dtype]:.3g} of the bound")
        assert worst <= ac.CYCLE_BOUND[dtype], f"{name} f = {f} {np.dtype(dtype).name}: {worst:.3g} against {ac.CYCLE_BOUND[dtype]:.3g}"


def test_more_lanes_per_row_than_one_are_exercised():
    """on grid's level 1 and on n129 the rule gives G > 1, and the reference with G lanes differs from the plain chain by rounding only"""
    assert fo.tail_of("grid", np.float64, 1).lanes[1] > 1 and fo.tail_of("n129", np.float64, 0).lanes[0] > 1
    ref = ac.reference_of("n129")
    v = ac.vectors(129)[0]
    split = fo.tail_of("n129", np.float64, 0).apply(v)
    plain = fo.Tail(ref, np.float64, 0, lanes_per_row=[1] * ref["levels"], **ac.options("n129")).apply(v)
    assert np.abs(split - plain).max() <= ac.CYCLE_BOUND[np.float64] * np.abs(plain).max()


def test_the_first_folded_level():
    rows = [4000000, 441111, 45913, 4697, 703, 511, 301]
    assert [fo.first_level(rows, r) for r in (0, 1, 300, 301, 1024, 8192, 65536)] == [7, 7, 7, 6, 4, 3, 2]
    assert fo.first_level([2025, 382, 43], 4096) == 0 and fo.first_level([], 4096) == 0
