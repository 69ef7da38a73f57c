"""CPU tier of "AMG: new values for a hierarchy" (include/spmv_mi355x.h): the symbols are exported, declared and bound, the struct has
the header's size, the refusals that touch no device come back, and the references the GPU tier compares against are themselves
checked here: the frozen loops of tests/amg_update_reference.c equal tests/amg_reference.c bit for bit when they are given its own
aggregates, agree with a scipy restatement of the frozen hierarchy within a measured bound, and the recorded premises, bounds and CG
counts of amg_update_cases.py are recomputed."""
import ctypes
import os

import numpy as np
import pytest

import amg_cases as ac
import amg_update_cases as uc
from conftest import ROOT

UPDATE_SYMBOLS = ["spmv_mi355x_amg_update_values_prepare", "spmv_mi355x_amg_update_values", "spmv_mi355x_amg_update_values_device",
                  "spmv_mi355x_amg_update_values_state", "spmv_mi355x_amg_update_info"]


def test_the_symbols_are_exported_declared_and_bound():
    import spmv_mi355x as E
    header = open(os.path.join(ROOT, "include", "spmv_mi355x.h")).read()
    for sym in UPDATE_SYMBOLS:
        assert hasattr(E.lib(), sym) and sym in E.SYMBOLS and sym + "(" in header, sym
    for name in ("update_values_prepare", "update_values", "update_values_device", "update_values_state", "update_info"):
        assert callable(getattr(E.Amg, name))
    # unsigned + 2 ints, (padding), a long, 5 doubles
    assert ctypes.sizeof(E.AmgUpdateStats) == 16 + 8 + 5 * 8 and E.AmgUpdateStats.updates.offset == 16
    for phrase in ("FROZEN, exactly what amg_create found", "tests/amg_update_reference.c", "re-aggregating when the strength pattern drifts",
                   "an asynchronous update", "update_values for fsai"):
        assert phrase in header, phrase


def test_refusals_that_touch_no_device():
    import spmv_mi355x as E
    L = E.lib()
    va = np.ones(4)
    info = E.AmgUpdateStats()
    info.struct_size = ctypes.sizeof(E.AmgUpdateStats)
    for call, prefix in ((lambda: L.spmv_mi355x_amg_update_values_prepare(None), b"amg_update_values_prepare: NULL handle"),
                         (lambda: L.spmv_mi355x_amg_update_values(None, va.ctypes.data_as(ctypes.c_void_p)), b"amg_update_values: NULL handle"),
                         (lambda: L.spmv_mi355x_amg_update_values(None, None), b"amg_update_values: NULL handle"),
                         (lambda: L.spmv_mi355x_amg_update_values_device(None, None, None), b"amg_update_values: NULL handle"),
                         (lambda: L.spmv_mi355x_amg_update_info(None, ctypes.byref(info)), b"amg_update_info: NULL handle")):
        assert call() == 1
        assert L.spmv_mi355x_last_error().startswith(prefix), L.spmv_mi355x_last_error()
    assert L.spmv_mi355x_amg_update_values_state(None) == 0 and b"NULL handle" in L.spmv_mi355x_last_error()
    assert np.all(va == 1)


# ---- the frozen reference ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ac.CASES)
def test_the_frozen_reference_given_the_references_aggregates_is_the_reference(name):
    rp, ci, _, n, _ = ac.case(name)
    for vset in ("v1", "x0.7") + tuple(v for c, v in uc.SAME_STRUCTURE + uc.FROZEN_CASES if c == name and v != "x0.7"):
        if n == 0 and vset != "v1":
            continue
        fresh = uc.fresh_of(name, vset)
        frozen = uc.frozen_reference(rp, ci, uc.values(name, vset), n, fresh)
        assert uc.equal_to_the_bit(frozen, fresh) is None, f"{name} {vset}: {uc.equal_to_the_bit(frozen, fresh)}"


def test_the_premises():
    """x0.7 and (n129, sym1e-2) keep the aggregates; sym0.5 and diag+1 do not on the grid, which is why the frozen reference exists"""
    for name, vset in uc.SAME_STRUCTURE:
        assert uc.same_structure(name, vset), (name, vset)
        assert uc.equal_to_the_bit(uc.frozen_of(name, vset), uc.fresh_of(name, vset)) is None
    assert not uc.same_structure("grid", "sym0.5") and not uc.same_structure("grid", "diag+1") and not uc.same_structure("grid", "sym1e-2")
    assert [L["n"] for L in uc.fresh_of("grid", "diag+1")["lev"]] == [2025, 382]
    assert [L["n"] for L in uc.frozen_of("grid", "diag+1")["lev"]] == [2025, 382, 43]
    assert [L["n"] for L in uc.fresh_of("aniso", "sym0.5")["lev"]] == [1600, 402, 120]
    print(f"[amg update] aniso, sym0.5: the same aggregates: {uc.same_structure('aniso', 'sym0.5')}; path_wrap, path9: "
          f"{uc.same_structure('path_wrap', 'path9')}")


def test_the_frozen_reference_against_the_restatement():
    measured = 0.0
    for name, vset in uc.FROZEN_CASES:
        own = uc.frozen_restatement_distance(name, vset, "longdouble")
        got = uc.frozen_restatement_distance(name, vset, uc.frozen_of(name, vset))
        print(f"[amg update] {name} {vset}: the restatement moves by {own:.3g} between fp64 and longdouble, the C loops lie {got:.3g} from it")
        measured = max(measured, own)
        assert got <= uc.FROZEN_BOUND, f"{name} {vset}: {got:.3g} against {uc.FROZEN_BOUND:.3g}"
    assert 0.5 * uc.FROZEN_MEASURED <= measured <= uc.FROZEN_MEASURED, measured
    assert np.isclose(uc.FROZEN_BOUND, 10 * uc.FROZEN_MEASURED, rtol=1e-12, atol=0)


def test_the_recorded_counts():
    """a frozen hierarchy converges like a fresh one, a stale one does not"""
    for vset, want in uc.FROZEN_COUNTS.items():
        fresh, frozen, stale = uc.grid_counts(vset)
        print(f"[amg update] grid {vset}: fresh {fresh}, frozen {frozen}, stale {stale}")
        assert (fresh, frozen, stale) == want
        assert frozen <= fresh + 1 and stale > frozen


def test_values_whose_coarse_diagonal_is_not_positive_exist():
    v2, level = uc.coarse_failure_values()
    rp, ci, va, n, _ = ac.case("grid")
    rows = np.repeat(np.arange(n), np.diff(rp))
    assert level == 1 and np.array_equal(v2[rows == ci], va[rows == ci]) and np.all(v2[rows == ci] > 0)
