"""CPU tier of spmv_mi355x_amg_create_with (include/spmv_mi355x.h "AMG: a caller's near-null vector and filtered prolongator
smoothing"): the symbols are exported, declared and bound; the new structs have the header's sizes and offsets; the refusals that
need no device come back with the prefix "amg_create_with:" in amg_create's order, the new ones where the header puts them; and what
the GPU tier compares against is checked here: tests/amg_prolongator_reference.c against the scipy restatement of steps 5a to 5c level
by level (on the reference's own A_l and aggregates, as test_amg_abi.py does), its update loops against its own build, the recorded
counts and cycle bounds of amg_prolongator_cases.py recomputed, and the cycle of every variant symmetric and positive."""
import ctypes
import inspect
import os

import numpy as np
import pytest
import scipy.sparse as sp

import amg_cases as ac
import amg_prolongator_cases as apc
import amg_update_cases as uc
from conftest import ROOT

SELL, F64 = 3, 0
CLOSE = 1e-14                 # test_amg_abi.py's rule: against scipy's products, relative to the largest entry
# test_amg_abi.py's good 3 x 3 matrix, and what is wrong with it from step 3 on
RP, CI, VA = [0, 2, 5, 7], [0, 1, 0, 1, 2, 1, 2], [4.0, -1.0, -1.0, 4.0, -1.0, -1.0, 4.0]
BAD_RP = [0, 2, 1, 7]                                     # 3. not monotone
DUP_CI = [0, 1, 0, 2, 2, 1, 2]                            # 4. row 1 stores column 2 twice
NEG_VA = [4.0, -1.0, -1.0, -4.0, -1.0, -1.0, 4.0]         # 5. the diagonal of row 1 is negative
SYMBOLS = ["spmv_mi355x_amg_create_with", "spmv_mi355x_amg_prolongator_info", "spmv_mi355x_amg_near_null"]


def test_the_symbols_are_exported_declared_and_bound():
    import spmv_mi355x as E
    header = open(os.path.join(ROOT, "include", "spmv_mi355x.h")).read()
    for sym in SYMBOLS:
        assert hasattr(E.lib(), sym) and sym in E.SYMBOLS and sym + "(" in header, sym
    assert list(inspect.signature(E.Amg.build).parameters)[:8] == ["row_ptr", "col_idx", "values", "n", "near_null", "filtered", "fmt", "dtype"]
    for name in ("prolongator_info", "near_null", "level_csr"):
        assert callable(getattr(E.Amg, name))
    assert "SPMV_MI355X_AMG_AF = 2" in header and E.AMG_AF == 2
    # what is built left the lists of what is not; what is still missing is listed
    for phrase in ("filtered prolongator smoothing, near-null-space vectors other than the constant", "filtered smoothing, W- and K-cycles"):
        assert phrase not in header
    for phrase in ("more than one near-null vector", "filtering with a threshold of its own", "gmres / minres / multi-RHS wiring",
                   "NOT BUILT: update_values for a hierarchy"):
        assert phrase in header, phrase


def test_struct_sizes_and_offsets():
    import spmv_mi355x as E
    O, S = E.AmgProlongatorOpts, E.AmgProlongatorStats
    assert ctypes.sizeof(O) == 16 and (O.struct_size.offset, O.filtered.offset, O.near_null.offset) == (0, 4, 8)
    # unsigned + 2 ints (+ 4 of padding), 2 arrays of 16 longs, 2 of 16 doubles
    assert ctypes.sizeof(S) == 16 + 4 * 16 * 8
    assert (S.filtered.offset, S.has_near_null.offset, S.nnz_filtered.offset, S.unfiltered_rows.offset, S.omega_p.offset,
            S.rho_p.offset) == (4, 8, 16, 144, 272, 400)
    # the structs of amg_create keep their bytes
    assert ctypes.sizeof(E.AmgOpts) == 32 and ctypes.sizeof(E.AmgStats) == 16 + 7 * 16 * 8 + 80


# ---- the refusals that need no device, in their order -----------------------------------------------------------------------------------

def _create(E, n, rp, ci, va, fmt=SELL, precision=F64, opts=None, amg=None, prol=None, out=True):
    p = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
    keep = [None if a is None else np.ascontiguousarray(a, t) for a, t in ((rp, np.int32), (ci, np.int32), (va, np.float64))]
    h = ctypes.c_void_p(0x1234)
    o = None if opts is None else (E._make_opts(opts) if isinstance(opts, dict) else opts)
    a = None
    if amg is not None:
        a = amg if isinstance(amg, E.AmgOpts) else E.AmgOpts(ctypes.sizeof(E.AmgOpts), *[dict(ac.DEFAULTS, **amg)[k] for k in ac.DEFAULTS])
    q, nn = None, None
    if prol is not None:
        if isinstance(prol, E.AmgProlongatorOpts):
            q = prol
        else:
            nn = None if prol.get("near_null") is None else np.ascontiguousarray(prol["near_null"], np.float64)
            q = E.AmgProlongatorOpts(ctypes.sizeof(E.AmgProlongatorOpts), prol.get("filtered", 0), None if nn is None else nn.ctypes.data)
    rc = E.lib().spmv_mi355x_amg_create_with(ctypes.byref(h) if out else None, fmt, precision, ctypes.c_long(n), *[p(a_) for a_ in keep],
                                             None if a is None else ctypes.byref(a), None if q is None else ctypes.byref(q),
                                             None if o is None else ctypes.byref(o))
    return rc, h, E.lib().spmv_mi355x_last_error()


def _refused(E, phrases, *args, **kw):
    rc, h, msg = _create(E, *args, **kw)
    assert rc == 1 and msg.startswith(b"amg_create_with: ") and all(ph in msg for ph in phrases), msg
    assert not kw.get("out", True) or h.value is None, "the out handle is cleared"


def test_refusals_in_their_order():
    import spmv_mi355x as E
    bad_nn = dict(near_null=[1.0, 0.0, np.nan], filtered=1)               # refused after item 5 only
    # 1. the scalars of amg_create, under the new prefix, whatever the prolongator options hold
    _refused(E, (b"unknown precision 7",), 3, None, None, None, precision=7, prol=dict(filtered=5))
    _refused(E, (b"unknown format 9",), 3, None, None, None, fmt=9, prol=dict(filtered=5))
    _refused(E, (b"n = -1",), -1, None, None, None, prol=dict(filtered=5))
    _refused(E, (b"opts->struct_size",), 3, None, None, None, opts=E.Opts(), prol=dict(filtered=5))
    _refused(E, (b"amg_opts->struct_size",), 3, None, None, None, amg=E.AmgOpts(), prol=E.AmgProlongatorOpts())
    _refused(E, (b"transpose",), 3, None, None, None, opts=dict(transpose=1), prol=dict(filtered=5))
    for field, bad in (("theta", 1.5), ("max_levels", 17), ("coarse_rows", 0), ("sweeps", 5), ("coarse_sweeps", 65)):
        _refused(E, (b"amg_opts->" + field.encode(),), 3, None, None, None, amg={field: bad}, prol=E.AmgProlongatorOpts())
    # then the new scalars: struct_size before filtered, both before the NULL pointers
    _refused(E, (b"prolongator_opts->struct_size not set",), 3, None, None, None, prol=E.AmgProlongatorOpts(0, 5, None))
    for bad in (-1, 2):
        _refused(E, (f"prolongator_opts->filtered = {bad}".encode(),), 3, None, None, None, prol=dict(filtered=bad))
    # 2. to 5. as amg_create, before the near-null vector is read
    _refused(E, (b"NULL argument", b" out"), 3, BAD_RP, CI, VA, out=False, prol=bad_nn)
    _refused(E, (b"NULL argument", b" row_ptr"), 3, None, CI, VA, prol=bad_nn)
    _refused(E, (b"row_ptr is not monotone at row 1",), 3, BAD_RP, DUP_CI, NEG_VA, prol=bad_nn)
    _refused(E, (b"row 1 of A stores column 2 twice",), 3, RP, DUP_CI, NEG_VA, prol=bad_nn)
    _refused(E, (b"the diagonal of row 1 of A is -4",), 3, RP, CI, NEG_VA, prol=bad_nn)
    # the new item after 5: every near_null[i] finite and not 0, the first bad row is named
    _refused(E, (b"near_null[1] = 0",), 3, RP, CI, VA, prol=bad_nn)
    for bad in (0.0, -0.0, np.nan, np.inf, -np.inf):
        _refused(E, (b"near_null[2] = ",), 3, RP, CI, VA, prol=dict(near_null=[1.0, -2.0, bad]))
    # amg_create keeps its own prefix
    rc = E.lib().spmv_mi355x_amg_create(None, SELL, 7, ctypes.c_long(3), None, None, None, None, None)
    assert rc == 1 and E.lib().spmv_mi355x_last_error().startswith(b"amg_create: unknown precision 7")
    # the two queries without a handle
    s = E.AmgProlongatorStats()
    s.struct_size = ctypes.sizeof(s)
    assert E.lib().spmv_mi355x_amg_prolongator_info(None, ctypes.byref(s)) == 1
    assert E.lib().spmv_mi355x_last_error().startswith(b"amg_prolongator_info: NULL handle")
    assert E.lib().spmv_mi355x_amg_near_null(None, 0, None) == 1 and E.lib().spmv_mi355x_last_error().startswith(b"amg_near_null: NULL handle")


# ---- the reference against the restatement ----------------------------------------------------------------------------------------------

def _scipy(c, shape):
    return sp.csr_matrix((c[2].copy(), c[1].copy(), c[0].copy()), shape)     # scipy sorts unsorted rows in place


@pytest.mark.parametrize("name,variant", apc.CASES)
def test_the_reference_against_the_restatement(name, variant):
    ref, opts = apc.reference_of(name, variant), apc.options(name)
    rp, ci, va, n, _, nn, filtered = apc.case(name, variant)
    assert ref["bad"] is None and (ref["filtered"], ref["has_nn"]) == (filtered, nn is not None)
    if name == "path_wrap":
        assert [L["n"] for L in ref["lev"]] == apc.PATH_NN_ROWS and not ref["stalled"] and ref["lev"][-1]["n"] <= 128
    if name == "hub":
        assert ref["lev"][0]["unfiltered_rows"] >= 1, "row 0 must fall back, or the case shows nothing"
        F = ref["lev"][0]["AF"]
        assert F[0][1] - F[0][0] == apc.HUB_COUPLED + 3, "row 0 keeps all its entries"
    if name == "aniso" and filtered:
        assert np.all(np.diff(ref["lev"][0]["AF"][0]) < np.diff(ref["lev"][0]["A"][0])), "every level-0 row has weak entries to lump"
    if n and nn is not None:
        assert np.array_equal(ref["lev"][0]["b"], nn)
    for l, L in enumerate(ref["lev"]):
        if L["P"] is None:
            assert (L["AF"], L["nnz_f"], L["omega_p"], L["rho_p"], L["unfiltered_rows"], L["t"].size) == (None, 0, 0, 0, 0, 0)
            continue
        nl, nc = L["n"], L["aggregates"]
        A = _scipy(L["A"], (nl, nl))
        agg, _, rounds = ac.restated_aggregates(A, opts["theta"])
        assert np.array_equal(L["agg"], agg) and L["rounds"] == rounds
        want = apc.restated_level(A, agg, nc, opts["theta"], L["b"] if ref["has_nn"] else None, filtered)
        assert L["unfiltered_rows"] == want["unfiltered_rows"]
        assert abs(L["rho_p"] - want["rho_p"]) <= 1e-14 * want["rho_p"] and abs(L["omega_p"] - want["omega_p"]) <= 1e-14 * want["omega_p"]
        if filtered:
            F = _scipy(L["AF"], (nl, nl))
            assert L["nnz_f"] == len(L["AF"][1]) <= len(L["A"][1]) and abs(F - want["AF"]).max() <= CLOSE * abs(A).max()
            # A_F in A's stored order: the map ascends, names the same columns and, off the diagonal, the same values
            assert np.all(np.diff(L["map"])[np.diff(np.repeat(np.arange(nl), np.diff(L["AF"][0]))) == 0] > 0)
            assert np.array_equal(L["A"][1][L["map"]], L["AF"][1])
            off = L["AF"][1] != np.repeat(np.arange(nl), np.diff(L["AF"][0]))
            assert np.array_equal(L["A"][2][L["map"]][off], L["AF"][2][off])
            # lumping keeps the row sums of the rows that did not fall back
            assert np.abs(np.asarray((F - A).sum(axis=1)).ravel()).max() <= CLOSE * abs(A).max() * max(np.diff(L["A"][0]).max(), 1)
        else:
            assert L["AF"] is None and L["nnz_f"] == len(L["A"][1]) and (L["omega_p"], L["rho_p"]) == (L["omega"], L["rho"])
        if ref["has_nn"]:
            assert np.abs(L["t"] - want["t"]).max() <= CLOSE * np.abs(want["t"]).max()
            b_next = ref["lev"][l + 1]["b"]
            assert np.abs(b_next - want["b_next"]).max() <= CLOSE * want["b_next"].max()
            # T b_{l+1} = b_l: the near-null vector is reproduced level by level, and every column of T has norm 1
            assert np.abs(L["t"] * b_next[agg] - L["b"]).max() <= CLOSE * np.abs(L["b"]).max()
            assert np.abs(np.bincount(agg, L["t"] ** 2, nc) - 1).max() <= 1e-14
        got_p, got_a = _scipy(L["P"], (nl, nc)), _scipy(ref["lev"][l + 1]["A"], (nc, nc))
        assert abs(got_p - want["P"]).max() <= CLOSE * abs(want["P"]).max()
        assert abs(got_a - want["A_next"]).max() <= CLOSE * abs(want["A_next"]).max()
        assert abs(got_a - got_a.T).max() <= 1e-13 * abs(got_a).max(), "the coarse operators stay symmetric to rounding"


def test_defaults_are_the_hierarchy_of_amg_reference():
    """filtered = 0 and no near-null vector: the loops of tests/amg_reference.c, bit for bit"""
    for name in ("grid", "aniso", "n129", "one", "empty"):
        rp, ci, va, n, _ = ac.case(name)
        a, b = ac.reference_of(name), apc.reference(rp, ci, va, n, **ac.options(name))
        assert uc.equal_to_the_bit(a, b) is None and all(np.array_equal(K["agg"], L["agg"]) for K, L in zip(a["lev"], b["lev"]))


def test_the_update_loops_on_the_same_values_are_the_build():
    for name, variant in (("grid", "both"), ("aniso", "both"), ("hub", "both"), ("grid", "nn"), ("aniso", "filtered")):
        ref = apc.reference_of(name, variant)
        again = apc.reference_update(ref, apc.case(name, variant)[2])
        assert again["bad"] is None and apc.same_structure(ref, again) and apc.first_difference(ref, again) is None, (name, variant)
    # a scale by 0.7 keeps every decision of strength: the update is the build on the new values (the contract's first rule)
    for name in ("grid", "aniso"):
        rp, ci, va, n, _, nn, filtered = apc.case(name, "both")
        fresh = apc.reference(rp, ci, 0.7 * va, n, nn, filtered, **apc.options(name))
        upd = apc.reference_update(apc.reference_of(name, "both"), 0.7 * va)
        assert apc.same_structure(fresh, upd) and apc.first_difference(fresh, upd) is None, name


# ---- the recorded figures ---------------------------------------------------------------------------------------------------------------

def test_the_recorded_counts():
    _, hist, stop = apc.path_restatement()
    assert stop == 1 and hist.size == apc.PATH_NN_COUNT
    assert apc.PATH_NN_COUNT <= 38 == ac.PATH_COUNT // 2, "at most half of what the constant takes"
    for which, want in apc.GRID_SCALED_COUNTS.items():
        assert apc.grid_scaled_count(which) == want, which
    assert apc.GRID_SCALED_COUNTS["nn"] < apc.GRID_SCALED_COUNTS["default"]


def test_the_recorded_cycle_bounds():
    for dtype in (np.float64, np.float32):
        got = apc.measured_cycle_difference(dtype)
        print(f"[amg] cycle restatement {np.dtype(dtype).name} against the next wider type: {got:.3g}")
        assert 0.5 * apc.CYCLE_MEASURED[dtype] <= got <= apc.CYCLE_MEASURED[dtype]
        assert np.isclose(apc.CYCLE_BOUND[dtype], 10 * apc.CYCLE_MEASURED[dtype], rtol=1e-12, atol=0)


def test_the_cycle_is_symmetric_and_positive():
    """M^-1 of the restatement in fp64: u.M^-1 v = v.M^-1 u to rounding and u.M^-1 u > 0, which is what CG needs"""
    for name, variant in apc.CYCLE_CASES:
        M = apc.cycle_restatement(name, variant, np.float64)
        u, v = np.random.default_rng(3).normal(size=(2, apc.base(name)[3]))
        assert abs(u @ M(v) - v @ M(u)) <= 1e-12 * abs(u @ M(v)) + 1e-12 * np.linalg.norm(u) * np.linalg.norm(M(v)) and u @ M(u) > 0, (name, variant)
