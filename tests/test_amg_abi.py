"""CPU tier of the smoothed-aggregation AMG (include/spmv_mi355x.h "AMG"): the symbols are exported, declared and bound; the structs
have the sizes and defaults of the header; every refusal of spmv_mi355x_amg_create that needs no device comes back in the header's
order (each case also carries the errors of LATER steps, which must not be the ones reported); and the references the GPU tier
compares against are themselves checked here: tests/amg_reference.c against the scipy restatement level by level (the aggregates
equal, P and the coarse operator close, every aggregate connected in S, the roots pairwise more than 2 apart), its dense factor and
solve against numpy, and the recorded CG counts and cycle bounds of amg_cases.py recomputed.

The restatement is given the reference's own A_l on every level: on `aniso` the coarse operator has entries that are equal in exact
arithmetic, so pass 2's "largest |a_ij|" is decided by the last bit and two correct products P^t A P may aggregate differently."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.csgraph

import amg_cases as ac
import pcg_tri_cases as pc
from conftest import ROOT

AMG_SYMBOLS = ["spmv_mi355x_amg_create", "spmv_mi355x_amg_destroy", "spmv_mi355x_amg_apply_device_async", "spmv_mi355x_amg_apply",
               "spmv_mi355x_amg_info", "spmv_mi355x_amg_level_matrices", "spmv_mi355x_amg_aggregates", "spmv_mi355x_amg_level_csr",
               "spmv_mi355x_amg_mem_footprint", "spmv_mi355x_pcg_amg"]
SELL, F64 = 3, 0
CLOSE = 1e-14                 # P and A_{l+1} against scipy's products, relative to the largest entry: a few roundings of fp64


def test_the_symbols_are_exported_declared_and_bound():
    import spmv_mi355x as E
    header = open(os.path.join(ROOT, "include", "spmv_mi355x.h")).read()
    for sym in AMG_SYMBOLS:
        assert hasattr(E.lib(), sym) and sym in E.SYMBOLS and sym + "(" in header, sym
    assert list(inspect.signature(E.Amg.__init__).parameters) == ["self", "row_ptr", "col_idx", "values", "n", "fmt", "dtype", "theta",
                                                                  "max_levels", "coarse_rows", "sweeps", "coarse_sweeps", "opts"]
    for name in ("info", "apply", "aggregates", "level_csr", "level_matrices", "close"):
        assert callable(getattr(E.Amg, name))
    for phrase in ("NOT CHECKABLE: that A is symmetric and positive definite", "NOT BUILT: update_values for a hierarchy"):
        assert phrase in header


def test_struct_sizes_and_defaults():
    import spmv_mi355x as E
    header = open(os.path.join(ROOT, "include", "spmv_mi355x.h")).read()
    assert ctypes.sizeof(E.AmgOpts) == 32 and E.AmgOpts.theta.offset == 8 and E.AmgOpts.coarse_sweeps.offset == 28
    assert "#define SPMV_MI355X_AMG_MAX_LEVELS 16" in header and E.AMG_MAX_LEVELS == 16
    # unsigned + 3 ints, 5 arrays of 16 longs, 2 of 16 doubles, 2 doubles, 2 longs, 6 doubles
    assert ctypes.sizeof(E.AmgStats) == 16 + 7 * 16 * 8 + 10 * 8 and E.AmgStats.rows.offset == 16
    assert E.AMG_DEFAULTS == ac.DEFAULTS == dict(theta=0.08, max_levels=10, coarse_rows=128, sweeps=1, coarse_sweeps=4)
    sig = inspect.signature(E.Amg.__init__).parameters
    assert {k: sig[k].default for k in ac.DEFAULTS} == ac.DEFAULTS
    for field, default, lo, hi in (("max_levels", 10, 1, 16), ("coarse_rows", 128, 1, 128), ("sweeps", 1, 1, 4), ("coarse_sweeps", 4, 1, 64)):
        assert re.search(rf"{field};\s*/\* .*default {default}, {lo}\.\.{hi}", header), field
    assert re.search(r"theta;\s*/\* .*default 0\.08", header)


# ---- the refusals that need no device, in their order -----------------------------------------------------------------------------

def _create(E, n, rp, ci, va, fmt=SELL, precision=F64, opts=None, amg=None, out=True):
    p = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
    keep = [None if a is None else np.ascontiguousarray(a, t) for a, t in ((rp, np.int32), (ci, np.int32), (va, np.float64))]
    h = ctypes.c_void_p(0x1234)
    o = None
    if opts is not None:
        o = E._make_opts(opts) if isinstance(opts, dict) else opts
    a = None
    if amg is not None:
        a = amg if isinstance(amg, E.AmgOpts) else E.AmgOpts(ctypes.sizeof(E.AmgOpts), *[dict(ac.DEFAULTS, **amg)[k] for k in ac.DEFAULTS])
    rc = E.lib().spmv_mi355x_amg_create(ctypes.byref(h) if out else None, fmt, precision, ctypes.c_long(n), *[p(a_) for a_ in keep],
                                        None if a is None else ctypes.byref(a), None if o is None else ctypes.byref(o))
    return rc, h, E.lib().spmv_mi355x_last_error()


def _refused(E, phrases, *args, **kw):
    rc, h, msg = _create(E, *args, **kw)
    assert rc == 1 and msg.startswith(b"amg_create: ") and all(ph in msg for ph in phrases), msg
    assert not kw.get("out", True) or h.value is None, "the out handle is cleared"


# a good 3 x 3 matrix, and what is wrong with it from step 3 on
RP, CI, VA = [0, 2, 5, 7], [0, 1, 0, 1, 2, 1, 2], [4.0, -1.0, -1.0, 4.0, -1.0, -1.0, 4.0]
BAD_RP = [0, 2, 1, 7]                                     # 3. not monotone
DUP_CI = [0, 1, 0, 2, 2, 1, 2]                            # 4. row 1 stores column 2 twice (and no diagonal: 5.)
NEG_VA = [4.0, -1.0, -1.0, -4.0, -1.0, -1.0, 4.0]         # 5. the diagonal of row 1 is negative


def test_refusals_in_their_order():
    import spmv_mi355x as E
    # 1. the scalars, whatever else is wrong (NULL arrays: step 2)
    _refused(E, (b"unknown precision 7",), 3, None, None, None, precision=7)
    _refused(E, (b"unknown format 9",), 3, None, None, None, fmt=9)
    _refused(E, (b"n = -1",), -1, None, None, None)
    _refused(E, (b"n = 2147483647",), 2 ** 31 - 1, None, None, None)
    _refused(E, (b"opts->struct_size",), 3, None, None, None, opts=E.Opts())
    _refused(E, (b"amg_opts->struct_size",), 3, None, None, None, amg=E.AmgOpts())
    _refused(E, (b"transpose",), 3, None, None, None, opts=dict(transpose=1))
    _refused(E, (b"symmetric_input",), 3, None, None, None, opts=dict(symmetric_input=1))
    _refused(E, (b"row block", b"row_end 2"), 3, None, None, None, opts=dict(row_begin=0, row_end=2))
    _refused(E, (b"value_storage",), 3, None, None, None, fmt=1, opts=dict(value_storage=1))
    # the options of the hierarchy, each on its own, both ends of every range
    for field, bad in (("theta", -0.01), ("theta", 1.5), ("theta", float("nan")), ("theta", float("inf")), ("max_levels", 0),
                       ("max_levels", 17), ("coarse_rows", 0), ("coarse_rows", 129), ("sweeps", 0), ("sweeps", 5), ("coarse_sweeps", 0),
                       ("coarse_sweeps", 65)):
        _refused(E, (b"amg_opts->" + field.encode(),), 3, None, None, None, amg={field: bad})
    # the first bad one is named
    _refused(E, (b"amg_opts->max_levels = 0",), 3, None, None, None, amg=dict(max_levels=0, sweeps=9))
    # 2. NULL pointers, before the pattern of A is read
    _refused(E, (b"NULL argument", b" out"), 3, BAD_RP, CI, VA, out=False)
    _refused(E, (b"NULL argument", b" row_ptr"), 3, None, CI, VA)
    _refused(E, (b"NULL argument", b" col_idx"), 3, RP, None, VA)
    _refused(E, (b"NULL argument", b" values"), 3, RP, CI, None)
    # 3. A's pattern, before its duplicates and the diagonal
    _refused(E, (b"row_ptr is not monotone at row 1",), 3, BAD_RP, DUP_CI, NEG_VA)
    _refused(E, (b"row_ptr must start at 0",), 3, [1, 2, 5, 7], DUP_CI, NEG_VA)
    _refused(E, (b"column index 3 out of range [0,3) at entry 4",), 3, RP, [0, 1, 0, 2, 3, 1, 2], NEG_VA)
    _refused(E, (b"column index -1 out of range",), 3, RP, [0, 1, 0, 2, -1, 1, 2], NEG_VA)
    # 4. a column twice in a row, in either triangle, before the diagonal
    _refused(E, (b"row 1 of A stores column 2 twice",), 3, RP, DUP_CI, NEG_VA)
    _refused(E, (b"row 2 of A stores column 1 twice",), 3, RP, [0, 1, 0, 1, 2, 1, 1], NEG_VA)
    # 5. the diagonal: missing, not positive, not finite; the first bad row is named
    _refused(E, (b"the diagonal of row 1 of A is -4",), 3, RP, CI, NEG_VA)
    _refused(E, (b"row 0 of A has no diagonal entry",), 3, RP, [1, 2, 0, 1, 2, 1, 2], NEG_VA)
    for bad in (0.0, -2.0, np.nan, np.inf):
        _refused(E, (b"the diagonal of row 2 of A",), 3, RP, CI, VA[:6] + [bad])


def test_pcg_amg_refusals_that_need_no_handle():
    """items 1 to 4 of pcg_tri with the prefix pcg_amg, before M is looked at: a NULL M with a NULL A is A's refusal (M == NULL under a
    handle of A is in the GPU tier)"""
    import spmv_mi355x as E
    b, x = np.full(4, 3.5), np.full(4, -7.25)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    info = E.PcgTriInfo()
    for size, tol, maxit, phrase in ((4, 1e-12, 10, b"struct_size"), (None, -1.0, 10, b"tol"), (None, float("nan"), 10, b"tol"),
                                     (None, 1e-12, -1, b"max_iterations"), (None, 1e-12, 10, b"NULL argument ( A")):
        info.struct_size = ctypes.sizeof(E.PcgTriInfo) if size is None else size
        rc = E.lib().spmv_mi355x_pcg_amg(None, p(b), p(x), None, tol, maxit, None, ctypes.byref(info))
        msg = E.lib().spmv_mi355x_last_error()
        assert rc == 1 and msg.startswith(b"pcg_amg: ") and phrase in msg, msg
    assert np.all(b == 3.5) and np.all(x == -7.25)


# ---- the reference against the restatement ------------------------------------------------------------------------------------------------

def _scipy(c, shape):
    return sp.csr_matrix((c[2].copy(), c[1].copy(), c[0].copy()), shape)     # scipy sorts unsorted rows in place


SHAPES = {"grid": [2025, 382, 43], "unsorted": [2025, 382, 43], "grid_weak": [2025], "aniso": [1600, 402, 120], "isolated": [400, 122],
          "n128": [128], "n129": [129, 18], "one": [1], "empty": [], "path_wrap": [ac.PATH_ROWS, 61893, 14612, 3450, 1055, 272]}


@pytest.mark.parametrize("name", ac.CASES)
def test_the_reference_against_the_restatement(name):
    ref, opts = ac.reference_of(name), ac.options(name)
    assert [L["n"] for L in ref["lev"]] == SHAPES[name] and ref["levels"] == len(SHAPES[name])
    assert ref["stalled"] == (name in ("grid_weak", "path_wrap"))
    if name == "grid_weak":
        assert ref["lev"][0]["aggregates"] == 2025 and np.array_equal(ref["lev"][0]["agg"], np.arange(2025))
    for l, L in enumerate(ref["lev"]):
        n = L["n"]
        A = _scipy(L["A"], (n, n))
        rho = float((np.asarray(abs(A).sum(axis=1)).ravel() / A.diagonal()).max())
        assert abs(L["rho"] - rho) <= 1e-14 * rho and abs(L["omega"] - 4 / (3 * rho)) <= 1e-14 * L["omega"] and L["omega"] < 2 / rho
        assert abs(A - A.T).max() <= 1e-13 * abs(A).max(), "the coarse operators stay symmetric to rounding"
        coarsened = l < ref["levels"] - 1 or ref["stalled"]
        assert (L["rounds"] > 0) == coarsened and L["agg"].shape == ((n,) if coarsened else (0,))
        if not coarsened:
            continue
        agg, roots, rounds = ac.restated_aggregates(A, opts["theta"])
        assert np.array_equal(L["agg"], agg) and L["rounds"] == rounds and L["aggregates"] == int(roots.sum()) == agg.max() + 1
        # the roots are pairwise more than 2 apart in S, and every aggregate is connected in S
        rows, cols, _ = ac.strong_edges(A, opts["theta"])
        S = sp.csr_matrix((np.ones(len(rows)), (rows, cols)), (n, n))
        S2 = (S + S @ S).tocsr()[roots][:, roots].tocoo()
        assert np.all(S2.row == S2.col), f"{name}: level {l}: two roots within distance 2"
        inside = agg[rows] == agg[cols]
        parts, _ = scipy.sparse.csgraph.connected_components(sp.csr_matrix((np.ones(int(inside.sum())), (rows[inside], cols[inside])),
                                                                           (n, n)), directed=False)
        assert parts == L["aggregates"], f"{name}: level {l}: {parts} connected pieces for {L['aggregates']} aggregates"
        if L["P"] is None:
            continue
        nc = L["aggregates"]
        T = sp.csr_matrix((np.ones(n), (np.arange(n), agg)), (n, nc))
        P = (T - sp.diags(L["omega"] / A.diagonal()) @ (A @ T)).tocsr()
        got_p, got_a = _scipy(L["P"], (n, nc)), _scipy(ref["lev"][l + 1]["A"], (nc, nc))
        assert np.all(np.diff(L["P"][1])[np.diff(np.repeat(np.arange(n), np.diff(L["P"][0]))) == 0] > 0), "P's columns ascend"
        assert abs(got_p - P).max() <= CLOSE * abs(P).max()
        want_a = (P.T @ A @ P).tocsr()
        assert abs(got_a - want_a).max() <= CLOSE * abs(want_a).max()
        # T 1 = 1: the constant is reproduced, P 1 = 1 - omega D^-1 A 1
        assert np.array_equal(T @ np.ones(nc), np.ones(n))


def test_unsorted_rows_give_the_same_aggregates():
    a, b = ac.reference_of("grid"), ac.reference_of("unsorted")
    for L, K in zip(a["lev"], b["lev"]):
        assert np.array_equal(L["agg"], K["agg"]) and L["n"] == K["n"]
        assert np.array_equal(L["A"][0], K["A"][0]) and (L["P"] is None or np.array_equal(L["P"][1], K["P"][1]))


@pytest.mark.parametrize("name", ("n128", "grid", "one"))
def test_the_dense_factor_and_solve(name):
    L = ac.reference_of(name)["lev"][-1]
    n = L["n"]
    assert n <= 128
    F = ac.reference_factor(*L["A"], n)
    D = _scipy(L["A"], (n, n)).toarray()
    C = np.zeros((n, n))
    C[np.tril_indices(n)] = F[:n * (n + 1) // 2]
    assert np.allclose(C, np.linalg.cholesky(D), rtol=1e-12, atol=0)
    for v in ac.vectors(n):
        x = ac.reference_dense_solve(F, v)
        want = np.linalg.solve(D, v)
        assert np.abs(x - want).max() <= 1e-12 * np.abs(want).max()
    # a pivot that is not positive abandons the factor
    assert ac.reference_factor([0, 2, 4], [0, 1, 0, 1], [1.0, 2.0, 2.0, 1.0], 2) is None


# ---- the recorded figures ------------------------------------------------------------------------------------------------------------------

def test_the_recorded_counts():
    for dtype, lim in pc.PREC.items():
        for name, want in ac.COUNTS[dtype].items():
            _, hist, stop = ac.grid_restatement(name, dtype, lim["tol"])
            assert stop == 1 and hist.size == want, (np.dtype(dtype).name, name, hist.size)
        # the condition of the issue: below IC(0), the best one-level count
        assert ac.COUNTS[dtype]["grid"] < pc.COUNTS[dtype]["ic0"]
    assert ac.COUNTS[np.float64]["grid"] < 34
    _, hist, stop = ac.path_restatement()
    assert stop == 1 and hist.size == ac.PATH_COUNT


def test_the_recorded_cycle_bounds():
    for dtype in (np.float64, np.float32):
        got = ac.measured_cycle_difference(dtype)
        print(f"[amg] cycle restatement {np.dtype(dtype).name} against the next wider type: {got:.3g}")
        assert 0.5 * ac.CYCLE_MEASURED[dtype] <= got <= ac.CYCLE_MEASURED[dtype]
        assert np.isclose(ac.CYCLE_BOUND[dtype], 10 * ac.CYCLE_MEASURED[dtype], rtol=1e-12, atol=0)


def test_the_cycle_is_symmetric_and_positive():
    """M^-1 of the restatement in fp64: u.M^-1 v = v.M^-1 u to rounding and u.M^-1 u > 0, which is what CG needs"""
    for name in ("grid", "grid_nu2", "grid_weak", "aniso", "isolated"):
        M = ac.cycle_restatement(name, np.float64)
        u, v = np.random.default_rng(3).normal(size=(2, ac.case(name)[3]))
        assert abs(u @ M(v) - v @ M(u)) <= 1e-12 * abs(u @ M(v)) + 1e-12 * np.linalg.norm(u) * np.linalg.norm(M(v)) and u @ M(u) > 0, name
