"""CPU tier of the multicolour ordering (include/spmv_mi355x.h "multicolour ordering"): the symbols are exported, declared and bound;
the argument errors that fire before a device is touched come back as rc 1 in the documented order; and the yardstick of the GPU tier
is itself checked: the colouring of tests/color_reference.c is proper on A + A^t and first-fit tight for every case, an independent
numpy restatement of the SYNCHRONOUS ROUNDS gives the same colours and the same round counts as the sequential greedy loop, the numpy
permuted matrix is P A P^t, and the CG iteration counts the GPU tier compares with are recomputed here."""
import ctypes
import inspect
import os

import numpy as np
import pytest
import scipy.sparse as sp

import color_cases as cc
import pcg_tri_cases as pc
import trsv_cases as tc
from conftest import ROOT, has_gpu
from trsv_cases import LOWER, UPPER

P = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
NAMES = ("spmv_mi355x_color_create", "spmv_mi355x_color_destroy", "spmv_mi355x_color_info", "spmv_mi355x_color_colors",
         "spmv_mi355x_color_perm", "spmv_mi355x_color_color_ptr", "spmv_mi355x_color_mem_footprint", "spmv_mi355x_color_permute_csr",
         "spmv_mi355x_color_permute_csr_device", "spmv_mi355x_color_permute_values", "spmv_mi355x_color_permute_values_device_async",
         "spmv_mi355x_color_permute_vectors", "spmv_mi355x_color_permute_vectors_device_async")


def test_the_symbols_are_exported_declared_and_bound():
    import spmv_mi355x as E
    header = open(os.path.join(ROOT, "include", "spmv_mi355x.h")).read()
    for sym in NAMES:
        assert hasattr(E.lib(), sym) and sym in E.SYMBOLS and sym + "(" in header, sym
    assert list(inspect.signature(E.Coloring.__init__).parameters) == ["self", "row_ptr", "col_idx", "n", "device"]
    assert list(inspect.signature(E.multicolor_system).parameters)[:4] == ["row_ptr", "col_idx", "values", "n"]
    for name in ("info", "permute_csr", "permute_csr_device", "permute_values", "permute_values_device", "permute", "unpermute",
                 "permute_device", "unpermute_device", "close"):
        assert callable(getattr(E.Coloring, name)), name
    assert ctypes.sizeof(E.ColorStats) == ctypes.sizeof(ctypes.c_size_t) + 7 * ctypes.sizeof(ctypes.c_long) + 4 * ctypes.sizeof(ctypes.c_double)
    assert "enum { SPMV_MI355X_COLOR_FORWARD = 0, SPMV_MI355X_COLOR_BACKWARD = 1 };" in header
    assert (E.COLOR_FORWARD, E.COLOR_BACKWARD) == (0, 1)
    for phrase in ("NOT BUILT: distance-2 colouring; balancing the colour classes; fewer colours than greedy gives",
                   "a multicolour smoother inside the AMG cycle", "the blocked and the row-partitioned forms"):
        assert phrase in header, phrase


# ---- the reference is a proper, first-fit tight colouring ----------------------------------------------------------------------------

@pytest.mark.parametrize("name", cc.CASES)
def test_the_reference_colouring_is_proper_and_tight(name):
    rp, ci, va, n = cc.matrix(name)
    ref = cc.reference(name)
    col = ref["colors"].astype(np.int64)
    assert col.shape == (n,) and (n == 0 or (col.min() == 0 and col.max() == ref["num_colors"] - 1))
    S = cc.adjacency(rp, ci, n).tocoo()
    assert np.all(col[S.row] != col[S.col]), "two adjacent rows share a colour"
    # every vertex of colour c > 0 has a neighbour of every colour below c: c distinct lower colours among its neighbours
    low = col[S.col] < col[S.row]
    pairs = np.unique(np.stack([S.row[low], col[S.col][low]]), axis=1)
    assert np.array_equal(np.bincount(pairs[0], minlength=n)[:n], col)
    # the permutation sorts by (colour, row)
    perm, rank, ptr = ref["perm"], ref["rank"], ref["color_ptr"]
    assert np.array_equal(np.sort(perm), np.arange(n)) and np.array_equal(rank[perm], np.arange(n))
    assert np.all(np.diff(col[perm]) >= 0) and np.all(np.diff(perm)[np.diff(col[perm]) == 0] > 0)
    assert ptr[0] == 0 and ptr[-1] == n and len(ptr) == ref["num_colors"] + 1
    for c in range(ref["num_colors"]):
        assert np.all(col[perm[ptr[c]:ptr[c + 1]]] == c)


def test_the_cases_are_what_they_say():
    got = {name: (cc.reference(name)["num_colors"], cc.reference(name)["rounds"]) for name in cc.CASES}
    assert got["grid"] == got["unsorted"] == got["dup"] == (5, 6)
    assert got["clique70"] == (70, 70) and got["stencil27"] == (16, 21)
    assert got["one"] == (1, 1) and got["empty"] == (0, 0) and got["star"][0] == 2
    for name in ("unsorted", "dup"):
        assert np.array_equal(cc.reference(name)["colors"], cc.reference("grid")["colors"])
    rp, ci, va, n = cc.matrix("unsorted")
    assert np.any(np.diff(ci)[np.diff(np.repeat(np.arange(n), np.diff(rp))) == 0] < 0)
    rp, ci, va, n = cc.matrix("dup")
    assert ci[rp[100] + 1] == ci[rp[100] + 2]
    # oneway: the colouring of A's own rows alone (A^t not walked) is a different one, and not proper on A + A^t
    rp, ci, va, n = cc.matrix("oneway")
    A = sp.csr_matrix((np.ones(len(ci)), ci.copy(), rp.copy()), shape=(n, n))
    assert (A != A.T).nnz > 0
    A.setdiag(0)
    A.eliminate_zeros()
    rows, _ = synchronous_rounds(A.indptr, A.indices, n)
    S = cc.adjacency(rp, ci, n).tocoo()
    assert np.any(rows[S.row] == rows[S.col]) and not np.array_equal(rows, cc.reference("oneway")["colors"])
    rp, ci, va, n = cc.matrix("path_wrap")
    assert n > 256 * 1024


# ---- the synchronous rounds, restated ----------------------------------------------------------------------------------------------------

def synchronous_rounds(indptr, indices, n):
    """(colors, rounds) of the header's rounds over the neighbour lists given (no vertex lists itself): every round reads `col` and
    writes `new`; an uncoloured vertex whose key exceeds the key of all its uncoloured neighbours takes the smallest colour its coloured
    neighbours do not hold. Written with whole-array operations, with no loop over vertices in key order."""
    key = cc.keys(n).astype(np.int64)                          # below 2^62: int64 holds them
    col = np.full(n, -1, np.int64)
    deg = np.diff(indptr)
    src = np.repeat(np.arange(n), deg)
    rounds = 0
    while np.any(col < 0):
        rounds += 1
        assert rounds <= n
        open_nb = col[indices] < 0
        best = np.full(n, -1, np.int64)
        np.maximum.at(best, src[open_nb], key[indices][open_nb])
        win = (col < 0) & (key > best)
        taken = np.zeros((int(win.sum()), int(col.max()) + 3), bool)
        slot = np.cumsum(win) - 1
        e = win[src] & ~open_nb
        taken[slot[src[e]], col[indices[e]]] = True
        new = col.copy()
        new[win] = np.argmin(taken, axis=1)                    # the first colour not taken
        col = new
    return col.astype(np.int32), rounds


@pytest.mark.parametrize("name", cc.CASES)
def test_the_synchronous_rounds_give_the_greedy_colouring_and_its_rounds(name):
    rp, ci, va, n = cc.matrix(name)
    S = cc.adjacency(rp, ci, n)
    col, rounds = synchronous_rounds(S.indptr, S.indices, n)
    ref = cc.reference(name)
    assert np.array_equal(col, ref["colors"]) and rounds == ref["rounds"]


# ---- the permuted matrix, restated ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", [c for c in cc.CASES if c not in ("path_wrap",)])
def test_the_restated_permuted_matrix_is_p_a_pt(name):
    rp, ci, va, n = cc.matrix(name)
    ref = cc.reference(name)
    rp_b, ci_b, va_b, emap = cc.permuted(name)
    assert np.array_equal(va_b, va[emap]) and np.array_equal(np.sort(emap), np.arange(len(ci)))
    rows_b = np.repeat(np.arange(n), np.diff(rp_b))
    assert np.all(np.diff(ci_b)[np.diff(rows_b) == 0] >= 0), "columns ascend in every row"
    same = (np.diff(rows_b) == 0) & (np.diff(ci_b) == 0)
    assert np.all(np.diff(emap)[same] > 0), "equal columns keep their stored order"
    A = sp.csr_matrix((va, ci, rp), shape=(n, n))
    B = sp.csr_matrix((va_b, ci_b, rp_b), shape=(n, n))
    perm = ref["perm"]
    if n:
        assert (B != A[perm][:, perm]).nnz == 0
    if name in ("grid", "stencil27"):
        # the point of it all: the level schedule of B's triangles is the colouring
        assert int(tc.levels_of(rp_b, ci_b, n, LOWER).max()) + 1 == ref["num_colors"]
        assert np.array_equal(tc.levels_of(rp_b, ci_b, n, LOWER), ref["colors"][perm])
        assert int(tc.levels_of(rp_b, ci_b, n, UPPER).max()) + 1 <= ref["num_colors"]
    if name == "grid":
        assert int(tc.levels_of(rp, ci, n, LOWER).max()) + 1 == 89


# ---- the iteration counts of the GPU tier --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_the_iteration_counts_under_the_multicolour_preconditioners(dtype):
    Q = cc.problem()
    tol = pc.PREC[dtype]["tol"]
    want = np.linalg.solve(Q.D, Q.b)
    assert np.allclose(want[Q.rank], pc.problem().solve(), rtol=1e-10, atol=0), "B (P x) = P b"
    for kind in ("sgs", "ic0"):
        x, hist, stop = Q.restatement(dtype, kind, tol)
        assert stop == 1 and len(hist) == cc.COUNTS[dtype][kind], (kind, len(hist))
        assert np.linalg.norm(x - want) <= pc.KAPPA * 10 * tol * np.linalg.norm(want)
    # weaker per iteration than the natural ordering's, stronger than Jacobi
    assert pc.COUNTS[dtype]["sgs"] < cc.COUNTS[dtype]["sgs"] < pc.COUNTS[dtype]["jacobi"]
    assert pc.COUNTS[dtype]["ic0"] < cc.COUNTS[dtype]["ic0"] < pc.COUNTS[dtype]["jacobi"]


# ---- refusals before a device is touched ---------------------------------------------------------------------------------------------------

def good():
    return np.array([0, 2, 5, 7], np.int32), np.array([0, 1, 0, 1, 2, 1, 2], np.int32)


def create(n=3, rp="good", ci="good", out="good", device=-1):
    import spmv_mi355x as E
    g = good()
    rp, ci = (g[k] if isinstance(a, str) else a for k, a in enumerate((rp, ci)))
    h = ctypes.c_void_p()
    rc = E.lib().spmv_mi355x_color_create(ctypes.byref(h) if out is not None else None, ctypes.c_long(n), P(rp), P(ci), device)
    msg = E.lib().spmv_mi355x_last_error().decode()
    if rc == 0:
        E.lib().spmv_mi355x_color_destroy(h)
    return rc, msg


BAD_RP, BAD_CI = np.array([0, 2, 1, 7], np.int32), np.array([0, 1, 0, 3, 2, 1, 2], np.int32)
ERRORS = [
    (1, "n_negative", dict(n=-1), "n = -1 out of range"),
    (2, "null_out", dict(out=None), "NULL argument ( out"),
    (2, "null_row_ptr", dict(rp=None), "NULL argument ( row_ptr"),
    (2, "null_col_idx", dict(ci=None), "NULL argument ( col_idx"),
    (3, "row_ptr_not_from_0", dict(rp=np.array([1, 2, 5, 7], np.int32)), "row_ptr must start at 0"),
    (3, "row_ptr_not_monotone", dict(rp=BAD_RP), "row_ptr is not monotone at row 1"),
    (3, "column_out_of_range", dict(ci=BAD_CI), "column index 3 out of range [0,3) at entry 3"),
    (3, "column_negative", dict(ci=np.array([0, 1, 0, 1, 2, -1, 2], np.int32)), "column index -1 out of range [0,3) at entry 5"),
]
BEHIND = {1: (dict(out=None), dict(rp=BAD_RP)), 2: (dict(rp=BAD_RP), dict(ci=BAD_CI)), 3: (dict(device=99),)}


@pytest.mark.parametrize("step,case,args,phrase", ERRORS, ids=[e[1] for e in ERRORS])
def test_create_errors_in_their_documented_order(step, case, args, phrase):
    rc, msg = create(**args)
    assert rc == 1
    assert msg.startswith("color_create: ") and phrase in msg, msg
    for behind in BEHIND[step]:
        if not set(behind) & set(args):
            rc, msg = create(**args, **behind)
            assert rc == 1 and msg.startswith("color_create: ") and phrase in msg, (behind, msg)


def test_the_device_comes_last():
    """a valid pattern (unsorted rows, duplicates and a missing diagonal are legal) and n = 0: without a GPU the library's no-device
    message, named as color_create's; with one a handle"""
    for args in (dict(), dict(ci=np.array([1, 0, 2, 1, 1, 2, 1], np.int32)), dict(n=0, rp=np.zeros(1, np.int32), ci=None)):
        rc, msg = create(**args)
        if has_gpu():
            assert rc == 0, msg
        else:
            assert rc == 1
            assert msg.startswith("color_create: no HIP device available: this engine has no CPU fallback"), msg


def test_the_entries_that_take_a_handle_refuse_null():
    import spmv_mi355x as E
    L = E.lib()
    ints, values, out, ptr = np.full(7, 5, np.int32), np.ones(7), np.full(7, 2.0), ctypes.c_void_p(5)
    stats = E.ColorStats()
    stats.struct_size = ctypes.sizeof(E.ColorStats)
    stats.rounds = -7
    vec = lambda *a: L.spmv_mi355x_color_permute_vectors(None, *a)
    for call, prefix in ((lambda: L.spmv_mi355x_color_info(None, ctypes.byref(stats)), b"color_info: "),
                         (lambda: L.spmv_mi355x_color_colors(None, P(ints)), b"color_colors: "),
                         (lambda: L.spmv_mi355x_color_perm(None, P(ints), P(ints)), b"color_perm: "),
                         (lambda: L.spmv_mi355x_color_color_ptr(None, P(ints)), b"color_color_ptr: "),
                         (lambda: L.spmv_mi355x_color_permute_csr(None, P(values), P(ints), P(ints), P(out), P(ints)), b"color_permute_csr: "),
                         (lambda: L.spmv_mi355x_color_permute_csr_device(None, ctypes.byref(ptr), ctypes.byref(ptr), ctypes.byref(ptr)),
                          b"color_permute_csr: "),
                         (lambda: L.spmv_mi355x_color_permute_values(None, P(values), P(out)), b"color_permute_values: "),
                         (lambda: L.spmv_mi355x_color_permute_values_device_async(None, P(values), P(out), None), b"color_permute_values: "),
                         (lambda: vec(0, 0, 1, P(values), 1, P(out), 1), b"color_permute_vectors: "),
                         (lambda: L.spmv_mi355x_color_permute_vectors_device_async(None, 1, 1, 2, P(values), 2, P(out), 3, None),
                          b"color_permute_vectors: ")):
        assert call() == 1
        msg = L.spmv_mi355x_last_error()
        assert msg.startswith(prefix) and b"NULL argument ( C" in msg, msg
    # the scalars of permute_vectors come before the handle: direction, precision, then k and the leading dimensions
    for args, phrase in (((2, 0, 1, P(values), 1, P(out), 1), b"direction must be 0 (forward) or 1 (backward) (got 2)"),
                         ((2, 7, 0, P(values), 1, P(out), 1), b"direction must be"),
                         ((0, 2, 1, P(values), 1, P(out), 1), b"precision must be 0 (fp64) or 1 (fp32) (got 2)"),
                         ((0, 2, 0, P(values), 1, P(out), 1), b"precision must be"),
                         ((0, 0, 0, P(values), 1, P(out), 1), b"need k >= 1, ldin >= k and ldout >= k (got k=0 ldin=1 ldout=1)"),
                         ((1, 1, 3, P(values), 2, P(out), 3), b"need k >= 1, ldin >= k and ldout >= k (got k=3 ldin=2 ldout=3)"),
                         ((1, 1, 3, P(values), 3, P(out), 2), b"need k >= 1, ldin >= k and ldout >= k (got k=3 ldin=3 ldout=2)")):
        assert vec(*args) == 1
        msg = L.spmv_mi355x_last_error()
        assert msg.startswith(b"color_permute_vectors: ") and phrase in msg, msg
    stats.struct_size = 0
    assert L.spmv_mi355x_color_info(None, ctypes.byref(stats)) == 1 and b"NULL argument ( C" in L.spmv_mi355x_last_error()
    assert np.all(ints == 5) and np.all(values == 1) and np.all(out == 2) and ptr.value == 5 and stats.rounds == -7
    assert L.spmv_mi355x_color_destroy(None) == 0
    assert L.spmv_mi355x_color_mem_footprint(None) == 0.0
