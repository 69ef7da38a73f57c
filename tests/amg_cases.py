"""What the two tiers of the AMG tests share (test_amg_abi.py on the CPU, test_gpu_amg.py on the GPU): the cases, the C reference of
tests/amg_reference.c (the header's hierarchy as sequential loops, gcc -O2 -ffp-contract=off), a scipy restatement of the hierarchy
with arithmetic of its own (np.maximum.at for the independent set, a lexsort for the aggregates, P = T - diag(omega / d) (A T) and
P^t A P by scipy's products), the restatement of the cycle in a dtype of choice, and the CG counts through pcg_tri_cases.restate.
Nothing here touches the engine. Everything is computed once and is read-only.

A case is (row_ptr, col_idx, values, n, opts) with opts the options that differ from DEFAULTS.

THE SIZE OF path_wrap. Every setup kernel of csrc/kernels_amg.hip is one lane per row, 256 lanes per workgroup and at most 1024
workgroups per launch (AMG_TB, AMG_MAX_GRID of csrc/amg.hpp); the cycle's vector kernels take solver_blocks() workgroups of 256 lanes,
at most 1024 as well. The largest first trip of any of them covers 256 * 1024 = 262 144 rows, so n = 262 144 + 37 sends the first
workgroup of every one of them into a second trip of its row loop on level 0.

The counts of pcg_tri_cases.restate on pcg_tri_cases.problem() (spd_grid(45), n = 2025) with M^-1 = one V(nu, nu) cycle of the
hierarchy of the C reference, tol 1e-12 in fp64 and 1e-5 in fp32 (COUNTS; recomputed in test_amg_abi.py), against 122 / 53 without a
preconditioner and 34 / 15 with IC(0), the best one-level count of pcg_tri_cases.COUNTS:

      hierarchy                         fp64   fp32
      grid, nu = 1                        20      9
      grid, nu = 2                        14      6
      grid_weak (one level, 4 sweeps)     52     23
and 76 for path_wrap at tol 1e-8 in fp64 (PATH_COUNT). path_wrap is 262 181 -> 61 893 -> 14 612 -> 3 450 -> 1 055 -> 272 rows and
stalls there (272 aggregates of 272 rows), so its last level takes the sweeps. The symmetric scaling S A S moves the near-null
vector of the path from the constant to S^-1 1, which the un-normalised tentative prolongator does not carry: row sums over the
diagonal grow from 0.1 on level 1 to 0.8 on level 3, the coarse operators turn diagonally dominant and nothing is strong on level 5.
The unscaled path of 20 000 rows (5 levels, a dense last one) takes 25 iterations to 1e-8 and 36 to 1e-12 with the same options;
near-null vectors other than the constant are not built.

THE BOUND OF THE CYCLE (CYCLE_MEASURED, CYCLE_BOUND; recomputed in test_amg_abi.py). The engine's SpMVs sum a row in another order
than scipy's, so apply(v) is compared with the restatement within ten times what the restatement itself moves by when its arithmetic
changes: for an fp64 handle the largest max-norm relative difference, over CYCLE_CASES and the vectors of vectors(), between the
restatement in fp64 and in np.longdouble (measured 8.54e-16), for an fp32 handle between the restatement in fp32 and in fp64
(measured 3.48e-7). CYCLE_MEASURED holds these rounded up to two digits, CYCLE_BOUND ten times that."""
import ctypes
import functools
import os
import subprocess
import tempfile

import numpy as np
import scipy.linalg
import scipy.sparse as sp

import fsai_cases as fc
import pcg_tri_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULTS = dict(theta=0.08, max_levels=10, coarse_rows=128, sweeps=1, coarse_sweeps=4)
SETUP_TB, SETUP_MAX_GRID = 256, 1024
PATH_ROWS = SETUP_TB * SETUP_MAX_GRID + 37
CASES = ("grid", "grid_weak", "aniso", "path_wrap", "isolated", "unsorted", "n128", "n129", "one", "empty")
CYCLE_CASES = ("grid", "grid_weak", "aniso", "isolated", "n128", "n129", "one")
COUNTS = {np.float64: {"grid": 20, "grid_nu2": 14, "grid_weak": 52}, np.float32: {"grid": 9, "grid_nu2": 6, "grid_weak": 23}}
PATH_COUNT, PATH_TOL = 76, 1e-8
CYCLE_MEASURED = {np.float64: 8.6e-16, np.float32: 3.5e-7}
CYCLE_BOUND = {np.float64: 8.6e-15, np.float32: 3.5e-6}


def _freeze(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def _csr(A):
    A = A.tocsr()
    A.sort_indices()
    return _freeze(A.indptr.astype(np.int32), A.indices.astype(np.int32), A.data.astype(np.float64))


@functools.lru_cache(maxsize=None)
def case(name):
    """(row_ptr, col_idx, values, n, opts) by name"""
    if name in ("grid", "grid_weak", "grid_nu2"):
        rp, ci, va, n, _ = pc.spd_grid(45)
        return rp, ci, va, n, {"grid": {}, "grid_weak": dict(theta=0.25), "grid_nu2": dict(sweeps=2)}[name]
    if name == "unsorted":
        rp, ci, va, n, _ = pc.spd_grid(45)
        return _freeze(*fc.shuffled_rows(rp, ci, va)) + (n, {})
    if name == "aniso":
        # coupling 1 along x and 0.01 along y: a_ij^2 / (d_i d_j) is 0.24 along x and 2.4e-5 along y, against theta^2 = 0.0064
        k, e = 40, 0.01
        I, E = sp.identity(k), sp.diags([-np.ones(k - 1), -np.ones(k - 1)], [-1, 1])
        return _csr(sp.kron(I, E) + e * sp.kron(E, I) + (2 + 2 * e + 0.01) * sp.identity(k * k)) + (k * k, {})
    if name == "isolated":
        # a 20 x 20 grid whose every 7th row keeps its diagonal only (and its column likewise)
        k = 20
        I, E = sp.identity(k), sp.diags([-np.ones(k - 1), -np.ones(k - 1)], [-1, 1])
        A = (sp.kron(I, E) + sp.kron(E, I) + 4.05 * sp.identity(k * k)).tocoo()
        keep = (A.row == A.col) | ((A.row % 7 != 0) & (A.col % 7 != 0))
        return _csr(sp.csr_matrix((A.data[keep], (A.row[keep], A.col[keep])), (k * k, k * k))) + (k * k, {})
    if name in ("n128", "n129"):
        n = int(name[1:])
        return _freeze(*fc._csr_of_dense(fc.banded(n, 3))) + (n, {})
    if name == "path_wrap":
        n = PATH_ROWS
        s = 1 + 0.2 * np.random.default_rng(2).uniform(-1, 1, n)
        A = sp.diags([-np.ones(n - 1), 2.0001 * np.ones(n), -np.ones(n - 1)], [-1, 0, 1]).tocsr()
        return _csr(sp.diags(s) @ A @ sp.diags(s)) + (n, {})
    if name == "one":
        return _freeze(np.array([0, 1], np.int32), np.zeros(1, np.int32), np.array([2.5])) + (1, {})
    if name == "empty":
        return _freeze(np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros(0)) + (0, {})
    raise KeyError(name)


def options(name):
    return dict(DEFAULTS, **case(name)[4])


def matrix(name):
    rp, ci, va, n, _ = case(name)
    return sp.csr_matrix((va.copy(), ci.copy(), rp.copy()), (n, n))     # scipy sorts unsorted rows in place


@functools.lru_cache(maxsize=None)
def vectors(n):
    """the test vectors of the cycle: uniform(-1, 1), the constant, one unit vector"""
    e = np.zeros(n)
    e[n // 2:n // 2 + 1] = 1.0
    return _freeze(np.random.default_rng(11).uniform(-1, 1, n), np.ones(n), e)


# ---- the reference -------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def reference_lib():
    out = os.path.join(tempfile.mkdtemp(prefix="amg_reference_"), "amg_reference.so")
    subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-shared", "-fPIC", os.path.join(ROOT, "tests", "amg_reference.c"), "-o", out,
                    "-lm"], check=True)
    lib = ctypes.CDLL(out)
    lib.amg_reference_build.restype = ctypes.c_void_p
    lib.amg_reference_build.argtypes = [ctypes.c_long, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_double, ctypes.c_int,
                                        ctypes.c_int]
    for f in (lib.amg_reference_free, lib.amg_reference_levels, lib.amg_reference_stalled):
        f.argtypes = [ctypes.c_void_p]
    lib.amg_reference_level.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    lib.amg_reference_aggregates.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
    lib.amg_reference_csr.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    return lib


_p = lambda a: a.ctypes.data_as(ctypes.c_void_p)


def reference(rp, ci, va, n, theta=DEFAULTS["theta"], max_levels=DEFAULTS["max_levels"], coarse_rows=DEFAULTS["coarse_rows"], **_):
    """the hierarchy of the sequential loops: dict(levels, stalled, lev = [dict(n, A = (rp, ci, va), P = (rp, ci, va) or None, agg (empty
    where the level was not coarsened), aggregates, rounds, omega, rho)])"""
    lib = reference_lib()
    arrs = [np.ascontiguousarray(a, t) for a, t in ((rp, np.int32), (ci, np.int32), (va, np.float64))]
    h = lib.amg_reference_build(n, *[_p(a) for a in arrs], theta, max_levels, coarse_rows)
    out = dict(levels=lib.amg_reference_levels(h), stalled=lib.amg_reference_stalled(h), lev=[])
    for l in range(out["levels"]):
        num, dbl = np.zeros(5, np.int64), np.zeros(2)
        lib.amg_reference_level(h, l, _p(num), _p(dbl))
        rows, nnz, nnz_p, aggregates, rounds = (int(v) for v in num)
        L = dict(n=rows, aggregates=aggregates, rounds=rounds, omega=float(dbl[0]), rho=float(dbl[1]), P=None)
        for which, count in ((0, nnz), (1, nnz_p)):
            if which == 0 or nnz_p:
                c = np.zeros(rows + 1, np.int32), np.zeros(count, np.int32), np.zeros(count)
                lib.amg_reference_csr(h, l, which, *[_p(a) for a in c])
                L["P" if which else "A"] = _freeze(*c)
        agg = np.full(rows if rounds else 0, -1, np.int32)
        if rounds:
            lib.amg_reference_aggregates(h, l, _p(agg))
        L["agg"], = _freeze(agg)
        out["lev"].append(L)
    lib.amg_reference_free(h)
    return out


@functools.lru_cache(maxsize=None)
def reference_of(name):
    rp, ci, va, n, _ = case(name)
    return reference(rp, ci, va, n, **options(name))


def reference_factor(rp, ci, va, n):
    """the packed Cholesky factor of the sequential loop, or None at a bad pivot"""
    F = np.zeros(n * (n + 1) // 2 + 1)
    ok = reference_lib().amg_reference_factor(ctypes.c_long(n), *[_p(np.ascontiguousarray(a, t)) for a, t in
                                              ((rp, np.int32), (ci, np.int32), (va, np.float64))], _p(F))
    return F if ok else None


def reference_dense_solve(F, b):
    """(L L^t)^-1 b of the sequential column loops, fp64"""
    b = np.ascontiguousarray(b, np.float64)
    x = np.zeros(max(len(b), 1))
    reference_lib().amg_reference_dense_solve(ctypes.c_long(len(b)), _p(F), _p(b), _p(x))
    return x[:len(b)]


# ---- the hierarchy, restated ---------------------------------------------------------------------------------------------------------

def strong_edges(A, theta):
    """(rows, cols, |a_ij|) of the strong off-diagonal entries of a scipy CSR"""
    C = A.tocoo()
    d = A.diagonal()
    keep = (C.row != C.col) & (C.data * C.data >= (theta * theta) * (d[C.row] * d[C.col]))
    return C.row[keep], C.col[keep], np.abs(C.data[keep])


def restated_aggregates(A, theta):
    """(agg, roots (bool), rounds) of steps 3 and 4"""
    n = A.shape[0]
    rows, cols, mag = strong_edges(A, theta)
    idx = np.arange(n, dtype=np.uint64)
    h = (idx * np.uint64(0x9E3779B1)) & np.uint64(0xffffffff)
    low = ((h >> np.uint64(1)) << np.uint64(31)) | idx
    state = np.ones(n, np.uint64)
    rounds = 0
    while (state == 1).any():
        rounds += 1
        own = (state << np.uint64(62)) | low
        key = own
        for _ in range(2):
            nxt = key.copy()
            np.maximum.at(nxt, rows, key[cols])
            key = nxt
        und = state == 1
        root = und & (key == own)
        out = und & ~root & ((key >> np.uint64(62)) == 2)
        state[root], state[out] = 2, 0
    roots = state == 2
    agg = np.where(roots, np.cumsum(roots) - 1, -1)
    for _ in range(2):
        use = (agg[rows] < 0) & (agg[cols] >= 0)
        r, c, m = rows[use], cols[use], mag[use]
        order = np.lexsort((c, -m, r))                    # by row, then the largest |a_ij|, then the smallest column
        r, c = r[order], c[order]
        first = np.concatenate([[True], r[1:] != r[:-1]]) if len(r) else np.zeros(0, bool)
        nxt = agg.copy()
        nxt[r[first]] = agg[c[first]]
        agg = nxt
    return agg, roots, rounds


def restated_hierarchy(A, theta=DEFAULTS["theta"], max_levels=DEFAULTS["max_levels"], coarse_rows=DEFAULTS["coarse_rows"], **_):
    """the levels as dicts(A, P or None, agg or None, roots, omega, rho) by scipy's own products; (levels, stalled)"""
    lev, stalled = [], False
    while A.shape[0]:
        n, d = A.shape[0], A.diagonal()
        rho = float((np.asarray(abs(A).sum(axis=1)).ravel() / d).max())
        L = dict(A=A, P=None, agg=None, roots=None, omega=4.0 / (3.0 * rho), rho=rho)
        lev.append(L)
        if n <= coarse_rows or len(lev) == max_levels:
            break
        L["agg"], L["roots"], _ = restated_aggregates(A, theta)
        nc = int(L["roots"].sum())
        if nc > 0.9 * n:
            stalled = True
            break
        T = sp.csr_matrix((np.ones(n), (np.arange(n), L["agg"])), (n, nc))
        L["P"] = (T - sp.diags(L["omega"] / d) @ (A @ T)).tocsr()
        A = (L["P"].T @ A @ L["P"]).tocsr()
    return lev, stalled


# ---- the cycle, restated ---------------------------------------------------------------------------------------------------------------

def _dense_solver(A, dtype):
    """b -> A^-1 b for the SPD last level: fp64 Cholesky for fp32 / fp64 vectors (what the engine does), a longdouble one otherwise"""
    D = A.toarray()
    if np.dtype(dtype) != np.longdouble:
        c = scipy.linalg.cho_factor(D)
        return lambda b: scipy.linalg.cho_solve(c, b.astype(np.float64)).astype(dtype)
    n = D.shape[0]
    L = np.zeros((n, n), np.longdouble)
    S = D.astype(np.longdouble)
    for k in range(n):
        L[k, k] = np.sqrt(S[k, k] - L[k, :k] @ L[k, :k])
        L[k + 1:, k] = (S[k + 1:, k] - L[k + 1:, :k] @ L[k, :k]) / L[k, k]

    def solve(b):
        y = b.astype(np.longdouble)
        for k in range(n):
            y[k] = (y[k] - L[k, :k] @ y[:k]) / L[k, k]
        for k in range(n - 1, -1, -1):
            y[k] = (y[k] - L[k + 1:, k] @ y[k + 1:]) / L[k, k]
        return y
    return solve


def cycle_of(ref, dtype, sweeps=DEFAULTS["sweeps"], coarse_sweeps=DEFAULTS["coarse_sweeps"], **_):
    """v -> M^-1 v in `dtype` (float32, float64 or longdouble) over the hierarchy of reference(): the operators and w = omega / d are
    the reference's fp64 numbers converted to dtype, every product and sum is dtype's. The last level is solved densely when it has
    at most 128 rows."""
    ops = []
    for L in ref["lev"]:
        n = L["n"]
        A = sp.csr_matrix((L["A"][2], L["A"][1], L["A"][0]), (n, n))
        op = dict(A=A.astype(dtype), w=(L["omega"] / A.diagonal()).astype(dtype), P=None)
        if L["P"] is not None:
            P = sp.csr_matrix((L["P"][2], L["P"][1], L["P"][0]), (n, L["aggregates"]))
            op["P"], op["R"] = P.astype(dtype), P.T.tocsr().astype(dtype)
        ops.append(op)
    if not ops:
        return lambda v: v.astype(dtype)
    last = ops[-1]
    dense = _dense_solver(sp.csr_matrix((ref["lev"][-1]["A"][2], ref["lev"][-1]["A"][1], ref["lev"][-1]["A"][0]),
                                        (ref["lev"][-1]["n"],) * 2), dtype) if ref["lev"][-1]["n"] <= 128 else None

    def smooth(op, x, b):
        return x + op["w"] * (b - op["A"] @ x)

    def cycle(l, b):
        op = ops[l]
        if op is last:
            if dense is not None:
                return dense(b)
            x = op["w"] * b
            for _ in range(coarse_sweeps - 1):
                x = smooth(op, x, b)
            return x
        x = op["w"] * b
        for _ in range(sweeps - 1):
            x = smooth(op, x, b)
        r = b - op["A"] @ x
        x = x + op["P"] @ cycle(l + 1, op["R"] @ r)
        for _ in range(sweeps):
            x = smooth(op, x, b)
        return x
    return lambda v: cycle(0, v.astype(dtype))


@functools.lru_cache(maxsize=None)
def cycle_restatement(name, dtype):
    return cycle_of(reference_of(name), dtype, **options(name))


def measured_cycle_difference(dtype):
    """the largest max-norm relative difference over CYCLE_CASES and vectors() between the restatement in dtype and in the next wider
    type (fp32 against fp64, fp64 against longdouble)"""
    wide = np.float64 if np.dtype(dtype) == np.float32 else np.longdouble
    worst = 0.0
    for name in CYCLE_CASES:
        lo, hi = cycle_restatement(name, dtype), cycle_restatement(name, wide)
        for v in vectors(case(name)[3]):
            v = v.astype(dtype)
            a, b = lo(v).astype(np.longdouble), hi(v.astype(wide)).astype(np.longdouble)
            worst = max(worst, float(np.abs(a - b).max() / np.abs(b).max()))
    return worst


# ---- the preconditioned solve, restated ------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def grid_restatement(name, dtype, tol, max_iterations=pc.MAX_ITERATIONS, negated=False):
    """(x, history, stop) of pcg_tri_cases.restate on pcg_tri_cases.problem() with M^-1 = the cycle of case `name` (a grid case)"""
    P = pc.problem()
    x, hist, stop = pc.restate(P.dense(dtype, negated), P.b, cycle_restatement(name, dtype), tol, max_iterations, dtype)
    x.setflags(write=False)
    hist.setflags(write=False)
    return x, hist, stop


@functools.lru_cache(maxsize=None)
def path_problem():
    """(A as scipy CSR, b) of path_wrap"""
    A = matrix("path_wrap")
    b, = _freeze(np.random.default_rng(7).uniform(-1, 1, A.shape[0]))
    return A, b


@functools.lru_cache(maxsize=None)
def path_restatement():
    A, b = path_problem()
    x, hist, stop = pc.restate(A, b, cycle_restatement("path_wrap", np.float64), PATH_TOL, pc.MAX_ITERATIONS, np.float64)
    return _freeze(x, hist) + (stop,)
