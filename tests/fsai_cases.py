"""What the two tiers of the FSAI tests share (test_fsai_abi.py on the CPU, test_gpu_fsai.py on the GPU): the matrices with their
patterns, the C reference of tests/fsai_reference.c (the header's arithmetic as one sequential loop, gcc -ffp-contract=off), the numpy
restatement (np.linalg.cholesky of A(J, J) per row, then a solve), and the CG iteration counts with M^-1 = G^t (G .) on the problem
of pcg_tri_cases.py. Nothing here touches the engine. Everything is computed once and is read-only.

A case is (row_ptr, col_idx, values, n, pattern) with pattern = (pat_row_ptr, pat_col_idx), or None for the lower triangle of A's own
pattern; pattern_of() gives the explicit pattern either way. The matrices hold BOTH triangles and are symmetric to the bit.

The counts of pcg_tri_cases.restate with M^-1 = G^t (G .), G from the C reference, tol 1e-12 in fp64 and 1e-5 in fp32 (COUNTS;
recomputed in test_fsai_abi.py):

      pattern                   fp64   fp32    cond(G A G^t), against 92.1 of A
      tril(A)                     58     25    21.2
      tril(A)^2 (<= 6 per row)    41     18    10.9
"""
import ctypes
import functools
import os
import subprocess
import tempfile

import numpy as np
import scipy.sparse as sp

import pcg_tri_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_ROW = 128
# the launch geometry of csrc/fsai.hpp for rows of at most 8 entries: 32 rows per workgroup, at most 2048 workgroups per launch
SMALL_BIN_ROWS, MAX_GRID = 32, 2048
COUNTS = {np.float64: {1: 58, 2: 41}, np.float32: {1: 25, 2: 18}}


# ---- the reference -------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def reference_lib():
    out = os.path.join(tempfile.mkdtemp(prefix="fsai_reference_"), "fsai_reference.so")
    subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-shared", "-fPIC", os.path.join(ROOT, "tests", "fsai_reference.c"), "-o", out,
                    "-lm"], check=True)
    lib = ctypes.CDLL(out)
    lib.fsai_reference.restype = ctypes.c_long
    return lib


def reference(rp, ci, va, n, pattern):
    """(G's fp64 values in the pattern's entry order, the rows that fell back) of the sequential loop"""
    prp, pci = pattern
    arrs = [np.ascontiguousarray(a, t) for a, t in ((rp, np.int32), (ci, np.int32), (va, np.float64), (prp, np.int32), (pci, np.int32))]
    g = np.full(max(int(prp[n]), 1), np.nan)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    fell = reference_lib().fsai_reference(ctypes.c_long(n), *[p(a) for a in arrs], p(g))
    assert fell >= 0
    g = g[:int(prp[n])]
    g.setflags(write=False)
    return g, int(fell)


def restatement(D, pattern):
    """the same rows in numpy from a dense A: np.linalg.cholesky of A(J, J), then C^t g = e_s. (values, rows that fell back)"""
    prp, pci = pattern
    n = len(prp) - 1
    g = np.zeros(int(prp[n]))
    fell = 0
    for i in range(n):
        J = pci[prp[i]:prp[i + 1]]
        S = D[np.ix_(J, J)]
        try:
            if not np.all(np.isfinite(S)):
                raise np.linalg.LinAlgError
            C = np.linalg.cholesky(S)
            e = np.zeros(len(J))
            e[-1] = 1.0
            g[prp[i]:prp[i + 1]] = np.linalg.solve(C.T, e)
        except np.linalg.LinAlgError:
            fell += 1
            g[prp[i + 1] - 1] = 1.0 / np.sqrt(D[i, i])
    return g, fell


# ---- patterns ------------------------------------------------------------------------------------------------------------------------

def tril_power(rp, ci, n, power=1):
    """the pattern of tril(A~)^power by scipy, columns ascending: A~ = the lower triangle of A's pattern with the diagonal added"""
    rows = np.repeat(np.arange(n), np.diff(rp))
    keep = ci <= rows
    L = sp.csr_matrix((np.ones(int(keep.sum()) + n), (np.append(rows[keep], np.arange(n)), np.append(ci[keep], np.arange(n)))), (n, n))
    L.data[:] = 1.0
    P = L.copy()
    for _ in range(power - 1):
        P = (P @ L).tocsr()
        P.data[:] = 1.0
    P.sum_duplicates()
    P.sort_indices()
    out = P.indptr.astype(np.int32), P.indices.astype(np.int32)
    for a in out:
        a.setflags(write=False)
    return out


def pattern_of(case):
    rp, ci, va, n, pattern = case
    return tril_power(rp, ci, n) if pattern is None else pattern


def dense_g(case, values, dtype=np.float64):
    """the dense G of a case from its values, narrowed to dtype as spmv_mi355x_create narrows them"""
    prp, pci = pattern_of(case)
    n = case[3]
    G = np.zeros((n, n), dtype)
    G[np.repeat(np.arange(n), np.diff(prp)), pci] = values.astype(dtype)
    return G


# ---- matrices ------------------------------------------------------------------------------------------------------------------------

def _freeze(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def _csr_of_dense(D, keep=None):
    """(row_ptr, col_idx, values) of the entries of D where keep (default: D != 0), columns ascending"""
    rows, cols = np.nonzero(D if keep is None else keep)
    rp = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=D.shape[0]))]).astype(np.int32)
    return rp, cols.astype(np.int32), np.ascontiguousarray(D[rows, cols])


@functools.lru_cache(maxsize=None)
def banded(n, half_bandwidth):
    """dense SPD by diagonal dominance: uniform(-1, 1) within the band, the diagonal = the row's sum of |a_ij| + 1"""
    rng = np.random.default_rng(1000 * n + half_bandwidth)
    L = np.tril(rng.uniform(-1, 1, (n, n)), -1)
    i, j = np.indices((n, n))
    L[i - j > half_bandwidth] = 0.0
    D = L + L.T
    D[np.arange(n), np.arange(n)] = np.abs(D).sum(axis=1) + 1.0
    D.setflags(write=False)
    return D


@functools.lru_cache(maxsize=None)
def random_symmetric(n=1000, widest=40):
    """dense SPD whose row i holds 0 .. min(i, widest - 1) entries left of the diagonal, at random places; every tenth row holds
    none, so rows of one pattern entry are spread among the others"""
    rng = np.random.default_rng(n + widest)
    L = np.zeros((n, n))
    for i in range(1, n):
        k = 0 if i % 10 == 0 else int(rng.integers(0, min(i, widest - 1) + 1))
        L[i, rng.permutation(i)[:k]] = rng.uniform(-1, 1, k)
    D = L + L.T
    D[np.arange(n), np.arange(n)] = np.abs(D).sum(axis=1) + 1.0
    D.setflags(write=False)
    return D


def shuffled_rows(rp, ci, va, seed=5):
    """the same CSR with the entries of every row in a random order"""
    rng = np.random.default_rng(seed)
    ci, va = ci.copy(), va.copy()
    for i in range(len(rp) - 1):
        o = rng.permutation(rp[i + 1] - rp[i]) + rp[i]
        ci[rp[i]:rp[i + 1]], va[rp[i]:rp[i + 1]] = ci[o], va[o]
    return rp, ci, va


@functools.lru_cache(maxsize=None)
def indefinite():
    """a symmetric matrix with a positive diagonal whose rows 0 and 1 hold the block [[1, 2], [2, 1]]: row 1 of G on the pattern
    {0, 1} meets the pivot 1 - 2 * 2 = -3 and falls back to (0, 1 / sqrt(1)); the other rows are diagonally dominant"""
    D = np.array([[1.0, 2.0, 0.0, 0.0, 0.0],
                  [2.0, 1.0, 0.0, 0.0, 0.0],
                  [0.0, 0.0, 4.0, -1.0, 0.5],
                  [0.0, 0.0, -1.0, 3.0, -1.0],
                  [0.0, 0.0, 0.5, -1.0, 5.0]])
    D.setflags(write=False)
    return D


@functools.lru_cache(maxsize=None)
def case(name):
    """(row_ptr, col_idx, values, n, pattern or None) by name; dense(name) is the same matrix dense where it is small"""
    if name in ("grid_tril", "grid_power2"):
        rp, ci, va, n, _ = pc.spd_grid(45)
        return rp, ci, va, n, None if name == "grid_tril" else tril_power(rp, ci, n, 2)
    if name.startswith("banded"):                         # banded70 (a row wider than a wave), banded127 (the cap), banded128 (refused)
        D = banded(400, int(name[6:]))
        return _freeze(*_csr_of_dense(D)) + (400, None)
    if name == "random":
        D = random_symmetric()
        return _freeze(*shuffled_rows(*_csr_of_dense(D))) + (1000, None)
    if name == "indefinite":
        return _freeze(*_csr_of_dense(indefinite())) + (5, None)
    if name == "empty":
        return _freeze(np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros(0)) + (0, None)
    if name == "one":
        return _freeze(np.array([0, 1], np.int32), np.zeros(1, np.int32), np.array([2.5])) + (1, None)
    if name == "tridiagonal_wrap":
        # 32 rows of this bin share a workgroup and a launch has at most 2048 workgroups: beyond 32 * 2048 = 65536 rows the
        # workgroups take a second trip of their row loop, here the first 2 of them (37 rows)
        n = SMALL_BIN_ROWS * MAX_GRID + 37
        s = 1 + 0.2 * np.random.default_rng(2).uniform(-1, 1, n)
        A = sp.diags([-np.ones(n - 1), 2.5 * np.ones(n), -np.ones(n - 1)], [-1, 0, 1]).tocsr()
        A = (sp.diags(s) @ A @ sp.diags(s)).tocsr()
        A.sort_indices()
        return _freeze(A.indptr.astype(np.int32), A.indices.astype(np.int32), A.data.copy()) + (n, None)
    raise KeyError(name)


def dense(name):
    if name in ("grid_tril", "grid_power2"):
        return pc.spd_grid(45)[4]
    if name.startswith("banded"):
        return banded(400, int(name[6:]))
    return {"random": random_symmetric, "indefinite": indefinite}[name]()


@functools.lru_cache(maxsize=None)
def reference_of(name):
    c = case(name)
    return reference(c[0], c[1], c[2], c[3], pattern_of(c))


# ---- the preconditioned solve, restated ------------------------------------------------------------------------------------------------

def grid_case(power):
    return "grid_tril" if power == 1 else "grid_power2"


@functools.lru_cache(maxsize=None)
def grid_apply(power, dtype):
    """v -> G^t (G v) in dtype for the FSAI of spd_grid(45) on tril(A)^power, G from the C reference narrowed to dtype"""
    name = grid_case(power)
    G = sp.csr_matrix(dense_g(case(name), reference_of(name)[0], dtype))
    Gt = G.T.tocsr()
    return lambda v: (Gt @ (G @ v).astype(dtype)).astype(dtype)


@functools.lru_cache(maxsize=None)
def grid_restatement(power, dtype, tol, max_iterations=pc.MAX_ITERATIONS, negated=False):
    """(x, history, stop) of pcg_tri_cases.restate on pcg_tri_cases.problem() with M^-1 = G^t (G .)"""
    P = pc.problem()
    x, hist, stop = pc.restate(P.dense(dtype, negated), P.b, grid_apply(power, dtype), tol, max_iterations, dtype)
    x.setflags(write=False)
    hist.setflags(write=False)
    return x, hist, stop
