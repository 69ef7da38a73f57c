"""What the two tiers of the multicolour ordering tests share (test_color_abi.py on the CPU, test_gpu_color.py on the GPU): the C
reference of tests/color_reference.c (first-fit greedy colouring in descending key order over A + A^t), the permutation and the
permuted matrix B = P A P^t restated in plain numpy, and the test matrices. Nothing here touches the engine. Everything is computed once
and is read-only.

Every matrix comes as (row_ptr, col_idx, values, n). The cases and what each exercises:

    grid        pcg_tri_cases.spd_grid(45), n = 2025         the reference operator
    unsorted    its rows shuffled                            rows not in column order
    dup         one column of it stored twice                duplicates
    oneway      diagonal + strict lower bidiagonal + a few   a nonsymmetric pattern: the colours come out wrong when A^t is not walked
                one-sided far entries
    clique70    dense 70 x 70                                70 colours, 70 rounds: the second window of 64 colours
    star        one row and column of 3000 entries           a wide row
    isolated    empty rows and diagonal-only rows            rows without neighbours
    stencil27   14^3, the 27-point stencil                   about 16 colours
    path_wrap   262 144 + 37 rows, tridiagonal               the first workgroup's second grid-stride trip
    one, empty  n = 1, n = 0                                 the degenerate sizes
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
CASES = ("grid", "unsorted", "dup", "oneway", "clique70", "star", "isolated", "stencil27", "path_wrap", "one", "empty")
HASH_MUL = 0x9E3779B1


# ---- the reference -------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def reference_lib():
    out = os.path.join(tempfile.mkdtemp(prefix="color_reference_"), "color_reference.so")
    subprocess.run(["gcc", "-O2", "-shared", "-fPIC", os.path.join(ROOT, "tests", "color_reference.c"), "-o", out], check=True)
    lib = ctypes.CDLL(out)
    lib.color_reference.restype = ctypes.c_long
    return lib


def keys(n):
    """key(i) of the header, as uint64"""
    i = np.arange(n, dtype=np.uint64)
    h = (i * np.uint64(HASH_MUL)) & np.uint64(0xffffffff)
    return ((h >> np.uint64(1)) << np.uint64(31)) | i


def color_of(rp, ci, n):
    """(colors, num_colors, rounds) of the sequential greedy loop"""
    rp = np.ascontiguousarray(rp, np.int32)
    ci = np.ascontiguousarray(ci, np.int32)
    colors = np.full(max(n, 1), -7, np.int32)
    rounds = ctypes.c_long(-1)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    nc = reference_lib().color_reference(ctypes.c_long(n), p(rp), p(ci), p(colors), ctypes.byref(rounds))
    return colors[:n], int(nc), int(rounds.value)


def permutation_of(colors, num_colors):
    """(perm, rank, color_ptr): the rows by (colour, row), the inverse, the first position of every colour"""
    n = len(colors)
    perm = np.argsort(colors, kind="stable").astype(np.int32)
    rank = np.empty(n, np.int32)
    rank[perm] = np.arange(n, dtype=np.int32)
    color_ptr = np.concatenate([[0], np.cumsum(np.bincount(colors, minlength=num_colors))]).astype(np.int32)
    return perm, rank, color_ptr


def permuted_of(rp, ci, va, n, rank):
    """(row_ptr, col_idx, values, entry_map) of B = P A P^t: the entries by (new row, new column), equal ones in stored order"""
    rows = np.repeat(np.arange(n), np.diff(rp))
    new_row, new_col = rank[rows], rank[ci]
    order = np.lexsort((new_col, new_row))                     # stable: ties keep the entry order
    rp_b = np.concatenate([[0], np.cumsum(np.bincount(new_row, minlength=n))]).astype(np.int32)
    return rp_b, new_col[order].astype(np.int32), np.ascontiguousarray(va[order]), order.astype(np.int32)


def adjacency(rp, ci, n):
    """the graph as a scipy CSR of ones: i ~ j when a_ij or a_ji is stored, i != j"""
    A = sp.csr_matrix((np.ones(len(ci)), np.asarray(ci), np.asarray(rp)), shape=(n, n))
    S = ((A + A.T) != 0).astype(np.int8).tolil()
    S.setdiag(0)
    S = S.tocsr()
    S.eliminate_zeros()
    S.sort_indices()
    return S


# ---- matrices ------------------------------------------------------------------------------------------------------------------------

def _frozen(rp, ci, va, n):
    out = (np.ascontiguousarray(rp, np.int32), np.ascontiguousarray(ci, np.int32), np.ascontiguousarray(va, np.float64), n)
    for a in out[:3]:
        a.setflags(write=False)
    return out


def _of_scipy(M):
    M = M.tocsr()
    M.sort_indices()
    return _frozen(M.indptr, M.indices, M.data, M.shape[0])


@functools.lru_cache(maxsize=None)
def matrix(name):
    if name == "grid":
        return _frozen(*pc.spd_grid(45)[:4])
    if name == "unsorted":                                # the same rows, every row in a random order
        rp, ci, va, n = matrix("grid")
        rows = np.repeat(np.arange(n), np.diff(rp))
        order = np.lexsort((np.random.default_rng(11).uniform(size=len(ci)), rows))
        return _frozen(rp, ci[order], va[order], n)
    if name == "dup":                                     # row 100 stores its second column twice, half the value each
        rp, ci, va, n = matrix("grid")
        e = rp[100] + 1
        ci2 = np.insert(ci, e, ci[e])
        va2 = np.insert(va, e, va[e] / 2)
        va2[e + 1] = va[e] / 2
        rp2 = rp.copy()
        rp2[101:] += 1
        return _frozen(rp2, ci2, va2, n)
    if name == "oneway":                                  # row i stores (i, i - 1) and (i, i); a few far entries on one side only
        n = 2000
        far = {5: 900, 17: 1500, 3: 1999, 1200: 40, 1999: 7}
        rp, ci, va = [0], [], []
        for i in range(n):
            c = sorted({i, i - 1, far.get(i, i)} - {-1})
            ci += c
            va += [4.0 if j == i else -1.0 for j in c]
            rp.append(len(ci))
        return _frozen(rp, ci, va, n)
    if name == "clique70":
        n = 70
        D = np.random.default_rng(70).uniform(-1, 1, (n, n))
        D[np.arange(n), np.arange(n)] = 80.0
        return _frozen(np.arange(n + 1) * n, np.tile(np.arange(n), n), D.ravel(), n)
    if name == "star":                                    # row 0 and column 0 are full
        n = 3000
        M = sp.lil_matrix((n, n))
        M[0, :] = -1.0
        M[:, 0] = -1.0
        M.setdiag(3000.0)
        return _of_scipy(M)
    if name == "isolated":                                # rows 0 - 9 empty, 10 - 19 their diagonal alone, then a path with gaps
        n = 60
        rp, ci, va = [0], [], []
        for i in range(n):
            if i >= 10:
                c = [i] if i < 20 or i % 7 == 0 else sorted({i - 1, i} if i % 7 != 1 else {i})
                ci += c
                va += [3.0 if j == i else -1.0 for j in c]
            rp.append(len(ci))
        return _frozen(rp, ci, va, n)
    if name == "stencil27":
        k = 14
        T = sp.diags([np.ones(k - 1), np.ones(k), np.ones(k - 1)], [-1, 0, 1])
        M = sp.kron(sp.kron(T, T), T).tocsr()
        M.data[:] = -1.0
        M.setdiag(27.0)
        return _of_scipy(M)
    if name == "path_wrap":
        n = 262144 + 37
        M = sp.diags([-np.ones(n - 1), 2.5 * np.ones(n), -np.ones(n - 1)], [-1, 0, 1])
        return _of_scipy(M)
    if name == "one":
        return _frozen([0, 1], [0], [2.5], 1)
    if name == "empty":
        return _frozen(np.zeros(1), np.zeros(0), np.zeros(0), 0)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def reference(name):
    """dict(colors, num_colors, rounds, perm, rank, color_ptr) of a named matrix, computed once"""
    rp, ci, va, n = matrix(name)
    colors, nc, rounds = color_of(rp, ci, n)
    perm, rank, color_ptr = permutation_of(colors, nc)
    out = dict(colors=colors, num_colors=nc, rounds=rounds, perm=perm, rank=rank, color_ptr=color_ptr)
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def permuted(name):
    """(row_ptr, col_idx, values, entry_map) of B for a named matrix under the reference's permutation, computed once"""
    rp, ci, va, n = matrix(name)
    out = permuted_of(rp, ci, va, n, reference(name)["rank"])
    for a in out:
        a.setflags(write=False)
    return out


# ---- the solves on the permuted grid ---------------------------------------------------------------------------------------------------

# the restatement's iteration counts on B = P A P^t of spd_grid(45), right-hand side P b, tol 1e-12 in fp64 and 1e-5 in fp32 under the
# multicolour SGS and IC(0) of B (recomputed in test_color_abi.py)
COUNTS = {np.float64: dict(sgs=50, ic0=49), np.float32: dict(sgs=21, ic0=21)}


class PermutedProblem:
    """pcg_tri_cases.problem() in the colour ordering: D, b, csr, k_row for shares_of_the_bounds, and the restated solves"""

    def __init__(self):
        P = pc.problem()
        ref = reference("grid")
        perm = ref["perm"]
        self.base, self.perm, self.rank, self.n = P, perm, ref["rank"], P.n
        self.D = np.ascontiguousarray(P.D[np.ix_(perm, perm)])
        self.b = np.ascontiguousarray(P.b[perm])
        self.k_row = P.k_row
        self.csr = permuted("grid")[:3]
        assert np.array_equal(pc.csr_of(self.D)[0], self.csr[0]) and np.array_equal(pc.csr_of(self.D)[1], self.csr[1])
        assert np.array_equal(pc.csr_of(self.D)[2], self.csr[2]), "B is the dense matrix permuted, to the bit"
        for a in (self.D, self.b):
            a.setflags(write=False)

    def apply(self, kind, dtype):
        import ilu0_cases as ic
        import trsv_blocked_cases as bc
        rp, ci, va = self.csr
        if kind == "sgs":
            return bc.sgs_apply(rp, ci, va, self.n, None, dtype)
        f, bad = ic.reference(rp, ci, va, self.n)
        assert bad == -1
        return ic.apply(rp, ci, f, self.n, None, dtype)

    @functools.lru_cache(maxsize=None)
    def restatement(self, dtype, kind, tol, max_iterations=pc.MAX_ITERATIONS):
        x, hist, stop = pc.restate(self.D.astype(dtype), self.b, self.apply(kind, dtype), tol, max_iterations, dtype)
        x.setflags(write=False)
        hist.setflags(write=False)
        return x, hist, stop


@functools.lru_cache(maxsize=None)
def problem():
    return PermutedProblem()
