"""What the two tiers of the SpGEMM tests share (test_spgemm_abi.py on the CPU, test_gpu_spgemm.py on the GPU): the pairs of matrices,
the C reference of tests/spgemm_reference.c (the header's loop run sequentially, gcc -ffp-contract=off) and the bound against scipy.
Nothing here touches the engine. Everything is computed once and is read-only.

A case is (A, B) with A = (row_ptr, col_idx, values, m, k) and B = (row_ptr, col_idx, values, k, n).

The geometry of csrc/spgemm.hpp, restated: the rows are binned on w = min(products, n) for the counting pass and on the width of
C's row for the pass that writes the columns and for the numeric one, bins 0 .. 16, 17 .. 64, 65 .. 128, 129 .. 512, 513 .. 1024,
1025 .. 2048 with tables of 32, 128, 256, 1024, 2048, 4096 slots in LDS and 8, 16, 32, 64, 64, 64 lanes per row, and a seventh bin
beyond with its tables in global memory; 32 rows of the first bin share a workgroup and a launch has at most 2048 workgroups. The hash of a column is (col * 0x9E3779B1 mod 2^32) >> (32 - log2(slots))."""
import ctypes
import functools
import os
import subprocess
import tempfile

import numpy as np
import scipy.sparse as sp

import pcg_tri_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN_WMAX = (16, 64, 128, 512, 1024, 2048)
BIN_SLOTS = (32, 128, 256, 1024, 2048, 4096)
BINS = len(BIN_WMAX) + 1
NARROW_BIN_ROWS, MAX_GRID = 32, 2048
HASH_MUL = 0x9E3779B1
U = 2.0 ** -53


def bin_of(w):
    return sum(w > s for s in BIN_WMAX)


def hash_of(col, slots):
    return ((np.asarray(col, np.uint64) * HASH_MUL) & 0xFFFFFFFF) >> np.uint64(32 - int(np.log2(slots)))


# ---- the reference -------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def reference_lib():
    out = os.path.join(tempfile.mkdtemp(prefix="spgemm_reference_"), "spgemm_reference.so")
    subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-shared", "-fPIC", os.path.join(ROOT, "tests", "spgemm_reference.c"), "-o", out,
                    "-lm"], check=True)
    lib = ctypes.CDLL(out)
    lib.spgemm_reference.restype = ctypes.c_long
    return lib


def _freeze(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def reference(A, B, a_values=None, b_values=None):
    """(c_row_ptr, c_col_idx, c_values) of the sequential loop; the values of the case unless others are given"""
    a_rp, a_ci, a_va, m, k = A
    b_rp, b_ci, b_va, kb, n = B
    assert k == kb
    arrs = [np.ascontiguousarray(a, t) for a, t in ((a_rp, np.int32), (a_ci, np.int32), (a_va if a_values is None else a_values, np.float64),
                                                    (b_rp, np.int32), (b_ci, np.int32), (b_va if b_values is None else b_values, np.float64))]
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    c_rp = np.zeros(m + 1, np.int32)
    f = reference_lib().spgemm_reference
    nnz = f(ctypes.c_long(m), ctypes.c_long(k), ctypes.c_long(n), *[p(a) for a in arrs], p(c_rp), None, None)
    assert nnz >= 0
    c_ci, c_va = np.zeros(max(nnz, 1), np.int32), np.full(max(nnz, 1), np.nan)
    assert f(ctypes.c_long(m), ctypes.c_long(k), ctypes.c_long(n), *[p(a) for a in arrs], p(c_rp), p(c_ci), p(c_va)) == nnz
    return _freeze(c_rp, c_ci[:nnz], c_va[:nnz])


def scipy_of(M, values=None, ones=False):
    rp, ci, va, rows, cols = M
    data = np.ones(len(ci)) if ones else np.asarray(va if values is None else values, np.float64)
    return sp.csr_matrix((data.copy(), np.asarray(ci).copy(), np.asarray(rp).copy()), shape=(rows, cols))


def scipy_pattern(A, B):
    """(row_ptr, col_idx) of the structural product: scipy on all-ones data, which cannot cancel"""
    P = (scipy_of(A, ones=True) @ scipy_of(B, ones=True)).tocsr()
    P.sum_duplicates()
    P.sort_indices()
    assert np.all(P.data > 0)
    return P.indptr.astype(np.int32), P.indices.astype(np.int32), P.data.copy()


def shares_of_the_bound(A, B, c_rp, c_ci, c_va, a_values=None, b_values=None):
    """|c - scipy's| / (2 L u (|A| |B|)(i, j)) per entry of C, L = the products of that entry; entries where the bound is 0 must be
    equal and count as 0"""
    m, n = A[3], B[4]
    rows = np.repeat(np.arange(m), np.diff(c_rp))
    # |A| from |values|: abs() of a scipy matrix sums the two occurrences of a column first
    abs_a = scipy_of(A, np.abs(A[2] if a_values is None else a_values))
    abs_b = scipy_of(B, np.abs(B[2] if b_values is None else b_values))
    products = (scipy_of(A, a_values) @ scipy_of(B, b_values), abs_a @ abs_b, scipy_of(A, ones=True) @ scipy_of(B, ones=True))
    if m * n <= 4e6:
        want, absp, L = (P.toarray()[rows, c_ci] for P in products)
    else:
        want, absp, L = (np.asarray(P.tocsr()[rows, c_ci]).ravel() for P in products)
    bound = 2 * L * U * absp
    err = np.abs(np.asarray(c_va) - want)
    assert np.all(err[bound == 0] == 0)
    return err / np.where(bound > 0, bound, 1.0)


# ---- matrices ------------------------------------------------------------------------------------------------------------------------

def _csr_rows(rows, cols, rng=None, values=None):
    """(row_ptr, col_idx, values, len(rows), cols) of a list of column lists, in the order given; values uniform(-1, 1) unless given"""
    rp = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    ci = np.concatenate([np.asarray(r, np.int32) for r in rows] + [np.zeros(0, np.int32)]).astype(np.int32)
    va = rng.uniform(-1, 1, len(ci)) if values is None else np.asarray(values, np.float64)
    return _freeze(rp, ci, va) + (len(rows), cols)


def _random_rows(rng, rows, cols, longest, empty_every, twice_every=0):
    """0 .. longest distinct columns per row in a random order; every empty_every-th row empty; every twice_every-th row repeats its
    first column at its end"""
    out = []
    for i in range(rows):
        c = [] if i % empty_every == 0 else list(rng.permutation(cols)[:int(rng.integers(0, longest + 1))])
        if twice_every and i % twice_every == 1 and c:
            c.append(c[0])
        out.append(c)
    return out


def tril_of(rp, ci, va, n):
    rows = np.repeat(np.arange(n), np.diff(rp))
    keep = ci <= rows
    lrp = np.concatenate([[0], np.cumsum(np.bincount(rows[keep], minlength=n))]).astype(np.int32)
    return _freeze(lrp, ci[keep].copy(), va[keep].copy()) + (n, n)


@functools.lru_cache(maxsize=None)
def case(name):
    rng = np.random.default_rng(sum(map(ord, name)))
    if name == "grid":                                    # spd_grid(45) squared: n = 2025, at most 25 products per row
        rp, ci, va, n, _ = pc.spd_grid(45)
        A = (rp, ci, va, n, n)
        return A, A
    if name == "grid_tril":                               # L L for L = tril(A): the pattern of fsai_pattern(power = 2)
        rp, ci, va, n, _ = pc.spd_grid(45)
        L = tril_of(rp, ci, va, n)
        return L, L
    if name == "rect":
        # 300 x 500 times 500 x 200, 0 .. 12 entries per row in a random order, empty rows in both (so columns of A meet empty rows
        # of B), a column twice in some rows of A
        return (_csr_rows(_random_rows(rng, 300, 500, 12, 7, twice_every=5), 500, rng),
                _csr_rows(_random_rows(rng, 500, 200, 12, 9), 200, rng))
    if name == "bins":
        # B's row t holds LENGTHS[t] columns. A's rows: one entry per row of B (products = width = the length: both binnings at
        # every boundary S and S + 1, and at the first and last width of every bin); the same entry twice (products = twice the
        # width: the symbolic and the numeric bin differ); and two rows of B at once.
        n = 6000
        lengths = [1] + [s + d for s in BIN_WMAX for d in (0, 1)] + [4000]
        B = _csr_rows([rng.permutation(n)[:L] for L in lengths], n, rng)
        rows = [[t] for t in range(len(lengths))] + [[t, t] for t in range(len(lengths))] + [[1, 0], [4, 2], [12, 7, 6], []]
        return _csr_rows(rows, len(lengths), rng), B
    if name == "global_table":                            # 300 entries against rows of 40 columns in n = 20 000: 12 000 products
        n = 20000
        B = _csr_rows([rng.permutation(n)[:40] for _ in range(300)], n, rng)
        return _csr_rows([list(rng.permutation(300)), [5], [], list(rng.permutation(300)[:100])], 300, rng), B
    if name == "dense_row":                               # a row of C with all n = 3000 columns out of 6000 products: min(products, n)
        n = 3000
        halves = [np.arange(0, 1500), np.arange(1500, 3000), np.arange(750, 2250), np.r_[np.arange(0, 750), np.arange(2250, 3000)]]
        B = _csr_rows([rng.permutation(h) for h in halves], n, rng)
        return _csr_rows([[0, 1, 2, 3], [2], [3, 0, 1, 2, 1]], 4, rng), B
    if name == "collide":
        # every column of the row hashes to slot 0 of the 4096-slot table, the largest in LDS (1025 .. 2048 columns): insertion t
        # probes t slots
        n = 1 << 23
        cols = np.nonzero(hash_of(np.arange(n), BIN_SLOTS[-1]) == 0)[0]
        assert len(cols) >= COLLIDE_WIDTH
        B = _csr_rows([rng.permutation(cols[:COLLIDE_WIDTH])], n, rng)
        return _csr_rows([[0], [0, 0], [0]], 1, rng), B
    if name == "cancel":                                  # A = [1, -1], B's two rows equal: C stores zeros
        b = rng.uniform(-1, 1, 5)
        B = _csr_rows([[4, 0, 9, 2, 7], [4, 0, 9, 2, 7]], 12, values=np.r_[b, b])
        return _csr_rows([[0, 1], [1, 0]], 2, values=[1.0, -1.0, -1.0, 1.0]), B
    if name == "wrap":
        # 32 rows of the first bin share a workgroup and a launch has at most 2048 workgroups: beyond 65536 rows the workgroups take a
        # second trip of their row loop, here the first 2 of them (37 rows)
        n = NARROW_BIN_ROWS * MAX_GRID + 37
        T = sp.diags([rng.uniform(-1, 1, n - 1), rng.uniform(1, 2, n), rng.uniform(-1, 1, n - 1)], [-1, 0, 1]).tocsr()
        T.sort_indices()
        A = _freeze(T.indptr.astype(np.int32), T.indices.astype(np.int32), T.data.copy()) + (n, n)
        return A, A
    if name.startswith("empty_"):                         # empty_m, empty_k, empty_n: that dimension is 0; empty_a: nnz(A) = 0
        m, k, n = (0 if name == "empty_m" else 5), (0 if name == "empty_k" else 4), (0 if name == "empty_n" else 6)
        a_rows = [[] for _ in range(m)] if name in ("empty_k", "empty_a") else _random_rows(rng, m, k, 3, 4)
        b_rows = [[] for _ in range(k)] if name == "empty_n" else _random_rows(rng, k, n, 3, 3)
        return _csr_rows(a_rows, k, rng), _csr_rows(b_rows, n, rng)
    raise KeyError(name)


COLLIDE_WIDTH = 1100
SMALL_CASES = ("grid", "grid_tril", "rect", "bins", "global_table", "dense_row", "cancel", "empty_m", "empty_k", "empty_n", "empty_a")
GPU_CASES = SMALL_CASES + ("collide", "wrap")


@functools.lru_cache(maxsize=None)
def reference_of(name):
    return reference(*case(name))
