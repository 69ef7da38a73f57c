"""What the two tiers of the sparse triangular solve tests share (test_trsv_abi.py, test_gpu_trsv.py): the test matrices, the numpy
restatement of the level rule and the plan rule of include/spmv_mi355x.h, and the C reference of tests/trsv_reference.c.

Every matrix is built as a LOWER form (dependencies j < i) with a stored diagonal and comes as (row_ptr, col_idx, values, n); mirror()
gives its UPPER form (row i -> n - 1 - i, column c -> n - 1 - c, each row's entries in their stored order). Off-diagonal values are
uniform in [-1, 1] and scaled so that each row's sum of |a_ij| is at most 0.9, diagonals lie in +-[1, 2]: |x|inf <= 10 |b|inf at any
depth of the dependency graph, so nothing overflows. Matrices and references are computed once and never modified."""
import ctypes
import functools
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOWER, UPPER = 0, 1
PRESCRIBED_WIDTHS = (1, 1, 1, 2000, 1, 70, 64, 65, 3, 3000, 1, 1)


# ---- the reference -------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def reference_lib():
    out = os.path.join(tempfile.mkdtemp(prefix="trsv_reference_"), "trsv_reference.so")
    subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-shared", "-fPIC", os.path.join(ROOT, "tests", "trsv_reference.c"), "-o", out,
                    "-lm"], check=True)
    return ctypes.CDLL(out)


def reference(rp, ci, va, n, uplo, unit, b, dtype):
    """x of the sequential loop in `dtype`; va is narrowed to dtype first, as the handle narrows it"""
    dtype = np.dtype(dtype)
    rp = np.ascontiguousarray(rp, np.int32)
    ci = np.ascontiguousarray(ci, np.int32)
    va = np.ascontiguousarray(np.asarray(va, np.float64).astype(dtype))
    b = np.ascontiguousarray(b, dtype)
    x = np.full(max(n, 1), np.nan, dtype)
    fn = reference_lib().trsv_reference_f64 if dtype == np.float64 else reference_lib().trsv_reference_f32
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    fn(ctypes.c_int(uplo), ctypes.c_int(1 if unit else 0), ctypes.c_long(n), p(rp), p(ci), p(va), p(b), p(x))
    return x[:n]


# ---- the rules, restated -------------------------------------------------------------------------------------------------------------

def levels_of(rp, ci, n, uplo):
    level = np.zeros(n, np.int32)
    for i in (range(n) if uplo == LOWER else range(n - 1, -1, -1)):
        c = ci[rp[i]:rp[i + 1]]
        c = c[c < i] if uplo == LOWER else c[c > i]
        if len(c):
            level[i] = level[c].max() + 1
    return level


def plan_of(level, chain_rows):
    """(levels, launches, max_level_rows) of the plan rule: a maximal run of levels with at most chain_rows rows is one launch"""
    if len(level) == 0:
        return 0, 0, 0
    rows = np.bincount(level)
    thin = rows <= chain_rows
    runs = int(thin[0]) + int(np.sum(thin[1:] & ~thin[:-1]))
    return len(rows), int(np.sum(~thin)) + runs, int(rows.max())


# ---- matrices ------------------------------------------------------------------------------------------------------------------------

def assemble(n, deps, rng, shuffle=True):
    """CSR of a lower form from deps[i] = the columns j < i of row i (duplicates kept as separate entries): scaled off-diagonal values,
    a diagonal in +-[1, 2] at a random place of the row (shuffle) or at its end."""
    rp = np.zeros(n + 1, np.int64)
    ci, va = [], []
    for i in range(n):
        d = np.asarray(deps[i], np.int64)
        a = rng.uniform(-1, 1, len(d))
        if len(d):
            a *= 0.9 / max(np.abs(a).sum(), 0.9)
        cols = np.append(d, i)
        vals = np.append(a, rng.uniform(1, 2) * rng.choice((-1.0, 1.0)))
        if shuffle:
            o = rng.permutation(len(cols))
            cols, vals = cols[o], vals[o]
        ci.append(cols)
        va.append(vals)
        rp[i + 1] = rp[i] + len(cols)
    return rp.astype(np.int32), np.concatenate(ci).astype(np.int32) if n else np.zeros(0, np.int32), \
        np.concatenate(va) if n else np.zeros(0), n


def mirror(rp, ci, va, n):
    rp = np.asarray(rp, np.int64)
    lens = np.diff(rp)[::-1]
    rp2 = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    ci2, va2 = np.empty_like(ci), np.empty_like(va)
    for i in range(n):
        s, e = rp[i], rp[i + 1]
        t = rp2[n - 1 - i]
        ci2[t:t + e - s] = n - 1 - ci[s:e]
        va2[t:t + e - s] = va[s:e]
    return rp2, ci2, va2, n


@functools.lru_cache(maxsize=None)
def lower_matrix(name):
    rng = np.random.default_rng(sum(map(ord, name)))
    if name == "empty":
        return assemble(0, [], rng)
    if name == "one":
        return assemble(1, [[]], rng)
    if name == "diagonal":                                # one level, several workgroups of the level kernel at chain_rows < 1500
        return assemble(1500, [[]] * 1500, rng)
    if name == "bidiagonal":                              # 4097 levels of one row: a pure chain across the 64- and 1024-row marks
        return assemble(4097, [[]] + [[i - 1] for i in range(1, 4097)], rng)
    if name == "prescribed":                              # level l has PRESCRIBED_WIDTHS[l] rows, level after level
        deps, start = [], [0]
        for l, w in enumerate(PRESCRIBED_WIDTHS):
            for _ in range(w):
                if l == 0:
                    deps.append([])
                else:
                    d = [rng.integers(start[l - 1], start[l])]                 # what puts the row into level l
                    d += list(rng.integers(0, start[l], rng.integers(0, 3)))    # anything earlier
                    deps.append(d)
            start.append(start[-1] + w)
        return assemble(start[-1], deps, rng)
    if name == "dag":                                     # 3000 rows, 0-8 columns among j < i, half of them within 4 of i
        deps = [[]]
        for i in range(1, 3000):
            k = rng.integers(0, 9)
            near = rng.integers(max(0, i - 4), i, k)
            far = rng.integers(0, i, k)
            deps.append(list(np.where(rng.random(k) < 0.5, near, far)))
        return assemble(3000, deps, rng)
    if name == "padding":                                 # level 1: one row of 700 entries among 299 rows of one entry
        deps = [[]] * 800
        for r in range(300):
            deps.append(list(rng.permutation(800)[:700]) if r == 100 else [rng.integers(0, 800)])
        return assemble(1100, deps, rng)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def stencil_full(k=24):
    """the 7-point stencil on a k^3 grid with BOTH triangles, columns ascending, values as above (diagonal dominant by the scaling)"""
    rng = np.random.default_rng(k)
    n = k ** 3
    idx = np.arange(n).reshape(k, k, k)
    rows, cols = [np.arange(n)], [np.arange(n)]
    for ax in range(3):
        lo = np.take(idx, range(k - 1), axis=ax).ravel()
        hi = np.take(idx, range(1, k), axis=ax).ravel()
        rows += [lo, hi]
        cols += [hi, lo]
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    o = np.lexsort((cols, rows))
    rows, cols = rows[o], cols[o]
    va = rng.uniform(-1, 1, len(rows)) * 0.9 / 6                              # at most 6 off-diagonals per row
    on = rows == cols
    va[on] = rng.uniform(1, 2, n) * rng.choice((-1.0, 1.0), n)
    rp = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n))]).astype(np.int32)
    return rp, cols.astype(np.int32), va, n


def triangle(rp, ci, va, n, uplo):
    """the kept triangle of a full matrix as its own CSR (stored order kept)"""
    rows = np.repeat(np.arange(n), np.diff(rp))
    keep = ci <= rows if uplo == LOWER else ci >= rows
    rp2 = np.concatenate([[0], np.cumsum(np.bincount(rows[keep], minlength=n))]).astype(np.int32)
    return rp2, ci[keep], va[keep], n


@functools.lru_cache(maxsize=None)
def matrix(name, uplo):
    """the named matrix in its LOWER or mirrored UPPER form"""
    if name == "stencil":
        return triangle(*stencil_full(), uplo)
    A = lower_matrix(name)
    return A if uplo == LOWER else mirror(*A)


def without_diagonal(rp, ci, va, n):
    rows = np.repeat(np.arange(n), np.diff(rp))
    keep = ci != rows
    rp2 = np.concatenate([[0], np.cumsum(np.bincount(rows[keep], minlength=n))]).astype(np.int32)
    return rp2, ci[keep], va[keep], n


def with_zero_diagonal(rp, ci, va, n):
    rows = np.repeat(np.arange(n), np.diff(rp))
    va = va.copy()
    va[ci == rows] = 0.0
    return rp, ci, va, n
