"""What the tests of the blocked triangular solve and of its GMRES caller share (test_trsv_blocked_abi.py, test_gpu_trsv_blocked.py,
test_gmres_tri_abi.py, test_gpu_gmres_tri.py), on top of trsv_cases.py, which is imported unchanged: the CSR with the dropped entries
removed, the numpy restatement of the blocked analysis of include/spmv_mi355x.h, one larger matrix, and the convection-diffusion
problem of the GMRES tests.

The blocked rule: block b owns the rows [b B, min(n, (b + 1) B)); an off-diagonal entry (i, j) of the chosen triangle is kept when
j // B == i // B. filtered() removes EVERY off-diagonal entry whose column lies in another block, those of the other triangle included:
the reference ignores that triangle anyway. A filtered matrix has no dependency between blocks, so trsv_cases.levels_of on it gives the
level of every row within its block, and trsv_cases.reference on it is what the blocked handle must return, bit for bit."""
import functools

import numpy as np

import trsv_cases as tc
from trsv_cases import LOWER, UPPER

BLOCK_ROWS_MAX = 16384


def filtered(rp, ci, va, n, B):
    """the CSR without the off-diagonal entries that couple two blocks of B rows (stored order kept)"""
    rows = np.repeat(np.arange(n), np.diff(rp))
    keep = (ci == rows) | (ci // B == rows // B)
    rp2 = np.concatenate([[0], np.cumsum(np.bincount(rows[keep], minlength=n))]).astype(np.int32)
    return rp2, ci[keep], va[keep], n


def dropped_of(rp, ci, n, uplo, B):
    """off-diagonal entries of the chosen triangle that cross a block boundary"""
    rows = np.repeat(np.arange(n), np.diff(rp))
    tri = ci < rows if uplo == LOWER else ci > rows
    return int(np.sum(tri & (ci // B != rows // B)))


def analysis_of(rp, ci, n, uplo, B):
    """the blocked analysis restated: dict(level_of_row, blocks, max_block_levels, max_level_rows, nnz_dropped)"""
    f = filtered(rp, ci, np.zeros(len(ci)), n, B)
    level = tc.levels_of(f[0], f[1], n, uplo)
    blocks = -(-n // B)
    if n == 0:
        return dict(level_of_row=level, blocks=0, max_block_levels=0, max_level_rows=0, nnz_dropped=0)
    # (block, level) pairs, counted
    key = (np.arange(n) // B).astype(np.int64) * (int(level.max()) + 1) + level
    return dict(level_of_row=level, blocks=blocks, max_block_levels=int(level.max()) + 1, max_level_rows=int(np.bincount(key).max()),
                nnz_dropped=dropped_of(rp, ci, n, uplo, B))


@functools.lru_cache(maxsize=None)
def big_dag(uplo):
    """20000 rows in the style of trsv_cases' dag: 0-8 columns among j < i, half of them within 4 of i. At B = 16384 a full block of
    128 KiB of fp64 LDS is followed by a short one."""
    n = 20000
    rng = np.random.default_rng(20000)
    deps = [[]]
    for i in range(1, n):
        k = rng.integers(0, 9)
        near = rng.integers(max(0, i - 4), i, k)
        far = rng.integers(0, i, k)
        deps.append(list(np.where(rng.random(k) < 0.5, near, far)))
    A = tc.assemble(n, deps, rng)
    return A if uplo == LOWER else tc.mirror(*A)


@functools.lru_cache(maxsize=None)
def matrix(name, uplo):
    return big_dag(uplo) if name == "big_dag" else tc.matrix(name, uplo)


# ---- the GMRES problem ---------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def convdiff(k=45):
    """(row_ptr, col_idx, values, n, dense) of the convection-diffusion operator on a k x k grid: row r = i k + j holds 4.1 on the
    diagonal, west -1.6, east -0.4, south -1.3, north -0.7, and is then multiplied by 1 + 0.2 u_r, u = default_rng(1).uniform(-1, 1,
    (n, 1)). Columns ascending."""
    n = k * k
    D = np.zeros((n, n))
    for i in range(k):
        for j in range(k):
            r = i * k + j
            D[r, r] = 4.1
            if j > 0:
                D[r, r - 1] = -1.6
            if j < k - 1:
                D[r, r + 1] = -0.4
            if i > 0:
                D[r, r - k] = -1.3
            if i < k - 1:
                D[r, r + k] = -0.7
    D *= 1 + 0.2 * np.random.default_rng(1).uniform(-1, 1, (n, 1))
    rows, cols = np.nonzero(D)
    rp = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n))]).astype(np.int32)
    out = (rp, cols.astype(np.int32), np.ascontiguousarray(D[rows, cols]), n, D)
    for a in (out[0], out[1], out[2], D):
        a.setflags(write=False)
    return out


def sgs_apply(rp, ci, va, n, B, dtype, B_upper="same"):
    """v -> U^-1 (diag(A) o (L^-1 v)) in `dtype`: the SGS of A by the C reference, L on the CSR filtered with B and U on the one
    filtered with B_upper (default: B; None: nothing filtered, the global triangle). The callable the GMRES restatement takes for
    "M v"."""
    B_upper = B if isinstance(B_upper, str) else B_upper
    lo = (rp, ci, va, n) if B is None else filtered(rp, ci, va, n, B)
    up = (rp, ci, va, n) if B_upper is None else filtered(rp, ci, va, n, B_upper)
    rows = np.repeat(np.arange(n), np.diff(rp))
    d = va[ci == rows].astype(dtype)
    assert len(d) == n

    def M(v):
        z = tc.reference(*lo, LOWER, False, v, dtype)
        z = (d * z).astype(dtype)
        return tc.reference(*up, UPPER, False, z, dtype)
    return M
