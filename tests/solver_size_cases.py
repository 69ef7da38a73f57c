"""Systems, right-hand sides and references of test_gpu_solver_sizes.py (GPU) and test_solver_size_cases.py (CPU tier): the
sizes at which the launch shape and the two-stage dot products of csrc/solvers_common.hpp change.

Nothing here touches the engine. The references are the oracle (oracle/solver_oracle.c) for PCG / BiCGSTAB and the numpy
restatements of test_gpu_minres.py, test_gpu_gmres.py and test_gpu_cgls.py, which only ever take A @ v and so run on the
scipy.sparse matrices below unchanged. Everything is computed once per (system, precision, parameters) and is read-only."""
import functools

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as sla

from test_gpu_cgls import restate as cgls_restate
from test_gpu_gmres import restate as gmres_restate
from test_gpu_minres import restate as minres_restate

# csrc/solvers_common.hpp, restated: a change there must fail test_solver_size_cases.py, not empty the tests
VB = 256                      # threads per block of the vector kernels
MAX_PART = 1024               # partial sums per quantity = the cap of the grid
PER_THREAD = 4                # elements of a thread before the cap binds
BLOCK_ROWS = PER_THREAD * VB  # 1024


def solver_blocks(length):
    """solver_blocks() of csrc/solvers_common.hpp: blocks of every vector kernel over `length` elements = partials per slot"""
    return min(MAX_PART, max(1, -(-length // BLOCK_ROWS)))


N1 = VB * BLOCK_ROWS + 1                    # 262 145: nb = 257, the partial loop's second trip (thread 0 alone, partial 256)
N2 = (MAX_PART + 1) * BLOCK_ROWS + 1        # 1 049 601 = 1025 * 1024 + 1: nb capped, the grid stride's 5th trip
LO1 = VB * BLOCK_ROWS                       # 262 144: the most elements with nb <= VB
LO2 = MAX_PART * BLOCK_ROWS                 # 1 048 576: the most elements without a 5th trip = the first row of the 5th trip at N2
FAR = 131071                                # the far band of spd / nsym
LSQ_SHORT = BLOCK_ROWS + 1                  # 1025: the short side of the CGLS shapes, 2 blocks
LSQ_TALL, LSQ_WIDE = (N1, LSQ_SHORT), (LSQ_SHORT, N1)
DIST_N, DIST_WORLD = 530000, 2              # both row blocks hold more than LO1 rows
KMAX = 9                                    # columns of the multi-RHS cases
MINRES_CASES = ((0.3, False), (0.0, True))  # (shift, minv given)
GMRES_CASES = ((8, False), (20, True))      # (restart, minv given)
LSQ_DAMPS = (0.0, 0.1)
SHARE = {np.float64: 0.5, np.float32: 0.25}             # of the history rows must qualify for the relative comparison (MINRES, GMRES)
# CGLS converges in 7 / 5 (fp64) and 3 / 2 (fp32) iterations here: the rows that qualify, as they are (test_gpu_solver_sizes.py)
LSQ_ROWS = {(LSQ_TALL, np.float64): 4, (LSQ_TALL, np.float32): 1, (LSQ_WIDE, np.float64): 2, (LSQ_WIDE, np.float32): 0}


def block_of(i, grid):
    """GRID_STRIDE of csrc/solvers_common.hpp: element i is thread i % (grid * VB) of the grid, on trip i // (grid * VB); its product
    goes into the partial of that thread's block. Elements are dealt to the blocks VB at a time, round and round: never i / 1024."""
    return (np.asarray(i) % (grid * VB)) // VB


def tail_rows(length, grid=None):
    """The elements of a vector of `length` values that only the new paths touch, in a grid of `grid` blocks (solver_blocks(length)
    unless the solver runs one grid for two lengths): with a 5th trip of the grid stride, the elements of that trip; else the
    elements whose partial lies past index VB - 1, which the second stage picks up on a second trip. May be empty."""
    grid = grid or solver_blocks(length)
    i = np.arange(length)
    if length > PER_THREAD * grid * VB:
        return i[PER_THREAD * grid * VB:]
    return i[block_of(i, grid) >= VB]


# ---- matrices ------------------------------------------------------------------------------------------------------------------------

def _bands(n, bands):
    offs = [o for o, _ in bands if abs(o) < n]
    A = sp.diags([np.full(n - abs(o), v) for o, v in bands if abs(o) < n], offs, shape=(n, n), format="csr", dtype=np.float64)
    A.sort_indices()
    A.indptr, A.indices = A.indptr.astype(np.int32), A.indices.astype(np.int32)
    return A


def spd(n):
    """symmetric, strictly diagonally dominant: eigenvalues in [1, 7]"""
    return _bands(n, [(-FAR, -0.5), (-1, -1.0), (0, 4.0), (1, -1.0), (FAR, -0.5)])


def stiff(n):
    """the 1-D Laplacian + 0.05 I: eigenvalues in (0.05, 4.05), CG needs more than RESTART_K = 100 iterations"""
    return _bands(n, [(-1, -1.0), (0, 2.05), (1, -1.0)])


def nsym(n):
    """nothing symmetric, strictly diagonally dominant (off-diagonal row sum 2.9 of 4)"""
    return _bands(n, [(-FAR, -0.2), (-1, -1.5), (0, 4.0), (1, -0.5), (FAR, -0.7)])


def lsq(m, n):
    """test_gpu_cgls.Problem's matrix in sparse form: per row up to min(6, n) entries at distinct random columns, uniform in
    (-0.5, 0.5) (6 draws, a repeated column kept once), then 4.0 added at (i % m, i % n) for i < max(m, n)."""
    rng = np.random.default_rng(1000 * m + n)
    k = min(6, n)
    cols, vals = rng.integers(0, n, (m, k)), rng.uniform(-0.5, 0.5, (m, k))
    order = np.argsort(cols, axis=1, kind="stable")
    cols, vals = np.take_along_axis(cols, order, 1), np.take_along_axis(vals, order, 1)
    keep = np.ones(cols.shape, bool)
    keep[:, 1:] = cols[:, 1:] != cols[:, :-1]
    rows = np.broadcast_to(np.arange(m)[:, None], cols.shape)
    i = np.arange(max(m, n))
    A = (sp.csr_matrix((vals[keep], (rows[keep], cols[keep])), shape=(m, n))
         + sp.csr_matrix((np.full(i.size, 4.0), (i % m, i % n)), shape=(m, n))).tocsr()
    A.sum_duplicates()
    A.sort_indices()
    A.indptr, A.indices = A.indptr.astype(np.int32), A.indices.astype(np.int32)
    return A


KINDS = dict(spd=spd, stiff=stiff, nsym=nsym)


def weigh_tail(b, rows):
    """scales b[rows] so that those rows together hold half of |b|^2 (no rows: b as it is)"""
    b = b.copy()
    if len(rows):
        tail = np.zeros(b.size, bool)
        tail[rows] = True
        b[tail] *= np.sqrt((b[~tail] ** 2).sum() / (b[tail] ** 2).sum())
    return b


def rhs(n, seed=11, rows=None):
    """default_rng(seed).uniform(0.5, 1.5, n) with `rows` (tail_rows(n) unless given) holding half of |b|^2"""
    b = np.random.default_rng(seed).uniform(0.5, 1.5, n)
    return weigh_tail(b, tail_rows(n) if rows is None else rows)


def preconditioner(A):
    """the MINRES / GMRES tests' minv_i = (1 / |d_ii|) (1 + 0.5 sin(i))"""
    return 1.0 / np.abs(A.diagonal()) * (1 + 0.5 * np.sin(np.arange(A.shape[0])))


class System:
    """One matrix with its right-hand side, shaped like the Problem classes of the solver test files where their helpers
    (explicit_norms, cancellation_floor) read it: D, b, k_row, k_col, norm2, minv."""

    def __init__(self, D, b, tail, minv=None, x_tail=None):
        self.D, self.b, self.tail, self.minv = D, b, tail, minv      # tail: the tail_rows of b; x_tail: those of x where they differ
        self.x_tail = tail if x_tail is None else x_tail
        self.m, self.n = D.shape
        self.k_row = int(np.diff(D.indptr).max())
        self.k_col = int(np.bincount(D.indices, minlength=self.n).max())
        for v in (b, D.data, D.indices, D.indptr) + (() if minv is None else (minv,)):
            v.setflags(write=False)

    @functools.cached_property
    def norm2(self):
        return float(sla.svds(self.D, k=1, return_singular_vectors=False, tol=1e-6)[0]) * (1 + 1e-5)

    @functools.cached_property
    def Dt(self):
        return self.D.T.tocsr()

    def handle(self, eng, fmt, dtype, **opts):
        return eng.Matrix(self.D.indptr, self.D.indices, self.D.data, self.m, self.n, fmt, dtype, **opts)

    def pre(self, given):
        return self.minv if given else None

    @functools.lru_cache(maxsize=None)
    def cast(self, dtype):
        return self.D.astype(dtype), (None if self.m == self.n else self.Dt.astype(dtype))


@functools.lru_cache(maxsize=None)
def system(kind, n):
    A = KINDS[kind](n)
    return System(A, rhs(n), tail_rows(n), preconditioner(A))


@functools.lru_cache(maxsize=None)
def lsq_system(m, n):
    grid = max(solver_blocks(m), solver_blocks(n))        # one grid for both lengths: the short side has no tail rows
    return System(lsq(m, n), rhs(m, rows=tail_rows(m, grid)), tail_rows(m, grid), x_tail=tail_rows(n, grid))


@functools.lru_cache(maxsize=None)
def columns(n, k=KMAX):
    """test_gpu_solver_multi._columns' seeds without its eigenvector column, each column with the tail weighting"""
    B = np.ascontiguousarray(np.stack([rhs(n, 11 + j) for j in range(k)], axis=1))
    B.setflags(write=False)
    return B


def dist_tail(offsets):
    """per rank, the global rows whose partial in that rank's own grid lies past index VB - 1"""
    return [int(offsets[r]) + tail_rows(int(offsets[r + 1] - offsets[r])) for r in range(len(offsets) - 1)]


def dist_rhs(offsets):
    """b of the distributed case: the tail rows of EVERY rank's block together hold half of |b|^2"""
    b = rhs(int(offsets[-1]), rows=np.concatenate(dist_tail(offsets)))
    b.setflags(write=False)
    return b


# ---- references (computed once, read-only) -------------------------------------------------------------------------------------------

def _frozen(r):
    for v in r.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return r


@functools.lru_cache(maxsize=None)
def oracle_solve(orc, method, kind, n, iters, seed=11, fp32=False, dist=False):
    """oracle.pcg / oracle.pbicgstab on KINDS[kind](n) with rhs(n, seed) (fp32: that b rounded to fp32, as the handle holds it)"""
    A = system(kind, n).D
    if dist:
        import spmv_dist
        b = dist_rhs(spmv_dist.row_partition(A.indptr, DIST_WORLD))
    else:
        b = rhs(n, seed)
    if fp32:
        b = b.astype(np.float32).astype(np.float64)
    return _frozen(getattr(orc, method)(A.indptr, A.indices, A.data, b, iters))


@functools.lru_cache(maxsize=None)
def minres_reference(kind, n, dtype, shift, given, tol, max_iterations=300):
    """(x, history, beta1, stop) of test_gpu_minres.restate"""
    S = system(kind, n)
    out = minres_restate(S.cast(dtype)[0], S.b, shift, S.pre(given), tol, max_iterations, dtype)
    out[0].setflags(write=False)
    out[1].setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def gmres_reference(kind, n, dtype, restart, given, tol, max_iterations=400):
    """(x, history, stop, restarts) of test_gpu_gmres.restate"""
    S = system(kind, n)
    out = gmres_restate(S.cast(dtype)[0], S.b, restart, S.pre(given), tol, max_iterations, dtype)
    out[0].setflags(write=False)
    out[1].setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def cgls_reference(m, n, dtype, damp, tol, max_iterations=300):
    """(x, history rows (|r|, |s|), |s0|) of test_gpu_cgls.restate"""
    S = lsq_system(m, n)
    A, At = S.cast(dtype)
    out = cgls_restate(A, At, S.b, damp, tol, max_iterations, dtype)
    out[0].setflags(write=False)
    out[1].setflags(write=False)
    return out


def pcg_restate(A, b, max_iterations, dot=None):
    """orc_pcg_f64 of oracle/solver_oracle.c in numpy, for max_iterations <= RESTART_K = 100 (no explicit check inside the loop),
    with a replaceable dot product. Returns (x, history rows (error, error_explicit, error_best), iterations): what
    oracle.pcg returns as x, history, iterations."""
    assert max_iterations <= 100
    dot = dot or (lambda u, v: float(u @ v))
    K = A.diagonal()
    x, r = np.zeros(len(b)), b.copy()
    z = r / K
    p = z.copy()
    err0 = np.sqrt(dot(r, r))
    eps = 1e-15 * np.sqrt(dot(b, b))
    hist, k = [], 0
    while k < max_iterations:
        err = np.sqrt(dot(r, r))
        if err < eps:
            break
        hist.append((err, err0, err0))
        Ap = A @ p
        zr = dot(z, r)
        ak = zr / dot(p, Ap)
        x = x + ak * p
        r = r - ak * Ap
        z = r / K
        p = z + (dot(z, r) / zr) * p
        k += 1
    e = b - A @ x
    return (x if np.sqrt(dot(e, e)) < err0 else np.zeros(len(b))), np.array(hist).reshape(-1, 3), k


def losing_dot(n, rows):
    """the fp64 dot product of the restatements over vectors of n values without `rows`: with rows = tail_rows(n), what a dropped
    partial past index VB - 1 (N1: partial 256) or a skipped 5th trip of the grid stride (N2) computes"""
    keep = np.ones(n, bool)
    keep[rows] = False
    return lambda u, v: float(u[keep].astype(np.float64) @ v[keep].astype(np.float64))


def permuted(A, *vectors, seed=5):
    """a symmetric random permutation of a square system: (P A P^t, P v ..., perm). The same problem in another summation order."""
    perm = np.random.default_rng(seed).permutation(A.shape[0])
    B = A[perm][:, perm].tocsr()
    B.sort_indices()
    B.indptr, B.indices = B.indptr.astype(np.int32), B.indices.astype(np.int32)
    return (B,) + tuple(None if v is None else v[perm] for v in vectors) + (perm,)
