"""What the tests of spmv_mi355x_pcg_tri share (test_pcg_tri_abi.py on the CPU, test_gpu_pcg_tri.py and test_gpu_pcg_tri_sizes.py on
the GPU), on top of trsv_cases.py and trsv_blocked_cases.py, which are imported unchanged: the SPD grid problem, the numpy
restatement of the header's recurrences, the preconditioners as callables built on the C reference of the triangular solve
(tests/trsv_reference.c), and IC(0) in numpy. Nothing here touches the engine. Everything is computed once and is read-only.

The problem: spd_grid(45), n = 2025, cond_2 = 92.1 (asserted <= KAPPA = 100 from the eigenvalues), b = default_rng(7).uniform(-1, 1,
n). The restatement's iteration counts, tol 1e-12 in fp64 and 1e-5 in fp32 (COUNTS; recomputed in test_pcg_tri_abi.py):

      preconditioner            fp64   fp32
      none                       122     53
      Jacobi                     109     48
      blocked SGS, B = 64         69     30
      blocked SGS, B = 100        58     25
      blocked SGS, B = 256        50     22
      global SGS                  40     17
      IC(0)                       34     15
"""
import functools

import numpy as np

import trsv_blocked_cases as bc
import trsv_cases as tc
from trsv_cases import LOWER, UPPER

KAPPA = 100.0
POLL = 32
MAX_ITERATIONS = 400
BLOCKS = (64, 100, 256)
# the family's bounds (test_gpu_gmres.py, test_gpu_minres.py): the explicit norms against numpy's, |b|, and the history rows compared
PREC = {np.float64: dict(tol=1e-12, norms=1e-10, norms0=1e-13, ratio=1e-8, hist=1e-6, share=0.6),
        np.float32: dict(tol=1e-5, norms=1e-4, norms0=1e-6, ratio=1e-2, hist=1e-3, share=0.3)}
# the preconditioners by name: "none", "jacobi", a block size, "sgs" (global), "mixed" (global lower, blocked upper with B >= n), "ic0"
KINDS = ("none", "jacobi") + BLOCKS + ("sgs", "ic0")
COUNTS = {np.float64: dict(zip(KINDS, (122, 109, 69, 58, 50, 40, 34))), np.float32: dict(zip(KINDS, (53, 48, 30, 25, 22, 17, 15)))}
MIXED_B = 4096                # >= n: a blocked handle that drops nothing


@functools.lru_cache(maxsize=None)
def spd_grid(k=45):
    """(row_ptr, col_idx, values, n, dense) of the SPD operator on a k x k grid: 4.1 on the diagonal, -1 to all four neighbours, then
    scaled symmetrically, S A S with s = 1 + 0.2 default_rng(1).uniform(-1, 1, n). Columns ascending. (-1 s_i) s_j and (-1 s_j) s_i
    are the same product, so the matrix is symmetric to the bit."""
    n = k * k
    D = np.zeros((n, n))
    for i in range(k):
        for j in range(k):
            r = i * k + j
            D[r, r] = 4.1
            if j > 0:
                D[r, r - 1] = -1.0
            if j < k - 1:
                D[r, r + 1] = -1.0
            if i > 0:
                D[r, r - k] = -1.0
            if i < k - 1:
                D[r, r + k] = -1.0
    s = 1 + 0.2 * np.random.default_rng(1).uniform(-1, 1, n)
    D = (s[:, None] * D) * s[None, :]
    rows, cols = np.nonzero(D)
    rp = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n))]).astype(np.int32)
    out = (rp, cols.astype(np.int32), np.ascontiguousarray(D[rows, cols]), n, D)
    for a in (out[0], out[1], out[2], D):
        a.setflags(write=False)
    return out


def csr_of(D):
    """(row_ptr, col_idx, values) of the non-zeros of a dense matrix, columns ascending"""
    n = D.shape[0]
    rows, cols = np.nonzero(D)
    rp = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n))]).astype(np.int32)
    return rp, cols.astype(np.int32), np.ascontiguousarray(D[rows, cols])


def ic0(D):
    """the IC(0) factor of a dense SPD matrix: the lower triangular L with the pattern of D's lower triangle and (L L^t)_ij = D_ij on
    that pattern, row by row. Returns the dense L."""
    n = D.shape[0]
    L = np.zeros((n, n))
    for i in range(n):
        for j in np.nonzero(D[i, :i])[0]:
            L[i, j] = (D[i, j] - L[i, :j] @ L[j, :j]) / L[j, j]
        d = D[i, i] - L[i, :i] @ L[i, :i]
        assert d > 0, f"IC(0) breaks down at row {i}: pivot {d}"
        L[i, i] = np.sqrt(d)
    return L


def restate(A, b, M, tol, max_iterations, dtype):
    """the header's recurrences in numpy: vectors in `dtype`, dots and scalars in fp64. A is anything with A @ v of `dtype`, M the
    callable of "M^-1 v" (None: z = r). Returns (x, history, stop)."""
    dt = np.dtype(dtype).type
    dot = lambda u, v: float(u.astype(np.float64) @ v.astype(np.float64))
    pos = lambda v: np.isfinite(v) and v > 0
    b = b.astype(dt)
    x = np.zeros(len(b), dt)
    r = b.copy()
    rnorm0 = np.sqrt(dot(b, b))
    if rnorm0 == 0:
        return x, np.zeros(0), 3
    if not np.isfinite(rnorm0):
        return x, np.zeros(0), 4
    z = r if M is None else M(r)
    p = z.copy()
    rz = dot(r, z)
    if not pos(rz):
        return x, np.zeros(0), 4
    hist, stop = [], 2
    for _ in range(max_iterations):
        q = A @ p
        pq = dot(p, q)
        if not pos(pq):
            stop = 4
            break
        alpha = dt(rz / pq)
        x = x + alpha * p
        r = r - alpha * q
        rr = dot(r, r)
        hist.append(np.sqrt(rr))
        if tol > 0 and np.sqrt(rr) <= tol * rnorm0:
            stop = 1
            break
        if rr == 0:
            stop = 5
            break
        z = r if M is None else M(r)
        rz_new = dot(r, z)
        if not pos(rz_new):
            stop = 4
            break
        beta = dt(rz_new / rz)
        rz = rz_new
        p = z + beta * p
    return x, np.array(hist), stop


def cancellation_floor(P, x, dtype):
    """test_gpu_gmres.py's: how far two correct evaluations of |b - A x| for the same x can lie apart, to first order in the unit
    roundoffs of the handle's precision and of numpy's fp64. P has D (dense or scipy.sparse), b and k_row."""
    u, u64, store = float(np.finfo(dtype).eps) / 2, 2.0 ** -53, int(np.dtype(dtype) == np.float32)
    x = np.abs(x.astype(np.float64))
    k = P.k_row
    ax, bn = np.linalg.norm(abs(P.D) @ x), np.linalg.norm(P.b)
    return (u * (k + store + 1) + u64 * (k + 1)) * ax + (u * (1 + store) + u64) * bn


def shares_of_the_bounds(P, got, dtype, want=None, kappa=KAPPA):
    """the figures of one solve, each as a share of its bound (<= 1 passes): the explicit norms of the returned x and |b| against
    numpy's; with `want` (the solution) also rnorm <= 10 tol |b| and |x - want| / |want| <= kappa 10 tol"""
    lim = PREC[dtype]
    bn = np.linalg.norm(P.b)
    x = got["x"].astype(np.float64)
    rn, xn = np.linalg.norm(P.b - P.D @ x), np.linalg.norm(x)
    floor_r = cancellation_floor(P, got["x"], dtype)
    bt = np.linalg.norm(P.b.astype(dtype).astype(np.float64))
    out = dict(rnorm_np=abs(got["rnorm"] - rn) / (lim["norms"] * rn + floor_r),
               xnorm_np=abs(got["xnorm"] - xn) / (lim["norms"] * xn) if xn else float(got["xnorm"] != 0),
               rnorm0_np=abs(got["rnorm0"] - bt) / (lim["norms0"] * bt))
    if want is not None:
        out["rnorm"] = got["rnorm"] / (10 * lim["tol"] * bn)
        out["x"] = np.linalg.norm(x - want) / np.linalg.norm(want) / (kappa * 10 * lim["tol"])
    return out


def tri_apply(lower, scale, upper, dtype):
    """v -> upper^-1 (scale o (lower^-1 v)) in `dtype` by the C reference: lower / upper are (rp, ci, va, n) or None, scale an array
    or None"""
    def M(v):
        z = v if lower is None else tc.reference(*lower, LOWER, False, v, dtype)
        if scale is not None:
            z = (scale.astype(dtype) * z).astype(dtype)
        return z if upper is None else tc.reference(*upper, UPPER, False, z, dtype)
    return M


class Problem:
    def __init__(self, k=45):
        rp, ci, va, n, D = spd_grid(k)
        self.n, self.D, self.csr = n, D, (rp, ci, va)
        assert np.array_equal(D, D.T), "symmetric to the bit"
        assert np.all(np.diff(ci)[np.diff(np.repeat(np.arange(n), np.diff(rp))) == 0] > 0), "columns ascending"
        self.k_row = int((D != 0).sum(axis=1).max())
        self.b = np.random.default_rng(7).uniform(-1, 1, n)
        self.diag = np.ascontiguousarray(np.diag(D))
        self.b.setflags(write=False)
        self.diag.setflags(write=False)

    @functools.lru_cache(maxsize=None)
    def solve(self):
        ev = np.linalg.eigvalsh(self.D)
        assert ev[0] > 0 and ev[-1] / ev[0] <= KAPPA, ev[-1] / ev[0]
        x = np.linalg.solve(self.D, self.b)
        x.setflags(write=False)
        return x

    @functools.lru_cache(maxsize=None)
    def cond(self):
        ev = np.linalg.eigvalsh(self.D)
        return float(ev[-1] / ev[0])

    @functools.lru_cache(maxsize=None)
    def dense(self, dtype, negated=False):
        A = (-self.D if negated else self.D).astype(dtype)
        A.setflags(write=False)
        return A

    @functools.lru_cache(maxsize=None)
    def ic0(self):
        """(L, csr of L, csr of L^t): the caller's IC(0) factors"""
        L = ic0(self.D)
        L.setflags(write=False)
        return L, csr_of(L), csr_of(np.ascontiguousarray(L.T))

    def apply(self, kind, dtype):
        """the callable of M^-1 for a kind of KINDS (or "mixed"), None for "none" """
        rp, ci, va = self.csr
        if kind == "none":
            return None
        if kind == "jacobi":
            return lambda v, d=(1.0 / self.diag).astype(dtype): d * v
        if kind == "ic0":
            _, lo, up = self.ic0()
            return tri_apply(lo + (self.n,), None, up + (self.n,), dtype)
        if kind == "sgs":
            return bc.sgs_apply(rp, ci, va, self.n, None, dtype)
        if kind == "mixed":
            return bc.sgs_apply(rp, ci, va, self.n, None, dtype, MIXED_B)
        return bc.sgs_apply(rp, ci, va, self.n, kind, dtype)

    @functools.lru_cache(maxsize=None)
    def restatement(self, dtype, kind, tol, max_iterations=MAX_ITERATIONS):
        x, hist, stop = restate(self.dense(dtype), self.b, self.apply(kind, dtype), tol, max_iterations, dtype)
        x.setflags(write=False)
        hist.setflags(write=False)
        return x, hist, stop


@functools.lru_cache(maxsize=None)
def problem():
    return Problem()
