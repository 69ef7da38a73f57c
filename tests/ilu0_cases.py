"""What the two tiers of the ILU(0) tests share (test_ilu0_abi.py on the CPU, test_gpu_ilu0.py on the GPU), on top of trsv_cases.py,
trsv_blocked_cases.py and pcg_tri_cases.py, which are imported unchanged: the C reference of tests/ilu0_reference.c, a dense numpy
restatement of the same loop, the test matrices, and the preconditioner M^-1 v = U^-1 (L^-1 v) as a callable built on the C reference
of the triangular solve (LOWER / UNIT of f, no scale, UPPER / STORED of f). Nothing here touches the engine. Everything is computed
once and is read-only.

Every matrix comes as (row_ptr, col_idx, values, n) with columns strictly ascending and a stored diagonal in every row."""
import ctypes
import functools
import os
import subprocess
import tempfile

import numpy as np

import pcg_tri_cases as pc
import trsv_blocked_cases as bc
import trsv_cases as tc
from trsv_cases import LOWER, UPPER

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLOCKS = (64, 100, 256)
# the restatement's iteration counts on spd_grid(45) under ILU(0), tol 1e-12 in fp64 and 1e-5 in fp32; None is the global form, whose
# counts are pcg_tri_cases.COUNTS["ic0"] (recomputed in test_ilu0_abi.py)
COUNTS = {np.float64: {None: 34, 64: 68, 100: 55, 256: 46}, np.float32: {None: 15, 64: 29, 100: 24, 256: 20}}


# ---- the reference -------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def reference_lib():
    out = os.path.join(tempfile.mkdtemp(prefix="ilu0_reference_"), "ilu0_reference.so")
    subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-shared", "-fPIC", os.path.join(ROOT, "tests", "ilu0_reference.c"), "-o", out,
                    "-lm"], check=True)
    lib = ctypes.CDLL(out)
    lib.ilu0_reference.restype = ctypes.c_long
    return lib


def reference(rp, ci, va, n, B=None):
    """(f, breakdown_row) of the sequential loop; B = None is the global form"""
    rp = np.ascontiguousarray(rp, np.int32)
    ci = np.ascontiguousarray(ci, np.int32)
    va = np.ascontiguousarray(va, np.float64)
    f = np.full(max(len(va), 1), np.nan)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    with np.errstate(all="ignore"):
        bad = reference_lib().ilu0_reference(ctypes.c_long(n), p(rp), p(ci), p(va), ctypes.c_long(B or 0), p(f))
    return f[:len(va)], int(bad)


def restatement(D, B=None):
    """the same loop on a dense matrix in numpy, the pattern being D != 0 (within the blocks of B rows when B is given): the dense F
    with unit L strictly below the diagonal and U on and above it; outside the pattern F keeps D. No fma: close to the reference,
    not equal."""
    n = D.shape[0]
    F = D.copy()
    S = D != 0
    if B is not None:
        blk = np.arange(n) // B
        S &= blk[:, None] == blk[None, :]
    cols = np.arange(n)
    for i in range(n):
        for k in np.nonzero(S[i, :i])[0]:
            F[i, k] = F[i, k] / F[k, k]
            js = np.nonzero(S[i] & S[k] & (cols > k))[0]
            F[i, js] -= F[i, k] * F[k, js]
    return F


def dense_of(rp, ci, va, n):
    D = np.zeros((n, n))
    D[np.repeat(np.arange(n), np.diff(rp)), ci] = va
    return D


# ---- matrices ------------------------------------------------------------------------------------------------------------------------

def _frozen(rp, ci, va, n):
    out = (np.ascontiguousarray(rp, np.int32), np.ascontiguousarray(ci, np.int32), np.ascontiguousarray(va, np.float64), n)
    for a in out[:3]:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def matrix(name):
    if name == "spd_grid":
        return _frozen(*pc.spd_grid(45)[:4])
    if name == "convdiff":
        return _frozen(*bc.convdiff(45)[:4])
    if name == "dense70":                                 # rows wider than a wave, every k step feeds the next: ILU(0) is LU
        n = 70
        D = np.random.default_rng(3).uniform(-1, 1, (n, n))
        D[np.arange(n), np.arange(n)] = 40.0
        return _frozen(np.arange(n + 1) * n, np.tile(np.arange(n), n), D.ravel(), n)
    if name == "arrow":                                   # two levels: 599 rows of two entries, one row of 600 entries and 599 k steps
        n = 600
        rp = np.concatenate([[0], 2 * np.arange(1, n), [2 * (n - 1) + n]])
        ci = np.concatenate([np.column_stack([np.arange(n - 1), np.full(n - 1, n - 1)]).ravel(), np.arange(n)])
        va = np.concatenate([np.column_stack([np.full(n - 1, 600.0), np.full(n - 1, -1.0)]).ravel(), np.full(n - 1, -1.0), [600.0]])
        return _frozen(rp, ci, va, n)
    if name == "random":                                  # 300 rows, 0-8 entries beside the diagonal anywhere in the row
        n = 300
        rng = np.random.default_rng(300)
        rp, ci, va = [0], [], []
        for i in range(n):
            k = 0 if i % 7 == 3 else rng.integers(0, 9)
            c = np.unique(np.append(rng.integers(0, n, k), i))
            a = rng.uniform(-1, 1, len(c))
            a[c == i] = np.abs(a[c != i]).sum() + rng.uniform(0.5, 1.5)          # strictly diagonally dominant
            ci.append(c)
            va.append(a)
            rp.append(rp[-1] + len(c))
        return _frozen(rp, np.concatenate(ci), np.concatenate(va), n)
    if name in ("pairs", "pairs_long"):                   # two levels of n / 2 rows: row 2m + 1 stores (2m, 2m + 1), row 2m its diagonal
        n = 70000 if name == "pairs" else 300000
        rng = np.random.default_rng(n)
        odd = np.arange(n) % 2 == 1
        rp = np.concatenate([[0], np.cumsum(np.where(odd, 2, 1))])
        ci = np.empty(rp[-1], np.int64)
        va = np.empty(rp[-1])
        dia = rp[1:] - 1
        ci[dia] = np.arange(n)
        va[dia] = rng.uniform(1, 2, n)
        ci[dia[odd] - 1] = np.arange(n)[odd] - 1
        va[dia[odd] - 1] = rng.uniform(-1, 1, n // 2)
        return _frozen(rp, ci, va, n)
    if name == "empty":
        return _frozen(np.zeros(1), np.zeros(0), np.zeros(0), 0)
    if name == "one":
        return _frozen([0, 1], [0], [2.5], 1)
    raise KeyError(name)


def singular():
    """[[1, 1], [1, 1]]: f = (1, 1, 1, 0), the pivot of row 1 is zero"""
    return _frozen([0, 2, 4], [0, 1, 0, 1], [1.0, 1.0, 1.0, 1.0], 2)


@functools.lru_cache(maxsize=None)
def factor(name, B=None):
    """the reference factor of a named matrix, computed once"""
    f, bad = reference(*matrix(name), B)
    f.setflags(write=False)
    return f, bad


def kept(rp, ci, n, B):
    """the entries the factorization with block size B touches (all of them for B = None)"""
    rows = np.repeat(np.arange(n), np.diff(rp))
    return np.ones(len(ci), bool) if B is None else ci // B == rows // B


# ---- the preconditioner ------------------------------------------------------------------------------------------------------------------

def apply(rp, ci, f, n, B, dtype):
    """v -> U^-1 (L^-1 v) in `dtype` by the C reference of the triangular solve: L = LOWER / UNIT and U = UPPER / STORED of the one
    array f, on the CSR filtered with B when B is given. The callable the restatements take for "M^-1 v"."""
    T = (rp, ci, f, n) if B is None else bc.filtered(rp, ci, f, n, B)

    def M(v):
        return tc.reference(*T, UPPER, False, tc.reference(*T, LOWER, True, v, dtype), dtype)
    return M


@functools.lru_cache(maxsize=None)
def pcg_restatement(dtype, B, tol, max_iterations=pc.MAX_ITERATIONS):
    """(x, history, stop) of pcg_tri_cases.restate on spd_grid(45) under the reference ILU(0)"""
    P = pc.problem()
    rp, ci, va, n = matrix("spd_grid")
    x, hist, stop = pc.restate(P.dense(dtype), P.b, apply(rp, ci, factor("spd_grid", B)[0], n, B, dtype), tol, max_iterations, dtype)
    x.setflags(write=False)
    hist.setflags(write=False)
    return x, hist, stop
