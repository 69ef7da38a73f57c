"""What the two tiers of the Jacobi-sweep triangular solve tests share (test_trsv_sweeps_abi.py, test_gpu_trsv_sweeps.py), on top of
trsv_cases.py, trsv_blocked_cases.py and pcg_tri_cases.py, which are imported unchanged: the C reference of
tests/trsv_sweeps_reference.c, the depth of every test matrix, and the swept SGS / IC(0) / ILU(0) preconditioners as callables for
the restatements. Nothing here touches the engine. Everything is computed once and is read-only.

The operation (include/spmv_mi355x.h "JACOBI SWEEPS"): x(1) = D^-1 b, x(m + 1) = D^-1 (b - N x(m)) for T = D + N. From `levels`
sweeps on the result has the bits of the exact solve (trsv_cases.reference): asserted in test_trsv_sweeps_abi.py.

CG on pcg_tri_cases.problem() (spd_grid(45), 89 levels) at PREC[dtype]["tol"], iterations of pcg_tri_cases.restate with the swept
reference as M^-1, the same sweep count on both triangles (COUNTS; recomputed in test_trsv_sweeps_abi.py):

      sweeps        1     2     4   >= 89
      fp64 SGS     109    58    42    40
      fp64 IC(0)   109    57    37    34
      fp32 SGS      48    25    18    17
      fp32 IC(0)    48    25    16    15
"""
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
MATRICES = ("one", "diagonal", "prescribed", "padding", "dag", "stencil")
SWEEPS_MAX = 1 << 20
CG_SWEEPS = (1, 2, 4, 89)
COUNTS = {np.float64: {"sgs": dict(zip(CG_SWEEPS, (109, 58, 42, 40))), "ic0": dict(zip(CG_SWEEPS, (109, 57, 37, 34)))},
          np.float32: {"sgs": dict(zip(CG_SWEEPS, (48, 25, 18, 17))), "ic0": dict(zip(CG_SWEEPS, (48, 25, 16, 15)))}}


@functools.lru_cache(maxsize=None)
def reference_lib():
    out = os.path.join(tempfile.mkdtemp(prefix="trsv_sweeps_reference_"), "trsv_sweeps_reference.so")
    subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-shared", "-fPIC", os.path.join(ROOT, "tests", "trsv_sweeps_reference.c"),
                    "-o", out, "-lm"], check=True)
    return ctypes.CDLL(out)


def reference(rp, ci, va, n, uplo, unit, b, dtype, sweeps):
    """x(sweeps) of the sequential restatement in `dtype`; va is narrowed to dtype first, as the handle narrows it"""
    assert sweeps >= 1
    dtype = np.dtype(dtype)
    rp = np.ascontiguousarray(rp, np.int32)
    ci = np.ascontiguousarray(ci, np.int32)
    va = np.ascontiguousarray(np.asarray(va, np.float64).astype(dtype))
    b = np.ascontiguousarray(b, dtype)
    x = np.full(max(n, 1), np.nan, dtype)
    w = np.full(max(n, 1), np.nan, dtype)
    fn = reference_lib().trsv_sweeps_reference_f64 if dtype == np.float64 else reference_lib().trsv_sweeps_reference_f32
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    fn(ctypes.c_int(uplo), ctypes.c_int(1 if unit else 0), ctypes.c_long(n), p(rp), p(ci), p(va), ctypes.c_long(sweeps), p(b), p(x), p(w))
    return x[:n]


@functools.lru_cache(maxsize=None)
def depth(name, uplo, B=None):
    """`levels` of trsv_info for a named matrix: the depth of the dependency graph, within the blocks of B rows when B is given"""
    A = bc.matrix(name, uplo)
    if A[3] == 0:
        return 0
    M = A if B is None else bc.filtered(*A, B)
    return int(tc.levels_of(M[0], M[1], M[3], uplo).max()) + 1


@functools.lru_cache(maxsize=None)
def rhs(n, dtype, seed=5):
    b = np.random.default_rng(seed).uniform(-1, 1, n).astype(dtype)
    b.setflags(write=False)
    return b


def sweep_counts(name, levels):
    """the sweep counts of the GPU bit tests: around 1 and around `levels`; the 708 levels of dag get a shorter list"""
    if name == "dag":
        return (1, 2, 5, levels)
    return tuple(sorted({s for s in (1, 2, 3, 5, levels - 1, levels, levels + 3) if s >= 1}))


# ---- the swept preconditioners, for the restatements -------------------------------------------------------------------------------------

def swept_tri_apply(lower, lower_unit, scale, upper, dtype, sweeps):
    """v -> upper~^-1 (scale o (lower~^-1 v)) in `dtype`, each ~^-1 the sweep reference with the same count: lower / upper are
    (rp, ci, va, n), scale an array or None"""
    def M(v):
        z = reference(*lower, LOWER, lower_unit, v, dtype, sweeps)
        if scale is not None:
            z = (scale.astype(dtype) * z).astype(dtype)
        return reference(*upper, UPPER, False, z, dtype, sweeps)
    return M


def cg_apply(kind, dtype, sweeps):
    """M^-1 of the swept SGS ("sgs": L~^-1, diag(A), U~^-1 over A's own CSR) or the swept IC(0) triple ("ic0") on pcg_tri_cases.problem()"""
    P = pc.problem()
    rp, ci, va = P.csr
    if kind == "sgs":
        A = (rp, ci, va, P.n)
        return swept_tri_apply(A, False, P.diag, A, dtype, sweeps)
    _, lo, up = P.ic0()
    return swept_tri_apply(lo + (P.n,), False, None, up + (P.n,), dtype, sweeps)


@functools.lru_cache(maxsize=None)
def cg_restatement(dtype, kind, sweeps):
    """(x, history, stop) of pcg_tri_cases.restate under the swept preconditioner at PREC[dtype]["tol"]"""
    P = pc.problem()
    x, hist, stop = pc.restate(P.dense(dtype), P.b, cg_apply(kind, dtype, sweeps), pc.PREC[dtype]["tol"], pc.MAX_ITERATIONS, dtype)
    x.setflags(write=False)
    hist.setflags(write=False)
    return x, hist, stop
