"""What the two tiers of the tests of spmv_mi355x_amg_create_with share (test_amg_prolongator_abi.py on the CPU,
test_gpu_amg_prolongator.py on the GPU): the cases and their variants, the C reference of tests/amg_prolongator_reference.c (steps 5a
to 5c of include/spmv_mi355x.h "AMG: a caller's near-null vector and filtered prolongator smoothing" as sequential loops, gcc -O2
-ffp-contract=off), a scipy restatement of those steps with arithmetic of its own (boolean masks and row sums for the filter,
np.bincount for the aggregate norms, scipy's products for P and P^t A P), and the recorded counts and bounds. Nothing here touches the
engine. Everything is computed once and is read-only.

A case is (name, variant). The variants:
      "filtered"   the operator of amg_cases.case(name), filtered = 1
      "nn"         S A S of it with s = 1 + 0.5 U(-1, 1) (seed 25, entry order kept), near_null = 1 / s
      "both"       the scaled operator with both
on `grid`, `aniso` (every level-0 row has weak entries to lump), `isolated`, `unsorted`, `n129`, `one` and `empty` of amg_cases, and
      ("path_wrap", "nn")   path_wrap as it is, with near_null = 1 / s of its own s = 1 + 0.2 U(-1, 1): 262 144 + 37 rows send the
                            first workgroup of every new kernel into a second trip on level 0
      ("hub", "filtered"), ("hub", "both")   the 20 x 20 five-point operator with 5.0 on the diagonal whose row 0 is also coupled
                            symmetrically by -0.11 to 46 nodes that are not its grid neighbours. All 46 are weak (0.0121 against
                            theta^2 d_i d_j = 0.16) and sum to -5.06 against 5.0: row 0 must fall back to all its entries. The
                            matrix is SPD since 0.11 sqrt(46) < 1.

THE COUNTS (recomputed in test_amg_prolongator_abi.py). pcg_tri_cases.restate to PATH_TOL = 1e-8 in fp64 with M^-1 = one V(1, 1)
cycle of the reference's hierarchy:
      path_wrap, as amg_create builds it          76   (amg_cases.PATH_COUNT; 6 levels, stalls at 272 rows, sweeps)
      path_wrap, near_null = 1 / s                PATH_NN_COUNT, at most 38 = half of it; PATH_NN_ROWS, a dense last level
      the scaled grid, as amg_create / "nn"       GRID_SCALED_COUNTS

THE BOUND OF THE CYCLE (CYCLE_MEASURED, CYCLE_BOUND; recomputed in the CPU tier), derived as amg_cases.CYCLE_BOUND is: ten times the
largest max-norm relative difference, over CYCLE_CASES and amg_cases.vectors(), between the restated cycle in fp64 and in longdouble
(for fp64 handles, measured 5.30e-16), in fp32 and in fp64 (for fp32 handles, measured 2.12e-7)."""
import ctypes
import functools
import os
import subprocess
import tempfile

import numpy as np
import scipy.sparse as sp

import amg_cases as ac
import pcg_tri_cases as pc

ROOT = ac.ROOT
VARIANTS = ("filtered", "nn", "both")
NAMES = ("grid", "aniso", "isolated", "unsorted", "n129", "one", "empty")
CASES = tuple((name, v) for name in NAMES for v in VARIANTS) + (("path_wrap", "nn"), ("hub", "filtered"), ("hub", "both"))
CYCLE_CASES = tuple(c for c in CASES if c[0] not in ("empty", "path_wrap", "unsorted"))
HUB_K, HUB_COUPLED, HUB_VALUE = 20, 46, -0.11
PATH_NN_COUNT, PATH_NN_ROWS = 29, [ac.PATH_ROWS, 61893, 14612, 3450, 815, 193, 47]
GRID_SCALED_COUNTS = {"default": 21, "nn": 18}
CYCLE_MEASURED = {np.float64: 5.3e-16, np.float32: 2.2e-7}
CYCLE_BOUND = {np.float64: 5.3e-15, np.float32: 2.2e-6}

_p = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
_freeze = ac._freeze


@functools.lru_cache(maxsize=None)
def base(name):
    """(row_ptr, col_idx, values, n, opts) of the unscaled operator"""
    if name != "hub":
        return ac.case(name)
    k = HUB_K
    I, E = sp.identity(k), sp.diags([-np.ones(k - 1), -np.ones(k - 1)], [-1, 1])
    A = (sp.kron(I, E) + sp.kron(E, I) + 5.0 * sp.identity(k * k)).tolil()
    far = [j for j in range(2, k * k) if j != k][::7][:HUB_COUPLED]       # neither 1 nor k, the grid neighbours of node 0
    assert len(far) == HUB_COUPLED
    for j in far:
        A[0, j] = A[j, 0] = HUB_VALUE
    return ac._csr(A.tocsr()) + (k * k, {})


@functools.lru_cache(maxsize=None)
def scaling(name):
    """s of the "nn" and "both" variants: path_wrap has its own"""
    n = base(name)[3]
    if name == "path_wrap":
        s = 1 + 0.2 * np.random.default_rng(2).uniform(-1, 1, n)
    else:
        s = 1 + 0.5 * np.random.default_rng(25).uniform(-1, 1, n)
    return _freeze(s)[0]


@functools.lru_cache(maxsize=None)
def case(name, variant):
    """(row_ptr, col_idx, values, n, opts, near_null or None, filtered)"""
    rp, ci, va, n, opts = base(name)
    filtered = variant in ("filtered", "both")
    if variant == "filtered":
        return rp, ci, va, n, opts, None, True
    s = scaling(name)
    if name != "path_wrap":                               # path_wrap is S A S already
        rows = np.repeat(np.arange(n), np.diff(rp))
        va, = _freeze(va * (s[rows] * s[ci]))
    return rp, ci, va, n, opts, _freeze(1.0 / s)[0], filtered


def options(name):
    return dict(ac.DEFAULTS, **base(name)[4])


def matrix(name, variant):
    rp, ci, va, n = case(name, variant)[:4]
    return sp.csr_matrix((va.copy(), ci.copy(), rp.copy()), (n, n))


# ---- the reference -------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def reference_lib():
    out = os.path.join(tempfile.mkdtemp(prefix="amg_prolongator_reference_"), "amg_prolongator_reference.so")
    subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-shared", "-fPIC", os.path.join(ROOT, "tests", "amg_prolongator_reference.c"), "-o",
                    out, "-lm"], check=True)
    lib = ctypes.CDLL(out)
    V, I, L, D = ctypes.c_void_p, ctypes.c_int, ctypes.c_long, ctypes.c_double
    lib.amg_prolongator_build.restype = V
    lib.amg_prolongator_build.argtypes = [L, V, V, V, D, I, I, I, V]
    lib.amg_prolongator_update.restype = V
    lib.amg_prolongator_update.argtypes = [V, V]
    for f in (lib.amg_prolongator_free, lib.amg_reference_levels, lib.amg_reference_stalled):
        f.argtypes = [V]
    lib.amg_prolongator_flags.argtypes = [V, V]
    lib.amg_reference_level.argtypes = [V, I, V, V]
    lib.amg_prolongator_level.argtypes = [V, I, V, V]
    lib.amg_reference_aggregates.argtypes = [V, I, V]
    lib.amg_reference_csr.argtypes = [V, I, I, V, V, V]
    lib.amg_prolongator_filtered_csr.argtypes = [V, I, V, V, V, V]
    lib.amg_prolongator_vectors.argtypes = [V, I, V, V]
    return lib


def _read(h):
    """the dict of amg_cases.reference with, per level, AF = (rp, ci, va) or None, map, nnz_f, unfiltered_rows, omega_p, rho_p, b, t;
    bad = (level, index) or None; "_h" is the C handle (kept alive: amg_prolongator_update reads it)"""
    lib = reference_lib()
    flags = np.zeros(4, np.int64)
    lib.amg_prolongator_flags(h, _p(flags))
    out = dict(levels=lib.amg_reference_levels(h), stalled=lib.amg_reference_stalled(h), lev=[], filtered=bool(flags[0]),
               has_nn=bool(flags[1]), bad=None if flags[2] < 0 else (int(flags[2]), int(flags[3])), _h=h)
    for l in range(out["levels"]):
        num, dbl, pnum, pdbl = np.zeros(5, np.int64), np.zeros(2), np.zeros(2, np.int64), np.zeros(2)
        lib.amg_reference_level(h, l, _p(num), _p(dbl))
        lib.amg_prolongator_level(h, l, _p(pnum), _p(pdbl))
        rows, nnz, nnz_p, aggregates, rounds = (int(v) for v in num)
        L = dict(n=rows, aggregates=aggregates, rounds=rounds, omega=float(dbl[0]), rho=float(dbl[1]), P=None, AF=None, map=None,
                 nnz_f=int(pnum[0]), unfiltered_rows=int(pnum[1]), omega_p=float(pdbl[0]), rho_p=float(pdbl[1]))
        for which, count in ((0, nnz), (1, nnz_p)):
            if which == 0 or nnz_p:
                c = np.zeros(rows + 1, np.int32), np.zeros(count, np.int32), np.zeros(count)
                lib.amg_reference_csr(h, l, which, *[_p(a) for a in c])
                L["P" if which else "A"] = _freeze(*c)
        if out["filtered"] and nnz_p:
            c = np.zeros(rows + 1, np.int32), np.zeros(L["nnz_f"], np.int32), np.zeros(L["nnz_f"]), np.zeros(L["nnz_f"], np.int32)
            lib.amg_prolongator_filtered_csr(h, l, *[_p(a) for a in c])
            L["AF"], L["map"] = _freeze(*c[:3]), _freeze(c[3])[0]
        agg = np.full(rows if rounds else 0, -1, np.int32)
        if rounds:
            lib.amg_reference_aggregates(h, l, _p(agg))
        L["agg"], = _freeze(agg)
        b, t = np.zeros(rows if out["has_nn"] else 0), np.zeros(rows if out["has_nn"] and nnz_p else 0)
        if out["has_nn"]:
            lib.amg_prolongator_vectors(h, l, _p(b), _p(t) if nnz_p else None)
        L["b"], L["t"] = _freeze(b, t)
        out["lev"].append(L)
    return out


def reference(rp, ci, va, n, near_null=None, filtered=False, theta=ac.DEFAULTS["theta"], max_levels=ac.DEFAULTS["max_levels"],
              coarse_rows=ac.DEFAULTS["coarse_rows"], **_):
    arrs = [np.ascontiguousarray(a, t) for a, t in ((rp, np.int32), (ci, np.int32), (va, np.float64))]
    nn = None if near_null is None else np.ascontiguousarray(near_null, np.float64)
    return _read(reference_lib().amg_prolongator_build(n, *[_p(a) for a in arrs], theta, max_levels, coarse_rows, int(filtered), _p(nn)))


def reference_update(ref, va):
    """the update loops: the structure of `ref` (levels, aggregates, kept patterns, t, b), the numbers of `va`"""
    va = np.ascontiguousarray(va, np.float64)
    return _read(reference_lib().amg_prolongator_update(ref["_h"], _p(va)))


@functools.lru_cache(maxsize=None)
def reference_of(name, variant):
    rp, ci, va, n, _, nn, filtered = case(name, variant)
    return reference(rp, ci, va, n, nn, filtered, **options(name))


def same_structure(a, b):
    """the premise of "an update equals amg_create_with on the new values": the same levels, aggregates AND kept patterns"""
    if a["levels"] != b["levels"] or a["stalled"] != b["stalled"]:
        return False
    for K, L in zip(a["lev"], b["lev"]):
        if K["n"] != L["n"] or not np.array_equal(K["agg"], L["agg"]) or (K["AF"] is None) != (L["AF"] is None):
            return False
        if K["AF"] is not None and not (np.array_equal(K["AF"][0], L["AF"][0]) and np.array_equal(K["map"], L["map"])):
            return False
    return True


def first_difference(a, b):
    """None, or what differs first between two hierarchies of _read()"""
    if a["levels"] != b["levels"]:
        return f"levels {a['levels']} and {b['levels']}"
    for l, (K, L) in enumerate(zip(a["lev"], b["lev"])):
        for k in ("omega", "rho", "omega_p", "rho_p", "unfiltered_rows", "nnz_f"):
            if K[k] != L[k]:
                return f"level {l}: {k} {K[k]!r} and {L[k]!r}"
        for which in ("A", "P", "AF"):
            if (K[which] is None) != (L[which] is None):
                return f"level {l}: {which} is missing on one side"
            if K[which] is not None and not all(np.array_equal(x, y) for x, y in zip(K[which], L[which])):
                return f"level {l}: {which} differs"
        if not (np.array_equal(K["b"], L["b"]) and np.array_equal(K["t"], L["t"])):
            return f"level {l}: b or t differs"
    return None


# ---- steps 5a to 5c, restated ----------------------------------------------------------------------------------------------------------

def restated_level(A, agg, nc, theta, b=None, filtered=False):
    """dict(AF, dF, unfiltered_rows, rho_p, omega_p, t, b_next, P, A_next) of one coarsened level from a scipy CSR A, its aggregates
    and its near-null vector, with scipy's own products and sums"""
    n = A.shape[0]
    d = A.diagonal()
    AF, dF, unf = A, d, 0
    if filtered:
        rows, cols, _ = ac.strong_edges(A, theta)
        S = sp.csr_matrix((np.ones(len(rows)), (rows, cols)), (n, n))
        kept = A.multiply(S).tocsr()                       # the strong off-diagonal entries
        weak = (A - kept - sp.diags(d)).tocsr()
        dF = d + np.asarray(weak.sum(axis=1)).ravel()
        back = ~(np.isfinite(dF) & (dF > 0))
        unf = int(back.sum())
        dF = np.where(back, d, dF)
        AF = (kept + sp.diags(back.astype(float)) @ weak + sp.diags(dF)).tocsr()
    rho_p = float((np.asarray(abs(AF).sum(axis=1)).ravel() / dF).max())
    omega_p = 4.0 / (3.0 * rho_p)
    if b is None:
        t, b_next = np.ones(n), None
    else:
        b_next = np.sqrt(np.bincount(agg, b * b, nc))
        t = b / b_next[agg]
    T = sp.csr_matrix((t, (np.arange(n), agg)), (n, nc))
    P = (T - sp.diags(omega_p / dF) @ (AF @ T)).tocsr()
    return dict(AF=AF, dF=dF, unfiltered_rows=unf, rho_p=rho_p, omega_p=omega_p, t=t, b_next=b_next, P=P, A_next=(P.T @ A @ P).tocsr())


# ---- the cycle and the solves, restated ------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def cycle_restatement(name, variant, dtype):
    """amg_cases.cycle_of over the reference's hierarchy: the cycle itself is untouched, its weights are step 1's omega / d"""
    return ac.cycle_of(reference_of(name, variant), dtype, **options(name))


def measured_cycle_difference(dtype):
    wide = np.float64 if np.dtype(dtype) == np.float32 else np.longdouble
    worst = 0.0
    for name, variant in CYCLE_CASES:
        lo, hi = cycle_restatement(name, variant, dtype), cycle_restatement(name, variant, wide)
        for v in ac.vectors(base(name)[3]):
            v = v.astype(dtype)
            a, b = lo(v).astype(np.longdouble), hi(v.astype(wide)).astype(np.longdouble)
            worst = max(worst, float(np.abs(a - b).max() / np.abs(b).max()))
    return worst


@functools.lru_cache(maxsize=None)
def path_restatement():
    """(x, history, stop) of CG on path_wrap to PATH_TOL with the cycle of ("path_wrap", "nn")"""
    A, b = ac.path_problem()
    x, hist, stop = pc.restate(A, b, cycle_restatement("path_wrap", "nn", np.float64), ac.PATH_TOL, pc.MAX_ITERATIONS, np.float64)
    return _freeze(x, hist) + (stop,)


@functools.lru_cache(maxsize=None)
def grid_scaled_count(which):
    """iterations of CG to PATH_TOL on the scaled grid with b of pcg_tri_cases.problem(): M^-1 the cycle of amg_cases.reference on it
    ("default") or of ("grid", "nn")"""
    rp, ci, va, n = case("grid", "nn")[:4]
    if which == "nn":
        M = cycle_restatement("grid", "nn", np.float64)
    else:
        M = ac.cycle_of(ac.reference(rp, ci, va, n, **options("grid")), np.float64, **options("grid"))
    _, hist, stop = pc.restate(matrix("grid", "nn"), pc.problem().b, M, ac.PATH_TOL, pc.MAX_ITERATIONS, np.float64)
    assert stop == 1
    return hist.size
