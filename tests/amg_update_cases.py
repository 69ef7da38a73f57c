"""What the two tiers of the tests of "AMG: new values for a hierarchy" share (test_amg_update_abi.py on the CPU,
test_gpu_amg_update.py on the GPU): the value sets V2, the frozen C reference of tests/amg_update_reference.c (the aggregates given,
steps 1, 5 and 6 as sequential loops; gcc -O2 -ffp-contract=off like amg_cases.reference_lib), a scipy restatement of the frozen
hierarchy in a dtype of choice (P = T - diag(omega / d) (A T), P^t A P by scipy's products), and the CG counts of a fresh, a frozen
and a stale hierarchy through pcg_tri_cases.restate. Nothing here touches the engine; everything is computed once and read-only.

THE VALUE SETS, on the pattern of a case of amg_cases.py with values V1 and n rows:
    x0.7      0.7 * V1
    sym<eps>  S V1 S with s = 1 + eps * default_rng(5).uniform(-1, 1, n), entry (i, j) times (s_i * s_j): symmetric to the bit
    diag+1    1.0 added to every diagonal entry
    path9     path_wrap built with default_rng(9) in place of default_rng(2)
same_structure(name, vset) is the computed premise of "equals amg_create on V2": tests/amg_reference.c finds the same levels, the
same stall and the same aggregates from V2 as from V1.

THE BOUND OF THE FROZEN RESTATEMENT (FROZEN_MEASURED, FROZEN_BOUND; recomputed in test_amg_update_abi.py). The C loops sum in another
order than scipy's products, so they are compared within ten times what the restatement itself moves by when its arithmetic changes
from fp64 to np.longdouble: the largest difference of any A_l or P_l over FROZEN_CASES, relative to the operator's largest entry
(measured 3.61e-15, on the third level of grid, diag+1). FROZEN_MEASURED holds that rounded up to two digits, FROZEN_BOUND ten times that.

THE COUNTS (FROZEN_COUNTS; recomputed in test_amg_update_abi.py): pcg_tri_cases.restate in fp64 at tol 1e-12 on the grid with V2 and
the b of pcg_tri_cases.problem(), M^-1 = the restated cycle over the fresh hierarchy of V2, over the frozen one (V1's aggregates,
V2's numbers) and over the stale one (all of V1)."""
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
SAME_STRUCTURE = (("grid", "x0.7"), ("aniso", "x0.7"), ("isolated", "x0.7"), ("unsorted", "x0.7"), ("n129", "x0.7"), ("n129", "sym1e-2"))
FROZEN_CASES = (("grid", "sym0.5"), ("aniso", "sym0.5"), ("grid", "diag+1"))
FROZEN_MEASURED = 3.7e-15
FROZEN_BOUND = 3.7e-14
# (fresh, frozen, stale) on the grid
FROZEN_COUNTS = {"sym0.5": (31, 31, 83), "diag+1": (14, 14, 42)}
COUNT_TOL = 1e-12

_p = lambda a: a.ctypes.data_as(ctypes.c_void_p)


@functools.lru_cache(maxsize=None)
def values(name, vset):
    """V2 of case `name`: nnz fp64 values in the case's entry order, read-only"""
    rp, ci, va, n, _ = ac.case(name)
    rows = np.repeat(np.arange(n), np.diff(rp))
    if vset == "v1":
        out = va.copy()
    elif vset == "x0.7":
        out = 0.7 * va
    elif vset.startswith("sym"):
        s = 1 + float(vset[3:]) * np.random.default_rng(5).uniform(-1, 1, n)
        out = va * (s[rows] * s[ci])
    elif vset == "diag+1":
        out = va + (rows == ci)
    elif vset == "path9":
        assert name == "path_wrap"
        s = 1 + 0.2 * np.random.default_rng(9).uniform(-1, 1, n)
        A = sp.diags([-np.ones(n - 1), 2.0001 * np.ones(n), -np.ones(n - 1)], [-1, 0, 1]).tocsr()
        B = (sp.diags(s) @ A @ sp.diags(s)).tocsr()
        B.sort_indices()
        assert np.array_equal(B.indptr, rp) and np.array_equal(B.indices, ci)
        out = B.data.astype(np.float64)
    else:
        raise KeyError(vset)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def reference_lib():
    out = os.path.join(tempfile.mkdtemp(prefix="amg_update_reference_"), "amg_update_reference.so")
    subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-shared", "-fPIC", os.path.join(ROOT, "tests", "amg_update_reference.c"), "-o", out,
                    "-lm"], check=True)
    lib = ctypes.CDLL(out)
    lib.amg_update_reference_build.restype = ctypes.c_void_p
    lib.amg_update_reference_build.argtypes = [ctypes.c_long, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int,
                                               ctypes.c_void_p, ctypes.c_void_p]
    lib.amg_update_reference_min_diagonal.restype = ctypes.c_double
    lib.amg_update_reference_min_diagonal.argtypes = [ctypes.c_void_p, ctypes.c_int]
    lib.amg_reference_free.argtypes = [ctypes.c_void_p]
    lib.amg_reference_levels.argtypes = [ctypes.c_void_p]
    lib.amg_reference_level.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    lib.amg_reference_csr.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    return lib


def frozen_reference(rp, ci, va, n, structure):
    """The hierarchy of the sequential loops on the values `va` with the levels and aggregates of `structure` (a dict of
    amg_cases.reference): the same dict, with agg / aggregates / rounds / stalled copied from `structure`, and min_diagonal per level."""
    lib = reference_lib()
    levels = structure["levels"]
    out = dict(levels=levels, stalled=structure["stalled"], lev=[])
    if levels == 0:
        return out
    coarsened = [L for L in structure["lev"] if L["P"] is not None]
    assert len(coarsened) == levels - 1
    agg = np.ascontiguousarray(np.concatenate([L["agg"] for L in coarsened] + [np.zeros(0, np.int32)]), np.int32)
    count = np.ascontiguousarray([L["aggregates"] for L in coarsened] + [0], np.int64)
    arrs = [np.ascontiguousarray(a, t) for a, t in ((rp, np.int32), (ci, np.int32), (va, np.float64))]
    h = lib.amg_update_reference_build(n, *[_p(a) for a in arrs], levels, _p(agg), _p(count))
    assert lib.amg_reference_levels(h) == levels
    for l, S in enumerate(structure["lev"]):
        num, dbl = np.zeros(5, np.int64), np.zeros(2)
        lib.amg_reference_level(h, l, _p(num), _p(dbl))
        rows, nnz, nnz_p = (int(v) for v in num[:3])
        L = dict(n=rows, aggregates=S["aggregates"], rounds=S["rounds"], omega=float(dbl[0]), rho=float(dbl[1]), P=None, agg=S["agg"],
                 min_diagonal=lib.amg_update_reference_min_diagonal(h, l))
        for which, cnt in ((0, nnz), (1, nnz_p)):
            if which == 0 or nnz_p:
                c = np.zeros(rows + 1, np.int32), np.zeros(cnt, np.int32), np.zeros(cnt)
                lib.amg_reference_csr(h, l, which, *[_p(a) for a in c])
                for a in c:
                    a.setflags(write=False)
                L["P" if which else "A"] = c
        out["lev"].append(L)
    lib.amg_reference_free(h)
    return out


@functools.lru_cache(maxsize=None)
def fresh_of(name, vset):
    """amg_cases.reference on V2: what amg_create finds from it"""
    rp, ci, _, n, _ = ac.case(name)
    return ac.reference(rp, ci, values(name, vset), n, **ac.options(name))


@functools.lru_cache(maxsize=None)
def frozen_of(name, vset):
    """the frozen hierarchy: the structure of V1, the numbers of V2"""
    rp, ci, _, n, _ = ac.case(name)
    return frozen_reference(rp, ci, values(name, vset), n, ac.reference_of(name))


def same_hierarchy_structure(a, b):
    return (a["levels"] == b["levels"] and a["stalled"] == b["stalled"] and
            all(K["n"] == L["n"] and np.array_equal(K["agg"], L["agg"]) for K, L in zip(a["lev"], b["lev"])))


@functools.lru_cache(maxsize=None)
def same_structure(name, vset):
    """the premise of "equals amg_create on V2", computed with tests/amg_reference.c"""
    return same_hierarchy_structure(ac.reference_of(name), fresh_of(name, vset))


def equal_to_the_bit(a, b):
    """None, or what differs first between two hierarchies of reference() / frozen_reference()"""
    if a["levels"] != b["levels"]:
        return f"levels {a['levels']} and {b['levels']}"
    for l, (K, L) in enumerate(zip(a["lev"], b["lev"])):
        if (K["omega"], K["rho"]) != (L["omega"], L["rho"]):
            return f"level {l}: omega, rho {K['omega']!r}, {K['rho']!r} and {L['omega']!r}, {L['rho']!r}"
        for which in ("A", "P"):
            if (K[which] is None) != (L[which] is None):
                return f"level {l}: {which} is missing on one side"
            if K[which] is not None and not all(np.array_equal(x, y) for x, y in zip(K[which], L[which])):
                return f"level {l}: {which} differs"
    return None


# ---- the frozen hierarchy, restated ----------------------------------------------------------------------------------------------------

def restated_frozen(A, structure, dtype=np.float64):
    """[(A_l, P_l or None, omega, rho)] of the frozen hierarchy over scipy's own products in `dtype` (float64 or longdouble)"""
    out = []
    A = A.astype(dtype)
    for S in structure["lev"]:
        n, d = A.shape[0], A.diagonal()
        rho = (np.asarray(abs(A).sum(axis=1)).ravel() / d).max()
        omega = dtype(4.0) / (dtype(3.0) * rho)
        if S["P"] is None:
            out.append((A, None, omega, rho))
            break
        T = sp.csr_matrix((np.ones(n, dtype), (np.arange(n), S["agg"])), (n, S["aggregates"]))
        P = (T - sp.diags(omega / d) @ (A @ T)).tocsr()
        out.append((A, P, omega, rho))
        A = (P.T.tocsr() @ (A @ P)).tocsr()
    return out


def _dense(c, shape):
    return sp.csr_matrix((c[2].copy(), c[1].copy(), c[0].copy()), shape).toarray()


def frozen_restatement_distance(name, vset, against):
    """the largest difference, relative to the operator's largest entry, of any A_l, P_l, omega or rho between the fp64 restatement of
    (name, vset) and `against`: "longdouble" (the restatement itself in np.longdouble) or a hierarchy of frozen_reference()"""
    A2 = sp.csr_matrix((values(name, vset).copy(), ac.case(name)[1].copy(), ac.case(name)[0].copy()), (ac.case(name)[3],) * 2)
    structure = ac.reference_of(name)
    lo = restated_frozen(A2, structure)
    worst = 0.0
    rel = lambda x, y: float(np.abs(x.astype(np.longdouble) - y).max() / np.abs(y).max())
    if isinstance(against, str):
        for (A, P, om, rho), (Ah, Ph, omh, rhoh) in zip(lo, restated_frozen(A2, structure, np.longdouble)):
            worst = max(worst, rel(A.toarray(), Ah.toarray()), float(abs(om - omh) / omh), float(abs(rho - rhoh) / rhoh))
            if P is not None:
                worst = max(worst, rel(P.toarray(), Ph.toarray()))
    else:
        for (A, P, om, rho), L in zip(lo, against["lev"]):
            worst = max(worst, rel(_dense(L["A"], A.shape), A.toarray()), abs(L["omega"] - om) / om, abs(L["rho"] - rho) / rho)
            if P is not None:
                worst = max(worst, rel(_dense(L["P"], P.shape), P.toarray()))
    return worst


# ---- the counts --------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def grid_counts(vset):
    """(fresh, frozen, stale) iterations of CG on the grid with V2 and the b of pcg_tri_cases.problem()"""
    rp, ci, _, n, _ = ac.case("grid")
    A2 = sp.csr_matrix((values("grid", vset).copy(), ci.copy(), rp.copy()), (n, n))
    b = pc.problem().b
    out = []
    for ref in (fresh_of("grid", vset), frozen_of("grid", vset), ac.reference_of("grid")):
        _, hist, stop = pc.restate(A2, b, ac.cycle_of(ref, np.float64, **ac.options("grid")), COUNT_TOL, pc.MAX_ITERATIONS, np.float64)
        assert stop == 1
        out.append(hist.size)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def coarse_failure_values(name="grid", factor=3.0):
    """Values whose level-0 diagonal is fine and whose coarse diagonal is not: the off-diagonal entries of V1 times `factor` make the
    matrix indefinite with its diagonal untouched. Returns (values, level) with `level` the first level of the frozen hierarchy whose
    diagonal is not positive, or (values, None) if there is none."""
    rp, ci, va, n, _ = ac.case(name)
    rows = np.repeat(np.arange(n), np.diff(rp))
    v2 = np.where(rows == ci, va, factor * va)
    v2.setflags(write=False)
    ref = frozen_reference(rp, ci, v2, n, ac.reference_of(name))
    bad = [l for l, L in enumerate(ref["lev"]) if not (np.isfinite(L["min_diagonal"]) and L["min_diagonal"] > 0)]
    return v2, (bad[0] if bad else None)
