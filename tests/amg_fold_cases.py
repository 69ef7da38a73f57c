"""What the two tiers of the fold tests share (test_amg_fold_abi.py on the CPU, test_gpu_amg_fold.py on the GPU): the C reference of
tests/amg_fold_reference.c (the folded tail of the V cycle as sequential loops; gcc -O2 -ffp-contract=off, once with -DREAL=float and
once with -DREAL=double), R by stable transposition, the rule of the lanes per row restated, and the cycle "above the first folded
level through the borrowed handles, the tail through the C reference" (modelled on python_cycle of test_gpu_amg.py). The cases are
amg_cases' own, unchanged. Nothing here touches the engine unless a handle is passed in.

A hierarchy is the dict of amg_cases.reference(): lev = [dict(n, A = (rp, ci, va), P = (rp, ci, va) or None, aggregates, omega)]."""
import ctypes
import functools
import os
import subprocess
import tempfile

import numpy as np

import amg_cases as ac

ROOT = ac.ROOT
FOLD_TB, MAX_LANES, DENSE_MAX, MAX_FOLD_ROWS = 1024, 64, 128, 65536
# (case, fold_rows or "rows1" = rows[1]): the first folded level sits at different depths; None = no level qualifies
FOLDS = (("grid", 4096), ("grid", "rows1"), ("grid", 1), ("grid_nu2", 4096), ("grid_nu2", "rows1"), ("n129", 4096), ("n129", 128), ("n128", 4096),
         ("one", 4096), ("grid_weak", 4096))
PATH_FOLDS = (4096, 1100)


def lanes(n, nnz):
    """the header's rule: the largest power of two <= min(64, nnz / n, 1024 / n) in integer division, 1 where that minimum is 0"""
    cap = min(MAX_LANES, nnz // n, FOLD_TB // n) if n > 0 else 1
    g = 1
    while 2 * g <= cap:
        g *= 2
    return g


def first_level(rows, fold_rows):
    """the first level with rows <= fold_rows; len(rows) when none has (or fold_rows = 0)"""
    return next((l for l, r in enumerate(rows) if fold_rows > 0 and r <= fold_rows), len(rows))


def fold_rows_of(name, spec):
    return ac.reference_of(name)["lev"][1]["n"] if spec == "rows1" else spec


def stable_transpose(rp, ci, va, n, nc):
    """the CSR of the transposed n x nc matrix: rows in order, inside a row the entries in ascending row of the input"""
    rows = np.repeat(np.arange(n, dtype=np.int32), np.diff(rp))
    order = np.argsort(ci, kind="stable")
    t_rp = np.zeros(nc + 1, np.int32)
    np.cumsum(np.bincount(ci, minlength=nc), out=t_rp[1:])
    return t_rp, rows[order].astype(np.int32), va[order]


@functools.lru_cache(maxsize=None)
def reference_lib(dtype):
    dtype = np.dtype(dtype)
    real = {np.dtype(np.float32): "float", np.dtype(np.float64): "double"}[dtype]
    out = os.path.join(tempfile.mkdtemp(prefix="amg_fold_reference_"), f"amg_fold_reference_{real}.so")
    subprocess.run(["gcc", "-O2", "-ffp-contract=off", f"-DREAL={real}", "-shared", "-fPIC", os.path.join(ROOT, "tests", "amg_fold_reference.c"),
                    "-o", out, "-lm"], check=True)
    lib = ctypes.CDLL(out)
    P = ctypes.c_void_p
    lib.amg_fold_reference_new.restype = P
    lib.amg_fold_reference_new.argtypes = [ctypes.c_int] * 3
    lib.amg_fold_reference_level.restype = None
    lib.amg_fold_reference_level.argtypes = [P, ctypes.c_int, ctypes.c_long, P, P, P, P, ctypes.c_int, ctypes.c_long, P, P, P, P, P, P]
    lib.amg_fold_reference_factor.restype = None
    lib.amg_fold_reference_factor.argtypes = [P, P]
    lib.amg_fold_reference_free.restype = None
    lib.amg_fold_reference_free.argtypes = [P]
    lib.amg_fold_reference_apply.restype = None
    lib.amg_fold_reference_apply.argtypes = [P, ctypes.c_int, P, P]
    lib.amg_fold_reference_lanes.restype = ctypes.c_int
    lib.amg_fold_reference_lanes.argtypes = [ctypes.c_long, ctypes.c_long]
    return lib


_p = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def weights(L, dtype):
    """w = omega / d in fp64, narrowed: the level's w"""
    rp, ci, va = L["A"]
    rows = np.repeat(np.arange(L["n"]), np.diff(rp))
    return (L["omega"] / va[rows == ci]).astype(dtype)


class Tail:
    """the C reference over the levels first .. last of a hierarchy, values narrowed to dtype as the engine narrows them (a cast);
    dense = None: the last level is solved densely when it has at most 128 rows and its factor exists; lanes_per_row = None: the rule"""

    def __init__(self, hier, dtype, first, sweeps=ac.DEFAULTS["sweeps"], coarse_sweeps=ac.DEFAULTS["coarse_sweeps"], lanes_per_row=None,
                 dense=None, **_):
        self.dtype, self.first, self.lib = np.dtype(dtype), first, reference_lib(dtype)
        lev = hier["lev"]
        self.rows = [L["n"] for L in lev]
        self.h = self.lib.amg_fold_reference_new(len(lev), sweeps, coarse_sweeps)
        self.lanes = []
        for l, L in enumerate(lev):
            G = lanes(L["n"], len(L["A"][1])) if lanes_per_row is None else lanes_per_row[l]
            self.lanes.append(G)
            if l < first:
                continue
            a = [np.ascontiguousarray(L["A"][0], np.int32), np.ascontiguousarray(L["A"][1], np.int32), L["A"][2].astype(dtype)]
            w = weights(L, dtype)
            pr, nc = [None] * 6, 0
            if L["P"] is not None:
                nc = L["aggregates"]
                p_rp, p_ci, p_va = (np.ascontiguousarray(L["P"][0], np.int32), np.ascontiguousarray(L["P"][1], np.int32), L["P"][2])
                r_rp, r_ci, r_va = stable_transpose(p_rp, p_ci, p_va, L["n"], nc)
                pr = [p_rp, p_ci, p_va.astype(dtype), r_rp, r_ci, r_va.astype(dtype)]
            self.lib.amg_fold_reference_level(self.h, l, L["n"], *[_p(v) for v in a], _p(w), G, nc, *[_p(v) for v in pr])
        Z = lev[-1]
        F = ac.reference_factor(*Z["A"], Z["n"]) if Z["n"] <= DENSE_MAX and dense is not False else None
        self.dense = F is not None
        if self.dense:
            self.lib.amg_fold_reference_factor(self.h, _p(F))

    def apply(self, v, level=None):
        """cycle(level, v) by the sequential loops; level defaults to the first folded one"""
        level = self.first if level is None else level
        assert level >= self.first
        v = np.ascontiguousarray(v, self.dtype)
        assert v.shape == (self.rows[level],)
        out = np.full(max(len(v), 1), np.nan, self.dtype)
        self.lib.amg_fold_reference_apply(self.h, level, _p(v), _p(out))
        return out[:len(v)]

    def close(self):
        if self.h:
            self.lib.amg_fold_reference_free(self.h)
            self.h = None

    def __del__(self):
        self.close()


@functools.lru_cache(maxsize=None)
def tail_of(name, dtype, first):
    """the reference tail of a case of amg_cases from level `first` on"""
    return Tail(ac.reference_of(name), dtype, first, **ac.options(name))


def hierarchy_of(M):
    """the dict of a live handle's hierarchy, from level_csr and info (after an update: the new values)"""
    info = M.info()
    lev = []
    for l in range(info["levels"]):
        last = l == info["levels"] - 1
        lev.append(dict(n=info["rows"][l], A=M.level_csr(l, "A"), P=None if last else M.level_csr(l, "P"),
                        aggregates=0 if last else info["rows"][l + 1], omega=info["omega"][l]))
    return dict(levels=info["levels"], lev=lev)


def folded_cycle(M, hier, tail, v, sweeps=ac.DEFAULTS["sweeps"], **_):
    """apply(v) of a folded hierarchy restated: the levels above tail.first through the borrowed handles (SpMVs on the device, the
    elementwise steps in numpy, as python_cycle of test_gpu_amg.py runs them), the rest by the C reference"""
    import torch
    dtype, nu, f = M.dtype.type, sweeps, tail.first
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()

    def product(H, x, y0=None):
        xd = dev(x)
        yd = torch.zeros(H.m, dtype=xd.dtype, device="cuda") if y0 is None else dev(y0)
        H.spmv_device(xd.data_ptr(), yd.data_ptr(), beta=0 if y0 is None else 1)
        torch.cuda.synchronize()
        return yd.cpu().numpy()

    def cycle(l, b):
        if l >= f:
            return tail.apply(b, l)
        A, P, R = M.level_matrices(l)
        w = weights(hier["lev"][l], dtype)
        sweep = lambda x: x + w * (b - product(A, x))
        x = w * b
        for _ in range(nu - 1):
            x = sweep(x)
        r = b - product(A, x)
        x = product(P, cycle(l + 1, product(R, r)), y0=x)
        for _ in range(nu):
            x = sweep(x)
        return x
    return cycle(0, np.ascontiguousarray(v, dtype))
