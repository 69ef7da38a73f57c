"""What the two tiers of the k-column tests share (test_pcg_tri_multi_abi.py on the CPU, test_gpu_pcg_tri_multi.py on the GPU), on
top of pcg_tri_cases.py, amg_cases.py and fsai_cases.py, which are imported unchanged: the column counts, the split of k into
chunks, the blocks of right-hand sides and the five columns of the freeze test. Nothing here touches the engine. Everything is
computed once and is read-only.

THE COLUMN COUNTS. The vector kernels serve chunks of 8, 4, 2 or 1 columns: k = 1 is the chunk of one, 3 = 2 + 1, 4 and 8 are one
chunk each, 9 = 8 + 1 puts a column behind a full chunk (and two workgroups on the dense solve of a hierarchy).

THE FREEZE COLUMNS (freeze_columns): the usual b; an eigenvector of the dense operator, for which plain CG has r = b - (b.b / b.Ab)
A b = 0 up to rounding after one body; the zero vector (stop 3); b with one NaN (stop 4 at 0 iterations, x = 0); another seeded b."""
import functools

import numpy as np

import amg_cases as ac
import pcg_tri_cases as pc

K_CYCLE = (1, 3, 8, 9)
K_SOLVE = (1, 3, 4, 8, 9)
MAX_KC = 8
FREEZE_STOPS = (1, 1, 3, 4, 1)


def chunks(k):
    """[(c0, kc)]: k as 8s, then the binary remainder"""
    out, c0 = [], 0
    while k - c0 >= MAX_KC:
        out.append((c0, MAX_KC))
        c0 += MAX_KC
    w = MAX_KC // 2
    while w >= 1:
        if k - c0 >= w:
            out.append((c0, w))
            c0 += w
        w //= 2
    return out


@functools.lru_cache(maxsize=None)
def cycle_block(n, k=max(K_CYCLE)):
    """n x k in fp64: amg_cases.vectors(n), then seeded uniform columns"""
    cols = list(ac.vectors(n))
    rng = np.random.default_rng(23)
    while len(cols) < k:
        cols.append(rng.uniform(-1, 1, n))
    V = np.ascontiguousarray(np.stack(cols[:k], axis=1))
    V.setflags(write=False)
    return V


@functools.lru_cache(maxsize=None)
def solve_block(k=max(K_SOLVE)):
    """n x k in fp64 for pcg_tri_cases.problem(): its b, then seeded uniform columns of differing scale"""
    P = pc.problem()
    rng = np.random.default_rng(29)
    cols = [P.b] + [(10.0 ** (j % 3 - 1)) * rng.uniform(-1, 1, P.n) for j in range(k - 1)]
    B = np.ascontiguousarray(np.stack(cols, axis=1))
    B.setflags(write=False)
    return B


@functools.lru_cache(maxsize=None)
def eigenvector():
    P = pc.problem()
    _, V = np.linalg.eigh(P.D)
    v = np.ascontiguousarray(V[:, P.n // 3])
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def freeze_columns():
    """n x 5 in fp64: see the module's docstring; the stops are FREEZE_STOPS"""
    P = pc.problem()
    nan = P.b.copy()
    nan[P.n // 2] = np.nan
    B = np.ascontiguousarray(np.stack([P.b, eigenvector(), np.zeros(P.n), nan, np.random.default_rng(31).uniform(-1, 1, P.n)], axis=1))
    B.setflags(write=False)
    return B


def near_null(n):
    """a positive near-null candidate that is not the constant"""
    v = 1 + 0.3 * np.random.default_rng(37).uniform(-1, 1, n)
    v.setflags(write=False)
    return v
