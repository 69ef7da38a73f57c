"""spmv_mi355x_pcg_tri at the sizes where csrc/solvers_common.hpp changes its path (the rule of test_gpu_solver_sizes.py, whose
docstring explains the sizes and the tail rows): n = N1 = 262 145 (nb = 257, the partial loop's second trip) and n = N2 = 1 049 601
(nb capped at 1024, the grid stride's 5th trip), in both precisions, on solver_size_cases.spd(n) with solver_size_cases.rhs(n), which
puts half of |b|^2 into the rows that only the second partial trip or the fifth grid-stride trip touches: rnorm0, the iteration count
and the explicit norms expose a lost tail.

Preconditioners: Jacobi as (None, solver_size_cases.preconditioner(A), None) and the blocked SGS of A at B = 4096 (sgs_precond): 65
and 257 blocks, the far band at +-131 071 is dropped entirely, the near band where it crosses a block boundary.

References: the numpy restatement of pcg_tri_cases.py on the scipy.sparse matrix, "M^-1 v" the C reference of
tests/trsv_reference.c on the filtered CSR. Its counts (recomputed here, asserted only as ranges):
      n     Jacobi fp64   SGS fp64   Jacobi fp32   SGS fp32
      N1        31           16          13            7
      N2        40           21          17            9
No dense solve exists at these sizes: the converged restatement stands in for it, and x (and x on the tail rows on its own) may lie
two x bounds from it. Bounds as in test_gpu_pcg_tri.py with the system's own norm-2 bound in place of KAPPA: by Gershgorin (diagonal
4, off-diagonal row sum 3) the eigenvalues of spd(n) lie in [1, 7], so |A|_2 <= 7 and cond_2 <= KAPPA_SPD = 7. (The largest singular
value itself, 6.52 at N1 and 6.95 at N2, costs minutes of Lanczos at N2; the Gershgorin bound costs nothing and is checked below.)
History: every preconditioned run is compared row by row (both are preconditioned here), at least SHARE of the rows qualifying."""
import functools

import numpy as np
import pytest

import pcg_tri_cases as pc
import solver_size_cases as C
import trsv_blocked_cases as bc
from pcg_tri_cases import PREC
from solver_size_cases import N1, N2, SHARE

pytestmark = pytest.mark.gpu

LAYOUTS = [("sell_c_sigma", {}), ("csr_vector", {})]
B_SGS = 4096
MAX_ITERATIONS = 200
KAPPA_SPD = 7.0
POLL = 32


@pytest.fixture(scope="module")
def eng():
    import spmv_mi355x as eng
    assert eng.device_count() >= 1, "no GPU visible: the -m gpu tests need an MI355X"
    return eng


@functools.lru_cache(maxsize=None)
def reference(n, dtype, kind):
    """(x, history, stop) of pcg_tri_cases.restate on spd(n) with rhs(n); kind "jacobi" or "sgs" """
    S = C.system("spd", n)
    A = S.D
    if kind == "jacobi":
        M = lambda v, d=S.minv.astype(dtype): d * v
    else:
        M = bc.sgs_apply(A.indptr, A.indices, A.data, n, B_SGS, dtype)
    out = pc.restate(S.cast(dtype)[0], S.b, M, PREC[dtype]["tol"], MAX_ITERATIONS, dtype)
    out[0].setflags(write=False)
    out[1].setflags(write=False)
    return out


@pytest.mark.parametrize("kind", ["jacobi", "sgs"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("n", [N1, N2])
def test_pcg_tri_against_the_restatement(eng, n, dtype, kind):
    S = C.system("spd", n)
    A = S.D
    lim, worst = PREC[dtype], {}
    assert (C.solver_blocks(N1), C.solver_blocks(N2)) == (C.VB + 1, C.MAX_PART)
    x_ref, ref, ref_stop = reference(n, dtype, kind)
    assert ref_stop == 1 and 5 <= ref.size <= 45
    if kind == "sgs":
        assert ref.size < reference(n, dtype, "jacobi")[1].size                # a property of the input
    off = np.asarray(abs(A).sum(axis=1)).ravel() - A.diagonal()
    assert (A.diagonal() - off).min() >= 1 and (A.diagonal() + off).max() <= KAPPA_SPD      # Gershgorin: eigenvalues in [1, 7]
    kappa = KAPPA_SPD
    bn = np.linalg.norm(S.b.astype(dtype).astype(np.float64))
    rows = np.nonzero(ref / bn > lim["ratio"])[0]
    assert rows.size and rows[-1] == rows.size - 1
    assert rows.size >= SHARE[dtype] * ref.size, f"{rows.size} of {ref.size} rows qualify"
    if kind == "jacobi":
        M = (None, S.minv.astype(dtype), None)
    else:
        M = eng.sgs_precond(A.indptr, A.indices, A.data, n, dtype, block_rows=B_SGS)
        assert M[0].block_info()["blocks"] == -(-n // B_SGS) and M[0].block_info()["nnz_dropped"] > n // 2
    for fmt, opts in LAYOUTS:
        H = S.handle(eng, fmt, dtype, **opts)
        what = f"spd({n}) {H.format_name} {np.dtype(dtype).name} precond={kind}"
        got = H.pcg_tri(S.b.astype(dtype), precond=M, tol=lim["tol"], max_iterations=MAX_ITERATIONS)
        H.close()
        k = got["iterations"]
        print(f"[pcg_tri sizes] {what}: {k} iterations (the restatement {ref.size}), rnorm {got['rnorm']:.3g}")
        assert got["stop"] == 1, f"{what}: stop {got['stop']} after {k} iterations"
        assert got["x"].dtype == dtype and got["x"].shape == (n,) and got["history"].shape == (k,)
        assert got["prnorm"] == got["history"][-1] and got["prnorm"] <= lim["tol"] * got["rnorm0"] * (1 + 1e-12), what
        assert k + 1 <= got["spmv_calls"] <= k + 1 + 2 * POLL, what
        assert abs(k - ref.size) <= 1 and k >= rows.size, f"{what}: {k} iterations, the restatement {ref.size}"
        shares = pc.shares_of_the_bounds(S, got, dtype)
        shares["rnorm"] = got["rnorm"] / (10 * lim["tol"] * np.linalg.norm(S.b))
        d = np.abs(got["history"][rows] - ref[rows]) / ref[rows]
        shares["history"] = d.max() / lim["hist"]
        # x, and x on the tail rows on its own, against the converged restatement's: each is within the x bound of the solution
        gx, rx, tail = got["x"].astype(np.float64), x_ref.astype(np.float64), S.tail
        x_bound = 2 * kappa * 10 * lim["tol"]
        shares["x"] = np.linalg.norm(gx - rx) / np.linalg.norm(rx) / x_bound
        shares["x_tail"] = np.linalg.norm(gx[tail] - rx[tail]) / np.linalg.norm(rx) / x_bound
        assert np.linalg.norm(rx[tail]) > 0.1 * np.linalg.norm(rx)            # the tail weighs in x as it does in b
        for key, v in shares.items():
            print(f"[pcg_tri sizes] {what}: {key} is {v:.3g} of its bound")
            assert v <= 1, f"{what}: {key} is {v:.3g} times its bound"
            worst[key] = max(worst.get(key, 0.0), float(v))
    for h in M:
        if h is not None and not isinstance(h, np.ndarray):
            h.close()
    print(f"[pcg_tri sizes] spd({n}) {np.dtype(dtype).name} precond={kind}: largest shares {worst}")
