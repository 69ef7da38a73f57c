"""spmv_mi355x_gmres_tri / Matrix.gmres(precond=(first, scale, second)) (include/spmv_mi355x.h "GMRES(m) right-preconditioned by
triangular solves") on the GPU, with the blocked SGS of A as the preconditioner: first = the LOWER / STORED blocked handle of A's CSR,
scale = diag(A), second = the UPPER / STORED one, block_rows B in {64, 100, 256}.

The problem is convdiff(45) of trsv_blocked_cases.py, n = 2025: cond_2 = 67.5 (asserted <= KAPPA = 70 from the singular values),
columns ascending, b = default_rng(7).uniform(-1, 1, n).

References, none of them the engine: numpy.linalg.solve on the dense matrix for the solution, numpy's explicit norms of the RETURNED
x, and a numpy restatement of the header's recurrences (test_gpu_gmres.py's restate with "M v" a callable: the C reference of
tests/trsv_reference.c on the filtered CSR, twice, with the scale between) for the history, the iterations and the restarts. The bounds
are test_gpu_gmres.py's:
  * info.rnorm <= 10 tol |b|;  |x - x*| / |x*| <= KAPPA 10 tol. (On the CPU the restatement uses under 10 % of the first and under
    2 % of the second.)
  * rnorm, xnorm against numpy's explicit values of the returned x: 1e-10 (fp64) / 1e-4 (fp32) relative, rnorm plus the cancellation
    floor; rnorm0 = |b| to 1e-13 / 1e-6.
  * iterations within 1 of the restatement's, restarts = (iterations - 1) // restart.
  * history against the restatement to rtol 1e-6 / 1e-3 on the rows with |g| / |b| above 1e-8 / 1e-2; at least 60 % / 30 % of the rows
    qualify (the restatement alone gives 64-73 % / 31-33 %).
The restatement's counts, recomputed here and never hard-coded in an assertion:
      case                          B = 64   B = 100   B = 256        minv = 1 / diag
      fp64, tol 1e-12, restart 20     121       80        60              217
      fp64, tol 1e-12, restart 7       90       75        62
      fp32, tol 1e-5,  restart 20      48       36        28
      fp32, tol 1e-5,  restart 7       48       36        28
The fp64 cases at B = 64 and 100 pass 2 * POLL = 64: the host's run-ahead and its stop on the progress word are exercised, in the
middle of a cycle in all but one of them (B = 100 at restart 20 stops at step 80, the end of a cycle: that path too). That the
blocked count lies below the count with minv = 1 / diag is asserted as a property of the input."""
import ctypes
import functools

import numpy as np
import pytest

import trsv_blocked_cases as bc

pytestmark = pytest.mark.gpu

LAYOUTS = [("sell_c_sigma", {}), ("csr_vector", {})]
DELTA = dict(sell_c=64, sell_delta=1, sell_sigma=64, sell_window=2)
BLOCKS = (64, 100, 256)
KAPPA = 70.0
POLL = 32
MAX_ITERATIONS = 400
PREC = {np.float64: dict(tol=1e-12, norms=1e-10, norms0=1e-13, ratio=1e-8, hist=1e-6, share=0.6),
        np.float32: dict(tol=1e-5, norms=1e-4, norms0=1e-6, ratio=1e-2, hist=1e-3, share=0.3)}
INFO_FIELDS = ("iterations", "stop", "restarts", "rnorm", "rnorm0", "prnorm", "xnorm")


@pytest.fixture(scope="module")
def eng():
    import spmv_mi355x as eng
    assert eng.device_count() >= 1, "no GPU visible: the -m gpu tests need an MI355X"
    return eng


# ---- the restatement -----------------------------------------------------------------------------------------------------------------

def restate(A, b, m, M, tol, max_iterations, dtype):
    """the header's recurrences in numpy: vectors in `dtype`, dots and scalars in fp64. A is a dense matrix of `dtype`, M the
    callable of "M v" (None: the identity). Returns (x, history, stop, restarts)."""
    dt = np.dtype(dtype).type
    n = len(b)
    b = b.astype(dt)
    dot = lambda u, v: float(u.astype(np.float64) @ v.astype(np.float64))
    M = M or (lambda v: v)
    x = np.zeros(n, dt)
    beta0 = np.sqrt(dot(b, b))
    hist, it, stop, restarts = [], 0, 2, 0
    if beta0 == 0:
        return x, np.zeros(0), 3, 0
    r, beta = b.copy(), beta0
    while it < max_iterations and stop == 2:
        V = [dt(1 / beta) * r]
        R, cs, sn, g = np.zeros((m + 1, m)), np.zeros(m), np.zeros(m), np.zeros(m + 1)
        g[0] = beta
        j = 0
        while j < m and it < max_iterations:
            w = A @ M(V[j])
            h = np.zeros(j + 2)
            for _ in range(2):                                   # CGS2: all dots of a pass from the same w
                c = np.array([dot(v, w) for v in V])
                for ci, v in zip(c, V):
                    w = w - dt(ci) * v
                h[:j + 1] += c
            hn = h[j + 1] = np.sqrt(dot(w, w))
            for i in range(j):
                t = cs[i] * h[i] + sn[i] * h[i + 1]
                h[i + 1] = -sn[i] * h[i] + cs[i] * h[i + 1]
                h[i] = t
            rho = np.hypot(h[j], h[j + 1])
            if not np.isfinite(rho) or rho == 0:                 # this column is dropped: j, it, x as before it
                stop = 4
                break
            cs[j], sn[j] = h[j] / rho, h[j + 1] / rho
            h[j] = rho
            R[:j + 1, j] = h[:j + 1]
            g[j + 1] = -sn[j] * g[j]
            g[j] = cs[j] * g[j]
            it += 1
            j += 1
            hist.append(abs(g[j]))
            if tol > 0 and abs(g[j]) <= tol * beta0:
                stop = 1
                break
            if hn == 0:
                stop = 5
                break
            V.append(dt(1 / hn) * w)
        y = np.linalg.solve(np.triu(R[:j, :j]), g[:j]) if j else np.zeros(0)
        u = np.zeros(n, dt)
        for yi, v in zip(y, V):
            u = u + dt(yi) * v
        x = x + M(u)
        if stop != 2 or it >= max_iterations:
            break
        r = b - A @ x
        beta = np.sqrt(dot(r, r))
        restarts += 1
        if not np.isfinite(beta):
            stop = 4
        elif beta == 0:
            stop = 5
    return x, np.array(hist), stop, restarts


class Problem:
    def __init__(self):
        rp, ci, va, n, D = bc.convdiff(45)
        self.n, self.D, self.csr = n, D, (rp, ci, va)
        assert np.all(np.diff(ci)[np.diff(np.repeat(np.arange(n), np.diff(rp))) == 0] > 0), "columns ascending"
        self.k_row = int((D != 0).sum(axis=1).max())
        self.b = np.random.default_rng(7).uniform(-1, 1, n)
        self.diag = np.ascontiguousarray(np.diag(D))
        self.b.setflags(write=False)
        self.diag.setflags(write=False)

    def handle(self, eng, fmt, dtype, values=None, **opts):
        rp, ci, va = self.csr
        return eng.Matrix(rp, ci, va if values is None else values, self.n, self.n, fmt, dtype, **opts)

    def sgs(self, eng, dtype, B, B_upper="same", values=None):
        """precond of the blocked SGS: (lower handle, diag(A), upper handle); B = None gives a global handle"""
        rp, ci, va = self.csr
        va = va if values is None else values
        B_upper = B if isinstance(B_upper, str) else B_upper
        L = eng.TriangularSolve(rp, ci, va, self.n, uplo="lower", dtype=dtype, block_rows=B)
        U = eng.TriangularSolve(rp, ci, va, self.n, uplo="upper", dtype=dtype, block_rows=B_upper)
        return L, self.diag.astype(dtype), U

    @functools.lru_cache(maxsize=None)
    def solve(self):
        sv = np.linalg.svd(self.D, compute_uv=False)
        assert sv[0] / sv[-1] <= KAPPA, sv[0] / sv[-1]
        x = np.linalg.solve(self.D, self.b)
        x.setflags(write=False)
        return x

    @functools.lru_cache(maxsize=None)
    def dense(self, dtype):
        A = self.D.astype(dtype)
        A.setflags(write=False)
        return A

    @functools.lru_cache(maxsize=None)
    def restatement(self, dtype, restart, B, tol, max_iterations=MAX_ITERATIONS, B_upper="same"):
        """B: a block size, None (the global SGS) or "minv" (the Jacobi preconditioner 1 / diag)"""
        if B == "minv":
            M = lambda v, d=(1.0 / self.diag).astype(dtype): d * v
        else:
            M = bc.sgs_apply(*self.csr, self.n, B, dtype, B_upper)
        x, hist, stop, restarts = restate(self.dense(dtype), self.b, restart, M, tol, max_iterations, dtype)
        x.setflags(write=False)
        hist.setflags(write=False)
        return x, hist, stop, restarts


@functools.lru_cache(maxsize=None)
def problem():
    return Problem()


def explicit_norms(P, x):
    x = x.astype(np.float64)
    return np.linalg.norm(P.b - P.D @ x), np.linalg.norm(x)


def cancellation_floor(P, x, dtype):
    """test_gpu_gmres.py's: how far two correct evaluations of |b - A x| for the same x can lie apart, to first order"""
    u, u64, store = float(np.finfo(dtype).eps) / 2, 2.0 ** -53, int(np.dtype(dtype) == np.float32)
    x = np.abs(x.astype(np.float64))
    k = P.k_row
    ax, bn = np.linalg.norm(np.abs(P.D) @ x), np.linalg.norm(P.b)
    return (u * (k + store + 1) + u64 * (k + 1)) * ax + (u * (1 + store) + u64) * bn


def shares_of_the_bounds(P, got, dtype, converged=True):
    """the figures of one solve, each as a share of its bound (<= 1 passes)"""
    lim = PREC[dtype]
    bn = np.linalg.norm(P.b)
    rn, xn = explicit_norms(P, got["x"])
    floor_r = cancellation_floor(P, got["x"], dtype)
    bt = np.linalg.norm(P.b.astype(dtype).astype(np.float64))
    out = dict(rnorm_np=abs(got["rnorm"] - rn) / (lim["norms"] * rn + floor_r),
               xnorm_np=abs(got["xnorm"] - xn) / (lim["norms"] * xn) if xn else float(got["xnorm"] != 0),
               rnorm0_np=abs(got["rnorm0"] - bt) / (lim["norms0"] * bt))
    if converged:
        want = P.solve()
        out["rnorm"] = got["rnorm"] / (10 * lim["tol"] * bn)
        out["x"] = np.linalg.norm(got["x"].astype(np.float64) - want) / np.linalg.norm(want) / (KAPPA * 10 * lim["tol"])
    return out


def allowance(restart):
    """SpMV launches the host may have enqueued past a stop: 2 * POLL inner steps and the restarts among them"""
    return 2 * POLL + 2 * POLL // restart + 1


def close(*handles):
    for h in handles:
        if h is not None and not isinstance(h, np.ndarray):
            h.close()


def _same(a, b, what):
    for k in INFO_FIELDS:
        assert a[k] == b[k], f"{what}: {k}: {a[k]!r} and {b[k]!r}"
    assert a["x"].tobytes() == b["x"].tobytes(), f"{what}: x"
    assert a["history"].tobytes() == b["history"].tobytes(), f"{what}: history"


# ---- 1. the dense solve, the explicit norms and the restatement --------------------------------------------------------------------

@pytest.mark.parametrize("restart", (20, 7))
@pytest.mark.parametrize("B", BLOCKS)
def test_blocked_sgs_against_the_dense_solve_and_the_restatement(eng, B, restart):
    P = problem()
    worst, counts = {}, {}
    for dtype, lim in PREC.items():
        name = np.dtype(dtype).name
        _, ref, ref_stop, ref_restarts = P.restatement(dtype, restart, B, lim["tol"])
        assert ref_stop == 1
        # a property of the input: the blocked SGS needs fewer steps than the Jacobi preconditioner
        _, jac, _, _ = P.restatement(dtype, restart, "minv", lim["tol"])
        assert ref.size < jac.size, (name, restart, B, ref.size, jac.size)
        if dtype == np.float64 and B in (64, 100):
            # the run-ahead is exercised, in the middle of a cycle in all but one case: B = 100 at restart 20 stops at step 80, a cycle's end
            assert ref.size > 2 * POLL and (ref.size % restart != 0) == ((B, restart) != (100, 20)), (B, restart, ref.size)
        bn = np.linalg.norm(P.b.astype(dtype).astype(np.float64))
        rows = np.nonzero(ref / bn > lim["ratio"])[0]
        assert rows[-1] == rows.size - 1                                   # a leading stretch
        assert rows.size >= lim["share"] * ref.size, f"{name}: {rows.size} of {ref.size} rows qualify"
        M = P.sgs(eng, dtype, B)
        for fmt, opts in LAYOUTS:
            A = P.handle(eng, fmt, dtype, **opts)
            what = f"convdiff(45) {A.format_name} {name} restart={restart} B={B}"
            got = A.gmres(P.b.astype(dtype), restart=restart, precond=M, tol=lim["tol"], max_iterations=MAX_ITERATIONS)
            A.close()
            k = got["iterations"]
            print(f"[gmres_tri] {what}: {k} iterations (the restatement {ref.size}, Jacobi {jac.size}), rnorm {got['rnorm']:.3g}")
            assert got["stop"] == 1, f"{what}: stop {got['stop']} after {k} iterations"
            assert got["x"].dtype == dtype and got["x"].shape == (P.n,) and got["history"].shape == (k,)
            assert got["prnorm"] == got["history"][-1] and got["prnorm"] <= lim["tol"] * got["rnorm0"] * (1 + 1e-12), what
            assert k + got["restarts"] + 1 <= got["spmv_calls"] <= k + got["restarts"] + 1 + allowance(restart), what
            for key, v in shares_of_the_bounds(P, got, dtype).items():
                print(f"[gmres_tri] {what}: {key} is {v:.3g} of its bound")
                assert v <= 1, f"{what}: {key} is {v:.3g} times its bound"
                worst[key] = max(worst.get(key, 0), float(v))
            counts[(name, fmt)] = (k, ref.size)
            assert abs(k - ref.size) <= 1 and k >= rows.size, f"{what}: {k} iterations, the restatement {ref.size}"
            assert got["restarts"] == (ref_restarts if k == ref.size else (k - 1) // restart), what
            d = np.abs(got["history"][rows] - ref[rows]) / ref[rows]
            print(f"[gmres_tri] {what}: largest history deviation {d.max():.3g} on {rows.size} rows")
            assert d.max() <= lim["hist"], f"{what}: history deviates by {d.max():.3g} at row {np.argmax(d)}"
        close(*M)
    print(f"[gmres_tri] B={B} restart={restart}: largest shares {worst}; (iterations, the restatement's) {counts}")


# ---- 2. the wiring, pinned to the bit ---------------------------------------------------------------------------------------------------

def test_a_scale_alone_is_the_solve_with_minv(eng):
    """precond = (None, s, None) with s > 0 is gmres(minv = s) bit for bit: x, the history and every info field. The separate scale
    kernel does the same one multiply as the fused path, in the inner steps and at the cycle ends."""
    P = problem()
    s = 1.0 / np.abs(P.diag) * (1 + 0.5 * np.sin(np.arange(P.n)))
    assert s.min() > 0
    for fmt, opts in LAYOUTS:
        for dtype, lim in PREC.items():
            A = P.handle(eng, fmt, dtype, **opts)
            for restart in (20, 7):
                a = A.gmres(P.b.astype(dtype), restart=restart, minv=s, tol=lim["tol"], max_iterations=MAX_ITERATIONS)
                b = A.gmres(P.b.astype(dtype), restart=restart, precond=(None, s, None), tol=lim["tol"], max_iterations=MAX_ITERATIONS)
                assert a["stop"] == 1 and a["restarts"] >= 1
                _same(a, b, f"{A.format_name} {np.dtype(dtype).name} restart={restart}")
            A.close()


# ---- 3. deterministic -----------------------------------------------------------------------------------------------------------------------

def test_two_solves_return_identical_bits(eng):
    P = problem()
    for dtype, lim in PREC.items():
        M = P.sgs(eng, dtype, 100)
        for fmt, opts in LAYOUTS:
            A = P.handle(eng, fmt, dtype, **opts)
            a = A.gmres(P.b.astype(dtype), restart=20, precond=M, tol=lim["tol"], max_iterations=MAX_ITERATIONS)
            b = A.gmres(P.b.astype(dtype), restart=20, precond=M, tol=lim["tol"], max_iterations=MAX_ITERATIONS)
            A.close()
            assert a["stop"] == 1
            _same(a, b, f"{fmt} {np.dtype(dtype).name}")
        close(*M)


# ---- 4. frozen after the stop -------------------------------------------------------------------------------------------------------

def raw_gmres_tri(eng, A, b, x, restart, M, tol, max_iterations, hist):
    """the C call on the caller's own buffers: (rc, info)"""
    info = eng.GmresInfo()
    info.struct_size = ctypes.sizeof(eng.GmresInfo)
    p = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
    first, scale, second = M
    S = eng.TriPrecond(ctypes.sizeof(eng.TriPrecond), None if first is None else first.h, p(scale), None if second is None else second.h)
    rc = eng.lib().spmv_mi355x_gmres_tri(A.h, p(b), p(x), restart, ctypes.byref(S), tol, max_iterations, p(hist), ctypes.byref(info))
    return rc, info


def test_frozen_after_the_stop(eng):
    """restart 20, B = 64: the stop falls past 2 * POLL = 64 in the middle of a cycle (step 121 of the restatement) and 200 more steps
    are allowed. The host runs ahead of the device; the triangular solves and the scale kernel it enqueued past the stop know nothing
    of the stop flag, and must leave x, the counters and the history as a solve that ends at the stop leaves them, the partial cycle
    applied exactly once."""
    P = problem()
    restart = 20
    b = np.ascontiguousarray(P.b)
    M = P.sgs(eng, np.float64, 64)
    for fmt, opts in LAYOUTS:
        A = P.handle(eng, fmt, np.float64, **opts)
        got = A.gmres(b, restart=restart, precond=M, tol=1e-12, max_iterations=MAX_ITERATIONS)
        k = got["iterations"]
        assert got["stop"] == 1 and k > 2 * POLL and k % restart != 0
        x_long, h_long = np.full(P.n, 7.0), np.full(k + 200, 7.0)
        rc, long_ = raw_gmres_tri(eng, A, b, x_long, restart, M, 1e-12, k + 200, h_long)
        assert rc == 0 and (long_.stop, long_.iterations) == (1, k)
        x_short, h_short = np.full(P.n, 7.0), np.full(k, 7.0)
        rc, short = raw_gmres_tri(eng, A, b, x_short, restart, M, 1e-12, k, h_short)
        assert rc == 0 and (short.stop, short.iterations) == (1, k)
        assert x_long.tobytes() == x_short.tobytes() == got["x"].tobytes()
        assert h_long[:k].tobytes() == h_short.tobytes() and np.all(h_long[:k] > 0)
        assert np.all(h_long[k:] == 0)
        assert (long_.restarts, long_.rnorm, long_.rnorm0, long_.prnorm, long_.xnorm) == \
               (short.restarts, short.rnorm, short.rnorm0, short.prnorm, short.xnorm)
        assert short.spmv_calls == k + short.restarts + 1
        assert k + long_.restarts + 1 <= long_.spmv_calls <= k + long_.restarts + 1 + allowance(restart)   # the host stopped enqueueing
        for key, v in shares_of_the_bounds(P, dict(got, x=x_long), np.float64).items():
            assert v <= 1, f"{A.format_name}: {key} is {v:.3g} times its bound"
        A.close()
    close(*M)


# ---- 5. tol = 0 -----------------------------------------------------------------------------------------------------------------------------

def test_tol_zero_runs_to_max_iterations(eng):
    """tol = 0 never stops on the tolerance: exactly max_iterations = 80 steps run at restart 7, B = 64 (the restatement converges at
    step 90), past the host's polling and no multiple of the restart length: the cycle end after the loop applies the partial cycle.
    x is the restatement's to the history tolerance: every cycle was applied once."""
    P = problem()
    restart, B, max_iterations = 7, 64, 80
    x_ref, ref, ref_stop, ref_restarts = P.restatement(np.float64, restart, B, 0.0, max_iterations)
    assert ref_stop == 2 and ref.size == max_iterations and ref_restarts == (max_iterations - 1) // restart
    rows = np.nonzero(ref / np.linalg.norm(P.b) > PREC[np.float64]["ratio"])[0]
    assert rows.size >= 40
    M = P.sgs(eng, np.float64, B)
    for fmt, opts in LAYOUTS:
        A = P.handle(eng, fmt, np.float64, **opts)
        got = A.gmres(P.b, restart=restart, precond=M, tol=0.0, max_iterations=max_iterations)
        what = f"{A.format_name} restart={restart} B={B}"
        A.close()
        assert (got["stop"], got["iterations"], got["restarts"]) == (2, max_iterations, ref_restarts), what
        assert got["history"].shape == (max_iterations,) and got["prnorm"] == got["history"][-1]
        assert got["spmv_calls"] == max_iterations + ref_restarts + 1, what
        d = np.abs(got["history"][rows] - ref[rows]) / ref[rows]
        assert d.max() <= PREC[np.float64]["hist"], f"{what}: history deviates by {d.max():.3g} at row {np.argmax(d)}"
        assert np.all(got["history"] > 0)
        dx = np.linalg.norm(got["x"] - x_ref) / np.linalg.norm(x_ref)
        assert dx <= PREC[np.float64]["hist"], f"{what}: x deviates from the restatement's by {dx:.3g}"
        for key, v in shares_of_the_bounds(P, got, np.float64, converged=False).items():
            assert v <= 1, f"{what}: {key} is {v:.3g} times its bound"
    close(*M)


# ---- 6. any handle serves ---------------------------------------------------------------------------------------------------------------

def test_a_global_handle_and_a_blocked_one_mix(eng):
    """first = the global LOWER handle, second = the UPPER one blocked at B = 100: the restatement with the same two operators"""
    P = problem()
    for dtype, lim in PREC.items():
        _, ref, ref_stop, _ = P.restatement(dtype, 20, None, lim["tol"], MAX_ITERATIONS, 100)
        assert ref_stop == 1
        M = P.sgs(eng, dtype, None, 100)
        assert M[0].block_info()["block_rows"] == 0 and M[2].block_info()["block_rows"] == 100
        A = P.handle(eng, "sell_c_sigma", dtype)
        got = A.gmres(P.b.astype(dtype), restart=20, precond=M, tol=lim["tol"], max_iterations=MAX_ITERATIONS)
        A.close()
        close(*M)
        assert got["stop"] == 1 and abs(got["iterations"] - ref.size) <= 1, (got["iterations"], ref.size)
        for key, v in shares_of_the_bounds(P, got, dtype).items():
            assert v <= 1, f"{np.dtype(dtype).name}: {key} is {v:.3g} times its bound"


def test_the_parts_alone(eng):
    """first alone and second alone (a Gauss-Seidel sweep each way as the right preconditioner) converge to the dense solve"""
    P = problem()
    L, s, U = P.sgs(eng, np.float64, 256)
    A = P.handle(eng, "sell_c_sigma", np.float64)
    for M in ((L, None, None), (None, None, U), (L, s, None), (None, s, U)):
        got = A.gmres(P.b, restart=20, precond=M, tol=1e-12, max_iterations=MAX_ITERATIONS)
        assert got["stop"] == 1, [type(m).__name__ for m in M]
        for key, v in shares_of_the_bounds(P, got, np.float64).items():
            assert v <= 1, f"{key} is {v:.3g} times its bound"
    A.close()
    close(L, U)


def test_a_value_storage_handle_solves_the_rounded_matrix(eng):
    """fp64 vectors over fp32-stored values give, bit for bit, the solve of the fp64 handle built from (double) (float) values, under
    the same preconditioner"""
    P = problem()
    rounded = P.csr[2].astype(np.float32).astype(np.float64)
    A4 = P.handle(eng, "sell_c_sigma", np.float64, **dict(DELTA, value_storage=1))
    A8 = P.handle(eng, "sell_c_sigma", np.float64, values=rounded, **dict(DELTA, sell_values=2))
    assert A4.format_name.endswith("_v4") and A4.value_dtype == np.float32 and A8.value_dtype == np.float64
    M = P.sgs(eng, np.float64, 100)
    a = A4.gmres(P.b, restart=20, precond=M, max_iterations=MAX_ITERATIONS)
    b = A8.gmres(P.b, restart=20, precond=M, max_iterations=MAX_ITERATIONS)
    A4.close()
    A8.close()
    close(*M)
    assert a["stop"] == 1
    _same(a, b, "value_storage = 1")
    Dr = P.D.astype(np.float32).astype(np.float64)
    assert np.linalg.norm(P.b - Dr @ a["x"]) <= 10 * 1e-12 * np.linalg.norm(P.b)          # the rounded matrix was solved


# ---- 7. the refusals that need a handle, in their order ---------------------------------------------------------------------------

def _refused(eng, A, n, M, phrases, struct_size=None, null=False):
    b, x, hist = np.full(n, 3.5), np.full(n, -7.25), np.full(10, 9.0)
    first, scale, second = M
    keep = None if scale is None else scale.copy()
    info = eng.GmresInfo()
    info.struct_size = ctypes.sizeof(eng.GmresInfo)
    info.iterations, info.stop, info.restarts, info.rnorm, info.spmv_calls = -5, -6, -4, -7.5, -8
    before = bytes(info)
    p = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
    S = eng.TriPrecond(ctypes.sizeof(eng.TriPrecond) if struct_size is None else struct_size, None if first is None else first.h,
                       p(scale), None if second is None else second.h)
    rc = eng.lib().spmv_mi355x_gmres_tri(A.h, p(b), p(x), 20, None if null else ctypes.byref(S), 1e-12, 10, p(hist), ctypes.byref(info))
    msg = eng.lib().spmv_mi355x_last_error()
    assert rc == 1 and msg.startswith(b"gmres_tri: ") and all(ph in msg for ph in phrases), msg
    assert np.all(b == 3.5) and np.all(x == -7.25) and np.all(hist == 9.0) and bytes(info) == before
    assert keep is None or keep.tobytes() == scale.tobytes()


def test_preconditioners_that_are_refused_in_their_order(eng):
    P = problem()
    rp, ci, va = P.csr
    A = P.handle(eng, "sell_c_sigma", np.float64)
    L, s, U = P.sgs(eng, np.float64, 100)
    small = eng.TriangularSolve(np.arange(4, dtype=np.int32), np.arange(3, dtype=np.int32), np.ones(3), 3, block_rows=2)
    single = eng.TriangularSolve(rp, ci, va, P.n, uplo="upper", dtype=np.float32, block_rows=100)
    bad = s.copy()
    bad[[7, 9]] = 0.0, np.nan
    # 1. M itself; whatever else is wrong comes later
    _refused(eng, A, P.n, (None, None, None), (b"NULL preconditioner",), null=True)
    _refused(eng, A, P.n, (small, bad, None), (b"struct_size",), struct_size=8)
    # 2. nothing in it
    _refused(eng, A, P.n, (None, None, None), (b"spmv_mi355x_gmres",))
    # 3. the handles, first before second, before the scale
    _refused(eng, A, P.n, (small, bad, single), (b"M->first", b"3 rows", b"2025"))
    _refused(eng, A, P.n, (L, bad, small), (b"M->second", b"3 rows"))
    _refused(eng, A, P.n, (L, bad, single), (b"M->second", b"precision"))
    _refused(eng, A, P.n, (single, None, U), (b"M->first", b"precision"))
    # 4. the scale: the first index that is zero or not finite; a negative entry is legal
    _refused(eng, A, P.n, (L, bad, U), (b"scale[7] = 0",))
    for at, value in ((0, np.nan), (2024, np.inf), (1000, -np.inf)):
        one = s.copy()
        one[at] = value
        _refused(eng, A, P.n, (None, one, None), (f"scale[{at}]".encode(),))
    with pytest.raises(eng.SpmvError, match=r"gmres_tri: scale\[7\]"):
        A.gmres(P.b, precond=(L, bad, U))
    with pytest.raises(ValueError, match="minv and precond"):
        A.gmres(P.b, minv=np.abs(s), precond=(L, s, U))
    got = A.gmres(P.b, restart=20, precond=(None, -np.abs(1.0 / s), None), tol=1e-12, max_iterations=MAX_ITERATIONS)
    assert got["stop"] == 1                                                   # a negative scale is a preconditioner like any other
    A.close()
    close(L, U, small, single)
