"""spmv_mi355x_gmres / Matrix.gmres (include/spmv_mi355x.h "GMRES(m)"): A x = b for a square nonsymmetric A on one handle.

References, none of them the engine: numpy.linalg.solve on the dense matrix for the solution, numpy's explicit norms of the RETURNED
x for info.rnorm / xnorm, and a numpy restatement of the header's recurrences (vectors in the handle's precision, dots and scalars
in fp64, like the solver) for the history, the iteration count and the restarts. Problems and references are computed once per
(shape, precision, restart, minv) and are read-only.

Test matrix nsym(n), seed 3000 + n: row i has d on the diagonal and, for each j of rng.choice(n, min(4, n), replace=False) with
j != i, an entry uniform in (-1, 1); d = 1.5 for n >= 700 and 2.0 below. Nothing about it is symmetric. b = default_rng(7)
.uniform(-1, 1, n). cond(A) <= 22 for the shapes used (asserted <= KAPPA = 25 below from the singular values). With the restatement,
for n in {2000, 1025, 700} and restart in {20, 7}: fp64 at tol 1e-12 stops after 104 .. 125 inner steps, past 2 * POLL = 64 (the
host's run-ahead and its stop on the progress word are exercised), in the middle of a cycle in all but one case (the pending-columns
path is exercised; nsym(700) with minv at m = 20 stops at step 120, the end of one), after >= 5 restarts at m = 20 and >= 14 at m = 7; fp32 at tol 1e-5 stops after 41 .. 51. Shapes: the smallest that exercise several
blocks of the vector kernels (1024 rows each), one row past a block, below a block, and 1 (the second trip of the partial sums and
the cap of the grid need 262 145 and 1 049 601 unknowns: test_gpu_solver_sizes.py).

The preconditioner under test: minv_i = (1 / |d_ii|) (1 + 0.5 sin(i)). It is a RIGHT preconditioner: the residual stays the true one.

Bounds:
  * stop 1 guarantees |g| <= tol |b| for the recursive 2-norm residual; the explicit one may exceed it by the project's factor 10
    (the CGLS and MINRES tests'): info.rnorm <= 10 tol |b|.
  * |x - x*| / |x*| <= kappa * that bound / |b| = KAPPA 10 tol.
  * rnorm, xnorm against numpy's explicit values of the returned x: 1e-10 (fp64) / 1e-4 (fp32) relative, rnorm plus the cancellation
    floor of cancellation_floor() (the residual at convergence is a difference of terms far larger than itself).
  * rnorm0 = |b| against numpy: an fp64 sum of products of values of the handle's precision: 1e-13 (fp64) / 1e-6 (fp32) relative.
  * iterations within 1 of the restatement's, restarts = (iterations - 1) // restart, the restatement's own rule.
  * history against the restatement: rows with |g_k| / |b| above 1e-8 (fp64) / 1e-2 (fp32) to rtol 1e-6 / 1e-3 (the CGLS and MINRES
    tests' bounds); at least 60 % of the fp64 rows and 30 % of the fp32 rows qualify. Two summation orders of the restatement itself
    (a symmetric permutation of the problem) differ on those rows by at most 5.1e-10 / 5.5e-7."""
import ctypes
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SHAPES = [2000, 1025, 700, 40, 3, 1]
LAYOUTS = [("sell_c_sigma", {}), ("sell_c_sigma", {"sell_window": 2}), ("csr_vector", {})]
DELTA = dict(sell_c=64, sell_delta=1, sell_sigma=64, sell_window=2)
CASES = ((20, False), (7, False), (20, True), (7, True))                     # (restart, minv given)
KAPPA = 25.0
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


# ---- problems and references (computed once, read-only) ----------------------------------------------------------------------------

def dense_to_csr(D):
    m = D.shape[0]
    rows, cols = np.nonzero(D)                           # row-major: rows in order, columns ascending
    rp = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=m))]).astype(np.int32)
    return rp, cols.astype(np.int32), np.ascontiguousarray(D[rows, cols], np.float64)


def nsym(n):
    rng = np.random.default_rng(3000 + n)
    d = 1.5 if n >= 700 else 2.0
    D = np.zeros((n, n))
    for i in range(n):
        D[i, i] = d
        for j in rng.choice(n, min(4, n), replace=False):
            if j != i:
                D[i, j] = rng.uniform(-1, 1)
    return D


def restate(A, b, m, minv, tol, max_iterations, dtype, dot=None):
    """the header's recurrences in numpy: vectors in `dtype`, dots and scalars in fp64. A is a matrix of `dtype`, dense or
    scipy.sparse (only A @ v is taken). `dot` replaces the fp64 dot product (test_solver_size_cases.py: a dot that loses rows).
    Returns (x, history, stop, restarts)."""
    dt = np.dtype(dtype).type
    n = len(b)
    b = b.astype(dt)
    dot = dot or (lambda u, v: float(u.astype(np.float64) @ v.astype(np.float64)))
    M = (lambda v: v) if minv is None else (lambda v, d=minv.astype(dt): d * v)
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
    def __init__(self, n):
        D = nsym(n)
        self.n, self.D = n, D
        self.csr = dense_to_csr(D)
        self.k_row = int((D != 0).sum(axis=1).max())
        self.b = np.random.default_rng(7).uniform(-1, 1, n)
        self.minv = 1.0 / np.abs(np.diag(D)) * (1 + 0.5 * np.sin(np.arange(n)))
        assert self.minv.min() > 0
        for v in (D, self.b, self.minv) + self.csr:
            v.setflags(write=False)

    def handle(self, eng, fmt, dtype, values=None, **opts):
        rp, ci, va = self.csr
        return eng.Matrix(rp, ci, va if values is None else values, self.n, self.n, fmt, dtype, **opts)

    def pre(self, given):
        return self.minv if given else None

    @functools.lru_cache(maxsize=None)
    def solve(self):
        sv = np.linalg.svd(self.D, compute_uv=False)
        assert sv[0] / sv[-1] <= KAPPA, (self.n, sv[0] / sv[-1])
        x = np.linalg.solve(self.D, self.b)
        x.setflags(write=False)
        return x

    @functools.lru_cache(maxsize=None)
    def dense(self, dtype):
        A = self.D.astype(dtype)
        A.setflags(write=False)
        return A

    @functools.lru_cache(maxsize=None)
    def restatement(self, dtype, restart, given, tol, max_iterations=MAX_ITERATIONS):
        x, hist, stop, restarts = restate(self.dense(dtype), self.b, restart, self.pre(given), tol, max_iterations, dtype)
        x.setflags(write=False)
        hist.setflags(write=False)
        return x, hist, stop, restarts


@functools.lru_cache(maxsize=None)
def problem(n):
    return Problem(n)


def explicit_norms(P, x):
    """numpy's explicit values for a returned x, in fp64 whatever the precision of x"""
    x = x.astype(np.float64)
    return np.linalg.norm(P.b - P.D @ x), np.linalg.norm(x)


def cancellation_floor(P, x, dtype):
    """How far two correct evaluations of |b - A x| for the same x can lie apart, to first order in the unit roundoffs u (the
    handle's precision) and u64 (numpy's): by the reverse triangle inequality the norms differ by at most the norm of the difference
    of the vectors. Component i: a sum of k products in any order, fused or not, errs by <= k u (|A| |x|)_i, k the most entries of a
    row; the subtraction from b_i adds u (|b_i| + (|A| |x|)_i); an fp32 handle holds A and b rounded to fp32, one more u on each of
    the two terms. The same for numpy with u64 and nothing rounded on storage."""
    u, u64, store = float(np.finfo(dtype).eps) / 2, 2.0 ** -53, int(np.dtype(dtype) == np.float32)
    x = np.abs(x.astype(np.float64))
    k = P.k_row
    ax, bn = np.linalg.norm(np.abs(P.D) @ x), np.linalg.norm(P.b)
    return (u * (k + store + 1) + u64 * (k + 1)) * ax + (u * (1 + store) + u64) * bn


def raw_gmres(eng, A, b, x, restart, minv, tol, max_iterations, hist):
    """the C call on the caller's own buffers: (rc, info)"""
    info = eng.GmresInfo()
    info.struct_size = ctypes.sizeof(eng.GmresInfo)
    p = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
    rc = eng.lib().spmv_mi355x_gmres(A.h, p(b), p(x), restart, p(minv), tol, max_iterations, p(hist), ctypes.byref(info))
    return rc, info


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


# ---- 1. against the dense solve, 2. history, iterations and restarts against the restatement --------------------------------------

@pytest.mark.parametrize("n", SHAPES)
def test_against_the_dense_solve(eng, n):
    P = problem(n)
    worst = {}
    for fmt, opts in LAYOUTS:
        for dtype, lim in PREC.items():
            A = P.handle(eng, fmt, dtype, **opts)
            for restart, given in CASES:
                what = f"nsym({n}) {A.format_name} {np.dtype(dtype).name} restart={restart} minv={given}"
                got = A.gmres(P.b.astype(dtype), restart=restart, minv=P.pre(given), tol=lim["tol"], max_iterations=MAX_ITERATIONS)
                k = got["iterations"]
                assert got["stop"] == 1, f"{what}: stop {got['stop']} after {k} iterations"
                assert got["x"].dtype == dtype and got["x"].shape == (P.n,) and got["history"].shape == (k,)
                assert got["prnorm"] == got["history"][-1] and got["prnorm"] <= lim["tol"] * got["rnorm0"] * (1 + 1e-12), what
                assert got["restarts"] == (k - 1) // restart, what
                assert k + got["restarts"] + 1 <= got["spmv_calls"] <= k + got["restarts"] + 1 + allowance(restart), what
                for key, v in shares_of_the_bounds(P, got, dtype).items():
                    assert v <= 1, f"{what}: {key} is {v:.3g} times its bound ({k} iterations, rnorm {got['rnorm']!r}, " \
                                   f"rnorm0 {got['rnorm0']!r}, xnorm {got['xnorm']!r})"
                    worst[key] = max(worst.get(key, 0), float(v))
            A.close()
    print(f"[gmres] nsym({n}): largest shares of the bounds " + ", ".join(f"{k} {v:.2g}" for k, v in worst.items()))


@pytest.mark.parametrize("n", SHAPES)
def test_history_against_the_restatement(eng, n):
    P = problem(n)
    worst, counts = {}, {}
    for fmt, opts in LAYOUTS:
        for dtype, lim in PREC.items():
            A = P.handle(eng, fmt, dtype, **opts)
            for restart, given in CASES:
                what = f"nsym({n}) {A.format_name} {np.dtype(dtype).name} restart={restart} minv={given}"
                got = A.gmres(P.b.astype(dtype), restart=restart, minv=P.pre(given), tol=lim["tol"], max_iterations=MAX_ITERATIONS)
                _, ref, ref_stop, ref_restarts = P.restatement(dtype, restart, given, lim["tol"])
                assert ref_stop == 1
                bn = np.linalg.norm(P.b.astype(dtype).astype(np.float64))
                rows = np.nonzero(ref / bn > lim["ratio"])[0]
                assert rows.size == 0 or rows[-1] == rows.size - 1                 # a leading stretch: |g| never increases in a cycle
                if n >= 700:
                    assert rows.size >= lim["share"] * ref.size, f"{what}: {rows.size} of {ref.size} rows qualify"
                    if dtype == np.float64:                                        # the run-ahead is exercised
                        assert ref.size > 2 * POLL, (what, ref.size)
                        assert ref_restarts >= (5 if restart == 20 else 14), (what, ref_restarts)
                k = got["iterations"]
                counts[(np.dtype(dtype).name, restart, given)] = (k, ref.size)
                assert abs(k - ref.size) <= 1 and k >= rows.size, f"{what}: {k} iterations, the restatement {ref.size}"
                assert got["restarts"] == (ref_restarts if k == ref.size else (k - 1) // restart), what
                if rows.size:
                    d = np.abs(got["history"][rows] - ref[rows]) / ref[rows]
                    worst[np.dtype(dtype).name] = max(worst.get(np.dtype(dtype).name, 0), float(d.max()))
                    assert d.max() <= lim["hist"], f"{what}: history deviates by {d.max():.3g} at row {np.argmax(d)}"
            A.close()
    print(f"[gmres] nsym({n}): largest history deviation {worst}; (iterations, the restatement's) {counts}")


# ---- 3. deterministic -----------------------------------------------------------------------------------------------------------------------

def _same(a, b, what):
    for k in INFO_FIELDS:
        assert a[k] == b[k], f"{what}: {k}"
    assert a["x"].tobytes() == b["x"].tobytes(), f"{what}: x"
    assert a["history"].tobytes() == b["history"].tobytes(), f"{what}: history"


def test_two_solves_return_identical_bits(eng):
    for n in (2000, 700):
        P = problem(n)
        for fmt, opts in LAYOUTS:
            for dtype, lim in PREC.items():
                A = P.handle(eng, fmt, dtype, **opts)
                for restart, given in ((20, False), (7, True)):
                    a = A.gmres(P.b.astype(dtype), restart=restart, minv=P.pre(given), tol=lim["tol"], max_iterations=MAX_ITERATIONS)
                    b = A.gmres(P.b.astype(dtype), restart=restart, minv=P.pre(given), tol=lim["tol"], max_iterations=MAX_ITERATIONS)
                    assert a["stop"] == 1
                    _same(a, b, f"nsym({n}) {A.format_name} {np.dtype(dtype).name} restart={restart} minv={given}")
                A.close()


# ---- 4. frozen after the stop -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("restart,given", ((20, True), (20, False), (7, False)))
def test_frozen_after_the_stop(eng, restart, given):
    """The stop falls past 2 * POLL = 64, for restart = 20 in the middle of a cycle (steps 105 and 122 of the restatement; 120 on
    nsym(700) with minv, the end of a cycle, is met by the tests above), and 200 more steps are allowed: the host runs ahead of the device,
    waits on the progress word and stops on what was posted; whatever it enqueued past the stop (steps, cycle ends, restarts) must
    leave x, the counters and the history as a solve that ends at the stop leaves them, the partial cycle applied exactly once."""
    P = problem(2000)
    b, minv = np.ascontiguousarray(P.b), np.ascontiguousarray(P.minv) if given else None
    for fmt, opts in LAYOUTS[:2]:
        A = P.handle(eng, fmt, np.float64, **opts)
        got = A.gmres(b, restart=restart, minv=minv, tol=1e-12, max_iterations=MAX_ITERATIONS)
        k = got["iterations"]
        assert got["stop"] == 1 and k > 2 * POLL and (restart == 7 or k % restart != 0)
        x_long, h_long = np.full(P.n, 7.0), np.full(k + 200, 7.0)
        rc, long_ = raw_gmres(eng, A, b, x_long, restart, minv, 1e-12, k + 200, h_long)
        assert rc == 0 and (long_.stop, long_.iterations) == (1, k)
        x_short, h_short = np.full(P.n, 7.0), np.full(k, 7.0)
        rc, short = raw_gmres(eng, A, b, x_short, restart, minv, 1e-12, k, h_short)
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


# ---- 5. tol = 0 -----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("restart,max_iterations", ((7, 84), (7, 80), (20, 100), (20, 93), (1, 40)))
def test_tol_zero_runs_to_max_iterations(eng, restart, max_iterations):
    """tol = 0 never stops on the tolerance: exactly max_iterations steps run, past the host's polling, for a multiple of the restart
    length (the last cycle end inside the loop applies the cycle, the one after the loop finds nothing) and for a non-multiple (the
    one after the loop applies the partial cycle). x is the restatement's to the history tolerance: every cycle was applied once."""
    P = problem(1025)
    for given in (False, True):
        x_ref, ref, ref_stop, ref_restarts = P.restatement(np.float64, restart, given, 0.0, max_iterations)
        assert ref_stop == 2 and ref.size == max_iterations and ref_restarts == (max_iterations - 1) // restart
        rows = np.nonzero(ref / np.linalg.norm(P.b) > PREC[np.float64]["ratio"])[0]
        assert rows.size >= 40
        for fmt, opts in LAYOUTS:
            A = P.handle(eng, fmt, np.float64, **opts)
            got = A.gmres(P.b, restart=restart, minv=P.pre(given), tol=0.0, max_iterations=max_iterations)
            what = f"{A.format_name} restart={restart} minv={given}"
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
            A.close()


# ---- 6. restart = 1, n = 1 --------------------------------------------------------------------------------------------------------------

def test_restart_one_converges(eng):
    """GMRES(1): every step is a cycle, one column, one rotation, a restart with its explicit residual. On nsym(40) (the symmetric
    part is positive definite: diagonal 2, at most 8 off-diagonals below 1/2 in a row of it, most rows far fewer) it converges."""
    P = problem(40)
    for dtype, lim in PREC.items():
        _, ref, ref_stop, ref_restarts = P.restatement(dtype, 1, False, lim["tol"])
        assert ref_stop == 1 and ref_restarts == ref.size - 1
        for fmt, opts in LAYOUTS:
            A = P.handle(eng, fmt, dtype, **opts)
            got = A.gmres(P.b.astype(dtype), restart=1, tol=lim["tol"], max_iterations=MAX_ITERATIONS)
            what = f"{A.format_name} {np.dtype(dtype).name}"
            assert got["stop"] == 1 and abs(got["iterations"] - ref.size) <= 1, f"{what}: {got['iterations']} vs {ref.size}"
            assert got["restarts"] == got["iterations"] - 1, what
            for key, v in shares_of_the_bounds(P, got, dtype).items():
                assert v <= 1, f"{what}: {key} is {v:.3g} times its bound"
            A.close()


def test_one_unknown(eng):
    """n = 1: one step solves it: whatever w - (v.w) v leaves, |g_1| is of the order of the roundoff, far below any tolerance."""
    P = problem(1)
    for fmt, opts in LAYOUTS:
        for dtype, lim in PREC.items():
            A = P.handle(eng, fmt, dtype, **opts)
            for given in (False, True):
                _, ref, ref_stop, _ = P.restatement(dtype, 7, given, lim["tol"], 10)
                assert (ref_stop, ref.size) == (1, 1)
                got = A.gmres(P.b.astype(dtype), restart=7, minv=P.pre(given), tol=lim["tol"], max_iterations=10)
                assert (got["stop"], got["iterations"], got["restarts"]) == (1, 1, 0), (A.format_name, given, got)
                want = P.b[0] / P.D[0, 0]
                assert abs(got["x"][0] - want) <= 4 * np.finfo(dtype).eps * abs(want)
                # 10 steps are allowed, fewer than 2 * POLL: the host enqueues them all, the restart after step 7 included
                assert 2 <= got["spmv_calls"] <= 2 + allowance(7) and got["spmv_calls"] == 10 + 1 + 1
            A.close()


# ---- 7. the other stops -----------------------------------------------------------------------------------------------------------------

def test_the_other_stops(eng):
    P = problem(40)
    for fmt, opts in LAYOUTS:
        for given in (False, True):
            A = P.handle(eng, fmt, np.float64, **opts)
            got = A.gmres(np.zeros(P.n), minv=P.pre(given))                    # b = 0
            assert (got["stop"], got["iterations"], got["restarts"]) == (3, 0, 0) and not got["x"].any()
            assert got["history"].shape == (0,)
            assert (got["rnorm"], got["rnorm0"], got["prnorm"], got["xnorm"]) == (0, 0, 0, 0)
            got = A.gmres(P.b, minv=P.pre(given), max_iterations=0)            # no step allowed
            assert (got["stop"], got["iterations"], got["restarts"]) == (2, 0, 0) and not got["x"].any()
            assert got["rnorm"] == got["rnorm0"] and abs(got["rnorm0"] - np.linalg.norm(P.b)) <= 1e-14 * np.linalg.norm(P.b)
            assert got["prnorm"] == got["rnorm0"] and got["xnorm"] == 0
            assert got["spmv_calls"] == 1
            A.close()


@pytest.mark.parametrize("dtype", (np.float64, np.float32), ids=("f64", "f32"))
def test_the_krylov_space_ends(eng, dtype):
    """A = 2 I, n = 40, b = 2 e_5 (|b| = 2 and v_0 = e_5 are exact, a b of general entries has v_0.v_0 != 1 and hn of the order of
    the roundoff squared, not 0): w = 2 e_5, c = 2, w - c v_0 == 0, hn == 0 with rho = 2: after 1 step stop 5 with tol = 0, stop 1
    (|g_1| = 0) with a tolerance, and x = b / 2 exactly. The restatement agrees."""
    n = 40
    rp, ci, va = np.arange(n + 1, dtype=np.int32), np.arange(n, dtype=np.int32), np.full(n, 2.0)
    b = np.zeros(n)
    b[5] = 2.0
    x_ref, ref, ref_stop, _ = restate(2 * np.eye(n, dtype=dtype), b, 7, None, 0.0, 50, dtype)
    assert ref_stop == 5 and ref.tolist() == [0.0] and np.array_equal(x_ref, b / 2)
    for fmt, opts in LAYOUTS:
        A = eng.Matrix(rp, ci, va, n, n, fmt, dtype, **opts)
        for tol, stop in ((0.0, 5), (PREC[dtype]["tol"], 1)):
            got = A.gmres(b.astype(dtype), restart=7, tol=tol, max_iterations=50)
            assert (got["stop"], got["iterations"], got["restarts"]) == (stop, 1, 0), f"{A.format_name} tol={tol}: {got}"
            assert np.array_equal(got["x"], (b / 2).astype(dtype))
            assert got["prnorm"] == 0 and got["history"].tolist() == [0.0] and got["rnorm"] == 0 and got["rnorm0"] == 2
        A.close()


def test_a_nan_in_the_matrix_is_a_breakdown(eng):
    P = problem(40)
    rp, ci, va = P.csr
    va = va.copy()
    va[5] = np.nan
    for fmt, opts in LAYOUTS:
        for given in (False, True):
            A = eng.Matrix(rp, ci, va, P.n, P.n, fmt, np.float64, **opts)
            got = A.gmres(P.b, minv=P.pre(given), max_iterations=50)
            assert (got["stop"], got["iterations"]) == (4, 0), f"{A.format_name}: {got['stop']}, {got['iterations']}"
            assert not got["x"].any() and got["history"].shape == (0,)
            A.close()


# ---- 8. refusals that need a handle ---------------------------------------------------------------------------------------------------

def _refused(eng, A, n_b, minv, phrases):
    b, x, hist = np.full(n_b, 3.5), np.full(n_b, -7.25), np.full(10, 9.0)
    keep = None if minv is None else minv.copy()
    info = eng.GmresInfo()
    info.struct_size = ctypes.sizeof(eng.GmresInfo)
    info.iterations, info.stop, info.restarts, info.rnorm, info.spmv_calls = -5, -6, -4, -7.5, -8
    before = bytes(info)
    p = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
    rc = eng.lib().spmv_mi355x_gmres(A.h, p(b), p(x), 20, p(minv), 1e-12, 10, p(hist), ctypes.byref(info))
    msg = eng.lib().spmv_mi355x_last_error()
    assert rc == 1 and b"gmres" in msg and all(ph in msg for ph in phrases), msg
    assert np.all(b == 3.5) and np.all(x == -7.25) and np.all(hist == 9.0) and bytes(info) == before
    assert keep is None or keep.tobytes() == minv.tobytes()


def test_handles_and_preconditioners_that_are_refused(eng):
    rng = np.random.default_rng(5)
    R = np.zeros((257, 63))
    for i in range(257):
        R[i, rng.choice(63, 4, replace=False)] = rng.uniform(-1, 1, 4)
    rp, ci, va = dense_to_csr(R)
    A = eng.Matrix(rp, ci, va, 257, 63, "csr_vector", np.float64)
    _refused(eng, A, 257, None, (b"257 x 63",))
    with pytest.raises(eng.SpmvError, match="gmres.*257 x 63"):
        A.gmres(np.ones(257))
    with pytest.raises(ValueError, match="b must have 257 values"):
        A.gmres(np.ones(63))
    A.close()

    P = problem(1025)
    for dtype in (np.float64, np.float32):
        A = P.handle(eng, "sell_c_sigma", dtype)
        for at, value in ((0, 0.0), (511, -0.5), (1024, np.nan), (700, np.inf)):
            minv = P.minv.astype(dtype)
            minv[at] = value
            _refused(eng, A, P.n, minv, (f"minv[{at}]".encode(),))
        minv = P.minv.astype(dtype)
        minv[[3, 9]] = -1.0, np.nan
        _refused(eng, A, P.n, minv, (b"minv[3]",))                            # the first such index
        with pytest.raises(eng.SpmvError, match=r"gmres: minv\[3\]"):
            A.gmres(P.b, minv=minv)
        with pytest.raises(eng.SpmvError, match="gmres: restart must be"):
            A.gmres(P.b, restart=129)
        A.close()


# ---- 9. handle support ------------------------------------------------------------------------------------------------------------------

def test_a_value_storage_handle_solves_the_rounded_matrix(eng):
    """DESIGN §4d's contract for the other solvers: fp64 vectors over fp32-stored values give, bit for bit, the solve of the fp64
    handle built from (double) (float) values (sell_values = 2: plain 8-byte values), and of the one that stores them in 7 bytes
    (sell_values = 1: lossless)."""
    P = problem(700)
    rounded = P.csr[2].astype(np.float32).astype(np.float64)
    A4 = P.handle(eng, "sell_c_sigma", np.float64, **dict(DELTA, value_storage=1))
    A8 = P.handle(eng, "sell_c_sigma", np.float64, values=rounded, **dict(DELTA, sell_values=2))
    A7 = P.handle(eng, "sell_c_sigma", np.float64, values=rounded, **dict(DELTA, sell_values=1))
    assert A4.format_name.endswith("_v4") and A4.value_dtype == np.float32
    assert not A8.format_name.endswith("_v4") and A8.value_dtype == np.float64 and A7.value_dtype == np.float64
    Dr = P.D.astype(np.float32).astype(np.float64)
    for restart, given in CASES:
        a = A4.gmres(P.b, restart=restart, minv=P.pre(given), max_iterations=MAX_ITERATIONS)
        b = A8.gmres(P.b, restart=restart, minv=P.pre(given), max_iterations=MAX_ITERATIONS)
        c = A7.gmres(P.b, restart=restart, minv=P.pre(given), max_iterations=MAX_ITERATIONS)
        assert a["stop"] == 1
        _same(a, b, f"restart={restart} minv={given}")
        _same(a, c, f"7-byte values, restart={restart} minv={given}")
        assert np.linalg.norm(P.b - Dr @ a["x"]) <= 10 * 1e-12 * np.linalg.norm(P.b)          # the rounded matrix was solved
    A4.close()
    A8.close()
    A7.close()
