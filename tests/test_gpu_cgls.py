"""spmv_mi355x_cgls / Matrix.cgls (include/spmv_mi355x.h "CGLS"): min |A x - b|^2 + damp |x|^2 over a handle of A and one of A^t.

References, none of them the engine: numpy.linalg.lstsq on the dense matrix (damped: on the stacked system [A; sqrt(damp) I],
[b; 0]) for the solution, numpy's explicit norms of the RETURNED x for info.rnorm / arnorm / xnorm, and a numpy restatement of the
recurrences (vectors in the handle's precision, dots in fp64, like the solver) for the history. Problems and references are
computed once per (shape, damp) and are read-only.

Test matrices: every row has min(6, n) entries at distinct random columns, uniform in (-0.5, 0.5); then A[i % m, i % n] += 4 for
i < max(m, n). cond(A) <= 1.7 at every shape used (asserted below), and the restatement reaches |s| <= 1e-12 |s0| in <= 21
iterations. Shapes: the smallest that exercise the solver's grid, nb = max(ceil(m / 1024), ceil(n / 1024)) blocks striding over
vectors of both lengths (tall 3 and 2, wide 1 and 3, one row past a block, below a block, and 1). A grid of 257 blocks of which 255
have no element of the short vectors: test_gpu_solver_sizes.py.

Bounds, where the issue behind this file left a scale open:
  * |x - x*| / |x*| <= kappa^2 * tol with kappa^2 taken as 3 (|(A^t A + damp)^-1| * |s|): 3e-12 (fp64, tol 1e-12), 3e-5 (fp32, 1e-5).
  * info.arnorm <= 10 * tol * arnorm0.
  * rnorm, arnorm, xnorm against numpy's explicit values of the returned x: 1e-10 (fp64) / 1e-4 (fp32) relative to numpy's value.
    Where the quantity is a difference of terms far larger than itself — arnorm = |A^t (b - A x) - damp x| at convergence, and
    rnorm = |b - A x| of the consistent systems (m <= n: full row rank) — the cancellation floor of cancellation_floor() is added:
    the first-order worst-case rounding error of the two evaluations, from the unit roundoffs, the entries per row and column and
    norms of the problem alone. It is about 10 eps |b| for rnorm and |A| times that for arnorm. rnorm of the inconsistent systems
    (m > n) and xnorm keep the plain relative bound.
  * history against the restatement: rows with |s_k| / |s0| above 1e-8 (fp64) / 1e-2 (fp32) to rtol 1e-6 / 1e-3 — the roundoff
    bound eps * kappa^2 * k divided by the ratio."""
import ctypes
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SHAPES = [(3000, 1100), (700, 2500), (1025, 1025), (257, 63), (5, 1), (1, 5), (1, 1)]
LAYOUTS = [("sell_c_sigma", {}), ("sell_c_sigma", {"sell_window": 2}), ("csr_vector", {})]
DELTA = dict(sell_c=64, sell_delta=1, sell_sigma=64, sell_window=2)
DAMPS = (0.0, 0.25)
PREC = {np.float64: dict(tol=1e-12, x=3e-12, norms=1e-10, ratio=1e-8, hist=1e-6),
        np.float32: dict(tol=1e-5, x=3e-5, norms=1e-4, ratio=1e-2, hist=1e-3)}


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


def np_transpose(rp, ci, va, m, n):
    """the caller's own CSR of A^t: a stable sort of the entries by column"""
    rows = np.repeat(np.arange(m, dtype=np.int32), np.diff(rp))
    order = np.argsort(ci, kind="stable")
    rp_t = np.concatenate([[0], np.cumsum(np.bincount(ci, minlength=n))]).astype(np.int32)
    return rp_t, rows[order].astype(np.int32), np.ascontiguousarray(va[order], np.float64)


def restate(A, At, b, damp, tol, max_iterations, dtype):
    """the recurrences in numpy: vectors in `dtype`, dots and scalars in fp64. A and At are matrices of `dtype`, dense or
    scipy.sparse (only A @ v and At @ v are taken). Returns (x, history rows (|r|, |s|), |s0|)."""
    dt = np.dtype(dtype).type
    dot = lambda v: float(v.astype(np.float64) @ v.astype(np.float64))
    x, r = np.zeros(A.shape[1], dt), b.astype(dt)
    s = At @ r
    p, gamma = s.copy(), dot(s)
    gamma0, hist = gamma, []
    for _ in range(max_iterations):
        q = A @ p
        alpha = dt(gamma / (dot(q) + damp * dot(p)))
        x = x + alpha * p
        r = r - alpha * q
        s = At @ r - dt(damp) * x
        gamma_new = dot(s)
        p = s + dt(gamma_new / gamma) * p
        gamma = gamma_new
        hist.append((np.sqrt(dot(r)), np.sqrt(gamma)))
        if np.sqrt(gamma) <= tol * np.sqrt(gamma0):
            break
    return x, np.array(hist), np.sqrt(gamma0)


class Problem:
    def __init__(self, m, n):
        rng = np.random.default_rng(1000 * m + n)
        D = np.zeros((m, n))
        for i in range(m):
            D[i, rng.choice(n, min(6, n), replace=False)] = rng.uniform(-0.5, 0.5, min(6, n))
        for i in range(max(m, n)):
            D[i % m, i % n] += 4.0
        self.m, self.n, self.D = m, n, D
        self.csr = dense_to_csr(D)
        sv = np.linalg.svd(D, compute_uv=False)
        assert sv[0] / sv[-1] <= 1.7, (m, n)
        self.norm2 = float(sv[0])
        self.k_row, self.k_col = int((D != 0).sum(axis=1).max()), int((D != 0).sum(axis=0).max())
        self.b = rng.uniform(-1, 1, m)
        for v in (D, self.b) + self.csr:
            v.setflags(write=False)

    def handles(self, eng, fmt, dtype, values=None, **opts):
        rp, ci, va = self.csr
        va = va if values is None else values
        return (eng.Matrix(rp, ci, va, self.m, self.n, fmt, dtype, **opts),
                eng.Matrix(rp, ci, va, self.m, self.n, fmt, dtype, transpose=1, **opts))

    @functools.lru_cache(maxsize=None)
    def lstsq(self, damp):
        if damp == 0:
            x = np.linalg.lstsq(self.D, self.b, rcond=None)[0]           # the minimum-norm solution when n > m
        else:
            S = np.vstack([self.D, np.sqrt(damp) * np.eye(self.n)])
            x = np.linalg.lstsq(S, np.concatenate([self.b, np.zeros(self.n)]), rcond=None)[0]
        x.setflags(write=False)
        return x

    @functools.lru_cache(maxsize=None)
    def restatement(self, dtype, damp, tol, max_iterations=300):
        """restate() on the dense matrix. Returns (x, history rows (|r|, |s|), |s0|)."""
        A = self.D.astype(dtype)
        x, hist, s0 = restate(A, A.T, self.b, damp, tol, max_iterations, dtype)
        hist.setflags(write=False)
        return x, hist, s0


@functools.lru_cache(maxsize=None)
def problem(m, n):
    return Problem(m, n)


def explicit_norms(P, x, damp):
    """numpy's explicit values for a returned x, in fp64 whatever the precision of x"""
    x = x.astype(np.float64)
    r = P.b - P.D @ x
    return np.linalg.norm(r), np.linalg.norm(P.D.T @ r - damp * x), np.linalg.norm(x)


def cancellation_floor(P, x, damp, dtype):
    """(floor of rnorm, floor of arnorm): how far two correct evaluations of |b - A x| and |A^t (b - A x) - damp x| for the same x
    can lie apart, to first order in the unit roundoffs u (the handle's precision) and u64 (numpy's). By the reverse triangle
    inequality the norms differ by at most the norm of the difference of the vectors.
      residual, component i: a sum of k products in any order, fused or not, errs by <= k u (|A| |x|)_i; the subtraction from b_i
        adds u (|b_i| + (|A| |x|)_i); an fp32 handle holds A and b rounded to fp32, one more u on each of the two terms. With k the
        most entries of a row: |dr| <= u ((k + store + 1) | |A| |x| | + (1 + store) |b|), store = 1 for fp32, and the same for
        numpy with u64 and store = 0.
      normal residual: A^t applied to the residual's difference, <= |A|_2 |dr|; the product with A^t, k' = the most entries of a
        column, and the subtraction of damp x: u ((k' + store + 1) | |A^t| |r| | + 2 damp |x|), and the same for numpy.
    The fp64 dots and square roots behind the norms err by a few u64 of the result, far inside 1e-10 of it."""
    u, u64, store = float(np.finfo(dtype).eps) / 2, 2.0 ** -53, int(np.dtype(dtype) == np.float32)
    x = x.astype(np.float64)
    absD = np.abs(P.D)
    ax, r = np.linalg.norm(absD @ np.abs(x)), P.b - P.D @ x
    bn, atr = np.linalg.norm(P.b), np.linalg.norm(absD.T @ np.abs(r))
    floor_r = (u * (P.k_row + store + 1) + u64 * (P.k_row + 1)) * ax + (u * (1 + store) + u64) * bn
    floor_ar = P.norm2 * floor_r + (u * (P.k_col + store + 1) + u64 * (P.k_col + 1)) * atr + 2 * (u + u64) * damp * np.linalg.norm(x)
    return floor_r, floor_ar


def raw_cgls(eng, A, At, b, x, damp, tol, max_iterations, hist):
    """the C call on the caller's own buffers: (rc, info)"""
    info = eng.LsqInfo()
    info.struct_size = ctypes.sizeof(eng.LsqInfo)
    p = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
    rc = eng.lib().spmv_mi355x_cgls(A.h, At.h, p(b), p(x), damp, tol, max_iterations, p(hist), ctypes.byref(info))
    return rc, info


def close(*handles):
    for M in handles:
        M.close()


# ---- 1. against lstsq, 2. history against the restatement --------------------------------------------------------------------------

@pytest.mark.parametrize("m,n", SHAPES, ids=[f"{m}x{n}" for m, n in SHAPES])
def test_against_lstsq(eng, m, n):
    P = problem(m, n)
    worst = {}
    for fmt, opts in LAYOUTS:
        for dtype, lim in PREC.items():
            A, At = P.handles(eng, fmt, dtype, **opts)
            assert (At.m, At.n, At.transposed) == (n, m, 1)
            for damp in DAMPS:
                what = f"{m}x{n} {A.format_name} {np.dtype(dtype).name} damp={damp}"
                got = A.cgls(At, P.b.astype(dtype), damp=damp, tol=lim["tol"], max_iterations=200)
                want = P.lstsq(damp)
                assert got["stop"] == 1, f"{what}: stop {got['stop']} after {got['iterations']} iterations"
                assert got["x"].dtype == dtype and got["x"].shape == (n,) and got["history"].shape == (got["iterations"], 2)
                err = np.linalg.norm(got["x"].astype(np.float64) - want) / np.linalg.norm(want)
                ar = got["arnorm"] / got["arnorm0"]
                rn, an, xn = explicit_norms(P, got["x"], damp)
                floor_r, floor_ar = cancellation_floor(P, got["x"], damp, dtype)
                if m > n:
                    floor_r = 0.0                                          # inconsistent: |r| is of the order of |b|, no cancellation
                dev = dict(x=err / lim["x"], arnorm=ar / (10 * lim["tol"]),
                           rnorm_np=abs(got["rnorm"] - rn) / (lim["norms"] * rn + floor_r),
                           arnorm_np=abs(got["arnorm"] - an) / (lim["norms"] * an + floor_ar),
                           xnorm_np=abs(got["xnorm"] - xn) / (lim["norms"] * xn))
                for k, v in dev.items():
                    assert v <= 1, f"{what}: {k} is {v:.3g} times its bound ({got['iterations']} iterations, rnorm {got['rnorm']!r} " \
                                   f"numpy {rn!r} floor {floor_r:.3g}, arnorm {got['arnorm']!r} numpy {an!r} floor {floor_ar:.3g})"
                    worst[k] = max(worst.get(k, 0), float(v))
            close(A, At)
    print(f"[cgls] {m}x{n}: largest shares of the bounds " + ", ".join(f"{k} {v:.2g}" for k, v in worst.items()))


@pytest.mark.parametrize("m,n", SHAPES, ids=[f"{m}x{n}" for m, n in SHAPES])
def test_history_against_the_restatement(eng, m, n):
    P = problem(m, n)
    worst = {}
    for fmt, opts in LAYOUTS:
        for dtype, lim in PREC.items():
            A, At = P.handles(eng, fmt, dtype, **opts)
            for damp in DAMPS:
                what = f"{m}x{n} {A.format_name} {np.dtype(dtype).name} damp={damp}"
                got = A.cgls(At, P.b.astype(dtype), damp=damp, tol=lim["tol"], max_iterations=200)
                _, ref, s0 = P.restatement(dtype, damp, lim["tol"])
                rows = np.nonzero(ref[:, 1] / s0 > lim["ratio"])[0]
                assert rows.size == 0 or rows[-1] == rows.size - 1                 # a leading stretch
                assert got["iterations"] >= rows.size, what
                assert abs(got["arnorm0"] - s0) <= lim["hist"] * s0, what
                if rows.size:
                    d = np.abs(got["history"][rows] - ref[rows]) / ref[rows]
                    worst[np.dtype(dtype).name] = max(worst.get(np.dtype(dtype).name, 0), float(d.max()))
                    assert d.max() <= lim["hist"], f"{what}: history deviates by {d.max():.3g} at row {np.argmax(d.max(axis=1))}"
                    assert np.all(np.diff(got["history"][rows, 0]) <= 0), f"{what}: |r| increases"
            close(A, At)
    print(f"[cgls] {m}x{n}: largest history deviation {worst}")


# ---- 3. At from the caller's own CSR, 4. deterministic ---------------------------------------------------------------------------------

def _same(a, b, what):
    assert a["iterations"] == b["iterations"] and a["stop"] == b["stop"], what
    assert a["x"].tobytes() == b["x"].tobytes(), f"{what}: x"
    assert a["history"].tobytes() == b["history"].tobytes(), f"{what}: history"
    for k in ("rnorm", "arnorm", "arnorm0", "xnorm"):
        assert a[k] == b[k], f"{what}: {k}"


@pytest.mark.parametrize("m,n", [(3000, 1100), (700, 2500)], ids=["tall", "wide"])
def test_at_from_the_callers_own_csr_gives_the_same_bits(eng, m, n):
    P = problem(m, n)
    rp, ci, va = P.csr
    t_rp, t_ci, t_va = np_transpose(rp, ci, va, m, n)
    for fmt, opts in LAYOUTS:
        A, At = P.handles(eng, fmt, np.float64, **opts)
        Own = eng.Matrix(t_rp, t_ci, t_va, n, m, fmt, np.float64, **opts)
        assert (Own.transposed, At.transposed) == (0, 1)
        for damp in DAMPS:
            a = A.cgls(At, P.b, damp=damp)
            b = A.cgls(Own, P.b, damp=damp)
            assert a["stop"] == 1
            _same(a, b, f"{m}x{n} {A.format_name} damp={damp}")
        close(A, At, Own)


def test_two_solves_return_identical_bits(eng):
    for m, n in ((3000, 1100), (700, 2500)):
        P = problem(m, n)
        for fmt, opts in LAYOUTS:
            for dtype, lim in PREC.items():
                A, At = P.handles(eng, fmt, dtype, **opts)
                a = A.cgls(At, P.b.astype(dtype), damp=0.25, tol=lim["tol"])
                b = A.cgls(At, P.b.astype(dtype), damp=0.25, tol=lim["tol"])
                assert a["stop"] == 1
                _same(a, b, f"{m}x{n} {A.format_name} {np.dtype(dtype).name}")
                close(A, At)


# ---- 5. frozen after the break ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("damp", DAMPS)
def test_frozen_after_the_break(eng, damp):
    """300 > 2 * POLL = 64: the host runs ahead of the device, waits on the progress word and stops on what was posted; whatever it
    enqueued past the break must leave x, the counter and the history as a solve that ends at the break leaves them."""
    P = problem(3000, 1100)
    b = np.ascontiguousarray(P.b)
    for fmt, opts in LAYOUTS[:2]:
        A, At = P.handles(eng, fmt, np.float64, **opts)
        x_long, h_long = np.full(P.n, 7.0), np.full((300, 2), 7.0)
        rc, long_ = raw_cgls(eng, A, At, b, x_long, damp, 1e-12, 300, h_long)
        assert rc == 0 and long_.stop == 1 and 0 < long_.iterations <= 30
        k = long_.iterations
        x_short, h_short = np.full(P.n, 7.0), np.full((k, 2), 7.0)
        rc, short = raw_cgls(eng, A, At, b, x_short, damp, 1e-12, k, h_short)
        assert rc == 0 and (short.stop, short.iterations) == (1, k)
        assert x_long.tobytes() == x_short.tobytes()
        assert h_long[:k].tobytes() == h_short.tobytes() and np.all(h_long[:k] > 0)
        assert np.all(h_long[k:] == 0)
        assert (long_.rnorm, long_.arnorm, long_.xnorm) == (short.rnorm, short.arnorm, short.xnorm)
        assert long_.spmv_calls < 3 + 2 * 300                              # the host stopped enqueueing
        close(A, At)


def test_tol_zero_runs_to_max_iterations(eng):
    """tol = 0 never stops on the tolerance. The tall system is inconsistent (|r| stays of the order of |b|), so s = A^t r - damp x
    stays a non-zero roundoff-level vector once converged and delta never vanishes: 150 iterations run, past the host's polling."""
    P = problem(3000, 1100)
    A, At = P.handles(eng, "sell_c_sigma", np.float64)
    got = A.cgls(At, P.b, damp=0.0, tol=0.0, max_iterations=150)
    assert (got["stop"], got["iterations"]) == (2, 150) and got["history"].shape == (150, 2)
    assert np.all(np.isfinite(got["x"])) and np.all(np.isfinite(got["history"]))
    assert got["spmv_calls"] == 3 + 2 * 150
    want = P.lstsq(0.0)
    assert np.linalg.norm(got["x"] - want) <= 3e-12 * np.linalg.norm(want)
    close(A, At)


# ---- 6. stops that are not convergence -----------------------------------------------------------------------------------------------

def test_stops_that_are_not_convergence(eng):
    P = problem(257, 63)
    for fmt, opts in LAYOUTS:
        A, At = P.handles(eng, fmt, np.float64, **opts)
        got = A.cgls(At, np.zeros(P.m))                                     # b = 0
        assert (got["stop"], got["iterations"]) == (3, 0) and not got["x"].any() and got["history"].shape == (0, 2)
        assert (got["rnorm"], got["arnorm"], got["arnorm0"], got["xnorm"]) == (0, 0, 0, 0)
        got = A.cgls(At, P.b, max_iterations=0)                             # no iteration allowed
        assert (got["stop"], got["iterations"]) == (2, 0) and not got["x"].any()
        assert abs(got["rnorm"] - np.linalg.norm(P.b)) <= 1e-14 * np.linalg.norm(P.b)
        assert got["arnorm"] == got["arnorm0"] and abs(got["arnorm0"] - np.linalg.norm(P.D.T @ P.b)) <= 1e-13 * got["arnorm0"]
        assert got["spmv_calls"] == 3
        close(A, At)
    # b orthogonal to the range of A: a matrix with an empty row, b non-zero only there
    D = P.D.copy()
    D[100, :] = 0
    rp, ci, va = dense_to_csr(D)
    b = np.zeros(P.m)
    b[100] = -2.5
    for fmt, opts in LAYOUTS:
        A = eng.Matrix(rp, ci, va, P.m, P.n, fmt, np.float64, **opts)
        At = eng.Matrix(rp, ci, va, P.m, P.n, fmt, np.float64, transpose=1, **opts)
        got = A.cgls(At, b)
        assert (got["stop"], got["iterations"]) == (3, 0) and not got["x"].any()
        assert got["rnorm"] == np.linalg.norm(b) == 2.5 and got["arnorm"] == 0
        close(A, At)
    # an all-zero matrix
    rp, ci, va = np.zeros(5, np.int32), np.zeros(0, np.int32), np.zeros(0)
    for fmt, opts in LAYOUTS:
        A = eng.Matrix(rp, ci, va, 4, 3, fmt, np.float64, **opts)
        At = eng.Matrix(rp, ci, va, 4, 3, fmt, np.float64, transpose=1, **opts)
        got = A.cgls(At, np.array([1.0, -2.0, 3.0, 0.5]))
        assert (got["stop"], got["iterations"]) == (3, 0) and got["x"].shape == (3,) and not got["x"].any()
        assert abs(got["rnorm"] - np.sqrt(14.25)) <= 1e-15 * 4
        close(A, At)


# ---- 7. mismatch errors that need handles ---------------------------------------------------------------------------------------------

def test_mismatched_handles_are_refused(eng):
    P = problem(257, 63)
    A, At = P.handles(eng, "csr_vector", np.float64)
    A32, At32 = P.handles(eng, "csr_vector", np.float32)
    b = np.ascontiguousarray(P.b)
    for other, phrase in ((A, b"A is 257 x 63, At is 257 x 63"), (At32, b"precision")):
        x, hist = np.full(P.n, -7.25), np.full((10, 2), 9.0)
        rc, info = raw_cgls(eng, A, other, b, x, 0.0, 1e-12, 10, hist)
        msg = eng.lib().spmv_mi355x_last_error()
        assert rc == 1 and b"cgls" in msg and phrase in msg, msg
        assert np.all(x == -7.25) and np.all(hist == 9.0) and info.iterations == 0
    with pytest.raises(eng.SpmvError, match="cgls"):
        A.cgls(A, P.b)
    with pytest.raises(ValueError, match="b must have 257 values"):
        A.cgls(At, P.b[:63])
    close(A, At, A32, At32)


# ---- 8. handle support ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("m,n", [(3000, 1100), (700, 2500)], ids=["tall", "wide"])
def test_a_value_storage_pair_solves_the_rounded_matrix(eng, m, n):
    """DESIGN §4d's contract for the other solvers: fp64 vectors over fp32-stored values give, bit for bit, the solve of fp64 handles
    built from (double) (float) values (sell_values = 2)."""
    P = problem(m, n)
    rounded = P.csr[2].astype(np.float32).astype(np.float64)
    A4, At4 = P.handles(eng, "sell_c_sigma", np.float64, **dict(DELTA, value_storage=1))
    A8, At8 = P.handles(eng, "sell_c_sigma", np.float64, values=rounded, **dict(DELTA, sell_values=2))
    assert A4.format_name.endswith("_v4") and At4.format_name.endswith("_v4") and A4.value_dtype == np.float32
    assert not A8.format_name.endswith("_v4") and A8.value_dtype == np.float64
    for damp in DAMPS:
        a = A4.cgls(At4, P.b, damp=damp)
        b = A8.cgls(At8, P.b, damp=damp)
        assert a["stop"] == 1
        _same(a, b, f"{m}x{n} damp={damp}")
        # and it is the rounded matrix that was solved: the residual of the normal equations of the ROUNDED matrix is at tol
        Dr = P.D.astype(np.float32).astype(np.float64)
        x = a["x"]
        assert np.linalg.norm(Dr.T @ (P.b - Dr @ x) - damp * x) <= 10 * 1e-12 * np.linalg.norm(Dr.T @ P.b)
    close(A4, At4, A8, At8)
