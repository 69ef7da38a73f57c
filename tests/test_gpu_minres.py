"""spmv_mi355x_minres / Matrix.minres (include/spmv_mi355x.h "MINRES"): (A - shift I) x = b for a symmetric indefinite A on one handle.

References, none of them the engine: numpy.linalg.solve on the dense matrix for the solution, numpy's explicit norms of the RETURNED
x for info.rnorm / xnorm, and a numpy restatement of the header's recurrences (vectors in the handle's precision, dots and scalars
in fp64, like the solver) for the history. Problems and references are computed once per (shape, shift, minv) and are read-only.

Test matrix kkt(n1, n2), seed 1000 n1 + n2: a saddle-point matrix [H B^t; B 0]. H has 4 on the diagonal and up to 4 symmetric
off-diagonals in (-0.5, 0.5) per row; row r of B has 2 at column r % n1 plus two entries in (-0.5, 0.5); the (2,2) block is 0: n2
zero diagonal entries (pcg and pbicgstab refuse the matrix) and n2 negative eigenvalues (CG is not defined for it).
cond(A - shift I) <= 20 for the shifts used (asserted below from the eigenvalues of A), and the restatement reaches
phibar <= 1e-12 beta1 in at most 125 iterations: past 2 * POLL = 64, so the host's run-ahead and its stop on the progress word are
exercised. Shapes: the smallest that exercise several blocks of the vector kernels (1024 rows each), one row past a block, below a
block, and 1 (the second trip of the partial sums and the cap of the grid need 262 145 and 1 049 601 unknowns:
test_gpu_solver_sizes.py).

The preconditioner under test: minv_i = (1 / |d_ii|, or 1 where d_ii = 0) * (1 + 0.5 sin(i)), within [0.125, 1.5].

Bounds:
  * stop 1 guarantees phibar <= tol beta1 in the M^-1 norm, r.(minv r) <= tol^2 b.(minv b); with min minv |r|^2 <= r.(minv r) and
    b.(minv b) <= max minv |b|^2 that is |r| <= tol sqrt(max minv / min minv) |b| in the 2-norm (factor 1 without minv), and the
    explicit residual may exceed the recursive one by the project's factor 10 (the CGLS tests'):
    info.rnorm <= 10 tol sqrt(max minv / min minv) |b|.
  * |x - x*| / |x*| <= kappa * that bound / |b|, kappa taken as 20.
  * rnorm, xnorm against numpy's explicit values of the returned x: 1e-10 (fp64) / 1e-4 (fp32) relative, rnorm plus the cancellation
    floor of cancellation_floor() (the residual at convergence is a difference of terms far larger than itself).
  * rnorm0 = |b| and prnorm0 = sqrt(b . minv b) against numpy: the dots are fp64 sums of products of values of the handle's
    precision, the product minv_i b_i is rounded once to that precision: 1e-13 (fp64) / 1e-6 (fp32) relative.
  * history against the restatement: rows with phibar_k / beta1 above 1e-8 (fp64) / 1e-2 (fp32) to rtol 1e-6 / 1e-3 (the CGLS
    tests' bounds: roundoff eps * kappa * k divided by the ratio); two summation orders of the restatement itself differ by at most
    1.4e-12 / 6.1e-7 on those rows."""
import ctypes
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SHAPES = [(2000, 1000), (700, 325), (1025, 0), (40, 23), (3, 2), (1, 0)]
LAYOUTS = [("sell_c_sigma", {}), ("sell_c_sigma", {"sell_window": 2}), ("csr_vector", {})]
DELTA = dict(sell_c=64, sell_delta=1, sell_sigma=64, sell_window=2)
CASES = ((0.0, False), (0.3, False), (0.0, True), (-0.2, True))               # (shift, minv given)
KAPPA = 20.0
PREC = {np.float64: dict(tol=1e-12, norms=1e-10, norms0=1e-13, ratio=1e-8, hist=1e-6),
        np.float32: dict(tol=1e-5, norms=1e-4, norms0=1e-6, ratio=1e-2, hist=1e-3)}
INFO_FIELDS = ("iterations", "stop", "rnorm", "rnorm0", "prnorm", "prnorm0", "xnorm")


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


def kkt(n1, n2):
    rng = np.random.default_rng(1000 * n1 + n2)
    n = n1 + n2
    D = np.zeros((n, n))
    for i in range(n1):
        D[i, i] = 4.0
        for j in rng.choice(n1, min(2, n1), replace=False):
            if j != i:
                v = rng.uniform(-0.5, 0.5)
                D[i, j] = v
                D[j, i] = v
    for r in range(n2):
        D[n1 + r, r % n1] += 2.0
        for j in rng.choice(n1, min(2, n1), replace=False):
            D[n1 + r, j] += rng.uniform(-0.5, 0.5)
    D[:n1, n1:] = D[n1:, :n1].T
    return D


def restate(A, b, shift, minv, tol, max_iterations, dtype, dot=None):
    """the header's recurrences in numpy: vectors in `dtype`, dots and scalars in fp64. A is a matrix of `dtype`, dense or
    scipy.sparse (only A @ v is taken). `dot` replaces the fp64 dot product (test_solver_size_cases.py: a dot that loses rows).
    Returns (x, history, beta1, stop)."""
    dt = np.dtype(dtype).type
    n = len(b)
    b = b.astype(dt)
    dot = dot or (lambda u, v: float(u.astype(np.float64) @ v.astype(np.float64)))
    M = (lambda v: v) if minv is None else (lambda v, d=minv.astype(dt): d * v)
    x, r1, y = np.zeros(n, dt), b, M(b)
    beta1 = dot(b, y)
    if beta1 == 0:
        return x, np.zeros(0), 0.0, 3
    beta1 = np.sqrt(beta1)
    oldb, beta, dbar, epsln, phibar, cs, sn = 0.0, beta1, 0.0, 0.0, beta1, -1.0, 0.0
    w, w2, r2, hist, stop = np.zeros(n, dt), np.zeros(n, dt), r1, [], 2
    for itn in range(1, max_iterations + 1):
        v = dt(1 / beta) * y
        y = A @ v - dt(shift) * v
        if itn >= 2:
            y = y - dt(beta / oldb) * r1
        alfa = dot(v, y)
        y = y - dt(alfa / beta) * r2
        r1, r2 = r2, y
        y = M(r2)
        oldb, beta = beta, dot(r2, y)
        if not (beta >= 0 and np.isfinite(beta) and np.isfinite(alfa)):
            stop = 4
            break
        beta = np.sqrt(beta)
        oldeps, delta, gbar = epsln, cs * dbar + sn * alfa, sn * dbar - cs * alfa
        epsln, dbar = sn * beta, -cs * beta
        gamma = max(np.hypot(gbar, beta), np.finfo(np.float64).eps)
        cs, sn = gbar / gamma, beta / gamma
        phi, phibar = cs * phibar, sn * phibar
        w1, w2 = w2, w
        w = (v - dt(oldeps) * w1 - dt(delta) * w2) * dt(1 / gamma)
        x = x + dt(phi) * w
        hist.append(phibar)
        if tol > 0 and phibar <= tol * beta1:
            stop = 1
            break
        if beta == 0:
            stop = 5
            break
    return x, np.array(hist), beta1, stop


class Problem:
    def __init__(self, n1, n2):
        D = kkt(n1, n2)
        n = n1 + n2
        assert np.array_equal(D, D.T) and not D[n1:, n1:].any()
        self.n1, self.n2, self.n, self.D = n1, n2, n, D
        self.csr = dense_to_csr(D)
        self.eig = np.linalg.eigvalsh(D)
        assert int((self.eig < 0).sum()) == n2
        self.k_row = int((D != 0).sum(axis=1).max())
        self.b = np.random.default_rng(7).uniform(-1, 1, n)
        d = np.diag(D)
        self.minv = 1.0 / np.where(d != 0, np.abs(d), 1.0) * (1 + 0.5 * np.sin(np.arange(n)))
        assert 0.125 <= self.minv.min() and self.minv.max() <= 1.5
        for v in (D, self.b, self.minv) + self.csr:
            v.setflags(write=False)

    def handle(self, eng, fmt, dtype, values=None, **opts):
        rp, ci, va = self.csr
        return eng.Matrix(rp, ci, va if values is None else values, self.n, self.n, fmt, dtype, **opts)

    def pre(self, given):
        return self.minv if given else None

    def norm_factor(self, given):
        """sqrt(max minv / min minv): the M^-1-norm stop rule in the 2-norm"""
        return float(np.sqrt(self.minv.max() / self.minv.min())) if given else 1.0

    @functools.lru_cache(maxsize=None)
    def solve(self, shift):
        ev = self.eig - shift                                               # the eigenvalues of A - shift I
        assert np.abs(ev).max() / np.abs(ev).min() <= KAPPA, (self.n1, self.n2, shift)
        x = np.linalg.solve(self.D - shift * np.eye(self.n), self.b)
        x.setflags(write=False)
        return x

    @functools.lru_cache(maxsize=None)
    def restatement(self, dtype, shift, given, tol, max_iterations=300):
        x, hist, beta1, stop = restate(self.D.astype(dtype), self.b, shift, self.pre(given), tol, max_iterations, dtype)
        hist.setflags(write=False)
        return x, hist, beta1, stop


@functools.lru_cache(maxsize=None)
def problem(n1, n2):
    return Problem(n1, n2)


def explicit_norms(P, x, shift):
    """numpy's explicit values for a returned x, in fp64 whatever the precision of x"""
    x = x.astype(np.float64)
    return np.linalg.norm(P.b - (P.D @ x - shift * x)), np.linalg.norm(x)


def cancellation_floor(P, x, shift, dtype):
    """How far two correct evaluations of |b - (A - shift I) x| for the same x can lie apart, to first order in the unit roundoffs u
    (the handle's precision) and u64 (numpy's): by the reverse triangle inequality the norms differ by at most the norm of the
    difference of the vectors. Component i: a sum of k products in any order, fused or not, errs by <= k u (|A| |x|)_i, k the most
    entries of a row plus one for the shift term; the subtraction from b_i adds u (|b_i| + (|A| |x|)_i); an fp32 handle holds A, b
    and the shift rounded to fp32, one more u on each of the two terms. The same for numpy with u64 and nothing rounded on storage."""
    u, u64, store = float(np.finfo(dtype).eps) / 2, 2.0 ** -53, int(np.dtype(dtype) == np.float32)
    x = np.abs(x.astype(np.float64))
    k = P.k_row + (shift != 0)
    ax, bn = np.linalg.norm(np.abs(P.D) @ x + abs(shift) * x), np.linalg.norm(P.b)
    return (u * (k + store + 1) + u64 * (k + 1)) * ax + (u * (1 + store) + u64) * bn


def raw_minres(eng, A, b, x, shift, minv, tol, max_iterations, hist):
    """the C call on the caller's own buffers: (rc, info)"""
    info = eng.MinresInfo()
    info.struct_size = ctypes.sizeof(eng.MinresInfo)
    p = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
    rc = eng.lib().spmv_mi355x_minres(A.h, p(b), p(x), shift, p(minv), tol, max_iterations, p(hist), ctypes.byref(info))
    return rc, info


def shares_of_the_bounds(P, got, shift, given, dtype):
    """item 1's figures for one solve, each as a share of its bound (<= 1 passes)"""
    lim = PREC[dtype]
    bn = np.linalg.norm(P.b)
    res_bound = 10 * lim["tol"] * P.norm_factor(given) * bn
    want = P.solve(shift)
    rn, xn = explicit_norms(P, got["x"], shift)
    floor_r = cancellation_floor(P, got["x"], shift, dtype)
    bt = P.b.astype(dtype).astype(np.float64)
    mt = np.ones(P.n) if not given else P.minv.astype(dtype)
    beta1 = np.sqrt(float(bt @ (mt * bt.astype(dtype)).astype(np.float64)))
    return dict(rnorm=got["rnorm"] / res_bound,
                x=np.linalg.norm(got["x"].astype(np.float64) - want) / np.linalg.norm(want) / (KAPPA * res_bound / bn),
                rnorm_np=abs(got["rnorm"] - rn) / (lim["norms"] * rn + floor_r),
                xnorm_np=abs(got["xnorm"] - xn) / (lim["norms"] * xn),
                rnorm0_np=abs(got["rnorm0"] - np.linalg.norm(bt)) / (lim["norms0"] * np.linalg.norm(bt)),
                prnorm0_np=abs(got["prnorm0"] - beta1) / (lim["norms0"] * beta1))


# ---- 1. against the dense solve, 2. history against the restatement ----------------------------------------------------------------

@pytest.mark.parametrize("n1,n2", SHAPES, ids=[f"{a}+{b}" for a, b in SHAPES])
def test_against_the_dense_solve(eng, n1, n2):
    P = problem(n1, n2)
    worst = {}
    for fmt, opts in LAYOUTS:
        for dtype, lim in PREC.items():
            A = P.handle(eng, fmt, dtype, **opts)
            for shift, given in CASES:
                what = f"kkt({n1},{n2}) {A.format_name} {np.dtype(dtype).name} shift={shift} minv={given}"
                got = A.minres(P.b.astype(dtype), shift=shift, minv=P.pre(given), tol=lim["tol"], max_iterations=300)
                assert got["stop"] == 1, f"{what}: stop {got['stop']} after {got['iterations']} iterations"
                assert got["x"].dtype == dtype and got["x"].shape == (P.n,) and got["history"].shape == (got["iterations"],)
                assert got["prnorm"] == got["history"][-1] and got["prnorm"] <= lim["tol"] * got["prnorm0"], what
                assert got["spmv_calls"] >= got["iterations"] + 1, what
                for k, v in shares_of_the_bounds(P, got, shift, given, dtype).items():
                    assert v <= 1, f"{what}: {k} is {v:.3g} times its bound ({got['iterations']} iterations, rnorm {got['rnorm']!r}, " \
                                   f"rnorm0 {got['rnorm0']!r}, prnorm0 {got['prnorm0']!r}, xnorm {got['xnorm']!r})"
                    worst[k] = max(worst.get(k, 0), float(v))
            A.close()
    print(f"[minres] kkt({n1},{n2}): largest shares of the bounds " + ", ".join(f"{k} {v:.2g}" for k, v in worst.items()))


@pytest.mark.parametrize("n1,n2", SHAPES, ids=[f"{a}+{b}" for a, b in SHAPES])
def test_history_against_the_restatement(eng, n1, n2):
    P = problem(n1, n2)
    worst = {}
    for fmt, opts in LAYOUTS:
        for dtype, lim in PREC.items():
            A = P.handle(eng, fmt, dtype, **opts)
            for shift, given in CASES:
                what = f"kkt({n1},{n2}) {A.format_name} {np.dtype(dtype).name} shift={shift} minv={given}"
                got = A.minres(P.b.astype(dtype), shift=shift, minv=P.pre(given), tol=lim["tol"], max_iterations=300)
                _, ref, beta1, _ = P.restatement(dtype, shift, given, lim["tol"])
                rows = np.nonzero(ref / beta1 > lim["ratio"])[0]
                assert rows.size == 0 or rows[-1] == rows.size - 1                 # a leading stretch: phibar never increases
                assert got["iterations"] >= rows.size, what
                assert abs(got["prnorm0"] - beta1) <= lim["hist"] * beta1, what
                if rows.size:
                    d = np.abs(got["history"][rows] - ref[rows]) / ref[rows]
                    worst[np.dtype(dtype).name] = max(worst.get(np.dtype(dtype).name, 0), float(d.max()))
                    assert d.max() <= lim["hist"], f"{what}: history deviates by {d.max():.3g} at row {np.argmax(d)}"
                    assert np.all(np.diff(got["history"][rows]) <= 0), f"{what}: phibar increases"
            A.close()
    print(f"[minres] kkt({n1},{n2}): largest history deviation {worst}")


# ---- 3. the gap this closes ------------------------------------------------------------------------------------------------------------

def test_the_saddle_point_matrix_pcg_and_pbicgstab_refuse(eng):
    P = problem(700, 325)
    rp, ci, va = P.csr
    for fmt, opts in LAYOUTS:
        A = P.handle(eng, fmt, np.float64, **opts)
        with pytest.raises(eng.SpmvError, match="zero in diagonal"):
            A.pcg(rp, ci, va, P.b, 100)
        with pytest.raises(eng.SpmvError, match="zero in diagonal"):
            A.pbicgstab(rp, ci, va, P.b, 100)
        got = A.minres(P.b, max_iterations=300)
        assert got["stop"] == 1 and 0 < got["iterations"] < 300
        assert got["rnorm"] <= 10 * 1e-12 * got["rnorm0"]
        A.close()


# ---- 4. deterministic -----------------------------------------------------------------------------------------------------------------------

def _same(a, b, what):
    for k in INFO_FIELDS:
        assert a[k] == b[k], f"{what}: {k}"
    assert a["x"].tobytes() == b["x"].tobytes(), f"{what}: x"
    assert a["history"].tobytes() == b["history"].tobytes(), f"{what}: history"


def test_two_solves_return_identical_bits(eng):
    for n1, n2 in ((2000, 1000), (700, 325)):
        P = problem(n1, n2)
        for fmt, opts in LAYOUTS:
            for dtype, lim in PREC.items():
                A = P.handle(eng, fmt, dtype, **opts)
                for shift, given in ((0.0, False), (-0.2, True)):
                    a = A.minres(P.b.astype(dtype), shift=shift, minv=P.pre(given), tol=lim["tol"], max_iterations=300)
                    b = A.minres(P.b.astype(dtype), shift=shift, minv=P.pre(given), tol=lim["tol"], max_iterations=300)
                    assert a["stop"] == 1
                    _same(a, b, f"kkt({n1},{n2}) {A.format_name} {np.dtype(dtype).name} shift={shift} minv={given}")
                A.close()


# ---- 5. frozen after the break ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shift", (0.0, -0.2))
def test_frozen_after_the_break(eng, shift):
    """The break falls past 2 * POLL = 64 and 300 iterations are allowed: the host runs ahead of the device, waits on the progress
    word and stops on what was posted; whatever it enqueued past the break must leave x, the counter and the history as a solve that
    ends at the break leaves them."""
    P = problem(2000, 1000)
    b, minv = np.ascontiguousarray(P.b), np.ascontiguousarray(P.minv)
    for fmt, opts in LAYOUTS[:2]:
        A = P.handle(eng, fmt, np.float64, **opts)
        x_long, h_long = np.full(P.n, 7.0), np.full(300, 7.0)
        rc, long_ = raw_minres(eng, A, b, x_long, shift, minv, 1e-12, 300, h_long)
        assert rc == 0 and long_.stop == 1 and 64 < long_.iterations < 300 - 64
        k = long_.iterations
        x_short, h_short = np.full(P.n, 7.0), np.full(k, 7.0)
        rc, short = raw_minres(eng, A, b, x_short, shift, minv, 1e-12, k, h_short)
        assert rc == 0 and (short.stop, short.iterations) == (1, k)
        assert x_long.tobytes() == x_short.tobytes()
        assert h_long[:k].tobytes() == h_short.tobytes() and np.all(h_long[:k] > 0)
        assert np.all(h_long[k:] == 0)
        assert (long_.rnorm, long_.rnorm0, long_.prnorm, long_.prnorm0, long_.xnorm) == \
               (short.rnorm, short.rnorm0, short.prnorm, short.prnorm0, short.xnorm)
        assert short.spmv_calls == 1 + k and k + 1 <= long_.spmv_calls < 1 + 300        # the host stopped enqueueing
        A.close()


# ---- 6. tol = 0 -----------------------------------------------------------------------------------------------------------------------------

def test_tol_zero_runs_to_max_iterations(eng):
    """tol = 0 never stops on the tolerance: 150 iterations run, past the host's polling, unless the restatement says the Lanczos
    process ends exactly (beta == 0) before that."""
    P = problem(1025, 0)
    _, ref, _, ref_stop = P.restatement(np.float64, 0.0, False, 0.0, 150)
    assert ref_stop in (2, 5)
    want_stop, want_its = ref_stop, len(ref)
    for fmt, opts in LAYOUTS:
        A = P.handle(eng, fmt, np.float64, **opts)
        got = A.minres(P.b, tol=0.0, max_iterations=150)
        assert (got["stop"], got["iterations"]) == (want_stop, want_its) and got["history"].shape == (want_its,)
        assert np.all(np.isfinite(got["x"])) and np.all(np.isfinite(got["history"]))
        assert all(np.isfinite(got[k]) for k in INFO_FIELDS)
        if want_stop == 2:
            assert got["spmv_calls"] == 150 + 1
        for k, v in shares_of_the_bounds(P, got, 0.0, False, np.float64).items():
            assert v <= 1, f"{A.format_name}: {k} is {v:.3g} times its bound"
        A.close()


# ---- 7. the other stops -----------------------------------------------------------------------------------------------------------------

def test_the_other_stops(eng):
    P = problem(40, 23)
    for fmt, opts in LAYOUTS:
        for given in (False, True):
            A = P.handle(eng, fmt, np.float64, **opts)
            got = A.minres(np.zeros(P.n), minv=P.pre(given))                   # b = 0
            assert (got["stop"], got["iterations"]) == (3, 0) and not got["x"].any() and got["history"].shape == (0,)
            assert (got["rnorm"], got["rnorm0"], got["prnorm"], got["prnorm0"], got["xnorm"]) == (0, 0, 0, 0, 0)
            got = A.minres(P.b, minv=P.pre(given), max_iterations=0)           # no iteration allowed
            assert (got["stop"], got["iterations"]) == (2, 0) and not got["x"].any()
            assert got["rnorm"] == got["rnorm0"] and abs(got["rnorm0"] - np.linalg.norm(P.b)) <= 1e-14 * np.linalg.norm(P.b)
            assert got["prnorm"] == got["prnorm0"] > 0 and got["xnorm"] == 0
            assert got["spmv_calls"] == 1
            A.close()


@pytest.mark.parametrize("dtype", (np.float64, np.float32), ids=("f64", "f32"))
def test_an_exact_lanczos_step_ends_the_process(eng, dtype):
    """A diagonal matrix and b = 2 e_100: v = e_100, alfa = d_100 and y - (alfa / 2) * 2 e_100 = 0 are exact in floating point, so
    beta_2 == 0 after one iteration: stop 5 with tol = 0, stop 1 (phibar = 0) with a tolerance, and x = 2 / d_100 e_100."""
    n = 1025
    d = (1 + np.arange(n) / 1024.0) * np.where(np.arange(n) % 3 == 1, -1.0, 1.0)      # distinct, both signs, exact in fp32
    assert len(set(d)) == n and d[100] < 0 and np.array_equal(d.astype(np.float32).astype(np.float64), d)
    rp, ci = np.arange(n + 1, dtype=np.int32), np.arange(n, dtype=np.int32)
    b = np.zeros(n)
    b[100] = 2.0
    want = b / d
    eps = float(np.finfo(dtype).eps)
    for fmt, opts in LAYOUTS:
        A = eng.Matrix(rp, ci, d, n, n, fmt, dtype, **opts)
        for tol, stop in ((0.0, 5), (1e-12, 1)):
            got = A.minres(b.astype(dtype), tol=tol, max_iterations=50)
            assert (got["stop"], got["iterations"]) == (stop, 1), f"{A.format_name} tol={tol}: {got['stop']}, {got['iterations']}"
            assert np.linalg.norm(got["x"].astype(np.float64) - want) <= 4 * eps * np.linalg.norm(want)
            assert got["prnorm"] == 0 and got["history"].tolist() == [0.0] and got["prnorm0"] == 2
        A.close()


def test_a_nan_in_the_matrix_is_a_breakdown(eng):
    P = problem(40, 23)
    rp, ci, va = P.csr
    va = va.copy()
    va[5] = np.nan
    for fmt, opts in LAYOUTS:
        for given in (False, True):
            A = eng.Matrix(rp, ci, va, P.n, P.n, fmt, np.float64, **opts)
            got = A.minres(P.b, minv=P.pre(given), max_iterations=50)
            assert (got["stop"], got["iterations"]) == (4, 0), f"{A.format_name}: {got['stop']}, {got['iterations']}"
            assert not got["x"].any() and got["history"].shape == (0,)
            A.close()


# ---- 8. refusals that need a handle ---------------------------------------------------------------------------------------------------

def _refused(eng, A, n_b, minv, phrases):
    b, x, hist = np.full(n_b, 3.5), np.full(n_b, -7.25), np.full(10, 9.0)
    keep = None if minv is None else minv.copy()
    info = eng.MinresInfo()
    info.struct_size = ctypes.sizeof(eng.MinresInfo)
    info.iterations, info.stop, info.rnorm, info.spmv_calls = -5, -6, -7.5, -8
    before = bytes(info)
    p = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
    rc = eng.lib().spmv_mi355x_minres(A.h, p(b), p(x), 0.0, p(minv), 1e-12, 10, p(hist), ctypes.byref(info))
    msg = eng.lib().spmv_mi355x_last_error()
    assert rc == 1 and b"minres" in msg and all(ph in msg for ph in phrases), msg
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
    with pytest.raises(eng.SpmvError, match="minres.*257 x 63"):
        A.minres(np.ones(257))
    with pytest.raises(ValueError, match="b must have 257 values"):
        A.minres(np.ones(63))
    A.close()

    P = problem(700, 325)
    rp, ci, va = P.csr
    for fmt, opts in LAYOUTS:
        B = eng.Matrix(rp, ci, va, P.n, P.n, fmt, np.float64, row_begin=100, row_end=400, **opts)      # rows 100..399 of A
        assert (B.m, B.n) == (300, P.n)
        _refused(eng, B, P.n, None, (b"300 x 1025",))
        B.close()
    for dtype in (np.float64, np.float32):
        A = P.handle(eng, "sell_c_sigma", dtype)
        for at, value in ((0, 0.0), (511, -0.5), (1024, np.nan), (700, np.inf)):
            minv = P.minv.astype(dtype)
            minv[at] = value
            _refused(eng, A, P.n, minv, (f"minv[{at}]".encode(),))
        minv = P.minv.astype(dtype)
        minv[[3, 9]] = -1.0, np.nan
        _refused(eng, A, P.n, minv, (b"minv[3]",))                            # the first such index
        with pytest.raises(ValueError, match="b must have 1025 values"):
            A.minres(P.b[:700])
        with pytest.raises(ValueError, match="minv must have 1025 values"):
            A.minres(P.b, minv=P.minv[:700])
        with pytest.raises(eng.SpmvError, match=r"minres: minv\[3\]"):
            A.minres(P.b, minv=minv)
        A.close()


# ---- 9. handle support ------------------------------------------------------------------------------------------------------------------

def test_a_value_storage_handle_solves_the_rounded_matrix(eng):
    """DESIGN §4d's contract for the other solvers: fp64 vectors over fp32-stored values give, bit for bit, the solve of the fp64
    handle built from (double) (float) values (sell_values = 2)."""
    P = problem(700, 325)
    rounded = P.csr[2].astype(np.float32).astype(np.float64)
    A4 = P.handle(eng, "sell_c_sigma", np.float64, **dict(DELTA, value_storage=1))
    A8 = P.handle(eng, "sell_c_sigma", np.float64, values=rounded, **dict(DELTA, sell_values=2))
    assert A4.format_name.endswith("_v4") and A4.value_dtype == np.float32
    assert not A8.format_name.endswith("_v4") and A8.value_dtype == np.float64
    Dr = P.D.astype(np.float32).astype(np.float64)
    for shift, given in CASES:
        a = A4.minres(P.b, shift=shift, minv=P.pre(given), max_iterations=300)
        b = A8.minres(P.b, shift=shift, minv=P.pre(given), max_iterations=300)
        assert a["stop"] == 1
        _same(a, b, f"shift={shift} minv={given}")
        # and it is the rounded matrix that was solved
        x = a["x"]
        assert np.linalg.norm(P.b - (Dr @ x - shift * x)) <= 10 * 1e-12 * P.norm_factor(given) * np.linalg.norm(P.b)
    A4.close()
    A8.close()


def test_a_symmetric_input_handle_of_the_lower_triangle(eng):
    """symmetric_input = 1: the handle is given one triangle and multiplies by the whole matrix. The LDS-window form accumulates with
    atomics, so the bounds of the dense-solve test are held, not identical bits."""
    P = problem(700, 325)
    rp, ci, va = dense_to_csr(np.tril(P.D))
    seen = set()
    for fmt, opts in (("csr_vector", {}), ("sell_c_sigma", {}), ("sell_c_sigma", {"sell_window": 1})):
        for dtype, lim in PREC.items():
            A = eng.Matrix(rp, ci, va, P.n, P.n, fmt, dtype, symmetric_input=1, **opts)
            assert (A.m, A.n) == (P.n, P.n)
            seen.add(A.format_name)
            for shift, given in CASES:
                what = f"{A.format_name} {np.dtype(dtype).name} shift={shift} minv={given}"
                got = A.minres(P.b.astype(dtype), shift=shift, minv=P.pre(given), tol=lim["tol"], max_iterations=300)
                assert got["stop"] == 1, f"{what}: stop {got['stop']} after {got['iterations']} iterations"
                for k, v in shares_of_the_bounds(P, got, shift, given, dtype).items():
                    assert v <= 1, f"{what}: {k} is {v:.3g} times its bound"
            A.close()
    print(f"[minres] symmetric_input handles: {sorted(seen)}")
