"""spmv_mi355x_pcg_tri / Matrix.pcg_tri (include/spmv_mi355x.h "CG preconditioned by triangular solves") on the GPU.

The problem is spd_grid(45) of pcg_tri_cases.py, n = 2025: symmetric to the bit, cond_2 = 92.1 (asserted <= KAPPA = 100 from the
eigenvalues), columns ascending, b = default_rng(7).uniform(-1, 1, n). fp64 runs with tol 1e-12, fp32 with tol 1e-5, max_iterations
400. Layouts: sell_c_sigma, csr_vector and the delta layout of test_gpu_gmres_tri.py; one case with value_storage = 1.

Preconditioners: none, Jacobi as (None, 1 / diag, None), the blocked SGS of A at B in {64, 100, 256}, the global SGS, a global handle
mixed with a blocked one of B >= n, and the IC(0) factors of pcg_tri_cases.ic0 with global handles.

References, none of them the engine: numpy.linalg.solve on the dense matrix for the solution, numpy's explicit norms of the RETURNED
x, and the numpy restatement of the header's recurrences (pcg_tri_cases.restate, "M^-1 v" the C reference of tests/trsv_reference.c on
the filtered CSR). The bounds are the family's (test_gpu_gmres.py):
  * info.rnorm <= 10 tol |b|;  |x - x*| / |x*| <= KAPPA 10 tol. (On the CPU the restatement uses under 10 % of the first and under
    3 % of the second: asserted in test_pcg_tri_abi.py.)
  * rnorm, xnorm against numpy's explicit values of the returned x: 1e-10 (fp64) / 1e-4 (fp32) relative, rnorm plus the cancellation
    floor; rnorm0 = |b| to 1e-13 / 1e-6.
  * iterations within 1 of the restatement's, stop == 1.
  * history against the restatement, PRECONDITIONED cases only, to rtol 1e-6 / 1e-3 on the rows with |r| / |b| above 1e-8 / 1e-2; at
    least 60 % / 30 % of the rows qualify (the restatement alone gives 65-69 % / 33-36 %). On the CPU two restatements that differ
    only in the summation order of the dots and of the SpMV rows agree on those rows to 1.3e-14 / 2e-7.
  * the un-preconditioned runs are NOT compared row by row: the same experiment gives 1.7e-5 in fp64, CG's own sensitivity over 122
    steps. For them: counts, norms and a strictly decreasing history.
The restatement's fp64 counts are 122 / 109 / 69 / 58 / 50 / 40 / 34 (none, Jacobi, B = 64, 100, 256, global SGS, IC(0)), recomputed
here and never hard-coded in an assertion. The un-preconditioned, Jacobi and B = 64 cases pass 2 * POLL = 64: the host's run-ahead
and its stop on the progress word are exercised. That every blocked count lies below the Jacobi count is asserted as a property of
the input."""
import ctypes

import numpy as np
import pytest

import pcg_tri_cases as pc
from pcg_tri_cases import BLOCKS, MAX_ITERATIONS, MIXED_B, POLL, PREC

pytestmark = pytest.mark.gpu

DELTA = dict(sell_c=64, sell_delta=1, sell_sigma=64, sell_window=2)
LAYOUTS = [("sell_c_sigma", {}), ("csr_vector", {}), ("sell_c_sigma", DELTA)]
INFO_FIELDS = ("iterations", "stop", "rnorm", "rnorm0", "prnorm", "xnorm")
KINDS = pc.KINDS + ("mixed",)


@pytest.fixture(scope="module")
def eng():
    import spmv_mi355x as eng
    assert eng.device_count() >= 1, "no GPU visible: the -m gpu tests need an MI355X"
    return eng


def handle(eng, P, fmt, dtype, values=None, **opts):
    rp, ci, va = P.csr
    return eng.Matrix(rp, ci, va if values is None else values, P.n, P.n, fmt, dtype, **opts)


def precond(eng, P, kind, dtype):
    """the (first, scale, second) of a kind of KINDS on the GPU, None for "none" """
    rp, ci, va = P.csr
    T = eng.TriangularSolve
    if kind == "none":
        return None
    if kind == "jacobi":
        return None, (1.0 / P.diag).astype(dtype), None
    if kind == "ic0":
        _, lo, up = P.ic0()
        return T(*lo, P.n, uplo="lower", dtype=dtype), None, T(*up, P.n, uplo="upper", dtype=dtype)
    B = {"sgs": None, "mixed": None}.get(kind, kind)
    B_upper = MIXED_B if kind == "mixed" else B
    return (T(rp, ci, va, P.n, uplo="lower", dtype=dtype, block_rows=B), P.diag.astype(dtype),
            T(rp, ci, va, P.n, uplo="upper", dtype=dtype, block_rows=B_upper))


def close(M):
    for h in M or ():
        if h is not None and not isinstance(h, np.ndarray):
            h.close()


def _same(a, b, what):
    for k in INFO_FIELDS:
        assert a[k] == b[k], f"{what}: {k}: {a[k]!r} and {b[k]!r}"
    assert np.array_equal(a["x"], b["x"]), f"{what}: x"
    assert np.array_equal(a["history"], b["history"]), f"{what}: history"


def raw(eng, A, b, x, M, tol, max_iterations, hist, struct_size=None, info=None):
    """the C call on the caller's own buffers: (rc, info). M = None passes a NULL preconditioner."""
    if info is None:
        info = eng.PcgTriInfo()
        info.struct_size = ctypes.sizeof(eng.PcgTriInfo)
    p = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
    S = None
    if M is not None:
        first, scale, second = M
        S = eng.TriPrecond(ctypes.sizeof(eng.TriPrecond) if struct_size is None else struct_size, None if first is None else first.h,
                           p(scale), None if second is None else second.h)
    rc = eng.lib().spmv_mi355x_pcg_tri(A.h, p(b), p(x), None if S is None else ctypes.byref(S), tol, max_iterations, p(hist),
                                       ctypes.byref(info))
    return rc, info


# ---- 1. the dense solve, the explicit norms and the restatement --------------------------------------------------------------------

@pytest.mark.parametrize("kind", KINDS, ids=[str(k) for k in KINDS])
def test_against_the_dense_solve_and_the_restatement(eng, kind):
    P = pc.problem()
    want = P.solve()
    worst, counts = {}, {}
    for dtype, lim in PREC.items():
        name = np.dtype(dtype).name
        _, ref, ref_stop = P.restatement(dtype, kind, lim["tol"])
        assert ref_stop == 1
        _, jac, _ = P.restatement(dtype, "jacobi", lim["tol"])
        if kind in BLOCKS:
            # a property of the input: the blocked SGS needs fewer steps than the Jacobi preconditioner
            assert ref.size < jac.size, (name, kind, ref.size, jac.size)
        if dtype == np.float64 and kind in ("none", "jacobi", 64):
            assert ref.size > 2 * POLL, (kind, ref.size)                    # the run-ahead is exercised
        bn = np.linalg.norm(P.b.astype(dtype).astype(np.float64))
        rows = np.nonzero(ref / bn > lim["ratio"])[0]
        assert rows[-1] == rows.size - 1                                   # a leading stretch
        assert rows.size >= lim["share"] * ref.size, f"{name}: {rows.size} of {ref.size} rows qualify"
        M = precond(eng, P, kind, dtype)
        for fmt, opts in LAYOUTS:
            A = handle(eng, P, fmt, dtype, **opts)
            what = f"spd_grid(45) {A.format_name} {name} precond={kind}"
            got = A.pcg_tri(P.b.astype(dtype), precond=M, tol=lim["tol"], max_iterations=MAX_ITERATIONS)
            A.close()
            k = got["iterations"]
            print(f"[pcg_tri] {what}: {k} iterations (the restatement {ref.size}, Jacobi {jac.size}), rnorm {got['rnorm']:.3g}")
            assert got["stop"] == 1, f"{what}: stop {got['stop']} after {k} iterations"
            assert got["x"].dtype == dtype and got["x"].shape == (P.n,) and got["history"].shape == (k,)
            assert got["prnorm"] == got["history"][-1] and got["prnorm"] <= lim["tol"] * got["rnorm0"] * (1 + 1e-12), what
            assert k + 1 <= got["spmv_calls"] <= k + 1 + 2 * POLL, what
            for key, v in pc.shares_of_the_bounds(P, got, dtype, want).items():
                print(f"[pcg_tri] {what}: {key} is {v:.3g} of its bound")
                assert v <= 1, f"{what}: {key} is {v:.3g} times its bound"
                worst[key] = max(worst.get(key, 0), float(v))
            counts[(name, A.format_name)] = (k, ref.size)
            assert abs(k - ref.size) <= 1, f"{what}: {k} iterations, the restatement {ref.size}"
            if kind == "none":
                assert np.all(np.diff(got["history"]) < 0), f"{what}: the history is not strictly decreasing"
                continue
            assert k >= rows.size, what
            d = np.abs(got["history"][rows] - ref[rows]) / ref[rows]
            print(f"[pcg_tri] {what}: largest history deviation {d.max():.3g} on {rows.size} rows")
            assert d.max() <= lim["hist"], f"{what}: history deviates by {d.max():.3g} at row {np.argmax(d)}"
        close(M)
    print(f"[pcg_tri] precond={kind}: largest shares {worst}; (iterations, the restatement's) {counts}")


# ---- 2. pinned to the bit ---------------------------------------------------------------------------------------------------------------

def test_two_solves_return_identical_bits(eng):
    P = pc.problem()
    for dtype, lim in PREC.items():
        for kind in ("none", 100):
            M = precond(eng, P, kind, dtype)
            for fmt, opts in LAYOUTS:
                A = handle(eng, P, fmt, dtype, **opts)
                a = A.pcg_tri(P.b.astype(dtype), precond=M, tol=lim["tol"], max_iterations=MAX_ITERATIONS)
                b = A.pcg_tri(P.b.astype(dtype), precond=M, tol=lim["tol"], max_iterations=MAX_ITERATIONS)
                assert a["stop"] == 1
                _same(a, b, f"{A.format_name} {np.dtype(dtype).name} precond={kind}")
                A.close()
            close(M)


def test_a_scale_of_ones_is_the_solve_without_a_preconditioner(eng):
    """precond = (None, ones, None) takes the preconditioned path (a z vector, the scale kernel, the r.z kernel) and must return the
    bits of precond = None, where z is r and r.z is the r.r of the update kernel; so must a struct of three NULL parts."""
    P = pc.problem()
    for dtype, lim in PREC.items():
        for fmt, opts in LAYOUTS:
            A = handle(eng, P, fmt, dtype, **opts)
            what = f"{A.format_name} {np.dtype(dtype).name}"
            a = A.pcg_tri(P.b.astype(dtype), tol=lim["tol"], max_iterations=MAX_ITERATIONS)
            b = A.pcg_tri(P.b.astype(dtype), precond=(None, np.ones(P.n), None), tol=lim["tol"], max_iterations=MAX_ITERATIONS)
            c = A.pcg_tri(P.b.astype(dtype), precond=(None, None, None), tol=lim["tol"], max_iterations=MAX_ITERATIONS)
            A.close()
            assert a["stop"] == 1
            _same(a, b, what + " ones")
            _same(a, c, what + " three NULL parts")


def test_blocked_handles_that_drop_nothing_are_the_global_ones(eng):
    """blocked handles with B >= n against global handles, and one of each: the same bits"""
    P = pc.problem()
    for dtype, lim in PREC.items():
        A = handle(eng, P, "sell_c_sigma", dtype)
        runs = {}
        for kind in ("sgs", MIXED_B, "mixed"):
            M = precond(eng, P, kind, dtype)
            if kind == MIXED_B:
                assert M[0].block_info()["block_rows"] == MIXED_B and M[0].block_info()["nnz_dropped"] == 0
            if kind == "mixed":
                assert M[0].block_info()["block_rows"] == 0 and M[2].block_info()["block_rows"] == MIXED_B
            runs[kind] = A.pcg_tri(P.b.astype(dtype), precond=M, tol=lim["tol"], max_iterations=MAX_ITERATIONS)
            close(M)
        A.close()
        assert runs["sgs"]["stop"] == 1
        _same(runs["sgs"], runs[MIXED_B], f"{np.dtype(dtype).name}: B >= n")
        _same(runs["sgs"], runs["mixed"], f"{np.dtype(dtype).name}: mixed")


def test_sgs_precond_is_the_hand_built_triple(eng):
    P = pc.problem()
    rp, ci, va = P.csr
    for dtype, lim in PREC.items():
        for B in (None, 100):
            M = eng.sgs_precond(rp, ci, va, P.n, dtype, block_rows=B)
            H = precond(eng, P, "sgs" if B is None else B, dtype)
            assert M[1].dtype == dtype and np.array_equal(M[1], H[1])
            assert M[0].block_info() == H[0].block_info() and M[2].block_info() == H[2].block_info()
            assert M[0].block_info()["block_rows"] == (B or 0)
            A = handle(eng, P, "sell_c_sigma", dtype)
            a = A.pcg_tri(P.b.astype(dtype), precond=M, tol=lim["tol"], max_iterations=MAX_ITERATIONS)
            b = A.pcg_tri(P.b.astype(dtype), precond=H, tol=lim["tol"], max_iterations=MAX_ITERATIONS)
            assert a["stop"] == 1
            _same(a, b, f"{np.dtype(dtype).name} B={B}")
            # the same triple serves gmres
            g = A.gmres(P.b.astype(dtype), restart=20, precond=M, tol=lim["tol"], max_iterations=MAX_ITERATIONS)
            h = A.gmres(P.b.astype(dtype), restart=20, precond=H, tol=lim["tol"], max_iterations=MAX_ITERATIONS)
            assert g["stop"] == 1 and np.array_equal(g["x"], h["x"]) and np.array_equal(g["history"], h["history"])
            A.close()
            close(M)
            close(H)


# ---- 3. frozen after the stop -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ("none", 64, "ic0"), ids=str)
def test_frozen_after_the_stop(eng, kind):
    """A tol that stops at step k returns the x, the iterations and the history[:k] of the same solve with max_iterations = k and
    tol = 0, whatever the host enqueued past the stop: SpMVs, triangular solves and scale kernels that know nothing of the stop flag.
    "none" and B = 64 stop past 2 * POLL = 64, IC(0) below it; in every case 200 further bodies are allowed, the host runs ahead of
    the device and stops enqueueing on the progress word."""
    P = pc.problem()
    b = np.ascontiguousarray(P.b)
    M = precond(eng, P, kind, np.float64)
    for fmt, opts in LAYOUTS:
        A = handle(eng, P, fmt, np.float64, **opts)
        got = A.pcg_tri(b, precond=M, tol=1e-12, max_iterations=MAX_ITERATIONS)
        k = got["iterations"]
        assert got["stop"] == 1 and (k > 2 * POLL) == (kind != "ic0")
        x_long, h_long = np.full(P.n, 7.0), np.full(k + 200, 7.0)
        rc, long_ = raw(eng, A, b, x_long, M, 1e-12, k + 200, h_long)
        assert rc == 0 and (long_.stop, long_.iterations) == (1, k)
        x_short, h_short = np.full(P.n, 7.0), np.full(k, 7.0)
        rc, short = raw(eng, A, b, x_short, M, 0.0, k, h_short)
        assert rc == 0 and (short.stop, short.iterations) == (2, k)
        assert np.array_equal(x_long, x_short) and np.array_equal(x_long, got["x"])
        assert np.array_equal(h_long[:k], h_short) and np.array_equal(h_short, got["history"]) and np.all(h_short > 0)
        assert np.all(h_long[k:] == 0)
        assert (long_.rnorm, long_.rnorm0, long_.prnorm, long_.xnorm) == (short.rnorm, short.rnorm0, short.prnorm, short.xnorm)
        assert short.spmv_calls == k + 1
        assert k + 1 <= long_.spmv_calls <= k + 1 + 2 * POLL                # the host stopped enqueueing
        if kind == "ic0":
            assert long_.spmv_calls > k + 1                                 # it did run ahead
        A.close()
    close(M)


# ---- 4. the stops ---------------------------------------------------------------------------------------------------------------------------

def test_the_stops(eng):
    P = pc.problem()
    M = precond(eng, P, 100, np.float64)
    for fmt, opts in LAYOUTS:
        A = handle(eng, P, fmt, np.float64, **opts)
        N = handle(eng, P, fmt, np.float64, values=-P.csr[2], **opts)
        what = A.format_name
        for pre in (None, M):
            # tol = 0 never stops on the tolerance
            got = A.pcg_tri(P.b, precond=pre, tol=0.0, max_iterations=10)
            _, ref, ref_stop = P.restatement(np.float64, "none" if pre is None else 100, 0.0, 10)
            assert (got["stop"], got["iterations"], got["spmv_calls"]) == (2, 10, 11) and ref_stop == 2, what
            assert got["history"].shape == (10,) and got["prnorm"] == got["history"][-1]
            np.testing.assert_allclose(got["history"], ref, rtol=1e-6, err_msg=what)
            for key, v in pc.shares_of_the_bounds(P, got, np.float64).items():
                assert v <= 1, f"{what}: {key} is {v:.3g} times its bound"
            # max_iterations = 0: x = 0, stop 2, rnorm = rnorm0
            got = A.pcg_tri(P.b, precond=pre, max_iterations=0)
            assert (got["stop"], got["iterations"], got["spmv_calls"]) == (2, 0, 1) and not got["x"].any(), what
            assert got["rnorm"] == got["rnorm0"] > 0 and got["xnorm"] == 0 and got["history"].shape == (0,)
            assert got["prnorm"] == pytest.approx(got["rnorm0"], rel=1e-14)
            # b = 0: stop 3, every norm 0
            got = A.pcg_tri(np.zeros(P.n), precond=pre, max_iterations=10)
            assert (got["stop"], got["iterations"]) == (3, 0) and not got["x"].any(), what
            assert got["rnorm"] == got["rnorm0"] == got["prnorm"] == got["xnorm"] == 0
        # -A: p.A p < 0 in the first body: stop 4, 0 iterations, x = 0, nothing in the history
        x, hist = np.full(P.n, 7.0), np.full(10, 7.0)
        rc, info = raw(eng, N, np.ascontiguousarray(P.b), x, None, 1e-12, 10, hist)
        assert rc == 0 and (info.stop, info.iterations) == (4, 0) and not x.any() and not hist.any(), what
        assert info.rnorm == info.rnorm0 > 0 and info.xnorm == 0 and info.prnorm == pytest.approx(info.rnorm0, rel=1e-14)
        # a negative scale is legal: r.z < 0 at the start: stop 4, 0 iterations
        got = A.pcg_tri(P.b, precond=(None, -1.0 / P.diag, None), max_iterations=10)
        assert (got["stop"], got["iterations"]) == (4, 0) and not got["x"].any() and got["rnorm"] == got["rnorm0"], what
        A.close()
        N.close()
    close(M)


def test_a_value_storage_handle_solves_the_rounded_matrix(eng):
    """fp64 vectors over fp32-stored values give, bit for bit, the solve of the fp64 handle built from (double) (float) values, under
    the same preconditioner; the rounding is symmetric, so the rounded matrix is SPD like A"""
    P = pc.problem()
    rounded = P.csr[2].astype(np.float32).astype(np.float64)
    A4 = handle(eng, P, "sell_c_sigma", np.float64, **dict(DELTA, value_storage=1))
    A8 = handle(eng, P, "sell_c_sigma", np.float64, values=rounded, **dict(DELTA, sell_values=2))
    assert A4.format_name.endswith("_v4") and A4.value_dtype == np.float32 and A8.value_dtype == np.float64
    M = precond(eng, P, 100, np.float64)
    a = A4.pcg_tri(P.b, precond=M, max_iterations=MAX_ITERATIONS)
    b = A8.pcg_tri(P.b, precond=M, max_iterations=MAX_ITERATIONS)
    A4.close()
    A8.close()
    close(M)
    assert a["stop"] == 1
    _same(a, b, "value_storage = 1")
    Dr = P.D.astype(np.float32).astype(np.float64)
    assert np.linalg.norm(P.b - Dr @ a["x"]) <= 10 * 1e-12 * np.linalg.norm(P.b)          # the rounded matrix was solved


# ---- 5. the refusals that need a handle, in their order ---------------------------------------------------------------------------

def _refused(eng, A, n, M, phrases, struct_size=None):
    b, x, hist = np.full(n, 3.5), np.full(n, -7.25), np.full(10, 9.0)
    scale = None if M is None else M[1]
    keep = None if scale is None else scale.copy()
    info = eng.PcgTriInfo()
    info.struct_size = ctypes.sizeof(eng.PcgTriInfo)
    info.iterations, info.stop, info.rnorm, info.spmv_calls = -5, -6, -7.5, -8
    before = bytes(info)
    rc, _ = raw(eng, A, b, x, M, 1e-12, 10, hist, struct_size=struct_size, info=info)
    msg = eng.lib().spmv_mi355x_last_error()
    assert rc == 1 and msg.startswith(b"pcg_tri: ") and all(ph in msg for ph in phrases), msg
    assert np.all(b == 3.5) and np.all(x == -7.25) and np.all(hist == 9.0) and bytes(info) == before
    assert keep is None or keep.tobytes() == scale.tobytes()


def test_refusals_in_their_order(eng):
    P = pc.problem()
    rp, ci, va = P.csr
    A = handle(eng, P, "sell_c_sigma", np.float64)
    L, s, U = precond(eng, P, 100, np.float64)
    small = eng.TriangularSolve(np.arange(4, dtype=np.int32), np.arange(3, dtype=np.int32), np.ones(3), 3, block_rows=2)
    single = eng.TriangularSolve(rp, ci, va, P.n, uplo="upper", dtype=np.float32, block_rows=100)
    wide = eng.Matrix(np.array([0, 1, 2], np.int32), np.array([0, 2], np.int32), np.ones(2), 2, 3, "csr_vector", np.float64)
    bad = s.copy()
    bad[[7, 9]] = 0.0, np.nan
    # 5. the shape, before anything of M
    _refused(eng, wide, 3, (small, bad[:3].copy(), None), (b"2 x 3",), struct_size=8)
    # 6. M itself; whatever else is wrong comes later
    _refused(eng, A, P.n, (small, bad, None), (b"struct_size",), struct_size=8)
    # 7. the handles, first before second, before the scale
    _refused(eng, A, P.n, (small, bad, single), (b"M->first", b"3 rows", b"2025"))
    _refused(eng, A, P.n, (L, bad, small), (b"M->second", b"3 rows"))
    _refused(eng, A, P.n, (L, bad, single), (b"M->second", b"precision"))
    _refused(eng, A, P.n, (single, None, U), (b"M->first", b"precision"))
    # 8. the scale: the first index that is zero or not finite
    _refused(eng, A, P.n, (L, bad, U), (b"scale[7] = 0",))
    for at, value in ((0, np.nan), (2024, np.inf), (1000, -np.inf)):
        one = s.copy()
        one[at] = value
        _refused(eng, A, P.n, (None, one, None), (f"scale[{at}]".encode(),))
    with pytest.raises(eng.SpmvError, match=r"pcg_tri: scale\[7\]"):
        A.pcg_tri(P.b, precond=(L, bad, U))
    A.close()
    wide.close()
    close((L, U, small, single))
