"""The factorized sparse approximate inverse on the GPU (include/spmv_mi355x.h "FSAI"): spmv_mi355x_fsai_* / Fsai and
spmv_mi355x_pcg_fsai / Matrix.pcg_tri(precond=<Fsai>).

1. The row kernel. G's fp64 values BIT FOR BIT those of tests/fsai_reference.c (the header's arithmetic as one sequential loop, gcc
   -ffp-contract=off; itself checked against numpy in test_fsai_abi.py) and fallback_rows equal to its count, on the cases of
   fsai_cases.py. Their rows hold 1 .. 128 pattern entries and hit every bin of csrc/fsai.hpp (1 .. 8, 9 .. 32, 33 .. 64, 65 .. 128):
   spd_grid(45) on tril(A) (s <= 3) and tril(A)^2 (s <= 6); banded SPD of n = 400 with half-bandwidth 70 (s = 71: wider than a wave)
   and 127 (s = 128: the cap), 128 being refused; a random symmetric pattern of n = 1000 with 1 .. 40 entries per row, rows of one
   entry among them and A's rows unsorted; a 2 x 2 indefinite local block (the breakdown rule); n = 0 and n = 1; and a tridiagonal
   matrix of 32 * 2048 + 37 rows: rows of at most 8 entries share a workgroup 32 at a time and a launch has at most 2048
   workgroups, so past 65536 rows the workgroups' row loop takes a second trip. Both precisions of the handle: values() is fp64 either
   way, and the G handle holds the narrowed values (G.spmv against numpy).
2. apply(v) bit for bit Gt.spmv(G.spmv(v)) through the borrowed handles, within 1e-12 / 1e-5 of numpy's |G^t| (|G| |v|) entry by
   entry (two SpMVs of at most 6 products per row: the rounding of the handle's precision stays two orders below that), and in place.
3. The solver, with the checks and bounds of test_gpu_pcg_tri.py for its preconditioned kinds, over its three layouts (A's, and G's
   and G^t's), two precisions and the patterns tril(A) and tril(A)^2: the dense solve, numpy's explicit norms, the history rows
   against pcg_tri_cases.restate with M^-1 = G^t (G .) from the C reference, the iteration count within 1 of fsai_cases.COUNTS
   (58 / 25 and 41 / 18); frozen after the stop; stops 2, 3 and 4; value_storage = 1 on A; the refusals that need a handle.
4. spmv_mi355x_pcg_tri still returns what it returned: the preconditioned body now takes "z = M^-1 r" as a callable, and the FSAI of
   the identity matrix (G = I exactly) enters that body a second way. Its solve must equal, bit for bit, precond = None and
   precond = (None, ones, None), which test_gpu_pcg_tri.py pins to each other; and the SGS solve is pinned to its hand-built triple,
   to itself, and to the restatement's count."""
import ctypes

import numpy as np
import pytest

import fsai_cases as fc
import pcg_tri_cases as pc
from pcg_tri_cases import MAX_ITERATIONS, POLL, PREC

pytestmark = pytest.mark.gpu

DELTA = dict(sell_c=64, sell_delta=1, sell_sigma=64, sell_window=2)
LAYOUTS = [("sell_c_sigma", {}), ("csr_vector", {}), ("sell_c_sigma", DELTA)]
INFO_FIELDS = ("iterations", "stop", "rnorm", "rnorm0", "prnorm", "xnorm")
APPLY_TOL = {np.float64: 1e-12, np.float32: 1e-5}
KERNEL_CASES = ("grid_tril", "grid_power2", "banded70", "banded127", "random", "indefinite", "one", "tridiagonal_wrap")


@pytest.fixture(scope="module")
def eng():
    import spmv_mi355x as eng
    assert eng.device_count() >= 1, "no GPU visible: the -m gpu tests need an MI355X"
    return eng


def fsai(eng, name, dtype=np.float64, fmt="sell_c_sigma", **opts):
    rp, ci, va, n, pattern = fc.case(name)
    return eng.Fsai(rp, ci, va, n, pattern, fmt, dtype, **opts)


def grid_fsai(eng, power, dtype, fmt="sell_c_sigma", **opts):
    return fsai(eng, fc.grid_case(power), dtype, fmt, **opts)


def handle(eng, P, fmt, dtype, values=None, **opts):
    rp, ci, va = P.csr
    return eng.Matrix(rp, ci, va if values is None else values, P.n, P.n, fmt, dtype, **opts)


def _same(a, b, what):
    for k in INFO_FIELDS:
        assert a[k] == b[k], f"{what}: {k}: {a[k]!r} and {b[k]!r}"
    assert np.array_equal(a["x"], b["x"]), f"{what}: x"
    assert np.array_equal(a["history"], b["history"]), f"{what}: history"


def raw(eng, A, b, x, F, tol, max_iterations, hist, info=None):
    """the C call on the caller's own buffers: (rc, info). F = None passes a NULL handle."""
    if info is None:
        info = eng.PcgTriInfo()
        info.struct_size = ctypes.sizeof(eng.PcgTriInfo)
    p = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
    rc = eng.lib().spmv_mi355x_pcg_fsai(None if A is None else A.h, p(b), p(x), None if F is None else F.h, tol, max_iterations, p(hist),
                                        ctypes.byref(info))
    return rc, info


# ---- 1. the row kernel -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", KERNEL_CASES)
def test_the_values_are_the_references_bit_for_bit(eng, name):
    c = fc.case(name)
    n = c[3]
    prp, pci = fc.pattern_of(c)
    want, want_fell = fc.reference_of(name)
    assert want_fell == (1 if name == "indefinite" else 0)
    for dtype in (np.float64, np.float32):
        F = fsai(eng, name, dtype)
        got, info = F.values(), F.info()
        assert got.dtype == np.float64 and got.shape == want.shape
        diff = np.nonzero(got != want)[0]
        worst = np.abs(got - want).max() if len(diff) else 0.0
        print(f"[fsai] {name} {np.dtype(dtype).name}: {len(diff)} of {len(want)} values differ from the C reference (largest {worst:.3g}); "
              f"kernel {info['kernel_seconds']:.3g} s, setup {info['setup_seconds']:.3g} s")
        assert len(diff) == 0, f"{name}: entry {diff[0]} is {got[diff[0]]!r}, the reference has {want[diff[0]]!r}"
        assert (info["n"], info["nnz"], info["max_row"], info["fallback_rows"]) == (n, len(want), int(np.diff(prp).max()), want_fell)
        # the G handle holds the values narrowed to the handle's precision, G^t their transpose
        assert (F.G.m, F.G.n, F.G.nnz, F.G.transposed, F.Gt.transposed) == (n, n, len(want), 0, 1) and F.G.dtype == dtype
        if n <= 2025:
            G = fc.dense_g(c, want, dtype).astype(np.float64)
            v = np.random.default_rng(3).uniform(-1, 1, n).astype(dtype)
            for M, D in ((F.G, G), (F.Gt, G.T)):
                err = np.abs(M.spmv(v).astype(np.float64) - D @ v.astype(np.float64))
                assert np.all(err <= APPLY_TOL[dtype] * (np.abs(D) @ np.abs(v).astype(np.float64))), (name, err.max())
        assert F.mem_footprint >= F.G.mem_footprint + F.Gt.mem_footprint
        F.close()
        F.close()                                                      # closing twice is harmless


def test_the_breakdown_row(eng):
    F = fsai(eng, "indefinite")
    prp, _ = fc.pattern_of(fc.case("indefinite"))
    g = F.values()
    assert g[prp[1]:prp[2]].tolist() == [0.0, 1.0] and F.info()["fallback_rows"] == 1 and np.all(np.isfinite(g))
    F.close()


def test_n_zero(eng):
    import torch
    for dtype in (np.float64, np.float32):
        F = fsai(eng, "empty", dtype)
        assert F.info()["n"] == F.info()["nnz"] == F.info()["max_row"] == F.info()["fallback_rows"] == 0
        assert F.G is None and F.Gt is None and F.values().shape == (0,) and F.apply(np.zeros(0, dtype)).shape == (0,)
        x = torch.full((8,), -7.25, dtype=torch.float64, device="cuda")
        F.apply_device(x.data_ptr(), x.data_ptr())
        F.apply_device(0, 0)
        torch.cuda.synchronize()
        assert bool(torch.all(x == -7.25)) and F.mem_footprint == 0
        F.close()


def test_a_row_of_129_entries_is_refused(eng):
    rp, ci, va, n, _ = fc.case("banded128")
    with pytest.raises(eng.SpmvError, match=r"fsai_create: .*row 128 has 129 entries"):
        eng.Fsai(rp, ci, va, n)


def test_an_explicit_pattern_is_the_default_one(eng):
    """pattern = None and the same pattern given explicitly (fsai_pattern, power 1) build the same G, A's rows unsorted"""
    rp, ci, va, n, _ = fc.case("random")
    pat = eng.fsai_pattern(rp, ci, n, 1)
    a, b = eng.Fsai(rp, ci, va, n), eng.Fsai(rp, ci, va, n, pat)
    assert np.array_equal(a.values(), b.values()) and np.array_equal(a.values(), fc.reference_of("random")[0])
    a.close()
    b.close()


# ---- 2. apply --------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("power", (1, 2))
def test_apply_is_the_two_products(eng, power):
    import torch
    name = fc.grid_case(power)
    c = fc.case(name)
    n = c[3]
    for dtype, tol in APPLY_TOL.items():
        G = fc.dense_g(c, fc.reference_of(name)[0], dtype).astype(np.float64)
        v = np.random.default_rng(9).uniform(-1, 1, n).astype(dtype)
        for fmt, opts in LAYOUTS:
            F = grid_fsai(eng, power, dtype, fmt, **opts)
            got = F.apply(v)
            assert got.dtype == dtype and np.array_equal(got, F.Gt.spmv(F.G.spmv(v))), (fmt, opts)
            err = np.abs(got.astype(np.float64) - G.T @ (G @ v.astype(np.float64)))
            bound = tol * (np.abs(G.T) @ (np.abs(G) @ np.abs(v).astype(np.float64)))
            print(f"[fsai] apply power {power} {np.dtype(dtype).name} {F.G.format_name}: {float((err / bound).max()):.3g} of its bound")
            assert np.all(err <= bound)
            # in place, and into another vector, on the device
            t = torch.from_numpy(v).cuda()
            u = torch.zeros_like(t)
            F.apply_device(t.data_ptr(), u.data_ptr())
            F.apply_device(t.data_ptr(), t.data_ptr())
            torch.cuda.synchronize()
            assert np.array_equal(t.cpu().numpy(), got) and np.array_equal(u.cpu().numpy(), got)
            F.close()


# ---- 3. the solver -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("power", (1, 2))
def test_against_the_dense_solve_and_the_restatement(eng, power):
    P = pc.problem()
    want = P.solve()
    worst, counts = {}, {}
    for dtype, lim in PREC.items():
        name = np.dtype(dtype).name
        _, ref, ref_stop = fc.grid_restatement(power, dtype, lim["tol"])
        assert ref_stop == 1 and abs(ref.size - fc.COUNTS[dtype][power]) <= 1
        bn = np.linalg.norm(P.b.astype(dtype).astype(np.float64))
        rows = np.nonzero(ref / bn > lim["ratio"])[0]
        assert rows[-1] == rows.size - 1                                   # a leading stretch
        assert rows.size >= lim["share"] * ref.size, f"{name}: {rows.size} of {ref.size} rows qualify"
        for fmt, opts in LAYOUTS:
            A = handle(eng, P, fmt, dtype, **opts)
            F = grid_fsai(eng, power, dtype, fmt, **opts)
            what = f"spd_grid(45) {A.format_name} {name} FSAI power {power}"
            got = A.pcg_tri(P.b.astype(dtype), precond=F, tol=lim["tol"], max_iterations=MAX_ITERATIONS)
            again = A.pcg_tri(P.b.astype(dtype), precond=F, tol=lim["tol"], max_iterations=MAX_ITERATIONS)
            A.close()
            F.close()
            _same(got, again, what)
            k = got["iterations"]
            print(f"[pcg_fsai] {what}: {k} iterations (the restatement {ref.size}), rnorm {got['rnorm']:.3g}")
            assert got["stop"] == 1, f"{what}: stop {got['stop']} after {k} iterations"
            assert got["x"].dtype == dtype and got["x"].shape == (P.n,) and got["history"].shape == (k,)
            assert got["prnorm"] == got["history"][-1] and got["prnorm"] <= lim["tol"] * got["rnorm0"] * (1 + 1e-12), what
            assert k + 1 <= got["spmv_calls"] <= k + 1 + 2 * POLL, what
            for key, v in pc.shares_of_the_bounds(P, got, dtype, want).items():
                print(f"[pcg_fsai] {what}: {key} is {v:.3g} of its bound")
                assert v <= 1, f"{what}: {key} is {v:.3g} times its bound"
                worst[key] = max(worst.get(key, 0), float(v))
            counts[(name, fmt, bool(opts))] = (k, ref.size)
            assert abs(k - ref.size) <= 1 and abs(k - fc.COUNTS[dtype][power]) <= 1, f"{what}: {k} iterations, the restatement {ref.size}"
            assert k >= rows.size, what
            d = np.abs(got["history"][rows] - ref[rows]) / ref[rows]
            print(f"[pcg_fsai] {what}: largest history deviation {d.max():.3g} on {rows.size} rows")
            assert d.max() <= lim["hist"], f"{what}: history deviates by {d.max():.3g} at row {np.argmax(d)}"
    print(f"[pcg_fsai] power {power}: largest shares {worst}; (iterations, the restatement's) {counts}")


@pytest.mark.parametrize("power", (1, 2))
def test_frozen_after_the_stop(eng, power):
    """A tol that stops at step k returns the x, the iterations and the history[:k] of the same solve with max_iterations = k and
    tol = 0, whatever the host enqueued past the stop: SpMVs with A, G and G^t, which know nothing of the stop flag and write only q,
    F's scratch vector and z. Both counts lie below 2 * POLL = 64, 200 further bodies are allowed: the host runs ahead of the device."""
    P = pc.problem()
    b = np.ascontiguousarray(P.b)
    for fmt, opts in LAYOUTS:
        A = handle(eng, P, fmt, np.float64, **opts)
        F = grid_fsai(eng, power, np.float64, fmt, **opts)
        got = A.pcg_tri(b, precond=F, tol=1e-12, max_iterations=MAX_ITERATIONS)
        k = got["iterations"]
        assert got["stop"] == 1 and k < 2 * POLL
        x_long, h_long = np.full(P.n, 7.0), np.full(k + 200, 7.0)
        rc, long_ = raw(eng, A, b, x_long, F, 1e-12, k + 200, h_long)
        assert rc == 0 and (long_.stop, long_.iterations) == (1, k)
        x_short, h_short = np.full(P.n, 7.0), np.full(k, 7.0)
        rc, short = raw(eng, A, b, x_short, F, 0.0, k, h_short)
        assert rc == 0 and (short.stop, short.iterations) == (2, k)
        assert np.array_equal(x_long, x_short) and np.array_equal(x_long, got["x"])
        assert np.array_equal(h_long[:k], h_short) and np.array_equal(h_short, got["history"]) and np.all(h_short > 0)
        assert np.all(h_long[k:] == 0)
        assert (long_.rnorm, long_.rnorm0, long_.prnorm, long_.xnorm) == (short.rnorm, short.rnorm0, short.prnorm, short.xnorm)
        assert short.spmv_calls == k + 1
        assert k + 1 < long_.spmv_calls <= k + 1 + 2 * POLL                 # the host ran ahead and stopped enqueueing
        A.close()
        F.close()


def test_the_stops(eng):
    P = pc.problem()
    for fmt, opts in LAYOUTS:
        A = handle(eng, P, fmt, np.float64, **opts)
        N = handle(eng, P, fmt, np.float64, values=-P.csr[2], **opts)
        F = grid_fsai(eng, 1, np.float64, fmt, **opts)
        what = A.format_name
        # stop 2: tol = 0 never stops on the tolerance
        got = A.pcg_tri(P.b, precond=F, tol=0.0, max_iterations=10)
        _, ref, ref_stop = fc.grid_restatement(1, np.float64, 0.0, 10)
        assert (got["stop"], got["iterations"], got["spmv_calls"]) == (2, 10, 11) and ref_stop == 2, what
        assert got["history"].shape == (10,) and got["prnorm"] == got["history"][-1]
        np.testing.assert_allclose(got["history"], ref, rtol=1e-6, err_msg=what)
        for key, v in pc.shares_of_the_bounds(P, got, np.float64).items():
            assert v <= 1, f"{what}: {key} is {v:.3g} times its bound"
        # max_iterations = 0: x = 0, stop 2, rnorm = rnorm0
        got = A.pcg_tri(P.b, precond=F, max_iterations=0)
        assert (got["stop"], got["iterations"], got["spmv_calls"]) == (2, 0, 1) and not got["x"].any(), what
        assert got["rnorm"] == got["rnorm0"] > 0 and got["xnorm"] == 0 and got["history"].shape == (0,)
        # stop 3: b = 0, every norm 0
        got = A.pcg_tri(np.zeros(P.n), precond=F, max_iterations=10)
        assert (got["stop"], got["iterations"]) == (3, 0) and not got["x"].any(), what
        assert got["rnorm"] == got["rnorm0"] == got["prnorm"] == got["xnorm"] == 0
        # stop 4: -A under the FSAI of A: r.z > 0 at the start, p.A p < 0 in the first body: 0 iterations, x = 0, an empty history
        x, hist = np.full(P.n, 7.0), np.full(10, 7.0)
        rc, info = raw(eng, N, np.ascontiguousarray(P.b), x, F, 1e-12, 10, hist)
        assert rc == 0 and (info.stop, info.iterations) == (4, 0) and not x.any() and not hist.any(), what
        assert info.rnorm == info.rnorm0 > 0 and info.xnorm == 0
        A.close()
        N.close()
        F.close()


def test_a_value_storage_handle_solves_the_rounded_matrix(eng):
    """fp64 vectors over fp32-stored values of A give, bit for bit, the solve of the fp64 handle built from (double) (float) values,
    under the same FSAI (built from the unrounded A)"""
    P = pc.problem()
    rounded = P.csr[2].astype(np.float32).astype(np.float64)
    A4 = handle(eng, P, "sell_c_sigma", np.float64, **dict(DELTA, value_storage=1))
    A8 = handle(eng, P, "sell_c_sigma", np.float64, values=rounded, **dict(DELTA, sell_values=2))
    assert A4.format_name.endswith("_v4") and A4.value_dtype == np.float32 and A8.value_dtype == np.float64
    F = grid_fsai(eng, 2, np.float64)
    a = A4.pcg_tri(P.b, precond=F, max_iterations=MAX_ITERATIONS)
    b = A8.pcg_tri(P.b, precond=F, max_iterations=MAX_ITERATIONS)
    A4.close()
    A8.close()
    F.close()
    assert a["stop"] == 1
    _same(a, b, "value_storage = 1")
    Dr = P.D.astype(np.float32).astype(np.float64)
    assert np.linalg.norm(P.b - Dr @ a["x"]) <= 10 * 1e-12 * np.linalg.norm(P.b)          # the rounded matrix was solved


def _refused(eng, A, n, F, phrases):
    b, x, hist = np.full(n, 3.5), np.full(n, -7.25), np.full(10, 9.0)
    info = eng.PcgTriInfo()
    info.struct_size = ctypes.sizeof(eng.PcgTriInfo)
    info.iterations, info.stop, info.rnorm, info.spmv_calls = -5, -6, -7.5, -8
    before = bytes(info)
    rc, _ = raw(eng, A, b, x, F, 1e-12, 10, hist, info=info)
    msg = eng.lib().spmv_mi355x_last_error()
    assert rc == 1 and msg.startswith(b"pcg_fsai: ") and all(ph in msg for ph in phrases), msg
    assert np.all(b == 3.5) and np.all(x == -7.25) and np.all(hist == 9.0) and bytes(info) == before


def test_refusals_in_their_order(eng):
    P = pc.problem()
    A = handle(eng, P, "sell_c_sigma", np.float64)
    wide = eng.Matrix(np.array([0, 1, 2], np.int32), np.array([0, 2], np.int32), np.ones(2), 2, 3, "csr_vector", np.float64)
    small = fsai(eng, "indefinite")
    single = grid_fsai(eng, 1, np.float32)
    # 5. the shape, before anything of F
    _refused(eng, wide, 3, None, (b"2 x 3",))
    # then F NULL: the message points to the solver without a preconditioner
    _refused(eng, A, P.n, None, (b"F is NULL", b"spmv_mi355x_pcg_tri"))
    # then n before the precision
    _refused(eng, A, P.n, small, (b"5 rows", b"2025"))
    _refused(eng, A, P.n, single, (b"precision",))
    with pytest.raises(eng.SpmvError, match=r"pcg_fsai: F is a preconditioner of 5 rows"):
        A.pcg_tri(P.b, precond=small)
    # what fsai_create leaves to spmv_mi355x_create comes back with both names
    rp, ci, va, n, _ = fc.case("grid_tril")
    with pytest.raises(eng.SpmvError, match=r"fsai_create: .*sell_c"):
        eng.Fsai(rp, ci, va, n, sell_c=7)
    A.close()
    wide.close()
    small.close()
    single.close()


# ---- 4. pcg_tri returns what it returned -----------------------------------------------------------------------------------------------

def test_pcg_tri_is_unchanged(eng):
    P = pc.problem()
    rp, ci, va = P.csr
    eye = (np.arange(P.n + 1, dtype=np.int32), np.arange(P.n, dtype=np.int32), np.ones(P.n))
    for dtype, lim in PREC.items():
        name = np.dtype(dtype).name
        I = eng.Fsai(*eye, P.n, dtype=dtype)
        assert np.array_equal(I.values(), np.ones(P.n)) and I.info()["fallback_rows"] == 0
        A = handle(eng, P, "sell_c_sigma", dtype)
        b = P.b.astype(dtype)
        none = A.pcg_tri(b, tol=lim["tol"], max_iterations=MAX_ITERATIONS)
        ones = A.pcg_tri(b, precond=(None, np.ones(P.n), None), tol=lim["tol"], max_iterations=MAX_ITERATIONS)
        ident = A.pcg_tri(b, precond=I, tol=lim["tol"], max_iterations=MAX_ITERATIONS)
        assert none["stop"] == 1 and abs(none["iterations"] - pc.COUNTS[dtype]["none"]) <= 1
        _same(none, ones, f"{name}: a scale of ones")
        _same(none, ident, f"{name}: the FSAI of the identity")
        I.close()
        # the SGS of A: sgs_precond against the hand-built triple, twice, and the restatement's count
        M = eng.sgs_precond(rp, ci, va, P.n, dtype, block_rows=100)
        H = (eng.TriangularSolve(rp, ci, va, P.n, uplo="lower", dtype=dtype, block_rows=100), P.diag.astype(dtype),
             eng.TriangularSolve(rp, ci, va, P.n, uplo="upper", dtype=dtype, block_rows=100))
        a = A.pcg_tri(b, precond=M, tol=lim["tol"], max_iterations=MAX_ITERATIONS)
        c = A.pcg_tri(b, precond=H, tol=lim["tol"], max_iterations=MAX_ITERATIONS)
        d = A.pcg_tri(b, precond=M, tol=lim["tol"], max_iterations=MAX_ITERATIONS)
        _, ref, _ = P.restatement(dtype, 100, lim["tol"])
        assert a["stop"] == 1 and abs(a["iterations"] - ref.size) <= 1
        _same(a, c, f"{name}: sgs_precond and the hand-built triple")
        _same(a, d, f"{name}: twice")
        for T in (M[0], M[2], H[0], H[2]):
            T.close()
        A.close()
