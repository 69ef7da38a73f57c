"""The Jacobi-sweep triangular solve on the GPU (include/spmv_mi355x.h "JACOBI SWEEPS"): spmv_mi355x_trsv_solve_sweeps*,
trsv_set_sweeps and the solvers that pick the sweeps up through a handle.

BITS. The contract is exact, so every comparison of a solve is equality of bytes and no tolerance appears in the first part of this
file. The reference is ALWAYS the sequential restatement of tests/trsv_sweeps_reference.c (trsv_sweeps_cases.reference; on the CSR
filtered by trsv_blocked_cases.filtered for a blocked handle), first asserted to be finite; from `levels` sweeps on the result is also
held to the SAME handle's exact solve(). x is pre-filled with NaN and sits at an odd element offset between guards; the guards, the
ld - k padding columns and b must survive, compared as bytes.

The matrices are those of trsv_cases.py, already the smallest that break the kernels of the exact solve: one row; 1500 rows in one
level (several workgroups, a short last slice); prescribed (slices of 1, 64, 65, 70, 2000 and 3000 rows); a 700-entry row among
one-entry rows (the unroll tail); dag (708 levels, most of one row: a wave per row); the 24^3 stencil. The sweep counts are 1, 2, 3, 5
and levels - 1, levels, levels + 3 (dag: 1, 2, 5, 708): the first-sweep kernel alone, both parities of the ping-pong, the boundary
of exactness and the cap min(sweeps, levels).

SOLVERS. pcg_tri, pcg_trsm_multi and gmres under swept triples on the problems of pcg_tri_cases.py and trsv_blocked_cases.convdiff
(n = 2025), against the numpy restatements with the sweep reference as M and under the bounds of test_gpu_pcg_tri.py /
test_gpu_gmres_tri.py (PREC, shares_of_the_bounds), which are imported, not restated."""
import functools

import numpy as np
import pytest

import ilu0_cases as ic
import pcg_tri_cases as pc
import trsv_blocked_cases as bc
import trsv_cases as tc
import trsv_sweeps_cases as sc
from trsv_cases import LOWER, UPPER

pytestmark = pytest.mark.gpu

GUARD = 8
SENTINEL = 777.0
SIDES = ((LOWER, "lower"), (UPPER, "upper"))
DTYPES = (np.float64, np.float32)
KS = (1, 2, 3, 5, 8, 11)
KMAX = max(KS)


@pytest.fixture(scope="module")
def eng():
    import spmv_mi355x as eng
    assert eng.device_count() >= 1, "no GPU visible: the -m gpu tests need an MI355X"
    assert hasattr(eng.lib(), "spmv_mi355x_trsv_solve_sweeps_device_async")
    return eng


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def word_of(dtype):
    return np.uint64 if np.dtype(dtype) == np.float64 else np.uint32


def sweep_device(T, b, sweeps, in_place=False, solve=None):
    """x of T.solve_sweeps_device for the vector b; x starts one element behind a guard of 8 (an odd element offset) and is followed
    by another guard. Checks both guards and, when not in place, b. `solve` replaces the call (the routed entries)."""
    import torch
    n, dtype = len(b), b.dtype
    lo = GUARD + 1
    hx = np.full(lo + n + GUARD, SENTINEL, dtype)
    hx[lo:lo + n] = b if in_place else np.nan
    tx = torch.from_numpy(hx.copy()).to("cuda")
    tb = tx if in_place else torch.from_numpy(np.array(b)).to("cuda")
    xp = tx.data_ptr() + lo * tx.element_size()
    bp = xp if in_place else tb.data_ptr()
    if solve is None:
        T.solve_sweeps_device(bp, xp, sweeps)
    else:
        solve(bp, xp)
    torch.cuda.synchronize()
    got = tx.cpu().numpy()
    assert np.all(got[:lo] == SENTINEL) and np.all(got[lo + n:] == SENTINEL), "a guard of x was overwritten"
    if not in_place:
        assert tb.cpu().numpy().tobytes() == np.ascontiguousarray(b).tobytes(), "b was modified"
    return np.ascontiguousarray(got[lo:lo + n])


def slices_of(rp, ci, n, uplo, B=None):
    """slices of the stored layout: every level (of every block) in pieces of 64 rows"""
    M = (rp, ci, None, n) if B is None else bc.filtered(rp, ci, np.zeros(len(ci)), n, B)
    level = tc.levels_of(M[0], M[1], n, uplo).astype(np.int64)
    key = level if B is None else (np.arange(n) // B) * (int(level.max()) + 1) + level
    return int(np.sum(-(-np.bincount(key)[np.bincount(key) > 0] // 64)))


@functools.lru_cache(maxsize=None)
def expected(name, B, uplo, unit, dtype, sweeps):
    """the reference x(sweeps) of the named matrix (filtered with B for a blocked handle) on sc.rhs, finite"""
    A = bc.matrix(name, uplo)
    M = A if B is None else bc.filtered(*A, B)
    x = sc.reference(*M, uplo, unit, sc.rhs(A[3], dtype), dtype, sweeps)
    assert np.all(np.isfinite(x)), "the reference overflowed: two non-finite results must not pass as equal"
    x.setflags(write=False)
    return x


def check_counts(T, name, B, uplo, unit, dtype, in_place_at=()):
    A = bc.matrix(name, uplo)
    n = A[3]
    levels = sc.depth(name, uplo, B)
    assert T.info["levels"] == levels
    b = sc.rhs(n, dtype)
    exact = T.solve(b)
    what = f"{name} B={B} uplo={uplo} unit={unit} {np.dtype(dtype).name}"
    for s in sc.sweep_counts(name, levels):
        want = expected(name, B, uplo, unit, dtype, s)
        got = sweep_device(T, b, s)
        assert same_bits(got, want), f"{what}: {s} sweeps of {levels} levels: {int(np.sum(got != want))} of {n} rows differ"
        if s >= levels:
            assert same_bits(got, exact), f"{what}: {s} sweeps >= {levels} levels against the handle's exact solve"
        if s in in_place_at:
            assert same_bits(sweep_device(T, b, s, in_place=True), want), f"{what}: {s} sweeps in place"
        assert same_bits(T.solve_sweeps(b, s), want), f"{what}: {s} sweeps, the host form"
    return levels


# ---- single solves ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=("f64", "f32"))
@pytest.mark.parametrize("unit", (False, True), ids=("stored", "unit"))
@pytest.mark.parametrize("uplo,side", SIDES, ids=("lower", "upper"))
@pytest.mark.parametrize("name", sc.MATRICES)
def test_a_sweep_solve_has_the_bits_of_the_restatement(eng, name, uplo, side, unit, dtype):
    A = tc.matrix(name, uplo)
    n = A[3]
    T = eng.TriangularSolve(*A, uplo=side, diag="unit" if unit else "stored", dtype=dtype)
    info, footprint = T.info, eng.lib().spmv_mi355x_trsv_mem_footprint(T.h)
    assert T.sweeps_info()["bytes"] == 0
    top = sc.depth(name, uplo)
    levels = check_counts(T, name, None, uplo, unit, dtype, in_place_at=(1, 2, 3, top if name == "dag" else top + 3))
    # what the handle allocated: the map, and two vectors once a solve ran more than one sweep; none of it in mem_footprint
    size = np.dtype(dtype).itemsize
    assert T.sweeps_info()["bytes"] == 4 * (slices_of(A[0], A[1], n, uplo) + 1) + (2 * n * size if levels > 1 else 0)
    assert T.info == info and eng.lib().spmv_mi355x_trsv_mem_footprint(T.h) == footprint and T.sweeps == 0
    T.close()


@pytest.mark.parametrize("B", (None, 64), ids=("global", "blocked"))
def test_no_rows_launch_nothing(eng, B):
    import torch
    rp, ci, va, n = tc.matrix("empty", LOWER)
    T = eng.TriangularSolve(rp, ci, va, n, block_rows=B)
    x = torch.full((32,), SENTINEL, dtype=torch.float64, device="cuda")
    T.solve_sweeps_device(x.data_ptr(), x.data_ptr(), 3)
    T.solve_sweeps_device(0, 0, 3)                          # no vector is needed for no rows
    T.solve_sweeps_multi_device(3, x.data_ptr(), 3, x.data_ptr(), 3, 2)
    T.set_sweeps(4)
    T.solve_device(x.data_ptr(), x.data_ptr())
    torch.cuda.synchronize()
    assert bool(torch.all(x == SENTINEL))
    assert T.solve_sweeps(np.zeros(0), 2).shape == (0,) and T.solve_sweeps_multi(np.zeros((0, 3)), 2).shape == (0, 3)
    assert T.sweeps_info(3) == dict(sweeps=4, effective=0, launches=0, bytes=0.0)
    T.close()


# ---- blocked handles ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=("f64", "f32"))
@pytest.mark.parametrize("uplo,side", SIDES, ids=("lower", "upper"))
@pytest.mark.parametrize("name", ("stencil", "dag"))
def test_a_blocked_handle_sweeps_the_filtered_matrix(eng, name, uplo, side, dtype):
    """B = 100 does not divide 64-row slices or the stencil's planes; UNIT runs at B = 100. B = 16384 >= n drops nothing: the global
    handle's bits."""
    A = tc.matrix(name, uplo)
    n = A[3]
    for B, unit in ((64, False), (100, False), (100, True), (256, False)):
        T = eng.TriangularSolve(*A, uplo=side, diag="unit" if unit else "stored", dtype=dtype, block_rows=B)
        assert T.block_info()["nnz_dropped"] == bc.dropped_of(A[0], A[1], n, uplo, B) > 0
        levels = check_counts(T, name, B, uplo, unit, dtype, in_place_at=(2, 3))
        assert T.sweeps_info()["bytes"] == 4 * (slices_of(A[0], A[1], n, uplo, B) + 1) + 2 * n * np.dtype(dtype).itemsize and levels > 1
        T.close()
    assert n <= 16384
    T, G = eng.TriangularSolve(*A, uplo=side, dtype=dtype, block_rows=16384), eng.TriangularSolve(*A, uplo=side, dtype=dtype)
    b = sc.rhs(n, dtype)
    for s in (1, 2, 5):
        assert same_bits(sweep_device(T, b, s), sweep_device(G, b, s)) and same_bits(sweep_device(T, b, s), expected(name, None, uplo, False, dtype, s))
    T.close()
    G.close()


# ---- k columns ----------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def block(n, dtype, seed=11):
    rng = np.random.default_rng(seed)
    B = np.ascontiguousarray(np.stack([(10.0 ** (j % 3 - 1)) * rng.uniform(-1, 1, n) for j in range(KMAX)], axis=1).astype(dtype))
    B.setflags(write=False)
    return B


def sweep_multi(T, Bh, sweeps, ld=None, shift=0, col0=0, in_place=False, solve=None):
    """test_gpu_trsv_multi.py's placement for solve_sweeps_multi_device: the n x k block Bh at the columns col0 .. col0 + k of an
    ld-wide block that starts `shift` elements behind the guard. Checks the guards, the padding columns and B."""
    import torch
    n, k = Bh.shape
    dtype = Bh.dtype
    ld = k if ld is None else ld
    assert ld >= col0 + k
    word = word_of(dtype)
    lo = GUARD + shift
    total = lo + n * ld + GUARD
    hb = np.full(total, SENTINEL, dtype)
    hb[lo:lo + n * ld] = np.array([0x7ff8000000000051], np.uint64).view(np.float64)[0] if dtype == np.float64 else \
        np.array([0x7fc00051], np.uint32).view(np.float32)[0]
    hb[lo:lo + n * ld].reshape(n, ld)[:, col0:col0 + k] = Bh
    hx = np.full(total, SENTINEL, dtype)
    hx[lo:lo + n * ld].reshape(n, ld)[:, col0:col0 + k] = np.nan
    written = np.zeros(total, bool)
    written[lo:lo + n * ld].reshape(n, ld)[:, col0:col0 + k] = True
    tb = torch.from_numpy(hb.copy()).to("cuda")
    tx = tb if in_place else torch.from_numpy(hx.copy()).to("cuda")
    off = (lo + col0) * tb.element_size()
    if solve is None:
        T.solve_sweeps_multi_device(k, tb.data_ptr() + off, ld, tx.data_ptr() + off, ld, sweeps)
    else:
        solve(k, tb.data_ptr() + off, ld, tx.data_ptr() + off, ld)
    torch.cuda.synchronize()
    got = tx.cpu().numpy()
    before = hb if in_place else hx
    assert got[~written].view(word).tobytes() == before[~written].view(word).tobytes(), "a guard or a padding column of X was overwritten"
    if not in_place:
        assert tb.cpu().numpy().view(word).tobytes() == hb.view(word).tobytes(), "B, its padding or its guards were modified"
    return np.ascontiguousarray(got[lo:lo + n * ld].reshape(n, ld)[:, col0:col0 + k])


MULTI = [("prescribed", None), ("dag", 100), ("padding", None)]


@pytest.mark.parametrize("dtype", DTYPES, ids=("f64", "f32"))
@pytest.mark.parametrize("uplo,side", SIDES, ids=("lower", "upper"))
@pytest.mark.parametrize("name,B", MULTI, ids=[f"{a}-{b}" for a, b in MULTI])
def test_every_column_has_the_bits_of_the_single_sweep_solve(eng, name, B, uplo, side, dtype):
    """k in (1, 2, 3, 5, 8, 11) = chunks 1 / 2 / 2+1 / 4+1 / 8 / 8+2+1: every KC runs. ld = k on an aligned base (vector rows),
    ld = k + 3 one element off alignment (scalar rows), the columns 3 .. 3 + k of a 16-wide block, in place with equal ld. UNIT runs
    on the upper side."""
    unit = uplo == UPPER
    A = tc.matrix(name, uplo)
    n = A[3]
    T = eng.TriangularSolve(*A, uplo=side, diag="unit" if unit else "stored", dtype=dtype, block_rows=B)
    levels = sc.depth(name, uplo, B)
    M = A if B is None else bc.filtered(*A, B)
    rhs = block(n, dtype)
    for s in (1, 2, 3, levels):
        want = np.stack([sc.reference(*M, uplo, unit, np.ascontiguousarray(rhs[:, j]), dtype, s) for j in range(KMAX)], axis=1)
        assert np.all(np.isfinite(want))
        singles = [sweep_device(T, np.ascontiguousarray(rhs[:, j]), s) for j in range(KMAX)]
        runs = [(k, {}) for k in KS] + [(k, dict(ld=k + 3, shift=1)) for k in (1, 3, 11)] + [(k, dict(ld=16, col0=3)) for k in (2, 8)] + \
            [(k, dict(in_place=True)) for k in (5, 11)] + [(11, dict(ld=14, shift=1, in_place=True))]
        for k, how in runs if s in (2, 3) else runs[::3]:
            got = sweep_multi(T, rhs[:, :k], s, **how)
            for j in range(k):
                assert same_bits(got[:, j], want[:, j]), f"{name} B={B} {s} sweeps, k = {k} {how}: column {j} against the restatement: " \
                    f"{int(np.sum(got[:, j] != want[:, j]))} of {n} rows differ"
                assert same_bits(got[:, j], singles[j]), f"{name} B={B} {s} sweeps, k = {k} {how}: column {j} against the single sweep solve"
        assert same_bits(T.solve_sweeps_multi(rhs[:, :5], s), want[:, :5]), "the host form"
    # the scratch grew to the widest chunk, 8 columns
    assert T.sweeps_info(11) == dict(sweeps=0, effective=0, launches=0,
                                     bytes=4.0 * (slices_of(A[0], A[1], n, uplo, B) + 1) + 2 * n * 8 * np.dtype(dtype).itemsize)
    T.close()


# ---- set_sweeps routes the solve entries --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=("f64", "f32"))
@pytest.mark.parametrize("B", (None, 100), ids=("global", "blocked"))
def test_set_sweeps_routes_the_solve_entries_and_zero_restores_the_exact_plan(eng, B, dtype):
    import torch
    A = tc.matrix("stencil", LOWER)
    n = A[3]
    T = eng.TriangularSolve(*A, dtype=dtype, block_rows=B)
    levels = sc.depth("stencil", LOWER, B)
    info, plan, footprint = T.info, T.solve_multi_plan(3), eng.lib().spmv_mi355x_trsv_mem_footprint(T.h)
    b, rhs = sc.rhs(n, dtype), np.ascontiguousarray(block(n, dtype)[:, :3])
    M = A if B is None else bc.filtered(*A, B)
    exact = tc.reference(*M, LOWER, False, b, dtype)
    exact3 = np.stack([tc.reference(*M, LOWER, False, np.ascontiguousarray(rhs[:, j]), dtype) for j in range(3)], axis=1)
    swept = expected("stencil", B, LOWER, False, dtype, 3)
    swept3 = np.stack([sc.reference(*M, LOWER, False, np.ascontiguousarray(rhs[:, j]), dtype, 3) for j in range(3)], axis=1)
    assert not same_bits(swept, exact) and same_bits(T.solve_sweeps(b, 3), swept)

    def timed(bp, xp):
        assert T.time_device(bp, xp, 2) > 0

    for setting, want, want3 in ((3, swept, swept3), (0, exact, exact3), (levels + 7, exact, exact3), (3, swept, swept3), (0, exact, exact3)):
        T.set_sweeps(setting)
        assert T.sweeps == setting and T.sweeps_info(3)["effective"] == min(setting, levels)
        assert T.sweeps_info(3)["launches"] == 2 * min(setting, levels)
        assert same_bits(T.solve(b), want), f"solve under set_sweeps({setting})"
        assert same_bits(sweep_device(T, b, None, solve=T.solve_device), want), f"solve_device under set_sweeps({setting})"
        assert same_bits(sweep_device(T, b, None, in_place=True, solve=T.solve_device), want), f"solve_device in place under set_sweeps({setting})"
        assert same_bits(sweep_device(T, b, None, solve=timed), want), f"time_device under set_sweeps({setting})"
        assert same_bits(T.solve_multi(rhs), want3), f"solve_multi under set_sweeps({setting})"
        assert same_bits(sweep_multi(T, rhs, None, ld=5, shift=1, solve=T.solve_multi_device), want3), f"solve_multi_device under set_sweeps({setting})"
        tb = torch.from_numpy(np.array(rhs)).to("cuda")
        tx = torch.full_like(tb, float("nan"))
        assert T.time_multi_device(3, tb.data_ptr(), 3, tx.data_ptr(), 3, 2) > 0 and same_bits(tx.cpu().numpy(), want3)
        # an explicit count is not the setting's business
        assert same_bits(T.solve_sweeps(b, 2), expected("stencil", B, LOWER, False, dtype, 2))
        assert T.info == info and T.solve_multi_plan(3) == plan and eng.lib().spmv_mi355x_trsv_mem_footprint(T.h) == footprint
    T.close()


# ---- determinism, update_values --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B", (None, 64), ids=("global", "blocked"))
def test_twice_the_same_bytes_and_new_values_after_update_values(eng, B):
    rp, ci, va, n = tc.matrix("prescribed", UPPER)
    T = eng.TriangularSolve(rp, ci, va, n, uplo="upper", block_rows=B)
    b = sc.rhs(n, np.float64)
    a, c = sweep_device(T, b, 4), sweep_device(T, b, 4)
    assert same_bits(a, c) and same_bits(a, expected("prescribed", B, UPPER, False, np.float64, 4))
    rows = np.repeat(np.arange(n), np.diff(rp))
    new = va * np.where(ci == rows, 1.25, -0.75)                              # still dominant: |off-diagonals| shrink, diagonals grow
    T.update_values_prepare(rp, ci)
    T.update_values(new)
    M = (rp, ci, new, n) if B is None else bc.filtered(rp, ci, new, n, B)
    for s in (1, 4, sc.depth("prescribed", UPPER, B)):
        want = sc.reference(*M, UPPER, False, b, np.float64, s)
        assert np.all(np.isfinite(want)) and not same_bits(want, expected("prescribed", B, UPPER, False, np.float64, s))
        assert same_bits(sweep_device(T, b, s), want), f"{s} sweeps on the new values"
    T.close()


# ---- the solvers ------------------------------------------------------------------------------------------------------------------------------

def swept_precond(eng, P, kind, dtype, sweeps):
    rp, ci, va = P.csr
    if kind == "sgs":
        return eng.sgs_precond(rp, ci, va, P.n, dtype=dtype, sweeps=sweeps)
    _, lo, up = P.ic0()
    T = eng.TriangularSolve
    return T(*lo, P.n, uplo="lower", dtype=dtype, sweeps=sweeps), None, T(*up, P.n, uplo="upper", dtype=dtype, sweeps=sweeps)


def close(M):
    for h in M or ():
        if h is not None and not isinstance(h, np.ndarray):
            h.close()


@pytest.mark.parametrize("sweeps", (1, 2, 4))
@pytest.mark.parametrize("kind", ("sgs", "ic0"))
def test_pcg_tri_under_a_swept_triple_against_the_restatement(eng, kind, sweeps):
    """stop 1, the restatement's iteration count, and test_gpu_pcg_tri.py's bounds for its preconditioned kinds: the explicit norms,
    rnorm <= 10 tol |b|, |x - x*| <= KAPPA 10 tol |x*|, the history on the qualifying rows"""
    P = pc.problem()
    want = P.solve()
    for dtype, lim in pc.PREC.items():
        name = np.dtype(dtype).name
        _, ref, ref_stop = sc.cg_restatement(dtype, kind, sweeps)
        assert ref_stop == 1 and ref.size == sc.COUNTS[dtype][kind][sweeps]
        bn = np.linalg.norm(P.b.astype(dtype).astype(np.float64))
        rows = np.nonzero(ref / bn > lim["ratio"])[0]
        assert rows[-1] == rows.size - 1 and rows.size >= lim["share"] * ref.size
        M = swept_precond(eng, P, kind, dtype, sweeps)
        assert M[0].sweeps == sweeps == M[2].sweeps and M[0].sweeps_info()["launches"] == sweeps
        A = eng.Matrix(*P.csr, P.n, P.n, "sell_c_sigma", dtype)
        what = f"spd_grid(45) {name} swept {kind}, {sweeps} sweeps"
        got = A.pcg_tri(P.b.astype(dtype), precond=M, tol=lim["tol"], max_iterations=pc.MAX_ITERATIONS)
        A.close()
        close(M)
        k = got["iterations"]
        print(f"[trsv_sweeps] {what}: {k} iterations (the restatement {ref.size}), stop {got['stop']}, rnorm {got['rnorm']:.3g}")
        for key, v in pc.shares_of_the_bounds(P, got, dtype, want).items():
            print(f"[trsv_sweeps] {what}: {key} is {v:.3g} of its bound")
        d = np.abs(got["history"][rows[rows < k]] - ref[rows[rows < k]]) / ref[rows[rows < k]]
        print(f"[trsv_sweeps] {what}: largest history deviation {d.max():.3g} on {rows.size} rows")
        assert got["stop"] == 1, f"{what}: stop {got['stop']} after {k} iterations"
        assert k == ref.size, f"{what}: {k} iterations, the restatement {ref.size}"
        assert got["prnorm"] == got["history"][-1] and got["prnorm"] <= lim["tol"] * got["rnorm0"] * (1 + 1e-12), what
        for key, v in pc.shares_of_the_bounds(P, got, dtype, want).items():
            assert v <= 1, f"{what}: {key} is {v:.3g} times its bound"
        assert d.max() <= lim["hist"], f"{what}: history deviates by {d.max():.3g} at row {np.argmax(d)}"


@pytest.mark.parametrize("dtype", DTYPES, ids=("f64", "f32"))
def test_pcg_trsm_multi_under_a_swept_triple_is_pcg_tri_column_by_column(eng, dtype):
    P = pc.problem()
    lim = pc.PREC[dtype]
    rng = np.random.default_rng(3)
    B = np.ascontiguousarray(np.stack([P.b, rng.uniform(-1, 1, P.n), 10 * rng.uniform(-1, 1, P.n)], axis=1).astype(dtype))
    A = eng.Matrix(*P.csr, P.n, P.n, "sell_c_sigma", dtype)
    for kind, sweeps in (("sgs", 2), ("ic0", 3)):
        M = swept_precond(eng, P, kind, dtype, sweeps)
        multi = A.pcg_trsm_multi(B, precond=M, tol=lim["tol"], max_iterations=pc.MAX_ITERATIONS)
        for j in range(3):
            one = A.pcg_tri(np.ascontiguousarray(B[:, j]), precond=M, tol=lim["tol"], max_iterations=pc.MAX_ITERATIONS)
            assert one["stop"] == 1 == multi[j]["stop"] and one["iterations"] == multi[j]["iterations"], (kind, j)
            assert same_bits(one["x"], multi[j]["x"]) and same_bits(one["history"], multi[j]["history"]), (kind, j)
            for f in ("rnorm", "rnorm0", "prnorm", "xnorm"):
                assert one[f] == multi[j][f], (kind, j, f)
        assert multi[0]["iterations"] == sc.cg_restatement(dtype, kind, sweeps)[1].size, kind      # column 0 is the problem's b
        close(M)
    A.close()


def test_gmres_under_the_swept_ilu0_against_the_restatement(eng):
    """convdiff(45), restart 20, ilu0_precond(sweeps=3): test_gpu_gmres_tri.py's restatement with "M v" = U~^-1 (L~^-1 v), three sweeps
    each over the reference ILU(0) factor, and that file's bounds"""
    import test_gpu_gmres_tri as gt
    P = gt.problem()
    rp, ci, va = P.csr
    f, _ = ic.reference(rp, ci, va, P.n)
    assert np.all(np.isfinite(f)) and np.all(f[ci == np.repeat(np.arange(P.n), np.diff(rp))] > 0)
    F = (rp, ci, f, P.n)
    for dtype, lim in gt.PREC.items():
        name = np.dtype(dtype).name
        Mv = lambda v: sc.reference(*F, UPPER, False, sc.reference(*F, LOWER, True, v, dtype, 3), dtype, 3)
        _, ref, ref_stop, ref_restarts = gt.restate(P.dense(dtype), P.b, 20, Mv, lim["tol"], gt.MAX_ITERATIONS, dtype)
        assert ref_stop == 1
        bn = np.linalg.norm(P.b.astype(dtype).astype(np.float64))
        rows = np.nonzero(ref / bn > lim["ratio"])[0]
        assert rows[-1] == rows.size - 1 and rows.size >= lim["share"] * ref.size
        M = eng.ilu0_precond(rp, ci, va, P.n, dtype=dtype, sweeps=3)
        assert M[0].sweeps == 3 == M[2].sweeps and M[0].block_info()["block_rows"] == 0
        A = P.handle(eng, "sell_c_sigma", dtype)
        what = f"convdiff(45) {name} restart=20 swept ILU(0), 3 sweeps"
        got = A.gmres(P.b.astype(dtype), restart=20, precond=M, tol=lim["tol"], max_iterations=gt.MAX_ITERATIONS)
        A.close()
        gt.close(*M)
        k = got["iterations"]
        print(f"[trsv_sweeps] {what}: {k} iterations (the restatement {ref.size}), stop {got['stop']}, rnorm {got['rnorm']:.3g}")
        for key, v in gt.shares_of_the_bounds(P, got, dtype).items():
            print(f"[trsv_sweeps] {what}: {key} is {v:.3g} of its bound")
        assert got["stop"] == 1, f"{what}: stop {got['stop']} after {k} iterations"
        for key, v in gt.shares_of_the_bounds(P, got, dtype).items():
            assert v <= 1, f"{what}: {key} is {v:.3g} times its bound"
        assert abs(k - ref.size) <= 1 and k >= rows.size, f"{what}: {k} iterations, the restatement {ref.size}"
        assert got["restarts"] == (ref_restarts if k == ref.size else (k - 1) // 20), what
        d = np.abs(got["history"][rows] - ref[rows]) / ref[rows]
        print(f"[trsv_sweeps] {what}: largest history deviation {d.max():.3g} on {rows.size} rows")
        assert d.max() <= lim["hist"], f"{what}: history deviates by {d.max():.3g} at row {np.argmax(d)}"
