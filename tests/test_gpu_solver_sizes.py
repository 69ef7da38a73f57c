"""Every Krylov solver at the sizes where csrc/solvers_common.hpp changes its path: the launch shape solver_blocks(len) =
min(MAX_PART, ceil(len / 1024)) blocks of VB = 256 threads, GRID_STRIDE, and the second stage of the dot products
(sum_partials, sum_partials_n, gmres_reduce_kernel: `for (i = threadIdx.x; i < nb; i += VB)` over the nb per-block partials).
The other solver test files stop at 3000 unknowns, nb <= 3.

Sizes (solver_size_cases.py; the restated solver_blocks is asserted in test_solver_size_cases.py and below).
Which element goes into which partial: GRID_STRIDE gives thread t = blockIdx.x * VB + threadIdx.x of the grid the elements t,
t + nb * VB, ...: elements are dealt to the blocks VB at a time, round and round, and element i lands in partial
(i % (nb * VB)) / VB (solver_size_cases.block_of), never in partial i / 1024. The "tail rows" below are derived from that mapping
(solver_size_cases.tail_rows; asserted in test_solver_size_cases.py).

  name          unknowns                  nb    what it reaches, and its tail rows
  N1            262 145 = 256 * 1024 + 1  257   the partial loop's second trip: thread 0 alone picks up a second partial, number 256.
                                                Block 256 owns the 768 rows 65 536 .., 131 328 .., 197 120 .. (256 each, trips 1 - 3):
                                                the tail rows. Row 262 144, the one row of the 4th trip, is block 253's.
  N2            1 049 601 = 1025*1024 + 1 1024  nb capped (ceil(len / 1024) = 1026), the partial loop takes 4 trips, the grid stride a
                                                5th: the 1025 rows 1 048 576 .. of blocks 0 - 3 and thread 0 of block 4: the tail rows
  CGLS tall     262 145 x 1025            257   one grid for both lengths: the 1025 short elements are blocks 0 - 3 and thread 0 of
  CGLS wide     1025 x 262 145            257   block 4, the other 252 blocks must store a zero partial for the short vectors. Tail
                                                rows: N1's on the long side (b when tall, x when wide), none on the short side
  distributed   530 000 on 2 ranks        259   each: both row blocks have 265 000 rows > 262 144, reduce_slots_kernel sums nb > VB
                                                partials before the all-reduce. Tail rows: per rank the 2856 rows of its partials
                                                256 - 258 in its own grid

Matrices (at most 5 entries per row, far = 131 071): spd(n) = diagonal 4, -1 at +-1, -0.5 at +-far; stiff(n) = tridiagonal 2.05, -1;
nsym(n) = diagonal 4, -1.5 below, -0.5 above, -0.7 at +far, -0.2 at -far; CGLS: test_gpu_cgls.Problem's construction in sparse form.
Right-hand side: default_rng(seed).uniform(0.5, 1.5, n), then the tail rows scaled to hold exactly half of |b|^2: a lost partial
256 or a skipped 5th trip moves |b| by 30 %, and test_solver_size_cases.py shows that the references with a dot product that
loses exactly those rows break the history bounds below by more than a factor 100, in both precisions (and the fp64 x bounds; the
fp32 x bounds of PCG and MINRES are too wide for that, and GMRES converges to the same x whatever rows its dots lose). The wide
CGLS shape has b on the short side: no tail rows, b as drawn. There the tail rows of the long vectors (s, p, x) carry their natural
0.3 % of the squares (5 % of |x|): a lost partial 256 moves |s0| by 1.5e-3, far above the fp64 bound of 1e-6 and 1.5 times the
fp32 bound of 1e-3; the matrix is prescribed and b has only 1025 entries to steer 262 145 with.

References, none of them the engine: oracle.pcg / oracle.pbicgstab, and the numpy restatements of test_gpu_minres.py,
test_gpu_gmres.py and test_gpu_cgls.py on the scipy.sparse matrix (they only take A @ v). No dense solve exists at these sizes: the
converged restatement stands in for it. Every bound is the one of the solver's own test file. Beside each, the largest distance
between two summation orders of the reference itself at these sizes (the reference on a symmetric random permutation of the
system, solver_size_cases.permuted; for CGLS rows and columns permuted independently), measured on the CPU; each is at most a
tenth of its bound (asserted at N1 in test_solver_size_cases.py):

  PCG (test_solvers.py)      first 20 history rows 1e-9: 4.3e-13 (spd(N1), 9 right-hand sides), 1.6e-13 (spd(N2)), 1.3e-13 (stiff(N1)),
                             7.0e-14 (spd(530 000)); iterations +-2: 33/33, 41/41, 154/154, 39/39; x and x on the tail rows 1e-9: 5.3e-16.
                             fp32 (test_gpu_pcg_fp32): iterations +-4, x 2e-4, history[:5, 0] 1e-4.
    history[100, 1]          stiff(N1), the explicit residual at iteration 100, is 1.5e-10 |b|: a difference of terms 1e10 times larger.
                             The two orders differ by up to 4.5e-6 of it (6.6e-16 |b|, 3 permutations), so 1e-9 relative cannot hold on
                             this entry; it is asserted to 1e-9 relative plus test_gpu_gmres.cancellation_floor (the first-order
                             rounding error of two evaluations of |b - A x|, as the explicit norms of the other files are): 4.7e-4 of
                             the entry, 100 times the two orders' distance. The floor is evaluated at the returned x, which differs from
                             x at iteration 100 by 4e-11 |x|: the floor by 4e-16 of itself. What the assertion can see: at iteration 100
                             the tail rows hold 30 % of |r|^2 (the residual of this b keeps its weight there), so partial 256 lost in
                             explicit_fin_kernel moves the entry by 16 %, 350 times the floor. A fault smaller than 4.7e-4 of the entry
                             passes this assertion; history[100, 0], the recurrence residual of the same iteration, is not asserted
                             (rows 20 .. are outside test_solvers.py's comparison).
  BiCGSTAB (test_solvers.py) history rows 1e-7: over the first 20 rows the two orders differ by up to 1.3e-8 (nsym(N2), from row 12 on;
                             5.5e-10 at nsym(N1)): the residual is not monotone and has fallen by 1e-5 by then, the differences of the
                             dot products are amplified. That lacks the factor 10, so the bound is kept and applied to the first
                             BICG_ROWS = 8 rows, where the distance is at most 6.0e-11 (6 systems, 2 permutations each). x 1e-9: 3.4e-16;
                             error_best <= 1e-10 |b|: 1.1e-15 |b|.
  MINRES (test_gpu_minres.py PREC)  qualifying history rows 1e-6 / 1e-3: 3.7e-15 / 9.8e-8; iterations equal (29 .. 39 / 12 .. 17); x
                             4.5e-16 / 1.2e-7.
  GMRES (test_gpu_gmres.py PREC)    qualifying history rows 1e-6 / 1e-3: 6.4e-11 / 1.4e-7; iterations and restarts equal (35 .. 49 with
                             4 and 5 restarts at restart 8, 14 .. 21 in fp32); x 1.1e-16 / 1.2e-7.
  CGLS (test_gpu_cgls.py PREC)      qualifying history rows 1e-6 / 1e-3: 7.4e-11 / 8.4e-7; |s0| 1e-6 / 1e-3: 2.1e-16 / 2.3e-10; iterations
                             equal (7 and 5 in fp64, 3 and 2 in fp32); x 2.0e-16 / 8.8e-8.
  x, and x on the tail rows on its own, of MINRES, GMRES, CGLS against the restatement's: both are within the solver's own x bound of
  the solution (KAPPA * 10 * tol * the norm factor of the minv for MINRES and GMRES, PREC["x"] for CGLS; KAPPA holds by Gershgorin:
  the eigenvalues of spd - shift I lie in [0.7, 7], the singular values of nsym in [1.1, 6.9]), so they differ by at most twice that
  bound of |x|.

Share of the history rows that must qualify for the relative comparison (so that it cannot go empty): at least half of the fp64 rows
and a quarter of the fp32 rows for MINRES and GMRES (the references: 0.62 .. 0.67 and 0.29 .. 0.38). The CGLS matrix has
cond 1.03 and 1.004 at these shapes (256 wrapped diagonals of 4 against 6 entries below 0.5) and converges in 7 / 5 (fp64) and 3 / 2 (fp32)
iterations: 4 of 7 and 1 of 3 rows qualify on the tall shape, 2 of 5 and NONE of 2 on the wide one. These counts are asserted as
they are; on the wide fp32 case the comparison with the restatement rests on |s0|, x and the iteration count, and the norms on numpy:
the history of CGLS is barely tested at these shapes, its dot products are (|s0|, the norms, alpha and beta through x).

What stays unreached: the CG restart branch of explicit_kernel at nb > 256 (the only known trigger, near_singular_neumann, was found
by search at n = 100 and is chaotic by construction); gmres_tri and the blocked triangular solve at these sizes; element offsets
beyond 2^31. Nothing here measures speed."""
import os
import sys

import numpy as np
import pytest

import solver_size_cases as C
import test_gpu_cgls as tc
import test_gpu_gmres as tg
import test_gpu_minres as tm
from conftest import ROOT
from solver_size_cases import GMRES_CASES, LO1, LSQ_DAMPS, LSQ_ROWS, MINRES_CASES, N1, N2, SHARE
from test_gpu_solver_multi import _assert_same, _is_deterministic
from test_solvers import HIST_ROWS

pytestmark = pytest.mark.gpu

LAYOUTS = [("sell_c_sigma", {}), ("csr_vector", {})]
DTYPES = [np.float64, np.float32]
DTYPE_IDS = ["f64", "f32"]
BICG_ROWS = 8                    # of HIST_ROWS: see the docstring
POLL = 32


@pytest.fixture(scope="module")
def eng():
    import spmv_mi355x as eng
    assert eng.device_count() >= 1, "no GPU visible: the -m gpu tests need an MI355X"
    return eng


def test_the_sizes_reach_what_the_docstring_says():
    assert (C.solver_blocks(N1), C.solver_blocks(N2)) == (C.VB + 1, C.MAX_PART) and -(-N2 // C.BLOCK_ROWS) == C.MAX_PART + 2
    assert C.tail_rows(N1).size == 768 and C.tail_rows(N2).size == 1025 and C.tail_rows(C.LSQ_SHORT, 257).size == 0


def _rel(a, b):
    return float(np.linalg.norm(a.astype(np.float64) - b.astype(np.float64)) / np.linalg.norm(b.astype(np.float64)))


def _report(tag, worst):
    print(f"[sizes] {tag}: largest shares of the bounds " + ", ".join(f"{k} {v:.2g}" for k, v in worst.items()))


def _note(worst, key, value, bound):
    worst[key] = max(worst.get(key, 0.0), float(value) / bound)


# ---- 1. PCG against the oracle, 2. past the explicit check ---------------------------------------------------------------------------

def _pcg_fp64_asserts(S, A, b, tail, got, want, worst, what, calls=True):
    """test_solvers.test_gpu_pcg_matches_oracle's assertions, and x on the tail rows on its own (calls: the launch count is the solve's own)"""
    assert abs(got["iterations"] - want["iterations"]) <= 2, f"{what}: {got['iterations']} iterations, the oracle {want['iterations']}"
    assert got["eps"] == pytest.approx(want["eps"], rel=1e-13), what
    assert got["eps_counter"] == pytest.approx(want["eps_counter"], rel=1e-13), what
    assert got["restarts"] == want["restarts"] == 0, what
    k = min(HIST_ROWS, got["iterations"], want["iterations"])
    _note(worst, "history", (np.abs(got["history"][:k] - want["history"][:k]) / np.abs(want["history"][:k])).max(), 1e-9)
    np.testing.assert_allclose(got["history"][:k], want["history"][:k], rtol=1e-9, err_msg=what)
    assert got["history"].shape == (got["iterations"], 3)
    _note(worst, "x", _rel(got["x"], want["x"]), 1e-9)
    _note(worst, "x_tail", _rel(got["x"][tail], want["x"][tail]), 1e-9)
    assert np.linalg.norm(got["x"] - want["x"]) <= 1e-9 * np.linalg.norm(want["x"]), what
    assert np.linalg.norm(got["x"][tail] - want["x"][tail]) <= 1e-9 * np.linalg.norm(want["x"][tail]), f"{what}: x on the tail rows"
    true_err = np.linalg.norm(b - A @ got["x"])
    assert got["error"] == pytest.approx(true_err, rel=1e-3, abs=1e-13 * np.linalg.norm(b)), what
    assert got["error"] == got["error_best"], "same kernels on the same vector: bit-equal"
    base = 1 + got["iterations"] + (got["iterations"] - 1) // 100 + 1
    assert not calls or base <= got["spmv_calls"] <= base + 3 * POLL + 1, what


def _pcg_fp32_asserts(tail, got, want, worst, what):
    """test_solvers.test_gpu_pcg_fp32's assertions, and x on the tail rows on its own"""
    assert got["x"].dtype == np.float32
    assert abs(got["iterations"] - want["iterations"]) <= 4, f"{what}: {got['iterations']} iterations, the oracle {want['iterations']}"
    _note(worst, "x", _rel(got["x"], want["x"]), 2e-4)
    _note(worst, "x_tail", _rel(got["x"][tail], want["x"][tail]), 2e-4)
    _note(worst, "history", (np.abs(got["history"][:5, 0] - want["history"][:5, 0]) / want["history"][:5, 0]).max(), 1e-4)
    assert np.linalg.norm(got["x"] - want["x"]) <= 2e-4 * np.linalg.norm(want["x"]), what
    assert np.linalg.norm(got["x"][tail] - want["x"][tail]) <= 2e-4 * np.linalg.norm(want["x"][tail]), f"{what}: x on the tail rows"
    np.testing.assert_allclose(got["history"][:5, 0], want["history"][:5, 0], rtol=1e-4, err_msg=what)


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("n", [N1, N2])
def test_pcg_matches_the_oracle(eng, oracle, n, dtype):
    S = C.system("spd", n)
    A, lo, worst = S.D, S.tail, {}
    iters = 1000 if dtype == np.float64 else 60
    want = C.oracle_solve(oracle, "pcg", "spd", n, iters, fp32=dtype == np.float32)
    assert 0 < want["iterations"] < 60
    for fmt, opts in LAYOUTS:
        M = S.handle(eng, fmt, dtype, **opts)
        what = f"spd({n}) {M.format_name} {np.dtype(dtype).name}"
        got = M.pcg(A.indptr, A.indices, A.data, S.b.astype(dtype), iters)
        if dtype == np.float64:
            _pcg_fp64_asserts(S, A, S.b, lo, got, want, worst, what)
        else:
            _pcg_fp32_asserts(lo, got, want, worst, what)
        M.close()
    _report(f"pcg spd({n}) {np.dtype(dtype).name}", worst)


def test_pcg_past_the_explicit_check(eng, oracle):
    """stiff(N1): the oracle needs 152 iterations, so explicit_kernel / explicit_fin_kernel run at iteration 100 with nb = 257."""
    S = C.system("stiff", N1)
    A, b, lo, worst = S.D, S.b, S.tail, {}
    want = C.oracle_solve(oracle, "pcg", "stiff", N1, 1000)
    assert 100 < want["iterations"] < 300
    for fmt, opts in LAYOUTS:
        M = S.handle(eng, fmt, np.float64, **opts)
        what = f"stiff({N1}) {M.format_name}"
        got = M.pcg(A.indptr, A.indices, A.data, b, 1000)
        _pcg_fp64_asserts(S, A, b, lo, got, want, worst, what)
        h = got["history"]
        assert got["iterations"] > 101
        for k in range(1, got["iterations"]):
            if k % 100:
                assert h[k, 1] == h[k - 1, 1], f"{what}: the explicit residual changed at iteration {k}"
        bound = 1e-9 * want["history"][100, 1] + tg.cancellation_floor(S, got["x"], np.float64)
        _note(worst, "history[100, 1]", abs(h[100, 1] - want["history"][100, 1]), bound)
        assert abs(h[100, 1] - want["history"][100, 1]) <= bound, f"{what}: {h[100, 1]!r}, the oracle {want['history'][100, 1]!r}"
        assert h[100, 1] < h[99, 1] and h[100, 2] == h[100, 1], what                  # re-evaluated and promoted at 100
        M.close()
    _report(f"pcg stiff({N1})", worst)


# ---- 3. BiCGSTAB against the oracle --------------------------------------------------------------------------------------------------

def _bicg_asserts(b, got, want, iters, worst, what):
    """test_solvers.test_gpu_bicgstab_matches_oracle's assertions, the history bound on the first BICG_ROWS rows"""
    assert got["iterations"] == want["iterations"] == iters, what
    _note(worst, "history", (np.abs(got["history"][:BICG_ROWS] - want["history"][:BICG_ROWS]) / want["history"][:BICG_ROWS]).max(), 1e-7)
    np.testing.assert_allclose(got["history"][:BICG_ROWS], want["history"][:BICG_ROWS], rtol=1e-7, err_msg=what)
    _note(worst, "x", _rel(got["x"], want["x"]), 1e-9)
    assert np.linalg.norm(got["x"] - want["x"]) <= 1e-9 * np.linalg.norm(want["x"]), what
    _note(worst, "error_best", got["error_best"], 1e-10 * np.linalg.norm(b))
    assert got["error_best"] <= 1e-10 * np.linalg.norm(b), what
    assert got["error"] == got["error_best"], what
    assert got["spmv_calls"] == 1 + 2 * iters + (iters - 1) // 100 + 1, what


@pytest.mark.parametrize("n,iters", [(N1, 101), (N2, 30)])
def test_bicgstab_matches_the_oracle(eng, oracle, n, iters):
    S = C.system("nsym", n)
    A, worst = S.D, {}
    want = C.oracle_solve(oracle, "pbicgstab", "nsym", n, iters)
    for fmt, opts in LAYOUTS:
        M = S.handle(eng, fmt, np.float64, **opts)
        got = M.pbicgstab(A.indptr, A.indices, A.data, S.b, iters)
        _bicg_asserts(S.b, got, want, iters, worst, f"nsym({n}) {M.format_name}")
        M.close()
    _report(f"bicgstab nsym({n})", worst)


# ---- 4. multi-RHS: every column against the oracle and, bit for bit, against the single solve ------------------------------------------

@pytest.mark.parametrize("n,k,dtype", [(N1, 3, np.float64), (N1, 9, np.float64), (N1, 3, np.float32), (N1, 9, np.float32),
                                       (N2, 9, np.float64)], ids=["N1-k3-f64", "N1-k9-f64", "N1-k3-f32", "N1-k9-f32", "N2-k9-f64"])
def test_pcg_multi_columns(eng, oracle, n, k, dtype):
    S = C.system("spd", n)
    A, lo, worst = S.D, S.tail, {}
    iters = 1000 if dtype == np.float64 else 60
    B = np.ascontiguousarray(C.columns(n)[:, :k], dtype)
    for fmt, opts in LAYOUTS:
        M = S.handle(eng, fmt, dtype, **opts)
        assert _is_deterministic(M, n), f"{M.format_name}: the single SpMV is expected to be deterministic here"
        got = M.pcg_multi(A.indptr, A.indices, A.data, B, iters)
        assert len(got) == k
        for j in range(k):
            what = f"spd({n}) {M.format_name} {np.dtype(dtype).name} k={k} column {j}"
            want = C.oracle_solve(oracle, "pcg", "spd", n, iters, seed=11 + j, fp32=dtype == np.float32)
            if dtype == np.float64:
                _pcg_fp64_asserts(S, A, B[:, j], lo, got[j], want, worst, what, calls=False)
            else:
                _pcg_fp32_asserts(lo, got[j], want, worst, what)
            single = M.pcg(A.indptr, A.indices, A.data, B[:, j].copy(), iters)
            _assert_same(got[j], single, what)
        last = max(g["iterations"] for g in got)
        base = 1 + last + (last - 1) // 100 + 1
        assert base <= got[0]["spmv_calls"] <= base + 3 * POLL + 1
        M.close()
    _report(f"pcg_multi spd({n}) k={k} {np.dtype(dtype).name}", worst)


def test_pbicgstab_multi_columns(eng, oracle):
    n, k, iters = N1, 5, 30
    S = C.system("nsym", n)
    A, worst = S.D, {}
    B = np.ascontiguousarray(C.columns(n)[:, :k])
    for fmt, opts in LAYOUTS:
        M = S.handle(eng, fmt, np.float64, **opts)
        assert _is_deterministic(M, n)
        got = M.pbicgstab_multi(A.indptr, A.indices, A.data, B, iters)
        for j in range(k):
            what = f"nsym({n}) {M.format_name} k={k} column {j}"
            want = C.oracle_solve(oracle, "pbicgstab", "nsym", n, iters, seed=11 + j)
            _bicg_asserts(B[:, j], got[j], want, iters, worst, what)
            single = M.pbicgstab(A.indptr, A.indices, A.data, B[:, j].copy(), iters)
            _assert_same(got[j], single, what)
        M.close()
    _report(f"pbicgstab_multi nsym({n}) k={k}", worst)


# ---- 5. MINRES, 6. GMRES against the restatements ------------------------------------------------------------------------------------

def _history_asserts(got_hist, ref, scale, dtype, lim, worst, what):
    """the rows of the restatement's history above lim['ratio'] * scale, a leading stretch, to lim['hist']; at least SHARE qualify"""
    rows = np.nonzero(ref / scale > lim["ratio"])[0]
    assert rows.size and rows[-1] == rows.size - 1
    assert rows.size >= SHARE[dtype] * ref.size, f"{what}: {rows.size} of {ref.size} rows qualify"
    assert got_hist.size >= rows.size, what
    d = np.abs(got_hist[rows] - ref[rows]) / ref[rows]
    _note(worst, "history", d.max(), lim["hist"])
    assert d.max() <= lim["hist"], f"{what}: history deviates by {d.max():.3g} at row {np.argmax(d)}"
    return rows


def _x_asserts(S, got_x, ref_x, x_bound, worst, what):
    """x, and x on the tail rows on its own, against the converged restatement's: each is within x_bound |x| of the solution"""
    got_x, ref_x, tail = got_x.astype(np.float64), ref_x.astype(np.float64), S.x_tail
    d = np.linalg.norm(got_x - ref_x) / np.linalg.norm(ref_x)
    dt = np.linalg.norm(got_x[tail] - ref_x[tail]) / np.linalg.norm(ref_x)
    _note(worst, "x", d, 2 * x_bound)
    _note(worst, "x_tail", dt, 2 * x_bound)
    assert d <= 2 * x_bound, f"{what}: x deviates from the restatement's by {d:.3g}"
    assert dt <= 2 * x_bound, f"{what}: x on the tail rows deviates from the restatement's by {dt:.3g} of |x|"
    assert np.linalg.norm(ref_x[tail]) > 0.1 * np.linalg.norm(ref_x)          # the tail weighs in x as it does in b


@pytest.mark.parametrize("shift,given", MINRES_CASES)
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("n", [N1, N2])
def test_minres_against_the_restatement(eng, n, dtype, shift, given):
    S = C.system("spd", n)
    lim, worst = tm.PREC[dtype], {}
    bn = np.linalg.norm(S.b)
    for fmt, opts in LAYOUTS:
        A = S.handle(eng, fmt, dtype, **opts)
        what = f"spd({n}) {A.format_name} {np.dtype(dtype).name} shift={shift} minv={given}"
        x_ref, ref, beta1, ref_stop = C.minres_reference("spd", n, dtype, shift, given, lim["tol"])
        got = A.minres(S.b.astype(dtype), shift=shift, minv=S.pre(given), tol=lim["tol"], max_iterations=300)
        assert got["stop"] == ref_stop == 1, f"{what}: stop {got['stop']} after {got['iterations']} iterations"
        assert abs(got["iterations"] - ref.size) <= 1, f"{what}: {got['iterations']} iterations, the restatement {ref.size}"
        assert got["x"].dtype == dtype and got["history"].shape == (got["iterations"],)
        assert got["prnorm"] == got["history"][-1] and got["prnorm"] <= lim["tol"] * got["prnorm0"], what
        assert got["spmv_calls"] >= got["iterations"] + 1, what
        assert abs(got["prnorm0"] - beta1) <= lim["hist"] * beta1, what
        rows = _history_asserts(got["history"], ref, beta1, dtype, lim, worst, what)
        assert np.all(np.diff(got["history"][rows]) <= 0), f"{what}: phibar increases"
        # the norms against numpy's explicit values of the returned x, as test_gpu_minres.shares_of_the_bounds
        nf = float(np.sqrt(S.minv.max() / S.minv.min())) if given else 1.0
        res_bound = 10 * lim["tol"] * nf * bn
        rn, xn = tm.explicit_norms(S, got["x"], shift)
        floor_r = tm.cancellation_floor(S, got["x"], shift, dtype)
        bt = S.b.astype(dtype).astype(np.float64)
        mt = np.ones(n) if not given else S.minv.astype(dtype)
        b1 = np.sqrt(float(bt @ (mt * bt.astype(dtype)).astype(np.float64)))
        shares = dict(rnorm=got["rnorm"] / res_bound,
                      rnorm_np=abs(got["rnorm"] - rn) / (lim["norms"] * rn + floor_r),
                      xnorm_np=abs(got["xnorm"] - xn) / (lim["norms"] * xn),
                      rnorm0_np=abs(got["rnorm0"] - np.linalg.norm(bt)) / (lim["norms0"] * np.linalg.norm(bt)),
                      prnorm0_np=abs(got["prnorm0"] - b1) / (lim["norms0"] * b1))
        for key, v in shares.items():
            assert v <= 1, f"{what}: {key} is {v:.3g} times its bound"
            _note(worst, key, v, 1.0)
        _x_asserts(S, got["x"], x_ref, tm.KAPPA * res_bound / bn, worst, what)
        A.close()
    _report(f"minres spd({n}) {np.dtype(dtype).name} shift={shift} minv={given}", worst)


@pytest.mark.parametrize("restart,given", GMRES_CASES)
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("n", [N1, N2])
def test_gmres_against_the_restatement(eng, n, dtype, restart, given):
    """restart 8 restarts 4 - 5 times in fp64 (the restart and residual kernels run at nb > 256); restart 20 takes the dot kernel
    through three tiles of 8 basis vectors."""
    S = C.system("nsym", n)
    lim, worst = tg.PREC[dtype], {}
    bn = np.linalg.norm(S.b)
    for fmt, opts in LAYOUTS:
        A = S.handle(eng, fmt, dtype, **opts)
        what = f"nsym({n}) {A.format_name} {np.dtype(dtype).name} restart={restart} minv={given}"
        x_ref, ref, ref_stop, ref_restarts = C.gmres_reference("nsym", n, dtype, restart, given, lim["tol"])
        assert ref_stop == 1 and (dtype != np.float64 or restart != 8 or 3 <= ref_restarts <= 5)
        got = A.gmres(S.b.astype(dtype), restart=restart, minv=S.pre(given), tol=lim["tol"], max_iterations=tg.MAX_ITERATIONS)
        k = got["iterations"]
        assert got["stop"] == 1, f"{what}: stop {got['stop']} after {k} iterations"
        assert got["x"].dtype == dtype and got["x"].shape == (n,) and got["history"].shape == (k,)
        assert got["prnorm"] == got["history"][-1] and got["prnorm"] <= lim["tol"] * got["rnorm0"] * (1 + 1e-12), what
        assert abs(k - ref.size) <= 1, f"{what}: {k} iterations, the restatement {ref.size}"
        assert got["restarts"] == (ref_restarts if k == ref.size else (k - 1) // restart) == (k - 1) // restart, what
        assert k + got["restarts"] + 1 <= got["spmv_calls"] <= k + got["restarts"] + 1 + tg.allowance(restart), what
        _history_asserts(got["history"], ref, np.linalg.norm(S.b.astype(dtype).astype(np.float64)), dtype, lim, worst, what)
        shares = tg.shares_of_the_bounds(S, got, dtype, converged=False)
        shares["rnorm"] = got["rnorm"] / (10 * lim["tol"] * bn)
        for key, v in shares.items():
            assert v <= 1, f"{what}: {key} is {v:.3g} times its bound"
            _note(worst, key, v, 1.0)
        _x_asserts(S, got["x"], x_ref, tg.KAPPA * 10 * lim["tol"], worst, what)
        A.close()
    _report(f"gmres nsym({n}) {np.dtype(dtype).name} restart={restart} minv={given}", worst)


# ---- 7. CGLS: one grid for two lengths -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("shape", [C.LSQ_TALL, C.LSQ_WIDE], ids=["tall", "wide"])
def test_cgls_against_the_restatement(eng, shape, dtype):
    m, n = shape
    S = C.lsq_system(m, n)
    lim, worst = tc.PREC[dtype], {}
    rp, ci, va = S.D.indptr, S.D.indices, S.D.data
    for fmt, opts in LAYOUTS:
        A = eng.Matrix(rp, ci, va, m, n, fmt, dtype, **opts)
        At = eng.Matrix(rp, ci, va, m, n, fmt, dtype, transpose=1, **opts)
        assert (At.m, At.n, At.transposed) == (n, m, 1)
        for damp in LSQ_DAMPS:
            what = f"{m}x{n} {A.format_name} {np.dtype(dtype).name} damp={damp}"
            x_ref, ref, s0 = C.cgls_reference(m, n, dtype, damp, lim["tol"])
            assert 0 < len(ref) < 150
            got = A.cgls(At, S.b.astype(dtype), damp=damp, tol=lim["tol"], max_iterations=200)
            k = got["iterations"]
            assert got["stop"] == 1, f"{what}: stop {got['stop']} after {k} iterations"
            assert got["x"].dtype == dtype and got["x"].shape == (n,) and got["history"].shape == (k, 2)
            assert abs(k - len(ref)) <= 1, f"{what}: {k} iterations, the restatement {len(ref)}"
            assert abs(got["arnorm0"] - s0) <= lim["hist"] * s0, what
            _note(worst, "arnorm0", abs(got["arnorm0"] - s0) / s0, lim["hist"])
            rows = np.nonzero(ref[:, 1] / s0 > lim["ratio"])[0]
            assert rows.size == LSQ_ROWS[(shape, dtype)] and (rows.size == 0 or rows[-1] == rows.size - 1), (what, rows)
            assert k >= rows.size, what
            if rows.size:
                d = np.abs(got["history"][rows] - ref[rows]) / ref[rows]
                _note(worst, "history", d.max(), lim["hist"])
                assert d.max() <= lim["hist"], f"{what}: history deviates by {d.max():.3g} at row {np.argmax(d.max(axis=1))}"
                assert np.all(np.diff(got["history"][rows, 0]) <= 0), f"{what}: |r| increases"
            rn, an, xn = tc.explicit_norms(S, got["x"], damp)
            floor_r, floor_ar = tc.cancellation_floor(S, got["x"], damp, dtype)
            if m > n:
                floor_r = 0.0                                              # inconsistent: |r| is of the order of |b|, no cancellation
            shares = dict(arnorm=got["arnorm"] / got["arnorm0"] / (10 * lim["tol"]),
                          rnorm_np=abs(got["rnorm"] - rn) / (lim["norms"] * rn + floor_r),
                          arnorm_np=abs(got["arnorm"] - an) / (lim["norms"] * an + floor_ar),
                          xnorm_np=abs(got["xnorm"] - xn) / (lim["norms"] * xn))
            for key, v in shares.items():
                assert v <= 1, f"{what}: {key} is {v:.3g} times its bound ({k} iterations, rnorm {got['rnorm']!r} numpy {rn!r} " \
                               f"floor {floor_r:.3g}, arnorm {got['arnorm']!r} numpy {an!r} floor {floor_ar:.3g})"
                _note(worst, key, v, 1.0)
            tail = S.x_tail                                                # the long side's rows of partial 256; none on the short side
            xr = x_ref.astype(np.float64)
            d = np.linalg.norm(got["x"].astype(np.float64) - xr) / np.linalg.norm(xr)
            dt_ = np.linalg.norm(got["x"][tail].astype(np.float64) - xr[tail]) / np.linalg.norm(xr)
            _note(worst, "x", d, 2 * lim["x"])
            _note(worst, "x_tail", dt_, 2 * lim["x"])
            assert d <= 2 * lim["x"], f"{what}: x deviates from the restatement's by {d:.3g}"
            assert (tail.size == 768) == (n > m) and (n < m or np.all(xr[tail] != 0)) and dt_ <= 2 * lim["x"], \
                f"{what}: x on the tail rows deviates by {dt_:.3g} of |x|"
        A.close()
        At.close()
    _report(f"cgls {m}x{n} {np.dtype(dtype).name}", worst)


# ---- 8. distributed PCG: reduce_slots_kernel over nb > VB partials -------------------------------------------------------------------

def _dist_worker(rank, world, port, q):
    for p in (os.path.join(ROOT, "spmv-research_amd", "python"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
        sys.path.insert(0, p)
    import torch
    import torch.distributed as dist
    import spmv_dist as D
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        torch.cuda.set_device(0)
        A = C.system("spd", C.DIST_N).D
        off = D.row_partition(A.indptr, world)
        b = C.dist_rhs(off)
        blk = D.local_block(A.indptr, A.indices, A.data, off, rank)
        S = D.DistributedSolver(dist, torch, blk, off, rank, world, fmt="csr_vector")
        r = S.pcg(b[off[rank]:off[rank + 1]], 1000)
        q.put((rank, r["x"], r["iterations"], r["history"], r["error"], r["error_best"], r["restarts"], dict(S.calls), S.m))
        dist.barrier()
    except Exception:                                             # surface the failure instead of a hung join
        import traceback
        q.put((rank, "ERROR", traceback.format_exc()))
    finally:
        dist.destroy_process_group()


def test_distributed_pcg_matches_single_gpu(eng, oracle):
    """test_gpu_dist_solver's assertions at 265 000 rows per rank: world 2, gloo ranks sharing the one GPU, row partition."""
    import spmv_dist as D
    import torch.multiprocessing as mp
    world, n = C.DIST_WORLD, C.DIST_N
    A = C.system("spd", n).D
    off = D.row_partition(A.indptr, world)
    assert np.all(np.diff(off) > LO1) and all(C.solver_blocks(int(m)) > C.VB for m in np.diff(off)), off
    b = C.dist_rhs(off)
    M = eng.Matrix(A.indptr, A.indices, A.data, n, n, "csr_vector")
    single = M.pcg(A.indptr, A.indices, A.data, b, 1000)
    M.close()
    want = C.oracle_solve(oracle, "pcg", "spd", n, 1000, dist=True)
    assert 0 < want["iterations"] < 60
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_dist_worker, args=(r, world, 29693, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = {}
    for _ in range(world):
        item = q.get(timeout=300)
        assert not (isinstance(item[1], str) and item[1] == "ERROR"), item[2]
        res[item[0]] = item[1:]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    x = np.concatenate([res[r][0] for r in range(world)])
    assert [res[r][7] for r in range(world)] == list(np.diff(off)) and x.shape == (n,)
    its = {res[r][1] for r in range(world)}
    assert len(its) == 1, f"ranks disagree on the iteration count: {its}"
    it = its.pop()
    assert abs(it - single["iterations"]) <= 2 and abs(it - want["iterations"]) <= max(2, 0.1 * want["iterations"])
    for r in range(1, world):                                      # identical scalars on every rank
        np.testing.assert_array_equal(res[r][2], res[0][2])
        assert res[r][3:6] == res[0][3:6]
    k = min(20, it, single["iterations"], want["iterations"])
    worst = {}
    _note(worst, "history_single", (np.abs(res[0][2][:k] - single["history"][:k]) / single["history"][:k]).max(), 1e-9)
    _note(worst, "history", (np.abs(res[0][2][:k] - want["history"][:k]) / want["history"][:k]).max(), 1e-9)
    np.testing.assert_allclose(res[0][2][:k], single["history"][:k], rtol=1e-9)
    np.testing.assert_allclose(res[0][2][:k], want["history"][:k], rtol=1e-9)
    _note(worst, "x_single", _rel(x, single["x"]), 1e-9)
    assert np.linalg.norm(x - single["x"]) <= 1e-9 * np.linalg.norm(single["x"])
    for r, tail in enumerate(C.dist_tail(off)):                    # each rank's rows of its partials 256 .. 258, against the oracle
        _note(worst, "x_tail", _rel(x[tail], want["x"][tail]), 1e-9)
        assert np.linalg.norm(x[tail] - want["x"][tail]) <= 1e-9 * np.linalg.norm(want["x"][tail]), f"rank {r}: x on its tail rows"
    assert np.linalg.norm(b - A @ x) == pytest.approx(res[0][3], rel=1e-3, abs=1e-13 * np.linalg.norm(b))
    calls = res[0][6]
    assert calls["spmv"] >= it + 2 and calls["allreduce"] >= 2 * it + 2
    _report(f"pcg_dist spd({n}) world {world}", worst)
