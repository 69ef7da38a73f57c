"""Multi-RHS solvers (spmv_mi355x_pcg_multi / spmv_mi355x_pbicgstab_multi, Matrix.pcg_multi / pbicgstab_multi) on the GPU.

The contract is exact: on a handle whose SpMV is deterministic, column j of a multi-RHS solve returns bit for bit what the
single-RHS solver returns for b_j on the same handle (x, history, iterations, error, error_best, eps, eps_counter,
restarts). Both run the same kernels (csrc/solvers.hip), so what the comparison checks is a column inside a chunk of
KC in {8, 4, 2} columns against the same column alone in the KC = 1 instantiation, and the SpMM against the SpMV. The
independent reference is the oracle: test_solvers.py compares the single solvers with it, and here the other layouts are
compared with it to the tolerances of test_solvers.py. The systems are those of test_solvers.py.
"""
import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as sla

from test_solvers import HIST_ROWS, SYSTEMS, near_singular_neumann, rhs, laplace2d

pytestmark = pytest.mark.gpu

FIELDS = ("iterations", "error", "error_best", "eps", "eps_counter", "restarts")
KMAX = 9

DETERMINISTIC_LAYOUTS = [
    ("csr_scalar", {}),
    ("csr_vector", {}),
    ("sell_c_sigma", {"sell_window": 2}),
    ("sell_c_sigma", {"sell_values": 1}),
]
LAYOUT_IDS = [f + "".join(f":{k}={v}" for k, v in o.items()) for f, o in DETERMINISTIC_LAYOUTS]


@pytest.fixture(scope="module")
def eng():
    import spmv_mi355x as eng
    assert eng.device_count() >= 1, "no GPU visible: the -m gpu tests need an MI355X"
    return eng


def _matrix(eng, A, fmt, dtype=np.float64, **opts):
    return eng.Matrix(A.indptr, A.indices, A.data, A.shape[0], A.shape[1], fmt, dtype, **opts)


def _fast_column(A):
    """b = K v for a generalized eigenvector A v = lambda K v (K = diag A): Jacobi-preconditioned CG is done after one step"""
    K = sp.diags(A.diagonal())
    _, V = sla.eigsh(A, k=1, M=K, which="LM")
    b = K @ V[:, 0]
    return b / np.abs(b).max()


def _columns(A, dtype):
    """KMAX right-hand sides; column 1 breaks after a couple of iterations, the others after many"""
    cols = [rhs(A, 11), _fast_column(A)] + [rhs(A, 12 + j) for j in range(KMAX - 2)]
    return np.ascontiguousarray(np.stack(cols, axis=1), dtype)


def _is_deterministic(M, n):
    x = np.random.default_rng(5).uniform(-1, 1, n)
    return np.array_equal(M.spmv(x), M.spmv(x))


def _bits_equal(a, b):
    """same shape, dtype, NaN positions, and bits everywhere else. Once a BiCGSTAB column has converged it divides 0/0 (as
    the reference does): which NaN comes out of an operation on two NaNs (sign, payload) is not part of the contract."""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and a[~na].tobytes() == b[~nb].tobytes()


def _assert_same(got, want, what):
    for f in FIELDS:
        assert got[f] == want[f], f"{what}: {f} {got[f]!r} != {want[f]!r}"
    assert _bits_equal(got["x"], want["x"]), f"{what}: x differs"
    if want["history"] is not None:
        assert _bits_equal(got["history"], want["history"]), f"{what}: history differs"


def _singles(M, A, B, method, iters):
    solve = M.pcg if method == "pcg" else M.pbicgstab
    return [solve(A.indptr, A.indices, A.data, B[:, j].copy(), iters) for j in range(B.shape[1])]


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("fmt,opts", DETERMINISTIC_LAYOUTS, ids=LAYOUT_IDS)
@pytest.mark.parametrize("name", ["laplace2d_40", "random_spd_2000"])
def test_pcg_multi_bit_identical_per_column(eng, name, fmt, opts, dtype):
    A = SYSTEMS[name]()
    M = _matrix(eng, A, fmt, dtype, **opts)
    assert _is_deterministic(M, A.shape[1]), f"{M.format_name}: the single SpMV is expected to be deterministic here"
    B = _columns(A, dtype)
    want = _singles(M, A, B, "pcg", 1000)
    its = [w["iterations"] for w in want]
    assert all(i > 0 for i in its), its
    if name == "laplace2d_40" and dtype == np.float64:
        # a frozen column sits through many iterations of the others (more than the host's polling lag of 2 * 32)
        assert max(its) - min(its) > 64, its
    for k in (1, 3, 4, 8, 9):
        got = M.pcg_multi(A.indptr, A.indices, A.data, B[:, :k], 1000)
        assert len(got) == k
        for j in range(k):
            _assert_same(got[j], want[j], f"{M.format_name} k={k} column {j}")
        # launches: the single solver's count for the latest-breaking column (test_gpu_pcg_matches_oracle)
        last = max(its[:k])
        base = 1 + last + (last - 1) // 100 + 1
        assert base <= got[0]["spmv_calls"] <= base + 3 * 32 + 1
        assert all(g["spmv_calls"] == got[0]["spmv_calls"] and g["seconds"] == got[0]["seconds"] for g in got)
    M.close()


@pytest.mark.parametrize("fmt,opts", DETERMINISTIC_LAYOUTS, ids=LAYOUT_IDS)
@pytest.mark.parametrize("name", ["nonsym_dd_1500", "laplace2d_40"])
def test_pbicgstab_multi_bit_identical_per_column(eng, name, fmt, opts):
    A = SYSTEMS[name]()
    M = _matrix(eng, A, fmt)
    assert _is_deterministic(M, A.shape[1])
    iters = 230
    B = _columns(A, np.float64)[:, :5]
    want = _singles(M, A, B, "pbicgstab", iters)
    for k in (1, 4, 5):
        got = M.pbicgstab_multi(A.indptr, A.indices, A.data, B[:, :k], iters)
        for j in range(k):
            assert got[j]["iterations"] == iters
            _assert_same(got[j], want[j], f"{M.format_name} k={k} column {j}")
        assert got[0]["spmv_calls"] == 1 + 2 * iters + (iters - 1) // 100 + 1
    M.close()


def test_pcg_multi_restart_column_replays_exactly(eng):
    A, b = near_singular_neumann()
    B = np.ascontiguousarray(np.stack([rhs(A, 21), b, rhs(A, 22)], axis=1))
    M = _matrix(eng, A, "csr_scalar")
    want = _singles(M, A, B, "pcg", 1000)
    assert want[1]["restarts"] >= 1
    got = M.pcg_multi(A.indptr, A.indices, A.data, B, 1000)
    assert got[1]["restarts"] >= 1
    for j in range(3):
        _assert_same(got[j], want[j], f"neumann column {j}")
    M.close()


@pytest.mark.parametrize("fmt", ["csr_stream", "csr_merge", "coo", "sell_c_sigma"])
@pytest.mark.parametrize("name", ["laplace2d_40", "random_spd_2000"])
def test_pcg_multi_other_layouts_match_oracle(eng, oracle, name, fmt):
    A = SYSTEMS[name]()
    # test_gpu_pcg_matches_oracle's tolerances hold for its own b; power-of-two multiples of it keep them exactly
    B = np.ascontiguousarray(np.stack([rhs(A) * s for s in (1.0, 0.5, 2.0, 4.0)], axis=1))
    M = _matrix(eng, A, fmt)
    got = M.pcg_multi(A.indptr, A.indices, A.data, B, 1000)
    for j in range(B.shape[1]):
        b = B[:, j]
        want = oracle.pcg(A.indptr, A.indices, A.data, b, 1000)
        g = got[j]
        assert abs(g["iterations"] - want["iterations"]) <= 2
        assert g["eps"] == pytest.approx(want["eps"], rel=1e-13)
        assert g["eps_counter"] == pytest.approx(want["eps_counter"], rel=1e-13)
        assert g["restarts"] == want["restarts"] == 0
        n = min(HIST_ROWS, g["iterations"], want["iterations"])
        np.testing.assert_allclose(g["history"][:n], want["history"][:n], rtol=1e-9)
        assert g["history"].shape == (g["iterations"], 3)
        assert np.linalg.norm(g["x"] - want["x"]) <= 1e-9 * np.linalg.norm(want["x"])
        true_err = np.linalg.norm(b - A @ g["x"])
        assert g["error"] == pytest.approx(true_err, rel=1e-3, abs=1e-13 * np.linalg.norm(b))
        assert g["error"] == g["error_best"]
    M.close()


def test_pcg_multi_respects_max_iterations(eng):
    A = SYSTEMS["laplace2d_40"]()
    M = _matrix(eng, A, "csr_vector")
    B = _columns(A, np.float64)[:, [0, 2, 3]]
    for iters in (0, 1, 7, 33, 100, 101):
        want = _singles(M, A, B, "pcg", iters)
        got = M.pcg_multi(A.indptr, A.indices, A.data, B, iters)
        for j in range(3):
            assert got[j]["iterations"] == want[j]["iterations"] == iters
            assert np.array_equal(got[j]["x"], want[j]["x"])
            assert got[j]["error_best"] == want[j]["error_best"]
            assert got[j]["history"].shape == (iters, 3)
    M.close()


def test_pcg_multi_error_paths_and_info_stride(eng):
    import ctypes
    A = laplace2d(5).tolil()
    A[3, 3] = 0
    A = A.tocsr()
    A.eliminate_zeros()
    M = _matrix(eng, A, "csr_vector")
    for solve in (M.pcg_multi, M.pbicgstab_multi):
        with pytest.raises(eng.SpmvError, match="zero in diagonal"):
            solve(A.indptr, A.indices, A.data, np.ones((25, 2)), 10)
    R = sp.random(6, 9, 0.5, random_state=0, format="csr")
    MR = _matrix(eng, R, "csr_vector")
    with pytest.raises(eng.SpmvError, match="pcg_multi: the matrix must be square"):
        MR.pcg_multi(R.indptr, R.indices, R.data, np.ones((6, 2)), 10)
    # k = 0 on a real handle: rc 1 before the device is touched, buffers untouched
    G = SYSTEMS["laplace2d_40"]()
    MG = _matrix(eng, G, "csr_vector")
    lib = eng.lib()
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    rp, ci, va = (np.ascontiguousarray(a) for a in (G.indptr.astype(np.int32), G.indices.astype(np.int32), G.data))
    B = np.ones((G.shape[0], 2))
    X = np.full((G.shape[0], 2), -7.25)
    assert lib.spmv_mi355x_pcg_multi(MG.h, ctypes.c_int(0), p(rp), p(ci), p(va), p(B), p(X), ctypes.c_long(10), None, None) == 1
    assert b"pcg_multi: k must be >= 1" in lib.spmv_mi355x_last_error()
    assert np.all(X == -7.25)
    # a larger caller struct_size is the array stride; each element is written with the size it can hold
    big = ctypes.sizeof(eng.SolverInfo) + 24
    raw = (ctypes.c_ubyte * (2 * big))(*([0xAB] * (2 * big)))
    ctypes.cast(raw, ctypes.POINTER(ctypes.c_uint))[0] = big
    assert lib.spmv_mi355x_pcg_multi(MG.h, ctypes.c_int(2), p(rp), p(ci), p(va), p(B), p(X), ctypes.c_long(400), None, raw) == 0
    want = MG.pcg(G.indptr, G.indices, G.data, B[:, 0].copy(), 400)
    for j in range(2):
        el = eng.SolverInfo.from_buffer(raw, j * big)
        assert el.struct_size == ctypes.sizeof(eng.SolverInfo)
        assert el.iterations == want["iterations"] and el.error_best == want["error_best"]
        assert bytes(raw[j * big + ctypes.sizeof(eng.SolverInfo):(j + 1) * big]) == b"\xab" * 24
    assert np.array_equal(X[:, 0], want["x"]) and np.array_equal(X[:, 1], want["x"])
    for h in (M, MR, MG):
        h.close()
