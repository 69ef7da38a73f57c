"""k right-hand sides through one AMG or FSAI cycle and one tol-based CG, on the GPU (include/spmv_mi355x.h "k right-hand sides ..."):
Amg.apply_multi* / Fsai.apply_multi* / Matrix.pcg_tri_multi against the single-vector calls on the same handles.

The contract is exact: on a handle whose SpMV is deterministic, column j of every k-column call holds the bits of the single call on
column j (shape, dtype and tobytes()). Every test first asserts that the handle's SpMV is deterministic. The vector kernels of the
solve are one KC-templated set (csrc/solver_pcg_tri.hip) and the single call is their k = 1, so what the comparison checks there is
a column inside a chunk of 8, 4 or 2 columns (or behind a full chunk) against the same column in a chunk of one. At k = 1 the
vector kernels are the same code on both sides; what differs is the matrix product and the preconditioner: the SpMM (k = 1) against
the SpMV, apply_multi (k = 1) against the single apply, the Jacobi scale kernel for k columns against tri_precond's. Beyond that:
the cycle's chunked vector kernels against its single-vector ones, the dense solve of a chunk against the single dense solve, and
the freeze of one column against its neighbours' progress.
The single calls themselves, and with them the KC = 1 kernels, are held to the restatements and references by test_gpu_amg.py,
test_gpu_fsai.py, test_gpu_pcg_tri.py and test_gpu_pcg_tri_sizes.py. Every test here needs the _multi entry points.

1. the cycle, column against single: amg_cases.CYCLE_CASES in both precisions (grid on every layout), nu = 2, a filtered hierarchy,
   a near-null vector; Fsai with power 1 and 2.            2. strided blocks, guard rows and NaN padding; in place.
3. the solve, column against single, for none / Jacobi / Fsai / Amg over the layouts, k in (1, 3, 4, 8, 9).
4. the freeze per column (stops 1, 1, 3, 4, 1).             5. max_iterations reached, and max_iterations = 0.
6. path_wrap: the second trip of the row loops.             7. apply_multi_plan.        8. after an update of the values.
9. twice the same bits."""
import numpy as np
import pytest

import amg_cases as ac
import pcg_tri_cases as pc
import pcg_tri_multi_cases as mc
from pcg_tri_cases import MAX_ITERATIONS, POLL, PREC

pytestmark = pytest.mark.gpu

DELTA = dict(sell_c=64, sell_delta=1, sell_sigma=64, sell_window=2)
LAYOUTS = [("sell_c_sigma", {}), ("csr_vector", {}), ("sell_c_sigma", DELTA)]           # test_gpu_amg.py's
LAYOUT_IDS = ["sell", "csr_vector", "sell_delta"]
INFO_FIELDS = ("iterations", "stop", "rnorm", "rnorm0", "prnorm", "xnorm")
DTYPES = [np.float64, np.float32]


@pytest.fixture(scope="module")
def eng():
    import spmv_mi355x as eng
    assert eng.device_count() >= 1, "no GPU visible: the -m gpu tests need an MI355X"
    for sym in ("spmv_mi355x_amg_apply_multi", "spmv_mi355x_pcg_amg_multi"):
        assert hasattr(eng.lib(), sym)
    return eng


def amg(eng, name, dtype=np.float64, fmt="sell_c_sigma", **opts):
    rp, ci, va, n, own = ac.case(name)
    return eng.Amg(rp, ci, va, n, fmt, dtype, **own, **opts)


def handle(eng, fmt, dtype, **opts):
    P = pc.problem()
    rp, ci, va = P.csr
    return eng.Matrix(rp, ci, va, P.n, P.n, fmt, dtype, **opts)


def deterministic(A):
    x = np.random.default_rng(5).uniform(-1, 1, A.n)
    return np.array_equal(A.spmv(x), A.spmv(x))


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def assert_columns(apply_multi, apply, V, ks, what):
    """apply_multi of the first k columns against apply per column, for every k"""
    singles = [apply(np.ascontiguousarray(V[:, j])) for j in range(max(ks))]
    for k in ks:
        got = apply_multi(np.ascontiguousarray(V[:, :k]))
        assert got.shape == (V.shape[0], k) and got.dtype == V.dtype
        for j in range(k):
            assert np.array_equal(got[:, j], singles[j]) and same_bits(np.ascontiguousarray(got[:, j]), singles[j]), \
                f"{what}: column {j} of k = {k}"
    return singles


def assert_same_solve(got, want, what):
    for f in INFO_FIELDS:                                    # a NaN (the norms of a column with a NaN in b) equals a NaN
        assert got[f] == want[f] or (got[f] != got[f] and want[f] != want[f]), f"{what}: {f}: {got[f]!r} and {want[f]!r}"
    assert same_bits(got["x"], want["x"]), f"{what}: x"
    assert same_bits(got["history"], want["history"]), f"{what}: history"


# ---- 1. the cycle, column against single ------------------------------------------------------------------------------------------------

CYCLE_RUNS = [(name, i) for name in ac.CYCLE_CASES for i in range(len(LAYOUTS) if name == "grid" else 1)] + [("grid_nu2", 0)]


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("name,layout", CYCLE_RUNS, ids=[f"{n}-{LAYOUT_IDS[i]}" for n, i in CYCLE_RUNS])
def test_the_cycle_of_a_block_is_the_cycle_of_each_column(eng, name, layout, dtype):
    fmt, opts = LAYOUTS[layout]
    M = amg(eng, name, dtype, fmt, **opts)
    assert deterministic(M.A)
    n = ac.case(name)[3]
    V = mc.cycle_block(n).astype(dtype)
    if name == "n128":
        assert M.info()["coarse"] == "dense" and M.info()["rows"] == [128]      # the whole triangle of LDS
    if name == "n129":
        assert M.levels > 1                                                     # one row too many: coarsened first
    assert_columns(M.apply_multi, M.apply, V, mc.K_CYCLE, f"{name} {fmt} {np.dtype(dtype).name}")
    M.close()


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("how", ["filtered", "near_null"])
def test_the_cycle_of_a_built_hierarchy(eng, how, dtype):
    rp, ci, va, n, _ = ac.case("grid")
    kw = dict(filtered=True) if how == "filtered" else dict(near_null=mc.near_null(n))
    M = eng.Amg.build(rp, ci, va, n, dtype=dtype, **kw)
    assert deterministic(M.A)
    assert_columns(M.apply_multi, M.apply, mc.cycle_block(n).astype(dtype), mc.K_CYCLE, f"{how} {np.dtype(dtype).name}")
    M.close()


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("power", [1, 2])
def test_fsai_of_a_block_is_fsai_of_each_column(eng, power, dtype):
    rp, ci, va, n, _ = pc.spd_grid(45)
    F = eng.Fsai(rp, ci, va, n, pattern=eng.fsai_pattern(rp, ci, n, power), dtype=dtype)
    V = mc.cycle_block(n).astype(dtype)
    assert_columns(F.apply_multi, F.apply, V, mc.K_CYCLE, f"fsai power {power} {np.dtype(dtype).name}")
    assert_columns(F.apply_multi, F.apply, V, (3,), "a smaller k after a larger one")
    F.close()


# ---- 2. strided blocks and guards --------------------------------------------------------------------------------------------------------

def _nan_of(dtype, payload):
    """a quiet NaN with `payload` in its low mantissa bits"""
    if np.dtype(dtype) == np.float64:
        return np.array([0x7ff8000000000000 | payload], np.uint64).view(np.float64)[0]
    return np.array([0x7fc00000 | payload], np.uint32).view(np.float32)[0]


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("which", ["amg", "fsai"])
def test_strided_blocks_leave_every_padding_and_guard_byte_alone(eng, which, dtype):
    import torch
    rp, ci, va, n, _ = ac.case("grid")
    M = amg(eng, "grid", dtype) if which == "amg" else eng.Fsai(rp, ci, va, n, dtype=dtype)
    if which == "amg":
        assert deterministic(M.A)
    V = mc.cycle_block(n).astype(dtype)
    tdt = torch.float64 if dtype == np.float64 else torch.float32
    word = np.uint64 if dtype == np.float64 else np.uint32
    for k in mc.K_CYCLE:
        singles = [M.apply(np.ascontiguousarray(V[:, j])) for j in range(k)]
        ldin, ldout = k + 3, k + 5
        host_in = np.full((n + 2, ldin), _nan_of(dtype, 0x51), dtype)
        host_in[1:n + 1, :k] = V[:, :k]
        host_out = np.full((n + 2, ldout), _nan_of(dtype, 0xa7), dtype)
        t_in = torch.from_numpy(host_in.copy()).to("cuda")
        t_out = torch.from_numpy(host_out.copy()).to("cuda")
        size = t_in.element_size()
        M.apply_multi_device(k, t_in.data_ptr() + ldin * size, ldin, t_out.data_ptr() + ldout * size, ldout)
        torch.cuda.synchronize()
        got, kept = t_out.cpu().numpy(), t_in.cpu().numpy()
        assert got.dtype == dtype and t_out.dtype == tdt
        for j in range(k):
            assert same_bits(np.ascontiguousarray(got[1:n + 1, j]), singles[j]), f"{which}: column {j} of k = {k}, strided"
        want = host_out.copy()
        want[1:n + 1, :k] = got[1:n + 1, :k]
        assert got.view(word).tobytes() == want.view(word).tobytes(), f"{which}: k = {k}: a padding or guard slot of out moved"
        assert kept.view(word).tobytes() == host_in.view(word).tobytes(), f"{which}: k = {k}: in moved"
        # in place, equal ld: the same columns, and the padding and the guard rows of the block stay
        t_io = torch.from_numpy(host_in.copy()).to("cuda")
        M.apply_multi_device(k, t_io.data_ptr() + ldin * size, ldin, t_io.data_ptr() + ldin * size, ldin)
        torch.cuda.synchronize()
        got = t_io.cpu().numpy()
        for j in range(k):
            assert same_bits(np.ascontiguousarray(got[1:n + 1, j]), singles[j]), f"{which}: column {j} of k = {k}, in place"
        want = host_in.copy()
        want[1:n + 1, :k] = got[1:n + 1, :k]
        assert got.view(word).tobytes() == want.view(word).tobytes(), f"{which}: k = {k}: in place, a padding or guard slot moved"
    with pytest.raises(eng.SpmvError, match=f"{which}_apply_multi: in == out needs ldin == ldout"):
        M.apply_multi_device(2, t_io.data_ptr(), 4, t_io.data_ptr(), 5)
    with pytest.raises(eng.SpmvError, match=f"{which}_apply_multi: ldin = 2, ldout = 3: both must be >= k = 3"):
        M.apply_multi_device(3, t_in.data_ptr(), 2, t_out.data_ptr(), 3)
    with pytest.raises(eng.SpmvError, match=f"{which}_apply_multi: k = 0"):
        M.apply_multi_device(0, t_in.data_ptr(), 4, t_out.data_ptr(), 4)
    with pytest.raises(eng.SpmvError, match=f"{which}_apply_multi: NULL argument"):
        M.apply_multi_device(2, 0, 4, t_out.data_ptr(), 4)
    M.close()


# ---- 3. the solve, column against single -------------------------------------------------------------------------------------------------

def precond_of(eng, kind, fmt, dtype, opts):
    """(precond for pcg_tri / pcg_tri_multi, the handle to solve on, what to close)"""
    P = pc.problem()
    rp, ci, va = P.csr
    if kind == "amg":
        M = amg(eng, "grid", dtype, fmt, **opts)
        return M, M.A, [M]
    A = handle(eng, fmt, dtype, **opts)
    if kind == "none":
        return None, A, [A]
    if kind == "jacobi":
        return (None, (1.0 / P.diag).astype(dtype), None), A, [A]
    F = eng.Fsai(rp, ci, va, P.n, dtype=dtype)
    return F, A, [F, A]


def single_count(kind, dtype):
    import fsai_cases as fc
    return {"none": pc.COUNTS[dtype]["none"], "jacobi": pc.COUNTS[dtype]["jacobi"], "amg": ac.COUNTS[dtype]["grid"],
            "fsai": fc.COUNTS[dtype][1]}[kind]


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("layout", range(len(LAYOUTS)), ids=LAYOUT_IDS)
@pytest.mark.parametrize("kind", ["none", "jacobi", "fsai", "amg"])
def test_the_solve_of_a_block_is_the_solve_of_each_column(eng, kind, layout, dtype):
    fmt, opts = LAYOUTS[layout]
    precond, A, owned = precond_of(eng, kind, fmt, dtype, opts)
    assert deterministic(A)
    tol = PREC[dtype]["tol"]
    B = mc.solve_block().astype(dtype)
    what = f"{kind} {LAYOUT_IDS[layout]} {np.dtype(dtype).name}"
    want = [A.pcg_tri(np.ascontiguousarray(B[:, j]), precond, tol, MAX_ITERATIONS) for j in range(B.shape[1])]
    print(f"[pcg_tri_multi] {what}: single iterations {[w['iterations'] for w in want]}, the table has {single_count(kind, dtype)}")
    assert all(w["stop"] == 1 for w in want)
    assert want[0]["iterations"] == single_count(kind, dtype), f"{what}: the single solve of b"
    for k in mc.K_SOLVE:
        got = A.pcg_tri_multi(np.ascontiguousarray(B[:, :k]), precond, tol, MAX_ITERATIONS)
        assert len(got) == k
        for j in range(k):
            assert_same_solve(got[j], want[j], f"{what}: column {j} of k = {k}")
        assert len({g["spmv_calls"] for g in got}) == 1 and len({g["seconds"] for g in got}) == 1
        latest = max(w["iterations"] for w in want[:k])
        assert latest <= got[0]["spmv_calls"] <= latest + 3 * POLL + 1, f"{what}: k = {k}: {got[0]['spmv_calls']} SpMMs, latest {latest}"
    for h in owned:
        h.close()


def test_a_triangular_part_is_refused(eng):
    P = pc.problem()
    rp, ci, va = P.csr
    A = handle(eng, "sell_c_sigma", np.float64)
    sgs = eng.sgs_precond(rp, ci, va, P.n, block_rows=64)
    B = mc.solve_block()[:, :2]
    for precond in (sgs, (sgs[0], None, None), (None, sgs[1], sgs[2])):
        with pytest.raises(eng.SpmvError, match="pcg_tri_multi: M has a triangular part .*no k-column triangular solve"):
            A.pcg_tri_multi(B, precond)
    for T in (sgs[0], sgs[2]):
        T.close()
    A.close()


# ---- 4. the freeze -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["none", "amg", "fsai"])
def test_a_stopped_column_is_frozen_while_its_neighbours_run(eng, kind):
    precond, A, owned = precond_of(eng, kind, "sell_c_sigma", np.float64, {})
    assert deterministic(A)
    B = mc.freeze_columns()
    want = [A.pcg_tri(np.ascontiguousarray(B[:, j]), precond, 1e-12, MAX_ITERATIONS) for j in range(5)]
    got = A.pcg_tri_multi(B, precond, 1e-12, MAX_ITERATIONS)
    print(f"[pcg_tri_multi] freeze, {kind}: iterations {[g['iterations'] for g in got]}, stops {[g['stop'] for g in got]}, "
          f"{got[0]['spmv_calls']} SpMMs")
    assert tuple(g["stop"] for g in got) == mc.FREEZE_STOPS
    if kind == "none":
        assert (got[0]["iterations"], got[1]["iterations"]) == (pc.COUNTS[np.float64]["none"], 1)
        assert got[0]["iterations"] - got[1]["iterations"] > 2 * POLL
    for j in range(5):
        assert_same_solve(got[j], want[j], f"freeze, {kind}: column {j}")
    for j in (2, 3):
        assert got[j]["iterations"] == 0 and not got[j]["x"].any() and got[j]["history"].size == 0
    assert got[2]["rnorm0"] == 0 and got[2]["rnorm"] == 0
    for h in owned:
        h.close()


# ---- 5. max_iterations reached -----------------------------------------------------------------------------------------------------------

def test_the_cap_stops_every_column_with_2(eng):
    M = amg(eng, "grid")
    assert deterministic(M.A)
    B = np.ascontiguousarray(mc.solve_block()[:, :3])
    want = [M.A.pcg_tri(np.ascontiguousarray(B[:, j]), M, 1e-12, 7) for j in range(3)]
    got = M.A.pcg_tri_multi(B, M, 1e-12, 7)
    for j in range(3):
        assert got[j]["stop"] == 2 and got[j]["iterations"] == 7 and got[j]["history"].shape == (7,)
        assert_same_solve(got[j], want[j], f"cap 7: column {j}")
    want = [M.A.pcg_tri(np.ascontiguousarray(B[:, j]), M, 1e-12, 0) for j in range(3)]
    got = M.A.pcg_tri_multi(B, M, 1e-12, 0)
    for j in range(3):
        assert got[j]["stop"] == 2 and got[j]["iterations"] == 0 and not got[j]["x"].any() and got[j]["history"].size == 0
        assert got[j]["rnorm"] == got[j]["rnorm0"] and abs(got[j]["rnorm0"] - np.linalg.norm(B[:, j])) <= 1e-13 * np.linalg.norm(B[:, j])
        assert_same_solve(got[j], want[j], f"cap 0: column {j}")
    M.close()


# ---- 6. where the row loops take a second trip -------------------------------------------------------------------------------------------

def test_path_wrap_takes_second_trips(eng):
    M = amg(eng, "path_wrap")
    n = ac.case("path_wrap")[3]
    assert n == 256 * 1024 + 37 and deterministic(M.A)
    rng = np.random.default_rng(41)
    B = np.ascontiguousarray(np.stack([ac.path_problem()[1], rng.uniform(-1, 1, n), np.ones(n)], axis=1))
    assert_columns(M.apply_multi, M.apply, B, (3,), "path_wrap: the cycle")
    want = [M.A.pcg_tri(np.ascontiguousarray(B[:, j]), M, 1e-12, 6) for j in range(3)]
    got = M.A.pcg_tri_multi(B, M, 1e-12, 6)
    for j in range(3):
        assert got[j]["stop"] == 2 and got[j]["iterations"] == 6
        assert_same_solve(got[j], want[j], f"path_wrap: column {j}")
    M.close()


# ---- 7. the plan -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout", range(len(LAYOUTS)), ids=LAYOUT_IDS)
def test_the_plan_counts_passes_and_launches(eng, layout):
    fmt, opts = LAYOUTS[layout]
    M = amg(eng, "grid", np.float64, fmt, **opts)
    info, o = M.info(), ac.options("grid")
    assert M.apply_multi_plan(1) == (info["spmvs_per_apply"], info["launches_per_apply"])
    nu, cs, nl, dense = o["sweeps"], o["coarse_sweeps"], info["levels"], info["coarse"] == "dense"
    for k in mc.K_CYCLE:
        passes = 0
        for l in range(nl):
            A, P, R = M.level_matrices(l)
            if l < nl - 1:
                passes += 2 * nu * A.spmm_plan(k)[0] + P.spmm_plan(k)[0] + R.spmm_plan(k)[0]
            elif not dense:
                passes += (cs - 1) * A.spmm_plan(k)[0]
        vector = (nl - 1) * (2 * nu + 1) + (1 if dense else cs)
        assert M.apply_multi_plan(k) == (passes, passes + len(mc.chunks(k)) * vector), k
    with pytest.raises(eng.SpmvError, match="amg_apply_multi_plan: k = 0"):
        M.apply_multi_plan(0)
    M.close()


# ---- 8. after an update ------------------------------------------------------------------------------------------------------------------

def test_an_update_of_the_values_keeps_the_blocks_working(eng):
    rp, ci, va, n, _ = ac.case("grid")
    M = amg(eng, "grid")
    V = mc.cycle_block(n)
    before = assert_columns(M.apply_multi, M.apply, V, (3, 9), "before the update")
    footprint = eng.lib().spmv_mi355x_amg_mem_footprint(M.h)
    assert footprint > M.mem_footprint                      # the blocks are counted
    M.update_values_prepare()
    M.update_values(0.7 * va)
    after = assert_columns(M.apply_multi, M.apply, V, (3, 9), "after the update")
    assert not np.array_equal(before[0], after[0])
    M.close()


# ---- 9. determinism ----------------------------------------------------------------------------------------------------------------------

def test_twice_the_same_bits(eng):
    M = amg(eng, "grid", np.float32)
    B = mc.solve_block().astype(np.float32)
    a = M.A.pcg_tri_multi(B, M, 1e-5, MAX_ITERATIONS)
    b = M.A.pcg_tri_multi(B, M, 1e-5, MAX_ITERATIONS)
    for j in range(B.shape[1]):
        assert_same_solve(a[j], b[j], f"column {j}")
    assert same_bits(M.apply_multi(B), M.apply_multi(B))
    M.close()
