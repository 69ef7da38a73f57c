"""The device ILU(0) (include/spmv_mi355x.h "ILU(0)") on the GPU. There is no tolerance on the factor: every case is held to the
sequential C loop of tests/ilu0_reference.c with np.array_equal, whatever the level schedule, the lanes per row and the block size.

Cases (ilu0_cases.matrix): spd_grid(45) and convdiff(45), global and at B = 64, 100, 256; the dense 70 x 70 matrix, whose rows are
wider than a wave and whose every k step feeds the next (the ordering hazard between steps); the arrow matrix (one row of 600 entries
and 599 k steps); a random nonsymmetric pattern with rows that hold only their diagonal; two levels of 35 000 rows (row indices past
65 536) and of 150 000 rows (more rows than one launch's workgroups hold at once: the grid-stride loop); n = 0 and n = 1.

The solvers take ilu0_precond's triple unchanged. Their references are the restatements of pcg_tri_cases.py and test_gpu_gmres_tri.py
run with the REFERENCE factor (ilu0_cases.apply), and the bounds are the family's (pcg_tri_cases.PREC, shares_of_the_bounds)."""
import numpy as np
import pytest

import ilu0_cases as ic
import pcg_tri_cases as pc
from pcg_tri_cases import MAX_ITERATIONS, PREC
from test_ilu0_abi import expected_info

pytestmark = pytest.mark.gpu

LAYOUTS = [("sell_c_sigma", {}), ("csr_vector", {})]
INFO_FIELDS = ("iterations", "stop", "rnorm", "rnorm0", "prnorm", "xnorm")


@pytest.fixture(scope="module")
def eng():
    import spmv_mi355x as eng
    assert eng.device_count() >= 1, "no GPU visible: the -m gpu tests need an MI355X"
    return eng


def device_copy(ptr, count):
    """`count` doubles at a device pointer, copied to the host"""
    import torch

    class View:
        __cuda_array_interface__ = dict(shape=(count,), typestr="<f8", data=(ptr, False), version=2, strides=None)
    torch.cuda.synchronize()
    return torch.as_tensor(View(), device="cuda").cpu().numpy().copy()


def close(M):
    for h in M or ():
        if h is not None and not isinstance(h, np.ndarray):
            h.close()


# ---- 1. the factor, bit for bit ------------------------------------------------------------------------------------------------------

CASES = [(name, B) for name in ("spd_grid", "convdiff") for B in (None, 64, 100, 256)] + \
        [("dense70", None), ("dense70", 32), ("arrow", None), ("arrow", 256), ("random", None), ("random", 50), ("random", 0),
         ("pairs", None), ("pairs", 4096), ("pairs_long", None), ("one", None), ("one", 0)]


@pytest.mark.parametrize("name,B", CASES, ids=[f"{n}-{b}" for n, b in CASES])
def test_the_factor_is_the_sequential_loop(eng, name, B):
    rp, ci, va, n = ic.matrix(name)
    F = eng.Ilu0(rp, ci, n, block_rows=B)
    used = None if B is None else F.info["block_rows"]
    assert used == (B or (4096 if B == 0 else None))
    want, bad = ic.factor(name, used)
    assert bad == -1
    with pytest.raises(eng.SpmvError, match="ilu0_values: the handle has not been factorized yet"):
        F.values()
    with pytest.raises(eng.SpmvError, match="ilu0_values: "):
        F.values_device()
    got = F.factor(va).values()
    assert got.dtype == np.float64 and got.shape == want.shape
    assert np.array_equal(got, want), f"{name} B={B}: {np.sum(got != want)} of {len(want)} entries differ from the reference"
    assert np.array_equal(device_copy(F.values_device(), len(want)), got)
    keep = ic.kept(rp, ci, n, used)
    assert np.array_equal(got[~keep], va[~keep])                              # dropped entries keep A's value
    info = F.info
    assert info["breakdown_row"] == -1 and info["factorizations"] == 1
    assert {k: info[k] for k in expected_info(name, used)} == expected_info(name, used)
    assert F.mem_footprint == 12 * len(ci) + 16 * n + 16
    # again: the same bits, and the count goes up
    assert np.array_equal(F.factor(va).values(), want) and F.info["factorizations"] == 2
    F.close()
    F.close()


def test_no_rows(eng):
    rp, ci, va, n = ic.matrix("empty")
    for B in (None, 0, 7):
        F = eng.Ilu0(rp, ci, 0, block_rows=B)
        assert F.factor(va).values().shape == (0,)
        F.factor_device(0)
        info = F.info
        assert (info["n"], info["nnz"], info["levels"], info["launches"], info["breakdown_row"], info["factorizations"]) == (0, 0, 0, 0, -1, 2)
        M = F.precond()
        assert M[1] is None and M[0].solve(np.zeros(0)).shape == (0,)
        close(M)
        F.close()


def test_new_values_on_a_handle_are_a_fresh_handle(eng):
    """factor() may be called any number of times: same pattern, new numbers"""
    for name, B in (("convdiff", None), ("convdiff", 100), ("random", None)):
        rp, ci, va, n = ic.matrix(name)
        v2 = va * (1 + 0.1 * np.random.default_rng(5).uniform(-1, 1, len(va)))
        rows = np.repeat(np.arange(n), np.diff(rp))
        v2[rows == ci] = va[rows == ci] * 1.5                                  # still diagonally dominant
        want2 = ic.reference(rp, ci, v2, n, B)[0]
        F = eng.Ilu0(rp, ci, n, block_rows=B)
        first = F.factor(va).values()
        second = F.factor(v2).values()
        third = F.factor(va).values()
        F.close()
        G = eng.Ilu0(rp, ci, n, block_rows=B)
        fresh = G.factor(v2).values()
        G.close()
        assert np.array_equal(second, fresh) and np.array_equal(second, want2) and not np.array_equal(first, second)
        assert np.array_equal(first, third) and np.array_equal(first, ic.factor(name, B)[0])


def test_factor_device_on_another_stream_is_factor(eng):
    import torch
    for name, B in (("spd_grid", None), ("spd_grid", 64), ("dense70", None), ("pairs", None)):
        rp, ci, va, n = ic.matrix(name)
        F = eng.Ilu0(rp, ci, n, block_rows=B)
        want = F.factor(va).values()
        assert np.array_equal(want, ic.factor(name, B)[0])
        F.factor(np.ones(len(va)))                                            # something else in f
        v = torch.from_numpy(np.array(va)).cuda()
        torch.cuda.synchronize()
        s = torch.cuda.Stream()
        F.factor_device(v.data_ptr(), s.cuda_stream)
        got = F.values()                                                      # synchronises
        assert np.array_equal(got, want), (name, B)
        assert np.array_equal(v.cpu().numpy(), va)                            # the caller's values are read, never written
        assert F.info["factorizations"] == 3 and F.info["breakdown_row"] == -1
        # in place: the handle's own array as the source
        once = F.factor(va).values()
        F.factor_device(F.values_device())
        assert np.array_equal(F.values(), ic.reference(rp, ci, once, n, B)[0])
        F.close()


# ---- 2. breakdown --------------------------------------------------------------------------------------------------------------------

def test_a_zero_pivot_is_reported_and_the_arithmetic_goes_on(eng):
    rp, ci, va, n = ic.singular()
    F = eng.Ilu0(rp, ci, n)
    f = F.factor(va).values()
    assert f.tolist() == [1.0, 1.0, 1.0, 0.0] and np.array_equal(f, ic.reference(rp, ci, va, n)[0])
    assert F.info["breakdown_row"] == 1
    with pytest.raises(eng.SpmvError, match=r"trsv_create: the diagonal of row 1 is 0"):
        F.precond()
    with pytest.raises(eng.SpmvError, match=r"trsv_create: the diagonal of row 1 is 0"):
        eng.ilu0_precond(rp, ci, va, n)
    # healthy numbers on the same handle clear it
    assert F.factor(np.array([2.0, 1.0, 1.0, 2.0])).info["breakdown_row"] == -1
    close(F.precond())
    F.close()


def test_the_lowest_bad_pivot_is_reported_wherever_it_arises(eng):
    """rows 3 and 10 of the random matrix hold only their diagonal (level 0, no launch visits them): a zero, a NaN or an Inf there is
    reported as row 3, and f is the reference's, NaNs included"""
    rp, ci, va, n = ic.matrix("random")
    rows = np.repeat(np.arange(n), np.diff(rp))
    F = eng.Ilu0(rp, ci, n)
    for value in (0.0, np.nan, np.inf):
        v = va.copy()
        v[(rows == ci) & np.isin(rows, (3, 10))] = value
        want, bad = ic.reference(rp, ci, v, n)
        assert bad == 3
        got = F.factor(v).values()
        assert np.array_equal(got, want, equal_nan=True) and F.info["breakdown_row"] == 3
    # a zero pivot of level 0 that a later row divides by: Inf and NaN flow through the last row of the arrow matrix as IEEE gives them
    rp, ci, va, n = ic.matrix("arrow")
    v = np.ones(len(va))
    v[0] = 0.0
    want, bad = ic.reference(rp, ci, v, n)
    G = eng.Ilu0(rp, ci, n)
    assert bad == 0 and np.array_equal(G.factor(v).values(), want, equal_nan=True) and G.info["breakdown_row"] == 0
    G.close()
    F.close()


# ---- 3. the solvers take the triple unchanged ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B", (None, 100), ids=str)
def test_pcg_tri_under_the_device_factor(eng, B):
    P = pc.problem()
    rp, ci, va = P.csr
    want = P.solve()
    for dtype, lim in PREC.items():
        name = np.dtype(dtype).name
        _, ref, ref_stop = ic.pcg_restatement(dtype, B, lim["tol"])
        assert ref_stop == 1 and ref.size == ic.COUNTS[dtype][B]
        bn = np.linalg.norm(P.b.astype(dtype).astype(np.float64))
        rows = np.nonzero(ref / bn > lim["ratio"])[0]
        assert rows[-1] == rows.size - 1 and rows.size >= lim["share"] * ref.size
        M = eng.ilu0_precond(rp, ci, va, P.n, dtype, block_rows=B)
        assert M[1] is None and M[0].block_info()["block_rows"] == M[2].block_info()["block_rows"] == (B or 0)
        for fmt, opts in LAYOUTS:
            A = eng.Matrix(rp, ci, va, P.n, P.n, fmt, dtype, **opts)
            what = f"spd_grid(45) {A.format_name} {name} ILU(0) B={B}"
            got = A.pcg_tri(P.b.astype(dtype), precond=M, tol=lim["tol"], max_iterations=MAX_ITERATIONS)
            A.close()
            k = got["iterations"]
            print(f"[ilu0] {what}: {k} iterations (the restatement {ref.size}), rnorm {got['rnorm']:.3g}")
            assert got["stop"] == 1 and k == ref.size, f"{what}: stop {got['stop']} after {k} iterations, the restatement {ref.size}"
            for key, v in pc.shares_of_the_bounds(P, got, dtype, want).items():
                print(f"[ilu0] {what}: {key} is {v:.3g} of its bound")
                assert v <= 1, f"{what}: {key} is {v:.3g} times its bound"
            d = np.abs(got["history"][rows] - ref[rows]) / ref[rows]
            print(f"[ilu0] {what}: largest history deviation {d.max():.3g} on {rows.size} rows")
            assert d.max() <= lim["hist"], f"{what}: history deviates by {d.max():.3g} at row {np.argmax(d)}"
        close(M)


def test_pcg_trsm_multi_columns_are_the_single_solves(eng):
    P = pc.problem()
    rp, ci, va = P.csr
    Bk = np.column_stack([P.b, np.random.default_rng(11).uniform(-1, 1, P.n), np.cos(np.arange(P.n))])
    for dtype, lim in PREC.items():
        for B in (None, 100):
            M = eng.ilu0_precond(rp, ci, va, P.n, dtype, block_rows=B)
            A = eng.Matrix(rp, ci, va, P.n, P.n, "sell_c_sigma", dtype)
            multi = A.pcg_trsm_multi(Bk.astype(dtype), precond=M, tol=lim["tol"], max_iterations=MAX_ITERATIONS)
            for j in range(3):
                one = A.pcg_tri(Bk[:, j].astype(dtype), precond=M, tol=lim["tol"], max_iterations=MAX_ITERATIONS)
                assert one["stop"] == 1
                for key in INFO_FIELDS:
                    assert multi[j][key] == one[key], (np.dtype(dtype).name, B, j, key)
                assert np.array_equal(multi[j]["x"], one["x"]) and np.array_equal(multi[j]["history"], one["history"])
            A.close()
            close(M)


def test_gmres_under_the_blocked_device_factor(eng):
    import test_gpu_gmres_tri as gt
    Pg = gt.problem()
    rp, ci, va = Pg.csr
    n, B, restart = Pg.n, 100, 20
    Mref = ic.apply(rp, ci, ic.factor("convdiff", B)[0], n, B, np.float64)
    _, ref, ref_stop, _ = gt.restate(Pg.dense(np.float64), Pg.b, restart, Mref, 1e-12, gt.MAX_ITERATIONS, np.float64)
    sgs = Pg.restatement(np.float64, restart, B, 1e-12)[1].size
    assert ref_stop == 1 and ref.size < sgs == 80                              # a property of the input
    M = eng.ilu0_precond(rp, ci, va, n, block_rows=B)
    for fmt, opts in LAYOUTS:
        A = Pg.handle(eng, fmt, np.float64, **opts)
        got = A.gmres(Pg.b, restart=restart, precond=M, tol=1e-12, max_iterations=gt.MAX_ITERATIONS)
        A.close()
        print(f"[ilu0] gmres({restart}) convdiff(45) {fmt} ILU(0) B={B}: {got['iterations']} iterations (the restatement {ref.size}, SGS {sgs})")
        assert got["stop"] == 1 and abs(got["iterations"] - ref.size) <= 1
        for key, v in gt.shares_of_the_bounds(Pg, got, np.float64).items():
            assert v <= 1, f"{fmt}: {key} is {v:.3g} times its bound"
    close(M)
