"""The folded tail of the AMG cycle on the GPU (include/spmv_mi355x.h "AMG: the small levels as one launch"): Amg.set_fold,
fold_info, apply_level, and apply / apply_multi / pcg_amg / pcg_amg_multi / update_values over a folded hierarchy, fp64 and fp32.

1. Bits. apply(v) with the fold equals "the levels above the first folded one through the borrowed handles, the tail through
   tests/amg_fold_reference.c" bit for bit over amg_cases.vectors; apply_level(f, .) alone equals the reference; twice the same bits;
   in place, f = 0 included. grid folds whole (f = 0) and from level 1, grid_nu2 runs nu = 2 inside the tail, n129 has a dense level
   under 129 rows, n128 and one are the dense solve alone, grid_weak the coarse sweeps alone, path_wrap (built once per module) folds
   levels 3 to 5 (3 450 rows over 1024 lanes: several trips of the row loop) and 4 to 5, its last level by sweeps.
2. Closeness. The same applies lie within amg_cases.CYCLE_BOUND of amg_cases.cycle_restatement, as the unfolded apply does.
3. Fold off is the unfolded apply: after set_fold(r) and set_fold(0), and with a fold_rows below every level's rows.
4. Counts: first_level, launches, apply_multi_plan, mem_footprint.
5. k columns: column j of apply_multi is apply on column j; a NaN column does not disturb its neighbours.
6. Solvers: pcg_amg stops with stop 1, column j of pcg_amg_multi is pcg_amg on b_j; the counts are printed beside amg_cases.COUNTS.
7. Updates: create(V1), set_fold, prepare, update(V2) is create(V2) + set_fold; the same with set_fold after prepare; a pivot that
   fails and comes back is followed.
8. Refusals in their order."""
import ctypes

import numpy as np
import pytest

import amg_cases as ac
import amg_fold_cases as fo
import amg_update_cases as uc
import pcg_tri_cases as pc
from pcg_tri_cases import MAX_ITERATIONS, PREC

pytestmark = pytest.mark.gpu

DTYPES = (np.float64, np.float32)
SOLVE_FIELDS = ("iterations", "stop", "rnorm", "rnorm0", "prnorm", "xnorm")


@pytest.fixture(scope="module")
def eng():
    import spmv_mi355x as eng
    assert eng.device_count() >= 1, "no GPU visible: the -m gpu tests need an MI355X"
    return eng


def amg(eng, name, dtype=np.float64, values=None, **opts):
    rp, ci, va, n, own = ac.case(name)
    return eng.Amg(rp, ci, va if values is None else values, n, "sell_c_sigma", dtype, **own, **opts)


@pytest.fixture(scope="module")
def path(eng):
    """path_wrap, built once per precision"""
    Ms = {dtype: amg(eng, "path_wrap", dtype) for dtype in DTYPES}
    yield Ms
    for M in Ms.values():
        M.close()


def in_place(M, v, level=None):
    """(out of place, in place) of apply_device or apply_level_device on device vectors"""
    import torch
    t = torch.from_numpy(v).cuda()
    u = torch.zeros_like(t)
    if level is None:
        M.apply_device(t.data_ptr(), u.data_ptr())
        M.apply_device(t.data_ptr(), t.data_ptr())
    else:
        M.apply_level_device(level, t.data_ptr(), u.data_ptr())
        M.apply_level_device(level, t.data_ptr(), t.data_ptr())
    torch.cuda.synchronize()
    return u.cpu().numpy(), t.cpu().numpy()


def check_bits_and_closeness(M, name, fold_rows, dtype):
    """items 1 and 2 for one hierarchy, one fold_rows and one precision"""
    ref = ac.reference_of(name)
    rows = [L["n"] for L in ref["lev"]]
    n = ac.case(name)[3]
    M.set_fold(fold_rows)
    f = fo.first_level(rows, fold_rows)
    info = M.fold_info()
    assert (info["fold_rows"], info["first_level"], info["folded_levels"]) == (fold_rows, f, len(rows) - f) and M.fold_rows == fold_rows
    assert f < len(rows), f"{name}: fold_rows = {fold_rows} folds nothing"
    tail = fo.tail_of(name, dtype, f)
    assert info["lanes_per_row"][f:] == tail.lanes[f:] and not any(info["lanes_per_row"][:f])
    want_of = ac.cycle_restatement(name, dtype)
    what = f"{name} fold_rows = {fold_rows} (f = {f}) {np.dtype(dtype).name}"
    worst = 0.0
    for v in ac.vectors(n):
        v = v.astype(dtype)
        got = M.apply(v)
        assert got.dtype == dtype and np.all(np.isfinite(got))
        assert np.array_equal(got, M.apply(v)), f"{what}: twice"
        want = fo.folded_cycle(M, ref, tail, v, **ac.options(name))
        diff = np.nonzero(got != want)[0]
        assert len(diff) == 0, f"{what}: {len(diff)} of {n} values differ from the handles + the C reference, first at {diff[:4]}"
        out, inp = in_place(M, v)
        assert np.array_equal(out, got) and np.array_equal(inp, got), f"{what}: in place"
        close = want_of(v).astype(np.float64)
        worst = max(worst, float(np.abs(got.astype(np.float64) - close).max() / np.abs(close).max()))
    for v in ac.vectors(rows[f]):
        v = v.astype(dtype)
        got = M.apply_level(f, v)
        want = tail.apply(v)
        diff = np.nonzero(got != want)[0]
        assert len(diff) == 0, f"{what}: apply_level: {len(diff)} of {rows[f]} values differ from the C reference, first at {diff[:4]}"
        assert np.array_equal(got, M.apply_level(f, v)), f"{what}: apply_level twice"
        out, inp = in_place(M, v, f)
        assert np.array_equal(out, got) and np.array_equal(inp, got), f"{what}: apply_level in place"
    if f + 1 < len(rows):
        # a level inside the tail: the launch starts there
        v = ac.vectors(rows[f + 1])[0].astype(dtype)
        assert np.array_equal(M.apply_level(f + 1, v), tail.apply(v, f + 1)), f"{what}: apply_level(f + 1)"
    print(f"[amg fold] {what}: lanes {info['lanes_per_row']}, launches {info['launches_per_apply']}, tail products {info['tail_products']}, "
          f"tail entries {info['tail_entries']}, {worst:.3g} from the restatement, {worst / ac.CYCLE_BOUND[dtype]:.3g} of the bound "
          f"{ac.CYCLE_BOUND[dtype]:.3g}")
    assert worst <= ac.CYCLE_BOUND[dtype], f"{what}: {worst:.3g} against {ac.CYCLE_BOUND[dtype]:.3g}"


# ---- 1. and 2. the bits and the closeness ------------------------------------------------------------------------------------------------

FOLDING = [f for f in fo.FOLDS if f[1] != 1]


@pytest.mark.parametrize("name,spec", FOLDING, ids=[f"{n}-{s}" for n, s in FOLDING])
def test_a_folded_apply_is_the_handles_above_and_the_reference_below(eng, name, spec):
    for dtype in DTYPES:
        M = amg(eng, name, dtype)
        check_bits_and_closeness(M, name, fo.fold_rows_of(name, spec), dtype)
        M.close()


@pytest.mark.parametrize("fold_rows", fo.PATH_FOLDS)
def test_path_wrap_folds_its_last_levels(eng, path, fold_rows):
    rows = [L["n"] for L in ac.reference_of("path_wrap")["lev"]]
    assert rows == [262181, 61893, 14612, 3450, 1055, 272] and fo.first_level(rows, fold_rows) == {4096: 3, 1100: 4}[fold_rows]
    for dtype in DTYPES:
        check_bits_and_closeness(path[dtype], "path_wrap", fold_rows, dtype)
        assert path[dtype].info()["coarse"] == "sweeps"
        path[dtype].set_fold(0)


def test_empty(eng):
    for dtype in DTYPES:
        M = amg(eng, "empty", dtype)
        M.set_fold(4096)
        info = M.fold_info()
        assert (info["fold_rows"], info["first_level"], info["folded_levels"], info["launches_per_apply"], info["bytes"]) == (4096, 0, 0, 0, 0)
        assert M.apply(np.zeros(0, dtype)).shape == (0,) and M.mem_footprint == 0
        with pytest.raises(eng.SpmvError, match=r"amg_apply_level: level 0 out of range"):
            M.apply_level_device(0, 8, 8)
        M.close()


# ---- 3. fold off ---------------------------------------------------------------------------------------------------------------------------

def _state(M, n):
    """what an apply, a k-column apply and the queries return; the footprint is read after the k-column blocks exist"""
    import spmv_mi355x
    info = M.info()
    return ({k: v for k, v in info.items() if not k.endswith("_seconds")}, [M.apply_multi_plan(k) for k in (1, 3, 8, 11)],
            [M.apply(v.astype(M.dtype)) for v in ac.vectors(n)], M.apply_multi(np.stack(ac.vectors(n), axis=1).astype(M.dtype)),
            spmv_mi355x.lib().spmv_mi355x_amg_mem_footprint(M.h))


def _same_state(a, b, what):
    assert a[0] == b[0] and a[1] == b[1], f"{what}: {a[:2]} and {b[:2]}"
    assert all(np.array_equal(x, y) for x, y in zip(a[2], b[2])) and np.array_equal(a[3], b[3]), f"{what}: apply"
    assert a[4] == b[4], f"{what}: mem_footprint"


@pytest.mark.parametrize("name", ("grid", "grid_weak", "n128"))
def test_fold_off_is_the_unfolded_apply(eng, name):
    n = ac.case(name)[3]
    for dtype in DTYPES:
        fresh = amg(eng, name, dtype)
        want = _state(fresh, n)
        assert fresh.fold_info()["fold_rows"] == 0 and fresh.fold_info()["first_level"] == fresh.levels and fresh.fold_info()["bytes"] == 0
        M = amg(eng, name, dtype)
        _state(M, n)                                                       # the k-column blocks exist, as they do in `fresh`
        M.set_fold(4096)
        assert M.fold_info()["first_level"] == 0 and M.mem_footprint > want[4]
        M.apply(ac.vectors(n)[0].astype(dtype))
        M.set_fold(0)
        _same_state(_state(M, n), want, f"{name} {np.dtype(dtype).name}: set_fold(4096), set_fold(0)")
        # no level qualifies: nothing folds
        low = min(M.info()["rows"]) - 1
        M.set_fold(low)
        info = M.fold_info()
        assert (info["fold_rows"], info["first_level"], info["folded_levels"], info["bytes"]) == (low, M.levels, 0, 0)
        _same_state(_state(M, n), want, f"{name} {np.dtype(dtype).name}: fold_rows = {low} folds nothing")
        M.close()
        fresh.close()


def test_fold_rows_of_one_row_folds_nothing_on_grid(eng):
    M = amg(eng, "grid")
    M.set_fold(1)
    assert M.fold_info()["first_level"] == M.levels == 3 and M.info()["launches_per_apply"] == 2 * 4 + 2 * 3 + 1
    M.close()


# ---- 4. counts -------------------------------------------------------------------------------------------------------------------------------

def _chunks(k):
    return k // 8 + bin(k % 8).count("1")


@pytest.mark.parametrize("name,spec", (("grid", 4096), ("grid", "rows1"), ("grid_nu2", "rows1"), ("grid_weak", 4096)))
def test_the_counts_follow_the_fold(eng, name, spec):
    opts = ac.options(name)
    nu, cs = opts["sweeps"], opts["coarse_sweeps"]
    M = amg(eng, name)
    before, footprint = M.info(), M.mem_footprint
    plans = {k: M.apply_multi_plan(k) for k in (1, 2, 3, 8, 11)}
    fold_rows = fo.fold_rows_of(name, spec)
    M.set_fold(fold_rows)
    info, fi = M.info(), M.fold_info()
    f = fo.first_level(before["rows"], fold_rows)
    dense = before["coarse"] == "dense"
    assert fi["first_level"] == f and fi["folded_levels"] == M.levels - f
    assert info["spmvs_per_apply"] == fi["spmvs_per_apply"] == f * (2 * nu + 2)
    assert info["launches_per_apply"] == fi["launches_per_apply"] == f * (2 * nu + 2) + f * (2 * nu + 1) + 1
    products = entries = 0
    for l in range(f, M.levels):
        last = l == M.levels - 1
        with_a = (0 if dense else cs - 1) if last else 2 * nu
        products += with_a + (0 if last else 2)
        entries += with_a * before["nnz"][l] + (0 if last else 2 * before["nnz_p"][l])
    assert (fi["tail_products"], fi["tail_entries"]) == (products, entries)
    assert before["spmvs_per_apply"] == info["spmvs_per_apply"] + products
    for k, (passes, launches) in plans.items():
        got = M.apply_multi_plan(k)
        above = sum(M.level_matrices(l)[i].spmm_plan(k)[0] * t for l in range(f) for i, t in ((0, 2 * nu), (1, 1), (2, 1)))
        assert got == (above, above + _chunks(k) * (f * (2 * nu + 1) + 1)), f"{name} k = {k}: {got}"
        assert got[1] < launches and got[0] <= passes
    assert M.apply_multi_plan(1) == (info["spmvs_per_apply"], info["launches_per_apply"])
    itemsize = 8
    want_bytes = 2 * M.levels * 112                                        # the two descriptor arrays
    for l in range(f, M.levels):
        want_bytes += (before["rows"][l] + 1) * 4 + before["nnz"][l] * (4 + itemsize)
        if l < M.levels - 1:
            want_bytes += (before["rows"][l] + 1 + before["rows"][l + 1] + 1) * 4 + 2 * before["nnz_p"][l] * (4 + itemsize)
    assert fi["bytes"] == want_bytes and M.mem_footprint == footprint + fi["bytes"]
    M.set_fold(0)
    assert M.mem_footprint == footprint and M.info()["launches_per_apply"] == before["launches_per_apply"]
    M.close()


# ---- 5. k columns ------------------------------------------------------------------------------------------------------------------------------

def check_columns(M, n, what):
    rng = np.random.default_rng(23)
    for k in (1, 2, 3, 8, 11):
        V = rng.uniform(-1, 1, (n, k)).astype(M.dtype)
        got = M.apply_multi(V)
        for j in range(k):
            diff = np.nonzero(got[:, j] != M.apply(np.ascontiguousarray(V[:, j])))[0]
            assert len(diff) == 0, f"{what} k = {k}: column {j} differs from the single apply at {diff[:4]}"
        if k > 1:
            W = V.copy()
            W[:, 1] = np.nan
            bad = M.apply_multi(W)
            keep = [j for j in range(k) if j != 1]
            assert np.array_equal(bad[:, keep], got[:, keep]) and np.all(np.isnan(bad[:, 1])), f"{what} k = {k}: a NaN column"


@pytest.mark.parametrize("spec", (4096, "rows1"))
def test_columns_of_apply_multi_are_single_applies_on_grid(eng, spec):
    for dtype in DTYPES:
        M = amg(eng, "grid", dtype)
        M.set_fold(fo.fold_rows_of("grid", spec))
        check_columns(M, M.n, f"grid {spec} {np.dtype(dtype).name}")
        M.set_fold(0)
        check_columns(M, M.n, f"grid, fold off again, {np.dtype(dtype).name}")
        M.close()


def test_columns_of_apply_multi_are_single_applies_on_path_wrap(eng, path):
    for dtype in DTYPES:
        M = path[dtype]
        M.set_fold(4096)
        check_columns(M, M.n, f"path_wrap 4096 {np.dtype(dtype).name}")
        M.set_fold(0)


# ---- 6. the solvers ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("spec", (4096, "rows1"))
def test_the_solvers_pick_the_fold_up(eng, spec):
    P = pc.problem()
    rng = np.random.default_rng(31)
    for dtype, lim in PREC.items():
        M = amg(eng, "grid", dtype)
        A = M.A
        b = P.b.astype(dtype)
        unfolded = A.pcg_tri(b, precond=M, tol=lim["tol"], max_iterations=MAX_ITERATIONS)
        M.set_fold(fo.fold_rows_of("grid", spec))
        got = A.pcg_tri(b, precond=M, tol=lim["tol"], max_iterations=MAX_ITERATIONS)
        print(f"[amg fold] pcg_amg grid fold {spec} {np.dtype(dtype).name}: {got['iterations']} iterations, unfolded {unfolded['iterations']}, "
              f"amg_cases.COUNTS {ac.COUNTS[dtype]['grid']}")
        assert got["stop"] == 1 and got["prnorm"] <= lim["tol"] * got["rnorm0"] * (1 + 1e-12)
        for key, v in pc.shares_of_the_bounds(P, got, dtype, P.solve()).items():
            assert v <= 1, f"fold {spec} {np.dtype(dtype).name}: {key} is {v:.3g} times its bound"
        B = np.stack([b] + [rng.uniform(-1, 1, P.n).astype(dtype) for _ in range(2)], axis=1)
        multi = A.pcg_tri_multi(B, precond=M, tol=lim["tol"], max_iterations=MAX_ITERATIONS)
        for j in range(B.shape[1]):
            single = got if j == 0 else A.pcg_tri(np.ascontiguousarray(B[:, j]), precond=M, tol=lim["tol"], max_iterations=MAX_ITERATIONS)
            for key in SOLVE_FIELDS:
                assert multi[j][key] == single[key], f"fold {spec} column {j}: {key}: {multi[j][key]!r} and {single[key]!r}"
            assert np.array_equal(multi[j]["x"], single["x"]) and np.array_equal(multi[j]["history"], single["history"]), f"column {j}"
        M.close()


# ---- 7. updates ------------------------------------------------------------------------------------------------------------------------------

def _snapshot(M, n):
    fi = M.fold_info()
    info = M.info()
    return ({k: info[k] for k in ("levels", "rows", "nnz", "nnz_p", "omega", "rho", "coarse_kind", "spmvs_per_apply", "launches_per_apply")}, fi,
            [M.apply(v.astype(M.dtype)) for v in ac.vectors(n)], M.apply_multi(np.stack(ac.vectors(n), axis=1).astype(M.dtype)))


def _same_snapshot(a, b, what):
    assert a[0] == b[0] and a[1] == b[1], f"{what}: {a[:2]} and {b[:2]}"
    assert all(np.array_equal(x, y) for x, y in zip(a[2], b[2])), f"{what}: apply"
    assert np.array_equal(a[3], b[3]), f"{what}: apply_multi"


@pytest.mark.parametrize("name,vset,spec", (("grid", "x0.7", 4096), ("grid", "x0.7", "rows1"), ("n129", "sym1e-2", 4096), ("n129", "x0.7", 128)))
def test_an_update_of_a_folded_hierarchy_is_create_and_set_fold(eng, name, vset, spec):
    assert uc.same_structure(name, vset)
    n, v1, v2 = ac.case(name)[3], ac.case(name)[2], uc.values(name, vset)
    fold_rows = fo.fold_rows_of(name, spec)
    for dtype in DTYPES:
        what = f"{name} {vset} fold {fold_rows} {np.dtype(dtype).name}"
        N = amg(eng, name, dtype, values=v2)
        N.set_fold(fold_rows)
        want = _snapshot(N, n)
        N.close()
        N = amg(eng, name, dtype)
        N.set_fold(fold_rows)
        first = _snapshot(N, n)
        N.close()
        # set_fold, prepare, update
        M = amg(eng, name, dtype)
        M.set_fold(fold_rows)
        M.update_values_prepare()
        M.update_values(v2)
        _same_snapshot(_snapshot(M, n), want, what + ": set_fold before prepare")
        # the tail is the reference over the updated hierarchy
        f = M.fold_info()["first_level"]
        tail = fo.Tail(fo.hierarchy_of(M), dtype, f, **ac.options(name))
        v = ac.vectors(M.info()["rows"][f])[0].astype(dtype)
        assert np.array_equal(M.apply_level(f, v), tail.apply(v)), what + ": apply_level after the update"
        M.update_values(v1)
        _same_snapshot(_snapshot(M, n), first, what + ": back to V1")
        M.close()
        # prepare, set_fold, update; and set_fold again after the update, from the values the update left on the device
        M = amg(eng, name, dtype)
        M.update_values_prepare()
        M.set_fold(fold_rows)
        M.update_values(v2)
        _same_snapshot(_snapshot(M, n), want, what + ": set_fold after prepare")
        M.set_fold(0)
        M.set_fold(fold_rows)
        _same_snapshot(_snapshot(M, n), want, what + ": set_fold after the update")
        M.close()


def test_a_pivot_that_fails_and_comes_back_is_followed(eng):
    rp, ci = [0, 2, 4], [0, 1, 0, 1]
    good, bad = np.array([2.0, 1.0, 1.0, 2.0]), np.array([1.0, 2.0, 2.0, 1.0])
    for dtype in DTYPES:
        one = np.ones(2, dtype)
        M = eng.Amg(rp, ci, good, 2, dtype=dtype)
        M.set_fold(16)
        created = (M.info()["coarse_kind"], M.info()["launches_per_apply"], M.fold_info()["tail_products"], M.apply(one))
        assert created[:3] == (0, 1, 0)
        M.update_values_prepare()
        M.update_values(bad)
        S = eng.Amg(rp, ci, bad, 2, dtype=dtype)
        S.set_fold(16)
        assert M.info()["coarse_kind"] == 2 == S.info()["coarse_kind"] and M.fold_info() == S.fold_info()
        assert (M.info()["launches_per_apply"], M.fold_info()["tail_products"]) == (1, 3)
        got = M.apply(one)
        hier = dict(lev=[dict(n=2, A=(np.array(rp, np.int32), np.array(ci, np.int32), bad), P=None, aggregates=0, omega=M.info()["omega"][0])])
        tail = fo.Tail(hier, dtype, 0)
        assert not tail.dense and np.all(np.isfinite(got)) and np.array_equal(got, S.apply(one)) and np.array_equal(got, tail.apply(one))
        S.close()
        M.update_values(good)
        assert (M.info()["coarse_kind"], M.info()["launches_per_apply"], M.fold_info()["tail_products"]) == created[:3]
        assert np.array_equal(M.apply(one), created[3])
        M.close()


# ---- 8. refusals ---------------------------------------------------------------------------------------------------------------------------

def test_refusals_in_their_order(eng):
    import torch
    L = eng.lib()
    M = amg(eng, "grid")
    t = torch.zeros(2025, dtype=torch.float64, device="cuda")
    p = t.data_ptr()
    err = lambda: L.spmv_mi355x_last_error()
    # NULL M before anything else
    assert L.spmv_mi355x_amg_set_fold(None, 70000) == 1 and err().startswith(b"amg_set_fold: NULL handle")
    assert L.spmv_mi355x_amg_apply_level_device_async(None, 99, None, None, None) == 1 and err().startswith(b"amg_apply_level: NULL handle")
    # fold_rows outside 0..65536
    for bad in (-1, 65537):
        assert L.spmv_mi355x_amg_set_fold(M.h, bad) == 1 and err().startswith(b"amg_set_fold: fold_rows = ") and b"0..65536" in err()
    assert M.fold_info()["fold_rows"] == 0
    M.set_fold(65536)
    assert M.fold_info()["first_level"] == 0
    # a level outside 0..levels-1 before NULL in or out
    for level in (-1, 3):
        assert L.spmv_mi355x_amg_apply_level_device_async(M.h, level, None, None, None) == 1
        assert err().startswith(b"amg_apply_level: level ") and b"out of range" in err()
    for a, b, names in ((None, p, (b" in",)), (p, None, (b" out",)), (None, None, (b" in", b" out"))):
        assert L.spmv_mi355x_amg_apply_level_device_async(M.h, 1, a, b, None) == 1
        assert err().startswith(b"amg_apply_level: NULL argument") and all(nm in err() for nm in names), err()
    # a hierarchy whose last update failed: before the level and the pointers
    v2, level = uc.coarse_failure_values()
    M.update_values_prepare()
    with pytest.raises(eng.SpmvError, match="amg_update_values"):
        M.update_values(v2)
    assert M.update_values_state() == 3
    assert L.spmv_mi355x_amg_set_fold(M.h, 0) == 1 and err().startswith(b"amg_set_fold: the last amg_update_values"), err()
    assert L.spmv_mi355x_amg_set_fold(M.h, -1) == 1 and err().startswith(b"amg_set_fold: fold_rows = ")
    assert L.spmv_mi355x_amg_apply_level_device_async(M.h, 99, None, None, None) == 1
    assert err().startswith(b"amg_apply_level: the last amg_update_values"), err()
    with pytest.raises(eng.SpmvError, match="amg_apply: the last amg_update_values"):
        M.apply(np.ones(2025))
    M.update_values(ac.case("grid")[2])
    assert M.update_values_state() == 2 and M.fold_info()["first_level"] == 0
    tail = fo.tail_of("grid", np.float64, 0)
    v = ac.vectors(2025)[0]
    assert np.array_equal(M.apply(v), tail.apply(v))
    info = eng.AmgFoldStats()
    assert L.spmv_mi355x_amg_fold_info(M.h, ctypes.byref(info)) == 1 and err().startswith(b"amg_fold_info: info->struct_size not set")
    assert L.spmv_mi355x_amg_fold_info(M.h, None) == 1 and err().startswith(b"amg_fold_info: NULL info")
    info.struct_size = 16
    assert L.spmv_mi355x_amg_fold_info(M.h, ctypes.byref(info)) == 0 and (info.struct_size, info.fold_rows, info.launches_per_apply) == (16, 65536, 0)
    M.close()
