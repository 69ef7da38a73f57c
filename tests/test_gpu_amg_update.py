"""New values for an AMG hierarchy on the GPU (include/spmv_mi355x.h "AMG: new values for a hierarchy"): spmv_mi355x_amg_update_* /
Amg.update_values*. Every test here needs the new symbols, so none of them passes without the feature.

1. Same structure. Where tests/amg_reference.c finds the same levels and aggregates from V2 as from V1 (computed, else the test skips;
   no case of amg_update_cases.SAME_STRUCTURE skips), create(V1) -> prepare -> update(V2) is create(V2) to the bit: level_csr of A and P
   on every level, omega, rho, apply, the launch counts, every handle's product, pcg_tri in x, history and info; the level-0 handle
   keeps its pointer; an update back to V1 restores create(V1)'s bits.
2. Frozen. Where the aggregates of V2 differ, every level's A, P, omega and rho equal tests/amg_update_reference.c bit for bit, the
   levels, rows, aggregates and patterns are V1's, CG takes the pinned frozen count within 1, and update_values_device from a torch
   tensor gives the host form's bits.
3. The dense factor alone, the pivot that fails and comes back, path_wrap at 262 181 rows (a second trip of the row loops of
   amg_diag_check_kernel and amg_weights_kernel), and the protocol with its refusals in their order.
Every refusal here is a checked return code."""
import numpy as np
import pytest

import amg_cases as ac
import amg_update_cases as uc
import pcg_tri_cases as pc
from pcg_tri_cases import MAX_ITERATIONS

pytestmark = pytest.mark.gpu

DELTA = dict(sell_c=64, sell_delta=1, sell_sigma=64, sell_window=2)
LAYOUTS = [("sell_c_sigma", {}), ("csr_vector", {}), ("sell_c_sigma", DELTA)]
INFO_FIELDS = ("iterations", "stop", "rnorm", "rnorm0", "prnorm", "xnorm")
FROZEN_INFO = ("levels", "stalled", "rows", "nnz", "nnz_p", "aggregates")
VALUE_INFO = ("omega", "rho", "coarse_kind", "spmvs_per_apply", "launches_per_apply")


@pytest.fixture(scope="module")
def eng():
    import spmv_mi355x as eng
    assert eng.device_count() >= 1, "no GPU visible: the -m gpu tests need an MI355X"
    for sym in ("spmv_mi355x_amg_update_values_prepare", "spmv_mi355x_amg_update_values_device"):
        assert hasattr(eng.lib(), sym)
    return eng


def amg(eng, name, dtype=np.float64, fmt="sell_c_sigma", values=None, **opts):
    rp, ci, va, n, own = ac.case(name)
    return eng.Amg(rp, ci, va if values is None else values, n, fmt, dtype, **own, **opts)


def rhs(n):
    return np.random.default_rng(3).uniform(-1, 1, n)


def snapshot(M, n, solve=True):
    """everything of a hierarchy that depends on its values"""
    info = M.info()
    out = dict(info={k: info[k] for k in FROZEN_INFO + VALUE_INFO}, csr={}, apply=[], products=[])
    for l in range(info["levels"]):
        out["csr"][l, "A"] = M.level_csr(l, "A")
        if info["nnz_p"][l]:
            out["csr"][l, "P"] = M.level_csr(l, "P")
        for H in M.level_matrices(l):
            if H is not None:
                out["products"].append((H.format_name, H.mem_footprint, H.spmv(np.random.default_rng(17 + l).uniform(-1, 1, H.n).astype(M.dtype))))
    for v in ac.vectors(n):
        out["apply"].append(M.apply(v.astype(M.dtype)))
    if solve and n:
        tol = pc.PREC[M.dtype.type]["tol"]
        out["solve"] = M.A.pcg_tri(rhs(n).astype(M.dtype), precond=M, tol=tol, max_iterations=MAX_ITERATIONS)
    return out


def assert_same(a, b, what, values_only=False):
    for k in VALUE_INFO if values_only else FROZEN_INFO + VALUE_INFO:
        assert a["info"][k] == b["info"][k], f"{what}: {k}: {a['info'][k]!r} and {b['info'][k]!r}"
    assert a["csr"].keys() == b["csr"].keys(), what
    for key in a["csr"]:
        for x, y, part in zip(a["csr"][key], b["csr"][key], ("row_ptr", "col_idx", "values")):
            diff = np.nonzero(x != y)[0] if x.shape == y.shape else [-1]
            assert len(diff) == 0, f"{what}: {part} of {key[1]}_{key[0]} differ at {diff[0]}"
    for x, y in zip(a["apply"], b["apply"]):
        assert np.array_equal(x, y), f"{what}: apply"
    assert len(a["products"]) == len(b["products"])
    for (fa, ma, ya), (fb, mb, yb) in zip(a["products"], b["products"]):
        assert (fa, ma) == (fb, mb) and np.array_equal(ya, yb), f"{what}: a handle ({fa}, {fb})"
    if "solve" in a and "solve" in b:
        for k in INFO_FIELDS:
            assert a["solve"][k] == b["solve"][k], f"{what}: pcg_tri: {k}: {a['solve'][k]!r} and {b['solve'][k]!r}"
        assert np.array_equal(a["solve"]["x"], b["solve"]["x"]) and np.array_equal(a["solve"]["history"], b["solve"]["history"]), what


def assert_is_reference(M, ref, what):
    info = M.info()
    assert info["levels"] == ref["levels"] and info["stalled"] == ref["stalled"] and info["rows"] == [L["n"] for L in ref["lev"]], what
    assert info["omega"] == [L["omega"] for L in ref["lev"]] and info["rho"] == [L["rho"] for L in ref["lev"]], what
    for l, L in enumerate(ref["lev"]):
        assert np.array_equal(M.aggregates(l), L["agg"]), f"{what}: the aggregates of level {l}"
        for which in ("A", "P"):
            if L[which] is None:
                assert info["nnz_p"][l] == 0
                continue
            rp, ci, va = M.level_csr(l, which)
            assert np.array_equal(rp, L[which][0]) and np.array_equal(ci, L[which][1]), f"{what}: the pattern of {which}_{l}"
            diff = np.nonzero(va != L[which][2])[0]
            assert len(diff) == 0, f"{what}: {which}_{l}: entry {diff[0]} is {va[diff[0]]!r}, the reference has {L[which][2][diff[0]]!r}"


# ---- 1. same structure -----------------------------------------------------------------------------------------------------------------

SAME = [(name, vset, fmt, opts) for name, vset in uc.SAME_STRUCTURE for fmt, opts in (LAYOUTS if name == "grid" else LAYOUTS[:1])]


@pytest.mark.parametrize("name,vset,fmt,opts", SAME, ids=[f"{n}-{v}-{f}{'-delta' if o else ''}" for n, v, f, o in SAME])
def test_an_update_is_create_on_the_new_values(eng, name, vset, fmt, opts):
    if not uc.same_structure(name, vset):
        pytest.skip(f"{name}, {vset}: tests/amg_reference.c finds other aggregates from V2")
    n = ac.case(name)[3]
    v2 = uc.values(name, vset)
    for dtype in (np.float64, np.float32):
        what = f"{name} {vset} {fmt} {np.dtype(dtype).name}"
        M = amg(eng, name, dtype, fmt, **opts)
        first, seconds = snapshot(M, n), M.info()["setup_seconds"]
        pointer = M.level_matrices(0)[0].h.value
        assert M.update_values_state() == 1
        M.update_values_prepare()
        assert M.update_values_state() == 2 and M.update_info()["prepared"] == 1 and M.update_info()["prepare_bytes"] > 0
        M.update_values(v2)
        assert M.update_values_state() == 2 and M.update_info()["updates"] == 1
        N = amg(eng, name, dtype, fmt, values=v2, **opts)
        want = snapshot(N, n)
        assert_same(snapshot(M, n), want, what)
        assert M.level_matrices(0)[0].h.value == pointer, "the level-0 handle stays the lent one"
        own = eng.Matrix(*ac.case(name)[:2], v2, n, n, fmt, dtype, **opts)
        x = rhs(n).astype(dtype)
        assert np.array_equal(M.A.spmv(x), own.spmv(x)), f"{what}: the level-0 handle holds V2"
        own.close()
        assert M.info()["setup_seconds"] == seconds and all(np.array_equal(M.aggregates(l), N.aggregates(l)) for l in range(M.levels))
        N.close()
        M.update_values(ac.case(name)[2])
        assert_same(snapshot(M, n), first, what + ": back to V1")
        M.close()


# ---- 2. frozen ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,vset", uc.FROZEN_CASES)
def test_a_frozen_hierarchy_is_the_frozen_reference(eng, name, vset):
    import torch
    rp, ci, va, n, _ = ac.case(name)
    v2 = uc.values(name, vset)
    ref, first = uc.frozen_of(name, vset), ac.reference_of(name)
    for dtype in (np.float64, np.float32):
        what = f"{name} {vset} {np.dtype(dtype).name}"
        M = amg(eng, name, dtype)
        before = M.info()
        M.update_values_prepare()
        M.update_values(v2)
        info = M.info()
        for k in FROZEN_INFO + ("mis_rounds", "setup_seconds"):
            assert info[k] == before[k], f"{what}: {k}"
        assert info["levels"] == first["levels"] == (3 if name == "grid" else info["levels"])
        assert_is_reference(M, ref, what)
        for l, L in enumerate(first["lev"]):
            assert np.array_equal(M.aggregates(l), L["agg"])
        host = snapshot(M, n, solve=False)
        if name == "grid":
            # the project's own b: the count of the restated frozen hierarchy within 1
            b = pc.problem().b.astype(dtype)
            got = M.A.pcg_tri(b, precond=M, tol=pc.PREC[dtype]["tol"], max_iterations=MAX_ITERATIONS)
            print(f"[amg update] {what}: {got['iterations']} iterations, the restatement's frozen count in fp64 is {uc.FROZEN_COUNTS[vset][1]}")
            assert got["stop"] == 1
            if dtype == np.float64:
                assert abs(got["iterations"] - uc.FROZEN_COUNTS[vset][1]) <= 1, what
        # the device form from a torch tensor, after an update to something else in between
        M.update_values(0.7 * va)
        t = torch.from_numpy(np.array(v2)).cuda()
        M.update_values_device(t.data_ptr())
        assert_same(snapshot(M, n, solve=False), host, what + ": update_values_device")
        M.close()


# ---- 3. the dense factor alone -----------------------------------------------------------------------------------------------------------

def _scaled(rp, ci, va, n, eps):
    s = 1 + eps * np.random.default_rng(5).uniform(-1, 1, n)
    rows = np.repeat(np.arange(n), np.diff(rp))
    return va * (s[rows] * s[ci])


@pytest.mark.parametrize("name", ("n128", "grid_last", "one"))
def test_the_dense_factor_alone(eng, name):
    """a hierarchy of one dense level: after an update, apply is L^-t L^-1 of the reference's factor of V2, bit for bit"""
    if name == "grid_last":
        L = ac.reference_of("grid")["lev"][-1]
        (rp, ci, va), n = L["A"], L["n"]
        assert n == 43
    else:
        rp, ci, va, n, _ = ac.case(name)
    for dtype in (np.float64, np.float32):
        M = eng.Amg(rp, ci, va, n, dtype=dtype)
        M.update_values_prepare()
        for v2 in (0.7 * va, _scaled(rp, ci, va, n, 0.01), va):
            M.update_values(v2)
            info = M.info()
            assert (M.levels, info["coarse"], info["launches_per_apply"], info["spmvs_per_apply"]) == (1, "dense", 1, 0)
            F = ac.reference_factor(rp, ci, v2, n)
            for v in ac.vectors(n):
                v = v.astype(dtype)
                want = ac.reference_dense_solve(F, v.astype(np.float64)).astype(dtype)
                got = M.apply(v)
                assert np.array_equal(got, want), f"{name} {np.dtype(dtype).name}: {np.nonzero(got != want)[0][:4]}"
        M.close()


def test_a_pivot_that_fails_and_comes_back(eng):
    rp, ci = [0, 2, 4], [0, 1, 0, 1]
    good, bad = np.array([2.0, 1.0, 1.0, 2.0]), np.array([1.0, 2.0, 2.0, 1.0])
    M = eng.Amg(rp, ci, good, 2)
    created = (M.info()["coarse_kind"], M.info()["spmvs_per_apply"], M.info()["launches_per_apply"], M.apply(np.ones(2)))
    assert created[:3] == (0, 0, 1)
    M.update_values_prepare()
    M.update_values(bad)
    info = M.info()
    S = eng.Amg(rp, ci, bad, 2)
    assert info["coarse"] == "sweeps after a failed pivot" and info["coarse_kind"] == 2 == S.info()["coarse_kind"]
    assert (info["spmvs_per_apply"], info["launches_per_apply"]) == (3, 7) == (S.info()["spmvs_per_apply"], S.info()["launches_per_apply"])
    got = M.apply(np.ones(2))
    assert np.all(np.isfinite(got)) and np.array_equal(got, S.apply(np.ones(2))) and M.update_values_state() == 2
    S.close()
    M.update_values(good)
    info = M.info()
    assert (info["coarse_kind"], info["spmvs_per_apply"], info["launches_per_apply"]) == created[:3]
    assert np.array_equal(M.apply(np.ones(2)), created[3])
    M.close()


# ---- 4. second trips -----------------------------------------------------------------------------------------------------------------------

def test_path_wrap_takes_second_trips(eng):
    """262 181 rows: the first workgroup of amg_diag_check_kernel and amg_weights_kernel walks a second trip of its row loop"""
    name, vset = "path_wrap", "path9"
    n = ac.case(name)[3]
    assert n == 256 * 1024 + 37
    M = amg(eng, name)
    M.update_values_prepare()
    M.update_values(uc.values(name, vset))
    assert_is_reference(M, uc.frozen_of(name, vset), "path_wrap, path9")
    got = M.apply(ac.vectors(n)[0])
    assert np.all(np.isfinite(got))
    if uc.same_structure(name, vset):
        N = amg(eng, name, values=uc.values(name, vset))
        assert np.array_equal(got, N.apply(ac.vectors(n)[0]))
        N.close()
    M.close()


# ---- 5. the protocol and the refusals ------------------------------------------------------------------------------------------------------

def test_the_protocol_and_the_refusals_in_their_order(eng):
    rp, ci, va, n, _ = ac.case("grid")
    rows = np.repeat(np.arange(n), np.diff(rp))
    M = amg(eng, "grid")
    v = ac.vectors(n)[0]
    before = M.apply(v)
    # update before prepare
    assert M.update_values_state() == 1
    with pytest.raises(eng.SpmvError, match=r"^amg_update_values: .*amg_update_values_prepare has not been called"):
        M.update_values(0.7 * va)
    assert np.array_equal(M.apply(v), before)
    M.update_values_prepare()
    assert M.update_values_state() == 2
    M.update_values_prepare()                                          # a second call does nothing
    kept = M.update_info()["prepare_bytes"]
    assert kept > 0 and M.update_info()["prepare_seconds"] > 0 and M.mem_footprint == eng.lib().spmv_mi355x_amg_mem_footprint(M.h)
    # NULL values under a live handle
    assert eng.lib().spmv_mi355x_amg_update_values(M.h, None) == 1
    assert eng.lib().spmv_mi355x_last_error().startswith(b"amg_update_values: NULL values")
    assert eng.lib().spmv_mi355x_amg_update_values_device(M.h, None, None) == 1
    assert eng.lib().spmv_mi355x_last_error().startswith(b"amg_update_values: NULL values")
    # a zero diagonal at row 7 of level 0: refused with the row named, nothing written
    zero = va.copy()
    zero[np.nonzero((rows == 7) & (ci == 7))[0][0]] = 0.0
    with pytest.raises(eng.SpmvError, match=r"^amg_update_values: the diagonal of row 7 of level 0 is 0"):
        M.update_values(zero)
    assert M.update_values_state() == 2 and np.array_equal(M.apply(v), before) and M.update_info()["updates"] == 0
    for l in range(M.levels):
        assert np.array_equal(M.level_csr(l, "A")[2], ac.reference_of("grid")["lev"][l]["A"][2])
    # a coarse diagonal that is not positive: the finer levels are rewritten, state 3, apply and pcg_amg refuse until an update succeeds
    v2, level = uc.coarse_failure_values()
    assert level == 1
    with pytest.raises(eng.SpmvError, match=r"^amg_update_values: the diagonal of row \d+ of level 1 is "):
        M.update_values(v2)
    assert M.update_values_state() == 3 and M.update_info()["failed"] == 1
    with pytest.raises(eng.SpmvError, match=r"^amg_apply: the last amg_update_values .* failed"):
        M.apply(v)
    with pytest.raises(eng.SpmvError, match=r"^pcg_amg: the last amg_update_values of M failed"):
        M.A.pcg_tri(rhs(n), precond=M)
    with pytest.raises(eng.SpmvError, match=r"level 0"):
        M.update_values(zero)                                          # a refusal at level 0 does not heal it
    assert M.update_values_state() == 3
    M.update_values(va)
    assert M.update_values_state() == 2 and M.update_info()["failed"] == 0 and np.array_equal(M.apply(v), before)
    M.close()


def test_a_unit_handle_is_refused_by_prepare(eng):
    """csr_merge drops a uniform value stream (a _unit handle), which takes no update: prepare names the level and the reason"""
    n = 300
    rp = np.arange(n + 1, dtype=np.int32)
    ci = np.arange(n, dtype=np.int32)
    M = eng.Amg(rp, ci, np.full(n, 2.0), n, "csr_merge", coarse_rows=128, max_levels=1)
    assert M.levels == 1 and "unit" in M.A.format_name
    before = M.apply(np.ones(n))
    assert M.update_values_state() == 0
    with pytest.raises(eng.SpmvError, match=r"^amg_update_values_prepare: level 0: A: .*uniform"):
        M.update_values_prepare()
    with pytest.raises(eng.SpmvError, match=r"^amg_update_values: level 0: A: .*uniform"):
        M.update_values(np.full(n, 3.0))
    assert M.update_info()["prepared"] == 0 and np.array_equal(M.apply(np.ones(n)), before)
    M.close()


def test_empty_prepares_and_updates_as_no_ops(eng):
    M = amg(eng, "empty")
    assert M.update_values_state() == 1
    M.update_values_prepare()
    assert M.update_values_state() == 2
    M.update_values(np.zeros(0))
    M.update_values_device(0)
    assert M.levels == 0 and M.apply(np.zeros(0)).shape == (0,) and M.update_info()["updates"] == 0
    M.close()
