"""spmv_mi355x_amg_create_with on the GPU (include/spmv_mi355x.h "AMG: a caller's near-null vector and filtered prolongator
smoothing"): Amg.build, Amg.prolongator_info, Amg.near_null, level_csr(l, "AF"). Every test here needs the new symbols, so none of
them passes without the feature.

1. The hierarchy. On every case and variant of amg_prolongator_cases.py, for fp64 and fp32 handles (the setup is fp64 either way) and
   on `grid` in two formats: levels, rows, aggregates, the patterns and fp64 values of A_l, A_F and P_l, b_l, omega, rho, omega_p,
   rho_p, nnz_filtered and unfiltered_rows equal tests/amg_prolongator_reference.c with np.array_equal. path_wrap (262 181 rows) sends
   the first workgroup of every new kernel into a second trip and ends in a dense last level of 47 rows; hub's row 0 falls back.
2. Defaults. Amg.build without options, and amg_create_with given NULL, against Amg / amg_create: equal infos (launches_per_apply
   included), aggregates, level_csr, handles and apply.
3. The cycle: apply against the same cycle driven through the borrowed handles, bit for bit, and within
   amg_prolongator_cases.CYCLE_BOUND of the scipy restatement. pcg_amg on path_wrap with its near-null vector against the restatement
   by the rule of test_gpu_amg.py::test_path_wrap_at_1e_8; the recorded count is at most 38. Frozen after the stop.
4. New values: ("grid", "x0.7") and ("aniso", "x0.7"), filtered with near-null, equal a fresh amg_create_with bit for bit; a sym0.5
   pair equals the reference's update loops (which of the two rules applies is computed here); a value that drives a filtered row's
   lumped diagonal below 0 on level 0 leaves the hierarchy untouched.
5. The refusals on the device, in their order.

THE 1e-160 OF THE ISSUE. An aggregate whose members all hold 1e-160 has s = k * 1e-320, a positive subnormal, and nrm = sqrt(s) near
1e-160: positive and finite, so the stated rule (a norm that is not a positive finite number) accepts it, and the hierarchy must
still equal the reference bit for bit, which is asserted. b * b underflows to 0 from about 1.5e-162 on: an aggregate of 1e-170 is
the refusal, and one of 1e200 the overflow."""
import ctypes

import numpy as np
import pytest

import amg_cases as ac
import amg_prolongator_cases as apc
import pcg_tri_cases as pc
from pcg_tri_cases import MAX_ITERATIONS, POLL

pytestmark = pytest.mark.gpu

INFO_FIELDS = ("iterations", "stop", "rnorm", "rnorm0", "prnorm", "xnorm")
SECONDS = ("setup_seconds", "coarsen_seconds", "spgemm_seconds", "transpose_seconds", "create_seconds", "download_seconds")


@pytest.fixture(scope="module")
def eng():
    import spmv_mi355x as eng
    assert eng.device_count() >= 1, "no GPU visible: the -m gpu tests need an MI355X"
    for sym in ("spmv_mi355x_amg_create_with", "spmv_mi355x_amg_prolongator_info", "spmv_mi355x_amg_near_null"):
        assert hasattr(eng.lib(), sym)
    return eng


def build(eng, name, variant, dtype=np.float64, fmt="sell_c_sigma", values=None, near_null="case", **opts):
    rp, ci, va, n, own, nn, filtered = apc.case(name, variant)
    return eng.Amg.build(rp, ci, va if values is None else values, n, nn if isinstance(near_null, str) else near_null, filtered, fmt, dtype,
                         **own, **opts)


def assert_is_reference(M, ref, what):
    info, pinfo = M.info(), M.prolongator_info()
    assert info["levels"] == ref["levels"] and info["stalled"] == ref["stalled"] and info["rows"] == [L["n"] for L in ref["lev"]], what
    assert info["aggregates"] == [L["aggregates"] for L in ref["lev"]] and info["mis_rounds"] == [L["rounds"] for L in ref["lev"]], what
    assert info["omega"] == [L["omega"] for L in ref["lev"]] and info["rho"] == [L["rho"] for L in ref["lev"]], what
    assert (pinfo["filtered"], pinfo["has_near_null"]) == (ref["filtered"], ref["has_nn"]), what
    for k, r in (("omega_p", "omega_p"), ("rho_p", "rho_p"), ("nnz_filtered", "nnz_f"), ("unfiltered_rows", "unfiltered_rows")):
        assert pinfo[k] == [L[r] for L in ref["lev"]], f"{what}: {k}: {pinfo[k]} and {[L[r] for L in ref['lev']]}"
    for l, L in enumerate(ref["lev"]):
        assert np.array_equal(M.aggregates(l), L["agg"]), f"{what}: the aggregates of level {l}"
        assert np.array_equal(M.near_null(l), L["b"]), f"{what}: b_{l}"
        for which in ("A", "AF", "P"):
            if L[which] is None:
                continue
            rp, ci, va = M.level_csr(l, which)
            assert np.array_equal(rp, L[which][0]) and np.array_equal(ci, L[which][1]), f"{what}: the pattern of {which}_{l}"
            diff = np.nonzero(va != L[which][2])[0]
            assert len(diff) == 0, f"{what}: {which}_{l}: entry {diff[0]} is {va[diff[0]]!r}, the reference has {L[which][2][diff[0]]!r}"
        if L["P"] is None:
            assert info["nnz_p"][l] == 0


# ---- 1. the hierarchy --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,variant", apc.CASES, ids=[f"{n}-{v}" for n, v in apc.CASES])
def test_the_hierarchy_is_the_references_bit_for_bit(eng, name, variant):
    ref = apc.reference_of(name, variant)
    n = apc.base(name)[3]
    for dtype in (np.float64, np.float32):
        for fmt in ("sell_c_sigma", "csr_vector") if name == "grid" else ("sell_c_sigma",):
            what = f"{name} {variant} {np.dtype(dtype).name} {fmt}"
            M = build(eng, name, variant, dtype, fmt)
            info, pinfo = M.info(), M.prolongator_info()
            print(f"[amg prolongator] {what}: rows {info['rows']}, coarse {info['coarse']}, entries per row "
                  f"{[round(z / max(r, 1), 1) for z, r in zip(info['nnz'], info['rows'])]}, filtered {pinfo['nnz_filtered']}, unfiltered rows "
                  f"{pinfo['unfiltered_rows']}, setup {info['setup_seconds']:.3g} s")
            assert_is_reference(M, ref, what)
            if n == 0:
                assert M.A is None and M.apply(np.zeros(0, dtype)).shape == (0,)
            else:
                dense = ref["lev"][-1]["n"] <= 128
                nl = ref["levels"]
                assert info["coarse"] == ("dense" if dense else "sweeps") and M.A.m == n and M.A.dtype == dtype
                assert info["spmvs_per_apply"] == (nl - 1) * 4 + (0 if dense else 3)
                assert info["launches_per_apply"] == info["spmvs_per_apply"] + (nl - 1) * 3 + (1 if dense else 4)
            M.close()
            M.close()


def test_path_wrap_ends_in_a_dense_level_and_hub_falls_back(eng):
    M = build(eng, "path_wrap", "nn")
    info = M.info()
    assert info["rows"] == apc.PATH_NN_ROWS and (info["stalled"], info["coarse"]) == (0, "dense")
    assert all(z <= 3 * r for z, r in zip(info["nnz"], info["rows"])), "every level stays a path"
    M.close()
    M = build(eng, "hub", "filtered")
    assert M.prolongator_info()["unfiltered_rows"][0] >= 1
    rp, _, _ = M.level_csr(0, "AF")
    assert rp[1] - rp[0] == apc.HUB_COUPLED + 3, "row 0 keeps all its entries"
    M.close()


# ---- 2. defaults -------------------------------------------------------------------------------------------------------------------------

def _everything(M, n):
    info = M.info()
    out = dict(info={k: v for k, v in info.items() if k not in SECONDS}, pinfo=M.prolongator_info(), csr=[], apply=[], products=[])
    for l in range(info["levels"]):
        out["csr"].append(M.level_csr(l, "A") + (M.aggregates(l), M.near_null(l)))
        if info["nnz_p"][l]:
            out["csr"].append(M.level_csr(l, "P"))
        for H in M.level_matrices(l):
            if H is not None:
                x = np.random.default_rng(17 + l).uniform(-1, 1, H.n).astype(M.dtype)
                out["products"].append((H.format_name, H.mem_footprint, H.spmv(x)))
    for v in ac.vectors(n):
        out["apply"].append(M.apply(v.astype(M.dtype)))
    return out


def _assert_equal(a, b, what):
    assert a["info"] == b["info"], f"{what}: {a['info']} and {b['info']}"
    assert a["pinfo"] == b["pinfo"], what
    assert len(a["csr"]) == len(b["csr"]) and all(np.array_equal(x, y) for s, t in zip(a["csr"], b["csr"]) for x, y in zip(s, t)), what
    assert all(np.array_equal(x, y) for x, y in zip(a["apply"], b["apply"])), f"{what}: apply"
    assert len(a["products"]) == len(b["products"])
    for (fa, ma, ya), (fb, mb, yb) in zip(a["products"], b["products"]):
        assert (fa, ma) == (fb, mb) and np.array_equal(ya, yb), f"{what}: a handle"


@pytest.mark.parametrize("name", ("grid", "aniso", "grid_weak", "n129", "one", "empty"))
def test_defaults_are_amg_create(eng, name):
    rp, ci, va, n, own = ac.case(name)
    for dtype in (np.float64, np.float32):
        for fmt in ("sell_c_sigma", "csr_vector") if name == "grid" else ("sell_c_sigma",):
            a = eng.Amg(rp, ci, va, n, fmt, dtype, **own)
            b = eng.Amg.build(rp, ci, va, n, None, False, fmt, dtype, **own)
            what = f"{name} {np.dtype(dtype).name} {fmt}"
            A, B = _everything(a, n), _everything(b, n)
            _assert_equal(A, B, what)
            assert B["pinfo"]["filtered"] == 0 and B["pinfo"]["has_near_null"] == 0 and b.near_null(0).size == 0 if n else True
            for l in range(a.levels):
                if A["info"]["nnz_p"][l]:
                    assert (B["pinfo"]["nnz_filtered"][l], B["pinfo"]["omega_p"][l], B["pinfo"]["rho_p"][l]) == \
                        (A["info"]["nnz"][l], A["info"]["omega"][l], A["info"]["rho"][l])
            if n:
                with pytest.raises(eng.SpmvError, match=r"amg_level_csr: .*filtered = 0"):
                    b.level_csr(0, "AF")
            a.close()
            b.close()


def test_a_null_prolongator_opts_is_amg_create(eng):
    rp, ci, va, n, _ = ac.case("grid")
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    arrs = [np.ascontiguousarray(a, t) for a, t in ((rp, np.int32), (ci, np.int32), (va, np.float64))]
    h = ctypes.c_void_p()
    rc = eng.lib().spmv_mi355x_amg_create_with(ctypes.byref(h), eng.FORMATS["sell_c_sigma"], 0, ctypes.c_long(n), *[p(a) for a in arrs], None,
                                               None, None)
    assert rc == 0, eng.lib().spmv_mi355x_last_error()
    M = eng.Amg(rp, ci, va, n)
    s = eng.AmgStats()
    s.struct_size = ctypes.sizeof(s)
    assert eng.lib().spmv_mi355x_amg_info(h, ctypes.byref(s)) == 0
    info = M.info()
    assert (s.levels, s.launches_per_apply, s.spmvs_per_apply, list(s.rows)[:s.levels], list(s.omega)[:s.levels]) == \
        (info["levels"], info["launches_per_apply"], info["spmvs_per_apply"], info["rows"], info["omega"])
    v = np.ascontiguousarray(ac.vectors(n)[0])
    out = np.zeros(n)
    assert eng.lib().spmv_mi355x_amg_apply(h, p(v), p(out)) == 0 and np.array_equal(out, M.apply(v))
    for l in range(info["levels"] - 1):
        va_l = np.zeros(info["nnz_p"][l])
        assert eng.lib().spmv_mi355x_amg_level_csr(h, l, eng.AMG_P, None, None, p(va_l)) == 0 and np.array_equal(va_l, M.level_csr(l, "P")[2])
    eng.lib().spmv_mi355x_amg_destroy(h)
    M.close()


# ---- 3. the cycle and the solver -------------------------------------------------------------------------------------------------------

def python_cycle(M, ref, opts, v):
    """test_gpu_amg.py's: the header's cycle through the borrowed handles, the elementwise steps in numpy, the dense last level by the C
    reference. The weights are step 1's omega / d of the unfiltered A_l."""
    import torch
    dtype = M.dtype.type
    nu, cs, nl = opts["sweeps"], opts["coarse_sweeps"], M.levels
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()

    def product(H, x, y0=None):
        xd = dev(x)
        yd = torch.zeros(H.m, dtype=xd.dtype, device="cuda") if y0 is None else dev(y0)
        H.spmv_device(xd.data_ptr(), yd.data_ptr(), beta=0 if y0 is None else 1)
        torch.cuda.synchronize()
        return yd.cpu().numpy()

    def cycle(l, b):
        A, P, R = M.level_matrices(l)
        L = ref["lev"][l]
        rows = np.repeat(np.arange(L["n"]), np.diff(L["A"][0]))
        d = L["A"][2][rows == L["A"][1]]
        w = (L["omega"] / d).astype(dtype)
        sweep = lambda x: x + w * (b - product(A, x))
        if l == nl - 1:
            if L["n"] <= 128:
                return ac.reference_dense_solve(ac.reference_factor(*L["A"], L["n"]), b.astype(np.float64)).astype(dtype)
            x = w * b
            for _ in range(cs - 1):
                x = sweep(x)
            return x
        x = w * b
        for _ in range(nu - 1):
            x = sweep(x)
        r = b - product(A, x)
        x = product(P, cycle(l + 1, product(R, r)), y0=x)
        for _ in range(nu):
            x = sweep(x)
        return x
    return cycle(0, np.ascontiguousarray(v, dtype))


@pytest.mark.parametrize("name,variant", apc.CYCLE_CASES, ids=[f"{n}-{v}" for n, v in apc.CYCLE_CASES])
def test_apply_is_the_cycle(eng, name, variant):
    n = apc.base(name)[3]
    ref, opts = apc.reference_of(name, variant), apc.options(name)
    for dtype in (np.float64, np.float32):
        want_of = apc.cycle_restatement(name, variant, dtype)
        M = build(eng, name, variant, dtype)
        worst = 0.0
        for v in ac.vectors(n):
            v = v.astype(dtype)
            got = M.apply(v)
            assert got.dtype == dtype and np.all(np.isfinite(got))
            assert np.array_equal(got, M.apply(v)), f"{name} {variant}: twice"
            assert np.array_equal(got, python_cycle(M, ref, opts, v)), f"{name} {variant}: the cycle through the borrowed handles"
            want = want_of(v).astype(np.float64)
            worst = max(worst, float(np.abs(got.astype(np.float64) - want).max() / np.abs(want).max()))
        print(f"[amg prolongator] cycle {name} {variant} {np.dtype(dtype).name}: {worst:.3g} from the restatement, "
              f"{worst / apc.CYCLE_BOUND[dtype]:.3g} of the bound {apc.CYCLE_BOUND[dtype]:.3g}")
        assert worst <= apc.CYCLE_BOUND[dtype], f"{name} {variant} {np.dtype(dtype).name}: {worst:.3g} against {apc.CYCLE_BOUND[dtype]:.3g}"
        M.close()


def test_the_dense_last_level_of_path_wrap(eng):
    """47 rows under a near-null vector: a hierarchy of that level alone applies L^-t L^-1 of the reference's factor, bit for bit"""
    L = apc.reference_of("path_wrap", "nn")["lev"][-1]
    (rp, ci, va), n = L["A"], L["n"]
    assert n == apc.PATH_NN_ROWS[-1] <= 128
    F = ac.reference_factor(rp, ci, va, n)
    assert F is not None
    for dtype in (np.float64, np.float32):
        M = eng.Amg.build(rp, ci, va, n, L["b"], True, dtype=dtype)
        assert (M.levels, M.info()["coarse"], M.info()["launches_per_apply"]) == (1, "dense", 1) and np.array_equal(M.near_null(0), L["b"])
        for v in ac.vectors(n):
            v = v.astype(dtype)
            assert np.array_equal(M.apply(v), ac.reference_dense_solve(F, v.astype(np.float64)).astype(dtype))
        M.close()


def _same(a, b, what):
    for k in INFO_FIELDS:
        assert a[k] == b[k], f"{what}: {k}: {a[k]!r} and {b[k]!r}"
    assert np.array_equal(a["x"], b["x"]) and np.array_equal(a["history"], b["history"]), what


def test_path_wrap_with_its_near_null_vector_at_1e_8(eng):
    """the rule of test_gpu_amg.py::test_path_wrap_at_1e_8 (the count within 5 % of the restatement's), and at most half of the 76 the
    constant takes"""
    A_sp, b = ac.path_problem()
    _, ref, ref_stop = apc.path_restatement()
    assert ref_stop == 1 and ref.size == apc.PATH_NN_COUNT <= 38 == ac.PATH_COUNT // 2
    M = build(eng, "path_wrap", "nn")
    got = M.A.pcg_tri(b, precond=M, tol=ac.PATH_TOL, max_iterations=MAX_ITERATIONS)
    again = M.A.pcg_tri(b, precond=M, tol=ac.PATH_TOL, max_iterations=MAX_ITERATIONS)
    info = M.info()
    M.close()
    _same(got, again, "path_wrap")
    k = got["iterations"]
    rn = np.linalg.norm(b - A_sp @ got["x"])
    print(f"[pcg_amg] path_wrap, near_null = 1 / s: {k} iterations (the restatement {ref.size}, the constant {ac.PATH_COUNT}), "
          f"|b - A x| / |b| = {rn / np.linalg.norm(b):.3g}, rows {info['rows']}, coarse {info['coarse']}")
    assert got["stop"] == 1 and rn <= 10 * ac.PATH_TOL * np.linalg.norm(b)
    assert abs(got["rnorm"] - rn) <= 1e-6 * rn + 1e-12 * np.linalg.norm(b)
    assert abs(k - ref.size) <= 0.05 * ref.size and k <= 38, f"{k} iterations, the restatement {ref.size}"


def test_the_scaled_grid_takes_the_recorded_count(eng):
    b = pc.problem().b
    M = build(eng, "grid", "nn")
    got = M.A.pcg_tri(b, precond=M, tol=ac.PATH_TOL, max_iterations=MAX_ITERATIONS)
    M.close()
    assert got["stop"] == 1 and abs(got["iterations"] - apc.GRID_SCALED_COUNTS["nn"]) <= 1, got["iterations"]


def test_frozen_after_the_stop(eng):
    """test_gpu_amg.py's: a tol that stops at step k returns the x, the iterations and the history[:k] of the same solve with
    max_iterations = k and tol = 0"""
    b = np.ascontiguousarray(pc.problem().b)
    n = b.size
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)

    def raw(A, M, x, tol, maxit, hist):
        info = eng.PcgTriInfo()
        info.struct_size = ctypes.sizeof(eng.PcgTriInfo)
        rc = eng.lib().spmv_mi355x_pcg_amg(A.h, p(b), p(x), M.h, tol, maxit, p(hist), ctypes.byref(info))
        return rc, info
    M = build(eng, "grid", "both")
    A = M.A
    got = A.pcg_tri(b, precond=M, tol=1e-12, max_iterations=MAX_ITERATIONS)
    k = got["iterations"]
    assert got["stop"] == 1 and k < 2 * POLL
    x_long, h_long = np.full(n, 7.0), np.full(k + 200, 7.0)
    rc, long_ = raw(A, M, x_long, 1e-12, k + 200, h_long)
    assert rc == 0 and (long_.stop, long_.iterations) == (1, k)
    x_short, h_short = np.full(n, 7.0), np.full(k, 7.0)
    rc, short = raw(A, M, x_short, 0.0, k, h_short)
    assert rc == 0 and (short.stop, short.iterations) == (2, k)
    assert np.array_equal(x_long, x_short) and np.array_equal(x_long, got["x"])
    assert np.array_equal(h_long[:k], h_short) and np.array_equal(h_short, got["history"]) and np.all(h_long[k:] == 0)
    assert (long_.rnorm, long_.rnorm0, long_.prnorm, long_.xnorm) == (short.rnorm, short.rnorm0, short.prnorm, short.xnorm)
    M.close()


# ---- 4. new values -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ("grid", "aniso"))
def test_an_update_is_create_with_on_the_new_values(eng, name):
    rp, ci, va, n, _, nn, filtered = apc.case(name, "both")
    v2 = 0.7 * va
    first, fresh = apc.reference_of(name, "both"), apc.reference(rp, ci, v2, n, nn, filtered, **apc.options(name))
    assert apc.same_structure(first, fresh), "x0.7 keeps every decision: the first rule of the contract applies"
    for dtype in (np.float64, np.float32):
        what = f"{name} both x0.7 {np.dtype(dtype).name}"
        M = build(eng, name, "both", dtype)
        before = _everything(M, n)
        assert M.update_values_state() == 1
        M.update_values_prepare()
        assert M.update_values_state() == 2
        M.update_values(v2)
        assert M.update_values_state() == 2 and M.update_info()["updates"] == 1
        N = build(eng, name, "both", dtype, values=v2)
        _assert_equal(_everything(M, n), _everything(N, n), what)
        assert_is_reference(M, fresh, what)
        N.close()
        M.update_values(va)
        _assert_equal(_everything(M, n), before, what + ": back to V1")
        M.close()


def test_a_frozen_update_is_the_references_update_loops(eng):
    name = "grid"
    rp, ci, va, n, _, nn, filtered = apc.case(name, "both")
    rows = np.repeat(np.arange(n), np.diff(rp))
    s = 1 + 0.5 * np.random.default_rng(5).uniform(-1, 1, n)               # amg_update_cases' sym0.5
    v2 = va * (s[rows] * s[ci])
    first = apc.reference_of(name, "both")
    fresh, frozen = apc.reference(rp, ci, v2, n, nn, filtered, **apc.options(name)), apc.reference_update(first, v2)
    assert frozen["bad"] is None
    same = apc.same_structure(first, fresh)
    print(f"[amg prolongator] grid both sym0.5: amg_create_with on the new values finds {'the same' if same else 'another'} structure")
    if same:
        assert apc.first_difference(fresh, frozen) is None
    for dtype in (np.float64, np.float32):
        M = build(eng, name, "both", dtype)
        M.update_values_prepare()
        M.update_values(v2)
        assert_is_reference(M, frozen, f"{name} both sym0.5 {np.dtype(dtype).name}")
        assert np.all(np.isfinite(M.apply(ac.vectors(n)[0].astype(dtype))))
        M.close()


def test_a_lumped_diagonal_that_turns_negative_on_level_0_leaves_the_hierarchy_untouched(eng):
    """aniso, filtered: the two weak entries of a row of the interior (-0.01 each, lumped at create) become -1.5 each, symmetrically:
    the stored diagonal 2.03 stays, the lumped one is -0.97 on a row that was filtered at create"""
    rp, ci, va, n, _, nn, filtered = apc.case("aniso", "filtered")
    i, k = 5 * 40 + 7, 40
    v2 = va.copy()
    for a, b in ((i, i - k), (i, i + k), (i - k, i), (i + k, i)):
        e = rp[a] + int(np.nonzero(ci[rp[a]:rp[a + 1]] == b)[0][0])
        assert v2[e] == -0.01
        v2[e] = -1.5
    upd = apc.reference_update(apc.reference_of("aniso", "filtered"), v2)
    assert upd["bad"] == (0, i), "the reference's update loops find the same row"
    M = build(eng, "aniso", "filtered")
    M.update_values_prepare()
    M.update_values(0.7 * va)
    before = _everything(M, n)
    with pytest.raises(eng.SpmvError, match=rf"amg_update_values: the lumped diagonal of row {i} of level 0 .*unchanged"):
        M.update_values(v2)
    assert M.update_values_state() == 2 and M.update_info()["updates"] == 1 and M.update_info()["failed"] == 0
    _assert_equal(_everything(M, n), before, "after the refused update")
    M.close()


# ---- 5. the refusals on the device -------------------------------------------------------------------------------------------------------

def test_refusals_in_their_order(eng):
    rp, ci, va, n, _, nn, _ = apc.case("isolated", "nn")
    ref = apc.reference_of("isolated", "nn")
    agg = ref["lev"][0]["agg"]
    g = int(agg[n // 2])
    members = agg == g
    # a negative entry is a near-null vector like any other; an aggregate of 1e-160 squares to subnormals and is accepted
    tiny = nn.copy()
    tiny[::3] *= -1
    tiny[members] = 1e-160
    want = apc.reference(rp, ci, va, n, tiny, False, **apc.options("isolated"))
    assert want["bad"] is None and want["lev"][1]["b"][g] > 0
    M = build(eng, "isolated", "nn", near_null=tiny)
    assert_is_reference(M, want, "isolated, an aggregate of 1e-160")
    M.close()
    # b * b underflows to 0, or overflows: refused under item 6 with the level and the aggregate
    for value in (1e-170, -1e-170, 1e200):
        bad = tiny.copy()
        bad[members] = value
        assert apc.reference(rp, ci, va, n, bad, False, **apc.options("isolated"))["bad"] == (0, g)
        with pytest.raises(eng.SpmvError, match=rf"amg_create_with: level 0: the norm of the near-null vector over aggregate {g} is "):
            build(eng, "isolated", "nn", near_null=bad)
    # the host's refusals come first: a near-null entry of 0 before anything of the device
    bad = tiny.copy()
    bad[members] = 1e-170
    bad[3] = 0.0
    with pytest.raises(eng.SpmvError, match=r"amg_create_with: near_null\[3\] = 0"):
        build(eng, "isolated", "nn", near_null=bad)
    # what amg_create_with leaves to spmv_mi355x_create comes back with both names
    with pytest.raises(eng.SpmvError, match=r"amg_create_with: .*sell_c"):
        build(eng, "grid", "both", sell_c=7)
    with pytest.raises(ValueError, match="near_null must have 400 values"):
        build(eng, "isolated", "nn", near_null=np.ones(3))
    # level_csr(AF): a level without a prolongator, and a hierarchy that was not filtered
    M = build(eng, "grid", "both")
    with pytest.raises(eng.SpmvError, match=r"amg_level_csr: level 2 is the last: it has no filtered operator"):
        M.level_csr(2, "AF")
    M.close()
    M = build(eng, "grid", "nn")
    with pytest.raises(eng.SpmvError, match=r"amg_level_csr: .*filtered = 0"):
        M.level_csr(0, "AF")
    M.close()
