"""CPU tier of the factorized sparse approximate inverse (include/spmv_mi355x.h "FSAI"): the symbols are exported, declared and
bound; every refusal of spmv_mi355x_fsai_create that needs no device comes back in the header's order (each case also carries the
errors of LATER steps, which must not be the ones reported); spmv_mi355x_fsai_pattern equals a dense boolean matrix power; and the
references the GPU tier compares against are themselves checked here: tests/fsai_reference.c against the numpy restatement
(np.linalg.cholesky per row, then a solve), diag(G A G^t) = 1, the fallback rule on an indefinite local block, and the CG iteration
counts of fsai_cases.COUNTS with M^-1 = G^t (G .)."""
import ctypes
import inspect
import os

import numpy as np
import pytest

import fsai_cases as fc
import pcg_tri_cases as pc
from conftest import ROOT

FSAI_SYMBOLS = ["spmv_mi355x_fsai_pattern", "spmv_mi355x_fsai_create", "spmv_mi355x_fsai_destroy", "spmv_mi355x_fsai_apply_device_async",
                "spmv_mi355x_fsai_apply", "spmv_mi355x_fsai_values", "spmv_mi355x_fsai_matrices", "spmv_mi355x_fsai_info",
                "spmv_mi355x_fsai_setup_split", "spmv_mi355x_fsai_mem_footprint", "spmv_mi355x_pcg_fsai"]
SELL, F64 = 3, 0


def test_the_symbols_are_exported_declared_and_bound():
    import spmv_mi355x as E
    header = open(os.path.join(ROOT, "include", "spmv_mi355x.h")).read()
    for sym in FSAI_SYMBOLS:
        assert hasattr(E.lib(), sym) and sym in E.SYMBOLS and sym + "(" in header, sym
    assert "#define SPMV_MI355X_FSAI_MAX_ROW 128" in header and E.FSAI_MAX_ROW == fc.MAX_ROW == 128
    assert list(inspect.signature(E.fsai_pattern).parameters) == ["row_ptr", "col_idx", "n", "power"]
    assert list(inspect.signature(E.Fsai.__init__).parameters) == ["self", "row_ptr", "col_idx", "values", "n", "pattern", "fmt", "dtype",
                                                                   "opts"]
    for name in ("apply", "values", "info", "close"):
        assert callable(getattr(E.Fsai, name))
    for phrase in ("NOT CHECKABLE: that A is symmetric and positive definite", "NOT BUILT: update_values for an fsai handle"):
        assert phrase in header


# ---- the refusals that need no device, in their order -----------------------------------------------------------------------------

def _create(E, n, rp, ci, va, prp=None, pci=None, fmt=SELL, precision=F64, opts=None, out=True):
    p = lambda a: None if a is None else np.ascontiguousarray(a).ctypes.data_as(ctypes.c_void_p)
    keep = [None if a is None else np.ascontiguousarray(a, t) for a, t in ((rp, np.int32), (ci, np.int32), (va, np.float64),
                                                                             (prp, np.int32), (pci, np.int32))]
    h = ctypes.c_void_p(0x1234)
    o = None
    if opts is not None:
        o = E._make_opts(opts) if isinstance(opts, dict) else opts
    rc = E.lib().spmv_mi355x_fsai_create(ctypes.byref(h) if out else None, fmt, precision, ctypes.c_long(n), *[p(a) for a in keep],
                                         None if o is None else ctypes.byref(o))
    return rc, h, E.lib().spmv_mi355x_last_error()


def _refused(E, phrases, *args, **kw):
    rc, h, msg = _create(E, *args, **kw)
    assert rc == 1 and msg.startswith(b"fsai_create: ") and all(ph in msg for ph in phrases), msg
    assert not kw.get("out", True) or h.value is None, "the out handle is cleared"


# a good 3 x 3 matrix, and what is wrong with it from step 3 on
RP, CI, VA = [0, 2, 5, 7], [0, 1, 0, 1, 2, 1, 2], [4.0, -1.0, -1.0, 4.0, -1.0, -1.0, 4.0]
BAD_RP = [0, 2, 1, 7]                                     # 3. not monotone
DUP_CI = [0, 1, 0, 0, 2, 1, 2]                            # 4. row 1 stores column 0 twice (and no diagonal: 6.)
BAD_PAT = ([0, 1, 3, 4], [0, 1, 0, 2])                    # 5. row 1 descends (and does not end with its diagonal)
NO_DIAG_VA = [4.0, -1.0, -1.0, -4.0, -1.0, -1.0, 4.0]     # 6. the diagonal of row 1 is negative


def test_refusals_in_their_order():
    import spmv_mi355x as E
    # 1. the scalars, whatever else is wrong (NULL arrays: step 2)
    _refused(E, (b"unknown precision 7",), 3, None, None, None, precision=7)
    _refused(E, (b"unknown format 9",), 3, None, None, None, fmt=9)
    _refused(E, (b"n = -1",), -1, None, None, None)
    _refused(E, (b"n = 2147483647",), 2 ** 31 - 1, None, None, None)
    unset = E.Opts()
    _refused(E, (b"struct_size",), 3, None, None, None, opts=unset)
    _refused(E, (b"transpose",), 3, None, None, None, opts=dict(transpose=1))
    _refused(E, (b"symmetric_input",), 3, None, None, None, opts=dict(symmetric_input=1))
    _refused(E, (b"row block", b"row_end 2"), 3, None, None, None, opts=dict(row_begin=0, row_end=2))
    _refused(E, (b"value_storage",), 3, None, None, None, fmt=1, opts=dict(value_storage=1))
    # 2. NULL pointers, before the pattern of A is read
    _refused(E, (b"NULL argument", b" out"), 3, BAD_RP, CI, VA, out=False)
    _refused(E, (b"NULL argument", b" row_ptr"), 3, None, CI, VA)
    _refused(E, (b"NULL argument", b" col_idx"), 3, RP, None, VA)
    _refused(E, (b"NULL argument", b" values"), 3, RP, CI, None)
    _refused(E, (b"NULL argument", b" pat_col_idx"), 3, BAD_RP, CI, VA, prp=BAD_PAT[0])
    _refused(E, (b"NULL argument", b" pat_row_ptr"), 3, BAD_RP, CI, VA, pci=BAD_PAT[1])
    # 3. A's pattern, before its duplicates, the pattern of G and the diagonal
    _refused(E, (b"row_ptr is not monotone at row 1",), 3, BAD_RP, DUP_CI, NO_DIAG_VA, *BAD_PAT)
    _refused(E, (b"row_ptr must start at 0",), 3, [1, 2, 5, 7], DUP_CI, NO_DIAG_VA, *BAD_PAT)
    _refused(E, (b"column index 3 out of range [0,3) at entry 4",), 3, RP, [0, 1, 0, 0, 3, 1, 2], NO_DIAG_VA, *BAD_PAT)
    _refused(E, (b"column index -1 out of range",), 3, RP, [0, 1, 0, 0, -1, 1, 2], NO_DIAG_VA, *BAD_PAT)
    # 4. a column stored twice in a row's lower triangle; twice in the upper triangle is nobody's business
    _refused(E, (b"row 1 of A stores column 0 twice",), 3, RP, DUP_CI, NO_DIAG_VA, *BAD_PAT)
    # 5. the pattern of G, before the diagonal of A
    _refused(E, (b"row 1 is not strictly ascending",), 3, RP, CI, NO_DIAG_VA, *BAD_PAT)
    _refused(E, (b"pat_row_ptr is not monotone at row 1",), 3, RP, CI, NO_DIAG_VA, [0, 2, 1, 3], [0, 1, 2])
    _refused(E, (b"pat_row_ptr must start at 0",), 3, RP, CI, NO_DIAG_VA, [1, 2, 3, 4], [0, 0, 1, 2])
    _refused(E, (b"row 0 holds column 1",), 3, RP, CI, NO_DIAG_VA, [0, 1, 2, 3], [1, 1, 2])
    _refused(E, (b"row 1 holds column -2",), 3, RP, CI, NO_DIAG_VA, [0, 1, 3, 4], [0, -2, 1, 2])
    _refused(E, (b"row 1 is not strictly ascending (column 1 after 1)",), 3, RP, CI, NO_DIAG_VA, [0, 1, 3, 4], [0, 1, 1, 2])
    _refused(E, (b"row 2 does not end with its diagonal",), 3, RP, CI, NO_DIAG_VA, [0, 1, 2, 3], [0, 1, 1])
    _refused(E, (b"row 1 does not end with its diagonal",), 3, RP, CI, NO_DIAG_VA, [0, 1, 1, 2], [0, 2])
    # 6. the diagonal of A: missing, not positive, not finite; the first bad row is named
    _refused(E, (b"the diagonal of row 1 of A is -4",), 3, RP, CI, NO_DIAG_VA)
    _refused(E, (b"the diagonal of row 1 of A is -4",), 3, RP, CI, NO_DIAG_VA, [0, 1, 3, 6], [0, 0, 1, 0, 1, 2])
    _refused(E, (b"row 0 of A has no diagonal entry",), 3, RP, [1, 1, 0, 1, 2, 1, 2], NO_DIAG_VA)
    for bad in (0.0, np.nan, np.inf):
        _refused(E, (b"the diagonal of row 2 of A",), 3, RP, CI, VA[:6] + [bad])


def test_a_row_of_129_entries_is_refused():
    """5.: the pattern's widest row may hold SPMV_MI355X_FSAI_MAX_ROW = 128 entries; given explicitly, and as the lower triangle of
    a banded A of half-bandwidth 128. The message gives the first such row and its count."""
    import spmv_mi355x as E
    rp, ci, va, n, _ = fc.case("banded128")
    _refused(E, (b"row 128 has 129 entries", b"SPMV_MI355X_FSAI_MAX_ROW = 128"), n, rp, ci, va)
    prp, pci = fc.tril_power(rp, ci, n)
    assert np.diff(prp).max() == 129
    _refused(E, (b"row 128 has 129 entries",), n, rp, ci, va, prp, pci)


def test_pcg_fsai_refusals_that_need_no_handle():
    """items 1 to 4 of pcg_tri with the prefix pcg_fsai, before F is looked at"""
    import spmv_mi355x as E
    b, x = np.full(4, 3.5), np.full(4, -7.25)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    info = E.PcgTriInfo()
    for size, tol, maxit, A, phrase in ((4, 1e-12, 10, None, b"struct_size"), (None, -1.0, 10, None, b"tol"),
                                        (None, float("nan"), 10, None, b"tol"), (None, 1e-12, -1, None, b"max_iterations"),
                                        (None, 1e-12, 10, None, b"NULL argument")):
        info.struct_size = ctypes.sizeof(E.PcgTriInfo) if size is None else size
        rc = E.lib().spmv_mi355x_pcg_fsai(A, p(b), p(x), None, tol, maxit, None, ctypes.byref(info))
        msg = E.lib().spmv_mi355x_last_error()
        assert rc == 1 and msg.startswith(b"pcg_fsai: ") and phrase in msg, msg
    assert np.all(b == 3.5) and np.all(x == -7.25)


# ---- fsai_pattern against a dense boolean matrix power ------------------------------------------------------------------------------

def _dense_power(rp, ci, n, power):
    L = np.zeros((n, n), np.float32)
    rows = np.repeat(np.arange(n), np.diff(rp))
    keep = ci <= rows
    L[rows[keep], ci[keep]] = 1
    L[np.arange(n), np.arange(n)] = 1
    P = L.copy()
    for _ in range(power - 1):
        P = ((P @ L) > 0).astype(np.float32)
    return P > 0


def _random_lower(n=300, seed=11):
    """a pattern with both triangles present, unsorted rows, columns repeated inside rows and some rows without a diagonal"""
    rng = np.random.default_rng(seed)
    rp, ci = [0], []
    for i in range(n):
        k = int(rng.integers(0, 7))
        cols = np.concatenate([rng.integers(0, n, k), rng.integers(max(0, i - 5), i + 1, 2), [] if i % 3 == 0 else [i]]).astype(np.int32)
        cols = np.concatenate([cols, cols[:2]])                               # duplicates
        ci.append(rng.permutation(cols))
        rp.append(rp[-1] + len(cols))
    return np.array(rp, np.int32), np.concatenate(ci).astype(np.int32), n


@pytest.mark.parametrize("which", ("spd_grid(45)", "random lower pattern"))
def test_fsai_pattern_is_the_dense_boolean_power(which):
    import spmv_mi355x as E
    if which == "spd_grid(45)":
        rp, ci, _, n, _ = pc.spd_grid(45)
    else:
        rp, ci, n = _random_lower()
    for power in (1, 2, 3):
        prp, pci = E.fsai_pattern(rp, ci, n, power)
        want = _dense_power(rp, ci, n, power)
        assert prp.dtype == np.int32 and prp[0] == 0 and prp[n] == want.sum() == len(pci), (which, power)
        got = np.zeros((n, n), bool)
        rows = np.repeat(np.arange(n), np.diff(prp))
        got[rows, pci] = True
        assert np.array_equal(got, want), (which, power)
        assert np.all(np.diff(pci)[np.diff(rows) == 0] > 0), "columns strictly ascending"
        assert np.all(pci[prp[1:] - 1] == np.arange(n)), "every row ends with its diagonal"
        s_rp, s_ci = fc.tril_power(rp, ci, n, power)                           # the pattern the cases use
        assert np.array_equal(prp, s_rp) and np.array_equal(pci, s_ci)
    if which == "spd_grid(45)":
        assert np.diff(E.fsai_pattern(rp, ci, n, 1)[0]).max() == 3 and np.diff(E.fsai_pattern(rp, ci, n, 2)[0]).max() == 6


def test_fsai_pattern_refusals():
    import spmv_mi355x as E
    rp, ci = np.array(RP, np.int32), np.array(CI, np.int32)
    for args, phrase in (((rp, ci, 3, 0), "power must be 1, 2 or 3"), ((rp, ci, 3, 4), "power must be 1, 2 or 3"),
                         ((rp, ci, -1, 1), "n = -1"), ((np.array(BAD_RP, np.int32), ci, 3, 1), "not monotone at row 1"),
                         ((rp, np.array([0, 1, 0, 1, 3, 1, 2], np.int32), 3, 1), "column index 3 out of range")):
        with pytest.raises(E.SpmvError, match="fsai_pattern: .*" + phrase):
            E.fsai_pattern(*args)
    e_rp, e_ci = E.fsai_pattern(np.zeros(1, np.int32), np.zeros(0, np.int32), 0, 2)
    assert e_rp.tolist() == [0] and e_ci.size == 0


# ---- the C reference against numpy ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ("grid_tril", "grid_power2", "banded70", "banded127", "random"))
def test_the_c_reference_against_numpy(name):
    """relative error per row <= 1e-12 and max |diag(G A G^t) - 1| <= 1e-13: the bounds the issue sets for spd_grid(45), held for
    the other small cases as well (their local systems are diagonally dominant, cond <= a few hundred)"""
    c, D = fc.case(name), fc.dense(name)
    prp, pci = fc.pattern_of(c)
    g, fell = fc.reference_of(name)
    want, want_fell = fc.restatement(D, (prp, pci))
    assert fell == want_fell == 0
    worst = 0.0
    for i in range(c[3]):
        a, b = g[prp[i]:prp[i + 1]], want[prp[i]:prp[i + 1]]
        worst = max(worst, np.linalg.norm(a - b) / np.linalg.norm(b))
    G = fc.dense_g(c, g)
    d = np.abs(((G @ D) * G).sum(axis=1) - 1).max()
    print(f"[fsai] {name}: the C reference against numpy {worst:.3g} per row, |diag(G A G^t) - 1| {d:.3g}, "
          f"widest row {np.diff(prp).max()}")
    assert worst <= 1e-12 and d <= 1e-13, (name, worst, d)
    assert np.all(g[prp[1:] - 1] > 0), "the diagonal of G is positive"


def test_the_fallback_rule_on_an_indefinite_block():
    c, D = fc.case("indefinite"), fc.dense("indefinite")
    prp, pci = fc.pattern_of(c)
    g, fell = fc.reference_of("indefinite")
    want, want_fell = fc.restatement(D, (prp, pci))
    assert fell == want_fell == 1
    assert g[prp[1]:prp[2]].tolist() == [0.0, 1.0]                             # (an explicit 0, 1 / sqrt(A(1, 1)))
    np.testing.assert_allclose(g, want, rtol=1e-14, atol=0)
    assert g[0] == 1.0 and np.all(np.isfinite(g))


def test_the_small_cases_hit_every_bin():
    """rows of 1 .. 8, 9 .. 32, 33 .. 64 and 65 .. 128 pattern entries (csrc/fsai.hpp), rows of one entry among them, the cap itself,
    and a row list longer than one launch's workgroups can take in one trip"""
    widths = {name: np.diff(fc.pattern_of(fc.case(name))[0]) for name in ("grid_power2", "banded70", "banded127", "random")}
    assert widths["grid_power2"].max() == 6 and widths["banded70"].max() == 71 and widths["banded127"].max() == fc.MAX_ROW
    r = widths["random"]
    assert r.min() == 1 and r.max() == 40 and (r == 1).sum() >= 100 and ((r > 8) & (r <= 32)).any() and (r > 32).any()
    assert ((widths["banded70"] > 32) & (widths["banded70"] <= 64)).any() and (widths["banded127"] > 64).any()
    n = fc.case("tridiagonal_wrap")[3]
    assert n > fc.SMALL_BIN_ROWS * fc.MAX_GRID and np.diff(fc.pattern_of(fc.case("tridiagonal_wrap"))[0]).max() == 2


# ---- the counts ------------------------------------------------------------------------------------------------------------------------------

def test_the_iteration_counts_of_the_table():
    """pcg_tri_cases.restate with M^-1 = G^t (G .), G from the C reference: the counts of fsai_cases.COUNTS, below Jacobi's, and the
    solution is the dense solve's within the GPU tier's bounds. cond(G A G^t) is 21.2 and 10.9 against 92.1."""
    P = pc.problem()
    want = P.solve()
    for power, cond in ((1, 21.2), (2, 10.9)):
        name = fc.grid_case(power)
        G = fc.dense_g(fc.case(name), fc.reference_of(name)[0])
        ev = np.linalg.eigvalsh(G @ P.D @ G.T)
        assert abs(ev[-1] / ev[0] - cond) < 0.05, (power, ev[-1] / ev[0])
        for dtype, lim in pc.PREC.items():
            x, hist, stop = fc.grid_restatement(power, dtype, lim["tol"])
            print(f"[fsai] power {power} {np.dtype(dtype).name}: {hist.size} iterations")
            assert stop == 1 and hist.size == fc.COUNTS[dtype][power], (power, dtype, hist.size)
            assert hist.size < pc.COUNTS[dtype]["jacobi"]
            assert np.linalg.norm(x.astype(np.float64) - want) / np.linalg.norm(want) <= pc.KAPPA * 10 * lim["tol"]
