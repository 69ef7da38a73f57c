"""CPU tier of the k-column AMG / FSAI apply and the k-column tol-based CG (include/spmv_mi355x.h "k right-hand sides through one AMG
or FSAI cycle and one tol-based CG"): the symbols are exported, declared and bound; the refusals that need no handle come back as
rc 1 with the entry's name in the message, in the documented order, before the NULL checks and before any device is touched, and
leave the caller's buffers and infos alone; and the shared cases are what the GPU tier assumes (pcg_tri_multi_cases.py)."""
import ctypes
import inspect
import os

import numpy as np
import pytest

import pcg_tri_cases as pc
import pcg_tri_multi_cases as mc
from conftest import ROOT

NAN, INF = float("nan"), float("inf")
SOLVES = ("pcg_tri_multi", "pcg_fsai_multi", "pcg_amg_multi")
NEW = ("spmv_mi355x_amg_apply_multi_device_async", "spmv_mi355x_amg_apply_multi", "spmv_mi355x_amg_apply_multi_plan",
       "spmv_mi355x_fsai_apply_multi_device_async", "spmv_mi355x_fsai_apply_multi") + tuple("spmv_mi355x_" + s for s in SOLVES)


def test_the_symbols_are_exported_declared_and_bound():
    import spmv_mi355x as E
    header = open(os.path.join(ROOT, "include", "spmv_mi355x.h")).read()
    for sym in NEW:
        assert hasattr(E.lib(), sym) and sym in E.SYMBOLS, sym
        assert f"int  {sym}(" in header, sym
    assert ("int  spmv_mi355x_amg_apply_multi_device_async(spmv_mi355x_amg * M, int k, const void * in_dev, long ldin, void * out_dev, "
            "long ldout,\n\t\tvoid * hip_stream);") in header
    assert "int  spmv_mi355x_amg_apply_multi(spmv_mi355x_amg * M, int k, const void * in_host, void * out_host);" in header
    assert ("int  spmv_mi355x_amg_apply_multi_plan(const spmv_mi355x_amg * M, int k, long * matrix_passes_out, long * launches_out);"
            in header)
    assert "int  spmv_mi355x_pcg_tri_multi(spmv_mi355x_matrix * A, int k, const void * B_host, void * X_out_host," in header
    assert list(inspect.signature(E.Matrix.pcg_tri_multi).parameters) == ["self", "B", "precond", "tol", "max_iterations", "history"]
    assert list(inspect.signature(E.Amg.apply_multi_device).parameters) == ["self", "k", "in_ptr", "ldin", "out_ptr", "ldout", "stream"]
    assert list(inspect.signature(E.Fsai.apply_multi_device).parameters) == ["self", "k", "in_ptr", "ldin", "out_ptr", "ldout", "stream"]
    for cls in (E.Amg, E.Fsai):
        assert list(inspect.signature(cls.apply_multi).parameters) == ["self", "V"]
    assert list(inspect.signature(E.Amg.apply_multi_plan).parameters) == ["self", "k"]


def test_the_header_no_longer_lists_multi_rhs_as_not_built():
    header = open(os.path.join(ROOT, "include", "spmv_mi355x.h")).read()
    assert "multi-RHS wiring other than CG's" in header and "pbicgstab wiring, multi-RHS" not in header
    assert "NOT BUILT: multi-RHS, the row-partitioned form, device-pointer b / x, a non-zero x0" not in header


# the handle is NULL in every case: k, the struct sizes and the scalars are checked before the NULL check
CASES = [
    ("null_handle", 3, None, 1e-12, 10, b"NULL argument"),
    ("null_B", 3, None, 1e-12, 10, b"NULL argument"),
    ("null_X_out", 3, None, 1e-12, 10, b"NULL argument"),
    ("k_zero", 0, None, 1e-12, 10, b"k = 0"),
    ("k_negative_before_everything", -2, 0, -1.0, -1, b"k = -2"),
    ("struct_size_unset_first", 3, 0, 1e-12, 10, b"infos[0].struct_size not set"),
    ("struct_size_unset_last", 3, 2, 1e-12, 10, b"infos[2].struct_size not set"),
    ("struct_size_before_tol", 3, 1, -1.0, -1, b"infos[1].struct_size not set"),
    ("tol_negative", 3, None, -1.0, 10, b"tol must be finite and >= 0"),
    ("tol_nan", 3, None, NAN, 10, b"tol must be finite and >= 0"),
    ("tol_inf", 3, None, INF, 10, b"tol must be finite and >= 0"),
    ("tol_before_max_iterations", 3, None, -1.0, -1, b"tol must be finite and >= 0"),
    ("max_iterations_negative", 3, None, 1e-12, -1, b"max_iterations < 0"),
]


def _infos(E, k, unset):
    infos = (E.PcgTriInfo * max(k, 1))()
    for j in range(max(k, 1)):
        infos[j].struct_size = 0 if j == unset else ctypes.sizeof(E.PcgTriInfo)
        infos[j].iterations, infos[j].stop, infos[j].rnorm, infos[j].spmv_calls = -5, -6, -7.5, -9
    return infos


@pytest.mark.parametrize("entry", SOLVES)
@pytest.mark.parametrize("case,k,unset,tol,max_iterations,phrase", CASES, ids=[c[0] for c in CASES])
def test_the_checks_that_need_no_handle_in_their_order(entry, case, k, unset, tol, max_iterations, phrase):
    import spmv_mi355x as E
    lib = E.lib()
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    B, X, hist = np.full((4, 3), 3.5), np.full((4, 3), -7.25), np.full(30, 9.0)
    infos = _infos(E, k, unset)
    before = bytes(infos)
    rc = getattr(lib, "spmv_mi355x_" + entry)(None, k, None if case == "null_B" else p(B), None if case == "null_X_out" else p(X), None,
                                               tol, max_iterations, p(hist), infos)
    assert rc == 1
    msg = lib.spmv_mi355x_last_error()
    assert msg.startswith(entry.encode() + b": ") and phrase in msg, msg
    if case.startswith("null"):
        assert b" A " in msg, msg
    if case == "null_B":
        assert b" B " in msg, msg
    if case == "null_X_out":
        assert b" X_out " in msg, msg
    assert np.all(B == 3.5) and np.all(X == -7.25) and np.all(hist == 9.0) and bytes(infos) == before


def test_null_infos_are_legal_and_the_next_check_fires():
    import spmv_mi355x as E
    for entry in SOLVES:
        rc = getattr(E.lib(), "spmv_mi355x_" + entry)(None, 2, None, None, None, -1.0, 10, None, None)
        assert rc == 1 and (entry + ": tol must be finite").encode() in E.lib().spmv_mi355x_last_error()


@pytest.mark.parametrize("part", ["first", "second", "both"])
def test_a_triangular_part_is_refused_before_the_null_check(part):
    """first / second are only compared with NULL here: the refusal needs neither a handle of A nor a device"""
    import spmv_mi355x as E
    lib = E.lib()
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    fake = np.zeros(8)                                   # any non-NULL address: it is never dereferenced
    scale = np.full(4, 0.5)
    M = E.TriPrecond(ctypes.sizeof(E.TriPrecond), p(fake) if part != "second" else None, p(scale), p(fake) if part != "first" else None)
    B, X = np.full((4, 2), 3.5), np.full((4, 2), -7.25)
    infos = _infos(E, 2, None)
    before = bytes(infos)
    rc = lib.spmv_mi355x_pcg_tri_multi(None, 2, p(B), p(X), ctypes.byref(M), 1e-12, 10, None, infos)
    msg = lib.spmv_mi355x_last_error()
    assert rc == 1 and msg.startswith(b"pcg_tri_multi: ") and b"triangular part" in msg and b"no k-column triangular solve" in msg, msg
    assert np.all(B == 3.5) and np.all(X == -7.25) and bytes(infos) == before
    # the scalars still come first, and a scale alone goes on to the NULL check
    rc = lib.spmv_mi355x_pcg_tri_multi(None, 2, p(B), p(X), ctypes.byref(M), -1.0, 10, None, infos)
    assert rc == 1 and b"tol must be finite" in lib.spmv_mi355x_last_error()
    M = E.TriPrecond(ctypes.sizeof(E.TriPrecond), None, p(scale), None)
    rc = lib.spmv_mi355x_pcg_tri_multi(None, 2, p(B), p(X), ctypes.byref(M), 1e-12, 10, None, infos)
    assert rc == 1 and b"pcg_tri_multi: NULL argument ( A )" in lib.spmv_mi355x_last_error()


APPLIES = [("amg_apply_multi", "M"), ("fsai_apply_multi", "F")]


@pytest.mark.parametrize("entry,name", APPLIES)
def test_the_applies_refuse_a_null_handle(entry, name):
    import spmv_mi355x as E
    lib = E.lib()
    v = np.ones((4, 2))
    p = v.ctypes.data_as(ctypes.c_void_p)
    assert getattr(lib, f"spmv_mi355x_{entry}")(None, 2, p, p) == 1
    assert f"{entry}: NULL argument ( {name} )".encode() in lib.spmv_mi355x_last_error()
    assert getattr(lib, f"spmv_mi355x_{entry}_device_async")(None, 2, p, 2, p, 2, None) == 1
    assert f"{entry}: NULL argument ( {name} )".encode() in lib.spmv_mi355x_last_error()


def test_the_plan_refuses_null_arguments():
    import spmv_mi355x as E
    lib = E.lib()
    a, b = ctypes.c_long(-3), ctypes.c_long(-4)
    assert lib.spmv_mi355x_amg_apply_multi_plan(None, 2, ctypes.byref(a), ctypes.byref(b)) == 1
    assert b"amg_apply_multi_plan: NULL argument ( M )" in lib.spmv_mi355x_last_error()
    assert (a.value, b.value) == (-3, -4)


def test_what_python_refuses_before_the_call():
    import spmv_mi355x as E

    class Handle:                                       # Matrix.pcg_tri_multi reads m, dtype and h, nothing else
        m, n, dtype, h = 4, 4, np.dtype(np.float64), None

    with pytest.raises(ValueError, match=r"B must have shape \(4, k\)"):
        E.Matrix.pcg_tri_multi(Handle(), np.ones(4))
    with pytest.raises(ValueError, match=r"B must have shape \(4, k\)"):
        E.Matrix.pcg_tri_multi(Handle(), np.ones((3, 2)))
    with pytest.raises(ValueError, match="TriangularSolve"):
        E.Matrix.pcg_tri_multi(Handle(), np.ones((4, 2)), precond=("lower", None, None))
    for precond in (None, (None, np.ones(4), None)):
        with pytest.raises(E.SpmvError, match="pcg_tri_multi: NULL argument"):
            E.Matrix.pcg_tri_multi(Handle(), np.ones((4, 2)), precond=precond)


# ---- the shared cases ------------------------------------------------------------------------------------------------------------------

def test_the_chunks_are_eights_then_the_binary_remainder():
    assert mc.chunks(1) == [(0, 1)] and mc.chunks(3) == [(0, 2), (2, 1)] and mc.chunks(4) == [(0, 4)] and mc.chunks(8) == [(0, 8)]
    assert mc.chunks(9) == [(0, 8), (8, 1)] and mc.chunks(23) == [(0, 8), (8, 8), (16, 4), (20, 2), (22, 1)]
    for k in range(1, 40):
        ch = mc.chunks(k)
        assert [c0 for c0, _ in ch] == list(np.cumsum([0] + [kc for _, kc in ch[:-1]])) and sum(kc for _, kc in ch) == k


def test_the_blocks_are_what_the_gpu_tier_assumes():
    P = pc.problem()
    B = mc.solve_block()
    assert B.shape == (P.n, 9) and np.array_equal(B[:, 0], P.b) and not B.flags.writeable
    assert len({B[:, j].tobytes() for j in range(9)}) == 9
    V = mc.cycle_block(P.n)
    assert V.shape == (P.n, 9) and np.array_equal(V[:, 1], np.ones(P.n)) and V[:, 2].sum() == 1.0


def test_the_freeze_columns_stop_as_the_gpu_tier_expects():
    P = pc.problem()
    A = P.dense(np.float64)
    B = mc.freeze_columns()
    assert B.shape == (P.n, 5)
    got = [pc.restate(A, B[:, j], None, 1e-12, pc.MAX_ITERATIONS, np.float64) for j in range(5)]
    assert tuple(g[2] for g in got) == mc.FREEZE_STOPS
    # the eigenvector column is done after one body, more than 2 POLL bodies before the usual b
    assert got[1][1].size == 1 and got[0][1].size == pc.COUNTS[np.float64]["none"] and got[0][1].size - 1 > 2 * pc.POLL
    for j in (2, 3):
        assert got[j][1].size == 0 and not got[j][0].any()
