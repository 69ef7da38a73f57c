"""The multicolour ordering (include/spmv_mi355x.h "multicolour ordering") on the GPU. There is no tolerance on anything the handle
returns: colours, permutation, round count, the permuted matrix and the moved vectors are held with np.array_equal to the sequential
greedy loop of tests/color_reference.c and to the numpy restatements of color_cases.py, for every case listed there.

The point of it all is checked on `grid` (spd_grid(45)) and `stencil27` (14^3): the existing analysis finds as many levels in tril(B) as
there are colours (89 in tril(A) of the grid), the existing triangular solve on B gives the bits of its own sequential reference, and
the existing ILU(0) on B takes at most num_colors launches and gives the bits of tests/ilu0_reference.c.

The solves run on pcg_tri_cases.problem() in the colour ordering: B (P x) = P b by Matrix.pcg_tri over a handle of B with sgs_precond /
ilu0_precond of B. Their references are the restatement of pcg_tri_cases.restate on the permuted dense matrix under the reference
preconditioners (color_cases.problem()); the bounds are the family's (pcg_tri_cases.PREC, shares_of_the_bounds) on the UNPERMUTED x
against the unpermuted problem: no new tolerance."""
import ctypes

import numpy as np
import pytest

import color_cases as cc
import ilu0_cases as ic
import pcg_tri_cases as pc
import trsv_cases as tc
from pcg_tri_cases import MAX_ITERATIONS, PREC
from trsv_cases import LOWER, UPPER

pytestmark = pytest.mark.gpu

INFO_FIELDS = ("iterations", "stop", "rnorm", "rnorm0", "prnorm", "xnorm")
SENTINEL = -77.5


@pytest.fixture(scope="module")
def eng():
    import spmv_mi355x as eng
    assert eng.device_count() >= 1, "no GPU visible: the -m gpu tests need an MI355X"
    return eng


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def close(M):
    for h in M or ():
        if h is not None and not isinstance(h, np.ndarray):
            h.close()


def device_ints(torch, ptr, count):
    """`count` int32 at a device pointer, copied to the host"""
    if count == 0:
        return np.zeros(0, np.int32)

    class View:
        __cuda_array_interface__ = dict(shape=(count,), typestr="<i4", data=(ptr, False), version=2, strides=None)
    torch.cuda.synchronize()
    return torch.as_tensor(View(), device="cuda").cpu().numpy().copy()


# ---- 1. the colouring ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", cc.CASES)
def test_the_colouring_is_the_greedy_loop(eng, name):
    rp, ci, va, n = cc.matrix(name)
    ref = cc.reference(name)
    first = None
    for again in range(2):
        C = eng.Coloring(rp, ci, n)
        info = C.info()
        got = dict(colors=C.colors, perm=C.perm, rank=C.rank, color_ptr=C.color_ptr)
        for k, v in got.items():
            assert v.dtype == np.int32 and np.array_equal(v, ref[k]), f"{name}: {k} differs from the reference in {np.sum(v != ref[k])} places"
        assert C.num_colors == info["num_colors"] == ref["num_colors"]
        assert info["rounds"] == ref["rounds"], f"{name}: {info['rounds']} rounds, the reference {ref['rounds']}"
        classes = np.diff(ref["color_ptr"])
        assert (info["n"], info["nnz"]) == (n, len(ci))
        assert (info["max_class"], info["min_class"]) == ((int(classes.max()), int(classes.min())) if n else (0, 0))
        assert info["symmetric"] == int(name in ("grid", "clique70", "star", "stencil27", "path_wrap", "one", "empty"))
        assert C.mem_footprint == (4 * (n + 1) + 4 * len(ci) + 8 * n if n else 0)
        if first is not None:
            for k in got:
                assert np.array_equal(got[k], first[k]), f"{name}: a second create gives another {k}"
        first = got
        C.close()
        C.close()


# ---- 2. the permuted matrix ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", cc.CASES)
def test_the_permuted_matrix_is_the_restatement(eng, torch, name):
    rp, ci, va, n = cc.matrix(name)
    want = cc.permuted(name)
    C = eng.Coloring(rp, ci, n)
    got = C.permute_csr(va)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == w.dtype and g.shape == w.shape, (name, k)
        assert np.array_equal(g.view(np.int64) if g.dtype == np.float64 else g, w.view(np.int64) if w.dtype == np.float64 else w), \
            f"{name}: output {k} of permute_csr differs from the restatement"
    assert np.array_equal(got[2], va[got[3]])
    pattern = C.permute_csr()                                 # without values: the pattern and the map alone
    assert pattern[2] is None and all(np.array_equal(pattern[k], want[k]) for k in (0, 1, 3))
    dev = C.permute_csr_device()
    for ptr, count, w in zip(dev, (n + 1, len(ci), len(ci)), (want[0], want[1], want[3])):
        assert np.array_equal(device_ints(torch, ptr, count), w)
    assert C.info()["permute_seconds"] > 0 or n == 0
    assert C.mem_footprint == (4 * (n + 1) + 8 * len(ci) + 8 * n if n else 0)
    # new values: the gather alone, on the host and on another stream of the device, from a pointer that is only 8-byte aligned
    v2 = np.random.default_rng(2).uniform(-1, 1, len(va))
    assert np.array_equal(C.permute_values(v2), v2[want[3]])
    buf = torch.full((len(va) + 1,), SENTINEL, dtype=torch.float64, device="cuda")
    buf[1:] = torch.from_numpy(v2).cuda()
    out = torch.full((len(va) + 2,), SENTINEL, dtype=torch.float64, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    C.permute_values_device(buf.data_ptr() + 8, out.data_ptr() + 8, side.cuda_stream)
    side.synchronize()
    res = out.cpu().numpy()
    assert res[0] == SENTINEL and res[-1] == SENTINEL and np.array_equal(res[1:-1], v2[want[3]])
    C.close()


def test_a_handle_of_b_is_refreshed_through_the_map(eng, torch):
    """values_A -> values_B on the device -> update_values_device of a handle of B: the SpMV of a handle created from the new B"""
    for name in ("grid", "oneway"):
        rp, ci, va, n = cc.matrix(name)
        col, rp_b, ci_b, va_b = eng.multicolor_system(rp, ci, va, n)
        assert all(np.array_equal(g, w) for g, w in zip((rp_b, ci_b, va_b), cc.permuted(name)[:3]))
        v2 = va * (1 + 0.3 * np.random.default_rng(9).uniform(-1, 1, len(va)))
        x = np.random.default_rng(10).uniform(-1, 1, n)
        for fmt in ("sell_c_sigma", "csr_vector"):
            M = eng.Matrix(rp_b, ci_b, va_b, n, n, fmt)
            M.update_values_prepare(rp_b)
            d_in = torch.from_numpy(v2).cuda()
            d_out = torch.empty(len(v2), dtype=torch.float64, device="cuda")
            stream = torch.cuda.current_stream().cuda_stream
            col.permute_values_device(d_in.data_ptr(), d_out.data_ptr(), stream)
            M.update_values_device(d_out.data_ptr(), stream)
            fresh = eng.Matrix(rp_b, ci_b, v2[cc.permuted(name)[3]], n, n, fmt)
            assert np.array_equal(M.spmv(x), fresh.spmv(x)), (name, fmt)
            M.close()
            fresh.close()
        col.close()


# ---- 3. vectors --------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("name", ["grid", "oneway", "path_wrap", "one"])
def test_vectors_move_between_the_orderings(eng, torch, name, dtype):
    rp, ci, va, n = cc.matrix(name)
    perm = cc.reference(name)["perm"]
    C = eng.Coloring(rp, ci, n)
    tdt = torch.float64 if dtype == np.float64 else torch.float32
    rng = np.random.default_rng(n)
    for k, ld_in, ld_out, lead in ((1, 1, 1, 0), (1, 3, 2, 1), (3, 5, 4, 1), (8, 8, 16, 0), (8, 9, 11, 3), (11, 11, 12, 0), (11, 14, 13, 2)):
        V = rng.uniform(-1, 1, (n, k)).astype(dtype)
        # the host form: ld = k
        fwd = C.permute(V if k > 1 else V[:, 0])
        assert fwd.dtype == dtype and np.array_equal(fwd, (V if k > 1 else V[:, 0])[perm])
        assert np.array_equal(C.unpermute(fwd), V if k > 1 else V[:, 0])
        # the device form: blocks with ld > k that start `lead` elements into guarded buffers
        src = torch.full((lead + n * ld_in + 5,), SENTINEL, dtype=tdt, device="cuda")
        block = np.full((n, ld_in), SENTINEL, dtype)
        block[:, :k] = V
        src[lead:lead + n * ld_in] = torch.from_numpy(block.ravel()).cuda()
        mid = torch.full((lead + n * ld_out + 5,), SENTINEL, dtype=tdt, device="cuda")
        back = torch.full((lead + n * ld_in + 5,), SENTINEL, dtype=tdt, device="cuda")
        w = np.dtype(dtype).itemsize
        C.permute_device(src.data_ptr() + lead * w, mid.data_ptr() + lead * w, k, dtype, ld_in, ld_out)
        C.unpermute_device(mid.data_ptr() + lead * w, back.data_ptr() + lead * w, k, dtype, ld_out, ld_in)
        torch.cuda.synchronize()
        m, b = mid.cpu().numpy(), back.cpu().numpy()
        got = m[lead:lead + n * ld_out].reshape(n, ld_out)
        what = f"{name} {np.dtype(dtype).name} k={k} ld={ld_in}->{ld_out} lead={lead}"
        assert np.array_equal(got[:, :k], V[perm]), what
        assert np.all(got[:, k:] == SENTINEL) and np.all(m[:lead] == SENTINEL) and np.all(m[lead + n * ld_out:] == SENTINEL), what
        again = b[lead:lead + n * ld_in].reshape(n, ld_in)
        assert np.array_equal(again[:, :k], V), what
        assert np.all(again[:, k:] == SENTINEL) and np.all(b[:lead] == SENTINEL) and np.all(b[lead + n * ld_in:] == SENTINEL), what
    C.close()


# ---- 4. the point of it all: the existing pieces on B ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["grid", "stencil27"])
def test_the_levels_of_b_are_the_colours(eng, name):
    rp, ci, va, n = cc.matrix(name)
    ref = cc.reference(name)
    col, rp_b, ci_b, va_b = eng.multicolor_system(rp, ci, va, n)
    lower, upper = eng.trsv_analyze(rp_b, ci_b, n, "lower"), eng.trsv_analyze(rp_b, ci_b, n, "upper")
    assert lower["levels"] == col.num_colors == ref["num_colors"]
    assert np.array_equal(lower["level_of_row"], ref["colors"][ref["perm"]])
    assert upper["levels"] <= col.num_colors
    natural = eng.trsv_analyze(rp, ci, n, "lower")["levels"]
    assert natural > 5 * col.num_colors
    if name == "grid":
        assert natural == 89
    # the exact solve of tril(B) and triu(B), unpermuted: the bits of the sequential fma loop on B
    b = np.random.default_rng(4).uniform(-1, 1, n)
    for dtype in (np.float64, np.float32):
        pb = col.permute(b.astype(dtype))
        for uplo, code in (("lower", LOWER), ("upper", UPPER)):
            T = eng.TriangularSolve(rp_b, ci_b, va_b, n, uplo=uplo, dtype=dtype)
            assert T.info["levels"] <= col.num_colors
            x = col.unpermute(T.solve(pb))
            T.close()
            want = np.empty(n, dtype)
            want[ref["perm"]] = tc.reference(rp_b, ci_b, va_b, n, code, False, b.astype(dtype)[ref["perm"]], dtype)
            assert np.array_equal(x, want), f"{name} {uplo} {np.dtype(dtype).name}: {np.sum(x != want)} of {n} values differ"
    # ILU(0) on B: at most one launch per colour, and the bits of the sequential loop
    F = eng.Ilu0(rp_b, ci_b, n)
    f = F.factor(va_b).values()
    info = F.info
    assert info["launches"] <= col.num_colors and info["levels"] == col.num_colors and info["breakdown_row"] == -1
    want, bad = ic.reference(rp_b, ci_b, va_b, n)
    assert bad == -1 and np.array_equal(f, want), f"{name}: {np.sum(f != want)} of {len(want)} entries of the factor differ"
    N = eng.Ilu0(rp, ci, n)
    assert N.info["launches"] > 5 * info["launches"]
    N.close()
    F.close()
    col.close()


# ---- 5. the solve ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["sgs", "ic0"])
def test_pcg_under_the_multicolour_preconditioners(eng, kind):
    P, Q = pc.problem(), cc.problem()
    rp, ci, va = P.csr
    want = P.solve()
    col, rp_b, ci_b, va_b = eng.multicolor_system(rp, ci, va, P.n)
    assert np.array_equal(col.perm, Q.perm) and all(np.array_equal(g, w) for g, w in zip((rp_b, ci_b, va_b), Q.csr))
    for dtype, lim in PREC.items():
        name = np.dtype(dtype).name
        _, ref, ref_stop = Q.restatement(dtype, kind, lim["tol"])
        assert ref_stop == 1 and ref.size == cc.COUNTS[dtype][kind]
        make = eng.sgs_precond if kind == "sgs" else eng.ilu0_precond
        M = make(rp_b, ci_b, va_b, P.n, dtype=dtype)
        assert M[0].info["levels"] <= col.num_colors and M[2].info["levels"] <= col.num_colors
        pb = col.permute(P.b.astype(dtype))
        runs = []
        for fmt in ("sell_c_sigma", "csr_vector"):
            A = eng.Matrix(rp_b, ci_b, va_b, P.n, P.n, fmt, dtype)
            what = f"P A P^t of spd_grid(45) {A.format_name} {name} precond=multicolour {kind}"
            got = A.pcg_tri(pb, precond=M, tol=lim["tol"], max_iterations=MAX_ITERATIONS)
            k = got["iterations"]
            print(f"[color] {what}: {k} iterations (the restatement {ref.size}; the natural ordering {pc.COUNTS[dtype][kind]})")
            assert got["stop"] == 1, f"{what}: stop {got['stop']} after {k} iterations"
            assert abs(k - ref.size) <= 1, f"{what}: {k} iterations, the restatement {ref.size}"
            back = dict(got, x=col.unpermute(got["x"]))
            assert back["x"].dtype == dtype
            for key, v in pc.shares_of_the_bounds(P, back, dtype, want).items():
                print(f"[color] {what}: {key} is {v:.3g} of its bound")
                assert v <= 1, f"{what}: {key} is {v:.3g} times its bound"
            # repeatable bit for bit
            again = A.pcg_tri(pb, precond=M, tol=lim["tol"], max_iterations=MAX_ITERATIONS)
            for f in INFO_FIELDS:
                assert got[f] == again[f], (what, f)
            assert np.array_equal(got["x"], again["x"]) and np.array_equal(got["history"], again["history"]), what
            runs.append(got)
            if fmt == "sell_c_sigma":
                # k = 3 columns: the single solves' bits per column
                rhs = [pb, col.permute(np.random.default_rng(21).uniform(-1, 1, P.n).astype(dtype)), (2 * pb).astype(dtype)]
                multi = A.pcg_trsm_multi(np.stack(rhs, axis=1), precond=M, tol=lim["tol"], max_iterations=MAX_ITERATIONS)
                for j, b_j in enumerate(rhs):
                    single = got if j == 0 else A.pcg_tri(b_j, precond=M, tol=lim["tol"], max_iterations=MAX_ITERATIONS)
                    for f in INFO_FIELDS:
                        assert multi[j][f] == single[f], (what, j, f)
                    assert np.array_equal(multi[j]["x"], single["x"]) and np.array_equal(multi[j]["history"], single["history"]), (what, j)
            A.close()
        close(M)
    col.close()


# ---- 6. refusals that need a device -----------------------------------------------------------------------------------------------------------

def test_refusals_on_a_live_handle(eng, torch):
    rp, ci, va, n = cc.matrix("grid")
    C = eng.Coloring(rp, ci, n)
    buf = torch.zeros(3 * n, dtype=torch.float64, device="cuda")
    with pytest.raises(eng.SpmvError, match=r"color_permute_vectors: in and out are the same block"):
        C.permute_device(buf.data_ptr(), buf.data_ptr())
    with pytest.raises(eng.SpmvError, match=r"color_permute_vectors: in and out are the same block"):
        C.unpermute_device(buf.data_ptr(), buf.data_ptr(), 3, np.float32)
    with pytest.raises(eng.SpmvError, match=r"color_permute_vectors: NULL argument \( out"):
        C.permute_device(buf.data_ptr(), 0)
    with pytest.raises(eng.SpmvError, match=r"color_permute_vectors: direction must be"):
        C.permute_device(buf.data_ptr(), buf.data_ptr() + 8 * n, direction=3)
    with pytest.raises(eng.SpmvError, match=r"color_permute_vectors: need k >= 1, ldin >= k and ldout >= k \(got k=2 ldin=1 ldout=2\)"):
        C.permute_device(buf.data_ptr(), buf.data_ptr() + 8 * n, 2, np.float64, 1, 2)
    with pytest.raises(eng.SpmvError, match=r"color_permute_values: values and out are the same array"):
        C.permute_values_device(buf.data_ptr(), buf.data_ptr())
    with pytest.raises(eng.SpmvError, match=r"color_permute_values: NULL argument \( values"):
        C.permute_values_device(0, buf.data_ptr())
    with pytest.raises(ValueError):
        C.permute_csr(va[:-1])
    host = np.ones(n)
    rc = eng.lib().spmv_mi355x_color_permute_vectors(C.h, 0, 0, 1, host.ctypes.data_as(ctypes.c_void_p), 1, host.ctypes.data_as(ctypes.c_void_p), 1)
    assert rc == 1 and eng.lib().spmv_mi355x_last_error().startswith(b"color_permute_vectors: in and out are the same block")
    with pytest.raises(eng.SpmvError, match=r"color_create: device 99 out of range"):
        eng.Coloring(rp, ci, n, device=99)
    assert np.array_equal(C.permute(host), host)              # the handle is as it was
    C.close()


def test_the_round_cap(eng):
    """a clique of m rows needs m rounds. The cap of the ABI is 4096; the create routine behind it takes a lower one for this test, so
    that the refusal is reached with 70 rows instead of 4097."""
    rp, ci, va, n = cc.matrix("clique70")
    fn = eng.lib().spmv_mi355x_color_create_capped_for_tests
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    h = ctypes.c_void_p()
    assert fn(ctypes.byref(h), n, p(rp), p(ci), -1, 69) == 1 and not h.value
    msg = eng.lib().spmv_mi355x_last_error().decode()
    assert msg.startswith("color_create: 1 rows are still uncoloured after 69 rounds (the cap; a clique of m rows needs m rounds)"), msg
    assert fn(ctypes.byref(h), n, p(rp), p(ci), -1, 70) == 0 and h.value
    stats = eng.ColorStats()
    stats.struct_size = ctypes.sizeof(eng.ColorStats)
    assert eng.lib().spmv_mi355x_color_info(h, ctypes.byref(stats)) == 0 and (stats.rounds, stats.num_colors) == (70, 70)
    assert eng.lib().spmv_mi355x_color_destroy(h) == 0
    for cap in (0, 4097):
        assert fn(ctypes.byref(h), n, p(rp), p(ci), -1, cap) == 1
        assert eng.lib().spmv_mi355x_last_error().startswith(b"color_create: round cap")
