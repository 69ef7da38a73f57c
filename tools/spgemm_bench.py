"""What the sparse product on the GPU (spmv_mi355x_spgemm_*; include/spmv_mi355x.h "SpGEMM") costs, symbolic and numeric apart,
against the same product by scipy.sparse on the host, over three legs:
    aa<N>        A A of the 27-point stencil of tools/solver_bench.py on an N^3 grid;
    galerkin<N>  P^t (A P) of the same stencil with piecewise-constant 2 x 2 x 2 aggregates (two plans, A P and then P^t (A P));
    aat          A A^t of a tall random matrix (--tall m,k,d: m rows, k columns, up to d entries per row).
In one process, alternating window by window (window 0 warms every leg up and is dropped), per product:
  symbolic:  SpGemm(...) from host patterns: the wall seconds of the call and the plan's own symbolic_seconds (the device part);
  numeric:   multiply_device on device-resident values, HIP events over --reps back-to-back calls;
  scipy:     the wall seconds of A @ B in CSR on the host (pattern and values at once: scipy has no split);
  torch:     torch.sparse.mm of the two CSR tensors on the device, HIP events, where it runs: a second reference only, never on the
             product path. Where it does not run the record says why.
Once per product the GPU result is compared with scipy's (the same pattern, the largest difference of a value over |A| |B|). The
medians over the windows are reported with their min .. max spreads. No threshold is set and no speed is promised.

    python tools/spgemm_bench.py                                      # aa64, galerkin160, aat
    python tools/spgemm_bench.py --legs aa96 --windows 5
One JSON line per product, and a table at the end."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "spmv-research_amd", "python"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)


def aggregates(N):
    """P (N^3 x (N/2)^3) of the piecewise-constant 2 x 2 x 2 aggregates, as a scipy CSR of ones"""
    import scipy.sparse as sp
    idx = np.arange(N ** 3, dtype=np.int64)
    z, y, x = idx // (N * N), (idx // N) % N, idx % N
    h = (N + 1) // 2
    agg = ((z // 2) * h + y // 2) * h + x // 2
    return sp.csr_matrix((np.ones(N ** 3), agg.astype(np.int32), np.arange(N ** 3 + 1, dtype=np.int32)), shape=(N ** 3, h ** 3))


def products_of(leg, args):
    """the (name, A, B) of a leg as scipy CSR matrices; a later product of a leg may take "previous" for the result before it"""
    import scipy.sparse as sp
    from solver_bench import stencil27
    if leg.startswith("aa") and leg != "aat":
        rp, ci, va, n = stencil27(int(leg[2:]), 27.0)
        A = sp.csr_matrix((va, ci, rp), shape=(n, n))
        return [(leg, A, A)]
    if leg.startswith("galerkin"):
        N = int(leg[len("galerkin"):])
        rp, ci, va, n = stencil27(N, 27.0)
        A = sp.csr_matrix((va, ci, rp), shape=(n, n))
        P = aggregates(N)
        Pt = P.T.tocsr()
        Pt.sort_indices()
        return [(leg + " A P", A, P), (leg + " Pt (A P)", Pt, "previous")]
    if leg == "aat":
        m, k, d = args.tall
        rng = np.random.default_rng(5)
        A = sp.csr_matrix((rng.uniform(-1, 1, m * d), rng.integers(0, k, m * d).astype(np.int32), np.arange(0, m * d + 1, d, dtype=np.int32)),
                          shape=(m, k))
        A.sum_duplicates()                                 # A^t is B: it must not hold a column twice in a row
        At = A.T.tocsr()
        At.sort_indices()
        return [(f"aat {m}x{k} d{d}", A, At)]
    raise SystemExit(f"unknown leg {leg}")


def time_events(torch, fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / reps


def run(E, torch, name, A, B, args):
    i32 = lambda a: np.ascontiguousarray(a, np.int32)
    make = lambda: E.SpGemm(i32(A.indptr), i32(A.indices), A.shape[0], A.shape[1], i32(B.indptr), i32(B.indices), B.shape[1])
    ta, tb = torch.from_numpy(np.array(A.data, np.float64)).cuda(), torch.from_numpy(np.array(B.data, np.float64)).cuda()
    P = make()
    info = P.info()
    tc = torch.empty(max(P.nnz, 1), dtype=torch.float64, device="cuda")
    numeric = lambda: P.multiply_device(ta.data_ptr(), tb.data_ptr(), tc.data_ptr(), torch.cuda.current_stream().cuda_stream)
    # once: against scipy
    S = (A @ B).tocsr()
    S.sort_indices()
    numeric()
    torch.cuda.synchronize()
    got = tc.cpu().numpy()[:P.nnz]
    same_pattern = bool(S.nnz == P.nnz and np.array_equal(S.indptr, P.row_ptr) and np.array_equal(S.indices, P.col_idx))
    worst = float("nan")
    if same_pattern and P.nnz:
        Sa = (abs(A) @ abs(B)).tocsr()
        Sa.sort_indices()
        worst = float((np.abs(got - S.data) / np.maximum(Sa.data, 1e-300)).max())
    # torch.sparse.mm on the device, where it runs
    torch_fn, torch_note = None, ""
    if args.torch:
        try:
            csr = lambda M: torch.sparse_csr_tensor(torch.from_numpy(i32(M.indptr)).cuda(), torch.from_numpy(i32(M.indices)).cuda(),
                                                    torch.from_numpy(np.array(M.data, np.float64)).cuda(), size=M.shape)
            Ta, Tb = csr(A), csr(B)
            torch_fn = lambda: torch.sparse.mm(Ta, Tb)
            Tc = torch_fn()
            torch.cuda.synchronize()
            torch_note = f"nnz {Tc._nnz()}"
        except Exception as e:                              # a reference that does not run is reported, not replaced
            torch_fn, torch_note = None, f"did not run: {type(e).__name__}: {str(e).splitlines()[0][:120]}"
    else:
        torch_note = "not asked for"
    legs = {k: [] for k in ("symbolic_wall", "symbolic_device", "numeric", "scipy", "torch")}
    for w in range(args.windows + 1):                         # window 0 warms every leg up and is dropped
        t0 = time.perf_counter()
        Q = make()
        t_sym = time.perf_counter() - t0
        t_dev = Q.info()["symbolic_seconds"]
        Q.close()
        t_num = time_events(torch, numeric, args.reps)
        t0 = time.perf_counter()
        A @ B
        t_sci = time.perf_counter() - t0
        t_tor = time_events(torch, torch_fn, max(1, args.reps // 4)) if torch_fn else float("nan")
        if w:
            for key, t in zip(legs, (t_sym, t_dev, t_num, t_sci, t_tor)):
                legs[key].append(t)
        print(f"# {name}: window {w} done", flush=True)
    rec = dict(product=name, m=A.shape[0], k=A.shape[1], n=B.shape[1], nnz_a=int(A.nnz), nnz_b=int(B.nnz), nnz_c=P.nnz,
               products=info["products"], max_row_products=info["max_row_products"], max_row_c=info["max_row_c"],
               symbolic_bin_rows=info["symbolic_bin_rows"], numeric_bin_rows=info["numeric_bin_rows"],
               symbolic_probes=info["symbolic_probes"], device_bytes=info["device_bytes"], same_pattern_as_scipy=same_pattern,
               worst_diff_over_abs_product=worst, torch_note=torch_note, windows=args.windows, reps=args.reps)
    for key, ts in legs.items():
        if np.isnan(ts).all():
            continue
        rec[key] = round(float(np.median(ts)), 6)
        rec[key + "_spread"] = [round(min(ts), 6), round(max(ts), 6)]
    print(json.dumps(rec), flush=True)
    P.close()
    return rec, S


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="aa64,galerkin160,aat", help="aa<N>, galerkin<N>, aat")
    ap.add_argument("--tall", default="200000,20000,8", help="m,k,d of the aat leg")
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--reps", type=int, default=8, help="multiplies per timed numeric leg")
    ap.add_argument("--no-torch", dest="torch", action="store_false", help="skip the torch.sparse.mm reference")
    args = ap.parse_args()
    if args.windows < 5:
        ap.error("--windows: at least 5")
    args.tall = [int(v) for v in args.tall.split(",")]
    os.environ.setdefault("OMP_NUM_THREADS", "16")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("spgemm_bench.py needs a GPU: the engine has no CPU path")
    import spmv_mi355x as E
    rows = []
    for leg in args.legs.split(","):
        previous = None
        for name, A, B in products_of(leg, args):
            rec, previous = run(E, torch, name, A, previous if isinstance(B, str) else B, args)
            rows.append(rec)
    sp_ = lambda r, k: f"{r[k]:10.5f} {r[k + '_spread'][0]:9.5f} ..{r[k + '_spread'][1]:9.5f}" if k in r else f"{'-':>31s}"
    print(f"{'product':26s} {'nnz(C)':>11s} {'products':>12s} {'symbolic s':>10s} {'spread':>20s} {'(device s)':>10s} {'numeric s':>10s} "
          f"{'spread':>20s} {'scipy s':>10s} {'spread':>20s} {'torch s':>10s} {'spread':>20s}")
    for r in rows:
        print(f"{r['product']:26s} {r['nnz_c']:11d} {r['products']:12d} {sp_(r, 'symbolic_wall')} {r['symbolic_device']:10.5f} "
              f"{sp_(r, 'numeric')} {sp_(r, 'scipy')} {sp_(r, 'torch')}")


if __name__ == "__main__":
    main()
