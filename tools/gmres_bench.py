"""An inner step of restarted GMRES (spmv_mi355x_gmres; include/spmv_mi355x.h "GMRES(m)") against one SpMV of the same handle.

For a workload twin of bench.py the tool builds one sell_c_sigma handle in its own best layout and in one process, alternating
window by window, times
  floor:   time_device(A), HIP events over `--reps` back-to-back launches: what a step's product costs on its own;
  gmres:   `--cycles` whole cycles (max_iterations = cycles * restart) with tol = 0 (no stop on the tolerance) for every restart
           length of --restarts and, with --minv, the right preconditioner 1 / max(|a_ii|, 1);
           ms per inner step = (info.seconds of that call - info.seconds of a call with max_iterations = 0, i.e. setup, the explicit
           residual and the downloads) / steps done: the mean over whole cycles, cycle ends and restarts included. info.seconds is
           wall time and both calls allocate (the basis of restart + 1 vectors too), so the subtraction leaves allocation jitter: a
           calibration call raises the cycles until the loop alone lasts `--min-ms`.
The medians over the windows are reported with their spreads, the ratio step / floor, and the byte model beside it: step j moves
about 3 j + 12 vector passes of n values, a mean of 1.5 m + 10.5 per step of a cycle; `model_ms` is that many passes at the rate of
the --stream-tbs argument (TB/s), for comparison only.

The tool times steps only. Whether GMRES converges on a twin is not its question: a step costs the same whether the residual falls
or not. A run that stops before max_iterations (a breakdown, or a Krylov space that ends) is reported as nothing to time.

    python tools/gmres_bench.py                                    # nlpkkt240 fp64 (vectors beyond the Infinity Cache), cant fp64 (launch-bound)
    python tools/gmres_bench.py --runs cant:f64,cant:f32 --restarts 10,30,60 --minv
One JSON line per run and restart length, and a table at the end.

--precond sgs is a second mode with another question: what a triangular preconditioner (spmv_mi355x_gmres_tri) buys. On generated
operators (stencil<N>: the 27-point stencil of tools/solver_bench.py with --stencil-diag on the diagonal; convdiff<k>: the
convection-diffusion operator of tests/trsv_blocked_cases.py on a k x k grid) it solves A x = b to --tol with no preconditioner, with
minv = 1 / diag and with the blocked SGS of A at every --block-rows value (0 = a global handle pair), and reports per variant the
inner steps, the seconds of the whole call (median of the windows, with the spread), ms per inner step = (seconds - seconds of a call
with max_iterations = 0) / steps, and that step against one SpMV of the handle timed in the same windows. No threshold is set: the
table is what tells a user whether to turn it on.

    python tools/gmres_bench.py --precond sgs --runs stencil160:f64,convdiff1000:f64 --restarts 30 --block-rows 1024,4096,16384
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "spmv-research_amd", "python")):
    if p not in sys.path:
        sys.path.insert(0, p)


def inverse_diagonal(rp, ci, va, m):
    """1 / max(|a_ii|, 1): positive whatever the diagonal holds (a KKT matrix has a zero block there)"""
    rows = np.repeat(np.arange(m, dtype=np.int64), np.diff(rp))
    on = ci == rows
    d = np.zeros(m)
    d[rows[on]] = np.abs(va[on])
    return 1.0 / np.maximum(d, 1.0)


def run(E, torch, A, data, workload, dts, extra, args):
    m, n = A["m"], A["n"]
    if m != n:
        raise SystemExit(f"{workload}: {m} x {n} is not square")
    rp, ci, va = A["row_ptr"], A["col_idx"], np.ascontiguousarray(A["values"], np.float64)
    np_dtype = np.float32 if dts == "f32" else np.float64
    opts = dict(extra)
    if dts == "mixed":
        opts["value_storage"] = 1
    MA = E.Matrix(rp, ci, va, m, n, "sell_c_sigma", np_dtype, **opts)
    tdt = torch.float32 if dts == "f32" else torch.float64
    xa = (torch.rand(n, device="cuda", dtype=torch.float64) * 2 - 1).to(tdt)
    ya = torch.empty(m + 64, dtype=tdt, device="cuda")
    stream = torch.cuda.current_stream()
    b = np.random.default_rng(7).uniform(-1, 1, m).astype(np_dtype)
    minv = inverse_diagonal(rp, ci, va, m).astype(np_dtype) if args.minv else None
    rows = []
    for restart in args.restarts:
        solve = lambda steps: MA.gmres(b, restart=restart, minv=minv, tol=0.0, max_iterations=steps, history=False)
        legs = {k: [] for k in ("spmv", "gmres", "fixed", "ratio")}
        cal = solve(args.cycles * restart)
        cal = solve(args.cycles * restart)                    # the first call warmed up
        if cal["iterations"] < 1:
            raise SystemExit(f"{workload} {dts}: no step completed (stop {cal['stop']})")
        cycles = int(min(2000, max(args.cycles, np.ceil(args.min_ms * cal["iterations"] / (cal["seconds"] * 1e3) / restart))))
        steps = cycles * restart
        for w in range(args.windows + 1):                     # window 0 warms every leg up and is dropped
            t_a = MA.time_device(xa.data_ptr(), ya.data_ptr(), args.reps, stream.cuda_stream)
            torch.cuda.synchronize()
            r = solve(steps)
            fixed = solve(0)["seconds"] * 1e3
            done = r["iterations"]
            if done != steps or r["stop"] != 2:               # a stop before max_iterations: the host's run-ahead would be in the time
                raise SystemExit(f"{workload} {dts}: stop {r['stop']} after {done} of {steps} steps, nothing to time")
            t_c = (r["seconds"] * 1e3 - fixed) / done
            if w:
                for name, t in zip(legs, (t_a, t_c, fixed, t_c / t_a)):
                    legs[name].append(t)
        passes = 1.5 * restart + 10.5
        rec = dict(workload=workload, dtype=dts, opts=extra, data=data, format=MA.format_name, m=int(m), nnz=int(MA.nnz),
                   restart=restart, minv=bool(args.minv), steps=int(done), cycles=cycles, restarts=int(r["restarts"]), stop=int(r["stop"]),
                   windows=args.windows, spmv_reps=args.reps, model_passes=passes,
                   model_ms=round(passes * m * np.dtype(np_dtype).itemsize / (args.stream_tbs * 1e9), 5))
        for name, ts in legs.items():
            unit = "" if name == "ratio" else "_ms"
            rec[name + unit] = round(float(np.median(ts)), 5)
            rec[name + "_spread"] = [round(min(ts), 5), round(max(ts), 5)]
        print(json.dumps(rec), flush=True)
        rows.append(rec)
    MA.close()
    return rows


def convdiff_csr(k):
    """the operator of tests/trsv_blocked_cases.convdiff on a k x k grid as CSR, columns ascending: diagonal 4.1, west -1.6, east
    -0.4, south -1.3, north -0.7, row r times 1 + 0.2 u_r with u = default_rng(1).uniform(-1, 1, n)"""
    n = k * k
    r = np.arange(n, dtype=np.int64)
    i, j = r // k, r % k
    parts = [(i > 0, -k, -1.3), (j > 0, -1, -1.6), (np.ones(n, bool), 0, 4.1), (j < k - 1, 1, -0.4), (i < k - 1, k, -0.7)]
    rows = np.concatenate([r[ok] for ok, _, _ in parts])
    cols = np.concatenate([r[ok] + d for ok, d, _ in parts])
    vals = np.concatenate([np.full(int(ok.sum()), v) for ok, _, v in parts])
    o = np.lexsort((cols, rows))
    rows, cols, vals = rows[o], cols[o], vals[o]
    vals = vals * (1 + 0.2 * np.random.default_rng(1).uniform(-1, 1, n))[rows]
    rp = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n))]).astype(np.int32)
    return rp, cols.astype(np.int32), vals, n


def run_precond(E, torch, workload, dts, args):
    if workload.startswith("stencil"):
        from solver_bench import stencil27
        rp, ci, va, n = stencil27(int(workload[len("stencil"):]), args.stencil_diag)
        rp = np.asarray(rp, np.int32)
    elif workload.startswith("convdiff"):
        rp, ci, va, n = convdiff_csr(int(workload[len("convdiff"):]))
    else:
        raise SystemExit(f"--precond sgs runs on stencil<N> and convdiff<k>, not on {workload}")
    np_dtype = np.float32 if dts == "f32" else np.float64
    tdt = torch.float32 if dts == "f32" else torch.float64
    MA = E.Matrix(rp, ci, va, n, n, "sell_c_sigma", np_dtype)
    xa = (torch.rand(n, device="cuda", dtype=torch.float64) * 2 - 1).to(tdt)
    ya = torch.empty(n + 64, dtype=tdt, device="cuda")
    stream = torch.cuda.current_stream()
    b = np.random.default_rng(7).uniform(-1, 1, n).astype(np_dtype)
    on = ci == np.repeat(np.arange(n, dtype=np.int32), np.diff(rp))
    diag = np.ascontiguousarray(va[on]).astype(np_dtype)
    assert len(diag) == n
    variants = [("none", {}), ("minv", dict(minv=(1.0 / diag).astype(np_dtype)))]
    handles = []
    for B in args.block_rows:
        L = E.TriangularSolve(rp, ci, va, n, "lower", "stored", np_dtype, block_rows=B or None)
        U = E.TriangularSolve(rp, ci, va, n, "upper", "stored", np_dtype, block_rows=B or None)
        handles += [L, U]
        dropped = (L.block_info()["nnz_dropped"] + U.block_info()["nnz_dropped"]) / max(int(on.size - n), 1)
        variants.append((f"sgs B={B}" if B else "sgs global", dict(precond=(L, diag, U), dropped_share=round(dropped, 4),
                                                                   trsv_launches=L.info["launches"] + U.info["launches"])))
    rows = []
    for restart in args.restarts:
        for name, kw in variants:
            extra = {k: kw[k] for k in ("dropped_share", "trsv_launches") if k in kw}
            call = {k: v for k, v in kw.items() if k in ("minv", "precond")}
            solve = lambda steps: MA.gmres(b, restart=restart, tol=args.tol, max_iterations=steps, history=False, **call)
            solve(args.max_iterations)                        # warms up
            legs = {k: [] for k in ("spmv", "seconds", "step", "ratio")}
            for w in range(args.windows):
                t_a = MA.time_device(xa.data_ptr(), ya.data_ptr(), args.reps, stream.cuda_stream)
                torch.cuda.synchronize()
                r = solve(args.max_iterations)
                fixed = solve(0)["seconds"]
                t_c = (r["seconds"] - fixed) * 1e3 / max(r["iterations"], 1)
                for key, t in zip(legs, (t_a, r["seconds"], t_c, t_c / t_a)):
                    legs[key].append(t)
            rec = dict(workload=workload, dtype=dts, format=MA.format_name, n=int(n), nnz=int(MA.nnz), restart=restart, precond=name,
                       tol=args.tol, steps=int(r["iterations"]), stop=int(r["stop"]), rnorm_over_b=float(r["rnorm"] / r["rnorm0"]),
                       windows=args.windows, **extra)
            for key, ts in legs.items():
                rec[key] = round(float(np.median(ts)), 5)
                rec[key + "_spread"] = [round(min(ts), 5), round(max(ts), 5)]
            print(json.dumps(rec), flush=True)
            rows.append(rec)
    MA.close()
    for T in handles:
        T.close()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", default="nlpkkt240:f64,cant:f64", help="workload:f64|f32|mixed[:k=v+k=v],...")
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--restarts", default="10,30", help="restart lengths, each timed on its own")
    ap.add_argument("--cycles", type=int, default=4, help="whole cycles per timed call, at least")
    ap.add_argument("--min-ms", type=float, default=300.0, help="raise the cycles until a timed call's loop lasts this long")
    ap.add_argument("--stream-tbs", type=float, default=4.0, help="TB/s of the byte model's column")
    ap.add_argument("--reps", type=int, default=50, help="SpMV launches per timed floor leg")
    ap.add_argument("--minv", action="store_true", help="precondition with 1 / max(|a_ii|, 1)")
    ap.add_argument("--scale", type=float, default=1.0, help="shrink the workloads")
    ap.add_argument("--precond", default="", choices=("", "sgs"), help="sgs: the preconditioner comparison on generated operators")
    ap.add_argument("--block-rows", default="1024,4096,16384", help="--precond sgs: block sizes of the blocked SGS, 0 = global handles")
    ap.add_argument("--tol", type=float, default=1e-8, help="--precond sgs: the tolerance to solve to")
    ap.add_argument("--max-iterations", type=int, default=3000, help="--precond sgs: the cap on the inner steps")
    ap.add_argument("--stencil-diag", type=float, default=27.0, help="--precond sgs: the diagonal of stencil<N> (26 neighbours of -1)")
    args = ap.parse_args()
    if args.windows < 5:
        ap.error("--windows: at least 5")
    args.restarts = [int(v) for v in args.restarts.split(",")]
    os.environ.setdefault("OMP_NUM_THREADS", "16")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("gmres_bench.py needs a GPU: the engine has no CPU path")
    import spmv_mi355x as E
    if args.precond:
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        args.block_rows = [int(v) for v in args.block_rows.split(",") if v != ""]
        rows = []
        for item in args.runs.split(","):
            w, dts = item.split(":")[:2]
            rows += run_precond(E, torch, w, dts, args)
        print(f"{'workload':13s} {'dtype':5s} {'m':>4s} {'precond':>13s} {'dropped':>8s} {'steps':>6s} {'stop':>4s} {'seconds':>9s} "
              f"{'spread':>19s} {'ms/step':>9s} {'spmv ms':>9s} {'step / spmv':>11s}")
        for r in rows:
            dropped = f"{100 * r['dropped_share']:7.2f}%" if "dropped_share" in r else " " * 8
            print(f"{r['workload']:13s} {r['dtype']:5s} {r['restart']:4d} {r['precond']:>13s} {dropped} {r['steps']:6d} {r['stop']:4d} "
                  f"{r['seconds']:9.4f} {r['seconds_spread'][0]:9.4f} ..{r['seconds_spread'][1]:8.4f} {r['step']:9.4f} {r['spmv']:9.4f} "
                  f"{r['ratio']:11.2f}")
        return
    import bench
    import spmv_host as H
    rows, loaded = [], {}
    for item in args.runs.split(","):
        w, dts, *more = item.split(":")
        extra = {kv.split("=")[0]: int(kv.split("=")[1]) for kv in (more[0].split("+") if more else [])}
        if w not in loaded:
            loaded.clear()                                 # one workload in host memory at a time
            loaded[w] = bench.load_workload(H, w, args.scale)
        A, data = loaded[w]
        rows += run(E, torch, A, data, w, dts, extra, args)
    print(f"{'workload':10s} {'dtype':6s} {'format':28s} {'m':>4s} {'minv':>5s} {'spmv ms':>9s} {'gmres ms/step':>13s} {'model ms':>9s} "
          f"{'step / floor':>12s}  spread of the ratio")
    for r in rows:
        print(f"{r['workload']:10s} {r['dtype']:6s} {r['format']:28s} {r['restart']:4d} {str(r['minv']):>5s} {r['spmv_ms']:9.4f} "
              f"{r['gmres_ms']:13.4f} {r['model_ms']:9.4f} {r['ratio']:12.3f}  {r['ratio_spread'][0]:.3f} .. {r['ratio_spread'][1]:.3f}")


if __name__ == "__main__":
    main()
