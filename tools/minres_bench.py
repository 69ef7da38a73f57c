"""A MINRES iteration (spmv_mi355x_minres; include/spmv_mi355x.h "MINRES") against its one-SpMV floor.

For a workload twin of bench.py the tool builds one sell_c_sigma handle in its own best layout and in one process, alternating
window by window, times
  floor:   time_device(A), HIP events over `--reps` back-to-back launches: what an iteration's product costs on its own;
  minres:  iterations with tol = 0 (no stop on the tolerance), --shift and, with --minv, the preconditioner 1 / max(|a_ii|, 1);
           ms per iteration = (info.seconds of that call - info.seconds of a call with max_iterations = 0, i.e. setup, the explicit
           residual and the downloads) / iterations done. info.seconds is wall time and both calls allocate, so the subtraction
           leaves allocation jitter of a fraction of a ms: a calibration call raises `--iters` until the loop alone lasts
           `--min-ms`, which keeps that jitter below a percent on the launch-bound workloads too.
The medians over the windows are reported with their spreads, and the ratio iteration / floor: 1.0 would be an iteration whose three
vector kernels (15 vector passes of n values; 16 with --minv) are free.

The tool times iterations only. Whether MINRES converges on a twin is not its question: the recurrences cost the same whether the
residual falls or not, and a twin's conditioning was never examined. The twins are not all symmetric either (the product does not
care); a run whose scalars leave the finite range ends in stop 4 before max_iterations and is reported as nothing to time.

    python tools/minres_bench.py                                   # nlpkkt240 fp64 (vectors beyond the Infinity Cache), cant fp64 (launch-bound)
    python tools/minres_bench.py --runs cant:f64,cant:f32 --windows 7 --minv
    python tools/minres_bench.py --runs nlpkkt240:f64:sell_values=2
One JSON line per run and a table at the end.
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
    solve = lambda iters: MA.minres(b, shift=args.shift, minv=minv, tol=0.0, max_iterations=iters, history=False)
    legs = {k: [] for k in ("spmv", "minres", "fixed", "ratio")}
    done = None
    cal = solve(args.iters)
    cal = solve(args.iters)                               # the first call warmed up
    if cal["iterations"] < 1:
        raise SystemExit(f"{workload} {dts}: no iteration completed (stop {cal['stop']})")
    iters = int(min(50000, max(args.iters, np.ceil(args.min_ms * cal["iterations"] / (cal["seconds"] * 1e3)))))
    for w in range(args.windows + 1):                     # window 0 warms every leg up and is dropped
        t_a = MA.time_device(xa.data_ptr(), ya.data_ptr(), args.reps, stream.cuda_stream)
        torch.cuda.synchronize()
        r = solve(iters)
        fixed = solve(0)["seconds"] * 1e3
        done = r["iterations"]
        if done < 1 or r["stop"] != 2:                    # a stop before max_iterations: the host's run-ahead would be in the time
            raise SystemExit(f"{workload} {dts}: stop {r['stop']} after {done} of {iters} iterations, nothing to time")
        t_c = (r["seconds"] * 1e3 - fixed) / done
        if w:
            for name, t in zip(legs, (t_a, t_c, fixed, t_c / t_a)):
                legs[name].append(t)
    rec = dict(workload=workload, dtype=dts, opts=extra, data=data, format=MA.format_name, m=int(m), nnz=int(MA.nnz), shift=args.shift,
               minv=bool(args.minv), iterations=int(done), stop=int(r["stop"]), prnorm_over_prnorm0=float(r["prnorm"] / r["prnorm0"]),
               windows=args.windows, spmv_reps=args.reps)
    for name, ts in legs.items():
        unit = "" if name == "ratio" else "_ms"
        rec[name + unit] = round(float(np.median(ts)), 5)
        rec[name + "_spread"] = [round(min(ts), 5), round(max(ts), 5)]
    print(json.dumps(rec), flush=True)
    MA.close()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", default="nlpkkt240:f64,cant:f64", help="workload:f64|f32|mixed[:k=v+k=v],...")
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--iters", type=int, default=200, help="MINRES iterations per timed call, at least")
    ap.add_argument("--min-ms", type=float, default=300.0, help="raise the iterations until a timed call's loop lasts this long")
    ap.add_argument("--reps", type=int, default=50, help="SpMV launches per timed floor leg")
    ap.add_argument("--shift", type=float, default=0.0)
    ap.add_argument("--minv", action="store_true", help="precondition with 1 / max(|a_ii|, 1)")
    ap.add_argument("--scale", type=float, default=1.0, help="shrink the workloads")
    args = ap.parse_args()
    if args.windows < 5:
        ap.error("--windows: at least 5")
    os.environ.setdefault("OMP_NUM_THREADS", "16")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("minres_bench.py needs a GPU: the engine has no CPU path")
    import bench
    import spmv_host as H
    import spmv_mi355x as E
    rows, loaded = [], {}
    for item in args.runs.split(","):
        w, dts, *more = item.split(":")
        extra = {kv.split("=")[0]: int(kv.split("=")[1]) for kv in (more[0].split("+") if more else [])}
        if w not in loaded:
            loaded.clear()                                 # one workload in host memory at a time
            loaded[w] = bench.load_workload(H, w, args.scale)
        A, data = loaded[w]
        rows.append(run(E, torch, A, data, w, dts, extra, args))
    print(f"{'workload':10s} {'dtype':6s} {'format':28s} {'minv':>5s} {'spmv ms':>9s} {'minres ms/it':>12s} {'it / floor':>10s}  spread of the ratio")
    for r in rows:
        print(f"{r['workload']:10s} {r['dtype']:6s} {r['format']:28s} {str(r['minv']):>5s} {r['spmv_ms']:9.4f} {r['minres_ms']:12.4f} "
              f"{r['ratio']:10.3f}  {r['ratio_spread'][0]:.3f} .. {r['ratio_spread'][1]:.3f}")


if __name__ == "__main__":
    main()
