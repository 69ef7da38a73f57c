"""What a triangular preconditioner buys the tol-based CG (spmv_mi355x_pcg_tri; include/spmv_mi355x.h "CG preconditioned by
triangular solves"), in iterations AND in seconds, and what one CG iteration costs against one SpMV of the same handle.

On a generated SPD operator (stencil<N>: the 27-point stencil of tools/solver_bench.py with --stencil-diag on the diagonal) the tool
builds one sell_c_sigma handle and, for every variant
    none | jacobi = (None, 1 / diag, None) | blocked SGS of A at every --block-rows value (0 = a global handle pair),
times in one process, alternating window by window (window 0 warms every leg up and is dropped):
  spmv:      time_device(A), HIP events over `--reps` back-to-back launches;
  trsv:      for the SGS variants, time_device of the lower and of the upper handle on their own, HIP events over `--reps` solves;
  solve:     the whole call to --tol: iterations, stop, info.seconds (wall time: uploads, allocations, the loop, the explicit
             residual, the download);
  iteration: a call with tol = 0 and max_iterations = --steps, minus a call with max_iterations = 0 (set-up, the explicit residual
             and the downloads), over --steps: ms per iteration with no stop and no run-ahead in it, and that against the SpMV.
The medians over the windows are reported with their min .. max spreads. No threshold is set and no speed is promised: the table is
what tells a user whether block SGS beats Jacobi in seconds and not only in iterations.

With --sweeps 2,3,4,8 the global SGS also runs with its two triangular solves replaced by that many Jacobi sweeps
(spmv_mi355x_trsv_set_sweeps, the same count on both handles; one pair of global handles serves every count and the exact leg), as
further variants in the same windows. grid2d<N> (the 5-point operator of tools/amg_bench.py, shift 0.001) is a workload too.

    python tools/pcg_tri_bench.py                                    # stencil160 fp64, B = 1024, 4096, 16384
    python tools/pcg_tri_bench.py --runs stencil160:f64,grid2d2000:f64 --block-rows 0,4096 --sweeps 2,3,4,8
    python tools/pcg_tri_bench.py --runs stencil96:f32 --block-rows 0,4096
One JSON line per variant, and a table at the end."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "spmv-research_amd", "python"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)


def run(E, torch, workload, dts, args):
    if workload.startswith("grid2d"):
        from amg_bench import grid2d
        rp, ci, va, n = grid2d(int(workload[len("grid2d"):]), 0.001)
    elif workload.startswith("stencil"):
        from solver_bench import stencil27
        rp, ci, va, n = stencil27(int(workload[len("stencil"):]), args.stencil_diag)
    else:
        raise SystemExit(f"pcg_tri_bench.py runs on stencil<N> and grid2d<N>, not on {workload}")
    rp = np.asarray(rp, np.int32)
    np_dtype = np.float32 if dts == "f32" else np.float64
    tdt = torch.float32 if dts == "f32" else torch.float64
    MA = E.Matrix(rp, ci, va, n, n, "sell_c_sigma", np_dtype)
    xa = (torch.rand(n, device="cuda", dtype=torch.float64) * 2 - 1).to(tdt)
    ya = torch.empty(n + 64, dtype=tdt, device="cuda")
    stream = torch.cuda.current_stream()
    b = np.random.default_rng(7).uniform(-1, 1, n).astype(np_dtype)
    offdiag = int(rp[-1]) - n
    diag = va[ci == np.repeat(np.arange(n, dtype=np.int32), np.diff(rp))]
    assert len(diag) == n
    variants = [("none", None, {}), ("jacobi", (None, (1.0 / diag).astype(np_dtype), None), {})]
    handles = []
    for B in args.block_rows:
        L, d, U = E.sgs_precond(rp, ci, va, n, np_dtype, block_rows=B or None)
        handles += [L, U]
        dropped = (L.block_info()["nnz_dropped"] + U.block_info()["nnz_dropped"]) / max(offdiag, 1)
        variants.append((f"sgs B={B}" if B else "sgs global", (L, d, U),
                         dict(dropped_share=round(dropped, 4), trsv_launches=L.info["launches"] + U.info["launches"],
                              block_levels=max(L.info["levels"], U.info["levels"]))))
        print(f"# built {variants[-1][0]}: {variants[-1][2]}", flush=True)
    if args.sweeps:
        # the swept variants share ONE global pair (that of --block-rows 0 when it is there); `sweeps` is set before a variant's legs
        pair = next((M for name, M, _ in variants if name == "sgs global"), None)
        if pair is None:
            pair = E.sgs_precond(rp, ci, va, n, np_dtype)
            handles += [pair[0], pair[2]]
        for s in args.sweeps:
            variants.append((f"sgs sweeps={s}", pair, dict(sweeps=s, trsv_launches=2 * min(s, pair[0].info["levels"]))))
    solve = lambda M, tol, steps: MA.pcg_tri(b, precond=M, tol=tol, max_iterations=steps, history=False)
    legs = {name: {k: [] for k in ("spmv", "seconds", "iter_ms", "ratio", "trsv_lower", "trsv_upper")} for name, _, _ in variants}
    last = {}
    for w in range(args.windows + 1):                         # window 0 warms every leg up and is dropped
        for name, M, extra in variants:
            for T in (M[0], M[2]) if M is not None and M[0] is not None else ():
                T.set_sweeps(extra.get("sweeps", 0))
            t_a = MA.time_device(xa.data_ptr(), ya.data_ptr(), args.reps, stream.cuda_stream)
            torch.cuda.synchronize()
            t_l = t_u = float("nan")
            if M is not None and M[0] is not None:
                t_l = M[0].time_device(xa.data_ptr(), ya.data_ptr(), args.reps, stream.cuda_stream)
                t_u = M[2].time_device(xa.data_ptr(), ya.data_ptr(), args.reps, stream.cuda_stream)
                torch.cuda.synchronize()
            r = solve(M, args.tol, args.max_iterations)
            fixed = solve(M, 0.0, 0)["seconds"]
            s = solve(M, 0.0, args.steps)
            if s["iterations"] != args.steps or s["stop"] != 2:
                raise SystemExit(f"{workload} {dts} {name}: stop {s['stop']} after {s['iterations']} of {args.steps} steps at tol = 0")
            t_c = (s["seconds"] - fixed) * 1e3 / args.steps
            last[name] = r
            if w:
                for key, t in zip(legs[name], (t_a, r["seconds"], t_c, t_c / t_a, t_l, t_u)):
                    legs[name][key].append(t)
        print(f"# window {w} done", flush=True)
    rows = []
    for name, M, extra in variants:
        r = last[name]
        rec = dict(workload=workload, dtype=dts, format=MA.format_name, n=int(n), nnz=int(MA.nnz), precond=name, tol=args.tol,
                   iterations=int(r["iterations"]), stop=int(r["stop"]), rnorm_over_b=float(r["rnorm"] / r["rnorm0"]),
                   windows=args.windows, steps=args.steps, spmv_reps=args.reps, **extra)
        for key, ts in legs[name].items():
            if np.isnan(ts).all():
                continue
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
    ap.add_argument("--runs", default="stencil160:f64", help="stencil<N>:f64|f32,...")
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--block-rows", default="1024,4096,16384", help="block sizes of the blocked SGS, 0 = global handles")
    ap.add_argument("--sweeps", default="", help="Jacobi-sweep counts of the global SGS to run beside the exact forms, e.g. 2,3,4,8")
    ap.add_argument("--tol", type=float, default=1e-8, help="the tolerance of the solve leg")
    ap.add_argument("--max-iterations", type=int, default=3000, help="the cap of the solve leg")
    ap.add_argument("--steps", type=int, default=200, help="iterations of the tol = 0 leg")
    ap.add_argument("--reps", type=int, default=50, help="launches per timed SpMV / triangular solve leg")
    ap.add_argument("--stencil-diag", type=float, default=27.0, help="the diagonal of stencil<N> (26 neighbours of -1)")
    args = ap.parse_args()
    if args.windows < 5:
        ap.error("--windows: at least 5")
    args.block_rows = [int(v) for v in args.block_rows.split(",") if v != ""]
    args.sweeps = [int(v) for v in args.sweeps.split(",") if v != ""]
    if any(v < 1 for v in args.sweeps):
        ap.error("--sweeps: sweep counts are at least 1")
    os.environ.setdefault("OMP_NUM_THREADS", "16")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("pcg_tri_bench.py needs a GPU: the engine has no CPU path")
    import spmv_mi355x as E
    rows = []
    for item in args.runs.split(","):
        w, dts = item.split(":")[:2]
        rows += run(E, torch, w, dts, args)
    print(f"{'workload':11s} {'dtype':5s} {'precond':>12s} {'dropped':>8s} {'iters':>6s} {'stop':>4s} {'seconds':>9s} {'spread':>19s} "
          f"{'ms/iter':>8s} {'spmv ms':>8s} {'iter / spmv':>11s} {'spread':>14s} {'L^-1 ms':>8s} {'U^-1 ms':>8s}")
    for r in rows:
        dropped = f"{100 * r['dropped_share']:7.2f}%" if "dropped_share" in r else " " * 8
        trsv = f"{r['trsv_lower']:8.4f} {r['trsv_upper']:8.4f}" if "trsv_lower" in r else ""
        print(f"{r['workload']:11s} {r['dtype']:5s} {r['precond']:>12s} {dropped} {r['iterations']:6d} {r['stop']:4d} {r['seconds']:9.4f} "
              f"{r['seconds_spread'][0]:9.4f} ..{r['seconds_spread'][1]:8.4f} {r['iter_ms']:8.4f} {r['spmv']:8.4f} {r['ratio']:11.2f} "
              f"{r['ratio_spread'][0]:6.2f} ..{r['ratio_spread'][1]:6.2f} {trsv}")


if __name__ == "__main__":
    main()
