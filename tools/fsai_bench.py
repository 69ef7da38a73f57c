"""What the FSAI preconditioner (spmv_mi355x_fsai_*; include/spmv_mi355x.h "FSAI") buys the tol-based CG in iterations AND in
seconds, what it costs to set up, and what one application costs against one SpMV of A. Follows tools/pcg_tri_bench.py: the same
operator (stencil<N>: the 27-point stencil of tools/solver_bench.py with --stencil-diag on the diagonal), one sell_c_sigma handle of
A, tol 1e-8, and for every variant
    none | jacobi = (None, 1 / diag, None) | fsai p = Fsai on the pattern tril(A)^p for every p of --power
in one process, alternating window by window (window 0 warms every leg up and is dropped):
  spmv:      time_device(A), HIP events over --reps back-to-back launches;
  apply:     for the FSAI variants, HIP events over --reps back-to-back apply_device calls (two SpMVs each);
  solve:     the whole call to --tol: iterations, stop, info.seconds;
  iteration: a call with tol = 0 and max_iterations = --steps, minus a call with max_iterations = 0, over --steps.
The setup of every FSAI handle is reported once (it is not repeated per window): the seconds of the row kernel, of the download of G,
of the two spmv_mi355x_create calls and of the whole fsai_create, the pattern's entries and widest row, the rows that fell back and
the bytes per non-zero of the G and G^t handles. The medians over the windows are reported with their min .. max spreads. No
threshold is set and no speed is promised.

    python tools/fsai_bench.py                                       # stencil160 fp64, power 1 and 2
    python tools/fsai_bench.py --runs stencil96:f32 --power 1
One JSON line per variant, and a table at the end."""
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


def run(E, torch, workload, dts, args):
    if not workload.startswith("stencil"):
        raise SystemExit(f"fsai_bench.py runs on stencil<N>, not on {workload}")
    from solver_bench import stencil27
    rp, ci, va, n = stencil27(int(workload[len("stencil"):]), args.stencil_diag)
    rp = np.asarray(rp, np.int32)
    np_dtype = np.float32 if dts == "f32" else np.float64
    tdt = torch.float32 if dts == "f32" else torch.float64
    MA = E.Matrix(rp, ci, va, n, n, "sell_c_sigma", np_dtype)
    xa = (torch.rand(n, device="cuda", dtype=torch.float64) * 2 - 1).to(tdt)
    ya = torch.empty(n + 64, dtype=tdt, device="cuda")
    stream = torch.cuda.current_stream()
    b = np.random.default_rng(7).uniform(-1, 1, n).astype(np_dtype)
    diag = va[ci == np.repeat(np.arange(n, dtype=np.int32), np.diff(rp))]
    assert len(diag) == n
    variants = [("none", None, {}), ("jacobi", (None, (1.0 / diag).astype(np_dtype), None), {})]
    handles = []
    for power in args.power:
        t0 = time.perf_counter()
        pat = None if power == 1 else E.fsai_pattern(rp, ci, n, power)
        t_pat = time.perf_counter() - t0
        F = E.Fsai(rp, ci, va, n, pat, "sell_c_sigma", np_dtype)
        handles.append(F)
        info = F.info()
        extra = dict(pattern_seconds=round(t_pat, 4), pattern_nnz=info["nnz"], max_row=info["max_row"], fallback_rows=info["fallback_rows"],
                     setup_seconds=round(info["setup_seconds"], 4), kernel_seconds=round(info["kernel_seconds"], 5),
                     download_seconds=round(info["download_seconds"], 4), create_g_seconds=round(info["create_g_seconds"], 4),
                     create_gt_seconds=round(info["create_gt_seconds"], 4), g_format=F.G.format_name, gt_format=F.Gt.format_name,
                     g_bytes_per_nnz=round(F.G.mem_footprint / info["nnz"], 3), gt_bytes_per_nnz=round(F.Gt.mem_footprint / info["nnz"], 3),
                     a_bytes_per_nnz=round(MA.mem_footprint / MA.nnz, 3))
        variants.append((f"fsai p={power}", F, extra))
        print(f"# built {variants[-1][0]}: {extra}", flush=True)
    solve = lambda M, tol, steps: MA.pcg_tri(b, precond=M, tol=tol, max_iterations=steps, history=False)

    def time_apply(F):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(args.reps):
            F.apply_device(xa.data_ptr(), ya.data_ptr(), stream.cuda_stream)
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1) / args.reps

    legs = {name: {k: [] for k in ("spmv", "seconds", "iter_ms", "ratio", "apply", "apply_ratio")} for name, _, _ in variants}
    last = {}
    for w in range(args.windows + 1):                         # window 0 warms every leg up and is dropped
        for name, M, _ in variants:
            t_a = MA.time_device(xa.data_ptr(), ya.data_ptr(), args.reps, stream.cuda_stream)
            torch.cuda.synchronize()
            t_f = time_apply(M) if isinstance(M, E.Fsai) else float("nan")
            r = solve(M, args.tol, args.max_iterations)
            fixed = solve(M, 0.0, 0)["seconds"]
            s = solve(M, 0.0, args.steps)
            if s["iterations"] != args.steps or s["stop"] != 2:
                raise SystemExit(f"{workload} {dts} {name}: stop {s['stop']} after {s['iterations']} of {args.steps} steps at tol = 0")
            t_c = (s["seconds"] - fixed) * 1e3 / args.steps
            last[name] = r
            if w:
                for key, t in zip(legs[name], (t_a, r["seconds"], t_c, t_c / t_a, t_f, t_f / t_a)):
                    legs[name][key].append(t)
        print(f"# window {w} done", flush=True)
    rows = []
    for name, M, extra in variants:
        r = last[name]
        rec = dict(workload=workload, dtype=dts, format=MA.format_name, n=int(n), nnz=int(MA.nnz), precond=name, tol=args.tol,
                   iterations=int(r["iterations"]), stop=int(r["stop"]), rnorm_over_b=float(r["rnorm"] / r["rnorm0"]),
                   windows=args.windows, steps=args.steps, reps=args.reps, **extra)
        for key, ts in legs[name].items():
            if np.isnan(ts).all():
                continue
            rec[key] = round(float(np.median(ts)), 5)
            rec[key + "_spread"] = [round(min(ts), 5), round(max(ts), 5)]
        print(json.dumps(rec), flush=True)
        rows.append(rec)
    MA.close()
    for F in handles:
        F.close()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", default="stencil160:f64", help="stencil<N>:f64|f32,...")
    ap.add_argument("--power", default="1,2", help="the patterns tril(A)^p, p in 1..3")
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--tol", type=float, default=1e-8, help="the tolerance of the solve leg")
    ap.add_argument("--max-iterations", type=int, default=3000, help="the cap of the solve leg")
    ap.add_argument("--steps", type=int, default=200, help="iterations of the tol = 0 leg")
    ap.add_argument("--reps", type=int, default=50, help="launches per timed SpMV / apply leg")
    ap.add_argument("--stencil-diag", type=float, default=27.0, help="the diagonal of stencil<N> (26 neighbours of -1)")
    args = ap.parse_args()
    if args.windows < 5:
        ap.error("--windows: at least 5")
    args.power = [int(v) for v in args.power.split(",") if v != ""]
    os.environ.setdefault("OMP_NUM_THREADS", "16")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("fsai_bench.py needs a GPU: the engine has no CPU path")
    import spmv_mi355x as E
    rows = []
    for item in args.runs.split(","):
        w, dts = item.split(":")[:2]
        rows += run(E, torch, w, dts, args)
    print(f"{'workload':11s} {'dtype':5s} {'precond':>10s} {'iters':>6s} {'stop':>4s} {'seconds':>9s} {'spread':>19s} {'ms/iter':>8s} "
          f"{'spmv ms':>8s} {'iter / spmv':>11s} {'apply ms':>9s} {'apply / spmv':>12s} {'spread':>14s}")
    for r in rows:
        ap_ = f"{r['apply']:9.4f} {r['apply_ratio']:12.2f} {r['apply_ratio_spread'][0]:6.2f} ..{r['apply_ratio_spread'][1]:6.2f}" if "apply" in r else ""
        print(f"{r['workload']:11s} {r['dtype']:5s} {r['precond']:>10s} {r['iterations']:6d} {r['stop']:4d} {r['seconds']:9.4f} "
              f"{r['seconds_spread'][0]:9.4f} ..{r['seconds_spread'][1]:8.4f} {r['iter_ms']:8.4f} {r['spmv']:8.4f} {r['ratio']:11.2f} {ap_}")
    print(f"{'workload':11s} {'dtype':5s} {'precond':>10s} {'nnz(G)':>11s} {'widest':>6s} {'fell':>5s} {'pattern s':>9s} {'setup s':>8s} {'kernel s':>9s} "
          f"{'download s':>10s} {'create G s':>10s} {'create Gt s':>11s} {'B/nnz G':>8s} {'B/nnz Gt':>8s} {'B/nnz A':>8s}")
    for r in rows:
        if "pattern_nnz" in r:
            print(f"{r['workload']:11s} {r['dtype']:5s} {r['precond']:>10s} {r['pattern_nnz']:11d} {r['max_row']:6d} {r['fallback_rows']:5d} "
                  f"{r['pattern_seconds']:9.3f} {r['setup_seconds']:8.3f} {r['kernel_seconds']:9.4f} {r['download_seconds']:10.3f} "
                  f"{r['create_g_seconds']:10.3f} {r['create_gt_seconds']:11.3f} {r['g_bytes_per_nnz']:8.2f} {r['gt_bytes_per_nnz']:8.2f} "
                  f"{r['a_bytes_per_nnz']:8.2f}")


if __name__ == "__main__":
    main()
