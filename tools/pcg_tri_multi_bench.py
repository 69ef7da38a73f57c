"""What k right-hand sides through one tol-based CG (Matrix.pcg_tri_multi) cost per right-hand side against k single solves
(Matrix.pcg_tri) on the same handles in the same run, and the same for the AMG cycle alone (Amg.apply_multi_device against k calls of
Amg.apply_device). Follows tools/amg_bench.py: one sell_c_sigma handle of A, and for every preconditioner
    none | jacobi = (None, 1 / diag(A), None) | fsai = Fsai on tril(A) | amg t=<theta> = Amg with every theta of --theta
(--fold-rows adds, per theta, a hierarchy per value whose small levels run as one launch: "amg t=<theta> fold=<rows>")
(--precond picks among them; sgs, not in the default list, adds the global SGS of A, sgs_precond, and with --block-rows a blocked
SGS per size: their k-column solves go through Matrix.pcg_trsm_multi and the k-column triangular solve)
and every k of --rhs, in one process, alternating window by window (window 0 warms every leg up and is dropped):
  solve:  per window the kmax single solves of the columns of B (seeded uniform), each to --tol with the cap --max-iterations, then
          the k-column solve of B[:, :k] for every k. Reported per k: info.seconds of the k-column solve over k, the mean of
          info.seconds of the first k single solves, and their ratio. Both sides stop by the same rule per column (the columns return
          the same bits), so a cap that is reached is reached on both sides.
  cycle:  for AMG, HIP events over --reps back-to-back apply_multi_device calls on a resident n x k block (ld = k), over k, against
          HIP events over --reps rounds of k apply_device calls on k resident vectors; ms per column and their ratio.
Beside the figures: apply_multi_plan(k) (matrix passes, launches) of the hierarchy, and spmm_plan(k) of A.
Each figure is the median over the windows with its min .. max spread. No threshold is set and no ratio is promised.

    python tools/pcg_tri_multi_bench.py                                   # grid2d2000:f64 and stencil160:f64, k = 1, 2, 4, 8
    python tools/pcg_tri_multi_bench.py --runs grid2d2000:f64 --rhs 1,4 --theta 0.08
    python tools/pcg_tri_multi_bench.py --runs stencil160:f64 --precond sgs,amg --block-rows 4096 --theta 0.08
One JSON line per (workload, preconditioner, k), and two tables at the end."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "spmv-research_amd", "python"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)


def operator(workload, args):
    if workload.startswith("stencil"):
        from solver_bench import stencil27
        rp, ci, va, n = stencil27(int(workload[len("stencil"):]), args.stencil_diag)
    elif workload.startswith("grid2d"):
        from amg_bench import grid2d
        rp, ci, va, n = grid2d(int(workload[len("grid2d"):]), args.shift)
    else:
        raise SystemExit(f"pcg_tri_multi_bench.py runs on stencil<N> and grid2d<N>, not on {workload}")
    return np.asarray(rp, np.int32), np.asarray(ci, np.int32), np.asarray(va, np.float64), n


def run(E, torch, workload, dts, args):
    rp, ci, va, n = operator(workload, args)
    np_dtype = np.float32 if dts == "f32" else np.float64
    tdt = torch.float32 if dts == "f32" else torch.float64
    kmax = max(args.rhs)
    MA = E.Matrix(rp, ci, va, n, n, "sell_c_sigma", np_dtype)
    B = np.ascontiguousarray(np.random.default_rng(7).uniform(-1, 1, (n, kmax)).astype(np_dtype))
    cols = [np.ascontiguousarray(B[:, j]) for j in range(kmax)]
    rows_of = np.repeat(np.arange(n), np.diff(rp))
    diag = np.zeros(n)
    diag[rows_of[ci == rows_of]] = va[ci == rows_of]
    variants = []
    if "none" in args.precond:
        variants.append(("none", None))
    if "jacobi" in args.precond:
        variants.append(("jacobi", (None, (1.0 / diag).astype(np_dtype), None)))
    if "sgs" in args.precond:                                 # the global SGS of A, and a blocked one per --block-rows value
        for size in [None] + args.block_rows:
            variants.append(("sgs" if size is None else f"sgs B={size}", E.sgs_precond(rp, ci, va, n, dtype=np_dtype, block_rows=size)))
            print(f"# built {variants[-1][0]}: launches per solve {variants[-1][1][0].info['launches']} + {variants[-1][1][2].info['launches']}",
                  flush=True)
    if "fsai" in args.precond:
        variants.append(("fsai", E.Fsai(rp, ci, va, n, None, "sell_c_sigma", np_dtype)))
    # per theta the hierarchy as it is created (fold off), then one of its own per --fold-rows value with the small levels folded
    for theta, fold in [(t, f) for t in args.theta for f in [0] + args.fold_rows] if "amg" in args.precond else ():
        variants.append((f"amg t={theta:g}" + (f" fold={fold}" if fold else ""),
                         E.Amg(rp, ci, va, n, "sell_c_sigma", np_dtype, theta=theta, sweeps=args.sweeps)))
        variants[-1][1].set_fold(fold)
        info = variants[-1][1].info()
        print(f"# built {variants[-1][0]}: rows {info['rows']}, coarse {info['coarse']}, first folded level "
              f"{variants[-1][1].fold_info()['first_level']}, spmvs {info['spmvs_per_apply']}, launches {info['launches_per_apply']}", flush=True)
    stream = torch.cuda.current_stream()
    xs = [(torch.rand(n, device="cuda", dtype=torch.float64) * 2 - 1).to(tdt) for _ in range(kmax)]
    ys = [torch.empty(n, dtype=tdt, device="cuda") for _ in range(kmax)]

    def events(f):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(args.reps):
            f()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1) / args.reps

    def cycle_ms(M, k):
        """(ms per column of apply_multi_device, ms per column of k apply_device calls)"""
        X = torch.stack(xs[:k], dim=1).contiguous()
        Y = torch.empty((n, k), dtype=tdt, device="cuda")
        M.apply_multi_device(k, X.data_ptr(), k, Y.data_ptr(), k, stream.cuda_stream)       # the blocks exist before the clock runs
        multi = events(lambda: M.apply_multi_device(k, X.data_ptr(), k, Y.data_ptr(), k, stream.cuda_stream))

        def singles():
            for j in range(k):
                M.apply_device(xs[j].data_ptr(), ys[j].data_ptr(), stream.cuda_stream)
        return multi / k, events(singles) / k

    legs = {(name, k): {key: [] for key in ("multi", "single", "ratio", "cycle_multi", "cycle_single", "cycle_ratio")}
            for name, _ in variants for k in args.rhs}
    last = {}
    for w in range(args.windows + 1):                         # window 0 warms every leg up and is dropped
        for name, M in variants:
            single = [MA.pcg_tri(c, precond=M, tol=args.tol, max_iterations=args.max_iterations, history=False) for c in cols]
            for k in args.rhs:
                solve = MA.pcg_trsm_multi if name.startswith("sgs") else MA.pcg_tri_multi
                got = solve(np.ascontiguousarray(B[:, :k]), precond=M, tol=args.tol, max_iterations=args.max_iterations, history=False)
                t_m = got[0]["seconds"] / k
                t_s = float(np.mean([s["seconds"] for s in single[:k]]))
                cm = cs = float("nan")
                if isinstance(M, E.Amg):
                    cm, cs = cycle_ms(M, k)
                last[(name, k)] = (got, single[:k])
                if w:
                    for key, t in zip(legs[(name, k)], (t_m, t_s, t_m / t_s, cm, cs, cm / cs)):
                        legs[(name, k)][key].append(t)
        print(f"# window {w} done", flush=True)
    rows = []
    for name, M in variants:
        for k in args.rhs:
            got, single = last[(name, k)]
            same = all(np.array_equal(g["x"], s["x"]) and g["iterations"] == s["iterations"] for g, s in zip(got, single))
            rec = dict(workload=workload, dtype=dts, format=MA.format_name, n=int(n), nnz_a=int(MA.nnz), precond=name, k=k, tol=args.tol,
                       max_iterations=args.max_iterations, iterations=[int(g["iterations"]) for g in got], stops=[int(g["stop"]) for g in got],
                       spmm_calls=int(got[0]["spmv_calls"]), columns_equal_singles=bool(same), spmm_plan_a=list(MA.spmm_plan(k)),
                       windows=args.windows, reps=args.reps)
            if isinstance(M, E.Amg):
                rec["plan_passes"], rec["plan_launches"] = M.apply_multi_plan(k)
                rec["single_spmvs"], rec["single_launches"] = M.info()["spmvs_per_apply"], M.info()["launches_per_apply"]
            for key, ts in legs[(name, k)].items():
                if np.isnan(ts).all():
                    continue
                rec[key] = round(float(np.median(ts)), 6)
                rec[key + "_spread"] = [round(float(np.min(ts)), 6), round(float(np.max(ts)), 6)]
            print(json.dumps(rec), flush=True)
            rows.append(rec)
    for _, M in variants:
        for h in M if isinstance(M, tuple) else (M,):
            if hasattr(h, "close"):
                h.close()
    MA.close()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", default="grid2d2000:f64,stencil160:f64", help="stencil<N>:f64|f32 or grid2d<N>:f64|f32, comma separated")
    ap.add_argument("--rhs", default="1,2,4,8", help="the column counts k")
    ap.add_argument("--precond", default="none,jacobi,fsai,amg", help="which of none, jacobi, sgs, fsai, amg to run; sgs is the global "
                    "SGS of A through Matrix.pcg_trsm_multi")
    ap.add_argument("--block-rows", default="", help="with --precond sgs: a blocked SGS per size beside the global one, e.g. 4096")
    ap.add_argument("--theta", default="0.08,0.03", help="the strength thresholds of the AMG variants")
    ap.add_argument("--fold-rows", default="", help="per theta also a hierarchy with the small levels folded into one launch "
                    "(Amg.set_fold) per value, e.g. 1024,8192, beside the unfolded one")
    ap.add_argument("--sweeps", type=int, default=1, help="nu of the V(nu, nu) cycle")
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--tol", type=float, default=1e-8, help="the tolerance of the solves")
    ap.add_argument("--max-iterations", type=int, default=200, help="the cap of the solves (reached alike by both sides)")
    ap.add_argument("--reps", type=int, default=20, help="cycles per timed apply leg")
    ap.add_argument("--stencil-diag", type=float, default=27.0, help="the diagonal of stencil<N> (26 neighbours of -1)")
    ap.add_argument("--shift", type=float, default=0.001, help="the shift of grid2d<N>: 4 + shift on the diagonal")
    args = ap.parse_args()
    if args.windows < 5:
        ap.error("--windows: at least 5")
    args.rhs = [int(v) for v in args.rhs.split(",") if v != ""]
    args.theta = [float(v) for v in args.theta.split(",") if v != ""]
    args.precond = [v for v in args.precond.split(",") if v != ""]
    if set(args.precond) - {"none", "jacobi", "sgs", "fsai", "amg"}:
        ap.error("--precond: a comma separated list of none, jacobi, sgs, fsai, amg")
    args.block_rows = [int(v) for v in args.block_rows.split(",") if v != ""]
    args.fold_rows = [int(v) for v in args.fold_rows.split(",") if v not in ("", "0")]
    os.environ.setdefault("OMP_NUM_THREADS", "16")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("pcg_tri_multi_bench.py needs a GPU: the engine has no CPU path")
    import spmv_mi355x as E
    rows = []
    for item in args.runs.split(","):
        w, dts = item.split(":")[:2]
        rows += run(E, torch, w, dts, args)
    print(f"{'workload':11s} {'dtype':5s} {'precond':>12s} {'k':>2s} {'iterations':>12s} {'SpMMs':>6s} {'s / rhs, k columns':>19s} "
          f"{'spread':>19s} {'s / rhs, single':>16s} {'spread':>19s} {'ratio':>6s} {'spread':>13s} {'bits':>5s}")
    for r in rows:
        its = f"{min(r['iterations'])}..{max(r['iterations'])}"
        print(f"{r['workload']:11s} {r['dtype']:5s} {r['precond']:>12s} {r['k']:2d} {its:>12s} {r['spmm_calls']:6d} {r['multi']:19.5f} "
              f"{r['multi_spread'][0]:9.5f} ..{r['multi_spread'][1]:8.5f} {r['single']:16.5f} {r['single_spread'][0]:9.5f} .."
              f"{r['single_spread'][1]:8.5f} {r['ratio']:6.2f} {r['ratio_spread'][0]:5.2f} ..{r['ratio_spread'][1]:5.2f} "
              f"{'same' if r['columns_equal_singles'] else 'DIFF':>5s}")
    print(f"{'workload':11s} {'dtype':5s} {'precond':>12s} {'k':>2s} {'passes':>6s} {'launches':>8s} {'single: spmvs':>13s} {'launches':>8s} "
          f"{'ms / column, k columns':>22s} {'ms / column, single':>19s} {'ratio':>6s} {'spread':>13s}")
    for r in rows:
        if "plan_passes" in r:
            print(f"{r['workload']:11s} {r['dtype']:5s} {r['precond']:>12s} {r['k']:2d} {r['plan_passes']:6d} {r['plan_launches']:8d} "
                  f"{r['single_spmvs']:13d} {r['single_launches']:8d} {r['cycle_multi']:22.4f} {r['cycle_single']:19.4f} "
                  f"{r['cycle_ratio']:6.2f} {r['cycle_ratio_spread'][0]:5.2f} ..{r['cycle_ratio_spread'][1]:5.2f}")


if __name__ == "__main__":
    main()
