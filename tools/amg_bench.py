"""What the smoothed-aggregation AMG (spmv_mi355x_amg_*; include/spmv_mi355x.h "AMG") buys the tol-based CG in iterations AND in
seconds, what it costs to set up, and what one cycle costs against one SpMV of A. Follows tools/fsai_bench.py: one sell_c_sigma handle
of A, tol 1e-8, and for every variant
    none | fsai = Fsai on tril(A) | amg t=<theta> = Amg with every theta of --theta
in one process, alternating window by window (window 0 warms every leg up and is dropped):
  spmv:      time_device(A), HIP events over --reps back-to-back launches;
  apply:     for the preconditioned variants, HIP events over --reps back-to-back apply_device calls;
  solve:     the whole call to --tol: iterations, stop, info.seconds (the setup is not in it);
  iteration: a call with tol = 0 and max_iterations = --steps, minus a call with max_iterations = 0, over --steps.
Operators:
  stencil<N>   the 27-point stencil of tools/solver_bench.py with --stencil-diag on the diagonal (27: cond 53). Its off-diagonals
               are -1 against a diagonal of 27: a_ij^2 / (d_i d_j) = 1 / 729 = 0.0014 lies below theta^2 = 0.0064 of the default
               theta, so the default hierarchy stalls at one level; 0.03 (0.0009) makes all 26 neighbours strong.
  grid2d<N>    the 5-point Laplacian on an N x N grid plus --shift on the diagonal (4 + shift, four neighbours of -1): the operator on
               which the one-level counts grow with N.
The setup of every handle is reported once (it is not repeated per window): for AMG the split of amg_info (coarsening kernels, SpGEMM,
transposition, handle creation, downloads), the rows per level and the operator complexity. The medians over the windows are
reported with their min .. max spreads. No threshold is set and no speed is promised.

    python tools/amg_bench.py                                        # stencil160 fp64
    python tools/amg_bench.py --runs grid2d2000:f64 --theta 0.08
    python tools/amg_bench.py --update                               # grid2d2000 and stencil160, fp64, theta 0.03
    python tools/amg_bench.py --runs grid2d2000:f64 --theta 0.08 --filtered --near-null
One JSON line per variant, and a table at the end.

--filtered adds, per theta, the hierarchy of spmv_mi355x_amg_create_with with filtered = 1 ("amg t=<theta> F") beside the default one.
--near-null adds the symmetrically scaled operator S A S of the workload, s = 1 + 0.5 U(-1, 1) from a fixed seed, with a handle of
its own and the same b: per theta the default hierarchy on it ("amg t=<theta> S") and the one given near_null = 1 / s ("... S+nn"),
beside the unscaled legs. Their spmv, solve and iteration legs run on the scaled handle.

--update times the other thing a caller with changing values can do: per theta, amg_create on every window (its setup_seconds: the
yardstick) against amg_update_values_prepare once and amg_update_values_device per window with the values already resident,
alternating between two value sets; the update's seconds are split into the SpGEMM numeric passes, the handles' blocking
update_values_device and the rest (amg_update_info). Medians over the windows with their spreads.

--fold-rows 0,1024,8192,65536 times the opt-in fold of the small levels (spmv_mi355x_amg_set_fold): per theta (and per --filtered
hierarchy) ONE hierarchy, and in every window every fold_rows of the list beside fold_rows = 0, the baseline of the same run: the
apply (HIP events over --reps applies), the tail alone (apply_level(f) with the fold against apply_level(f) without it, f the leg's
first folded level) and the whole solve to --tol with its iteration count. set_fold is called outside the timed stretches."""
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


def grid2d(k, shift):
    """(row_ptr, col_idx, values, n) of the 5-point operator on a k x k grid: 4 + shift on the diagonal, -1 to the four neighbours"""
    import scipy.sparse as sp
    I, E = sp.identity(k, format="csr"), sp.diags([-np.ones(k - 1), -np.ones(k - 1)], [-1, 1], format="csr")
    A = (sp.kron(I, E) + sp.kron(E, I) + (4.0 + shift) * sp.identity(k * k, format="csr")).tocsr()
    A.sort_indices()
    return A.indptr.astype(np.int32), A.indices.astype(np.int32), A.data.astype(np.float64), k * k


def run(E, torch, workload, dts, args):
    if workload.startswith("stencil"):
        from solver_bench import stencil27
        rp, ci, va, n = stencil27(int(workload[len("stencil"):]), args.stencil_diag)
    elif workload.startswith("grid2d"):
        rp, ci, va, n = grid2d(int(workload[len("grid2d"):]), args.shift)
    else:
        raise SystemExit(f"amg_bench.py runs on stencil<N> and grid2d<N>, not on {workload}")
    rp = np.asarray(rp, np.int32)
    np_dtype = np.float32 if dts == "f32" else np.float64
    tdt = torch.float32 if dts == "f32" else torch.float64
    MA = E.Matrix(rp, ci, va, n, n, "sell_c_sigma", np_dtype)
    xa = (torch.rand(n, device="cuda", dtype=torch.float64) * 2 - 1).to(tdt)
    ya = torch.empty(n + 64, dtype=tdt, device="cuda")
    stream = torch.cuda.current_stream()
    b = np.random.default_rng(7).uniform(-1, 1, n).astype(np_dtype)
    variants = [("none", None, {}, MA)]                       # (name, preconditioner, what its setup reports, the handle of A it solves)
    t0 = time.perf_counter()
    F = E.Fsai(rp, ci, va, n, None, "sell_c_sigma", np_dtype)
    variants.append(("fsai", F, dict(setup_seconds=round(F.info()["setup_seconds"], 4), wall_setup_seconds=round(time.perf_counter() - t0, 4)),
                     MA))
    print(f"# built fsai: {variants[-1][2]}", flush=True)
    MS = s = vs = None
    if args.near_null:
        s = 1 + 0.5 * np.random.default_rng(25).uniform(-1, 1, n)
        vs = np.asarray(va, np.float64) * (s[np.repeat(np.arange(n), np.diff(rp))] * s[np.asarray(ci)])
        MS = E.Matrix(rp, ci, vs, n, n, "sell_c_sigma", np_dtype)
    builds = []                                               # (suffix, values, near_null, filtered, the handle of A), per theta
    for theta in args.theta:
        builds.append((theta, "", va, None, None, MA))
        if args.filtered:
            builds.append((theta, " F", va, None, True, MA))
        if args.near_null:
            builds.append((theta, " S", vs, None, None, MS))
            builds.append((theta, " S+nn", vs, 1.0 / s, False, MS))
    for theta, suffix, values, near_null, filtered, H in builds:
        t0 = time.perf_counter()
        if filtered is None:
            M = E.Amg(rp, ci, values, n, "sell_c_sigma", np_dtype, theta=theta, sweeps=args.sweeps)
        else:
            M = E.Amg.build(rp, ci, values, n, near_null, filtered, "sell_c_sigma", np_dtype, theta=theta, sweeps=args.sweeps)
        wall = time.perf_counter() - t0
        info, pinfo = M.info(), M.prolongator_info()
        extra = dict(theta=theta, sweeps=args.sweeps, levels=info["levels"], rows=info["rows"], nnz=info["nnz"], mis_rounds=info["mis_rounds"],
                     entries_per_row=[round(z / max(r, 1), 1) for z, r in zip(info["nnz"], info["rows"])], filtered=pinfo["filtered"],
                     near_null=pinfo["has_near_null"], nnz_filtered=pinfo["nnz_filtered"], unfiltered_rows=pinfo["unfiltered_rows"],
                     coarse=info["coarse"], stalled=info["stalled"], operator_complexity=round(info["operator_complexity"], 4),
                     grid_complexity=round(info["grid_complexity"], 4), spmvs_per_apply=info["spmvs_per_apply"],
                     launches_per_apply=info["launches_per_apply"], wall_setup_seconds=round(wall, 4),
                     **{k: round(info[k], 4) for k in ("setup_seconds", "coarsen_seconds", "spgemm_seconds", "transpose_seconds",
                                                       "create_seconds", "download_seconds")},
                     mem_over_a=round(M.mem_footprint / MA.mem_footprint, 3))
        variants.append((f"amg t={theta:g}{suffix}", M, extra, H))
        print(f"# built {variants[-1][0]}: {extra}", flush=True)
    solve = lambda H, M, tol, steps: H.pcg_tri(b, precond=M, tol=tol, max_iterations=steps, history=False)

    def time_apply(M):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(args.reps):
            M.apply_device(xa.data_ptr(), ya.data_ptr(), stream.cuda_stream)
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1) / args.reps

    legs = {name: {k: [] for k in ("spmv", "seconds", "iter_ms", "ratio", "apply", "apply_ratio")} for name, _, _, _ in variants}
    last = {}
    for w in range(args.windows + 1):                         # window 0 warms every leg up and is dropped
        for name, M, _, H in variants:
            t_a = H.time_device(xa.data_ptr(), ya.data_ptr(), args.reps, stream.cuda_stream)
            torch.cuda.synchronize()
            t_f = time_apply(M) if M is not None else float("nan")
            r = solve(H, M, args.tol, args.max_iterations)
            fixed = solve(H, M, 0.0, 0)["seconds"]
            st = solve(H, M, 0.0, args.steps)
            # a preconditioned solve may reach r = 0 or lose r.z > 0 in the rounding floor before --steps: then the leg is not timed
            t_c = (st["seconds"] - fixed) * 1e3 / args.steps if (st["iterations"], st["stop"]) == (args.steps, 2) else float("nan")
            last[name] = r
            if w:
                for key, t in zip(legs[name], (t_a, r["seconds"], t_c, t_c / t_a, t_f, t_f / t_a)):
                    legs[name][key].append(t)
        print(f"# window {w} done", flush=True)
    rows = []
    for name, M, extra, _ in variants:
        r = last[name]
        rec = dict(workload=workload, dtype=dts, format=MA.format_name, n=int(n), nnz_a=int(MA.nnz), precond=name, tol=args.tol,
                   iterations=int(r["iterations"]), stop=int(r["stop"]), rnorm_over_b=float(r["rnorm"] / r["rnorm0"]),
                   windows=args.windows, steps=args.steps, reps=args.reps, **extra)
        for key, ts in legs[name].items():
            if np.isnan(ts).all():
                continue
            rec[key] = round(float(np.nanmedian(ts)), 5)
            rec[key + "_spread"] = [round(float(np.nanmin(ts)), 5), round(float(np.nanmax(ts)), 5)]
        print(json.dumps(rec), flush=True)
        rows.append(rec)
    for _, M, _, _ in variants:
        if M is not None:
            M.close()
    MA.close()
    if MS is not None:
        MS.close()
    return rows


def run_update(E, torch, workload, dts, args):
    """--update: amg_create against amg_update_values_prepare (once) and amg_update_values_device with the values resident, per theta.
    Every window creates a hierarchy from scratch (the yardstick: create is what a caller without update pays per value set) and
    updates the prepared one, alternating between 0.7 V1 and V1 so that every update meets other numbers; window 0 is dropped."""
    if workload.startswith("stencil"):
        from solver_bench import stencil27
        rp, ci, va, n = stencil27(int(workload[len("stencil"):]), args.stencil_diag)
    elif workload.startswith("grid2d"):
        rp, ci, va, n = grid2d(int(workload[len("grid2d"):]), args.shift)
    else:
        raise SystemExit(f"amg_bench.py runs on stencil<N> and grid2d<N>, not on {workload}")
    rp, va = np.asarray(rp, np.int32), np.asarray(va, np.float64)
    np_dtype = np.float32 if dts == "f32" else np.float64
    resident = [torch.from_numpy(np.array(0.7 * va)).cuda(), torch.from_numpy(np.array(va)).cuda()]
    rows = []
    for theta in args.theta:
        make = lambda: E.Amg(rp, ci, va, n, "sell_c_sigma", np_dtype, theta=theta, sweeps=args.sweeps)
        M = make()
        t0 = time.perf_counter()
        M.update_values_prepare()
        prepare_wall = time.perf_counter() - t0
        info = M.info()
        legs = {k: [] for k in ("create", "create_wall", "update", "update_wall", "spgemm", "handles", "rest")}
        for w in range(args.windows + 1):
            t0 = time.perf_counter()
            N = make()
            create_wall = time.perf_counter() - t0
            create = N.info()["setup_seconds"]
            N.close()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            M.update_values_device(resident[w % 2].data_ptr())
            update_wall = time.perf_counter() - t0
            u = M.update_info()
            if w:
                for key, t in zip(legs, (create, create_wall, u["update_seconds"], update_wall, u["spgemm_seconds"], u["handle_seconds"],
                                         u["update_seconds"] - u["spgemm_seconds"] - u["handle_seconds"])):
                    legs[key].append(t)
            print(f"# update window {w} done", flush=True)
        u = M.update_info()
        rec = dict(workload=workload, dtype=dts, leg="update", theta=theta, n=int(n), nnz_a=int(rp[-1]), levels=info["levels"], rows=info["rows"],
                   coarse=M.info()["coarse"], windows=args.windows, prepare_seconds=round(u["prepare_seconds"], 5),
                   prepare_wall_seconds=round(prepare_wall, 5), prepare_bytes_over_footprint=round(u["prepare_bytes"] / M.mem_footprint, 3))
        for key, ts in legs.items():
            rec[key] = round(float(np.median(ts)), 6)
            rec[key + "_spread"] = [round(float(np.min(ts)), 6), round(float(np.max(ts)), 6)]
        rec["create_over_update"] = round(rec["create"] / rec["update"], 2)
        print(json.dumps(rec), flush=True)
        rows.append(rec)
        M.close()
    return rows


def run_fold(E, torch, workload, dts, args):
    """--fold-rows: every fold_rows beside fold_rows = 0 on the same hierarchy, window by window (window 0 is dropped)"""
    if workload.startswith("stencil"):
        from solver_bench import stencil27
        rp, ci, va, n = stencil27(int(workload[len("stencil"):]), args.stencil_diag)
    elif workload.startswith("grid2d"):
        rp, ci, va, n = grid2d(int(workload[len("grid2d"):]), args.shift)
    else:
        raise SystemExit(f"amg_bench.py runs on stencil<N> and grid2d<N>, not on {workload}")
    rp = np.asarray(rp, np.int32)
    np_dtype = np.float32 if dts == "f32" else np.float64
    tdt = torch.float32 if dts == "f32" else torch.float64
    stream = torch.cuda.current_stream()
    b = np.random.default_rng(7).uniform(-1, 1, n).astype(np_dtype)
    xa = (torch.rand(n, device="cuda", dtype=torch.float64) * 2 - 1).to(tdt)
    ya = torch.empty(n + 64, dtype=tdt, device="cuda")
    folds = [0] + [f for f in args.fold_rows if f != 0]

    def timed(call):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(args.reps):
            call()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1) / args.reps

    rows = []
    for theta in args.theta:
        for filtered in ((False, True) if args.filtered else (False,)):
            if filtered:
                M = E.Amg.build(rp, ci, va, n, None, True, "sell_c_sigma", np_dtype, theta=theta, sweeps=args.sweeps)
            else:
                M = E.Amg(rp, ci, va, n, "sell_c_sigma", np_dtype, theta=theta, sweeps=args.sweeps)
            info = M.info()
            print(f"# built amg t={theta:g}{' F' if filtered else ''}: levels {info['levels']}, rows {info['rows']}, nnz {info['nnz']}, coarse "
                  f"{info['coarse']}, launches {info['launches_per_apply']}", flush=True)
            legs = {f: {k: [] for k in ("apply", "tail", "tail_unfolded", "seconds")} for f in folds}
            last, fold_info = {}, {}
            for w in range(args.windows + 1):
                for f in folds:
                    M.set_fold(f)
                    fi = fold_info[f] = M.fold_info()
                    t_apply = timed(lambda: M.apply_device(xa.data_ptr(), ya.data_ptr(), stream.cuda_stream))
                    t_tail = t_plain = float("nan")
                    level = fi["first_level"]
                    if level < info["levels"]:
                        t_tail = timed(lambda: M.apply_level_device(level, xa.data_ptr(), ya.data_ptr(), stream.cuda_stream))
                        M.set_fold(0)
                        t_plain = timed(lambda: M.apply_level_device(level, xa.data_ptr(), ya.data_ptr(), stream.cuda_stream))
                        M.set_fold(f)
                    r = M.A.pcg_tri(b, precond=M, tol=args.tol, max_iterations=args.max_iterations, history=False)
                    last[f] = r
                    if w:
                        for key, t in zip(legs[f], (t_apply, t_tail, t_plain, r["seconds"])):
                            legs[f][key].append(t)
                print(f"# fold window {w} done", flush=True)
            for f in folds:
                fi, r = fold_info[f], last[f]
                rec = dict(workload=workload, dtype=dts, leg="fold", theta=theta, filtered=int(filtered), sweeps=args.sweeps, n=int(n),
                           levels=info["levels"], rows=info["rows"], coarse=info["coarse"], fold_rows=f, first_level=fi["first_level"],
                           folded_levels=fi["folded_levels"], launches=fi["launches_per_apply"], spmvs=fi["spmvs_per_apply"],
                           tail_products=fi["tail_products"], tail_entries=fi["tail_entries"], lanes_per_row=fi["lanes_per_row"],
                           fold_bytes=fi["bytes"], iterations=int(r["iterations"]), stop=int(r["stop"]), windows=args.windows, reps=args.reps)
                for key, ts in legs[f].items():
                    if np.isnan(ts).all():
                        continue
                    rec[key] = round(float(np.nanmedian(ts)), 5)
                    rec[key + "_spread"] = [round(float(np.nanmin(ts)), 5), round(float(np.nanmax(ts)), 5)]
                print(json.dumps(rec), flush=True)
                rows.append(rec)
            M.close()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", default=None, help="stencil<N>:f64|f32 or grid2d<N>:f64|f32, comma separated (default stencil160:f64; "
                    "with --update grid2d2000:f64,stencil160:f64)")
    ap.add_argument("--theta", default=None, help="the strength thresholds of the AMG variants (default 0.08,0.03; with --update 0.03)")
    ap.add_argument("--update", action="store_true", help="time amg_create against update_values_prepare and update_values_device "
                    "instead of the solves")
    ap.add_argument("--filtered", action="store_true", help="per theta also the hierarchy with filtered prolongator smoothing")
    ap.add_argument("--near-null", action="store_true", help="also S A S of the workload (s = 1 +- 0.5, a fixed seed): per theta the "
                    "default hierarchy on it and the one given near_null = 1 / s")
    ap.add_argument("--fold-rows", default=None, help="time the opt-in fold instead of the solves: the fold_rows values, comma separated "
                    "(0, the baseline, always runs beside them)")
    ap.add_argument("--sweeps", type=int, default=1, help="nu of the V(nu, nu) cycle")
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--tol", type=float, default=1e-8, help="the tolerance of the solve leg")
    ap.add_argument("--max-iterations", type=int, default=5000, help="the cap of the solve leg")
    ap.add_argument("--steps", type=int, default=50, help="iterations of the tol = 0 leg")
    ap.add_argument("--reps", type=int, default=50, help="launches per timed SpMV / apply leg")
    ap.add_argument("--stencil-diag", type=float, default=27.0, help="the diagonal of stencil<N> (26 neighbours of -1)")
    ap.add_argument("--shift", type=float, default=0.001, help="the shift of grid2d<N>: 4 + shift on the diagonal")
    args = ap.parse_args()
    if args.windows < 5:
        ap.error("--windows: at least 5")
    args.runs = args.runs or ("grid2d2000:f64,stencil160:f64" if args.update else "stencil160:f64")
    args.theta = [float(v) for v in (args.theta or ("0.03" if args.update else "0.08,0.03")).split(",") if v != ""]
    os.environ.setdefault("OMP_NUM_THREADS", "16")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("amg_bench.py needs a GPU: the engine has no CPU path")
    import spmv_mi355x as E
    rows = []
    if args.fold_rows is not None:
        args.fold_rows = [int(v) for v in args.fold_rows.split(",") if v != ""]
    for item in args.runs.split(","):
        w, dts = item.split(":")[:2]
        rows += (run_fold if args.fold_rows is not None else run_update if args.update else run)(E, torch, w, dts, args)
    if args.fold_rows is not None:
        nan = float("nan")
        print(f"{'workload':11s} {'theta':>6s} {'F':>1s} {'fold_rows':>9s} {'first':>5s} {'launches':>8s} {'apply ms':>9s} {'spread':>19s} "
              f"{'tail ms':>8s} {'unfolded':>8s} {'tail entries':>12s} {'iters':>6s} {'solve s':>8s} {'spread':>19s}")
        for r in rows:
            print(f"{r['workload']:11s} {r['theta']:6g} {r['filtered']:1d} {r['fold_rows']:9d} {r['first_level']:5d} {r['launches']:8d} "
                  f"{r['apply']:9.4f} {r['apply_spread'][0]:9.4f} ..{r['apply_spread'][1]:8.4f} {r.get('tail', nan):8.4f} "
                  f"{r.get('tail_unfolded', nan):8.4f} {r['tail_entries']:12d} {r['iterations']:6d} {r['seconds']:8.4f} "
                  f"{r['seconds_spread'][0]:9.4f} ..{r['seconds_spread'][1]:8.4f}")
        return
    if args.update:
        print(f"{'workload':11s} {'dtype':5s} {'theta':>6s} {'levels':>6s} {'create s':>9s} {'spread':>19s} {'prepare s':>9s} {'update s':>9s} "
              f"{'spread':>19s} {'spgemm':>8s} {'handles':>8s} {'rest':>8s} {'create / update':>15s} {'kept / footprint':>16s}")
        for r in rows:
            print(f"{r['workload']:11s} {r['dtype']:5s} {r['theta']:6g} {r['levels']:6d} {r['create']:9.4f} {r['create_spread'][0]:9.4f} .."
                  f"{r['create_spread'][1]:8.4f} {r['prepare_seconds']:9.4f} {r['update']:9.4f} {r['update_spread'][0]:9.4f} .."
                  f"{r['update_spread'][1]:8.4f} {r['spgemm']:8.4f} {r['handles']:8.4f} {r['rest']:8.4f} {r['create_over_update']:15.2f} "
                  f"{r['prepare_bytes_over_footprint']:16.3f}")
        return
    nan = float("nan")
    print(f"{'workload':11s} {'dtype':5s} {'precond':>16s} {'iters':>6s} {'stop':>4s} {'seconds':>9s} {'spread':>19s} {'ms/iter':>8s} "
          f"{'spmv ms':>8s} {'iter / spmv':>11s} {'apply ms':>9s} {'apply / spmv':>12s}")
    for r in rows:
        print(f"{r['workload']:11s} {r['dtype']:5s} {r['precond']:>16s} {r['iterations']:6d} {r['stop']:4d} {r['seconds']:9.4f} "
              f"{r['seconds_spread'][0]:9.4f} ..{r['seconds_spread'][1]:8.4f} {r.get('iter_ms', nan):8.4f} {r['spmv']:8.4f} "
              f"{r.get('ratio', nan):11.2f} {r.get('apply', nan):9.4f} {r.get('apply_ratio', nan):12.2f}")
    print(f"{'workload':11s} {'precond':>16s} {'levels':>6s} {'coarse':>7s} {'op cx':>6s} {'spmvs':>5s} {'launches':>8s} {'setup s':>8s} {'coarsen':>8s} "
          f"{'spgemm':>8s} {'transp':>8s} {'handles':>8s} {'download':>8s} {'wall s':>8s}  rows")
    for r in rows:
        if "levels" in r:
            print(f"{r['workload']:11s} {r['precond']:>16s} {r['levels']:6d} {r['coarse'][:7]:>7s} {r['operator_complexity']:6.3f} "
                  f"{r['spmvs_per_apply']:5d} {r['launches_per_apply']:8d} {r['setup_seconds']:8.3f} {r['coarsen_seconds']:8.3f} "
                  f"{r['spgemm_seconds']:8.3f} {r['transpose_seconds']:8.3f} {r['create_seconds']:8.3f} {r['download_seconds']:8.3f} "
                  f"{r['wall_setup_seconds']:8.3f}  {r['rows']}  entries per row {r['entries_per_row']}")


if __name__ == "__main__":
    main()
