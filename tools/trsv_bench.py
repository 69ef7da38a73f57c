"""A sparse triangular solve (spmv_mi355x_trsv_*; include/spmv_mi355x.h "sparse triangular solve") against its floor, and the
chain_rows sweep behind the default.

For the LOWER triangle (diagonal included) of each workload twin of bench.py and of the 27-point stencil of tools/solver_bench.py the
tool prints n, the kept entries, the levels and the widest level, and per chain_rows value the launches of the plan. In one process,
alternating window by window, it times
  floor:  time_device of an E.Matrix (sell_c_sigma, its own best layout) built from the same triangle: one SpMV reads the same
          entries with no dependency between rows, so no triangular solve of this matrix can be faster;
  trsv:   time_device of one TriangularSolve handle per chain_rows value, `reps` back-to-back solves under HIP events, reps
          calibrated so that a leg lasts about --leg-ms.
The medians over the windows are reported with their spreads, and the ratio solve / floor.
With --block-rows the blocked form (spmv_mi355x_trsv_create_blocked) of the same triangle is timed beside them, one handle per block
size, in the same process and the same alternating windows: per size the blocks, the most levels of a block, the share of the
triangle's off-diagonal entries that the blocks drop, ms, the ratio to the floor and the ratio to the global plan of the same run
(the first --chain-rows value). A blocked handle solves a different, easier system: the ratio says what the launch plan costs, what
the dropped entries cost a solver is tools/gmres_bench.py's question.
With --rhs the k-column solve (spmv_mi355x_trsv_solve_multi_device_async) of the first --chain-rows handle and of every --block-rows
handle is timed for each k beside the single solve of the same handle, again in the same windows: per k the passes and launches of
the plan, ms per solve, and ms per column over the single solve's ms (1 / k when a pass costs what a single solve costs).

    python tools/trsv_bench.py                                       # cant, nlpkkt240, stencil160, fp64
    python tools/trsv_bench.py --runs cant:f64,cant:f32,stencil40:f64 --windows 7 --chain-rows 64,256,1024,4096
    python tools/trsv_bench.py --runs nlpkkt240:f64 --scale 0.25
    python tools/trsv_bench.py --runs cant:f64,cant:f32,stencil160:f64,nlpkkt240:f64 --chain-rows 256 --block-rows 1024,2048,4096,8192,16384
    python tools/trsv_bench.py --runs stencil160:f64 --chain-rows 256 --block-rows 1024,2048,4096 --rhs 1,2,4,8
With --sweeps the Jacobi-sweep solve (spmv_mi355x_trsv_set_sweeps) of the first --chain-rows handle is timed for each sweep count in
the same windows, through the same time_device call: per count the effective sweeps and launches, ms per solve, ms per sweep, and the
ratios to the exact solve of that handle and to the floor SpMV. With --rhs as well, each k-column sweep solve is timed too and
reported per column. The sweep solve approximates the system the exact solve solves: what that costs a solver is
tools/pcg_tri_bench.py's question.
    python tools/trsv_bench.py --runs stencil160:f64 --chain-rows 256 --sweeps 1,2,3,4,8
With --update nothing above is timed. Instead, per run and per variant (the global handle of the first --chain-rows value and the
blocked handle of every --block-rows value), the tool times in one process and in alternating windows
  create:  TriangularSolve(...) on new values V2: host analysis, layout and nine uploads, which is what a handle cost before it
           could take new values;
  update:  update_values_device on V2 resident on the device, with a synchronise behind it (spmv_mi355x_trsv_update_values_device),
           and the same call once more at once ("again": the same work without the host-bound create in front of it);
  host:    update_values on V2 in host memory (the upload of row_ptr[n] doubles included);
and reports the medians with min .. max, update_values_prepare's seconds (once), the bytes an update moves by the layout's own count,
slots * (4 + 8 + sizeof T) + n * (4 + 8 + sizeof T) under DIAG_STORED, and whether the updated handle has the fresh handle's bytes.
grid2d<N> (the 5-point operator of tools/amg_bench.py) is a workload of every mode. No ratio is asserted.
    python tools/trsv_bench.py --update --runs stencil160:f64,grid2d2000:f64 --chain-rows 256 --block-rows 4096
One JSON line per run and a table at the end.
"""
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


def lower_triangle(rp, ci, va, n):
    """the entries with column <= row, stored order kept; row by row in blocks so that no index array of the full size is held twice"""
    rp = np.asarray(rp, np.int64)
    keep = np.empty(len(ci), bool)
    counts = np.zeros(n, np.int64)
    step = 1 << 20
    for r0 in range(0, n, step):
        r1 = min(n, r0 + step)
        rows = np.repeat(np.arange(r0, r1, dtype=np.int32), np.diff(rp[r0:r1 + 1]))
        k = ci[rp[r0]:rp[r1]] <= rows
        keep[rp[r0]:rp[r1]] = k
        counts[r0:r1] = np.bincount(rows[k] - r0, minlength=r1 - r0)
    rp2 = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    return rp2, np.ascontiguousarray(ci[keep]), np.ascontiguousarray(va[keep])


def safe_diagonal(rp, ci, va, n):
    """the twins were made for SpMV: where a row's diagonal is missing from the pattern the tool cannot add one (the pattern is the
    workload), so such a workload is solved under DIAG_UNIT; a stored zero or tiny diagonal is replaced by 1 (timing does not care)"""
    rows = np.repeat(np.arange(n, dtype=np.int32), np.diff(rp))
    on = ci == rows
    has = np.zeros(n, bool)
    has[rows[on]] = True
    va = va.copy()
    d = va[on]
    d[~np.isfinite(d) | (np.abs(d) < 1e-30)] = 1.0
    va[on] = d
    return va, bool(has.all()) and int(on.sum()) == n


def run(E, torch, name, rp, ci, va, n, dts, data, args):
    np_dtype = np.float32 if dts == "f32" else np.float64
    tdt = torch.float32 if dts == "f32" else torch.float64
    t0 = time.perf_counter()
    rp, ci, va = lower_triangle(rp, ci, va, n)
    va, stored = safe_diagonal(rp, ci, va, n)
    t_tri = time.perf_counter() - t0
    M = E.Matrix(rp, ci, va, n, n, "sell_c_sigma", np_dtype)
    x = (torch.rand(n, device="cuda", dtype=torch.float64) * 2 - 1).to(tdt)
    y = torch.empty(n + 64, dtype=tdt, device="cuda")
    b = (torch.rand(n, device="cuda", dtype=torch.float64) * 2 - 1).to(tdt)
    out = torch.empty(n, dtype=tdt, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    handles, create_s = {}, {}
    for c in args.chain_rows:
        t0 = time.perf_counter()
        handles[c] = E.TriangularSolve(rp, ci, va, n, "lower", "stored" if stored else "unit", np_dtype, chain_rows=c)
        create_s[c] = time.perf_counter() - t0
    for B in args.block_rows:                             # keyed ("b", B): the blocked handles ride in the same windows
        t0 = time.perf_counter()
        handles[("b", B)] = E.TriangularSolve(rp, ci, va, n, "lower", "stored" if stored else "unit", np_dtype, block_rows=B)
        create_s[("b", B)] = time.perf_counter() - t0
    infos = {c: T.info for c, T in handles.items()}
    reps = {}
    for c, T in handles.items():                          # the first solve warms up, the second calibrates
        T.time_device(b.data_ptr(), out.data_ptr(), 1, stream)
        one = T.time_device(b.data_ptr(), out.data_ptr(), 2, stream)
        reps[c] = int(min(200, max(3, np.ceil(args.leg_ms / max(one, 1e-3)))))
    legs = {"spmv": []}
    legs.update({c: [] for c in handles})
    # --rhs: the k-column solve of every handle beside its single solve, in the same windows. One n x max(k) block serves every k
    # with ld = k. A k-column leg runs a k-th of the single leg's solves (at least 3), so a leg that costs k times as much lasts as long.
    multi = {c: T for c, T in handles.items() if args.rhs and (isinstance(c, tuple) or c == args.chain_rows[0])}
    if multi:
        bk = (torch.rand(n * max(args.rhs), device="cuda", dtype=torch.float64) * 2 - 1).to(tdt)
        xk = torch.empty(n * max(args.rhs), dtype=tdt, device="cuda")
        for c, T in multi.items():
            for k in args.rhs:
                T.time_multi_device(k, bk.data_ptr(), k, xk.data_ptr(), k, 1, stream)          # warm-up: code objects, the LDS grant
                legs[(c, k)] = []
    # --sweeps: the first handle under set_sweeps(s), through the same timing entries; the setting is back at 0 (exact) after each leg
    swept = handles[args.chain_rows[0]]
    sweep_reps = {}
    for s in args.sweeps:
        swept.set_sweeps(s)
        swept.time_device(b.data_ptr(), out.data_ptr(), 1, stream)                                # warm-up: the map, the scratch
        one = swept.time_device(b.data_ptr(), out.data_ptr(), 2, stream)
        sweep_reps[s] = int(min(200, max(3, np.ceil(args.leg_ms / max(one, 1e-3)))))
        legs[("s", s)] = []
        for k in args.rhs:
            swept.time_multi_device(k, bk.data_ptr(), k, xk.data_ptr(), k, 1, stream)
            legs[("s", s, k)] = []
        swept.set_sweeps(0)
    for w in range(args.windows + 1):                     # window 0 warms every leg up and is dropped
        t = {"spmv": M.time_device(x.data_ptr(), y.data_ptr(), args.reps, stream)}
        for c, T in handles.items():
            t[c] = T.time_device(b.data_ptr(), out.data_ptr(), reps[c], stream)
            for k in args.rhs if c in multi else ():
                t[(c, k)] = T.time_multi_device(k, bk.data_ptr(), k, xk.data_ptr(), k, max(3, reps[c] // k), stream)
        for s in args.sweeps:
            swept.set_sweeps(s)
            t[("s", s)] = swept.time_device(b.data_ptr(), out.data_ptr(), sweep_reps[s], stream)
            for k in args.rhs:
                t[("s", s, k)] = swept.time_multi_device(k, bk.data_ptr(), k, xk.data_ptr(), k, max(3, sweep_reps[s] // k), stream)
            swept.set_sweeps(0)
        torch.cuda.synchronize()
        if w:
            for k, v in t.items():
                legs[k].append(v)
    first = infos[args.chain_rows[0]]
    rec = dict(workload=name, dtype=dts, data=data, n=int(n), nnz_kept=int(first["nnz_kept"]), diag="stored" if stored else "unit",
               levels=int(first["levels"]), max_level_rows=int(first["max_level_rows"]), floor_format=M.format_name,
               spmv_ms=round(float(np.median(legs["spmv"])), 5), spmv_spread=[round(min(legs["spmv"]), 5), round(max(legs["spmv"]), 5)],
               windows=args.windows, triangle_seconds=round(t_tri, 2), sweep=[], blocked=[])
    global_ms = float(np.median(legs[args.chain_rows[0]]))
    off_diagonal = int(first["nnz_kept"]) - (n if stored else 0)
    rec["rhs"] = []
    for c, T in multi.items():
        single = legs[c]
        for k in args.rhs:
            ts, plan = legs[(c, k)], T.solve_multi_plan(k)
            rec["rhs"].append(dict(block_rows=int(c[1]) if isinstance(c, tuple) else 0, k=k, passes=plan["matrix_passes"],
                                   launches=plan["launches"], max_chunk=plan["max_chunk"], reps=max(3, reps[c] // k),
                                   ms=round(float(np.median(ts)), 5), spread=[round(min(ts), 5), round(max(ts), 5)],
                                   single_ms=round(float(np.median(single)), 5), single_spread=[round(min(single), 5), round(max(single), 5)],
                                   per_column_over_single=round(float(np.median(ts)) / k / float(np.median(single)), 4)))
    rec["sweeps"] = []
    for s in args.sweeps:
        swept.set_sweeps(s)
        for k in [0] + args.rhs:                          # 0: the single solve
            ts, info = legs[("s", s, k) if k else ("s", s)], swept.sweeps_info(max(k, 1))
            ms = float(np.median(ts))
            rec["sweeps"].append(dict(sweeps=s, k=k, effective=info["effective"], launches=info["launches"],
                                      reps=max(3, sweep_reps[s] // k) if k else sweep_reps[s], ms=round(ms, 5),
                                      spread=[round(min(ts), 5), round(max(ts), 5)], ms_per_sweep=round(ms / max(info["effective"], 1), 5),
                                      per_column_ms=round(ms / max(k, 1), 5), per_column_over_exact=round(ms / max(k, 1) / global_ms, 4),
                                      per_column_over_floor=round(ms / max(k, 1) / rec["spmv_ms"], 2), scratch_bytes=int(info["bytes"])))
        swept.set_sweeps(0)
    for c, T in handles.items():
        ts = legs[c]
        if isinstance(c, tuple):
            blk = T.block_info()
            rec["blocked"].append(dict(block_rows=int(blk["block_rows"]), blocks=int(blk["blocks"]),
                                       max_block_levels=int(blk["max_block_levels"]), max_level_rows=int(infos[c]["max_level_rows"]),
                                       dropped_share=round(blk["nnz_dropped"] / max(off_diagonal, 1), 4), reps=reps[c],
                                       ms=round(float(np.median(ts)), 5), spread=[round(min(ts), 5), round(max(ts), 5)],
                                       over_floor=round(float(np.median(ts)) / rec["spmv_ms"], 2),
                                       over_global=round(float(np.median(ts)) / global_ms, 4), create_seconds=round(create_s[c], 2),
                                       mem_footprint=int(T.mem_footprint)))
            T.close()
            continue
        rec["sweep"].append(dict(chain_rows=int(infos[c]["chain_rows"]), launches=int(infos[c]["launches"]), reps=reps[c],
                                 ms=round(float(np.median(ts)), 5), spread=[round(min(ts), 5), round(max(ts), 5)],
                                 over_floor=round(float(np.median(ts)) / rec["spmv_ms"], 2), create_seconds=round(create_s[c], 2),
                                 mem_footprint=int(T.mem_footprint)))
        T.close()
    M.close()
    print(json.dumps(rec), flush=True)
    return rec


def spread(ts):
    return dict(median=round(float(np.median(ts)), 6), min=round(min(ts), 6), max=round(max(ts), 6))


def run_update(E, torch, name, rp, ci, va, n, dts, args):
    """--update: a fresh handle on V2 against update_values of a handle that exists; one JSON line per variant"""
    np_dtype = np.float32 if dts == "f32" else np.float64
    rp, ci, va = lower_triangle(rp, ci, va, n)
    va, stored = safe_diagonal(rp, ci, va, n)
    diag = "stored" if stored else "unit"
    v2 = va * np.random.default_rng(2).uniform(1.0, 1.5, len(va))
    dev = torch.from_numpy(v2).cuda()
    torch.cuda.synchronize()
    out = []
    for key in [("chain_rows", args.chain_rows[0])] + [("block_rows", B) for B in args.block_rows]:
        make = lambda v: E.TriangularSolve(rp, ci, v, n, "lower", diag, np_dtype, **{key[0]: key[1]})
        T = make(va)
        t0 = time.perf_counter()
        T.update_values_prepare(rp, ci)
        prepare = time.perf_counter() - t0
        create, update, again, host = [], [], [], []
        for w in range(args.windows + 1):                 # window 0 warms every leg up and is dropped
            t0 = time.perf_counter()
            fresh = make(v2)
            t1 = time.perf_counter()
            T.update_values_device(dev.data_ptr())
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            T.update_values_device(dev.data_ptr())        # again at once: the same work without the host-bound pause before it
            torch.cuda.synchronize()
            t2b = time.perf_counter()
            T.update_values(v2)
            t3 = time.perf_counter()
            if w:
                create.append(t1 - t0)
                update.append(t2 - t1)
                again.append(t2b - t2)
                host.append(t3 - t2b)
            if w < args.windows:
                fresh.close()
        a, b = T.stored_values(), fresh.stored_values()
        same = all((x is None and y is None) or np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(a, b))
        slots, size = len(a[0]), np.dtype(np_dtype).itemsize
        rec = dict(workload=name, dtype=dts, n=int(n), nnz=int(len(ci)), variant=f"{key[0]}={key[1]}", diag=diag, slots=slots,
                   levels=T.info["levels"], launches=T.info["launches"], prepare_seconds=round(prepare, 4), create_seconds=spread(create),
                   update_device_seconds=spread(update), update_device_again_seconds=spread(again), update_host_seconds=spread(host),
                   update_bytes=int((slots + (n if stored else 0)) * (4 + 8 + size)), map_mib=round(T.update_values_bytes / 2 ** 20, 1),
                   handle_mib=round(T.mem_footprint / 2 ** 20, 1), windows=args.windows, same_bytes=bool(same))
        print(json.dumps(rec), flush=True)
        out.append(rec)
        T.close()
        fresh.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", default="cant:f64,nlpkkt240:f64,stencil160:f64", help="workload|stencil<N>:f64|f32,...")
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--chain-rows", default="64,256,1024,4096", help="the thresholds to sweep, first = the one the header line reports")
    ap.add_argument("--block-rows", default="", help="block sizes of the blocked form to time beside the plans, e.g. 1024,2048,4096,8192,16384")
    ap.add_argument("--rhs", default="", help="column counts of the k-column solve to time beside the single solve, e.g. 1,2,4,8")
    ap.add_argument("--sweeps", default="", help="Jacobi-sweep counts to time beside the exact solve of the first --chain-rows handle, e.g. 1,2,3,4,8")
    ap.add_argument("--reps", type=int, default=20, help="SpMV launches per timed floor leg")
    ap.add_argument("--leg-ms", type=float, default=40.0, help="solves per timed leg: as many as last about this long (3 .. 200)")
    ap.add_argument("--scale", type=float, default=1.0, help="shrink the workload twins")
    ap.add_argument("--update", action="store_true", help="time a fresh handle on new values against update_values of an existing one")
    args = ap.parse_args()
    if args.windows < 5:
        ap.error("--windows: at least 5")
    args.chain_rows = [int(c) for c in args.chain_rows.split(",")]
    args.block_rows = [int(c) for c in args.block_rows.split(",") if c]
    args.rhs = [int(c) for c in args.rhs.split(",") if c]
    args.sweeps = [int(c) for c in args.sweeps.split(",") if c]
    if any(k < 1 for k in args.sweeps):
        ap.error("--sweeps: sweep counts are at least 1")
    if any(k < 1 for k in args.rhs):
        ap.error("--rhs: column counts are at least 1")
    os.environ.setdefault("OMP_NUM_THREADS", "16")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("trsv_bench.py needs a GPU: the engine has no CPU path")
    import bench
    import spmv_host as H
    import spmv_mi355x as E
    from solver_bench import stencil27
    rows = []
    for item in args.runs.split(","):
        w, dts = item.split(":")
        if w.startswith("stencil"):
            rp, ci, va, n = stencil27(int(w[len("stencil"):]))
            data = "generated"
        elif w.startswith("grid2d"):
            from amg_bench import grid2d
            rp, ci, va, n = grid2d(int(w[len("grid2d"):]), 0.001)
            data = "generated"
        else:
            A, data = bench.load_workload(H, w, args.scale)
            if A["m"] != A["n"]:
                raise SystemExit(f"{w}: {A['m']} x {A['n']} is not square")
            rp, ci, va, n = A["row_ptr"], A["col_idx"], np.ascontiguousarray(A["values"], np.float64), A["n"]
            del A
        if args.update:
            rows += run_update(E, torch, w, np.asarray(rp, np.int32), ci, np.ascontiguousarray(va, np.float64), n, dts, args)
            continue
        rows.append(run(E, torch, w, rp, ci, va, n, dts, data, args))
        del rp, ci, va
    if args.update:
        print(f"{'workload':11s} {'dtype':5s} {'variant':>16s} {'slots':>10s} {'create s':>9s} {'update s':>9s} {'host form s':>11s} "
              f"{'create / update':>15s} {'update GB/s':>11s}")
        for r in rows:
            c, u = r["create_seconds"]["median"], r["update_device_seconds"]["median"]
            print(f"{r['workload']:11s} {r['dtype']:5s} {r['variant']:>16s} {r['slots']:10d} {c:9.4f} {u:9.6f} "
                  f"{r['update_host_seconds']['median']:11.4f} {c / max(u, 1e-9):15.1f} {r['update_bytes'] / max(u, 1e-9) / 1e9:11.1f}")
        return
    print(f"{'workload':11s} {'dtype':5s} {'n':>9s} {'kept nnz':>10s} {'levels':>7s} {'widest':>8s} {'spmv ms':>9s} | "
          f"{'chain_rows':>10s} {'launches':>8s} {'trsv ms':>9s} {'spread':>19s} {'/ floor':>8s}")
    for r in rows:
        for k, s in enumerate(r["sweep"]):
            head = (f"{r['workload']:11s} {r['dtype']:5s} {r['n']:9d} {r['nnz_kept']:10d} {r['levels']:7d} {r['max_level_rows']:8d} "
                    f"{r['spmv_ms']:9.4f}") if k == 0 else " " * 65
            print(f"{head} | {s['chain_rows']:10d} {s['launches']:8d} {s['ms']:9.4f} {s['spread'][0]:9.4f} ..{s['spread'][1]:8.4f} "
                  f"{s['over_floor']:8.2f}")
    if args.block_rows:
        print(f"{'workload':11s} {'dtype':5s} | {'block_rows':>10s} {'blocks':>7s} {'levels':>7s} {'widest':>7s} {'dropped':>8s} {'trsv ms':>9s} "
              f"{'spread':>19s} {'/ floor':>8s} {'/ global':>9s}")
        for r in rows:
            for s in r["blocked"]:
                print(f"{r['workload']:11s} {r['dtype']:5s} | {s['block_rows']:10d} {s['blocks']:7d} {s['max_block_levels']:7d} "
                      f"{s['max_level_rows']:7d} {100 * s['dropped_share']:7.2f}% {s['ms']:9.4f} {s['spread'][0]:9.4f} ..{s['spread'][1]:8.4f} "
                      f"{s['over_floor']:8.2f} {s['over_global']:9.4f}")
    if args.sweeps:
        print(f"{'workload':11s} {'dtype':5s} | {'sweeps':>6s} {'k':>6s} {'run':>4s} {'launches':>8s} {'solve ms':>9s} {'spread':>19s} "
              f"{'ms / sweep':>10s} {'exact ms':>9s} {'column / exact':>14s} {'column / spmv':>13s}")
        for r in rows:
            for s in r["sweeps"]:
                print(f"{r['workload']:11s} {r['dtype']:5s} | {s['sweeps']:6d} {s['k'] or 'single':>6} {s['effective']:4d} {s['launches']:8d} "
                      f"{s['ms']:9.4f} {s['spread'][0]:9.4f} ..{s['spread'][1]:8.4f} {s['ms_per_sweep']:10.4f} {r['sweep'][0]['ms']:9.4f} "
                      f"{s['per_column_over_exact']:14.4f} {s['per_column_over_floor']:13.2f}")
    if args.rhs:
        print(f"{'workload':11s} {'dtype':5s} | {'block_rows':>10s} {'k':>3s} {'passes':>6s} {'launches':>8s} {'solve ms':>9s} {'spread':>19s} "
              f"{'single ms':>9s} {'spread':>19s} {'per column / single':>19s}")
        for r in rows:
            for s in r["rhs"]:
                print(f"{r['workload']:11s} {r['dtype']:5s} | {s['block_rows'] or 'global':>10} {s['k']:3d} {s['passes']:6d} {s['launches']:8d} "
                      f"{s['ms']:9.4f} {s['spread'][0]:9.4f} ..{s['spread'][1]:8.4f} {s['single_ms']:9.4f} {s['single_spread'][0]:9.4f} .."
                      f"{s['single_spread'][1]:8.4f} {s['per_column_over_single']:19.4f}")


if __name__ == "__main__":
    main()
