"""New values for an existing handle against a new handle: what spmv_mi355x_update_values saves a caller who changes the numbers of
its matrix and never the pattern (include/spmv_mi355x.h "new values for an existing handle").

For a workload twin of bench.py, in one process and alternating window by window:
  create:        E.Matrix(...) from the host arrays (what such a caller pays today: destroy + create), wall clock;
  update:        update_values from a host array of new values (a transient device copy + the kernels), wall clock;
  update_device: update_values_device from values already resident on the device, wall clock (the call is blocking), once with the
                 LDS-staged scatter (SPMV_MI355X_UPDATE_STAGE=1) and once with the per-lane walk (=0);
  spmv:          one SpMV on the handle, HIP events over `reps` launches.
The median of the windows is reported per leg, with the spread. After the timing the updated handle's product is compared bit for
bit with that of the last freshly created handle of the same values.

    python tools/update_values_bench.py                                  # nlpkkt240 fp64 (7-byte values on auto), fp64 plain, mixed; cant
    python tools/update_values_bench.py --runs cant:f64 --windows 7
    python tools/update_values_bench.py --runs nlpkkt240:f64:sell_values=2+sell_split=1
One JSON line per run and a table at the end.

--transpose runs the same protocol on the handle of A^t (opts.transpose = 1; "TRANSPOSED HANDLES" in the header): the new values stay
in A's entry order, update_values_prepare_transposed is timed once, and the legs are
  update_device: update_values_device on the A^t handle (one gather through the entry map + the update above), wall clock;
  update:        update_values from a host array of nnz(A) values, wall clock;
  create_t:      E.Matrix(..., transpose=1) from the host arrays with the new values: what this update replaces, wall clock;
  spmv_t:        one SpMV of the A^t handle, HIP events over `reps` launches.
    python tools/update_values_bench.py --transpose --runs nlpkkt240:f64,cant:f64
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "spmv-research_amd", "python")):
    if p not in sys.path:
        sys.path.insert(0, p)


def wall(torch, fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def run(E, torch, A, data, workload, fmt, base_opts, dts, extra, windows, reps):
    m, n = A["m"], A["n"]
    rp, ci, V1 = A["row_ptr"], A["col_idx"], np.ascontiguousarray(A["values"], np.float64)
    opts = dict(base_opts)
    opts.update(extra)
    np_dtype = np.float32 if dts == "f32" else np.float64
    if dts == "mixed":
        opts["value_storage"] = 1
    # new numbers of the same kind: the old ones, each scaled by a factor in [1, 2)
    rng = np.random.default_rng(5)
    V2 = V1 * rng.uniform(1.0, 1.999, V1.size)
    tdt = torch.float32 if dts == "f32" else torch.float64
    x = (torch.rand(n, device="cuda", dtype=torch.float64) * 2 - 1).to(tdt)
    y = torch.empty(m + 64, dtype=tdt, device="cuda")
    stream = torch.cuda.current_stream()
    M = E.Matrix(rp, ci, V1, m, n, fmt, np_dtype, **opts)
    if M.update_values_state() == 0:
        raise SystemExit(f"{workload} {dts} {extra}: {M.format_name} takes no update: {E.lib().spmv_mi355x_last_error().decode()}")
    t_prepare, _ = wall(torch, lambda: M.update_values_prepare(rp))
    dV = [torch.from_numpy(V1).cuda(), torch.from_numpy(V2).cuda()]
    hV = [V1, V2]
    legs = {"create": [], "update": [], "update_device_staged": [], "update_device_walk": [], "spmv": []}
    fresh = None
    for w in range(windows + 1):                          # window 0 warms every leg up and is dropped
        k = (w + 1) % 2                                   # the values alternate, so every update really changes the array
        if fresh is not None:
            fresh.close()
        t_c, fresh = wall(torch, lambda: E.Matrix(rp, ci, hV[k], m, n, fmt, np_dtype, **opts))
        t_u, _ = wall(torch, lambda: M.update_values(hV[k]))
        os.environ["SPMV_MI355X_UPDATE_STAGE"] = "1"
        t_s, _ = wall(torch, lambda: M.update_values_device(dV[k].data_ptr(), stream.cuda_stream))
        os.environ["SPMV_MI355X_UPDATE_STAGE"] = "0"
        t_w, _ = wall(torch, lambda: M.update_values_device(dV[k].data_ptr(), stream.cuda_stream))
        os.environ.pop("SPMV_MI355X_UPDATE_STAGE")
        t_v = M.time_device(x.data_ptr(), y.data_ptr(), reps, stream.cuda_stream)
        if w:
            for name, t in zip(legs, (t_c, t_u, t_s, t_w, t_v)):
                legs[name].append(t)
    y2 = torch.empty_like(y)
    M.spmv_device(x.data_ptr(), y.data_ptr(), 0, stream.cuda_stream)
    fresh.spmv_device(x.data_ptr(), y2.data_ptr(), 0, stream.cuda_stream)
    torch.cuda.synchronize()
    if M.format_name != fresh.format_name or not torch.equal(y[:m], y2[:m]):
        raise SystemExit(f"{workload} {dts}: the updated handle ({M.format_name}) differs from the fresh one ({fresh.format_name})")
    rec = dict(workload=workload, dtype=dts, opts=extra, data=data, format=M.format_name, nnz=int(M.nnz), windows=windows, spmv_reps=reps,
               prepare_ms=round(t_prepare, 3))
    for name, ts in legs.items():
        rec[name + "_ms"] = round(float(np.median(ts)), 4)
        rec[name + "_spread"] = [round(min(ts), 4), round(max(ts), 4)]
    rec["create_over_update_device"] = round(rec["create_ms"] / min(rec["update_device_staged_ms"], rec["update_device_walk_ms"]), 2)
    print(json.dumps(rec), flush=True)
    M.close()
    fresh.close()
    return rec


def run_transposed(E, torch, A, data, workload, fmt, base_opts, dts, extra, windows, reps):
    m, n = A["m"], A["n"]
    rp, ci, V1 = A["row_ptr"], A["col_idx"], np.ascontiguousarray(A["values"], np.float64)
    opts = dict(base_opts)
    opts.update(extra)
    opts["transpose"] = 1
    np_dtype = np.float32 if dts == "f32" else np.float64
    if dts == "mixed":
        opts["value_storage"] = 1
    rng = np.random.default_rng(5)
    V2 = V1 * rng.uniform(1.0, 1.999, V1.size)
    tdt = torch.float32 if dts == "f32" else torch.float64
    x = (torch.rand(m, device="cuda", dtype=torch.float64) * 2 - 1).to(tdt)      # A^t is n x m
    y = torch.empty(n + 64, dtype=tdt, device="cuda")
    stream = torch.cuda.current_stream()
    M = E.Matrix(rp, ci, V1, m, n, fmt, np_dtype, **opts)
    t_prepare, _ = wall(torch, lambda: M.update_values_prepare_transposed(rp, ci, m, n))
    if M.update_values_state() != 2:
        raise SystemExit(f"{workload} {dts} {extra}: {M.format_name} takes no update: {E.lib().spmv_mi355x_last_error().decode()}")
    dV = [torch.from_numpy(V1).cuda(), torch.from_numpy(V2).cuda()]
    hV = [V1, V2]
    legs = {"update_device": [], "update": [], "create_t": [], "spmv_t": []}
    fresh = None
    for w in range(windows + 1):                          # window 0 warms every leg up and is dropped
        k = (w + 1) % 2
        if fresh is not None:
            fresh.close()
        t_d, _ = wall(torch, lambda: M.update_values_device(dV[k].data_ptr(), stream.cuda_stream))
        t_u, _ = wall(torch, lambda: M.update_values(hV[k]))
        t_c, fresh = wall(torch, lambda: E.Matrix(rp, ci, hV[k], m, n, fmt, np_dtype, **opts))
        t_v = M.time_device(x.data_ptr(), y.data_ptr(), reps, stream.cuda_stream)
        if w:
            for name, t in zip(legs, (t_d, t_u, t_c, t_v)):
                legs[name].append(t)
    y2 = torch.empty_like(y)
    M.spmv_device(x.data_ptr(), y.data_ptr(), 0, stream.cuda_stream)
    fresh.spmv_device(x.data_ptr(), y2.data_ptr(), 0, stream.cuda_stream)
    torch.cuda.synchronize()
    if M.format_name != fresh.format_name or not torch.equal(y[:n], y2[:n]):
        raise SystemExit(f"{workload} {dts}: the updated handle ({M.format_name}) differs from the fresh one ({fresh.format_name})")
    rec = dict(workload=workload, dtype=dts, opts=extra, data=data, transpose=1, format=M.format_name, nnz=int(M.nnz), windows=windows,
               spmv_reps=reps, prepare_transposed_ms=round(t_prepare, 3))
    for name, ts in legs.items():
        rec[name + "_ms"] = round(float(np.median(ts)), 4)
        rec[name + "_spread"] = [round(min(ts), 4), round(max(ts), 4)]
    rec["create_t_over_update_device"] = round(rec["create_t_ms"] / rec["update_device_ms"], 2)
    print(json.dumps(rec), flush=True)
    M.close()
    fresh.close()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", default="nlpkkt240:f64,nlpkkt240:f64:sell_values=2,nlpkkt240:mixed,cant:f64", help="workload:f64|f32|mixed[:k=v+k=v],...")
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20, help="SpMV launches per timed window")
    ap.add_argument("--scale", type=float, default=1.0, help="shrink the workloads")
    ap.add_argument("--transpose", action="store_true", help="the legs of the A^t handle (update_values_prepare_transposed)")
    args = ap.parse_args()
    if args.windows < 5:
        ap.error("--windows: at least 5")
    os.environ.setdefault("OMP_NUM_THREADS", "16")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("update_values_bench.py needs a GPU: the engine has no CPU path")
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
        rows.append((run_transposed if args.transpose else run)(E, torch, A, data, w, bench.DEFAULT_FORMAT.get(w, "csr_vector"),
                                                                bench.DEFAULT_OPTS.get(w, {}), dts, extra, args.windows, args.reps))
    if args.transpose:
        print(f"{'workload':10s} {'format of A^t':30s} {'prepare_t ms':>12s} {'update_dev ms':>22s} {'update ms':>22s} {'create_t ms':>24s} {'spmv_t ms':>9s} {'create_t/dev':>12s}")
        sp = lambda r, k: f"{r[k + '_ms']:.3f} [{r[k + '_spread'][0]:.3f}, {r[k + '_spread'][1]:.3f}]"
        for r in rows:
            print(f"{r['workload']:10s} {r['format']:30s} {r['prepare_transposed_ms']:12.2f} {sp(r, 'update_device'):>22s} {sp(r, 'update'):>22s} "
                  f"{sp(r, 'create_t'):>24s} {r['spmv_t_ms']:9.4f} {r['create_t_over_update_device']:12.2f}")
        return
    print(f"{'workload':10s} {'format':30s} {'create ms':>10s} {'update ms':>10s} {'dev staged':>10s} {'dev walk':>10s} {'spmv ms':>9s} {'create/dev':>10s}")
    for r in rows:
        print(f"{r['workload']:10s} {r['format']:30s} {r['create_ms']:10.2f} {r['update_ms']:10.2f} {r['update_device_staged_ms']:10.3f} "
              f"{r['update_device_walk_ms']:10.3f} {r['spmv_ms']:9.4f} {r['create_over_update_device']:10.2f}")


if __name__ == "__main__":
    main()
