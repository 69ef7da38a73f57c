"""k vectors at once against k single-vector SpMVs, on the workloads of bench.py and the handle bench.py builds for them.

For k in {1, 2, 4, 8} two legs alternate in one process, both on torch-allocated vectors (so placement does not differ between them):
  single: k launches of spmv_device, one per contiguous column x_j -> y_j;
  spmm:   one spmm_device on a row-major (n, k) tensor X -> (m, k) tensor Y.
Each leg is timed in windows (HIP events on the launch stream inside a synchronize bracket, after a warm-up); the median window of
each leg is reported as ms per call of the leg, ms per vector, and the spmm / single ratio. Before timing, the spmm columns are
checked bit for bit against the single-vector products.

    python tools/spmm_bench.py                                   # nlpkkt240 fp64, nlpkkt240 fp32, cant fp64
    python tools/spmm_bench.py --runs nlpkkt240:f64 --ks 4 --windows 7
    python tools/spmm_bench.py --runs cant:f64:sell_window=2        # options on top of bench.py's (key=value, '+'-separated)
One JSON line per (workload, dtype, k) and a table at the end.
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


def time_window(torch, stream, fn, reps):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for _ in range(reps):
        fn()
    e1.record(stream)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def run(E, H, bench, torch, workload, dts, extra, ks, windows, reps, warmup, scale):
    A, data = bench.load_workload(H, workload, scale)
    m, n = A["m"], A["n"]
    fmt = bench.DEFAULT_FORMAT.get(workload, "csr_vector")
    opts = dict(bench.DEFAULT_OPTS.get(workload, {}))
    opts.update(extra)
    np_dtype = np.float64 if dts == "f64" else np.float32
    M = E.Matrix(A["row_ptr"], A["col_idx"], A["values"], m, n, fmt, np_dtype, **opts)
    del A
    tdt = torch.float64 if dts == "f64" else torch.float32
    stream = torch.cuda.current_stream()
    sp = stream.cuda_stream
    g = torch.Generator(device="cuda")
    g.manual_seed(14)
    out = []
    for k in ks:
        X = (torch.rand((n, k), generator=g, device="cuda", dtype=torch.float64) * 2 - 1).to(tdt)
        Y = torch.empty((m, k), dtype=tdt, device="cuda")
        xs = [X[:, j].contiguous() for j in range(k)]
        ys = [torch.empty(m + 64, dtype=tdt, device="cuda") for _ in range(k)]

        def single():
            for j in range(k):
                M.spmv_device(xs[j].data_ptr(), ys[j].data_ptr(), 0, sp)

        def spmm():
            M.spmm_device(k, X.data_ptr(), k, Y.data_ptr(), k, 0, sp)

        single()
        spmm()
        torch.cuda.synchronize()
        for j in range(k):
            if not torch.equal(Y[:, j], ys[j][:m]):
                raise SystemExit(f"{workload} {dts} k={k}: spmm column {j} differs from the single-vector product")
        for _ in range(warmup):
            single()
            spmm()
        t_single, t_spmm = [], []
        for _ in range(windows):                       # the two legs alternate window by window
            t_single.append(time_window(torch, stream, single, reps))
            t_spmm.append(time_window(torch, stream, spmm, reps))
        ms1, ms2 = float(np.median(t_single)), float(np.median(t_spmm))
        rec = dict(workload=workload, dtype=dts, opts=extra, data=data, format=M.format_name, k=k, windows=windows, reps=reps,
                   single_ms=round(ms1, 4), spmm_ms=round(ms2, 4), single_ms_per_vector=round(ms1 / k, 4),
                   spmm_ms_per_vector=round(ms2 / k, 4), ratio=round(ms2 / ms1, 4),
                   single_spread=[round(min(t_single), 4), round(max(t_single), 4)], spmm_spread=[round(min(t_spmm), 4), round(max(t_spmm), 4)])
        print(json.dumps(rec), flush=True)
        out.append(rec)
        del X, Y, xs, ys
    M.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", default="nlpkkt240:f64,nlpkkt240:f32,cant:f64", help="workload:dtype,...")
    ap.add_argument("--ks", default="1,2,4,8")
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20, help="calls of a leg per timed window")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--scale", type=float, default=1.0, help="shrink the workloads (tests only)")
    args = ap.parse_args()
    if args.windows < 5:
        ap.error("--windows: at least 5")
    os.environ.setdefault("OMP_NUM_THREADS", "16")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("spmm_bench.py needs a GPU: the engine has no CPU path")
    import bench
    import spmv_host as H
    import spmv_mi355x as E
    ks = [int(k) for k in args.ks.split(",")]
    rows = []
    for item in args.runs.split(","):
        w, dts, *more = item.split(":")
        extra = {kv.split("=")[0]: int(kv.split("=")[1]) for kv in (more[0].split("+") if more else [])}
        rows += run(E, H, bench, torch, w, dts, extra, ks, args.windows, args.reps, args.warmup, args.scale)
    print(f"{'workload':12s} {'format':28s} {'dtype':5s} {'k':>2s} {'single ms':>10s} {'spmm ms':>10s} {'ms/vec 1':>9s} {'ms/vec k':>9s} {'ratio':>6s}")
    for r in rows:
        print(f"{r['workload']:12s} {r['format']:28s} {r['dtype']:5s} {r['k']:2d} {r['single_ms']:10.4f} {r['spmm_ms']:10.4f} {r['single_ms_per_vector']:9.4f} "
              f"{r['spmm_ms_per_vector']:9.4f} {r['ratio']:6.3f}")


if __name__ == "__main__":
    main()
