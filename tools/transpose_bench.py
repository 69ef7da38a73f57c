"""A handle of A^t built on the GPU (opts.transpose = 1; include/spmv_mi355x.h "transposed handles") against what a caller pays without it.

For a workload twin of bench.py, in one process and alternating window by window:
  stream_t:     create_from_stream with transpose = 1 on a CSR resident in device memory (the transposition + the builder);
  stream:       the same call without transposition (the builder alone);
  create_t:     spmv_mi355x_create with transpose = 1 from the host arrays (upload, transposition, download, builder);
  host_t:       a scipy host transposition (csr -> csc arrays) followed by create() — what such a caller does today;
  spmv / spmv_t one SpMV of the A handle and one of the A^t handle, HIP events over `reps` launches.
The two stream legs are timed with HIP events on the current stream around the create_from_stream call (the pieces are appended
before, outside the timed region) and with the wall clock beside them; create_t and host_t are wall clock. The median of the windows is reported per
leg, with the spread. After the timing the product of the stream_t handle is compared bit for bit with that of the create_t handle.

    python tools/transpose_bench.py                                   # nlpkkt240 fp64, cant fp64 (delta layout)
    python tools/transpose_bench.py --runs cant:f64 --windows 7
    python tools/transpose_bench.py --runs nlpkkt240:f64:sell_values=2
One JSON line per run and a table at the end.
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

STREAM_OPTS = dict(sell_c=64, sell_delta=1, sell_window=2)         # what create_from_stream builds: the SELL-64 delta layout


def wall(torch, fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def stream_of(E, A, pieces=8):
    m, rp, ci, va = A["m"], A["row_ptr"], A["col_idx"], A["values"]
    st = E.CsrStream(m, A["n"], int(rp[m]))
    cuts = [m * k // pieces for k in range(pieces + 1)]
    for r0, r1 in zip(cuts[:-1], cuts[1:]):
        if r1 > r0:
            st.append(rp[r0:r1 + 1] - rp[r0], ci[rp[r0]:rp[r1]], va[rp[r0]:rp[r1]])
    return st


def finish_timed(torch, st, np_dtype, opts):
    """(event ms, wall ms, handle) of create_from_stream alone: the stream is filled before"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    M = st.finish("sell_c_sigma", np_dtype, **opts)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), (time.perf_counter() - t0) * 1e3, M


def run(E, torch, A, data, workload, dts, extra, windows, reps):
    import scipy.sparse as sp
    m, n = A["m"], A["n"]
    rp, ci, va = A["row_ptr"], A["col_idx"], np.ascontiguousarray(A["values"], np.float64)
    A = dict(A, values=va)
    opts = dict(STREAM_OPTS)
    opts.update(extra)
    np_dtype = np.float32 if dts == "f32" else np.float64
    if dts == "mixed":
        opts["value_storage"] = 1
    tdt = torch.float32 if dts == "f32" else torch.float64
    xa = (torch.rand(n, device="cuda", dtype=torch.float64) * 2 - 1).to(tdt)       # x of A, y of A^t has n values
    xt = (torch.rand(m, device="cuda", dtype=torch.float64) * 2 - 1).to(tdt)
    ya = torch.empty(m + 64, dtype=tdt, device="cuda")
    yt = torch.empty(n + 64, dtype=tdt, device="cuda")
    stream = torch.cuda.current_stream()
    legs = {k: [] for k in ("stream_t", "stream_t_wall", "stream", "stream_wall", "create_t", "host_t", "host_t_scipy", "spmv", "spmv_t")}
    keep = {}
    for w in range(windows + 1):                          # window 0 warms every leg up and is dropped
        for M in keep.values():
            M.close()
        t_st, t_stw, keep["stream_t"] = finish_timed(torch, stream_of(E, A), np_dtype, dict(opts, transpose=1))
        t_s, t_sw, keep["stream"] = finish_timed(torch, stream_of(E, A), np_dtype, opts)
        t_ct, keep["create_t"] = wall(torch, lambda: E.Matrix(rp, ci, va, m, n, "sell_c_sigma", np_dtype, transpose=1, **opts))
        t0 = time.perf_counter()
        T = sp.csr_matrix((va, ci, rp), shape=(m, n)).tocsc()           # the CSC arrays of A are the CSR arrays of A^t
        t_sc = (time.perf_counter() - t0) * 1e3
        t_h, keep["host_t"] = wall(torch, lambda: E.Matrix(T.indptr, T.indices, T.data, n, m, "sell_c_sigma", np_dtype, **opts))
        del T
        t_v = keep["stream"].time_device(xa.data_ptr(), ya.data_ptr(), reps, stream.cuda_stream)
        t_vt = keep["stream_t"].time_device(xt.data_ptr(), yt.data_ptr(), reps, stream.cuda_stream)
        if w:
            for name, t in zip(legs, (t_st, t_stw, t_s, t_sw, t_ct, t_h + t_sc, t_sc, t_v, t_vt)):
                legs[name].append(t)
    y2 = torch.empty_like(yt)
    keep["stream_t"].spmv_device(xt.data_ptr(), yt.data_ptr(), 0, stream.cuda_stream)
    keep["create_t"].spmv_device(xt.data_ptr(), y2.data_ptr(), 0, stream.cuda_stream)
    torch.cuda.synchronize()
    if keep["stream_t"].format_name != keep["create_t"].format_name or not torch.equal(yt[:n], y2[:n]):
        raise SystemExit(f"{workload} {dts}: the handle from the stream ({keep['stream_t'].format_name}) differs from create()'s ({keep['create_t'].format_name})")
    rec = dict(workload=workload, dtype=dts, opts=extra, data=data, format=keep["stream"].format_name, format_t=keep["stream_t"].format_name,
               m=int(m), n=int(n), nnz=int(keep["stream"].nnz), windows=windows, spmv_reps=reps)
    for name, ts in legs.items():
        rec[name + "_ms"] = round(float(np.median(ts)), 4)
        rec[name + "_spread"] = [round(min(ts), 4), round(max(ts), 4)]
    rec["transposition_ms"] = round(rec["stream_t_ms"] - rec["stream_ms"], 4)
    print(json.dumps(rec), flush=True)
    for M in keep.values():
        M.close()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", default="nlpkkt240:f64,cant:f64", help="workload:f64|f32|mixed[:k=v+k=v],...")
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20, help="SpMV launches per timed window")
    ap.add_argument("--scale", type=float, default=1.0, help="shrink the workloads")
    args = ap.parse_args()
    if args.windows < 5:
        ap.error("--windows: at least 5")
    os.environ.setdefault("OMP_NUM_THREADS", "16")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("transpose_bench.py needs a GPU: the engine has no CPU path")
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
        rows.append(run(E, torch, A, data, w, dts, extra, args.windows, args.reps))
    print(f"{'workload':10s} {'format of A^t':30s} {'stream_t ms':>11s} {'stream ms':>10s} {'create_t ms':>11s} {'host_t ms':>10s} {'spmv ms':>9s} {'spmv_t ms':>9s}")
    for r in rows:
        print(f"{r['workload']:10s} {r['format_t']:30s} {r['stream_t_ms']:11.2f} {r['stream_ms']:10.2f} {r['create_t_ms']:11.2f} {r['host_t_ms']:10.2f} "
              f"{r['spmv_ms']:9.4f} {r['spmv_t_ms']:9.4f}")


if __name__ == "__main__":
    main()
