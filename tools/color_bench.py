"""What the multicolour ordering costs and what it buys (spmv_mi355x_color_*; include/spmv_mi355x.h "multicolour ordering").

Every leg is compared with the same quantity on the NATURAL ordering in the same run, all legs of a workload in one process, the timed
legs in --windows alternating windows after a warm-up window that is dropped. Per workload the tool reports
  setup:   seconds of Coloring(...) split as info() splits them (transposition, rounds, sort), against the sequential greedy loop of
           tests/color_reference.c on the host (and whether the device has its colours); colours, rounds, the largest and smallest
           class; seconds of the first permute_csr (forms B on the device) and of a later one (copies);
  spmv:    ms of one SpMV of a handle of B = P A P^t against a handle of A with the same options, and their format names (the
           permutation may cost the SELL delta layout its index-free slices: this ratio taxes every iteration);
  trsv:    ms and launches of one exact solve of tril(B) against the exact solve and the 2-sweep solve of tril(A);
  ilu0:    seconds and launches of Ilu0.factor_device on B against A (resident values, a synchronise behind each);
  pcg_tri: whole solves to --tol, seconds and iterations: plain CG on A; exact, 2-sweep and blocked (--block-rows) SGS and ILU(0) on A;
           multicolour SGS and ILU(0) on B, where the time INCLUDES permuting b and unpermuting x on the device.
No threshold is set and no speed is promised; a leg that loses is reported as it comes out.

Workloads are tools/ilu0_bench.py's, with :f64 or :f32 for the precision of the handles (the factorization is always fp64): stencil<N>,
grid2d<N> (symmetric positive definite: every leg) and generated twins such as cant (setup, spmv, and with --add-diagonal trsv and ilu0;
no whole solves).

    python tools/color_bench.py --runs stencil160:f64,grid2d2000:f64,cant:f64 --windows 7
One JSON line per leg."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "spmv-research_amd", "python"), os.path.join(ROOT, "tools"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def spread(ts, digits=6):
    return dict(median=round(float(np.median(ts)), digits), min=round(min(ts), digits), max=round(max(ts), digits))


def close(M):
    for h in M or ():
        if h is not None and not isinstance(h, np.ndarray):
            h.close()


def out(workload, leg, **rec):
    print(json.dumps(dict(workload=workload, leg=leg, **rec)), flush=True)


def setup_leg(E, cc, workload, rp, ci, va, n, args):
    t0 = time.perf_counter()
    col = E.Coloring(rp, ci, n)
    create = time.perf_counter() - t0
    info = col.info()
    rec = dict(n=int(n), nnz=int(len(ci)), create_seconds=round(create, 4), colors=info["num_colors"], rounds=info["rounds"],
               symmetric=info["symmetric"], max_class=info["max_class"], min_class=info["min_class"],
               transpose_seconds=round(info["transpose_seconds"], 5), round_seconds=round(info["round_seconds"], 5),
               sort_seconds=round(info["sort_seconds"], 5))
    if not args.no_reference:
        t0 = time.perf_counter()
        colors, nc, rounds = cc.color_of(rp, ci, n)
        rec["host_greedy_seconds"] = round(time.perf_counter() - t0, 4)
        rec["same_colours"] = bool(np.array_equal(colors, col.colors)) and rounds == info["rounds"]
    t0 = time.perf_counter()
    rp_b, ci_b, va_b, emap = col.permute_csr(va)
    rec["permute_csr_first_seconds"] = round(time.perf_counter() - t0, 4)
    rec["permute_on_device_seconds"] = round(col.info()["permute_seconds"], 5)
    t0 = time.perf_counter()
    col.permute_csr(va)
    rec["permute_csr_again_seconds"] = round(time.perf_counter() - t0, 4)
    rec["mem_mib"] = round(col.mem_footprint / 2 ** 20, 1)
    out(workload, "setup", **rec)
    return col, rp_b, ci_b, va_b


def spmv_leg(E, torch, workload, A, B, n, tdt, args):
    x = torch.rand(n, dtype=tdt, device="cuda")
    y = torch.zeros(n, dtype=tdt, device="cuda")
    ms = {"A": [], "B": []}
    for w in range(args.windows + 1):
        for name, M in (("A", A), ("B", B)):
            t = M.time_device(x.data_ptr(), y.data_ptr(), args.iters)
            if w:
                ms[name].append(t)
    a, b = spread(ms["A"], 5), spread(ms["B"], 5)
    out(workload, "spmv", natural_ms=a, multicolour_ms=b, natural_format=A.format_name, multicolour_format=B.format_name,
        multicolour_over_natural=round(b["median"] / a["median"], 3), windows=args.windows)


def trsv_leg(E, torch, workload, natural, colour, n, dtype, tdt, args):
    """natural / colour: (rp, ci, va) of A and of B"""
    b = torch.rand(n, dtype=tdt, device="cuda")
    x = torch.zeros(n, dtype=tdt, device="cuda")
    TA = E.TriangularSolve(*natural, n, uplo="lower", dtype=dtype)
    TB = E.TriangularSolve(*colour, n, uplo="lower", dtype=dtype)
    legs = (("natural exact", TA, 0), ("natural 2 sweeps", TA, 2), ("multicolour exact", TB, 0))
    ms = {leg[0]: [] for leg in legs}
    launches = {}
    for w in range(args.windows + 1):
        for name, T, s in legs:
            T.set_sweeps(s)
            t = T.time_device(b.data_ptr(), x.data_ptr(), args.trsv_iters)
            launches[name] = T.sweeps_info()["launches"] if s else T.info["launches"]
            if w:
                ms[name].append(t)
    TA.set_sweeps(0)
    rec = {name.replace(" ", "_") + "_ms": spread(t, 5) for name, t in ms.items()}
    out(workload, "trsv lower", levels_natural=TA.info["levels"], levels_multicolour=TB.info["levels"],
        launches={k.replace(" ", "_"): v for k, v in launches.items()}, windows=args.windows,
        natural_exact_over_multicolour=round(rec["natural_exact_ms"]["median"] / rec["multicolour_exact_ms"]["median"], 2),
        natural_2_sweeps_over_multicolour=round(rec["natural_2_sweeps_ms"]["median"] / rec["multicolour_exact_ms"]["median"], 2), **rec)
    TA.close()
    TB.close()


def ilu0_leg(E, torch, workload, natural, colour, n, args):
    rec, secs = {}, {"natural": [], "multicolour": []}
    hs = {}
    for name, (rp, ci, va) in (("natural", natural), ("multicolour", colour)):
        try:
            hs[name] = (E.Ilu0(rp, ci, n), torch.from_numpy(np.ascontiguousarray(va)).cuda())
        except E.SpmvError as e:
            out(workload, "ilu0", refused=str(e))
            close(h for h, _ in hs.values())
            return
    torch.cuda.synchronize()
    for w in range(args.windows + 1):
        for name, (F, dev) in hs.items():
            t0 = time.perf_counter()
            F.factor_device(dev.data_ptr())
            torch.cuda.synchronize()
            if w:
                secs[name].append(time.perf_counter() - t0)
    for name, (F, dev) in hs.items():
        info = F.info
        rec[name] = dict(seconds=spread(secs[name]), launches=info["launches"], levels=info["levels"], breakdown_row=info["breakdown_row"])
        F.close()
    out(workload, "ilu0 factor_device", windows=args.windows,
        natural_over_multicolour=round(rec["natural"]["seconds"]["median"] / rec["multicolour"]["seconds"]["median"], 2), **rec)


def pcg_leg(E, torch, workload, A, B, natural, colour, col, n, dtype, tdt, args):
    b = np.random.default_rng(7).uniform(-1, 1, n).astype(dtype)
    rp, ci, va = natural
    triples = {"sgs exact": E.sgs_precond(rp, ci, va, n, dtype=dtype), "ilu0 exact": E.ilu0_precond(rp, ci, va, n, dtype=dtype)}
    for Bk in args.block_rows:
        triples[f"sgs B={Bk}"] = E.sgs_precond(rp, ci, va, n, dtype=dtype, block_rows=Bk)
        triples[f"ilu0 B={Bk}"] = E.ilu0_precond(rp, ci, va, n, dtype=dtype, block_rows=Bk)
    colour_triples = {"sgs multicolour": E.sgs_precond(*colour, n, dtype=dtype), "ilu0 multicolour": E.ilu0_precond(*colour, n, dtype=dtype)}
    legs = [("none", None, 0)]
    for name in triples:
        legs.append((name, name, 0))
        if name.endswith("exact"):
            legs.append((name.replace("exact", "2 sweeps"), name, 2))
    legs += [(name, name, 0) for name in colour_triples]
    d_b = torch.from_numpy(b).cuda()
    d_pb, d_px, d_x = (torch.zeros(n, dtype=tdt, device="cuda") for _ in range(3))
    times, last = {leg[0]: [] for leg in legs}, {}
    for w in range(args.windows + 1):
        for leg, name, s in legs:
            if name in colour_triples:
                M = colour_triples[name]
                t0 = time.perf_counter()
                col.permute_device(d_b.data_ptr(), d_pb.data_ptr(), 1, dtype)
                torch.cuda.synchronize()
                pb = d_pb.cpu().numpy()
                t1 = time.perf_counter()
                r = B.pcg_tri(pb, precond=M, tol=args.tol, max_iterations=args.max_iterations, history=False)
                t2 = time.perf_counter()
                d_px.copy_(torch.from_numpy(r["x"]))
                col.unpermute_device(d_px.data_ptr(), d_x.data_ptr(), 1, dtype)
                torch.cuda.synchronize()
                t3 = time.perf_counter()
                seconds = r["seconds"] + (t1 - t0) + (t3 - t2)      # the two copies across the host are pcg_tri's own host interface
                launches = M[0].info["launches"] + M[2].info["launches"]
            else:
                M = triples.get(name)
                for T in (M[0], M[2]) if M else ():
                    T.set_sweeps(s)
                r = A.pcg_tri(b, precond=M, tol=args.tol, max_iterations=args.max_iterations, history=False)
                seconds = r["seconds"]
                launches = sum(T.sweeps_info()["launches"] if s else T.info["launches"] for T in (M[0], M[2])) if M else 0
            last[leg] = (r, launches)
            if w:
                times[leg].append(seconds)
        print(f"# {workload}: window {w} done", flush=True)
    best = min(float(np.median(t)) for t in times.values())
    for leg, name, s in legs:
        r, launches = last[leg]
        t = spread(times[leg])
        out(workload, "pcg_tri", variant=leg, tol=args.tol, iterations=int(r["iterations"]), stop=int(r["stop"]),
            rnorm_over_b=float(r["rnorm"] / r["rnorm0"]), seconds=t, trsv_launches_per_iteration=launches,
            over_fastest=round(t["median"] / best, 2), windows=args.windows)
    for M in list(triples.values()) + list(colour_triples.values()):
        close(M)


def run(E, torch, cc, workload, dtype, args):
    from ilu0_bench import load
    rp, ci, va, n, kind = load(workload, args)
    rp, ci, va = np.asarray(rp, np.int32), np.asarray(ci, np.int32), np.asarray(va, np.float64)
    tdt = torch.float64 if dtype == np.float64 else torch.float32
    col, rp_b, ci_b, va_b = setup_leg(E, cc, workload, rp, ci, va, n, args)
    A = E.Matrix(rp, ci, va, n, n, args.format, dtype)
    B = E.Matrix(rp_b, ci_b, va_b, n, n, args.format, dtype)
    spmv_leg(E, torch, workload, A, B, n, tdt, args)
    rows = np.repeat(np.arange(n), np.diff(rp))
    has_diagonal = np.unique(rows[ci == rows]).size == n
    del rows
    if has_diagonal:
        trsv_leg(E, torch, workload, (rp, ci, va), (rp_b, ci_b, va_b), n, dtype, tdt, args)
        ilu0_leg(E, torch, workload, (rp, ci, va), (rp_b, ci_b, va_b), n, args)
    else:
        out(workload, "trsv lower", skipped="rows without a stored diagonal (try --add-diagonal)")
    if kind == "spd" and not args.no_solve:
        pcg_leg(E, torch, workload, A, B, (rp, ci, va), (rp_b, ci_b, va_b), col, n, dtype, tdt, args)
    A.close()
    B.close()
    col.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", default="stencil160:f64,grid2d2000:f64,cant:f64", help="workload:precision, comma separated")
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--format", default="sell_c_sigma")
    ap.add_argument("--block-rows", default="4096", help="block sizes of the blocked natural-order legs, comma separated")
    ap.add_argument("--iters", type=int, default=50, help="SpMVs per timed window")
    ap.add_argument("--trsv-iters", type=int, default=5, help="triangular solves per timed window")
    ap.add_argument("--tol", type=float, default=1e-8)
    ap.add_argument("--max-iterations", type=int, default=3000)
    ap.add_argument("--stencil-diag", type=float, default=27.0)
    ap.add_argument("--shift", type=float, default=0.001)
    ap.add_argument("--scale", type=float, default=1.0, help="the scale of a generated twin")
    ap.add_argument("--add-diagonal", action="store_true", help="generated twins: use A + diag(1 + row sums of |a|)")
    ap.add_argument("--no-solve", action="store_true", help="no whole solves")
    ap.add_argument("--no-reference", action="store_true", help="skip the sequential greedy loop on the host")
    args = ap.parse_args()
    args.block_rows = [int(v) for v in args.block_rows.split(",") if v != ""]
    os.environ.setdefault("OMP_NUM_THREADS", "16")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("color_bench.py needs a GPU: the engine has no CPU path")
    import color_cases as cc
    import spmv_mi355x as E
    for item in args.runs.split(","):
        workload, _, prec = item.partition(":")
        if prec not in ("", "f64", "f32"):
            ap.error(f"--runs: precision of {item} must be f64 or f32")
        run(E, torch, cc, workload, np.float32 if prec == "f32" else np.float64, args)


if __name__ == "__main__":
    main()
