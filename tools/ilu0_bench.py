"""What the device ILU(0) costs and what it buys (spmv_mi355x_ilu0_*; include/spmv_mi355x.h "ILU(0)").

For every workload and every variant (global, and blocked at every --block-rows value) the tool reports
  create:    seconds of spmv_mi355x_ilu0_create (host checks and analysis, uploads), once;
  factor:    seconds of the blocking host call (upload of the values included) and of factor_device on resident values with a
             synchronise behind it, medians over --windows calls after one warm-up, with min .. max;
  host:      seconds of the sequential C loop of tests/ilu0_reference.c on the same values (gcc -O2), once, and whether the device
             factor has its bits;
  levels, launches, the share of A's entries the blocks drop.
On the symmetric positive definite workloads it then solves A x = b with spmv_mi355x_pcg_tri to --tol under ILU(0) (each variant),
under the global SGS of A and under no preconditioner: iterations, seconds, and ms per iteration from a tol = 0 run of --steps
iterations minus a run of 0 iterations. On convdiff<k> it solves with gmres(--restart) under the blocked ILU(0) and the blocked SGS.
No threshold is set and no speed is promised.

Workloads: stencil<N> (the 27-point stencil of tools/solver_bench.py, --stencil-diag on the diagonal), grid2d<N> (the 5-point operator
of tools/amg_bench.py with --shift), convdiff<k> (tools/gmres_bench.py), and any generated twin of spmv_host.gen_named such as cant
(factorization only; its columns are sorted first, and a pattern ILU(0) refuses is reported with the refusal: the cant twin stores
a diagonal in few of its rows, --add-diagonal factorizes A + diag(1 + row sums of |a|) instead).

    python tools/ilu0_bench.py                                       # stencil160, grid2d2000, cant, convdiff1000; global and B = 4096
    python tools/ilu0_bench.py --runs grid2d2000 --block-rows 1024,4096,16384
    python tools/ilu0_bench.py --runs stencil160 --no-solve          # factorization only
With --refresh nothing above is solved. Per workload and variant the tool factorizes V1, builds the triple with precond() and then
times, in one process and in --windows alternating windows after a warm-up, a refactorization on new values V2 two ways:
  rebuild:  factor(V2) + precond(): host values in, f copied back, two trsv_create calls; the only path before trsv handles could
            take new values, and still callable;
  refresh:  factor_device(V2 resident) + update_precond(triple) and a synchronise: no host copy of f, no analysis, no layout;
and, apart from the factorization, precond() alone against update_precond() alone. Medians with min .. max, the bytes the two
updates move by the layout's own count, and whether the refreshed handles have the rebuilt handles' bytes. No ratio is asserted.
    python tools/ilu0_bench.py --refresh --runs stencil160,grid2d2000 --block-rows 4096 --windows 7
With --sweeps 2,3,4,8 nothing above is timed either. On every symmetric positive definite workload the tool solves A x = b with
spmv_mi355x_pcg_tri to --tol under the GLOBAL ILU(0) and the GLOBAL SGS of A with their triangular solves replaced by that many Jacobi
sweeps (spmv_mi355x_trsv_set_sweeps, the same count on both handles), and beside them under the exact global forms, the blocked forms
at every --block-rows value and no preconditioner. One pair of global handles per preconditioner serves every sweep count. All legs run
in one process in --windows alternating windows after a warm-up window: per leg the iterations, the stop code, the median seconds of
the whole call with min .. max, the launches of the two triangular solves per iteration, and the ratio to the fastest leg. No ratio is
asserted; a sweep count that loses is reported as it comes out.
    python tools/ilu0_bench.py --sweeps 2,3,4,8 --runs stencil160,grid2d2000 --block-rows 4096 --windows 5
One JSON line per variant."""
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


def load(workload, args):
    """(row_ptr, col_idx, values, n, kind): kind is "spd", "nonsymmetric" or "factor only" """
    if workload.startswith("stencil"):
        from solver_bench import stencil27
        return stencil27(int(workload[len("stencil"):]), args.stencil_diag) + ("spd",)
    if workload.startswith("grid2d"):
        from amg_bench import grid2d
        return grid2d(int(workload[len("grid2d"):]), args.shift) + ("spd",)
    if workload.startswith("convdiff"):
        from gmres_bench import convdiff_csr
        return convdiff_csr(int(workload[len("convdiff"):])) + ("nonsymmetric",)
    import scipy.sparse as sp
    import spmv_host as H
    A = H.gen_named(workload, args.scale)
    if A["m"] != A["n"]:
        raise SystemExit(f"{workload} is {A['m']} x {A['n']}: ILU(0) needs a square matrix")
    S = sp.csr_matrix((A["values"], A["col_idx"], A["row_ptr"]), shape=(A["m"], A["n"]))
    S.sum_duplicates()
    if args.add_diagonal:                                     # A + diag(1 + the row sums of |a|): a stored, dominant diagonal in every row
        S = (S + sp.diags(1.0 + np.asarray(abs(S).sum(axis=1)).ravel())).tocsr()
    S.sort_indices()
    return S.indptr.astype(np.int32), S.indices.astype(np.int32), S.data.astype(np.float64), A["n"], "factor only"


def spread(ts):
    return dict(median=round(float(np.median(ts)), 6), min=round(min(ts), 6), max=round(max(ts), 6))


def factor_legs(E, torch, ic, workload, rp, ci, va, n, B, args):
    t0 = time.perf_counter()
    F = E.Ilu0(rp, ci, n, block_rows=B)
    create = time.perf_counter() - t0
    dev = torch.from_numpy(va).cuda()
    torch.cuda.synchronize()
    host, device = [], []
    for w in range(args.windows + 1):                         # window 0 warms up and is dropped
        t0 = time.perf_counter()
        F.factor(va)
        t1 = time.perf_counter()
        F.factor_device(dev.data_ptr())
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        if w:
            host.append(t1 - t0)
            device.append(t2 - t1)
    info = F.info
    rec = dict(workload=workload, n=int(n), nnz=int(len(ci)), variant="global" if B is None else f"B={info['block_rows']}",
               create_seconds=round(create, 4), factor_host_values=spread(host), factor_device_values=spread(device),
               levels=info["levels"], launches=info["launches"], max_level_rows=info["max_level_rows"],
               dropped_share=round(info["nnz_dropped"] / max(len(ci), 1), 4), breakdown_row=info["breakdown_row"],
               mem_mib=round(F.mem_footprint / 2 ** 20, 1), windows=args.windows)
    if not args.no_reference:
        t0 = time.perf_counter()
        want, bad = ic.reference(rp, ci, va, n, None if B is None else info["block_rows"])
        rec["reference_seconds"] = round(time.perf_counter() - t0, 4)
        rec["bit_identical"] = bool(np.array_equal(F.values(), want, equal_nan=True)) and bad == info["breakdown_row"]
    return F, rec


def refresh_legs(E, torch, workload, rp, ci, va, n, B, args):
    """--refresh: factor + precond() against factor_device + update_precond on the same new values"""
    rows = np.repeat(np.arange(n), np.diff(rp))
    v2 = np.where(rows == ci, 1.3, 0.9) * va                  # same pattern, still symmetric and dominant
    del rows
    dev = torch.from_numpy(v2).cuda()
    torch.cuda.synchronize()
    F = E.Ilu0(rp, ci, n, block_rows=B)
    M = F.factor(va).precond()
    t0 = time.perf_counter()
    F.update_precond(M)                                       # prepares both handles: once
    prepare = time.perf_counter() - t0
    rebuild, refresh, handles_new, handles_upd = [], [], [], []
    W = None
    for w in range(args.windows + 1):                         # window 0 warms up and is dropped
        close(W)
        t0 = time.perf_counter()
        F.factor(v2)
        t1 = time.perf_counter()
        W = F.precond()
        t2 = time.perf_counter()
        F.factor_device(dev.data_ptr())
        torch.cuda.synchronize()                              # only to time the two halves apart: a caller enqueues straight on
        t3 = time.perf_counter()
        F.update_precond(M)
        torch.cuda.synchronize()
        t4 = time.perf_counter()
        if w:
            rebuild.append(t2 - t0)
            handles_new.append(t2 - t1)
            refresh.append(t4 - t2)
            handles_upd.append(t4 - t3)
    same = all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for k in (0, 2)
               for x, y in zip(M[k].stored_values(), W[k].stored_values()) if x is not None)
    slots = [len(M[k].stored_values()[0]) for k in (0, 2)]
    info = F.info
    rec = dict(workload=workload, n=int(n), nnz=int(len(ci)), variant="global" if B is None else f"B={info['block_rows']}",
               prepare_and_first_update_seconds=round(prepare, 4), rebuild_seconds=spread(rebuild), refresh_seconds=spread(refresh),
               precond_seconds=spread(handles_new), update_precond_seconds=spread(handles_upd),
               update_bytes=int((slots[0] + slots[1] + n) * 20), f_bytes=int(8 * len(ci)), trsv_launches=M[0].info["launches"] + M[2].info["launches"],
               ilu0_launches=info["launches"], windows=args.windows, same_bytes=bool(same))
    close(M)
    close(W)
    F.close()
    return rec


def pcg_legs(E, A, b, M, args):
    r = A.pcg_tri(b, precond=M, tol=args.tol, max_iterations=args.max_iterations, history=False)
    fixed = A.pcg_tri(b, precond=M, tol=0.0, max_iterations=0, history=False)["seconds"]
    s = A.pcg_tri(b, precond=M, tol=0.0, max_iterations=args.steps, history=False)
    return dict(iterations=int(r["iterations"]), stop=int(r["stop"]), seconds=round(r["seconds"], 4),
                rnorm_over_b=float(r["rnorm"] / r["rnorm0"]), ms_per_iteration=round((s["seconds"] - fixed) * 1e3 / args.steps, 4))


def close(M):
    for h in M or ():
        if h is not None and not isinstance(h, np.ndarray):
            h.close()


def sweep_legs(E, workload, rp, ci, va, n, args):
    """--sweeps: whole pcg_tri solves under swept, exact and blocked ILU(0) / SGS and under nothing, in alternating windows"""
    A = E.Matrix(rp, ci, va, n, n, "sell_c_sigma", np.float64)
    b = np.random.default_rng(7).uniform(-1, 1, n)
    triples = {"ilu0 global": E.ilu0_precond(rp, ci, va, n), "sgs global": E.sgs_precond(rp, ci, va, n)}
    for B in args.block_rows:
        triples[f"ilu0 B={B}"] = E.ilu0_precond(rp, ci, va, n, block_rows=B)
        triples[f"sgs B={B}"] = E.sgs_precond(rp, ci, va, n, block_rows=B)
    legs = [("none", None, 0)]
    for name in triples:
        legs.append((name, name, 0))
        if name.endswith("global"):
            legs += [(f"{name} sweeps={s}", name, s) for s in args.sweeps]
    times, last = {leg[0]: [] for leg in legs}, {}
    for w in range(args.windows + 1):                         # window 0 warms every leg up (code objects, scratch) and is dropped
        for leg, name, s in legs:
            M = triples.get(name)
            for T in (M[0], M[2]) if M else ():
                T.set_sweeps(s)
            r = A.pcg_tri(b, precond=M, tol=args.tol, max_iterations=args.max_iterations, history=False)
            last[leg] = (r, sum(T.sweeps_info()["launches"] if s else T.info["launches"] for T in (M[0], M[2])) if M else 0)
            if w:
                times[leg].append(r["seconds"])
        print(f"# {workload}: window {w} done", flush=True)
    best = min(float(np.median(t)) for t in times.values())
    for leg, name, s in legs:
        r, launches = last[leg]
        t = spread(times[leg])
        print(json.dumps(dict(workload=workload, n=int(n), nnz=int(len(ci)), variant=leg, sweeps=s, tol=args.tol, iterations=int(r["iterations"]),
                              stop=int(r["stop"]), rnorm_over_b=float(r["rnorm"] / r["rnorm0"]), seconds=t, trsv_launches_per_iteration=launches,
                              over_fastest=round(t["median"] / best, 2), windows=args.windows)), flush=True)
    for M in triples.values():
        close(M)
    A.close()


def run(E, torch, ic, workload, args):
    rp, ci, va, n, kind = load(workload, args)
    rp = np.asarray(rp, np.int32)
    if args.sweeps:
        if kind != "spd":
            raise SystemExit(f"--sweeps compares whole CG solves: {workload} is not one of the SPD workloads")
        sweep_legs(E, workload, rp, np.asarray(ci, np.int32), np.asarray(va, np.float64), n, args)
        return
    if args.refresh:
        for B in [None] + list(args.block_rows):
            print(json.dumps(refresh_legs(E, torch, workload, rp, np.asarray(ci, np.int32), np.asarray(va, np.float64), n, B, args)),
                  flush=True)
        return
    A = None if kind == "factor only" or args.no_solve else E.Matrix(rp, ci, va, n, n, "sell_c_sigma", np.float64)
    b = np.random.default_rng(7).uniform(-1, 1, n)
    variants = ([None] if kind != "nonsymmetric" else []) + list(args.block_rows)
    for B in variants:
        try:
            F, rec = factor_legs(E, torch, ic, workload, rp, ci, va, n, B, args)
        except E.SpmvError as e:
            print(json.dumps(dict(workload=workload, variant="global" if B is None else f"B={B}", refused=str(e))), flush=True)
            continue
        if A is not None:
            t0 = time.perf_counter()
            M = F.precond()
            rec["trsv_handles_seconds"] = round(time.perf_counter() - t0, 4)
            rec["trsv_launches"] = M[0].info["launches"] + M[2].info["launches"]
            if kind == "spd":
                rec["pcg_tri"] = pcg_legs(E, A, b, M, args)
            else:
                g = A.gmres(b, restart=args.restart, precond=M, tol=args.tol, max_iterations=args.max_iterations, history=False)
                rec["gmres"] = dict(restart=args.restart, iterations=int(g["iterations"]), stop=int(g["stop"]), seconds=round(g["seconds"], 4))
            close(M)
        F.close()
        print(json.dumps(rec), flush=True)
    if A is None:
        return
    if kind == "spd":
        for name, M in (("sgs global", E.sgs_precond(rp, ci, va, n)), ("none", None)):
            print(json.dumps(dict(workload=workload, variant=name, pcg_tri=pcg_legs(E, A, b, M, args))), flush=True)
            close(M)
    else:
        for B in args.block_rows:
            M = E.sgs_precond(rp, ci, va, n, block_rows=B)
            g = A.gmres(b, restart=args.restart, precond=M, tol=args.tol, max_iterations=args.max_iterations, history=False)
            print(json.dumps(dict(workload=workload, variant=f"sgs B={B}", gmres=dict(restart=args.restart, iterations=int(g["iterations"]),
                                  stop=int(g["stop"]), seconds=round(g["seconds"], 4)))), flush=True)
            close(M)
    A.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", default="stencil160,grid2d2000,cant,convdiff1000", help="workloads, comma separated")
    ap.add_argument("--block-rows", default="4096", help="block sizes of the blocked variants, comma separated (the global one always runs)")
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--tol", type=float, default=1e-8)
    ap.add_argument("--max-iterations", type=int, default=3000)
    ap.add_argument("--steps", type=int, default=50, help="iterations of the tol = 0 leg")
    ap.add_argument("--restart", type=int, default=30)
    ap.add_argument("--stencil-diag", type=float, default=27.0)
    ap.add_argument("--shift", type=float, default=0.001)
    ap.add_argument("--scale", type=float, default=1.0, help="the scale of a generated twin")
    ap.add_argument("--add-diagonal", action="store_true",
                    help="generated twins: factorize A + diag(1 + row sums of |a|) (the cant twin stores a diagonal in few of its rows)")
    ap.add_argument("--no-solve", action="store_true", help="factorization only")
    ap.add_argument("--refresh", action="store_true",
                    help="time factor + precond() against factor_device + update_precond on new values of the same pattern")
    ap.add_argument("--no-reference", action="store_true", help="skip the sequential loop on the host")
    ap.add_argument("--sweeps", default="", help="Jacobi-sweep counts: whole CG solves under swept global ILU(0) / SGS beside the exact, "
                    "the blocked and the unpreconditioned ones, e.g. 2,3,4,8")
    args = ap.parse_args()
    args.block_rows = [int(v) for v in args.block_rows.split(",") if v != ""]
    args.sweeps = [int(v) for v in args.sweeps.split(",") if v != ""]
    if any(v < 1 for v in args.sweeps):
        ap.error("--sweeps: sweep counts are at least 1")
    os.environ.setdefault("OMP_NUM_THREADS", "16")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("ilu0_bench.py needs a GPU: the engine has no CPU path")
    import ilu0_cases as ic
    import spmv_mi355x as E
    for workload in args.runs.split(","):
        run(E, torch, ic, workload, args)


if __name__ == "__main__":
    main()
