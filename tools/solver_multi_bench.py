#!/usr/bin/env python3
"""Time the multi-RHS solvers (spmv_mi355x_pcg_multi / _pbicgstab_multi) against k single-RHS solves in the same run.

System: tools/solver_bench.py's 27-point stencil on an N^3 grid. Right-hand sides b_j = 2^j * 1: every column takes the
single solver's iterations (powers of two scale every quantity exactly), so ms per iteration compare directly. For each
k the single and the multi solve alternate `--reps` times; ms per iteration = (best seconds - fixed seconds of a
0-iteration call) / iterations, and per RHS it is divided by k. Writes one JSON object to stdout (and --out).
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(ROOT), "spmv-research_amd", "python"))
sys.path.insert(0, ROOT)

from solver_bench import stencil27  # noqa: E402


def per_iteration(fn, fixed_fn, reps):
    r, best = None, None
    for _ in range(reps):
        r = fn()
        best = r["seconds"] if best is None else min(best, r["seconds"])
    fixed = min(fixed_fn()["seconds"] for _ in range(3))
    return (best - fixed) / max(r["iterations"], 1) * 1e3, r["iterations"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=160)
    ap.add_argument("--rhs", default="1,2,4,8")
    ap.add_argument("--iters", type=int, default=300)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--methods", default="pcg,pbicgstab")
    ap.add_argument("--opts", default="", help="handle options, e.g. sell_window=2")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import spmv_mi355x as eng

    row_ptr, col, val, m = stencil27(args.grid)
    opts = {kv.split("=")[0]: int(kv.split("=")[1]) for kv in args.opts.split(",") if kv}
    M = eng.Matrix(row_ptr, col, val, m, m, "sell_c_sigma", **opts)
    ks = [int(k) for k in args.rhs.split(",")]
    res = {"system": f"stencil27 {args.grid}^3", "rows": m, "nnz": len(col), "format_name": M.format_name, "opts": opts,
           "iters": args.iters, "methods": {}}
    B_all = np.ascontiguousarray(np.stack([np.ones(m) * 2.0 ** j for j in range(max(ks))], axis=1))
    b = B_all[:, 0].copy()
    for method in args.methods.split(","):
        single = getattr(M, method)
        multi = getattr(M, method + "_multi")
        single(row_ptr, col, val, b, 10, history=False)                     # warm-up
        out = {}
        for k in ks:
            B = np.ascontiguousarray(B_all[:, :k])
            multi(row_ptr, col, val, B, 10, history=False)
            s_t, m_t = [], []
            for _ in range(args.reps):                                       # legs alternate
                s_t.append(single(row_ptr, col, val, b, args.iters, history=False))
                m_t.append(multi(row_ptr, col, val, B, args.iters, history=False))
            s_fixed = min(single(row_ptr, col, val, b, 0, history=False)["seconds"] for _ in range(3))
            m_fixed = min(multi(row_ptr, col, val, B, 0, history=False)[0]["seconds"] for _ in range(3))
            its = s_t[-1]["iterations"]
            assert all(r[0]["iterations"] == its for r in m_t), "every column should take the single solver's iterations"
            s_ms = (min(r["seconds"] for r in s_t) - s_fixed) / max(its, 1) * 1e3
            m_ms = (min(r[0]["seconds"] for r in m_t) - m_fixed) / max(its, 1) * 1e3
            out[str(k)] = {"iterations": its, "single_ms_per_iteration": round(s_ms, 5), "multi_ms_per_iteration": round(m_ms, 5),
                           "multi_ms_per_iteration_per_rhs": round(m_ms / k, 5), "per_rhs_ratio": round(m_ms / k / s_ms, 3)}
            print(f"[solver_multi_bench] {args.grid}^3 {M.format_name} {method} k={k}: {out[str(k)]}", file=sys.stderr, flush=True)
        res["methods"][method] = out
    M.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
