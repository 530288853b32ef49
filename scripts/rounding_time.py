#!/usr/bin/env python3
"""Randomized rounding, host against device (exps/test.jl:71-105): both modes at n = 1e5, G(n, 2e-4), r = 32, 100 trials.
The host side is rounding.py on a factor fetched with get_factor (the download is part of its time); the device side is
one sdplr_hip_round call including its Γ upload and cuts download, with the graph upload (once per instance) and the
whole ``*_device`` callback timed beside it, and the per-kernel device times of one profiled call.  Prints one JSON line.

    python scripts/rounding_time.py [--n 100000] [--p 2e-4] [--rank 32] [--trials 100] [--reps 5]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import sdplrplus_jl_amd as sj  # noqa: E402
from sdplrplus_jl_amd import cabi, problems, rounding  # noqa: E402


def best_of(reps, fn):
    out, ts = None, []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        ts.append(time.perf_counter() - t0)
    return out, min(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100000)
    ap.add_argument("--p", type=float, default=2e-4)
    ap.add_argument("--rank", type=int, default=32)
    ap.add_argument("--trials", type=int, default=100)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-reps", type=int, default=1)
    args = ap.parse_args()
    A = problems.gnp_graph(args.n, args.p, 1)
    data = problems.maxcut_data(A)
    var = sj.build_solver(sj.load_hip(), data, args.rank, sj.BurerMonteiroConfig(seed=0, printlevel=0))
    rng = np.random.Generator(np.random.PCG64(5))
    R = rng.standard_normal((args.n, args.rank))
    var.set_factor(cabi.F_RT, R / np.linalg.norm(R, axis=1, keepdims=True))
    mk = lambda: np.random.Generator(np.random.PCG64(9))
    out = {"n": args.n, "edges": int(A.nnz // 2), "r": args.rank, "trials": args.trials}
    _, out["graph_upload_s"] = best_of(args.reps, lambda: var.round_set_graph(A))
    for name, mode, host_fn, dev_fn in (("maxcut", 0, rounding.maxcut_rounding, rounding.maxcut_rounding_device),
                                        ("bisection", 1, rounding.minimumbisection_rounding,
                                         rounding.minimumbisection_rounding_device)):
        hv, ht = best_of(args.host_reps, lambda: host_fn(A, var.get_factor(cabi.F_RT), mk(), args.trials))

        def call():
            g = mk()
            gauss = np.stack([g.standard_normal(args.rank) for _ in range(args.trials)])
            cuts, best, _, _ = var.round(mode, args.trials, gauss)
            return float(cuts[best])

        call()                                                   # (first call: the work arrays are allocated)
        dv, dt = best_of(args.reps, call)
        _, ct = best_of(args.reps, lambda: dev_fn(var, A, mk(), args.trials))
        var.profile_enable(True)
        call()
        prof = {k: round(v[1], 4) for k, v in var.profile().items() if k.startswith("round_")}
        var.profile_enable(False)
        out[name] = {"host_s": ht, "device_call_s": dt, "device_callback_s": ct, "speedup": ht / dt, "host_value": hv,
                     "device_value": dv, "kernel_ms": prof}
    var.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
