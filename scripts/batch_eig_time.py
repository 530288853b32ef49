#!/usr/bin/env python3
"""The eigenvalue certificate of a batch: one sdplr_hip_batch_S_eigval against the loop of sdplr_hip_S_eigval calls it
replaces, on the BASELINE config 5 batch — 64 MaxCut instances (Gset G1–G9 + 55 seeded G(800, 0.06) graphs), n = 800,
rank 10, solved with the batch's own tolerances (exps/batch_test.txt: ptol = objtol = 0.01), the eigensolve with
DIMACS_errors' own arguments (nev = 1, SA, ncv = 100, tol = 0, no start vector) on S = C − Diag(λ) of each solution.

  (a) the 64 eigensolves as a loop of sdplr_hip_S_eigval;
  (b) one sdplr_hip_batch_S_eigval (skipped, with its results, when the loaded library has no such symbol: pointing
      SDPLR_HIP_LIBRARY at a build of the parent commit makes (a) the parent's code, not a switch in the code under test);
  (c) the solve_lockstep wall with eval_DIMACS_errs off and on, and the share of err6 / 𝒜ᵀ preprocessing in the certificate.

Warm up once, then the median of ``--reps``, (a) and (b) interleaved.  Prints one JSON line (and writes it to ``--out``).

    python scripts/batch_eig_time.py [--instances 64] [--rank 10] [--reps 3] [--out profiles/x.json] [--commit HASH]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import sdplrplus_jl_amd as sj  # noqa: E402
from sdplrplus_jl_amd import batch, cabi, problems  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--instances", type=int, default=64)
    ap.add_argument("--rank", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-solve", action="store_true", help="skip leg (c)")
    ap.add_argument("--commit", default="", help="hash of the commit the loaded library was built from (recorded)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import gen_batch_test
    import run_batch
    names = gen_batch_test.default_graphs(55)[: args.instances]
    graphs = [run_batch.load_graph(g) for g in names]
    abi = sj.load_hip()
    have = bool(getattr(abi, "has_eig_batch", False)) and hasattr(cabi, "batch_S_eigval")
    assert abi.warmup(max(1, min(2 * len(graphs), 256))) == 0
    n = int(graphs[0].shape[0])
    datas = [problems.maxcut_data(A) for A in graphs]
    kw = dict(abi=abi, ptol=1e-2, objtol=1e-2, seed=0, printlevel=0, prior_trace_bound=float(n))
    out = {"instances": len(graphs), "n": n, "r": args.rank, "reps": args.reps, "commit": args.commit,
           "library": abi.version_string(), "has_batch_S_eigval": have,
           "cycles_per_launch": int(os.environ.get("SDPLR_HIP_BATCH_EIG_CYCLES", "8")) if have else None}
    sols = batch.solve_lockstep(datas, args.rank, **kw)
    assert not any(isinstance(x, Exception) for x in sols)
    cfg = sj.BurerMonteiroConfig(seed=0, printlevel=0)
    hs = [sj.build_solver(abi, d, args.rank, cfg) for d in datas]
    for s, x in zip(hs, sols):         # S = C − Diag(λ) of the solution, as DIMACS_errors sets it (src/coreop.jl:434-436)
        s.set_factor(cabi.F_RT, x["Rt"])
        s.y = np.concatenate([-np.asarray(x["lambda"])[:s.m], [1.0]])   # (the result's λ is −y: m + 1 long)
        s.At_preprocess()
    req = (1, "SA", min(100, n), 0.0, 100000, None)

    def loop():
        return [s.S_eigval(*req) for s in hs]

    def one_call():
        res = cabi.batch_S_eigval(abi, hs, [req] * len(hs))
        assert not any(isinstance(x, Exception) for x in res)
        return res

    a = loop()
    out["loop_matvecs"] = [int(x[1]) for x in a]
    out["loop_converged"] = int(sum(x[2] for x in a))
    if have:
        b = one_call()
        out["routes"] = {"shared": int(sum(x[3] == 1 for x in b)), "single": int(sum(x[3] == 0 for x in b))}
        out["batch_matvecs"] = [int(x[1]) for x in b]
        out["batch_converged"] = int(sum(x[2] for x in b))
        out["max_abs_diff"] = float(max(abs(x[0][0] - y[0][0]) for x, y in zip(a, b)))
    tl, tb = [], []
    for _ in range(args.reps):
        t0 = time.perf_counter(); loop(); tl.append(time.perf_counter() - t0)
        if have:
            t0 = time.perf_counter(); one_call(); tb.append(time.perf_counter() - t0)
    out["loop_s"] = statistics.median(tl)
    out["loop_all_s"] = [round(x, 6) for x in tl]
    if have:
        out["batch_s"] = statistics.median(tb)
        out["batch_all_s"] = [round(x, 6) for x in tb]
        out["ratio_loop_over_batch"] = out["loop_s"] / out["batch_s"]
    # what stays per instance inside the certificate: 𝒜ᵀ preprocessing and err6 (one SpMM and one device dot)
    t0 = time.perf_counter()
    for s in hs:
        s.At_preprocess()
        s.At_left(cabi.F_SCRATCH, cabi.F_RT)
        s.factor_dot(cabi.F_RT, cabi.F_SCRATCH)
    out["per_instance_rest_s"] = time.perf_counter() - t0
    for s in hs:
        s.close()
    if not args.no_solve:
        for key, extra in (("lockstep_wall_s", {}), ("lockstep_wall_dimacs_s", {"eval_DIMACS_errs": True})):
            walls = []
            for _ in range(max(2, args.reps)):
                t0 = time.perf_counter()
                res = batch.solve_lockstep(datas, args.rank, **kw, **extra)
                walls.append(time.perf_counter() - t0)
                assert not any(isinstance(x, Exception) for x in res)
            out[key] = statistics.median(walls[1:])
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
