#!/usr/bin/env python3
"""The high-precision dual bound of a lockstep batch (``eigval_highprecision=True``): BASELINE config 5 — 64 MaxCut
instances (Gset G1–G9 + 55 seeded G(800, 0.06) graphs), n = 800, rank 10, the batch's own tolerances (exps/batch_test.txt:
ptol = objtol = 0.01).

  (a) the ``solve_lockstep`` wall with ``eigval_highprecision=True`` (and, for scale, with it off);
  (b) the time inside dual bounds during (a): the wall of the ``cabi.batch_dual_obj_hp`` calls where the library has them;
      the sum of the instances' ``dual_time`` otherwise (there every bound runs alone and blocking inside its stepper, so
      the sum is the wall);
  (c) on handles put into the state of each solution: one ``batch_dual_obj_hp`` of 64 against a loop of 64
      ``dual_obj_hp`` (skipped when the loaded library has neither).

The script runs unchanged in a checkout of the commit before the entry points existed (it then reports (a) and (b) alone):
that is how the parent's figures in profiles/r07_batch_dual_hp_time.json were taken, alternating with this commit's in one
session.  Warm up once, then ``--reps`` timed runs; prints one JSON line (and writes it to ``--out``).

    python scripts/batch_dual_hp_time.py [--instances 64] [--rank 10] [--reps 3] [--out profiles/x.json] [--commit HASH]
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
    ap.add_argument("--commit", default="", help="hash of the commit this checkout is (recorded)")
    ap.add_argument("--only-batch-call", action="store_true", help="leg (c)'s batched call alone, once (for a kernel trace)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import gen_batch_test
    import run_batch
    names = gen_batch_test.default_graphs(55)[: args.instances]
    graphs = [run_batch.load_graph(g) for g in names]
    abi = sj.load_hip()
    have = bool(getattr(abi, "has_dual_hp", False)) and hasattr(cabi, "batch_dual_obj_hp")
    assert abi.warmup(max(1, min(2 * len(graphs), 256))) == 0
    n = int(graphs[0].shape[0])
    datas = [problems.maxcut_data(A) for A in graphs]
    kw = dict(abi=abi, ptol=1e-2, objtol=1e-2, seed=0, printlevel=0, prior_trace_bound=float(n))
    out = {"instances": len(graphs), "n": n, "r": args.rank, "reps": args.reps, "commit": args.commit,
           "library": abi.version_string(), "has_dual_obj_hp": have}

    inside = []
    if have:
        real = cabi.batch_dual_obj_hp

        def timed(abi_, svs, reqs):
            t0 = time.perf_counter()
            res = real(abi_, svs, reqs)
            inside.append((time.perf_counter() - t0, len(svs), sum(1 for x in res if not isinstance(x, Exception) and x[5] == 1)))
            return res

        cabi.batch_dual_obj_hp = timed

    def solve(**extra):
        del inside[:]
        t0 = time.perf_counter()
        res = batch.solve_lockstep(datas, args.rank, **kw, **extra)
        wall = time.perf_counter() - t0
        assert not any(isinstance(x, Exception) for x in res)
        return wall, res

    if not args.only_batch_call:
        solve(eigval_highprecision=True)      # warm-up
        walls, ins, walls_off = [], [], []
        for _ in range(args.reps):
            w, res = solve(eigval_highprecision=True)
            walls.append(w)
            ins.append(sum(x[0] for x in inside) if have else float(sum(x["dual_time"] for x in res)))
            if have:
                out["dual_hp_calls"] = len(inside)
                out["dual_hp_items"] = int(sum(x[1] for x in inside))
                out["dual_hp_items_shared_route"] = int(sum(x[2] for x in inside))
            out["major_iterations"] = [int(x["majoriter"]) for x in res]
            walls_off.append(solve()[0])
        out["lockstep_wall_hp_s"] = statistics.median(walls)
        out["lockstep_wall_hp_all_s"] = [round(x, 6) for x in walls]
        out["inside_dual_bounds_s"] = statistics.median(ins)
        out["inside_dual_bounds_all_s"] = [round(x, 6) for x in ins]
        out["lockstep_wall_default_s"] = statistics.median(walls_off)
        out["lockstep_wall_default_all_s"] = [round(x, 6) for x in walls_off]
    if have:
        cabi.batch_dual_obj_hp = real
        sols = solve()[1]
        cfg = sj.BurerMonteiroConfig(seed=0, printlevel=0)
        hs = [sj.build_solver(abi, d, args.rank, cfg) for d in datas]
        normb = float(np.sqrt(n))
        for s, d, x in zip(hs, datas, sols):    # the solution's R, λ and σ, primal_vio_raw current
            s.set_factor(cabi.F_RT, x["Rt"])
            s.λ = np.asarray(x["lambda"])[:s.m]
            s.σ = float(x["sigma"])
            s.fg(d.normC(), normb)
        rng = np.random.Generator(np.random.PCG64(5))
        reqs = [(float(n), min(100, n), 1e-6, 100000, rng.standard_normal(n)) for _ in hs]

        def loop():
            return [s.dual_obj_hp(*q) for s, q in zip(hs, reqs)]

        def one_call():
            res = cabi.batch_dual_obj_hp(abi, hs, reqs)
            assert not any(isinstance(x, Exception) for x in res)
            return res

        b = one_call()
        out["routes"] = {"shared": int(sum(x[5] == 1 for x in b)), "single": int(sum(x[5] == 0 for x in b))}
        out["batch_matvecs"] = [int(x[2]) for x in b]
        if not args.only_batch_call:
            a = loop()
            out["loop_matvecs"] = [int(x[2]) for x in a]
            out["max_abs_diff_mineig"] = float(max(abs(x[1] - y[1]) for x, y in zip(a, b)))
            out["max_abs_diff_dual_value"] = float(max(abs(x[0] - y[0]) for x, y in zip(a, b)))
            tl, tb = [], []
            for _ in range(args.reps):
                t0 = time.perf_counter(); loop(); tl.append(time.perf_counter() - t0)
                t0 = time.perf_counter(); one_call(); tb.append(time.perf_counter() - t0)
            out["loop_s"], out["batch_s"] = statistics.median(tl), statistics.median(tb)
            out["loop_all_s"], out["batch_all_s"] = [round(x, 6) for x in tl], [round(x, 6) for x in tb]
            out["ratio_loop_over_batch"] = out["loop_s"] / out["batch_s"]
        for s in hs:
            s.close()
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
