#!/usr/bin/env python3
"""One sdplr_hip_batch_round against the loop of sdplr_hip_round calls it replaces, on the BASELINE config 5 shape: 64 MaxCut
and 64 MinimumBisection instances (Gset G1–G9 + 55 seeded G(800, 0.06) graphs), n = 800, r = 10, 100 trials.  The factors
are random — the rounding's cost does not depend on the solution.  Graphs are set and Γ is drawn before the clock starts;
each timed call includes its uploads, launches, downloads and waits.  Warm up once, then best of ``--reps``, the two sides
interleaved.  The config-5 lockstep wall (64 MaxCut solves, second pass) is measured in the same process for the share.
Prints one JSON line (and writes it to ``--out``).

    python scripts/batch_rounding_time.py [--instances 64] [--rank 10] [--trials 100] [--reps 5] [--out profiles/x.json]
"""
import argparse
import json
import os
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
    ap.add_argument("--trials", type=int, default=100)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-solve", action="store_true", help="skip the config-5 lockstep wall")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import gen_batch_test
    import run_batch
    names = gen_batch_test.default_graphs(55)[: args.instances]
    graphs = [run_batch.load_graph(g) for g in names]
    abi = sj.load_hip()
    assert abi.warmup(max(1, min(2 * len(graphs), 256))) == 0
    cfg = sj.BurerMonteiroConfig(seed=0, printlevel=0)
    rng = np.random.Generator(np.random.PCG64(5))
    out = {"instances": len(graphs), "n": int(graphs[0].shape[0]), "r": args.rank, "trials": args.trials, "reps": args.reps}
    sets = {}
    for name, mode, build in (("maxcut", 0, problems.maxcut_data), ("bisection", 1, problems.minimum_bisection_data)):
        hs = [sj.build_solver(abi, build(A), args.rank, cfg) for A in graphs]
        for s, A in zip(hs, graphs):
            R = rng.standard_normal((s.n, args.rank))
            s.set_factor(cabi.F_RT, R / np.linalg.norm(R, axis=1, keepdims=True))
            s.round_set_graph(A)
        sets[name] = (hs, [(mode, args.trials, rng.standard_normal((args.trials, args.rank))) for _ in hs])

    def loop(hs, reqs):
        return [s.round(*q)[0] for s, q in zip(hs, reqs)]

    def one_call(hs, reqs):
        res = cabi.batch_round(abi, hs, reqs)
        assert all(x[4] == 1 for x in res)
        return [x[0] for x in res]

    both = (sets["maxcut"][0] + sets["bisection"][0], sets["maxcut"][1] + sets["bisection"][1])
    for name, (hs, reqs) in list(sets.items()) + [("both", both)]:
        a, b = loop(hs, reqs), one_call(hs, reqs)                    # warm-up: work arrays, the kernel's first launch
        assert all(np.array_equal(x, y) for x, y in zip(a, b)), name  # the same bits
        tl, tb = [], []
        for _ in range(args.reps):
            t0 = time.perf_counter(); loop(hs, reqs); tl.append(time.perf_counter() - t0)
            t0 = time.perf_counter(); one_call(hs, reqs); tb.append(time.perf_counter() - t0)
        out[name] = {"items": len(hs), "loop_s": min(tl), "batch_s": min(tb), "loop_all_s": [round(x, 6) for x in tl],
                     "batch_all_s": [round(x, 6) for x in tb], "ratio": min(tl) / min(tb)}
    for hs, _ in sets.values():
        for s in hs:
            s.close()
    if not args.no_solve:
        datas = [problems.maxcut_data(A) for A in graphs]
        kw = dict(abi=abi, ptol=1e-2, objtol=1e-2, seed=0, printlevel=0, prior_trace_bound=float(out["n"]))
        walls = []
        for _ in range(2):
            t0 = time.perf_counter()
            res = batch.solve_lockstep(datas, args.rank, **kw)
            walls.append(time.perf_counter() - t0)
            assert not any(isinstance(x, Exception) for x in res)
        out["lockstep_wall_s"] = walls[-1]
        for name in ("maxcut", "bisection"):
            out[name]["loop_share_of_wall"] = out[name]["loop_s"] / walls[-1]
            out[name]["batch_share_of_wall"] = out[name]["batch_s"] / walls[-1]
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
