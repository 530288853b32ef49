#!/usr/bin/env python3
"""Records tests/golden/dual_hp_oracle_parent.json: what ``sdplr(data=…, abi=<CPU oracle>, eigval_highprecision=True)``
returns on the commit BEFORE the high-precision dual bound became a request of ``sdplr_steps`` (REQ_DUAL_HP).  The
fallback of ``serve`` for an ABI without ``dual_obj_hp`` is that commit's host sequence moved, so
tests/test_dual_hp_steps.py asks for equality with these values.

Run once, at that commit:  python scripts/record_dual_hp_parent.py
The instances and arguments below are the ones the test uses (``CASES``, ``KW``); floats are stored as hex strings."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import sdplrplus_jl_amd as sj                      # noqa: E402
from sdplrplus_jl_amd import problems              # noqa: E402
from oracle import oracle                          # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "dual_hp_oracle_parent.json")
KW = dict(seed=2, printlevel=0, ptol=1e-3, objtol=1e-3, prior_trace_bound=40.0, eigval_highprecision=True)
CASES = [("maxcut", 11), ("maxcut", 12), ("minimum_bisection", 11), ("minimum_bisection", 12)]
R = 4


def data_of(problem: str, seed: int):
    A = problems.gnp_graph(40, 0.2, seed)
    return problems.maxcut_data(A) if problem == "maxcut" else problems.minimum_bisection_data(A)


def main():
    oracle.build()
    abi = oracle.abi()
    rec = []
    for problem, seed in CASES:
        ans = sj.sdplr(data=data_of(problem, seed), r=R, abi=abi, **KW)
        rec.append({"problem": problem, "graph_seed": seed, "obj": float(ans["obj"]).hex(),
                    "max_dual_value": float(ans["max_dual_value"]).hex(), "iter": int(ans["iter"]),
                    "majoriter": int(ans["majoriter"]), "lambda": [float(x).hex() for x in ans["lambda"]]})
        print(problem, seed, ans["obj"], ans["max_dual_value"], ans["iter"], ans["majoriter"])
    with open(OUT, "w") as f:
        json.dump({"r": R, "n": 40, "p": 0.2, "kw": {k: v for k, v in KW.items()}, "cases": rec}, f, indent=1)
        f.write("\n")
    print("wrote", OUT)


if __name__ == "__main__":
    main()
