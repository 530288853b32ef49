"""The high-precision dual bound (``eigval_highprecision``, src/coreop.jl:389-400) as a request of ``sdplr_steps``, on the
CPU checker's ABI — which has no ``dual_obj_hp``, so ``serve`` answers with the host sequence the stepper itself ran before
the bound became a request.  The results are therefore compared for EQUALITY with values recorded on the commit before that
change (tests/golden/dual_hp_oracle_parent.json, written by scripts/record_dual_hp_parent.py)."""
import importlib
import json
import os

import numpy as np
import pytest

import sdplrplus_jl_amd as sj
from sdplrplus_jl_amd import batch, problems

sdplr_mod = importlib.import_module("sdplrplus_jl_amd.sdplr")     # (the package exports the function of the same name)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "dual_hp_oracle_parent.json")))
KW = dict(seed=2, printlevel=0, ptol=1e-3, objtol=1e-3, prior_trace_bound=40.0)


def data_of(problem, seed):
    A = problems.gnp_graph(GOLDEN["n"], GOLDEN["p"], seed)
    return problems.maxcut_data(A) if problem == "maxcut" else problems.minimum_bisection_data(A)


def _requests(data, oracle_abi, **kw):
    cfg = sj.BurerMonteiroConfig(**dict(KW, **kw))
    var = sj.build_solver(oracle_abi, data, GOLDEN["r"], cfg)
    steps = sdplr_mod.sdplr_steps(data, var, cfg)
    seen = []
    try:
        req = next(steps)
        while True:
            seen.append(req)
            req = steps.send(sdplr_mod.serve(var, req))
    except StopIteration as done:
        var.close()
        return seen, done.value


def test_every_dual_bound_is_a_dual_hp_request(oracle_abi):
    data = data_of("maxcut", 11)
    seen, ans = _requests(data, oracle_abi, eigval_highprecision=True)
    kinds = [q[0] for q in seen]
    hp = [q for q in seen if q[0] == sdplr_mod.REQ_DUAL_HP]
    assert hp and sdplr_mod.REQ_DUAL not in kinds
    for q in hp:
        assert q[1:5] == (40.0, min(100, data.n), 1e-6, 100000) and np.asarray(q[5]).shape == (data.n,)
    # a dual bound follows every major iteration that met its primal tolerance: as many as the default run's REQ_DUALs up to
    # the point where the two bounds (ARPACK-grade against Lanczos) part ways — at least the first one
    seen0, _ = _requests(data, oracle_abi)
    kinds0 = [q[0] for q in seen0]
    assert sdplr_mod.REQ_DUAL_HP not in kinds0 and sdplr_mod.REQ_DUAL in kinds0
    first = kinds.index(sdplr_mod.REQ_DUAL_HP)
    assert kinds0.index(sdplr_mod.REQ_DUAL) == first and kinds[:first] == kinds0[:first]
    assert ans["max_dual_value"] <= ans["obj"] + 1e-6 * abs(ans["obj"])


@pytest.mark.parametrize("case", GOLDEN["cases"], ids=lambda c: f"{c['problem']}-{c['graph_seed']}")
def test_oracle_results_equal_the_parent_commit(oracle_abi, case):
    assert GOLDEN["kw"] == dict(KW, eigval_highprecision=True)
    ans = sj.sdplr(data=data_of(case["problem"], case["graph_seed"]), r=GOLDEN["r"], abi=oracle_abi,
                   eigval_highprecision=True, **KW)
    assert ans["iter"] == case["iter"] and ans["majoriter"] == case["majoriter"]
    assert float(ans["obj"]) == float.fromhex(case["obj"])
    assert float(ans["max_dual_value"]) == float.fromhex(case["max_dual_value"])
    assert np.array_equal(ans["lambda"], np.array([float.fromhex(x) for x in case["lambda"]]))


def test_lockstep_without_the_entry_point_is_one_by_one(oracle_abi, monkeypatch):
    assert not oracle_abi.has_dual_hp
    called = []
    monkeypatch.setattr(batch.cabi, "batch_dual_obj_hp", lambda *a: called.append(a) or [])
    cases = GOLDEN["cases"][:1] + GOLDEN["cases"][2:3]
    datas = [data_of(c["problem"], c["graph_seed"]) for c in cases]
    lock = batch.solve_lockstep(datas, GOLDEN["r"], abi=oracle_abi, eigval_highprecision=True, **KW)
    assert not called
    for c, d, b in zip(cases, datas, lock):
        a = sj.sdplr(data=d, r=GOLDEN["r"], abi=oracle_abi, eigval_highprecision=True, **KW)
        for key in ("obj", "max_dual_value", "iter", "majoriter"):
            assert a[key] == b[key], key
        assert np.array_equal(a["lambda"], b["lambda"]) and np.array_equal(a["Rt"], b["Rt"])
        assert b["iter"] == c["iter"] and float(b["max_dual_value"]) == float.fromhex(c["max_dual_value"])
