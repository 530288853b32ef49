"""The Armijo backtracking (src/linesearch.jl:139-191) and the inequality step of the HIP library against a reference above
FP64 (helpers.armijo_hp; the CPU oracle is held to the same bounds in tests/test_armijo_reference.py).

States.  armijo_cases.SIZES × ARMIJO_T: linesearch_armijo(α_max) on states set through set_vec / set_scalar (helpers.armijo_state:
a Laplacian cost, one equality row and m − 1 single-entry inequality rows; λ_ub = +∞, 0, ½ and 1½ times λ − σv, and a block of
rows that cross the cap between two trial steps; D = t·(−G) with t from the recorded table; α_max ∈ {1e-3, 1, 4}).  Per state:
A_RD and A_DD termwise against A_pair_hp; the device's k from α = α_max/2^k bit for bit; ℒ against L[k] of armijo_hp on the
handle's own A_RD, A_DD to c·u·T[k], c = linesearch_c(m); the decision rule with τ[k] = c·u·(T0 + T[k] + 1e-4·α_k·T_slope) —
every k below the device's has margin < τ, and the device's own k is 50 or has margin ≥ −τ; on a decided state (|margin| > 10·τ
for every k ≤ k_hp) α = α_max/2^k_hp with no tolerance; the commit (helpers.commit_check).

Measured on an MI355X (bound = 1), worst error/bound per size over its states; no state undecided at any size (0/11 … 0/5), α
bit for bit on every one:
    (n, m, r)          A_RD    A_DD    ℒ        commit
    (12, 1, 3)         0.030   0.0036  0.019    0.17
    (16, 2, 3)         0.083   0.086   0.0094   0.18
    (16, 63, 3)        0.16    0.33    0.020    0.29
    (16, 64, 33)       0.030   0.039   0.019    0.26
    (16, 65, 1)        0.25    0.25    0.078    0.25
    (24, 255, 3)       0.26    0.25    0.064    0.42
    (24, 256, 1)       0.28    0.26    0.012    0.24
    (24, 257, 33)      0.024   0.046   0.020    0.36
    (48, 511, 3)       0.22    0.27    0.0021   0.32
    (48, 513, 1)       0.28    0.27    0.0028   0.32
    (48, 1025, 33)     0.022   0.054   0.0084   0.39
    (363, 65600, 2)    0.37    0.40    0.0065   0.54
Exhaustion (D = +G, m ∈ {1, 65, 256, 257}): all 50 rejections decided, k = 50, ℒ ≤ 0.014, commit ≤ 0.24.  Caps (y, fused y, λ at
m ∈ {1, 255, 256, 257, 1025}): free side ≤ 0.50 of 2u·(|λ| + σ|v|), a third of the rows capped, each λ_ub exactly.  One loop
iteration, every route: ineq_0.05 k = 15, 𝒜 0.13, ℒ 0.0047, commit 0.21, fused y 0.41, G ≤ 0.032; builder m = 257 k = 11, 𝒜 0.26,
ℒ 0.0032, commit 0.28, fused y 0.49, G 0.11; both decided.

Inside the loops (test_armijo_through_one_iteration): one iteration on a cleared history through inner_loop(use_armijo = 1)
on the eager, graph, NO_FAST, NO_UPDFUSE, DOT_DESCENT and NO_LRFUSE routes, on ineq_0.05 at n = 12 (the structured fast route,
whose step kernel rebuilds G from P and W under the caps) and on the m = 257 builder instance (generic): dirt, (α, ℒ) by the
rule above with D = −G of the handle's own G, R to 1 ulp, the commit, the fused y on both sides of the cap, and the new G
against S_and_G_hp through fg_cases.check_g_state.  The graph route replays a batch of two iterations (the library captures graphs
from a budget of four iterations on) whose first ends the loop (fprec_eps = +∞: the relative-decrease exit), so that the state
after the first iteration is what is read.
"""
import numpy as np
import pytest

import armijo_cases as ac
import fg_cases as fc
from sdplrplus_jl_amd import cabi
from helpers import (ARMIJO_K, LD, U53, A_pair_hp, _ld, armijo_base, armijo_decision_ok, armijo_hp, armijo_k_of, armijo_state,
                     assert_route, check_armijo_call, commit_check, device_pattern, fg_hp, make_data, make_solver, set_route,
                     worst_ratio)

pytestmark = pytest.mark.gpu

@pytest.mark.parametrize("size", ac.SIZES, ids=lambda s: f"n{s[0]}-m{s[1]}-r{s[2]}")
def test_armijo_states(hip_abi, size):
    out = ac.run_size(hip_abi, size)
    ac.report("hip", size, out)
    assert not out["bad"], (len(out["bad"]), out["bad"][:6])
    assert 10 * len(out["undecided"]) <= out["n"], out["undecided"]


@pytest.mark.parametrize("size", [(12, 1, 3), (16, 65, 1), (24, 256, 1), (24, 257, 33)], ids=lambda s: f"n{s[0]}-m{s[1]}-r{s[2]}")
def test_armijo_exhausted_and_tie(hip_abi, size):
    """D = +G: every trial step whose margin exceeds its round-off is rejected (asserted above FP64 on the CPU), so the device's k
    is one allowed by the rule — at the first margin inside its round-off at the earliest, else 50, α_max/2⁵⁰ — ℒ is the value at
    that α and the commit is done with it; the call returns no error and the handle goes on working (done and err are not left
    set: the next f! runs).  D = 0: α = α_max at once and pv_raw unchanged bit for bit."""
    base = armijo_base(*size)
    s_, _ = make_solver(hip_abi, base["data"], size[2], seed=5, h=4)
    st = armijo_state(base, 1.0, 1.0, "ascent")
    res = check_armijo_call(base, st, s_)
    ref = res["ref"]
    big = np.flatnonzero(np.abs(ref["margin"][:ARMIJO_K]) > ref["tau"][:ARMIJO_K])
    assert big.size and np.all(ref["margin"][big] < 0)
    print(f"armijo exhaustion m={size[1]}: k {res['k_dev']} (last decided rejection {int(big[-1])}) L {res['L']:.3g} commit {res['commit']:.3g}")
    assert res["on_grid"] and res["decision_ok"] and res["k_dev"] > int(big[-1]), (res["k_dev"], big)
    assert res["obj_is_last"] and res["pv_is_raw"] and all(res[k] <= 1.0 for k in ac.RATIOS), res
    s_.Rt = st["R"]
    assert np.isfinite(s_.f())
    tie = armijo_state(base, 0.0, 4.0, "tie")
    res = check_armijo_call(base, tie, s_)
    assert res["alpha"] == 4.0 and res["k_dev"] == 0 and np.array_equal(s_.primal_vio_raw, tie["pv_raw"]), res
    assert res["L"] <= 1.0 and res["obj_is_last"] and res["pv_is_raw"]
    s_.close()


def cap_sides(got, lam, ub, v, sigma):
    """min(λ_ub, λ − σv) on both sides of the cap: `got` must be λ_ub exactly wherever the long-double λ − σv exceeds λ_ub by more
    than 2u·(|λ| + σ|v|), and within that bound of λ − σv wherever it is below λ_ub by more; in between either.  (The compiler
    may contract λ − σv to an FMA: no bits asserted on the free side.)  → (worst error/bound on the free side, rows capped)."""
    lam_, ub_, v_, sg = _ld(lam), _ld(ub), _ld(v), LD(sigma)
    free = lam_ - sg * v_
    bound = 2 * LD(U53) * (np.abs(lam_) + sg * np.abs(v_))
    capped, below = np.asarray(free - ub_ > bound), np.asarray(ub_ - free > bound)
    g = _ld(got)
    assert np.array_equal(np.asarray(got)[capped], np.asarray(ub)[capped]), "a capped row is not λ_ub exactly"
    mid = ~capped & ~below
    assert np.all((g[mid] == ub_[mid]) | (np.abs(g[mid] - free[mid]) <= bound[mid]))
    return worst_ratio(g[below], free[below], bound[below]), int(capped.sum())


@pytest.mark.parametrize("n,m", [(12, 1), (24, 255), (24, 256), (24, 257), (48, 1025)])
def test_update_lambda_with_caps(hip_abi, monkeypatch, n, m):
    """y after g!, λ after update_lambda() and the y the commit fuses for the next g! (one Armijo iteration of the loop), each
    from the handle's own primal_vio_raw, across the block boundaries of the m-sized kernels with caps that bind on some rows."""
    set_route(monkeypatch, "eager")
    base = armijo_base(n, m, 3)
    s_, _ = make_solver(hip_abi, base["data"], 3, seed=5, h=4)
    s_.Rt, s_.λ_ub, s_.λ, s_.σ = base["R"], base["ub"], base["lam"], base["sigma"]
    nC, nb = base["data"].normC(), float(np.linalg.norm(base["bs"]))
    st = s_.fg(nC, nb)
    v = s_.primal_vio_raw[:m]
    ry, ncap = cap_sides(-s_.y[:m], base["lam"], base["ub"], v, base["sigma"])
    assert m == 1 or 0 < ncap < m - 1
    out = s_.inner_loop(nC, nb, True, True, 1, 0.0, -1e300, 1, 0.0, *st)
    assert out[4] == 1 and out[3] != 0.0
    v = s_.primal_vio_raw[:m]
    rf, _ = cap_sides(-s_.y[:m], base["lam"], base["ub"], v, base["sigma"])
    assert s_.y[m] == 1.0
    s_.update_lambda()
    rl, ncap2 = cap_sides(s_.λ, base["lam"], base["ub"], v, base["sigma"])
    print(f"caps m={m}: error/bound y {ry:.3g} fused y {rf:.3g} lambda {rl:.3g}; capped rows {ncap}, {ncap2}")
    assert ry <= 1.0 and rf <= 1.0 and rl <= 1.0
    s_.close()


# ---- Armijo inside the loops --------------------------------------------------------------------------------------------------
STEP_ROUTES = ["eager", "no_fast", "no_updfuse", "dot_descent", "no_lrfuse", "graph"]
_INST = {}


def _instance(name):
    """(data, C, As, pattern, split, r, expected loop kind per route) — ineq_0.05 at n = 12 is the structured fast route unless
    NO_FAST; the builder at m = 257 has general rows: generic on every route."""
    if name not in _INST:
        if name == "ineq_0.05":
            data, C, As, bs = make_data("ineq_0.05", 2, 12, 0.4)
            _INST[name] = dict(data=data, C=C, As=As, bs=bs, pattern=device_pattern(C, As), split=None, r=3, fast=True)
        else:
            b = armijo_base(24, 257, 3)
            _INST[name] = dict(data=b["data"], C=b["C"], As=b["As"], bs=b["bs"], pattern=b["pattern"], split=b["split"], r=3, fast=False)
    return _INST[name]


def _loop_kind(hip_abi, inst, lam, ub, nC, nb):
    """The scope names a twin handle under profile_enable() reports for the same one-iteration loop."""
    t, _ = make_solver(hip_abi, inst["data"], inst["r"], seed=11, h=4)
    t.λ_ub, t.λ = ub, lam
    t.profile_enable()
    t.inner_loop(nC, nb, True, True, 1, 0.0, -1e300, 1, 0.0, *t.fg(nC, nb))
    names = set(t.profile())
    t.close()
    return names


@pytest.mark.parametrize("route", STEP_ROUTES)
@pytest.mark.parametrize("name", ["ineq_0.05", "builder257"])
def test_armijo_through_one_iteration(hip_abi, monkeypatch, name, route):
    inst = _instance(name)
    data, C, As, r = inst["data"], inst["C"], inst["As"], inst["r"]
    m = data.m
    set_route(monkeypatch, route)
    s_, _ = make_solver(hip_abi, data, r, seed=11, h=4)
    nC, nb = data.normC(), float(np.linalg.norm(data.b))
    # a seeded λ ≤ 0 on the inequality rows, and caps by the recipe of fg_cases from the violation at the start point
    rng = np.random.Generator(np.random.PCG64(61))
    lam = 0.1 * rng.standard_normal(m)
    ct = np.asarray(data.constraint_types, dtype=bool)
    R0 = s_.Rt
    free = np.asarray(fg_hp(C, As, inst["bs"], R0, lam, np.full(m, np.inf), 2.0)["yt"], dtype=np.float64)
    ub = np.full(m, np.inf)
    q = np.flatnonzero(ct)
    ub[q] = 0.0
    ub[q[1::4]] = 0.5 * free[q[1::4]]
    ub[q[3::4]] = 1.5 * free[q[3::4]]
    with np.errstate(invalid="ignore"):
        lam = np.where(lam > ub, ub - np.abs(ub) - 0.01, lam)
    s_.λ_ub, s_.λ = ub, lam
    st = s_.fg(nC, nb)
    G0, pv0, obj0, y0 = s_.Gt, s_.primal_vio_raw, s_.obj, s_.y
    graph = route == "graph"
    out = s_.inner_loop(nC, nb, True, True, 1, 0.0, 1e300 if graph else -1e300, 4 if graph else 1, 0.0, *st)
    assert out[4] == 1 and out[5] == (1 if graph else 2), out
    stats = s_.stats()
    assert_route(route, name, r, 4, stats, armijo=True)
    L, alpha = out[0], out[3]
    D = -G0
    # (the relative-decrease exit leaves dirt unscaled: no lbfgs_update! before it)
    assert alpha != 0.0 and np.array_equal(s_.dirt, D if graph else alpha * D)
    ard, add = s_.A_RD, s_.A_DD
    a1, a2 = A_pair_hp(C, As, R0, D, inst["split"]), A_pair_hp(C, As, D, D, inst["split"])
    rA = max(worst_ratio(ard, 2 * a1["q"], a1["depth"] * LD(U53) * 2 * a1["mag"]), worst_ratio(add, a2["q"], a2["depth"] * LD(U53) * a2["mag"]))
    ref = armijo_hp(pv0, obj0, lam, ub, y0, 2.0, 1.0, ard, add)
    k = armijo_k_of(alpha, 1.0)
    assert k is not None and armijo_decision_ok(ref, k), (alpha, k, ref["k_hp"])
    if ref["decided"]:
        assert k == ref["k_hp"]
    rL = worst_ratio([L], [ref["L"][k]], [ref["c"] * LD(U53) * ref["T"][k]])
    R1 = s_.Rt
    assert np.all(np.abs(R1 - (R0 + alpha * D)) <= np.spacing(np.abs(R1)))
    cm = commit_check(s_, pv0, alpha, m)
    assert cm["obj_is_last"] and cm["pv_is_raw"]
    y1 = s_.y
    assert y1[m] == 1.0
    rY, ncap = cap_sides(-y1[:m], lam, ub, s_.primal_vio_raw[:m], 2.0)
    worst = dict(S=0.0, G=0.0)
    fc.check_g_state(dict(C=C, As=As, pattern=inst["pattern"]), dict(R=R1), y1, None, None, s_.Gt, worst, big=True)
    print(f"armijo loop step {name} {route}: k {k} (decided {ref['decided']}) error/bound A {rA:.3g} L {rL:.3g} commit {cm['commit']:.3g} "
          f"fused y {rY:.3g} G {worst['G']:.3g}; capped rows {ncap}")
    assert rA <= 1.0 and rL <= 1.0 and cm["commit"] <= 1.0 and rY <= 1.0 and worst["G"] <= 1.0
    s_.close()
    if route in ("eager", "no_fast"):
        names = _loop_kind(hip_abi, inst, lam, ub, nC, nb)
        assert {"armijo_partials", "armijo_pick", "ls_commit"} <= names, sorted(names)
        assert ("fast_step" in names) == (inst["fast"] and route != "no_fast"), (name, route, sorted(names))


def test_batch_call_with_inequalities_runs_per_instance(hip_abi, monkeypatch):
    """sdplr_hip_batch_major_iteration with inequality data: neither the resident loop nor the group launch takes an Armijo
    loop, so every item falls back to its own call — and gives that call's result bit for bit."""
    set_route(monkeypatch, "resident_batch")
    datas = [make_data("ineq_0.05", s, 12, 0.4)[0] for s in (2, 3, 4)]
    S = [make_solver(hip_abi, d, 3, seed=11, h=4)[0] for d in datas]
    T = [make_solver(hip_abi, d, 3, seed=11, h=4)[0] for d in datas]
    norms = [(d.normC(), float(np.linalg.norm(d.b))) for d in datas]
    res = cabi.batch_major_iteration(hip_abi, S, [(nc, nb, 1, 1, 1, 0, 2.0, 0.0, -1e300, 3, 0.0) for nc, nb in norms])
    for s_, t_, o, (nc, nb) in zip(S, T, res, norms):
        assert not isinstance(o, Exception), o
        st = s_.stats()
        assert st["resident_loops"] == 0 and st["group_launch_loops"] == 0 and st["resident_shared_launches"] == 0, st
        one = t_.major_iteration(nc, nb, True, True, 1, 0, 2.0, 0.0, -1e300, 3, 0.0)
        assert tuple(o[:6]) == tuple(one[:6]) and o[4] == 3 and np.array_equal(s_.Rt, t_.Rt)
        s_.close(); t_.close()
