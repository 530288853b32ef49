"""The reference side of tests/test_gpu_armijo.py, without a GPU: the Armijo backtracking of src/linesearch.jl:139-191 restated
above FP64 (helpers.armijo_hp), the claims of the state generator (helpers.armijo_state, armijo_cases.ARMIJO_T) asserted on
that restatement, and the CPU oracle — a plain FP64 implementation that shares no code with the HIP kernels — held to the very
bounds the GPU module asks of the HIP library.  That the oracle meets them shows they are attainable in FP64.
"""
import numpy as np
import pytest

import armijo_cases as ac
from helpers import (ARMIJO_K, LD, U53, armijo_base, armijo_hp, armijo_state, armijo_state_ref, check_armijo_call, crossings,
                     lagrangian_dense, make_solver)


def test_armijo_hp_is_the_lagrangian_along_the_line():
    """L[k] of armijo_hp is ℒ(R + α_k·D) of src/coreop.jl:6-9 formed from dense matrices at the moved point, L0 that at R, and the
    slope that of :171: the restatement is the function it claims."""
    base = armijo_base(16, 63, 3)
    st = armijo_state(base, 2.0 ** -10, 1.0)
    ref = armijo_state_ref(st)
    C, As, bs = base["C"], base["As"], base["bs"]
    for k in (0, 1, 5):
        a = ref["alpha"][k]
        want = lagrangian_dense(C, As, bs, st["R"] + a * st["D"], st["lam"], st["ub"], st["sigma"])
        assert abs(float(ref["L"][k]) - want) <= 1e-11 * float(ref["T"][k]), k
    assert abs(float(ref["L0"]) - lagrangian_dense(C, As, bs, st["R"], st["lam"], st["ub"], st["sigma"])) <= 1e-11 * float(ref["T0"])
    # the slope of :171 takes y·A_RD over EVERY row; ∂ℒ/∂α at 0 has no term from a row on which the cap wins (λ̃ = λ_ub is
    # constant there).  The two agree where such rows have λ_ub = 0, as the solver sets it; with other caps the reference's
    # slope is what is restated — the difference quotient is compared with the sum over the free rows
    h = 2.0 ** -26
    fd = (lagrangian_dense(C, As, bs, st["R"] + h * st["D"], st["lam"], st["ub"], st["sigma"])
          - lagrangian_dense(C, As, bs, st["R"] - h * st["D"], st["lam"], st["ub"], st["sigma"])) / (2 * h)
    m, ard = base["m"], np.asarray(2 * st["a1"]["q"], dtype=np.float64)
    free = ~ref["capped0"]
    assert ref["capped0"].any() and abs(fd - (ard[m] + np.dot(st["y"][:m][free], ard[:m][free]))) <= 1e-6 * float(ref["T_slope"])
    assert float(ref["slope"]) == pytest.approx(ard[m] + np.dot(st["y"][:m], ard[:m]), rel=1e-12)
    assert float(ref["slope"]) < 0        # D = −t·G with G the gradient of the capped ℒ: a descent direction


@pytest.mark.parametrize("size", ac.SIZES, ids=lambda s: f"n{s[0]}-m{s[1]}-r{s[2]}")
def test_generator_claims_and_oracle_bounds(oracle_abi, size):
    """Per size, above FP64: the depths 0, 1, a middle one and ≥ 20 are all reached (the one large size has a handful of states:
    0 or 1, a middle one and ≥ 20), every descent state is decided, and from m = 2 on every state that backtracks has a row of
    its crossing block change sides of the cap between two consecutive trial steps k ≤ k_hp.  Then the oracle's
    linesearch_armijo on every state: all ratios ≤ 1, the decision rule, α bit for bit on decided states, the exact properties;
    at most 1 state in 10 undecided on the oracle's own A_RD, A_DD."""
    n, m, r = size
    depths = []
    for tag, st in ac.states(size):
        ref = armijo_state_ref(st)
        assert ref["decided"], (tag, ref["k_hp"])
        depths.append(ref["k_hp"])
        if m >= 2 and ref["k_hp"] >= 1:
            assert crossings(ref, st["cross"]) >= 1, tag
    assert (0 in depths or m > 60000) and (1 in depths or (m > 60000 and 0 in depths)), depths
    assert any(2 <= k < 20 for k in depths) and any(k >= 20 for k in depths), depths
    out = ac.run_size(oracle_abi, size)
    ac.report("oracle", size, out)
    assert not out["bad"], (len(out["bad"]), out["bad"][:6])
    assert 10 * len(out["undecided"]) <= out["n"], out["undecided"]


@pytest.mark.parametrize("size", [(12, 1, 3), (16, 65, 1), (24, 256, 1), (24, 257, 33)], ids=lambda s: f"n{s[0]}-m{s[1]}-r{s[2]}")
def test_exhaustion_and_tie_states(oracle_abi, size):
    """D = +t·G: above FP64 no trial step is accepted whose margin exceeds its round-off — every k < 50 with |margin| > τ has
    margin < 0 — so the search ends at k with |margin[k]| ≤ τ[k] or runs out at α_max/2⁵⁰; the oracle's answer obeys the rule
    and ℒ, the commit and the exact properties hold at its α.  D = 0: A_RD = A_DD = 0, every margin is exactly 0 and the first
    step is accepted (`≤`, :178): α = α_max and pv_raw unchanged bit for bit."""
    base = armijo_base(*size)
    s_, _ = make_solver(oracle_abi, base["data"], size[2], seed=5, h=4)
    st = armijo_state(base, 1.0, 1.0, "ascent")
    ref = armijo_state_ref(st)
    big = np.abs(ref["margin"][:ARMIJO_K]) > ref["tau"][:ARMIJO_K]
    assert big[0] and np.all(ref["margin"][:ARMIJO_K][big] < 0), ref["margin"][:ARMIJO_K][big]
    res = check_armijo_call(base, st, s_)
    assert res["on_grid"] and res["decision_ok"] and res["obj_is_last"] and res["pv_is_raw"], res
    assert res["k_dev"] >= int(np.flatnonzero(big)[-1]) + 1 and all(res[k] <= 1.0 for k in ac.RATIOS), res
    tie = armijo_state(base, 0.0, 4.0, "tie")
    ref = armijo_state_ref(tie)
    assert np.all(ref["margin"] == 0) and ref["k_hp"] == 0
    res = check_armijo_call(base, tie, s_)
    assert res["alpha"] == 4.0 and res["k_dev"] == 0 and np.array_equal(s_.primal_vio_raw, tie["pv_raw"]), res
    assert res["L"] <= 1.0 and res["obj_is_last"] and res["pv_is_raw"]
    s_.close()
