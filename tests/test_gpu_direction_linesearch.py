"""The L-BFGS direction (src/lbfgs.jl:77-124) and the exact line search (src/linesearch.jl:4-127) of the HIP library,
operator by operator, against references above FP64 (helpers.two_loop_hp, helpers.quartic_hp, helpers.quartic_min_hp; the
CPU oracle is held to the same bounds in tests/test_direction_linesearch_reference.py).

Direction.  The library evaluates the recursion in Gram form for h ≤ 16 (k_dense.h: every ⟨s_j, q⟩ a difference of
already-rounded dots) and literally above; the reference takes every dot on the running vector q.  The histories are
built through the ABI on the gradient field of an SPD quadratic (helpers.drive_quadratic_history: κ ∈ {1e2, 1e6, 1e10},
exact line-search steps above FP64, 3h + 2 updates, a direction checked before every update), at N ≫ h, N ≈ h and N < h, on
every sub-wave rank shape, and once with a nearly repeated pair.  For each direction the literal FP64 evaluation of the
same state (the oracle, loaded through set_factor / set_vec / set_scalar) gives e_lit, and the library must meet
    e ≤ 8·e_lit + γ·max(M)/‖dir_hp‖∞,   γ = (2h + 4 + ⌈log₂ N⌉)·u
— likewise the returned descent (scale ΣM|G|) and V_LBFGS_A.

Line search.  States set through set_vec / set_scalar (helpers.linesearch_state: four aims for the derivative's roots, D
scaled by t ∈ {1, 1e-2, 1e-4, 1e-6}, α_max ∈ {1e-3, 0.5, 1, 4}) on the seven equality families at r ∈ {1, 3, 33}: A_RD and
A_DD termwise, ℒ against the quartic above FP64 at the returned α, the optimality gap, 0 ≤ α ≤ α_max, and the commit.

Measured on an MI355X (bound = 1): direction, N ≫ h (12x3, 9x32, 7x33, every h and κ): e/e_lit ≤ 8.6, error/bound ≤ 0.57;
N ≈ h or N < h: see _BROKEN below, the rest ≤ 0.88; nearly repeated pair: e/e_lit 1.86, error/bound 0.064.  Line search,
largest over all states and families: A_RD 0.24, A_DD 0.28, ℒ 0.41, optimality gap 0.0043, commit 0.24.

Inside the loops (test_direction_and_fallback_inside_the_loop, test_alpha_and_L_through_one_iteration): the two-handle
recipe and the one-iteration (α, ℒ) check on the graph, eager, stored-form, no-fused-update, dot-descent, NO_FAST, NO_FAST2,
NO_LRFUSE routes, the resident loop (TEAM 1 and 3), the resident loop in a batch call and the edge path's group launch; every
route read from stats().  Largest e/e_lit and error/bound of the in-loop direction per route, measured on an MI355X:
    instance            graph         resident (team 3)   batch / group
    maxcut 12x3         4.09  0.119   3.17  0.141         3.17  0.141
    maxcut 12x32        -             0.995 0.036         0.995 0.036
    lovasz_theta 12x3   1.65  0.059   (launches: same)    1.48  0.048 (group)
    minbis 12x3         0.97  0.038   1.17  0.039         2.11  0.066
    maxcut 300x8 (ring) 0.53  0.026   0.52  0.015         -
Over all routes: error/bound ≤ 0.143, e/e_lit ≤ 4.09; the fallback was taken exactly where descent_hp ≥ 0 and no state was
left undecided (nor by the oracle: tests/test_direction_linesearch_reference.py); the constructed wrong-sign state falls
back on every route.  One iteration: ℒ error/bound ≤ 0.035 over all routes and instances.  Per-history direction figures
are printed by every test (run with -s); the maxima per shape are above.

Not covered: the Gram form's effect on the fallback decision at N ≤ h INSIDE a loop (the in-loop instances have N ≫ h).
"""
import numpy as np
import pytest

from helpers import (FAMILIES_EQ, LS_AMAX, LS_RECIPES, LS_T, check_direction_snapshots, check_linesearch_call,
                     drive_quadratic_history, linesearch_base, linesearch_state, make_data, make_solver)

pytestmark = pytest.mark.gpu

SHAPES = [(12, 3), (5, 2), (3, 1), (12, 1), (12, 2), (9, 32), (7, 33)]
HS = [1, 3, 4, 5, 16, 17]
KAPPAS = [1e2, 1e6, 1e10]


def _report(tag, res):
    w = res["worst"]
    print(f"direction {tag}: e/e_lit {w['ratio_lit']:.3g}  error/bound dir {w['dir']:.3g} descent {w['desc']:.3g} "
          f"a {w['a']:.3g}  (literal error / termwise bound {w['lit_dir']:.3g}, error / running bound {w['run']:.3g})")


class GramFormBreaksTheBound(AssertionError):
    """The measured loss of the Gram form, on the histories and quantities listed in _BROKEN and nowhere else."""


# Where the Gram form (h ≤ 16) breaks the bound on an MI355X: (n, r, h, κ) → {quantity: measured error/bound}.  All are
# histories with N = n·r ≤ h or barely above it (the y_j linearly dependent or nearly so) from κ = 1e6 on; every κ = 1e2
# history, every N ≫ h history and every quantity not listed here holds and is asserted as such.  The listed quantity must
# stay under 4× the measured figure (a further loss is a failure, not an expected one); a case that comes to hold turns
# its strict xfail into a failure, and the entry is then taken out.
_BROKEN = {(5, 2, 16, 1e6): {"dir": 117.0}, (5, 2, 16, 1e10): {"dir": 1.31e4},
           (3, 1, 3, 1e6): {"dir": 503.0}, (3, 1, 3, 1e10): {"dir": 3.03e3},
           (3, 1, 4, 1e10): {"dir": 1.88e3},
           (3, 1, 5, 1e6): {"dir": 4.2e4}, (3, 1, 5, 1e10): {"dir": 1.65e3},
           (3, 1, 16, 1e6): {"dir": 187.0}, (3, 1, 16, 1e10): {"dir": 1.6e4, "desc": 2.58},
           (12, 1, 16, 1e6): {"dir": 2.68e3}, (12, 1, 16, 1e10): {"dir": 4.34e3},
           # (the next one sits on the edge of the bound — a 1.01 — and may come to hold, or V_LBFGS_A alone may, after a harmless
           # change of summation order: the strict xfail then fails, and the entry is narrowed or taken out)
           (12, 2, 16, 1e10): {"dir": 2.83, "a": 1.01}}
_DIR_CASES = [pytest.param(n, r, h, k, marks=pytest.mark.xfail(strict=True, raises=GramFormBreaksTheBound,
                                                             reason=f"Gram form, N = {n * r}, h = {h}: error/bound {_BROKEN[(n, r, h, k)]}"))
              if (n, r, h, k) in _BROKEN else (n, r, h, k) for n, r in SHAPES for h in HS for k in KAPPAS]


@pytest.mark.parametrize("n,r,h,kappa", _DIR_CASES)
def test_direction_op_by_op(hip_abi, oracle_abi, n, r, h, kappa):
    """h ≤ 16: the Gram form, held to 8·e_lit + termwise.  h = 17: the literal route (k_lit_*), the oracle's recursion in
    another summation order, held to the larger of that and the running bound (helpers.check_direction_snapshots)."""
    data, *_ = make_data("maxcut", 1, n, 0.6)
    g, _ = make_solver(hip_abi, data, r, seed=3, h=h)
    o, _ = make_solver(oracle_abi, data, r, seed=4, h=h)
    snaps = drive_quadratic_history(g, h, kappa, seed=n * 100 + r, updates=3 * h + 2)
    assert len(snaps) == 3 * h + 3
    res = check_direction_snapshots(snaps, h, o, literal=h > 16)
    g.close(); o.close()
    _report(f"{n}x{r} h={h} kappa={kappa:g} jumps={res['jumps']}", res)
    known = _BROKEN.get((n, r, h, kappa), {})
    w = res["worst"]
    for q in ("dir", "desc", "a"):
        if q in known:
            assert w[q] <= 4 * known[q], (q, w[q], known[q])
        else:
            assert w[q] <= 1.0, (q, w[q], [b for b in res["bad"] if f" {q}:" in b][:4])
    if any(w[q] > 1.0 for q in known):
        raise GramFormBreaksTheBound({q: w[q] for q in known})


def test_direction_on_a_nearly_repeated_pair(hip_abi, oracle_abi):
    """Two consecutive pairs whose s differ by 1e-9 relative (the direction written from the host, the step repeated):
    SY and YY then have two rows equal to nine digits."""
    data, *_ = make_data("maxcut", 1, 12, 0.6)
    g, _ = make_solver(hip_abi, data, 3, seed=3, h=4)
    o, _ = make_solver(oracle_abi, data, 3, seed=4, h=4)
    snaps = drive_quadratic_history(g, 4, 1e6, seed=55, updates=9, repeat_at=6)
    S, lat = snaps[7]["S"], snaps[7]["latest"] - 1
    rel = np.linalg.norm(S[lat] - S[(lat - 1) % 4]) / np.linalg.norm(S[lat])
    assert 1e-11 < rel < 1e-8, rel
    res = check_direction_snapshots(snaps, 4, o)
    _report("12x3 h=4 kappa=1e6 repeated pair", res)
    g.close(); o.close()
    assert not res["bad"], res["bad"][:6]


@pytest.mark.parametrize("r", [1, 3, 33])
@pytest.mark.parametrize("family", list(FAMILIES_EQ))
def test_linesearch_states(hip_abi, family, r):
    base = linesearch_base(family, r)
    g, _ = make_solver(hip_abi, base["data"], r, seed=5, h=4)
    worst = dict(A_RD=0.0, A_DD=0.0, L=0.0, opt=0.0, commit=0.0)
    bad = []
    for amax in LS_AMAX:
        for t in LS_T:
            for recipe in LS_RECIPES:
                st = linesearch_state(base, t, amax, recipe)
                if st is None:
                    continue
                res = check_linesearch_call(base, st, g)
                tag = (t, amax, recipe if st["claimed"] else "aim:" + recipe)
                if not (res["inside"] and res["obj_is_last"] and res["pv_is_raw"]):
                    bad.append((tag, "exact properties", res))
                if recipe == "beyond" and st["claimed"] and res["alpha"] != amax:
                    bad.append((tag, "alpha != alpha_max", res["alpha"]))
                for k in worst:
                    worst[k] = max(worst[k], res[k])
                    if not res[k] <= 1.0:
                        bad.append((tag, k, res[k]))
    g.close()
    print(f"line search {family} r={r}: error/bound " + " ".join(f"{k} {v:.3g}" for k, v in worst.items()))
    assert not bad, (len(bad), bad[:6])


@pytest.mark.parametrize("family", list(FAMILIES_EQ))
def test_linesearch_quadratic_branch(hip_abi, family):
    """t = 1e-6 at α_max = 4: |4b₄| < eps/2 above FP64 (asserted on the CPU for every family), so the device's own b₄ — a sum
    of squares, good to a few ulp — takes the branch of src/linesearch.jl:70-83: the checks of check 4 on that branch."""
    base = linesearch_base(family, 3)
    g, _ = make_solver(hip_abi, base["data"], 3, seed=5, h=4)
    for recipe in LS_RECIPES[1:]:
        st = linesearch_state(base, LS_T[-1], 4.0, recipe)
        assert st["quad_branch"] and st["b4x4"] < np.finfo(np.float64).eps / 2
        res = check_linesearch_call(base, st, g)
        assert res["inside"] and all(res[k] <= 1.0 for k in ("A_RD", "A_DD", "L", "opt", "commit")), (recipe, res)
    g.close()


# ---- checks 2 and 3: the direction and the fallback decision inside the loops ----------------------------------------------
from sdplrplus_jl_amd import cabi, problems                                             # noqa: E402
from helpers import (U53, direction_errors, history_snapshot, lanczos_instance, linesearch_c, loop_state_direction, poly_hp,  # noqa: E402
                     quartic_hp, quartic_min_hp)

from helpers import LOOP_ROUTES, RESIDENT_FAMILIES, assert_route as _assert_route, set_route as _set_route        # noqa: E402


def _loop_datas(family, route):
    if family == "maxcut300":
        return [problems.maxcut_data(problems.gnp_graph(300, 0.05, 7))]
    if family == "lowrank60_8":
        return [lanczos_instance(family)["data"]]
    return [make_data(family, s, 12, 0.4)[0] for s in ((2, 3, 4) if route in ("resident_batch", "group") else (2,))]


def _run_loops(hip_abi, monkeypatch, route, datas, r, h, iters, lam=None):
    """Fresh handles, [λ,] fg!, `iters` iterations in one call — through inner_loop, or for the two batch routes through one
    sdplr_hip_batch_major_iteration (no λ update, σ as it is: lbfgs_clear!, fg!, the loop) → [(handle, (ℒ, ‖G‖, ‖pv‖, α, iterations, exit))]."""
    _set_route(monkeypatch, route)
    S = [make_solver(hip_abi, d, r, seed=11, h=h)[0] for d in datas]
    norms = [(d.normC(), float(np.linalg.norm(d.b))) for d in datas]
    if lam is not None:
        for s_, l in zip(S, lam):
            s_.λ = l
    if route in ("resident_batch", "group"):
        res = cabi.batch_major_iteration(hip_abi, S, [(nc, nb, 1, 1, 0, 0, 2.0, 0.0, -1e300, iters, 0.0) for nc, nb in norms])
        outs = []
        for o in res:
            assert not isinstance(o, Exception), o
            outs.append(tuple(o[:6]))
    else:
        outs = [s_.inner_loop(nc, nb, True, True, False, 0.0, -1e300, iters, 0.0, *s_.fg(nc, nb)) for s_, (nc, nb) in zip(S, norms)]
    for o in outs:
        assert o[4] == iters and o[5] == 2, o
    return list(zip(S, outs))


LOOP_CASES = [(f, r, route) for f, r in (("maxcut", 3), ("maxcut", 32), ("lovasz_theta", 3), ("minimum_bisection", 3), ("maxcut300", 8))
              for route in LOOP_ROUTES if route != "no_lrfuse" and (route != "group" or f == "lovasz_theta")
              and (route != "resident_batch" or f in ("maxcut", "minimum_bisection"))]


@pytest.mark.parametrize("family,r,route", LOOP_CASES)
def test_direction_and_fallback_inside_the_loop(hip_abi, oracle_abi, monkeypatch, family, r, route):
    """Two sets of handles from the same start: A runs k = 2h + 1 iterations in one call, B runs k + 1 (a third repeats A
    bit for bit).  A's G, s, y, latest (reading materialises a ring) define iteration k + 1's direction above FP64; B's dirt
    is fl(α·dir) with α its last step.  ‖dirt_B − α·dir_hp‖/‖α·dir_hp‖ ≤ 8·e_lit + γ·max(M)/‖dir_hp‖∞ + 2u, e_lit from the
    oracle's lbfgs_dir on A's state; Rt_B = fl(Rt_A + dirt_B) to 1 ulp; and where |descent_hp| exceeds its own bound the
    route fell back to −G (dirt_B = fl(α·(−G)) exactly) if and only if descent_hp ≥ 0 (src/sdplr.jl:202).  maxcut300 is
    the instance on which the ring form is taken; lovasz_theta is the edge path, in a batch call its group launch."""
    datas = _loop_datas(family, route)
    excluded = []
    for h in (3, 4, 5):
        k = 2 * h + 1
        As_, Bs_, Cs_ = (_run_loops(hip_abi, monkeypatch, route, datas, r, h, it) for it in (k, k + 1, k))
        for data, (A, oa), (B, ob), (C, oc) in zip(datas, As_, Bs_, Cs_):
            if route == "group" and h > 4:
                assert A.stats()["group_launch_loops"] == 0
            _assert_route(route, family, r, h, A.stats())
            _assert_route(route, family, r, h, B.stats())
            sn, RA = history_snapshot(A, h), A.Rt
            assert oa == oc and np.array_equal(RA, C.Rt) and np.array_equal(sn["G"], C.Gt)
            dB, RB, alpha = B.dirt, B.Rt, ob[3]
            assert alpha != 0.0
            o, _ = make_solver(oracle_abi, data, r, seed=11, h=h)
            d = loop_state_direction(sn, h, o)
            o.close()
            hp = d["hp"]
            fell_back = bool(np.array_equal(dB, alpha * (-sn["G"])))
            if d["decided"]:
                assert fell_back == bool(hp["descent"] >= 0), (h, float(hp["descent"]), fell_back)
            else:
                excluded.append(h)
            if not fell_back:
                err = direction_errors(hp, dB / alpha, 0.0)["e"]
                bound = 8 * d["lit"]["e"] + d["sc"]["e"] + 2 * U53
                print(f"loop direction {family} r={r} h={h} {route}: e/e_lit {err / max(d['lit']['e'], 1e-300):.3g} error/bound {err / bound:.3g}")
                assert err <= bound, (h, err, d["lit"]["e"], d["sc"]["e"])
            assert np.all(np.abs(RB - (RA + dB)) <= np.spacing(np.abs(RB))), h
            for s_ in (A, B, C):
                s_.close()
    assert len(excluded) <= 1, excluded
    if excluded:
        print(f"fallback decision {family} r={r} {route}: undecided at h = {excluded}")


@pytest.mark.parametrize("route", [rt for rt in LOOP_ROUTES if rt not in ("no_lrfuse", "resident_batch", "group")])
def test_every_route_falls_back_on_a_wrong_sign_state(hip_abi, monkeypatch, route):
    """The fresh_g recipe of tests/test_gpu_ring.py: the newest pair replaced by (s = G, y = 0, ρ = −1e6/‖G‖²) makes
    ⟨dir, G⟩ ≈ +1e6·‖G‖² — the wrong sign by a wide margin; after a fresh g! the next iteration must step along −G exactly.
    (The batch entry points rebuild the history in their prologue, so they cannot be handed this state.)"""
    family, r = ("maxcut300", 8) if route in ("graph", "eager") else ("maxcut", 3)
    data = _loop_datas(family, route)[0]
    normC, normb = data.normC(), float(np.linalg.norm(data.b))
    h = 4
    _set_route(monkeypatch, route)
    s_, _ = make_solver(hip_abi, data, r, seed=11, h=h)
    st = s_.inner_loop(normC, normb, True, True, False, 0.0, -1e300, h + 2, 0.0, *s_.fg(normC, normb))[:3]
    j = int(s_.get_scalar(cabi.S_LBFGS_LATEST)) - 1
    G = s_.Gt
    s_.set_factor(cabi.F_LBFGS_S + j, G)
    s_.set_factor(cabi.F_LBFGS_Y + j, np.zeros_like(G))
    rho = s_.get_vec(cabi.V_LBFGS_RHO)
    rho[j] = -1e6 / float(np.sum(G * G))
    s_.set_vec(cabi.V_LBFGS_RHO, rho)
    s_.g()
    G = s_.Gt
    out = s_.inner_loop(normC, normb, True, True, False, 0.0, -1e300, 1, 0.0, *st)
    assert out[4] == 1 and out[3] != 0.0
    assert np.array_equal(s_.dirt, out[3] * (-G))
    _assert_route(route, family, r, h, s_.stats())
    s_.close()


# ---- check 4 inside the loops: (α, ℒ) of one iteration on a cleared history ---------------------------------------------------
STEP_CASES = [(f, route) for f in ("maxcut", "lovasz_theta", "minimum_bisection", "cutnorm", "maxcut300", "lowrank60_8")
              for route in LOOP_ROUTES if route != "graph" and (route != "group" or f == "lovasz_theta")      # (one iteration is never replayed)
              and (route != "resident_batch" or f in ("maxcut", "minimum_bisection", "cutnorm"))
              and (route != "no_lrfuse" or f in ("lowrank60_8", "minimum_bisection", "maxcut300"))]


@pytest.mark.parametrize("family,route", STEP_CASES)
def test_alpha_and_L_through_one_iteration(hip_abi, monkeypatch, family, route):
    """inner_loop(max_local_iters = 1) on a cleared history with a seeded λ: the direction is −G exactly (asserted), so the
    quartic above FP64 is taken with D = −G of the DEVICE's own G — read before the call — and carries no term for the
    gradient's error (the issue's form takes D from hp_gradient and widens the bound by that error; this one asks no less).
    |ℒ − f_hp(α)| ≤ c·u·T(α), f_hp(α) − min f_hp ≤ 2c·u·T(1), 0 ≤ α ≤ 1; the iterate R + α·D to 1 ulp.  This is what reaches
    k_ls_solve_fast (both), the fused low-rank variant (lowrank60_8; SDPLR_HIP_NO_LRFUSE its counterpart) and the resident
    SOLVE stage; lovasz_theta in a batch call is the group launch."""
    if family in ("maxcut300", "lowrank60_8"):
        datas = _loop_datas(family, route)
        if family == "lowrank60_8":
            inst = lanczos_instance(family)
            mats = [(inst["C"], inst["As"], inst["bs"])]
        else:
            mats = [problems.maxcut(problems.gnp_graph(300, 0.05, 7))]
    else:
        seeds = (2, 3, 4) if route in ("resident_batch", "group") else (2,)
        full = [make_data(family, s, 12, 0.4) for s in seeds]
        datas, mats = [f[0] for f in full], [f[1:] for f in full]
    r, h = (8 if family == "maxcut300" else 3), 4
    rng = np.random.Generator(np.random.PCG64(61))
    lam = [0.1 * rng.standard_normal(d.m) for d in datas]
    # the state before the step, from twin handles on the plain route (fg! is the same state on every route: pinned above FP64
    # in tests/test_gpu_fg_operators.py; here only R, λ and what f! left are read, and G of the very handle that steps — below)
    _set_route(monkeypatch, route)
    S = [make_solver(hip_abi, d, r, seed=11, h=h)[0] for d in datas]
    norms = [(d.normC(), float(np.linalg.norm(d.b))) for d in datas]
    pre = []
    for s_, l, (nc, nb) in zip(S, lam, norms):
        s_.λ = l
        st = s_.fg(nc, nb)
        pre.append(dict(st=st, R=s_.Rt, G=s_.Gt, pv=s_.primal_vio_raw, obj=s_.obj))
    if route in ("resident_batch", "group"):
        res = cabi.batch_major_iteration(hip_abi, S, [(nc, nb, 1, 1, 0, 0, 2.0, 0.0, -1e300, 1, 0.0) for nc, nb in norms])
        outs = [tuple(o[:6]) for o in res]
    else:
        outs = [s_.inner_loop(nc, nb, True, True, False, 0.0, -1e300, 1, 0.0, *p["st"]) for s_, p, (nc, nb) in zip(S, pre, norms)]
    for s_, p, out, (C_, As_, bs_), l, d in zip(S, pre, outs, mats, lam, datas):
        assert out[4] == 1 and out[5] == 2, out
        _assert_route(route, family, r, h, s_.stats())
        L, alpha = out[0], out[3]
        D = -p["G"]
        assert alpha != 0.0 and np.array_equal(s_.dirt, alpha * D)           # the cleared history: dir = −G, then s = α·dir
        q = quartic_hp(C_, As_, bs_, p["R"], D, l, p["pv"], p["obj"], 2.0)
        mn = quartic_min_hp(q["b"], 1.0)
        cc = linesearch_c(d.m)
        f_at = poly_hp(q["b"], alpha)
        rL = float(abs(np.longdouble(L) - f_at) / (cc * U53 * mn["T"](alpha)))
        ropt = float((f_at - mn["fmin"]) / (2 * cc * U53 * mn["T"](1.0)))
        print(f"loop step {family} {route}: L error/bound {rL:.3g} optimality gap/bound {ropt:.3g} alpha {alpha:.6g}")
        assert 0.0 <= alpha <= 1.0 and rL <= 1.0 and ropt <= 1.0, (rL, ropt, alpha)
        assert np.all(np.abs(s_.Rt - (p["R"] + s_.dirt)) <= np.spacing(np.abs(s_.Rt)))
        s_.close()
