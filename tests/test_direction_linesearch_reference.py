"""The reference side of tests/test_gpu_direction_linesearch.py, without a GPU: the two-loop recursion of
src/lbfgs.jl:77-124 and the exact line search of src/linesearch.jl:8-112 restated above FP64 (helpers.two_loop_hp,
helpers.quartic_hp, helpers.quartic_min_hp), and the CPU oracle — a plain FP64 implementation that shares no code with the
HIP kernels — held to the very bounds the GPU module asks of the HIP library.  That the oracle meets them shows they are
attainable in FP64.  The line-search recipes' root structure is asserted here, above FP64.
"""
import numpy as np
import pytest

from oracle import oracle
from helpers import (FAMILIES_EQ, LD, LS_AMAX, LS_RECIPES, LS_T, U53, check_direction_snapshots, check_linesearch_call,
                     drive_quadratic_history, linesearch_base, linesearch_state, make_data, make_solver, poly_hp, poly_T,
                     quartic_hp, quartic_min_hp, two_loop_hp)

SHAPES = [(12, 3), (5, 2), (3, 1), (12, 1), (12, 2), (9, 32), (7, 33)]
HS = [1, 3, 4, 5, 16, 17]
KAPPAS = [1e2, 1e6, 1e10]


def test_two_loop_hp_is_the_bfgs_matrix():
    """On a history whose pairs are exact (y = H·s in long double, rounded once) the recursion applies the inverse BFGS
    matrix built by the textbook update H⁺ = (I − ρsyᵀ)H(I − ρysᵀ) + ρssᵀ from H₀ = I over the same pairs, oldest first;
    empty slots (ρ = 0) drop out; negate flips the sign; h = 0 returns G itself."""
    rng = np.random.Generator(np.random.PCG64(3))
    N, h = 10, 4
    A = rng.standard_normal((N, N))
    Hq = A @ A.T + N * np.eye(N)
    for filled, latest in ((4, 2), (2, 2), (4, 4)):
        S = [np.zeros(N) for _ in range(h)]
        Y = [np.zeros(N) for _ in range(h)]
        order = [(latest - filled + k) % h for k in range(filled)]        # slots, oldest → newest
        for j in order:
            S[j] = rng.standard_normal(N)
            Y[j] = Hq @ S[j]
        G = rng.standard_normal(N)
        B = np.eye(N, dtype=LD)
        for j in order:
            s, y = S[j].astype(LD), Y[j].astype(LD)
            rho = 1 / np.dot(y, s)
            V = np.eye(N, dtype=LD) - rho * np.outer(y, s)
            B = V.T @ B @ V + rho * np.outer(s, s)
        want = -(B @ G.astype(LD))
        got = two_loop_hp(G, S, Y, latest, True)
        assert np.max(np.abs(got["dir"] - want)) <= 1e-15 * np.max(np.abs(want))
        assert abs(got["descent"] - np.dot(want, G.astype(LD))) <= 1e-15 * abs(got["descent"])
        assert np.all(got["M"] >= np.abs(got["dir"]) * (1 - 1e-15))
        assert np.array_equal(two_loop_hp(G, S, Y, latest, False)["dir"], -got["dir"])
    assert np.array_equal(two_loop_hp(G, [], [], 0, True)["dir"], G.astype(LD))


@pytest.mark.parametrize("h", HS)
@pytest.mark.parametrize("n,r", SHAPES)
def test_oracle_meets_the_direction_bounds(oracle_abi, n, r, h):
    """Every history of the GPU module built on the oracle (the same recipe through the same ABI), every direction along
    it: e ≤ 8·e_lit + γ·max(M)/‖dir_hp‖∞ holds trivially for dir (the oracle IS the literal evaluation, on a second handle
    loaded through set_factor/set_vec/set_scalar — this pins that loading reproduces the state bit for bit), and the
    literal error itself is printed on the termwise scale.  No history stops before its 3h + 2 updates."""
    data, *_ = make_data("maxcut", 1, n, 0.6)
    for kappa in KAPPAS:
        s_, _ = make_solver(oracle_abi, data, r, seed=3, h=h)
        o2, _ = make_solver(oracle_abi, data, r, seed=4, h=h)
        snaps = drive_quadratic_history(s_, h, kappa, seed=n * 100 + r, updates=3 * h + 2)
        assert len(snaps) == 3 * h + 3, (kappa, len(snaps))
        res = check_direction_snapshots(snaps, h, o2)
        print(f"oracle direction {n}x{r} h={h} kappa={kappa:g}: literal error / termwise bound {res['worst']['lit_dir']:.3g}")
        assert not res["bad"], res["bad"][:5]
        assert res["worst"]["ratio_lit"] <= 1.0 + 1e-12      # same code, same state: the same bits
        # the running bound of two_loop_hp (what a literal evaluation in another order is held to) is attainable
        print(f"   literal error / running bound {res['worst']['lit_run']:.3g}, centre jumps {res['jumps']}")
        assert res["worst"]["lit_run"] <= 1.0
        s_.close(); o2.close()


def test_oracle_meets_the_direction_bounds_on_a_nearly_repeated_pair(oracle_abi):
    data, *_ = make_data("maxcut", 1, 12, 0.6)
    s_, _ = make_solver(oracle_abi, data, 3, seed=3, h=4)
    o2, _ = make_solver(oracle_abi, data, 3, seed=4, h=4)
    snaps = drive_quadratic_history(s_, 4, 1e6, seed=55, updates=9, repeat_at=6)
    S = snaps[7]["S"]
    lat = snaps[7]["latest"] - 1
    rel = np.linalg.norm(S[lat] - S[(lat - 1) % 4]) / np.linalg.norm(S[lat])
    assert 1e-11 < rel < 1e-8, rel       # the two newest s differ by ≈ 1e-9 relative (the steps are equal to within it)
    res = check_direction_snapshots(snaps, 4, o2)
    assert not res["bad"], res["bad"][:5]
    s_.close(); o2.close()


# ---- the scalar stage -------------------------------------------------------------------------------------------------------
def _families(rng, k):
    """The four adversarial families of quartics, k cases each → (b[5], α_max)."""
    out = []
    for _ in range(k):      # tiny leading coefficient, down to 1e-16
        b = rng.standard_normal(5)
        b[1] = -abs(b[1])
        b[4] = abs(b[4]) * 10.0 ** rng.uniform(-16, 0)
        out.append((b, 1.0))
    for _ in range(k):      # near-double roots of the derivative, perturbations down to 1e-14
        r1 = rng.uniform(0.05, 0.9)
        r2 = r1 * (1 + 10.0 ** rng.uniform(-14, -3))
        r3 = rng.uniform(0.05, 3.0)
        out.append((_from_roots((r1, r2, r3), rng), 1.0))
    for _ in range(k):      # three stationary points inside [0, 1]
        out.append((_from_roots(np.sort(rng.uniform(0.02, 0.98, 3)), rng), 1.0))
    for _ in range(k):      # solver-like scaling b_k ∝ |D|^k
        d = 10.0 ** rng.uniform(-6, 2)
        b = rng.standard_normal(5) * d ** np.arange(5)
        b[1], b[4] = -abs(b[1]), abs(b[4])
        out.append((b, float(rng.choice([1e-3, 0.5, 1.0, 4.0]))))
    return out


def _from_roots(roots, rng):
    """b with derivative 4b₄·Π(α − ρ_i), b₄ > 0 (so f'(0) < 0 for positive roots), a random b₀."""
    b4 = abs(rng.standard_normal()) + 0.1
    r1, r2, r3 = roots
    d = 4 * b4 * np.array([-r1 * r2 * r3, r1 * r2 + r1 * r3 + r2 * r3, -(r1 + r2 + r3), 1.0])
    return np.array([rng.standard_normal(), d[0], d[1] / 2, d[2] / 3, d[3] / 4])


def test_quartic_min_hp_finds_planted_minima():
    rng = np.random.Generator(np.random.PCG64(12))
    for _ in range(200):
        roots = np.sort(rng.uniform(0.02, 0.98, 3))
        b = _from_roots(roots, rng)
        mn = quartic_min_hp(b, 1.0)
        f1, f3 = poly_hp(b, roots[0]), poly_hp(b, roots[2])     # the two minima of a quartic with three stationary points
        assert abs(mn["fmin"] - min(f1, f3)) <= 1e-15 * poly_T(b, 1.0)
        assert mn["fmin"] <= min(poly_hp(b, 0.0), poly_hp(b, 1.0))
    mn = quartic_min_hp([1.0, -1.0, 0.0, 0.0, 0.0], 4.0)          # a line: the end point
    assert mn["alpha"] == 4.0 and mn["fmin"] == -3.0
    mn = quartic_min_hp([1.0, 0.0, 0.0, 0.0, 0.0], 4.0)
    assert mn["fmin"] == 1.0


def test_oracle_quartic_argmin_on_adversarial_families():
    """oracle.quartic_argmin (bracketing) on ≈ 2 000 quartics of each family: 0 ≤ α ≤ α_max, the value it returns is the
    quartic's at its α to 12·u·T(α), and f_hp(α) − min f_hp ≤ 12·u·T(α_max): one Horner evaluation (eight roundings) decides
    between candidates, so a candidate can win or lose by that much and no more."""
    rng = np.random.Generator(np.random.PCG64(2024))
    worst = 0.0
    for b, amax in _families(rng, 2000):
        rc, a, f = oracle.quartic_argmin(b, amax)
        assert rc == 0 and 0.0 <= a <= amax
        mn = quartic_min_hp(b, amax)
        fa = poly_hp(b, a)
        assert abs(LD(f) - fa) <= 12 * U53 * poly_T(b, a)
        gap = float(fa - mn["fmin"]) / (U53 * poly_T(b, amax))
        worst = max(worst, gap)
        assert gap <= 12.0, (list(b), amax, a, float(mn["alpha"]), gap)
    print(f"oracle.quartic_argmin: largest optimality gap {worst:.3g} u T(alpha_max)")


# ---- the line-search states -------------------------------------------------------------------------------------------------
def _derivative(b):
    return np.array([k * b[k] for k in range(1, 5)], dtype=LD)


@pytest.mark.parametrize("r", [1, 3, 33])
@pytest.mark.parametrize("family", list(FAMILIES_EQ))
def test_linesearch_recipes_and_oracle(oracle_abi, family, r):
    """Every state of the GPU module: the root structure each recipe claims, verified above FP64 on the λ as rounded; then
    the oracle's linesearch(α_max) on it, held to the bounds of check 4."""
    base = linesearch_base(family, r)
    m = len(base["As"])
    o, _ = make_solver(oracle_abi, base["data"], r, seed=5, h=4)
    worst = dict(A_RD=0.0, A_DD=0.0, L=0.0, opt=0.0, commit=0.0)
    quad, count = 0, 0
    for amax in LS_AMAX:
        for t in LS_T:
            for recipe in LS_RECIPES:
                st = linesearch_state(base, t, amax, recipe)
                if st is None:
                    assert recipe == "three_roots" and t < 1.0      # the only combination that cannot be met
                    continue
                count += 1
                quad += st["quad_branch"]
                q = quartic_hp(base["C"], base["As"], base["bs"], st["R"], st["D"], st["lam"], st["pv_raw"], st["obj"], st["sigma"])
                b = q["b"]
                db = _derivative(b)
                ddb = np.array([k * db[k] for k in range(1, 4)], dtype=LD)
                am = LD(amax)
                assert b[1] < 0 and b[4] > 0
                grid = am * np.arange(1, 2001, dtype=LD) / 2000
                dgrid = db[0] + grid * (db[1] + grid * (db[2] + grid * db[3]))
                scale = lambda x: poly_T(db, x)
                # b₁ … b₄ scale as t¹ … t⁴, so roots of the size of α_max ask b₁ to cancel to ≈ t²·α_max² of its terms: from
                # t = 1e-4 on that is below what long double resolves of the state, and no structure is claimed — those
                # states serve the scaling b_k ∝ |D|^k and the quadratic branch, with the recipe as the aim of λ only
                assert st["claimed"] == (t >= 1e-2)
                if not st["claimed"]:
                    pass
                elif recipe == "three_roots":
                    for rt in st["roots"]:
                        assert 0 < rt < am
                        lo, hi = rt * (1 - LD(1e-6)), rt * (1 + LD(1e-6))
                        assert poly_hp(db, lo) * poly_hp(db, hi) < 0, (t, amax, rt)     # a sign change at each planted root
                elif recipe == "near_double":
                    # aimed at a gap of 1e-9; what long double can certify: at the stationary point of f′ next to the pair
                    # f′ is below 1e-15 of its term magnitude — a double root to every FP64 evaluation — and negative before it
                    x = st["roots"][0]
                    for _ in range(20):
                        x = x - poly_hp(ddb, x) / poly_hp(np.array([ddb[1], 2 * ddb[2]], dtype=LD), x)
                    assert abs(x - st["roots"][0]) <= 1e-6 * st["roots"][0] and 0 < x < am
                    assert abs(poly_hp(db, x)) <= 1e-15 * scale(x), (t, amax, float(poly_hp(db, x)), scale(x))
                    assert poly_hp(db, x / 2) < 0
                    r3 = st["roots"][2]          # the third root, where the recipe put it (a sign change: f′ > 0 beyond it)
                    assert r3 > 0 and poly_hp(db, r3 * (1 - LD(1e-6))) < 0 < poly_hp(db, r3 * (1 + LD(1e-6)))
                elif recipe == "beyond":
                    assert np.all(dgrid < 0)
                    assert quartic_min_hp(b, amax)["alpha"] == am
                else:
                    rt = st["roots"][0]
                    assert poly_hp(db, rt * (1 - LD(1e-6))) < 0 < poly_hp(db, rt * (1 + LD(1e-6)))
                    assert np.all(dgrid > 0)
                    assert quartic_min_hp(b, amax)["alpha"] <= rt * (1 + LD(1e-6))
                res = check_linesearch_call(base, st, o)
                assert res["inside"] and res["obj_is_last"] and res["pv_is_raw"], (t, amax, recipe, res)
                if recipe == "beyond":
                    assert res["alpha"] == amax
                for k in worst:
                    worst[k] = max(worst[k], res[k])
                    assert res[k] <= 1.0, (t, amax, recipe, k, res)
    o.close()
    assert count == 4 * (4 * 3 + 1), count
    print(f"oracle line search {family} r={r} (m={m}): error/bound " + " ".join(f"{k} {v:.3g}" for k, v in worst.items()))


def test_some_states_reach_the_quadratic_branch():
    """|4b₄| < eps (src/linesearch.jl:70) needs (c·t)⁴·σ‖q2‖² small; c grows as α_max shrinks, so t = 1e-6 reaches the branch
    at the larger α_max: at α_max = 4 on every family (what tests/test_gpu_direction_linesearch.py relies on), with a
    margin of 2 so that the device's own b₄ (a sum of squares, good to a few ulp) is on the same side."""
    for family in FAMILIES_EQ:
        base = linesearch_base(family, 3)
        st = linesearch_state(base, LS_T[-1], 4.0, "beyond")
        assert st["quad_branch"] and st["b4x4"] < np.finfo(np.float64).eps / 2, (family, st["b4x4"])
        assert not linesearch_state(base, 1.0, 4.0, "beyond")["quad_branch"]


@pytest.mark.parametrize("family,r", [("maxcut", 3), ("maxcut", 32), ("lovasz_theta", 3), ("minimum_bisection", 3)])
def test_oracle_leaves_no_fallback_decision_out(oracle_abi, family, r):
    """Check 3's states — k = 2h + 1 iterations of the loop from the start point, h ∈ {3, 4, 5}, on the instances of
    tests/test_gpu_direction_linesearch.py — on the oracle: the sign of descent_hp is decided on every one (|descent_hp|
    above its own error bound), it is a descent direction, and the oracle's next iteration does not fall back."""
    from helpers import history_snapshot, loop_state_direction
    data, *_ = make_data(family, 2, 12, 0.4)
    normC, normb = data.normC(), float(np.linalg.norm(data.b))
    for h in (3, 4, 5):
        o, _ = make_solver(oracle_abi, data, r, seed=11, h=h)
        out = o.inner_loop(normC, normb, True, True, False, 0.0, -1e300, 2 * h + 1, 0.0, *o.fg(normC, normb))
        assert out[4] == 2 * h + 1
        sn = history_snapshot(o, h)
        o2, _ = make_solver(oracle_abi, data, r, seed=11, h=h)
        d = loop_state_direction(sn, h, o2)
        o2.close()
        assert d["decided"] and d["hp"]["descent"] < 0, (h, float(d["hp"]["descent"]))
        nxt = o.inner_loop(normC, normb, True, True, False, 0.0, -1e300, 1, 0.0, *out[:3])
        assert nxt[3] != 0.0 and not np.array_equal(o.dirt, nxt[3] * (-sn["G"]))
        o.close()
