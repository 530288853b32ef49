"""The references of tests/test_gpu_fg_operators.py (helpers.fg_hp, S_and_G_hp, A_pair_hp) against the dense ones the suite
already trusts, every case of that file on the CPU oracle with the same assertions (fg_cases.run_case: this is how the bounds
are validated without a GPU), and a mutation check per quantity: an output with one term, one column or one chunk partial
missing must exceed its bound — while the old tolerance, rel() < 1e-12, lets the same output pass on the graded inputs."""
import numpy as np
import pytest

import sdplrplus_jl_amd as sj
from helpers import (FAMILIES_EQ, GRID, LD, U53, A_pair_hp, S_and_G_hp, S_dense_hp, _ld, dense, fg_hp, hp_gradient, make_data,
                     primal_vio_dense, worst_ratio)
import fg_cases as fc

KINDS = ["general_constraint_diag_cost", "two_general", "duplicates_and_missing_diag", "all_lowrank", "lowrank_cost_multi_column",
         "edge_constraints_sparse_cost"]


def rel(a, b):          # the old tolerance's measure (tests/test_gpu_parity.py)
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    return float(np.max(np.abs(a - b)) / (1.0 + np.max(np.abs(b)))) if a.size else 0.0


def _against_dense(C, As, bs, R, lam, sigma):
    m, n = len(As), C.shape[0]
    ref = fg_hp(C, As, bs, R, lam, np.full(m, np.inf), sigma)
    pv = primal_vio_dense(C, As, bs, R)
    # the dense recomputation is plain FP64: it meets the bound it is a reference for, with n² terms per output
    tol = (n * n + R.shape[1] + 4) * U53 * np.asarray(ref["T"], dtype=float)
    assert np.all(np.abs(pv - np.asarray(ref["v"], dtype=float)) <= tol + 1e-300)
    y = np.concatenate([-np.asarray(ref["yt"], dtype=np.float64), [1.0]])
    sg = S_and_G_hp(C, As, y, R)
    p = sg["pattern"]
    Sd = S_dense_hp(C, [A for A in As if not isinstance(A, sj.SymLowRankMatrix)] + ([] if isinstance(C, sj.SymLowRankMatrix) else [C]),
                    np.array([y[i] for i, A in enumerate(list(As) + [C]) if not isinstance(A, sj.SymLowRankMatrix)])) \
        if p["nnzS"] else np.zeros((n, n))
    if p["nnzS"]:
        assert worst_ratio(np.asarray(sg["full"], dtype=np.float64), Sd[p["f_row"], p["f_col"]], 4 * U53 * sg["full_mag"]) <= 1
        mask = np.zeros((n, n), dtype=bool)
        mask[p["f_row"], p["f_col"]] = True
        assert not np.any(np.asarray(Sd, dtype=np.float64)[~mask])
    return ref, y, sg


@pytest.mark.parametrize("family", list(FAMILIES_EQ))
def test_fg_hp_against_hp_gradient_and_dense(family):
    for seed, n, p, r in GRID[::3]:
        data, C, As, bs = make_data(family, seed, n, p)
        rng = np.random.Generator(np.random.PCG64(seed))
        R = rng.uniform(-1, 1, size=(data.n, r))
        lam = 0.1 * rng.standard_normal(data.m)
        ref, y, sg = _against_dense(C, As, bs, R, lam, 2.0)
        # the two references of G: hp_gradient forms y itself above FP64, S_and_G_hp takes the rounded y — they differ by
        # that rounding, u·|y_k| per matrix, i.e. by at most u·G_mag
        G2 = hp_gradient(C, As, bs, R, lam, 2.0)
        assert worst_ratio(np.asarray(sg["G"], dtype=np.float64), G2, 4 * U53 * sg["G_mag"]) <= 1


@pytest.mark.parametrize("kind", KINDS)
def test_fg_hp_on_unusual_structures(kind):
    from test_gpu_parity import _random_problem
    rng = np.random.Generator(np.random.PCG64(77))
    C, As, bs = _random_problem(kind, 14, rng)
    R = rng.uniform(-1, 1, size=(14, 5))
    ref, y, sg = _against_dense(C, As, bs, R, 0.1 * rng.standard_normal(len(As)), 2.0)
    Sfull = np.zeros((14, 14), dtype=LD)
    for yi, M in zip(y, list(As) + [C]):
        Sfull += LD(yi) * (_ld(M.B) * _ld(M.D)) @ _ld(M.B).T if isinstance(M, sj.SymLowRankMatrix) else LD(yi) * _ld(dense(M))
    assert worst_ratio(np.asarray(sg["G"], dtype=np.float64), 2 * Sfull @ _ld(R), 4 * U53 * sg["G_mag"]) <= 1
    D = rng.uniform(-1, 1, size=(14, 5))
    q = A_pair_hp(C, As, R, D)
    X = (_ld(R) @ _ld(D).T + _ld(D) @ _ld(R).T) / 2
    want = [np.sum(((_ld(M.B) * _ld(M.D)) @ _ld(M.B).T if isinstance(M, sj.SymLowRankMatrix) else _ld(dense(M))) * X) for M in list(As) + [C]]
    assert worst_ratio(np.asarray(q["q"], dtype=np.float64), want, 4 * U53 * q["mag"]) <= 1


ORACLE_WORST = {}


@pytest.mark.parametrize("name,r", [(n, r) for n, c in fc.CASES.items() for r in c["ranks"]])
def test_every_gpu_case_on_the_oracle(oracle_abi, name, r):
    worst, carve, _, _ = fc.run_case(oracle_abi, name, r)
    fc.report("oracle", name, r, worst, carve)
    for k, v in worst.items():
        ORACLE_WORST[k] = max(ORACLE_WORST.get(k, 0.0), v)
    fc.assert_case(name, r, worst, carve)
    assert sum(carve) == 0, "λ_ub is chosen so that the oracle needs no capping carve-out"


def test_oracle_maxima_are_reported():
    print("fg oracle maxima: " + " ".join(f"{k} {v:.3g}" for k, v in ORACLE_WORST.items()))


def _graded_state(oracle_abi, name, r):
    """The oracle's outputs on the case's graded input with λ graded: (case, input, v, y, G, references)."""
    bc = fc.built(name)
    inp = next(i for i in fc.case_inputs(name, r) if i["kind"] == "graded")
    s_ = fc.new_handle(oracle_abi, bc["data"], r)
    fc._load(s_, inp)
    s_.f()
    v = s_.primal_vio_raw
    s_.g()
    y, G = s_.y, s_.Gt
    s_.close()
    return bc, inp, v, y, G, S_and_G_hp(bc["C"], bc["As"], y, inp["R"], bc["pattern"])


def test_mutations_exceed_the_bounds_and_pass_the_old_tolerance(oracle_abi):
    bc, inp, v, y, G, gref = _graded_state(oracle_abi, "segmented", 3)
    ref, R, As = inp["ref"], inp["R"], bc["As"]
    assert worst_ratio(v, ref["v"], ref["bound_v"]) <= 1 and worst_ratio(G, gref["G"], gref["bound_G"]) <= 1
    T = np.asarray(ref["T"], dtype=np.float64)
    # (1) one term dropped from the smallest-scaled constraint: its largest one
    i = int(np.argmin(np.where(T[:-1] > 0, T[:-1], np.inf)))
    A = As[i]
    terms = A.vs * np.sum(R[A.is_] * R[A.js], axis=1)
    mut = v.copy()
    mut[i] -= terms[int(np.argmax(np.abs(terms)))]
    assert worst_ratio(mut, ref["v"], ref["bound_v"]) > 1 and rel(mut, v) < 1e-12
    # (3) one chunk partial dropped from a multi-chunk segment: the first CHUNK = 2048 upper-triangular entries of the 2049- and
    # of the 4097-entry constraint
    for i in (4, 5):
        A = As[i]
        up = np.flatnonzero(A.is_ <= A.js)
        assert up.size in (2049, 4097)
        e = up[:2048]
        t = A.vs[e] * np.sum(R[A.is_[e]] * R[A.js[e]], axis=1) * np.where(A.is_[e] == A.js[e], 1.0, 2.0)
        mut = v.copy()
        mut[i] -= float(np.sum(t))
        assert worst_ratio(mut, ref["v"], ref["bound_v"]) > 1 and rel(mut, v) < 1e-12
    # (2) the smallest-scaled row of G without the last column of its row of S — on the graph with isolated vertices, where
    # such a row is 2⁻⁴⁰ of the largest
    bc, inp, v, y, G, gref = _graded_state(oracle_abi, "fast_isolated", 8)
    R = inp["R"]
    assert worst_ratio(G, gref["G"], gref["bound_G"]) <= 1
    p = bc["pattern"]
    Gmag = np.asarray(np.max(gref["G_mag"], axis=1), dtype=np.float64)
    rows = np.bincount(p["f_col"], minlength=p["n"])
    j = int(np.argmin(np.where((rows > 0) & (Gmag > 0), Gmag, np.inf)))
    e = int(np.flatnonzero(p["f_col"] == j)[-1])
    mut = G.copy()
    mut[j] -= 2 * float(gref["full"][e]) * R[p["f_row"][e]]
    assert worst_ratio(mut, gref["G"], gref["bound_G"]) > 1 and rel(mut, G) < 1e-12
