"""The reference side of tests/test_gpu_lanczos_steps.py, without a GPU: S and the Lanczos recurrence of
src/coreop.jl:461-500 restated above FP64 (helpers.S_dense_hp, helpers.lanczos_hp), and the CPU oracle — a plain
double-precision implementation that shares no code with the HIP kernels — held to the very bounds the GPU module asks
of every HIP route.  That the oracle meets them shows the bounds are attainable in FP64.

Largest error/bound ratio of the oracle over every two-step probe of an instance (bound = 1.0; measured with
np.longdouble as the reference type), as printed by test_oracle_meets_the_two_step_bounds_on_every_probe:

    maxcut150 0.201   maxcut257_hubs 0.444   wmaxcut300_w3 0.0282   wmaxcut300_w400 0.0271
    minbis150 0.00612 lovasz150 0.0058       lowrank60_3+6 0.0138   lowrank60_8 0.0412
"""
import numpy as np
import pytest

from helpers import (LANCZOS_INSTANCES, break_instance, S_dense, S_dense_hp, WIDE, lanczos_hp, lanczos_instance, make_data, make_solver,
                     set_S, two_step_max_ratio, two_step_ratio, two_step_reference, whole_run_checks)


def _tridiag_eigs(al, be):
    al, be = np.asarray(al, dtype=float), np.asarray(be, dtype=float)
    k = al.size
    return np.linalg.eigvalsh(np.diag(al) + np.diag(be[:k - 1], 1) + np.diag(be[:k - 1], -1))


@pytest.mark.parametrize("n", [12, 150])
@pytest.mark.parametrize("family", ["maxcut", "minimum_bisection", "lovasz_theta"])
def test_lanczos_hp_against_oracle_and_dense_spectrum(oracle_abi, family, n):
    """The families of test_lanczos_and_dual_obj: α₁, β₁, α₂, β₂ of the helper and of oracle.lanczos inside the two-step
    bounds; the tridiagonal of a full helper run (n − 1 steps above FP64) has the spectrum of S."""
    data, C, As, bs = make_data(family, 3, n, 0.4 if n == 12 else 0.08)
    rng = np.random.Generator(np.random.PCG64(44))
    y = rng.standard_normal(data.m + 1)
    S = S_dense_hp(C, As, y)
    assert np.max(np.abs(np.asarray(S, dtype=float) - S_dense(C, As, y))) <= 1e-13 * np.max(np.abs(S_dense(C, As, y)))
    X = rng.standard_normal((n, 4))
    ref = two_step_reference(S, X, lowrank=family != "maxcut")
    o, _ = make_solver(oracle_abi, data, 3, seed=4)
    set_S(o, y)
    for k in range(X.shape[1]):
        ah, bh, kh, V = lanczos_hp(S, X[:, k], 2)
        assert kh == 2 and len(V) == 2
        # the column-wise reference of the probes IS the literal recurrence (same type, same operations up to the order
        # of two sums): far inside the bound
        assert two_step_ratio(ref, k, ah, bh) <= (1e-3 if WIDE else 1.0)
        ao, bo, ko = o.lanczos(2, X[:, k])
        assert ko == 2 and two_step_ratio(ref, k, ao, bo) <= 1.0
    o.close()
    if n == 12 or WIDE:
        # the whole run (cap q ≤ n − 1 of :465): Ritz values of an (n − 1)-step run above FP64 interlace Λ(S) and the
        # extreme ones have converged at this size
        a, b, k, V = lanczos_hp(S, X[:, 0], 10 * n)
        assert k == n - 1 == len(V)
        lam = np.linalg.eigvalsh(np.asarray(S, dtype=float))
        th = _tridiag_eigs(a, b)
        scale = np.max(np.abs(lam))
        assert lam[0] - 1e-12 * scale <= th[0] and th[-1] <= lam[-1] + 1e-12 * scale
        if n == 12:
            # n − 1 of n steps: Cauchy interlacing, λ_j ≤ θ_j ≤ λ_{j+1}
            assert np.all(lam[:-1] - 1e-12 * scale <= th) and np.all(th <= lam[1:] + 1e-12 * scale)
        else:
            assert abs(th[0] - lam[0]) <= 1e-8 * scale and abs(th[-1] - lam[-1]) <= 1e-8 * scale


def test_lanczos_hp_break_and_cap(oracle_abi):
    """The break test of :494 and the cap of :465 where both are exact (helpers.break_instance), helper and oracle."""
    data, y, S = break_instance(150)
    n = data.n
    assert float(S[3, 3]) == float(S[4, 4]) == 5 / 64 and float(S[3, 4]) == 1 / 64 and float(S[7, 7]) == 8 / 64
    assert np.count_nonzero(np.asarray(S, dtype=float)) == n + 2
    e = np.eye(n)
    o, _ = make_solver(oracle_abi, data, 4, seed=3)
    set_S(o, y)
    for x, steps, a_first in ((e[3] + e[4], 1, 6 / 64), (e[3] - e[4], 1, 4 / 64), (e[3], 2, 5 / 64), (e[7], 1, 8 / 64)):
        a, b, k, V = lanczos_hp(S, x, 6)
        ao, bo, ko = o.lanczos(6, x)
        assert k == ko == steps
        for al, be in ((a, b), (ao, bo)):
            assert abs(float(be[-1])) < np.sqrt(n) * np.finfo(float).eps * float(np.max(np.sum(np.abs(S), axis=1)))
            assert abs(float(al[0]) - a_first) <= 4 * 2.0 ** -53 * a_first
    a, b, k, V = lanczos_hp(S, np.ones(n), 1000)
    assert k == n - 1 == o.lanczos(1000, np.ones(n))[2]
    o.close()


@pytest.mark.parametrize("name", list(LANCZOS_INSTANCES))
def test_oracle_meets_the_two_step_bounds_on_every_probe(oracle_abi, name):
    """Every start vector of every instance of the GPU module on the oracle: inside the bounds (ratio ≤ 1); a whole run of
    q = min(60, n − 1) steps inside the containment and clustering windows."""
    inst = lanczos_instance(name)
    assert inst["ref"]["live"].sum() >= inst["n"]          # (only the rows without off-diagonal entries break at once)
    o, _ = make_solver(oracle_abi, inst["data"], 4, seed=3)
    set_S(o, inst["y"])
    worst = two_step_max_ratio(inst, o)
    print(f"oracle two-step ratio {name}: {worst:.3g}  (kappa max {np.max(inst['ref']['kappa'][inst['ref']['live']]):.3g})")
    assert worst <= 1.0
    q = min(60, inst["n"] - 1)
    al, be, k = o.lanczos(q, inst["X"][:, 0])
    assert k == q
    whole_run_checks(inst, al, be, q)
    o.close()
