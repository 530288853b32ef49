"""GPU tests of the high-precision dual bound as one device call (include/sdplr_hip_dual_hp.h): sdplr_hip_dual_obj_hp and
sdplr_hip_batch_dual_obj_hp (k_dual_hp.h: the prologue grid; k_eig_resident.h: the eigensolver's).

State is set directly: a random R, λ and σ, then one fg so that primal_vio_raw is current.  Sizes: n = 5 (ncv = n, no
restart), 64 and 65 (a wave boundary in the prologue's reductions: m = n for MaxCut), 130 (ncv = 100 < n: thick restarts);
per size MaxCut, MinimumBisection (a rank-one constraint in the operator) and mu_conductance_ineq with a λ for which
min(λ_ub, ·) clips some constraints and leaves others.

How the two scalar checks of the bound are stated here.
 * dual_value = −⟨y[1:m], b⟩ + tb·min(ev, 0).  The bound m·eps·Σ|yᵢbᵢ| is the one for re-ordering a sum of m terms, so it
   is asserted on the sum itself: with tb = 0 the call returns −⟨y, b⟩ as the device summed it.  With tb = n the value must
   then be the IEEE result of ``d0 + tb·min(ev, 0)`` bit for bit (the same device sum, one product and one addition on the
   host side of the library).  Together they say what the formula within that bound says, without charging the rounding
   of the last addition (≈ eps·tb·|ev|, which for mu_conductance's tiny b exceeds m·eps·Σ|yᵢbᵢ|) to the dot product.
 * 0 ≤ mineig − λ_min(S) ≤ tol·max(eps^⅔, |λ_min + 1|): λ_min comes from numpy's eigvalsh of the dense S in FP64, whose own
   error is of the order n·eps·‖S‖∞; the lower side is asserted as −n·eps·‖S‖∞ ≤ mineig − λ_min (a Ritz value of the
   exactly Krylov-closed n = 5 case equals λ_min to the last bits, on either side of eigvalsh's)."""
import importlib

import numpy as np
import pytest

import sdplrplus_jl_amd as sj
from sdplrplus_jl_amd import batch, cabi, problems

from helpers import S_dense_hp, make_solver

pytestmark = pytest.mark.gpu
sdplr_mod = importlib.import_module("sdplrplus_jl_amd.sdplr")
EPS = float(np.finfo(np.float64).eps)
TOL = 1e-6
SIZES = (5, 64, 65, 130)
FAMILIES = ("maxcut", "minimum_bisection", "mu_conductance_ineq")
CASES = [(f, n) for n in SIZES for f in FAMILIES]


@pytest.fixture(autouse=True)
def _small_instances_take_their_own_route(monkeypatch):
    for k in ("SDPLR_HIP_FORCE_GRAPH", "SDPLR_HIP_NO_RESIDENT", "SDPLR_HIP_NO_BATCH_EIG", "SDPLR_HIP_BATCH_EIG_NMAX",
              "SDPLR_HIP_BATCH_EIG_CYCLES", "SDPLR_HIP_NO_FUSED_DUAL"):
        monkeypatch.delenv(k, raising=False)


def graph(n, seed):
    """G(n, p) plus the cycle 0-1-…-(n−1)-0: every degree ≥ 2, unit weights."""
    import scipy.sparse as sp
    A = sp.lil_matrix(problems.gnp_graph(n, min(1.0, 6.0 / n), seed))
    for i in range(n):
        j = (i + 1) % n
        A[i, j] = A[j, i] = 1.0
    return sp.csc_matrix(A)


_CACHE = {}


def instance(family, n):
    """(data, C, As, b, constraint types) of one instance, built once."""
    if (family, n) not in _CACHE:
        A = graph(n, 7 + n)
        ct = None
        if family == "maxcut":
            C_, As, bs = problems.maxcut(A)
        elif family == "minimum_bisection":
            C_, As, bs = problems.minimum_bisection(A)
        else:
            C_, As, bs, ct = problems.mu_conductance_ineq(A, 0.05)
        _CACHE[(family, n)] = (sj.SDPData(C_, As, bs, ct), C_, As, np.asarray(bs, dtype=np.float64), ct)
    return _CACHE[(family, n)]


def state(abi, family, n, r=3):
    """A handle in the state a dual bound finds: random R (the seed's), λ and σ set, primal_vio_raw current after one fg."""
    data, _, _, _, ct = instance(family, n)
    g, _ = make_solver(abi, data, r, seed=n)
    rng = np.random.Generator(np.random.PCG64(1000 + n))
    lam = 0.3 * rng.standard_normal(data.m)
    g.λ = np.minimum(lam, g.λ_ub)
    g.σ = 3.0
    g.fg(data.normC(), float(np.linalg.norm(data.b)))
    return g


def y_formula(g):
    m = g.m
    t = g.λ - g.σ * g.primal_vio_raw[:m]
    return t, np.concatenate([-np.minimum(g.λ_ub, t), [1.0]])


def v0_of(n):
    return np.random.Generator(np.random.PCG64(77 + n)).standard_normal(n)


def host_sequence(g, tb, ncv, v0):
    """The bound as ``sdplr_steps`` ran it from the host before it became one call."""
    m = g.m
    g.y = y_formula(g)[1]
    g.At_preprocess()
    vals, matvecs, nconv = g.S_eigval(1, "SA", ncv, TOL, 100000, v0)
    return float(-(g.y[:m] @ g.b) + tb * min(vals[0], 0.0)), float(vals[0]), matvecs, nconv


def dot_bound(y, b):
    m = b.size
    return m * EPS * float(np.sum(np.abs(y[:m] * b)))


def ritz_bound(ev):
    return TOL * max(EPS ** (2.0 / 3.0), abs(ev + 1.0))


@pytest.mark.parametrize("family,n", CASES)
def test_single_call_against_the_existing_pieces(hip_abi, family, n, monkeypatch):
    data, C_, As, b, ct = instance(family, n)
    a, t = state(hip_abi, family, n), state(hip_abi, family, n)
    tval, y_host = y_formula(a)
    if ct is not None:           # min(λ_ub, ·) clips at least one inequality row and leaves at least one
        assert np.any(tval[ct] > 0.0) and np.any(tval[ct] < 0.0)
    ncv, v0, tb = min(100, n), v0_of(n), float(n)
    # the twin: sdplr_hip_dual_obj on the multi-launch path (enq_copy2y), then the eigensolve piece by piece
    monkeypatch.setenv("SDPLR_HIP_NO_FUSED_DUAL", "1")
    t.dual_obj(tb, 0, v0)
    monkeypatch.delenv("SDPLR_HIP_NO_FUSED_DUAL")
    y_t = t.y
    assert np.array_equal(y_t, y_host)
    t.At_preprocess()
    vals_t, mv_t, nc_t = t.S_eigval(1, "SA", ncv, TOL, 100000, v0)
    d0, ev0, _, _ = a.dual_obj_hp(0.0, ncv, TOL, 100000, v0)
    d1, ev, mv, nc = a.dual_obj_hp(tb, ncv, TOL, 100000, v0)
    y_a = a.y
    assert np.array_equal(y_a, y_t)
    assert np.array_equal(a.get_vec(cabi.V_S_NZVAL), t.get_vec(cabi.V_S_NZVAL))
    assert np.array_equal([ev], vals_t) and ev0 == ev and (mv, nc) == (mv_t, nc_t)
    host_dot = float(y_a[:data.m] @ b)
    print(f"{family} n={n}: ev {ev:.15e} matvecs {mv} nconv {nc} | dot err {abs(-d0 - host_dot):.3e} bound {dot_bound(y_a, b):.3e}")
    assert abs(-d0 - host_dot) <= dot_bound(y_a, b)
    assert d1 == d0 + tb * min(ev, 0.0)
    # against the definition: λ_min of the dense S that the data and y define
    if nc == 1:
        S = np.asarray(S_dense_hp(C_, As, y_a), dtype=np.float64)
        lam_min = float(np.linalg.eigvalsh(S)[0])
        ref_err = n * EPS * float(np.abs(S).sum(axis=1).max())
        print(f"    mineig − λ_min = {ev - lam_min:.3e}  (bound {ritz_bound(lam_min):.3e}, reference's own error {ref_err:.3e})")
        assert -ref_err <= ev - lam_min <= ritz_bound(lam_min)
    if n == 5:
        assert nc == 1 and mv == 5             # the Krylov space closed: no restart
    if n == 130:                               # ncv < n: thick restarts (with a basis of 20 certainly), the same iterates
        assert mv >= 100
        d2, ev2, mv2, nc2 = a.dual_obj_hp(tb, 20, TOL, 100000, v0)
        vals2, mv2_t, nc2_t = t.S_eigval(1, "SA", 20, TOL, 100000, v0)
        assert mv2 > 20 and np.array_equal([ev2], vals2) and (mv2, nc2) == (mv2_t, nc2_t)
        assert nc2 != 1 or abs(ev2 - ev) <= 2 * ritz_bound(ev)
    a.close(); t.close()


@pytest.fixture(scope="module")
def singles(hip_abi):
    """Per case what the single call leaves: (y, S.nzval, dual at tb = 0, dual at tb = n, mineig, matvecs, nconv)."""
    import os
    saved = {k: os.environ.pop(k) for k in ("SDPLR_HIP_FORCE_GRAPH", "SDPLR_HIP_NO_RESIDENT") if k in os.environ}
    try:
        out = {}
        for family, n in CASES:
            g = state(hip_abi, family, n)
            d0 = g.dual_obj_hp(0.0, min(100, n), TOL, 100000, v0_of(n))[0]
            d1, ev, mv, nc = g.dual_obj_hp(float(n), min(100, n), TOL, 100000, v0_of(n))
            out[(family, n)] = (g.y, g.get_vec(cabi.V_S_NZVAL), d0, d1, ev, mv, nc)
            g.close()
        return out
    finally:
        os.environ.update(saved)


def _requests(tb_of):
    return [(tb_of(n), min(100, n), TOL, 100000, v0_of(n)) for _, n in CASES]


def test_batch_shares_the_launches(hip_abi, singles):
    gs = [state(hip_abi, f, n) for f, n in CASES]
    twins = [state(hip_abi, f, n) for f, n in CASES]
    before = [g.stats()["resident_shared_launches"] for g in gs]
    res0 = cabi.batch_dual_obj_hp(hip_abi, gs, _requests(lambda n: 0.0))
    res = cabi.batch_dual_obj_hp(hip_abi, gs, _requests(float))
    assert all(not isinstance(x, Exception) for x in res0 + res)
    # twins prepared by the single-instance sequence, their eigenvalues by the batch eigenvalue call
    for g in twins:
        g.y = y_formula(g)[1]
        g.At_preprocess()
    eig = cabi.batch_S_eigval(hip_abi, twins, [(1, "SA", min(100, n), TOL, 100000, v0_of(n)) for _, n in CASES])
    for k, (f, n) in enumerate(CASES):
        y1, nz1, s0, s1, ev1, mv1, nc1 = singles[(f, n)]
        (d0, e0, _, _, _, route0), (d1, ev, mv, nc, y_out, route) = res0[k], res[k]
        b = instance(f, n)[3]
        assert route0 == 1 and route == 1, (f, n)
        assert np.array_equal(y_out, y1) and np.array_equal(gs[k].y, y1), (f, n)
        assert np.array_equal(twins[k].y, y1)
        gs[k].y = np.zeros(y1.size)                  # S is the bound's and is not re-assembled by whoever reads it next
        assert np.array_equal(gs[k].get_vec(cabi.V_S_NZVAL), twins[k].get_vec(cabi.V_S_NZVAL)), (f, n)
        assert np.array_equal(gs[k].get_vec(cabi.V_S_NZVAL), nz1)
        assert eig[k][3] == 1 and np.array_equal([ev], eig[k][0]) and (mv, nc) == eig[k][1:3] and e0 == ev, (f, n)
        print(f"{f} n={n}: |ev − single| {abs(ev - ev1):.3e} (bound {2 * ritz_bound(ev):.3e}) dot err "
              f"{abs(-d0 - float(y1[:b.size] @ b)):.3e} (bound {dot_bound(y1, b):.3e}) matvecs {mv} / {mv1}")
        assert nc == 1 and nc1 == 1
        assert abs(ev - ev1) <= 2 * ritz_bound(ev), (f, n)
        assert abs(-d0 - float(y1[:b.size] @ b)) <= dot_bound(y1, b), (f, n)
        assert d1 == d0 + float(n) * min(ev, 0.0), (f, n)
        assert gs[k].stats()["resident_shared_launches"] == before[k] + 2
    for g in gs + twins:
        g.close()


def test_batch_switched_off_is_the_single_call(hip_abi, singles, monkeypatch):
    gs = [state(hip_abi, f, n) for f, n in CASES]
    monkeypatch.setenv("SDPLR_HIP_NO_BATCH_EIG", "1")
    res = cabi.batch_dual_obj_hp(hip_abi, gs, _requests(float))
    for k, (f, n) in enumerate(CASES):
        y1, nz1, _, s1, ev1, mv1, nc1 = singles[(f, n)]
        d1, ev, mv, nc, y_out, route = res[k]
        assert route == 0 and (d1, ev, mv, nc) == (s1, ev1, mv1, nc1), (f, n)
        assert np.array_equal(y_out, y1) and np.array_equal(gs[k].y, y1)
        assert np.array_equal(gs[k].get_vec(cabi.V_S_NZVAL), nz1)
    for g in gs:
        g.close()


def _items(gs, ys):
    arr = (cabi.DualHpItem * len(gs))()
    for it, g, y in zip(arr, gs, ys):
        it.s = g._h.value
        it.trace_bound, it.ncv, it.tol, it.maxiter = float(g.n), 0, TOL, 100000
        it.v0 = None
        it.y_out = y.ctypes.data_as(cabi._pf64)
        it.dual_value, it.mineig, it.n_matvec, it.n_converged, it.route, it.status = 77.0, 77.0, -5, -5, 55, 55
    return arr


def test_errors_fail_alone_and_duplicates_fail_the_call(hip_abi):
    cases = [("maxcut", 64), ("minimum_bisection", 65), ("maxcut", 5)]
    gs = [state(hip_abi, f, n) for f, n in cases]
    ys = [np.full(g.m + 1, 77.0) for g in gs]
    arr = _items(gs, ys)
    arr[1].maxiter = 0
    y_before = gs[1].y
    assert hip_abi.batch_dual_obj_hp(3, arr) == cabi.ERR_INVALID_ARG
    assert [q.status for q in arr] == [0, cabi.ERR_INVALID_ARG, 0]
    assert arr[0].route == 1 and arr[2].route == 1 and arr[0].mineig != 77.0 and arr[2].n_converged == 1
    assert ys[0][-1] == 1.0 and ys[2][-1] == 1.0 and np.all(ys[1] == 77.0)
    assert np.array_equal(gs[1].y, y_before)                 # the failing item's y was not written
    res = cabi.batch_dual_obj_hp(hip_abi, gs, [(5.0, 0, TOL, 100000, None), (5.0, 0, TOL, 0, None), (5.0, 0, TOL, 100000, None)])
    assert isinstance(res[1], cabi.SdplrError) and res[1].code == cabi.ERR_INVALID_ARG
    assert not isinstance(res[0], Exception) and not isinstance(res[2], Exception)
    with pytest.raises(cabi.SdplrError):
        gs[1].dual_obj_hp(5.0, 0, TOL, 0, None)
    # a duplicate handle: the whole call, nothing written
    ys = [np.full(g.m + 1, 77.0) for g in (gs[0], gs[1], gs[0])]
    arr = _items([gs[0], gs[1], gs[0]], ys)
    assert hip_abi.batch_dual_obj_hp(3, arr) == cabi.ERR_INVALID_ARG
    assert all((q.status, q.route, q.n_matvec, q.n_converged, q.dual_value, q.mineig) == (55, 55, -5, -5, 77.0, 77.0) for q in arr)
    assert all(np.all(y == 77.0) for y in ys)
    assert hip_abi.batch_dual_obj_hp(0, None) == 0 and cabi.batch_dual_obj_hp(hip_abi, [], []) == []
    for g in gs:
        g.close()


@pytest.mark.parametrize("route", ["single", "batch"])
def test_handle_state_after_the_call(hip_abi, route):
    family, n = "maxcut", 130
    data = instance(family, n)[0]
    a, t = state(hip_abi, family, n), state(hip_abi, family, n)
    ncv, v0, tb = 100, v0_of(n), float(n)
    dt, evt, _, _ = host_sequence(t, tb, ncv, v0)
    if route == "single":
        d, ev, _, _ = a.dual_obj_hp(tb, ncv, TOL, 100000, v0)
        assert ev == evt                             # the same kernels on the same S
    else:
        d, ev, _, _, _, r1 = cabi.batch_dual_obj_hp(hip_abi, [a], [(tb, ncv, TOL, 100000, v0)])[0]
        assert r1 == 1 and abs(ev - evt) <= 2 * ritz_bound(ev)
    assert np.array_equal(a.y, t.y)
    # a following S_eigval and At_left use the bound's S as it stands (an overwritten y would show a re-assembly)
    a.y = np.zeros(n + 1)
    t.y = np.zeros(n + 1)
    assert np.array_equal(a.S_eigval(1, "SA", ncv, TOL, 100000, v0)[0], [evt])
    a.At_left(cabi.F_SCRATCH, cabi.F_RT)
    t.At_left(cabi.F_SCRATCH, cabi.F_RT)
    assert np.array_equal(a.get_factor(cabi.F_SCRATCH), t.get_factor(cabi.F_SCRATCH))
    # a following major iteration: the iterates of the twin that had the host sequence
    args = (data.normC(), float(np.linalg.norm(data.b)), True, True, False, True, 6.0, 1e-3, 1e-8, 20, 0.0)
    ra, rt = a.major_iteration(*args), t.major_iteration(*args)
    assert ra == rt and np.array_equal(a.Rt, t.Rt) and np.array_equal(a.λ, t.λ)
    a.close(); t.close()


def test_lockstep_sends_the_bounds_as_one_call(hip_abi, monkeypatch):
    datas = [problems.maxcut_data(problems.gnp_graph(64, 0.1, 30 + k)) for k in range(4)]
    kw = dict(abi=hip_abi, seed=2, printlevel=0, prior_trace_bound=64.0, eigval_highprecision=True)
    ones = [sj.sdplr(data=d, r=4, **kw) for d in datas]
    calls, eig_calls, shared = [], [], []
    real = cabi.batch_dual_obj_hp

    def counted(abi, svs, reqs):
        before = [s.stats()["resident_shared_launches"] for s in svs]
        out = real(abi, svs, reqs)
        calls.append(len(svs))
        shared.extend(s.stats()["resident_shared_launches"] - b0 for s, b0 in zip(svs, before))
        assert all(not isinstance(x, Exception) and x[5] == 1 for x in out)
        return out

    monkeypatch.setattr(cabi, "batch_dual_obj_hp", counted)
    real_eig = cabi.DeviceSolver.S_eigval
    monkeypatch.setattr(cabi.DeviceSolver, "S_eigval", lambda self, *a, **k: eig_calls.append(1) or real_eig(self, *a, **k))
    lock = batch.solve_lockstep(datas, 4, **kw)
    assert calls and not eig_calls
    assert shared and all(x == 1 for x in shared)
    for d, a, b in zip(datas, ones, lock):
        assert not isinstance(b, Exception), b
        assert a["iter"] == b["iter"] and a["majoriter"] == b["majoriter"] and np.array_equal(a["Rt"], b["Rt"])
        # the bound of the same y: the eigenvalues of two converged runs of the same test, scaled by the trace bound, and the
        # re-ordered dot product (b = 1)
        # max_dual_value = Σλ + 64·min(ev, 0) with λ = −y[1:m] of the best bound
        lam = a["lambda"][:d.m]
        ev = (a["max_dual_value"] - float(np.sum(lam))) / 64.0
        slack = 64.0 * 2 * ritz_bound(ev) + d.m * EPS * float(np.sum(np.abs(lam)))
        print(f"lockstep: max_dual_value {a['max_dual_value']:.12e} / {b['max_dual_value']:.12e} slack {slack:.3e}")
        assert abs(a["max_dual_value"] - b["max_dual_value"]) <= slack
