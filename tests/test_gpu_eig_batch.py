"""GPU tests of sdplr_hip_batch_S_eigval (include/sdplr_hip_eig_batch.h, sdplrplus.jl_amd/csrc/k_eig_resident.h): the
thick-restart Lanczos of sdplr_hip_S_eigval with one workgroup per instance, a whole batch in one launch.

S comes from a short solve (fg, a few inner iterations, dual_obj); the reference is numpy's dense ``eigvalsh`` of the S that
C, the constraint matrices and the device's y define.  The bound is the project's own (tests/test_gpu_baseline_sizes.py):
1e-8·max(|ref₀|, ‖S‖∞) — a hundred times the residual the convergence test admits at tol = 1e-10."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

import sdplrplus_jl_amd as sj
from sdplrplus_jl_amd import batch, cabi, problems

from helpers import S_dense_hp, make_solver

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-10


@pytest.fixture(autouse=True)
def _small_instances_take_their_own_route(monkeypatch):
    monkeypatch.delenv("SDPLR_HIP_FORCE_GRAPH", raising=False)
    monkeypatch.delenv("SDPLR_HIP_NO_RESIDENT", raising=False)
    for k in ("SDPLR_HIP_NO_BATCH_EIG", "SDPLR_HIP_BATCH_EIG_NMAX", "SDPLR_HIP_BATCH_EIG_CYCLES"):
        monkeypatch.delenv(k, raising=False)


def graph(n, p, seed):
    """G(n, p) plus the cycle 0-1-…-(n−1)-0: every degree ≥ 1 (n ≥ 2), unit weights."""
    if n == 1:
        return sp.csc_matrix((1, 1))
    A = sp.lil_matrix(problems.gnp_graph(n, p, seed))
    for i in range(n):
        j = (i + 1) % n
        if i != j:
            A[i, j] = A[j, i] = 1.0
    return sp.csc_matrix(A)


FAMILY = {"maxcut": problems.maxcut, "minimum_bisection": problems.minimum_bisection, "cutnorm": problems.cutnorm,
          "lovasz_theta": problems.lovasz_theta}
_CACHE = {}


def instance(family, n, seed=5):
    """(data, C, As) of one instance, built once."""
    key = (family, n, seed)
    if key not in _CACHE:
        if family == "cutnorm":
            rng = np.random.Generator(np.random.PCG64(seed))
            M = sp.csc_matrix((rng.random((n // 2, n // 2)) < 0.3) * 1.0 + sp.eye(n // 2))     # every row and column has an entry
            C_, As, bs = problems.cutnorm(M)
        else:
            C_, As, bs = FAMILY[family](graph(n, min(1.0, 6.0 / max(n, 2)), seed))
        _CACHE[key] = (sj.SDPData(C_, As, bs), C_, As)
    return _CACHE[key]


def solved(hip_abi, family, n, r=4, seed=5, iters=3):
    """A handle whose S is current after a short solve → (solver, dense S in FP64)."""
    data, C_, As = instance(family, n, seed)
    g, _ = make_solver(hip_abi, data, r, seed=seed)
    normC, normb = data.normC(), float(np.linalg.norm(data.b))
    st = g.fg(normC, normb)
    if iters and data.n >= 2:
        g.inner_loop(normC, normb, True, True, False, 0.0, -1e300, iters, 0.0, *st)
    if data.n >= 2:
        g.dual_obj(float(data.n), 0, np.ones(data.n))
    else:                                       # (the dual bound's Lanczos needs n ≥ 2: y as copy2y_λ! sets it)
        g.y = np.concatenate([-g.λ, [1.0]])
    g.At_preprocess()
    return g, np.asarray(S_dense_hp(C_, As, g.y), dtype=np.float64)


def bound(S, ref):
    return 1e-8 * max(abs(ref[0]), float(np.abs(S).sum(axis=1).max()))


def wanted(S, nev, which):
    lam = np.linalg.eigvalsh(S)
    return lam[:nev] if which == "SA" else lam[::-1][:nev]


def one(hip_abi, g, req):
    res = cabi.batch_S_eigval(hip_abi, [g], [req])[0]
    assert not isinstance(res, Exception), res
    return res


@pytest.mark.parametrize("family,n,nev,which", [
    ("maxcut", 1, 1, "SA"), ("maxcut", 2, 1, "SA"), ("maxcut", 63, 1, "SA"), ("maxcut", 64, 2, "SA"), ("maxcut", 65, 5, "SA"),
    ("maxcut", 300, 1, "SA"), ("maxcut", 513, 1, "SA"), ("maxcut", 800, 1, "SA"), ("maxcut", 300, 2, "LA"),
    ("minimum_bisection", 300, 1, "SA"), ("minimum_bisection", 300, 5, "LA"), ("cutnorm", 120, 2, "SA"),
    ("lovasz_theta", 60, 1, "SA"), ("lovasz_theta", 60, 2, "LA")])
def test_eigenvalues_against_dense_eigvalsh(hip_abi, family, n, nev, which):
    g, S = solved(hip_abi, family, n)
    ref = wanted(S, nev, which)
    vals, matvecs, nconv, route = one(hip_abi, g, (nev, which, 0, TOL, 1000, None))
    err = float(np.max(np.abs(vals - ref)))
    print(f"{family} n={n} nev={nev} {which}: err {err:.3e} bound {bound(S, ref):.3e} matvecs {matvecs}")
    assert route == 1 and nconv == nev
    assert err <= bound(S, ref), (vals, ref)
    g.close()


def test_krylov_space_closes(hip_abi):
    # n ≤ ncv: the basis spans everything, all n eigenvalues
    g, S = solved(hip_abi, "maxcut", 12)
    vals, _, nconv, route = one(hip_abi, g, (12, "SA", 100, TOL, 1000, None))
    ref = np.linalg.eigvalsh(S)
    assert route == 1 and nconv == 12 and np.max(np.abs(vals - ref)) <= bound(S, ref)
    g.close()
    # S diagonal (an empty graph): S = Diag(y) — and three distinct eigenvalues: the early-β exit, exact values
    n = 40
    data = sj.SDPData(*problems.maxcut(sp.csc_matrix((n, n))))
    for y in (np.concatenate([np.arange(1.0, n + 1), [1.0]]), np.concatenate([np.repeat([2.0, 3.0, 5.0], [10, 10, 20]), [1.0]])):
        g, _ = make_solver(hip_abi, data, 2, seed=1)
        g.y = y
        g.At_preprocess()
        lam = np.sort(y[:n])
        nev = 3
        vals, matvecs, nconv, route = one(hip_abi, g, (nev, "SA", 100, TOL, 1000, None))   # m = n, or β₃ at round-off
        assert route == 1 and nconv == nev
        assert np.max(np.abs(vals - np.unique(lam)[:nev])) <= 1e-8 * np.max(np.abs(lam)), (vals, lam[:nev])
        g.close()


def test_restarts_are_independent_of_the_launch_cap(hip_abi, monkeypatch):
    g, S = solved(hip_abi, "maxcut", 300)
    req = (1, "SA", 8, TOL, 100000, None)
    a = one(hip_abi, g, req)
    monkeypatch.setenv("SDPLR_HIP_BATCH_EIG_CYCLES", "1")
    b = one(hip_abi, g, req)
    ref = wanted(S, 1, "SA")
    print("restarts: matvecs", a[1], "err", abs(a[0][0] - ref[0]), "bound", bound(S, ref))
    assert a[1] > 3 * 8                       # several cycles: the second run took several launches
    assert a[3] == b[3] == 1 and a[2] == b[2] == 1
    assert np.array_equal(a[0], b[0]) and a[1] == b[1]
    assert abs(a[0][0] - ref[0]) <= bound(S, ref)
    g.close()


def test_budget_exhausted(hip_abi):
    g, S = solved(hip_abi, "maxcut", 300)
    vals, matvecs, nconv, route = one(hip_abi, g, (2, "SA", 5, TOL, 1, None))
    lam = np.linalg.eigvalsh(S)
    assert route == 1 and nconv < 2 and matvecs == 5
    assert np.all(np.isfinite(vals)) and np.all(vals >= lam[0] - bound(S, lam)) and np.all(vals <= lam[-1] + bound(S, lam))
    g.close()


def test_results_do_not_depend_on_the_batch(hip_abi):
    mix = [("maxcut", 63, 3, 1), ("minimum_bisection", 300, 4, 2), ("cutnorm", 120, 5, 1), ("maxcut", 513, 8, 1),
           ("lovasz_theta", 60, 4, 1), ("maxcut", 65, 2, 5), ("maxcut", 64, 6, 2), ("maxcut", 12, 2, 1)]
    others = [solved(hip_abi, f, n, r=r)[0] for f, n, r, _ in mix]
    oreq = [(nev, "SA", 0, TOL, 1000, None) for *_, nev in mix]
    me, S = solved(hip_abi, "maxcut", 300)
    req = (2, "SA", 20, TOL, 1000, None)
    alone = one(hip_abi, me, req)
    assert alone[3] == 1 and alone[2] == 2
    runs = []
    for pos in (0, 3, 8, 8):
        svs, reqs = list(others), list(oreq)
        svs.insert(pos, me)
        reqs.insert(pos, req)
        res = cabi.batch_S_eigval(hip_abi, svs, reqs)
        assert all(not isinstance(x, Exception) and x[3] == 1 for x in res)
        assert np.array_equal(res[pos][0], alone[0]) and res[pos][1:] == alone[1:]
        runs.append(res)
    for x, y in zip(runs[2], runs[3]):       # two runs of the whole batch
        assert np.array_equal(x[0], y[0]) and x[1:] == y[1:]
    for s in others + [me]:
        s.close()


def test_totality_and_routes(hip_abi, monkeypatch):
    gs = [solved(hip_abi, "maxcut", n)[0] for n in (63, 300, 65)]
    reqs = [(1, "SA", 0, TOL, 1000, None), (2, "SA", 30, TOL, 1000, None), (1, "LA", 0, TOL, 1000, None)]
    singles = [g.S_eigval(*q) for g, q in zip(gs, reqs)]
    monkeypatch.setenv("SDPLR_HIP_BATCH_EIG_NMAX", "100")          # n = 300 is not taken
    res = cabi.batch_S_eigval(hip_abi, gs, reqs)
    assert [x[3] for x in res] == [1, 0, 1]
    assert np.array_equal(res[1][0], singles[1][0]) and res[1][1:3] == singles[1][1:]
    monkeypatch.delenv("SDPLR_HIP_BATCH_EIG_NMAX")
    monkeypatch.setenv("SDPLR_HIP_NO_BATCH_EIG", "1")
    res = cabi.batch_S_eigval(hip_abi, gs, reqs)
    for x, s1 in zip(res, singles):
        assert x[3] == 0 and np.array_equal(x[0], s1[0]) and x[1:3] == s1[1:]
    monkeypatch.delenv("SDPLR_HIP_NO_BATCH_EIG")
    gs[2].profile_enable(True)                                       # per-kernel profiling: that item alone
    res = cabi.batch_S_eigval(hip_abi, gs, reqs)
    assert [x[3] for x in res] == [1, 1, 0]
    gs[2].profile_enable(False)
    for g in gs:
        g.close()
    monkeypatch.setenv("SDPLR_HIP_FORCE_GRAPH", "1")                 # the suite's default: every instance a "large" one
    gs = [solved(hip_abi, "maxcut", n)[0] for n in (63, 65)]
    res = cabi.batch_S_eigval(hip_abi, gs, reqs[:2])
    assert [x[3] for x in res] == [0, 0]
    for g in gs:
        g.close()


def _items(gs, nev=1):
    arr = (cabi.EigItem * len(gs))()
    outs = [np.full(max(nev, 1), 77.0) for _ in gs]
    for it, g, o in zip(arr, gs, outs):
        it.s = g._h.value if g is not None else None
        it.nev, it.which, it.ncv, it.tol, it.maxiter = nev, 0, 0, TOL, 1000
        it.evals = o.ctypes.data_as(cabi._pf64)
        it.n_matvec, it.n_converged, it.route, it.status = -5, -5, 55, 55
    return arr, outs


def test_errors_fail_alone(hip_abi):
    gs = [solved(hip_abi, "maxcut", n)[0] for n in (63, 64, 65, 12)]
    data, *_ = instance("maxcut", 12)
    raw = sj.DeviceSolver(hip_abi, data.n, data.m, 2, 4)              # never finalized
    arr, outs = _items(gs + [raw])
    arr[1].nev = 0
    arr[2].evals = None
    rc = hip_abi.batch_S_eigval(len(arr), arr)
    assert rc == cabi.ERR_INVALID_ARG
    assert [q.status for q in arr] == [0, cabi.ERR_INVALID_ARG, cabi.ERR_INVALID_ARG, 0, cabi.ERR_STATE]
    assert arr[0].route == 1 and arr[3].route == 1 and outs[0][0] != 77.0 and outs[3][0] != 77.0
    # a duplicate handle: the whole call, nothing written
    arr, outs = _items([gs[0], gs[1], gs[0]])
    assert hip_abi.batch_S_eigval(3, arr) == cabi.ERR_INVALID_ARG
    assert all((q.status, q.route, q.n_matvec, q.n_converged) == (55, 55, -5, -5) for q in arr)
    assert all(o[0] == 77.0 for o in outs)
    assert hip_abi.batch_S_eigval(0, None) == 0 and cabi.batch_S_eigval(hip_abi, [], []) == []
    raw.close()
    for g in gs:
        g.close()


def test_solver_state_is_untouched(hip_abi):
    twins = [solved(hip_abi, "maxcut", 300, r=6, seed=9)[0] for _ in range(2)]
    a, b = twins
    before = (a.Rt.copy(), a.λ.copy(), a.y.copy(), a.Gt.copy())
    assert one(hip_abi, a, (1, "SA", 0, TOL, 1000, None))[3] == 1
    for x, z in zip(before, (a.Rt, a.λ, a.y, a.Gt)):
        assert np.array_equal(x, z)
    data, *_ = instance("maxcut", 300, 9)
    normC, normb = data.normC(), float(np.linalg.norm(data.b))
    args = (normC, normb, True, True, False, True, 4.0, 1e-3, 1e-8, 20, 0.0)
    ra, rb = a.major_iteration(*args), b.major_iteration(*args)
    assert ra == rb and np.array_equal(a.Rt, b.Rt) and np.array_equal(a.λ, b.λ)
    a.close(); b.close()


def test_lockstep_certificate_is_one_call(hip_abi, monkeypatch):
    datas = [problems.maxcut_data(graph(100, 0.06, 40 + k)) for k in range(6)]
    kw = dict(abi=hip_abi, seed=2, printlevel=0, eval_DIMACS_errs=True)
    ones = [sj.sdplr(data=d, r=5, **kw) for d in datas]
    calls = []
    real = cabi.batch_S_eigval
    monkeypatch.setattr(cabi, "batch_S_eigval", lambda abi, svs, reqs: calls.append(len(svs)) or real(abi, svs, reqs))
    lock = batch.solve_lockstep(datas, 5, **kw)
    assert calls == [6]
    for d, a, b in zip(datas, ones, lock):
        assert a["iter"] == b["iter"] and a["obj"] == b["obj"]
        assert np.array_equal(a["Rt"], b["Rt"]) and np.array_equal(a["lambda"], b["lambda"])
        ea, eb = a["DIMACS_errs"], b["DIMACS_errs"]
        assert np.array_equal(ea[[0, 1, 2, 4, 5]], eb[[0, 1, 2, 4, 5]])
        # S = C − Diag(λ): its off-diagonal is C's, so ‖S‖∞ ≥ the largest off-diagonal row sum of |C| (a bound never above
        # the issue's scale max(|λ_min|, ‖S‖∞), whatever the final λ)
        Cd = sp.csr_matrix(d.C)
        scale = float(abs(Cd - sp.diags(Cd.diagonal())).sum(axis=1).max())
        assert abs(ea[3] - eb[3]) <= 1e-8 * scale / (1.0 + d.normC()), (ea[3], eb[3])
    off = batch.solve_lockstep(datas, 5, abi=hip_abi, seed=2, printlevel=0)
    assert calls == [6]
    for a, b in zip(ones, off):
        assert np.array_equal(a["Rt"], b["Rt"]) and a["iter"] == b["iter"] and not b["DIMACS_errs"].any()


def test_c_example_runs_on_the_device(tmp_path, hip_abi):
    ldir = os.path.join(ROOT, "sdplrplus.jl_amd", "lib")
    exe = tmp_path / "batch_eig_hip"
    subprocess.check_call(["gcc", "-O2", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "batch_eig_c_abi.c"),
                           "-L", ldir, "-lsdplr_hip", "-lm", f"-Wl,-rpath,{ldir}", "-Wl,-rpath-link,/opt/rocm/lib", "-o", str(exe)])
    env = {k: v for k, v in os.environ.items() if k not in ("SDPLR_HIP_FORCE_GRAPH", "SDPLR_HIP_NO_RESIDENT")}
    out = subprocess.run([str(exe), "5"], capture_output=True, text=True, timeout=120, env=env)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip().endswith("OK")
    # instance k of the example: the circulant graph C_n(1..d), y = (1, …, 1; 1): S = I + C, the same S through Python
    rows = [ln.split() for ln in out.stdout.splitlines() if ln.startswith("instance")]
    assert len(rows) == 5
    for row in rows:
        n, d, lam_c = int(row[row.index("n") + 2]), int(row[row.index("d") + 2]), float(row[row.index("lambda_min") + 2])
        edges = np.array([(j, (j + t) % n) for j in range(n) for t in range(1, d + 1)])
        data = problems.maxcut_data(problems.graph_from_edges(n, edges))
        g, _ = make_solver(hip_abi, data, 2, seed=0)
        g.y = np.ones(n + 1)
        g.At_preprocess()
        vals, _, nconv, route = one(hip_abi, g, (1, "SA", 0, TOL, 1000, None))
        assert route == 1 and nconv == 1
        assert abs(vals[0] - lam_c) <= 1e-8 * max(abs(vals[0]), 1.0 + d)      # ‖S‖∞ ≤ 1 + d
        g.close()
