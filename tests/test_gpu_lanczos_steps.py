"""The Lanczos recurrence (src/coreop.jl:461-500) and the dual bound (:376-415) of the HIP library, step by step and on
every route that computes them, against a reference above FP64 (helpers.S_dense_hp, helpers.lanczos_hp; the CPU oracle
is held to the same bounds in tests/test_lanczos_reference.py).

Routes (forced with the library's environment toggles; which one ran is read from stats()):
  gather     k_lz_spmv<8> (+ k_spmv_long with hub rows) + k_lz_step, as a captured graph or eagerly
  band       k_lz_band<pal|val> (+ hub blocks) + k_lz_step_band, as a captured graph or eagerly
  resident   k_rs_lanczos_ell<true|false> on the structured instances, k_rs_lanczos on the others: one launch
  classic    run_lanczos_classic (the reference's three-kernel form; also what more than SDPLR_LRMAX low-rank columns take):
             none of the three Lanczos counters moves
  k_lz_spmv<4|16|32>: the width is read once per process, so these run in a child process each.
stats() has one counter per launch shape, not per kernel: that the palette band kernel ran (and not the value form) is
shown by its run NOT being the value form's bit for bit with 3 weights and being it with 400; which of k_rs_lanczos_ell
<true|false> and k_rs_lanczos served a resident call follows from the instance (structured with unit weights / with
RESIDENT_LZ_STREAM or weights / not structured: rs_lanczos_ell_applies, rs_lz_ell_lds) and is not observable here.

Two-step probes: lanczos(2, x) depends on S·x, one three-term step and one more S·(·) only, so it is well conditioned
(κ = 4·‖|S|‖∞/β₁ ≤ 4e3 here) however ill-conditioned a long run is, and pins the SpMV layout and both step kernels entry
by entry: x = e_j of every row moves α₂ by O(1) for a dropped or doubled entry.  Bounds: helpers.two_step_reference.

Largest error/bound ratio per route over all probes (bound = 1), measured on an MI355X; the CPU oracle, measured by
tests/test_lanczos_reference.py, in the last column.  What dominates on every side is the one rounding of each entry
y·A[i,j] of S, which the reference does not make — hence the equal figures:

  instance          gather  gather<4|16|32>  band    resident  classic  oracle
  maxcut150         0.201   0.201            0.201   0.201     0.201    0.201
  maxcut257_hubs    0.444   0.444            0.444   0.444     0.444    0.444
  wmaxcut300_w3     0.0179  -                0.0179  0.0172    0.0172   0.0282
  wmaxcut300_w400   0.0186  -                0.0186  0.0154    0.0154   0.0271
  minbis150         0.00598 0.00598          0.00598 0.00612   0.00612  0.00612
  lovasz150         0.00517 -                0.00517 0.0058    0.0058   0.0058
  lowrank60_3+6     -       -                -       -         0.0138   0.0138
  lowrank60_8       0.0126  -                -       0.0185    0.0185   0.0412
(graph replay and eager launches of one route give the same figures: they are bit-identical, test_whole_runs_on_every_route.)
Whole runs: the smallest Ritz values of all routes and the oracle lie within 2.3e-13 of each other where 2τ ≥ 1e-11.
"""
import json
import os
import subprocess
import sys

import ctypes as C
import numpy as np
import pytest

from sdplrplus_jl_amd import cabi
from helpers import (LANCZOS_INSTANCES, U53, break_instance, lanczos_gamma, lanczos_hp, lanczos_instance, make_data,
                     make_solver, set_S, two_step_max_ratio, whole_run_checks)

pytestmark = pytest.mark.gpu

TOGGLES = ["SDPLR_HIP_LZBAND_MIN_N", "SDPLR_HIP_LZBAND_BW", "SDPLR_HIP_LZBAND_CH", "SDPLR_HIP_NO_LZBAND", "SDPLR_HIP_NO_LZPAL",
           "SDPLR_HIP_HUB_THRESH", "SDPLR_HIP_CLASSIC_LANCZOS", "SDPLR_HIP_NO_RESIDENT", "SDPLR_HIP_RESIDENT_LZ_STREAM",
           "SDPLR_HIP_FORCE_GRAPH", "SDPLR_HIP_NO_GRAPH", "SDPLR_HIP_LZ_REPS", "SDPLR_HIP_NO_FUSED_DUAL"]
COUNTERS = ("resident_lanczos", "lanczos_graph_replays", "lanczos_eager_rounds")


@pytest.fixture(autouse=True)
def _routes_are_chosen_here(monkeypatch):
    for k in TOGGLES:
        monkeypatch.delenv(k, raising=False)


def _band(bw, ch):
    return {"SDPLR_HIP_LZBAND_MIN_N": "1", "SDPLR_HIP_LZBAND_BW": str(bw), "SDPLR_HIP_LZBAND_CH": str(ch)}


GRAPH = {"SDPLR_HIP_FORCE_GRAPH": "1"}
EAGER = {"SDPLR_HIP_FORCE_GRAPH": "1", "SDPLR_HIP_NO_GRAPH": "1"}
NO_BAND = {"SDPLR_HIP_NO_LZBAND": "1"}


def routes_of(name: str):
    """[(route, environment, the stats() counter that must move — None: none of the three may)]."""
    family, n, plans, hub, lowrank = LANCZOS_INSTANCES[name]
    base = {"SDPLR_HIP_HUB_THRESH": str(hub)} if hub is not None else {}
    if family == "two_lowrank":       # ST = 9 > SDPLR_LRMAX: the classic route on its own, whatever else is asked for
        return [("classic(own)/graph-env", {**GRAPH}, None), ("classic(own)/small-env", {}, None)]
    out = [("gather/graph", {**base, **GRAPH, **NO_BAND}, "lanczos_graph_replays"),
           ("gather/eager", {**base, **EAGER, **NO_BAND}, "lanczos_eager_rounds"),
           ("gather/eager(no-resident)", {**base, "SDPLR_HIP_NO_RESIDENT": "1", **NO_BAND}, "lanczos_eager_rounds")]
    for k, (bw, ch) in enumerate(plans):
        out.append((f"band{bw}x{ch}/graph", {**base, **GRAPH, **_band(bw, ch)}, "lanczos_graph_replays"))
        if k == 0:
            out.append((f"band{bw}x{ch}/eager", {**base, **EAGER, **_band(bw, ch)}, "lanczos_eager_rounds"))
        if name.startswith("wmaxcut"):
            out.append((f"band{bw}x{ch}-values/graph", {**base, **GRAPH, **_band(bw, ch), "SDPLR_HIP_NO_LZPAL": "1"},
                        "lanczos_graph_replays"))
    out.append(("resident", {**base}, "resident_lanczos"))
    if name == "maxcut150":
        out.append(("resident/stream", {**base, "SDPLR_HIP_RESIDENT_LZ_STREAM": "1"}, "resident_lanczos"))
    out.append(("classic", {**base, **GRAPH, "SDPLR_HIP_CLASSIC_LANCZOS": "1"}, None))
    return out


ALL = [(name, route, env, counter) for name in LANCZOS_INSTANCES for route, env, counter in routes_of(name)]
IDS = [f"{name}-{route}" for name, route, _, _ in ALL]


def solver_on(hip_abi, monkeypatch, inst, env, y=None):
    for k in TOGGLES:               # (again: tests that walk several routes call this once per route)
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    s_, _ = make_solver(hip_abi, inst["data"], 4, seed=3)
    return set_S(s_, inst["y"] if y is None else y)


def assert_route(s_, counter, calls=None):
    st = s_.stats()
    for c in COUNTERS:
        if c == counter:
            assert st[c] > 0 and (calls is None or c != "resident_lanczos" or st[c] == calls), (counter, st)
        else:
            assert st[c] == 0, (counter, c, st)


# ---- 2. two-step probes --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,route,env,counter", ALL, ids=IDS)
def test_two_step_probes(hip_abi, monkeypatch, name, route, env, counter):
    inst = lanczos_instance(name)
    s_ = solver_on(hip_abi, monkeypatch, inst, env)
    worst = two_step_max_ratio(inst, s_)
    assert_route(s_, counter, calls=int(inst["ref"]["live"].sum()))
    s_.close()
    print(f"two-step ratio {name} {route}: {worst:.3g}")
    assert worst <= 1.0, (name, route, worst)


_CHILD = r"""
import json, os, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import sdplrplus_jl_amd as sj
from helpers import lanczos_instance, make_solver, set_S, two_step_max_ratio
hip = sj.load_hip()
out = {}
for name in ("maxcut150", "maxcut257_hubs", "minbis150"):
    inst = lanczos_instance(name)
    s_, _ = make_solver(hip, inst["data"], 4, seed=3)
    set_S(s_, inst["y"])
    worst, probes = two_step_max_ratio(inst, s_), s_.stats()
    q, v0 = min(60, inst["n"] - 1), inst["X"][:, 0]
    al, be, k = s_.lanczos(q, v0)
    ev = s_.approx_mineigval_lanczos(q, v0)
    out[name] = dict(worst=worst, probes=probes, alpha=list(al), beta=list(be), steps=k, approx=ev,
                     ritz=s_.tridiag_mineig(al, be), stats=s_.stats())
    s_.close()
print("RESULT " + json.dumps(out))
"""
_WIDTH_RUNS = {}


def _gather_width_run(lpr):
    """One child process per width of k_lz_spmv (SDPLR_HIP_LZ_LPR is read once per process), started once per session."""
    if lpr not in _WIDTH_RUNS:
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        env = {k: v for k, v in os.environ.items() if k not in TOGGLES}
        env.update(SDPLR_HIP_LZ_LPR=str(lpr), SDPLR_HIP_FORCE_GRAPH="1", SDPLR_HIP_NO_LZBAND="1", SDPLR_HIP_HUB_THRESH="8")
        p = subprocess.run([sys.executable, "-c", _CHILD, root], env=env, capture_output=True, text=True, timeout=120)
        assert p.returncode == 0, p.stderr[-2000:]
        _WIDTH_RUNS[lpr] = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    return _WIDTH_RUNS[lpr]


@pytest.mark.parametrize("lpr", [4, 8, 16, 32])
def test_two_step_probes_and_whole_runs_on_every_gather_width(hip_abi, oracle_abi, lpr):
    """k_lz_spmv<4|8|16|32> in a child process each (what this test is about); hub rows (k_spmv_long: threshold 8 on all
    three instances) and a rank-one term ride along.  The two-step probes, and the 60-step run with the checks of
    test_whole_runs_on_every_route: containment, clustering, approx_mineigval_lanczos = tridiag_mineig, the smallest Ritz
    value within 2τ of the oracle's and of the default width's; the widths differ by the order of a row's sum only, so
    their runs are close and — the sums being reordered — need not be bit-identical."""
    res, res8 = _gather_width_run(lpr), _gather_width_run(8)
    for name, r in res.items():
        inst = lanczos_instance(name)
        q, v0 = min(60, inst["n"] - 1), inst["X"][:, 0]
        print(f"two-step ratio {name} gather<{lpr}>/graph: {r['worst']:.3g}")
        for st in (r["probes"], r["stats"]):
            assert st["lanczos_graph_replays"] > 0 and st["resident_lanczos"] == 0 and st["lanczos_eager_rounds"] == 0
        assert r["stats"]["lanczos_graph_replays"] > r["probes"]["lanczos_graph_replays"]      # the whole run's replays
        assert r["worst"] <= 1.0, (name, lpr, r["worst"])
        al, be = np.array(r["alpha"]), np.array(r["beta"])
        assert r["steps"] == q == al.size
        tau = whole_run_checks(inst, al, be, q)
        assert r["approx"] == r["ritz"]
        o, _ = make_solver(oracle_abi, inst["data"], 4, seed=3)
        set_S(o, inst["y"])
        ao, bo, ko = o.lanczos(q, v0)
        ritz_o = o.tridiag_mineig(ao, bo)
        o.close()
        assert r["ritz"] == o.tridiag_mineig(al, be)        # (the coefficients came through JSON unchanged)
        print(f"whole run {name} gather<{lpr}>: |Ritz - oracle| {abs(r['ritz'] - ritz_o):.3g}, |Ritz - width 8| "
              f"{abs(r['ritz'] - res8[name]['ritz']):.3g}, 2 tau {2 * tau:.3g}")
        assert abs(r["ritz"] - ritz_o) <= 2 * tau and abs(r["ritz"] - res8[name]["ritz"]) <= 2 * tau


# ---- 3. whole runs -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(LANCZOS_INSTANCES))
def test_whole_runs_on_every_route(hip_abi, oracle_abi, monkeypatch, name):
    """q = min(60, n − 1) steps on every route: containment and clustering of the Ritz values (helpers.whole_run_checks),
    approx_mineigval_lanczos = tridiag_mineig of the same run exactly, graph replay = eager launches bit for bit, every
    route's smallest Ritz value within 2τ of every other's and of the oracle's."""
    inst = lanczos_instance(name)
    q, v0 = min(60, inst["n"] - 1), inst["X"][:, 0]
    o, _ = make_solver(oracle_abi, inst["data"], 4, seed=3)
    set_S(o, inst["y"])
    ao, bo, ko = o.lanczos(q, v0)
    assert ko == q
    tau = whole_run_checks(inst, ao, bo, q)
    ritz = {"oracle": o.tridiag_mineig(ao, bo)}
    o.close()
    runs = {}
    for route, env, counter in routes_of(name):
        s_ = solver_on(hip_abi, monkeypatch, inst, env)
        al, be, k = s_.lanczos(q, v0)
        assert k == q, (route, k)
        assert_route(s_, counter, calls=1)
        assert whole_run_checks(inst, al, be, q) == tau
        ritz[route] = s_.tridiag_mineig(al, be)
        assert s_.approx_mineigval_lanczos(q, v0) == ritz[route], route
        runs[route] = (al, be)
        s_.close()
    for route in runs:
        if route.endswith("/graph") and route[:-6] + "/eager" in runs:      # the same kernels in the same order
            other = runs[route[:-6] + "/eager"]
            assert np.array_equal(runs[route][0], other[0]) and np.array_equal(runs[route][1], other[1]), route
    if "gather/eager(no-resident)" in runs:
        assert np.array_equal(runs["gather/eager"][0], runs["gather/eager(no-resident)"][0])
        assert np.array_equal(runs["gather/eager"][1], runs["gather/eager(no-resident)"][1])
    if name == "wmaxcut300_w3":       # the palette kernel ran: another summation order than the value form's, so not its bits
        assert not (np.array_equal(runs["band128x40/graph"][0], runs["band128x40-values/graph"][0]) and
                    np.array_equal(runs["band128x40/graph"][1], runs["band128x40-values/graph"][1]))
    if name == "wmaxcut300_w400":     # more than 255 weights: the palette plan falls back to the value form
        assert np.array_equal(runs["band128x40/graph"][0], runs["band128x40-values/graph"][0])
        assert np.array_equal(runs["band128x40/graph"][1], runs["band128x40-values/graph"][1])
    lo, hi = min(ritz.values()), max(ritz.values())
    print(f"whole run {name}: tau {tau:.3g}, Ritz spread {hi - lo:.3g}")
    assert hi - lo <= 2 * tau, (ritz, tau)


def _dual_expected(s_, data, y, lam, trace_bound):
    ld = np.longdouble
    m = data.m
    yb = y[:m].astype(ld) * data.b.astype(ld)
    return float(-np.sum(yb) + ld(trace_bound) * min(ld(lam), ld(0))), 4 * m * U53 * float(np.sum(np.abs(yb)))


@pytest.mark.parametrize("form", ["fused", "no_fused", "launches"])
@pytest.mark.parametrize("name", ["maxcut150", "minbis150"])
def test_dual_obj_value(hip_abi, monkeypatch, name, form):
    """dual_obj = −⟨y[:m], b⟩ + trace_bound·min(λ, 0) (src/coreop.jl:412) of the λ it returns and the y it leaves, summed
    above FP64, to 4·m·u·Σ|yᵢbᵢ|; λ itself is the smallest Ritz value of q = 2⌈√max(iter,100)·ln n⌉ ≤ n − 1 steps on the
    S of that y; the three forms agree on λ exactly where they run the same recurrence."""
    inst = lanczos_instance(name)
    data, n, v0 = inst["data"], inst["n"], inst["X"][:, 1]
    env = {"fused": {}, "no_fused": {"SDPLR_HIP_NO_FUSED_DUAL": "1"}, "launches": {**GRAPH, **NO_BAND}}[form]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    s_, _ = make_solver(hip_abi, data, 4, seed=3)
    s_.f()
    for n_call, it in enumerate((0, 100, 10 ** 4), 1):
        q = min(int(2 * np.ceil(np.sqrt(max(it, 100)) * np.log(n))), n - 1)
        assert q == (n - 1 if it == 10 ** 4 else 102)       # n = 150: 2⌈10·ln 150⌉ = 102, 2⌈100·ln 150⌉ = 1004 → n − 1
        dv, lam = s_.dual_obj(float(n), it, v0)
        y = s_.y.copy()
        want, tol = _dual_expected(s_, data, y, lam, float(n))
        assert abs(dv - want) <= tol, (form, it, dv, want, tol)
        st = s_.stats()
        if form == "launches":
            assert st["lanczos_graph_replays"] > 0 and st["resident_lanczos"] == 0
        else:
            assert st["lanczos_graph_replays"] == 0 and st["lanczos_eager_rounds"] == 0
        al, be, k = s_.lanczos(q, v0)        # the same route on the S(y) the call left
        # (fused: the tridiagonal's smallest eigenvalue by multisection on the device — test_resident_lanczos_and_dual_obj
        # pins it to the host's bisection bit for bit on its instances; here to the bisection's own resolution)
        assert k == q and abs(s_.tridiag_mineig(al, be) - lam) <= (0.0 if form != "fused" else 4 * U53 * max(1.0, abs(lam)))
        if form != "launches":
            assert s_.stats()["resident_lanczos"] == 2 * n_call
    s_.close()


def test_batch_dual_obj_value(hip_abi, monkeypatch):
    """sdplr_hip_batch_dual_obj on three instances of different size and family: each item's value against its own λ and
    the y that comes back with it, and against the single call on a second handle in the same state."""
    insts = [lanczos_instance("maxcut257_hubs")["data"], lanczos_instance("minbis150")["data"],
             make_data("lovasz_theta", 3, 30, 0.3)[0]]
    for it in (0, 100, 10 ** 4):
        solvers, twins, args = [], [], []
        for k, data in enumerate(insts):
            for group in (solvers, twins):
                s_, _ = make_solver(hip_abi, data, 4, seed=3 + k)
                s_.f()
                group.append(s_)
            v0 = np.random.Generator(np.random.PCG64(70 + k)).standard_normal(data.n)
            args.append((float(data.n), it, v0))
        res = cabi.batch_dual_obj(hip_abi, solvers, args)
        for k, (data, out) in enumerate(zip(insts, res)):
            assert not isinstance(out, Exception), out
            dv, lam, y = out
            assert np.array_equal(y, solvers[k].y)
            want, tol = _dual_expected(solvers[k], data, y, lam, float(data.n))
            assert abs(dv - want) <= tol, (k, it, dv, want, tol)
            d1, l1 = twins[k].dual_obj(*args[k])
            assert (d1, l1) == (dv, lam), (k, it)
        for k in (0, 1):       # the two structured instances shared one launch of the batch kernel
            st = solvers[k].stats()
            assert st["resident_lanczos"] == 1 and st["resident_shared_launches"] == 1, st
        for s_ in solvers + twins:
            s_.close()


# ---- 4. step counts and exits --------------------------------------------------------------------------------------------
STEP_ROUTES = [("gather", {**GRAPH, **NO_BAND}, "lanczos_graph_replays"),
               ("band/reps1", {**GRAPH, **_band(64, 16), "SDPLR_HIP_LZ_REPS": "1"}, "lanczos_graph_replays"),
               ("band/reps2", {**GRAPH, **_band(64, 16), "SDPLR_HIP_LZ_REPS": "2"}, "lanczos_graph_replays"),
               ("resident", {}, "resident_lanczos")]
STEP_IDS = [r[0] for r in STEP_ROUTES]
SENTINEL = -7.25e300


def raw_lanczos(s_, q, v0, pad=8):
    """sdplr_hip_lanczos on sentinel-filled arrays → (rc, α, β, steps): what the call left in ALL of both arrays."""
    v0 = np.ascontiguousarray(v0, dtype=np.float64)
    al, be = np.full(max(q, 1) + pad, SENTINEL), np.full(max(q, 1) + pad, SENTINEL)
    st = C.c_int64(-1)
    pd = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    rc = s_.abi.lanczos(s_._h, int(q), pd(v0), pd(al), pd(be), C.byref(st))
    return int(rc), al, be, int(st.value)


@pytest.mark.parametrize("route,env,counter", STEP_ROUTES, ids=STEP_IDS)
def test_step_counts(hip_abi, monkeypatch, route, env, counter):
    """Every q around the rounding of ⌈(q + 1)/3⌉ rotations, the graph's length (3·reps steps) and the cap n − 1: steps =
    min(q, n − 1), the coefficients are the first ones of the longest run bit for bit, nothing past them is touched."""
    inst = lanczos_instance("maxcut150")
    n, v0 = inst["n"], inst["X"][:, 2]
    s_ = solver_on(hip_abi, monkeypatch, inst, env)
    rc, a_full, b_full, k_full = raw_lanczos(s_, n - 1, v0)
    assert rc == cabi.OK and k_full == n - 1
    for q in (1, 2, 3, 4, 5, 6, 7, 23, 24, 25, 148, 149, 150, 1000):
        rc, al, be, k = raw_lanczos(s_, q, v0)
        assert rc == cabi.OK and k == min(q, n - 1), (q, k)
        assert np.array_equal(al[:k], a_full[:k]) and np.array_equal(be[:k], b_full[:k]), q
        assert np.all(al[k:] == SENTINEL) and np.all(be[k:] == SENTINEL), q
    assert_route(s_, counter)
    rc, al, be, k = raw_lanczos(s_, 0, v0)
    assert rc == cabi.ERR_INVALID_ARG and np.all(al == SENTINEL) and np.all(be == SENTINEL)
    s_.close()


def test_single_row_instance_is_refused(hip_abi, monkeypatch):
    """n = 1: q is clipped to n − 1 = 0 steps (src/coreop.jl:465), which the library refuses with SDPLR_ERR_INVALID_ARG."""
    import scipy.sparse as sp
    import sdplrplus_jl_amd as sj
    from sdplrplus_jl_amd import problems
    monkeypatch.setenv("SDPLR_HIP_FORCE_GRAPH", "1")
    C_, As, bs = problems.maxcut(sp.csc_matrix((1, 1)))
    s_, _ = make_solver(hip_abi, sj.SDPData(C_, As, bs), 2, seed=1)
    rc, al, be, k = raw_lanczos(s_, 3, np.ones(1))
    assert rc == cabi.ERR_INVALID_ARG and np.all(al == SENTINEL) and np.all(be == SENTINEL)
    s_.close()


@pytest.mark.parametrize("route,env,counter", STEP_ROUTES, ids=STEP_IDS)
def test_exact_break(hip_abi, monkeypatch, route, env, counter):
    """helpers.break_instance: an eigenvector as start vector breaks at step 1, e₃ — a 2-dimensional invariant subspace — at
    step 2: inside a rotation of the three buffers, inside the captured graph, inside the resident loop.  Steps and values
    against lanczos_hp; a generic start vector on the same handle afterwards runs all its steps (lz_done is reset)."""
    data, y, S = break_instance(150)
    n = data.n
    A = float(np.max(np.sum(np.abs(S), axis=1)))
    g = lanczos_gamma(S, False)
    e = np.eye(n)
    inst = dict(data=data, y=y)
    s_ = solver_on(hip_abi, monkeypatch, inst, env)
    generic = np.random.Generator(np.random.PCG64(8)).standard_normal(n)
    for x in (e[3] + e[4], e[3] - e[4], e[3], e[7]):
        ah, bh, kh, _ = lanczos_hp(S, x, 6)
        rc, al, be, k = raw_lanczos(s_, 6, x)
        assert rc == cabi.OK and k == kh, (x[:6], k, kh)
        assert np.all(np.abs(al[:k] - np.asarray(ah, dtype=float)) <= g * A)
        assert np.all(np.abs(be[:k - 1] - np.asarray(bh[:k - 1], dtype=float)) <= g * A)
        assert abs(be[k - 1]) <= np.sqrt(n) * np.finfo(float).eps * A
        # the call copies q entries back: behind the k steps taken the zeros both arrays are cleared to, behind q nothing
        assert np.all(al[k:6] == 0.0) and np.all(be[k:6] == 0.0)
        assert np.all(al[6:] == SENTINEL) and np.all(be[6:] == SENTINEL)
        al, be, k = s_.lanczos(6, generic)
        assert k == 6 and np.all(be > 1e-6 * A)
    assert_route(s_, counter)
    s_.close()


@pytest.mark.parametrize("name,route,env,counter",
                         [a for a in ALL if a[0] in ("maxcut150", "minbis150", "lowrank60_8", "lowrank60_3+6")],
                         ids=[i for a, i in zip(ALL, IDS) if a[0] in ("maxcut150", "minbis150", "lowrank60_8", "lowrank60_3+6")])
def test_power_of_two_scaling(hip_abi, oracle_abi, monkeypatch, name, route, env, counter):
    """y·2^±40 scales S, hence every α and β, by exactly 2^±40: a power of two commutes with every rounding of the
    recurrence.  y·2⁻⁶⁰ puts β₁ under the ABSOLUTE threshold √n·ε of :494: one step, as on the oracle."""
    inst = lanczos_instance(name)
    v0, q = inst["X"][:, 3], 12
    s_ = solver_on(hip_abi, monkeypatch, inst, env)
    a0, b0, k0 = s_.lanczos(q, v0)
    assert k0 == q
    for p in (40, -40):
        set_S(s_, inst["y"] * 2.0 ** p)
        a1, b1, k1 = s_.lanczos(q, v0)
        assert k1 == q and np.array_equal(a1, a0 * 2.0 ** p) and np.array_equal(b1, b0 * 2.0 ** p), (route, p)
    set_S(s_, inst["y"] * 2.0 ** -60)
    o, _ = make_solver(oracle_abi, inst["data"], 4, seed=3)
    set_S(o, inst["y"] * 2.0 ** -60)
    assert s_.lanczos(q, v0)[2] == o.lanczos(q, v0)[2] == 1
    assert_route(s_, counter)
    o.close(); s_.close()
