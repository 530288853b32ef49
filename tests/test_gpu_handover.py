"""Hand-overs: what one handle carries from one call to the next when the calls do not take the same route, when a loop
leaves through the line search's "not a descent direction" error, and when one call carries the gradient forward for
hundreds of iterations.

A  the error exit (src/linesearch.jl:60-62) on every route of the inner loop: the state it leaves is the oracle's — R and G
   untouched, y_next = −G parked in the slot lbfgs_dir! had claimed (src/lbfgs.jl:121-123) — and the handle carries on.
B  one handle moved between the multi-launch route (history in ring form, k_dense.h), the resident loop (k_resident.h) and
   the resident group launch of batch_major_iteration, in production mode (no SDPLR_HIP_FORCE_GRAPH).
C  G carried forward by G_new = G_old + 2(αW + d∘R − d′∘R′) (k_sparse.h) for 512 and 1000 iterations in one call, against a
   gradient evaluated above FP64 (helpers.hp_gradient); the second run ends in the stalled regime (α = 0, s = y = 0).
D  the refresh by age (SDPLR_HIP_P_REFRESH_ITERS) falls due between calls of their own and never in a resumed loop.

The oracle halves of A and C are pinned without a GPU in test_oracle_endtoend.py."""
import sys

import numpy as np
import pytest

from helpers import (carry_bound, history_state, hp_gradient, long_carry_instance, make_solver, not_descent_instance,
                     oracle_moving_iterations, same_state)
from sdplrplus_jl_amd import cabi, problems

pytestmark = pytest.mark.gpu

H = 4


def rel(a, b):
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(np.asarray(b)), 1e-300))


def loop(s_, nC, nb, k, st, fprec=-1e300):
    return s_.inner_loop(nC, nb, True, True, False, 0.0, fprec, k, 0.0, *st[:3])


def delta(after, before):
    return {k: after[k] - before[k] for k in after}


# ---- A: the not-descent exit --------------------------------------------------------------------------------------------
def _not_descent_calls(s_, nC, nb, k1, failing_call=None):
    """fg → k1 iterations → look → G ← −G → a loop of 5 (raises) → look → fg → 5 iterations → look."""
    st = s_.fg(nC, nb)
    out1 = loop(s_, nC, nb, k1, st)
    G = s_.get_factor(cabi.F_GT)                # the look: a ring is turned back into the stored form here
    s_.set_factor(cabi.F_GT, -G)
    R_before = s_.Rt
    with pytest.raises(cabi.SdplrError) as ei:
        if failing_call is None:
            loop(s_, nC, nb, 5, out1)
        else:
            failing_call(out1)
    after_error = history_state(s_, H)
    after_error["lam"] = s_.λ
    out2 = loop(s_, nC, nb, 5, s_.fg(nC, nb))
    at_end = history_state(s_, H)
    return dict(out1=out1, code=ei.value.code, msg=str(ei.value), R_before=R_before, G_written=-G, after_error=after_error,
                out2=out2, at_end=at_end)


def _check_not_descent(run, ora):
    assert run["code"] == cabi.ERR_NOT_DESCENT and "cubic[1]" in run["msg"]
    e, oe = run["after_error"], ora["after_error"]
    assert np.array_equal(e["R"], run["R_before"])
    assert rel(e["R"], oe["R"]) < 1e-8 and rel(e["G"], oe["G"]) < 1e-7
    for j in range(H):
        assert rel(e["S"][j], oe["S"][j]) < 1e-7, ("s", j)
        assert rel(e["Y"][j], oe["Y"][j]) < 1e-7, ("y", j)
    assert np.allclose(e["rho"], oe["rho"], rtol=1e-6)
    assert rel(e["lam"], oe["lam"]) < 1e-12 and rel(e["y"], oe["y"]) < 1e-8
    assert run["out2"][4] == ora["out2"][4] == 5 and run["out2"][5] == ora["out2"][5]
    assert np.allclose(run["out2"][:3], ora["out2"][:3], rtol=1e-8)
    assert rel(run["at_end"]["R"], ora["at_end"]["R"]) < 1e-8


def _same_run(a, b, dirt_after_error=True):
    assert a["out1"] == b["out1"] and a["out2"] == b["out2"]
    x, z = a["after_error"], b["after_error"]
    if not dirt_after_error:     # (the refused direction itself: not part of what the issue of these tests compares)
        x, z = dict(x, D=None), dict(z, D=None)
    same_state(x, z)
    same_state(a["at_end"], b["at_end"])


@pytest.mark.parametrize("k1", [6, 9])
def test_not_descent_exit_on_the_multi_launch_routes(hip_abi, oracle_abi, monkeypatch, k1):
    """Ring form (default), stored form (SDPLR_HIP_NO_RING), eager launches (SDPLR_HIP_NO_GRAPH): status, R untouched,
    everything readable equal to the oracle's right after the error and after fg! + 5 more iterations; ring ≡ stored ≡
    eager bitwise.  k1 = 6: the first ring has passed h pairs; 9: it has wrapped (h + 1 positions) before the look."""
    data, r, seed = not_descent_instance("launches")
    nC, nb = data.normC(), float(np.linalg.norm(data.b))
    o, _ = make_solver(oracle_abi, data, r, seed=seed, h=H)
    ora = _not_descent_calls(o, nC, nb, k1)
    o.close()
    runs, stats = {}, {}
    for variant, env in (("ring", None), ("stored", "SDPLR_HIP_NO_RING"), ("eager", "SDPLR_HIP_NO_GRAPH")):
        if env:
            monkeypatch.setenv(env, "1")
        g, _ = make_solver(hip_abi, data, r, seed=seed, h=H)
        runs[variant] = _not_descent_calls(g, nC, nb, k1)
        stats[variant] = g.stats()
        g.close()
        if env:
            monkeypatch.delenv(env)
    for variant in ("stored", "ring", "eager"):
        _check_not_descent(runs[variant], ora)
    _same_run(runs["ring"], runs["stored"])
    _same_run(runs["eager"], runs["ring"])
    # the routes: three ring loops (the failing one entered a ring of its own on the stored pairs) and three materialisations
    # (the look, the look after the error, the closing look); none on the stored form; no graph replay on the eager route
    assert stats["ring"]["ring_history_loops"] == 3 and stats["ring"]["ring_materializations"] == 3
    # (a hipGraph batch is graph_iters = 8 iterations: only the first loop of k1 = 9 is long enough for one)
    assert stats["ring"]["graph_batches"] == (1 if k1 >= 8 else 0) and stats["ring"]["resident_loops"] == 0
    assert stats["stored"]["ring_history_loops"] == 0 and stats["stored"]["p_less_loops"] == 2
    assert stats["eager"]["graph_batches"] == 0 and stats["eager"]["eager_batches"] >= 3 and stats["eager"]["ring_history_loops"] == 3


@pytest.mark.parametrize("k1", [6, 9])
def test_not_descent_exit_on_the_resident_routes(hip_abi, oracle_abi, monkeypatch, k1):
    """The same calls where one workgroup runs the whole loop (no SDPLR_HIP_FORCE_GRAPH; n = 300, r = 8), through
    inner_loop and through the group launch of batch_major_iteration.  major_iteration's own prologue rebuilds G (fg!), so
    a group reaches the error only when it resumes a loop (SDPLR_MAJOR_RESUME): two handles, both resumed on a G written
    behind their backs, both refused."""
    monkeypatch.delenv("SDPLR_HIP_FORCE_GRAPH", raising=False)
    monkeypatch.delenv("SDPLR_HIP_NO_RESIDENT", raising=False)
    data, r, seed = not_descent_instance("resident")
    nC, nb = data.normC(), float(np.linalg.norm(data.b))
    o, _ = make_solver(oracle_abi, data, r, seed=seed, h=H)
    ora = _not_descent_calls(o, nC, nb, k1)
    o.close()
    g, _ = make_solver(hip_abi, data, r, seed=seed, h=H)
    run = _not_descent_calls(g, nC, nb, k1)
    st = g.stats()
    g.close()
    _check_not_descent(run, ora)
    assert st["resident_loops"] == 3 and st["graph_batches"] == 0 and st["eager_batches"] == 0
    # the group path: the twin is brought to the same point by the same calls and refused in the same launch
    a, _ = make_solver(hip_abi, data, r, seed=seed, h=H)
    b, _ = make_solver(hip_abi, data, r, seed=seed, h=H)
    outb = loop(b, nC, nb, k1, b.fg(nC, nb))
    b.set_factor(cabi.F_GT, -b.get_factor(cabi.F_GT))
    res = []

    def resume_both(out1):
        args = [(nC, nb, 1, 1, 0, cabi.MAJOR_RESUME, 2.0, 0.0, -1e300, 5, 0.0) + tuple(t[:3]) for t in (out1, outb)]
        res.extend(cabi.batch_major_iteration(hip_abi, [a, b], args))
        raise res[0]

    grp = _not_descent_calls(a, nC, nb, k1, failing_call=resume_both)
    assert all(isinstance(x, cabi.SdplrError) and x.code == cabi.ERR_NOT_DESCENT for x in res)
    _check_not_descent(grp, ora)
    # a group launch and a single launch run the same kernel on an instance; dirt after the refusal is left out: the two entry
    # points leave different arrays there (the single one restores a pending dirt ← s_latest first), and the oracle's dirt —
    # the refused direction — is not compared on any route
    _same_run(grp, run, dirt_after_error=False)
    assert a.stats()["resident_shared_launches"] == 1 and b.stats()["resident_shared_launches"] == 1
    assert np.array_equal(b.Rt, grp["R_before"]) and rel(b.Gt, ora["after_error"]["G"]) < 1e-7
    a.close(); b.close()


# ---- B: one handle, several routes ----------------------------------------------------------------------------------------
B_N, B_R = 300, 16


def _b_data(seed):
    return problems.maxcut_data(problems.gnp_graph(B_N, 8.0 / B_N, seed))


class Walk:
    """The same calls on a HIP handle and on the oracle; the route of every HIP call is asserted from the counters."""

    def __init__(self, hip_abi, oracle_abi, monkeypatch, data, seed):
        self.mp, self.hip_abi = monkeypatch, hip_abi
        self.nC, self.nb = data.normC(), float(np.linalg.norm(data.b))
        self.g, _ = make_solver(hip_abi, data, B_R, seed=seed, h=H)
        self.o, _ = make_solver(oracle_abi, data, B_R, seed=seed, h=H)
        self.sg, self.so = self.g.fg(self.nC, self.nb), self.o.fg(self.nC, self.nb)
        assert np.allclose(self.sg, self.so, rtol=1e-11)
        self.updated = False

    def _counted(self, route, call):
        before = self.g.stats()
        if route == "launches":
            self.mp.setenv("SDPLR_HIP_NO_RESIDENT", "1")
        elif route == "profiler":
            self.g.profile_enable(True)
        try:
            out = call()
        finally:
            self.mp.delenv("SDPLR_HIP_NO_RESIDENT", raising=False)
            if route == "profiler":
                self.g.profile_enable(False)
        d = delta(self.g.stats(), before)
        if route == "resident":
            assert d["resident_loops"] == 1 and d["ring_history_loops"] == 0 and d["graph_batches"] + d["eager_batches"] == 0, d
        else:     # the multi-launch route, history in ring form
            assert d["ring_history_loops"] == 1 and d["resident_loops"] == 0 and d["resident_shared_launches"] == 0, d
            if route == "launches":     # (the profiler's own launch loop counts no batches)
                assert d["eager_batches"] + d["graph_batches"] >= 1, d
        return out

    def _agree(self, rg, ro):
        assert rg[4] == ro[4] and rg[5] == ro[5], (rg, ro)
        assert np.allclose(rg[:3], ro[:3], rtol=1e-8), (rg, ro)
        self.sg, self.so = rg[:3], ro[:3]
        self.updated = rg[4] > 0 and rg[5] != 1     # (the relative-decrease exit leaves before lbfgs_update!)

    def loop(self, route, k, fprec=-1e300):
        rg = self._counted(route, lambda: loop(self.g, self.nC, self.nb, k, self.sg, fprec))
        self._agree(rg, loop(self.o, self.nC, self.nb, k, self.so, fprec))
        return rg

    def major(self, route, upd, sigma, k):
        st_in = lambda st: st if upd == cabi.MAJOR_RESUME else ()
        rg = self._counted(route, lambda: self.g.major_iteration(self.nC, self.nb, True, True, False, upd, sigma, 0.0, -1e300, k, 0.0, *st_in(self.sg)))
        self._agree(rg, self.o.major_iteration(self.nC, self.nb, True, True, False, upd, sigma, 0.0, -1e300, k, 0.0, *st_in(self.so)))
        return rg

    def batch_args(self, upd, sigma, k):
        return (self.nC, self.nb, 1, 1, 0, upd, sigma, 0.0, -1e300, k, 0.0) + (tuple(self.sg) if upd == cabi.MAJOR_RESUME else ())

    def after_batch(self, res, d, upd, sigma, k):
        assert not isinstance(res, Exception), res
        assert d["resident_shared_launches"] == 1 and d["resident_loops"] == 1 and d["ring_history_loops"] == 0, d
        st_in = self.so if upd == cabi.MAJOR_RESUME else ()
        self._agree(res[:6], self.o.major_iteration(self.nC, self.nb, True, True, False, upd, sigma, 0.0, -1e300, k, 0.0, *st_in))

    def look(self):
        """What the hand-over left: the oracle's state, and a history consistent with itself — ρ_j⟨s_j, y_j⟩ = 1 for every
        stored pair, dirt the newest pair's s, G the gradient from scratch at R (g!, made on both sides)."""
        a = history_state(self.g, H)
        assert rel(a["R"], self.o.Rt) < 1e-8 and rel(a["G"], self.o.Gt) < 1e-7
        for j in range(H):
            if np.any(a["S"][j]) or np.any(a["Y"][j]):
                assert abs(a["rho"][j] * float(np.sum(a["S"][j] * a["Y"][j])) - 1.0) < 1e-10, j
        if self.updated:
            latest = int(self.g.get_scalar(cabi.S_LBFGS_LATEST))
            assert latest == int(self.o.get_scalar(cabi.S_LBFGS_LATEST))
            assert np.array_equal(a["D"], a["S"][latest - 1])
        self.g.g(); self.o.g()
        assert rel(a["G"], self.g.Gt) < 1e-10
        return a

    def close(self):
        self.g.close(); self.o.close()


def batch(hip_abi, walks, upd, sigma, k):
    before = [w.g.stats() for w in walks]
    res = cabi.batch_major_iteration(hip_abi, [w.g for w in walks], [w.batch_args(upd, sigma, k) for w in walks])
    for w, q, b in zip(walks, res, before):
        w.after_batch(q, delta(w.g.stats(), b), upd, sigma, k)
    return res


@pytest.fixture
def production_mode(monkeypatch):
    monkeypatch.delenv("SDPLR_HIP_FORCE_GRAPH", raising=False)
    monkeypatch.delenv("SDPLR_HIP_NO_RESIDENT", raising=False)
    monkeypatch.delenv("SDPLR_HIP_NO_RING", raising=False)
    monkeypatch.delenv("SDPLR_HIP_NO_GRAPH", raising=False)


def test_ring_loop_then_resident_loop_then_ring_loop(hip_abi, oracle_abi, monkeypatch, production_mode):
    """Sequence 1: a ring loop of 7 (wraps) → the resident loop, 5 iterations, on the ring the first call left → a ring loop of
    4 on the pairs the resident kernel stored."""
    w = Walk(hip_abi, oracle_abi, monkeypatch, _b_data(41), 5)
    w.loop("launches", 7)
    w.loop("resident", 5)
    w.look()
    w.loop("launches", 4)
    w.look()
    st = w.g.stats()
    assert st["ring_history_loops"] == 2 and st["resident_loops"] == 1 and st["ring_materializations"] == 2
    w.close()


def test_ring_loop_under_the_profiler_then_a_resident_batch(hip_abi, oracle_abi, monkeypatch, production_mode):
    """Sequence 2: per-kernel timing keeps a small instance on the multi-launch route; with the profiler off again the handle
    joins a resident group launch with its history still in ring form — the launch clears the history and writes G at its own
    place, so the ring has to go first (update_lambda 0, then 1)."""
    ws = [Walk(hip_abi, oracle_abi, monkeypatch, _b_data(42 + i), 6 + i) for i in range(2)]
    for w in ws:
        w.loop("profiler", 7)
    batch(hip_abi, ws, 0, 2.0, 6)
    for w in ws:
        w.look()
        w.loop("profiler", 5)
    batch(hip_abi, ws, 1, 4.0, 6)
    for w in ws:
        w.look()
        w.close()


def test_ring_left_by_the_relative_decrease_exit_then_a_resident_batch(hip_abi, oracle_abi, monkeypatch, production_mode):
    """Sequence 2 with nothing else in the way: a ring loop that made an update leaves dirt ← s_latest pending, and making
    that copy turns the ring back into the stored form on the way into the group launch.  A ring loop that leaves before
    lbfgs_update! (src/sdplr.jl:238-241) leaves no such copy: the group path has to drop the ring itself."""
    ws = [Walk(hip_abi, oracle_abi, monkeypatch, _b_data(42 + i), 6 + i) for i in range(2)]
    for w in ws:
        w.loop("profiler", 7)
        out = w.loop("profiler", 6, fprec=1e300)
        assert out[4] == 1 and out[5] == 1
    batch(hip_abi, ws, 0, 2.0, 6)
    for w in ws:
        w.look()
        w.close()


def test_ring_loop_then_a_resumed_resident_batch(hip_abi, oracle_abi, monkeypatch, production_mode):
    """Sequence 2, resumed: a capped round in a group (SDPLR_MAJOR_RESUME follows), continued on the multi-launch route — a ring
    again — and resumed in the group: the resumed resident loop reads the stored pairs, so the ring is materialised first."""
    ws = [Walk(hip_abi, oracle_abi, monkeypatch, _b_data(42 + i), 6 + i) for i in range(2)]
    for w in ws:
        w.loop("profiler", 7)
    batch(hip_abi, ws, 0, 4.0, 4)
    for w in ws:
        w.major("launches", cabi.MAJOR_RESUME, 4.0, 3)
    batch(hip_abi, ws, cabi.MAJOR_RESUME, 4.0, 5)
    for w in ws:
        w.look()
        w.close()


def test_resident_relative_decrease_exit_then_ring_then_clear_then_resident(hip_abi, oracle_abi, monkeypatch, production_mode):
    """Sequence 3: the resident loop leaves before lbfgs_update! (y_next = −G_old parked, dirt unscaled) → a ring loop enters
    on that history → lbfgs_clear! drops the ring → the resident loop."""
    w = Walk(hip_abi, oracle_abi, monkeypatch, _b_data(44), 7)
    w.loop("resident", 6)
    out = w.loop("resident", 6, fprec=1e300)
    assert out[4] == 1 and out[5] == 1
    w.loop("launches", 5)
    w.look()
    w.loop("launches", 3)
    w.g.lbfgs_clear(); w.o.lbfgs_clear()
    w.loop("resident", 5)
    w.look()
    w.close()


@pytest.mark.parametrize("upd", [0, 1])
def test_group_launch_equals_the_single_launch_after_a_ring_loop(hip_abi, oracle_abi, monkeypatch, production_mode, upd):
    """Sequence 4: ring loop → major_iteration on one handle; ring loop → batch_major_iteration (a group of two) on its twin.
    The single-instance entry point is the reference of the group path: bitwise."""
    data = _b_data(45)
    single = Walk(hip_abi, oracle_abi, monkeypatch, data, 8)
    grouped = [Walk(hip_abi, oracle_abi, monkeypatch, data, 8), Walk(hip_abi, oracle_abi, monkeypatch, _b_data(46), 9)]
    for w in [single] + grouped:
        w.loop("launches", 7)
    rs = single.major("resident", upd, 4.0, 8)
    rb = batch(hip_abi, grouped, upd, 4.0, 8)
    assert tuple(rb[0][:6]) == tuple(rs)
    a, b = single.look(), grouped[0].look()
    same_state(a, b)
    grouped[1].look()
    for w in [single] + grouped:
        w.close()


# ---- C: the long carry ------------------------------------------------------------------------------------------------------
def _long_carry(hip_abi, monkeypatch, K, ring):
    """fg! → ONE inner_loop call of K iterations on the multi-launch route → (loop's result, G as the loop left it, G from
    scratch at the same point with its norm, R, λ, σ, counters)."""
    data, C, As, bs, r, seed = long_carry_instance()
    nC, nb = data.normC(), float(np.linalg.norm(data.b))
    if ring:
        monkeypatch.delenv("SDPLR_HIP_NO_RING", raising=False)
    else:
        monkeypatch.setenv("SDPLR_HIP_NO_RING", "1")
    g, _ = make_solver(hip_abi, data, r, seed=seed, h=H)
    R0 = g.Rt
    st0 = g.fg(nC, nb)
    y0 = g.y
    out = loop(g, nC, nb, K, st0)
    st = history_state(g, H)
    g.g()
    Gf, gn_f = g.Gt, g.norms(nC, nb)[0]
    res = dict(out=out, state=st, Gc=st["G"], Gf=Gf, gn_f=gn_f, R0=R0, y0=y0, lam=g.λ, sigma=g.σ, stats=g.stats(), nC=nC)
    g.close()
    monkeypatch.delenv("SDPLR_HIP_NO_RING", raising=False)
    return res, (C, As, bs)


def _check_carry(res, prob, K_moving):
    C, As, bs = prob
    R = res["state"]["R"]
    assert np.all(np.isfinite(R)) and np.all(np.isfinite(res["Gc"])) and np.all(np.isfinite(res["out"][:4]))
    G_hp = hp_gradient(C, As, bs, R, res["lam"], res["sigma"])
    e_f = float(np.max(np.abs(res["Gf"] - G_hp)))
    e_c = float(np.max(np.abs(res["Gc"] - G_hp)))
    T, bound = carry_bound(C, res["y0"], res["state"]["y"], res["R0"], R, K_moving)
    u = 2.0 ** -53
    print(f"carried: {e_c / (u * T):.3g}  scratch: {e_f / (u * T):.3g}  allowed: {(e_f + bound) / (u * T):.3g}  (units of 2^-53·T, T = {T:.4g})")
    assert e_c <= e_f + bound
    # ‖G‖ as the loop returned it against norms() on the gradient from scratch, in the norm's own scaling (‖G‖_F / normC)
    n, r = R.shape
    assert abs(res["out"][1] - res["gn_f"]) <= np.sqrt(n * r) * (e_f + bound) / res["nC"]
    return e_c / (u * T), e_f / (u * T)


def test_gradient_carried_for_512_iterations(hip_abi, monkeypatch):
    """One call of 512 iterations, still moving at the end (the oracle's α ≈ 0.1 at iteration 500): G as the loop left it
    against helpers.hp_gradient at the device's R, λ, σ, elementwise in the ∞-norm.  Allowed: the error e_f of the from-scratch
    g! at the same point plus 8·K·2⁻⁵³·T, T = ‖2(|C| + Diag|y|)·|R|‖∞ — fewer than eight roundings per entry and step, each of a
    term bounded by T.  Ring form and stored form agree bitwise after the 512 iterations.
    Measured on an MI355X, in units of 2⁻⁵³·T (T = 66.4): carried 4.95, from scratch 5.21, allowed 4.1e3 — no drift to see."""
    ring, prob = _long_carry(hip_abi, monkeypatch, 512, True)
    stored, _ = _long_carry(hip_abi, monkeypatch, 512, False)
    assert ring["out"][4] == 512 and ring["out"][5] == 2 and ring["out"][3] > 0.0
    assert ring["stats"]["ring_history_loops"] == 1 and ring["stats"]["p_less_loops"] == 1 and ring["stats"]["resident_loops"] == 0
    assert stored["stats"]["ring_history_loops"] == 0 and stored["stats"]["p_less_loops"] == 1
    assert ring["out"] == stored["out"]
    same_state(ring["state"], stored["state"])
    _check_carry(ring, prob, 512)
    _check_carry(stored, prob, 512)


def test_loop_in_the_stalled_regime(hip_abi, oracle_abi, monkeypatch):
    """One call of 1000 iterations: the oracle stops moving after 573 (the line search returns α = 0, the new pair is s = 0,
    y = 0) and returns the same finite (ℒ, ‖G‖, ‖pv‖) to the end of the budget.  The HIP loop, ring form and stored form: no
    error, the oracle's exit and count, finite R and G, ℒ to 1e-10, ring ≡ stored bitwise, and the carried G inside the bound
    of the test above with K the number of iterations that moved.  (The trajectories are not compared elementwise.)
    Measured on an MI355X, in units of 2⁻⁵³·T (T = 66.4): carried 5.15, from scratch 5.78, allowed 4.6e3."""
    K_moving, ora = oracle_moving_iterations(oracle_abi, 1000)
    assert 500 < K_moving < 750 and ora[3] == 0.0
    ring, prob = _long_carry(hip_abi, monkeypatch, 1000, True)
    stored, _ = _long_carry(hip_abi, monkeypatch, 1000, False)
    for run in (ring, stored):
        assert run["out"][4] == ora[4] == 1000 and run["out"][5] == ora[5] == 2
        assert run["out"][0] == pytest.approx(ora[0], rel=1e-10)
    assert ring["stats"]["ring_history_loops"] == 1 and stored["stats"]["ring_history_loops"] == 0
    assert ring["out"] == stored["out"]
    same_state(ring["state"], stored["state"])
    _check_carry(ring, prob, K_moving)
    _check_carry(stored, prob, K_moving)


# ---- D: a refresh by age between calls, and none in a resumed loop --------------------------------------------------------
REFRESH_AGE, CAP = 4, 3


def _refresh_and_resume_child():
    """Runs in a process of its own (SDPLR_HIP_P_REFRESH_ITERS is read once per process): prints one JSON line with the
    counters of the three handles per instance, after asserting cap + resume ≡ uncapped itself (arrays stay here)."""
    import json

    from sdplrplus_jl_amd import load_hip
    hip_abi = load_hip()
    report, lc = {}, long_carry_instance()
    for name, (data, r, seed) in (("not_descent", not_descent_instance("launches")), ("long_carry", lc[:1] + lc[4:])):
        nC, nb = data.normC(), float(np.linalg.norm(data.b))
        major = lambda s_, upd, k, st=(): s_.major_iteration(nC, nb, True, True, False, upd, 2.0, 0.0, -1e300, k, 0.0, *st[:3])
        # three calls of their own: G is 2·CAP ≥ REFRESH_AGE iterations old in front of the third
        a, _ = make_solver(hip_abi, data, r, seed=seed, h=H)
        st, per_call = a.fg(nC, nb), []
        for _ in range(3):
            before = a.stats()
            st = loop(a, nC, nb, CAP, st)
            assert st[4] == CAP and st[5] == 2, st
            per_call.append(delta(a.stats(), before))
        a.close()
        # one loop of 3·CAP iterations in three pieces, and in one
        b, _ = make_solver(hip_abi, data, r, seed=seed, h=H)
        out_b, pieces = major(b, 0, CAP), []
        for _ in range(2):
            assert out_b[4] == CAP and out_b[5] == 2, out_b
            before = b.stats()
            out_b = major(b, cabi.MAJOR_RESUME, CAP, out_b)
            pieces.append(delta(b.stats(), before))
        stats_b = b.stats()
        c, _ = make_solver(hip_abi, data, r, seed=seed, h=H)
        out_c = major(c, 0, 3 * CAP)
        stats_c = c.stats()
        print(name, "resumed:", out_b, "uncapped:", out_c, file=sys.stderr)
        assert out_b[:4] == out_c[:4] and out_b[4] == CAP and out_c[4] == 3 * CAP and out_b[5] == out_c[5] == 2
        same_state(history_state(b, H), history_state(c, H))
        b.close(); c.close()
        report[name] = dict(calls=per_call, pieces=pieces, resumed=stats_b, uncapped=stats_c)
    print(json.dumps(report))


def test_refresh_by_age_between_calls_and_none_in_a_resumed_loop():
    """SDPLR_HIP_P_REFRESH_ITERS = 4 on the fast2 route (P-less step kernel, history in ring form), two instances.  Three calls
    of 3 iterations: in front of the third the carried G is 6 iterations old, so it is formed from scratch — at its own place,
    which ends the ring the first two calls shared (one materialisation), and the call enters a ring of its own.  The same 9
    iterations as one major_iteration capped at 3 and two SDPLR_MAJOR_RESUME calls of 3: a resumed loop takes the kernel the
    capped call took and refreshes nothing by age — one ring throughout, no materialisation — and is one uncapped call of 9
    bit for bit (asserted in the child, where the arrays are)."""
    import json
    import os
    import subprocess
    tests = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, SDPLR_HIP_P_REFRESH_ITERS=str(REFRESH_AGE), SDPLR_HIP_FORCE_GRAPH="1")
    for k in ("SDPLR_HIP_NO_RING", "SDPLR_HIP_NO_GRAPH", "SDPLR_HIP_NO_RESIDENT", "SDPLR_HIP_NO_PDROP"):
        env.pop(k, None)
    code = (f"import sys; sys.path[:0] = [{tests!r}, {os.path.dirname(tests)!r}]; "
            "import test_gpu_handover as t; t._refresh_and_resume_child()")
    p = subprocess.run([sys.executable, "-s", "-c", code], env=env, capture_output=True, text=True, timeout=300)
    print(p.stdout, p.stderr[-3000:])
    assert p.returncode == 0, p.stderr[-3000:]
    report = json.loads(p.stdout.strip().splitlines()[-1])
    assert set(report) == {"not_descent", "long_carry"}
    for name, rep in report.items():
        for i, d in enumerate(rep["calls"]):      # every call P-less and on a ring; only the third one due for its refresh
            assert d["p_less_loops"] == 1 and d["ring_history_loops"] == 1 and d["resident_loops"] == 0, (name, i, d)
            assert d["ring_materializations"] == (1 if i == 2 else 0), (name, i, d)
        for i, d in enumerate(rep["pieces"]):     # the resumed pieces: the capped call's kernel, its ring kept
            assert d["p_less_loops"] == 1 and d["ring_history_loops"] == 1 and d["ring_materializations"] == 0, (name, i, d)
        assert rep["resumed"]["p_less_loops"] == 3 and rep["resumed"]["ring_history_loops"] == 3, (name, rep["resumed"])
        assert rep["resumed"]["ring_materializations"] == 0 and rep["uncapped"]["ring_materializations"] == 0, name
        assert rep["uncapped"]["p_less_loops"] == 1 and rep["uncapped"]["ring_history_loops"] == 1, (name, rep["uncapped"])
