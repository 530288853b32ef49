"""The ring-route direction kernel sweeps from the last element pair down, and the history loads of the step and direction
kernels choose their cache policy by row range (csrc/k_dense.h, k_sparse.h; SDPLR_HIP_LLC_WINDOW_KB, a byte budget in KiB
read when a handle is created).  k_lbfgs_dir_ring is elementwise and the step kernel keeps its order, so neither the order
nor the policy can change a value: every comparison here is BITWISE against the stored form (SDPLR_HIP_NO_RING=1), and a
difference means an element visited twice or never, or a wrong tail.

The instances are tiny, so their arenas fit the Infinity Cache and the library would load everything plain; the children
run with SDPLR_HIP_DIR_NT_ABOVE_MB=0 (read once per process: hence the child processes), which makes the window code the
one that runs.  SDPLR_HIP_NB_DENSE=3 / SDPLR_HIP_NB_STEP=2 shrink the grids — for every variant alike — so that these
sizes take several trips with a partial last one.  The mid budget of a case is chosen so that both boundaries lie strictly
inside the matrix, the step kernel's inside a tile of 4 rows and the direction kernel's inside a block of 256 pairs.

The window sizes are mirrored here from their definition:
  w_dir = ⌊B / (step + direction bytes per row)⌋, w_step = ⌊(B − gather bytes) / (the same)⌋, clamped to [0, n];
  B ≥ the arena: n and n; B = 0: no window."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as sp

from helpers import history_state, make_solver, same_state
from sdplrplus_jl_amd import cabi, problems

pytestmark = pytest.mark.gpu

NB_DENSE, NB_STEP, TILE_ROWS, BLOCK = 3, 2, 4, 256
HUGE_KB = 1 << 30
ITERS = 12

# name → (family, n, G(n, p) seed or None for the triangle, r, h, solver seed, iterations run and looked at before the 12)
CASES = {
    "one_block_n3_r2": ("maxcut", 3, None, 2, 4, 1, 0),        # n·r/2 = 3 pairs: less than one block; one lane per row
    "one_block_n3_r6": ("maxcut", 3, None, 6, 4, 1, 0),        # the same with four lanes per row: 9 pairs
    "n257_r32": ("maxcut", 257, 41, 32, 4, 3, 0),              # 4112 pairs = 16 blocks + 16; 257 rows = 64 tiles + 1
    "n1000_r6": ("maxcut", 1000, 42, 6, 4, 5, 0),              # 3000 pairs: neither a multiple of 256 nor of 3 × 256
    "minbis_n150": ("minbis", 150, 43, 8, 4, 7, 0),            # the P-based step kernel (PB = true); 150 rows = 37 tiles + 2
    "h2_n301_r16": ("maxcut", 301, 44, 16, 2, 9, 0),
    "stored_history_n421_r10": ("maxcut", 421, 45, 10, 4, 11, 3),   # the ring grows into the stored pairs: ring_n < h at first
}


def _instance(case):
    family, n, gseed, r, h, seed, pre = CASES[case]
    A = sp.csc_matrix(np.ones((3, 3)) - np.eye(3)) if gseed is None else problems.gnp_graph(n, 8.0 / n, gseed)
    data = problems.maxcut_data(A) if family == "maxcut" else problems.minimum_bisection_data(A)
    return data, int(A.nnz) + n, family == "minbis"      # (nnz of the full pattern of S: the graph and the diagonal)


def windows(B, n, r, h, pb, nnzS):
    row = 8 * r
    arena = (3 + 2 * h + 2) * ((n * r + 31) // 32 * 32) * 8
    if B >= arena:
        return n, n
    per_row = row * ((5 + 2 * h - 1 + (2 if pb else 0)) + (2 * h + 2))
    gather = (3 + (1 if pb else 0)) * n * row + 4 * (n + 1) + 12 * nnzS
    clamp = lambda w: max(0, min(n, w))
    return clamp(B // per_row), clamp((B - gather) // per_row if B >= gather else 0)


def mid_budget_kb(n, r, h, pb, nnzS):
    """The budget whose lower window is nearest n/3 among those that put both boundaries strictly inside, the step kernel's
    inside a tile and the direction kernel's inside a block (and inside a trip of NB_DENSE blocks)."""
    N2, best = n * r // 2, None
    for kb in range(1, 1 << 14):
        wd, ws = windows(kb << 10, n, r, h, pb, nnzS)
        if wd >= n:
            break
        cut = N2 - ws * r // 2         # pairs the direction kernel visits before it reaches the window
        if not (0 < ws <= wd < n):
            continue
        if n >= 2 * TILE_ROWS and ((n - wd) % TILE_ROWS == 0 or cut % BLOCK == 0 or cut % (NB_DENSE * BLOCK) == 0):
            continue
        if best is None or abs(ws - n // 3) < abs(best[1] - n // 3):
            best = (kb, ws)
    assert best is not None
    return best[0]


def _child(case):
    """One case in a process of its own: the stored form and the ring route under three budgets, from the same start; the
    arrays are compared here, the counters go back as one JSON line."""
    from sdplrplus_jl_amd import load_hip
    hip = load_hip()
    family, n, gseed, r, h, seed, pre = CASES[case]
    data, nnzS, pb = _instance(case)
    nC, nb = data.normC(), float(np.linalg.norm(data.b))
    mid = mid_budget_kb(n, r, h, pb, nnzS)

    def run(budget_kb):
        os.environ.pop("SDPLR_HIP_NO_RING", None)
        os.environ.pop("SDPLR_HIP_LLC_WINDOW_KB", None)
        if budget_kb is None:
            os.environ["SDPLR_HIP_NO_RING"] = "1"
        else:
            os.environ["SDPLR_HIP_LLC_WINDOW_KB"] = str(budget_kb)
        s_, _ = make_solver(hip, data, r, seed=seed, h=h)
        st, outs = s_.fg(nC, nb), []
        for k in ([pre] if pre else []) + [ITERS]:
            try:
                out = s_.inner_loop(nC, nb, True, True, False, 0.0, -1e300, k, 0.0, *st[:3])
            except cabi.SdplrError as e:      # (the triangle converges to round-off: whatever its loop does, both forms do)
                out = st[:3] + ("error", e.code)
            outs.append(out)
            stats = s_.stats()                # (before the look: it counts a materialisation)
            state = history_state(s_, h)      # the look: s_j, y_j materialised through get_factor
            st = out
        s_.close()
        return outs, state, stats

    ref_outs, ref_state, ref_stats = run(None)
    assert ref_stats["ring_history_loops"] == 0
    print(case, "stored form:", ref_outs, file=sys.stderr)
    assert n == 3 or all(out[4] == k for out, k in zip(ref_outs, ([pre] if pre else []) + [ITERS])), ref_outs
    report = dict(n=n, mid_kb=mid, nnzS=nnzS, variants={})
    for name, kb in (("none", 0), ("mid", mid), ("huge", HUGE_KB)):
        outs, state, stats = run(kb)
        assert outs == ref_outs, (name, outs, ref_outs)
        same_state(state, ref_state)
        ran_pb = stats["p_less_loops"] == 0
        report["variants"][name] = dict(stats=stats, pb=ran_pb, expect=list(windows(kb << 10, n, r, h, ran_pb, nnzS)))
    print(json.dumps(report))


def _fallback_child():
    """The recipe of test_gpu_ring.py::test_ring_takes_the_steepest_descent_fallback (the newest stored pair replaced by
    s = G, y = 0, ρ ≪ 0; a fresh g!): the next loop falls back in its first iteration, fb = 1 in k_lbfgs_dir_ring.  After ONE
    iteration the newest pair is s = fl(α·D) with D = −G bit for bit; three more calls stay bitwise the stored form."""
    from sdplrplus_jl_amd import load_hip
    hip = load_hip()
    data = problems.maxcut_data(problems.gnp_graph(200, 0.06, 17))
    nC, nb = data.normC(), float(np.linalg.norm(data.b))
    n, r, h = 200, 8, 4
    mid = mid_budget_kb(n, r, h, False, int(problems.gnp_graph(200, 0.06, 17).nnz) + n)

    def run(budget_kb):
        os.environ.pop("SDPLR_HIP_NO_RING", None)
        os.environ.pop("SDPLR_HIP_LLC_WINDOW_KB", None)
        if budget_kb is None:
            os.environ["SDPLR_HIP_NO_RING"] = "1"
        else:
            os.environ["SDPLR_HIP_LLC_WINDOW_KB"] = str(budget_kb)
        s_, _ = make_solver(hip, data, r, seed=5, h=h)
        st = s_.inner_loop(nC, nb, True, True, False, 0.0, -1e300, h + 2, 0.0, *s_.fg(nC, nb))[:3]
        j = int(s_.get_scalar(cabi.S_LBFGS_LATEST)) - 1
        G = s_.Gt
        s_.set_factor(cabi.F_LBFGS_S + j, G)
        s_.set_factor(cabi.F_LBFGS_Y + j, np.zeros_like(G))
        rho = s_.get_vec(cabi.V_LBFGS_RHO)
        rho[j] = -1e6 / float(np.sum(G * G))
        s_.set_vec(cabi.V_LBFGS_RHO, rho)
        s_.g()
        G0 = s_.Gt.copy()
        out = s_.inner_loop(nC, nb, True, True, False, 0.0, -1e300, 1, 0.0, *st)
        assert out[4] == 1, out
        first = history_state(s_, h)
        newest = int(s_.get_scalar(cabi.S_LBFGS_LATEST)) - 1
        assert np.array_equal(first["S"][newest], out[3] * (-G0))          # s = fl(α·D), D = −G
        outs, st = [out], out[:3]
        for k in (1, 6):
            out = s_.inner_loop(nC, nb, True, True, False, 0.0, -1e300, k, 0.0, *st)
            st = out[:3]
            outs.append(out)
        stats = s_.stats()
        last = history_state(s_, h)
        s_.close()
        return outs, first, last, stats

    ref = run(None)
    report = {}
    for name, kb in (("none", 0), ("mid", mid), ("huge", HUGE_KB)):
        got = run(kb)
        assert got[0] == ref[0], (name, got[0], ref[0])
        same_state(got[1], ref[1])
        same_state(got[2], ref[2])
        report[name] = got[3]
    print(json.dumps(report))


def _run_child(call):
    tests = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, SDPLR_HIP_FORCE_GRAPH="1", SDPLR_HIP_DIR_NT_ABOVE_MB="0", SDPLR_HIP_NB_DENSE=str(NB_DENSE),
               SDPLR_HIP_NB_STEP=str(NB_STEP))
    for k in ("SDPLR_HIP_NO_RING", "SDPLR_HIP_NO_GRAPH", "SDPLR_HIP_NO_RESIDENT", "SDPLR_HIP_NO_PDROP", "SDPLR_HIP_LLC_WINDOW_KB"):
        env.pop(k, None)
    code = (f"import sys; sys.path[:0] = [{tests!r}, {os.path.dirname(tests)!r}]; "
            f"import test_gpu_sweep_window as t; t.{call}")
    p = subprocess.run([sys.executable, "-s", "-c", code], env=env, capture_output=True, text=True, timeout=300)
    print(p.stdout, p.stderr[-3000:])
    assert p.returncode == 0, p.stderr[-3000:]
    return json.loads(p.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("case", list(CASES))
def test_reversed_sweep_and_windows_are_the_stored_form_bit_for_bit(case):
    """R, G, dirt, every materialised s_j and y_j, ρ, y and the loops' scalar returns after 12 iterations (asserted in the
    child) under budget 0, a budget with both boundaries inside the matrix, and a huge one; here: the route and the windows
    that ran."""
    rep = _run_child(f"_child({case!r})")
    n, loops = rep["n"], 2 if CASES[case][6] else 1
    for name, v in rep["variants"].items():
        st = v["stats"]
        assert st["ring_history_loops"] == loops and st["resident_loops"] == 0, (name, st)
        assert v["pb"] == (CASES[case][0] == "minbis"), (name, st)
        assert [st["ring_window_dir_rows"], st["ring_window_step_rows"]] == v["expect"], (name, st, v["expect"])
    wd, ws = rep["variants"]["mid"]["expect"]
    assert 0 < ws <= wd < n
    assert rep["variants"]["none"]["expect"] == [0, 0] and rep["variants"]["huge"]["expect"] == [n, n]


def test_steepest_descent_fallback_under_the_reversed_sweep():
    rep = _run_child("_fallback_child()")
    for name, st in rep.items():
        assert st["ring_history_loops"] == 4, (name, st)
    assert rep["none"]["ring_window_dir_rows"] == 0 and rep["huge"]["ring_window_step_rows"] == 200
    assert 0 < rep["mid"]["ring_window_step_rows"] <= rep["mid"]["ring_window_dir_rows"] < 200


def test_an_arena_that_fits_the_cache_keeps_its_hints(hip_abi, monkeypatch):
    """Below the size test of the direction kernel (the arena fits the Infinity Cache) only the sweep order changes: the
    direction kernel loads everything plain, the step kernel keeps its non-temporal history loads, whatever the budget."""
    monkeypatch.delenv("SDPLR_HIP_NO_RING", raising=False)
    data = problems.maxcut_data(problems.gnp_graph(257, 8.0 / 257, 41))
    nC, nb = data.normC(), float(np.linalg.norm(data.b))
    for kb in ("0", "64", str(HUGE_KB)):
        monkeypatch.setenv("SDPLR_HIP_LLC_WINDOW_KB", kb)
        s_, _ = make_solver(hip_abi, data, 32, seed=3, h=4)
        s_.inner_loop(nC, nb, True, True, False, 0.0, -1e300, 3, 0.0, *s_.fg(nC, nb))
        st = s_.stats()
        s_.close()
        assert st["ring_history_loops"] == 1 and (st["ring_window_dir_rows"], st["ring_window_step_rows"]) == (0, 257), (kb, st)
