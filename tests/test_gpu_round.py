"""Randomized rounding on the device (include/sdplr_hip_round.h, k_round.h) against the numpy restatement of its
definitions (tests/round_reference.py): labels, cuts, best trial and best labelling bit for bit; summation-order bound
for real weights; the host callbacks on a real solution; the call reads solver state and writes none."""
import os

import numpy as np
import pytest

import sdplrplus_jl_amd as sj
from sdplrplus_jl_amd import cabi, problems, rounding

from helpers import make_solver, not_descent_instance
import round_reference as ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53


def handle(hip_abi, n, r, h=0):
    """A finalized handle with n rows at rank r: MaxCut on a path (every row has a constraint and, for n ≥ 2, an edge).  The
    rounding reads nothing of the instance but the factor slot."""
    import scipy.sparse as sp
    if n >= 2:
        i = np.arange(n - 1)
        A = sp.coo_matrix((np.ones(2 * (n - 1)), (np.concatenate([i, i + 1]), np.concatenate([i + 1, i]))), shape=(n, n)).tocsc()
        data = problems.maxcut_data(A)
    else:
        data = sj.SDPData(sp.identity(1, format="csc"), [sj.SparseMatrixCOO([0], [0], [1.0], 1, 1)], np.ones(1))
    s, _ = make_solver(hip_abi, data, r, h=h)
    return s


def special_factor(n, r, rng, dup=False):
    """A Gaussian factor with the rows the definitions single out: a zero row, a row of −0.0 (z = −0.0 exactly under every
    γ > 0 … and +0.0 under the others: both label +1 and tie with the zero row), and — dup — runs of bitwise-equal rows
    placed so that their equal keys straddle the ⌊n/2⌋ threshold whatever γ is (more than half the rows are one row)."""
    R = rng.standard_normal((n, r))
    if dup and n >= 16:
        idx = rng.permutation(n)[: n // 2 + 8]       # (five of them may become special rows below: still more than half)
        R[idx] = R[idx[0]]
    if n >= 3:
        R[n // 3] = 0.0
        R[n - 1] = -0.0
    if n >= 9:
        R[[1, n // 2, n - 2]] = 0.0          # several zero rows: ±0.0 ties in index order
    return R


def check_exact(s, R, gauss, A, mode, slot=cabi.F_RT):
    want = ref.rounding(R, gauss, A, mode)
    cuts, best, xb, lab = s.round(mode, gauss.shape[0], gauss, slot=slot, want_best=True, want_labels=True)
    assert np.array_equal(lab, want["labels"]), (mode, np.argwhere(lab != want["labels"])[:5])
    assert np.array_equal(cuts, want["cuts"]), (mode, cuts[:4], want["cuts"][:4])
    assert best == want["best"] and np.array_equal(xb, want["x_best"])
    if mode == 1:
        n = R.shape[0]
        # ⌊n/2⌋ labels are +1 and the other n − ⌊n/2⌋ are −1: every trial's labels sum to 2⌊n/2⌋ − n, of magnitude
        # n − 2⌊n/2⌋ (0 for even n; for odd n the odd vertex out is on the −1 side, as in exps/test.jl:92-96)
        tot = lab.astype(np.int64).sum(axis=1)
        assert np.all(np.abs(tot) == n - 2 * (n // 2)) and np.all(tot == 2 * (n // 2) - n)
    return want


# a covering subset of n × r × T × E: every n, r, T and E of the grid at least once, the word boundary (63, 64, 65) in n
# and in T against each other, n below, at and above one block of 256 vertices, r at and above the LDS chunk of 32
CASES = [
    (1, 1, 1, 0), (1, 3, 65, 1), (2, 2, 63, 1), (2, 33, 64, 0),
    (63, 1, 64, 255), (64, 3, 65, 256), (65, 10, 63, 257), (64, 32, 100, 1), (63, 33, 130, 256),
    (257, 2, 130, 3000), (257, 32, 1, 255), (257, 33, 64, 257),
    (1000, 10, 100, 5000), (1000, 33, 65, 0), (1000, 3, 130, 4000), (1000, 32, 63, 1),
]


@pytest.mark.parametrize("n,r,T,E", CASES)
def test_labels_and_cuts_exact(hip_abi, n, r, T, E):
    """Checks 1 and 2: both modes on ±1-weighted graphs, where every sum is exact in FP64 — everything array_equal."""
    rng = np.random.Generator(np.random.PCG64(7000 + 31 * n + 7 * r + T))
    A = ref.random_graph(n, E, rng)
    s = handle(hip_abi, n, r)
    s.round_set_graph(A)
    for mode, dup in ((0, False), (1, False), (1, True)):
        R = special_factor(n, r, rng, dup=dup)
        gauss = rng.standard_normal((T, r))
        if r == 1 and T > 2:
            gauss[1] = abs(gauss[1])         # the −0.0 row under a positive and a negative γ
            gauss[2] = -abs(gauss[2])
        s.set_factor(cabi.F_RT, R)
        want = check_exact(s, R, gauss, A, mode)
        if n >= 3 and r == 1 and T > 2:
            zz = want["z"][n - 1]
            assert zz[1] == 0 and np.signbit(zz[1]) and not np.signbit(zz[2])      # the comparator did see a −0.0
        if mode == 1 and dup and n >= 16:
            # the duplicated rows do tie across the threshold: some of them on either side, in every trial
            z = want["z"]
            srt = np.sort(z + 0.0, axis=0)
            assert np.all(srt[n // 2 - 1] == srt[n // 2])
    s.close()


@pytest.mark.parametrize("mode", [0, 1])
def test_real_weights_within_the_summation_bound(hip_abi, mode):
    """Check 3: uniform weights in (0, 1): labels exact, |cut − comparator| ≤ γ_E·Σ|a_ij|, γ_E = E·u/(1 − E·u) — the bound of a
    sum of E terms in ANY order, which holds for the device's order and the comparator's alike (so twice it between them)."""
    n, r, T, E = 1000, 10, 100, 5000
    rng = np.random.Generator(np.random.PCG64(515 + mode))
    A = ref.random_graph(n, E, rng, weights="real")
    R = special_factor(n, r, rng)
    gauss = rng.standard_normal((T, r))
    s = handle(hip_abi, n, r)
    s.round_set_graph(A)
    s.set_factor(cabi.F_RT, R)
    want = ref.rounding(R, gauss, A, mode)
    cuts, best, xb, lab = s.round(mode, T, gauss, want_best=True, want_labels=True)
    s.close()
    assert np.array_equal(lab, want["labels"])
    I, J, W = ref.edges_of(A)
    bound = (E * U / (1 - E * U)) * float(np.sum(np.abs(W)))
    # each side is within `bound` of the exact sum of its own labelling's weights; the labellings are equal
    err = np.abs(cuts - want["cuts"])
    print("real weights, mode", mode, "max |cut - comparator| =", float(err.max()), "bound", bound)
    assert np.all(err <= bound)
    assert np.array_equal(xb, lab[best])
    pick = np.argmax if mode == 0 else np.argmin
    assert best == int(pick(cuts))


_BIG = {}


def _big():
    if not _BIG:
        n, r, T = 20000, 32, 100
        rng = np.random.Generator(np.random.PCG64(20000))
        A = problems.gnp_graph(n, 1e-3, 11)
        I, J, W = ref.edges_of(A)
        W = rng.choice([-1.0, 1.0], size=W.size)
        _BIG.update(n=n, r=r, T=T, A=(I, J, W), R=special_factor(n, r, rng), gauss=rng.standard_normal((T, r)))
    return _BIG


@pytest.mark.parametrize("mode", [0, 1])
def test_one_size_across_every_block_boundary(hip_abi, mode):
    """Check 4: n = 20 000, r = 32, T = 100, G(n, 1e-3) with ±1 weights: many blocks of every kernel, two trial blocks (the
    second one partial), ≈ 2·10⁵ edges over all 256 scoring blocks — exact."""
    b = _big()
    s = handle(hip_abi, b["n"], b["r"])
    s.round_set_graph(b["A"])
    s.set_factor(cabi.F_RT, b["R"])
    check_exact(s, b["R"], b["gauss"], b["A"], mode)
    s.close()


_G1 = {}


def _g1_solution(oracle_abi, problem):
    """Gset G1 (n = 800) at r = 10, solved by the CPU checker: the same R on every machine."""
    if problem not in _G1:
        z = np.load(os.path.join(ROOT, "tests", "golden", "gset_G1_G9.npz"))
        A = problems.graph_from_edges(int(z["G1_n"]), z["G1"])
        data = (problems.maxcut_data if problem == "MaxCut" else problems.minimum_bisection_data)(A)
        res = sj.sdplr(data=data, r=10, abi=oracle_abi, seed=0, printlevel=0, ptol=1e-2, objtol=1e-2,
                       prior_trace_bound=float(data.n), maxtime=600.0)
        _G1[problem] = (A, data, res["Rt"])
    return _G1[problem]


# seeds for which the comparator alone (sequential projection against the BLAS projection, both on the CPU) leaves out no
# trial: chosen by running exactly the masks below on the development machine without a device
G1_SEED = {"MaxCut": 11, "MinimumBisection": 11}


@pytest.mark.parametrize("problem", ["MaxCut", "MinimumBisection"])
def test_against_the_host_callbacks_on_a_real_solution(hip_abi, oracle_abi, problem):
    """Check 5.  The host callback projects with a BLAS GEMV, whose sum may differ from the sequential one by
    ≤ 4·r·u·Σ_k|R_ik γ_kt| =: b_it.  Mode 0: a label may flip only where |z_it| ≤ b_it.  Mode 1: the split may move only if
    the gap between the two sides of the threshold, z_(⌊n/2⌋+1) − z_(⌊n/2⌋), is ≤ 2·max_i b_it.  Trials with such an entry are
    left out (at most 5 of 100); on all others the per-trial cuts are equal (unit weights: exact)."""
    A, data, R = _g1_solution(oracle_abi, problem)
    mode = 0 if problem == "MaxCut" else 1
    seed, T, r, n = G1_SEED[problem], 100, R.shape[1], R.shape[0]
    host_fn = rounding.maxcut_rounding if mode == 0 else rounding.minimumbisection_rounding
    dev_fn = rounding.maxcut_rounding_device if mode == 0 else rounding.minimumbisection_rounding_device
    s, _ = make_solver(hip_abi, data, r)
    s.set_factor(cabi.F_RT, R)
    mk = lambda: np.random.Generator(np.random.PCG64(seed))
    g_host, g_dev = mk(), mk()
    host_best = host_fn(A, R, g_host, T)
    dev_best = dev_fn(s, A, g_dev, T)
    assert g_host.standard_normal() == g_dev.standard_normal()         # both consumed the generator alike
    # per trial
    g = mk()
    gauss = np.stack([g.standard_normal(r) for _ in range(T)])
    cuts, best, _, lab = s.round(mode, T, gauss, want_labels=True)
    s.close()
    assert dev_best == cuts[best]
    L = problems._laplacian(A, 1.0)
    zseq = ref.project(R, gauss)
    bnd = 4 * r * U * (np.abs(R) @ np.abs(gauss).T)                     # (n, T)
    host_cuts, skip = np.zeros(T), np.zeros(T, dtype=bool)
    for t in range(T):
        zb = R @ gauss[t]
        if mode == 0:
            x = np.sign(zb)
            x[x == 0] = 1.0
            skip[t] = np.any(np.abs(zseq[:, t]) <= bnd[:, t])
        else:
            perm = np.argsort(zb, kind="stable")
            x = np.zeros(n)
            x[perm] = np.where((np.arange(1, n + 1) * 2) <= n, 1.0, -1.0)
            srt = np.sort(zseq[:, t])
            skip[t] = srt[n // 2] - srt[n // 2 - 1] <= 2 * bnd[:, t].max()
        host_cuts[t] = rounding.eval_cut(L, x)
    print(problem, "trials left out:", int(skip.sum()), "host best", host_best, "device best", dev_best)
    assert skip.sum() <= 5
    assert np.array_equal(cuts[~skip], host_cuts[~skip])
    if not skip.any():
        assert dev_best == host_best


def _two_majors(s, nC, nb, rounds=None):
    """major iteration (6 inner iterations) → [rounds] → major iteration with the λ update → everything readable."""
    out1 = s.major_iteration(nC, nb, True, True, False, 0, 2.0, 0.0, -1e300, 6, 0.0)
    got = rounds(s) if rounds else None
    out2 = s.major_iteration(nC, nb, True, True, False, 1, 2.0, 0.0, -1e300, 6, 0.0)
    st = s.stats()
    return dict(out1=out1, out2=out2, R=s.Rt.copy(), G=s.Gt.copy(), lam=s.λ.copy(), obj=s.obj, sigma=s.σ), got, st


@pytest.mark.parametrize("route", ["launches", "resident"])
def test_round_reads_state_and_writes_none(hip_abi, monkeypatch, route):
    """Check 6: a major iteration, round (both modes, twice each), another major iteration: R, G, λ and the returned scalars
    equal the same sequence without the round calls bit for bit — on the multi-launch route with the history in ring form
    (which the call must leave a ring: no materialisation more than without it) and on the resident route."""
    if route == "resident":
        monkeypatch.delenv("SDPLR_HIP_FORCE_GRAPH", raising=False)
        monkeypatch.delenv("SDPLR_HIP_NO_RESIDENT", raising=False)
    monkeypatch.delenv("SDPLR_HIP_NO_RING", raising=False)
    data, r, seed = not_descent_instance(route)
    nC, nb = data.normC(), float(np.linalg.norm(data.b))
    rng = np.random.Generator(np.random.PCG64(61))
    A = ref.random_graph(data.n, 2000, rng)
    gauss = rng.standard_normal((70, r))

    def rounds(s):
        s.round_set_graph(A)
        R_now = s.Rt.copy()
        res = []
        for mode in (0, 1):
            a = s.round(mode, 70, gauss, want_best=True, want_labels=True)
            b = s.round(mode, 70, gauss, want_best=True, want_labels=True)
            assert a[1] == b[1] and all(np.array_equal(x, y) for x, y in zip((a[0],) + a[2:], (b[0],) + b[2:]))
            want = ref.rounding(R_now, gauss, A, mode)
            assert np.array_equal(a[3], want["labels"]) and np.array_equal(a[0], want["cuts"]) and a[1] == want["best"]
            res.append(a)
        return res

    a, _ = make_solver(hip_abi, data, r, seed=seed, h=4)
    plain, _, st_plain = _two_majors(a, nC, nb)
    a.close()
    b, _ = make_solver(hip_abi, data, r, seed=seed, h=4)
    with_round, got, st_round = _two_majors(b, nC, nb, rounds)
    b.close()
    assert got is not None
    assert plain["out1"] == with_round["out1"] and plain["out2"] == with_round["out2"]
    for k in ("R", "G", "lam"):
        assert np.array_equal(plain[k], with_round[k]), k
    assert plain["obj"] == with_round["obj"] and plain["sigma"] == with_round["sigma"]
    assert plain["out1"][4] == 6 and plain["out2"][4] == 6
    for k in ("ring_history_loops", "ring_materializations", "resident_loops", "graph_batches", "eager_batches", "p_less_loops"):
        assert st_plain[k] == st_round[k], (k, st_plain[k], st_round[k])
    if route == "resident":
        assert st_round["resident_loops"] == 2 and st_round["ring_history_loops"] == 0
    else:
        assert st_round["ring_history_loops"] == 2 and st_round["resident_loops"] == 0


def test_slots_rank_graph_replacement_errors_and_profile(hip_abi):
    """Check 7."""
    n, r, T = 300, 4, 70
    rng = np.random.Generator(np.random.PCG64(77))
    A1, A2 = ref.random_graph(n, 900, rng), ref.random_graph(n, 500, rng)
    s = handle(hip_abi, n, r, h=4)
    gauss = rng.standard_normal((T, r))
    # before a graph is set
    with pytest.raises(sj.SdplrError) as e:
        s.round(0, T, gauss)
    assert e.value.code == cabi.ERR_STATE
    s.round_set_graph(A1)
    R = rng.standard_normal((n, r))
    s.set_factor(cabi.F_RT, R)
    # a scratch slot; R itself is not what is rounded
    Q = rng.standard_normal((n, r))
    s.set_factor(cabi.F_SCRATCH, Q)
    for mode in (0, 1):
        check_exact(s, Q, gauss, A1, mode, slot=cabi.F_SCRATCH)
        check_exact(s, R, gauss, A1, mode, slot=cabi.F_RT)
    # the second graph wins
    s.round_set_graph(A2)
    check_exact(s, R, gauss, A2, 0)
    # the profiler sees the new kernels
    s.profile_enable(True)
    s.round(1, T, gauss, want_best=True)
    prof = s.profile()
    s.profile_enable(False)
    for name in ("round_project", "round_select", "round_pack", "round_score", "round_fold", "round_labels"):
        assert name in prof and prof[name][0] >= 1, (name, sorted(prof))
    assert prof["round_project"][0] == 2 and prof["round_select"][0] == 2          # two trial blocks
    # errors
    def code(fn):
        with pytest.raises(sj.SdplrError) as e:
            fn()
        return e.value.code
    assert code(lambda: s.round(2, T, gauss)) == cabi.ERR_INVALID_ARG
    assert code(lambda: s.round(-1, T, gauss)) == cabi.ERR_INVALID_ARG
    assert code(lambda: s.round(0, T, gauss, slot=7)) == cabi.ERR_INVALID_ARG
    assert code(lambda: s.round(0, T, gauss, slot=cabi.F_LBFGS_S + 4)) == cabi.ERR_INVALID_ARG
    assert code(lambda: s.round(0, 0, np.zeros((0, r)))) == cabi.ERR_INVALID_ARG
    assert code(lambda: s.round(0, 4097, np.zeros((4097, r)))) == cabi.ERR_INVALID_ARG
    i, j, w = np.array([0, n]), np.array([1, 2]), np.ones(2)
    assert code(lambda: s.round_set_graph((i, j, w))) == cabi.ERR_INVALID_ARG
    assert code(lambda: s.round_set_graph((np.array([-1]), np.array([2]), np.ones(1)))) == cabi.ERR_INVALID_ARG
    check_exact(s, R, gauss, A2, 1)          # a refused graph leaves the one in place
    # 1-based indices through the raw entry point: n is then a legal index, 0 is not
    I1, J1, W1 = (np.ascontiguousarray(a) for a in (np.array([1, n], dtype=np.int64), np.array([n, 1], dtype=np.int64), np.ones(2)))
    assert hip_abi.round_set_graph(s._h, 1, 2, cabi._pl(I1), cabi._pl(J1), cabi._pd(W1)) == cabi.OK
    check_exact(s, R, gauss, (np.array([0]), np.array([n - 1]), np.ones(1)), 0)
    I0 = np.zeros(1, dtype=np.int64)
    assert hip_abi.round_set_graph(s._h, 1, 1, cabi._pl(I0), cabi._pl(J1), cabi._pd(W1)) == cabi.ERR_INVALID_ARG
    # the largest trial count
    gbig = rng.standard_normal((4096, r))
    cuts, best, _, _ = s.round(0, 4096, gbig)
    want = ref.rounding(R, gbig, (np.array([0]), np.array([n - 1]), np.ones(1)), 0)
    assert np.array_equal(cuts, want["cuts"]) and best == want["best"]
    # after reset_rank to 2r: Γ of the new height, the graph kept
    s.round_set_graph(A1)
    s.reset_rank(2 * r)
    R2 = rng.standard_normal((n, 2 * r))
    s.set_factor(cabi.F_RT, R2)
    with pytest.raises(ValueError):
        s.round(0, T, gauss)                 # the old height
    g2 = rng.standard_normal((T, 2 * r))
    for mode in (0, 1):
        check_exact(s, R2, g2, A1, mode)
    s.close()
    # before finalize
    raw = sj.DeviceSolver(hip_abi, 8, 8, 2, 0)
    with pytest.raises(sj.SdplrError) as e:
        raw.round_set_graph(A1)
    assert e.value.code == cabi.ERR_STATE
    with pytest.raises(sj.SdplrError) as e:
        raw.round(0, 1, np.zeros((1, 2)))
    assert e.value.code == cabi.ERR_STATE
    raw.close()
