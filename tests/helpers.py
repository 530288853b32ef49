"""Shared helpers of the parity tests: dense recomputation of everything the operators produce
(the reference's own checking style, test/coreop.jl:8-16,122-127) and solver construction."""
import itertools

import numpy as np
import scipy.sparse as sp

import sdplrplus_jl_amd as sj
from sdplrplus_jl_amd import cabi, problems

# the reference's unit-test grid, test/coreop.jl:46-47: seed = position in product([5,8,12],[.4,.7],[2,3])
GRID = [(seed + 1, n, p, r) for seed, (r, p, n) in
        enumerate(itertools.product([2, 3], [0.4, 0.7], [5, 8, 12]))]

FAMILIES_EQ = {
    "maxcut": problems.maxcut,
    "lovasz_theta": problems.lovasz_theta,
    "minimum_bisection": problems.minimum_bisection,
    "cutnorm": problems.cutnorm,
    "mu_conductance_0.01": lambda A: problems.mu_conductance(A, 0.01),
    "mu_conductance_0.05": lambda A: problems.mu_conductance(A, 0.05),
    "mu_conductance_0.1": lambda A: problems.mu_conductance(A, 0.1),
}


def dense(M) -> np.ndarray:
    if sp.issparse(M):
        return M.toarray()
    return M.toarray()


def make_data(family: str, seed: int, n: int, p: float):
    rng = np.random.Generator(np.random.PCG64(1000 + seed))
    A = problems.make_random_graph(n, p, rng)
    while A.nnz == 0:  # an empty graph has Vol(G) = 0 (μ-conductance bounds become infinite)
        A = problems.make_random_graph(n, p, rng)
    if family.startswith("ineq_"):
        mu = float(family.split("_")[1])
        C, As, bs, ct = problems.mu_conductance_ineq(A, mu)
        return sj.SDPData(C, As, bs, ct), C, As, bs
    C, As, bs = FAMILIES_EQ[family](A)
    return sj.SDPData(C, As, bs), C, As, bs


def primal_vio_dense(C, As, bs, R) -> np.ndarray:
    """[⟨Aᵢ, RRᵀ⟩ − bᵢ ; ⟨C, RRᵀ⟩]  (test/coreop.jl:8-16); R is n×r."""
    X = R @ R.T
    out = np.zeros(len(bs) + 1)
    for i, A in enumerate(As):
        out[i] = np.sum(dense(A) * X) - bs[i]
    out[-1] = np.sum(dense(C) * X)
    return out


def S_dense(C, As, y) -> np.ndarray:
    """Σ yᵢ·Aᵢ + y_{m+1}·C  (test/coreop.jl:122-127)."""
    S = y[-1] * dense(C)
    for i, A in enumerate(As):
        S = S + y[i] * dense(A)
    return S


def make_solver(abi, data, r, seed=0, sigma0=2.0, h=4):
    cfg = sj.BurerMonteiroConfig(σ_0=sigma0, numlbfgsvecs=h, seed=seed, printlevel=0)
    return sj.build_solver(abi, data, r, cfg), cfg


def lagrangian_dense(C, As, bs, R, lam, lam_ub, sigma) -> float:
    """ℒ of src/coreop.jl:6-9 from dense matrices."""
    pv = primal_vio_dense(C, As, bs, R)
    v = pv[:-1]
    yt = np.minimum(lam_ub, lam - sigma * v)
    return pv[-1] + np.sum(yt * yt - lam * lam) / (2 * sigma)


# ---- a third voice above FP64 ------------------------------------------------------------------------------------------
def _two_prod_terms(a: np.ndarray, b: np.ndarray) -> list:
    """a∘b as an exact sum of doubles: p = fl(a·b) and the error of that product (Veltkamp split + Dekker)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    p = a * b
    ca, cb = 134217729.0 * a, 134217729.0 * b
    ah, bh = ca - (ca - a), cb - (cb - b)
    al, bl = a - ah, b - bh
    e = ((ah * bh - p) + ah * bl + al * bh) + al * bl
    return list(p) + list(e)


def _hp_dot(a, b):
    """⟨a, b⟩ of two double vectors above FP64: extended precision where numpy has it, else math.fsum of exact products."""
    if np.finfo(np.longdouble).eps < 1e-18:
        return np.dot(np.asarray(a, dtype=np.longdouble), np.asarray(b, dtype=np.longdouble))
    import math
    return math.fsum(_two_prod_terms(a, b))


def hp_gradient(C, As, bs, R, lam, sigma) -> np.ndarray:
    """G = 2·S·R with S = C + Σ yᵢAᵢ, y = −(λ − σ·v), v = 𝒜(RRᵀ) − b (src/coreop.jl:305-317 for equality constraints),
    from dense matrices in np.longdouble (64-bit mantissa: every sum of n ≤ 10³ terms is good to ≈ n·2⁻⁶⁴).  Where
    np.longdouble is no wider than a double the sums are formed by math.fsum over exact products instead (v, y and the
    entries of S are then rounded to double once each).  R is n×r; returned n×r, as np.longdouble where that is the wider type."""
    wide = np.finfo(np.longdouble).eps < 1e-18
    ld = np.longdouble if wide else np.float64
    R64 = np.asarray(R, dtype=np.float64)
    n, r = R64.shape
    Rl = R64.astype(ld)
    if wide:
        X = Rl @ Rl.T
    else:
        X = np.array([[_hp_dot(R64[i], R64[j]) for j in range(n)] for i in range(n)])
    S = np.asarray(dense(C), dtype=np.float64).astype(ld).copy()
    for i, A in enumerate(As):
        if hasattr(A, "is_"):          # SparseMatrixCOO: ⟨A, X⟩ over its entries only
            ii, jj, vv = A.is_, A.js, A.vs
        else:
            Ad = np.asarray(dense(A), dtype=np.float64)
            ii, jj = np.nonzero(Ad)
            vv = Ad[ii, jj]
        if wide:
            v = np.sum(vv.astype(ld) * X[ii, jj]) - ld(bs[i])
            yi = -(ld(lam[i]) - ld(sigma) * v)
            np.add.at(S, (ii, jj), yi * vv.astype(ld))
        else:
            import math
            v = math.fsum(_two_prod_terms(vv, X[ii, jj]) + [-float(bs[i])])
            yi = -(float(lam[i]) - float(sigma) * v)
            np.add.at(S, (ii, jj), yi * vv)
    if wide:
        return 2 * (S @ Rl)
    G = np.empty((n, r))
    for i in range(n):
        for j in range(r):
            G[i, j] = 2.0 * _hp_dot(S[i], R64[:, j])
    return G


# ---- shared by test_gpu_handover.py and the CPU tests that pin its oracle halves -----------------------------------------
def history_state(s_, h) -> dict:
    """Everything of the factor arena and the history that can be read through the ABI."""
    S = [s_.get_factor(cabi.F_LBFGS_S + j).copy() for j in range(h)]
    Y = [s_.get_factor(cabi.F_LBFGS_Y + j).copy() for j in range(h)]
    return dict(R=s_.Rt.copy(), G=s_.Gt.copy(), D=s_.get_factor(cabi.F_DIRT).copy(), S=S, Y=Y,
                rho=s_.get_vec(cabi.V_LBFGS_RHO).copy(), y=s_.y.copy())


def same_state(a: dict, b: dict):
    for k in ("R", "G", "D", "rho", "y"):
        if a[k] is None and b[k] is None:
            continue
        assert np.array_equal(a[k], b[k], equal_nan=True), k
    for j, (x, z) in enumerate(zip(a["S"], b["S"])):
        assert np.array_equal(x, z, equal_nan=True), ("s", j)
    for j, (x, z) in enumerate(zip(a["Y"], b["Y"])):
        assert np.array_equal(x, z, equal_nan=True), ("y", j)


def not_descent_instance(route: str):
    """(data, rank, solver seed) of the not-descent recipe: fg!, a loop, G ← −G written from the host, a loop.  The direction
    −H·(−G) passes the descent test against the G it was formed from and is refused by the line search (cubic[1] > 0).
    "launches": the instance of test_ring_on_the_eager_route_and_under_the_profiler; "resident": that of
    test_resident_loop_is_run_to_run_deterministic."""
    if route == "resident":
        return problems.maxcut_data(problems.gnp_graph(300, 0.05, 7)), 8, 2
    return problems.maxcut_data(problems.gnp_graph(420, 0.03, 33)), 16, 8


def long_carry_instance():
    """The first case of test_ring_form_is_the_stored_form_bit_for_bit, with its dense matrices: (data, C, As, bs, r, seed)."""
    A = problems.gnp_graph(600, 8.0 / 600, 132)
    C, As, bs = problems.maxcut(A)
    return problems.maxcut_data(A), C, As, bs, 32, 3


def oracle_moving_iterations(oracle_abi, K: int):
    """The oracle on long_carry_instance(), K iterations one per call (bit for bit the single call of K: pinned in
    test_oracle_endtoend.py) → (number of iterations whose step α ≠ 0, the last call's result with iterations = K)."""
    data, _, _, _, r, seed = long_carry_instance()
    nC, nb = data.normC(), float(np.linalg.norm(data.b))
    o, _ = make_solver(oracle_abi, data, r, seed=seed, h=4)
    st = o.fg(nC, nb)
    moving = 0
    for _ in range(K):
        out = o.inner_loop(nC, nb, True, True, False, 0.0, -1e300, 1, 0.0, *st[:3])
        assert out[4] == 1 and out[5] == 2
        moving += out[3] != 0.0
        st = out
    o.close()
    return moving, st[:4] + (K, 2)


def carry_bound(C, y0, y1, R0, R1, K: int):
    """(T, 8·K·2⁻⁵³·T) for a MaxCut-shaped instance (unit diagonal constraints, y[-1] the cost matrix's coefficient):
    T = ‖2(|y_C|·|C| + Diag|y|)·|R|‖∞ over the entries, the larger of the loop's first and last point.  One carried step
    G_new = G_old + 2(αW + d∘R − d′∘R′) rounds fewer than eight times per entry, each time a term bounded by T."""
    absC = np.abs(dense(C))
    T = 0.0
    for y, R in ((y0, R0), (y1, R1)):
        n = R.shape[0]
        M = 2.0 * (abs(y[-1]) * absC + np.diag(np.abs(y[:n]))) @ np.abs(R)
        T = max(T, float(np.max(M)))
    return T, 8.0 * K * 2.0 ** -53 * T
