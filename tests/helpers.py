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


# ---- Lanczos / dual bound above FP64 (tests/test_lanczos_reference.py, tests/test_gpu_lanczos_steps.py) -------------------
WIDE = np.finfo(np.longdouble).eps < 1e-18
U53 = 2.0 ** -53


def _hp_terms_of(M, yi: float):
    """yi·M as (row, col, exact terms) triples: every product as a sum of doubles (used where longdouble is a double)."""
    if isinstance(M, sj.SymLowRankMatrix):
        from fractions import Fraction
        n, s = M.B.shape
        ii, jj = np.divmod(np.arange(n * n), n)
        vv = np.empty(n * n)
        for i in range(n):
            for j in range(n):
                acc = sum(Fraction(M.B[i, c]) * Fraction(M.D[c]) * Fraction(M.B[j, c]) for c in range(s))
                vv[i * n + j] = float(acc * Fraction(yi))
        return ii, jj, [vv]
    if hasattr(M, "is_"):
        ii, jj, vv = M.is_, M.js, M.vs
    elif isinstance(M, sj.Diagonal):
        ii = jj = np.arange(M.diag.size)
        vv = M.diag
    else:
        co = sp.coo_matrix(M)
        ii, jj, vv = co.row, co.col, co.data
    t = _two_prod_terms(vv, np.full(len(vv), float(yi)))
    k = len(vv)
    return np.asarray(ii), np.asarray(jj), [np.asarray(t[:k]), np.asarray(t[k:])]


def S_dense_hp(C, As, y) -> np.ndarray:
    """Σ yᵢ·Aᵢ + y_{m+1}·C (test/coreop.jl:122-127) from the matrices' own entries in np.longdouble (a low-rank matrix as
    B·D·Bᵀ in that type).  Where np.longdouble is no wider than a double every entry is the math.fsum of its exact
    product terms instead, rounded once.  That fallback (and _hp_matvec's, lanczos_hp's) is NOT exercised on x86, where
    longdouble has 64 mantissa bits; in it S·v and the dot products are correctly rounded but the vector updates of the
    recurrence are plain double operations, so the reference is then only partly above FP64."""
    mats = list(As) + [C]
    y = np.asarray(y, dtype=np.float64)
    n = C.shape[0]
    if not WIDE:
        import math
        cells = {}
        for M, yi in zip(mats, y):
            ii, jj, terms = _hp_terms_of(M, float(yi))
            for t in terms:
                for i, j, v in zip(ii, jj, t):
                    cells.setdefault((int(i), int(j)), []).append(float(v))
        S = np.zeros((n, n))
        for (i, j), ts in cells.items():
            S[i, j] = math.fsum(ts)
        return S
    ld = np.longdouble
    S = np.zeros((n, n), dtype=ld)
    for M, yi in zip(mats, y):
        yi = ld(yi)
        if isinstance(M, sj.SymLowRankMatrix):
            B = M.B.astype(ld)
            S += yi * ((B * M.D.astype(ld)) @ B.T)
        elif hasattr(M, "is_"):
            np.add.at(S, (M.is_, M.js), yi * M.vs.astype(ld))
        elif isinstance(M, sj.Diagonal):
            S[np.arange(n), np.arange(n)] += yi * M.diag.astype(ld)
        else:
            co = sp.coo_matrix(M)
            np.add.at(S, (co.row, co.col), yi * co.data.astype(ld))
    return S


def _hp_matvec(S, v):
    if WIDE:
        return S @ v
    return np.array([_hp_dot(S[i], v) for i in range(S.shape[0])])


def lanczos_hp(S, v0, q: int):
    """The recurrence of src/coreop.jl:461-500 as written — normalise, Av, α, the three-term update, β, the break test
    |β| < √n·eps(Float64) (:494), q ≤ n − 1 (:465) — in the type of S (np.longdouble from S_dense_hp; with doubles the dot
    products go through _hp_dot).  → (α[:steps], β[:steps], steps, [v_1 … v_steps])."""
    n = S.shape[0]
    q = min(int(q), n - 1)
    ty = S.dtype.type
    dot = (lambda a, b: np.dot(a, b)) if WIDE else (lambda a, b: ty(_hp_dot(a, b)))
    alpha, beta = np.zeros(q, dtype=S.dtype), np.zeros(q, dtype=S.dtype)
    v = np.asarray(v0, dtype=np.float64).astype(S.dtype)
    v = v / np.sqrt(dot(v, v))
    v_pre = np.zeros(n, dtype=S.dtype)
    it, V = 0, []
    for i in range(q):
        it += 1
        V.append(v.copy())
        Av = _hp_matvec(S, v)
        alpha[i] = dot(v, Av)
        Av = Av - alpha[i] * v if i == 0 else Av - (alpha[i] * v + beta[i - 1] * v_pre)
        beta[i] = np.sqrt(dot(Av, Av))
        if abs(beta[i]) < np.sqrt(float(n)) * np.finfo(np.float64).eps:
            break
        v_pre, v = v, Av / beta[i]
    return alpha[:it], beta[:it], it, V


def lanczos_gamma(S, lowrank: bool) -> float:
    """γ = 4·(d + ⌈log₂ n⌉ + 8)·2⁻⁵³, d the longest row of S (n where a low-rank term is present): a row of d products summed
    in any order, a dot product of n terms summed pairwise, and a handful of roundings in the step itself — times four."""
    n = S.shape[0]
    d = n if lowrank else int(np.max(np.count_nonzero(np.asarray(S, dtype=np.float64), axis=1)))
    return 4.0 * (d + int(np.ceil(np.log2(n))) + 8) * U53


def lanczos_tau(C, As, y, q: int, lowrank: bool) -> float:
    """τ = q·γ·‖|S|‖∞ of the S that y defines: every eigenvalue of the tridiagonal of a correct q-step run lies within τ of
    the spectrum's hull, and the smallest Ritz values of two correct runs on that S are asked to agree within 2τ."""
    S = S_dense_hp(C, As, y)
    return q * lanczos_gamma(S, lowrank) * float(np.max(np.sum(np.abs(S), axis=1)))


def two_step_reference(S, X, lowrank: bool) -> dict:
    """lanczos(2, x) of every column x of X above FP64, with the bounds a correct FP64 implementation meets:
    |α₁ − ref| ≤ γ·|v|ᵀ|S||v|, |β₁ − ref| ≤ γ·A, |α₂ − ref|, |β₂ − ref| ≤ κ·γ·A with A = ‖|S|‖∞, κ = 4·A/β₁.  Columns
    whose β₁ is exactly 0 are marked (live = False: the run breaks there); a live column with κ > 4e3 is an error of the
    test's construction."""
    ty = S.dtype
    X = np.asarray(X, dtype=np.float64).astype(ty)
    absS = np.abs(S)
    A = float(np.max(np.sum(absS, axis=1)))
    g = lanczos_gamma(S, lowrank)
    mv = (lambda M, V: M @ V) if WIDE else (lambda M, V: np.stack([_hp_matvec(M, V[:, k]) for k in range(V.shape[1])], axis=1))
    cdot = (lambda P, Q: np.sum(P * Q, axis=0)) if WIDE else (lambda P, Q: np.array([_hp_dot(P[:, k], Q[:, k]) for k in range(P.shape[1])]))
    V = X / np.sqrt(cdot(X, X))
    W = mv(S, V)
    a1 = cdot(V, W)
    R = W - a1 * V
    b1 = np.sqrt(cdot(R, R))
    live = np.asarray(b1 != 0)
    safe = np.where(live, b1, 1)
    V2 = R / safe
    W2 = mv(S, V2)
    a2 = cdot(V2, W2)
    R2 = W2 - (a2 * V2 + b1 * V)
    b2 = np.sqrt(cdot(R2, R2))
    kappa = 4.0 * A / np.asarray(safe, dtype=np.float64)
    assert np.all(kappa[live] <= 4e3), ("ill-conditioned probe", float(np.max(kappa[live])))
    vSv = np.asarray(cdot(np.abs(V), mv(absS, np.abs(V))), dtype=np.float64)
    return dict(a1=a1, b1=b1, a2=a2, b2=b2, live=live, A=A, gamma=g, kappa=kappa,
                bound_a1=g * vSv, bound_b1=np.full(X.shape[1], g * A), bound_2=kappa * g * A)


def two_step_ratio(ref: dict, k: int, al, be) -> float:
    """Largest error/bound ratio of one probe's (α₁, β₁, α₂, β₂) against column k of two_step_reference."""
    ty = ref["a1"].dtype.type
    out = [abs(ty(al[0]) - ref["a1"][k]) / ref["bound_a1"][k] if ref["bound_a1"][k] > 0 else (0.0 if ty(al[0]) == ref["a1"][k] else np.inf),
           abs(ty(be[0]) - ref["b1"][k]) / ref["bound_b1"][k],
           abs(ty(al[1]) - ref["a2"][k]) / ref["bound_2"][k],
           abs(ty(be[1]) - ref["b2"][k]) / ref["bound_2"][k]]
    return float(max(out))


def _weighted_graph(A, n_weights: int, rng):
    """The graph of A with integer-multiple-of-½ weights, every one of the n_weights values present."""
    A = sp.coo_matrix(A)
    up = A.row < A.col
    w = 0.5 * rng.integers(1, n_weights + 1, size=int(up.sum())).astype(float)
    k = min(n_weights, w.size)
    w[:k] = 0.5 * np.arange(1, k + 1)
    r, c = A.row[up], A.col[up]
    return sp.coo_matrix((np.concatenate([w, w]), (np.concatenate([r, c]), np.concatenate([c, r]))), shape=A.shape).tocsc()


def _drop_vertex(A, j: int):
    """A without the edges of vertex j: a row of S with no off-diagonal entry."""
    A = sp.lil_matrix(A)
    A[j, :] = 0
    A[:, j] = 0
    A = sp.csc_matrix(A)
    A.eliminate_zeros()
    return A


# name → (family, n, band plans (BW, CH) forced on, hub threshold, has a low-rank term)
LANCZOS_INSTANCES = {
    "maxcut150": ("maxcut", 150, [(64, 16), (64, 7), (128, 40)], None, False),
    "maxcut257_hubs": ("maxcut", 257, [(64, 16)], 8, False),
    "wmaxcut300_w3": ("maxcut", 300, [(128, 40)], None, False),
    "wmaxcut300_w400": ("maxcut", 300, [(128, 40)], None, False),
    "minbis150": ("minimum_bisection", 150, [(64, 7)], None, True),
    "lovasz150": ("lovasz_theta", 150, [(64, 16)], None, True),
    "lowrank60_3+6": ("two_lowrank", 60, [], None, True),
    "lowrank60_8": ("one_lowrank", 60, [], None, True),
}
_LZ_CACHE = {}


def lanczos_instance(name: str) -> dict:
    """One instance of the Lanczos step tests, built once: the data, its matrices, a seeded y (the same S on every side),
    S above FP64, the start vectors (eight Gaussian ones, e_j of EVERY row — each row is the last of a band, chunk or slice
    on some plan — e_j + e_{j+1} of every adjacent pair, first + last, each hub row with a neighbour, the isolated row with
    a neighbour) and their two-step reference."""
    if name in _LZ_CACHE:
        return _LZ_CACHE[name]
    family, n, plans, hub, lowrank = LANCZOS_INSTANCES[name]
    rng = np.random.Generator(np.random.PCG64(4400 + sorted(LANCZOS_INSTANCES).index(name)))
    iso = None
    if family in ("maxcut", "minimum_bisection", "lovasz_theta"):
        p = {150: 0.08, 257: 0.03, 300: 0.08}[n]
        A = problems.gnp_graph(n, p, 21 + n)
        iso = n // 3
        A = _drop_vertex(A, iso)
        if name.startswith("wmaxcut"):
            A = _weighted_graph(A, int(name.split("_w")[1]), rng)
        C, As, bs = FAMILIES_EQ[family](A)
    else:
        def sym_sparse(density):
            M = sp.random(n, n, density=density, random_state=np.random.RandomState(int(rng.integers(1 << 30))), format="csr")
            M = sp.triu(M, k=1)
            return sp.csc_matrix(M + M.T + sp.diags(rng.standard_normal(n)))
        lr = lambda s: sj.SymLowRankMatrix(rng.standard_normal(s), rng.standard_normal((n, s)))
        C = sym_sparse(0.2)
        As = ([lr(3), lr(6)] if family == "two_lowrank" else [lr(8)]) + \
             [sj.SparseMatrixCOO([i], [i], [1.0 + i], n, n) for i in range(n)]
        bs = rng.standard_normal(len(As))
    data = sj.SDPData(C, As, bs)
    y = rng.standard_normal(data.m + 1)
    S = S_dense_hp(C, As, y)
    S64 = np.asarray(S, dtype=np.float64)
    cols, labels = [], []
    for k in range(8):
        cols.append(rng.standard_normal(n)); labels.append(f"gauss{k}")
    E = np.eye(n)
    for j in range(n):
        cols.append(E[j]); labels.append(f"e{j}")
    pairs = [(j, j + 1) for j in range(n - 1)] + [(0, n - 1)]
    offd = S64 - np.diag(np.diag(S64))
    deg = np.count_nonzero(S64, axis=1)
    if hub is not None:
        hubs = [int(j) for j in np.nonzero(deg > hub)[0]]
        assert hubs and len(hubs) < n, "the instance needs hub rows and ordinary rows"
        pairs += [(j, int(np.nonzero(offd[j])[0][0])) for j in hubs]
    if iso is not None and not lowrank:
        assert not offd[iso].any()
        pairs.append((iso, int(np.nonzero(offd[(iso + 1) % n])[0][0])))
    for i, j in pairs:
        cols.append(E[i] + E[j]); labels.append(f"e{i}+e{j}")
    X = np.ascontiguousarray(np.stack(cols, axis=1))
    ref = two_step_reference(S, X, lowrank)
    out = dict(name=name, family=family, n=n, plans=plans, hub=hub, lowrank=lowrank, data=data, C=C, As=As, bs=bs, y=y,
               S=S, S64=S64, X=X, labels=labels, ref=ref, iso=iso)
    _LZ_CACHE[name] = out
    return out


def two_step_max_ratio(inst: dict, solver) -> float:
    """lanczos(2, x) of every live start vector of the instance on `solver` (y set, S assembled) → the largest
    error/bound ratio."""
    ref, worst = inst["ref"], 0.0
    for k in range(inst["X"].shape[1]):
        if not ref["live"][k]:
            continue
        al, be, st = solver.lanczos(2, inst["X"][:, k])
        assert st == 2, (inst["labels"][k], st)
        r = two_step_ratio(ref, k, al, be)
        worst = max(worst, r)
    return worst


def set_S(solver, y):
    solver.y = y
    solver.At_preprocess()
    return solver


def whole_run_checks(inst: dict, al, be, q: int):
    """What any correct finite-precision Lanczos run of q steps satisfies against the spectrum Λ of S (eigvalsh of S above
    FP64 rounded to double): every eigenvalue of T inside [λ_min − τ, λ_max + τ], τ = q·γ·A; every Ritz value θ whose
    residual estimate β_q·|s_q| is below 1e-8·A within √q·γ·A + 1e-8·A of Λ (Paige; ghost copies allowed).  → τ."""
    ref = inst["ref"]
    A, g = ref["A"], ref["gamma"]
    lam = inst.setdefault("eig", np.linalg.eigvalsh(inst["S64"]))
    tau = q * g * A
    al, be = np.asarray(al, dtype=float), np.asarray(be, dtype=float)
    k = al.size
    T = np.diag(al) + np.diag(be[:k - 1], 1) + np.diag(be[:k - 1], -1)
    th, s = np.linalg.eigh(T)
    assert lam[0] - tau <= th[0] and th[-1] <= lam[-1] + tau, (th[0] - lam[0], th[-1] - lam[-1], tau)
    resid = abs(be[k - 1]) * np.abs(s[-1, :])
    conv = resid < 1e-8 * A
    if conv.any():
        dist = np.min(np.abs(th[conv][:, None] - lam[None, :]), axis=1)
        assert np.all(dist <= np.sqrt(q) * g * A + 1e-8 * A), (float(np.max(dist)), np.sqrt(q) * g * A + 1e-8 * A)
    return tau


def break_instance(n: int = 150):
    """S = (Diag(1..n) + [[1, 1], [1, 0]] on rows 3, 4)/64 as a MaxCut instance whose graph has the one edge {3, 4}: the
    block is [[5, 1], [1, 5]]/64, e₃ ± e₄ are eigenvectors (break at step 1), e₃ spans a 2-dimensional invariant subspace
    (break at step 2, β₂ = 0 exactly).  The factor 2⁻⁶ keeps the round-off of the e₃ ± e₄ runs (a few ulp of 6/64·2^-½ ≈
    1e-17) a hundred times below the ABSOLUTE break threshold √n·ε of src/coreop.jl:494, so no run here breaks — or fails
    to — by a coincidence of rounding.  → (data, y, S above FP64)."""
    A = sp.coo_matrix(([1.0, 1.0], ([3, 4], [4, 3])), shape=(n, n)).tocsc()
    C, As, bs = problems.maxcut(A)
    y = np.arange(1.0, n + 1) / 64
    y[3] = y[4] = 6.0 / 64                      # S_jj = y_j + y_C·C_jj = 6/64 − 1/64 = 5/64
    y = np.concatenate([y, [1.0 / 16]])         # C = −¼L: S_34 = y_C·¼ = 1/64, C_jj = −¼
    S = S_dense_hp(C, As, y)
    return sj.SDPData(C, As, bs), y, S


# ---- L-BFGS direction and exact line search above FP64 (tests/test_direction_linesearch_reference.py,
# ---- tests/test_gpu_direction_linesearch.py) -------------------------------------------------------------------------------
LD = np.longdouble


def _ld(a):
    return np.asarray(a, dtype=np.float64).astype(LD)


def two_loop_hp(G, S_list, Y_list, latest: int, negate: bool = True) -> dict:
    """The recursion of src/lbfgs.jl:77-124 as written — every dot taken on the running vector — in np.longdouble, on the
    FP64 arrays read back from a handle (slot j of the handle = S_list[j], Y_list[j]; `latest` 1-based as the reference
    keeps it).  ρ_j is recomputed as 1/⟨y_j, s_j⟩; a slot whose ⟨y_j, s_j⟩ is exactly 0 is an empty (cleared) one: ρ_j = 0
    as lbfgs_clear! leaves it, so its α and γ vanish.  → dir, descent = ⟨dir, G⟩, alpha and gamma by slot, rho by slot, and
    the termwise magnitude M = |G| + Σ|α_l||y_l| + Σ|γ_l||s_l| elementwise (what the final combination's terms add up to in
    absolute value: any evaluation of dir rounds against it)."""
    shape = np.shape(G)
    g = _ld(G).ravel()
    h = len(S_list)
    d = g.copy()
    M = np.abs(g)
    al, ga, rho = np.zeros(h, dtype=LD), np.zeros(h, dtype=LD), np.zeros(h, dtype=LD)
    if h == 0:              # :88-91: returns before the negation
        return dict(dir=d.reshape(shape), descent=np.dot(d, g), alpha=al, gamma=ga, rho=rho, M=M.reshape(shape),
                    run=dict(e=0.0, desc=float((g.size + 1) * LD(U53) * np.dot(np.abs(d), np.abs(g))), a=0.0))
    S = [_ld(s).ravel() for s in S_list]
    Y = [_ld(y).ravel() for y in Y_list]
    # Running error bound of the LITERAL recursion in FP64, to first order and for ANY order of its sums (a dot of N terms
    # within (N + 1)·u of Σ|terms|): E bounds |d_fp − d| elementwise, ea[j] |α_fp − α|.  Per stage: the dot inherits ⟨|v|, E⟩
    # and adds its own (N + 1)u⟨|v|, |d| + E⟩; ρ_j = fl(1/fl⟨y, s⟩) is off by (N + 1)u·⟨|y|, |s|⟩/|⟨y, s⟩| + 2u relative; the
    # coefficient's product rounds once; the axpy rounds its product and its sum.  Times 1.01 for the second-order terms.
    u, N = LD(U53), g.size
    gd = (N + 1) * u
    E, ea, erho = np.zeros(N, dtype=LD), np.zeros(h, dtype=LD), np.zeros(h, dtype=LD)
    for j in range(h):
        ys = np.dot(Y[j], S[j])
        rho[j] = 1 / ys if ys != 0 else LD(0)
        erho[j] = gd * np.dot(np.abs(Y[j]), np.abs(S[j])) / abs(ys) + 2 * u if ys != 0 else LD(0)
    j = int(latest) - 1
    for _ in range(h):      # :93-102, newest → oldest
        sd = np.dot(S[j], d)
        e_sd = np.dot(np.abs(S[j]), E) + gd * np.dot(np.abs(S[j]), np.abs(d) + E)
        al[j] = rho[j] * sd
        ea[j] = LD(1.01) * (abs(rho[j]) * e_sd + (erho[j] + u) * abs(al[j]))
        d = d - al[j] * Y[j]
        E = LD(1.01) * (E + ea[j] * np.abs(Y[j]) + u * (np.abs(d) + 2 * abs(al[j]) * np.abs(Y[j])))
        M = M + np.abs(al[j]) * np.abs(Y[j])
        j = h - 1 if j <= 0 else j - 1
    j = int(latest) % h
    for _ in range(h):      # :104-113, oldest → newest
        yd = np.dot(Y[j], d)
        e_yd = np.dot(np.abs(Y[j]), E) + gd * np.dot(np.abs(Y[j]), np.abs(d) + E)
        beta = rho[j] * yd
        ga[j] = al[j] - beta
        eg = LD(1.01) * (ea[j] + abs(rho[j]) * e_yd + (erho[j] + u) * abs(beta) + u * abs(ga[j]))
        d = d + ga[j] * S[j]
        E = LD(1.01) * (E + eg * np.abs(S[j]) + u * (np.abs(d) + 2 * abs(ga[j]) * np.abs(S[j])))
        M = M + np.abs(ga[j]) * np.abs(S[j])
        j = 0 if j == h - 1 else j + 1
    if negate:
        d = -d
    run = dict(e=float(np.sqrt(np.sum(E * E)) / np.sqrt(np.sum(d * d))),
               desc=float(np.dot(E, np.abs(g)) + gd * np.dot(np.abs(d) + E, np.abs(g))),
               a=float(np.sqrt(np.sum(ea * ea)) / np.sqrt(np.sum(al * al))) if np.any(al != 0) else 0.0)
    return dict(dir=d.reshape(shape), descent=np.dot(d, g), alpha=al, gamma=ga, rho=rho, M=M.reshape(shape), run=run)


def direction_gamma(h: int, N: int) -> float:
    """γ = (2h + 4 + ⌈log₂ N⌉)·u: 2h + 1 terms combined one after the other, each product rounded once, the coefficients'
    own last rounding, and a pairwise dot of N terms where one follows."""
    return (2 * h + 4 + int(np.ceil(np.log2(max(N, 2))))) * U53


def direction_errors(hp: dict, dirt, descent, a=None) -> dict:
    """e = ‖dir − dir_hp‖₂/‖dir_hp‖₂, |descent − descent_hp|, ‖a − α_hp‖₂/‖α_hp‖₂ of one evaluation against two_loop_hp."""
    dd = _ld(dirt) - hp["dir"]
    nrm = np.sqrt(np.sum(hp["dir"] ** 2))
    out = dict(e=float(np.sqrt(np.sum(dd ** 2)) / nrm), desc=float(abs(LD(descent) - hp["descent"])))
    if a is not None and len(hp["alpha"]):
        na = np.sqrt(np.sum(hp["alpha"] ** 2))
        out["a"] = float(np.sqrt(np.sum((_ld(a) - hp["alpha"]) ** 2)) / na) if na > 0 else 0.0
    return out


def direction_scales(hp: dict, G, S_list, h: int) -> dict:
    """The termwise parts of the bounds of check 1: γ·max(M)/‖dir_hp‖∞ for dir, γ·Σ M|G| for descent,
    γ·max_j |ρ_j|⟨|s_j|, M⟩/‖α_hp‖∞ for the coefficients (M dominates the running vector's terms at every stage)."""
    N = int(np.size(G))
    g = direction_gamma(h, N)
    M = hp["M"].ravel()
    out = dict(gamma=g, e=float(g * np.max(M) / np.max(np.abs(hp["dir"]))),
               desc=float(g * np.sum(M * np.abs(_ld(G).ravel()))))
    if h and np.max(np.abs(hp["alpha"])) > 0:
        sc = max(abs(hp["rho"][j]) * np.dot(np.abs(_ld(S_list[j]).ravel()), M) for j in range(h))
        out["a"] = float(g * sc / np.max(np.abs(hp["alpha"])))
    else:
        out["a"] = 0.0
    return out


def spd_quadratic(N: int, kappa: float, seed: int):
    """H = Q·Diag(1 … κ, log-spaced)·Qᵀ in np.longdouble from a double Q (QR of a Gaussian matrix): symmetric positive
    definite exactly, condition number κ up to the few ulp by which Q misses orthogonality; and a start point."""
    rng = np.random.Generator(np.random.PCG64(9100 + seed))
    Q, _ = np.linalg.qr(rng.standard_normal((N, N)))
    ev = np.logspace(0.0, np.log10(kappa), N) if N > 1 else np.array([kappa])
    Ql = Q.astype(LD)
    H = (Ql * ev.astype(LD)) @ Ql.T
    H = (H + H.T) / 2
    return H, rng.standard_normal(N).astype(LD)


def history_snapshot(s_, h: int) -> dict:
    return dict(G=s_.Gt.copy(), S=[s_.get_factor(cabi.F_LBFGS_S + j).copy() for j in range(h)],
                Y=[s_.get_factor(cabi.F_LBFGS_Y + j).copy() for j in range(h)],
                rho=s_.get_vec(cabi.V_LBFGS_RHO).copy() if h else np.zeros(0),
                latest=int(s_.get_scalar(cabi.S_LBFGS_LATEST)) if h else 0)


def drive_quadratic_history(s_, h: int, kappa: float, seed: int, updates: int, repeat_at: int = -1) -> list:
    """An L-BFGS history built through the ABI on the handle s_ (so it holds exactly the s, y, ρ a solve would leave): the
    gradient field G(x) = fl(H·x) of spd_quadratic on N = n·r unknowns, Gt = G, lbfgs_dir(negate), the step α of the exact
    line search −⟨d, Hx⟩/⟨d, Hd⟩ above FP64, x += α·d, Gt = G(x), lbfgs_update(α) — `updates` times, then one more
    direction with negate = False.  repeat_at = k: at update k the direction is replaced from the host by the previous
    one times (1 + 1e-9·ξ), ξ uniform in [−1, 1] — two consecutive pairs whose s differ by 1e-9 relative.
    → one snapshot per direction: the state read back BEFORE the call (G, S, Y, rho, latest) and what the call returned
    (dir, descent, a, negate).  The quadratic is homogeneous and, where N is not much larger than h, solved to round-off in
    N steps and then again by sixteen orders of magnitude per cycle: 3h + 2 updates would leave the doubles.  So whenever
    ‖G‖ has fallen below 1e-10·‖G₀‖ — far inside the regime ‖q‖ ≪ ‖G‖ the histories are for — the quadratic's centre jumps to
    a fresh Gaussian point of the start point's size, G(x) = fl(H·(x − c)): the pair formed across the jump is one of a
    function that is not quadratic, all others satisfy y = H·s to round-off."""
    n, r = s_.n, s_.r
    H, x = spd_quadratic(n * r, kappa, seed)
    rng = np.random.Generator(np.random.PCG64(77 + seed))
    s_.lbfgs_clear()
    snaps, prev = [], None
    c, x0n = np.zeros(n * r, dtype=LD), np.sqrt(np.sum(x * x))
    G = np.asarray(H @ x, dtype=np.float64).reshape(n, r)
    g0 = float(np.linalg.norm(G))
    for k in range(updates + 1):
        s_.Gt = G
        snap = history_snapshot(s_, h)
        negate = k < updates
        snap["descent"] = s_.lbfgs_dir(negate)
        snap["dir"], snap["negate"] = s_.dirt.copy(), negate
        snap["a"] = s_.get_vec(cabi.V_LBFGS_A).copy() if h else np.zeros(0)
        snaps.append(snap)
        if not negate:
            break
        d64 = snap["dir"]
        if k == repeat_at and prev is not None:
            d64 = prev * (1.0 + 1e-9 * rng.uniform(-1.0, 1.0, size=prev.shape))
            s_.dirt = d64
        d = d64.astype(LD).ravel()
        alpha = float(-np.dot(d, H @ (x - c)) / np.dot(d, H @ d))
        if k == repeat_at and prev is not None:
            alpha = snaps[-2]["step"]        # the same step length again: s repeats to 1e-9, not just its direction
        x = x + LD(alpha) * d
        G = np.asarray(H @ (x - c), dtype=np.float64).reshape(n, r)
        if float(np.linalg.norm(G)) < 1e-10 * g0:
            snap["jump"] = True
            c = c + x0n * rng.standard_normal(n * r).astype(LD) / np.sqrt(LD(n * r))
            G = np.asarray(H @ (x - c), dtype=np.float64).reshape(n, r)
        s_.Gt = G
        s_.lbfgs_update(alpha)
        prev = d64.copy()                # the direction s was formed from
        snap["step"] = alpha
    return snaps


def load_history(o, snap: dict, h: int):
    """A snapshot's state into another handle of the same (n, r, h): the slots, ρ, latest and G."""
    for j in range(h):
        o.set_factor(cabi.F_LBFGS_S + j, snap["S"][j])
        o.set_factor(cabi.F_LBFGS_Y + j, snap["Y"][j])
    if h:
        o.set_vec(cabi.V_LBFGS_RHO, snap["rho"])
        o.set_scalar(cabi.S_LBFGS_LATEST, float(snap["latest"]))
    o.Gt = snap["G"]


def check_direction_snapshots(snaps: list, h: int, oracle_solver, literal: bool = False) -> dict:
    """Check 1 on every snapshot: the literal FP64 evaluation (the oracle, on the same state) gives e_lit; the evaluation
    under test must meet e ≤ 8·e_lit + γ·max(M)/‖dir_hp‖∞, and the same for descent (scale ΣM|G|) and the coefficients.
    literal = True (the evaluation under test IS the literal recursion, in another summation order): e_lit is then ONE sample
    of the same error distribution, and on few unknowns the ratio of two such samples exceeds 8 every dozen draws (for two
    half-normal magnitudes P(ratio > 8) = (2/π)·atan(1/8) ≈ 8 %); such an evaluation is held to the larger of the bound above
    and the running bound of two_loop_hp, which every correct literal evaluation meets whatever its order.
    → per quantity the largest error/bound with its step, the largest e/e_lit, the literal evaluation's own largest
    error/running bound (≤ 1 shows the running bound attainable), the number of centre jumps, and the failures as text."""
    worst = dict(ratio_lit=0.0, dir=0.0, desc=0.0, a=0.0, lit_dir=0.0, lit_run=0.0, run=0.0)
    bad = []
    for k, sn in enumerate(snaps):
        hp = two_loop_hp(sn["G"], sn["S"], sn["Y"], sn["latest"], sn["negate"])
        load_history(oracle_solver, sn, h)
        dl = oracle_solver.lbfgs_dir(sn["negate"])
        lit = direction_errors(hp, oracle_solver.dirt, dl, oracle_solver.get_vec(cabi.V_LBFGS_A) if h else None)
        err = direction_errors(hp, sn["dir"], sn["descent"], sn["a"] if h else None)
        sc = direction_scales(hp, sn["G"], sn["S"], h)
        worst["lit_dir"] = max(worst["lit_dir"], lit["e"] / sc["e"])
        if lit["e"] > 0:
            worst["ratio_lit"] = max(worst["ratio_lit"], err["e"] / lit["e"])
        for key, name in (("e", "dir"), ("desc", "desc"), ("a", "a")):
            if key not in err:
                continue
            if hp["run"][key] > 0:
                worst["lit_run"] = max(worst["lit_run"], lit[key] / hp["run"][key])
                worst["run"] = max(worst["run"], err[key] / hp["run"][key])
            bound = 8 * lit[key] + sc[key]
            if literal:
                bound = max(bound, hp["run"][key])
            ratio = err[key] / bound if bound > 0 else (0.0 if err[key] == 0 else np.inf)
            worst[name] = max(worst[name], ratio)
            if not ratio <= 1.0:
                bad.append(f"step {k} {name}: err {err[key]:.3g} lit {lit[key]:.3g} termwise {sc[key]:.3g} ratio {ratio:.3g}")
    return dict(worst=worst, bad=bad, jumps=sum(1 for sn in snaps if sn.get("jump")))


# -- the exact line search ---------------------------------------------------------------------------------------------------
def _mat_hp(M) -> np.ndarray:
    if isinstance(M, sj.SymLowRankMatrix):
        B = M.B.astype(LD)
        return (B * M.D.astype(LD)) @ B.T
    if hasattr(M, "is_"):           # SparseMatrixCOO: its entries, duplicates added
        out = np.zeros((M.n, M.n) if hasattr(M, "n") else M.shape, dtype=LD)
        np.add.at(out, (np.asarray(M.is_), np.asarray(M.js)), np.asarray(M.vs, dtype=np.float64).astype(LD))
        return out
    return np.asarray(dense(M), dtype=np.float64).astype(LD)


def loop_state_direction(sn: dict, h: int, oracle_solver) -> dict:
    """The direction of the iteration that follows a loop's state (history_snapshot of a handle after k iterations): above
    FP64, with the literal FP64 evaluation (the oracle's lbfgs_dir on the same state) as e_lit, the termwise scales, and
    whether the sign of descent_hp is decided: |descent_hp| > 8·|descent_lit − descent_hp| + γ·ΣM|G| (check 3)."""
    hp = two_loop_hp(sn["G"], sn["S"], sn["Y"], sn["latest"], True)
    load_history(oracle_solver, sn, h)
    dl = oracle_solver.lbfgs_dir(True)
    lit = direction_errors(hp, oracle_solver.dirt, dl)
    sc = direction_scales(hp, sn["G"], sn["S"], h)
    return dict(hp=hp, lit=lit, sc=sc, decided=bool(abs(float(hp["descent"])) > 8 * lit["desc"] + sc["desc"]))


def quartic_hp(C, As, bs, R, D, lam, pv_raw, obj, sigma) -> dict:
    """src/linesearch.jl:8-56 in np.longdouble from dense matrices: A_RD = 𝒜(RDᵀ + DRᵀ) (with its ×2, :13), A_DD = 𝒜(DDᵀ)
    (both of length m + 1, the cost matrix last), the quartic's coefficients b_0 … b_4 (:44-56) with p0 = obj and −q0 =
    pv_raw[:m] as given — and for each output the sum of the magnitudes of its terms (A_RD_mag, A_DD_mag, b_mag): the
    scale any FP64 evaluation of it rounds against.  bs is not read (pv_raw carries it); kept for the call's symmetry."""
    Rl, Dl = _ld(R), _ld(D)
    X, XX = Rl @ Dl.T, Dl @ Dl.T
    X = X + X.T
    aX = np.abs(Rl) @ np.abs(Dl).T
    aX, aXX = aX + aX.T, np.abs(Dl) @ np.abs(Dl).T
    mats = list(As) + [C]
    m = len(As)
    q1, q2, q1m, q2m = (np.zeros(m + 1, dtype=LD) for _ in range(4))
    for i, A in enumerate(mats):
        Al = _mat_hp(A)
        q1[i], q2[i] = np.sum(Al * X), np.sum(Al * XX)
        q1m[i], q2m[i] = np.sum(np.abs(Al) * aX), np.sum(np.abs(Al) * aXX)
    lam_, nq0, sg, p0 = _ld(lam), _ld(pv_raw)[:m], LD(sigma), LD(obj)
    a1, a2, m1, m2 = q1[:m], q2[:m], q1m[:m], q2m[:m]
    al, an = np.abs(lam_), np.abs(nq0)
    b = np.array([p0 - np.dot(lam_, nq0) + sg * np.dot(nq0, nq0) / 2,
                  q1[m] - np.dot(lam_, a1) + sg * np.dot(nq0, a1),
                  q2[m] - np.dot(lam_ - sg * nq0, a2) + sg * np.dot(a1, a1) / 2,
                  sg * np.dot(a1, a2),
                  sg * np.dot(a2, a2) / 2], dtype=LD)
    bm = np.array([abs(p0) + np.dot(al, an) + sg * np.dot(an, an) / 2,
                   q1m[m] + np.dot(al, m1) + sg * np.dot(an, m1),
                   q2m[m] + np.dot(al + sg * an, m2) + sg * np.dot(m1, m1) / 2,
                   sg * np.dot(m1, m2),
                   sg * np.dot(m2, m2) / 2], dtype=LD)
    return dict(A_RD=q1, A_DD=q2, A_RD_mag=q1m, A_DD_mag=q2m, b=b, b_mag=bm)


def poly_hp(b, a):
    a = LD(a)
    v = LD(0)
    for c in b[::-1]:
        v = v * a + LD(c)
    return v


def poly_T(b, a) -> float:
    """T(α) = Σ|b_k|·α^k."""
    return float(poly_hp(np.abs(np.asarray(b, dtype=LD)), abs(a)))


def quartic_min_hp(b, alpha_max) -> dict:
    """The global minimum of b_0 + … + b_4·α⁴ over [0, α_max] in np.longdouble: the stationary points from np.roots on the
    derivative (real parts of all of them — a pair that rounding made complex still marks where the derivative nearly
    vanishes), polished by Newton in long double and kept where they stay inside, both end points, and — as a guard against
    a stationary point np.roots misplaced — the best point of a 4001-point grid refined by ternary search; the smallest
    value wins.  → alpha, fmin, and T = poly_T(b, ·)."""
    b = np.asarray(b, dtype=LD)
    amax = LD(alpha_max)
    db = np.array([k * b[k] for k in range(1, 5)], dtype=LD)
    ddb = np.array([k * db[k] for k in range(1, 4)], dtype=LD)
    cands = [LD(0), amax]
    d64 = np.asarray(db, dtype=np.float64)
    if np.all(np.isfinite(d64)) and np.any(d64 != 0):
        for z in np.roots(d64[::-1]):
            x = LD(z.real)
            for _ in range(8):
                fp, fpp = poly_hp(db, x), poly_hp(ddb, x)
                if fpp == 0 or not np.isfinite(fp / fpp):
                    break
                x = x - fp / fpp
            for c in (LD(z.real), x):
                if np.isfinite(c) and 0 <= c <= amax:
                    cands.append(c)
    grid = amax * np.arange(4001, dtype=LD) / 4000
    vals = b[0] + grid * (b[1] + grid * (b[2] + grid * (b[3] + grid * b[4])))
    k = int(np.argmin(vals))
    lo, hi = grid[max(k - 1, 0)], grid[min(k + 1, 4000)]
    for _ in range(200):
        m1, m2 = lo + (hi - lo) / 3, hi - (hi - lo) / 3
        if poly_hp(b, m1) <= poly_hp(b, m2):
            hi = m2
        else:
            lo = m1
    cands.append((lo + hi) / 2)
    fv = [poly_hp(b, c) for c in cands]
    i = int(np.argmin(fv))
    return dict(alpha=cands[i], fmin=fv[i], T=lambda a: poly_T(b, a))


LS_T = (1.0, 1e-2, 1e-4, 1e-6)
LS_AMAX = (1e-3, 0.5, 1.0, 4.0)
LS_RECIPES = ("three_roots", "near_double", "beyond", "zero_plus")
LS_SIGMA = 2.0
_LS_CACHE = {}


def linesearch_base(family: str, r: int) -> dict:
    """(seed, n, p) = (2, 12, 0.4) of `family` with a seeded Gaussian R (n×r), σ = 2, a seeded λ₀, the violation
    𝒜(RRᵀ) − b and objective at R, and G = ∇ℒ(R; λ₀) above FP64 (hp_gradient) rounded to double."""
    key = (family, r)
    if key not in _LS_CACHE:
        data, C, As, bs = make_data(family, 2, 12, 0.4)
        rng = np.random.Generator(np.random.PCG64(5200 + 7 * r + sorted(FAMILIES_EQ).index(family)))
        R = rng.standard_normal((data.n, r))
        lam0 = rng.standard_normal(data.m)
        Rl = R.astype(LD)
        XX = Rl @ Rl.T
        pv = np.array([np.sum(_mat_hp(A) * XX) for A in As] + [np.sum(_mat_hp(C) * XX)], dtype=LD)
        pv[:data.m] -= _ld(bs)
        G = np.asarray(hp_gradient(C, As, bs, R, lam0, LS_SIGMA), dtype=np.float64)
        _LS_CACHE[key] = dict(family=family, r=r, data=data, C=C, As=As, bs=bs, R=R, G=G, pv_raw=np.asarray(pv, dtype=np.float64),
                              nnz=[int(np.count_nonzero(np.asarray(_mat_hp(A), dtype=np.float64))) for A in list(As) + [C]])
    return _LS_CACHE[key]


def linesearch_state(base: dict, t: float, amax: float, recipe: str):
    """One line-search state: D = fl(t·D₀), D₀ = ±c·G with sign and c such that the derivative's roots sum to 0.9·α_max at
    t = 1 (the sum is −3b₃/4b₄ = −3⟨q1, q2⟩/2‖q2‖², a property of R and D alone), and λ chosen above FP64 so that b₁ and b₂
    — the two coefficients λ moves — give the derivative 4b₄·Π(α − ρ_i) the roots of the recipe (the third root or the real
    part of a complex pair follows from the fixed sum):
      three_roots   ρ = Σ·(1/6, 1/3, 1/2), all inside (0, α_max): needs Σ/2 < α_max, i.e. t = 1
      near_double   ρ, ρ·(1 + 1e-9) with ρ = 0.3·α_max, the third root Σ − ρ₁ − ρ₂ > 0
      beyond        one real root 2·α_max and a complex pair: the derivative is negative on [0, α_max]
      zero_plus     one real root 1e-9·α_max and a complex pair: the minimiser is at 0⁺
    λ = x₁q1 + x₂q2 on all but two components, rounded, then the two left out absorb what the rounding moved (they are of
    the size of that residual, so their own rounding is ≈ 2⁻¹⁰⁶ relative).  pv_raw and obj are the true ones at R.
    The structure is claimed (claimed = True, asserted above FP64 in tests/test_direction_linesearch_reference.py) at
    t ≥ 1e-2 only.  b₁ … b₄ scale as t¹ … t⁴, so roots of the size of α_max ask b₁ to cancel to ≈ t²·α_max² of its terms; from
    t = 1e-4 on that is below what FP64 — and soon long double — resolves of the state, and the recipe is only where λ was
    aimed.  What those states pin is the scaling b_k ∝ |D|^k, the quadratic branch |4b₄| < eps (:70), and a λ whose b₁ and
    b₂ are differences of much larger terms: A_RD, A_DD, ℒ, the optimality gap and the commit are checked on them as on
    every state, against the quartic the state really has.
    → None where the recipe cannot be met (three_roots at t < 1), else the arrays to set and the targets."""
    C, As, bs, R, G, pv_raw = (base[k] for k in ("C", "As", "bs", "R", "G", "pv_raw"))
    m = len(As)
    sg = LD(LS_SIGMA)
    z = np.zeros(m)
    q = quartic_hp(C, As, bs, R, -G, z, pv_raw, pv_raw[m], LS_SIGMA)
    sum_unit = -3 * q["b"][3] / (4 * q["b"][4])
    c = float(abs(sum_unit) / (LD(0.9) * LD(amax)))
    D = np.asarray(t * (np.sign(float(sum_unit)) * c * (-G)), dtype=np.float64)
    q = quartic_hp(C, As, bs, R, D, z, pv_raw, pv_raw[m], LS_SIGMA)
    b3, b4 = q["b"][3], q["b"][4]
    Sm = -3 * b3 / (4 * b4)
    am = LD(amax)
    if recipe == "three_roots":
        if not Sm / 2 < am:
            return None
        roots = (Sm / 6, Sm / 3, Sm / 2)
        e2, e3 = roots[0] * roots[1] + roots[0] * roots[2] + roots[1] * roots[2], roots[0] * roots[1] * roots[2]
    elif recipe == "near_double":
        r1 = LD(0.3) * am
        r2 = r1 * (1 + LD(1e-9))
        r3 = Sm - r1 - r2
        if not r3 > 0:
            return None
        roots = (r1, r2, r3)
        e2, e3 = r1 * r2 + r1 * r3 + r2 * r3, r1 * r2 * r3
    else:
        r1 = 2 * am if recipe == "beyond" else LD(1e-9) * am
        a = (Sm - r1) / 2
        bb = am + abs(a)
        roots = (r1,)
        e2, e3 = 2 * a * r1 + a * a + bb * bb, r1 * (a * a + bb * bb)
    b1t, b2t = -4 * b4 * e3, 2 * b4 * e2
    q1, q2, nq0 = q["A_RD"][:m], q["A_DD"][:m], _ld(pv_raw)[:m]
    L1 = q["A_RD"][m] + sg * np.dot(nq0, q1) - b1t
    L2 = q["A_DD"][m] + sg * np.dot(nq0, q2) + sg * np.dot(q1, q1) / 2 - b2t
    dets = np.abs(np.outer(q1, q2) - np.outer(q2, q1)) / (np.outer(np.abs(q1), np.abs(q2)) + np.outer(np.abs(q2), np.abs(q1)) + LD(1e-300))
    i, j = np.unravel_index(int(np.argmax(dets)), dets.shape)
    keep = np.ones(m, dtype=bool)
    keep[[i, j]] = False
    u1, u2 = q1 * keep, q2 * keep
    g11, g12, g22 = np.dot(u1, u1), np.dot(u1, u2), np.dot(u2, u2)
    det = g11 * g22 - g12 * g12
    x1, x2 = (L1 * g22 - L2 * g12) / det, (L2 * g11 - L1 * g12) / det
    lam = np.asarray(x1 * u1 + x2 * u2, dtype=np.float64)
    ll = _ld(lam)
    r1_, r2_ = L1 - np.dot(ll, q1), L2 - np.dot(ll, q2)
    d2 = q1[i] * q2[j] - q1[j] * q2[i]
    lam[i], lam[j] = float((r1_ * q2[j] - r2_ * q1[j]) / d2), float((r2_ * q1[i] - r1_ * q2[i]) / d2)
    return dict(R=R, D=D, lam=lam, pv_raw=pv_raw.copy(), obj=float(pv_raw[m]), sigma=LS_SIGMA, t=t, amax=amax, recipe=recipe,
                claimed=bool(t >= 1e-2), b4x4=float(4 * b4),
                roots=roots, sum=Sm, quad_branch=bool(abs(float(4 * b4)) < np.finfo(np.float64).eps))


def apply_linesearch_state(s_, st: dict):
    s_.Rt, s_.dirt = st["R"], st["D"]
    s_.λ = st["lam"]
    s_.primal_vio_raw = st["pv_raw"]
    s_.obj, s_.σ = st["obj"], st["sigma"]


def linesearch_c(m: int) -> float:
    """c = 2·(⌈log₂ m⌉ + 12): the eight or ten sums over m constraints taken pairwise, and a dozen roundings in the
    coefficients and Horner's rule — times two."""
    return 2.0 * (int(np.ceil(np.log2(max(m, 2)))) + 12)


def commit_check(solver, pv_raw0, alpha, m: int) -> dict:
    """The commit of either line search (:118-124 / :184-188) is a kernel of its own that reads the A_RD and A_DD the call
    left: pv_raw + α(α·A_DD + A_RD) of THOSE vectors (themselves held to their references) in long double, to 4 ulp of its term
    magnitudes; V_PV is its max with the lower bounds and S_OBJ its last entry, to the same.  → commit (error/bound) and the
    exact properties obj_is_last, pv_is_raw."""
    a = LD(alpha)
    ard, add = _ld(solver.A_RD), _ld(solver.A_DD)
    want = _ld(pv_raw0) + a * (a * add + ard)
    tol = 4 * U53 * (np.abs(_ld(pv_raw0)) + a * (a * np.abs(add) + np.abs(ard)))
    pv = solver.primal_vio_raw
    lb = _ld(solver.primal_vio_lb)
    errs = np.concatenate([np.abs(_ld(pv) - want), np.abs(_ld(solver.primal_vio) - np.maximum(want[:m], lb)),
                           [abs(LD(solver.obj) - want[m])]])
    tols = np.concatenate([tol, tol[:m], [tol[m]]])
    ok = tols > 0
    assert np.all(errs[~ok] == 0)
    return dict(commit=float(np.max(errs[ok] / tols[ok])), obj_is_last=bool(solver.obj == pv[m]),
                pv_is_raw=bool(np.array_equal(solver.primal_vio, np.maximum(pv[:m], solver.primal_vio_lb))))


def check_linesearch_call(base: dict, st: dict, solver) -> dict:
    """Check 4 on one state and one handle (state applied, linesearch(α_max) run here).  → error/bound ratios
    (A_RD, A_DD, L, opt, commit) and the exact properties as booleans; nothing is asserted here."""
    C, As, bs = base["C"], base["As"], base["bs"]
    m, r = len(As), base["r"]
    apply_linesearch_state(solver, st)
    alpha, L = solver.linesearch(st["amax"])
    q = quartic_hp(C, As, bs, st["R"], st["D"], st["lam"], st["pv_raw"], st["obj"], st["sigma"])
    out = {}
    # d = 3: a term A_jk·R_jc·D_kc of ⟨A, RDᵀ + DRᵀ⟩ is two products, and the ×2 of :13 (or the sum of the two halves) a third
    depth = np.array([3 + int(np.ceil(np.log2(k + r))) + 4 for k in base["nnz"]]) * U53
    for name, got in (("A_RD", solver.A_RD), ("A_DD", solver.A_DD)):
        err = np.abs(_ld(got) - q[name])
        bound = depth * q[name + "_mag"]
        ok = bound > 0
        assert np.all(err[~ok] == 0), name
        out[name] = float(np.max(err[ok] / bound[ok])) if ok.any() else 0.0
    mn = quartic_min_hp(q["b"], st["amax"])
    cc = linesearch_c(m)
    f_at = poly_hp(q["b"], alpha)
    out["L"] = float(abs(LD(L) - f_at) / (cc * U53 * mn["T"](alpha)))
    out["opt"] = float((f_at - mn["fmin"]) / (2 * cc * U53 * mn["T"](st["amax"])))
    out["inside"] = bool(0.0 <= alpha <= st["amax"])
    out["alpha"], out["alpha_hp"] = alpha, float(mn["alpha"])
    out.update(commit_check(solver, st["pv_raw"], alpha, m))
    return out


# ---- f!, g!, 𝒜 and 𝒜ᵀ above FP64 from the matrices' own entries (tests/test_fg_reference.py, tests/test_gpu_fg_operators.py) ----
def _hp_matmul(A, B):
    """A·B of two double matrices above FP64 (np.longdouble; where that is a double, every entry through _hp_dot)."""
    A, B = np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)
    if WIDE:
        Al, Bl = A.astype(LD), B.astype(LD)
        if A.shape[0] <= 16:       # a few long rows (Bᵀ·R of a low-rank term): one vectorised pass per row
            return np.stack([np.sum(Al[i][:, None] * Bl, axis=0) for i in range(A.shape[0])]).reshape(A.shape[0], B.shape[1])
        if A.shape[1] <= 16:       # a few columns (B·(Bᵀ R)): a sum of outer products
            return sum((Al[:, k][:, None] * Bl[k][None, :] for k in range(A.shape[1])), np.zeros((A.shape[0], B.shape[1]), dtype=LD))
        return Al @ Bl
    return np.array([[_hp_dot(A[i], B[:, j]) for j in range(B.shape[1])] for i in range(A.shape[0])]).reshape(A.shape[0], B.shape[1])


def _hp_rowdots(U, V, I, J):
    """⟨U_I[k], V_J[k]⟩ for every k above FP64."""
    if WIDE:
        return np.sum(_ld(U)[I] * _ld(V)[J], axis=1)
    return np.array([_hp_dot(U[i], V[j]) for i, j in zip(I, J)], dtype=np.float64).reshape(len(I))


def _hp_segsum(w, x, owner, size):
    """out[owner[k]] += w[k]·x[k] above FP64 (w double, x in the wide type; with doubles: math.fsum of exact products)."""
    if WIDE:
        out = np.zeros(size, dtype=LD)
        np.add.at(out, owner, _ld(w) * x)
        return out
    import math
    out = np.zeros(size)
    order = np.argsort(owner, kind="stable")
    cuts = np.searchsorted(owner[order], np.arange(size + 1))
    for k in range(size):
        sel = order[cuts[k]:cuts[k + 1]]
        if sel.size:
            out[k] = math.fsum(_two_prod_terms(np.asarray(w, dtype=np.float64)[sel], np.asarray(x, dtype=np.float64)[sel]))
    return out


def split_matrices(C, As):
    """The matrices' own entries: the sparse ones concatenated as (I, J, V, owner) — owner the index into the (m + 1)-vectors,
    the cost matrix last; entries in stored order, duplicates kept — and the low-rank ones as (owner, D, B)."""
    from sdplrplus_jl_amd.structs import _entries_findnz_order
    Is, Js, Vs, Os, lows = [], [], [], [], []
    for gid, M in enumerate(list(As) + [C]):
        if isinstance(M, sj.SymLowRankMatrix):
            lows.append((gid, M.D, M.B))
            continue
        I, J, V = _entries_findnz_order(M)
        Is.append(I); Js.append(J); Vs.append(V); Os.append(np.full(len(I), gid, dtype=np.int64))
    cat = lambda xs, dt: np.concatenate(xs).astype(dt) if xs else np.zeros(0, dtype=dt)
    return (cat(Is, np.int64), cat(Js, np.int64), cat(Vs, np.float64), cat(Os, np.int64)), lows


def A_pair_hp(C, As, U, V, split=None) -> dict:
    """q[i] = ⟨Aᵢ, (UVᵀ + VUᵀ)/2⟩ for every matrix (cost last) above FP64, entry by entry (a low-rank one as Σ_c d_c⟨Bᵀ_cU,
    Bᵀ_cV⟩), never an n×n array; mag[i] the sum of the magnitudes of its elementary products, Σ|a_jk|(⟨|U_j|,|V_k|⟩ +
    ⟨|V_j|,|U_k|⟩)/2; depth[i] the roundings an FP64 evaluation makes on the way to one output in ANY summation order:
    k·r products and their sum per stored upper-triangular entry (k = 1 for U = V, else 2), the Lᵢ entries' sum, and four for
    the weights, the halving and the last store → k·r + Lᵢ + 4; a low-rank matrix k·n·s·r + r + 4."""
    U64, V64 = np.asarray(U, dtype=np.float64), np.asarray(V, dtype=np.float64)
    same = U64 is V64 or np.array_equal(U64, V64)
    k = 1 if same else 2
    n, r = U64.shape
    (I, J, W, own), lows = split or split_matrices(C, As)
    M = len(As) + 1
    aU, aV = np.abs(U64), np.abs(V64)
    if same:
        d, dm = _hp_rowdots(U64, U64, I, J), _hp_rowdots(aU, aU, I, J)
    else:
        d = (_hp_rowdots(U64, V64, I, J) + _hp_rowdots(V64, U64, I, J)) / 2
        dm = (_hp_rowdots(aU, aV, I, J) + _hp_rowdots(aV, aU, I, J)) / 2
    q, mag = _hp_segsum(W, d, own, M), _hp_segsum(np.abs(W), dm, own, M)
    depth = np.zeros(M)
    np.add.at(depth, own[I <= J], 1.0)
    depth += k * r + 4
    for gid, D, B in lows:
        WU, aWU = _hp_matmul(B.T, U64), _hp_matmul(np.abs(B).T, aU)
        WV, aWV = (WU, aWU) if same else (_hp_matmul(B.T, V64), _hp_matmul(np.abs(B).T, aV))
        q[gid] = np.sum(_ld(D)[:, None] * WU * WV) if WIDE else _hp_dot(np.repeat(D, r), (WU * WV).ravel())
        mag[gid] = np.sum(np.abs(_ld(D))[:, None] * aWU * aWV)
        depth[gid] = k * n * len(D) * r + r + 4
    return dict(q=q, mag=mag, depth=depth)


def fg_hp(C, As, bs, R, lam, lam_ub, sigma) -> dict:
    """f! of src/coreop.jl:6-31 above FP64 from the matrices' own entries: v = 𝒜(RRᵀ) − b per constraint, obj = ⟨C, RRᵀ⟩,
    ỹ = min(λ_ub, λ − σv), ℒ = obj + Σ(ỹ² − λ²)/(2σ) — with T[i] = Σ|a_jk|⟨|R_j|,|R_k|⟩ + |bᵢ| (a low-rank matrix:
    Σ_c|d_c|·‖|b_c|ᵀ|R|‖² + |bᵢ|; index m the cost matrix) and the bounds of a correct FP64 evaluation in any summation order:
      bound_v[i] = (r + Lᵢ + 4)·u·T[i]            (A_pair_hp's depth; n·s·r + r + 4 for a low-rank matrix)
      bound_L    = (m + 6)·u·(|obj| + Σ(ỹ² + λ²)/(2σ)) + bound_v[m] + Σ|ỹᵢ|·bound_v[i] + σ/2·Σ bound_v[i]²
    (ℒ depends on vᵢ through ỹᵢ²/(2σ), whose derivative is −ỹᵢ wherever the cap is not active and 0 where it is)."""
    m = len(As)
    a = A_pair_hp(C, As, R, R)
    bl = _ld(bs)
    v = a["q"].copy()
    v[:m] -= bl
    T = a["mag"].copy()
    T[:m] += np.abs(bl)
    bound_v = a["depth"] * LD(U53) * T
    lam_, ub, sg = _ld(lam), _ld(lam_ub), LD(sigma)
    yt = np.minimum(ub, lam_ - sg * v[:m])
    obj = v[m]
    L = obj + np.sum(yt * yt - lam_ * lam_) / (2 * sg)
    Lmag = abs(obj) + np.sum(yt * yt + lam_ * lam_) / (2 * sg)
    bound_L = (m + 6) * LD(U53) * Lmag + bound_v[m] + np.sum(np.abs(yt) * bound_v[:m]) + sg / 2 * np.sum(bound_v[:m] ** 2)
    return dict(v=v, obj=obj, yt=yt, L=L, T=T, depth=a["depth"], bound_v=bound_v, bound_L=bound_L)


def ytilde_from(pv_raw, lam, lam_ub, sigma) -> dict:
    """ỹ = min(λ_ub, λ − σv) above FP64 from a given double v (the device's own primal_vio_raw), the bound 3u·(|λ| + σ|v|) of
    its FP64 evaluation (one product, one difference, and a fused or unfused form of the two), and near = the entries whose
    capping decision is within that bound of a tie without being one (either branch is then a correct answer)."""
    m = len(lam)
    lam_, ub, v, sg = _ld(lam), _ld(lam_ub), _ld(pv_raw)[:m], LD(sigma)
    t = lam_ - sg * v
    bound = 3 * LD(U53) * (np.abs(lam_) + sg * np.abs(v))
    with np.errstate(invalid="ignore"):
        near = np.asarray((np.abs(t - ub) <= bound) & (t != ub))        # (t = ub exactly: both branches give ub)
    return dict(yt=np.minimum(ub, t), free=t, ub=ub, bound=bound, near=near, capped=np.asarray(t > ub))


def device_pattern(C, As, split=None) -> dict:
    """The pattern S is kept on (src/preprocess.jl:24-169), rebuilt here from the matrices' own entries: the union of the sparse
    matrices' upper-triangular entries in CSC order (V_TRIU_S_NZVAL), the union of all their entries in CSC order (V_S_NZVAL),
    each full entry's position (min, max) in the upper one, and per aggregated entry its position and owner."""
    n = C.shape[0]
    (I, J, W, own), lows = split or split_matrices(C, As)
    up = I <= J
    keyT = np.unique(J[up] * n + I[up])
    keyF = np.unique(J * n + I)
    fr, fc = keyF % n, keyF // n
    mapped = np.searchsorted(keyT, np.maximum(fr, fc) * n + np.minimum(fr, fc))
    assert keyF.size == 0 or np.array_equal(keyT[mapped], np.maximum(fr, fc) * n + np.minimum(fr, fc)), "an entry without its mirror"
    pos = np.searchsorted(keyT, J[up] * n + I[up])
    return dict(n=n, nnzT=int(keyT.size), nnzS=int(keyF.size), t_row=keyT % n, t_col=keyT // n, f_row=fr, f_col=fc,
                mapped=mapped, pos=pos, own=own[up], val=W[up], lows=lows)


def S_and_G_hp(C, As, y, R, pattern=None, with_G=True) -> dict:
    """From a given double y (the device's own; y[m] the cost matrix's coefficient) above FP64: the entries of S = Σ y_k·A_k on
    the device's pattern (upper and full; the low-rank terms are not part of it), G = 2·(S + Σ y_k·B_kD_kB_kᵀ)·R, and the scales
      S_mag[e] = Σ_k |y_k||a_k,e|,  G_mag = 2·(|S|_termwise·|R|)   (a low-rank term as |y_k|·|B||D|(|B|ᵀ|R|))
    with the bounds of a correct FP64 evaluation in any summation order:
      bound_S[e] = (c_e + 2)·u·S_mag[e]     c_e the stored entries (of all matrices, duplicates counted) that fall on e
      bound_G[j] = (d_j + c_max + s_tot + 4)·u·G_mag[j]   d_j the length of row j of S (n where a low-rank term is present: its
                   projection Bᵀ R sums n products), s_tot the low-rank columns."""
    p = pattern or device_pattern(C, As)
    n = p["n"]
    R64 = np.asarray(R, dtype=np.float64)
    r = R64.shape[1]
    y64 = np.asarray(y, dtype=np.float64)
    u = LD(U53)
    St = _hp_segsum(p["val"], _ld(y64[p["own"]]), p["pos"], p["nnzT"])
    Sm = _hp_segsum(np.abs(p["val"]), np.abs(_ld(y64[p["own"]])), p["pos"], p["nnzT"])
    ce = np.bincount(p["pos"], minlength=p["nnzT"]).astype(np.float64)
    out = dict(pattern=p, triu=St, triu_mag=Sm, c=ce, bound_triu=(ce + 2) * u * Sm,
               full=St[p["mapped"]], full_mag=Sm[p["mapped"]], bound_full=((ce + 2) * u * Sm)[p["mapped"]])
    if not with_G:
        return out
    ty = LD if WIDE else np.float64
    G, Gm = np.zeros((n, r), dtype=ty), np.zeros((n, r), dtype=ty)
    if p["nnzS"]:
        # column j of the full pattern: G_j += S_e·R_row (𝒜t!(y, x, aux, var), src/coreop.jl:260-279); the entries are sorted by
        # column, so every row of G is one contiguous segment (no running sum across rows of very different size)
        starts = np.flatnonzero(np.diff(np.concatenate([[-1], p["f_col"]])))
        cols = p["f_col"][starts]
        if WIDE:
            G[cols] = np.add.reduceat(out["full"][:, None] * _ld(R64)[p["f_row"]], starts, axis=0)
            Gm[cols] = np.add.reduceat(out["full_mag"][:, None] * np.abs(_ld(R64))[p["f_row"]], starts, axis=0)
        else:
            S64 = sp.csc_matrix((np.asarray(out["full"], dtype=np.float64), (p["f_col"], p["f_row"])), shape=(n, n)).toarray()
            Sm64 = sp.csc_matrix((np.asarray(out["full_mag"], dtype=np.float64), (p["f_col"], p["f_row"])), shape=(n, n)).toarray()
            G, Gm = _hp_matmul(S64, R64), _hp_matmul(Sm64, np.abs(R64))
    s_tot = 0
    for gid, D, B in p["lows"]:
        s_tot += len(D)
        W, Wm = _hp_matmul(B.T, R64), _hp_matmul(np.abs(B).T, np.abs(R64))
        for c in range(len(D)):        # (one outer product per column, in the wide type)
            G = G + (ty(y64[gid]) * ty(D[c]) * B[:, c].astype(ty))[:, None] * W[c][None, :].astype(ty)
            Gm = Gm + (abs(ty(y64[gid]) * ty(D[c])) * np.abs(B[:, c]).astype(ty))[:, None] * Wm[c][None, :].astype(ty)
    d = np.full(n, float(n)) if p["lows"] else np.bincount(p["f_col"], minlength=n).astype(np.float64)
    cmax = float(ce.max()) if ce.size else 0.0
    out.update(G=2 * G, G_mag=2 * Gm, d=d, bound_G=((d + cmax + s_tot + 4) * u)[:, None] * (2 * Gm))
    return out


def worst_ratio(got, want, bound) -> float:
    """max |got − want|/bound over EVERY element; an element whose bound is 0 must be exact (else inf)."""
    err = np.abs(_ld(got) - np.asarray(want, dtype=LD))
    bound = np.asarray(bound, dtype=LD)
    if err.size == 0:
        return 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1), np.where(err == 0, 0.0, np.inf))
    ratio = np.where(np.isnan(ratio), np.inf, ratio)
    return float(np.max(ratio))


# ---- the loop routes, shared by tests/test_gpu_direction_linesearch.py and tests/test_gpu_armijo.py --------------------------
LOOP_TOGGLES = ["SDPLR_HIP_NO_RING", "SDPLR_HIP_NO_UPDFUSE", "SDPLR_HIP_DOT_DESCENT", "SDPLR_HIP_NO_FAST", "SDPLR_HIP_NO_FAST2",
                "SDPLR_HIP_NO_GRAPH", "SDPLR_HIP_TEAM", "SDPLR_HIP_NO_RESIDENT", "SDPLR_HIP_GRAPH_ITERS", "SDPLR_HIP_NO_LRFUSE",
                "SDPLR_HIP_NO_GROUP_LAUNCH"]
# route → (environment, SDPLR_HIP_FORCE_GRAPH kept: the suite's default, which keeps the resident loop out)
LOOP_ROUTES = {
    "graph": ({"SDPLR_HIP_GRAPH_ITERS": "2"}, True),           # (batches shorter than k: several replays)
    "eager": ({"SDPLR_HIP_NO_GRAPH": "1"}, True),
    "stored": ({"SDPLR_HIP_NO_RING": "1"}, True),
    "no_updfuse": ({"SDPLR_HIP_NO_UPDFUSE": "1"}, True),
    "dot_descent": ({"SDPLR_HIP_DOT_DESCENT": "1"}, True),
    "no_fast": ({"SDPLR_HIP_NO_FAST": "1"}, True),
    "no_fast2": ({"SDPLR_HIP_NO_FAST2": "1"}, True),
    "no_lrfuse": ({"SDPLR_HIP_NO_LRFUSE": "1"}, True),
    "resident_team1": ({"SDPLR_HIP_TEAM": "1"}, False),
    "resident_team3": ({"SDPLR_HIP_TEAM": "3"}, False),
    "resident_batch": ({}, False),                             # three instances in one sdplr_hip_batch_major_iteration
    "group": ({}, True),                                       # the same call on the edge path: the group launch
}
RESIDENT_FAMILIES = ("maxcut", "maxcut300", "minimum_bisection", "cutnorm")   # (the edge path and low-rank terms stay on launches)


def set_route(monkeypatch, route):
    env, force_graph = LOOP_ROUTES[route]
    for k in LOOP_TOGGLES:
        monkeypatch.delenv(k, raising=False)
    if force_graph:
        monkeypatch.setenv("SDPLR_HIP_FORCE_GRAPH", "1")
    else:
        monkeypatch.delenv("SDPLR_HIP_FORCE_GRAPH", raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def assert_route(route, family, r, h, st, armijo=False):
    """Which route ran, from stats(): the resident loop (one workgroup, h ≤ 4: above that the library itself goes back to
    launches), its shared batch launch, the group launch (h ≤ 4), graph replays or eager batches, the ring form (taken at
    n = 300, r = 8 and at n = 12, r = 32, under graph and eager, h ≤ 4 — not at n = 12, r = 3) and the P-less step kernel, which the fused-update, dot-descent and
    NO_FAST/NO_FAST2 toggles — having no counter of their own — switch off together with the ring.
    armijo: a loop with inequality data.  The resident loop, the group launch, the ring form and the P-less step kernel all
    refuse it, whatever the route asks for: every iteration is a graph replay or an eager batch of launches."""
    tag = (route, family, r, h, st)
    if armijo:
        assert st["resident_loops"] == 0 and st["resident_shared_launches"] == 0 and st["group_launch_loops"] == 0, tag
        assert st["ring_history_loops"] == 0 and st["p_less_loops"] == 0 and st["inner_iterations"] >= 1, tag
        if route == "graph":
            assert st["graph_batches"] >= 1, tag
        if route == "eager":
            assert st["graph_batches"] == 0 and st["eager_batches"] >= 1, tag
        return
    resident = route.startswith("resident") and family in RESIDENT_FAMILIES and h <= 4
    if resident:
        assert st["resident_loops"] >= 1 and st["graph_batches"] == 0 and st["eager_batches"] == 0, tag
        assert (st["resident_shared_launches"] >= 1) == (route == "resident_batch"), tag
        return
    assert st["resident_loops"] == 0 and st["resident_shared_launches"] == 0, tag
    if route == "group" and h <= 4:        # (h = 5: the library runs the batch's items one by one)
        assert st["group_launch_loops"] >= 1 and family == "lovasz_theta", tag
        return
    assert st["group_launch_loops"] == 0, tag
    if route == "graph":
        assert st["graph_batches"] >= 2, tag
    if route == "eager":
        assert st["graph_batches"] == 0 and st["eager_batches"] >= 1, tag
    ring = (family == "maxcut300" or (family == "maxcut" and r == 32)) and route in ("graph", "eager", "no_lrfuse") and h <= 4
    if not (family == "maxcut" and r == 32 and h > 4):        # (not measured: left open rather than guessed)
        assert (st["ring_history_loops"] >= 1) == ring, tag
    if route in ("no_updfuse", "dot_descent", "no_fast", "no_fast2"):
        assert st["p_less_loops"] == 0, tag
    elif family in ("maxcut", "maxcut300") and r != 32 and h <= 4 and not route.startswith("resident"):
        assert st["p_less_loops"] >= 1, tag


# ---- Armijo backtracking above FP64 (tests/test_armijo_reference.py, tests/test_gpu_armijo.py) -------------------------------
ARMIJO_K = 50            # halvings at the most (src/linesearch.jl:177)


def _adot(a, b):
    """⟨a, b⟩ above FP64: of long doubles where numpy has them, else of the doubles' exact products (_hp_dot)."""
    return np.dot(a, b) if WIDE else _hp_dot(a, b)


def armijo_hp(pv_raw, obj, lam, lam_ub, y, sigma, alpha_max, A_RD, A_DD) -> dict:
    """src/linesearch.jl:139-191 above FP64, from the A_RD and A_DD a call left (both of length m + 1, the objective's entry
    last; A_RD with its ×2).  For k = 0 … 50, α_k = α_max/2^k (exact halvings):
      L[k]      = obj + α_k·p1 + α_k²·p2 + Σ_i (λ̃_i(α_k)² − λ_i²)/(2σ),  λ̃_i(α) = min(λ_ub_i, λ_i − σ·g_i(α)),
                  g_i(α) = pv_raw_i + α·A_RD_i + α²·A_DD_i                                               (eval_AL, :157-165)
      L0, slope = ℒ(0) and p1 + ⟨y[:m], A_RD[:m]⟩                                                         (:167, :171)
      margin[k] = L0 + 1e-4·α_k·slope − L[k]: the step is accepted at the first k with margin ≥ 0          (:173-181)
      T[k]      = |obj| + α_k|p1| + α_k²|p2| + Σ_i [(λ̃_i² + λ_i²)/(2σ) + |λ̃_i|·(|λ_i|/σ + |g0_i| + α_k|q1_i| + α_k²|q2_i|)]
                  — the sum's own terms, and to first order what rounding g_i and λ − σ·g_i does inside the square; the latter
                  is zero on a row where the cap wins (there λ̃ = λ_ub exactly).  T0 the same at α = 0.
      T_slope   = |p1| + Σ|y_i·q1_i|
      tau[k]    = c·u·(T0 + T[k] + 1e-4·α_k·T_slope),  c = linesearch_c(m): what an FP64 evaluation of margin[k] may be off by
      k_hp      = the first k with margin ≥ 0, or 50
      decided   = |margin[k]| > 10·tau[k] for every k ≤ k_hp (k < 50: after the 50th halving nothing is tested any more)
      capped[k] = the rows on which the cap wins at α_k.
    Without a wider long double the sums are math.fsum over exact products of doubles (the rows' own values are then formed
    in double)."""
    m = len(lam)
    g0, q1, q2 = _ld(pv_raw)[:m], _ld(A_RD)[:m], _ld(A_DD)[:m]
    p1, p2 = LD(np.float64(A_RD[m])), LD(np.float64(A_DD[m]))
    lam_, ub, sg, ob = _ld(lam), _ld(lam_ub), LD(np.float64(sigma)), LD(np.float64(obj))
    l2 = _adot(lam_, lam_)
    ag0, aq1, aq2, al = np.abs(g0), np.abs(q1), np.abs(q2), np.abs(lam_) / sg
    one = np.ones(m, dtype=LD)

    def at(a):
        free = lam_ - sg * (g0 + a * q1 + a * a * q2)
        cap = np.asarray(free > ub)
        lt = np.where(cap, ub, free)
        t2 = _adot(lt, lt)
        sens = np.where(cap, 0, np.abs(lt) * (al + ag0 + a * aq1 + a * a * aq2))
        L = ob + a * p1 + a * a * p2 + (t2 - l2) / (2 * sg)
        T = abs(ob) + a * abs(p1) + a * a * abs(p2) + (t2 + l2) / (2 * sg) + _adot(sens, one)
        return L, T, cap

    alphas = np.array([LD(np.float64(alpha_max)) * LD(2.0) ** -k for k in range(ARMIJO_K + 1)], dtype=LD)
    L0, T0, cap0 = at(LD(0))
    yl = _ld(y)[:m]
    slope, T_slope = p1 + _adot(yl, q1), abs(p1) + _adot(np.abs(yl), aq1)
    vals = [at(a) for a in alphas]
    L, T = np.array([v[0] for v in vals], dtype=LD), np.array([v[1] for v in vals], dtype=LD)
    c = linesearch_c(m)
    c1 = LD(np.float64(1e-4))
    margin = L0 + c1 * alphas * slope - L
    tau = c * LD(U53) * (T0 + T + c1 * alphas * T_slope)
    acc = np.flatnonzero(margin[:ARMIJO_K] >= 0)
    k_hp = int(acc[0]) if acc.size else ARMIJO_K
    upto = min(k_hp, ARMIJO_K - 1)
    return dict(alpha=np.asarray(alphas, dtype=np.float64), L=L, T=T, L0=L0, T0=T0, slope=slope, T_slope=T_slope, margin=margin,
                tau=tau, k_hp=k_hp, c=c, decided=bool(np.all(np.abs(margin[:upto + 1]) > 10 * tau[:upto + 1])),
                capped=np.stack([v[2] for v in vals]), capped0=cap0)


def armijo_k_of(alpha: float, alpha_max: float):
    """k with alpha == α_max/2^k bit for bit, or None."""
    for k in range(ARMIJO_K + 1):
        if alpha == float(alpha_max) * 2.0 ** -k:
            return k
    return None


def armijo_decision_ok(ref: dict, k_dev: int) -> bool:
    """A device answer k_dev is right iff every k < k_dev has margin < τ (legitimately rejected) and k_dev = 50 or
    margin[k_dev] ≥ −τ (legitimately accepted)."""
    g, tau = ref["margin"], ref["tau"]
    return bool(np.all(g[:k_dev] < tau[:k_dev]) and (k_dev == ARMIJO_K or g[k_dev] >= -tau[k_dev]))


_ARM_CACHE = {}


def armijo_base(n: int, m: int, r: int, seed: int = 0) -> dict:
    """A problem of the Armijo tests with any row count m ≤ n(n+1)/2 + 1: the cost is a graph Laplacian on n vertices, row 0 an
    equality with a full (unit) diagonal, rows 1 … m − 1 inequalities that are single symmetric entries (i, j), i ≤ j, drawn
    without repetition, with seeded values and right-hand sides.  With it: a seeded Gaussian R (n×r) and λ, σ = 2, pv_raw and
    obj the true ones at R above FP64, λ_ub by the recipe of fg_cases.case_inputs (+∞ on the equality row; the inequality rows
    cycle through 0 and ½ and 1½ times λ − σv; λ moved strictly below λ_ub where it was above), y as g! leaves it, and G = 2·S(y)·R
    above FP64 — the gradient of the capped ℒ, which hp_gradient's equality form is not.  Built once and left unchanged.  The
    SDPData is handed over as one batch (no pass over m Python objects in its constructor)."""
    key = (n, m, r, seed)
    if key in _ARM_CACHE:
        return _ARM_CACHE[key]
    from sdplrplus_jl_amd.structs import SparseBatch
    assert 1 <= m <= n * (n + 1) // 2 + 1
    rng = np.random.Generator(np.random.PCG64(8800 + 131 * seed + m))
    A = problems.gnp_graph(n, min(0.5, 6.0 / n), 500 + n + seed)
    C = sp.csc_matrix(sp.diags(np.asarray(A.sum(axis=1)).ravel()) - A)
    ju, iu = np.triu_indices(n)          # (row ≥ col of the transpose: every pair i ≤ j once)
    pick = rng.choice(iu.size, size=m - 1, replace=False)
    pi, pj = np.minimum(iu[pick], ju[pick]), np.maximum(iu[pick], ju[pick])
    vals = rng.standard_normal(m - 1) * 2.0 ** rng.integers(-3, 4, size=m - 1)
    As = [sj.SparseMatrixCOO(np.arange(n), np.arange(n), np.ones(n), n, n)]
    for i, j, v in zip(pi.tolist(), pj.tolist(), vals.tolist()):
        As.append(sj.SparseMatrixCOO([i], [i], [v], n, n) if i == j else sj.SparseMatrixCOO([i, j], [j, i], [v, v], n, n))
    bs = rng.standard_normal(m)
    ct = np.arange(m) > 0
    split = split_matrices(C, As)
    (I, J, V, own), _ = split
    ptr = np.concatenate([[0], np.cumsum(np.bincount(own, minlength=m + 1))]).astype(np.int64)
    data = sj.SDPData.from_batch(C, bs, SparseBatch(n, ptr, I, J, V, np.arange(m + 1, dtype=np.int64)), [], ct)
    pattern = device_pattern(C, As, split)
    R = rng.standard_normal((n, r))
    lam = rng.standard_normal(m)
    sigma = LS_SIGMA
    a = A_pair_hp(C, As, R, R, split)
    pv = a["q"].copy()
    pv[:m] -= _ld(bs)
    pv_raw = np.asarray(pv, dtype=np.float64)
    free = np.asarray(_ld(lam) - LD(sigma) * _ld(pv_raw)[:m], dtype=np.float64)
    ub = np.full(m, np.inf)
    q = np.flatnonzero(ct)
    ub[q] = 0.0
    ub[q[1::4]] = 0.5 * free[q[1::4]]
    ub[q[3::4]] = 1.5 * free[q[3::4]]
    with np.errstate(invalid="ignore"):
        lam = np.where(lam > ub, ub - np.abs(ub) - 0.01, lam)
    y = np.concatenate([-np.asarray(ytilde_from(pv_raw, lam, ub, sigma)["yt"], dtype=np.float64), [1.0]])
    G = np.asarray(S_and_G_hp(C, As, y, R, pattern)["G"], dtype=np.float64)
    out = dict(n=n, m=m, r=r, seed=seed, C=C, As=As, bs=bs, ct=ct, data=data, split=split, pattern=pattern, R=R, lam=lam, ub=ub,
               sigma=sigma, pv_raw=pv_raw, obj=float(pv_raw[m]), G=G)
    _ARM_CACHE[key] = out
    return out


def armijo_state(base: dict, t: float, amax: float, kind: str = "descent") -> dict:
    """One state on armijo_base: D = fl(t·(−G)) (kind "descent"), fl(t·G) ("ascent": every trial step is rejected until the
    margin drops below its own round-off — the exhaustion state) or 0 ("tie": ℒ(α) = ℒ(0) and the slope 0 for every α, accepted
    at once by `≤`).  A block of inequality rows — the last min(16, ⌈#inequalities/4⌉) of them — gets
    λ_ub_i = fl(λ_i − σ·g_i(α*)), α* = ¾·α_max/2^j with j cycling through k₀ − 1 … k₀ − 4 (not below 0), k₀ the step the search
    accepts without this block: those rows sit ON the cap at a point strictly between the trial steps α_j and α_{j+1}, so they
    change sides while the search backtracks past it (asserted above FP64 in tests/test_armijo_reference.py; an α* far above
    the accepted step would put g_i(α*)² — growing as t⁴ — into ℒ(0) as a constant and drown every margin in its round-off).  y is then what g! leaves for that λ_ub.  Also the references of 𝒜(RDᵀ + DRᵀ) and 𝒜(DDᵀ)
    above FP64 with their termwise magnitudes and depths (A_pair_hp)."""
    C, As, R, G, m = base["C"], base["As"], base["R"], base["G"], base["m"]
    D = {"descent": -t * G, "ascent": t * G, "tie": np.zeros_like(G)}[kind]
    a1, a2 = A_pair_hp(C, As, R, D, base["split"]), A_pair_hp(C, As, D, D, base["split"])
    lam, ub, sg = base["lam"], base["ub"].copy(), LD(base["sigma"])
    ineq = np.flatnonzero(base["ct"])
    cross = ineq[len(ineq) - min(16, -(-len(ineq) // 4)):] if len(ineq) and kind != "tie" else ineq[:0]
    if cross.size:
        ard, add = np.asarray(2 * a1["q"], dtype=np.float64), np.asarray(a2["q"], dtype=np.float64)
        y0 = np.concatenate([-np.asarray(ytilde_from(base["pv_raw"], lam, ub, base["sigma"])["yt"], dtype=np.float64), [1.0]])
        k0 = armijo_hp(base["pv_raw"], base["obj"], lam, ub, y0, base["sigma"], amax, ard, add)["k_hp"]
        j = np.maximum(0, k0 - 1 - np.arange(cross.size) % 4)
        astar = LD(np.float64(amax)) * LD(0.75) * LD(2.0) ** -j.astype(LD)
        gi = _ld(base["pv_raw"])[cross] + astar * (2 * a1["q"][cross]) + astar * astar * a2["q"][cross]
        ub[cross] = np.asarray(_ld(lam)[cross] - sg * gi, dtype=np.float64)
    y = np.concatenate([-np.asarray(ytilde_from(base["pv_raw"], lam, ub, base["sigma"])["yt"], dtype=np.float64), [1.0]])
    return dict(R=R, D=np.asarray(D, dtype=np.float64), lam=lam, ub=ub, y=y, pv_raw=base["pv_raw"].copy(), obj=base["obj"],
                sigma=base["sigma"], t=t, amax=amax, kind=kind, cross=cross, a1=a1, a2=a2)


def armijo_state_ref(st: dict) -> dict:
    """armijo_hp on the state's own 𝒜 vectors above FP64 rounded to double: what the generator's claims are stated on."""
    ard, add = np.asarray(2 * st["a1"]["q"], dtype=np.float64), np.asarray(st["a2"]["q"], dtype=np.float64)
    return armijo_hp(st["pv_raw"], st["obj"], st["lam"], st["ub"], st["y"], st["sigma"], st["amax"], ard, add)


def crossings(ref: dict, rows) -> int:
    """Rows among `rows` that change sides of the cap between two consecutive trial steps k, k + 1 ≤ k_hp."""
    cap = ref["capped"][:ref["k_hp"] + 1][:, rows]
    return int(np.sum(np.any(cap[1:] != cap[:-1], axis=0))) if cap.shape[0] > 1 else 0


def apply_armijo_state(s_, st: dict):
    apply_linesearch_state(s_, st)
    s_.λ_ub = st["ub"]
    s_.y = st["y"]


def check_armijo_call(base: dict, st: dict, solver) -> dict:
    """One state on one handle (applied and linesearch_armijo(α_max) run here).  → error/bound ratios A_RD, A_DD (termwise against
    A_pair_hp), L (ℒ against L[k_dev] of armijo_hp on the handle's own A_RD, A_DD, bound c·u·T[k_dev]), commit (commit_check), and
    the exact properties: on_grid (α = α_max/2^k_dev bit for bit for some k_dev ≤ 50), decision_ok (armijo_decision_ok),
    alpha_exact (a decided state: k_dev = k_hp), obj_is_last, pv_is_raw; with k_dev, k_hp, decided.  Nothing is asserted here."""
    m = base["m"]
    apply_armijo_state(solver, st)
    alpha, L = solver.linesearch_armijo(st["amax"])
    ard, add = solver.A_RD, solver.A_DD
    a1, a2 = st["a1"], st["a2"]
    out = dict(A_RD=worst_ratio(ard, 2 * a1["q"], a1["depth"] * LD(U53) * 2 * a1["mag"]),
               A_DD=worst_ratio(add, a2["q"], a2["depth"] * LD(U53) * a2["mag"]))
    ref = armijo_hp(st["pv_raw"], st["obj"], st["lam"], st["ub"], st["y"], st["sigma"], st["amax"], ard, add)
    k = armijo_k_of(alpha, st["amax"])
    out.update(alpha=alpha, k_dev=k, k_hp=ref["k_hp"], decided=ref["decided"], on_grid=k is not None, ref=ref)
    if k is None:
        out.update(L=np.inf, decision_ok=False, alpha_exact=False)
    else:
        out["L"] = worst_ratio([L], [ref["L"][k]], [ref["c"] * LD(U53) * ref["T"][k]])
        out["decision_ok"] = armijo_decision_ok(ref, k)
        out["alpha_exact"] = bool(k == ref["k_hp"]) if ref["decided"] else True
    out.update(commit_check(solver, st["pv_raw"], alpha, m))
    return out
