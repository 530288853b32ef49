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
