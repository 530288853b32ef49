"""The cases and the checks shared by tests/test_fg_reference.py (the CPU oracle) and tests/test_gpu_fg_operators.py (the HIP
library): f!, g!, fg!, 𝒜 and both 𝒜ᵀ against helpers.fg_hp / S_and_G_hp / A_pair_hp, every element held to error/bound ≤ 1.

A case is (matrices, constraint types, ranks, environment, expected form).  Its inputs are four seeded R (plain, graded,
near-feasible, zero rows) times λ ∈ {0, graded} times σ ∈ {2, 1e3}; a `lean` case (large, or one of a long list of ranks) takes
the four R with the four (λ, σ) pairs dealt round-robin instead of the full product."""
import numpy as np
import scipy.sparse as sp

import sdplrplus_jl_amd as sj
from sdplrplus_jl_amd import cabi, problems
from helpers import (LD, U53, A_pair_hp, S_and_G_hp, _ld, device_pattern, fg_hp, make_data, worst_ratio, ytilde_from)

QUANTITIES = ("v", "L", "y", "S", "G", "gnorm", "pnorm", "A1", "A2", "At_S", "At_left", "At_right")
TOGGLES = ("SDPLR_HIP_NO_FAST", "SDPLR_HIP_NO_FAST_FG", "SDPLR_HIP_TILE_K", "SDPLR_HIP_NO_TILE_UNIFORM", "SDPLR_HIP_HUB_THRESH",
           "SDPLR_HIP_NO_RESIDENT_ROWVEC", "SDPLR_HIP_NO_RESIDENT", "SDPLR_HIP_NO_TILE", "SDPLR_HIP_NO_EDGE", "SDPLR_HIP_TEAM")


def _coo_sym(n, pairs, vals):
    I, J, V = [], [], []
    for (i, j), v in zip(pairs, vals):
        I.append(i); J.append(j); V.append(v)
        if i != j:
            I.append(j); J.append(i); V.append(v)
    return sj.SparseMatrixCOO(I, J, V, n, n)


def _sym_sparse(n, density, rng, diag=True):
    M = sp.random(n, n, density=density, random_state=np.random.RandomState(int(rng.integers(1 << 30))), format="csr")
    M = sp.triu(M, k=1)
    M = M + M.T
    if diag:
        M = M + sp.diags(rng.standard_normal(n))
    return sp.csc_matrix(M)


def segmented_problem():
    """n = 96: constraints with exactly 1, 16, 17, 2048, 2049 and 4097 upper-triangular entries (SHORT_MAX = 16: the last short
    and the first long segment; CHUNK = 2048: one chunk, two chunks with a one-entry tail, three chunks), 260 single-entry
    constraints (a second block of 256 short segments) and a sparse cost: two general matrices, so the generic kernels."""
    n = 96
    rng = np.random.Generator(np.random.PCG64(9601))
    iu = np.array([(i, j) for j in range(n) for i in range(j + 1)])
    As = []
    for L in (1, 16, 17, 2048, 2049, 4097):
        sel = iu[rng.choice(len(iu), size=L, replace=False)]
        # (the two multi-chunk constraints are 2⁻⁴⁸ of the others: a whole chunk partial of theirs is then below 1e-12 of the
        # largest output and far above their own bound — what tests/test_fg_reference.py drops)
        scale = 2.0 ** -48 if L > 2048 else 1.0
        As.append(_coo_sym(n, [tuple(p) for p in sel], scale * rng.standard_normal(L) * 2.0 ** rng.integers(-6, 7, size=L)))
    for k in range(260):
        i, j = sorted(int(x) for x in rng.integers(0, n, size=2))
        As.append(_coo_sym(n, [(i, j)], [float(rng.standard_normal()) * 2.0 ** int(rng.integers(-6, 7))]))
    C = _sym_sparse(n, 0.1, rng)
    counts = [int(np.sum(A.is_ <= A.js)) for A in As]
    assert counts[:6] == [1, 16, 17, 2048, 2049, 4097] and sum(c <= 16 for c in counts) >= 257
    return C, As, rng.standard_normal(len(As)), None


def _graph_isolated(n, p, seed, iso):
    A = sp.lil_matrix(problems.gnp_graph(n, p, seed))
    for j in iso:
        A[j, :] = 0
        A[:, j] = 0
    A = sp.csc_matrix(A)
    A.eliminate_zeros()
    return A


def _star_plus_gnp(n, p, seed):
    """G(n, p) plus a star at vertex 5: one row of the pattern longer than max(64, 3·mean) — the layout's own hub test."""
    A = sp.lil_matrix(problems.gnp_graph(n, p, seed))
    A[5, :] = 1.0
    A[:, 5] = 1.0
    A[5, 5] = 0.0
    A = sp.csc_matrix(A)
    deg = np.diff(A.indptr) + 1                      # (the diagonal is part of every row of S)
    assert deg[5] > max(64, 3 * deg.sum() / n) and np.sum(deg > max(64, 3 * deg.sum() / n)) == 1
    return A


def _lowrank_problem(n, cols, seed, sparse_rows=True):
    """Low-rank terms of `cols` columns each next to unit diagonal constraints and a sparse cost."""
    rng = np.random.Generator(np.random.PCG64(seed))
    lr = lambda s: sj.SymLowRankMatrix(rng.standard_normal(s), rng.standard_normal((n, s)))
    As = [lr(s) for s in cols]
    if sparse_rows:
        As += [_coo_sym(n, [(i, i)], [1.0 + 0.01 * i]) for i in range(n)]
        C = _sym_sparse(n, 0.1, rng)
    else:
        C = lr(1)
    return C, As, rng.standard_normal(len(As)), None


def _random_kind(kind, n, seed):
    from test_gpu_parity import _random_problem
    C, As, bs = _random_problem(kind, n, np.random.Generator(np.random.PCG64(seed)))
    return C, As, bs, None


def _family(family, n, p=0.3, seed=5):
    def build():
        data, C, As, bs = make_data(family, seed, n, p)
        return C, As, bs, (data.constraint_types if data.has_inequalities else None)
    return build


def _of_graph(builder, graph):
    def build():
        C, As, bs = builder(graph())
        return C, As, bs, None
    return build


_RANKS = (1, 2, 3, 5, 8, 16, 27, 32, 33, 64, 100, 128, 129, 200)
NF = {"SDPLR_HIP_NO_FAST": "1"}
# name → dict(build, ranks, env, form ∈ {"fast", "generic", "resident"}, scopes the launch form must show, lean, big,
#             launches: the suite's SDPLR_HIP_FORCE_GRAPH kept (False: removed, the resident route is open))
CASES = {}


def _case(name, build, ranks, form, env=None, scopes=(), lean=False, big=False, hubs=None):
    CASES[name] = dict(name=name, build=build, ranks=tuple(ranks), form=form, env=dict(env or {}), scopes=tuple(scopes), lean=lean,
                       big=big, launches=form != "resident", hubs=hubs)


_GEN = ("sddmm_uu", "segreduce", "spmm")
_case("segmented", segmented_problem, (3, 32), "generic", scopes=_GEN + ("seg_finalize",))
_case("ranks_fast", _of_graph(problems.maxcut, lambda: problems.gnp_graph(70, 0.3, 70)), _RANKS, "fast", lean=True)
_case("ranks_generic", _of_graph(problems.maxcut, lambda: problems.gnp_graph(70, 0.3, 70)), _RANKS, "generic", env=NF, scopes=_GEN, lean=True)
for _tk in (None, 3, 8, 16):
    _env = {} if _tk is None else {"SDPLR_HIP_TILE_K": str(_tk)}
    _case(f"fast_maxcut300_k{_tk}", _of_graph(problems.maxcut, lambda: problems.gnp_graph(300, 0.05, 7)), (8,), "fast", env=_env)
    _case(f"fast_cutnorm300_k{_tk}", _of_graph(problems.cutnorm, lambda: problems.gnp_graph(150, 0.08, 9)), (8,), "fast", env=_env, lean=True)
_case("fast_isolated", _of_graph(problems.maxcut, lambda: _graph_isolated(300, 0.05, 7, (0, 17, 150, 299))), (8,), "fast")
_case("fast_no_tile_uniform", _of_graph(problems.maxcut, lambda: problems.gnp_graph(300, 0.05, 7)), (8,), "fast",
      env={"SDPLR_HIP_NO_TILE_UNIFORM": "1"})
_case("fast_fg_off", _of_graph(problems.maxcut, lambda: problems.gnp_graph(300, 0.05, 7)), (8,), "generic",
      env={"SDPLR_HIP_NO_FAST_FG": "1"}, scopes=_GEN)
_case("hub_star_lovasz", _of_graph(problems.lovasz_theta, lambda: _star_plus_gnp(400, 0.02, 3)), (6,), "generic", scopes=_GEN, hubs=(1, None), lean=True)
_case("hub_star_maxcut", _of_graph(problems.maxcut, lambda: _star_plus_gnp(400, 0.02, 3)), (6,), "generic", env=NF, scopes=_GEN, hubs=(1, None), lean=True)
_case("hub_many_lovasz", _of_graph(problems.lovasz_theta, lambda: problems.gnp_graph(600, 0.03, 4)), (6,), "generic",
      env={"SDPLR_HIP_HUB_THRESH": "8"}, scopes=_GEN, hubs=(257, 8), lean=True)
_case("hub_many_maxcut", _of_graph(problems.maxcut, lambda: problems.gnp_graph(600, 0.03, 4)), (6,), "generic",
      env={"SDPLR_HIP_HUB_THRESH": "8", **NF}, scopes=_GEN, hubs=(257, 8), lean=True)
_case("lowrank_st1", lambda: _lowrank_problem(64, (1,), 31), (4,), "generic", scopes=("lr_project", "lr_finalize"))
_case("lowrank_st8", lambda: _lowrank_problem(64, (3, 5), 32), (4,), "generic", scopes=("lr_project", "lr_finalize"))
_case("lowrank_st9", lambda: _lowrank_problem(64, (3, 6), 33), (4,), "generic", scopes=("lr_project", "lr_finalize"))
_case("lowrank_minbis60", _family("minimum_bisection", 60, 0.2), (4,), "generic", scopes=("lr_project",))
_case("lowrank_all", lambda: _random_kind("all_lowrank", 64, 77), (5,), "generic", scopes=("lr_project",))
_case("lowrank_cost_multi", lambda: _random_kind("lowrank_cost_multi_column", 64, 78), (5,), "generic", scopes=("lr_project",))
_case("lowrank_big", lambda: _lowrank_problem(32768, (1,), 34, sparse_rows=False), (128,), "generic",
      scopes=("lr_project", "lr_reduce"), lean=True, big=True)
_case("ineq_0.05", _family("ineq_0.05", 40), (4,), "generic")
_case("mu_conductance_0.05_n40", _family("mu_conductance_0.05", 40), (4,), "generic")
for _n in (12, 513, 1024, 1025):
    _case(f"resident_maxcut{_n}", _of_graph(problems.maxcut, lambda _n=_n: problems.gnp_graph(_n, min(0.5, 6.0 / _n), 40 + _n)), (3, 10),
          "resident", lean=_n > 12)
_case("resident_cutnorm", _of_graph(problems.cutnorm, lambda: problems.gnp_graph(60, 0.1, 9)), (3,), "resident")
_case("resident_minbis", _family("minimum_bisection", 60, 0.2), (3,), "resident")
_case("resident_rows_global", _of_graph(problems.maxcut, lambda: problems.gnp_graph(1025, 6.0 / 1025, 1065)), (16,), "resident", lean=True)
_case("resident_rowvec_off", _of_graph(problems.maxcut, lambda: problems.gnp_graph(1025, 6.0 / 1025, 1065)), (16,), "launch",
      env={"SDPLR_HIP_NO_RESIDENT_ROWVEC": "1"}, lean=True)
CASES["resident_rowvec_off"]["launches"] = False
ALL_FAMILIES = ("maxcut", "lovasz_theta", "minimum_bisection", "cutnorm", "mu_conductance_0.01", "mu_conductance_0.05",
                "mu_conductance_0.1", "ineq_0.01", "ineq_0.05", "ineq_0.1")
_FAMILY_FORM = {"maxcut": "fast", "cutnorm": "fast"}
for _f in ALL_FAMILIES:
    _case(f"family_{_f}", _family(_f, 40), (4,), _FAMILY_FORM.get(_f, "generic"), lean=True)
    if _f in ("maxcut", "cutnorm", "minimum_bisection"):
        _case(f"family_{_f}_resident", _family(_f, 40), (4,), "resident", lean=True)

_BUILT = {}


def built(name):
    """The case's matrices, pattern and inputs, built once and left unchanged."""
    if name not in _BUILT:
        C, As, bs, ct = CASES[name]["build"]()
        bs = np.asarray(bs, dtype=np.float64)
        ct = np.zeros(len(As), dtype=bool) if ct is None else np.asarray(ct, dtype=bool)
        _BUILT[name] = dict(C=C, As=As, bs=bs, ct=ct, data=sj.SDPData(C, As, bs, ct if ct.any() else None),
                            pattern=device_pattern(C, As), inputs={})
    return _BUILT[name]


def four_R(bc, r, seed):
    """plain U(−1, 1); graded: row j times 2^k_j, k_j uniform in −20 … 20 (row 0: −20, the last row: 20); near-feasible: every row that a single-diagonal-entry
    constraint a·X_jj = b (b/a > 0) is attached to scaled to ‖R_j‖² = b/a, so that v cancels to round-off (no such constraint:
    R scaled as a whole so that the first constraint with ⟨A, RRᵀ⟩·b > 0 does); zero rows: plain with rows 0, ⌊n/2⌋, n − 1 zero."""
    n = bc["C"].shape[0]
    rng = np.random.Generator(np.random.PCG64(seed))
    plain = rng.uniform(-1.0, 1.0, size=(n, r))
    k = rng.integers(-20, 21, size=n)
    k[0], k[n - 1] = -20, 20                  # both ends of the range are present in every case
    graded = plain * 2.0 ** k[:, None]
    near = rng.uniform(-1.0, 1.0, size=(n, r))
    done = np.zeros(n, dtype=bool)
    for i, A in enumerate(bc["As"]):
        if isinstance(A, sj.SparseMatrixCOO) and A.is_.size == 1 and A.is_[0] == A.js[0]:
            j, a = int(A.is_[0]), float(A.vs[0])
            if not done[j] and bc["bs"][i] / a > 0:
                near[j] *= np.sqrt(bc["bs"][i] / a) / np.linalg.norm(near[j])
                done[j] = True
    if not done.any():
        q = np.asarray(A_pair_hp(bc["C"], bc["As"], near, near)["q"], dtype=np.float64)
        for i in range(len(bc["As"])):
            if q[i] * bc["bs"][i] > 0:
                near *= np.sqrt(bc["bs"][i] / q[i])
                break
    zero = rng.uniform(-1.0, 1.0, size=(n, r))
    zero[[0, n // 2, n - 1]] = 0.0
    return dict(plain=plain, graded=graded, near=near, zero=zero)


def case_inputs(name, r):
    """[(tag, R, λ, λ_ub, σ, reference of f!, first of its R)] — the references above FP64 computed once per (case, rank).
    λ_ub: +∞ on equality rows; on inequality rows alternately 0 (the solver's own) and ½ or 1½ times λ − σv above FP64, which
    puts the row on either side of the cap by a factor and never near the tie."""
    bc = built(name)
    if r in bc["inputs"]:
        return bc["inputs"][r]
    case = CASES[name]
    C, As, bs, ct = bc["C"], bc["As"], bc["bs"], bc["ct"]
    m = len(As)
    seed = 7000 + 13 * sorted(CASES).index(name) + r
    Rs = four_R(bc, r, seed)
    rng = np.random.Generator(np.random.PCG64(seed + 1))
    lam1 = 0.1 * rng.standard_normal(m) * 2.0 ** rng.integers(-10, 11, size=m)
    mults = [(np.zeros(m), 2.0), (lam1, 1e3), (np.zeros(m), 1e3), (lam1, 2.0)]
    out = []
    for k, (kind, R) in enumerate(Rs.items()):
        picks = [mults[k]] if case["lean"] else mults
        for j, (lam, sigma) in enumerate(picks):
            ub = np.full(m, np.inf)
            if ct.any():
                free = np.asarray(fg_hp(C, As, bs, R, lam, ub, sigma)["yt"], dtype=np.float64)
                q = np.flatnonzero(ct)
                ub[q] = 0.0
                ub[q[1::4]] = 0.5 * free[q[1::4]]
                ub[q[3::4]] = 1.5 * free[q[3::4]]
            # λ ≤ λ_ub as the solver keeps it (src/structs.jl:225-240), and where it had to be moved, strictly below: with λ = λ_ub
            # a near-feasible row (v ≈ 0) would sit on the capping tie by construction
            lam0 = not lam.any()
            with np.errstate(invalid="ignore"):
                lam = np.where(lam > ub, ub - np.abs(ub) - 0.01, lam)
            out.append(dict(tag=f"{kind}/lam{'0' if lam0 else 'g'}/sigma{sigma:g}", R=R, lam=lam, ub=ub, sigma=sigma,
                            ref=fg_hp(C, As, bs, R, lam, ub, sigma), first=j == 0, kind=kind))
    bc["inputs"][r] = out
    return out


def new_handle(abi, data, r):
    cfg = sj.BurerMonteiroConfig(σ_0=2.0, numlbfgsvecs=4, seed=1, printlevel=0)
    return sj.build_solver(abi, data, r, cfg)


def _load(s_, inp):
    s_.Rt = inp["R"]
    s_.λ_ub = inp["ub"]
    s_.λ = inp["lam"]
    s_.σ = inp["sigma"]


def check_f_state(bc, inp, pv_raw, pv, obj, L, lb, worst, carve):
    """v (every constraint and the objective) and ℒ against fg_hp; obj and primal_vio exactly what they are defined from."""
    ref = inp["ref"]
    m = len(bc["As"])
    worst["v"] = max(worst["v"], worst_ratio(pv_raw, ref["v"], ref["bound_v"]))
    worst["L"] = max(worst["L"], worst_ratio([L], [ref["L"]], [ref["bound_L"]]))
    assert obj == pv_raw[m], (inp["tag"], obj, pv_raw[m])
    assert np.array_equal(pv, np.maximum(pv_raw[:m], lb)), inp["tag"]


def check_y(bc, inp, pv_raw, y, worst, carve):
    """y = −ỹ from the handle's own primal_vio_raw; an entry within the bound of the capping tie may sit on either branch and
    is counted."""
    m = len(bc["As"])
    yt = ytilde_from(pv_raw, inp["lam"], inp["ub"], inp["sigma"])
    assert y[m] == 1.0
    got = -_ld(y[:m])
    err = np.abs(got - yt["yt"])
    near = yt["near"]
    if near.any():
        err = np.where(near, np.minimum(np.abs(got - yt["ub"]), np.abs(got - yt["free"])), err)
        carve.append(int(near.sum()))
    worst["y"] = max(worst["y"], worst_ratio(err, np.zeros(m), yt["bound"]))
    return yt


def check_g_state(bc, inp, y, St, Sf, G, worst, big=False):
    ref = S_and_G_hp(bc["C"], bc["As"], y, inp["R"], bc["pattern"])
    if not big:
        assert St.size == bc["pattern"]["nnzT"] and Sf.size == bc["pattern"]["nnzS"]
        worst["S"] = max(worst["S"], worst_ratio(St, ref["triu"], ref["bound_triu"]), worst_ratio(Sf, ref["full"], ref["bound_full"]))
    worst["G"] = max(worst["G"], worst_ratio(G, ref["G"], ref["bound_G"]))
    return ref


def check_norms(G, pv, gn, pn, normC, normb, worst):
    """‖G‖/normC and ‖pv‖/normb from the handle's own G and pv: a sum of N non-negative terms in any order is good to N·u
    relative, its root to half of that, and the root, the division and the returned value round once each: (N/2 + 3)·u."""
    for key, arr, got, div in (("gnorm", G, gn, normC), ("pnorm", pv, pn, normb)):
        want = np.sqrt(np.sum(_ld(arr) ** 2)) / LD(div)
        worst[key] = max(worst[key], worst_ratio([got], [want], [(arr.size / 2 + 3) * LD(U53) * want]))


def run_case(abi, name, r, hip=False):
    """The whole sequence of one (case, rank) on the library behind `abi` → (worst error/bound per quantity, capping carve-outs,
    stats of the fused handle, number of fg! calls on it).  Asserts error/bound ≤ 1 for every quantity at the end, so that a
    failing run still reports all of them."""
    case, bc = CASES[name], built(name)
    C, As, data = bc["C"], bc["As"], bc["data"]
    m, n = len(As), C.shape[0]
    worst = {k: 0.0 for k in QUANTITIES}
    carve = []
    a, b = new_handle(abi, data, r), new_handle(abi, data, r)
    lb = a.primal_vio_lb
    normC, normb = 3.0, 2.0
    n_fg = 0
    rng = np.random.Generator(np.random.PCG64(99 + r))
    for inp in case_inputs(name, r):
        R = inp["R"]
        # ---- f!, then g!, one by one (always the generic kernels) ----
        _load(a, inp)
        L = a.f()
        pv_raw, pv, obj = a.primal_vio_raw, a.primal_vio, a.obj
        check_f_state(bc, inp, pv_raw, pv, obj, L, lb, worst, carve)
        a.g()
        y = a.y
        check_y(bc, inp, pv_raw, y, worst, carve)
        G = a.Gt
        if case["big"]:
            gref = check_g_state(bc, inp, y, None, None, G, worst, big=True)
        else:
            gref = check_g_state(bc, inp, y, a.get_vec(cabi.V_TRIU_S_NZVAL), a.get_vec(cabi.V_S_NZVAL), G, worst)
        gn, pn = a.norms(normC, normb, True, True)
        check_norms(G, pv, gn, pn, normC, normb, worst)
        # ---- fg! on the second handle, which never runs f! or g! alone: the fused routes ----
        _load(b, inp)
        Lb, gnb, pnb = b.fg(normC, normb, True, True)
        n_fg += 1
        pvb_raw, pvb, yb, Gb = b.primal_vio_raw, b.primal_vio, b.y, b.Gt
        check_f_state(bc, inp, pvb_raw, pvb, b.obj, Lb, lb, worst, carve)
        check_y(bc, inp, pvb_raw, yb, worst, carve)
        if np.array_equal(yb, y):
            worst["G"] = max(worst["G"], worst_ratio(Gb, gref["G"], gref["bound_G"]))
        else:
            check_g_state(bc, inp, yb, None, None, Gb, worst, big=True)
        check_norms(Gb, pvb, gnb, pnb, normC, normb, worst)
        if case["big"] or not inp["first"]:
            continue
        # ---- 𝒜 in modes 1 and 2 (the latter is what the exact line search launches), 𝒜ᵀ with a graded y ----
        D = rng.uniform(-1.0, 1.0, size=R.shape) * 2.0 ** rng.integers(-8, 9, size=n)[:, None]
        a.dirt = D
        a.A(cabi.F_RT, cabi.F_DIRT, cabi.V_A_DD)
        q1 = A_pair_hp(C, As, R, D)
        worst["A1"] = max(worst["A1"], worst_ratio(a.get_vec(cabi.V_A_DD), q1["q"], q1["depth"] * LD(U53) * q1["mag"]))
        try:
            a.linesearch(1.0)
        except cabi.SdplrError:          # (the quartic of an arbitrary state may have no admissible root: 𝒜 has run by then)
            pass
        q2 = A_pair_hp(C, As, D, D)
        worst["A2"] = max(worst["A2"], worst_ratio(a.A_RD, 2 * q1["q"], q1["depth"] * LD(U53) * 2 * q1["mag"]),
                          worst_ratio(a.A_DD, q2["q"], q2["depth"] * LD(U53) * q2["mag"]))
        yr = rng.standard_normal(m + 1) * 2.0 ** rng.integers(-10, 11, size=m + 1)
        a.Rt = R
        a.y = yr
        a.At_preprocess()
        sref = S_and_G_hp(C, As, yr, R, bc["pattern"])
        worst["At_S"] = max(worst["At_S"], worst_ratio(a.get_vec(cabi.V_TRIU_S_NZVAL), sref["triu"], sref["bound_triu"]),
                            worst_ratio(a.get_vec(cabi.V_S_NZVAL), sref["full"], sref["bound_full"]))
        a.At_left(cabi.F_GT, cabi.F_RT)
        worst["At_left"] = max(worst["At_left"], worst_ratio(a.Gt, sref["G"] / 2, sref["bound_G"] / 2))
        x = rng.uniform(-1.0, 1.0, size=(n, 3)) * 2.0 ** rng.integers(-8, 9, size=n)[:, None]
        xref = S_and_G_hp(C, As, yr, x, bc["pattern"])
        worst["At_right"] = max(worst["At_right"], worst_ratio(a.At_right(x), xref["G"] / 2, xref["bound_G"] / 2))
    stats = b.stats() if hip else {}
    a.close(); b.close()
    return worst, carve, stats, n_fg


def report(lib, name, r, worst, carve):
    print(f"fg {lib} {name} r={r}: error/bound " + " ".join(f"{k} {worst[k]:.3g}" for k in QUANTITIES) + f"  cap ties {sum(carve)}")


def assert_case(name, r, worst, carve):
    bad = {k: v for k, v in worst.items() if not v <= 1.0}
    assert not bad, (name, r, bad)
    assert sum(carve) <= 2, (name, r, carve)
