"""GPU parity at the BASELINE.json sizes (run on the MI355X box with -m gpu): the HIP library against the CPU oracle
on the north-star inputs themselves — same R₀, λ₀ = 0, σ₀ — through the C ABI.

north_star: "Results match the … CPU reference on the same inputs within a stated FP64 tolerance (1e-8 on ‖grad‖ and
primal objective)".  Here: fg! + 5 native inner iterations (src/sdplr.jl:190-278) on both libraries; ℒ, ‖grad‖, ‖pv‖,
obj to 1e-8 relative and R to 1e-8 (max-norm, relative), at full grids (nb_step = 512, nb_tile = 1024 blocks — the
class of bug a small instance cannot see); the first 10 of the 232 Lanczos steps of the dual bound
(src/coreop.jl:481-500) to 1e-9; config 5 (64 MaxCut instances, 8 in flight) on the route it takes by default."""
import os

import numpy as np
import pytest
import scipy.sparse as sp

import sdplrplus_jl_amd as sj
from sdplrplus_jl_amd import batch, cabi, problems
from helpers import make_solver

pytestmark = pytest.mark.gpu

TOL = 1e-8          # BASELINE.json north_star tolerance on ‖grad‖ and the primal objective
ITERS = 5


def rel(a, b):
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    return float(np.max(np.abs(a - b)) / (1.0 + np.max(np.abs(b))))


def _instance(which):
    if which == "maxcut_n1e5":          # BASELINE.json configs[1]: the north-star instance of bench.py
        return problems.maxcut_data(problems.gnp_graph(100_000, 2e-4, 20240610)), 0
    if which == "lovasz_chunglu_5e4":   # configs[2] stand-in: Chung–Lu power law, n ≈ 5e4, |E| ≈ 2.5e5
        return problems.lovasz_theta_data(problems.chung_lu_graph(50_000, 10.0, 2.5, 3)), 1
    if which == "minbis_n1e5":          # configs[3]
        return problems.minimum_bisection_data(problems.gnp_graph(100_000, 2e-4, 4)), 2
    raise KeyError(which)


def _sparse_S_and_tau(data, y, q):
    """(S without its rank-one term as CSR, c of the rank-one term c·11ᵀ, τ) for S = Σ yᵢAᵢ + y_C·C assembled from the batched
    constraint set.  τ = q·γ·A as in helpers.whole_run_checks: γ = 4·(d + ⌈log₂ n⌉ + 8)·2⁻⁵³ with d the longest row (n with a
    rank-one term), A = ‖|S|‖∞ — with the rank-one term row i of |S| sums to Σ_{j in the row's pattern}(|S_ij + c| − |c|) + n·|c|."""
    n, b = data.n, data.sparse
    w = np.repeat(np.asarray(y)[b.global_inds], np.diff(b.ent_ptr))
    Ssp = sp.coo_matrix((b.V * w, (b.I, b.J)), shape=(n, n)).tocsr()
    Ssp.sum_duplicates()
    c = 0.0
    for gid, M in data.lowrank:
        assert M.B.shape[1] == 1 and np.all(M.B == 1.0)
        c += y[gid] * M.D[0]
    shifted = Ssp.copy()
    shifted.data = np.abs(shifted.data + c) - abs(c)
    A = float(np.max(np.asarray(shifted.sum(axis=1)).ravel() + n * abs(c)))
    d = n if data.lowrank else int(np.max(np.diff(Ssp.indptr)))
    gamma = 4.0 * (d + int(np.ceil(np.log2(n))) + 8) * 2.0 ** -53
    return Ssp, c, q * gamma * A


def _lambda_min_and_tau(data, y, q):
    """(λ_min(S), τ, ‖S·z − λ·z‖): scipy's eigsh for the smallest eigenvalue of the sparse S plus its rank-one term as a
    LinearOperator, run to a residual far below τ (the caller asserts it)."""
    import scipy.sparse.linalg as sla
    n = data.n
    Ssp, c, tau = _sparse_S_and_tau(data, y, q)
    op = sla.LinearOperator((n, n), matvec=lambda x: Ssp @ x + c * np.sum(x), dtype=np.float64)
    vals, vecs = sla.eigsh(op, k=1, which="SA", tol=1e-12, ncv=48, maxiter=20000,
                           v0=np.random.Generator(np.random.PCG64(17)).standard_normal(n))
    z = vecs[:, 0]
    return float(vals[0]), tau, float(np.linalg.norm(op.matvec(z) - vals[0] * z))


@pytest.mark.parametrize("which", ["maxcut_n1e5", "lovasz_chunglu_5e4", "minbis_n1e5"])
def test_first_iterations_match_oracle_at_baseline_size(hip_abi, oracle_abi, which):
    data, seed = _instance(which)
    r = 32
    normC, normb = data.normC(), float(np.linalg.norm(data.b))
    out = {}
    for name, abi in (("hip", hip_abi), ("oracle", oracle_abi)):
        s, _ = make_solver(abi, data, r, seed=seed)
        st = s.fg(normC, normb)
        res = s.inner_loop(normC, normb, True, True, False, 0.0, -1e300, ITERS, 0.0, *st)
        assert res[4] == ITERS and res[5] == 2
        out[name] = dict(fg=st, L=res[0], gnorm=res[1], pvnorm=res[2], alpha=res[3], obj=s.obj, R=s.Rt, G=s.Gt,
                         pv=s.primal_vio_raw, y=s.y)
        if name == "hip":
            # the Lanczos recurrence on the S this state defines, q = 2⌈√100·ln n⌉ (src/coreop.jl:402)
            v0 = np.random.Generator(np.random.PCG64(5)).standard_normal(data.n)
            out["v0"] = v0
        q = int(2 * np.ceil(np.sqrt(100.0) * np.log(data.n)))
        s.dual_obj(float(data.n), 0, out["v0"])                 # copy2y + 𝒜t_preprocess! (:384-385) + Lanczos
        al, be, k = s.lanczos(q, out["v0"])
        assert k == q
        out[name].update(lz_alpha=al, lz_beta=be, q=q, ritz=s.tridiag_mineig(al, be), y_S=s.y)
        s.close()
    h, o = out["hip"], out["oracle"]
    assert np.allclose(h["fg"], o["fg"], rtol=1e-11)
    for key in ("L", "gnorm", "pvnorm", "obj"):
        assert abs(h[key] - o[key]) <= TOL * max(abs(o[key]), 1e-300), (which, key, h[key], o[key])
    assert abs(h["alpha"] - o["alpha"]) <= 1e-7 * max(1.0, abs(o["alpha"]))
    assert rel(h["R"], o["R"]) < TOL
    # G = 2·S·R amplifies the 1e-9 difference of the two R's (their step sizes differ in the 9th digit: the root finders
    # are not the same code) by ‖S‖; with a rank-one constraint 11ᵀ the amplification of a COMMON shift of all
    # rows is n·y_k, not ‖S‖ — MinBisection at n = 1e5 shows 2e-7 on max|G| while ‖grad‖ itself agrees to 1e-8.
    assert rel(h["G"], o["G"]) < (1e-6 if data.lowrank else 10 * TOL)
    assert rel(h["pv"], o["pv"]) < TOL and rel(h["y"], o["y"]) < TOL
    # Plain Lanczos (no re-orthogonalisation, src/coreop.jl:481-500) is only comparable while its recurrence is
    # well conditioned: a round-off ε in step j comes back multiplied by ≈ ‖S‖/β_j in step j + 1, and once a Ritz pair has
    # converged (β collapses) the two runs decouple.  Steps are compared to 1e-8 (the two S already differ by the
    # 1e-9 of the two R they come from) while ε·Π_j(‖S‖/β_j) < 1e-10,
    # ten at most: all ten on MaxCut (‖S‖/β ≈ 2-7); two on Lovász-θ and one on MinBisection, whose rank-one terms
    # (−11ᵀ, y·11ᵀ: λ_max ≈ 5e4 resp. 7e7 against β ≈ 30 … 1e3) converge within three steps.
    scale = np.max(np.abs(o["lz_alpha"][:10]))
    amp, K = np.finfo(float).eps, 0
    while K < 10 and amp < 1e-10:
        K += 1
        amp *= scale / o["lz_beta"][K - 1]
    assert K >= 1 and (which != "maxcut_n1e5" or K == 10), (K, o["lz_beta"][:10])
    assert np.allclose(h["lz_alpha"][:K], o["lz_alpha"][:K], rtol=1e-8, atol=1e-12 * scale), (K, h["lz_alpha"][:K], o["lz_alpha"][:K])
    assert np.allclose(h["lz_beta"][:K], o["lz_beta"][:K], rtol=1e-8, atol=1e-12 * scale)
    # … and what the dual bound actually uses, the smallest Ritz value of all q steps (src/coreop.jl:502-513)
    assert abs(h["ritz"] - o["ritz"]) <= 1e-6 * scale, (h["ritz"], o["ritz"])
    # … and a bound that does not ask two decoupled runs to agree: every eigenvalue of the tridiagonal of a correct
    # finite-precision run lies within τ = q·γ·‖|S|‖∞ of the spectrum of the S it ran on (the y dual_obj left), so the Ritz
    # value the dual bound uses is no smaller than λ_min − τ.  λ_min: eigsh, whose value is a Ritz value itself (never below
    # the true λ_min), converged to a residual below τ/10 (MaxCut: 2e-13 against τ = 1.7e-10).
    lam_min, tau, resid = _lambda_min_and_tau(data, h["y_S"], h["q"])
    print(f"{which}: Ritz {h['ritz']:.12g}, lambda_min {lam_min:.12g}, tau {tau:.3g}, eigsh residual {resid:.3g}")
    assert resid <= 0.1 * tau, (resid, tau)
    assert h["ritz"] >= lam_min - tau, (h["ritz"], lam_min, tau)


def test_twenty_five_iterations_stay_within_the_north_star_tolerance(hip_abi, oracle_abi):
    """Round-off differences between the two implementations (summation orders, the cubic's root finder) grow along the
    L-BFGS trajectory by ≈ 1.5–1.6× per inner iteration on the north-star instance (measured: 3e-13 after 5 iterations,
    1.5e-9 on ‖grad‖ after 25, decoupled trajectories after ≈ 60 — scripts/drift_vs_oracle.py): nonconvex descent is
    that sensitive, on any pair of FP64 implementations.  25 iterations is as far as BASELINE.json's 1e-8 can be asked of
    the STATE; beyond it the comparison is on what the solve returns (test_gpu_parity.py, scripts/stress_solve.py)."""
    data, seed = _instance("maxcut_n1e5")
    normC, normb = data.normC(), float(np.linalg.norm(data.b))
    out = {}
    for name, abi in (("hip", hip_abi), ("oracle", oracle_abi)):
        s, _ = make_solver(abi, data, 32, seed=seed)
        res = s.inner_loop(normC, normb, True, True, False, 0.0, -1e300, 25, 0.0, *s.fg(normC, normb))
        assert res[4] == 25
        out[name] = (np.array([res[0], res[1], res[2], s.obj]), s.Rt)
        s.close()
    (vh, Rh), (vo, Ro) = out["hip"], out["oracle"]
    assert np.all(np.abs(vh - vo) <= TOL * np.abs(vo)), (vh, vo)
    assert rel(Rh, Ro) < TOL


def _batch_instances():
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gset_G1_G9.npz"))
    graphs = [problems.graph_from_edges(int(z[f"G{k}_n"]), z[f"G{k}"]) for k in range(1, 10)]
    graphs += [problems.gnp_graph(800, 0.06, seed) for seed in range(10, 65)]
    return graphs


def test_config5_full_batch_on_its_default_route(hip_abi, oracle_abi, monkeypatch):
    """BASELINE.json configs[4] on one GPU: all 64 MaxCut instances of the batch (Gset G1–G9 as in
    exps/batch_test.txt:1-9 — rank 10, ptol = objtol = 0.01 — plus 55 seeded G(800, 0.06)), 8 in flight, WITHOUT
    SDPLR_HIP_FORCE_GRAPH: n·r = 8000 < 2¹⁷, so this is the eager route the batch really takes.  Every objective,
    dual bound and iteration count must equal a serial run of the same instance bit for bit, and G1–G9 must land
    within the objtol window of the oracle's solve of the same seed."""
    monkeypatch.delenv("SDPLR_HIP_FORCE_GRAPH", raising=False)
    graphs = _batch_instances()
    assert len(graphs) == 64 and graphs[0].shape == (800, 800) and graphs[0].nnz == 38352
    kw = dict(make_data=problems.maxcut_data, ptol=0.01, objtol=0.01, seed=0, prior_trace_bound=800.0)
    conc = batch.gather(batch.solve_local(graphs, 0, 1, 10, concurrency=8, **kw), 64)
    ser = batch.gather(batch.solve_local(graphs, 0, 1, 10, concurrency=1, **kw), 64)
    assert conc.shape == ser.shape == (64, batch.N_FIELDS)
    assert np.array_equal(conc[:, :4], ser[:, :4])            # index, obj, max_dual_value, iterations
    # every solve stopped on the reference's test (src/sdplr.jl:335-345): relative duality gap ≤ objtol.  (The iterate is
    # only ptol-feasible, so its objective may lie slightly BELOW the dual bound: weak duality binds feasible points.)
    gap = (conc[:, 1] - conc[:, 2]) / np.minimum(np.abs(conc[:, 1]), np.abs(conc[:, 2]))
    assert np.all(gap <= 1e-2) and np.all(gap >= -1e-2)
    # best known cuts of G1–G9 are 11 624 … 12 083-ish SDP bounds: −obj lies in between ±1 %
    assert np.all((-conc[:9, 1] >= 11400 * 0.99) & (-conc[:9, 1] <= 12100 * 1.01))
    ora = batch.gather(batch.solve_local(graphs[:9], 0, 1, 10, abi=oracle_abi, concurrency=1, **kw), 9)
    # both stop with a relative duality gap ≤ objtol = 1e-2 around the same SDP value
    assert np.all(np.abs(conc[:9, 1] - ora[:, 1]) <= 1e-2 * np.abs(ora[:, 1]))
    assert np.all(np.abs(conc[:9, 2] - ora[:, 2]) <= 2e-2 * np.abs(ora[:, 2]))


def test_production_scale_grids_n3e5(hip_abi, monkeypatch):
    """n = 3·10⁵, r = 32 MaxCut: more than 1024·16 tiles' worth of rows (the tile kernel's grid-stride loop), 24-bit
    column packing with n > 2¹⁸, full step / update grids.  Five iterations on the default route and on the routes
    with the tile kernel / fused update / singleton fusion switched off, each checked against a scipy recomputation
    of the state (𝒜, G = 2(C + Diag y)R, W = A_g·D through P = A_g·R) and against the default route to 1e-9."""
    n, r = 300_000, 32
    A = problems.gnp_graph(n, 20.0 / n, 77)
    data = problems.maxcut_data(A)
    normC, normb = data.normC(), float(np.linalg.norm(data.b))

    def run():
        g, _ = make_solver(hip_abi, data, r, seed=3)
        st = g.fg(normC, normb)
        res = g.inner_loop(normC, normb, True, True, False, 0.0, -1e300, 5, 0.0, *st)
        out = (res, g.Rt, g.Gt, g.primal_vio_raw, g.y, g.dirt)
        g.close()
        return out

    base = run()
    res, R, G, pv, y, D = base
    assert res[4] == 5
    C = data.C
    assert np.max(np.abs(pv[:-1] - (np.einsum("ij,ij->i", R, R) - 1.0))) < 1e-9
    CR = C @ R
    assert abs(pv[-1] - float(np.sum(CR * R))) < 1e-10 * abs(pv[-1])
    Gref = 2 * (CR + y[:-1, None] * R)
    assert np.max(np.abs(G - Gref)) < 1e-10 * np.max(np.abs(Gref))
    assert res[1] == pytest.approx(np.linalg.norm(Gref) / normC, rel=1e-10)
    for toggle in ("SDPLR_HIP_NO_TILE", "SDPLR_HIP_NO_UPDFUSE", "SDPLR_HIP_NO_FAST2"):
        monkeypatch.setenv(toggle, "1")
        alt = run()
        monkeypatch.delenv(toggle)
        assert np.allclose(alt[0][:3], res[:3], rtol=1e-9), toggle
        assert rel(alt[1], R) < 1e-9 and rel(alt[2], G) < 1e-8 and rel(alt[5], D) < 1e-7, toggle


def test_row_offsets_just_below_2_pow_32(hip_abi):
    """8·n·r = 4.26e9 < 2³² = 4.29e9 (n = 2²⁰, r = 508): the largest factor the 32-bit row byte offsets of the tile /
    fused step kernels serve (beyond it the library must — and does — take the 64-bit row kernels).  r = 508 also
    means whole-wave groups with four chunks per row, the last one ragged.  Checked with scipy identities after fg!
    and after 3 inner iterations."""
    n, r = 1 << 20, 508
    assert 8 * n * r < 2 ** 32 <= 8 * n * (r + 4)
    A = problems.gnp_graph(n, 8.0 / n, 5)
    data = problems.maxcut_data(A)
    g, _ = make_solver(hip_abi, data, r, seed=4)
    normC, normb = data.normC(), float(np.linalg.norm(data.b))
    st = g.fg(normC, normb)
    res = g.inner_loop(normC, normb, True, True, False, 0.0, -1e300, 3, 0.0, *st)
    assert res[4] == 3 and res[0] < st[0]
    R = g.Rt
    pv = g.primal_vio_raw
    assert np.max(np.abs(pv[:-1] - (np.einsum("ij,ij->i", R, R) - 1.0))) < 1e-8
    CR = data.C @ R
    assert abs(pv[-1] - float(np.sum(CR * R))) < 1e-10 * abs(pv[-1])
    y = g.y
    G = g.Gt
    CR += y[:-1, None] * R
    CR *= 2.0
    assert np.max(np.abs(G - CR)) < 1e-10 * np.max(np.abs(CR))
    g.close()


def test_scratch_slots_and_device_vectors(hip_abi, oracle_abi):
    """𝒜!(out, aux, Ut[, Vt]) on the caller's own matrices (SDPLR_F_SCRATCH / SDPLR_V_SCRATCH) leaves the solver state
    alone; 𝒜t!(y, aux, x, var) on device vectors (sdplr_hip_At_right_device) equals the host-vector form."""
    import ctypes as C
    from helpers import make_data, primal_vio_dense
    data, Cm, As, bs = make_data("minimum_bisection", 3, 40, 0.3)
    g, _ = make_solver(hip_abi, data, 6, seed=1)
    normC, normb = data.normC(), float(np.linalg.norm(data.b))
    st = g.fg(normC, normb)
    before = (g.Rt, g.Gt, g.primal_vio_raw, g.A_RD, g.A_DD)
    rng = np.random.Generator(np.random.PCG64(3))
    U, V = rng.standard_normal((data.n, 6)), rng.standard_normal((data.n, 6))
    out = g.A_of(U)
    ref = primal_vio_dense(Cm, As, np.zeros(len(bs)), U)
    assert np.max(np.abs(out - ref)) < 1e-10 * (1 + np.max(np.abs(ref)))
    out2 = g.A_of(U, V)
    X = (U @ V.T + V @ U.T) / 2
    ref2 = np.array([np.sum(A_.toarray() * X) for A_ in As] + [np.sum(Cm.toarray() * X)])
    assert np.max(np.abs(out2 - ref2)) < 1e-10 * (1 + np.max(np.abs(ref2)))
    after = (g.Rt, g.Gt, g.primal_vio_raw, g.A_RD, g.A_DD)
    assert all(np.array_equal(a, b) for a, b in zip(before, after))
    # device vectors: raw hipMalloc'ed buffers through the HIP runtime the library itself uses
    hip = C.CDLL("libamdhip64.so.7")      # the soname libsdplr_hip.so is linked against: the same loaded runtime
    n, k = data.n, 3
    x = np.asfortranarray(rng.standard_normal((n, k)))
    dx, dy = C.c_void_p(), C.c_void_p()
    assert hip.hipMalloc(C.byref(dx), C.c_size_t(8 * n * k)) == 0 and hip.hipMalloc(C.byref(dy), C.c_size_t(8 * n * k)) == 0
    assert hip.hipMemcpy(dx, x.ctypes.data_as(C.c_void_p), C.c_size_t(8 * n * k), 1) == 0
    g.At_right_device(dx.value, dy.value, k)
    yd = np.empty((n, k), order="F")
    assert hip.hipMemcpy(yd.ctypes.data_as(C.c_void_p), dy, C.c_size_t(8 * n * k), 2) == 0
    assert np.array_equal(yd, g.At_right(x))
    rc = g.abi.At_right_device(g._h, x.ctypes.data_as(C.c_void_p), dy, 1)                    # a host pointer is refused
    assert rc == cabi.ERR_INVALID_ARG
    hip.hipFree(dx); hip.hipFree(dy)
    assert g.stats()["graph_capture_failures"] == 0
    g.close()


def test_device_eigensolver_against_arpack(hip_abi):
    """SDP_S_eigval on the device (thick-restart Lanczos, basis in HBM; src/coreop.jl:351-374) against scipy's ARPACK
    applied to the same S on the host: the two smallest eigenvalues to 1e-8 of ‖S‖ — MaxCut n = 2·10⁴ (sparse S) and
    MinBisection n = 2·10⁴ (S with a rank-one term, λ_max ≫ |λ_min|); and DIMACS err6 = ⟨Rt, Rt·S⟩ as one device dot."""
    from scipy.sparse.linalg import LinearOperator, eigsh
    for builder, seed in ((problems.maxcut_data, 11), (problems.minimum_bisection_data, 12)):
        A = problems.gnp_graph(20_000, 6e-4, seed)
        data = builder(A)
        n, m = data.n, data.m
        g, _ = make_solver(hip_abi, data, 8, seed=seed)
        normC, normb = data.normC(), float(np.linalg.norm(data.b))
        st = g.fg(normC, normb)
        g.inner_loop(normC, normb, True, True, False, 0.0, -1e300, 30, 0.0, *st)
        g.dual_obj(float(n), 0, np.ones(n))                      # y = copy2y_λ_sub_pvio!, S current
        y = g.y
        S = sp.csr_matrix(data.C) + sp.diags(y[:n])
        lowrank = y[n] if data.lowrank else 0.0
        Sop = LinearOperator((n, n), matvec=lambda x: S @ x + lowrank * np.ones(n) * np.sum(x), dtype=np.float64)
        ref = np.sort(eigsh(Sop, k=2, which="SA", tol=1e-10, ncv=60)[0])
        scale = max(abs(ref[0]), float(abs(S).sum(axis=1).max()), abs(lowrank) * n)
        v0 = np.random.Generator(np.random.PCG64(1)).standard_normal(n)
        ev = sj.SDP_S_eigval(g, 2, True, which="SA", ncv=60, tol=1e-10, v0=v0)
        assert np.max(np.abs(ev - ref)) <= 1e-8 * scale, (ev, ref)
        vals, matvecs, nconv = g.S_eigval(2, "SA", 60, 1e-10, 1000, v0)
        assert nconv == 2 and matvecs >= 60
        la = g.S_eigval(1, "LA", 40, 1e-8, 1000, v0)[0][0]
        assert la == pytest.approx(eigsh(Sop, k=1, which="LA", tol=1e-10)[0][0], rel=1e-7)
        # err6 numerator on the device vs numpy
        R = g.Rt
        g.At_left(cabi.F_SCRATCH, cabi.F_RT)
        xz = g.factor_dot(cabi.F_RT, cabi.F_SCRATCH)
        ref_xz = float(np.sum(R * (S @ R + lowrank * np.outer(np.ones(n), R.sum(axis=0)))))
        assert xz == pytest.approx(ref_xz, rel=1e-10, abs=1e-8 * scale)
        g.close()


@pytest.mark.parametrize("n", [131072, 262144 - 1000])
def test_lanczos_band_plan_at_full_bands_and_chunks(hip_abi, monkeypatch, n):
    """n = 2¹⁷ and just below 2¹⁸: a full 16 384-column band AND a full 4 096-row chunk would need all 160 KB of LDS next
    to the band kernel's static arrays — the plan must take more chunks instead (and the launch must succeed).  The band
    form's coefficients against the gather form's over the first well-conditioned steps, the Ritz value of 60 steps."""
    A = problems.gnp_graph(n, 12.0 / n, 21)
    data = problems.maxcut_data(A)
    normC, normb = data.normC(), float(np.linalg.norm(data.b))
    v0 = np.random.Generator(np.random.PCG64(3)).standard_normal(n)
    out = {}
    for form in ("band", "gather"):
        if form == "gather":
            monkeypatch.setenv("SDPLR_HIP_NO_LZBAND", "1")
        g, _ = make_solver(hip_abi, data, 4, seed=1)
        st = g.fg(normC, normb)
        g.inner_loop(normC, normb, True, True, False, 0.0, -1e300, 3, 0.0, *st)
        d, e = g.dual_obj(float(n), 0, v0)
        a, b, k = g.lanczos(60, v0)
        out[form] = (d, e, a, b, k, g.tridiag_mineig(a, b), g.y)
        g.close()
    (d1, e1, a1, b1, k1, m1, y1), (d2, e2, a2, b2, k2, m2, y2) = out["band"], out["gather"]
    assert k1 == k2 == 60 and np.array_equal(y1, y2)        # the same S on both forms
    assert np.allclose(a1[:8], a2[:8], rtol=1e-9, atol=1e-12) and np.allclose(b1[:8], b2[:8], rtol=1e-9, atol=1e-12)
    # two correct runs on the same S: smallest Ritz values within 2τ, τ = q·γ·‖|S|‖∞ (60 steps; dual_obj: 2⌈10·ln n⌉ steps)
    q_dual = int(2 * np.ceil(10.0 * np.log(n)))
    tau60, tau_dual = (_sparse_S_and_tau(data, y1, q)[2] for q in (60, q_dual))
    print(f"n = {n}: Ritz difference {abs(m1 - m2):.3g} (2 tau {2 * tau60:.3g}), dual_obj's {abs(e1 - e2):.3g} (2 tau {2 * tau_dual:.3g})")
    assert abs(m1 - m2) <= 2 * tau60 and abs(e1 - e2) <= 2 * tau_dual and d1 == pytest.approx(d2, rel=1e-6)


def _omp_oracle():
    import ctypes as C
    from oracle import oracle
    oracle.build()
    omp = sj.CABI(oracle.LIB_OMP, "sdplr_oracle_")
    C.CDLL("libgomp.so.1").omp_set_num_threads(min(16, len(os.sched_getaffinity(0))))
    return omp


def test_schedule_parity_at_baseline_size_maxcut(hip_abi):
    """End to end at the north-star size (MaxCut G(1e5, 2e-4), r = 32, ptol = objtol = 1e-2): _sdplr's schedule — the σ
    sequence, the tolerances η/ω of every major iteration, the rank history, the stop by the duality-gap test
    (src/sdplr.jl:310-357) — on the HIP library and on the oracle (its OpenMP build: the same source,
    tests/test_oracle_omp.py ties it to the one-thread checker; ≈ 17 s).  The two trajectories decouple in round-off after
    ≈ 60 inner iterations, so inner iteration counts may differ by a few; the schedule may not, and
    objective and dual bound must agree within objtol."""
    n = 100_000
    data = problems.maxcut_data(problems.gnp_graph(n, 2e-4, 20240610))
    kw = dict(r=32, ptol=1e-2, objtol=1e-2, seed=0, prior_trace_bound=float(n), printlevel=0)
    a = sj.sdplr(data=data, abi=hip_abi, **kw)
    b = sj.sdplr(data=data, abi=_omp_oracle(), **kw)
    sa, sb = a["schedule"], b["schedule"]
    assert a["majoriter"] == b["majoriter"] and len(sa) == len(sb)
    assert [(t[0], t[2], t[3], t[4], t[5]) for t in sa] == [(t[0], t[2], t[3], t[4], t[5]) for t in sb]   # σ, η, ω, rank per major iteration
    assert a["r"] == b["r"] == 32
    for res in (a, b):   # both stopped by the gap test, not by a limit
        assert res["primal_vio"] <= 1e-2 and res["min_duality_gap"] <= 1e-2
    assert abs(a["obj"] - b["obj"]) <= 1e-2 * abs(b["obj"])
    assert abs(a["max_dual_value"] - b["max_dual_value"]) <= 1e-2 * abs(b["max_dual_value"])
    ia, ib = a["iter"], b["iter"]
    assert abs(ia - ib) <= 0.25 * max(ia, ib), (ia, ib)


def test_schedule_parity_at_baseline_size_minimum_bisection(hip_abi):
    """MinBisection n = 1e5, r = 32: the landscape is flat, the inner loops stop on a coarse gradient test, and the count of
    inner iterations per major iteration — with it the later σ decisions — is sensitive to round-off (on the same inputs:
    HIP 16–19 major iterations to convergence, the OpenMP oracle 30; until its dot product was made to add the threads' sums
    in thread order the OpenMP oracle even differed from itself run to run).  The comparison with the oracle therefore covers the first four major iterations — identical σ/η/ω/rank
    schedule, objectives within 10 % of each other — and the full solve is checked on its own terms: stop by the gap test
    within the reference's tolerances (src/sdplr.jl:335-345)."""
    n = 100_000
    data = problems.minimum_bisection_data(problems.gnp_graph(n, 2e-4, 4))
    kw = dict(r=32, ptol=1e-2, objtol=1e-2, seed=0, prior_trace_bound=float(n), printlevel=0)
    a = sj.sdplr(data=data, abi=hip_abi, maxmajoriter=4, **kw)
    b = sj.sdplr(data=data, abi=_omp_oracle(), maxmajoriter=4, **kw)
    sa, sb = a["schedule"], b["schedule"]
    assert len(sa) == len(sb) == 4
    assert [(t[0], t[2], t[3], t[4], t[5]) for t in sa] == [(t[0], t[2], t[3], t[4], t[5]) for t in sb]
    assert sa[0][1] == sb[0][1] and sa[1][1] == sb[1][1]          # the first inner loops (12 and 0 iterations) are still in step
    assert a["obj"] == pytest.approx(b["obj"], rel=0.1)
    full = sj.sdplr(data=data, abi=hip_abi, **kw)
    assert full["primal_vio"] <= 1e-2 and full["min_duality_gap"] <= 1e-2 and full["majoriter"] < 100


@pytest.mark.parametrize("which", ["maxcut_n1e5", "minbis_n1e5"])
def test_ring_form_of_the_history_is_bitwise_the_stored_form_at_baseline_size(hip_abi, monkeypatch, which):
    """The loop keeps lbfgshis.vecs[j].s / .y (src/lbfgs.jl:4-12) as (α_j, dir_j) and (G_j, G_{j+1}) (csrc/k_dense.h, "ring
    form"; tests/test_gpu_ring.py on small instances): at the north-star size — full grids, hipGraph batches, the ring wrapped
    five times — R, G, every s_j and y_j after 3 + 22 iterations equal the stored-form run (SDPLR_HIP_NO_RING) bit for bit."""
    data, seed = _instance(which)
    r, h = 32, 4
    normC, normb = data.normC(), float(np.linalg.norm(data.b))
    got = {}
    for ring in (True, False):
        if ring:
            monkeypatch.delenv("SDPLR_HIP_NO_RING", raising=False)
        else:
            monkeypatch.setenv("SDPLR_HIP_NO_RING", "1")
        s, _ = make_solver(hip_abi, data, r, seed=seed, h=h)
        st = s.fg(normC, normb)
        o1 = s.inner_loop(normC, normb, True, True, False, 0.0, -1e300, 3, 0.0, *st)
        o2 = s.inner_loop(normC, normb, True, True, False, 0.0, -1e300, 22, 0.0, *o1[:3])
        assert s.stats()["ring_history_loops"] == (2 if ring else 0)
        got[ring] = (o1, o2, s.Rt, s.Gt, [s.get_factor(cabi.F_LBFGS_S + j) for j in range(h)],
                     [s.get_factor(cabi.F_LBFGS_Y + j) for j in range(h)], s.get_factor(cabi.F_DIRT))
        s.close()
    a, b = got[True], got[False]
    assert a[0] == b[0] and a[1] == b[1]
    assert np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3]) and np.array_equal(a[6], b[6])
    for j in range(h):
        assert np.array_equal(a[4][j], b[4][j]) and np.array_equal(a[5][j], b[5][j]), j
