"""sdplr_hip_batch_round (include/sdplr_hip_round_batch.h, k_round_batch.h) on the device: one call rounds a whole batch of
handles that differ in n, r, graph, trial count and mode.  The bar: every item bit-identical to the numpy restatement of
the definitions (tests/round_reference.py) and — for real weights, where the summation order shows — to sdplr_hip_round
on the same handle; errors stay per item; the route rule; the call reads solver state and writes none; and the whole
path through ``batch.solve_lockstep(rounding=…)``."""
import os

import numpy as np
import pytest

import sdplrplus_jl_amd as sj
from sdplrplus_jl_amd import batch, cabi, problems, rounding

from helpers import make_data, make_solver
import round_reference as ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the (n, r, T, E) of tests/test_gpu_round.py's CASES, now mixed inside one call
CASES = [
    (1, 1, 1, 0), (1, 3, 65, 1), (2, 2, 63, 1), (2, 33, 64, 0),
    (63, 1, 64, 255), (64, 3, 65, 256), (65, 10, 63, 257), (64, 32, 100, 1), (63, 33, 130, 256),
    (257, 2, 130, 3000), (257, 32, 1, 255), (257, 33, 64, 257),
    (1000, 10, 100, 5000), (1000, 33, 65, 0), (1000, 3, 130, 4000), (1000, 32, 63, 1),
]


def handle(hip_abi, n, r, h=0):
    """A finalized handle with n rows at rank r (MaxCut on a path): the rounding reads nothing of it but the factor slot."""
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
    """The recipe of tests/test_gpu_round.py: a Gaussian factor with zero rows and a row of −0.0 (±0.0 label +1 and tie in
    index order) and — dup — more than half the rows bitwise equal, so that equal keys straddle the ⌊n/2⌋ threshold."""
    R = rng.standard_normal((n, r))
    if dup and n >= 16:
        idx = rng.permutation(n)[: n // 2 + 8]
        R[idx] = R[idx[0]]
    if n >= 3:
        R[n // 3] = 0.0
        R[n - 1] = -0.0
    if n >= 9:
        R[[1, n // 2, n - 2]] = 0.0
    return R


def assert_item(got, want, route=None):
    cuts, best, xb, lab, rt = got
    assert np.array_equal(lab, want["labels"]), np.argwhere(lab != want["labels"])[:5]
    assert np.array_equal(cuts, want["cuts"]), (cuts[:4], want["cuts"][:4])
    assert best == want["best"] and np.array_equal(xb, want["x_best"])
    if route is not None:
        assert rt == route


_MIX = {}


def _mix(hip_abi):
    """Sixteen live handles, one per case, half in each mode (bisection items on duplicated rows), with the comparator's
    answer — computed once and shared by the tests below, which leave the handles as they are."""
    if not _MIX:
        items = []
        for k, (n, r, T, E) in enumerate(CASES):
            rng = np.random.Generator(np.random.PCG64(9000 + 31 * n + 7 * r + T))
            mode = k % 2
            A = ref.random_graph(n, E, rng)
            R = special_factor(n, r, rng, dup=(mode == 1 and k % 4 == 1))
            gauss = rng.standard_normal((T, r))
            s = handle(hip_abi, n, r)
            s.round_set_graph(A)
            s.set_factor(cabi.F_RT, R)
            items.append(dict(s=s, mode=mode, T=T, gauss=gauss, want=ref.rounding(R, gauss, A, mode)))
        _MIX["items"] = items
    return _MIX["items"]


def _call(hip_abi, items):
    return cabi.batch_round(hip_abi, [q["s"] for q in items], [(q["mode"], q["T"], q["gauss"], cabi.F_RT, True, True) for q in items])


def test_mixed_batch_is_exact_in_one_shared_launch(hip_abi):
    items = _mix(hip_abi)
    assert sorted(q["mode"] for q in items) == [0] * 8 + [1] * 8
    for q, got in zip(items, _call(hip_abi, items)):
        assert_item(got, q["want"], route=1)
        if q["mode"] == 1:
            n = got[3].shape[1]
            assert np.all(got[3].astype(np.int64).sum(axis=1) == 2 * (n // 2) - n)


def test_route_rule(hip_abi, monkeypatch):
    """SDPLR_HIP_BATCH_ROUND_NMAX between two of the call's n: above it sdplr_hip_round serves, below it the shared launch;
    SDPLR_HIP_NO_BATCH_ROUND=1: sdplr_hip_round serves everything.  The bits do not depend on the route."""
    items = _mix(hip_abi)
    monkeypatch.setenv("SDPLR_HIP_BATCH_ROUND_NMAX", "100")
    for q, got in zip(items, _call(hip_abi, items)):
        assert_item(got, q["want"], route=1 if q["s"].n <= 100 else 0)
    monkeypatch.delenv("SDPLR_HIP_BATCH_ROUND_NMAX")
    monkeypatch.setenv("SDPLR_HIP_NO_BATCH_ROUND", "1")
    for q, got in zip(items, _call(hip_abi, items)):
        assert_item(got, q["want"], route=0)
    # per-kernel profiling on one handle: that item alone leaves the shared launch
    monkeypatch.delenv("SDPLR_HIP_NO_BATCH_ROUND")
    items[5]["s"].profile_enable(True)
    res = _call(hip_abi, items[4:8])
    items[5]["s"].profile_enable(False)
    assert [x[4] for x in res] == [1, 0, 1, 1]
    for q, got in zip(items[4:8], res):
        assert_item(got, q["want"])


def test_count_one_count_zero_and_two_calls(hip_abi):
    items = _mix(hip_abi)
    assert cabi.batch_round(hip_abi, [], []) == []
    assert hip_abi.batch_round(0, None) == cabi.OK
    for k in (0, 9, 12):
        (got,) = _call(hip_abi, [items[k]])
        assert_item(got, items[k]["want"], route=1)
    a, b = _call(hip_abi, items[8:14]), _call(hip_abi, items[8:14])
    for x, y in zip(a, b):
        assert x[1] == y[1] and x[4] == y[4] and all(np.array_equal(p, q) for p, q in zip((x[0],) + x[2:4], (y[0],) + y[2:4]))


@pytest.mark.parametrize("mode", [0, 1])
def test_batch_equals_single_for_real_weights(hip_abi, mode):
    """The summation-order contract: with uniform weights in (0, 1) the batch call's cuts are the bits of sdplr_hip_round on
    the same handle (E = 5000: five scoring blocks, so block order, wave order and the group stride all matter; E = 3000:
    three, an odd count for the two-blocks-per-round fold)."""
    hs, reqs, wants, singles = [], [], [], []
    for n, r, T, E in ((1000, 10, 100, 5000), (257, 33, 130, 3000)):
        rng = np.random.Generator(np.random.PCG64(515 + mode + n))
        A = ref.random_graph(n, E, rng, weights="real")
        R = special_factor(n, r, rng)
        gauss = rng.standard_normal((T, r))
        s = handle(hip_abi, n, r)
        s.round_set_graph(A)
        s.set_factor(cabi.F_RT, R)
        hs.append(s)
        reqs.append((mode, T, gauss, cabi.F_RT, True, True))
        wants.append(ref.rounding(R, gauss, A, mode))
        singles.append(s.round(mode, T, gauss, want_best=True, want_labels=True))
    res = cabi.batch_round(hip_abi, hs, reqs)
    for s in hs:
        s.close()
    for got, one, want in zip(res, singles, wants):
        assert got[4] == 1
        assert np.array_equal(got[0], one[0]), np.abs(got[0] - one[0]).max()
        assert got[1] == one[1] and np.array_equal(got[2], one[2]) and np.array_equal(got[3], one[3])
        assert np.array_equal(got[3], want["labels"])


def test_ranks_differ_after_reset_rank(hip_abi):
    n, r, T = 300, 4, 70
    rng = np.random.Generator(np.random.PCG64(78))
    A = ref.random_graph(n, 900, rng)
    hs = [handle(hip_abi, n, r, h=4) for _ in range(3)]
    for s in hs:
        s.round_set_graph(A)                 # (the graph survives reset_rank)
    hs[1].reset_rank(2 * r)
    hs[2].reset_rank(3 * r + 1)
    reqs, wants = [], []
    for k, s in enumerate(hs):
        R, gauss = rng.standard_normal((n, s.r)), rng.standard_normal((T, s.r))
        s.set_factor(cabi.F_RT, R)
        reqs.append((k % 2, T, gauss, cabi.F_RT, True, True))
        wants.append(ref.rounding(R, gauss, A, k % 2))
    assert [s.r for s in hs] == [4, 8, 13]
    res = cabi.batch_round(hip_abi, hs, reqs)
    # a scratch slot of one handle beside R of the others
    Q = rng.standard_normal((n, hs[0].r))
    hs[0].set_factor(cabi.F_SCRATCH, Q)
    res2 = cabi.batch_round(hip_abi, hs, [reqs[0][:3] + (cabi.F_SCRATCH, True, True)] + reqs[1:])
    for s in hs:
        s.close()
    for got, want in zip(res, wants):
        assert_item(got, want, route=1)
    assert_item(res2[0], ref.rounding(Q, reqs[0][2], A, 0), route=1)
    assert_item(res2[1], wants[1], route=1)


def test_errors_stay_per_item(hip_abi):
    n, r, T = 120, 5, 70
    rng = np.random.Generator(np.random.PCG64(79))
    A = ref.random_graph(n, 400, rng)
    hs = [handle(hip_abi, n, r) for _ in range(4)]
    Rs = [rng.standard_normal((n, r)) for _ in hs]
    gauss = rng.standard_normal((T, r))
    for k, s in enumerate(hs):
        if k != 1:
            s.round_set_graph(A)             # handle 1: no graph
        s.set_factor(cabi.F_RT, Rs[k])
    modes = [0, 1, 2, 1]                     # item 2: a bad mode
    arr = (cabi.RoundItem * 4)()
    cuts = [np.full(T, -7.0) for _ in hs]
    for k, s in enumerate(hs):
        arr[k].s, arr[k].mode, arr[k].slot, arr[k].trials = s._h.value, modes[k], cabi.F_RT, T
        arr[k].gauss, arr[k].cuts, arr[k].best = cabi._pd(gauss), cabi._pd(cuts[k]), -1
    assert hip_abi.batch_round(4, arr) == cabi.ERR_STATE          # the first non-zero status
    assert [arr[k].status for k in range(4)] == [cabi.OK, cabi.ERR_STATE, cabi.ERR_INVALID_ARG, cabi.OK]
    assert arr[0].route == 1 and arr[3].route == 1
    for k in (0, 3):
        want = ref.rounding(Rs[k], gauss, A, modes[k])
        assert np.array_equal(cuts[k], want["cuts"]) and arr[k].best == want["best"]
    assert np.all(cuts[1] == -7.0) and np.all(cuts[2] == -7.0)
    # the Python wrapper hands each item its own exception
    res = cabi.batch_round(hip_abi, hs, [(m, T, gauss) for m in modes])
    assert isinstance(res[1], sj.SdplrError) and res[1].code == cabi.ERR_STATE
    assert isinstance(res[2], sj.SdplrError) and res[2].code == cabi.ERR_INVALID_ARG
    assert np.array_equal(res[0][0], cuts[0]) and np.array_equal(res[3][0], cuts[3])
    # other per-item refusals: trial count, slot
    res = cabi.batch_round(hip_abi, [hs[0], hs[3]], [(0, 0, np.zeros((0, r))), (1, T, gauss, 7)])
    assert [x.code for x in res] == [cabi.ERR_INVALID_ARG, cabi.ERR_INVALID_ARG]
    # a duplicated handle fails the whole call, and nothing is written
    for k in (0, 3):
        cuts[k][:] = -7.0
        arr[k].best, arr[k].status, arr[k].route = -1, 55, 55
    arr[3].s = hs[0]._h.value
    assert hip_abi.batch_round(4, arr) == cabi.ERR_INVALID_ARG
    assert b"twice" in hip_abi.last_error(None)
    assert all(np.all(c == -7.0) for c in cuts)
    assert [(arr[k].best, arr[k].status, arr[k].route) for k in (0, 3)] == [(-1, 55, 55)] * 2
    with pytest.raises(sj.SdplrError) as e:
        cabi.batch_round(hip_abi, [hs[0], hs[0]], [(0, T, gauss)] * 2)
    assert e.value.code == cabi.ERR_INVALID_ARG
    for s in hs:
        s.close()


def test_batch_round_reads_state_and_writes_none(hip_abi, monkeypatch):
    """Four resident-route MaxCut instances (n = 64, r = 4): major iteration → batch_round (twice: same bits) → major
    iteration equals the same sequence without the rounding — R, G, λ, the scalars and the counters."""
    monkeypatch.delenv("SDPLR_HIP_FORCE_GRAPH", raising=False)
    monkeypatch.delenv("SDPLR_HIP_NO_RESIDENT", raising=False)
    datas = [make_data("maxcut", 11 + k, 64, 0.2)[0] for k in range(4)]
    norms = [(d.normC(), float(np.linalg.norm(d.b))) for d in datas]
    rng = np.random.Generator(np.random.PCG64(62))
    graphs = [ref.random_graph(64, 300, rng) for _ in datas]
    gauss = [rng.standard_normal((70, 4)) for _ in datas]

    def run(with_round):
        hs = [make_solver(hip_abi, d, 4, seed=5, h=4)[0] for d in datas]
        args = lambda upd: [(nc, nb, 1, 1, 0, upd, 2.0, 0.0, -1e300, 6, 0.0) for nc, nb in norms]
        out1 = cabi.batch_major_iteration(hip_abi, hs, args(0))
        if with_round:
            for s, A in zip(hs, graphs):
                s.round_set_graph(A)
            Rs = [s.Rt.copy() for s in hs]
            reqs = [(k % 2, 70, gauss[k], cabi.F_RT, True, True) for k in range(4)]
            a, b = cabi.batch_round(hip_abi, hs, reqs), cabi.batch_round(hip_abi, hs, reqs)
            for k in range(4):
                assert_item(a[k], ref.rounding(Rs[k], gauss[k], graphs[k], k % 2), route=1)
                assert a[k][1] == b[k][1] and all(np.array_equal(p, q) for p, q in zip((a[k][0],) + a[k][2:4], (b[k][0],) + b[k][2:4]))
        out2 = cabi.batch_major_iteration(hip_abi, hs, args(1))
        state = [dict(R=s.Rt.copy(), G=s.Gt.copy(), lam=s.λ.copy(), obj=s.obj, sigma=s.σ, stats=s.stats()) for s in hs]
        for s in hs:
            s.close()
        return out1, out2, state

    p1, p2, plain = run(False)
    r1, r2, rounded = run(True)
    assert p1 == r1 and p2 == r2
    for a, b in zip(plain, rounded):
        for k in ("R", "G", "lam"):
            assert np.array_equal(a[k], b[k]), k
        assert a["obj"] == b["obj"] and a["sigma"] == b["sigma"]
        assert a["stats"] == b["stats"]
        assert a["stats"]["resident_loops"] == 2


def test_solve_lockstep_with_rounding(hip_abi, monkeypatch):
    """Four Gset fixtures (two as MaxCut, two as MinimumBisection, r = 10) through solve_lockstep with the rounding on: the
    solves are those of rounding=None bit for bit, and callback_res is what the *_rounding_device callback returns on a
    one-by-one solve with the same seed."""
    monkeypatch.delenv("SDPLR_HIP_FORCE_GRAPH", raising=False)
    monkeypatch.delenv("SDPLR_HIP_NO_RESIDENT", raising=False)
    z = np.load(os.path.join(ROOT, "tests", "golden", "gset_G1_G9.npz"))
    graphs = [problems.graph_from_edges(int(z[f"{g}_n"]), z[g]) for g in ("G1", "G2", "G3", "G4")]
    kinds = ["maxcut", "maxcut", "bisection", "bisection"]
    datas = [(problems.maxcut_data if k == "maxcut" else problems.minimum_bisection_data)(A) for k, A in zip(kinds, graphs)]
    kw = dict(ptol=1e-2, objtol=1e-2, maxtime=120.0, printlevel=0, prior_trace_bound=800.0, seed=0)
    mk = lambda k: np.random.Generator(np.random.PCG64(100 + k))
    plain = batch.solve_lockstep(datas, 10, abi=hip_abi, **kw)
    assert all("callback_res" not in x and "callback_time" not in x for x in plain)
    got = batch.solve_lockstep(datas, 10, abi=hip_abi, rounding=[(kinds[k], graphs[k], mk(k)) for k in range(4)], **kw)
    for k in range(4):
        a, b = plain[k], got[k]
        assert a["obj"] == b["obj"] and a["iter"] == b["iter"] and a["majoriter"] == b["majoriter"]
        assert np.array_equal(a["Rt"], b["Rt"]) and np.array_equal(a["lambda"], b["lambda"])
        assert set(b) == set(a) | {"callback_res", "callback_time"} and b["callback_time"] >= 0.0
        fn = rounding.maxcut_rounding_device if kinds[k] == "maxcut" else rounding.minimumbisection_rounding_device
        g = mk(k)
        one = sj.sdplr(data=datas[k], r=10, abi=hip_abi, callback=lambda var, d, k=k, g=g: fn(var, graphs[k], g), **kw)
        assert np.array_equal(one["Rt"], b["Rt"])
        assert b["callback_res"] == one["callback_res"], (k, b["callback_res"], one["callback_res"])
    # the callbacks' answers through the batch helper's loop (A/B switch) are the same numbers
    hs = [handle(hip_abi, 800, 10) for _ in range(2)]
    for s, x in zip(hs, got[1:3]):
        s.set_factor(cabi.F_RT, x["Rt"])
    routes = []
    both = rounding.batch_rounding_device(hs, graphs[1:3], [mk(1), mk(2)], kinds[1:3], routes=routes)
    loop = rounding.batch_rounding_device(hs, graphs[1:3], [mk(1), mk(2)], kinds[1:3], loop=True)
    for s in hs:
        s.close()
    assert routes == [1, 1] and both == loop == [got[1]["callback_res"], got[2]["callback_res"]]


def test_batch_round_example_runs_from_plain_c(tmp_path, hip_abi):
    import re
    import shutil
    import subprocess
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    ldir = os.path.join(ROOT, "sdplrplus.jl_amd", "lib")
    exe = tmp_path / "batch_round_hip"
    subprocess.check_call(["gcc", "-O2", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "batch_round_c_abi.c"),
                           "-L", ldir, "-lsdplr_hip", "-lm", f"-Wl,-rpath,{ldir}", "-Wl,-rpath-link,/opt/rocm/lib", "-o", str(exe)])
    out = subprocess.run([str(exe), "5", "6", "70"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip().endswith("OK")
    rows = re.findall(r"best cut = (\S+) \(trial (\d+)\)  route = (\d)", out.stdout)
    assert len(rows) == 5 and all(rt == "1" for _, _, rt in rows), out.stdout


def test_close_the_shared_handles(hip_abi):
    """(last in the file: the handles of _mix are released)"""
    for q in _MIX.pop("items", []):
        q["s"].close()
