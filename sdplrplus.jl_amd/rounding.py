"""Randomized rounding callbacks of the reference's experiment runner (exps/test.jl:67-105): they turn the factor R of an
SDP solution into a cut / a bisection.  Host-side post-processing of one downloaded n×r factor (100 GEMVs), not part
of the device path.  The ``*_device`` twins below run the same roundings behind the C ABI on the factor where it lies
(include/sdplr_hip_round.h): nothing factor-sized is downloaded."""
from __future__ import annotations

import numpy as np

from . import problems


def eval_cut(L, x) -> float:
    """Cut value ¼·xᵀLx of a ±1 labelling (exps/test.jl:67-69)."""
    return 0.25 * float(x @ (L @ x))


def maxcut_rounding(A, R: np.ndarray, rng: np.random.Generator, trials: int = 100) -> float:
    """Goemans–Williamson hyperplane rounding, best of `trials` (exps/test.jl:71-81).  R is n×r."""
    L = problems._laplacian(A, 1.0)
    best = -np.inf
    for _ in range(trials):
        x = np.sign(R @ rng.standard_normal(R.shape[1]))
        x[x == 0] = 1.0
        best = max(best, eval_cut(L, x))
    return best


def minimumbisection_rounding(A, R: np.ndarray, rng: np.random.Generator, trials: int = 100) -> float:
    """Sort a random projection and split it in halves, best of `trials` (exps/test.jl:83-98)."""
    L = problems._laplacian(A, 1.0)
    n = R.shape[0]
    best = np.inf
    for _ in range(trials):
        perm = np.argsort(R @ rng.standard_normal(R.shape[1]), kind="stable")
        part = np.zeros(n)
        part[perm] = np.where((np.arange(1, n + 1) * 2) <= n, 1.0, -1.0)
        best = min(best, eval_cut(L, part))
    return best


def _gauss(rng: np.random.Generator, trials: int, r: int) -> np.ndarray:
    gauss = np.empty((trials, r))
    for t in range(trials):                  # one draw per trial, as the host callbacks consume the generator
        gauss[t] = rng.standard_normal(r)
    return gauss


def _round_device(var, A, rng: np.random.Generator, trials: int, mode: int) -> float:
    from . import cabi
    if trials > cabi.ROUND_MAX_TRIALS:
        raise ValueError(f"at most {cabi.ROUND_MAX_TRIALS} trials per call")
    var.round_set_graph(A)
    cuts, best, _, _ = var.round(mode, trials, _gauss(rng, trials, var.r))
    return float(cuts[best])


def maxcut_rounding_device(var, A, rng: np.random.Generator, trials: int = 100) -> float:
    """``maxcut_rounding`` on the device, on the factor R of the live handle ``var`` (a ``DeviceSolver``): same draws from
    ``rng``, same return value up to the summation order of the projection."""
    return _round_device(var, A, rng, trials, 0)


def minimumbisection_rounding_device(var, A, rng: np.random.Generator, trials: int = 100) -> float:
    """``minimumbisection_rounding`` on the device, on the factor R of the live handle ``var``."""
    return _round_device(var, A, rng, trials, 1)


ROUNDING_MODES = {"maxcut": 0, "bisection": 1}


def batch_rounding_device(vars, As, rngs, mode, trials: int = 100, abi=None, routes=None, loop: bool = False) -> list:
    """The ``*_device`` callbacks for a whole batch of live handles in ONE library call (include/sdplr_hip_round_batch.h):
    ``vars[k]`` is rounded on graph ``As[k]`` with the draws of ``rngs[k]``; ``mode`` is "maxcut" | "bisection" (or 0 | 1), one
    for all or one per instance.  Each graph is uploaded once, each instance takes the draws its own callback would take.
    → the best cut per instance, bit for bit what ``maxcut_rounding_device`` / ``minimumbisection_rounding_device`` return
    (an instance whose item failed: its exception).  ``routes``: a list that receives what served each item (1: the shared
    launch, 0: the single-instance call).  ``loop=True`` makes the calls one by one instead (A/B runs)."""
    from . import cabi
    vars = list(vars)
    if trials > cabi.ROUND_MAX_TRIALS:
        raise ValueError(f"at most {cabi.ROUND_MAX_TRIALS} trials per call")
    modes = [mode] * len(vars) if isinstance(mode, (str, int)) else list(mode)
    modes = [ROUNDING_MODES[m] if isinstance(m, str) else int(m) for m in modes]
    if not (len(vars) == len(As) == len(rngs) == len(modes)):
        raise ValueError("vars, As, rngs (and mode, when it is a sequence) must have the same length")
    if not vars:
        return []
    reqs = []
    for v, A, rng, m in zip(vars, As, rngs, modes):
        v.round_set_graph(A)
        reqs.append((m, trials, _gauss(rng, trials, v.r)))
    if loop:
        if routes is not None:
            routes[:] = [0] * len(vars)
        out = []
        for v, q in zip(vars, reqs):
            cuts, best, _, _ = v.round(*q)
            out.append(float(cuts[best]))
        return out
    res = cabi.batch_round(abi if abi is not None else vars[0].abi, vars, reqs)
    if routes is not None:
        routes[:] = [None if isinstance(x, Exception) else x[4] for x in res]
    return [x if isinstance(x, Exception) else float(x[0][x[1]]) for x in res]
