"""The sizes, states and checks shared by tests/test_armijo_reference.py (the CPU oracle) and tests/test_gpu_armijo.py (the HIP
library): linesearch_armijo(α_max) on states set through the ABI, against helpers.armijo_hp.

A size is (n, m, r).  The row counts m are the edges of the Armijo kernels' layout: 1, 2, 63, 64, 65 (wave and block tails),
255, 256, 257 (the grid of m + 1 rows going from one block to two; at m = 256 the commit's second block holds the objective's
row alone), 511, 513, 1025 (several blocks) and 65 600 (the grid capped at 256 blocks, every thread striding a second time).

ARMIJO_T records per size the (α_max, log₂ t) of its descent states D = fl(t·(−G)), picked on the CPU from a sweep of t over
2⁻¹² … 2¹² so that the reference's accepted step k_hp hits 0, 1, a middle value and ≥ 20 with every state decided
(tests/test_armijo_reference.py asserts it)."""
import numpy as np

from helpers import armijo_base, armijo_state, check_armijo_call, make_solver

SIZES = [(12, 1, 3), (16, 2, 3), (16, 63, 3), (16, 64, 33), (16, 65, 1), (24, 255, 3), (24, 256, 1), (24, 257, 33), (48, 511, 3),
         (48, 513, 1), (48, 1025, 33), (363, 65600, 2)]
ARMIJO_T = {
    (12, 1, 3): [(1e-3, -12), (1e-3, 4), (1e-3, 8), (1.0, -12), (1.0, -6), (1.0, -5), (1.0, 2), (1.0, 12), (4.0, -6), (4.0, 4), (4.0, 11)],
    (16, 2, 3): [(1e-3, -12), (1e-3, 1), (1e-3, 4), (1.0, -12), (1.0, -9.5), (1.0, -9), (1.0, -2), (1.0, 9), (4.0, -10), (4.0, 0), (4.0, 7)],
    (16, 63, 3): [(1e-3, -12), (1e-3, -1), (1e-3, 3), (1.0, -12), (1.0, -11), (1.0, -10), (1.0, -3), (1.0, 8), (4.0, -11), (4.0, -1), (4.0, 6)],
    (16, 64, 33): [(1e-3, -12), (1e-3, -3), (1e-3, 1), (1.0, -12), (1.0, -5), (1.0, 6), (4.0, -12), (4.0, -3), (4.0, 4)],
    (16, 65, 1): [(1e-3, -12), (1e-3, 2), (1e-3, 6), (1.0, -12), (1.0, -8), (1.0, -7), (1.0, 0), (1.0, 11), (4.0, -8), (4.0, 2), (4.0, 9)],
    (24, 255, 3): [(1e-3, -12), (1e-3, -1), (1e-3, 3), (1.0, -12), (1.0, -11), (1.0, -9), (1.0, -3), (1.0, 8), (4.0, -11), (4.0, -1), (4.0, 6)],
    (24, 256, 1): [(1e-3, -12), (1e-3, -1), (1e-3, 3), (1.0, -12), (1.0, -11), (1.0, -10), (1.0, -3), (1.0, 8), (4.0, -11), (4.0, -1), (4.0, 6)],
    (24, 257, 33): [(1e-3, -12), (1e-3, -3), (1e-3, 1), (1.0, -12), (1.0, -5), (1.0, 6), (4.0, -12), (4.0, -3), (4.0, 4)],
    (48, 511, 3): [(1e-3, -12), (1e-3, -2), (1e-3, 2), (1.0, -12), (1.0, -11), (1.0, -4), (1.0, 7), (4.0, -12), (4.0, -2), (4.0, 5)],
    (48, 513, 1): [(1e-3, -12), (1e-3, -1), (1e-3, 3), (1.0, -12), (1.0, -11), (1.0, -10), (1.0, -3), (1.0, 8), (4.0, -11), (4.0, -1), (4.0, 6)],
    (48, 1025, 33): [(1e-3, -12), (1e-3, -4), (1e-3, 0), (1.0, -12), (1.0, -6), (1.0, 5), (4.0, -12), (4.0, -4), (4.0, 3)],
    (363, 65600, 2): [(1e-3, -12), (1e-3, -4), (1.0, -6), (1.0, 6), (4.0, -12)],
}
RATIOS = ("A_RD", "A_DD", "L", "commit")
EXACT = ("on_grid", "decision_ok", "alpha_exact", "obj_is_last", "pv_is_raw")
_STATES = {}


def states(size) -> list:
    """[(tag, state)] of one size: its descent states, built once."""
    if size not in _STATES:
        base = armijo_base(*size)
        _STATES[size] = [(f"amax={amax:g} t=2^{e:g}", armijo_state(base, 2.0 ** e, amax)) for amax, e in ARMIJO_T[size]]
    return _STATES[size]


def run_size(abi, size) -> dict:
    """check_armijo_call on every descent state of the size on a fresh handle of the library behind `abi` → the worst
    error/bound per quantity, the failures as text, the depths reached and the undecided states."""
    base = armijo_base(*size)
    s_, _ = make_solver(abi, base["data"], size[2], seed=5, h=4)
    worst = {k: 0.0 for k in RATIOS}
    bad, depths, undecided = [], [], []
    for tag, st in states(size):
        res = check_armijo_call(base, st, s_)
        depths.append(res["k_dev"])
        if not res["decided"]:
            undecided.append(tag)
        for k in RATIOS:
            worst[k] = max(worst[k], res[k])
            if not res[k] <= 1.0:
                bad.append((tag, k, res[k]))
        for k in EXACT:
            if not res[k]:
                bad.append((tag, k, res["k_dev"], res["k_hp"], res["alpha"]))
    s_.close()
    return dict(worst=worst, bad=bad, depths=depths, undecided=undecided, n=len(depths))


def report(lib, size, out):
    print(f"armijo {lib} n={size[0]} m={size[1]} r={size[2]}: error/bound " + " ".join(f"{k} {v:.3g}" for k, v in out["worst"].items())
          + f"  depths {out['depths']}  undecided {len(out['undecided'])}/{out['n']}")
