"""f! (𝒜(RRᵀ) − b, objective, ℒ), g! (y, S, G = 2·S·R), fg! on its fused routes, the two-argument 𝒜 (modes 1 and 2) and both
orientations of 𝒜ᵀ of the HIP library against references above FP64 (helpers.fg_hp, S_and_G_hp, A_pair_hp), at the edges of
the device layout: the segmented reduction's thresholds, every sub-wave rank shape and rows of more than 128 doubles, the fast
fg! and its tile heights, hub rows, low-rank terms up to and beyond SDPLR_LRMAX and the k_lr_reduce split (n·r = 2²²),
inequalities on both sides of the cap, the resident k_rs_fg at its register window, and every family.  Every element of every
output is held to error/bound ≤ 1 with the derived bounds of helpers.py; each stage is checked from the handle's own output of
the stage before it.  The cases, inputs and checks are fg_cases.py's and run unchanged on the CPU oracle in
tests/test_fg_reference.py.  Each case asserts the form that ran: stats()["resident_fg"], and for the launch forms the scope
names a twin handle under profile_enable() reports (profiling closes the resident route: hence a twin)."""
import numpy as np
import pytest

import fg_cases as fc

pytestmark = pytest.mark.gpu

FAST = {"spmm_P", "fg_tail", "fg_G"}


def _twin_scopes(hip_abi, name, r):
    bc = fc.built(name)
    t = fc.new_handle(hip_abi, bc["data"], r)
    t.profile_enable()
    fc._load(t, fc.case_inputs(name, r)[0])
    t.fg(3.0, 2.0, True, True)
    names = set(t.profile())
    t.close()
    return names


@pytest.mark.parametrize("name,r", [(n, r) for n, c in fc.CASES.items() for r in c["ranks"]])
def test_fg_operators(hip_abi, monkeypatch, name, r):
    case = fc.CASES[name]
    for k in fc.TOGGLES:
        monkeypatch.delenv(k, raising=False)
    if case["launches"]:
        monkeypatch.setenv("SDPLR_HIP_FORCE_GRAPH", "1")
    else:
        monkeypatch.delenv("SDPLR_HIP_FORCE_GRAPH", raising=False)
    for k, v in case["env"].items():
        monkeypatch.setenv(k, v)
    worst, carve, stats, n_fg = fc.run_case(hip_abi, name, r, hip=True)
    fc.report("hip", name, r, worst, carve)
    # ---- the form that ran ----
    if case["form"] == "resident":
        assert stats["resident_fg"] == n_fg, (name, r, stats)
    else:
        assert stats["resident_fg"] == 0, (name, r, stats)
        names = _twin_scopes(hip_abi, name, r)
        if case["form"] == "fast":
            assert FAST <= names and "sddmm_uu" not in names, (name, r, sorted(names))
        elif case["form"] == "generic":
            assert not (FAST & names) and "spmm" in names and set(case["scopes"]) <= names, (name, r, sorted(names))
            assert ("lr_reduce" in names) == (name == "lowrank_big"), (name, sorted(names))
        else:   # "launch": the resident route refused (its LDS budget), whichever launch form the instance then takes
            assert FAST <= names or "spmm" in names, (name, r, sorted(names))
    if case["hubs"]:
        p = fc.built(name)["pattern"]
        rows = np.bincount(p["f_col"], minlength=p["n"])
        at_least, thresh = case["hubs"]
        thresh = thresh if thresh is not None else max(64, 3 * p["nnzS"] // p["n"])
        assert np.sum(rows > thresh) >= at_least and np.sum(rows <= thresh) > 0, (name, int(np.sum(rows > thresh)))
    fc.assert_case(name, r, worst, carve)
