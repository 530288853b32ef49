"""CPU-side checks of the rounding extension of the C ABI (include/sdplr_hip_round.h): the header is exactly
``cabi.ROUND_SIGNATURES``, the cross-compiled library exports both entry points, the CPU checker's ABI — which has no
rounding — still loads, nothing computes without a device, and ``sdplr(..., callback=f)`` hands f a live handle."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import sdplrplus_jl_amd as sj
from sdplrplus_jl_amd import cabi, problems

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "sdplr_hip_round.h")


def header_functions(path, prefix):
    """name → argument count of every function the header declares (comments stripped first)."""
    txt = open(path).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    out = {}
    for m in re.finditer(r"\b(?:int32_t|const char\*|void)\s+" + prefix + r"(\w+)\s*\(([^;]*?)\)\s*;", txt, flags=re.S):
        args = [a.strip() for a in m.group(2).replace("\n", " ").split(",")]
        args = [] if args in ([""], ["void"]) else args
        out[m.group(1)] = args
    return out


_CTYPE = {"sdplr_hip_solver*": cabi._vp, "int32_t": cabi._i32, "int64_t": cabi._i64, "const int64_t*": cabi._pi64,
          "int64_t*": cabi._pi64, "const double*": cabi._pf64, "double*": cabi._pf64, "int8_t*": cabi._pi8}


def test_round_header_is_the_round_signature_table():
    decl = header_functions(HEADER, "sdplr_hip_")
    assert set(decl) == set(cabi.ROUND_SIGNATURES), set(decl) ^ set(cabi.ROUND_SIGNATURES)
    for name, args in decl.items():
        types = [_CTYPE[a.rsplit(" ", 1)[0].strip()] for a in args]      # "const double* gauss" → "const double*"
        assert types == cabi.ROUND_SIGNATURES[name], name
    # an extension, not a change: nothing of it in the base header or the base table
    base = open(os.path.join(ROOT, "include", "sdplr_hip.h")).read()
    assert "sdplr_hip_round" not in base and not set(cabi.ROUND_SIGNATURES) & set(cabi.SIGNATURES)
    assert '#include "sdplr_hip.h"' in open(HEADER).read()


def test_library_exports_the_round_symbols(hip_abi):
    for name in cabi.ROUND_SIGNATURES:
        assert hasattr(hip_abi.lib, "sdplr_hip_" + name)
        assert getattr(hip_abi, name).argtypes == cabi.ROUND_SIGNATURES[name]
    assert hip_abi.has_round


def test_oracle_abi_loads_without_the_round_symbols(oracle_abi):
    assert not oracle_abi.has_round
    for name in cabi.ROUND_SIGNATURES:
        assert not hasattr(oracle_abi, name)
    s = sj.build_solver(oracle_abi, problems.maxcut_data(problems.gnp_graph(12, 0.5, 1)), 2,
                        sj.BurerMonteiroConfig(seed=0, printlevel=0))
    with pytest.raises(NotImplementedError):
        s.round_set_graph(problems.gnp_graph(12, 0.5, 1))
    with pytest.raises(NotImplementedError):
        s.round(0, 1, np.zeros((1, 2)))
    s.close()


def test_round_needs_a_device(hip_abi):
    """Without a device no handle exists (create refuses, tests/test_cabi_symbols.py), and the two entry points refuse
    before they look at their handle."""
    n = C.c_int32(-1)
    assert hip_abi.device_count(C.byref(n)) == 0
    if n.value > 0:
        # with a device the same calls get as far as the handle check
        assert hip_abi.round_set_graph(None, 0, 0, None, None, None) == cabi.ERR_INVALID_ARG
        return
    best = C.c_int64(0)
    g, c = np.zeros(2), np.zeros(1)
    assert hip_abi.round_set_graph(None, 0, 0, None, None, None) == cabi.ERR_NO_DEVICE
    assert hip_abi.round(None, 0, cabi.F_RT, 1, cabi._pd(g), cabi._pd(c), C.byref(best), None, None) == cabi.ERR_NO_DEVICE
    assert b"no usable HIP device" in hip_abi.last_error(None)


# what sdplr() returned before it had a callback (src/sdplr.jl:426-448 plus this package's "schedule" and the
# preprocess_time of :130-131)
TODAYS_KEYS = {"Rt", "lambda", "Rt0", "lambda0", "sigma", "grad_norm", "primal_vio", "obj", "max_dual_value", "min_duality_gap",
               "totaltime", "dual_time", "primaltime", "iter", "majoriter", "DIMACS_errs", "ptol", "objtol", "fprec",
               "rankupd_tol", "r", "schedule", "preprocess_time"}


def test_sdplr_callback_runs_on_the_live_handle(oracle_abi):
    data = problems.maxcut_data(problems.gnp_graph(30, 0.3, 5))
    kw = dict(data=data, r=4, abi=oracle_abi, seed=1, printlevel=0, ptol=1e-2, objtol=1e-2, prior_trace_bound=30.0)
    plain = sj.sdplr(**kw)
    seen = []

    def f(var, d):
        seen.append((d is data, var.Rt.copy(), var.r))      # the handle answers: it is still open
        return 42.5

    res = sj.sdplr(callback=f, **kw)
    assert len(seen) == 1 and seen[0][0] and seen[0][2] == res["r"]
    assert np.array_equal(seen[0][1], res["Rt"])
    assert res["callback_res"] == 42.5 and res["callback_time"] >= 0.0
    assert set(res) == set(plain) | {"callback_res", "callback_time"}
    assert set(plain) == TODAYS_KEYS
    assert "callback_res" not in plain and "callback_time" not in plain
    assert np.array_equal(plain["Rt"], res["Rt"])
    # an explicit keyword of sdplr, not a config field routed through the loop over kwargs
    assert not hasattr(sj.BurerMonteiroConfig(), "callback")


@pytest.mark.skipif(shutil.which("gcc") is None, reason="no gcc")
def test_round_example_compiles_strictly(tmp_path):
    subprocess.check_call(["gcc", "-std=c99", "-O2", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-c",
                           os.path.join(ROOT, "examples", "round_c_abi.c"), "-o", str(tmp_path / "ex.o")])
