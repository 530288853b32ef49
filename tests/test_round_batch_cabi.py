"""CPU-side checks of the batch rounding extension of the C ABI (include/sdplr_hip_round_batch.h): the header declares
exactly ``cabi.ROUND_BATCH_SIGNATURES`` on top of sdplr_hip_round.h and nothing of it leaks into the two existing headers
or their tables, the cross-compiled library exports the symbol, the item struct's ctypes mirror has the C layout, nothing
computes without a device, the CPU checker's ABI loads and refuses, the example compiles strictly, and
``solve_lockstep(rounding=None)`` returns what it returned before."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import sdplrplus_jl_amd as sj
from sdplrplus_jl_amd import batch, cabi, problems, rounding

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
HEADER = os.path.join(INC, "sdplr_hip_round_batch.h")

_CTYPE = {"sdplr_hip_solver*": cabi._vp, "int32_t": cabi._i32, "int64_t": cabi._i64, "const double*": cabi._pf64,
          "double*": cabi._pf64, "int8_t*": cabi._pi8}


def _stripped(path):
    return re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)


def _struct_fields(txt, name):
    """[(C type, field name)] of ``typedef struct name { … } name;`` — ``int32_t a, b;`` gives two fields."""
    body = re.search(r"typedef\s+struct\s+" + name + r"\s*\{(.*?)\}\s*" + name + r"\s*;", txt, flags=re.S).group(1)
    out = []
    for decl in body.split(";"):
        decl = " ".join(decl.split())
        if not decl:
            continue
        m = re.match(r"(.*?[\s\*])(\w+(?:\s*,\s*\w+)*)$", decl)
        for f in m.group(2).split(","):
            out.append((m.group(1).strip(), f.strip()))
    return out


def test_batch_round_header_is_the_signature_table():
    txt = _stripped(HEADER)
    decl = {m.group(1): [a.strip() for a in m.group(2).split(",")]
            for m in re.finditer(r"\bint32_t\s+sdplr_hip_(\w+)\s*\(([^;]*?)\)\s*;", txt, flags=re.S)}
    assert set(decl) == set(cabi.ROUND_BATCH_SIGNATURES) == {"batch_round"}
    assert [a.rsplit(" ", 1)[0] for a in decl["batch_round"]] == ["int32_t", "sdplr_hip_round_item*"]
    assert cabi.ROUND_BATCH_SIGNATURES["batch_round"] == [cabi._i32, C.POINTER(cabi.RoundItem)]
    # the struct, field by field
    fields = _struct_fields(txt, "sdplr_hip_round_item")
    assert [f for _, f in fields] == [f for f, _ in cabi.RoundItem._fields_]
    assert [_CTYPE[t] for t, _ in fields] == [t for _, t in cabi.RoundItem._fields_]
    # a header of its own on top of the rounding header; nothing of it in the existing headers or tables
    assert '#include "sdplr_hip_round.h"' in open(HEADER).read()
    for other in ("sdplr_hip.h", "sdplr_hip_round.h"):
        base = open(os.path.join(INC, other)).read()
        assert "batch_round" not in base and "sdplr_hip_round_item" not in base, other
    assert not set(cabi.ROUND_BATCH_SIGNATURES) & (set(cabi.SIGNATURES) | set(cabi.ROUND_SIGNATURES))


@pytest.mark.skipif(shutil.which("gcc") is None, reason="no gcc")
def test_round_item_mirror_has_the_c_layout(tmp_path):
    names = [f for f, _ in cabi.RoundItem._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sdplr_hip_round_batch.h"\n'
                   'int main(void) { printf("%zu", sizeof(sdplr_hip_round_item));\n'
                   + "".join(f'  printf(" %zu %zu", offsetof(sdplr_hip_round_item, {f}), sizeof(((sdplr_hip_round_item*)0)->{f}));\n'
                             for f in names) + "  return 0; }\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I", INC, str(src), "-o", str(exe)])
    nums = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    assert nums[0] == C.sizeof(cabi.RoundItem)
    for k, f in enumerate(names):
        d = getattr(cabi.RoundItem, f)
        assert (nums[1 + 2 * k], nums[2 + 2 * k]) == (d.offset, d.size), f


def test_library_exports_batch_round(hip_abi):
    assert hasattr(hip_abi.lib, "sdplr_hip_batch_round")
    assert hip_abi.has_round_batch and hip_abi.batch_round.argtypes == cabi.ROUND_BATCH_SIGNATURES["batch_round"]


def test_batch_round_needs_a_device(hip_abi):
    n = C.c_int32(-1)
    assert hip_abi.device_count(C.byref(n)) == 0
    arr = (cabi.RoundItem * 2)()
    for q in arr:
        q.status, q.route, q.best = 55, 55, -1
    if n.value > 0:
        # with a device the same call gets as far as the items: null handles
        assert hip_abi.batch_round(1, arr) == cabi.ERR_INVALID_ARG and arr[0].status == cabi.ERR_INVALID_ARG
        assert hip_abi.batch_round(-1, arr) == cabi.ERR_INVALID_ARG
        return
    assert hip_abi.batch_round(2, arr) == cabi.ERR_NO_DEVICE
    assert b"no usable HIP device" in hip_abi.last_error(None)
    assert [(q.status, q.route, q.best) for q in arr] == [(55, 55, -1)] * 2          # before looking at any item
    assert hip_abi.batch_round(-1, arr) == cabi.ERR_INVALID_ARG
    assert hip_abi.batch_round(1, None) == cabi.ERR_INVALID_ARG


def test_oracle_abi_loads_and_refuses(oracle_abi):
    assert not oracle_abi.has_round_batch and not hasattr(oracle_abi, "batch_round")
    A = problems.gnp_graph(12, 0.5, 1)
    s = sj.build_solver(oracle_abi, problems.maxcut_data(A), 2, sj.BurerMonteiroConfig(seed=0, printlevel=0))
    with pytest.raises(NotImplementedError):
        cabi.batch_round(oracle_abi, [s], [(0, 1, np.zeros((1, 2)))])
    with pytest.raises(NotImplementedError):
        rounding.batch_rounding_device([s], [A], [np.random.default_rng(0)], "maxcut", trials=3)
    s.close()


@pytest.mark.skipif(shutil.which("gcc") is None, reason="no gcc")
def test_batch_round_example_compiles_strictly(tmp_path):
    subprocess.check_call(["gcc", "-std=c99", "-O2", "-Wall", "-Wextra", "-Werror", "-I", INC, "-c",
                           os.path.join(ROOT, "examples", "batch_round_c_abi.c"), "-o", str(tmp_path / "ex.o")])


# what sdplr() returns without a callback (tests/test_round_cabi.py)
TODAYS_KEYS = {"Rt", "lambda", "Rt0", "lambda0", "sigma", "grad_norm", "primal_vio", "obj", "max_dual_value", "min_duality_gap",
               "totaltime", "dual_time", "primaltime", "iter", "majoriter", "DIMACS_errs", "ptol", "objtol", "fprec",
               "rankupd_tol", "r", "schedule", "preprocess_time"}


def test_solve_lockstep_without_rounding_is_todays(oracle_abi):
    graphs = [problems.gnp_graph(20 + 4 * k, 0.3, 5 + k) for k in range(3)]
    datas = [problems.maxcut_data(A) for A in graphs]
    kw = dict(abi=oracle_abi, seed=1, printlevel=0, ptol=1e-2, objtol=1e-2, prior_trace_bound=30.0)
    base = batch.solve_lockstep(datas, 4, **kw)
    none = batch.solve_lockstep(datas, 4, rounding=None, **kw)
    for a, b, d in zip(base, none, datas):
        assert set(a) == set(b) == TODAYS_KEYS
        assert a["obj"] == b["obj"] and a["iter"] == b["iter"] and np.array_equal(a["Rt"], b["Rt"])
        one = sj.sdplr(data=d, r=4, **kw)
        assert np.array_equal(one["Rt"], b["Rt"]) and one["iter"] == b["iter"]
    # the rounding needs the device library: the CPU checker's ABI refuses, after the solves, with every handle closed
    rngs = [np.random.default_rng(k) for k in range(3)]
    with pytest.raises(NotImplementedError):
        batch.solve_lockstep(datas, 4, rounding=[("maxcut", A, g) for A, g in zip(graphs, rngs)], **kw)
    with pytest.raises(ValueError):
        batch.solve_lockstep(datas, 4, rounding=[("maxcut", graphs[0], rngs[0])], **kw)
