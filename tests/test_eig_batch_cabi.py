"""CPU-side checks of the batch eigenvalue extension of the C ABI (include/sdplr_hip_eig_batch.h): the header declares
exactly ``cabi.EIG_BATCH_SIGNATURES`` on top of sdplr_hip.h and nothing of it leaks into the three existing headers or
their tables, the cross-compiled library exports the symbol, the item struct's ctypes mirror has the C layout, nothing
computes without a device, the CPU checker's ABI loads and refuses, the example compiles strictly, and the eigensolve of
``DIMACS_errors`` as a request of ``sdplr_steps`` gives what the public function gives."""
import ctypes as C
import importlib
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import sdplrplus_jl_amd as sj
from sdplrplus_jl_amd import batch, cabi, problems

sdplr_mod = importlib.import_module("sdplrplus_jl_amd.sdplr")     # (the package exports the function of the same name)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
HEADER = os.path.join(INC, "sdplr_hip_eig_batch.h")

_CTYPE = {"sdplr_hip_solver*": cabi._vp, "int32_t": cabi._i32, "int64_t": cabi._i64, "double": cabi._f64,
          "const double*": cabi._pf64, "double*": cabi._pf64}


def _stripped(path):
    return re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)


def _struct_fields(txt, name):
    """[(C type, field name)] of ``typedef struct name { … } name;`` — ``int64_t a, b;`` gives two fields."""
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


def test_batch_eig_header_is_the_signature_table():
    txt = _stripped(HEADER)
    decl = {m.group(1): [a.strip() for a in m.group(2).split(",")]
            for m in re.finditer(r"\bint32_t\s+sdplr_hip_(\w+)\s*\(([^;]*?)\)\s*;", txt, flags=re.S)}
    assert set(decl) == set(cabi.EIG_BATCH_SIGNATURES) == {"batch_S_eigval"}
    assert [a.rsplit(" ", 1)[0] for a in decl["batch_S_eigval"]] == ["int32_t", "sdplr_hip_eig_item*"]
    assert cabi.EIG_BATCH_SIGNATURES["batch_S_eigval"] == [cabi._i32, C.POINTER(cabi.EigItem)]
    fields = _struct_fields(txt, "sdplr_hip_eig_item")
    assert [f for _, f in fields] == [f for f, _ in cabi.EigItem._fields_]
    assert [_CTYPE[t] for t, _ in fields] == [t for _, t in cabi.EigItem._fields_]
    # a header of its own on top of sdplr_hip.h; nothing of it in the existing headers or tables
    assert '#include "sdplr_hip.h"' in open(HEADER).read()
    for other in ("sdplr_hip.h", "sdplr_hip_round.h", "sdplr_hip_round_batch.h"):
        base = open(os.path.join(INC, other)).read()
        assert "batch_S_eigval" not in base and "sdplr_hip_eig_item" not in base, other
    assert not set(cabi.EIG_BATCH_SIGNATURES) & (set(cabi.SIGNATURES) | set(cabi.ROUND_SIGNATURES) | set(cabi.ROUND_BATCH_SIGNATURES))


@pytest.mark.skipif(shutil.which("gcc") is None, reason="no gcc")
def test_eig_item_mirror_has_the_c_layout(tmp_path):
    names = [f for f, _ in cabi.EigItem._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sdplr_hip_eig_batch.h"\n'
                   'int main(void) { printf("%zu", sizeof(sdplr_hip_eig_item));\n'
                   + "".join(f'  printf(" %zu %zu", offsetof(sdplr_hip_eig_item, {f}), sizeof(((sdplr_hip_eig_item*)0)->{f}));\n'
                             for f in names) + "  return 0; }\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I", INC, str(src), "-o", str(exe)])
    nums = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    assert nums[0] == C.sizeof(cabi.EigItem)
    for k, f in enumerate(names):
        d = getattr(cabi.EigItem, f)
        assert (nums[1 + 2 * k], nums[2 + 2 * k]) == (d.offset, d.size), f


def test_library_exports_batch_S_eigval(hip_abi):
    assert hasattr(hip_abi.lib, "sdplr_hip_batch_S_eigval")
    assert hip_abi.has_eig_batch and hip_abi.batch_S_eigval.argtypes == cabi.EIG_BATCH_SIGNATURES["batch_S_eigval"]


def test_batch_S_eigval_needs_a_device(hip_abi):
    n = C.c_int32(-1)
    assert hip_abi.device_count(C.byref(n)) == 0
    arr = (cabi.EigItem * 2)()
    for q in arr:
        q.status, q.route, q.n_matvec, q.n_converged = 55, 55, -1, -1
    if n.value > 0:
        # with a device the same call gets as far as the items: null handles
        assert hip_abi.batch_S_eigval(1, arr) == cabi.ERR_INVALID_ARG and arr[0].status == cabi.ERR_INVALID_ARG
        assert hip_abi.batch_S_eigval(-1, arr) == cabi.ERR_INVALID_ARG
        return
    assert hip_abi.batch_S_eigval(2, arr) == cabi.ERR_NO_DEVICE
    assert b"no usable HIP device" in hip_abi.last_error(None)
    assert [(q.status, q.route, q.n_matvec, q.n_converged) for q in arr] == [(55, 55, -1, -1)] * 2   # before looking at any item
    assert hip_abi.batch_S_eigval(-1, arr) == cabi.ERR_INVALID_ARG
    assert hip_abi.batch_S_eigval(1, None) == cabi.ERR_INVALID_ARG


def test_oracle_abi_loads_and_refuses(oracle_abi):
    assert not oracle_abi.has_eig_batch and not hasattr(oracle_abi, "batch_S_eigval")
    A = problems.gnp_graph(12, 0.5, 1)
    s = sj.build_solver(oracle_abi, problems.maxcut_data(A), 2, sj.BurerMonteiroConfig(seed=0, printlevel=0))
    with pytest.raises(NotImplementedError):
        cabi.batch_S_eigval(oracle_abi, [s], [(1, "SA", 0, 0.0, 100, None)])
    s.close()


@pytest.mark.skipif(shutil.which("gcc") is None, reason="no gcc")
def test_batch_eig_example_compiles_strictly(tmp_path):
    subprocess.check_call(["gcc", "-std=c99", "-O2", "-Wall", "-Wextra", "-Werror", "-I", INC, "-c",
                           os.path.join(ROOT, "examples", "batch_eig_c_abi.c"), "-o", str(tmp_path / "ex.o")])


def test_certificate_through_the_request_path(oracle_abi, monkeypatch):
    """``sdplr(..., eval_DIMACS_errs=True)``: the eigensolve travels as one REQ_EIG request, the six errors are those of the
    public ``DIMACS_errors`` on the same final state; a lockstep batch on an ABI without the batch call serves the
    requests one by one, with the same results."""
    data = problems.maxcut_data(problems.gnp_graph(24, 0.3, 3))
    kw = dict(abi=oracle_abi, seed=1, printlevel=0, ptol=1e-2, objtol=1e-2, prior_trace_bound=30.0)
    seen, direct = [], []
    real = sdplr_mod.serve
    monkeypatch.setattr(sdplr_mod, "serve", lambda var, req: seen.append(req[0]) or real(var, req))
    ans = sj.sdplr(data=data, r=4, eval_DIMACS_errs=True,
                   callback=lambda var, d: direct.append(sj.DIMACS_errors(d, var)), **kw)
    assert seen.count(sdplr_mod.REQ_EIG) == 2 and seen[-1] == sdplr_mod.REQ_EIG        # the solve's, then the callback's
    assert seen[-2] == sdplr_mod.REQ_EIG and sdplr_mod.REQ_EIG not in seen[:-2]
    assert ans["DIMACS_errs"].shape == (6,) and ans["DIMACS_errs"][3] >= 0.0 and ans["DIMACS_errs"].any()
    assert np.array_equal(ans["DIMACS_errs"], direct[0])
    off = sj.sdplr(data=data, r=4, **kw)
    assert not off["DIMACS_errs"].any() and np.array_equal(off["Rt"], ans["Rt"]) and off["iter"] == ans["iter"]
    datas = [data, problems.maxcut_data(problems.gnp_graph(30, 0.3, 4))]
    lock = batch.solve_lockstep(datas, 4, eval_DIMACS_errs=True, **kw)
    assert np.array_equal(lock[0]["DIMACS_errs"], ans["DIMACS_errs"]) and np.array_equal(lock[0]["Rt"], ans["Rt"])
    two = sj.sdplr(data=datas[1], r=4, eval_DIMACS_errs=True, **kw)
    assert np.array_equal(lock[1]["DIMACS_errs"], two["DIMACS_errs"]) and lock[1]["iter"] == two["iter"]
