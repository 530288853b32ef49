"""CPU-side checks of the high-precision dual bound's extension of the C ABI (include/sdplr_hip_dual_hp.h): the header
declares exactly ``cabi.DUAL_HP_SIGNATURES`` on top of sdplr_hip.h and nothing of it leaks into the existing headers or their
tables, the item struct's ctypes mirror has the C layout (field order, offsets, sizeof from a C program compiled against the
header), the cross-compiled library exports both symbols, nothing computes without a device, and the CPU checker's ABI
loads and refuses."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

import sdplrplus_jl_amd as sj
from sdplrplus_jl_amd import cabi, problems

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
HEADER = os.path.join(INC, "sdplr_hip_dual_hp.h")

_CTYPE = {"sdplr_hip_solver*": cabi._vp, "int32_t": cabi._i32, "int64_t": cabi._i64, "double": cabi._f64,
          "const double*": cabi._pf64, "double*": cabi._pf64, "int64_t*": cabi._pi64,
          "sdplr_hip_dual_hp_item*": C.POINTER(cabi.DualHpItem)}


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


def test_dual_hp_header_is_the_signature_table():
    txt = _stripped(HEADER)
    decl = {m.group(1): [" ".join(a.split()) for a in m.group(2).split(",")]
            for m in re.finditer(r"\bint32_t\s+sdplr_hip_(\w+)\s*\(([^;]*?)\)\s*;", txt, flags=re.S)}
    assert set(decl) == set(cabi.DUAL_HP_SIGNATURES) == {"dual_obj_hp", "batch_dual_obj_hp"}
    for name, args in decl.items():
        assert [_CTYPE[a.rsplit(" ", 1)[0]] for a in args] == cabi.DUAL_HP_SIGNATURES[name], name
    assert [a.rsplit(" ", 1)[1] for a in decl["dual_obj_hp"]] == [
        "s", "trace_bound", "ncv", "tol", "maxiter", "v0", "dual_value", "mineig", "n_matvec", "n_converged"]
    fields = _struct_fields(txt, "sdplr_hip_dual_hp_item")
    assert [f for _, f in fields] == [f for f, _ in cabi.DualHpItem._fields_] == [
        "s", "trace_bound", "ncv", "tol", "maxiter", "v0", "y_out", "dual_value", "mineig", "n_matvec", "n_converged",
        "route", "status"]
    assert [_CTYPE[t] for t, _ in fields] == [t for _, t in cabi.DualHpItem._fields_]
    # a header of its own on top of sdplr_hip.h, citing the reference lines; nothing of it in the existing headers or tables
    raw = open(HEADER).read()
    assert '#include "sdplr_hip.h"' in raw and "src/coreop.jl:376-415" in raw
    for other in ("sdplr_hip.h", "sdplr_hip_round.h", "sdplr_hip_round_batch.h", "sdplr_hip_eig_batch.h"):
        base = open(os.path.join(INC, other)).read()
        assert "dual_obj_hp" not in base and "sdplr_hip_dual_hp_item" not in base, other
    assert not set(cabi.DUAL_HP_SIGNATURES) & (set(cabi.SIGNATURES) | set(cabi.ROUND_SIGNATURES) |
                                               set(cabi.ROUND_BATCH_SIGNATURES) | set(cabi.EIG_BATCH_SIGNATURES))


@pytest.mark.skipif(shutil.which("gcc") is None, reason="no gcc")
def test_dual_hp_item_mirror_has_the_c_layout(tmp_path):
    names = [f for f, _ in cabi.DualHpItem._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sdplr_hip_dual_hp.h"\n'
                   'int main(void) { printf("%zu", sizeof(sdplr_hip_dual_hp_item));\n'
                   + "".join(f'  printf(" %zu %zu", offsetof(sdplr_hip_dual_hp_item, {f}), sizeof(((sdplr_hip_dual_hp_item*)0)->{f}));\n'
                             for f in names) + "  return 0; }\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I", INC, str(src), "-o", str(exe)])
    nums = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    assert nums[0] == C.sizeof(cabi.DualHpItem)
    for k, f in enumerate(names):
        d = getattr(cabi.DualHpItem, f)
        assert (nums[1 + 2 * k], nums[2 + 2 * k]) == (d.offset, d.size), f


def test_library_exports_both_symbols(hip_abi):
    assert hasattr(hip_abi.lib, "sdplr_hip_dual_obj_hp") and hasattr(hip_abi.lib, "sdplr_hip_batch_dual_obj_hp")
    assert hip_abi.has_dual_hp
    for name, argtypes in cabi.DUAL_HP_SIGNATURES.items():
        assert getattr(hip_abi, name).argtypes == argtypes


def test_dual_hp_needs_a_device(hip_abi):
    n = C.c_int32(-1)
    assert hip_abi.device_count(C.byref(n)) == 0
    arr = (cabi.DualHpItem * 2)()
    for q in arr:
        q.status, q.route, q.n_matvec, q.n_converged, q.dual_value, q.mineig = 55, 55, -1, -1, 7.0, 7.0
    assert hip_abi.batch_dual_obj_hp(0, None) == cabi.OK and hip_abi.batch_dual_obj_hp(0, arr) == cabi.OK
    assert hip_abi.batch_dual_obj_hp(-1, arr) == cabi.ERR_INVALID_ARG
    assert hip_abi.batch_dual_obj_hp(1, None) == cabi.ERR_INVALID_ARG
    d, e = C.c_double(7.0), C.c_double(7.0)
    mv, nc = C.c_int64(-1), C.c_int64(-1)
    single = lambda: hip_abi.dual_obj_hp(None, 1.0, 0, 1e-6, 10, None, C.byref(d), C.byref(e), C.byref(mv), C.byref(nc))
    if n.value > 0:
        # with a device the same calls get as far as the handles: null ones
        assert hip_abi.batch_dual_obj_hp(1, arr) == cabi.ERR_INVALID_ARG and arr[0].status == cabi.ERR_INVALID_ARG
        assert single() == cabi.ERR_INVALID_ARG
        return
    assert hip_abi.batch_dual_obj_hp(2, arr) == cabi.ERR_NO_DEVICE
    assert b"no usable HIP device" in hip_abi.last_error(None)
    assert [(q.status, q.route, q.n_matvec, q.n_converged, q.dual_value, q.mineig) for q in arr] == [(55, 55, -1, -1, 7.0, 7.0)] * 2
    assert single() == cabi.ERR_NO_DEVICE                              # before the handle is looked at
    assert b"no usable HIP device" in hip_abi.last_error(None)
    assert (d.value, e.value, mv.value, nc.value) == (7.0, 7.0, -1, -1)


def test_oracle_abi_loads_and_refuses(oracle_abi):
    assert not oracle_abi.has_dual_hp and not hasattr(oracle_abi, "dual_obj_hp") and not hasattr(oracle_abi, "batch_dual_obj_hp")
    s = sj.build_solver(oracle_abi, problems.maxcut_data(problems.gnp_graph(12, 0.5, 1)), 2,
                        sj.BurerMonteiroConfig(seed=0, printlevel=0))
    with pytest.raises(NotImplementedError):
        s.dual_obj_hp(12.0, 0, 1e-6, 100, None)
    with pytest.raises(NotImplementedError):
        cabi.batch_dual_obj_hp(oracle_abi, [s], [(12.0, 0, 1e-6, 100, None)])
    s.close()


def test_julia_binding_calls_dual_obj_hp_as_declared():
    """julia/SDPLRPlusHIP.jl: ``dual_obj(...; highprecision=true)`` is one ccall of sdplr_hip_dual_obj_hp (looked up by name:
    an extension), with the header's argument types, and neither runs g! nor downloads y."""
    src = open(os.path.join(ROOT, "julia", "SDPLRPlusHIP.jl")).read()
    assert "Libdl.dlsym(Libdl.dlopen(LIBSDPLR_HIP), :sdplr_hip_dual_obj_hp)" in src
    body = src[src.index("function dual_obj(data, var::SolverVars, aux::HIPAux, trace_bound, iter::Integer; highprecision::Bool=false)"):]
    body = body[:body.index("\nend\n")]
    hp = body[body.index("if highprecision"):body.index("    end\n")]
    m = re.search(r"ccall\(hip_dual_obj_hp_ptr\(\),\s*Int32,\s*\(([^)]*)\),\s*(.*?)\), aux\.handle\)", hp, flags=re.S)
    jl = {cabi._vp: "Ptr{Cvoid}", cabi._f64: "Float64", cabi._i64: "Int64", cabi._pf64: "Ptr{Float64}", cabi._pi64: "Ptr{Int64}"}
    types = [t.strip() for t in m.group(1).replace("\n", " ").split(",") if t.strip()]
    assert types == [jl[t] for t in cabi.DUAL_HP_SIGNATURES["dual_obj_hp"]]
    depth, nvals = 0, 1
    for ch in m.group(2):
        depth += ch in "([{"
        depth -= ch in ")]}"
        nvals += ch == "," and depth == 0
    assert nvals == len(types)
    assert "g!(" not in hp and "hip_get_vec!" not in hp and "SDP_S_eigval(" not in hp
