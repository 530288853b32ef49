"""The rounding methods of julia/SDPLRPlusHIP.jl (unexecuted, like the rest of that file) checked statically against
include/sdplr_hip_round.h: every ccall through LIBSDPLR_HIP_ROUND names a symbol of that header, with its argument count
and matching C types, and passes as many values as types."""
import os
import re

from sdplrplus_jl_amd import cabi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JL = os.path.join(ROOT, "julia", "SDPLRPlusHIP.jl")
HDR = os.path.join(ROOT, "include", "sdplr_hip_round.h")

C2JL = {"int32_t": "Int32", "int64_t": "Int64", "sdplr_hip_solver*": "Ptr{Cvoid}", "double*": "Ptr{Float64}",
        "const double*": "Ptr{Float64}", "int64_t*": "Ptr{Int64}", "const int64_t*": "Ptr{Int64}", "int8_t*": "Ptr{Int8}"}


def header_signatures():
    txt = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    out = {}
    for m in re.finditer(r"\bint32_t\s+sdplr_hip_(\w+)\s*\(([^;]*?)\)\s*;", txt, flags=re.S):
        args = [re.sub(r"\s+", " ", a.strip()) for a in m.group(2).replace("\n", " ").split(",")]
        out[m.group(1)] = [a.rsplit(" ", 1)[0] for a in args]
    return out


def test_round_ccalls_match_the_round_header():
    sigs = header_signatures()
    assert set(sigs) == set(cabi.ROUND_SIGNATURES)
    src = open(JL).read()
    calls = list(re.finditer(r"ccall\(\(:sdplr_hip_(\w+),\s*LIBSDPLR_HIP_ROUND\),\s*(\w+),\s*\(([^)]*)\),([^\n]*\n[^\n]*)", src))
    assert {m.group(1) for m in calls} == set(sigs)
    for m in calls:
        types = [t.strip() for t in m.group(3).replace("\n", " ").split(",") if t.strip()]
        assert m.group(2) == "Int32"
        assert types == [C2JL[c] for c in sigs[m.group(1)]], m.group(1)
        values = m.group(4).split("), aux.handle)")[0]
        depth, n = 0, 1
        for ch in values:
            depth += ch in "([{"
            depth -= ch in ")]}"
            n += ch == "," and depth == 0
        assert n == len(types), (m.group(1), n, len(types))
    assert "const LIBSDPLR_HIP_ROUND = LIBSDPLR_HIP" in src
    for pat in (r"function maxcut_rounding\(A::SparseMatrixCSC\{Float64\}, aux::HIPAux",
                r"function minimumbisection_rounding\(A::SparseMatrixCSC\{Float64\}, aux::HIPAux"):
        assert re.search(pat, src), pat
