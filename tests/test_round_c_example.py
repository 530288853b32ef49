"""examples/round_c_abi.c — a MaxCut solve followed by the device rounding, from plain C through include/sdplr_hip.h and
include/sdplr_hip_round.h: compiled, run as a fresh child process on the HIP library, and its printed best cut compared
with the comparator's (tests/round_reference.py) on the R and Γ the program dumps."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import round_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "examples", "round_c_abi.c")
INC = os.path.join(ROOT, "include")

pytestmark = pytest.mark.skipif(shutil.which("gcc") is None, reason="no gcc")


@pytest.mark.gpu
def test_round_example_runs_on_the_device(tmp_path, hip_abi):
    ldir = os.path.join(ROOT, "sdplrplus.jl_amd", "lib")
    exe, dump = tmp_path / "round_hip", tmp_path / "dump.bin"
    subprocess.check_call(["gcc", "-O2", "-I", INC, SRC, "-L", ldir, "-lsdplr_hip", "-lm", f"-Wl,-rpath,{ldir}",
                           "-Wl,-rpath-link,/opt/rocm/lib", "-o", str(exe)])
    n, r = 1000, 8
    out = subprocess.run([str(exe), str(n), str(r), str(dump)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip().endswith("OK") and "sdplr_hip" in out.stdout.splitlines()[0]
    m = re.search(r"best cut = (\S+) \(trial (\d+)\)", out.stdout)
    assert m, out.stdout
    raw = open(dump, "rb").read()
    hdr = np.frombuffer(raw[:24], dtype=np.int64)
    assert tuple(hdr[:2]) == (n, r)
    T = int(hdr[2])
    body = np.frombuffer(raw[24:], dtype=np.float64)
    R, gauss = body[: n * r].reshape(n, r), body[n * r:].reshape(T, r)
    j = np.arange(n)
    I = np.concatenate([j] * 3)
    J = np.concatenate([(j + d) % n for d in (1, 2, 3)])
    lo, hi = np.minimum(I, J), np.maximum(I, J)
    want = ref.rounding(R, gauss, (lo, hi, np.ones(lo.size)), 0)
    assert float(m.group(1)) == want["cuts"][want["best"]] and int(m.group(2)) == want["best"]
