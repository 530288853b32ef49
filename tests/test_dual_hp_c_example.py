"""examples/dual_hp_c_abi.c — the high-precision dual bound through include/sdplr_hip_dual_hp.h from plain C: the source
compiles against the header (``cc -fsyntax-only``, and strictly with gcc); on a GPU box the same source is linked with
libsdplr_hip.so and must report OK."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "examples", "dual_hp_c_abi.c")
INC = os.path.join(ROOT, "include")
CC = shutil.which("cc") or shutil.which("gcc")

pytestmark = pytest.mark.skipif(CC is None, reason="no C compiler")


def test_example_passes_syntax_only():
    subprocess.check_call([CC, "-std=c99", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", INC, SRC])


def test_example_compiles_strictly(tmp_path):
    subprocess.check_call([CC, "-std=c99", "-O2", "-Wall", "-Wextra", "-Werror", "-I", INC, "-c", SRC, "-o", str(tmp_path / "ex.o")])


@pytest.mark.gpu
def test_example_runs_on_the_device(tmp_path, hip_abi):
    ldir = os.path.join(ROOT, "sdplrplus.jl_amd", "lib")
    exe = tmp_path / "dual_hp_hip"
    subprocess.check_call([CC, "-O2", "-I", INC, SRC, "-L", ldir, "-lsdplr_hip", "-lm", f"-Wl,-rpath,{ldir}",
                           "-Wl,-rpath-link,/opt/rocm/lib", "-o", str(exe)])
    env = {k: v for k, v in os.environ.items() if k not in ("SDPLR_HIP_FORCE_GRAPH", "SDPLR_HIP_NO_RESIDENT")}
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120, env=env)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip().endswith("OK")
    rows = [ln for ln in out.stdout.splitlines() if ln.startswith("instance")]
    assert len(rows) == 2 and all(ln.split()[-1] == "1" for ln in rows)      # route 1: the shared launches
