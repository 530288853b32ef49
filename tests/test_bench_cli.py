"""bench.py's command line on CPU (`--selftest-cpu`: the CPU checker on a small instance, same code path as on the GPU):
a plain run carries the headline figure only, `--full` adds the per-kernel profile and the roofline, `--steps` sets the
number of timed steps, and `--dump-outputs DIR` writes the arrays of the last timed step — the same from run to run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")
DUMPED = {"state": (5,), "Rt": (300, 8), "Gt": (300, 8), "primal_vio_raw": (301,), "y": (301,)}


def _run(*extra):
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "SDPLR_BENCH_FORCE_LAUNCH",
              "SDPLR_BENCH_FORCE_DIST"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--selftest-cpu", *extra], env=env, capture_output=True,
                       text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, lines
    return json.loads(lines[0])


@pytest.fixture(scope="module")
def plain(tmp_path_factory):
    out = tmp_path_factory.mktemp("dump_a")
    return _run("--steps", "7", "--warmup", "3", "--dump-outputs", str(out)), out


def test_plain_run_has_the_headline_and_nothing_that_needs_runs_of_its_own(plain):
    d, _ = plain
    assert d["steps"] == 7 and d["warmup"] == 3 and d["n_gpus"] == 1
    assert d["unit"] == "iterations/s" and d["higher_is_better"] is True and d["dtype"] == "f64"
    assert d["ms_per_step"] > 0 and abs(d["value"] - 1e3 / d["ms_per_step"]) < 1e-9 * d["value"]
    for key in ("roofline", "kernels_eager_profile", "cpu_baseline", "parity", "other_configs"):
        assert key not in d, key


def test_full_adds_the_profile_and_the_roofline(plain, tmp_path):
    d = _run("--steps", "7", "--warmup", "3", "--full", "--dump-outputs", str(tmp_path))
    assert d["steps"] == 7 and d["ms_per_step"] > 0
    assert "kernels_eager_profile" in d and d["roofline"]["bound"] == "hbm"     # (the CPU checker times no kernels)
    # the outputs are those of the last TIMED step, whatever --full runs after it
    for n in DUMPED:
        assert np.array_equal(np.load(os.path.join(plain[1], n + ".npy")), np.load(os.path.join(tmp_path, n + ".npy"))), n


def test_steps_sets_the_number_of_timed_steps(plain, tmp_path):
    """The CPU checker is deterministic and its loop resumes bit for bit, so the state after the timed steps is a function
    of warm-up + steps: 7 + 3 and 3 + 7 end in the same arrays, one more timed step does not."""
    _, out = plain
    a, b = tmp_path / "a", tmp_path / "b"
    assert _run("--steps", "3", "--warmup", "7", "--dump-outputs", str(a))["steps"] == 3
    assert _run("--steps", "8", "--warmup", "3", "--dump-outputs", str(b))["steps"] == 8
    for n in DUMPED:
        ref = np.load(os.path.join(out, n + ".npy"))
        assert np.array_equal(ref, np.load(a / (n + ".npy"))), n
        assert not np.array_equal(ref, np.load(b / (n + ".npy"))), n


def test_dump_outputs_writes_the_last_timed_step(plain):
    d, out = plain
    assert sorted(os.listdir(out)) == sorted(n + ".npy" for n in DUMPED)
    arrays = {n: np.load(os.path.join(out, n + ".npy")) for n in DUMPED}
    for n, shape in DUMPED.items():
        assert arrays[n].dtype == np.float64 and arrays[n].shape == shape and np.all(np.isfinite(arrays[n])), n
    L, gnorm, pvnorm, alpha, obj = arrays["state"]
    assert obj == d["objectives"][0] and gnorm > 0 and alpha > 0
    # the arrays belong to that very state: the norms the inner loop returned are theirs (src/sdplr.jl:224-234; MaxCut has
    # equality constraints only, so primal_vio is primal_vio_raw without its last entry, the objective)
    from sdplrplus_jl_amd import problems
    import bench
    data = problems.maxcut_data(problems.gnp_graph(300, 0.05, bench.GRAPH_SEED))
    assert abs(np.linalg.norm(arrays["Gt"]) / data.normC() - gnorm) < 1e-12 * gnorm
    assert abs(np.linalg.norm(arrays["primal_vio_raw"][:-1]) / np.linalg.norm(data.b) - pvnorm) < 1e-12 * pvnorm
    assert arrays["primal_vio_raw"][-1] == obj


def test_dump_outputs_is_the_same_from_run_to_run(plain, tmp_path):
    _, out = plain
    _run("--steps", "7", "--warmup", "3", "--dump-outputs", str(tmp_path))
    for n in DUMPED:
        assert np.array_equal(np.load(os.path.join(out, n + ".npy")), np.load(os.path.join(tmp_path, n + ".npy"))), n
