"""`bench.py --dump-outputs DIR`: the state the last timed step left, written so that two builds can be compared output for output.

The run on the host shim (no GPU) and the run on the device check the same thing: `state.npy` is the seeded field advanced by
`--warmup` + `--repeats` x `--steps` Euler steps - so `--steps` really is the length of a timed region -, bit for bit what the CPU oracle
computes, and a second run with the same arguments writes the same bytes.
"""

from __future__ import annotations

import json
import os
import subprocess
import sys

import numpy as np
import pytest

import pde_hip
from helpers import ROOT, host_faces, interior, oracle_grid, to_full
from oracle import pde_oracle as O
from pde_hip import _abi


def _run_bench(tmp_path, name, env, steps, warmup, repeats, size):
    out_dir = tmp_path / name
    cmd = [sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup), "--size", str(size), "--repeats", str(repeats),
           "--no-cpu-baseline", "--no-extra", "--dump-outputs", str(out_dir)]
    proc = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env={**os.environ, **env}, cwd=str(ROOT))
    lines = [ln for ln in proc.stdout.splitlines() if ln.startswith("{")]
    assert proc.returncode == 0 and len(lines) == 1, proc.stderr[-3000:]
    return json.loads(lines[0]), out_dir


def _expected_state(size, steps):
    grid = pde_hip.UnitGrid([size] * 3, periodic=True)
    eq = pde_hip.DiffusionPDE(1.0)
    state = pde_hip.ScalarField.random_uniform(grid, rng=np.random.default_rng(0))
    rhs = O.make_rhs(_abi.RHS_DIFFUSION, 1.0, host_faces(grid.get_boundary_conditions(eq.bc)).c)
    return interior(grid, O.euler_run(oracle_grid(grid), rhs, to_full(grid, state.data), 0.1, steps))


def _check_dump(tmp_path, env, steps=5, warmup=3, repeats=2, size=24):
    line, out_dir = _run_bench(tmp_path, "first", env, steps, warmup, repeats, size)
    assert line["steps"] == steps and line["outputs"]["state"] == {"file": "state.npy", "dtype": "float64", "of_shape": [size] * 3, "sampled": False, "shape": [size] * 3}
    assert sorted(p.name for p in out_dir.iterdir()) == ["state.npy"]
    state = np.load(out_dir / "state.npy", allow_pickle=False)
    assert state.dtype == np.float64 and state.shape == (size,) * 3
    np.testing.assert_array_equal(state, _expected_state(size, warmup + repeats * steps))
    # one step more per timed region is another state: the flag sets the number of timed steps
    assert not np.array_equal(state, _expected_state(size, warmup + repeats * (steps + 1)))
    _, again = _run_bench(tmp_path, "second", env, steps, warmup, repeats, size)
    assert (again / "state.npy").read_bytes() == (out_dir / "state.npy").read_bytes()


def test_bench_dumps_the_state_of_the_last_timed_step_on_the_host_shim(tmp_path):
    import shimlib

    _check_dump(tmp_path, {"PDEHIP_LIB": str(shimlib.build()), "PDEHIP_ALLOW_LIB_OVERRIDE": "1", "PDEHIP_SHIM_FUSED": "1", "OMP_NUM_THREADS": "2"})


@pytest.mark.gpu
def test_bench_dumps_the_state_of_the_last_timed_step(tmp_path):
    _check_dump(tmp_path, {}, steps=7, warmup=4, repeats=2, size=96)


def test_a_large_output_is_dumped_as_a_fixed_seeded_sample(tmp_path):
    """Above the value budget the file holds the values at indices that depend on the array's size alone: the same cells from run to run."""
    import bench

    assert bench.DUMP_MAX_VALUES * 8 < 64e6
    rng = np.random.default_rng(5)
    big, other = rng.random((40, 50, 60)), rng.random((40, 50, 60))
    info = bench.dump_outputs(str(tmp_path / "a"), {"state": big}, max_values=1000)["state"]
    bench.dump_outputs(str(tmp_path / "b"), {"state": other}, max_values=1000)
    assert info["sampled"] and info["shape"] == [1000] and info["of_shape"] == [40, 50, 60]
    got, got_other = np.load(tmp_path / "a" / "state.npy"), np.load(tmp_path / "b" / "state.npy")
    index = np.sort(np.random.default_rng(bench.DUMP_SEED).integers(0, big.size, size=1000))
    assert got.dtype == np.float64 and len(set(index.tolist())) > 990
    np.testing.assert_array_equal(got, big.reshape(-1)[index])
    np.testing.assert_array_equal(got_other, other.reshape(-1)[index])
    # a float32 array is stored as float64 (exactly), whole when it fits
    small = rng.random((3, 4)).astype(np.float32)
    assert not bench.dump_outputs(str(tmp_path / "a"), {"small": small}, max_values=1000)["small"]["sampled"]
    stored = np.load(tmp_path / "a" / "small.npy")
    assert stored.dtype == np.float64 and np.array_equal(stored, small)
