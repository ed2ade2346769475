"""Writes tests/golden/f32p.npz: what the REFERENCE's torch backend computes on float32 fields for the cases of ``f32p_cases`` - the
Laplacian with value / derivative / mixed faces and the explicit Euler loop of ``DiffusionPDE(0.7)`` with periodic and
``auto_periodic_neumann`` axes.  Before anything is written every result is compared with the numpy fp32 restatement
(``f32p_cases.laplace_full`` / ``euler_steps``): they must be equal BIT FOR BIT, with ``backend.torch.compile`` off and on.  Needs the
reference py-pde and torch (CPU) on the path; run from the repository root:

    python tests/golden/make_golden_f32p.py <path to the reference>
"""

from __future__ import annotations

import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))
sys.path.append(sys.argv[1])

import pde  # noqa: E402
import f32p_cases as FC  # noqa: E402


def reference_results(compile_flag: bool) -> dict:
    pde.config["backend.torch.compile"] = compile_flag
    out = {}
    for shape in FC.GOLDEN_LAPLACE_SHAPES:
        nd = len(shape)
        dx = FC.DX[nd]
        grid = pde.CartesianGrid(FC.bounds_for(shape, dx), shape)
        np.testing.assert_allclose(grid.discretization, dx, rtol=1e-15)
        valid = FC.golden_field(shape)
        out[f"field/{nd}d"] = valid
        for name, bc in FC.GOLDEN_LAPLACE_BCS.items():
            field = pde.ScalarField(grid, valid, dtype=np.float32)
            ref = field.laplace(bc, backend="torch").data
            assert ref.dtype == np.float32
            ghosts = field.copy()
            ghosts.set_ghost_cells(bc)
            assert ghosts._data_full.dtype == np.float32
            mine = FC.laplace_full(ghosts._data_full, grid.discretization)
            assert np.array_equal(mine, ref), f"laplace {shape} {name}: the restatement differs from the reference in {int((mine != ref).sum())} cells"
            out[f"lap/{nd}d/{name}"] = ref
    eq = pde.DiffusionPDE(FC.GOLDEN_D)          # bc: auto_periodic_neumann
    for cid, shape, periodic in FC.GOLDEN_EULER_CASES:
        nd = len(shape)
        dx = FC.DX[nd]
        grid = pde.CartesianGrid(FC.bounds_for(shape, dx), shape, periodic=list(periodic))
        dt = FC.stable_dt(grid.discretization, FC.GOLDEN_D)
        assert dt * FC.GOLDEN_D * float(np.sum(grid.discretization ** -2)) < 0.5
        valid = FC.golden_field(shape)
        for n in FC.GOLDEN_EULER_STEPS:
            field = pde.ScalarField(grid, valid, dtype=np.float32)
            res, info = eq.solve(field, t_range=n * dt, dt=dt, backend="torch", solver="euler", tracker=None, ret_info=True)
            assert info["solver"]["steps"] == n, (cid, n, info["solver"]["steps"])
            assert res.data.dtype == np.float32
            mine = FC.euler_steps(valid, grid.discretization, periodic, FC.GOLDEN_D, dt, n)
            assert np.array_equal(mine, res.data), f"euler {cid} {n} steps: the restatement differs from the reference in {int((mine != res.data).sum())} cells"
            out[f"euler/{cid}/{n}"] = res.data
    return out


plain = reference_results(False)
compiled = reference_results(True)
assert plain.keys() == compiled.keys()
for key in plain:
    assert np.array_equal(plain[key], compiled[key]), f"{key}: torch.compile changes the bits"
np.savez_compressed(HERE / "f32p.npz", **plain)
print({k: v.shape for k, v in plain.items()})
