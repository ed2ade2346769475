"""Golden solutions of the reference's `solve_poisson_equation` on all-periodic grids with power-of-two extents (run in the build
container; needs the reference, `PDEHIP_REFERENCE` or /root/reference): the grids `method="fft"` of pde_hip/poisson.py takes.

The matrix is singular there, so the reference goes through lsmr and its `allclose` test (pde/backends/scipy/operators/common.py:112-141).
Recorded: case definitions (JSON), right-hand sides, solutions, or the message of the error.  As in make_golden_poisson.py the script
asserts that no recorded case sits near the `allclose` decision.

    python tests/golden/make_golden_poisson_fft.py   ->  tests/golden/poisson_fft.npz
"""
from __future__ import annotations

import json
import os
import sys
import warnings
from pathlib import Path

import numpy as np

sys.path.insert(0, os.environ.get("PDEHIP_REFERENCE") or "/root/reference")
warnings.filterwarnings("ignore")
import pde  # noqa: E402

HERE = Path(__file__).resolve().parent

CASES = [
    {"id": "1d-32", "shape": [32], "bounds": [[0, 8.0]], "periodic": [True], "bc": "periodic", "rhs": "zero-mean"},
    {"id": "2d-16x8", "shape": [16, 8], "bounds": [[0, 12.0], [0, 12.0]], "periodic": [True, True], "bc": "periodic", "rhs": "zero-mean"},
    {"id": "3d-8x4x8", "shape": [8, 4, 8], "bounds": [[0, 4.0], [0, 5.0], [0, 16.0]], "periodic": [True, True, True], "bc": "periodic", "rhs": "zero-mean"},
    {"id": "2d-16x8-nonzero-mean", "shape": [16, 8], "bounds": [[0, 12.0], [0, 12.0]], "periodic": [True, True], "bc": "periodic", "rhs": "shifted",
     "raises": True},
]


def main():
    from pde.backends.scipy.operators.cartesian import _get_laplace_matrix
    from scipy import sparse

    rng = np.random.default_rng(43)
    out = {"cases": json.dumps(CASES)}
    for case in CASES:
        grid = pde.CartesianGrid(case["bounds"], case["shape"], periodic=case["periodic"])
        data = rng.uniform(-1, 1, grid.shape)
        data += (1.0 if case["rhs"] == "shifted" else 0.0) - data.mean()
        rhs = pde.ScalarField(grid, data)
        out[f"{case['id']}/rhs"] = data
        out[f"{case['id']}/dx"] = np.asarray(grid.discretization)
        matrix, vector = _get_laplace_matrix(grid.get_boundary_conditions(case["bc"]))
        b = data.ravel() - vector.toarray()[:, 0]
        if case.get("raises"):
            try:
                pde.solve_poisson_equation(rhs, case["bc"])
            except RuntimeError as err:
                out[f"{case['id']}/message"] = str(err)
                x = sparse.linalg.lsmr(matrix.tocsc(), b)[0]
                excess = np.abs(matrix @ x - b) - (1e-5 + 1e-5 * np.abs(b))
                assert excess.max() > 100 * 1e-5, (case["id"], excess.max())
            else:
                raise AssertionError(f"{case['id']}: the reference was expected to raise")
            continue
        res = pde.solve_poisson_equation(rhs, case["bc"])
        slack = np.abs(matrix @ res.data.ravel() - b) / (1e-5 + 1e-5 * np.abs(b))
        assert slack.max() < 1e-2, (case["id"], slack.max())
        out[f"{case['id']}/solution"] = res.data
        out[f"{case['id']}/label"] = str(res.label)
        print(case["id"], "dx", grid.discretization, "max |u|", float(np.abs(res.data).max()), "allclose slack", float(slack.max()))
    np.savez_compressed(HERE / "poisson_fft.npz", **out)


if __name__ == "__main__":
    main()
