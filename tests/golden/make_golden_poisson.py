"""Golden solutions of the reference's `poisson_solver` (run in the build container; needs /root/reference).

`pde.solve_poisson_equation` / `pde.solve_laplace_equation` (pde/pdes/laplace.py:28-125) with the scipy backend's sparse solver
(pde/backends/scipy/operators/common.py:71-146): spsolve for regular systems, lsmr for the singular ones (every face periodic or
Neumann), RuntimeError when the least-squares solution fails `allclose(A x, rhs, rtol=1e-5, atol=1e-5)`.  Recorded: case definitions
(JSON), right-hand sides, solutions, or the message of the error.  The script asserts that no recorded case sits near that `allclose`
decision: accepted solutions satisfy it with a factor 100 to spare, the refused one violates it by a factor 100.

    python tests/golden/make_golden_poisson.py   ->  tests/golden/poisson.npz
"""
from __future__ import annotations

import json
import sys
import warnings
from pathlib import Path

import numpy as np

sys.path.insert(0, "/root/reference")
warnings.filterwarnings("ignore")
import pde  # noqa: E402

HERE = Path(__file__).resolve().parent

MIXED = {"type": "mixed", "value": 0.8, "const": 0.3}
CASES = [
    {"id": "1d-dirichlet", "shape": [64], "bounds": [[0, 64]], "periodic": [False], "bc": [{"value": 0.0}], "rhs": "random"},
    {"id": "1d-value-derivative", "shape": [64], "bounds": [[0, 8.0]], "periodic": [False], "bc": [[{"value": 1.5}, {"derivative": -0.4}]], "rhs": "random"},
    {"id": "2d-dx-walls", "shape": [48, 40], "bounds": [[0, 12.0], [0, 30.0]], "periodic": [False, False],
     "bc": [[{"value": 0.7}, {"derivative": 0.25}], [MIXED, {"value": -1.0}]], "rhs": "random"},
    {"id": "2d-dx-periodic-mixed", "shape": [48, 40], "bounds": [[0, 12.0], [0, 30.0]], "periodic": [True, False],
     "bc": ["periodic", [MIXED, {"derivative": 0.1}]], "rhs": "random"},
    {"id": "3d-dirichlet", "shape": [24, 20, 16], "bounds": [[0, 24], [0, 20], [0, 16]], "periodic": [False, False, False], "bc": {"value": 0.0}, "rhs": "random"},
    {"id": "3d-faces", "shape": [24, 20, 16], "bounds": [[0, 12.0], [0, 20.0], [0, 4.0]], "periodic": [True, False, False],
     "bc": ["periodic", [{"value": 0.5}, MIXED], [{"derivative": -0.2}, {"value": 2.0}]], "rhs": "random"},
    {"id": "2d-periodic-zero-mean", "shape": [48, 40], "bounds": [[0, 12.0], [0, 30.0]], "periodic": [True, True], "bc": ["periodic", "periodic"], "rhs": "zero-mean"},
    {"id": "3d-neumann-zero-mean", "shape": [12, 10, 8], "bounds": [[0, 12], [0, 10], [0, 8]], "periodic": [False, False, False],
     "bc": {"derivative": 0.0}, "rhs": "zero-mean"},
    {"id": "2d-periodic-nonzero-mean", "shape": [16, 12], "bounds": [[0, 16], [0, 12]], "periodic": [True, True], "bc": ["periodic", "periodic"],
     "rhs": "shifted", "raises": True},
    {"id": "2d-laplace", "shape": [32, 24], "bounds": [[0, 8.0], [0, 12.0]], "periodic": [False, False],
     "bc": [[{"value": 1.0}, {"value": -0.5}], [{"value": 0.25}, {"value": 2.0}]], "rhs": "laplace"},
]


def main():
    rng = np.random.default_rng(41)
    out = {"cases": json.dumps(CASES)}
    for case in CASES:
        grid = pde.CartesianGrid(case["bounds"], case["shape"], periodic=case["periodic"])
        data = rng.uniform(-1, 1, grid.shape)
        if case["rhs"] == "zero-mean":
            data -= data.mean()
        elif case["rhs"] == "shifted":
            data += 1.0 - data.mean()
        elif case["rhs"] == "laplace":
            data[...] = 0
        rhs = pde.ScalarField(grid, data)
        out[f"{case['id']}/rhs"] = data
        # the matrix form of the problem, to measure the distance from the `allclose` decision
        bcs = grid.get_boundary_conditions(case["bc"])
        from pde.backends.scipy.operators.cartesian import _get_laplace_matrix

        matrix, vector = _get_laplace_matrix(bcs)
        b = data.ravel() - vector.toarray()[:, 0]
        if case.get("raises"):
            try:
                pde.solve_poisson_equation(rhs, case["bc"])
            except RuntimeError as err:
                out[f"{case['id']}/message"] = str(err)
                from scipy import sparse

                x = sparse.linalg.lsmr(matrix.tocsc(), b)[0]
                excess = np.abs(matrix @ x - b) - (1e-5 + 1e-5 * np.abs(b))
                assert excess.max() > 100 * 1e-5, (case["id"], excess.max())
            else:
                raise AssertionError(f"{case['id']}: the reference was expected to raise")
            continue
        if case["rhs"] == "laplace":
            res = pde.solve_laplace_equation(grid, case["bc"])
        else:
            res = pde.solve_poisson_equation(rhs, case["bc"])
        x = res.data.ravel()
        slack = np.abs(matrix @ x - b) / (1e-5 + 1e-5 * np.abs(b))
        assert slack.max() < 1e-2, (case["id"], slack.max())
        out[f"{case['id']}/solution"] = res.data
        out[f"{case['id']}/label"] = str(res.label)
        print(case["id"], "max |u|", float(np.abs(res.data).max()), "allclose slack", float(slack.max()))
    np.savez_compressed(HERE / "poisson.npz", **out)


if __name__ == "__main__":
    main()
