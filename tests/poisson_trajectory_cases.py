"""The cases of tests/test_hip_poisson_trajectory.py (device against the restated loops, iteration by iteration) and the CPU side of
their tolerances: `restated` runs the restatement of a case (tests/poisson_cases.py `cg`, tests/poisson_mg_cases.py `mgcg`) with one
of its two summation modes, `spread` measures how far the two modes drift apart, `python tests/poisson_trajectory_cases.py` prints
the table of the test module's docstring and the `TOL` dictionary below.

Each shape is there for a path of the launch geometry (csrc/pdehip_sweep.h: 256 threads per workgroup, at most 8192 workgroups, two
cells per thread where the fastest axis is even):
  1-D 1, 2, 3 cells        rows shorter than a wave, an axis of extent 1 / 2
  1-D 257, 2-D 33 x 31     one cell per thread with a ragged last workgroup
  1-D 1 000 001            ONE long row with one cell per thread: 3907 workgroups, a ragged last one (below the cap, which takes
                           2 097 152 cells of such a row: the seeded fault at the cap does not touch this case)
  5 x 1, 64 x 2 (periodic) a fastest axis of extent 1; a periodic axis of extent 2, both neighbours the same cell
  2048 x 2050              two cells per thread just above the cap (2 099 200 pieces)
  16 x 2 x 18              the middle axis periodic with extent 2
  129 x 128 x 129          2 130 048 cells, one per thread: above the cap
  160 x 160 x 168          2 150 400 pieces of two cells: above the cap
"""

from __future__ import annotations

import functools

import numpy as np

if __name__ == "__main__":      # run as a script: the paths tests/conftest.py sets up
    import sys
    from pathlib import Path

    _root = Path(__file__).resolve().parent.parent
    sys.path[:0] = [str(_root), str(_root / "py-pde_amd"), str(_root / "tests")]

import pde_hip
from poisson_cases import FACES1, FACES2, FACES3, MIXED, cg
from poisson_mg_cases import mgcg

NEUMANN = {"derivative": 0.0}
KS = (1, 2, 5)
EPS = float(np.finfo(np.float64).eps)
FLOOR = 4 * EPS      # 4 ulp: of max|x_k| for an iterate; of the norm of the right-hand side for a residual (alpha one ulp off moves r_k = r - alpha q by that much)

# id -> (shape, periodic, bc, singular)
SHAPES = {
    "1d-1": ([1], [False], FACES1, False),
    "1d-2": ([2], [False], FACES1, False),
    "1d-3": ([3], [False], FACES1, False),
    "1d-64": ([64], [False], FACES1, False),
    "1d-257": ([257], [False], FACES1, False),
    "1d-1000001": ([1000001], [False], FACES1, False),
    "2d-5x1": ([5, 1], [False, False], FACES2, False),
    "2d-64x2-periodic": ([64, 2], [False, True], [[{"value": 0.5}, MIXED], "periodic"], False),
    "2d-33x31": ([33, 31], [False, False], {"value": 0.0}, False),
    "2d-40x51": ([40, 51], [True, False], ["periodic", {"value": 0.3}], False),
    "2d-2048x2050": ([2048, 2050], [False, False], FACES2, False),
    "3d-24x20x32-faces": ([24, 20, 32], [False, False, True], FACES3, False),
    "3d-16x2x18-periodic": ([16, 2, 18], [False, True, False], [{"value": 0.5}, "periodic", {"derivative": 0.1}], False),
    "3d-3x3x3": ([3, 3, 3], [False, False, False], [[{"value": 0.5}, MIXED], {"value": 1.0}, {"derivative": 0.1}], False),
    "3d-129x128x129": ([129, 128, 129], [False, False, True], FACES3, False),
    "3d-160x160x168": ([160, 160, 168], [False, False, True], FACES3, False),
    "3d-24x20x32-all-periodic": ([24, 20, 32], [True, True, True], "periodic", True),
    "3d-24x21x32-neumann-periodic": ([24, 21, 32], [False, True, False], [NEUMANN, "periodic", NEUMANN], True),
    "3d-129x128x129-neumann-periodic": ([129, 128, 129], [False, True, True], [NEUMANN, "periodic", "periodic"], True),
}
BIG = 1_000_000      # cells from which the restatement of a whole solve is too slow for a test, with the exceptions of COUNTED
SPIKES = ("spike-last", "spike-first", "spike-end-of-first-row")
# Iteration counts to rtol = 1e-8 are compared on every case below BIG cells and on these preconditioned cases above the cap of 8192
# workgroups (one cell per thread, two cells per thread, a singular system whose sum, shift and check kernels run after convergence).
# What is left out, case by case (restatement on one core of the build machine):
#   1d-1000001 cg                 conjugate gradients on a 1-D row need about as many iterations as it has cells: 10^6 passes
#   1d-1000001 mgcg               the extent is odd: one level of 10^6 cells, 32 Jacobi sweeps per cycle; the residual is 0.39 of the
#                                 right-hand side after 20 restated iterations: no convergence within the method's 200
#   2d-2048x2050 mgcg             does not converge within the method's 200 iterations (spacings 1 : 0.5, residual 3e-3 of the
#                                 right-hand side after 200 restated iterations, which take 120 s)
#   2d-2048x2050, 3d-129x128x129, 3d-160x160x168, 3d-129x128x129-neumann-periodic with cg
#                                 several hundred to some thousand iterations of 0.2 - 0.5 s each: minutes per case
COUNTED = ("3d-129x128x129/random/f64/mgcg", "3d-160x160x168/random/f64/mgcg", "3d-129x128x129-neumann-periodic/random/f64/mgcg")


def _case(sid, rhs="random", dtype="f64", method="cg", ks=KS):
    cells = int(np.prod(SHAPES[sid][0]))
    # conjugate gradients end after at most `cells` updates: beyond cells - 1 an iterate is rounding noise around the solution
    ks = tuple(k for k in ks if k < cells) or (1,)
    cid = f"{sid}/{rhs}/{dtype}/{method}"
    return {"id": cid, "shape_id": sid, "rhs": rhs, "dtype": dtype, "method": method, "ks": tuple(ks), "converge": cells < BIG or cid in COUNTED, "cells": cells}


def _all_cases():
    out = []
    for sid in SHAPES:
        out.append(_case(sid))
        out.append(_case(sid, method="mgcg"))
    # a right-hand side that is zero but for ONE cell at a tail of the row loop: a piece dropped there changes x_1 in the first digit
    for sid in ("1d-3", "1d-257", "1d-1000001", "2d-5x1", "2d-33x31", "2d-2048x2050", "3d-3x3x3", "3d-16x2x18-periodic", "3d-129x128x129", "3d-160x160x168"):
        for rhs in SPIKES:
            out.append(_case(sid, rhs=rhs, ks=(1, 2) if int(np.prod(SHAPES[sid][0])) < BIG else (1,)))
    for sid in ("2d-33x31", "3d-160x160x168"):
        out.append(_case(sid, rhs="spike-last", method="mgcg", ks=(1,)))
    for sid in ("1d-257", "2d-40x51", "3d-24x20x32-faces", "3d-24x21x32-neumann-periodic"):
        out.append(_case(sid, dtype="f32"))
        out.append(_case(sid, dtype="f32", method="mgcg"))
    return out


CASES = _all_cases()
CASE_BY_ID = {c["id"]: c for c in CASES}


def make_grid(sid):
    shape, periodic, _, _ = SHAPES[sid]
    # spacings 1 : 0.5 : 2 like the large-grid tests: a transposed scale shows
    return pde_hip.CartesianGrid([[0, n * s] for n, s in zip(shape, (1.0, 0.5, 2.0))], shape, periodic=periodic)


def make_rhs(case) -> np.ndarray:
    shape, _, _, singular = SHAPES[case["shape_id"]]
    if case["rhs"] == "random":
        f = np.random.default_rng(case["cells"]).uniform(-1, 1, shape)
        if singular:
            f -= f.mean()      # (a consistent right-hand side: the converged solve passes the reference's acceptance test)
    else:
        f = np.zeros(shape)
        where = {"spike-last": (-1,) * len(shape), "spike-first": (0,) * len(shape), "spike-end-of-first-row": (0,) * (len(shape) - 1) + (-1,)}[case["rhs"]]
        f[where] = 1.0
    return f.astype(np.float32) if case["dtype"] == "f32" else f


@functools.lru_cache(maxsize=4)
def restated(cid: str, sums: str = "exact"):
    """The restated loop of case `cid` for as many updates as the largest k of the case, with rtol = atol = 0 like the device runs it
    compares with.  A `Trajectory` (iterates kept for the k of the case)."""
    case = CASE_BY_ID[cid]
    _, _, bc, singular = SHAPES[case["shape_id"]]
    solve = cg if case["method"] == "cg" else mgcg
    return solve(make_grid(case["shape_id"]), bc, make_rhs(case), rtol=0.0, atol=0.0, maxiter=max(case["ks"]), singular=singular, sums=sums, keep=set(case["ks"]))


CONVERGE_RTOL = 1e-8


def restated_count(cid: str, sums: str = "exact") -> int:
    """Iterations of the restated loop to rtol = 1e-8."""
    case = CASE_BY_ID[cid]
    shape, _, bc, singular = SHAPES[case["shape_id"]]
    solve = cg if case["method"] == "cg" else mgcg
    maxiter = 200 if case["method"] == "mgcg" else max(1000, 50 * max(shape))
    traj = solve(make_grid(case["shape_id"]), bc, make_rhs(case), rtol=CONVERGE_RTOL, atol=0.0, maxiter=maxiter, singular=singular, sums=sums, keep=())
    assert traj.status == 0, (cid, traj.status, traj.iterations)
    return traj.iterations


def demean(case, x):
    """Singular systems: the iterates are compared with their mean removed (the preconditioner may add a constant, which the matrix
    does not see; the device removes it only from a converged solution)."""
    return x - x.mean() if SHAPES[case["shape_id"]][3] else x


def residual_after(traj, k: int) -> float:
    """sqrt(r_k.r_k): the `residual` the device reports when `maxiter = k` stops it - rr of the stop test of iteration k + 1."""
    return float(np.sqrt(traj.scalars[k][2])) if k < len(traj.scalars) else traj.residual


def spread(cid: str) -> dict:
    """k -> (relative spread of x_k, of the residual after k updates) between the two summation modes; key 0: of the norm of the
    right-hand side.  The spread of a residual is taken relative to the residual, where that is above 4 ulp of the right-hand side."""
    case = CASE_BY_ID[cid]
    a, b = restated(cid, "exact"), restated(cid, "numpy")
    # (one cell: the first update is exact, r_1 = 0 and the loop ends converged instead of at maxiter)
    assert a.iterations == b.iterations == max(case["ks"]) and a.status == b.status and a.status in (0, 1), (cid, a.iterations, b.iterations, a.status, b.status)
    out = {0: (0.0, abs(a.rhs_norm - b.rhs_norm) / a.rhs_norm)}
    for k in case["ks"]:
        xa, xb = demean(case, a.iterates[k - 1]), demean(case, b.iterates[k - 1])
        ra, rb = residual_after(a, k), residual_after(b, k)
        out[k] = (float(np.abs(xa - xb).max() / np.abs(xa).max()), max(0.0, abs(ra - rb) - FLOOR * a.rhs_norm) / ra if ra else 0.0)
    return out


F32_ULP = 2.0 ** -23            # fp32 fields: x_k is compared after the cast, which moves a value by at most one ulp of fp32 more


def allowed(case, measured: dict) -> tuple[float, float]:
    """(relative error allowed on x_k, on residual and rhs_norm): 16 x the largest spread over the k of the case, at least 4 ulp."""
    tol_x = max(FLOOR, 16 * max(v[0] for v in measured.values()))
    tol_r = max(FLOOR, 16 * max(v[1] for v in measured.values()))
    return tol_x, tol_r


def measure(ids=None):
    rows = {}
    for case in CASES:
        if ids and case["id"] not in ids:
            continue
        restated.cache_clear()
        m = spread(case["id"])
        rows[case["id"]] = (max(v[0] for v in m.values()), max(v[1] for v in m.values()), *allowed(case, m))
        sx, sr, tx, tr = rows[case["id"]]
        print(f"  {case['id']:<48} {','.join(map(str, sorted(k for k in m if k))):<6} {sx:9.2e} {sr:9.2e} {tx:9.2e} {tr:9.2e} {0.1 / case['cells']:9.2e}", flush=True)
    return rows


# id -> (relative error allowed on x_k, on residual / rhs_norm): what `measure` printed (16 x the spread, at least 4 ulp)
TOL: dict[str, tuple[float, float]] = {
    "1d-1/random/f64/cg": (8.88e-16, 8.88e-16),
    "1d-1/random/f64/mgcg": (8.88e-16, 8.88e-16),
    "1d-2/random/f64/cg": (8.88e-16, 8.88e-16),
    "1d-2/random/f64/mgcg": (8.88e-16, 8.88e-16),
    "1d-3/random/f64/cg": (1.70e-15, 8.88e-16),
    "1d-3/random/f64/mgcg": (8.88e-16, 8.88e-16),
    "1d-64/random/f64/cg": (8.25e-15, 8.88e-16),
    "1d-64/random/f64/mgcg": (1.65e-13, 1.48e-13),
    "1d-257/random/f64/cg": (1.09e-14, 8.88e-16),
    "1d-257/random/f64/mgcg": (1.55e-14, 8.88e-16),
    "1d-1000001/random/f64/cg": (9.30e-14, 8.69e-14),
    "1d-1000001/random/f64/mgcg": (1.11e-13, 1.21e-13),
    "2d-5x1/random/f64/cg": (1.79e-15, 8.88e-16),
    "2d-5x1/random/f64/mgcg": (3.57e-15, 8.88e-16),
    "2d-64x2-periodic/random/f64/cg": (1.18e-14, 8.88e-16),
    "2d-64x2-periodic/random/f64/mgcg": (1.37e-14, 8.88e-16),
    "2d-33x31/random/f64/cg": (5.97e-15, 8.88e-16),
    "2d-33x31/random/f64/mgcg": (8.88e-16, 8.88e-16),
    "2d-40x51/random/f64/cg": (9.05e-15, 8.88e-16),
    "2d-40x51/random/f64/mgcg": (4.51e-15, 8.88e-16),
    "2d-2048x2050/random/f64/cg": (7.75e-14, 5.24e-15),
    "2d-2048x2050/random/f64/mgcg": (5.28e-14, 5.91e-14),
    "3d-24x20x32-faces/random/f64/cg": (5.41e-15, 8.88e-16),
    "3d-24x20x32-faces/random/f64/mgcg": (5.79e-15, 8.88e-16),
    "3d-16x2x18-periodic/random/f64/cg": (1.17e-14, 8.88e-16),
    "3d-16x2x18-periodic/random/f64/mgcg": (4.69e-15, 8.88e-16),
    "3d-3x3x3/random/f64/cg": (1.02e-14, 8.88e-16),
    "3d-3x3x3/random/f64/mgcg": (3.34e-15, 8.88e-16),
    "3d-129x128x129/random/f64/cg": (1.08e-14, 3.26e-15),
    "3d-129x128x129/random/f64/mgcg": (1.91e-14, 3.26e-15),
    "3d-160x160x168/random/f64/cg": (1.61e-14, 2.52e-15),
    "3d-160x160x168/random/f64/mgcg": (1.68e-14, 2.52e-15),
    "3d-24x20x32-all-periodic/random/f64/cg": (1.01e-14, 8.88e-16),
    "3d-24x20x32-all-periodic/random/f64/mgcg": (8.66e-15, 8.88e-16),
    "3d-24x21x32-neumann-periodic/random/f64/cg": (4.49e-15, 8.88e-16),
    "3d-24x21x32-neumann-periodic/random/f64/mgcg": (4.73e-15, 8.88e-16),
    "3d-129x128x129-neumann-periodic/random/f64/cg": (1.28e-14, 2.16e-15),
    "3d-129x128x129-neumann-periodic/random/f64/mgcg": (2.42e-14, 2.16e-15),
    "1d-3/spike-last/f64/cg": (4.17e-15, 8.88e-16),
    "1d-3/spike-first/f64/cg": (8.88e-16, 8.88e-16),
    "1d-3/spike-end-of-first-row/f64/cg": (4.17e-15, 8.88e-16),
    "1d-257/spike-last/f64/cg": (8.88e-16, 8.88e-16),
    "1d-257/spike-first/f64/cg": (1.80e-15, 8.88e-16),
    "1d-257/spike-end-of-first-row/f64/cg": (8.88e-16, 8.88e-16),
    "1d-1000001/spike-last/f64/cg": (8.88e-16, 8.88e-16),
    "1d-1000001/spike-first/f64/cg": (8.88e-16, 8.88e-16),
    "1d-1000001/spike-end-of-first-row/f64/cg": (8.88e-16, 8.88e-16),
    "2d-5x1/spike-last/f64/cg": (8.88e-16, 3.25e-15),
    "2d-5x1/spike-first/f64/cg": (3.83e-15, 8.88e-16),
    "2d-5x1/spike-end-of-first-row/f64/cg": (3.83e-15, 8.88e-16),
    "2d-33x31/spike-last/f64/cg": (8.88e-16, 8.88e-16),
    "2d-33x31/spike-first/f64/cg": (8.88e-16, 8.88e-16),
    "2d-33x31/spike-end-of-first-row/f64/cg": (8.88e-16, 8.88e-16),
    "2d-2048x2050/spike-last/f64/cg": (2.95e-13, 2.45e-13),
    "2d-2048x2050/spike-first/f64/cg": (2.95e-13, 1.90e-13),
    "2d-2048x2050/spike-end-of-first-row/f64/cg": (2.96e-13, 1.95e-13),
    "3d-3x3x3/spike-last/f64/cg": (7.21e-15, 3.19e-15),
    "3d-3x3x3/spike-first/f64/cg": (4.91e-15, 8.88e-16),
    "3d-3x3x3/spike-end-of-first-row/f64/cg": (4.91e-15, 8.88e-16),
    "3d-16x2x18-periodic/spike-last/f64/cg": (3.61e-15, 3.35e-15),
    "3d-16x2x18-periodic/spike-first/f64/cg": (3.61e-15, 3.35e-15),
    "3d-16x2x18-periodic/spike-end-of-first-row/f64/cg": (3.61e-15, 3.35e-15),
    "3d-129x128x129/spike-last/f64/cg": (1.00e-14, 1.05e-14),
    "3d-129x128x129/spike-first/f64/cg": (2.50e-15, 7.03e-15),
    "3d-129x128x129/spike-end-of-first-row/f64/cg": (2.50e-15, 7.03e-15),
    "3d-160x160x168/spike-last/f64/cg": (5.25e-14, 1.66e-14),
    "3d-160x160x168/spike-first/f64/cg": (4.50e-14, 1.66e-14),
    "3d-160x160x168/spike-end-of-first-row/f64/cg": (4.50e-14, 1.66e-14),
    "2d-33x31/spike-last/f64/mgcg": (8.88e-16, 8.88e-16),
    "3d-160x160x168/spike-last/f64/mgcg": (4.68e-15, 1.66e-14),
    "1d-257/random/f32/cg": (4.35e-15, 8.88e-16),
    "1d-257/random/f32/mgcg": (1.86e-14, 8.88e-16),
    "2d-40x51/random/f32/cg": (1.06e-14, 8.88e-16),
    "2d-40x51/random/f32/mgcg": (4.51e-15, 8.88e-16),
    "3d-24x20x32-faces/random/f32/cg": (5.41e-15, 8.88e-16),
    "3d-24x20x32-faces/random/f32/mgcg": (2.90e-15, 8.88e-16),
    "3d-24x21x32-neumann-periodic/random/f32/cg": (4.49e-15, 8.88e-16),
    "3d-24x21x32-neumann-periodic/random/f32/mgcg": (4.73e-15, 8.88e-16),
}


TINY = 1e-12      # a residual below this part of the right-hand side is rounding noise: the loop has solved the system (one cycle on a
                  # grid of a few cells is nearly an exact solve) and the number says nothing about a dot product


def residual_bound(tol_r: float, rhs_norm: float, residual: float) -> float | None:
    """The relative error allowed on a residual, floor included: tol_r + 4 ulp of the right-hand side in units of the residual; the
    tests hold it below 0.1 / cells.  None for a residual that is noise (`TINY`): there only the floor itself is asserted."""
    return None if residual <= TINY * rhs_norm else tol_r + FLOOR * rhs_norm / residual


def tolerance(case) -> tuple[float, float]:
    tol_x, tol_r = (max(t, FLOOR) for t in TOL[case["id"]])      # (the table prints three digits: 8.88e-16 is the floor)
    return (tol_x + F32_ULP if case["dtype"] == "f32" else tol_x), tol_r


# ---- the CPU checks of the table (tests/test_poisson_cpu.py: "cg", tests/test_poisson_mg_cpu.py: "mgcg") ----------------------------
def check_tolerances(method):
    """Every allowed error of the device tests is below 0.1 / cells, the floor of the residual included; the table entry IS 16 x the
    spread measured here (three printed digits: 1 % of slack), so a widened entry fails; and the restatement's own second summation
    mode stays inside it."""
    for case in CASES:
        if case["method"] != method:
            continue
        cid = case["id"]
        tol_x, tol_r = tolerance(case)
        assert max(tol_x, tol_r) < 0.1 / case["cells"], cid
        worst = spread(cid)
        exact = restated(cid, "exact")
        for k in case["ks"]:
            res = residual_after(exact, k)
            bound = residual_bound(tol_r, exact.rhs_norm, res)
            assert bound is None or bound < 0.1 / case["cells"], (cid, k)
        restated.cache_clear()
        spread_x, spread_r = max(v[0] for v in worst.values()), max(v[1] for v in worst.values())
        assert spread_x <= TOL[cid][0] and spread_r <= TOL[cid][1], (cid, worst)
        assert TOL[cid][0] <= 1.01 * max(FLOOR, 16 * spread_x) and TOL[cid][1] <= 1.01 * max(FLOOR, 16 * spread_r), (cid, worst, TOL[cid])


def check_equal_iteration_counts(method):
    for case in CASES:
        if case["converge"] and case["method"] == method:
            assert restated_count(case["id"], "exact") == restated_count(case["id"], "numpy") > 0, case["id"]


if __name__ == "__main__":
    measured = measure(set(sys.argv[1:]))
    print("TOL = {")
    for cid, (_, _, tx, tr) in measured.items():
        print(f"    {cid!r}: ({tx:.2e}, {tr:.2e}),")
    print("}")
