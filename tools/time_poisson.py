"""Timing of the Poisson solver on the device: milliseconds per conjugate-gradient iteration and iterations / wall time to a given
tolerance, all-Dirichlet faces, fp64, random right-hand side.  Prints a markdown table (profiles/poisson_time.md is one run of it).

    python tools/time_poisson.py [--sizes 256 512] [--rtol 1e-8] [--fixed 200]

Per size two solves on device-resident arrays: `--fixed` iterations with rtol = 0 (the solve ends in ConvergenceError by design: the
time is that of exactly that many iterations, batches of 32) and one solve to `--rtol`.  Bytes an iteration must move: 11 array passes
of 8 bytes per cell (sweep 1 reads r and writes w; sweep 2 reads r, w, p, q, x and writes p, q, x, r).
"""
from __future__ import annotations

import argparse
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "py-pde_amd")]

import pde_hip  # noqa: E402
from pde_hip.device import DeviceArray  # noqa: E402


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--rtol", type=float, default=1e-8)
    ap.add_argument("--fixed", type=int, default=200)
    args = ap.parse_args()
    backend = pde_hip.get_backend("hip")
    print(f"device: {backend.device_name}\n")
    print("| grid | ms / iteration | GB / iteration | TB/s | iterations to rtol | wall s to rtol | true residual / ||f - v|| |")
    print("|---|---|---|---|---|---|---|")
    for n in args.sizes:
        grid = pde_hip.UnitGrid([n, n, n])
        info = backend.grid_info(grid, np.float64)
        f = np.random.default_rng(n).uniform(-1, 1, grid.shape)
        rhs = DeviceArray(info).set_valid(f, backend.stream)
        out = DeviceArray(info)
        bc = {"value": 0.0}
        fixed = grid.make_operator("poisson_solver", bc, backend=backend, rtol=0.0, maxiter=args.fixed)
        per_iter = []
        for _ in range(3):      # the first call creates the handle
            backend.synchronize()
            t0 = time.perf_counter()
            try:
                fixed(rhs, out=out)
            except pde_hip.ConvergenceError:
                pass
            backend.synchronize()
            per_iter.append((time.perf_counter() - t0) / args.fixed * 1e3)
        ms = min(per_iter[1:])
        gb = 11 * 8 * n**3 / 1e9
        op = grid.make_operator("poisson_solver", bc, backend=backend, rtol=args.rtol)
        op(rhs, out=out)       # warm-up: handle
        backend.synchronize()
        t0 = time.perf_counter()
        op(rhs, out=out)
        backend.synchronize()
        wall = time.perf_counter() - t0
        u = pde_hip.ScalarField(grid, out.get_valid(stream=backend.stream))
        resid = np.linalg.norm((u.laplace(bc).data - f).ravel()) / np.linalg.norm(f.ravel())
        print(f"| {n}^3 | {ms:.3f} | {gb:.2f} | {gb / ms:.2f} | {op.info['iterations']} | {wall:.2f} | {resid:.2e} |", flush=True)


if __name__ == "__main__":
    main()
