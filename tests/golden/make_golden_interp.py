"""Writes tests/golden/interp.npz: full arrays - face, edge and corner ghost cells - that the REFERENCE's numpy
``BoundariesList.set_ghost_cells(data_full, set_corners=True)`` (pde/grids/boundaries/axes.py:458-501) produces for the small fields of
``interp_cases.GOLDEN_CASES``.  Needs the reference py-pde on the path (no numba); run from the repository root:

    python tests/golden/make_golden_interp.py <path to the reference>
"""

from __future__ import annotations

import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))
sys.path.append(sys.argv[1])

import pde  # noqa: E402
from interp_cases import GOLDEN_BOUNDS, GOLDEN_CASES, field_data  # noqa: E402

out = {}
for cid, shape, periodic, bc in GOLDEN_CASES:
    grid = pde.CartesianGrid(GOLDEN_BOUNDS[len(shape)], shape, periodic=list(periodic))
    valid = field_data(shape, seed=len(cid))
    full = np.zeros(tuple(n + 2 for n in shape))
    full[(slice(1, -1),) * len(shape)] = valid
    grid.get_boundary_conditions(bc).set_ghost_cells(full, set_corners=True)
    out[cid + "/valid"] = valid
    out[cid + "/full"] = full
np.savez_compressed(HERE / "interp.npz", **out)
print({k: v.shape for k, v in out.items()})
