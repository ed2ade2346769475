"""Writes tests/golden/smooth.npz: what the REFERENCE's own ``DataFieldBase.smooth`` (pde/fields/datafield_base.py:988-1035, scipy's
``gaussian_filter1d`` axis by axis) gives for the small fields of ``smooth_cases.GOLDEN``, the result after every axis (the same scipy call
on the result of the axis before; the last one is asserted to be the reference's result) and the weights of every axis as scipy computes
them.  fp32 fields are smoothed into an fp32 field (``out=``), so every pass rounds once to fp32.  Needs the reference py-pde and scipy;
run from the repository root:

    python tests/golden/make_golden_smooth.py <path to the reference>
"""

from __future__ import annotations

import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))
sys.path.insert(0, str(HERE.parent.parent / "py-pde_amd"))
sys.path.append(sys.argv[1])

import pde  # noqa: E402
from scipy import ndimage  # noqa: E402
from scipy.ndimage._filters import _gaussian_kernel1d  # noqa: E402
from smooth_cases import GOLDEN, golden_bounds, golden_input  # noqa: E402

out = {}
for cid, (cls, dtype, shape, periodic, dx, sigma) in GOLDEN.items():
    grid = pde.CartesianGrid(golden_bounds(cid), shape, periodic=list(periodic))
    assert np.allclose(grid.discretization, dx, rtol=1e-15), (cid, grid.discretization)
    field = getattr(pde, cls)(grid, golden_input(cid), dtype=dtype)
    assert field.data.dtype == np.dtype(dtype)
    result = field.smooth(sigma, out=field.copy())
    in_place = field.copy()
    assert in_place.smooth(sigma, out=in_place) is in_place and in_place.data.tobytes() == result.data.tobytes()
    stage, radii = field.data, []
    for axis in range(len(shape)):
        sigma_cells = sigma / grid.discretization[axis]
        nxt = np.empty_like(stage)
        ndimage.gaussian_filter1d(stage, sigma=sigma_cells, axis=axis - len(shape), output=nxt, mode="wrap" if periodic[axis] else "reflect")
        stage = nxt
        radius = int(4.0 * float(sigma_cells) + 0.5)
        out[f"{cid}/w{axis}"] = _gaussian_kernel1d(float(sigma_cells), 0, radius)[::-1][radius:].copy()
        out[f"{cid}/axis{axis}"] = stage
        radii.append(radius)
    assert stage.tobytes() == result.data.tobytes() and stage.dtype == result.data.dtype
    out[f"{cid}/out"] = result.data
    print(cid, shape, "radii", radii, result.data.dtype)
np.savez_compressed(HERE / "smooth.npz", **out)
print((HERE / "smooth.npz").stat().st_size, "bytes")
