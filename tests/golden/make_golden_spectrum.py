"""Writes tests/golden/spectrum.npz: what the REFERENCE's own ``spectral_density`` (tests/tools/test_spectral.py:13-37: the wave-vector
magnitudes from ``fftfreq`` and ``|fftn(data) / data.size|**2 / prod(dx)``) gives for the small fields of ``spectrum_cases.GOLDEN`` - per
case the input, the discretisation, \\|k\\| and the density on the full frequency grid, as data only.  Needs the reference py-pde with its
tests and scipy; run from the repository root:

    python tests/golden/make_golden_spectrum.py <path to the reference>
"""

from __future__ import annotations

import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))
sys.path.insert(0, str(HERE.parent.parent / "py-pde_amd"))
sys.path.append(sys.argv[1])
sys.path.append(str(Path(sys.argv[1]) / "tests" / "tools"))

from spectrum_cases import GOLDEN, golden_input  # noqa: E402
from test_spectral import spectral_density  # noqa: E402

out = {}
for name, (shape, dx) in GOLDEN.items():
    data = golden_input(name)
    k, density = spectral_density(data, dx=list(dx))
    assert k.shape == density.shape == tuple(shape)
    out[f"{name}/data"], out[f"{name}/dx"], out[f"{name}/k"], out[f"{name}/density"] = data, np.array(dx), k, density
    print(name, shape, dx, "largest |k|", k.max(), "total", density.sum())
np.savez_compressed(HERE / "spectrum.npz", **out)
print((HERE / "spectrum.npz").stat().st_size, "bytes")
