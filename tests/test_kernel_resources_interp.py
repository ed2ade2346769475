"""Guard: the interpolation kernels use no scratch memory when compiled for gfx950 (CPU-only check of the built library's code-object
metadata, like tests/test_kernel_resources_poisson.py): the point kernel, the table and row kernels of regridding and the kernel of the
edge and corner ghost cells, in every instance (fp64 / fp32, 1 to 3 axes)."""

from __future__ import annotations

import pytest

from test_kernel_resources import LIB, LLVM_BIN, _kernel_metadata

OWN = ("interp_points_kernel", "regrid_tables_kernel", "regrid_kernel", "ghost_corners_kernel")


def test_interpolation_kernels_have_no_scratch(tmp_path):
    if not LIB.exists() or not (LLVM_BIN / "llvm-objdump").exists():
        pytest.skip("built library or llvm tools not available")
    kernels = _kernel_metadata(tmp_path)
    own = [(n, s, v) for n, s, v in kernels if any(k in n for k in OWN)]
    for needle in OWN:
        assert any(needle in n for n, _, _ in own), f"no {needle} in the library's code objects"
    assert sum("interp_points_kernel" in n for n, _, _ in own) == 6 and sum("regrid_kernel" in n for n, _, _ in own) == 6
    offenders = [(n, s) for n, s, _ in own if s]
    assert not offenders, f"interpolation kernels spilling to scratch: {offenders[:5]}"
    assert max(v for _, _, v in own) <= 128, "the gather kernels keep four waves per SIMD"
