"""Guard: the kernels of the implicit Euler / Crank-Nicolson solvers use no scratch memory when compiled for gfx950 (CPU-only check of
the built library's code-object metadata, like tests/test_kernel_resources.py): the stage sweeps that carry the fixed-point epilogue
(lap_march_kernel, mode LAP_STAGE = 10), the pointwise form of the iteration and the final sum of the convergence norm."""

from __future__ import annotations

import re

import pytest

from test_kernel_resources import LIB, LLVM_BIN, _kernel_metadata


def test_fixed_point_instances_have_no_scratch(tmp_path):
    if not LIB.exists() or not (LLVM_BIN / "llvm-objdump").exists():
        pytest.skip("built library or llvm tools not available")
    kernels = _kernel_metadata(tmp_path)
    stage = [(n, s, v) for n, s, v in kernels if re.search(r"lap_march_kernelI[df](?:Li\d+E){5}Li10E", n)]
    own = [(n, s, v) for n, s, v in kernels if "fixedpoint_" in n]
    assert len(stage) >= 8, "no LAP_STAGE instances of lap_march_kernel in the library's code objects"
    for needle in ("fixedpoint_combine_kernel", "fixedpoint_finish_kernel", "fixedpoint_begin_kernel", "fixedpoint_init_kernel"):
        assert any(needle in n for n, _, _ in own), f"no {needle} in the library's code objects"
    offenders = [(n, s) for n, s, _ in stage + own if s]
    assert not offenders, f"fixed-point kernels spilling to scratch: {offenders[:5]}"
