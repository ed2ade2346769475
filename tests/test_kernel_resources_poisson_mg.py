"""Guard: the kernels of the multigrid-preconditioned Poisson solver are in the gfx950 code objects of the built library and use no
scratch memory (CPU-only check of the code-object metadata, like tests/test_kernel_resources_poisson.py, whose list of the solver's
kernels it shares), in one instance per access width - and per loop form for the update the two loops share; the stage sweeps of
lap_march_kernel still use none."""

from __future__ import annotations

import re

import pytest

from test_kernel_resources import LIB, LLVM_BIN, _kernel_metadata
from test_kernel_resources_poisson import OWN


def test_solver_kernels_are_built_per_width_and_loop_form_without_scratch(tmp_path):
    if not LIB.exists() or not (LLVM_BIN / "llvm-objdump").exists():
        pytest.skip("built library or llvm tools not available")
    kernels = _kernel_metadata(tmp_path)
    own = [(n, s) for n, s, _ in kernels if "poisson_" in n]
    stage = [(n, s) for n, s, _ in kernels if re.search(r"lap_march_kernelI[df](?:Li\d+E){5}Li10E", n)]
    for needle in OWN:
        assert any(needle in n for n, _ in own), f"no {needle} in the library's code objects"
    for needle in ("poisson_mg_smooth0_kernel", "poisson_mg_sweep_kernel", "poisson_mg_restrict_kernel", "poisson_mg_apply_kernel", "poisson_apply_kernel"):
        assert len([n for n, _ in own if needle in n]) == 2, f"{needle}: one instance per access width expected"
    assert len([n for n, _ in own if "poisson_update_kernel" in n]) == 4, "poisson_update_kernel: one instance per access width and loop form expected"
    assert len([n for n, _ in own if "poisson_finish_kernel" in n]) == 2, "poisson_finish_kernel: one instance per loop form expected"
    assert len(stage) >= 8
    offenders = [(n, s) for n, s in own + stage if s]
    assert not offenders, f"kernels spilling to scratch: {offenders[:5]}"
