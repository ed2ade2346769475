"""Guard: the kernels of the Poisson solver use no scratch memory when compiled for gfx950 (CPU-only check of the built library's
code-object metadata, like tests/test_kernel_resources_fixedpoint.py): the stencil sweep with the two dot products, the pointwise
update, the one-workgroup kernel behind the sweep and the kernels around a solve.  The stage sweeps of lap_march_kernel are checked
too: a conjugate-gradient epilogue inside them was tried and cost some of them scratch, which is why sweep 1 is a kernel of its own."""

from __future__ import annotations

import re

import pytest

from test_kernel_resources import LIB, LLVM_BIN, _kernel_metadata

# every kernel of the solver: the loop both methods share, the kernels around a solve, the multigrid cycle
OWN = ("poisson_update_kernel", "poisson_finish_kernel", "poisson_apply_kernel", "poisson_rhs_kernel", "poisson_reduce_kernel",
       "poisson_check_kernel", "poisson_store_kernel", "poisson_shift_kernel", "poisson_sum_kernel", "poisson_init_kernel",
       "poisson_mg_smooth0_kernel", "poisson_mg_sweep_kernel", "poisson_mg_restrict_kernel", "poisson_mg_prolong_kernel",
       "poisson_mg_coarse_kernel", "poisson_mg_face_kernel", "poisson_mg_apply_kernel", "poisson_mg_open_kernel")


def test_poisson_instances_have_no_scratch(tmp_path):
    if not LIB.exists() or not (LLVM_BIN / "llvm-objdump").exists():
        pytest.skip("built library or llvm tools not available")
    kernels = _kernel_metadata(tmp_path)
    stage = [(n, s, v) for n, s, v in kernels if re.search(r"lap_march_kernelI[df](?:Li\d+E){5}Li10E", n)]
    own = [(n, s, v) for n, s, v in kernels if "poisson_" in n]
    assert len(stage) >= 8, "no LAP_STAGE instances of lap_march_kernel in the library's code objects"
    for needle in OWN:
        assert any(needle in n for n, _, _ in own), f"no {needle} in the library's code objects"
    offenders = [(n, s) for n, s, _ in stage + own if s]
    assert not offenders, f"kernels of the Poisson solver spilling to scratch: {offenders[:5]}"
