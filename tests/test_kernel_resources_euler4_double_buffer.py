"""Guard: the four-step sweep with two barriers per phase keeps the resources its occupancy needs (CPU-only check of the built library's
code-object metadata, like tests/test_kernel_resources_euler4.py).  The second buffers of the images of levels 1 and 2 are dynamic LDS, asked
for at the launch: the static allocation stays the four images, and static plus dynamic fit the 160 KiB of a CU.  No scratch and at most
168 VGPR + AGPR per lane (three waves per SIMD) in all four instances: with two barriers instead of four the compiler is free to read
several levels ahead of the arithmetic, and must not pay for it with registers it does not have."""

from __future__ import annotations

import pytest

from test_kernel_resources import LIB, LLVM_BIN
from test_kernel_resources_euler4 import LDS_BYTES, _euler4_metadata

ALT_BYTES = 2 * (36 + 4 * 720 + 36) * 8   # two buffers: a guard run, four arrays of 720 doubles, a guard run (pdehip_euler4_plan.h)


def test_euler4_double_buffer_resources(tmp_path):
    if not LIB.exists() or not (LLVM_BIN / "llvm-objdump").exists():
        pytest.skip("built library or llvm tools not available")
    kernels = _euler4_metadata(tmp_path)
    assert len(kernels) == 4, sorted(kernels)
    for name, md in kernels.items():
        assert md["private_segment_fixed_size"] == 0, (name, md)                 # no scratch
        assert md["vgpr_count"] + md["agpr_count"] <= 168, (name, md)            # three waves per SIMD
        assert md["group_segment_fixed_size"] == LDS_BYTES == 102144, (name, md)   # the static part alone
        assert md["group_segment_fixed_size"] + ALT_BYTES <= 160 * 1024, (name, md)
