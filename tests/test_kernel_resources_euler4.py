"""Guard: the four-step sweep keeps the resources its occupancy needs (CPU-only check of the built library's code-object metadata, like
tests/test_kernel_resources.py): no scratch; one workgroup of 768 threads per CU = three waves per SIMD, so at most 168 VGPR + AGPR per lane and
the LDS of its four plane buffers within the 160 KiB of a CU; both instances in both builds (exactv, fastv)."""

from __future__ import annotations

import re
import subprocess

import pytest

from test_kernel_resources import LIB, LLVM_BIN

LDS_BYTES = 4 * 42 * 76 * 8   # four levels x (40 + 2) rows x (72 + 4) cells (pdehip_euler4_plan.h)


def _euler4_metadata(tmp_path):
    """name -> the integer fields of the kernel's metadata note"""
    import shutil

    work = tmp_path / "lib.so"
    shutil.copy(LIB, work)
    subprocess.run([str(LLVM_BIN / "llvm-objdump"), "--offloading", str(work)], capture_output=True, text=True, check=True, timeout=300)
    out = {}
    for co in sorted(tmp_path.glob("lib.so.*gfx950*")):
        notes = subprocess.run([str(LLVM_BIN / "llvm-readelf"), "--notes", str(co)], capture_output=True, text=True, check=True, timeout=300).stdout
        for block in notes.split("- .agpr_count")[1:]:
            block = ".agpr_count" + block
            name = re.search(r"\.name:\s+(\S+)", block)
            if name and "euler4_kernel" in name.group(1):
                out[name.group(1)] = {k: int(v) for k, v in re.findall(r"\.(\w+):\s+(\d+)\s*$", block.split("- .agpr_count")[0], flags=re.M)}
    return out


def test_euler4_kernel_resources(tmp_path):
    if not LIB.exists() or not (LLVM_BIN / "llvm-objdump").exists():
        pytest.skip("built library or llvm tools not available")
    kernels = _euler4_metadata(tmp_path)
    for ns in ("exactv", "fastv"):
        for m2 in ("Li0E", "Li6E"):   # E2_DIFFUSION, E2_DIFFUSION_UNIT
            assert any(ns in n and f"euler4_kernelId{m2}" in n for n in kernels), (ns, m2, sorted(kernels))
    assert len(kernels) == 4
    for name, md in kernels.items():
        assert md["private_segment_fixed_size"] == 0, (name, md)
        assert md["max_flat_workgroup_size"] == 768, (name, md)
        assert md["vgpr_count"] + md["agpr_count"] <= 168, (name, md)   # three waves per SIMD
        assert md["group_segment_fixed_size"] == LDS_BYTES <= 160 * 1024, (name, md)
