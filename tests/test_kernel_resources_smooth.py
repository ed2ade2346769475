"""Guard: the smoothing kernels (csrc/pdehip_smooth.hip) as compiled for gfx950 (CPU-only check of the built library's code-object
metadata, like tests/test_kernel_resources_project.py): every instance is there for double and float, none uses scratch memory, none
needs more than 128 vector registers (latency-bound streaming kernels: at least 4 waves per SIMD of the 512-register file), none takes
more than 80 KiB of LDS per workgroup (two workgroups in the 160 KiB of a CU; the tiles are sized for four)."""

from __future__ import annotations

import re
import subprocess

import pytest

from test_kernel_resources import LIB, LLVM_BIN, _kernel_metadata

# kernel -> instances: rows and cells for the two types; the march for fp64 (one cell, pairs) and fp32 (one cell, quads)
OWN = {"gauss_row_kernel": 2, "gauss_march_kernel": 4, "gauss_cell_kernel": 2}
TYPES = {"gauss_row_kernel": ("IdE", "IfE"), "gauss_march_kernel": ("IdLi1E", "IdLi2E", "IfLi1E", "IfLi4E"), "gauss_cell_kernel": ("IdE", "IfE")}


def test_smoothing_kernels_resources(tmp_path):
    if not LIB.exists() or not (LLVM_BIN / "llvm-objdump").exists():
        pytest.skip("built library or llvm tools not available")
    kernels = _kernel_metadata(tmp_path)
    own = [(n, s, v) for n, s, v in kernels if any(k in n for k in OWN)]
    for needle, count in OWN.items():
        found = sorted(n for n, _, _ in own if needle in n)
        assert len(found) == count, f"{needle}: {len(found)} instances, expected {count}: {found}"
        for tag in TYPES[needle]:
            assert any(needle + tag in n for n in found), f"{needle}: no instance {tag}: {found}"
    offenders = [(n, s) for n, s, _ in own if s]
    assert not offenders, f"smoothing kernels spilling to scratch: {offenders[:5]}"
    print(sorted((v, n) for n, _, v in own))
    assert max(v for _, _, v in own) <= 128, sorted((v, n) for n, _, v in own)[-3:]


def test_smoothing_kernels_lds(tmp_path):
    """``.group_segment_fixed_size`` of every instance in the code object's notes: at most 80 KiB, and the LDS instances do use LDS."""
    if not LIB.exists() or not (LLVM_BIN / "llvm-objdump").exists():
        pytest.skip("built library or llvm tools not available")
    _kernel_metadata(tmp_path)      # (unbundles the code objects into tmp_path)
    sizes = {}
    for co in sorted(tmp_path.glob("lib.so.*gfx950*")):
        notes = subprocess.run([str(LLVM_BIN / "llvm-readelf"), "--notes", str(co)], capture_output=True, text=True, check=True, timeout=300).stdout
        for block in notes.split("- .agpr_count")[1:]:
            name = re.search(r"\.name:\s+(\S+)", block)
            lds = re.search(r"\.group_segment_fixed_size:\s+(\d+)", block)
            if name and lds and any(k in name.group(1) for k in OWN):
                sizes[name.group(1)] = int(lds.group(1))
    assert len(sizes) == sum(OWN.values()), sorted(sizes)
    print(sorted(sizes.items()))
    assert max(sizes.values()) <= 80 * 1024
    assert all((size > 0) == ("gauss_cell_kernel" not in name) for name, size in sizes.items()), sizes
