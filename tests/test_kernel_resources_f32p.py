"""Guard: the kernels of the pure-fp32 arithmetic mode (csrc/pdehip_f32p.inc) exist in the built library, once (exact build only), and keep the
resources their occupancy design needs (CPU-only check of the code-object metadata, like tests/test_kernel_resources_euler4.py):

* no scratch in any of them;
* ``euler32_kernel`` (two steps per sweep): three level-0 planes of R + 4 rows and three level-1 planes of R + 2 rows of four cells per lane
  (152 data registers at R = 4) - designed for TWO waves per SIMD, i.e. at most 256 VGPR + AGPR per lane; its LDS is the exchange of the
  level-1 cells at the chunk ends: 3 slots x 4 waves x 2 sides x R floats = 384 bytes;
* ``lap32_kernel`` (the march): 64 data registers - FOUR waves per SIMD, at most 128 VGPR + AGPR; no LDS;
* ``f32p_generic_kernel`` (one cell per thread; three Laplacian and three Euler instances): EIGHT waves per SIMD, at most 64; no LDS.
"""

from __future__ import annotations

import re
import shutil
import subprocess

import pytest

from test_kernel_resources import LIB, LLVM_BIN

NAMES = ("euler32_kernel", "lap32_kernel", "f32p_generic_kernel")


def _metadata(tmp_path):
    """name -> the integer fields of the kernel's metadata note"""
    work = tmp_path / "lib.so"
    shutil.copy(LIB, work)
    subprocess.run([str(LLVM_BIN / "llvm-objdump"), "--offloading", str(work)], capture_output=True, text=True, check=True, timeout=300)
    out = {}
    for co in sorted(tmp_path.glob("lib.so.*gfx950*")):
        notes = subprocess.run([str(LLVM_BIN / "llvm-readelf"), "--notes", str(co)], capture_output=True, text=True, check=True, timeout=300).stdout
        for block in notes.split("- .agpr_count")[1:]:
            block = ".agpr_count" + block
            name = re.search(r"\.name:\s+(\S+)", block)
            if name and any(n in name.group(1) for n in NAMES):
                out[name.group(1)] = {k: int(v) for k, v in re.findall(r"\.(\w+):\s+(\d+)\s*$", block.split("- .agpr_count")[0], flags=re.M)}
    return out


def test_f32p_kernel_resources(tmp_path):
    if not LIB.exists() or not (LLVM_BIN / "llvm-objdump").exists():
        pytest.skip("built library or llvm tools not available")
    kernels = _metadata(tmp_path)
    count = {n: sum(n in k for k in kernels) for n in NAMES}
    assert count == {"euler32_kernel": 1, "lap32_kernel": 1, "f32p_generic_kernel": 6}, sorted(kernels)
    assert not any("fastv" in k for k in kernels)            # built once: there is no contracted twin of this mode
    limits = {"euler32_kernel": (256, 384), "lap32_kernel": (128, 0), "f32p_generic_kernel": (64, 0)}
    for name, md in kernels.items():
        regs, lds = limits[next(n for n in NAMES if n in name)]
        assert md["private_segment_fixed_size"] == 0, (name, md)
        assert md["vgpr_count"] + md["agpr_count"] <= regs, (name, md)
        assert md["group_segment_fixed_size"] == lds, (name, md)
    euler = next(md for name, md in kernels.items() if "euler32_kernel" in name)
    assert euler["max_flat_workgroup_size"] == 256           # at most four waves span a row of 1024 cells
