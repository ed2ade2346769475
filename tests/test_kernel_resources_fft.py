"""Guard: the transform and shell kernels (csrc/pdehip_fft.hip) as compiled for gfx950 (CPU-only check of the built library's code-object
metadata, like tests/test_kernel_resources_hist.py): every kernel is there in each instance, none uses scratch memory, none needs more
than 64 vector registers.  The cap is that of 8 waves per SIMD: a workgroup of the transform holds 8 KiB to 136 KiB of LDS, so LDS and
not registers decides how many of them a CU holds (up to 16 workgroups of 256 threads at 8 KiB - all 8 waves per SIMD), and the shell
sweeps are streaming sweeps like the histogram's."""

from __future__ import annotations

import pytest

from test_kernel_resources import LIB, LLVM_BIN, _kernel_metadata

# kernel -> instances: the row pass per field type (the conversion to fp64 is at its load), everything behind it works on the fp64 spectrum
OWN = {"fft_rows_kernel": 2, "fft_lines_kernel": 1, "shell_max_kernel": 1, "shell_params_kernel": 1, "shell_limb_kernel": 1}


def test_fft_kernels_resources(tmp_path):
    if not LIB.exists() or not (LLVM_BIN / "llvm-objdump").exists():
        pytest.skip("built library or llvm tools not available")
    kernels = _kernel_metadata(tmp_path)
    own = [(n, s, v) for n, s, v in kernels if any(k in n for k in OWN)]
    for needle, count in OWN.items():
        found = sorted(n for n, _, _ in own if needle in n)
        assert len(found) == count, f"{needle}: {len(found)} instances, expected {count}: {found}"
    offenders = [(n, s) for n, s, _ in own if s]
    assert not offenders, f"transform kernels spilling to scratch: {offenders[:5]}"
    print(sorted((v, n) for n, _, v in own))
    assert max(v for _, _, v in own) <= 64, sorted((v, n) for n, _, v in own)[-3:]
