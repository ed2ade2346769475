"""Guard: the kernels of the inverse transform (csrc/pdehip_fft.hip) and of the direct Poisson solve (csrc/pdehip_fftsolve.hip) as compiled
for gfx950 (CPU-only check of the built library's code-object metadata, like tests/test_kernel_resources_fft.py): every kernel is there
in each instance, none uses scratch memory, none needs more than 64 vector registers.  The cap and its argument are those of the forward
kernels: a workgroup of a transform pass holds 8 KiB to 136 KiB of LDS, so LDS and not registers decides how many of them a CU holds, and
the division and the test are streaming sweeps."""

from __future__ import annotations

import pytest

from test_kernel_resources import LIB, LLVM_BIN, _kernel_metadata

# kernel -> instances: the row pass per field type (the rounding to the field type is at its store); the test reads both field types in
# one instance
OWN = {"inverse_rows_kernel": 2, "inverse_lines_kernel": 1, "fftsolve_divide_kernel": 1, "fftsolve_check_kernel": 1}


def test_fftsolve_kernels_resources(tmp_path):
    if not LIB.exists() or not (LLVM_BIN / "llvm-objdump").exists():
        pytest.skip("built library or llvm tools not available")
    kernels = _kernel_metadata(tmp_path)
    own = [(n, s, v) for n, s, v in kernels if any(k in n for k in OWN)]
    for needle, count in OWN.items():
        found = sorted(n for n, _, _ in own if needle in n)
        assert len(found) == count, f"{needle}: {len(found)} instances, expected {count}: {found}"
    # the names must stay clear of the substrings the sibling guards count by
    for n, _, _ in own:
        assert not any(word in n for word in ("poisson_", "fft_rows_kernel", "fft_lines_kernel", "shell_")), n
    offenders = [(n, s) for n, s, _ in own if s]
    assert not offenders, f"kernels spilling to scratch: {offenders[:5]}"
    print(sorted((v, n) for n, _, v in own))
    assert max(v for _, _, v in own) <= 64, sorted((v, n) for n, _, v in own)[-3:]
