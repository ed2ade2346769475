"""Guard: the histogram and selection kernels (csrc/pdehip_hist.hip) as compiled for gfx950 (CPU-only check of the built library's
code-object metadata, like tests/test_kernel_resources_stats.py): every kernel is there in each instance, none uses scratch memory, none
needs more than 64 vector registers - they are streaming sweeps and have no reason to limit occupancy."""

from __future__ import annotations

import pytest

from test_kernel_resources import LIB, LLVM_BIN, _kernel_metadata

# kernel -> instances: the sweeps exist for fp64 (one cell, pairs) and fp32 (one cell, quads), with and without the norm; the histogram
# sweep also for equal bins (a scaled guess) and general edges (a binary search); the scan behind each selection pass per field type
OWN = {"hist_sweep_kernel": 16, "select_sweep_kernel": 8, "select_scan_kernel": 2}


def test_histogram_kernels_resources(tmp_path):
    if not LIB.exists() or not (LLVM_BIN / "llvm-objdump").exists():
        pytest.skip("built library or llvm tools not available")
    kernels = _kernel_metadata(tmp_path)
    own = [(n, s, v) for n, s, v in kernels if any(k in n for k in OWN)]
    for needle, count in OWN.items():
        found = sorted(n for n, _, _ in own if needle in n)
        assert len(found) == count, f"{needle}: {len(found)} instances, expected {count}: {found}"
    offenders = [(n, s) for n, s, _ in own if s]
    assert not offenders, f"histogram kernels spilling to scratch: {offenders[:5]}"
    print(sorted((v, n) for n, _, v in own))
    assert max(v for _, _, v in own) <= 64, sorted((v, n) for n, _, v in own)[-3:]
