"""Guard: the domain-property kernels (csrc/pdehip_props.hip) as compiled for gfx950 (CPU-only check of the built library's code-object
metadata, like tests/test_kernel_resources_domains.py): every kernel is there in each instance, none uses scratch memory, none needs more
than 128 vector registers - the sweeps are latency-bound on gathers and atomics and want at least four waves per SIMD."""

from __future__ import annotations

import pytest

from test_kernel_resources import LIB, LLVM_BIN, _kernel_metadata

# kernel -> instances: the sum kernel without a field, with an fp64 and with an fp32 field
OWN = {"props_init_kernel": 1, "props_anchor_kernel": 1, "props_sum_kernel": 3}


def test_domain_property_kernels_resources(tmp_path):
    if not LIB.exists() or not (LLVM_BIN / "llvm-objdump").exists():
        pytest.skip("built library or llvm tools not available")
    kernels = _kernel_metadata(tmp_path)
    own = [(n, s, v) for n, s, v in kernels if any(k in n for k in OWN)]
    for needle, count in OWN.items():
        found = sorted(n for n, _, _ in own if needle in n)
        assert len(found) == count, f"{needle}: {len(found)} instances, expected {count}: {found}"
    offenders = [(n, s) for n, s, _ in own if s]
    assert not offenders, f"domain-property kernels spilling to scratch: {offenders[:5]}"
    print(sorted((v, n) for n, _, v in own))
    assert max(v for _, _, v in own) <= 128, sorted((v, n) for n, _, v in own)[-3:]
