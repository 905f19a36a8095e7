"""-m "not gpu": the adaptive jitter-buffer kernel in the saved gfx950 ISA (tools/kernel_resources.py: fresh_resources): k_jb_adaptive is
in the code object, spills nothing and uses no scratch, and has the LDS of k_jb_receive<false>, whose geometry and phases it shares (the
delay of a tick rides in free bits of its descriptor, not in LDS of its own)."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


@pytest.fixture(scope="module")
def resources():
    import kernel_resources as kr

    return kr.fresh_resources()


def test_jb_adaptive_no_spill_and_the_fixed_kernels_lds(resources):
    by = {r["demangled"]: r for r in resources if "k_jb_" in r["demangled"]}
    assert set(by) == {"void igdsp::k_jb_receive<false>", "void igdsp::k_jb_receive<true>", "igdsp::k_jb_adaptive"}, set(by)
    r, fixed = by["igdsp::k_jb_adaptive"], by["void igdsp::k_jb_receive<false>"]
    assert r["spill"] == 0 and r["sgpr_spill"] == 0 and r["scratch"] == 0, r
    assert r["lds"] == fixed["lds"], (r, fixed)
    assert r["vgpr"] <= 168, r                                            # three waves per SIMD, as the LDS allows
