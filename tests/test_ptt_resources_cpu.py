"""-m "not gpu": the PTT arbitration kernels in the saved gfx950 ISA (tools/kernel_resources.py: fresh_resources): every instantiation the
launcher can pick is there, none spills VGPRs or uses scratch, and the LDS / VGPR budget ptt_route relies on holds."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


@pytest.fixture(scope="module")
def resources():
    import kernel_resources as kr

    return kr.fresh_resources()


def test_ptt_kernels_no_spill_and_budget(resources):
    """Blocks of kPttWaves = 4 waves, one per SIMD (so up to 512 VGPRs would fit; the emit keeps kPttU frame loads in flight in far
    fewer), the G.711 form's 64 KiB LUT + 32 KiB of selections + 32 KiB of ops within the 160 KiB LDS of a CU, and k_ptt_slots as a plain
    256-thread kernel without LDS."""
    ptt = [r for r in resources if "k_ptt_" in r["demangled"]]
    names = {r["demangled"] for r in ptt}
    # every input form of the product kernel and of the compute-free yardstick, and the slot pass
    assert {f"void igdsp::k_ptt_arbitrate<{i}, {c}>" for i in (0, 1, 2) for c in ("false", "true")} <= names, names
    assert any("k_ptt_slots" in x for x in names), names
    for r in ptt:
        assert r["spill"] == 0 and r["scratch"] == 0, r
        assert r["vgpr"] <= 128, r                                       # room to spare at one wave per SIMD
        assert r["lds"] <= 160 * 1024, r
        if r["demangled"] == "void igdsp::k_ptt_arbitrate<0, false>":
            assert r["lds"] >= 64 * 1024 + 32 * 1024 + 32 * 1024, r     # the LUT, the selections and the ops are all there
        if r["demangled"] in ("void igdsp::k_ptt_arbitrate<1, false>", "void igdsp::k_ptt_arbitrate<2, false>"):
            assert 64 * 1024 <= r["lds"] < 96 * 1024, r                 # selections and ops, no LUT without G.711
        if "k_ptt_slots" in r["demangled"]:
            assert r["lds"] == 0, r
