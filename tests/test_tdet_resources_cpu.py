"""-m "not gpu": the tone detector's kernels in the saved gfx950 ISA (tools/kernel_resources.py: fresh_resources): the six
instantiations of k_tdet the launcher can pick and the list's two passes are there, none spills a VGPR or uses scratch, and the LDS /
VGPR budget of the residency tdet_route's geometry is written for holds."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

WAVES, RESIDENT, CU_LDS = 8, 3, 160 * 1024      # kTdetWaves, kTdetResident (csrc/igdsp_route.h)


@pytest.fixture(scope="module")
def resources():
    import kernel_resources as kr

    return kr.fresh_resources()


def test_tdet_kernels_no_spill_and_budget(resources):
    """k_tdet<COPY, E0>: blocks of kTdetWaves = 8 waves, four channels each.  The block's LDS is one plan's table (16 KiB), 32 channel
    buffers of 384 values and the channels' plan indices; kTdetResident = 3 blocks share the CU's 160 KiB, so 6 waves share a SIMD's 512
    VGPRs.  No VGPR spill, no scratch.  k_tdet_list<WRITE> has no LDS."""
    ks = [r for r in resources if "k_tdet" in r["demangled"]]
    names = {r["demangled"] for r in ks}
    assert names == {f"void igdsp::k_tdet<{c}, {o}>" for c in ("false", "true") for o in (0, 1, 2)} | {
        "void igdsp::k_tdet_list<false>", "void igdsp::k_tdet_list<true>"}, names
    lds = 128 * 16 * 8 + WAVES * 4 * (128 + 256) * 2 + WAVES * 4 * 4
    for r in ks:
        assert r["file"] == "igdsp_k_tdet"
        assert r["spill"] == 0 and r["scratch"] == 0, r
        if "k_tdet<" in r["demangled"]:
            assert r["vgpr"] <= 512 // (WAVES * RESIDENT // 4), r
            assert r["lds"] == lds and r["lds"] * RESIDENT <= CU_LDS, r
        else:
            assert r["lds"] == 0 and r["vgpr"] <= 64, r
    # no other stage's resource test picks these kernels up by substring
    for other in ("k_plc", "k_jb_", "k_snd", "k_bss_", "k_rs<", "k_conf_mix", "k_tx_", "k_tone", "k_link", "k_ptt", "k_dbuf<", "k_meter", "k_roundtrip",
                  "k_encode", "k_window", "k_spec"):
        assert not any(other in n for n in names), other
