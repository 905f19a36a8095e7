"""-m "not gpu": the voice detector's kernels in the saved gfx950 ISA (tools/kernel_resources.py: fresh_resources): the four
instantiations of k_vad and the two of k_vad_list the launcher can pick are there, none spills a VGPR or uses scratch, and the LDS /
VGPR budget of the residency vad_route's geometry is written for holds."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

WAVES, RESIDENT, CU_LDS = 4, 6, 160 * 1024      # kVadWaves, kVadResident (csrc/igdsp_route.h)
LDS = 128 * 8 + 16 * (280 * 2 + 256 * 2 + 3 * 12 * 8 + 16)  # kVadLdsBytes


@pytest.fixture(scope="module")
def resources():
    import kernel_resources as kr

    return kr.fresh_resources()


def test_vad_kernels_no_spill_and_budget(resources):
    """k_vad<IN_G711, COPY>: blocks of kVadWaves = 4 waves, four channels each.  kVadResident = 6 blocks share a CU, so 6 waves share a
    SIMD's 512 VGPRs and the blocks its LDS.  No VGPR spill, no scratch."""
    ks = [r for r in resources if "k_vad<" in r["demangled"]]
    names = {r["demangled"] for r in ks}
    assert names == {f"void igdsp::k_vad<{g}, {c}>" for g in ("false", "true") for c in ("false", "true")}, names
    for r in ks:
        assert r["file"] == "igdsp_k_vad"
        assert r["spill"] == 0 and r["scratch"] == 0, r
        assert r["vgpr"] <= 512 // (WAVES * RESIDENT // 4), r
        assert r["lds"] == LDS and r["lds"] * RESIDENT <= CU_LDS, r
    ls = [r for r in resources if "k_vad_list<" in r["demangled"]]
    assert {r["demangled"] for r in ls} == {f"void igdsp::k_vad_list<{w}>" for w in ("false", "true")}
    for r in ls:
        assert r["file"] == "igdsp_k_vad" and r["spill"] == 0 and r["scratch"] == 0 and r["lds"] == 0, r
    # no other stage's resource test picks these kernels up by substring
    for other in ("k_plc", "k_jb_", "k_snd", "k_bss_", "k_rs<", "k_conf_mix", "k_tx_", "k_tone", "k_link", "k_ptt", "k_dbuf<", "k_meter", "k_roundtrip",
                  "k_encode", "k_window", "k_spec", "k_tdet", "k_ec<", "k_agc"):
        assert not any(other in n for n in names), other
