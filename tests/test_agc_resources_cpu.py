"""-m "not gpu": the level control's kernels in the saved gfx950 ISA (tools/kernel_resources.py: fresh_resources): the four
instantiations of k_agc the launcher can pick are there, none spills a VGPR or uses scratch, and the LDS / VGPR budget of the residency
agc_route's geometry is written for holds."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

WAVES, RESIDENT, CU_LDS = 4, 8, 160 * 1024      # kAgcWaves, kAgcResident (csrc/igdsp_route.h)


@pytest.fixture(scope="module")
def resources():
    import kernel_resources as kr

    return kr.fresh_resources()


def test_agc_kernels_no_spill_and_budget(resources):
    """k_agc<IN_G711, COPY>: blocks of kAgcWaves = 4 waves, two channels each, no LDS.  kAgcResident = 8 blocks share a CU, so 8 waves
    share a SIMD's 512 VGPRs.  No VGPR spill, no scratch."""
    ks = [r for r in resources if "k_agc<" in r["demangled"]]
    names = {r["demangled"] for r in ks}
    assert names == {f"void igdsp::k_agc<{g}, {c}>" for g in ("false", "true") for c in ("false", "true")}, names
    for r in ks:
        assert r["file"] == "igdsp_k_agc"
        assert r["spill"] == 0 and r["scratch"] == 0, r
        assert r["vgpr"] <= 512 // (WAVES * RESIDENT // 4), r
        assert r["lds"] == 0 and r["lds"] * RESIDENT <= CU_LDS, r
    # no other stage's resource test picks these kernels up by substring
    for other in ("k_plc", "k_jb_", "k_snd", "k_bss_", "k_rs<", "k_conf_mix", "k_tx_", "k_tone", "k_link", "k_ptt", "k_dbuf<", "k_meter", "k_roundtrip",
                  "k_encode", "k_window", "k_spec", "k_tdet", "k_ec<"):
        assert not any(other in n for n in names), other
