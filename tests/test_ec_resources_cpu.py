"""-m "not gpu": the echo canceller's kernels in the saved gfx950 ISA (tools/kernel_resources.py: fresh_resources): the eight
instantiations of k_ec the launcher can pick are there, none spills a VGPR or uses scratch, and the LDS / VGPR budget of the residency
ec_route's geometry is written for holds."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

WAVES, RESIDENT, CU_LDS = 4, 3, 160 * 1024      # kEcWaves, kEcResident (csrc/igdsp_route.h)


@pytest.fixture(scope="module")
def resources():
    import kernel_resources as kr

    return kr.fresh_resources()


def test_ec_kernels_no_spill_and_budget(resources):
    """k_ec<NEAR_G711, L, COPY>: blocks of kEcWaves = 4 waves, four channels each.  The block's LDS is 16 channels' far buffer (8 + 256 +
    256 + 8 values) and near buffer (8 + 256 values); kEcResident = 3 blocks share a CU, so 3 waves share a SIMD's 512 VGPRs.  No VGPR
    spill, no scratch."""
    ks = [r for r in resources if "k_ec<" in r["demangled"]]
    names = {r["demangled"] for r in ks}
    assert names == {f"void igdsp::k_ec<{g}, {L}, {c}>" for g in ("false", "true") for L in (128, 256) for c in ("false", "true")}, names
    lds = WAVES * 4 * ((8 + 256 + 256 + 8) + (8 + 256)) * 2
    for r in ks:
        assert r["file"] == "igdsp_k_ec"
        assert r["spill"] == 0 and r["scratch"] == 0, r
        assert r["vgpr"] <= 512 // (WAVES * RESIDENT // 4), r
        assert r["lds"] == lds and r["lds"] * RESIDENT <= CU_LDS, r
    # no other stage's resource test picks these kernels up by substring
    for other in ("k_plc", "k_jb_", "k_snd", "k_bss_", "k_rs<", "k_conf_mix", "k_tx_", "k_tone", "k_link", "k_ptt", "k_dbuf<", "k_meter", "k_roundtrip",
                  "k_encode", "k_window", "k_spec", "k_tdet"):
        assert not any(other in n for n in names), other
