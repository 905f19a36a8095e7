"""-m "not gpu": the delay buffer's kernels in the saved gfx950 ISA (tools/kernel_resources.py: fresh_resources): both instantiations
the launcher can pick are there, neither spills a VGPR or uses scratch, and the LDS / VGPR budget of the residency dbuf_route's
geometry is written for holds."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

WAVES, RESIDENT, WIN, CU_LDS = 4, 8, 280, 160 * 1024      # kDbufWaves, kDbufResident (csrc/igdsp_route.h), IGDSP_DBUF_WIN


@pytest.fixture(scope="module")
def resources():
    import kernel_resources as kr

    return kr.fresh_resources()


def test_dbuf_kernels_no_spill_and_budget(resources):
    """k_dbuf<COPY>: blocks of kDbufWaves = 4 waves, a channel each.  The walk hides its memory round trips behind other waves, so the
    kernel is kept small enough for kDbufResident = 8 blocks per CU: 8 waves share a SIMD's 512 VGPRs, 8 blocks the CU's 160 KiB of LDS
    (per wave the shrink's 280-sample window and its shifted copy; the yardstick has no shrink and no LDS).  No VGPR spill, no scratch."""
    ks = [r for r in resources if "k_dbuf<" in r["demangled"]]
    names = {r["demangled"] for r in ks}
    assert names == {"void igdsp::k_dbuf<false>", "void igdsp::k_dbuf<true>"}, names
    lds = WAVES * 2 * WIN * 2
    for r in ks:
        assert r["file"] == "igdsp_k_dbuf"
        assert r["spill"] == 0 and r["scratch"] == 0, r
        assert r["vgpr"] <= 512 // RESIDENT, r
        assert r["lds"] == (0 if "<true>" in r["demangled"] else lds), r
        assert r["lds"] * RESIDENT <= CU_LDS, r
    # no other stage's resource test picks these kernels up by substring
    for other in ("k_plc", "k_jb_", "k_snd", "k_bss_", "k_rs<", "k_conf_mix", "k_tx_", "k_tone", "k_link", "k_ptt"):
        assert not any(other in n for n in names), other
