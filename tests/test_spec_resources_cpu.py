"""-m "not gpu": the spectrum kernels in the saved gfx950 ISA (tools/kernel_resources.py: fresh_resources): both instantiations the
launcher can pick are there, neither spills a VGPR or uses scratch, and the LDS / VGPR budget of the residency spec_route's geometry is
written for holds."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

WAVES, RESIDENT, TILE_ROW, CU_LDS = 4, 4, 72, 160 * 1024      # kSpecWaves, kSpecResident, kSpecTileRow (csrc/igdsp_route.h)


@pytest.fixture(scope="module")
def resources():
    import kernel_resources as kr

    return kr.fresh_resources()


def test_spec_kernels_no_spill_and_budget(resources):
    """k_spec<COPY>: blocks of kSpecWaves = 4 waves, a channel each.  The lane keeps the averaged array and two passes' twiddle factors in
    registers, so the kernel is sized for kSpecResident = 4 blocks per CU: 4 waves share a SIMD's 512 VGPRs, 4 blocks the CU's 160 KiB of
    LDS (per wave the 2 KiB ring and the 8 x 72-point tile).  No VGPR spill, no scratch."""
    ks = [r for r in resources if "k_spec<" in r["demangled"]]
    names = {r["demangled"] for r in ks}
    assert names == {"void igdsp::k_spec<false>", "void igdsp::k_spec<true>"}, names
    lds = WAVES * (1024 * 2 + 8 * TILE_ROW * 8)
    for r in ks:
        assert r["file"] == "igdsp_k_spec"
        assert r["spill"] == 0 and r["scratch"] == 0, r
        assert r["vgpr"] <= 512 // RESIDENT, r
        assert r["lds"] == lds, r
        assert r["lds"] * RESIDENT <= CU_LDS, r
    # no other stage's resource test picks these kernels up by substring
    for other in ("k_plc", "k_jb_", "k_snd", "k_bss_", "k_rs<", "k_conf_mix", "k_tx_", "k_tone", "k_link", "k_ptt", "k_dbuf<", "k_meter", "k_roundtrip",
                  "k_encode", "k_window"):
        assert not any(other in n for n in names), other
