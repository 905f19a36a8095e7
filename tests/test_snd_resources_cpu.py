"""-m "not gpu": the sound-card kernels in the saved gfx950 ISA (tools/kernel_resources.py: fresh_resources): every instantiation the
launcher can pick is there, none spills VGPRs or uses scratch, and the LDS / VGPR budget snd_route relies on holds."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

WAVES, TILE = 8, 4096                                                    # kSndWaves, kSndTileBytes (csrc/igdsp_route.h)


@pytest.fixture(scope="module")
def resources():
    import kernel_resources as kr

    return kr.fresh_resources()


def test_snd_kernels_no_spill_and_budget(resources):
    """k_snd<DIR, MODE, VEC>: blocks of kSndWaves = 8 waves, two per SIMD, so up to 256 VGPRs each; the vector form keeps kSndU = 4 items
    of 4 pieces = 64 VGPRs of loads in flight.  LDS: one 4 KiB tile per wave and nothing else; the yardstick (MODE 3) keeps no tile."""
    snd = [r for r in resources if "k_snd<" in r["demangled"]]
    names = {r["demangled"] for r in snd}
    # both directions x {both, bulk only, records only} x {vector, general}; the yardstick has one direction
    want = {f"void igdsp::k_snd<{d}, {m}, {v}>" for d in (0, 1) for m in (0, 1, 2) for v in ("false", "true")}
    want |= {f"void igdsp::k_snd<0, 3, {v}>" for v in ("false", "true")}
    assert want == names, want ^ names
    for r in snd:
        assert r["spill"] == 0 and r["sgpr_spill"] == 0 and r["scratch"] == 0, r
        assert r["vgpr"] <= 256, r
        if ", 3, " in r["demangled"]:
            assert r["lds"] == 0, r
        else:
            assert r["lds"] == WAVES * TILE, r
