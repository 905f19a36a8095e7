"""-m "not gpu": the tone generator's kernels in the saved gfx950 ISA (tools/kernel_resources.py: fresh_resources): every instantiation
the launcher can pick is there, none spills or uses scratch, and the LDS / VGPR budget tone_route relies on holds."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

WAVES, TABLE = 16, 4096                                                  # kToneWaves, the pair table (csrc/igdsp_route.h)


@pytest.fixture(scope="module")
def resources():
    import kernel_resources as kr

    return kr.fresh_resources()


def test_tone_kernels_no_spill_and_budget(resources):
    """k_tone<VEC, MODE>: blocks of kToneWaves = 16 waves, four per SIMD, so at most 128 VGPRs each.  LDS: the 4 KiB pair table and
    nothing else; the yardstick (MODE 3) keeps no table.  k_tone_state: a thread per port, no LDS."""
    tone = [r for r in resources if "k_tone<" in r["demangled"]]
    names = {r["demangled"] for r in tone}
    want = {f"void igdsp::k_tone<{v}, {m}>" for v in ("false", "true") for m in (0, 1, 2, 3)}
    assert want == names, want ^ names
    for r in tone:
        assert r["spill"] == 0 and r["sgpr_spill"] == 0 and r["scratch"] == 0, r
        assert r["vgpr"] <= 512 // (WAVES // 4), r
        assert r["lds"] == (0 if ", 3>" in r["demangled"] else TABLE), r
    state = [r for r in resources if r["demangled"].endswith("igdsp::k_tone_state")]
    assert len(state) == 1 and state[0]["lds"] == 0 and state[0]["spill"] == 0 and state[0]["scratch"] == 0, state
