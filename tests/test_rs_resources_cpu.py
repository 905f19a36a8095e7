"""-m "not gpu": the rate converter's kernels in the saved gfx950 ISA (tools/kernel_resources.py: fresh_resources): every instantiation
the launcher can pick is there, none spills or uses scratch, and the LDS / VGPR budget of the residency rs_route sizes its grid for
holds."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

WAVES, FACTORS, MAX_RESIDENT, CU_LDS = 4, (2, 3, 4, 6), 3, 160 * 1024    # kRsWaves, kRsMaxResident (csrc/igdsp_route.h)


def lds_bytes(direction, R):
    """rs_lds_bytes: per wave and channel a tile of (24 + 256) (UP) / 280 R (DOWN) int16 and R 16-byte record slots; UP: the 1 KiB table"""
    ch, tile = (16, 24 + 256) if direction == 0 else (4, 280 * R)
    return WAVES * ch * (tile * 2 + R * 16) + (1024 if direction == 0 else 0)


def resident(direction, R):
    """rs_resident: the blocks a CU holds"""
    return min(MAX_RESIDENT, CU_LDS // (lds_bytes(direction, R) + 16))


@pytest.fixture(scope="module")
def resources():
    import kernel_resources as kr

    return kr.fresh_resources()


def test_rs_kernels_no_spill_and_budget(resources):
    """k_rs<DIR, R, COPY, VEC>: blocks of kRsWaves = 4 waves, one per SIMD.  rs_route sizes the grid for rs_resident blocks per CU: 3,
    and 2 for DOWN by 6 whose 54 KiB tiles admit no third.  That many waves share a SIMD's 512 VGPRs (allocated in eights), that many
    blocks the CU's 160 KiB of LDS, and a static block stays below 64 KiB.  No spill of either kind, no scratch.  k_rs_state: 192
    threads, the 1 KiB table."""
    rs = [r for r in resources if "k_rs<" in r["demangled"]]
    names = {r["demangled"] for r in rs}
    want = {f"void igdsp::k_rs<{d}, {R}, {c}, {v}>" for d in (0, 1) for R in FACTORS for c in ("false", "true") for v in ("false", "true")}
    assert want == names, want ^ names
    for r in rs:
        d, R = (int(v) for v in r["demangled"].split("<")[1].split(",")[:2])
        res = resident(d, R)
        assert res == (2 if (d, R) == (1, 6) else 3)
        assert r["spill"] == 0 and r["sgpr_spill"] == 0 and r["scratch"] == 0, r
        assert r["vgpr"] <= 512 // res // 8 * 8, r                        # 168 (three waves per SIMD) / 256 (two)
        assert r["lds"] <= 65536 and lds_bytes(d, R) <= r["lds"] <= lds_bytes(d, R) + 16, r       # (+ the alignment of the slots)
        assert r["lds"] * res <= CU_LDS, r
    state = [r for r in resources if r["demangled"].endswith("igdsp::k_rs_state")]
    assert len(state) == 1 and state[0]["lds"] == 1024 and state[0]["spill"] == 0 and state[0]["sgpr_spill"] == 0 and state[0]["scratch"] == 0, state
