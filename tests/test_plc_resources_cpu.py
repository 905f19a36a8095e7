"""-m "not gpu": the concealment kernels must not spill VGPRs or use scratch (their SGPR spills stay in VGPR lanes), and must keep the budget their launch geometry relies on: blocks of
kPlcWaves = 4 independent waves, each with 4 KiB of tick kinds ([kPlcPart][kPlcCh] u16), 3 KiB of per-piece partials and 2 KiB of
history, cycle and state in LDS — about 37 KiB per block, so four blocks (16 waves) fit a CU's 160 KiB — and registers for at least four
waves per SIMD."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


@pytest.fixture(scope="module")
def plc_resources():
    from igate4xsoftphonedsp_amd import build as b
    import kernel_resources as kr

    srcs = [os.path.join(b.CSRC, s) for s in b.DEVICE_SOURCES] + [os.path.join(b.CSRC, h) for h in ("igdsp_internal.h", "igdsp_device.h",
                                                                                                 "igdsp_route.h")]
    files = kr.asm_files()
    if len(files) < len(b.DEVICE_SOURCES) - 2 or any(os.path.getmtime(s) > min(os.path.getmtime(a) for a in files) for s in srcs):
        b.build(save_asm=True)
    return [r for r in kr.resources() if "k_plc" in r["demangled"]]


def test_plc_kernels_no_spill_and_budget(plc_resources):
    names = {r["demangled"] for r in plc_resources}
    assert {"void igdsp::k_plc<false>", "void igdsp::k_plc<true>"} <= names, names
    for r in plc_resources:
        assert r["spill"] == 0 and r["scratch"] == 0, r
        assert r["sgpr_spill"] <= 40, r                                  # SGPRs spill into VGPR lanes only: no memory
        assert r["vgpr"] <= 128, r                                        # four waves per SIMD
        assert 32 * 1024 <= r["lds"] <= 160 * 1024 // 4, r               # the kinds are there; four blocks per CU
