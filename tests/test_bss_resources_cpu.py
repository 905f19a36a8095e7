"""-m "not gpu": the best-signal-selection kernels must not spill and must keep the budget their launch geometry relies on: blocks of
kBssWaves = 4 waves (one wave per SIMD, so up to 512 VGPRs would fit; the emit keeps kBssU frame loads in flight in far fewer), the G.711
form's 64 KiB LUT + 32 KiB of vote keys within the 160 KiB LDS of a CU, and k_bss_words as a plain 256-thread kernel without LDS."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


@pytest.fixture(scope="module")
def bss_resources():
    from igate4xsoftphonedsp_amd import build as b
    import kernel_resources as kr

    srcs = [os.path.join(b.CSRC, s) for s in b.DEVICE_SOURCES] + [os.path.join(b.CSRC, h) for h in ("igdsp_internal.h", "igdsp_device.h",
                                                                                                 "igdsp_route.h", "igdsp_q7.h")]
    files = kr.asm_files()
    if len(files) < len(b.DEVICE_SOURCES) - 2 or any(os.path.getmtime(s) > min(os.path.getmtime(a) for a in files) for s in srcs):
        b.build(save_asm=True)
    return [r for r in kr.resources() if "k_bss_" in r["demangled"]]


def test_bss_kernels_no_spill_and_budget(bss_resources):
    names = {r["demangled"] for r in bss_resources}
    # every input form of the product kernel and of the compute-free yardstick, and the words pass
    assert {f"void igdsp::k_bss_select<{i}, {c}>" for i in (0, 1, 2) for c in ("false", "true")} <= names, names
    assert any("k_bss_words" in x for x in names), names
    for r in bss_resources:
        assert r["spill"] == 0 and r["scratch"] == 0, r
        assert r["vgpr"] <= 128, r                                       # room to spare at one wave per SIMD
        assert r["lds"] <= 160 * 1024, r
        if r["demangled"] == "void igdsp::k_bss_select<0, false>":
            assert r["lds"] >= 64 * 1024 + 32 * 1024, r                 # the LUT and the vote keys are both there
        if "k_bss_words" in r["demangled"]:
            assert r["lds"] == 0, r
