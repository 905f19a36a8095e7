"""-m "not gpu": the conference mix's kernels must not spill and must keep the budget its launch geometry relies on: one block of
kConfWaves = 16 waves per CU (<= 128 VGPRs for 4 waves per SIMD), the G.711 form's 64 KiB LUT + 32 KiB wide-form partials within the
160 KiB LDS of a CU."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


@pytest.fixture(scope="module")
def conf_resources():
    from igate4xsoftphonedsp_amd import build as b
    import kernel_resources as kr

    srcs = [os.path.join(b.CSRC, s) for s in b.DEVICE_SOURCES] + [os.path.join(b.CSRC, h) for h in ("igdsp_internal.h", "igdsp_device.h", "igdsp_route.h")]
    files = kr.asm_files()
    if len(files) < len(b.DEVICE_SOURCES) - 2 or any(os.path.getmtime(s) > min(os.path.getmtime(a) for a in files) for s in srcs):
        b.build(save_asm=True)
    return [r for r in kr.resources() if "k_conf_mix" in r["demangled"]]


def test_conf_kernels_no_spill_and_budget(conf_resources):
    names = {r["demangled"] for r in conf_resources}
    # both input forms of the product kernel and of the compute-free yardstick: every instantiation the launchers can pick
    assert {"void igdsp::k_conf_mix<0, false>", "void igdsp::k_conf_mix<1, false>", "void igdsp::k_conf_mix<0, true>",
            "void igdsp::k_conf_mix<1, true>"} <= names, names
    for r in conf_resources:
        assert r["spill"] == 0 and r["scratch"] == 0, r                  # (SGPR spills land in VGPR lanes, not in memory)
        assert r["vgpr"] <= 128, r
        assert r["lds"] <= 160 * 1024, r
        if r["demangled"] == "void igdsp::k_conf_mix<0, false>":
            assert r["lds"] >= 64 * 1024 + 32 * 1024, r                # the LUT and the partials are both there
