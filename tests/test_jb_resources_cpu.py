"""-m "not gpu": the jitter-buffer kernels must not spill and must keep the budget their launch geometry relies on: blocks of kJbWaves = 4
independent waves, each with 8 KiB of descriptors ([kJbPart][kJbCh] u32) and 3.5 KiB of ring tags, sources and store list in LDS — about
42 KiB per block, so three blocks (12 waves) fit a CU's 160 KiB — and registers for at least three waves per SIMD."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


@pytest.fixture(scope="module")
def jb_resources():
    from igate4xsoftphonedsp_amd import build as b
    import kernel_resources as kr

    srcs = [os.path.join(b.CSRC, s) for s in b.DEVICE_SOURCES] + [os.path.join(b.CSRC, h) for h in ("igdsp_internal.h", "igdsp_device.h",
                                                                                                 "igdsp_route.h", "igdsp_rtp.h")]
    files = kr.asm_files()
    if len(files) < len(b.DEVICE_SOURCES) - 2 or any(os.path.getmtime(s) > min(os.path.getmtime(a) for a in files) for s in srcs):
        b.build(save_asm=True)
    return [r for r in kr.resources() if "k_jb_" in r["demangled"]]


def test_jb_kernels_no_spill_and_budget(jb_resources):
    names = {r["demangled"] for r in jb_resources}
    assert {"void igdsp::k_jb_receive<false>", "void igdsp::k_jb_receive<true>"} <= names, names
    for r in jb_resources:
        assert r["spill"] == 0 and r["sgpr_spill"] == 0 and r["scratch"] == 0, r
        assert r["vgpr"] <= 168, r                                        # three waves per SIMD: what the LDS allows
        assert 32 * 1024 <= r["lds"] <= 160 * 1024 // 3, r               # the descriptors are there; three blocks per CU
