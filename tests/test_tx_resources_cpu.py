"""-m "not gpu": the TX packetizer's kernels must not spill, and must keep the register / LDS budget its launch geometry relies on
(one block of 8 waves per CU in the table form: <= 256 VGPRs for 2 waves per SIMD, 18 KiB static LDS beside the 128 KiB table)."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


@pytest.fixture(scope="module")
def tx_resources():
    from igate4xsoftphonedsp_amd import build as b
    import kernel_resources as kr

    srcs = [os.path.join(b.CSRC, s) for s in b.DEVICE_SOURCES] + [os.path.join(b.CSRC, h) for h in ("igdsp_internal.h", "igdsp_device.h")]
    if len(kr.asm_files()) < 4 or any(os.path.getmtime(s) > min(os.path.getmtime(a) for a in kr.asm_files()) for s in srcs):
        b.build(save_asm=True)
    return [r for r in kr.resources() if "k_tx_packetize" in r["demangled"]]


def test_tx_kernel_no_spill_and_budget(tx_resources):
    names = {r["demangled"] for r in tx_resources}
    # every (input form, encoder lineage) instantiation the launcher can pick
    assert {"void igdsp::k_tx_packetize<0, 1>", "void igdsp::k_tx_packetize<1, 0>", "void igdsp::k_tx_packetize<1, 1>",
            "void igdsp::k_tx_packetize<2, 0>", "void igdsp::k_tx_packetize<2, 1>"} <= names, names
    for r in tx_resources:
        assert r["spill"] == 0 and r["scratch"] == 0, r
        assert r["vgpr"] <= 256, r
        assert r["lds"] + 2 * 65536 <= 160 * 1024, r
