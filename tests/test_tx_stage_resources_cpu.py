"""-m "not gpu": the staged send path's kernel (k_tx_staged) must not spill or use scratch, and must keep the register / LDS budget
its route relies on: blocks of kTsWaves x 64 threads, 4 096 waves resident at 65 536 legs -> at least 4 waves per SIMD (<= 128 VGPRs),
static LDS only, small enough for several blocks per CU."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


@pytest.fixture(scope="module")
def staged_resources():
    from igate4xsoftphonedsp_amd import build as b
    import kernel_resources as kr

    srcs = [os.path.join(b.CSRC, s) for s in b.DEVICE_SOURCES] + [os.path.join(b.CSRC, h) for h in ("igdsp_internal.h", "igdsp_device.h", "igdsp_txstage.h", "igdsp_route.h")]
    files = kr.asm_files()
    if not any("igdsp_k_txstage" in f for f in files) or any(os.path.getmtime(s) > min(os.path.getmtime(a) for a in files) for s in srcs):
        b.build(save_asm=True)
    return [r for r in kr.resources() if "k_tx_staged" in r["demangled"]]


def test_staged_kernel_no_spill_and_budget(staged_resources):
    assert [r["demangled"] for r in staged_resources] == ["igdsp::k_tx_staged"], staged_resources
    r = staged_resources[0]
    assert r["spill"] == 0 and r["sgpr_spill"] == 0 and r["scratch"] == 0, r
    assert r["vgpr"] <= 128, r
    assert r["lds"] <= 16 * 1024, r
