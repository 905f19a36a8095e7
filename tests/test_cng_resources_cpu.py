"""-m "not gpu": the comfort-noise generator's kernels in the saved gfx950 ISA (tools/kernel_resources.py: fresh_resources): the six
instantiations of k_cng the launcher can pick are there, none spills a VGPR or uses scratch (b[10] and kq[10] are registers, never a
run-time indexed array), the VGPR / LDS budget of the residency cng_route's geometry is written for holds, and the sample loop holds
the number of vector instructions tools/cng_bench.py's floor is computed from."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

RESIDENT, VGPRS, CU_LDS = 4, 128, 160 * 1024     # kCngResident, kCngVgprs (csrc/igdsp_route.h)
LDS_MAX = 64 * (256 // 2 + 1) * 4 + 64            # tile_lds_bytes(kCngChans, 256): dynamic, asked for by the launcher


@pytest.fixture(scope="module")
def resources():
    import kernel_resources as kr

    return kr.fresh_resources()


def test_cng_kernels_no_spill_and_budget(resources):
    """k_cng<IN, COPY>: a block is one wave of 64 channels; kCngResident = 4 blocks share a CU, one wave a SIMD, so a wave may take up to
    128 VGPRs at the 4 waves per SIMD the launch bound leaves room for; the tile is dynamic LDS (none is static).  No VGPR spill, no
    scratch."""
    ks = [r for r in resources if "k_cng<" in r["demangled"]]
    names = {r["demangled"] for r in ks}
    assert names == {f"void igdsp::k_cng<{i}, {c}>" for i in (0, 1, 2) for c in ("false", "true")}, names
    for r in ks:
        assert r["file"] == "igdsp_k_cng"
        assert r["spill"] == 0 and r["scratch"] == 0, r
        assert r["vgpr"] <= VGPRS <= 512 // RESIDENT, r
        assert r["lds"] == 0 and LDS_MAX * RESIDENT <= CU_LDS, r


def test_bench_floor_counts_the_sample_loop(resources):
    """tools/cng_bench.py's floor takes VALU_PER_SAMPLE vector instructions a sample: the saved ISA's sample loop (the block of k_cng<2,
    false> that holds v_sad_u8, two samples a turn) holds exactly twice that, and the other two run forms the same"""
    import re

    import kernel_resources as kr

    text = open(os.path.join(ROOT, "tools", "cng_bench.py")).read()
    per_sample = float(re.search(r"^VALU_PER_SAMPLE = ([0-9.]+)\s", text, re.M).group(1))
    path = os.path.join(kr.ASM_DIR, "igdsp_k_cng-hip-amdgcn-amd-amdhsa-gfx950.s")
    for form in (0, 1, 2):
        assert kr.loop_valu_count(path, f"_ZN5igdsp5k_cngILi{form}ELb0EEEvNS_7CngArgsE", "v_sad_u8") == 2 * per_sample, form
