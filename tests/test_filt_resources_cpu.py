"""-m "not gpu": the filter's kernels in the saved gfx950 ISA (tools/kernel_resources.py: fresh_resources): the eight instantiations
of k_filt the launcher can pick are there, none spills a VGPR or uses scratch (the sections' coefficients and histories and the next
frame's pieces are registers, never a run-time indexed array), the VGPR / LDS budget of the residency filt_route's geometry is written
for holds, and each sample loop holds the number of vector instructions tools/filt_bench.py's floor is computed from."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

RESIDENT, VGPRS, CU_LDS = 4, 256, 160 * 1024     # kFiltResident, kFiltVgprs (csrc/igdsp_route.h)
LDS_MAX = 64 * (256 // 2 + 1) * 4 + 64            # tile_lds_bytes(kFiltChans, 256): dynamic, asked for by the launcher


@pytest.fixture(scope="module")
def resources():
    import kernel_resources as kr

    return kr.fresh_resources()


def test_filt_kernels_no_spill_and_budget(resources):
    """k_filt<IN, S, COPY>: a block is one wave of 64 channels; kFiltResident = 4 blocks share a CU, one wave a SIMD and never more than
    two, so a wave may take up to 256 of a SIMD's 512 VGPRs; the tile is dynamic LDS (none is static).  No VGPR spill, no scratch."""
    ks = [r for r in resources if "k_filt<" in r["demangled"]]
    names = {r["demangled"] for r in ks}
    want = {f"void igdsp::k_filt<{i}, {s}, false>" for i in (1, 2) for s in (1, 2, 4)} | {f"void igdsp::k_filt<{i}, 1, true>" for i in (1, 2)}
    assert names == want, names ^ want
    for r in ks:
        assert r["file"] == "igdsp_k_filt"
        assert r["spill"] == 0 and r["scratch"] == 0, r
        assert r["vgpr"] <= VGPRS and 2 * VGPRS <= 512, r
        assert r["lds"] == 0 and LDS_MAX * RESIDENT <= CU_LDS, r


def test_bench_floor_counts_the_sample_loop(resources):
    """tools/filt_bench.py's floor takes VALU_PER_SAMPLE[S] vector instructions a sample: the saved ISA's sample loop (the block of
    k_filt<IN, S, false> that holds v_mad_i32_i24, two samples a turn) holds exactly twice that, from codes and from PCM"""
    import ast
    import re

    import kernel_resources as kr

    text = open(os.path.join(ROOT, "tools", "filt_bench.py")).read()
    per_sample = ast.literal_eval(re.search(r"^VALU_PER_SAMPLE = (\{[^}]*\})", text, re.M).group(1))
    assert sorted(per_sample) == [1, 2, 4]
    path = os.path.join(kr.ASM_DIR, "igdsp_k_filt-hip-amdgcn-amd-amdhsa-gfx950.s")
    for form in (1, 2):
        for s, v in per_sample.items():
            assert kr.loop_valu_count(path, f"_ZN5igdsp6k_filtILi{form}ELi{s}ELb0EEEvNS_8FiltArgsE", "v_mad_i32_i24") == 2 * v, (form, s)
            assert kr.loop_count(path, f"_ZN5igdsp6k_filtILi{form}ELi{s}ELb0EEEvNS_8FiltArgsE", "v_mad_i32_i24") == 10 * s, (form, s)
