"""-m "not gpu": the noise suppressor's kernels in the saved gfx950 ISA (tools/kernel_resources.py: fresh_resources): the four
instantiations of k_ns the launcher can pick are there, none spills a VGPR or uses scratch (the next frame's pieces are registers, never
a run-time indexed array; everything else lives in LDS), the VGPR / LDS budget of the residency ns_route's geometry is written for holds,
and the blocks of one forward and one inverse butterfly hold the number of vector instructions tools/ns_bench.py's floor is computed
from."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

RESIDENT, VGPRS, CU_LDS = 8, 256, 160 * 1024     # kNsResident, kNsVgprs (csrc/igdsp_route.h)
LDS_MAX = 4 * (1072 + 1680 + 640)                 # ns_lds_bytes(320): dynamic, asked for by the launcher


@pytest.fixture(scope="module")
def resources():
    import kernel_resources as kr

    return kr.fresh_resources()


def test_ns_kernels_no_spill_and_budget(resources):
    """k_ns<IN, COPY>: a block is one wave of four channels; kNsResident = 8 blocks share a CU, two waves a SIMD, so a wave may take up
    to 256 of a SIMD's 512 VGPRs; state, points and rows are dynamic LDS (none is static).  No VGPR spill, no scratch."""
    ks = [r for r in resources if "k_ns<" in r["demangled"]]
    names = {r["demangled"] for r in ks}
    want = {f"void igdsp::k_ns<{i}, {c}>" for i in (1, 2) for c in ("false", "true")}
    assert names == want, names ^ want
    for r in ks:
        assert r["file"] == "igdsp_k_ns"
        assert r["spill"] == 0 and r["scratch"] == 0, r
        assert r["vgpr"] <= VGPRS and (RESIDENT // 4) * VGPRS <= 512, r
        assert r["lds"] == 0 and LDS_MAX * RESIDENT <= CU_LDS, r


def test_bench_floor_counts_the_butterflies(resources):
    """tools/ns_bench.py's floor takes VALU_PER_BUTTERFLY vector instructions a butterfly: in the saved ISA of k_ns<IN, false> the two
    loop blocks with four v_mad_i64_i32 (the four products of one complex product), two LDS reads and two LDS writes are the forward
    and the inverse pass's butterfly, in that order, and hold exactly those counts, from codes and from PCM"""
    import ast
    import re

    import kernel_resources as kr

    text = open(os.path.join(ROOT, "tools", "ns_bench.py")).read()
    per = ast.literal_eval(re.search(r"^VALU_PER_BUTTERFLY = (\{[^}]*\})", text, re.M).group(1))
    assert sorted(per) == ["forward", "inverse"]
    path = os.path.join(kr.ASM_DIR, "igdsp_k_ns-hip-amdgcn-amd-amdhsa-gfx950.s")
    for form in (1, 2):
        blocks = kr.block_counts(path, f"_ZN5igdsp4k_nsILi{form}ELb0EEEvNS_6NsArgsE")
        fly = [b for b in blocks if b["loop"] and b["names"].get("v_mad_i64_i32", 0) == 4 and b["lds"] == 4]
        assert [b["valu"] for b in fly] == [per["forward"], per["inverse"]], (form, [(b["label"], b["valu"]) for b in fly])
    for form in (1, 2):                                                      # the yardstick runs no transform: no 64-bit product in a loop
        blocks = kr.block_counts(path, f"_ZN5igdsp4k_nsILi{form}ELb1EEEvNS_6NsArgsE")
        assert not [b for b in blocks if b["names"].get("v_mad_i64_i32", 0) >= 4]
