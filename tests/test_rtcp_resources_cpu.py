"""-m "not gpu": the RTCP / SRTCP kernels in the saved gfx950 ISA (tools/kernel_resources.py: fresh_resources): k_rtcp_build,
k_rtcp_parse (each with its yardstick) and the three instantiations of k_srtcp the launcher can pick are there, in their own translation unit; none spills a
VGPR or uses scratch (the report's words, the walk's fields, the round keys and a piece's words are never a run-time indexed array);
the VGPR / LDS budget of the residency the routes' geometry is written for holds; the yardstick holds no AES round and no compression,
the two real instantiations hold SRTP's."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

RESIDENT, VGPRS, CU_LDS = 8, 256, 160 * 1024     # kRtcpResident / kSrtpResident, kRtcpVgprs / kSrtpVgprs (csrc/igdsp_route.h)
LDS = {"void igdsp::k_rtcp_build<false>": 64 * 35 * 4 + 256, "void igdsp::k_rtcp_build<true>": 64 * 35 * 4 + 256,   # kRtcpBuildLdsBytes: the rows, a size a row
       "void igdsp::k_rtcp_parse<false>": 64 * 17 * 4 + 256, "void igdsp::k_rtcp_parse<true>": 64 * 17 * 4 + 256,   # kRtcpParseLdsBytes: the tile, a limit a row
       "void igdsp::k_srtcp<0, false>": 1024 + 64 * 17 * 4 + 2 * 256 + 44 * 256, "void igdsp::k_srtcp<1, false>": 1024 + 64 * 17 * 4 + 2 * 256 + 44 * 256}   # kSrtpLdsBytes
PROTECT, UNPROTECT, MOVE = ("_ZN5igdsp7k_srtcpILi0ELb0EEEvNS_8SrtpArgsE", "_ZN5igdsp7k_srtcpILi1ELb0EEEvNS_8SrtpArgsE", "_ZN5igdsp7k_srtcpILi0ELb1EEEvNS_8SrtpArgsE")


@pytest.fixture(scope="module")
def resources():
    import kernel_resources as kr

    return kr.fresh_resources()


def test_rtcp_kernels_no_spill_and_budget(resources):
    """a block is one wave of 64 legs; 8 blocks share a CU, two waves a SIMD, so a wave may take up to 256 of a SIMD's 512 registers,
    accumulation registers included; the LDS is static.  No VGPR spill, no scratch."""
    import kernel_resources as kr

    ks = [r for r in resources if r["file"] == "igdsp_k_rtcp"]
    names = {r["demangled"] for r in ks}
    want = set(LDS) | {"void igdsp::k_srtcp<0, true>"}
    assert names == want, names ^ want
    text = open(os.path.join(kr.ASM_DIR, "igdsp_k_rtcp-hip-amdgcn-amd-amdhsa-gfx950.s")).read()
    meta = text[text.index("amdhsa.kernels:"):]
    for r in ks:
        assert r["spill"] == 0 and r["scratch"] == 0, r
        blk = next(b for b in meta.split("  - .agpr_count:")[1:] if re.search(r"\.name:\s+" + re.escape(r["name"]) + r"\s", b))
        agpr = int(blk.split()[0])
        assert r["vgpr"] <= VGPRS and agpr == 0 and (RESIDENT // 4) * VGPRS <= 512, (r, agpr)     # .vgpr_count is the unified total
        if r["demangled"] in LDS:
            assert r["lds"] == LDS[r["demangled"]] and r["lds"] * RESIDENT <= CU_LDS, r
        else:
            assert r["lds"] <= LDS["void igdsp::k_srtcp<0, false>"], r


def test_srtcp_holds_srtps_blocks_and_the_yardstick_none():
    """protect and unprotect hold the four AES blocks of a piece (at least 100 v_alignbit_b32 and 160 LDS reads each) and the inner
    hash's compression in a loop, as k_srtp does (tests/test_srtp_resources_cpu.py says how they are told apart); the yardstick holds
    neither"""
    import kernel_resources as kr

    path = os.path.join(kr.ASM_DIR, "igdsp_k_rtcp-hip-amdgcn-amd-amdhsa-gfx950.s")
    for kernel in (PROTECT, UNPROTECT):
        assert len(kr.blocks_with(path, kernel, "v_alignbit_b32", 100, lds_at_least=160)) == 4, kernel
        sha = [b for b in kr.blocks_with(path, kernel, "v_alignbit_b32", 200) if b["lds"] == 0]
        assert len([b for b in sha if b["loop"]]) == 1 and len([b for b in sha if not b["loop"]]) == 1, (kernel, [(b["label"], b["loop"], b["valu"]) for b in sha])
    assert not kr.blocks_with(path, MOVE, "v_alignbit_b32", 20)
