"""-m "not gpu": the SRTP kernels in the saved gfx950 ISA (tools/kernel_resources.py: fresh_resources): the three instantiations of k_srtp
the launcher can pick are there, none spills a VGPR or uses scratch (the round keys, the hash schedule and a piece's words are never a
run-time indexed array), the VGPR / LDS budget of the residency srtp_route's geometry is written for holds, and the blocks of one
AES-128 block and one SHA-1 compression hold the number of vector instructions tools/srtp_bench.py's floor is computed from."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

RESIDENT, VGPRS, CU_LDS = 8, 256, 160 * 1024     # kSrtpResident, kSrtpVgprs (csrc/igdsp_route.h)
LDS = 1024 + 64 * 17 * 4 + 2 * 256 + 44 * 256    # kSrtpLdsBytes: the table, the tile, two words a row, the round keys
PROTECT, UNPROTECT, MOVE = ("_ZN5igdsp6k_srtpILi0ELb0EEEvNS_8SrtpArgsE", "_ZN5igdsp6k_srtpILi1ELb0EEEvNS_8SrtpArgsE", "_ZN5igdsp6k_srtpILi0ELb1EEEvNS_8SrtpArgsE")


@pytest.fixture(scope="module")
def resources():
    import kernel_resources as kr

    return kr.fresh_resources()


def test_srtp_kernels_no_spill_and_budget(resources):
    """k_srtp<DIR, MOVE>: a block is one wave of 64 legs; kSrtpResident = 8 blocks share a CU, two waves a SIMD, so a wave may take up to
    256 of a SIMD's 512 registers, accumulation registers included; the LDS is static.  No VGPR spill, no scratch."""
    ks = [r for r in resources if "k_srtp<" in r["demangled"]]
    names = {r["demangled"] for r in ks}
    want = {"void igdsp::k_srtp<0, false>", "void igdsp::k_srtp<1, false>", "void igdsp::k_srtp<0, true>"}
    assert names == want, names ^ want
    import kernel_resources as kr

    text = open(os.path.join(kr.ASM_DIR, "igdsp_k_srtp-hip-amdgcn-amd-amdhsa-gfx950.s")).read()
    for r in ks:
        assert r["file"] == "igdsp_k_srtp"
        assert r["spill"] == 0 and r["scratch"] == 0, r
        meta = text[text.index("amdhsa.kernels:"):]
        blk = next(b for b in meta.split("  - .agpr_count:")[1:] if re.search(r"\.name:\s+" + re.escape(r["name"]) + r"\s", b))
        agpr = int(blk.split()[0])
        assert r["vgpr"] <= VGPRS and agpr == 0 and (RESIDENT // 4) * VGPRS <= 512, (r, agpr)     # .vgpr_count is the unified total
        assert r["lds"] <= LDS and LDS * RESIDENT <= CU_LDS, r
        if "false>" in r["demangled"]:
            assert r["lds"] == LDS, r


def test_bench_floor_counts_the_blocks(resources):
    """tools/srtp_bench.py's floor takes VALU_PER_AES vector instructions an AES block and VALU_PER_SHA1 a compression: in the saved ISA
    of protect and of unprotect the four blocks with the table words' rotations (at least 100 v_alignbit_b32) and at least 160 LDS reads
    are the four AES blocks of a piece, the loop block with at least 200 v_alignbit_b32 and no LDS instruction is the inner hash's
    compression, and they hold exactly those counts; the outer hash's compression (its padding is constants) holds no more; the
    yardstick holds neither."""
    import kernel_resources as kr

    text = open(os.path.join(ROOT, "tools", "srtp_bench.py")).read()
    per_aes = int(re.search(r"^VALU_PER_AES = (\d+)", text, re.M).group(1))
    per_sha = int(re.search(r"^VALU_PER_SHA1 = (\d+)", text, re.M).group(1))
    path = os.path.join(kr.ASM_DIR, "igdsp_k_srtp-hip-amdgcn-amd-amdhsa-gfx950.s")
    for kernel in (PROTECT, UNPROTECT):
        aes = kr.blocks_with(path, kernel, "v_alignbit_b32", 100, lds_at_least=160)
        assert [b["valu"] for b in aes] == [per_aes] * 4, (kernel, [(b["label"], b["valu"], b["lds"]) for b in aes])
        sha = [b for b in kr.blocks_with(path, kernel, "v_alignbit_b32", 200) if b["lds"] == 0]
        inner, outer = [b for b in sha if b["loop"]], [b for b in sha if not b["loop"]]
        assert [b["valu"] for b in inner] == [per_sha] and len(outer) == 1 and outer[0]["valu"] <= per_sha, (kernel, [(b["label"], b["loop"], b["valu"]) for b in sha])
    assert not kr.blocks_with(path, MOVE, "v_alignbit_b32", 20)               # the yardstick: no AES round, no compression
