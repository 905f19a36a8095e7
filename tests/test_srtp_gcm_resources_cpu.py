"""-m "not gpu": the AES-GCM SRTP kernels in the saved gfx950 ISA (tools/kernel_resources.py: fresh_resources): the three instantiations of
k_srtp_gcm the launcher can pick are there (a leg's key size is in its state, so there is none per key size), none spills a VGPR or
uses scratch (the round keys, the multiples of H and a piece's words are never a run-time indexed private array), the VGPR / LDS budget
of the residency srtp_gcm_route's geometry is written for holds, and the blocks of one AES block and of one word of a GHASH multiply
hold the number of vector instructions tools/srtp_gcm_bench.py's floor is computed from."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

RESIDENT, VGPRS, CU_LDS = 4, 512, 160 * 1024     # kSrtpGcmResident, kSrtpGcmVgprs (csrc/igdsp_route.h)
LDS = 1024 + 64 * 17 * 4 + 2 * 256 + 60 * 256 + 64 * 256 + 64    # kSrtpGcmLdsBytes: the table, the tile, two words a row, the round keys, the multiples of H, the reduction
PROTECT, UNPROTECT, MOVE = ("_ZN5igdsp10k_srtp_gcmILi0ELb0EEEvNS_11SrtpGcmArgsE", "_ZN5igdsp10k_srtp_gcmILi1ELb0EEEvNS_11SrtpGcmArgsE",
                            "_ZN5igdsp10k_srtp_gcmILi0ELb1EEEvNS_11SrtpGcmArgsE")
ASM = "igdsp_k_srtp_gcm-hip-amdgcn-amd-amdhsa-gfx950.s"


@pytest.fixture(scope="module")
def resources():
    import kernel_resources as kr

    return kr.fresh_resources()


def test_srtp_gcm_kernels_no_spill_and_budget(resources):
    """k_srtp_gcm<DIR, MOVE>: a block is one wave of 64 legs; kSrtpGcmResident = 4 blocks share a CU, one wave a SIMD, so a wave may take
    a SIMD's 512 registers, accumulation registers included; the LDS is static, and a fifth block's would not fit.  No VGPR spill, no
    scratch."""
    import kernel_resources as kr

    ks = [r for r in resources if "k_srtp_gcm<" in r["demangled"]]
    names = {r["demangled"] for r in ks}
    want = {"void igdsp::k_srtp_gcm<0, false>", "void igdsp::k_srtp_gcm<1, false>", "void igdsp::k_srtp_gcm<0, true>"}
    assert names == want, names ^ want
    assert not [r for r in resources if "k_srtp<" in r["demangled"] and r["file"] != "igdsp_k_srtp"]      # the SRTP kernels' collection is not touched
    text = open(os.path.join(kr.ASM_DIR, ASM)).read()
    for r in ks:
        assert r["file"] == "igdsp_k_srtp_gcm"
        assert r["spill"] == 0 and r["scratch"] == 0, r
        meta = text[text.index("amdhsa.kernels:"):]
        blk = next(b for b in meta.split("  - .agpr_count:")[1:] if re.search(r"\.name:\s+" + re.escape(r["name"]) + r"\s", b))
        agpr = int(blk.split()[0])
        assert r["vgpr"] <= VGPRS and agpr == 0 and -(-RESIDENT // 4) * VGPRS <= 512, (r, agpr)     # .vgpr_count is the unified total
        assert r["lds"] <= LDS and LDS * RESIDENT <= CU_LDS < LDS * (RESIDENT + 1), r
        if "false>" in r["demangled"]:
            assert r["lds"] == LDS, r


def test_bench_floor_counts_the_blocks(resources):
    """tools/srtp_gcm_bench.py's floor takes VALU_PER_AES vector instructions an AES block and four times VALU_PER_GHASH_WORD a multiply.
    In the saved ISA of protect and of unprotect the four blocks with the rotations of thirteen table rounds (156 v_alignbit_b32) and
    at least 200 LDS instructions are the four AES blocks of a piece: the smallest holds exactly VALU_PER_AES, none more than two above
    it (a block begins with what stands in front of it in its piece).  The blocks with the eight nibbles' shifts (24 v_alignbit_b32)
    and 20 to 30 LDS instructions are one trip of a multiply's loop over a word: four call sites a pass, each exactly
    VALU_PER_GHASH_WORD.  The length block's multiply and J0's AES block share one block, which holds no more than the two together.
    The yardstick holds neither."""
    import kernel_resources as kr

    text = open(os.path.join(ROOT, "tools", "srtp_gcm_bench.py")).read()
    per_aes = int(re.search(r"^VALU_PER_AES = (\d+)", text, re.M).group(1))
    per_word = int(re.search(r"^VALU_PER_GHASH_WORD = (\d+)", text, re.M).group(1))
    skipped = int(re.search(r"^VALU_AES_ROUNDS_10_13 = (\d+)", text, re.M).group(1))
    assert 3 * per_aes < 14 * skipped < 14 * per_aes * 4 // 13     # four of the fourteen rounds (the last is the cheapest) and four selects
    path = os.path.join(kr.ASM_DIR, ASM)
    for kernel in (PROTECT, UNPROTECT):
        aes = [b for b in kr.blocks_with(path, kernel, "v_alignbit_b32", 156, lds_at_least=200) if b["names"]["v_alignbit_b32"] == 156]
        assert len(aes) == 4 and min(b["valu"] for b in aes) == per_aes and max(b["valu"] for b in aes) <= per_aes + 2, (kernel, [(b["label"], b["valu"], b["lds"]) for b in aes])
        mul = [b for b in kr.blocks_with(path, kernel, "v_alignbit_b32", 24, lds_at_least=20) if b["names"]["v_alignbit_b32"] == 24 and b["lds"] <= 30]
        assert [b["valu"] for b in mul] == [per_word] * 4, (kernel, [(b["label"], b["valu"], b["lds"]) for b in mul])
        last = [b for b in kr.blocks_with(path, kernel, "v_alignbit_b32", 157, lds_at_least=200)]
        assert len(last) == 1 and last[0]["valu"] <= per_aes + 4 * per_word, (kernel, [(b["label"], b["valu"], b["lds"]) for b in last])
    assert not kr.blocks_with(path, MOVE, "v_alignbit_b32", 20)               # the yardstick: no AES round, no multiply
