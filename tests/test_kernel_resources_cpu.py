"""-m "not gpu": no hot kernel may spill.  Builds the gfx950 code objects with `--asm` (hipcc cross-compiles without a GPU) and
reads the kernel descriptors out of the saved ISA: `.vgpr_spill_count` and `.private_segment_fixed_size` must be 0 for every
kernel that touches the payload stream (round 1 shipped the headline instantiation with 3 spilled VGPRs = 16 B of scratch per
lane), and the LDS / VGPR budgets the launch geometry relies on must hold, for the payload kernels and for each device stage.  The
saved ISA is rebuilt first when it is older than any device source, header or build.py (tools/kernel_resources.py: fresh_resources)."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

HOT = ("k_meter_chunk64", "k_meter_rtp64", "k_meter_image", "k_meter_strided", "k_meter_tiny", "k_meter_wave_per_frame", "k_roundtrip_lut64", "k_roundtrip_blk64", "k_roundtrip_strided", "k_roundtrip_chunk64",
       "k_roundtrip_general", "k_encode_lut16", "k_encode_v8", "k_depayload64", "k_wav_expand16", "k_flush_fold", "k_window_update", "k_window_finish")


@pytest.fixture(scope="module")
def resources():
    import kernel_resources as kr

    return kr.fresh_resources()


def test_no_hot_kernel_spills(resources):
    seen = set()
    for r in resources:
        name = r["demangled"]
        if not any(h in name for h in HOT) or "DIAG" in name:
            continue
        if "k_meter_chunk64<false, false, true>" in name:          # the cycle-stamp diagnostic instantiation
            continue
        seen.add(next(h for h in HOT if h in name))
        assert r["spill"] == 0 and r["scratch"] == 0, (name, r)
    assert seen == set(HOT), set(HOT) - seen


def test_launch_geometry_budgets(resources):
    by = {r["demangled"]: r for r in resources}
    lim = {"k_meter_chunk64<false, true, false>": 128, "k_meter_chunk64<false, false, false>": 128,      # 16 waves / CU
           "k_meter_chunk64<true, true, false>": 168, "k_meter_chunk64<true, false, false>": 168,        # 12 waves / CU
           "k_roundtrip_lut64<0>": 168, "k_roundtrip_lut64<1>": 168, "k_encode_lut16<0>": 128, "k_encode_lut16<1>": 128,
           "k_roundtrip_blk64<0>": 168, "k_roundtrip_blk64<1>": 168,                                      # up to 12 waves / CU (6 launched)
           "k_meter_rtp64<true, false, false, 2>": 170, "k_meter_rtp64<true, false, true, 2>": 170, "k_meter_rtp64<true, true, false, 2>": 170}   # 12 waves / CU
    for k, v in lim.items():
        r = by["void igdsp::" + k]
        assert r["vgpr"] <= v, (k, r)
        assert r["lds"] <= 160 * 1024, (k, r)


def test_tx_kernel_no_spill_and_budget(resources):
    """The TX packetizer's kernels must not spill, and must keep the register / LDS budget its launch geometry relies on (one block of 8
    waves per CU in the table form: <= 256 VGPRs for 2 waves per SIMD, 18 KiB static LDS beside the 128 KiB table)."""
    tx_resources = [r for r in resources if "k_tx_packetize" in r["demangled"]]
    names = {r["demangled"] for r in tx_resources}
    # every (input form, encoder lineage) instantiation the launcher can pick
    assert {"void igdsp::k_tx_packetize<0, 1>", "void igdsp::k_tx_packetize<1, 0>", "void igdsp::k_tx_packetize<1, 1>",
            "void igdsp::k_tx_packetize<2, 0>", "void igdsp::k_tx_packetize<2, 1>"} <= names, names
    for r in tx_resources:
        assert r["spill"] == 0 and r["scratch"] == 0, r
        assert r["vgpr"] <= 256, r
        assert r["lds"] + 2 * 65536 <= 160 * 1024, r


def test_staged_kernel_no_spill_and_budget(resources):
    """The staged send path's kernel (k_tx_staged) must not spill or use scratch, and must keep the register / LDS budget its route relies
    on: blocks of kTsWaves x 64 threads, 4 096 waves resident at 65 536 legs -> at least 4 waves per SIMD (<= 128 VGPRs), static LDS
    only, small enough for several blocks per CU."""
    staged_resources = [r for r in resources if "k_tx_staged" in r["demangled"]]
    assert [r["demangled"] for r in staged_resources] == ["igdsp::k_tx_staged"], staged_resources
    r = staged_resources[0]
    assert r["spill"] == 0 and r["sgpr_spill"] == 0 and r["scratch"] == 0, r
    assert r["vgpr"] <= 128, r
    assert r["lds"] <= 16 * 1024, r


def test_conf_kernels_no_spill_and_budget(resources):
    """The conference mix's kernels must not spill and must keep the budget its launch geometry relies on: one block of kConfWaves = 16
    waves per CU (<= 128 VGPRs for 4 waves per SIMD), the G.711 form's 64 KiB LUT + 32 KiB wide-form partials within the 160 KiB LDS of
    a CU."""
    conf_resources = [r for r in resources if "k_conf_mix" in r["demangled"]]
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


def test_bss_kernels_no_spill_and_budget(resources):
    """The best-signal-selection kernels must not spill and must keep the budget their launch geometry relies on: blocks of kBssWaves = 4
    waves (one wave per SIMD, so up to 512 VGPRs would fit; the emit keeps kBssU frame loads in flight in far fewer), the G.711 form's
    64 KiB LUT + 32 KiB of vote keys within the 160 KiB LDS of a CU, and k_bss_words as a plain 256-thread kernel without LDS."""
    bss_resources = [r for r in resources if "k_bss_" in r["demangled"]]
    names = {r["demangled"] for r in bss_resources}
    # every input form of the product kernel and of the compute-free yardstick, and the words pass
    assert {f"void igdsp::k_bss_select<{i}, {c}>" for i in (0, 1, 2) for c in ("false", "true")} <= names, names
    assert any("k_bss_words" in x for x in names), names
    for r in bss_resources:
        assert r["spill"] == 0 and r["scratch"] == 0, r
        assert r["vgpr"] <= 128, r                                       # room to spare at one wave per SIMD
        assert r["lds"] <= 160 * 1024, r
        if r["demangled"] == "void igdsp::k_bss_select<0, false>":
            assert r["lds"] >= 64 * 1024 + 32 * 1024, r                 # the LUT and the vote keys are both there
        if "k_bss_words" in r["demangled"]:
            assert r["lds"] == 0, r


def test_jb_kernels_no_spill_and_budget(resources):
    """The jitter-buffer kernels must not spill and must keep the budget their launch geometry relies on: blocks of kJbWaves = 4
    independent waves, each with 8 KiB of descriptors ([kJbPart][kJbCh] u32) and 3.5 KiB of ring tags, sources and store list in LDS —
    about 42 KiB per block, so three blocks (12 waves) fit a CU's 160 KiB — and registers for at least three waves per SIMD."""
    jb_resources = [r for r in resources if "k_jb_" in r["demangled"]]
    names = {r["demangled"] for r in jb_resources}
    assert {"void igdsp::k_jb_receive<false>", "void igdsp::k_jb_receive<true>"} <= names, names
    for r in jb_resources:
        assert r["spill"] == 0 and r["sgpr_spill"] == 0 and r["scratch"] == 0, r
        assert r["vgpr"] <= 168, r                                        # three waves per SIMD: what the LDS allows
        assert 32 * 1024 <= r["lds"] <= 160 * 1024 // 3, r               # the descriptors are there; three blocks per CU


def test_plc_kernels_no_spill_and_budget(resources):
    """The concealment kernels must not spill VGPRs or use scratch (their SGPR spills stay in VGPR lanes), and must keep the budget their
    launch geometry relies on: blocks of kPlcWaves = 4 independent waves, each with 4 KiB of tick kinds ([kPlcPart][kPlcCh] u16), 3 KiB
    of per-piece partials and 2 KiB of history, cycle and state in LDS — about 37 KiB per block, so four blocks (16 waves) fit a CU's
    160 KiB — and registers for at least four waves per SIMD."""
    plc_resources = [r for r in resources if "k_plc" in r["demangled"]]
    names = {r["demangled"] for r in plc_resources}
    assert {"void igdsp::k_plc<false>", "void igdsp::k_plc<true>"} <= names, names
    for r in plc_resources:
        assert r["spill"] == 0 and r["scratch"] == 0, r
        assert r["sgpr_spill"] <= 40, r                                  # SGPRs spill into VGPR lanes only: no memory
        assert r["vgpr"] <= 128, r                                        # four waves per SIMD
        assert 32 * 1024 <= r["lds"] <= 160 * 1024 // 4, r               # the kinds are there; four blocks per CU
