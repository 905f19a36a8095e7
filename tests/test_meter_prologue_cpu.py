"""-m "not gpu": the shape of the headline kernel's prologue, loop and record store, read from the saved gfx950 ISA (the `--asm` build,
tools/kernel_resources.py) of the two shipped meter-only instantiations k_meter_chunk64<false, *, false>:

  (i)   the record store carries the cache policy IGDSP_RECORD_STORE selects by default (2 = write-through: a 16-byte buffer store
        with `sc1` and nothing else), and it is the kernel's only 16-byte store;
  (ii)  the first item's payload loads are issued before the LUT fill's barrier: at least one 16-byte global load precedes the first
        `s_barrier` (all ten do), and nothing before that barrier drains them or waits for a device atomic;
  (iii) the main loop keeps counted waits on its loads: no `s_waitcnt vmcnt(0)` between the loop head and its back edge, EXCEPT the
        one the work queue has always carried — lane 0 of the wave that draws a batch's first slot waits for the value its own
        device atomic returns (one wave in sixteen iterations; the loop structure is not this test's subject).  That wait is
        recognised by its place: it is the first wait behind a returning `global_atomic_add`, with no load between the two;
  (iv)  none of the instructions the project bans (scalar stores / scalar atomics / scalar cache write-back) appears in any saved ISA.
"""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

METER_ASM = "igdsp_k_meter-hip-amdgcn-amd-amdhsa-gfx950.s"
KERNELS = ("_ZN5igdsp15k_meter_chunk64ILb0ELb1ELb0EEEvPKhS2_jjP17igdsp_frame_statsPsP15igdsp_aggregatejPmPj",      # <false, true, false>: the headline
           "_ZN5igdsp15k_meter_chunk64ILb0ELb0ELb0EEEvPKhS2_jjP17igdsp_frame_statsPsP15igdsp_aggregatejPmPj")      # <false, false, false>
# spelled in pieces: no source file of the project holds these words
BANNED = ("s_" + "store_dword", "s_buffer_" + "store", "s_scratch_" + "store", "s_" + "atomic", "s_buffer_" + "atomic", "s_dcache_" + "wb",
          "s_dcache_" + "discard")


@pytest.fixture(scope="module")
def asm():
    import kernel_resources as kr

    kr.fresh_resources()                       # rebuilds _asm/ when a source is newer
    return {os.path.basename(p): open(p).read() for p in kr.asm_files()}


def kernel_body(text, symbol):
    """The instruction lines and block labels of one kernel, from its label to its s_endpgm; comments and directives dropped."""
    start = text.index("\n" + symbol + ":")
    end = text.index("s_endpgm", start)
    out = []
    for line in text[start:end].split("\n")[2:]:
        line = line.split(";")[0].strip()
        if line and (not line.startswith(".") or (line.startswith(".LBB") and line.endswith(":"))):
            out.append(line)
    return out


def main_loop(body):
    """(head, back edge) positions of the main loop: the widest backward branch around the record store."""
    labels = {l[:-1]: i for i, l in enumerate(body) if l.endswith(":")}
    store = next(i for i, l in enumerate(body) if re.match(r"(buffer|global)_store_dwordx4", l))
    best = None
    for i, l in enumerate(body):
        m = re.match(r"s_c?branch\S*\s+(\.LBB\S+)", l)
        if m and labels.get(m.group(1), i) < store < i and (best is None or i - labels[m.group(1)] > best[1] - best[0]):
            best = (labels[m.group(1)], i)
    assert best is not None, "no loop around the record store"
    return best


def full_drains(lines):
    """Positions of the `vmcnt(0)` waits in `lines` that are NOT the queue's wait for its own returning atomic."""
    bad = []
    for i, l in enumerate(lines):
        if "vmcnt(0)" not in l:
            continue
        prev = next((p for p in reversed(lines[:i]) if re.match(r"(global|buffer)_(load|atomic)|s_waitcnt.*vmcnt", p)), "")
        if not prev.startswith("global_atomic_add"):
            bad.append((i, l))
    return bad


@pytest.mark.parametrize("symbol", KERNELS)
def test_record_store_policy(asm, symbol):
    body = kernel_body(asm[METER_ASM], symbol)
    stores = [l for l in body if re.match(r"(buffer|global)_store_dwordx4", l)]
    assert len(stores) == 1, stores
    st = stores[0]
    assert st.startswith("buffer_store_dwordx4"), st
    assert set(re.findall(r"\b(sc0|sc1|nt)\b", st)) == {"sc1"}, st      # write-through, the default of IGDSP_RECORD_STORE


@pytest.mark.parametrize("symbol", KERNELS)
def test_loads_before_first_barrier(asm, symbol):
    body = kernel_body(asm[METER_ASM], symbol)
    barrier = next(i for i, l in enumerate(body) if l.startswith("s_barrier"))
    head = body[:barrier]
    early = [l for l in head if l.startswith("global_load_dwordx4")]
    print(f"{len(early)} 16-byte loads before the first s_barrier (instruction {barrier})")
    assert len(early) >= 1
    assert len(early) == 10, early             # both halves of the first item
    assert all(re.search(r"\bnt\b", l) for l in early), early
    assert not any("vmcnt(0)" in l for l in head), [l for l in head if "vmcnt" in l]
    assert not any(l.startswith("global_atomic") for l in head), "the block's first two batches are static: no atomic before the loads"


@pytest.mark.parametrize("symbol", KERNELS)
def test_no_full_drain_in_main_loop(asm, symbol):
    body = kernel_body(asm[METER_ASM], symbol)
    head, back = main_loop(body)
    loop = body[head:back + 1]
    assert sum(l.startswith("global_load_dwordx4") for l in loop) == 10, "the loop refills both halves"
    counts = sorted({int(x) for l in loop for x in re.findall(r"vmcnt\((\d+)\)", l)})
    print(f"main loop: instructions {head}..{back}, vmcnt waits {counts}")
    assert any(c > 0 for c in counts), "the loop waits for its loads with counted waits"
    assert full_drains(loop) == []
    assert sum("vmcnt(0)" in l for l in loop) <= 1      # the queue's own atomic, once


def test_no_banned_instruction(asm):
    assert asm
    for name, text in asm.items():
        low = text.lower()
        for word in BANNED:
            assert word not in low, (name, word)
