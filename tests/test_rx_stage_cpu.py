"""-m "not gpu": the drop-in receive path's staging (csrc/igdsp_rxstage.h, no HIP include) on the CPU, through
tests/rxstage/rx_stage_driver.cpp built with g++.  A scripted staging sequence is snapshotted into an upload block and the used span
of every section is compared byte for byte with the rules below, written out by hand from the snapshot:

- the snapshot of channels [0, nch) is split into parts [nch * i / n, nch * (i + 1) / n); part i owns frame indices from c0 * 8 on
  (8 = IGDSP_STAGE_DEPTH) in every section, and walks its channels in order, each channel's frames oldest first;
- a 160-byte frame is group A: record id = c0 * 8 + (group A frames of the part so far), its bytes at payA + 160 id, its PT at ptA[id];
- any other length is group B: ib = c0 * 8 + (group B frames of the part so far), its bytes at payB + 256 ib, lenB[ib] = length,
  ptB[ib] = PT, record id = ib | 0x80000000;
- seq[c0 * 8 + k] = {record id, the channel's ED-137 word when the frame was staged} for the part's k-th frame;
- runs[c] = {c0 * 8 + seq entries of the part before channel c, frames of channel c};
- a channel holds 8 frames: staging a 9th overwrites the oldest, counts it as dropped and returns IGDSP_EBUSY.

Nothing outside those places is written (the block starts zeroed and the spans are compared whole).  The published double buffer's
reader / flip / rewrite protocol is checked by the driver's pubtest."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "igate4xsoftphonedsp_amd", "csrc")

OK, EBUSY = 0, -16                              # IGDSP_OK, IGDSP_EBUSY
DEPTH, SLOT, A_LEN, REC_B = 8, 256, 160, 0x80000000
W1 = 0xA0000001

# (channel, pt, length, tag) frames and (channel, word) changes, in staging order
SCRIPT = [
    ("stage", 0, 0, 160, 1), ("stage", 0, 8, 24, 2), ("word", 0, W1), ("stage", 0, 0, 164, 3), ("stage", 0, 8, 1, 4),
    ("stage", 0, 0, 255, 5), ("stage", 0, 8, 160, 6),
    ("stage", 2, 8, 160, 7), ("stage", 2, 0, 24, 8),
    ("word", 3, 0x10000000), ("stage", 3, 0, 160, 9), ("word", 3, 0x30000000), ("stage", 3, 8, 164, 10),
] + [("stage", 5, 0, 160 if k % 3 else 24, 20 + k) for k in range(10)] + [
    ("stage", 6, 0, 0, 40),                     # an empty payload stages nothing (channel 6 is not seen)
]
CHANNELS = 8


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = tmp_path_factory.mktemp("rxstage") / "rx_stage_driver"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-pthread", "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                    os.path.join(ROOT, "tests", "rxstage", "rx_stage_driver.cpp"), "-o", str(exe)], check=True, capture_output=True, timeout=300)
    return str(exe)


def run(driver, lines):
    r = subprocess.run([driver], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout.splitlines()


def script_lines(parts):
    out = [f"init {CHANNELS}"]
    for cmd, *args in SCRIPT:
        out.append(" ".join([cmd] + [str(a) for a in args]))
    return out + [f"snap {parts}", "counts", f"snap {parts}"]


def payload(length, tag):
    return bytes((tag + i) & 0xFF for i in range(length))


def model():
    """What each channel holds after SCRIPT: the newest 8 frames, each as (pt, length, tag, word); and the per-stage return codes."""
    rings, word, rcs, dropped = {}, {}, [], {}
    for cmd, ch, *args in SCRIPT:
        if cmd == "word":
            word[ch] = args[0]
            continue
        pt, length, tag = args
        rc = OK
        if length:
            ring = rings.setdefault(ch, [])
            if len(ring) == DEPTH:
                ring.pop(0)
                dropped[ch] = dropped.get(ch, 0) + 1
                rc = EBUSY
            ring.append((pt, length, tag, word.get(ch, 0)))
        rcs.append(rc)
    return rings, rcs, dropped


def expected_snapshot(rings, nch, n_parts):
    """The upload block's used spans, built by the rules in the module docstring."""
    frames = CHANNELS * DEPTH
    payA, ptA, payB, ptB = bytearray(frames * A_LEN), bytearray(frames), bytearray(frames * SLOT), bytearray(frames)
    lenB, seq, runs = [0] * frames, [0] * (2 * frames), [0] * (2 * nch)
    parts = []
    for i in range(n_parts):
        c0, c1 = nch * i // n_parts, nch * (i + 1) // n_parts
        base, nA, nB, nS = c0 * DEPTH, 0, 0, 0
        for c in range(c0, c1):
            s0 = nS
            for pt, length, tag, w in rings.get(c, []):
                if length == A_LEN:
                    rid = base + nA
                    nA += 1
                    payA[rid * A_LEN:(rid + 1) * A_LEN] = payload(length, tag)
                    ptA[rid] = pt
                else:
                    ib = base + nB
                    nB += 1
                    payB[ib * SLOT:ib * SLOT + length] = payload(length, tag)
                    lenB[ib], ptB[ib] = length, pt
                    rid = ib | REC_B
                seq[2 * (base + nS):2 * (base + nS) + 2] = [rid, w]
                nS += 1
            runs[2 * c], runs[2 * c + 1] = base + s0, nS - s0
        parts.append((c0, c1, nA, nB, nS))
    # each section's span ends with the last part's share of it
    endA, endB, endS = (max([c0 * DEPTH + p[k] for c0, _, *p in parts if p[k]] or [0]) for k in range(3))
    return parts, {"payA": payA[:endA * A_LEN].hex(), "ptA": ptA[:endA].hex(), "payB": payB[:endB * SLOT].hex(), "lenB": lenB[:endB],
                   "ptB": ptB[:endB].hex(), "seq": seq[:2 * endS], "runs": runs}


def parse(lines):
    """-> return codes, [snapshot dicts], counts"""
    rcs, snaps, counts = [], [], {}
    for ln in lines:
        key, _, rest = ln.partition(" ")
        if key == "rc":
            rcs.append(int(rest))
        elif key == "snap":
            nch, n = map(int, rest.split())
            snaps.append({"nch": nch, "n": n, "parts": []})
        elif key == "part":
            snaps[-1]["parts"].append(tuple(map(int, rest.split())))
        elif key in ("payA", "ptA", "payB", "ptB"):
            snaps[-1][key] = rest.strip()
        elif key in ("lenB", "seq", "runs"):
            snaps[-1][key] = [int(x) for x in rest.split()]
        elif key == "count":
            c, seen, dropped = map(int, rest.split())
            counts[c] = (seen, dropped)
    return rcs, snaps, counts


def frames_per_channel(snap):
    """channel -> [(pt, payload bytes, word)] decoded from the block by its own records"""
    payA, payB, ptA, ptB = bytes.fromhex(snap["payA"]), bytes.fromhex(snap["payB"]), bytes.fromhex(snap["ptA"]), bytes.fromhex(snap["ptB"])
    out = {}
    for c in range(snap["nch"]):
        first, count = snap["runs"][2 * c], snap["runs"][2 * c + 1]
        fr = []
        for k in range(first, first + count):
            rid, w = snap["seq"][2 * k], snap["seq"][2 * k + 1]
            if rid & REC_B:
                ib = rid & ~REC_B
                fr.append((ptB[ib], payB[ib * SLOT:ib * SLOT + snap["lenB"][ib]], w))
            else:
                fr.append((ptA[rid], payA[rid * A_LEN:(rid + 1) * A_LEN], w))
        out[c] = fr
    return out


@pytest.mark.parametrize("n_parts", [1, 4])
def test_snapshot_layout(driver, n_parts):
    rcs, snaps, counts = parse(run(driver, script_lines(n_parts)))
    rings, want_rcs, dropped = model()
    assert rcs == want_rcs
    snap, again = snaps
    nch = 6                                       # 1 + the highest channel that staged a frame
    assert (snap["nch"], snap["n"]) == (nch, n_parts)
    parts, want = expected_snapshot(rings, nch, n_parts)
    assert snap["parts"] == parts
    for key, val in want.items():
        assert snap[key] == val, key
    # every frame was taken, and the next snapshot finds nothing
    assert [again["runs"][2 * c + 1] for c in range(nch)] == [0] * nch
    assert all(p[4] == 0 for p in again["parts"])
    for c in range(nch):
        assert counts[c] == (len(rings.get(c, [])), dropped.get(c, 0))


def test_full_ring_drops_the_oldest(driver):
    rcs, snaps, counts = parse(run(driver, [f"init {CHANNELS}"] + [f"stage 5 0 160 {20 + k}" for k in range(10)] + ["snap 1", "counts"]))
    assert rcs == [OK] * 8 + [EBUSY] * 2
    assert counts[5] == (8, 2)
    frames = frames_per_channel(snaps[0])[5]
    assert [f[1] for f in frames] == [payload(160, 20 + k) for k in range(2, 10)]     # the newest 8, oldest first


def test_parts_keep_each_channels_frames(driver):
    one = frames_per_channel(parse(run(driver, script_lines(1)))[1][0])
    four = frames_per_channel(parse(run(driver, script_lines(4)))[1][0])
    rings, _, _ = model()
    assert one == four
    for c, fr in one.items():
        assert fr == [(pt, payload(length, tag), w) for pt, length, tag, w in rings.get(c, [])]
    assert [w for _, _, w in one[0]] == [0, 0, W1, W1, W1, W1]        # the word changed between the 2nd and the 3rd frame


def test_published_set(driver):
    assert run(driver, ["pubtest"]) == ["pub ok"]
