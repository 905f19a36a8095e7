"""-m "not gpu": the argument rule of igdsp_ns_run (ns_run in csrc/igdsp_args.h), compiled with g++ alone through
tests/route/ns_args_driver.cpp: every clause in its order and which code wins when two apply: the frame length and cfg ahead of
everything, nothing to do, the required buffers and the input's form, the range, the alignment (the codes 8, the PCM rows, the state,
rows out, records and PCM records 16 bytes: what the kernel's loads and stores take), the overlap of byte ranges.
tests/test_gpu_ns.py replays clauses through the library."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "igate4xsoftphonedsp_amd", "csrc")
EINVAL, ERANGE = -22, -34
BASE = dict(g711="x", codec="x", pcm="0", ctl="x", cfg=1, floor=5827, over=24, init=16, track=4, rise=9, state="x", out="x", rec="x", stats="x", C=5, F=3, n=160)
PCM = dict(g711="0", codec="0", pcm="x")
BIG = dict(C=0x10000000, F=16)

# (overrides, rc, run, the verdict names its rule).  Sizes at the base shape: g711 2 400, codec 5, pcm 4 800, ctl 5, state 5 360,
# out 4 800, rec 240, stats 240
CASES = [
    (dict(), 0, 1, 0), (PCM, 0, 1, 0), (dict(ctl="0"), 0, 1, 0), (dict(rec="0", stats="0"), 0, 1, 0), (dict(out="0", stats="0"), 0, 1, 0),
    (dict(out="0", rec="0"), 0, 1, 0), (dict(n=80), 0, 1, 0), (dict(n=240), 0, 1, 0), (dict(n=320), 0, 1, 0),
    # 1. the frame length and cfg, whether or not there is work
    (dict(n=0), EINVAL, 0, 0), (dict(n=8), EINVAL, 0, 0), (dict(n=40), EINVAL, 0, 0), (dict(n=81), EINVAL, 0, 0), (dict(n=168), EINVAL, 0, 0),
    (dict(n=256), EINVAL, 0, 0), (dict(n=400), EINVAL, 0, 0), (dict(C=0, n=8), EINVAL, 0, 0), (dict(F=0, n=321), EINVAL, 0, 0), (dict(cfg=0), EINVAL, 0, 0),
    (dict(cfg=0, C=0), EINVAL, 0, 0),
    (dict(floor=0), EINVAL, 0, 0), (dict(floor=32769), EINVAL, 0, 0), (dict(over=15), EINVAL, 0, 0), (dict(over=65), EINVAL, 0, 0), (dict(init=0), EINVAL, 0, 0),
    (dict(init=256), EINVAL, 0, 0), (dict(track=0), EINVAL, 0, 0), (dict(track=9), EINVAL, 0, 0), (dict(rise=3), EINVAL, 0, 0), (dict(rise=13), EINVAL, 0, 0),
    (dict(rise=13, F=0), EINVAL, 0, 0),
    (dict(floor=1, over=16, init=1, track=1, rise=4), 0, 1, 0), (dict(floor=32768, over=64, init=255, track=8, rise=12), 0, 1, 0),
    # 2. nothing to do, whatever else is wrong
    (dict(C=0), 0, 0, 0), (dict(F=0), 0, 0, 0), (dict(C=0, state="0", out="x2"), 0, 0, 0),
    # 3. exactly one input, the codes with their laws; the state; at least one output
    (dict(pcm="x"), EINVAL, 0, 0), (dict(g711="0", codec="0"), EINVAL, 0, 0), (dict(codec="0"), EINVAL, 0, 0), ({**PCM, "codec": "x"}, 0, 1, 0),
    (dict(state="0"), EINVAL, 0, 0), (dict(out="0", rec="0", stats="0"), EINVAL, 0, 0),
    # 4. the range: channels x frames
    (BIG, ERANGE, 0, 0), (dict(C=0xFFFFFFE0, F=1), ERANGE, 0, 0), (dict(C=0xFFFFFFDF, F=1), 0, 1, 0),
    ({**BIG, "n": 0}, EINVAL, 0, 0), ({**BIG, "state": "0"}, EINVAL, 0, 0), ({**BIG, "cfg": 0}, EINVAL, 0, 0),
    # 5. alignment
    ({**PCM, "pcm": "x2"}, EINVAL, 0, 0), ({**PCM, "pcm": "x8"}, EINVAL, 0, 0), (dict(g711="x1"), EINVAL, 0, 0), (dict(g711="x4"), EINVAL, 0, 0),
    (dict(state="x8"), EINVAL, 0, 0), (dict(out="x8"), EINVAL, 0, 0), (dict(out="x2"), EINVAL, 0, 0), (dict(rec="x8"), EINVAL, 0, 0), (dict(stats="x8"), EINVAL, 0, 0),
    (dict(g711="x8", codec="x3", ctl="x1", state="x16", out="x16", rec="x16", stats="x16"), 0, 1, 0), ({**PCM, "pcm": "x16"}, 0, 1, 0),
    ({**BIG, "rec": "x4"}, ERANGE, 0, 0),                                 # too many frames wins over the alignment
    # 6. the state or an output that overlaps an input, or another of them: the rule with a text; the alignment wins over it
    (dict(state="g711"), EINVAL, 0, 1), (dict(state="g711+2384"), EINVAL, 0, 1), (dict(state="g711+2400"), 0, 1, 0),
    (dict(stats="ctl"), EINVAL, 0, 1), (dict(stats="ctl+16"), 0, 1, 0), (dict(stats="codec"), EINVAL, 0, 1), ({**PCM, "stats": "codec"}, 0, 1, 0),
    ({**PCM, "out": "pcm+4784"}, EINVAL, 0, 1), ({**PCM, "out": "pcm+4800"}, 0, 1, 0),
    (dict(rec="state+5344"), EINVAL, 0, 1), (dict(rec="state+5360"), 0, 1, 0), (dict(stats="rec+224"), EINVAL, 0, 1), (dict(stats="rec+240"), 0, 1, 0),
    (dict(rec="out+4784"), EINVAL, 0, 1), (dict(rec="out+4800"), 0, 1, 0), (dict(out="stats+224"), EINVAL, 0, 1), (dict(out="stats+240"), 0, 1, 0),
    (dict(rec="stats+232"), EINVAL, 0, 0),                                # misaligned and overlapping: no text
    (dict(codec="g711", ctl="g711"), 0, 1, 0),                            # inputs may share memory
]


@pytest.fixture(scope="module")
def verdicts(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path_factory.mktemp("ns_args") / "ns_args_driver")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                    os.path.join(ROOT, "tests", "route", "ns_args_driver.cpp"), "-o", exe], check=True, capture_output=True, timeout=300)
    lines = [" ".join(f"{k}={v}" for k, v in {**BASE, **over}.items()) for over, _, _, _ in CASES]
    r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    out = r.stdout.splitlines()
    assert len(out) == len(lines)
    return [dict(kv.split("=") for kv in line.split()) for line in out]


@pytest.mark.parametrize("i", range(len(CASES)), ids=[f"{j}:" + (",".join(f"{k}={v}" for k, v in c[0].items()) or "base")[:60] for j, c in enumerate(CASES)])
def test_rule(verdicts, i):
    _, rc, run, why = CASES[i]
    v = verdicts[i]
    assert (int(v["rc"]), int(v["run"]), int(v["why"])) == (rc, run, why)
