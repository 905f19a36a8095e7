"""-m "not gpu": the argument rule of igdsp_cng_run (cng_run in csrc/igdsp_args.h), compiled with g++ alone through
tests/route/cng_args_driver.cpp: every clause in its order and which code wins when two apply: the frame length ahead of everything,
nothing to do, the required buffers and the voice input's form, the range, the alignment (the codes 8, the payloads, PCM rows, the
state, rows out, records and PCM records 16 bytes: what the kernel's loads and stores take), the overlap of byte ranges.
tests/test_gpu_cng.py replays clauses through the library."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "igate4xsoftphonedsp_amd", "csrc")
EINVAL, ERANGE = -22, -34
BASE = dict(kind="x", sid="x", sid_len="x", g711="x", codec="x", pcm="0", ctl="x", seed="x", state="x", out="x", len="x", rec="x", stats="x", C=5, F=3, n=160)
PCM = dict(g711="0", codec="0", pcm="x")
NOVOICE = dict(g711="0", codec="0", pcm="0")
BIG = dict(C=0x10000000, F=16)

# (overrides, rc, run, the verdict names its rule).  Sizes at the base shape: kind 15, sid 240, sid_len 15, g711 2 400, codec 5, pcm 4 800,
# ctl 5, seed 20, state 480, out 4 800, len 30, rec 240, stats 240
CASES = [
    (dict(), 0, 1, 0), (PCM, 0, 1, 0), (NOVOICE, 0, 1, 0), (dict(sid_len="0", ctl="0", seed="0"), 0, 1, 0), (dict(len="0", rec="0", stats="0"), 0, 1, 0),
    (dict(n=16), 0, 1, 0), (dict(n=256), 0, 1, 0), (dict(n=24), 0, 1, 0),
    # 1. the frame length, whether or not there is work
    (dict(n=0), EINVAL, 0, 0), (dict(n=8), EINVAL, 0, 0), (dict(n=20), EINVAL, 0, 0), (dict(n=162), EINVAL, 0, 0), (dict(n=264), EINVAL, 0, 0),
    (dict(C=0, n=8), EINVAL, 0, 0), (dict(F=0, n=257), EINVAL, 0, 0),
    # 2. nothing to do, whatever else is wrong
    (dict(C=0), 0, 0, 0), (dict(F=0), 0, 0, 0), (dict(C=0, kind="0", sid="0", state="0", out="x2"), 0, 0, 0),
    # 3. kind, payloads, state and rows out are required; at most one voice input, the codes with their laws
    (dict(kind="0"), EINVAL, 0, 0), (dict(sid="0"), EINVAL, 0, 0), (dict(state="0"), EINVAL, 0, 0), (dict(out="0"), EINVAL, 0, 0),
    (dict(pcm="x"), EINVAL, 0, 0), (dict(codec="0"), EINVAL, 0, 0), ({**PCM, "codec": "x"}, 0, 1, 0), ({**NOVOICE, "codec": "x"}, 0, 1, 0),
    # 4. the range: channels x frames
    (BIG, ERANGE, 0, 0), (dict(C=0xFFFFFFE0, F=1), ERANGE, 0, 0), (dict(C=0xFFFFFFDF, F=1), 0, 1, 0),
    ({**BIG, "n": 0}, EINVAL, 0, 0), ({**BIG, "state": "0"}, EINVAL, 0, 0),
    # 5. alignment: 8 for the codes, 16 for the payloads, the PCM rows, the state, the rows out, the records and the PCM records
    ({**PCM, "pcm": "x2"}, EINVAL, 0, 0), ({**PCM, "pcm": "x8"}, EINVAL, 0, 0), (dict(g711="x1"), EINVAL, 0, 0), (dict(g711="x4"), EINVAL, 0, 0),
    (dict(sid="x8"), EINVAL, 0, 0), (dict(sid="x4"), EINVAL, 0, 0), (dict(state="x8"), EINVAL, 0, 0), (dict(out="x8"), EINVAL, 0, 0), (dict(out="x2"), EINVAL, 0, 0),
    (dict(rec="x8"), EINVAL, 0, 0), (dict(stats="x8"), EINVAL, 0, 0),
    (dict(kind="x1", sid="x16", sid_len="x3", g711="x8", codec="x3", ctl="x1", seed="x4", state="x16", out="x16", len="x2", rec="x16", stats="x16"), 0, 1, 0),
    ({**PCM, "pcm": "x16"}, 0, 1, 0),
    ({**BIG, "rec": "x4"}, ERANGE, 0, 0),                                 # too many frames wins over the alignment
    # 6. the state or an output that overlaps an input, or another of them: the rule with a text; the alignment wins over it
    (dict(state="g711"), EINVAL, 0, 1), (dict(state="g711+2384"), EINVAL, 0, 1), (dict(state="g711+2400"), 0, 1, 0),
    (dict(len="kind+14"), EINVAL, 0, 1), (dict(len="kind+15"), 0, 1, 0), (dict(len="sid_len+14"), EINVAL, 0, 1), (dict(len="ctl+4"), EINVAL, 0, 1),
    (dict(len="ctl+5"), 0, 1, 0), (dict(len="seed+19"), EINVAL, 0, 1), (dict(len="seed+20"), 0, 1, 0), (dict(len="codec+4"), EINVAL, 0, 1),
    (dict(out="sid+224"), EINVAL, 0, 1), (dict(out="sid+240"), 0, 1, 0), ({**PCM, "out": "pcm+4784"}, EINVAL, 0, 1), ({**PCM, "out": "pcm+4800"}, 0, 1, 0),
    ({**PCM, "len": "codec"}, 0, 1, 0),                                   # without codes d_codec is not a buffer
    (dict(rec="state+464"), EINVAL, 0, 1), (dict(rec="state+480"), 0, 1, 0), (dict(stats="rec+224"), EINVAL, 0, 1), (dict(stats="rec+240"), 0, 1, 0),
    (dict(rec="out+4784"), EINVAL, 0, 1), (dict(rec="out+4800"), 0, 1, 0), (dict(len="out+4799"), EINVAL, 0, 1), (dict(len="out+4800"), 0, 1, 0),
    (dict(len="stats+239"), EINVAL, 0, 1), (dict(len="stats+240"), 0, 1, 0), (dict(out="len+16"), EINVAL, 0, 1), (dict(out="len+32"), 0, 1, 0),
    (dict(rec="stats+232"), EINVAL, 0, 0),                                # misaligned and overlapping: no text
    (dict(codec="g711", ctl="g711", kind="sid", sid_len="sid"), 0, 1, 0),  # inputs may share memory
]


@pytest.fixture(scope="module")
def verdicts(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path_factory.mktemp("cng_args") / "cng_args_driver")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                    os.path.join(ROOT, "tests", "route", "cng_args_driver.cpp"), "-o", exe], check=True, capture_output=True, timeout=300)
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
